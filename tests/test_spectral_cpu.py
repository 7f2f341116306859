"""CPU side of the device spectral clustering: the fp64 restatement of tests/spectral_ref.py against the recorded output of the
reference's sklearn recipe (tests/golden/make_golden_spectral.py) and against live sklearn, the product's host half
(utils/phrase_cluster.spectral_block / spectral_start / spectral_ritz / spectral_sign_flip), the recorded cluster map, the refusals
that need no GPU, and the build plumbing of csrc/spectral.hip."""
import functools
import json
import os
import re

import numpy as np
import pytest

from tests import spectral_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = [("blobs600", 6), ("edge600", 6), ("blobs257", 4), ("blobs1000", 10)]
NAMES = [c[0] for c in CASES]
SYMBOLS = ["tag_spectral_chain", "tag_spectral_gram_ws_bytes", "tag_spectral_gram", "tag_spectral_rows", "tag_spectral_apply"]


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(GOLDEN, "spectral.npz")) as f:
        out = {k: f[k] for k in f.files}
    x = out["blobs600/x"].copy()                    # edge600: a zero row and a duplicated row
    x[5] = 0
    x[77] = x[78]
    out["edge600/x"] = x
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated(name):
    """The fp64 restatement of one recorded case, computed once and shared."""
    return R.spectral_ref(golden()[f"{name}/x"], dict(CASES)[name], steps=6)


def test_fixture_is_the_generator_and_the_reference_recipe_finds_the_planted_clusters():
    g = golden()
    for name, shape in (("blobs600", (600, 16, 6, 0.3)), ("blobs257", (257, 8, 4, 0.2)), ("blobs1000", (1000, 32, 10, 0.5))):
        x, planted = R.generate(*shape)
        assert np.array_equal(x, g[f"{name}/x"]) and np.array_equal(planted, g[f"{name}/planted"])
        assert R.same_partition(g[f"{name}/labels"], planted)
    keep = np.arange(600) != 5                      # the zero row has affinity 1/2 to every row: it is the only difference
    assert R.same_partition(g["edge600/labels"][keep], g["edge600/planted"][keep])
    for name in NAMES:
        assert g[f"{name}/gap"] >= 1e-3 and 1e-7 <= g[f"{name}/err32"] <= 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_recorded_embedding(name):
    g, ref = golden(), restated(name)
    err = R.vector_errors(ref["maps"], g[f"{name}/maps"])
    print(f"{name}: block {ref['block']}, per-vector error {err.max():.3g} of the largest entry, residuals "
          f"{['%.2g' % v for v in ref['residuals']]}")
    assert err.max() <= 1e-6
    assert np.abs(ref["eigenvalues"] - g[f"{name}/eigenvalues"]).max() <= 1e-12
    assert ref["residuals"][-1] <= 1e-8 and ref["residuals"][0] <= 1e-3


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_live_sklearn(name):
    manifold = pytest.importorskip("sklearn.manifold")
    x, k = golden()[f"{name}/x"], dict(CASES)[name]
    maps = manifold.spectral_embedding(R.dense_affinity(x), n_components=k, eigen_solver="arpack", drop_first=False, random_state=1)
    err = R.vector_errors(restated(name)["maps"], maps)
    print(f"{name}: per-vector error against live sklearn {err.max():.3g}")
    assert err.max() <= 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_emulated_fp32_stays_at_the_recorded_error(name):
    g = golden()
    r32 = R.spectral_ref(g[f"{name}/x"], dict(CASES)[name], steps=6, dtype=np.float32)
    err = R.vector_errors(r32["maps"], g[f"{name}/maps"]).max()
    print(f"{name}: emulated fp32 {err:.3g} (recorded {float(g[f'{name}/err32']):.3g}), residuals "
          f"{['%.2g' % v for v in r32['residuals']]}")
    assert err <= 8 * g[f"{name}/err32"]


def test_operator_is_sklearns_normalised_laplacian():
    """M = Y Y^T - diag(e) equals D^-1/2 (A - diag A) D^-1/2 of the dense affinity, entry by entry."""
    x = golden()["blobs257/x"]
    A = R.dense_affinity(x)
    A0 = A - np.diag(np.diag(A))
    d = A0.sum(1)
    want = A0 / np.sqrt(np.outer(d, d))
    Y, s, e, deg = R.rows_ref(R.unit_rows(x))
    assert np.abs(deg - d).max() <= 1e-10 and np.abs(Y @ Y.T - np.diag(e) - want).max() <= 1e-14


def test_host_half_of_the_fit():
    from texttoaudiogrounding_amd.utils.phrase_cluster import spectral_block, spectral_ritz, spectral_sign_flip, spectral_start
    assert spectral_block(600, 16, 6) == 12 and spectral_block(257, 8, 4) == 8 and spectral_block(1000, 32, 10) == 20
    assert spectral_block(100, 4, 4) == 5 and spectral_block(3, 16, 2) == 3 and spectral_block(50, 16, 1) == 2
    assert spectral_block(600, 16, 6, block=6) == 6 and R.default_block(16, 6) == 12
    for bad in (5, 18):
        with pytest.raises(ValueError, match="expected n_clusters = 6 <= block <= "):
            spectral_block(600, 16, 6, block=bad)
    # the start: orthonormal eigenvectors of Y Y^T
    x = golden()["blobs257/x"]
    Y, s, e, _ = R.rows_ref(R.unit_rows(x))
    mu, coef = spectral_start(Y.T @ Y, 8)
    X0 = Y @ coef
    assert np.all(np.diff(mu) <= 0) and np.abs(X0.T @ X0 - np.eye(8)).max() <= 1e-12
    assert np.abs(Y @ (Y.T @ X0) - X0 * mu).max() <= 1e-12
    with pytest.raises(ValueError, match="fewer than 3 independent directions"):
        spectral_start(np.diag([1.0, 0.5, 0.0]), 3)
    # Rayleigh-Ritz on a block that is neither orthonormal nor aligned
    g = np.random.RandomState(0)
    Xb = X0 @ (np.eye(8) + 0.3 * g.randn(8, 8))
    MX = Y @ (Y.T @ Xb) - e[:, None] * Xb
    lam, C = spectral_ritz(Xb.T @ Xb, Xb.T @ MX)
    lam_ref, C_ref = R.ritz(Xb.T @ Xb, Xb.T @ MX)
    assert np.array_equal(lam, lam_ref) and np.array_equal(C, C_ref)
    assert coef.flags["C_CONTIGUOUS"] and C.flags["C_CONTIGUOUS"]          # (the device reads them through a pointer, row-major)
    V = Xb @ C
    assert np.all(np.diff(lam) <= 0) and np.abs(V.T @ V - np.eye(8)).max() <= 1e-12
    assert np.abs(V.T @ (MX @ C) - np.diag(lam)).max() <= 1e-12
    with pytest.raises(ValueError, match="lost rank"):
        spectral_ritz(np.zeros((2, 2)), np.eye(2))
    # the sign flip is sklearn's
    m = np.array([[0.1, -0.2, 0.0], [-0.5, 0.1, 0.0], [0.5, 0.2, 0.0]], dtype=np.float32)
    out = spectral_sign_flip(m)
    assert out.dtype == np.float32 and out.tolist() == (m * np.array([-1, -1, 1], dtype=np.float32)).tolist()
    assert np.array_equal(out, R.sign_flip(m)) and m[1, 0] == np.float32(-0.5)                 # (the input is left alone)
    extmath = pytest.importorskip("sklearn.utils.extmath")
    r = g.randn(40, 5)
    assert np.array_equal(spectral_sign_flip(r), extmath._deterministic_vector_sign_flip(r.T).T)


def test_recorded_cluster_map_is_the_recorded_labels():
    from texttoaudiogrounding_amd.utils.phrase_cluster import cluster_map_from_labels
    with open(os.path.join(GOLDEN, "spectral", "blobs257_result.json")) as f:
        want = json.load(f)
    mine = cluster_map_from_labels([f"row {i}" for i in range(257)], golden()["blobs257/labels"])
    assert mine == want and list(mine) == list(want)


def test_refusals_need_no_gpu():
    from texttoaudiogrounding_amd.utils.phrase_cluster import SpectralClustering
    model = SpectralClustering()
    assert (model.n_clusters, model.n_init, model.random_state, model.block, model.max_iter, model.tol, model.device) == \
        (8, 10, None, None, 10, 2e-7, "cuda:0")
    assert model.labels_ is None and model.maps_ is None
    for kw in ({"n_clusters": 0}, {"n_init": 0}, {"max_iter": 0}):
        with pytest.raises(ValueError, match="must be >= 1"):
            SpectralClustering(**kw)
    with pytest.raises(ValueError, match="tol must be > 0"):
        SpectralClustering(tol=0.0)
    x = np.random.RandomState(0).randn(20, 3).astype(np.float32)
    with pytest.raises(ValueError, match=r"rank D \+ 1, it has no more eigenvectors"):
        SpectralClustering(5).fit(x)
    with pytest.raises(ValueError, match=r"min\(3, 4\)"):
        SpectralClustering(4).fit(x[:3])
    with pytest.raises(ValueError, match="expected n_clusters = 2 <= block"):
        SpectralClustering(2, block=5).fit(x)
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[7, 1] = bad
        with pytest.raises(ValueError, match="NaN or infinite"):
            SpectralClustering(2).fit(y)
    with pytest.raises(ValueError, match="expected a"):
        SpectralClustering(2).fit(x[0])
    one = SpectralClustering(1).fit(x[:1])
    assert one.labels_.tolist() == [0] and one.labels_.dtype == np.int64 and one.n_iter_ == 0 and one.maps_.shape == (1, 1)


def test_build_plumbing():
    from texttoaudiogrounding_amd import dispatch, lib, ops
    header = open(os.path.join(ROOT, "include", "tag_hip.h")).read()
    makefile = open(os.path.join(ROOT, "texttoaudiogrounding_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bspectral\.hip\b", makefile, flags=re.M)
    for s in SYMBOLS:
        assert s in lib.declared_symbols() and re.search(rf"\b{s}\s*\(", header), s
    chain = int(re.search(r"^#define TAG_SPECTRAL_CHAIN (\d+)$", header, flags=re.M).group(1))
    assert ops.SPECTRAL_CHAIN == dispatch.SPECTRAL_CHAIN == chain
    src = open(os.path.join(ROOT, "texttoaudiogrounding_amd", "csrc", "spectral.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "cooperative" not in code.lower() and "__shared__" not in code
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in code
