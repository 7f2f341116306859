"""csrc/spectral.hip and utils/phrase_cluster.SpectralClustering against fp64 (tests/spectral_ref.py) and the recorded output of the
reference's sklearn recipe (tests/golden/make_golden_spectral.py).

Bounds.  gram: a slice of L = ops.SPECTRAL_CHAIN rows is one fp32 chain in which no term passes through more than L roundings, and
the slices are added in fp64: |err_ab| <= L 2^-24 sum_i |w_i P_ia Q_ib| + one fp64 ulp of that sum, whatever N is.  rows: the
arithmetic is fp64 and each output is rounded to fp32 once; the fp64 sums are folded in another order than numpy's, which can move
a result across a rounding boundary: one fp32 ulp, 2^-23 relative.  apply: (Dp + 2) 2^-24 (|Y||T| + |e X|).  fit: every vector of
``maps_`` within 8 x the recorded emulated-fp32 error of tests/spectral_ref.py of sklearn's recorded vector (the MFMA adds in
another order than numpy), relative to the vector's largest entry."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import spectral_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [("blobs600", 6), ("edge600", 6), ("blobs257", 4), ("blobs1000", 10)]
NAMES = [c[0] for c in CASES]
WIDTHS = [(1, 1), (1, 33), (31, 1), (32, 32), (33, 65), (130, 130)]
IDS = lambda s: "x".join(map(str, s))       # noqa: E731


def chain():
    from texttoaudiogrounding_amd import ops
    return ops.SPECTRAL_CHAIN


def row_counts():
    L = chain()
    return [1, 2, L - 1, L, L + 1, 2 * L + 3, 1031]


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
def fitted(name):
    """One device fit per recorded case, shared and left unchanged."""
    from texttoaudiogrounding_amd.utils.phrase_cluster import SpectralClustering
    return SpectralClustering(dict(CASES)[name], random_state=1, device="cuda:0").fit(golden()[f"{name}/x"])


def padded(a, pad, dev):
    """A device view of ``a`` inside a wider buffer whose padding holds NaN: a read past the width poisons the result."""
    a = np.asarray(a, dtype=np.float32)
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), device=dev, dtype=torch.float32)
    buf[:, :a.shape[1]] = torch.from_numpy(a).to(dev)
    return buf[:, :a.shape[1]]


def check_gram(out, P, Q, w, tag):
    want, mag = R.gram_ref(P, Q, w)
    got = out.cpu().numpy()
    assert out.dtype == torch.float64 and got.shape == want.shape
    bound = R.gram_bound(mag, chain())
    err = np.abs(got - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{tag}: largest |err| {err.max():.3g}, {worst:.3f} of the bound")
    assert np.all(err <= bound)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# spectral_gram
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", WIDTHS, ids=IDS)
def test_gram_is_within_the_chain_bound_of_fp64(dev, widths):
    from texttoaudiogrounding_amd import ops
    p, q = widths
    for N in row_counts():
        g = np.random.RandomState(N + 7 * p + 13 * q)
        P, Q = g.randn(N, p).astype(np.float32), g.randn(N, q).astype(np.float32)
        w = g.uniform(0.1, 2.0, size=N).astype(np.float32)
        Pd, Qd = padded(P, 3, dev), padded(Q, 5, dev)
        check_gram(ops.spectral_gram(Pd, Qd), P, Q, None, f"N {N} {p} x {q}")
        check_gram(ops.spectral_gram(Pd, Qd, torch.from_numpy(w).to(dev)), P, Q, w, f"N {N} {p} x {q} weighted")
        check_gram(ops.spectral_gram(torch.from_numpy(P).to(dev), torch.from_numpy(Q).to(dev)), P, Q, None, f"N {N} {p} x {q} dense")


def test_gram_of_five_tiles_a_side(dev):
    from texttoaudiogrounding_amd import ops
    N, p = 1031, 513
    g = np.random.RandomState(5)
    P, Q = g.randn(N, p).astype(np.float32), g.randn(N, p).astype(np.float32)
    w = g.uniform(0.1, 2.0, size=N).astype(np.float32)
    Pd, Qd = padded(P, 3, dev), padded(Q, 1, dev)
    a = check_gram(ops.spectral_gram(Pd, Qd, torch.from_numpy(w).to(dev)), P, Q, w, "1031 513 x 513 weighted")
    b = ops.spectral_gram(Pd, Qd, torch.from_numpy(w).to(dev)).cpu().numpy()
    assert np.array_equal(a.view(np.int64), b.view(np.int64))              # the same bits on every run
    s = check_gram(ops.spectral_gram(Pd, Pd), P, P, None, "1031 513 x 513 P is Q")
    assert np.array_equal(s.view(np.int64), s.T.view(np.int64))
    # the half that was computed holds the bits of the full product of two distinct buffers with the same values
    full = check_gram(ops.spectral_gram(Pd, padded(P, 1, dev)), P, P, None, "1031 513 x 513 two buffers")
    assert np.array_equal(np.triu(s).view(np.int64), np.triu(full).view(np.int64))


@pytest.mark.parametrize("p", [1, 31, 130])
def test_gram_of_a_matrix_with_itself_is_bit_symmetric(dev, p):
    from texttoaudiogrounding_amd import ops
    for N in row_counts():
        g = np.random.RandomState(N + p)
        P = g.randn(N, p).astype(np.float32)
        w = g.uniform(0.1, 2.0, size=N).astype(np.float32)
        Pd = padded(P, 2, dev)
        for wv in (None, w):
            out = ops.spectral_gram(Pd, Pd, None if wv is None else torch.from_numpy(wv).to(dev))
            got = check_gram(out, P, P, wv, f"N {N} {p} x {p} P is Q{'' if wv is None else ' weighted'}")
            assert np.array_equal(got.view(np.int64), got.T.view(np.int64))
            again = ops.spectral_gram(Pd, Pd, None if wv is None else torch.from_numpy(wv).to(dev)).cpu().numpy()
            assert np.array_equal(got.view(np.int64), again.view(np.int64))


def test_gram_refuses_bad_arguments_before_any_launch(dev):
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.lib import load
    assert ops.query("tag_spectral_chain") == ops.SPECTRAL_CHAIN
    L = ops.SPECTRAL_CHAIN
    assert ops.query("tag_spectral_gram_ws_bytes", 2 * L + 3, 33, 65) == 3 * 33 * 65 * 4
    assert ops.query("tag_spectral_gram_ws_bytes", L, 1, 1) == 4 and ops.query("tag_spectral_gram_ws_bytes", 0, 4, 4) == 0
    assert ops.query("tag_spectral_gram_ws_bytes", 10, 32769, 4) == 0
    P = torch.ones(8, 4, device=dev)
    out = torch.full((4, 4), 7.0, device=dev, dtype=torch.float64)
    ws = torch.empty(64, device=dev, dtype=torch.float64)
    fn, st = load().tag_spectral_gram, torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()        # noqa: E731
    for args, word in (((ptr(P), 4, ptr(P), 4, None, ptr(out), 4, 0, 4, 4, ptr(ws)), "N, p, q must be >= 1 (got 0, 4, 4)"),
                       ((ptr(P), 4, ptr(P), 4, None, ptr(out), 4, 8, 0, 4, ptr(ws)), "(got 8, 0, 4)"),
                       ((ptr(P), 3, ptr(P), 4, None, ptr(out), 4, 8, 4, 4, ptr(ws)), "ldp = 3"),
                       ((ptr(P), 4, ptr(P), 4, None, ptr(out), 3, 8, 4, 4, ptr(ws)), "ldo = 3"),
                       ((ptr(P), 4, ptr(P), 4, None, ptr(out), 4, 8, 4, 4, None), "argument check failed"),
                       ((None, 4, ptr(P), 4, None, ptr(out), 4, 8, 4, 4, ptr(ws)), "argument check failed")):
        assert fn(*args, st) != 0
        assert word in load().tag_last_error().decode(), (word, load().tag_last_error().decode())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                         # nothing was launched
    with pytest.raises(RuntimeError, match="expected P's device .* and N = 8 rows"):
        ops.spectral_gram(P, torch.ones(7, 4, device=dev))
    with pytest.raises(RuntimeError, match=r"w: expected float32 \(8,\)"):
        ops.spectral_gram(P, P, torch.ones(7, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.spectral_gram(torch.ones(8, 4), torch.ones(8, 4))
    with pytest.raises(RuntimeError, match="expected a float32 matrix"):
        ops.spectral_gram(P.double(), P)


# ---------------------------------------------------------------------------------------------------------------------
# spectral_rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 5, 33, 512])
def test_rows_equal_fp64_at_fp32_rounding(dev, D):
    from texttoaudiogrounding_amd import ops
    N = 70
    g = np.random.RandomState(D)
    x = g.randn(N, D).astype(np.float32)
    if D == 1:
        x = np.abs(x)                               # (on a line a row opposite to the rest has no degree; that is the next test)
    x[11] = 0
    u = R.unit_rows(x, np.float32)
    Yw, sw, ew, deg = R.rows_ref(u)
    assert deg.min() > 0
    t = torch.from_numpy(u.astype(np.float64).sum(0)).to(dev)
    Y, s, e = ops.spectral_rows(padded(u, 3, dev), t)
    assert tuple(Y.shape) == (N, D + 1) and Y.stride(0) % 4 == 0 and Y.data_ptr() % 16 == 0
    for got, want, name in ((Y, Yw, "Y"), (s, sw, "s"), (e, ew, "e")):
        got = got.cpu().numpy().astype(np.float64)
        err = np.abs(got - want)
        print(f"D {D} {name}: largest error {float((err / np.abs(want).max()).max()):.3g} of the largest entry")
        assert got.shape == want.shape and np.all(err <= 2.0 ** -23 * np.abs(want))
    assert bool((Y[11, :D] == 0).all()) and float(Y[11, D]) > 0


def test_rows_report_a_row_without_degree(dev):
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.utils.phrase_cluster import SpectralClustering
    for u in ([[1.0, 0.0], [-1.0, 0.0]], [[1.0], [-1.0]]):
        u = torch.tensor(u, device=dev)
        Y, s, e = ops.spectral_rows(u, u.double().sum(0))
        assert s.tolist() == [0.0, 0.0] and e.tolist() == [0.0, 0.0] and bool((Y == 0).all())
        with pytest.raises(ValueError, match="row 0 has degree <= 0"):
            SpectralClustering(1, device=dev).fit(u)
    with pytest.raises(RuntimeError, match=r"t: expected float64 \(2,\)"):
        ops.spectral_rows(torch.ones(3, 2, device=dev), torch.ones(2, device=dev))
    # one opposite row among others keeps a positive degree and is not reported
    u = torch.tensor([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0]], device=dev)
    _, s, _ = ops.spectral_rows(u, u.double().sum(0))
    assert bool((s > 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# spectral_apply
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dp,pad", [(2, 2), (34, 1), (513, 3)])
def test_apply_is_within_the_bound_of_fp64(dev, Dp, pad):
    """pad: (2, 2) and (513, 3) give 16-byte aligned rows of Y (one load of four floats), (34, 1) does not."""
    from texttoaudiogrounding_amd import ops
    for N, b in [(N, b) for N in (1, 257) for b in (1, 6, 33)] + [(300, 130)]:
        g = np.random.RandomState(N + 3 * Dp + 5 * b)
        Y, T, X = g.randn(N, Dp).astype(np.float32), g.randn(Dp, b).astype(np.float32), g.randn(N, b).astype(np.float32)
        e = g.uniform(0.0, 1.0, size=N).astype(np.float32)
        want, mag = R.apply_ref(Y, T, e, X)
        Xd = padded(X, 1, dev)
        out = ops.spectral_apply(padded(Y, pad, dev), padded(T, 2, dev), torch.from_numpy(e).to(dev), Xd)
        got = out.cpu().numpy().astype(np.float64)
        err, bound = np.abs(got - want), R.apply_bound(mag, Dp)
        print(f"N {N} Dp {Dp} b {b}: largest |err| {err.max():.3g}, {float((err / bound).max()):.3f} of the bound")
        assert out.dtype == torch.float32 and got.shape == (N, b) and np.all(err <= bound)
        again = ops.spectral_apply(padded(Y, pad, dev), padded(T, 2, dev), torch.from_numpy(e).to(dev), Xd, out=Xd)
        assert again.data_ptr() == Xd.data_ptr() and np.array_equal(again.cpu().numpy().view(np.int32), out.cpu().numpy().view(np.int32))


def test_apply_refuses_bad_arguments(dev):
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.lib import load
    Y, T, e, X = torch.ones(5, 3, device=dev), torch.ones(3, 2, device=dev), torch.ones(5, device=dev), torch.ones(5, 2, device=dev)
    with pytest.raises(RuntimeError, match=r"needs T \(3, b\) and X \(5, b\)"):
        ops.spectral_apply(Y, torch.ones(4, 2, device=dev), e, X)
    with pytest.raises(RuntimeError, match=r"needs T \(3, b\) and X \(5, b\)"):
        ops.spectral_apply(Y, T, e, torch.ones(5, 3, device=dev))
    with pytest.raises(RuntimeError, match=r"e: expected float32 \(5,\)"):
        ops.spectral_apply(Y, T, torch.ones(4, device=dev), X)
    with pytest.raises(RuntimeError, match="out: expected a float32"):
        ops.spectral_apply(Y, T, e, X, out=torch.ones(5, 3, device=dev))
    out = torch.full((5, 2), 7.0, device=dev)
    fn, st = load().tag_spectral_apply, torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()        # noqa: E731
    for args, word in (((ptr(Y), 3, ptr(T), 2, ptr(e), ptr(X), 2, ptr(out), 2, 0, 3, 2), "(got 0, 3, 2)"),
                       ((ptr(Y), 2, ptr(T), 2, ptr(e), ptr(X), 2, ptr(out), 2, 5, 3, 2), "ldy = 2"),
                       ((ptr(Y), 3, ptr(T), 1, ptr(e), ptr(X), 2, ptr(out), 2, 5, 3, 2), "ldt = 1"),
                       ((ptr(Y), 3, ptr(T), 2, None, ptr(X), 2, ptr(out), 2, 5, 3, 2), "argument check failed")):
        assert fn(*args, st) != 0
        assert word in load().tag_last_error().decode(), (word, load().tag_last_error().decode())
    rows = load().tag_spectral_rows
    assert rows(ptr(Y), 2, ptr(torch.ones(3, device=dev, dtype=torch.float64)), ptr(out), 4, ptr(e), ptr(e), 5, 3, st) != 0
    assert "ldu = 2" in load().tag_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                         # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# SpectralClustering
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fit_reproduces_sklearns_embedding_and_partition(name):
    g, model = golden(), fitted(name)
    k = dict(CASES)[name]
    N = g[f"{name}/x"].shape[0]
    assert model.maps_.shape == (N, k) and model.maps_.dtype == np.float32 and model.labels_.dtype == np.int64
    err = R.vector_errors(model.maps_, g[f"{name}/maps"])
    tol = 8 * float(g[f"{name}/err32"])
    print(f"{name}: block {model.block_}, {model.n_iter_} iterations, residuals {['%.2g' % v for v in model.residuals_]}, "
          f"per-vector error {err.max():.3g} of the largest entry (allowed {tol:.3g}, emulated fp32 {float(g[f'{name}/err32']):.3g})")
    assert np.all(err <= tol)
    assert len(model.residuals_) == model.n_iter_ and model.residuals_[-1] <= model.tol
    assert np.abs(model.eigenvalues_ - g[f"{name}/eigenvalues"]).max() <= 1e-5
    assert R.same_partition(model.labels_, g[f"{name}/labels"])             # ARI = 1: every row, every case


@pytest.mark.parametrize("name", NAMES)
def test_two_fits_with_one_seed_give_the_same_bits(name):
    from texttoaudiogrounding_amd.utils.phrase_cluster import SpectralClustering
    first = fitted(name)
    again = SpectralClustering(dict(CASES)[name], random_state=1, device="cuda:0").fit(golden()[f"{name}/x"])
    assert np.array_equal(first.labels_, again.labels_)
    assert np.array_equal(first.maps_.view(np.int32), again.maps_.view(np.int32))
    assert first.residuals_ == again.residuals_ and first.n_iter_ == again.n_iter_


def test_fit_edges(dev):
    from texttoaudiogrounding_amd.utils.phrase_cluster import SpectralClustering
    x = golden()["blobs257/x"]
    one = SpectralClustering(1, random_state=1, device=dev).fit(x)
    assert one.labels_.tolist() == [0] * 257 and one.maps_.shape == (257, 1) and one.block_ == 2
    # the leading vector of the normalised operator is deg^1/2, so sklearn's first map is constant: 1 / sqrt(sum deg)
    assert np.abs(one.maps_ / one.maps_[0, 0] - 1).max() <= 1e-5 and abs(one.eigenvalues_[0] - 1.0) <= 1e-5
    with pytest.raises(ValueError, match=r"rank D \+ 1, it has no more eigenvectors"):
        SpectralClustering(10, device=dev).fit(x)
    full = SpectralClustering(9, random_state=1, device=dev).fit(x)          # k = D + 1: the whole rank, no guard column
    assert full.block_ == 9 and full.maps_.shape == (257, 9) and len(set(full.labels_.tolist())) == 9
    two = SpectralClustering(2, random_state=1, device=dev).fit(torch.tensor([[1.0, 0.1], [0.9, 0.0], [0.0, 1.0], [0.1, 0.9]]))
    assert R.same_partition(two.labels_, [0, 0, 1, 1])


def test_cluster_map_is_the_recorded_one_up_to_the_numbering(dev):
    from texttoaudiogrounding_amd.utils.phrase_cluster import spectral_cluster_map
    with open(os.path.join(GOLDEN, "spectral", "blobs257_result.json")) as f:
        want = json.load(f)
    x = golden()["blobs257/x"]
    out = spectral_cluster_map({f"row {i}": row for i, row in enumerate(x)}, 4, seed=1, device=dev)
    assert set(out) == {"model", "result"} and out["model"].labels_.shape == (257,)
    got = out["result"]
    assert sorted(map(tuple, got.values())) == sorted(map(tuple, want.values()))
    assert [v[0] for v in got.values()] == [v[0] for v in want.values()]    # keys in order of first appearance, as the reference's
    assert all(key == str(out["model"].labels_[int(v[0].split()[1])]) for key, v in got.items())
