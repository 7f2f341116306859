"""Host-side checks of the BERTScore phrase-to-label map (csrc/bertscore.hip, dispatch.bertscore_map, utils/bertscore_map.py,
tools/prepare_phrase_bertscore.py): the build plumbing and the argument checks of the loaded library, which refuse before any
launch; the fp64 restatement of tests/bertscore_ref.py against cases worked out by hand; the wrapper's packing and chunking and
the tool's table with dispatch.bertscore_map replaced by the restatement; every argument error of the wrapper."""
import ctypes
import importlib.util
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests import bertscore_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["tag_bertscore_map", "tag_bertscore_map_ws_bytes"]
TAG_EINVAL = -1                      # include/tag_hip.h


def _tool():
    spec = importlib.util.spec_from_file_location("prepare_phrase_bertscore_tool", os.path.join(ROOT, "tools", "prepare_phrase_bertscore.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_bertscore_hip_is_built_and_declared_with_matching_arity():
    from texttoaudiogrounding_amd import lib
    header = open(os.path.join(ROOT, "include", "tag_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = dict(re.findall(r"\b(tag_bertscore[a-z_]*)\s*\(([^)]*)\)\s*;", code))
    assert sorted(protos) == SYMBOLS
    assert sorted(s for s in lib.declared_symbols() if s.startswith("tag_bertscore")) == SYMBOLS
    for name, params in protos.items():
        assert len(params.split(",")) == len(lib._SIGS[name][1]), name
    assert lib._SIGS["tag_bertscore_map_ws_bytes"][0] is ctypes.c_size_t and lib._SIGS["tag_bertscore_map"][0] is ctypes.c_int
    assert int(re.search(r"#define TAG_ABI_VERSION (\d+)", header).group(1)) == lib.ABI_VERSION == 3
    make = open(os.path.join(ROOT, "texttoaudiogrounding_amd", "csrc", "Makefile")).read()
    assert "bertscore.hip" in re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    from texttoaudiogrounding_amd import dispatch, ops
    assert ops.bertscore_map is dispatch.bertscore_map and dispatch.BERTSCORE_SLOTS == (8, 16, 32)
    assert [dispatch.bertscore_slot(L) for L in (1, 8, 9, 16, 17, 32)] == [8, 8, 16, 16, 32, 32]
    with pytest.raises(ValueError, match="exceed the largest slot 32"):
        dispatch.bertscore_slot(33)


def test_library_checks_its_arguments_before_any_launch():
    from texttoaudiogrounding_amd import lib
    h = lib.load()
    assert h.tag_abi_version() == 3
    # 40 phrases of slot 16 = 5 row blocks, 527 labels of slot 8 = 33 column tiles: one slice per tile, 16 bytes per phrase and slice
    assert lib.query("tag_bertscore_map_ws_bytes", 40, 527, 768, 16, 8) == 33 * 40 * 16
    assert lib.query("tag_bertscore_map_ws_bytes", 1, 1, 1, 8, 8) == 16
    big = 2**31 - 128
    for shape in ((0, 4, 4, 8, 8), (4, 0, 4, 8, 8), (4, 4, 0, 8, 8), (-1, 4, 4, 8, 8), (4, 4, 4, 4, 8), (4, 4, 4, 8, 64), (4, 4, 4, 12, 8),
                  (big // 8, 4, 4, 8, 8), (4, big // 32, 4, 8, 32)):
        assert lib.query("tag_bertscore_map_ws_bytes", *shape) == 0, shape
    assert lib.query("tag_bertscore_map_ws_bytes", big // 8 - 1, 4, 4, 8, 8) > 0
    # refused with a message before any launch (no GPU is touched): the pointers below are never dereferenced on the host
    p = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)

    def args(a=p, lda=8, a_len=p, a_w=p, b=p, ldb=8, b_len=p, b_w=p, sa=8, sb=8, N=4, C=4, D=8, outs=(p,) * 4, scores=None, ws=p):
        return (a, lda, a_len, a_w, b, ldb, b_len, b_w, sa, sb, N, C, D) + tuple(outs) + (scores, ws, None)
    bad = [(args(N=0), b"N, C, D must be >= 1 (got 0, 4, 8)"), (args(C=-3), b"(got 4, -3, 8)"), (args(D=0), b"(got 4, 4, 0)"),
           (args(sa=4), b"slot_a = 4, slot_b = 8: the accepted slots are 8, 16 and 32"),
           (args(sb=24), b"slot_a = 8, slot_b = 24: the accepted slots are 8, 16 and 32"),
           (args(lda=7), b"lda = 7, ldb = 8 must be >= D = 8"), (args(ldb=3), b"lda = 8, ldb = 3 must be >= D = 8"),
           (args(N=big // 8), b"N = 268435440 phrases of slot 8 are more than 2147483519 token rows (row index limit)"),
           (args(C=big // 32, sb=32), b"C = 67108860 labels of slot 32 are more than 2147483519 token rows (column index limit)"),
           (args(D=2**31 - 32, lda=2**31 - 1, ldb=2**31 - 1), b"D = 2147483616 exceeds 2147483615 (chunk index limit)")]
    bad += [(args(**{k: None}), b"argument check failed") for k in ("a", "a_len", "a_w", "b", "b_len", "b_w", "ws")]
    bad += [(args(outs=(p,) * i + (None,) + (p,) * (3 - i)), b"argument check failed") for i in range(4)]
    for call_args, message in bad:
        assert h.tag_bertscore_map(*call_args) == TAG_EINVAL and message in h.tag_last_error(), (message, h.tag_last_error())


def test_restatement_on_hand_computed_cases():
    f64 = torch.float64
    e = torch.eye(4, dtype=f64)
    # phrase: tokens e0, (e0 + e1) / sqrt 2 given as 3 (e0 + e1) (normalised inside), a third slot past the length;
    # label 0: e0, e1;  label 1: e2 alone (its second slot is past the length and holds e0, which must not be used)
    a = torch.stack([e[0], 3 * (e[0] + e[1]), e[2]])[None]
    b = torch.stack([torch.stack([e[0], 5 * e[1]]), torch.stack([e[2], e[0]])])
    a_len, b_len = torch.tensor([2]), torch.tensor([2, 1])
    a_w, b_w = torch.tensor([[1.0, 3.0, 100.0]], dtype=f64), torch.tensor([[1.0, 1.0], [2.0, 100.0]], dtype=f64)
    prf = R.scores(a, a_len, a_w, b, b_len, b_w)
    h = 0.5 ** 0.5
    # label 0: s = [[1, 0], [h, h]]: row maxima 1, h -> P = (1 + 3 h) / 4; column maxima 1, h -> R = (1 + h) / 2
    P0, R0 = (1 + 3 * h) / 4, (1 + h) / 2
    assert abs(prf[0, 0, 0].item() - P0) < 1e-15 and abs(prf[1, 0, 0].item() - R0) < 1e-15
    assert abs(prf[2, 0, 0].item() - 2 * P0 * R0 / (P0 + R0)) < 1e-15
    # label 1: every valid cosine is 0 -> P = R = 0, and P + R == 0 gives F = 0 (not NaN)
    assert prf[:, 0, 1].tolist() == [0.0, 0.0, 0.0]
    assert R.select(prf)[0].tolist() == [0]
    # length 1 on both sides: P = R = F = the one cosine, whatever the weight
    one = R.scores(a[:, 1:2], torch.tensor([1]), torch.tensor([[0.25]], dtype=f64), b[:1, :1], torch.tensor([1]),
                   torch.tensor([[7.0]], dtype=f64))
    assert np.allclose(one[:, 0, 0].numpy(), [h, h, h], atol=1e-15)
    # a zero weight sum gives P = 0 (and then F = 0), R is unaffected; the same for the label side
    zp = R.scores(a, a_len, torch.zeros(1, 3, dtype=f64), b, b_len, b_w)
    assert zp[0, 0, 0].item() == 0.0 and abs(zp[1, 0, 0].item() - R0) < 1e-15 and zp[2, 0, 0].item() == 0.0
    zr = R.scores(a, a_len, a_w, b, b_len, torch.zeros(2, 2, dtype=f64))
    assert abs(zr[0, 0, 0].item() - P0) < 1e-15 and zr[1, 0, 0].item() == 0.0 and zr[2, 0, 0].item() == 0.0
    # label 0 negated: s = [[-1, 0], [-h, -h]]: row maxima 0, -h; column maxima -h, 0
    neg = R.scores(a, a_len, a_w, -b, b_len, b_w)
    assert abs(neg[0, 0, 0].item() - (0 - 3 * h) / 4) < 1e-15 and abs(neg[1, 0, 0].item() - (-h + 0) / 2) < 1e-15
    # every valid cosine negative: -(e0 + e1) against the phrase gives s = [[-h], [-1]], and neither the padded third row (which
    # scores 0) nor anything else past a length enters a maximum: P = (-h - 3) / 4, R = -h
    allneg = R.scores(a, a_len, a_w, -(e[0] + e[1])[None, None, :].repeat(1, 2, 1), torch.tensor([1]), b_w[:1])
    assert abs(allneg[0, 0, 0].item() - (-h - 3) / 4) < 1e-15 and abs(allneg[1, 0, 0].item() + h) < 1e-15
    # ties go to the lowest index
    tie = R.scores(a, a_len, a_w, torch.cat([b[1:], b[:1], b[:1]]), torch.tensor([1, 2, 2]), torch.cat([b_w[1:], b_w[:1], b_w[:1]]))
    assert R.select(tie)[0].tolist() == [1] and tie[2, 0, 1] == tie[2, 0, 2]


def test_special_token_weights():
    from texttoaudiogrounding_amd import dispatch
    from texttoaudiogrounding_amd.utils.bertscore_map import token_weights
    lens = [1, 2, 3, 5]
    want = [[0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 1, 1, 1, 0, 0]]
    assert token_weights(lens, 6).tolist() == want and token_weights(lens, 6).dtype == np.float32
    assert R.default_weights(lens, 6).tolist() == want
    assert dispatch.bertscore_default_weights(torch.tensor(lens, dtype=torch.int32), 6).tolist() == want
    assert token_weights(lens, 6, special_tokens=False).tolist() == [[1] * n + [0] * (6 - n) for n in lens]
    assert R.default_weights(lens, 6, special_tokens=False).tolist() == token_weights(lens, 6, special_tokens=False).tolist()
    # a phrase of [CLS] x y [SEP] against a label of [CLS] x [SEP]: only x and y weigh, the special tokens still match
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(1, 4, 6, generator=g, dtype=torch.float64), torch.randn(1, 3, 6, generator=g, dtype=torch.float64)
    prf = R.scores(a, [4], R.default_weights([4], 4), b, [3], R.default_weights([3], 3))
    s = R.unit(a[0]) @ R.unit(b[0]).T
    assert abs(prf[0, 0, 0].item() - (s[1].max() + s[2].max()).item() / 2) < 1e-15 and abs(prf[1, 0, 0].item() - s[:, 1].max().item()) < 1e-15
    # an item of length 2 has no weight left under the default weights: P = 0 for a phrase, R = 0 for a label
    assert R.scores(a, [2], R.default_weights([2], 4), b, [3], R.default_weights([3], 3))[0, 0, 0].item() == 0.0
    assert R.scores(a, [4], R.default_weights([4], 4), b, [2], R.default_weights([2], 3))[1, 0, 0].item() == 0.0


@pytest.fixture()
def host_dispatch(monkeypatch):
    from texttoaudiogrounding_amd import dispatch
    calls = []

    def stand_in(a, a_len, a_w, b, b_len, b_w, want_scores=False, normalize=True):
        calls.append((tuple(a.shape), tuple(b.shape)))
        return R.host_bertscore_map(a, a_len, a_w, b, b_len, b_w, want_scores=want_scores, normalize=normalize)
    monkeypatch.setattr(dispatch, "bertscore_map", stand_in)
    return calls


def _ragged(seed, items, L, D):
    g = np.random.RandomState(seed)
    return [g.randn(g.randint(1, L + 1), D).astype(np.float32) for _ in range(items)]


def test_wrapper_packs_chunks_and_weighs(host_dispatch):
    from texttoaudiogrounding_amd.utils.bertscore_map import BertScoreMap, pack_tokens, token_weights
    labels, phrases = _ragged(1, 7, 5, 12), _ragged(2, 11, 9, 12)
    phrases[4] = phrases[4][:1]
    tok, lens = pack_tokens(phrases)
    assert tok.shape == (11, max(len(p) for p in phrases), 12) and lens.tolist() == [len(p) for p in phrases] and lens.dtype == np.int32
    assert all(np.array_equal(tok[k, : len(p)], p) and not tok[k, len(p):].any() for k, p in enumerate(phrases))
    ltok, llen = pack_tokens(labels)
    for special in (True, False):
        want = R.scores(torch.from_numpy(tok).double(), lens, torch.from_numpy(token_weights(lens, tok.shape[1], special)),
                        torch.from_numpy(ltok).double(), llen, torch.from_numpy(token_weights(llen, ltok.shape[1], special))).float()
        best, f, p, r = R.select(want)
        del host_dispatch[:]
        whole = BertScoreMap(labels, device="cpu", special_tokens=special).map(phrases, want_scores=True)
        assert len(host_dispatch) == 1 and host_dispatch[0][1] == ltok.shape
        assert whole.best.dtype == np.int64 and whole.best.tolist() == best.tolist() and whole.scores.shape == (3, 11, 7)
        assert np.array_equal(whole.best_f, f) and np.array_equal(whole.best_p, p) and np.array_equal(whole.best_r, r)
        assert np.array_equal(whole.scores, want.numpy())
        del host_dispatch[:]
        parts = BertScoreMap(labels, device="cpu", chunk_rows=4, special_tokens=special).map(phrases, want_scores=True)
        assert [c[0][0] for c in host_dispatch] == [4, 4, 3]                  # three calls, each as wide as its longest phrase
        assert [c[0][1] for c in host_dispatch] == [max(len(p) for p in phrases[k: k + 4]) for k in (0, 4, 8)]
        assert all(np.array_equal(x, y) for x, y in zip(parts, whole))
        assert BertScoreMap(labels, device="cpu", special_tokens=special).map(phrases).scores is None
    # explicit weights (an idf table) per token
    wl, wp = [np.arange(1, len(v) + 1) for v in labels], [np.full(len(v), 0.5) for v in phrases]
    given = BertScoreMap(labels, device="cpu", label_weights=wl).map(phrases, phrase_weights=wp, want_scores=True)
    a_w, b_w = np.zeros(tok.shape[:2], np.float32), np.zeros(ltok.shape[:2], np.float32)
    for k, v in enumerate(wp):
        a_w[k, : len(v)] = v
    for k, v in enumerate(wl):
        b_w[k, : len(v)] = v
    want = R.scores(torch.from_numpy(tok).double(), lens, torch.from_numpy(a_w), torch.from_numpy(ltok).double(), llen, torch.from_numpy(b_w))
    assert np.array_equal(given.scores, want.float().numpy())
    for call, message in [(lambda: BertScoreMap([]), "at least one item"),
                          (lambda: BertScoreMap([np.zeros((33, 4))]), r"33 tokens; an item has 1 \.\. 32 tokens"),
                          (lambda: BertScoreMap([np.zeros((0, 4))]), r"0 tokens; an item has 1 \.\. 32 tokens"),
                          (lambda: BertScoreMap([np.zeros(4)]), "expected a"),
                          (lambda: BertScoreMap(labels, chunk_rows=0), "chunk_rows = 0 must be >= 1"),
                          (lambda: BertScoreMap(labels, label_weights=wl[:3]), "3 weight rows for 7 items"),
                          (lambda: BertScoreMap(labels).map([np.zeros((2, 5))]), r"expected a \(L, 12\) array"),
                          (lambda: BertScoreMap(labels).map(phrases, phrase_weights=[np.ones(40)] * 11), "40 weights for")]:
        with pytest.raises(ValueError, match=message):
            call()


def test_tool_writes_the_table(host_dispatch, tmp_path):
    tool = _tool()
    labels = {f"label {k}": v for k, v in enumerate(_ragged(3, 5, 4, 10))}
    phrases = {f"a phrase {k}": v for k, v in enumerate(_ragged(4, 6, 7, 10))}
    paths = {k: str(tmp_path / k) for k in ("p.pkl", "l.pkl", "o.tsv")}
    for name, table in (("p.pkl", phrases), ("l.pkl", labels)):
        with open(paths[name], "wb") as f:
            pickle.dump(table, f)
    from texttoaudiogrounding_amd.utils.bertscore_map import BertScoreMap
    for flags, special in (([], True), (["--no_special_tokens"], False)):
        args = tool.build_parser().parse_args(["--phrase_emb", paths["p.pkl"], "--label_emb", paths["l.pkl"], "--output", paths["o.tsv"],
                                               "--device", "cpu"] + flags)
        assert args.no_special_tokens == (not special)
        tool.main(args)
        want = BertScoreMap(list(labels.values()), device="cpu", special_tokens=special).map(list(phrases.values()))
        lines = open(paths["o.tsv"]).read().split("\n")
        assert lines[0] == "phrase\tindex\tsim" and lines[-1] == "" and len(lines) == 8
        for line, phrase, index, f in zip(lines[1:], phrases, want.best, want.best_f):
            assert line == f"{phrase}\t{index}\t{str(np.float32(f))}" and np.float32(line.split("\t")[2]) == f
    assert tool.build_parser().parse_args(["--phrase_emb", "p", "--label_emb", "l", "--output", "o"]).device == "cuda:0"
    out = str(tmp_path / "x.tsv")
    tool.write_table([("a dog", 3, np.float32(0.25)), ("b", 0, np.float32(1 / 3))], out)
    assert open(out).read() == "phrase\tindex\tsim\na dog\t3\t0.25\nb\t0\t0.33333334\n"


def test_wrapper_refuses_bad_arguments_and_host_tensors():
    from texttoaudiogrounding_amd import ops
    z = torch.zeros(2, 3, 4)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)                           # noqa: E731
    cases = [
        (ValueError, r"a_len: lengths must lie in \[1, 3\] .* got \[0, 3\]", dict(a_len=i32(0, 3))),
        (ValueError, r"b_len: lengths must lie in \[1, 3\] .* got \[1, 4\]", dict(b_len=i32(1, 4))),
        (ValueError, r"a: L = 40 tokens per item exceed the limit 32", dict(a=torch.zeros(2, 40, 4))),
        (ValueError, r"a_len: lengths must lie in \[1, 32\] \(L = 40, the limit is 32 tokens per item\), got \[1, 33\]",
         dict(a=torch.zeros(2, 40, 4), a_len=i32(33, 1))),
        (RuntimeError, r"b \(2, 3, 5\) on cpu: expected a's device cpu and D = 4", dict(b=torch.zeros(2, 3, 5))),
        (RuntimeError, r"b \(2, 3, 4\) on meta: expected a's device cpu", dict(b=torch.zeros(2, 3, 4, device="meta"))),
        (RuntimeError, r"a: expected a float32 .* got torch.float64", dict(a=z.double())),
        (RuntimeError, r"b: expected a float32 .* got torch.float16", dict(b=z.half())),
        (RuntimeError, r"a: expected a float32 \(items >= 1, L >= 1, D >= 1\) tensor", dict(a=torch.zeros(2, 4))),
        (RuntimeError, r"a: expected a float32", dict(a=z.numpy())),
        (RuntimeError, r"a_len: expected an int32 / int64 \(2,\) tensor", dict(a_len=torch.tensor([1.0, 2.0]))),
        (RuntimeError, r"b_len: expected an int32 / int64 \(2,\) tensor", dict(b_len=i32(1, 2, 3))),
        (RuntimeError, r"a_w: expected a float32 \(2, 3\) tensor", dict(a_w=torch.zeros(2, 2))),
        (RuntimeError, r"b_w: expected a float32 \(2, 3\) tensor", dict(b_w=torch.zeros(2, 3, dtype=torch.float64))),
        (RuntimeError, r"expected tensors on the MI355X \(cuda\) device, got cpu; the HIP path has no CPU fallback", dict()),
    ]
    for exc, message, change in cases:
        kw = dict(a=z, a_len=None, a_w=None, b=z, b_len=None, b_w=None)
        kw.update(change)
        with pytest.raises(exc, match=message):
            ops.bertscore_map(kw["a"], kw["a_len"], kw["a_w"], kw["b"], kw["b_len"], kw["b_w"])
    from texttoaudiogrounding_amd.utils.bertscore_map import BertScoreMap
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BertScoreMap([np.ones((2, 4), np.float32)], device="cpu").map([np.ones((3, 4), np.float32)])
