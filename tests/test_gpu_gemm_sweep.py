"""csrc/gemm.hip over its edge shapes: the dense GEMM in both tile sizes, every transposition and both arithmetics (exact-fp32
MFMA, bf16-operand MFMA), split-K with ragged and EMPTY K slices, every epilogue (bias, activations 0 / 1 / 3 / 4 / 5, accumulate,
ldc > N), the align scatter epilogue with its clamp and its backward, tag_colsum, tag_relu_backward and the l2norm row kernels,
each against plain fp64 torch on the same seeded CPU inputs (the epilogue in the kernel's order: act(AB + bias + C_old)).  The
shapes are the smallest that reach each branch of the launcher; the split counts the tables claim are asserted through
tag_gemm_ws_bytes, the tile size and loader form through the kernel trace recorded in docs/experiments_gemm_sweep.md.

Every operand is staged in a buffer whose padding (ld > extent) holds NaN, every output in a buffer whose padding columns and
guard row hold a sentinel that must be bit-unchanged afterwards; split-K workspaces start as NaN.

Tolerances are the ones the project already asserts for these kernels with the max-normalised ``relerr``: 2e-6 for products
(bf16-MFMA: against the fp64 product of the bf16-ROUNDED operands), 1e-6 for column sums, 2e-6 align / l2norm forward, 2e-5
align / l2norm gradients, exact where a docstring says exact.  Every comparison also evaluates the same reference in fp32 on
the CPU and prints its distance from fp64 (the ``floor``).  The rule of tests/test_gpu_path.py::assert_crnn_grad_close (bound =
4 x max(floor, 1e-6)) applies to the cases FLOOR_RULE names, where summation order alone pushes the error past the plain bound
(docs/experiments_gemm_sweep.md lists them with error and floor); every other comparison asserts the plain bound.  Nothing is
calibrated on the kernels."""
import functools
import math
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import tag_oracle as O

pytestmark = pytest.mark.gpu

PROD, COLSUM, FWD, GRAD = 2e-6, 1e-6, 2e-6, 2e-5
SENT = -1234.5                      # sentinel of output padding and guard rows (exact in fp32)
#: Names (of close()) whose bound is 4 x max(floor, 1e-6) instead of the plain one.  tanh behind the K = 1031 product on the
#: exact-fp32 MFMA: the pre-activations reach about 4.5, and their summation error (1.3e-6 of that maximum, the fp32 CPU product
#: 0.7e-6) is kept at full size where tanh has slope one while the scale of the comparison shrinks to tanh's 1 -- the fp32 CPU
#: reference is 1.7e-6 from fp64 there, the kernel 3.4e-6.
FLOOR_RULE = re.compile(r"gemm64 \(200, 130, 1031\) ta \d tb \d fp32 bias act 4")


def relerr(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)


@pytest.fixture(scope="module")
def ops(dev):
    from texttoaudiogrounding_amd import ops as _ops
    yield _ops
    _BIG_OUT.clear()
    big_case.cache_clear()
    torch.cuda.empty_cache()


def close(name, got, ref64, ref32, bound):
    """got (HIP) against ref64 within ``bound``; floor = the fp32 CPU reference's own distance from ref64 (a tensor, or that
    distance already taken), printed for comparison.  The comparison runs where ref64 lives (the 134 MB products keep their
    reference on the device).  A reference that is zero to fp64 rounding (the gradient through F.normalize at D = 1) has no
    scale to normalise by: the same bound then holds for the absolute values (the inputs are of order one)."""
    ref64 = torch.as_tensor(ref64).detach()
    got = torch.as_tensor(got).detach().to(ref64.device).double()
    assert ref64.dtype == torch.float64 and got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), name
    zero_ref = ref64.abs().max().item() < 1e-12
    if zero_ref:
        err, how = got.abs().max().item(), "abs (zero reference)"
    else:
        err, how = relerr(got, ref64), "rel"
    if isinstance(ref32, float):
        floor = ref32
    else:
        ref32 = torch.as_tensor(ref32).detach().to(ref64.device).double()
        floor = ref32.abs().max().item() if zero_ref else relerr(ref32, ref64)
    if FLOOR_RULE.match(name):
        bound, how = 4 * max(floor, 1e-6), how + ", floor rule"
    print(f"  {name:66s} err {err:.2e}  fp32-cpu floor {floor:.2e}  bound {bound:.2e}  {how}")
    assert err <= bound, (name, err, floor, bound)


def leaf(t, dtype):
    return t.detach().to(dtype, copy=True).requires_grad_(True)


# ------------------------------------------------------------------------------------------------ staging
def staged(x, ld, dev, off4=False):
    """The CPU matrix x (rows, cols) as a device buffer of leading dimension ld >= cols whose padding is NaN (the kernels
    zero-fill what lies outside a tile; they never read it).  off4: the storage starts 4 bytes after a 16-byte boundary."""
    rows, cols = x.shape
    assert ld >= cols
    flat = torch.full((rows * ld + 8,), float("nan"), device=dev)
    start = (-(flat.data_ptr() // 4)) % 4 + (1 if off4 else 0)
    buf = flat[start:start + rows * ld].view(rows, ld)
    buf[:, :cols] = x.to(dev)
    assert buf.data_ptr() % 16 == (4 if off4 else 0)
    return buf


def out_buffer(M, N, ldc, dev, c_old=None):
    """(M + 1, ldc) of SENT; rows 0..M-1, columns 0..N-1 hold c_old when the call accumulates"""
    buf = torch.full((M + 1, ldc), SENT, device=dev)
    if c_old is not None:
        buf[:M, :N] = c_old.to(dev)
    return buf


def assert_padding_untouched(name, buf, M, N):
    assert bool((buf[:M, N:] == SENT).all()) and bool((buf[M] == SENT).all()), f"{name}: wrote outside C(M, N)"


ACTS = {0: lambda v: v, 1: torch.relu, 3: F.gelu, 4: torch.tanh, 5: torch.sigmoid}       # F.gelu: the erf form


def gemm_ref(A, Bm, bias, c_old, act, dtype, bf):
    """act(A Bm + bias + C_old) in ``dtype`` on the CPU; bf: the operands rounded to bf16 first (products of bf16 values are
    exact in fp32, so what remains is the accumulation)"""
    if bf:
        A, Bm = A.bfloat16(), Bm.bfloat16()
    v = A.to(dtype) @ Bm.to(dtype)
    if bias is not None:
        v = v + bias.to(dtype)
    if c_old is not None:
        v = v + c_old.to(dtype)
    return ACTS[act](v)


def gemm_call(ops, dev, A, Bm, ta, tb, bf, lda=None, ldb=None, ldc=None, bias=None, act=0, c_old=None, ws=None, off4=False):
    """One tag_gemm / tag_gemm_bf16 call on the logical A (M, K), Bm (K, N): A is stored (K, M) when ta, Bm (N, K) when tb.
    Returns the (M, N) view of the output buffer after checking its padding and guard row."""
    (M, K), N = A.shape, Bm.shape[1]
    As, Bs = (A.t() if ta else A), (Bm.t() if tb else Bm)
    lda, ldb, ldc = lda or As.shape[1], ldb or Bs.shape[1], ldc or N
    Ad, Bd = staged(As, lda, dev, off4), staged(Bs, ldb, dev, off4)
    C = out_buffer(M, N, ldc, dev, c_old)
    ops.call("tag_gemm_bf16" if bf else "tag_gemm", ops.ptr(Ad), lda, int(ta), ops.ptr(Bd), ldb, int(tb), ops.ptr(C), ldc, M, N, K,
             ops.ptr(None if bias is None else bias.to(dev)), act, int(c_old is not None), ops.ptr(ws))
    torch.cuda.synchronize()
    assert_padding_untouched(f"gemm ({M},{N},{K}) ta {int(ta)} tb {int(tb)} bf {int(bf)}", C, M, N)
    return C[:M, :N]


def gemm_inputs(M, N, K, seed):
    """A / sqrt(K): the products are of order one, so the activations are compared where they bend"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, K, generator=g) / math.sqrt(K), torch.randn(K, N, generator=g), torch.randn(N, generator=g),
            torch.randn(M, N, generator=g))


TRANS = [(False, False), (False, True), (True, False), (True, True)]
TRANS_IDS = [f"ta{int(a)}-tb{int(b)}" for a, b in TRANS]
MATH_IDS = ["fp32", "bf16"]


def wide(n):
    """a leading dimension above n that keeps rows 16-byte aligned"""
    return (n + 3) // 4 * 4 + 4


def odd(n):
    """an odd leading dimension above n: no row but the first is 16-byte aligned (a_al / b_al false)"""
    return n + 1 if n % 2 == 0 else n + 2


# ------------------------------------------------------------------------------------------------ 1. dense GEMM, 64-tiles
# (M, N, K), all below gemm_big_min 128-tiles and called without a workspace, so gemm_kernel<.., 64, ..>, one K slice:
#   (1, 1, 1)          one element, K of 1: a chunk with 31 zero-filled k, 63 zero-filled rows
#   (3, 2, 5)          K tail of 1 past a float4, M and N below one float4
#   (64, 64, 32)       the smallest FAST problem: one whole tile, one whole chunk (kiters = 1: the tail `step` alone)
#   (64, 64, 33)       one element of K tail: the same tile no longer FAST, two chunks
#   (63, 65, 31)       one row short of a tile / one column into a second tile, K one short of a chunk, odd natural ld
#   (65, 127, 100)     two m-tiles, N one short of two tiles, four chunks with a K tail of 4
#   (200, 130, 1031)   4 x 3 tiles, 33 chunks, K tail of 7 (1031 = 32 * 32 + 7)
DENSE_SHAPES = [(1, 1, 1), (3, 2, 5), (64, 64, 32), (64, 64, 33), (63, 65, 31), (65, 127, 100), (200, 130, 1031)]
LD_SHAPES = {(3, 2, 5), (64, 64, 32), (63, 65, 31), (65, 127, 100), (200, 130, 1031)}      # also with wide and odd ld
# also every epilogue ((3, 2, 5) and not (1, 1, 1): a max-normalised error needs more than one element -- gelu of a single negative
# pre-activation is a cancellation 1 + erf(x) that the fp32 CPU reference resolves no better than the kernel)
EPI_SHAPES = {(3, 2, 5), (64, 64, 32), (63, 65, 31), (200, 130, 1031)}


@pytest.mark.parametrize("bf", [False, True], ids=MATH_IDS)
@pytest.mark.parametrize("ta,tb", TRANS, ids=TRANS_IDS)
@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=["x".join(map(str, s)) for s in DENSE_SHAPES])
def test_gemm_dense_64_tiles(ops, dev, shape, ta, tb, bf):
    M, N, K = shape
    A, Bm, bias, c_old = gemm_inputs(M, N, K, 1000 * M + 10 * N + K)
    tag = f"gemm64 {shape} ta {int(ta)} tb {int(tb)} {MATH_IDS[bf]}"
    la, lb = (M if ta else K), (K if tb else N)                   # natural leading dimensions

    failed = []

    def check(what, act=0, with_bias=False, acc=False, **ld):
        b, c = (bias if with_bias else None), (c_old if acc else None)
        out = gemm_call(ops, dev, A, Bm, ta, tb, bf, bias=b, act=act, c_old=c, **ld)
        try:
            close(f"{tag} {what}", out, gemm_ref(A, Bm, b, c, act, torch.float64, bf), gemm_ref(A, Bm, b, c, act, torch.float32, bf), PROD)
        except AssertionError as e:                         # every variant of a case is measured before the case fails
            failed.append(str(e))

    check("plain")
    if shape in LD_SHAPES:
        check("wide ld", lda=wide(la), ldb=wide(lb), ldc=wide(N))
        check("odd ld", lda=odd(la), ldb=odd(lb), ldc=odd(N))
        check("odd lda only", lda=odd(la))
        check("odd ldb only", ldb=odd(lb))
    if shape in EPI_SHAPES:
        for act in ACTS:
            check(f"bias act {act}", act=act, with_bias=True)
            check(f"bias act {act} accumulate ldc > N", act=act, with_bias=True, acc=True, ldc=N + 3)
        check("accumulate alone", acc=True)
    assert not failed, failed


def test_gemm_rejects_unknown_activation_and_narrow_ldc(ops, dev):
    """act 2 (the align clamp) is not offered by tag_gemm; ldc < N is refused before a launch"""
    x = torch.zeros(4, 4, device=dev)
    for act, ldc in ((2, 4), (0, 3)):
        with pytest.raises(RuntimeError, match="argument check failed"):
            ops.call("tag_gemm", ops.ptr(x), 4, 0, ops.ptr(x), 4, 0, ops.ptr(x), ldc, 4, 4, 4, None, act, 0, None)


# ------------------------------------------------------------------------------------------------ 2. split-K
# (M, N, K, splits): a workspace is handed to the C ABI directly, so every transposition is sliced (dispatch.gemm offers one to
# transA products only).  kchunk = ceil(K / splits) rounded up to 32; slice s covers [s kchunk, min((s + 1) kchunk, K)):
#   (64, 64, 1024, 4)        kchunk 256: four whole slices of one whole tile -> FAST
#   (100, 33, 1030, 4)       kchunk 288: the last slice is 166 long (5 chunks and a K tail of 6), ragged tiles
#   (70, 65, 2049, 8)        kchunk 288: the last slice is 33 long (one chunk and one element)
#   (128, 64, 4100, 16)      kchunk 288: slice 14 is 68 long, slice 15 starts at 4320 > K: EMPTY (negative kiters)
#   (64, 64, 8200, 32)       kchunk 288: slice 28 is 136 long, slices 29 .. 31 are EMPTY; whole tiles, yet not FAST
#   (1000, 1030, 1024, 3)    272 tiles (below the 384 at which slicing stops); M N = 1,030,000 > 2048 x 256: the second
#                            grid-stride trip of splitk_reduce_kernel
SPLIT_SHAPES = [(64, 64, 1024, 4), (100, 33, 1030, 4), (70, 65, 2049, 8), (128, 64, 4100, 16), (64, 64, 8200, 32),
                (1000, 1030, 1024, 3)]


@functools.lru_cache(maxsize=2)
def split_case(M, N, K):
    A, Bm, bias, c_old = gemm_inputs(M, N, K, 7 * M + 3 * N + K)
    refs = {(bf, epi): tuple(gemm_ref(A, Bm, bias if epi else None, c_old if epi else None, 3 if epi else 0, dt, bf)
                             for dt in (torch.float64, torch.float32)) for bf in (False, True) for epi in (False, True)}
    return A, Bm, bias, c_old, refs


@pytest.mark.parametrize("bf", [False, True], ids=MATH_IDS)
@pytest.mark.parametrize("ta,tb", TRANS, ids=TRANS_IDS)
@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=["x".join(map(str, s[:3])) + f"-s{s[3]}" for s in SPLIT_SHAPES])
def test_gemm_split_k(ops, dev, shape, ta, tb, bf):
    """Raw K-slice partials + splitk_reduce_kernel, plain and with the whole epilogue (bias, gelu, accumulate, ldc > N) in the
    reduce kernel; the slices are summed in a fixed order, so a second run is bit-equal."""
    M, N, K, splits = shape
    nbytes = ops.query("tag_gemm_ws_bytes", M, N, K)
    assert nbytes == splits * M * N * 4, f"the table claims {splits} K slices for {shape[:3]}, the library says {nbytes / (M * N * 4)}"
    A, Bm, bias, c_old, refs = split_case(M, N, K)
    tag = f"splitk {shape[:3]} s{splits} ta {int(ta)} tb {int(tb)} {MATH_IDS[bf]}"
    for epi in (False, True):
        kw = dict(bias=bias, act=3, c_old=c_old, ldc=N + 5) if epi else {}
        runs = []
        for _ in range(2):
            ws = torch.full((splits * M * N,), float("nan"), device=dev)
            runs.append(gemm_call(ops, dev, A, Bm, ta, tb, bf, ws=ws, **kw))
        assert torch.equal(runs[0], runs[1]), f"{tag}: two runs differ"
        close(f"{tag} {'bias gelu accumulate ldc > N' if epi else 'plain'}", runs[0], *refs[(bf, epi)], PROD)


# ------------------------------------------------------------------------------------------------ 3. dense GEMM, 128-tiles
# (M, N, K), at the product's own threshold (gemm_big_min = 2048 128-tiles; no option and no environment is touched):
#   (8197, 4099, 70)    65 x 33 = 2145 ragged tiles, three chunks with a K tail of 6 -> the tail-aware loader at T = 128
#   (8192, 4096, 96)    64 x 32 = exactly 2048 whole tiles -> FAST; three chunks: the odd-kiters tail `step` of the two-stage loop
#   (8192, 4096, 64)    the same tiles, two chunks: the unrolled pair alone
# Each output is 134 MB: the reference lives on the device, one per (shape, arithmetic), shared by the four transpositions.
BIG_SHAPES = [(8197, 4099, 70), (8192, 4096, 96), (8192, 4096, 64)]
_BIG_OUT = {}          # (shape, ta, tb, bf) -> the ragged shape's non-transposed-A products, for the batch-invariance check


def big_inputs(shape):
    M, N, K = shape
    return gemm_inputs(M, N, K, M + N + K)[:2]


@functools.lru_cache(maxsize=1)
def big_case(shape, bf, dev):
    A, Bm = big_inputs(shape)
    ref64 = gemm_ref(A, Bm, None, None, 0, torch.float64, bf)
    floor = relerr(gemm_ref(A, Bm, None, None, 0, torch.float32, bf), ref64)
    return A, Bm, ref64.to(dev), floor


def big_product(ops, dev, shape, ta, tb, bf):
    key = (shape, ta, tb, bf)
    if key in _BIG_OUT:
        return _BIG_OUT[key]
    A, Bm = big_inputs(shape)
    out = gemm_call(ops, dev, A, Bm, ta, tb, bf, ldc=shape[1] + (1 if shape[1] % 128 else 0))
    if shape == BIG_SHAPES[0] and not ta:
        _BIG_OUT[key] = out
    return out


@pytest.mark.parametrize("ta,tb", TRANS, ids=TRANS_IDS)
@pytest.mark.parametrize("bf", [False, True], ids=MATH_IDS)
@pytest.mark.parametrize("shape", BIG_SHAPES, ids=["x".join(map(str, s)) for s in BIG_SHAPES])
def test_gemm_dense_128_tiles(ops, dev, shape, bf, ta, tb):
    """Against fp64; the whole shapes also against the same operands 4 bytes off a 16-byte boundary, which take the tail-aware
    loader: identical K order, identical products -> bit-identical."""
    assert ((shape[0] + 127) // 128) * ((shape[1] + 127) // 128) >= 2048 and ops.query("tag_gemm_ws_bytes", *shape) == 0
    A, Bm, ref64, floor = big_case(shape, bf, dev)
    out = big_product(ops, dev, shape, ta, tb, bf)
    close(f"gemm128 {shape} ta {int(ta)} tb {int(tb)} {MATH_IDS[bf]}", out, ref64, floor, PROD)
    if shape[0] % 128 == 0:
        slow = gemm_call(ops, dev, A, Bm, ta, tb, bf, off4=True)
        assert torch.equal(out, slow), "FAST and tail-aware loaders differ"
    else:
        # the natural leading dimensions of this shape (70, 4099, 8197) leave no row 16-byte aligned: once more with aligned rows,
        # where the tail-aware loader takes whole float4s inside a tile and single elements at its edges -- the same arithmetic
        M, N, K = shape
        al = gemm_call(ops, dev, A, Bm, ta, tb, bf, lda=wide(M if ta else K), ldb=wide(K if tb else N), ldc=wide(N))
        assert torch.equal(out, al), "aligned and unaligned tail-aware loads differ"


@pytest.mark.parametrize("tb", [False, True], ids=["tb0", "tb1"])
@pytest.mark.parametrize("bf", [False, True], ids=MATH_IDS)
def test_gemm_rows_do_not_depend_on_the_batch(ops, dev, bf, tb):
    """dispatch.gemm's promise at kernel level: with A stored (M, K) and no workspace an output row is one fixed-order sum
    over k whatever M is -- rows 0 .. 69 of the (8197, 4099, 70) product (128-tiles) are bit-equal to the (70, 4099, 70)
    product of the same rows (2 x 65 64-tiles)."""
    shape = BIG_SHAPES[0]
    A, Bm = big_inputs(shape)
    many = big_product(ops, dev, shape, False, tb, bf)
    few = gemm_call(ops, dev, A[:70].contiguous(), Bm, False, tb, bf)
    assert torch.equal(many[:70], few)


# ------------------------------------------------------------------------------------------------ 4. align
# (B, T, N, D): the GEMM is (B T, B N, D) with A and B both k-contiguous and the sigmoid -> clamp -> (B, B, T, N) scatter epilogue
#   (1, 1, 1, 1)         one element
#   (2, 70, 3, 33)       B T = 140: three m-tiles, the clip boundary (row 70) inside the second; D tail
#   (5, 13, 17, 100)     B N = 85: two n-tiles, clip boundaries inside both and inside the one m-tile
#   (9, 250, 8, 512)     36 x 2 tiles, whole K chunks, ragged tiles, the runner's T and D
#   (64, 250, 33, 40)    (16000, 2112): 125 x 17 = 2125 128-tiles -- the scatter epilogue at T = 128 (the token head's shape)
ALIGN_SHAPES = [(1, 1, 1, 1), (2, 70, 3, 33), (5, 13, 17, 100), (9, 250, 8, 512)]
ALIGN_BIG = (64, 250, 33, 40)
ALIGN_MODES = [(False, False), (False, True), (True, False), (True, True)]            # (l2norm, scaled)
ALIGN_IDS = [f"l2{int(n)}-scaled{int(s)}" for n, s in ALIGN_MODES]


def align_inputs(B, T, N, D, l2norm, scaled, seed):
    """Logits of about N(0, 1/4) in every mode without l2norm (audio 0.5 randn; both operands times D^-1/4 where nothing
    divides by sqrt(D)), so every probability is far from the clamp and from saturation
    (within [0.005, 0.995], asserted on the reference).  At D = 1 F.normalize divides by |x|:
    magnitudes are drawn from [0.5, 1.5] there, so that the identically vanishing gradient is compared at inputs of order one."""
    g = torch.Generator().manual_seed(seed)
    audio, text = 0.5 * torch.randn(B, T, D, generator=g), torch.randn(B, N, D, generator=g)
    if D == 1:
        audio, text = (torch.sign(v) * (0.5 + torch.rand(v.shape, generator=g)) for v in (audio, text))
    if not l2norm and not scaled:
        audio, text = audio * D ** -0.25, text * D ** -0.25
    return audio, text, torch.randn(B, B, T, N, generator=g)


def align_ref(audio, text, dout, l2norm, scaled, dtype, backward=True):
    a, t = leaf(audio, dtype), leaf(text, dtype)
    out = O.align_dot_product(a, t, l2norm, scaled)
    if not backward:
        return out.detach().contiguous(), None, None
    out.backward(dout.to(dtype))
    return out.detach().contiguous(), a.grad, t.grad


@pytest.mark.parametrize("l2norm,scaled", ALIGN_MODES, ids=ALIGN_IDS)
@pytest.mark.parametrize("shape", ALIGN_SHAPES, ids=["x".join(map(str, s)) for s in ALIGN_SHAPES])
def test_align_sweep(ops, dev, shape, l2norm, scaled):
    B, T, N, D = shape
    audio, text, dout = align_inputs(B, T, N, D, l2norm, scaled, 31 * T + D)
    ref, r32 = (align_ref(audio, text, dout, l2norm, scaled, dt) for dt in (torch.float64, torch.float32))
    assert 0.005 <= ref[0].min().item() and ref[0].max().item() <= 0.995, "input precondition (not the kernel)"
    a, t = audio.to(dev), text.to(dev)
    out = ops.align_dot(a, t, l2norm, scaled)
    da, dt = ops.align_dot_backward(a, t, out, dout.to(dev), l2norm, scaled)
    tag = f"align {shape} l2norm {int(l2norm)} scaled {int(scaled)}"
    close(tag + " out", out, ref[0], r32[0], FWD)
    close(tag + " daudio", da, ref[1], r32[1], GRAD)
    close(tag + " dtext", dt, ref[2], r32[2], GRAD)


@pytest.mark.parametrize("l2norm,scaled", ALIGN_MODES, ids=ALIGN_IDS)
def test_align_128_tile_scatter(ops, dev, l2norm, scaled):
    """The token head's shape: the forward in all four modes, the backward in one (l2norm, scaled: both l2norm row kernels, the
    non-transposed (16000, 40, 2112) product and the 24-slice split-K (2112, 40, 16000) product)."""
    B, T, N, D = ALIGN_BIG
    assert ((B * T + 127) // 128) * ((B * N + 127) // 128) >= 2048
    back = l2norm and scaled
    audio, text, dout = align_inputs(B, T, N, D, l2norm, scaled, 77)
    ref, r32 = (align_ref(audio, text, dout, l2norm, scaled, dt, back) for dt in (torch.float64, torch.float32))
    assert 0.005 <= ref[0].min().item() and ref[0].max().item() <= 0.995, "input precondition (not the kernel)"
    a, t = audio.to(dev), text.to(dev)
    out = ops.align_dot(a, t, l2norm, scaled)
    tag = f"align {ALIGN_BIG} l2norm {int(l2norm)} scaled {int(scaled)}"
    close(tag + " out", out, ref[0].to(dev), relerr(r32[0], ref[0]), FWD)
    if back:
        da, dt = ops.align_dot_backward(a, t, out, dout.to(dev), l2norm, scaled)
        close(tag + " daudio", da, ref[1], r32[1], GRAD)
        close(tag + " dtext", dt, ref[2], r32[2], GRAD)


def test_align_clamp_floor_and_gate(ops, dev):
    """(2, 70, 3, 33), scaled: coordinate 0 of every audio frame is 1 and text rows (0, 1) / (1, 2) are -30 sqrt(D) / +30 sqrt(D)
    times e_0, so their logits are -30 / +30 against every frame: sigmoid(-30) = 9.4e-14 is clamped to float32(1e-7) and the
    `p > 1e-7` gate of align_dscore_kernel passes no gradient; sigmoid(+30) rounds to 1.0f, where p (1 - p) is 0.  d score is
    exactly zero in both columns, so dtext of both rows is exactly zero."""
    B, T, N, D = 2, 70, 3, 33
    audio, text, dout = align_inputs(B, T, N, D, False, True, 5)
    audio[..., 0] = 1.0
    text[..., 0] *= 0.5
    text[0, 1], text[1, 2] = 0.0, 0.0
    text[0, 1, 0], text[1, 2, 0] = -30.0 * math.sqrt(D), 30.0 * math.sqrt(D)
    prob = torch.sigmoid(audio.double().reshape(-1, D) @ text.double().reshape(-1, D).t() / math.sqrt(D))      # (B T, B N), unclamped
    low, high = torch.zeros(B * N, dtype=torch.bool), torch.zeros(B * N, dtype=torch.bool)
    low[0 * N + 1], high[1 * N + 2] = True, True
    assert not ((prob >= 0.5e-7) & (prob <= 2e-7)).any(), "input precondition: no probability beside the clamp threshold"
    assert (prob[:, low] < 0.5e-7).all() and (prob[:, high] > 1 - 1e-9).all() and (prob[:, ~(low | high)] > 0.02).all()
    ref, r32 = (align_ref(audio, text, dout, False, True, dt) for dt in (torch.float64, torch.float32))
    a, t = audio.to(dev), text.to(dev)
    out = ops.align_dot(a, t, False, True)
    o = out.cpu()                                                       # (B, B2, T, N)
    assert torch.equal(o[:, 0, :, 1], torch.full((B, T), 1e-7)) and torch.equal(o[:, 1, :, 2], torch.ones(B, T))
    ds = torch.full((B * T, B * N), float("nan"), device=dev)
    ops.call("tag_align_dot_dscore", ops.ptr(out), ops.ptr(dout.to(dev)), ops.ptr(ds), 1, B, T, N, D)
    ds = ds.cpu()
    assert (ds[:, low | high] == 0).all() and (ds[:, ~(low | high)] != 0).all()
    da, dt = ops.align_dot_backward(a, t, out, dout.to(dev), False, True)
    assert (dt.cpu().reshape(B * N, D)[low | high] == 0).all()
    close("align clamp out", out, ref[0], r32[0], FWD)
    close("align clamp daudio", da, ref[1], r32[1], GRAD)
    close("align clamp dtext", dt, ref[2], r32[2], GRAD)


@pytest.mark.parametrize("scaled", [False, True])
def test_align_forward_normalising_into_its_workspace(ops, dev, scaled):
    """tag_align_dot_forward's own l2norm = 1 path (both operands normalised into ws) is the same arithmetic as the two row
    kernel launches followed by l2norm = 0, which is what dispatch.align_dot does."""
    B, T, N, D = 5, 13, 17, 100
    audio, text, _ = align_inputs(B, T, N, D, True, scaled, 9)
    a, t = audio.to(dev), text.to(dev)
    ws = torch.full((B * T * D + B * N * D,), float("nan"), device=dev)
    out = torch.full((B, B, T, N), float("nan"), device=dev)
    ops.call("tag_align_dot_forward", ops.ptr(a), ops.ptr(t), ops.ptr(out), 1, int(scaled), B, T, N, D, ops.ptr(ws))
    assert torch.equal(out, ops.align_dot(a, t, True, scaled))
    with pytest.raises(RuntimeError, match="argument check failed"):      # l2norm without a workspace is refused
        ops.call("tag_align_dot_forward", ops.ptr(a), ops.ptr(t), ops.ptr(out), 1, int(scaled), B, T, N, D, None)


# ------------------------------------------------------------------------------------------------ 5. the small kernels
# tag_colsum: colsum_partial_kernel runs nblk = min(256, ceil(M / 64)) row blocks of 4 rows per trip, colsum_final_kernel folds
# them 16 at a time:  M = 1 -> nblk 1 (a single row: three of the four row lanes idle), 63 / 64 -> 1, 65 -> 2, 1024 -> 16 (each
# of the 16 fold groups holds one), 1025 -> 17 (group 0 holds two), 40000 -> the 256-block cap, 40 row trips per lane.
# N = 1, 15, 16, 17 (the 16-column blocks of the final kernel: below / at / above one), 63, 64, 65 (the 64-column stripes of the
# partial kernel), 100.
COLSUM_M = [1, 63, 64, 65, 1024, 1025, 40000]
COLSUM_N = [1, 15, 16, 17, 63, 64, 65, 100]


@pytest.mark.parametrize("M", COLSUM_M)
def test_colsum_sweep(ops, dev, M):
    assert ops.query("tag_colsum_ws_bytes", M, 1) == min(256, (M + 63) // 64) * 8
    for N in COLSUM_N:
        for ld in (N, N + 3):
            x = torch.randn(M, N, generator=torch.Generator().manual_seed(M + N)) + 0.5           # column means of 0.5
            out = torch.full((N + 1,), SENT, device=dev)
            ops.colsum(staged(x, ld, dev), M, N, ld=ld, out=out)
            assert out[N].item() == SENT
            close(f"colsum M {M} N {N} ld {ld}", out[:N], x.double().sum(0), x.sum(0), COLSUM)


@pytest.mark.parametrize("n", [1, 255, 256 * 4096 + 777])
def test_relu_backward_in_place(ops, dev, n):
    """dx = dy where y > 0 else 0, written over dy (as ops.relu_backward calls it), exact; y holds exact 0.0 and -0.0 (no
    gradient at either).  n = 256 * 4096 + 777: the grid is capped at 4096 blocks, 777 threads take a second trip."""
    g = torch.Generator().manual_seed(n % 1000)
    y, dy = torch.randn(n, generator=g), torch.randn(n, generator=g)
    y[0::5], y[1::7] = 0.0, -0.0
    if n == 1:
        y[0] = 0.7
    want = torch.where(y > 0, dy, torch.zeros(()))
    dyd = dy.to(dev)
    got = ops.relu_backward(y.to(dev), dyd)
    assert got.data_ptr() == dyd.data_ptr() and torch.equal(got.cpu(), want)
    if n > 1:
        assert (want[0::5] == 0).all() and (want != 0).sum() > n // 4


# l2norm rows: one wave per row, 4 rows per block, lanes stride D by 64
#   rows 1 (three waves return at once), 3, 4 (one block), 5 (a second block of one row), 130 (33 blocks, the last with two)
#   D 1, 63, 64 (one trip), 65 (a second trip of one lane), 300, 1024, 1500 (24 trips, a tail of 28)
L2_ROWS = [1, 3, 4, 5, 130]
L2_D = [1, 63, 64, 65, 300, 1024, 1500]


def l2norm_ref(x, du, dtype):
    xs = leaf(x, dtype)
    y = F.normalize(xs, dim=-1)
    y.backward(du.to(dtype))
    return y.detach(), xs.grad


@pytest.mark.parametrize("D", L2_D)
def test_l2norm_rows_sweep(ops, dev, D):
    """Forward and backward of F.normalize.  Row 1 (where there is one) is all zero: the 1e-12 clamp gives y = 0 and dx = du *
    1e12, as fp64 autograd does; that row is compared on its own, or its 1e12 would be the scale of the whole tensor."""
    for rows in L2_ROWS:
        g = torch.Generator().manual_seed(100 * rows + D)
        x, du = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
        if D == 1:
            x = torch.sign(x) * (0.5 + torch.rand(rows, D, generator=g))      # |x| of order one: see align_inputs
        live = torch.ones(rows, dtype=torch.bool)
        if rows > 1:
            x[1], live[1] = 0.0, False
        ref, r32 = l2norm_ref(x, du, torch.float64), l2norm_ref(x, du, torch.float32)
        xd, dud = x.to(dev), du.to(dev)
        y, dx = torch.full((rows + 1, D), SENT, device=dev), torch.full((rows + 1, D), SENT, device=dev)
        ops.call("tag_l2norm_rows_forward", ops.ptr(xd), ops.ptr(y), rows, D)
        ops.call("tag_l2norm_rows_backward", ops.ptr(xd), ops.ptr(dud), ops.ptr(dx), rows, D)
        assert bool((y[rows] == SENT).all()) and bool((dx[rows] == SENT).all())
        y, dx = y[:rows].cpu(), dx[:rows].cpu()
        tag = f"l2norm rows {rows} D {D}"
        close(tag + " y", y[live], ref[0][live], r32[0][live], FWD)
        close(tag + " dx", dx[live], ref[1][live], r32[1][live], GRAD)
        if rows > 1:
            assert (y[1] == 0).all() and (ref[0][1] == 0).all()
            close(tag + " dx of the zero row", dx[1], ref[1][1], r32[1][1], GRAD)
            assert relerr(ref[1][1], du[1].double() * 1e12) < 1e-12          # what the reference itself gives there
