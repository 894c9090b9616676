"""bf16x6 matrix mode (include/gcdm_matrix_mode.h) through the C ABI on an MI355X: gcdm_op_gemm at every tile edge and stride pattern, split K,
exact cases, magnitudes, invariances and non-finite operands, then gcdm_mp_fwd / gcdm_mp_bwd and gcdm_gcp2_fwd / gcdm_gcp2_bwd against the fp64
references of tests/mp_train_ref.py and tests/gcp2_ref.py, through the harnesses of the fp32-mode C-ABI tests.

GEMM harness: every operand sits between NaN-filled guard regions with NaN in every stride gap, optionally one float off its allocation's
base, so an element outside [0, M) x [0, K) x [0, N) that is dereferenced and used poisons the result; the output is NaN inside and has
sentinel guard words around it.

The bar is the project's own, per tensor and per row:  max|got - ref64| <= M * max|ref32 - ref64| + 8 * 2^-24 * max|ref64|,  ref32 being the
CPU fp32 product on ONE thread.  M = 4 for every tensor of this file: the GEMM, the 36 tensors of the message layer (the fp32-mode table of
exceptions, mp_train_ref.MARGINS with its M = 16 for dh and the bias gradients, is emptied for these cases: no tensor was measured to need
it in this mode) and the GCP2's (whose table is empty in fp32 mode too).

What constrains the split in the plain GEMM cases is not the M term: every one of them lands under the 8 * 2^-24 max|ref64| floor, so
"factor 0" below means "under the floor", not headroom under M = 4.  The sharp checks of gcdm_op_gemm are the bit-exact ones (integers; the
three-image case, which fails if an image is dropped, misplaced in k or mis-scaled) and the magnitude case that gives every row its own floor.

Worst factors measured in bf16x6 mode on an MI355X (the tests print them, "MEASURED ...", with the raw errors in units of 2^-24 max|ref64|):

    case                                                     worst factor needed   tensor
    gemm, every shape x stride pattern x bias x offset        0                     (every error under the 8 * 2^-24 floor)
    split K (each slice, and the reduced result)              0
    operands scaled 2^-100 ... 2^100 (per call, per row)      0
    clean rows / columns beside non-finite ones               0
    message layer [3], [8, 1], [1, 2, 7, 13, 9, 3], QM9       0 / 0 / 0
    message layer [3], [8, 1], [1, 2, 7, 13, 9, 3], GEOM      0 / 0.49 / 0          scalar_message_attention.0.bias (one number)
    message layer star_in, QM9 / GEOM                         1.56 / 0              scalar_message_attention.0.bias
    GCP2 pos and ff, M = 1, 65, 131, QM9 and GEOM             0

No tensor needs more than 4, so none has an M of its own; fp32 mode itself needs up to 4.3 / 2.4 (dh) on [1, 2, 7, 13, 9, 3]
(tests/test_mp_train_cabi_gpu.py).
"""
import ctypes as C
import importlib
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gcp2_ref as G2  # noqa: E402
import mp_train_ref as R  # noqa: E402
import test_gcp2_fused_cabi_gpu as gcp2_cabi  # noqa: E402
import test_mp_train_cabi_gpu as mp_cabi  # noqa: E402

pkg = importlib.import_module("bio-diffusion_amd")
ops = pkg.ops
pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
GUARD = 64
M_BAR = 4
NAN = float("nan")
PATTERNS = {"Ak_Bn": (True, True), "Ak_Bk": (True, False), "Am_Bn": (False, True), "Am_Bk": (False, False)}


@pytest.fixture(autouse=True)
def bf16x6():
    """Every test of this file runs in bf16x6 mode and leaves the process in fp32 mode, whatever happens inside."""
    ops.set_matrix_mode("bf16x6")
    try:
        yield
    finally:
        ops.set_matrix_mode("f32")
        assert ops.get_matrix_mode() == "f32"


def _lib():
    return pkg._native.load_ops()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class _In:
    """mat [r, c] stored row-major with leading dimension c + pad, NaN in the pad columns, GUARD NaN words before and after, the first element
    `off` floats past a 256-byte aligned address."""

    def __init__(self, mat, pad, off):
        r, c = mat.shape
        self.ld = c + pad
        buf = torch.full((GUARD + off + r * self.ld + GUARD,), NAN, dtype=torch.float32)
        buf[GUARD + off:GUARD + off + r * self.ld].view(r, self.ld)[:, :c] = mat.to(torch.float32)
        self.buf = buf.to(DEV)
        self.p = C.c_void_p(self.buf.data_ptr() + 4 * (GUARD + off))


class _Out:
    SENTINEL = 12345.5

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), self.SENTINEL, dtype=torch.float32, device=DEV)
        self.buf[GUARD:GUARD + n] = NAN
        self.p = C.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def get(self):
        h = self.buf.cpu()
        assert bool((h[:GUARD] == self.SENTINEL).all()) and bool((h[GUARD + self.n:] == self.SENTINEL).all()), "write outside the output"
        return h[GUARD:GUARD + self.n]


def run_gemm(A, B, bias=None, pattern="Ak_Bn", pad=3, off=0, slices=1, parts=False):
    """C = A B (+ bias) through gcdm_op_gemm (and gcdm_op_reduce_slices when slices > 1) in the current mode -> C [M, N] fp32 on the host
    (with parts: also the slices [slices, M, N])."""
    M, K = A.shape
    N = B.shape[1]
    a_kfast, b_nfast = PATTERNS[pattern]
    Ad = _In(A if a_kfast else A.t(), pad, off)
    Bd = _In(B if b_nfast else B.t(), pad, off)
    sam, sak = (Ad.ld, 1) if a_kfast else (1, Ad.ld)
    sbk, sbn = (Bd.ld, 1) if b_nfast else (1, Bd.ld)
    bd = None if bias is None else bias.to(torch.float32).to(DEV)
    part = _Out(slices * M * N)
    lib = _lib()
    assert lib.gcdm_op_gemm(Ad.p, sam, sak, Bd.p, sbk, sbn, part.p, None if bd is None else C.c_void_p(bd.data_ptr()), M, N, K, slices, _stream()) == 0
    if slices == 1:
        out = part.get().view(M, N)
        return (out, out.view(1, M, N)) if parts else out
    out = _Out(M * N)
    assert lib.gcdm_op_reduce_slices(part.p, out.p, M * N, slices, _stream()) == 0
    res = out.get().view(M, N)
    return (res, part.get().view(slices, M, N)) if parts else res


def refs(A, B, bias=None):
    """(ref64, ref32) of A B + bias for fp32-valued operands: fp64, and torch's fp32 product on the CPU on one thread."""
    A32, B32 = A.to(torch.float32), B.to(torch.float32)
    r64 = A32.double() @ B32.double()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        r32 = A32 @ B32
        if bias is not None:
            r32 = r32 + bias.to(torch.float32)
    finally:
        torch.set_num_threads(threads)
    if bias is not None:
        r64 = r64 + bias.to(torch.float32).double()
    return r64, r32.double()


def needed(got, r64, r32, rows=None):
    """The factor M the bar would need: (for the whole tensor, for its worst row).  A NaN or Inf in got needs inf."""
    got = got.double()
    if rows is not None:
        got, r64, r32 = got[rows], r64[rows], r32[rows]
    if not r64.numel():
        return 0.0, 0.0
    err = (got - r64).abs().nan_to_num(nan=math.inf)
    gap = (r32 - r64).abs()
    floor = 8 * U * float(r64.abs().max())

    def need(e, g):
        over = (e - floor).clamp(min=0)
        return float(torch.where(over > 0, over / g, torch.zeros_like(over)).max())

    return need(err.max(), gap.max()), need(err.max(dim=1).values, gap.max(dim=1).values)


def hold(got, r64, r32, what, rows=None, margin=M_BAR):
    n = needed(got, r64, r32, rows)
    g_, a_, b_ = (t if rows is None else t[rows] for t in (got.double(), r64, r32))
    scale = U * float(a_.abs().max()) if a_.numel() and float(a_.abs().max()) > 0 else 1.0
    print(f"MEASURED {what}: factor needed tensor {n[0]:.3g} / worst row {n[1]:.3g}; max|got - ref64| = {float((g_ - a_).abs().max()) / scale:.2f}, "
          f"max|ref32 - ref64| = {float((b_ - a_).abs().max()) / scale:.2f} (in 2^-24 max|ref64|; the floor is 8)")
    assert n[0] <= margin and n[1] <= margin, f"{what}: needs M = {n[0]:.3g} (tensor) / {n[1]:.3g} (worst row) > {margin}"
    return max(n)


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------------
MS, NS, KS = (1, 63, 64, 65, 131), (1, 31, 33, 64, 65), (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 273)


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_gemm_at_every_tile_edge_against_fp64(pattern):
    """Every M, N and K of the lists appears under every stride pattern; bias on / off, base pointers on / one float off a 256-byte boundary and
    leading dimensions 0 / 3 floats wider than the row alternate (K = 273 with pad 0 is the training step's odd row stride)."""
    g = _gen(40 + list(PATTERNS).index(pattern))
    worst = 0.0
    for ik, K in enumerate(KS):
        for im, M in enumerate(MS):
            N = NS[(im + ik + list(PATTERNS).index(pattern)) % len(NS)]
            A, B = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)
            bias = torch.randn(N, generator=g) if (im + ik) % 2 else None
            off, pad = (im + ik // 2) % 2, 3 * ((im + ik // 3) % 2)
            got = run_gemm(A, B, bias, pattern, pad, off)
            r64, r32 = refs(A, B, bias)
            worst = max(worst, hold(got, r64, r32, f"gemm {pattern} M={M} N={N} K={K} bias={bias is not None} off={off} pad={pad}"))
    print(f"MEASURED gemm {pattern}: worst factor over the shapes {worst:.3g}")


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("K,slices", [(40, 3), (20, 4)])
def test_split_k_and_empty_trailing_slices(pattern, K, slices):
    """Slices of 16: K = 40 in 3 is 16 + 16 + 8; K = 20 in 4 is 16 + 4 and two empty slices, which must write zeros (and touch no memory: the
    operands end in NaN guards).  The bias goes into slice 0 only; the reduced result is held to the bar."""
    g = _gen(60 + K)
    M, N = 65, 33
    A, B, bias = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g), torch.randn(N, generator=g).abs() + 1
    got, part = run_gemm(A, B, bias, pattern, 3, 1, slices, parts=True)
    for z in range(slices):
        lo, hi = 16 * z, min(16 * z + 16, K)
        if lo >= K:
            assert not bool(part[z].any()), f"empty slice {z} is not zero"
        else:
            hold(part[z], *refs(A[:, lo:hi], B[lo:hi], bias if z == 0 else None), f"split-K {pattern} K={K} slice {z}")
    hold(got, *refs(A, B, bias), f"split-K {pattern} K={K} in {slices} reduced")


# ---- exact cases -----------------------------------------------------------------------------------------------------------------------------
def _bit_equal(got, want64, what):
    want = want64.to(torch.float32)
    assert torch.equal(want.double(), want64), f"{what}: the expected result is not an fp32 number"
    bad = got.view(torch.int32) != want.view(torch.int32)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} entries differ, first at {bad.nonzero()[0].tolist()}: {got[bad][0].item()!r} vs {want[bad][0].item()!r}"


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_small_integers_are_exact(pattern):
    g = _gen(70)
    for M, N in ((131, 65), (1, 1), (64, 33)):
        A = torch.randint(-8, 9, (M, 273), generator=g).double()
        B = torch.randint(-8, 9, (273, N), generator=g).double()
        bias = torch.randint(-8, 9, (N,), generator=g).double()
        _bit_equal(run_gemm(A, B, bias, pattern, 0, 1), A @ B + bias, f"integers {pattern} M={M} N={N}")


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("swap", [False, True], ids=["three_images_in_A", "three_images_in_B"])
def test_all_three_images_arrive_at_their_scale(pattern, swap):
    """X = +-(1 + 2^-9 + 2^-17) 2^e has the images 2^e, 2^(e-9), 2^(e-17); Y holds one power of two per column.  Every product is exact, the
    sums (|sum of signs| <= 62 at K = 31 with e and e + 1 mixed in a row: 6 bits on top of the 18 of the pattern) are exact in each accumulator
    and in their merge, so the result is the fp64 one bit for bit -- unless an image is dropped, lands in the wrong k, or is scaled wrongly."""
    g = _gen(80)
    M, N, K = 65, 33, 31
    e_row = torch.randint(-20, 21, (M, 1), generator=g)
    e = e_row + torch.randint(0, 2, (M, K), generator=g)
    sign = torch.randint(0, 2, (M, K), generator=g).double() * 2 - 1
    X = sign * (1 + 2.0 ** -9 + 2.0 ** -17) * torch.ldexp(torch.ones(M, K, dtype=torch.float64), e)
    Y = torch.ldexp(torch.ones(K, N, dtype=torch.float64), torch.randint(-20, 21, (1, N), generator=g).expand(K, N))
    assert torch.equal(X.float().double(), X)
    if swap:
        got = run_gemm(Y.t().contiguous(), X.t().contiguous(), None, pattern, 3, 1)
        _bit_equal(got, Y.t() @ X.t(), f"images in B {pattern}")
    else:
        _bit_equal(run_gemm(X, Y, None, pattern, 3, 1), X @ Y, f"images in A {pattern}")


# ---- magnitudes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2s", [-100, -50, 50, 100])
def test_operands_far_from_one(log2s):
    """A 2^s against B 2^-s: no prescale and no guard, so the result is the unscaled one within the bar, and finite."""
    g = _gen(90)
    A, B = torch.randn(65, 273, generator=g), torch.randn(273, 33, generator=g)
    s = 2.0 ** log2s
    for pattern in ("Ak_Bk", "Am_Bn"):
        got = run_gemm((A.double() * s), (B.double() / s), None, pattern, 0, 1)
        assert bool(torch.isfinite(got).all())
        hold(got, *refs(A, B), f"scales 2^{log2s} {pattern}")


def test_rows_of_every_magnitude_in_one_product():
    """Row m of A scaled by 2^-100 ... 2^100: each row is held to the bar with ITS OWN floor (8 U max|row of ref64|), and every output is finite."""
    g = _gen(91)
    M, K, N = 131, 273, 33
    A, B = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)
    ex = torch.linspace(-100, 100, M).round().to(torch.int32)
    As = torch.ldexp(A.double(), ex[:, None].expand(M, K))
    got = run_gemm(As, B, None, "Ak_Bk", 0, 1)
    assert bool(torch.isfinite(got).all())
    r64, r32 = refs(As, B)
    worst = 0.0
    for m in range(M):
        worst = max(worst, max(needed(got, r64, r32, slice(m, m + 1))))
    print(f"MEASURED rows scaled 2^-100 .. 2^100: worst factor of a row against its own floor {worst:.3g}")
    assert worst <= M_BAR


# ---- invariance ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_bits_repeat_and_do_not_depend_on_the_row_count(pattern):
    g = _gen(95)
    A, B, bias = torch.randn(131, 273, generator=g), torch.randn(273, 65, generator=g), torch.randn(65, generator=g)
    first = run_gemm(A, B, bias, pattern, 3, 1)
    again = run_gemm(A, B, bias, pattern, 3, 1)
    assert torch.equal(first.view(torch.int32), again.view(torch.int32)), "two runs differ"
    alone = run_gemm(A[70:71], B, bias, pattern, 3, 1)
    assert torch.equal(first[70:71].view(torch.int32), alone.view(torch.int32)), "row 70 of M = 131 differs from the M = 1 product of that row"


def test_fp32_mode_is_untouched_by_a_bf16x6_call():
    g = _gen(96)
    A, B = torch.randn(131, 273, generator=g), torch.randn(273, 65, generator=g)
    ops.set_matrix_mode("f32")
    before = run_gemm(A, B, None, "Ak_Bk", 0, 0)
    ops.set_matrix_mode("bf16x6")
    between = run_gemm(A, B, None, "Ak_Bk", 0, 0)
    ops.set_matrix_mode("f32")
    after = run_gemm(A, B, None, "Ak_Bk", 0, 0)
    assert torch.equal(before.view(torch.int32), after.view(torch.int32))
    assert not torch.equal(before.view(torch.int32), between.view(torch.int32)), "the two modes gave the same bits: the switch does nothing?"
    ops.set_matrix_mode("bf16x6")        # the fixture's finally restores f32


# ---- non-finite operands -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("side", ["A", "B"])
def test_non_finite_operands_poison_what_depends_on_them_and_nothing_else(pattern, side):
    """+Inf, NaN and 3.4e38 (>= 2^127: outside the mode's range) in three rows of A (columns of B): every output of those rows (columns) is
    non-finite, every other output meets the bar."""
    g = _gen(97)
    M, K, N = 131, 40, 65
    A, B = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)
    B[B == 0] = 1.0
    A[A == 0] = 1.0
    hit = [3, 70, 130] if side == "A" else [2, 33, 64]
    X = A if side == "A" else B.t()
    X[hit[0], 5], X[hit[1], 20], X[hit[2], 39] = float("inf"), NAN, 3.4e38
    got = run_gemm(A, B, None, pattern, 3, 1)
    clean = torch.ones(M if side == "A" else N, dtype=torch.bool)
    clean[hit] = False
    gv = got if side == "A" else got.t()
    assert not bool(torch.isfinite(gv[~clean]).any()), "a finite result depends on a non-finite or out-of-range operand"
    A0, B0 = A.clone(), B.clone()
    (A0 if side == "A" else B0.t())[hit] = 0
    r64, r32 = refs(A0, B0)
    if side == "A":
        hold(got[clean], r64[clean], r32[clean], f"clean rows {pattern}")
    else:
        hold(got[:, clean], r64[:, clean], r32[:, clean], f"clean columns {pattern}")


# ---- the fused entries -------------------------------------------------------------------------------------------------------------------------
def _mp_graph(name):
    return R.star_in() if name == "star_in" else R.fc_graph([int(n) for n in name.split("x")])


@pytest.mark.parametrize("case", mp_cabi.CASES)
@pytest.mark.parametrize("name", ["3", "8x1", "1x2x7x13x9x3", "star_in"])
def test_message_layer_forward_and_backward_against_fp64(case, name, monkeypatch):
    """gcdm_mp_fwd + gcdm_mp_bwd in bf16x6 mode through the harness of tests/test_mp_train_cabi_gpu.py, with that file's table of exceptions
    emptied: every one of the 36 tensors, dh and the bias gradients included, is held to M = 4, per tensor and per row."""
    assert ops.get_matrix_mode() == "bf16x6"
    monkeypatch.setattr(mp_cabi, "MARGINS", {})
    mp_cabi._check_case(case, _mp_graph(name))


@pytest.mark.parametrize("case", ["qm9", "geom"])
@pytest.mark.parametrize("inst", ["pos", "ff"])
def test_gcp2_forward_and_backward_against_fp64(case, inst):
    """gcdm_gcp2_fwd + gcdm_gcp2_bwd in bf16x6 mode (the gate contraction through Ps included: VO = 1 and VO = 32) through the harness and under
    the bar of tests/test_gcp2_fused_cabi_gpu.py."""
    assert ops.get_matrix_mode() == "bf16x6"
    d = G2.instances(case)[inst]
    W = G2.make_weights(d)
    for M in (1, 65, 131):
        gcp2_cabi._check(f"bf16x6 {case} {inst}", d, W, *G2.make_rows(d, M, seed=5 + M))
