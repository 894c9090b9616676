"""Each module-level operator of libgcdm_ops.so on its own, forward and backward, against a plain fp64 reference on the CPU.

The composed module path (tests/test_modules_gpu.py) runs these operators only at the model's widths; here every operator meets the
shapes, strides, slice counts, special values and degenerate graphs where kernels go wrong.  References: the oracle's function where it
has one (oracle/gcdm_oracle.py: localize, edge_features, orientations, centralize, safe_norm, _act, scalarize / vectorize in edge mode,
fully_connected_edges) on float64 inputs, otherwise the reference's formula restated with its file:line; backwards against torch.autograd
of that fp64 reference.  GEMM, colsum and reduce_slices are called through the C ABI (include/gcdm_ops.h) with explicit strides,
everything else through bio-diffusion_amd/ops.py.

Two kinds of data:
* small integers (entries in -3..3, frames with integer rows): every fp32 product and partial sum is exact in any order, atomics included,
  so the result must EQUAL the fp64 result bit for bit -- an index, stride, slice or bias error shows at any size;
* Gaussian data, against a bound derived from fp32 arithmetic, written next to each assert.
"""
import ctypes as C
import importlib
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import gcdm_oracle as O  # noqa: E402

pkg = importlib.import_module("bio-diffusion_amd")
ops = pkg.ops
pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24                     # unit roundoff of fp32
TINY = 2.0 ** -126                 # smallest normal fp32
GUARD = 64                         # guard words around every output the C ABI writes


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, g, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(torch.float64)


def _gauss(shape, g):
    return torch.randn(tuple(shape), generator=g, dtype=torch.float64)


def _ulp(y):
    """ulp of the fp32 number nearest to y (0 for y = 0)."""
    y = y.abs()
    _, e = torch.frexp(y)
    return torch.where(y == 0, torch.zeros_like(y), torch.ldexp(torch.ones_like(y), e - 24))


def _gamma(n):
    return n * U / (1 - n * U)


def _lib():
    return pkg._native.load_ops()


def _ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + 4 * offset)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _exact(got, want, what):
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} entries differ, first at {bad.nonzero()[0].tolist()}: {got[bad][0].item()} vs {want[bad][0].item()}"


def _within(got, want, bound, what):
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs()
    bad = ~(err <= bound)                                  # NaN in got fails too
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} entries outside the bound, worst ratio {(err / bound).nan_to_num(math.inf).max().item():.3g} "
                                 f"at {bad.nonzero()[0].tolist()}")


# ---- GEMM through the C ABI ------------------------------------------------------------------------------------------------------------------
class _Out:
    """An output of `n` floats inside a larger device buffer: NaN inside (an entry the kernel does not write shows), a finite sentinel in the
    GUARD words before and after (a stray write shows)."""
    SENTINEL = 12345.5

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), self.SENTINEL, dtype=torch.float32, device=DEV)
        self.buf[GUARD:GUARD + n] = float("nan")
        self.p = _ptr(self.buf, GUARD)

    def get(self):
        h = self.buf.cpu()
        assert bool((h[:GUARD] == self.SENTINEL).all()) and bool((h[GUARD + self.n:] == self.SENTINEL).all()), "write outside the output"
        return h[GUARD:GUARD + self.n]


def _embed(mat, ld):
    """mat [r, c] (c <= ld) as the leading columns of an [r, ld] row-major device matrix whose other columns are NaN, followed by a NaN tail
    (never empty, so the pointer is not null): a read of an unused column or past the matrix poisons the result."""
    r, c = mat.shape
    buf = torch.full((r * ld + GUARD,), float("nan"), dtype=torch.float32)
    buf[:r * ld].view(r, ld)[:, :c] = mat.to(torch.float32)
    return buf.to(DEV)


def _gemm_operands(A, B, pattern, pad):
    """The four stride patterns of k_gemm: A k-fast (A[m][k]) or m-fast (stored as A^T), B n-fast (B[k][n]) or k-fast (stored as B^T); every
    stored matrix has `pad` NaN columns beyond its width (sam > K etc.)."""
    M, K = A.shape
    N = B.shape[1]
    a_kfast, b_nfast = pattern in (0, 1), pattern in (0, 2)
    if a_kfast:
        Ad, sam, sak = _embed(A, K + pad), K + pad, 1
    else:
        Ad, sam, sak = _embed(A.t(), M + pad), 1, M + pad
    if b_nfast:
        Bd, sbk, sbn = _embed(B, N + pad), N + pad, 1
    else:
        Bd, sbk, sbn = _embed(B.t(), K + pad), 1, K + pad
    return Ad, sam, sak, Bd, sbk, sbn


def _run_gemm(A, B, bias, pattern, pad, slices=1):
    """C = A B (+ bias) through gcdm_op_gemm (+ gcdm_op_reduce_slices when slices > 1); returns C [M, N] (fp32 on the host)."""
    M, K = A.shape
    N = B.shape[1]
    Ad, sam, sak, Bd, sbk, sbn = _gemm_operands(A, B, pattern, pad)
    bd = None if bias is None else bias.to(torch.float32).to(DEV)
    part = _Out(slices * M * N)
    lib = _lib()
    assert lib.gcdm_op_gemm(_ptr(Ad), sam, sak, _ptr(Bd), sbk, sbn, part.p, None if bd is None else _ptr(bd), M, N, K, slices, _stream()) == 0
    if slices == 1:
        return part.get().view(M, N)
    out = _Out(M * N)
    assert lib.gcdm_op_reduce_slices(part.p, out.p, M * N, slices, _stream()) == 0
    part.get()                                                      # guards of the partial buffer
    return out.get().view(M, N)


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("pattern", [0, 1, 2, 3], ids=["Ak_Bn", "Ak_Bk", "Am_Bn", "Am_Bk"])
def test_gemm_small_integers_equal_fp64_at_every_tile_edge(pattern, pad):
    """gcdm_op_gemm, all four stride patterns (pattern 3, sak != 1 and sbn != 1, is reachable only through the C ABI), with and without a
    leading dimension wider than the row: small-integer operands, so C must equal the fp64 product exactly."""
    g = _gen(100 + 10 * pattern + pad)
    for M in (1, 63, 64, 65, 129):
        for N in (1, 31, 64, 65):
            for K in (0, 1, 15, 16, 17, 1000):
                A, B = _ints((M, K), g), _ints((K, N), g)
                bias = _ints((N,), g) if (M + N + K) % 2 else None
                want = A @ B + (0 if bias is None else bias)
                _exact(_run_gemm(A, B, bias, pattern, pad), want, f"gemm M={M} N={N} K={K} bias={bias is not None}")


@pytest.mark.parametrize("pattern", [0, 1, 2, 3], ids=["Ak_Bn", "Ak_Bk", "Am_Bn", "Am_Bk"])
def test_gemm_split_k_slices_and_bias_once(pattern):
    """Split K: slice z writes C + z M N, gcdm_op_reduce_slices adds them.  slices * 16 > K leaves trailing slices empty (they must write 0);
    the bias is added exactly once.  Small integers: exact."""
    g = _gen(200 + pattern)
    M, N = 65, 33
    for K in (1, 17, 513, 40000):
        A, B = _ints((M, K), g), _ints((K, N), g)
        bias = _ints((N,), g).clamp(min=1)                          # nonzero: a bias added in more than one slice shows
        for slices in (1, 2, 3, 7, 64):
            for b in (None, bias):
                want = A @ B + (0 if b is None else b)
                _exact(_run_gemm(A, B, b, pattern, 3, slices), want, f"gemm K={K} slices={slices} bias={b is not None}")


@pytest.mark.parametrize("pattern", [0, 1, 2, 3], ids=["Ak_Bn", "Ak_Bk", "Am_Bn", "Am_Bk"])
def test_gemm_gaussian_within_the_summation_bound(pattern):
    """Gaussian operands: |C - C64| <= gamma_n (|A| |B| + |bias|) with n = K (+ 1 for the bias), gamma_n = n u / (1 - n u) -- the bound of
    an n-term dot product computed in fp32 in ANY order (Higham, Accuracy and Stability, 3.1), so it holds for every slicing."""
    g = _gen(300 + pattern)
    for M, N, K, slices in ((129, 65, 1000, 1), (63, 31, 17, 1), (1, 64, 1000, 1), (65, 33, 40000, 7), (64, 65, 513, 64)):
        A, B = _gauss((M, K), g), _gauss((K, N), g)
        bias = _gauss((N,), g)
        A, B, bias = A.float().double(), B.float().double(), bias.float().double()     # the fp32 inputs the kernel sees
        got = _run_gemm(A, B, bias, pattern, 0, slices)
        bound = _gamma(K + 1) * (A.abs() @ B.abs() + bias.abs())
        _within(got, A @ B + bias, bound, f"gemm gaussian M={M} N={N} K={K} slices={slices}")


# ---- linear (autograd): dx, dW on the split path, db on both sides of M = 4096 ------------------------------------------------------------------
LEADS = {6: (2, 3), 4095: (5, 819), 4096: (64, 64), 4097: (17, 241), 100000: (100, 1000)}


def _linear_ref(x, W, b, dy):
    """nn.Linear of GCP / GCP2 (gcpnet.py:85-118, 320-348): y = x W^T + b, and its fp64 autograd."""
    x64, W64, b64 = (t.clone().requires_grad_() for t in (x, W, b))
    y = F.linear(x64, W64, b64)
    y.backward(dy)
    return y.detach(), x64.grad, W64.grad, b64.grad


def _linear_hip(x, W, b, dy):
    xd, Wd, bd = (t.to(torch.float32).to(DEV).requires_grad_() for t in (x, W, b))
    y = ops.linear(xd, Wd, bd)
    y.backward(dy.to(torch.float32).to(DEV))
    return y, xd.grad, Wd.grad, bd.grad


@pytest.mark.parametrize("M", sorted(LEADS))
def test_linear_forward_and_gradients(M):
    """ops.linear on a 3-D input.  dW = dy^T x runs split-K once M >= 512 rows; db switches from gcdm_op_colsum to colsum_slices +
    reduce_slices at M = 4096 (ops.py).  Small integers: y, dx, dW, db equal fp64 autograd exactly.  Gaussian: within the gamma_n bound of
    each contraction, and a second backward pass gives dW and db bit for bit (fixed summation order)."""
    K, N = 24, 40
    g = _gen(M)
    lead = LEADS[M]
    x, W, b, dy = _ints((*lead, K), g), _ints((N, K), g), _ints((N,), g), _ints((*lead, N), g)
    ref = _linear_ref(x, W, b, dy)
    for got, want, what in zip(_linear_hip(x, W, b, dy), ref, ("y", "dx", "dW", "db")):
        _exact(got, want, f"linear M={M} {what}")

    x, W, b, dy = (t.float().double() for t in (_gauss((*lead, K), g), _gauss((N, K), g), _gauss((N,), g), _gauss((*lead, N), g)))
    y64, dx64, dW64, db64 = _linear_ref(x, W, b, dy)
    y, dx, dW, db = _linear_hip(x, W, b, dy)
    _within(y, y64, _gamma(K + 1) * (x.abs() @ W.abs().t() + b.abs()), "y")          # K products + bias
    _within(dx, dx64, _gamma(N) * (dy.abs() @ W.abs()), "dx")                         # N products
    x2, dy2 = x.reshape(M, K), dy.reshape(M, N)
    _within(dW, dW64, _gamma(M) * (dy2.abs().t() @ x2.abs()), "dW")                   # M products
    _within(db, db64, _gamma(M) * dy2.abs().sum(0), "db")                             # M terms
    _, _, dW_again, db_again = _linear_hip(x, W, b, dy)
    assert torch.equal(dW, dW_again) and torch.equal(db, db_again), "dW / db differ between two backward passes"


# ---- colsum / colsum_slices / reduce_slices through the C ABI ------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [0, 1, 4095, 4096, 4097])
def test_colsum_and_colsum_slices_equal_fp64(M):
    """Bias gradient db = sum over rows of dy: gcdm_op_colsum, and gcdm_op_colsum_slices (slice counts up to more than M, whose trailing
    slices are empty and must write 0) + gcdm_op_reduce_slices.  Small integers: exact."""
    g = _gen(400 + M)
    lib = _lib()
    for N in (1, 63, 64, 65, 352):
        dy = _ints((M, N), g)
        dyd = torch.cat((dy.flatten(), torch.zeros(1, dtype=torch.float64))).to(torch.float32).to(DEV)   # never empty: not a null pointer
        want = dy.sum(0)
        out = _Out(N)
        assert lib.gcdm_op_colsum(_ptr(dyd), out.p, M, N, _stream()) == 0
        _exact(out.get(), want, f"colsum M={M} N={N}")
        for slices in (1, 3, 256, M + 5):
            part, out = _Out(slices * N), _Out(N)
            assert lib.gcdm_op_colsum_slices(_ptr(dyd), part.p, M, N, slices, _stream()) == 0
            assert lib.gcdm_op_reduce_slices(part.p, out.p, N, slices, _stream()) == 0
            _exact(out.get(), want, f"colsum_slices M={M} N={N} slices={slices}")
            rows = -(-M // slices)
            p = part.get().view(slices, N).double()
            for z in range(slices):                                     # each slice: the sum of its own row range (0 when empty)
                if z in (0, 1, slices - 1) or z * rows >= M:
                    _exact(p[z], dy[z * rows:(z + 1) * rows].sum(0), f"colsum_slices part {z} of {slices}, M={M} N={N}")


# ---- element-wise nonlinearities -------------------------------------------------------------------------------------------------------------
ACTS = ["silu", "relu", "sigmoid", "leakyrelu", "selu"]             # kinds 1..5 of gcdm_op_act


def _act_grid():
    lin = torch.linspace(-30, 30, 20001, dtype=torch.float64)
    lg = torch.logspace(-12, 0, 2001, dtype=torch.float64)
    return torch.cat((lin, lg, -lg, torch.tensor([0.0, -0.0], dtype=torch.float64))).float().double()


def _act_check(name, x, dy, what):
    """forward: |y - y64| <= 8 ulp(y64) + 2^-126 (torch's own fp32 meets this with margin: <= 2.3 ulp on the grid);
    backward: |dx - dx64| <= 8 ulp(dx64) + 8 u |dy| m(x) + 2^-126, where m is the size of the intermediate whose rounding the formula
    amplifies -- sigmoid' = s (1 - s) and silu' = s (1 + x (1 - s)) subtract s (rounded, error ~ u s) from 1, so m = s for sigmoid,
    s (1 + |x|) for silu, 0 for the others."""
    xd = x.to(torch.float32).to(DEV).requires_grad_()
    y = ops.act(xd, name)
    y.backward(dy.to(torch.float32).to(DEV))
    x64 = x.clone().requires_grad_()
    y64 = O._act(name)(x64)
    y64.backward(dy)
    _within(y, y64.detach(), 8 * _ulp(y64.detach()) + TINY, f"{name} forward {what}")
    s = torch.sigmoid(x)
    m = {"sigmoid": s, "silu": s * (1 + x.abs())}.get(name, torch.zeros_like(x))
    _within(xd.grad, x64.grad, 8 * _ulp(x64.grad) + 8 * U * dy.abs() * m + TINY, f"{name} backward {what}")


@pytest.mark.parametrize("name", ACTS)
def test_act_over_the_grid_within_8_ulp(name):
    """x in [-30, 30] and +-logspace(-12, 0), +-0 included; dy = 1."""
    x = _act_grid()
    _act_check(name, x, torch.ones_like(x), "grid")


@pytest.mark.parametrize("name", ACTS)
def test_act_sizes_around_the_block(name):
    g = _gen(500 + ACTS.index(name))
    for n in (1, 255, 256, 257, 2 ** 20 + 3):
        x = (8 * _gauss((n,), g)).float().double()
        _act_check(name, x, _gauss((n,), g).float().double(), f"n={n}")


@pytest.mark.parametrize("name", ACTS)
def test_act_special_values_follow_torch(name):
    """+-0, +-inf, NaN: torch's fp32 result (NaN where torch gives NaN: relu, like the others, must propagate NaN -- the sampler's NaN-in-vel
    guard depends on it).  The derivative at exactly 0 follows torch's convention: relu 0, leakyrelu 0.01, selu scale * alpha."""
    x = torch.tensor([0.0, -0.0, math.inf, -math.inf, math.nan, 1.0, -1.0])
    y = ops.act(x.to(DEV), name).cpu()
    ref = O._act(name)(x)
    assert torch.equal(torch.isnan(y), torch.isnan(ref)), (name, y.tolist(), ref.tolist())
    inf = torch.isinf(ref)
    assert torch.equal(y[inf], ref[inf]), (name, y.tolist(), ref.tolist())
    ok = torch.isfinite(ref)
    _within(y[ok], ref[ok].double(), 8 * _ulp(ref[ok].double()) + TINY, f"{name} special values")
    x0 = torch.zeros(1, device=DEV, requires_grad=True)
    ops.act(x0, name).backward(torch.ones(1, device=DEV))
    want = {"silu": 0.5, "relu": 0.0, "sigmoid": 0.25, "leakyrelu": 0.01, "selu": 1.0507009873554804934193349852946 * 1.6732632423543772848170429916717}[name]
    assert abs(x0.grad.item() - want) <= 8 * U * abs(want), (name, x0.grad.item(), want)


# ---- safe_norm ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rep", [False, True], ids=["pre", "rep"])
def test_safe_norm_both_layouts(rep):
    """out = sqrt(sum_xyz v^2 + 1e-8) + 1e-8 (O.safe_norm, components/__init__.py:275-286), with zero vectors and components of 1e-20 and
    1e18.  Forward: the sum of three squares and eps (all >= 0) has relative error <= gamma_6 (6 u); the sqrt halves it and adds one rounding,
    + eps one more: <= 5 u, asserted as 8 u |out64|.  Backward dv = dout v / (out - eps): out - eps recovers sqrt(s + eps) to <= 6 u, one
    division and two products: <= 10 u, asserted as 16 u |dout| |v| / sqrt(s + eps) (+ 2^-126)."""
    g = _gen(600 + rep)
    lib_dim = -1 if rep else -2
    for Cn in (1, 3, 17, 352):
        M = 37
        v = _gauss((M, Cn, 3) if rep else (M, 3, Cn), g)
        vv = v if rep else v.transpose(1, 2)                            # a [M, C, 3] view either way
        vv[0] = 0.0
        vv[1, :, 0], vv[1, :, 1:] = 1e-20, 0.0
        vv[2] = 1e18
        vv[3, :, 0], vv[3, :, 1], vv[3, :, 2] = 1e18, 1e-20, 0.0
        v = v.float().double()
        dout = _gauss((M, Cn), g).float().double()
        vd = v.to(torch.float32).to(DEV).requires_grad_()
        out = (ops.safe_norm_rep if rep else ops.safe_norm_pre)(vd)
        out.backward(dout.to(torch.float32).to(DEV))
        v64 = v.clone().requires_grad_()
        out64 = O.safe_norm(v64, dim=lib_dim)
        out64.backward(dout)
        _within(out, out64.detach(), 8 * U * out64.detach(), f"safe_norm C={Cn}")
        root = torch.sqrt((v ** 2).sum(lib_dim) + 1e-8).unsqueeze(lib_dim)
        _within(vd.grad, v64.grad, 16 * U * dout.unsqueeze(lib_dim).abs() * v.abs() / root + TINY, f"safe_norm backward C={Cn}")


# ---- scalarize / vectorize / rowscale ----------------------------------------------------------------------------------------------------------
def _scalarize_ref(u_pre, Fm):
    """scalarize in edge mode (components/__init__.py:174-224; O.scalarize for CH = 3): out[m][3 c + r] = F[m][r][:] . u[m][:][c]."""
    return torch.einsum("mrx,mxc->mcr", Fm, u_pre).reshape(u_pre.shape[0], -1)


def _vectorize_ref(gate, Fm):
    """vectorize in edge mode (components/__init__.py:227-272; O.vectorize for KC = 3): out[m][k] = sum_r gate[m][3 k + r] F[m][r]."""
    return torch.matmul(gate.reshape(gate.shape[0], -1, 3), Fm)


def test_scalarize_vectorize_references_agree_with_the_oracle():
    g = _gen(700)
    u, Fm, gate = _gauss((5, 3, 3), g), _gauss((5, 3, 3), g), _gauss((5, 9), g)
    row = torch.arange(5)
    assert torch.allclose(_scalarize_ref(u, Fm), O.scalarize(u.transpose(1, 2), row, Fm, False, 5))
    assert torch.allclose(_vectorize_ref(gate, Fm), O.vectorize(gate, row, Fm, False, 5))


def _autograd_pair(fn_hip, fn_ref, inputs, dout):
    dev = [t.to(torch.float32).to(DEV).requires_grad_() for t in inputs]
    y = fn_hip(*dev)
    y.backward(dout.to(torch.float32).to(DEV))
    ref = [t.clone().requires_grad_() for t in inputs]
    y64 = fn_ref(*ref)
    y64.backward(dout)
    return (y, *[t.grad for t in dev]), (y64.detach(), *[t.grad for t in ref])


@pytest.mark.parametrize("M", [1, 257])
def test_scalarize_vectorize_rowscale_small_integers_exact(M):
    """Frames with integer rows, integer vectors / gates / gradients: forward and backward equal fp64 autograd exactly."""
    g = _gen(710 + M)
    for CH in (1, 3, 16, 33):
        Fm = _ints((M, 3, 3), g)
        got, want = _autograd_pair(lambda u: ops.scalarize(u, Fm.float().to(DEV)), lambda u: _scalarize_ref(u, Fm), [_ints((M, 3, CH), g)],
                                   _ints((M, 3 * CH), g))
        for a, b, what in zip(got, want, ("out", "du")):
            _exact(a, b, f"scalarize M={M} CH={CH} {what}")
        got, want = _autograd_pair(lambda gt: ops.vectorize(gt, Fm.float().to(DEV)), lambda gt: _vectorize_ref(gt, Fm), [_ints((M, 3 * CH), g)],
                                   _ints((M, CH, 3), g))
        for a, b, what in zip(got, want, ("out", "dgate")):
            _exact(a, b, f"vectorize M={M} KC={CH} {what}")
        got, want = _autograd_pair(ops.rowscale, lambda v, s: v * s.unsqueeze(-1), [_ints((M, CH, 3), g), _ints((M, CH), g)], _ints((M, CH, 3), g))
        for a, b, what in zip(got, want, ("out", "dv", "dg")):
            _exact(a, b, f"rowscale M={M} C={CH} {what}")


# ---- graph plumbing -------------------------------------------------------------------------------------------------------------------------
SIZES = [0, 1, 2, 19, 0, 181, 1, 0]


def _fc_ref(sizes):
    n = torch.tensor(sizes, dtype=torch.int64)
    if int(n.sum()) == 0:
        return torch.zeros((2, 0), dtype=torch.int64)
    return torch.stack(O.fully_connected_edges(O.num_nodes_to_batch_index(n)))


@pytest.mark.parametrize("sizes", [SIZES, [181], [1], [0], [3, 0], [0, 0, 2]], ids=["ragged", "one181", "one1", "empty", "trailing0", "leading0"])
def test_fully_connected_edge_index_equals_oracle(sizes):
    got = ops.fully_connected_edge_index(torch.tensor(sizes), DEV).cpu()
    want = _fc_ref(sizes)
    assert torch.equal(got, want), (sizes, got.shape, want.shape)


def _hand_graph():
    """A row-sorted edge list over 10 nodes: nodes 0 (first), 4 (interior) and 9 (last) have no edges; (1, 2), (3, 9) and (7, 7) repeat."""
    row = torch.tensor([1, 1, 1, 2, 3, 3, 3, 5, 5, 6, 7, 7, 7, 8])
    col = torch.tensor([2, 2, 0, 2, 9, 9, 4, 5, 1, 0, 7, 7, 3, 8])
    return torch.stack((row, col)), 10


def _graphs():
    ei, N = _hand_graph()
    fc = _fc_ref(SIZES)
    return [("hand", ei, N), ("fc", fc, sum(SIZES))]


def _scatter_ref(x, row, N, mean):
    """torch_scatter.scatter(x, row, dim=0, dim_size=N, reduce=sum | mean) (gcpnet.py:723; components/__init__.py:214, 262): counts clamped to 1."""
    out = torch.zeros((N, *x.shape[1:]), dtype=x.dtype).index_add_(0, row, x)
    if not mean:
        return out
    cnt = torch.zeros(N, dtype=x.dtype).index_add_(0, row, torch.ones(row.shape[0], dtype=x.dtype)).clamp(min=1)
    return out / cnt.reshape(-1, *[1] * (x.dim() - 1))


@pytest.mark.parametrize("which", [0, 1], ids=["hand", "fc_ragged"])
def test_graph_rowptr_gathers_and_segment_sums(which):
    """Graph / gcdm_op_rowptr against torch.searchsorted; gather_row / gather_col (ScalarVector.idx, gcpnet.py:688-689) and their backwards
    (a segment sum over the sorted row index, atomics over the repeated column index); scatter_rows sum and mean.  Small integers: sums
    exact; a mean is an exact sum and one division, so within u |y64|.  Nodes without edges get 0 under mean (count clamped to 1)."""
    name, ei, N = _graphs()[which]
    g = _gen(800 + which)
    graph = ops.Graph(ei.to(DEV), N)
    row, col = ei[0], ei[1]
    E = row.shape[0]
    assert torch.equal(graph.rowptr.cpu().long(), torch.searchsorted(row, torch.arange(N + 1), side="left")), name
    for shape in ((N, 5), (N, 3, 3)):
        for by_row, idx in ((True, row), (False, col)):
            x, dout = _ints(shape, g), _ints((E, *shape[1:]), g)
            got, want = _autograd_pair(lambda t: (ops.gather_row if by_row else ops.gather_col)(t, graph), lambda t: t[idx], [x], dout)
            for a, b, what in zip(got, want, ("out", "dx")):
                _exact(a, b, f"{name} gather by_row={by_row} {shape} {what}")
        for mean in (False, True):
            x, dout = _ints((E, *shape[1:]), g), _ints(shape, g)
            got, want = _autograd_pair(lambda t: ops.scatter_rows(t, graph, "mean" if mean else "sum"), lambda t: _scatter_ref(t, row, N, mean),
                                       [x], dout)
            for a, b, what in zip(got, want, ("out", "dx")):
                if mean:
                    _within(a, b, U * b.abs(), f"{name} scatter mean {shape} {what}")
                else:
                    _exact(a, b, f"{name} scatter sum {shape} {what}")
            empty = (torch.bincount(row, minlength=N) == 0)
            assert bool((got[0].cpu()[empty] == 0).all()), "a node without edges must get 0"
    # run to run: the segment sums (forward and the gather_row backward) are deterministic on Gaussian data
    x = _gauss((E, 7), g).float().to(DEV)
    assert torch.equal(ops.scatter_rows(x, graph), ops.scatter_rows(x, graph))
    xn = _gauss((N, 7), g).float().to(DEV).requires_grad_()
    grads = []
    for _ in range(2):
        xn.grad = None
        ops.gather_row(xn, graph).backward(x)
        grads.append(xn.grad.clone())
    assert torch.equal(grads[0], grads[1])


def test_mean_frames_with_edge_mask():
    """Per-node mean of the frames of its edges, masked edges contributing zeros but counting (the reference's scatter-mean of
    `frames * edge_mask`, components/__init__.py:214); nodes without edges: 0.  Small integers: within u |y64| (one division)."""
    g = _gen(900)
    for name, ei, N in _graphs():
        graph = ops.Graph(ei.to(DEV), N)
        E = ei.shape[1]
        frames = _ints((E, 3, 3), g)
        mask = torch.rand(E, generator=g) < 0.7
        got = ops.mean_frames(frames.float().to(DEV), graph, mask.to(DEV))
        want = _scatter_ref(frames * mask.double().reshape(-1, 1, 1), ei[0], N, True)
        _within(got, want, U * want.abs(), f"mean_frames {name}")
        got = ops.mean_frames(frames.float().to(DEV), graph)
        want = _scatter_ref(frames, ei[0], N, True)
        _within(got, want, U * want.abs(), f"mean_frames {name} unmasked")


def test_graph_refuses_an_unsorted_edge_list_and_out_of_range_nodes():
    ei, N = _hand_graph()
    bad = ei.clone()
    bad[0, [3, 4]] = torch.tensor([3, 2])
    with pytest.raises(ValueError, match="sorted"):
        ops.Graph(bad.to(DEV), N)
    for r, c in ((0, 13), (1, 13), (0, 0), (1, 5)):
        bad = ei.clone()
        bad[r, c] = N if c != 0 else -1
        with pytest.raises(IndexError):
            ops.Graph(bad.to(DEV), N)
    ops.Graph(ei.to(DEV), N)                                            # the valid list still builds


def test_embedding_with_repeated_indices():
    """nn.Embedding (gcpnet.py:540-549, 569-570): forward gathers rows, backward adds every repeat's gradient (fp32 atomics; small integers:
    exact in any order)."""
    g = _gen(950)
    W = _ints((7, 5), g)
    idx = torch.tensor([[3, 3, 3, 0, 6, 3], [0, 0, 1, 3, 3, 6], [6, 6, 6, 6, 6, 6], [2, 3, 3, 3, 3, 3]])
    got, want = _autograd_pair(lambda w: ops.embedding(w, idx.to(DEV)), lambda w: w[idx], [W], _ints((*idx.shape, 5), g))
    for a, b, what in zip(got, want, ("out", "dW")):
        _exact(a, b, f"embedding {what}")


# ---- geometry -------------------------------------------------------------------------------------------------------------------------------
def _positions(N, g):
    """Integer positions in -4..4 with the degenerate pairs: x1 = 2 x0 (x_i parallel to x_j: b = 0), x2 = x0 (coincident atoms), x3 = 0."""
    x = _ints((N, 3), g, -4, 4)
    if N >= 2:
        x[1] = 2 * x[0]
    if N >= 3:
        x[2] = x[0]
    if N >= 4:
        x[3] = 0
    return x


def _localize_raw(x, row, col):
    """localize without norm_x_diff (components/__init__.py:123-171): a = x_i - x_j, b = x_i x x_j, c = a x b."""
    a = x[row] - x[col]
    b = torch.linalg.cross(x[row], x[col], dim=-1)
    return torch.stack((a, b, torch.linalg.cross(a, b, dim=-1)), dim=1)


@pytest.mark.parametrize("N", [1, 2, 257])
def test_localize_frames(N):
    """Fully connected edges with self-loops (zero frame), parallel and coincident atoms.  norm_x_diff = 0: integer positions, every term
    exact -> equal.  norm_x_diff = 1 (O.localize): a = d / (|d| + 1) with |d|^2 exact, then sqrt, + 1, division, product: <= 4 u per
    component, asserted as 8 u |a64|, same for b; c = a x b from those: <= 12 u (|a_i b_j| + |a_j b_i|), asserted as 16 u |a64| |b64|."""
    g = _gen(1000 + N)
    x = _positions(N, g)
    row, col = O.fully_connected_edges(torch.zeros(N, dtype=torch.int64))
    ei = torch.stack((row, col)).to(DEV)
    xd = x.float().to(DEV)
    _exact(ops.localize(xd, ei, False), _localize_raw(x, row, col), f"localize raw N={N}")
    got = ops.localize(xd, ei, True)
    want = O.localize(x, row, col)
    a, b = want[:, 0], want[:, 1]
    bound = torch.stack((8 * U * a.abs(), 8 * U * b.abs(), 16 * U * a.norm(dim=-1, keepdim=True) * b.norm(dim=-1, keepdim=True).expand(-1, 3)), 1)
    _within(got, want, bound, f"localize N={N}")
    self_loop = row == col
    assert bool((got.cpu()[self_loop] == 0).all()), "a self-loop's frame is 0"


@pytest.mark.parametrize("N", [1, 2, 257])
def test_edge_features_and_orientations(N):
    """O.edge_features / O.orientations on integer positions: e = |d|^2 exact; the unit vectors d / |d| take sqrt, reciprocal and product:
    <= 3 u per component, asserted as 4 u |ref|; coincident atoms and self-loops give 0, not NaN."""
    g = _gen(1100 + N)
    x = _positions(N, g)
    row, col = O.fully_connected_edges(torch.zeros(N, dtype=torch.int64))
    e, xi = ops.edge_features(x.float().to(DEV), torch.stack((row, col)).to(DEV))
    e64, xi64 = O.edge_features(x, row, col)
    _exact(e, e64, f"edge_features e N={N}")
    _within(xi, xi64, 4 * U * xi64.abs(), f"edge_features xi N={N}")
    ori = ops.orientations(x.float().to(DEV))
    ori64 = O.orientations(x)
    _within(ori, ori64, 4 * U * ori64.abs(), f"orientations N={N}")


@pytest.mark.parametrize("D", [3, 9])
def test_centralize_and_its_backward(D):
    """centralize (O.centralize, components/__init__.py:45-92, edm branch) with masked rows zero on input -- the reference asserts that
    (components/__init__.py:56-57).  Molecules: 4 atoms with 1 masked, 1 atom, 3 atoms all masked, 1 masked atom, 6 atoms with 2 masked.
    Integer inputs: the molecule's sum is exact, then one division and one subtraction: <= u |mean| + u |out|, asserted as 2 u (|x| + |mean|).
    Backward: the kernel applies the same projection to dout; on unmasked rows that is the reference's autograd.  Masked rows are 0 forward
    and backward (the kernel's output there is the constant 0; the reference's is x itself, which must be 0).  An all-masked molecule
    gives 0 here, while the reference's edm branch divides 0 / 0 and returns NaN there."""
    g = _gen(1200 + D)
    sizes = [4, 1, 3, 1, 6]
    on = torch.tensor([1, 0, 1, 1] + [1] + [0, 0, 0] + [0] + [1, 0, 1, 1, 0, 1], dtype=torch.bool)
    bi = O.num_nodes_to_batch_index(torch.tensor(sizes))
    N = bi.shape[0]
    x = _ints((N, D), g) * on.unsqueeze(-1)
    dout = _ints((N, D), g)
    xd = x.float().to(DEV).requires_grad_()
    out = ops.centralize(xd, bi.to(DEV), on.to(DEV))
    out.backward(dout.float().to(DEV))
    x64 = x.clone().requires_grad_()
    out64 = O.centralize(x64, bi, len(sizes), on)
    live = on                                                            # (the all-masked molecule has no unmasked row)
    out64.backward(dout)
    out, dx = out.detach().cpu().double(), xd.grad.cpu().double()
    mean = x64.detach() - out64.detach()
    _within(out[live], out64.detach()[live], 2 * U * (x[live].abs() + mean[live].abs()), f"centralize D={D}")
    assert bool((out[~on] == 0).all()) and bool((dx[~on] == 0).all()), "masked rows are 0 forward and backward"
    dmean = (dout * on.unsqueeze(-1) - x64.grad)[live]                    # the molecule's mean of dout over its unmasked rows
    _within(dx[live], x64.grad[live], 2 * U * ((dout[live]).abs() + dmean.abs()), f"centralize backward D={D}")
    all_masked = bi == 2
    assert bool(torch.isnan(out64.detach()[all_masked]).all()), "the reference divides 0 / 0 for an all-masked molecule"
    assert bool((out[all_masked] == 0).all())
    assert bool((out[bi == 1] == 0).all()), "a one-atom molecule centres to 0"
