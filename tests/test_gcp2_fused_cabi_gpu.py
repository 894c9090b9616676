"""gcdm_gcp2_fwd / gcdm_gcp2_bwd (include/gcdm_gcp2_train.h) called directly through the C ABI on an MI355X, against oracle.gcdm_oracle.gcp2 in
fp64 on the CPU and its fp64 autograd (tests/gcp2_ref.py) -- never the operator path, never the code under test.

Harness (run_fwd / run_bwd): every output, the forward workspace, the tape and the backward scratch are exactly the advertised number of floats
inside a larger buffer, NaN inside, sentinel guard words around.  A read of workspace no kernel wrote poisons the result, a write past the
advertised size breaks a guard, an output entry no kernel wrote stays NaN and fails every bar.

The bar (gcp2_ref.compare) is measured, not fixed: per tensor and, for s_out / v_out / ds / dv, per row,
max|got - ref64| <= M * max|ref32 - ref64| + 8 * 2^-24 * max|ref64|, ref32 being the oracle's own fp32 CPU run on ONE thread.  M = 4 everywhere
except the tensors of MARGINS (none above 16); the measured worst factors are printed by every test ("MEASURED ...") and recorded in DESIGN.md 3.6.

Measured on an MI355X (worst factor needed per case, over the tensors and rows of all row counts 1, 63, 64, 65, 193, 1 216; QM9 / GEOM dims):

    case                                   worst factor        tensor (reason where above 1)
    golden edge / node / nodeff / proj     0                   (all errors under the 8 U floor)
    edge embedding, M <= 1 216             < 1 / < 1
    edge embedding, M = 21 888             1.34 / 0.73         vector_up.weight, vector_out_scale.bias 1.30: 16 split-K slices, each a sequential chain
                                                               of 3 M / 16 (M / 16) terms, against torch's blocked column sum
    node embedding                         0.78 / 0.76         ds
    feed-forward (2s, 2v) -> (s, v)        1.70 / 1.70         scalar_out.2.weight at M = 1 (its gap is one fp32 product per entry); s_out rows 1.24:
                                                               K = 537 and K = 256 summed in sequence by the MFMA, blocked by the oracle's fp32 run
    position (s, v) -> (s, 1)              3.29 / 3.29         one row of s_out at M = 1 216 (K = 273 in sequence; the tensor as a whole needs 0.73)
    projection (s, v) -> (h_in, 0)         0.32 / 1.17         s_out
    self-conditioning widths               1.00 / 0.67         ds
    identity / silu in each place, ff 0/1  0.14
    v = 0 rows                             0.89                s_out
    zero frames (mask, isolated node)      3.09                vector_out_scale.bias of the position GCP (VO = 1): ONE number, a single draw
    saturated gates                        1.00                vector_out_scale.bias
    the module through autograd            1.41                s_out

No tensor needs more than M = 4, so MARGINS is empty.  (An earlier version of the saturated case scaled s by 300 instead of setting the biases; it
needed 28.9 on one row of v_out.  The cause was the input, not the kernels: see saturated_case.)
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gcp2_ref as R  # noqa: E402

pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
TILE = 64                          # rows per workgroup of the GEMM kernels (the down kernels take 4)
MARGINS = {}                       # tensor -> M for documented exceptions (docstring table)


def _lib():
    return native.load_ops()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cd(d):
    return native.Gcp2Dims(d["SI"], d["VI"], d["SO"], d["VO"], d["H"], d["ff"], d["a0"], d["a1"])


class _Out:
    """`n` floats inside a larger device buffer: NaN inside, a finite sentinel in the GUARD words before and after."""
    SENTINEL = 12345.5

    def __init__(self, n):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * GUARD,), self.SENTINEL, dtype=torch.float32, device=DEV)
        self.inner = self.buf[GUARD:GUARD + self.n]
        self.inner.fill_(float("nan"))
        self.p = C.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def check(self):
        assert bool((self.buf[:GUARD] == self.SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == self.SENTINEL).all()), "write outside the buffer"

    def untouched(self):
        self.check()
        return bool(self.inner.isnan().all())

    def get(self):
        self.check()
        return self.inner.cpu()

    def bits(self):
        return self.inner.view(torch.int32).clone()


def _bytes(which, M, d):
    n = int(_lib().gcdm_gcp2_workspace_bytes(which, M, C.byref(_cd(d))))
    assert n >= 0 and n % 4 == 0
    return n // 4


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev_weights(W, d):
    ws = [W[k].to(DEV).contiguous() for k in R.weight_keys(d["ff"], d["VO"])]
    return ws, (C.c_void_p * len(ws))(*[w.data_ptr() for w in ws])


def run_fwd(d, W, s, v, F, row_mask, tape, stream=None):
    M = s.shape[0]
    ws, wp = _dev_weights(W, d)
    t = [x.to(DEV).contiguous() for x in (s, v, F.reshape(-1, 9))]
    mk = None if row_mask is None else row_mask.to(torch.uint8).to(DEV).contiguous()
    s_out, v_out, work = _Out(M * d["SO"]), _Out(M * d["VO"] * 3), _Out(_bytes(int(tape), M, d))
    st = _lib().gcdm_gcp2_fwd(_ptr(t[0]), _ptr(t[1]), _ptr(t[2]), _ptr(mk), wp, s_out.p, v_out.p if d["VO"] else None, work.p, int(tape), M,
                              C.byref(_cd(d)), stream if stream is not None else _stream())
    torch.cuda.synchronize()
    for o in (s_out, v_out, work):
        o.check()
    del ws, mk
    return st, s_out, v_out, work


def run_bwd(d, W, s, v, F, row_mask, tape, rs, rv, stream=None):
    M = s.shape[0]
    ws, wp = _dev_weights(W, d)
    t = [x.to(DEV).contiguous() for x in (rs, rv, s, v, F.reshape(-1, 9))]
    mk = None if row_mask is None else row_mask.to(torch.uint8).to(DEV).contiguous()
    outs = dict(ds=_Out(M * d["SI"]), dv=_Out(M * d["VI"] * 3), dweights=_Out(_bytes(3, M, d)), scratch=_Out(_bytes(2, M, d)))
    st = _lib().gcdm_gcp2_bwd(_ptr(t[0]), _ptr(t[1]) if d["VO"] else None, _ptr(t[2]), _ptr(t[3]), _ptr(t[4]), _ptr(mk), wp, tape.p, outs["scratch"].p,
                              outs["ds"].p, outs["dv"].p, outs["dweights"].p, M, C.byref(_cd(d)), stream if stream is not None else _stream())
    torch.cuda.synchronize()
    for o in outs.values():
        o.check()
    tape.check()
    del ws, mk
    return st, outs


def _named(d, W, M, s_out, v_out, outs=None):
    got = {"s_out": s_out.get().view(M, d["SO"]), "v_out": v_out.get().view(M, d["VO"], 3)}
    if outs is not None:
        got["ds"], got["dv"] = outs["ds"].get().view(M, d["SI"]), outs["dv"].get().view(M, d["VI"], 3)
        dw, o = outs["dweights"].get(), 0
        for k in R.weight_keys(d["ff"], d["VO"]):
            n = W[k].numel()
            got[k] = dw[o:o + n].view(W[k].shape)
            o += n
        assert o == dw.numel()
    return got


def _check(what, d, W, s, v, F, rs, rv, row_mask=None):
    """Forward with a tape + backward against fp64 under the measured bar; the tape-free forward bitwise against the taped one; the tape
    unchanged by the backward."""
    M = s.shape[0]
    ref64, ref32 = R.references(W, d, s, v, F, rs, rv, row_mask)
    st, s_out, v_out, tape = run_fwd(d, W, s, v, F, row_mask, 1)
    assert st == 0
    before = tape.bits()
    st, outs = run_bwd(d, W, s, v, F, row_mask, tape, rs, rv)
    assert st == 0
    assert torch.equal(before, tape.bits()), "the backward wrote to the tape"
    st, s0, v0, _ = run_fwd(d, W, s, v, F, row_mask, 0)
    assert st == 0
    assert torch.equal(s0.bits(), s_out.bits()) and torch.equal(v0.bits(), v_out.bits()), "the tape-free forward differs from the taped one"
    got = _named(d, W, M, s_out, v_out, outs)
    failures, ratios = R.compare(got, ref64, ref32, MARGINS, what)
    name, worst = R.worst_ratio(ratios)
    print(f"\nMEASURED {what} M={M}: worst factor {worst:.3g} ({name}); tensor / row: " +
          ", ".join(f"{k}={r[0]:.2f}/{r[1]:.2f}" for k, r in ratios.items() if max(r) > 1))
    assert not failures, "\n".join(failures)
    return got


# ---- the reference's recorded evaluations ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,node", [("edge", False), ("node", True), ("nodeff", True), ("proj", True)])
def test_golden_fixture(golden_dir, name, node):
    g = {k: torch.tensor(v) for k, v in np.load(os.path.join(golden_dir, "fn_gcp2.npz")).items()}
    d, W, s, v, F, _, want_s, want_v = R.golden_case(g, name, node)
    M = s.shape[0]
    st, s_out, v_out, _ = run_fwd(d, W, s, v, F, None, 0)
    assert st == 0
    assert (s_out.get().view(M, -1) - want_s).abs().max().item() <= 2e-6
    if want_v is not None:
        assert (v_out.get().view(M, -1, 3) - want_v).abs().max().item() <= 2e-6
    g_ = torch.Generator().manual_seed(11)
    rs, rv = torch.randn((M, d["SO"]), generator=g_), torch.randn((M, d["VO"], 3), generator=g_)
    _check(f"golden {name}", d, W, s, v, F, rs, rv)


# ---- the five production instances --------------------------------------------------------------------------------------------------------------
ROWS = (1, TILE - 1, TILE, TILE + 1, 3 * TILE + 1, 64 * 19)


@pytest.mark.parametrize("case", ["qm9", "geom"])
@pytest.mark.parametrize("inst", ["edge", "node", "ff", "pos", "proj"])
def test_production_instance(case, inst):
    d = R.instances(case)[inst]
    W = R.make_weights(d)
    for M in ROWS:
        _check(f"{case} {inst}", d, W, *R.make_rows(d, M, seed=5 + M))


@pytest.mark.parametrize("case", ["qm9", "geom"])
def test_edge_embedding_at_the_edge_count_of_a_training_batch(case):
    d = R.instances(case)["edge"]
    _check(f"{case} edge", d, R.make_weights(d), *R.make_rows(d, 64 * 19 * 18, seed=9))


@pytest.mark.parametrize("case", ["qm9", "geom"])
@pytest.mark.parametrize("inst", ["edge", "node"])
def test_self_conditioning_input_widths(case, inst):
    d = R.instances(case, self_cond=True)[inst]
    _check(f"{case} {inst} self-cond", d, R.make_weights(d), *R.make_rows(d, TILE + 1, seed=4))


# ---- degenerate rows ---------------------------------------------------------------------------------------------------------------------------
SMALL = dict(SI=10, VI=6, SO=70, VO=5, H=3)          # SO: one full column tile + a partial one


@pytest.mark.parametrize("ff", [0, 1])
@pytest.mark.parametrize("a0,a1", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_identity_and_silu_in_each_place(ff, a0, a1):
    d = R.dims(**SMALL, ff=ff, a0=a0, a1=a1)
    _check(f"small ff={ff} acts=({a0},{a1})", d, R.make_weights(d), *R.make_rows(d, TILE + 3, seed=2))


@pytest.mark.parametrize("inst", ["edge", "pos", "ff"])
def test_zero_vectors_take_the_safe_norm_eps_branch(inst):
    d = R.instances("qm9")[inst]
    s, v, F, rs, rv = R.make_rows(d, TILE + 1, seed=6)
    v[::3] = 0.0                                     # |vh| = sqrt(1e-8) + 1e-8, gradient 0
    v[1, 0] = 1e-6
    got = _check(f"v = 0 {inst}", d, R.make_weights(d), s, v, F, rs, rv)
    assert torch.isfinite(got["dv"]).all()


@pytest.mark.parametrize("inst", ["node", "pos", "proj"])
def test_zero_frames_from_the_mask_and_from_an_isolated_node(inst):
    d = R.instances("qm9")[inst]
    s, v, F, rs, rv = R.make_rows(d, TILE + 1, seed=7)
    F[5] = 0.0                                       # an isolated node: the mean over no edges
    mask = torch.ones(TILE + 1, dtype=torch.bool)
    mask[[0, 17, TILE]] = False
    W = R.make_weights(d)
    got = _check(f"zero frames {inst}", d, W, s, v, F, rs, rv, row_mask=mask)
    # a masked row is the row with a zero frame: same bits
    F0 = F * mask.float().reshape(-1, 1, 1)
    st, s1, v1, _ = run_fwd(d, W, s, v, F0, None, 0)
    assert st == 0 and torch.equal(s1.get().view_as(got["s_out"]), got["s_out"])


def saturated_case(inst):
    """Inputs with every gate and every p far from 0: the last bias of scalar_out is +-50 by channel (|p| large: silu and its derivative at their
    0 / 1 ends, exp(-p) over and under 1), vector_out_scale.bias is +-200 by channel (every sigmoid at 0 or 1 to the last bit, its derivative 0).
    Scaling s instead leaves a few gates of a row in the sigmoid's transition; that row's fp32-vs-fp64 gap is then the rounding of ONE gate
    pre-activation, a single draw: a second fp32 run of the oracle itself (K summed in pairs in sequence) needs M = 15.8 per row of v_out
    there, so that input measures the draw, not the code."""
    d = R.instances("qm9")[inst]
    W = R.make_weights(d)
    sign = lambda n: 1.0 - 2.0 * (torch.arange(n) % 2)
    W["scalar_out.2.bias" if d["ff"] else "scalar_out.bias"] = 50.0 * sign(d["SO"])
    W["vector_out_scale.bias"] = 200.0 * sign(d["VO"])
    return d, W, R.make_rows(d, TILE + 1, seed=8)


@pytest.mark.parametrize("inst", ["edge", "pos", "ff"])
def test_saturated_gates(inst):
    d, W, rows = saturated_case(inst)
    got = _check(f"saturated {inst}", d, W, *rows)
    assert all(torch.isfinite(t).all() for t in got.values())
    sg = got["v_out"].abs().amax(dim=(0, 2))
    assert (sg[1::2] < 1e-30).all() and (d["VO"] == 1 or (sg[0::2] > 1e-3).all())          # closed and open gates, by channel


# ---- header contracts ----------------------------------------------------------------------------------------------------------------------------
def test_empty_work_writes_nothing():
    d = R.instances("qm9")["pos"]
    W = R.make_weights(d)
    ws, wp = _dev_weights(W, d)
    outs = [_Out(256) for _ in range(6)]
    cd = _cd(d)
    assert _lib().gcdm_gcp2_fwd(outs[0].p, outs[0].p, outs[0].p, None, wp, outs[1].p, outs[2].p, outs[3].p, 1, 0, C.byref(cd), _stream()) == 0
    assert _lib().gcdm_gcp2_bwd(outs[0].p, outs[0].p, outs[0].p, outs[0].p, outs[0].p, None, wp, outs[3].p, outs[4].p, outs[1].p, outs[2].p, outs[5].p, 0,
                                C.byref(cd), _stream()) == 0
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)


def test_bad_arguments_return_minus_one_with_the_guards_intact():
    d = R.instances("qm9")["pos"]
    W = R.make_weights(d)
    M = 5
    s, v, F, rs, rv = R.make_rows(d, M)
    ws, wp = _dev_weights(W, d)
    t = [x.to(DEV).contiguous() for x in (s, v, F.reshape(-1, 9), rs, rv)]
    o = dict(s_out=_Out(M * d["SO"]), v_out=_Out(M * 3), work=_Out(_bytes(1, M, d)), scratch=_Out(_bytes(2, M, d)), ds=_Out(M * d["SI"]),
             dv=_Out(M * d["VI"] * 3), dw=_Out(_bytes(3, M, d)))
    lib = _lib()

    def fwd(**kw):
        a = dict(s=_ptr(t[0]), v=_ptr(t[1]), F=_ptr(t[2]), mask=None, w=wp, s_out=o["s_out"].p, v_out=o["v_out"].p, work=o["work"].p, tape=1, M=M, cd=_cd(d))
        a.update(kw)
        return lib.gcdm_gcp2_fwd(a["s"], a["v"], a["F"], a["mask"], a["w"], a["s_out"], a["v_out"], a["work"], a["tape"], a["M"],
                                 None if a["cd"] is None else C.byref(a["cd"]), _stream())

    def bwd(**kw):
        a = dict(rs=_ptr(t[3]), rv=_ptr(t[4]), s=_ptr(t[0]), v=_ptr(t[1]), F=_ptr(t[2]), mask=None, w=wp, tape=o["work"].p, scratch=o["scratch"].p,
                 ds=o["ds"].p, dv=o["dv"].p, dw=o["dw"].p, M=M, cd=_cd(d))
        a.update(kw)
        return lib.gcdm_gcp2_bwd(a["rs"], a["rv"], a["s"], a["v"], a["F"], a["mask"], a["w"], a["tape"], a["scratch"], a["ds"], a["dv"], a["dw"], a["M"],
                                 None if a["cd"] is None else C.byref(a["cd"]), _stream())

    bad_w = (C.c_void_p * len(ws))(*[w.data_ptr() for w in ws])
    bad_w[3] = None
    big = _cd(d)
    big.VO = 65
    for kw in (dict(s=None), dict(v=None), dict(F=None), dict(w=None), dict(w=bad_w), dict(s_out=None), dict(v_out=None), dict(work=None), dict(tape=2),
               dict(tape=-1), dict(M=-1), dict(M=2 ** 28 + 1), dict(cd=None), dict(cd=big)):
        assert fwd(**kw) == -1, kw
    for kw in (dict(rs=None), dict(rv=None), dict(s=None), dict(v=None), dict(F=None), dict(w=None), dict(w=bad_w), dict(tape=None), dict(scratch=None),
               dict(ds=None), dict(dv=None), dict(dw=None), dict(M=-1), dict(cd=None), dict(cd=big)):
        assert bwd(**kw) == -1, kw
    torch.cuda.synchronize()
    assert all(x.untouched() for x in o.values())


def test_bitwise_repeatable_and_row_invariant_and_on_a_side_stream():
    for inst in ("ff", "pos"):
        d = R.instances("qm9")[inst]
        W = R.make_weights(d)
        M = 3 * TILE + 1
        s, v, F, rs, rv = R.make_rows(d, M, seed=12)
        runs = []
        side = torch.cuda.Stream()
        for stream in (None, None, C.c_void_p(side.cuda_stream)):
            st, s_out, v_out, tape = run_fwd(d, W, s, v, F, None, 1, stream=stream)
            assert st == 0
            st, outs = run_bwd(d, W, s, v, F, None, tape, rs, rv, stream=stream)
            assert st == 0
            runs.append([s_out.bits(), v_out.bits(), tape.bits()] + [outs[k].bits() for k in ("ds", "dv", "dweights")])
            assert not any(outs[k].get().isnan().any() for k in ("ds", "dv", "dweights")), "an advertised output entry was not written"
            assert not s_out.get().isnan().any() and not v_out.get().isnan().any()
        for other in runs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(runs[0], other)), "two runs differ in their bits"
        # a row alone, and inside another batch at another position, has the same bits
        s_all, v_all = runs[0][0].view(M, d["SO"]), runs[0][1].view(M, d["VO"] * 3)
        for r in (0, TILE - 1, TILE, M - 1):
            st, s1, v1, _ = run_fwd(d, W, s[r:r + 1], v[r:r + 1], F[r:r + 1], None, 0)
            assert st == 0 and torch.equal(s1.bits().view(-1), s_all[r]) and torch.equal(v1.bits().view(-1), v_all[r]), (inst, r)
        perm = torch.randperm(M, generator=torch.Generator().manual_seed(1))[:TILE + 7]
        st, s2, v2, _ = run_fwd(d, W, s[perm], v[perm], F[perm], None, 0)
        assert st == 0 and torch.equal(s2.bits().view(len(perm), -1), s_all[perm.to(DEV)]) and torch.equal(v2.bits().view(len(perm), -1), v_all[perm.to(DEV)])
