"""gcdm_egnn_train_edge_fwd / gcdm_egnn_train_edge_bwd (include/gcdm_egnn_train.h) called directly through the C ABI on an MI355X, against the
hand-written fp64 reference (tests/egnn_train_ref.py, reference (b), which tests/test_egnn_train_cpu.py holds to fp64 autograd at 6e-13).

Shapes: (H, Eh) = (32, 8) -- K = 146, no multiple of 16 -- and (64, 64), e_in 1 and 2, molecules of 1, 2, 3, 17, 33 and 70 atoms in one batch of
126 atoms (no multiple of 32): a one-slot owner, slot lists that cross a 16-edge MFMA tile, a wave's share and a round of 128 (backward) or 256
(forward) edges; the same molecules five times over (630 atoms: owner blocks of three owners that hold several molecules, molecules split over
owner blocks) and 1000 molecules of 9 atoms (owner blocks of 32, more blocks than workgroups); a batch of one atom; a coincident pair.

Harness: every buffer the library writes (M, dx, the eleven gradients, the workspace) sits at exactly its advertised size inside a NaN buffer with
GUARD words either side.

The bar (egnn_dynamics_ref.compare): per tensor err <= M * gap + floor for the whole tensor and for every row against that row's own gap.  gap:
the distance between reference (b) in float32 (CPU, one thread) and in float64 on the same inputs; floor: 8 ulp of the tensor's largest fp64
magnitude.  Nothing in the bar comes from the kernel.  M = 4 for every tensor and row, except a row of dx, M = 16: the forward is k_edge's
arithmetic, and that is egnn_dynamics_ref.ROW_MARGINS["dx"], measured and explained in tests/test_egnn_dynamics_cabi_gpu.py.

Worst M needed on an MI355X, whole tensor / worst row against its own gap (0.00: within the floor):

    case                            M     dx    gA    gB         gx    gV    gW2   gb2   gC1        gc1b  gc2   gc2b  gscale
    H = 32, Eh = 8,  e_in = 1       0.00  0.00  0.00  0.00       0.00  0.00  0.00  0.00  0.00       0.00  0.00  0.00  0.00
    H = 32, Eh = 8,  e_in = 2       0.00  0.00  0.00  0.16/0.27  0.00  0.00  0.00  0.00  0.02/0.03  1.08  0.11  3.28  0.00
    H = 64, Eh = 64, e_in = 1       0.00  0.00  0.00  0.32/0.66  0.00  0.00  0.00  0.00  0.00       0.00  0.00  0.00  0.00
    H = 64, Eh = 64, e_in = 2       0.00  0.00  0.00  0.00       0.00  0.00  0.00  0.00  0.09/0.13  0.00  0.00  0.00  0.00
    630 atoms, 3 owners per block   0.00  0.00  0.00  0.16/0.49  0.00  0.00  0.00  0.00  0.00       0.00  0.00  0.00  0.00
    9000 atoms, capped grid         0.00  0.00  0.00  0.01/0.01  0.00  0.00  0.00  0.00  0.00       0.00  0.00  0.00  0.00
    one atom                        0.00 in every tensor (dx, gx, gscale exactly 0)
    coincident atoms                0.00 in every tensor

No tensor needs a named entry.  The sums over all edges of a launch (gb2, gC1, gc1b, gc2, gc2b, gscale) are a round's plain sum added to a
compensated register pair; as one plain running sum per thread they needed 8.77 (gb2), 7.28 (gc2), 5.49 (a row of gC1) and 4.52 (gc2b) on the
first case, which was the summation and not the bar.
"""
import ctypes as C
import importlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import egnn_dynamics_ref as er  # noqa: E402
import egnn_train_ref as tr  # noqa: E402

pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
pytestmark = pytest.mark.gpu
DEV = "cuda"
G = er.GUARD
_CASES = {}
IN_ORDER = ("A", "B", "V", "W2", "b2", "C1", "c1b", "c2", "c2b", "scale", "x", "x0")
ROWWISE = ("M", "dx", "gA", "gB", "gx", "gV", "gW2", "gC1")            # the others are vectors and scalars: one row


class Guarded:
    """`n` floats at their exact size inside a NaN buffer with G guard words either side."""

    def __init__(self, n):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * G,), float("nan"), dtype=torch.float32, device=DEV)
        self.inner = self.buf[G:G + self.n]

    def ptr(self):
        return C.c_void_p(self.inner.data_ptr())

    def guards_intact(self):
        return bool(self.buf[:G].isnan().all()) and bool(self.buf[G + self.n:].isnan().all())

    def untouched(self):
        return bool(self.buf.isnan().all())


def lib():
    return native.load_ops()


def case(H, Eh, e_in, sizes, seed=7, coincident=()):
    key = (H, Eh, e_in, tuple(sizes), seed, tuple(coincident))
    if key not in _CASES:
        b = tr.make_block(H, Eh, e_in, sizes, seed, coincident)
        _CASES[key] = (b, tr.block_references(b))
    return _CASES[key]


def device_inputs(b):
    d = {k: b[k].to(DEV).contiguous() for k in IN_ORDER + ("gM", "gdx")}
    d["xsc"] = None if b["xsc"] is None else b["xsc"].to(DEV).contiguous()
    sizes = b["sizes"]
    noff = torch.zeros(len(sizes) + 1, dtype=torch.int32)
    noff[1:] = torch.cumsum(torch.tensor(sizes), 0)
    d["noff"] = noff.to(DEV)
    d["nmol"] = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes)).to(DEV)
    return d


def shapes(b):
    N, K = int(sum(b["sizes"])), 2 * (2 * b["H"] + b["Eh"] + 1)
    return dict(M=(N, 16), dx=(N, 3), gA=(N, K), gB=(N, K), gx=(N, 3), gV=(3, K), gW2=(16, K), gb2=(16,), gC1=(64, 16), gc1b=(64,), gc2=(64,),
                gc2b=(1,), gscale=(1,))


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def run_fwd(b, d, **override):
    sh = shapes(b)
    out = {k: Guarded(int(torch.Size(sh[k]).numel())) for k in ("M", "dx")}
    a = dict(N=int(sum(b["sizes"])), B=len(b["sizes"]), H=b["H"], Eh=b["Eh"], e_in=b["e_in"], xsc=d["xsc"])
    a.update(override)
    st = lib().gcdm_egnn_train_edge_fwd(*[_ptr(d[k]) for k in IN_ORDER], _ptr(a["xsc"]), _ptr(d["noff"]), _ptr(d["nmol"]), out["M"].ptr(), out["dx"].ptr(),
                                        a["N"], a["B"], a["H"], a["Eh"], a["e_in"], None)
    torch.cuda.synchronize()
    return st, out


def run_bwd(b, d, **override):
    sh = shapes(b)
    N = int(sum(b["sizes"]))
    out = {k: Guarded(int(torch.Size(sh[k]).numel())) for k in tr.GRADS}
    out["ws"] = Guarded(lib().gcdm_egnn_train_workspace_bytes(N, b["H"], b["Eh"], b["e_in"]) // 4)
    a = dict(N=N, B=len(b["sizes"]), H=b["H"], Eh=b["Eh"], e_in=b["e_in"], xsc=d["xsc"], gdx=d["gdx"])
    a.update(override)
    st = lib().gcdm_egnn_train_edge_bwd(*[_ptr(d[k]) for k in IN_ORDER], _ptr(a["xsc"]), _ptr(d["noff"]), _ptr(d["nmol"]), _ptr(d["gM"]), _ptr(a["gdx"]),
                                        out["ws"].ptr(), *[out[k].ptr() for k in tr.GRADS], a["N"], a["B"], a["H"], a["Eh"], a["e_in"], None)
    torch.cuda.synchronize()
    return st, out


def both(b, d):
    """Forward and backward on poisoned buffers -> dict of device tensors in their shapes; guards and full coverage asserted."""
    sh = shapes(b)
    st, fo = run_fwd(b, d)
    assert st == 0, lib().gcdm_egnn_train_last_error()
    before = lib().gcdm_egnn_train_launches()
    st, bo = run_bwd(b, d)
    assert st == 0, lib().gcdm_egnn_train_last_error()
    assert lib().gcdm_egnn_train_launches() - before == native.EGNN_TRAIN_BWD_LAUNCHES
    got = {}
    for k, o in list(fo.items()) + list(bo.items()):
        assert o.guards_intact(), f"{k}: a write outside the buffer"
        if k != "ws":
            assert not bool(o.inner.isnan().any()), f"{k} holds entries the kernels did not write"
            got[k] = o.inner.view(sh[k]).clone()
    return got


def judge(what, got, refs):
    r64, r32 = refs
    failures, ratios = [], {}
    for k in ("M", "dx") + tr.GRADS:
        rs = (lambda v: v) if k in ROWWISE else (lambda v: v.reshape(1, -1))
        f, r = er.compare(k, rs(got[k]), rs(r64[k]), rs(r32[k]), margins=tr.MARGINS, row_margins=tr.ROW_MARGINS, what=what + " ")
        failures += f
        ratios[k] = r
    print(f"\nMEASURED {what}: worst M needed (tensor / row) " + "  ".join(f"{k} {a:.2f}/{b:.2f}" for k, (a, b) in ratios.items()))
    for f in failures:
        print("  " + f)
    assert not failures, failures


@pytest.mark.parametrize("e_in", [1, 2])
@pytest.mark.parametrize("H,Eh", er.DIMS)
def test_forward_and_backward_per_tensor_and_row_against_fp64(H, Eh, e_in):
    b, refs = case(H, Eh, e_in, er.SIZES)
    assert sum(b["sizes"]) % 32
    got = both(b, device_inputs(b))
    judge(f"H={H} Eh={Eh} e_in={e_in}", got, refs)
    assert float(got["gx"][0].abs().max()) == 0.0, "gx of the one-atom molecule: the diagonal's cancelling pair was formed"
    if e_in == 1:
        assert float(got["gV"][1].abs().max()) == 0.0


@pytest.mark.parametrize("what,sizes,e_in", [("630 atoms, 3 owners per block", er.SIZES * 5, 2), ("9000 atoms, capped grid", [9] * 1000, 1)])
def test_owner_blocks_of_several_owners_and_the_capped_grid(what, sizes, e_in):
    """The owner block shrinks with the batch so that a small one still covers the chip: 126 atoms run one owner per block.  630 atoms run three
    (blocks that hold several molecules, molecules split over blocks); 9000 atoms run 32, in 282 blocks on 256 workgroups that loop."""
    b, refs = case(32, 8, e_in, sizes)
    judge(what, both(b, device_inputs(b)), refs)


def test_a_batch_of_one_single_atom():
    """One node, one slot (the diagonal): dx and gx are exactly zero, the weight gradients are those of the self-edge."""
    b, refs = case(32, 8, 1, [1], seed=11)
    got = both(b, device_inputs(b))
    assert float(got["dx"].abs().max()) == 0.0 and float(got["gx"].abs().max()) == 0.0 and float(got["gscale"].abs().max()) == 0.0
    assert float(got["gA"].abs().max()) > 0.0 and torch.equal(got["gA"], got["gB"])
    judge("one atom", got, refs)


def test_a_coincident_pair_of_distinct_atoms_is_finite_and_within_the_bar():
    """|d| = 0 off the diagonal: the clamp branch, g_d = 2 d (w_r . g_z1) + w scale g_t / 1e-8.  A case of its own: its rows of gx are of the size
    scale / 1e-8 and would set the floor of every other row."""
    b, refs = case(32, 8, 1, [3, 5], seed=9, coincident=((0, 1), (6, 4)))
    got = both(b, device_inputs(b))
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    assert float(got["gx"].abs().max()) > 1e5
    judge("coincident atoms", got, refs)


def test_two_backward_runs_give_identical_bits():
    b, _ = case(64, 64, 2, er.SIZES)
    d = device_inputs(b)
    first, again = both(b, d), both(b, d)
    for k in first:
        assert torch.equal(first[k].view(torch.int32), again[k].view(torch.int32)), f"{k} differs from run to run"


def test_the_forward_of_a_molecule_has_the_same_bits_alone_and_in_the_batch():
    b, _ = case(64, 64, 2, er.SIZES)
    d = device_inputs(b)
    st, full = run_fwd(b, d)
    assert st == 0
    o = 0
    for n in er.SIZES:
        rows = slice(o, o + n)
        sub = dict(b, sizes=[n], **{k: b[k][rows] for k in ("A", "B", "x", "x0", "xsc", "gM", "gdx")})
        st, alone = run_fwd(sub, device_inputs(sub))
        assert st == 0
        for k, w in (("M", 16), ("dx", 3)):
            assert torch.equal(alone[k].inner.view(n, w).view(torch.int32), full[k].inner.view(-1, w)[rows].view(torch.int32)), \
                f"molecule of {n} atoms: {k} depends on the batch"
        o += n


def test_refusals_leave_the_outputs_poisoned():
    b, _ = case(32, 8, 1, er.SIZES)
    d = device_inputs(b)
    before = lib().gcdm_egnn_train_launches()
    for override in (dict(H=48), dict(H=288), dict(Eh=0), dict(e_in=2), dict(e_in=3), dict(N=-1), dict(B=0), dict(B=1 << 30), dict(N=1 << 30),
                     dict(xsc=d["x0"])):
        for run in (run_fwd, run_bwd):
            st, out = run(b, d, **override)
            assert st == -1, override
            assert lib().gcdm_egnn_train_last_error()
            assert all(o.untouched() for o in out.values()), override
    assert lib().gcdm_egnn_train_launches() == before


def test_zero_upstream_coordinate_gradient_gives_gscale_exactly_zero():
    b, _ = case(32, 8, 2, er.SIZES)
    d = device_inputs(b)
    st, out = run_bwd(b, d, gdx=torch.zeros_like(d["gdx"]))
    assert st == 0
    assert float(out["gscale"].inner.abs().max()) == 0.0 and float(out["gc2b"].inner.abs().max()) == 0.0
    assert float(out["gA"].inner.abs().max()) > 0.0


def test_a_node_with_an_inconsistent_molecule_index_has_no_edges():
    b, _ = case(32, 8, 1, [3, 5], seed=13)
    d = device_inputs(b)
    d["nmol"] = d["nmol"].clone()
    d["nmol"][4] = 7                                                            # out of range: node 4 owns no slot list
    st, fo = run_fwd(b, d)
    assert st == 0 and float(fo["M"].inner.view(-1, 16)[4].abs().max()) == 0.0 and float(fo["dx"].inner.view(-1, 3)[4].abs().max()) == 0.0
    st, bo = run_bwd(b, d)
    assert st == 0 and all(o.guards_intact() for o in bo.values())
    K = 2 * (2 * 32 + 8 + 1)
    assert float(bo["gA"].inner.view(-1, K)[4].abs().max()) == 0.0 and float(bo["gB"].inner.view(-1, K)[4].abs().max()) == 0.0
    assert not any(bool(bo[k].inner.isnan().any()) for k in tr.GRADS)
