"""gcdm_egnn_dyn_pack / gcdm_egnn_dyn_layer (include/gcdm_egnn_dynamics.h) called directly through the C ABI on an MI355X, against the fp64
restatement (tests/egnn_dynamics_ref.py), per layer and per atom row.

Shapes: (H, Eh) = (32, 8) -- 2 D = 146, so the K of the edge GEMM is padded to 160 -- and (64, 64), two layers, e_in 1 and 2, molecules of
1, 2, 3, 17, 33 and 70 atoms in one batch (egnn_dynamics_ref.SIZES): a one-slot receiver, receivers whose slot lists cross a 16-edge MFMA tile, a
wave's 64 edges and a round of 256, workgroups (32 receivers) that hold several molecules and molecules that span several workgroups.

Harness: every buffer the library writes (packed weights, workspace, h_out, x_out and the three debug outputs) sits at exactly its advertised
size inside a larger buffer, everything NaN including GUARD words either side.  The layers are chained on the device as a forward chains them.

The bar (egnn_dynamics_ref.compare, the convention of tests/test_mp_train_cabi_gpu.py): per tensor err <= M * gap + floor for the whole tensor
and for every row against that row's own gap.  gap: the distance between the restatement in float32 (CPU, one thread) and in float64 on the same
inputs; floor: 8 ulp of the tensor's largest fp64 magnitude.  Nothing in the bar comes from the kernel.  The tensors: per layer the receiver
sums m [N, 16] and dx [N, 3], the LayerNorm output ln [N, H] and the layer's outputs h [N, H], x [N, 3].  M = 4 for every whole tensor
(egnn_dynamics_ref.MARGINS is empty); for a row against its own gap M = 4 too, except the two coordinate tensors dx and x, M = 16
(egnn_dynamics_ref.ROW_MARGINS), and this table is the only rationale.

Worst M needed on an MI355X, whole tensor / worst row against its own gap (0.00: within the floor), layer 0 then layer 1:

    configuration              m            dx                       ln      h                        x
    H = 32, Eh = 8,  e_in = 1  0.00, 0.12/0.15   0.00, 0.27/0.51     0.00    0.00, 0.46/0.71          0.00, 0.84/7.45
    H = 32, Eh = 8,  e_in = 2  0.00, 0.00        0.00, 0.06/0.06     0.00    0.00                     0.00, 0.65/0.67
    H = 64, Eh = 64, e_in = 1  0.00, 0.00        0.00, 0.00          0.00    0.00                     0.00, 0.19/0.24
    H = 64, Eh = 64, e_in = 2  0.00, 0.00        2.41/4.42, 0.98/2.15   0.00    0.00                  2.82/5.00, 1.22/2.76
    coincident atoms           0.00              0.00, 0.30/1.73     0.00    0.00                     0.00
    one atom                   0.00              0.00 (dx exactly 0) 0.00    0.00                     0.00

The exception.  Every whole tensor is inside M = 4 (worst 2.82).  What exceeds 4 is a ROW of dx or x against that row's own fp32 gap: 4.42,
5.00 and 7.45.  A row of these tensors is three numbers, each a sum of up to 70 terms w_ij (x_j - x_i) / |x_j - x_i| * scale that point in all
directions and cancel; the row's gap is the largest of three draws of the restatement's own fp32 rounding and comes close to zero by chance,
while the kernel's w_ij carries the rounding of a 2 D-term pre-activation formed as A_i + B_j + r0 u + r w_r from separately rounded parts
(the column split of DESIGN.md 3.10, the same cause as classifier_ref.MARGINS["hot"]) through tanh(coors_mlp(.)).  The wide tensors m, ln and
h, whose rows are maxima over 16 / H numbers, stay at M = 4 per row.  Summation order, not a wrong term: the same rows are bit-identical
from run to run and between a molecule alone and inside the batch (the last test), and a wrong or missing slot moves dx by O(scale) = 0.5,
five orders of magnitude above the bar.
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

pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
pytestmark = pytest.mark.gpu
DEV = "cuda"
G = er.GUARD
_CASES = {}


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


def cfg_of(H, Eh, e_in, L=2):
    return dict(H=H, Eh=Eh, L=L, num_atom_types=5, include_charges=True, condition_on_time=True, num_context=0, self_condition=e_in == 2)


def dims(cfg):
    return cfg["H"], cfg["Eh"], 2 if cfg["self_condition"] else 1, cfg["L"]


def pack(W, cfg):
    H, Eh, e_in, L = dims(cfg)
    ts = [t.to(DEV).contiguous() for t in er.ordered_tensors(W, L)]
    packed = Guarded(lib().gcdm_egnn_dyn_workspace_bytes(1, 0, H, Eh, e_in, L) // 4)
    table = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    st = lib().gcdm_egnn_dyn_pack(table, len(ts), H, Eh, e_in, L, packed.ptr(), None)
    torch.cuda.synchronize()
    assert st == 0, lib().gcdm_egnn_dyn_last_error()
    assert packed.guards_intact() and not bool(packed.inner.isnan().any())
    return packed


def topology(sizes):
    noff = torch.zeros(len(sizes) + 1, dtype=torch.int32)
    noff[1:] = torch.cumsum(torch.tensor(sizes), 0)
    nmol = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes))
    return noff.to(DEV), nmol.to(DEV)


def run_layer(l, packed, cfg, h, x, x0, xsc, sizes, **override):
    """One gcdm_egnn_dyn_layer call on NaN-poisoned outputs and workspace -> (status, dict of Guarded outputs)."""
    H, Eh, e_in, L = dims(cfg)
    N, B = int(sum(sizes)), len(sizes)
    noff, nmol = topology(sizes)
    out = dict(h=Guarded(N * H), x=Guarded(N * 3), m=Guarded(N * 16), dx=Guarded(N * 3), ln=Guarded(N * H),
               ws=Guarded(lib().gcdm_egnn_dyn_workspace_bytes(0, N, H, Eh, e_in, L) // 4))
    a = dict(layer=l, N=N, B=B, H=H, Eh=Eh, e_in=e_in, L=L)
    a.update(override)
    st = lib().gcdm_egnn_dyn_layer(a["layer"], C.c_void_p(h.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(x0.data_ptr()),
                                   None if xsc is None else C.c_void_p(xsc.data_ptr()), C.c_void_p(noff.data_ptr()), C.c_void_p(nmol.data_ptr()),
                                   packed.ptr(), out["ws"].ptr(), out["h"].ptr(), out["x"].ptr(), out["m"].ptr(), out["dx"].ptr(), out["ln"].ptr(),
                                   a["N"], a["B"], a["H"], a["Eh"], a["e_in"], a["L"], None)
    torch.cuda.synchronize()
    return st, out


def case(H, Eh, e_in, sizes, seed=7):
    """(cfg, W, references, device inputs of layer 0) of a configuration, computed once and shared."""
    key = (H, Eh, e_in, tuple(sizes), seed)
    if key not in _CASES:
        cfg = cfg_of(H, Eh, e_in)
        W = er.make_weights(cfg, seed=seed)
        xh, t, bi, ctx, sc = er.make_inputs(cfg, sizes, seed=seed + 1)
        _CASES[key] = (cfg, W, er.references(W, cfg, xh, t, bi, None, ctx, sc), sc)
    return _CASES[key]


def chain(cfg, W, ref, sc, sizes, packed=None):
    """The layers on the device, fed with the fp32 rounding of the restatement's layer-0 inputs and chained.  -> per layer dict of CPU tensors."""
    packed = pack(W, cfg) if packed is None else packed
    p = ref.probe64
    h, x = p["h_in"].float().to(DEV).contiguous(), p["x_in"].float().to(DEV).contiguous()
    x0 = p["x_init"].float().to(DEV).contiguous()
    xsc = None if sc is None else sc[:, :3].float().to(DEV).contiguous()
    N, H = h.shape
    layers = []
    for l in range(cfg["L"]):
        st, out = run_layer(l, packed, cfg, h, x, x0, xsc, sizes)
        assert st == 0, lib().gcdm_egnn_dyn_last_error()
        assert all(o.guards_intact() for o in out.values()), "a write outside a buffer"
        got = dict(h=out["h"].inner.view(N, H), x=out["x"].inner.view(N, 3), m=out["m"].inner.view(N, 16), dx=out["dx"].inner.view(N, 3),
                   ln=out["ln"].inner.view(N, H))
        for k, v in got.items():
            assert not bool(v.isnan().any()), f"layer {l}: {k} holds entries the kernels did not write"
        layers.append({k: v.clone() for k, v in got.items()})
        h, x = layers[-1]["h"], layers[-1]["x"]
    return layers


def judge(what, layers, ref):
    failures, ratios = [], {}
    for l, got in enumerate(layers):
        for k in ("m", "dx", "ln", "h", "x"):
            f, r = er.compare(k, got[k], ref.probe64[k][l], ref.probe32[k][l], what=f"{what} layer {l} ")
            failures += f
            ratios[f"{k}{l}"] = r
    print(f"\nMEASURED {what}: worst M needed (tensor / row) " + "  ".join(f"{k} {a:.2f}/{b:.2f}" for k, (a, b) in ratios.items()))
    for f in failures:
        print("  " + f)
    assert not failures, failures


@pytest.mark.parametrize("e_in", [1, 2])
@pytest.mark.parametrize("H,Eh", er.DIMS)
def test_every_layer_per_row_against_fp64(H, Eh, e_in):
    cfg, W, ref, sc = case(H, Eh, e_in, er.SIZES)
    judge(f"H={H} Eh={Eh} e_in={e_in}", chain(cfg, W, ref, sc, er.SIZES), ref)


def test_coincident_atoms_contribute_zero_not_nan():
    """|rel| = 0 off the diagonal too: two atoms of a molecule at one point.  The clamp gives 0 / 1e-8 = 0, not NaN."""
    sizes = [3, 5]
    cfg = cfg_of(32, 8, 1)
    W = er.make_weights(cfg, seed=9)
    xh, t, bi, ctx, sc = er.make_inputs(cfg, sizes, seed=10)
    xh[1, :3] = xh[0, :3]
    xh[4, :3] = xh[6, :3]
    ref = er.references(W, cfg, xh, t, bi, None, ctx, sc)
    layers = chain(cfg, W, ref, sc, sizes)
    for got in layers:
        assert bool(torch.isfinite(got["dx"]).all()) and bool(torch.isfinite(got["x"]).all())
    judge("coincident atoms", layers, ref)


def test_a_batch_of_one_single_atom():
    """One node, one slot (the diagonal): m is the self-message, dx is exactly zero, x is unchanged."""
    sizes = [1]
    cfg = cfg_of(32, 8, 1)
    W = er.make_weights(cfg, seed=11)
    xh, t, bi, ctx, sc = er.make_inputs(cfg, sizes, seed=12)
    ref = er.references(W, cfg, xh, t, bi, None, ctx, sc)
    layers = chain(cfg, W, ref, sc, sizes)
    for got in layers:
        assert float(got["dx"].abs().max()) == 0.0 and float(got["m"].abs().max()) > 0.0
    assert torch.equal(layers[-1]["x"].cpu(), ref.probe64["x_in"].float())
    judge("one atom", layers, ref)


def test_refusals_leave_the_outputs_poisoned():
    cfg, W, ref, sc = case(32, 8, 1, er.SIZES)
    packed = pack(W, cfg)
    p = ref.probe64
    h, x, x0 = (p[k].float().to(DEV).contiguous() for k in ("h_in", "x_in", "x_init"))
    before = lib().gcdm_egnn_dyn_launches()
    for override in (dict(H=48), dict(H=288), dict(Eh=0), dict(e_in=2), dict(e_in=3), dict(layer=2), dict(layer=-1), dict(L=0), dict(N=-1), dict(B=0),
                     dict(B=1 << 30), dict(N=1 << 30)):
        st, out = run_layer(0, packed, cfg, h, x, x0, None, er.SIZES, **override)
        assert st == -1, override
        assert lib().gcdm_egnn_dyn_last_error()
        assert all(o.untouched() for o in out.values()), override
    st, out = run_layer(0, packed, cfg, h, x, x0, x0, er.SIZES)                    # xsc with e_in = 1
    assert st == -1 and all(o.untouched() for o in out.values())
    assert lib().gcdm_egnn_dyn_launches() == before
    st, out = run_layer(0, packed, cfg, h, x, x0, None, er.SIZES)
    assert st == 0 and lib().gcdm_egnn_dyn_launches() == before + 1


@pytest.mark.parametrize("H,Eh", er.DIMS)
def test_a_molecule_has_the_same_bits_alone_in_the_batch_and_from_run_to_run(H, Eh):
    cfg, W, ref, sc = case(H, Eh, 2, er.SIZES)
    packed = pack(W, cfg)
    first = chain(cfg, W, ref, sc, er.SIZES, packed)
    again = chain(cfg, W, ref, sc, er.SIZES, packed)
    for a, b in zip(first, again):
        for k in a:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{k} differs from run to run"
    o = 0
    for n in er.SIZES:                                       # each molecule alone: its rows of the batch's inputs, layer by layer
        rows = slice(o, o + n)
        sub = type(ref)(probe64={k: (v[rows] if not isinstance(v, list) else [u[rows] for u in v]) for k, v in ref.probe64.items()})
        alone = chain(cfg, W, sub, None if sc is None else sc[rows], [n], packed)
        # layer 0 sees the same inputs in both runs; layer 1 sees layer 0's outputs, which must already be the same bits
        for l, (a, b) in enumerate(zip(alone, first)):
            for k in a:
                assert torch.equal(a[k].view(torch.int32), b[k][rows].view(torch.int32)), f"molecule of {n} atoms: {k} of layer {l} depends on the batch"
        o += n
