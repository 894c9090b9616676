"""The fused message layer for training (ops.message_layer, include/gcdm_mp_train.h) on an MI355X: forward and every gradient against
oracle.message_passing under fp64 autograd and against the operator path, masked frames, bitwise determinism, the no_grad forward, the tape's
lifetime, and the whole network with GCPNetDynamics.set_message_path("fused")."""
import importlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mp_train_ref as R
import synth
from oracle import gcdm_oracle as O

pkg = importlib.import_module("bio-diffusion_amd")
ops = pkg.ops
DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu

SIZES = [1, 2, 7, 13, 9, 3]            # ragged, n = 1 and n = 2, molecules straddling 64-edge tiles; E = 313 (not a multiple of 64)


def _layer(case, seed=3):
    d = synth.DATASET_DIMS[case]
    net = pkg.GCPNetDynamics(**pkg.default_cfgs(case))
    W = synth.make_weights(synth.dynamics_shapes(d["S"], d["V"], d["Se"], d["Ve"], d["L"], synth.dims_h_in(d)), seed=seed, scale_2d=0.5)
    net.load_state_dict(W)
    pre = "interaction_layers.0.interaction."
    mp = net.interaction_layers[0].interaction
    P = {k[len(pre):]: v for k, v in W.items() if k.startswith(pre)}
    return mp.to(DEV).train(), P, d


def _inputs(d, sizes=SIZES, seed=5):
    g = torch.Generator().manual_seed(seed)
    bi = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    N = int(bi.numel())
    row, col = O.fully_connected_edges(bi)
    E = int(row.numel())
    x = torch.randn(N, 3, generator=g)
    frames = O.localize(x, row, col)
    h = torch.randn(N, d["S"], generator=g)
    chi = torch.randn(N, d["V"], 3, generator=g)
    e = torch.rand(E, d["Se"], generator=g) * 2
    xi = torch.randn(E, d["Ve"], 3, generator=g)
    return h, chi, e, xi, frames, row, col


def _run(mp, h, chi, e, xi, frames, ei, node_mask=None, r=None):
    """forward + backward of sum(agg . r) through the module; -> (agg_s, agg_v, grads of inputs, grads of parameters)."""
    leaves = [t.to(DEV).clone().requires_grad_(True) for t in (h, chi, e, xi)]
    mp.zero_grad(set_to_none=True)
    a_s, a_v = mp((leaves[0], leaves[1]), (leaves[2], leaves[3]), ei, frames.to(DEV), node_mask=node_mask)
    if r is not None:
        ((a_s * r[0]).sum() + (a_v * r[1]).sum()).backward()
    return (a_s.detach(), a_v.detach(), [t.grad for t in leaves],
            {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in mp.named_parameters()})


def _named(a_s, a_v, gi, gp):
    """the 36 tensors of mp_train_ref.compare from _run()'s result"""
    return {"agg_s": a_s, "agg_v": a_v, **dict(zip(("dh", "dchi", "de", "dxi"), gi)), **gp}


def _rand_r(N, seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, 256, generator=g).to(DEV), torch.randn(N, 32, 3, generator=g).to(DEV)


@pytest.mark.parametrize("case", ["qm9", "geom"])
def test_fused_message_layer_matches_oracle_fp64_and_operator_path(case):
    mp, P, d = _layer(case)
    h, chi, e, xi, frames, row, col = _inputs(d)
    ei = torch.stack((row, col)).to(DEV)
    r = _rand_r(h.shape[0])
    # fp64 and fp32 autograd through the oracle: the bar is M x the oracle's own fp32-vs-fp64 gap (mp_train_ref.compare), per tensor and per row
    g = R.make_graph("fc", h.shape[0], row, col)
    inp = SimpleNamespace(h=h, chi=chi, e=e, xi=xi, frames=frames)
    rr = torch.cat((r[0].cpu(), r[1].cpu().reshape(-1, 96)), dim=1)
    ref64, ref32 = R.references(P, d, inp, g, rr)

    mp.set_path("operators")
    op_s, op_v, op_gi, op_gp = _run(mp, h, chi, e, xi, frames, ei, r=r)
    mp.set_path("fused")
    f_s, f_v, f_gi, f_gp = _run(mp, h, chi, e, xi, frames, ei, r=r)

    assert set(f_gp) == set(P)
    for k in P:
        assert f_gp[k] is not None, k
    failures, _ = R.compare(_named(f_s, f_v, f_gi, f_gp), ref64, ref32)
    assert not failures, "\n".join(failures)

    for got, op, want in ((f_s, op_s, ref64["agg_s"]), (f_v, op_v, ref64["agg_v"])):
        scale = max(1.0, want.abs().max().item())
        assert (got - op).abs().max().item() <= 1e-5 * scale

    def rel(a, b):
        return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item() / max(b.detach().abs().max().item(), 1e-12)

    for name, got, op in zip(("dh", "dchi", "de", "dxi"), f_gi, op_gi):
        assert rel(got, op) <= 1e-4, (name, rel(got, op))
    for k in P:
        assert rel(f_gp[k], op_gp[k]) <= 1e-4, (k, rel(f_gp[k], op_gp[k]))


def test_partial_node_mask_matches_operator_path():
    mp, P, d = _layer("qm9")
    h, chi, e, xi, frames, row, col = _inputs(d)
    N = h.shape[0]
    mask = torch.ones(N, dtype=torch.bool)
    mask[[0, 4, 11, N - 1]] = False
    mask = mask.to(DEV)
    ei = torch.stack((row, col)).to(DEV)
    r = _rand_r(N)
    mp.set_path("operators")
    op = _run(mp, h, chi, e, xi, frames, ei, node_mask=mask, r=r)
    mp.set_path("fused")
    fu = _run(mp, h, chi, e, xi, frames, ei, node_mask=mask, r=r)
    for a, b in ((fu[0], op[0]), (fu[1], op[1])):
        assert (a - b).abs().max().item() <= 1e-5 * max(1.0, b.abs().max().item())
    for a, b in list(zip(fu[2], op[2])) + [(fu[3][k], op[3][k]) for k in op[3]]:
        assert (a - b).abs().max().item() <= 1e-4 * max(b.abs().max().item(), 1e-12)
    # and against fp64: the oracle on frames zeroed where an end point is masked, under the measured bar
    g = R.make_graph("fc", N, row, col)
    edge_mask = mask.cpu()[row] & mask.cpu()[col]
    rr = torch.cat((r[0].cpu(), r[1].cpu().reshape(-1, 96)), dim=1)
    ref64, ref32 = R.references(P, d, SimpleNamespace(h=h, chi=chi, e=e, xi=xi, frames=frames), g, rr, edge_mask)
    failures, _ = R.compare(_named(*fu), ref64, ref32)
    assert not failures, "\n".join(failures)


def test_backward_is_bitwise_deterministic():
    mp, P, d = _layer("qm9")
    h, chi, e, xi, frames, row, col = _inputs(d, sizes=[9, 1, 17, 2, 11])
    ei = torch.stack((row, col)).to(DEV)
    r = _rand_r(h.shape[0])
    mp.set_path("fused")
    a = _run(mp, h, chi, e, xi, frames, ei, r=r)
    b = _run(mp, h, chi, e, xi, frames, ei, r=r)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def test_no_grad_forward_is_bit_identical_and_keeps_no_tape():
    mp, P, d = _layer("qm9")
    h, chi, e, xi, frames, row, col = _inputs(d)
    ei = torch.stack((row, col)).to(DEV)
    mp.set_path("fused")
    N, E = h.shape[0], row.numel()
    args = ((h.to(DEV), chi.to(DEV)), (e.to(DEV), xi.to(DEV)), ei, frames.to(DEV))
    mp(*args)                                        # graph cache and column order warm
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        n_s, n_v = mp(*args)
    torch.cuda.synchronize()
    out_bytes = 4 * N * 352
    assert torch.cuda.memory_allocated() - base <= out_bytes + 4096          # the workspace went back on return
    g_s, g_v = mp(*args)
    tape = ops.mp_workspace_bytes(1, N, E, 64, 16)
    assert tape > ops.mp_workspace_bytes(0, N, E, 64, 16)
    assert torch.cuda.memory_allocated() - base >= tape                      # the grad-recording forward keeps its tape
    assert torch.equal(n_s, g_s.detach()) and torch.equal(n_v, g_v.detach())


def test_tape_is_freed_after_backward_and_double_backward_refused():
    mp, P, d = _layer("qm9")
    h, chi, e, xi, frames, row, col = _inputs(d)
    ei = torch.stack((row, col)).to(DEV)
    mp.set_path("fused")
    r = _rand_r(h.shape[0])
    _run(mp, h, chi, e, xi, frames, ei, r=r)         # warm: gradients of the parameters exist, caches built
    torch.cuda.synchronize()
    hh = h.to(DEV).requires_grad_(True)
    rest = (chi.to(DEV), e.to(DEV), xi.to(DEV), frames.to(DEV))
    mp.zero_grad(set_to_none=False)
    base = torch.cuda.memory_allocated()
    a_s, a_v = mp((hh, rest[0]), (rest[1], rest[2]), ei, rest[3])
    loss = (a_s * r[0]).sum() + (a_v * r[1]).sum()
    loss.backward()
    del a_s, a_v, loss
    hh.grad = None
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() <= base
    a_s, _ = mp((hh, rest[0]), (rest[1], rest[2]), ei, rest[3])
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(a_s.sum(), hh, create_graph=True)


def test_fused_path_refuses_what_the_kernels_cannot_take():
    mp, P, d = _layer("qm9")
    h, chi, e, xi, frames, row, col = _inputs(d)
    mp.set_path("fused")
    perm = torch.randperm(row.numel(), generator=torch.Generator().manual_seed(0))
    ei = torch.stack((row, col))[:, perm].to(DEV)
    with pytest.raises(ValueError, match="sorted"):
        mp((h.to(DEV), chi.to(DEV)), (e.to(DEV), xi.to(DEV)), ei, frames[perm].to(DEV))
    ei = torch.stack((row, col)).to(DEV)
    with pytest.raises(TypeError, match="fp32"):
        mp((h.to(DEV).double(), chi.to(DEV).double()), (e.to(DEV).double(), xi.to(DEV).double()), ei, frames.to(DEV).double())
    with pytest.raises(ValueError):
        mp((h.to(DEV), chi.to(DEV)), (e[:, :16].to(DEV), xi.to(DEV)), ei, frames.to(DEV))


def test_whole_network_gradients_match_oracle_autograd_on_fused_message_path():
    """test_modules_gpu.py::test_module_path_gradients_match_oracle_autograd with set_message_path("fused"), same bars."""
    d = synth.DATASET_DIMS["qm9"]
    net = pkg.GCPNetDynamics(**pkg.default_cfgs("qm9"))
    W = synth.make_weights(synth.dynamics_shapes(d["S"], d["V"], d["Se"], d["Ve"], d["L"], synth.dims_h_in(d)), seed=3, scale_2d=0.5)
    net.load_state_dict(W)
    net = net.to(DEV).train()
    net.set_message_path("fused")
    assert net.message_path == "fused"
    xh, t, bi, nn_, _ = synth.make_inputs([5, 9, 3, 12], synth.dims_feat(d), seed=2)
    torch.manual_seed(0)
    r = torch.randn(len(bi), xh.shape[1])
    Wg = {k: v.clone().requires_grad_(True) for k, v in W.items()}
    lo = (O.dynamics_forward(Wg, O.OracleConfig(num_layers=d["L"]), xh, t, bi) * r).sum()
    lo.backward()
    batch = dict(batch=bi.to(DEV), mask=torch.ones(len(bi), dtype=torch.bool, device=DEV), props_context=None)
    _, out = net(batch, xh.to(DEV), t.to(DEV))
    lh = (out * r.to(DEV)).sum()
    lh.backward()
    assert abs(lh.item() - lo.item()) <= 1e-5 * max(1.0, abs(lo.item()))
    params = dict(net.named_parameters())
    for k, v in Wg.items():
        assert params[k].grad is not None, k
        rel = (params[k].grad.cpu() - v.grad).abs().max().item() / max(v.grad.abs().max().item(), 1e-12)
        assert rel <= 1e-4, (k, rel)


@pytest.mark.parametrize("case", ["qm9", "geom"])
def test_training_step_on_fused_message_path_matches_reference_autograd(case, golden_dir):
    """test_modules_gpu.py::test_training_loss_and_gradients_match_reference_autograd with set_message_path("fused"), same bars."""
    g = np.load(os.path.join(golden_dir, f"train_full_{case}.npz"), allow_pickle=False)
    d = synth.DATASET_DIMS[case]
    cls = pkg.GEOMMoleculeGenerationDDPM if case == "geom" else pkg.QM9MoleculeGenerationDDPM
    model = cls(**pkg.default_cfgs(case))
    shapes = synth.dynamics_shapes(d["S"], d["V"], d["Se"], d["Ve"], d["L"], synth.dims_h_in(d))
    model.ddpm.dynamics_network.load_state_dict(synth.make_weights(shapes, seed=int(g["weight_seed"]), scale_2d=float(g["weight_scale"])))
    model = model.to(DEV).train()
    model.ddpm.dynamics_network.set_message_path("fused")
    nn_ = torch.tensor(g["num_nodes"])
    bi = torch.repeat_interleave(torch.arange(len(nn_)), nn_).to(DEV)
    N, F = int(nn_.sum()), synth.dims_feat(d)
    tape = O.TapeNoise(int(g["noise_seed"]))
    noise = [torch.cat((tape(N, 3), tape(N, F)), dim=-1)]
    t_int = torch.tensor(g["t_int"]).view(-1, 1)
    batch = pkg.config.AttrDict(x=torch.tensor(g["x"]).to(DEV), one_hot=torch.tensor(g["one_hot"]).to(DEV), charges=torch.tensor(g["charges"]).to(DEV),
                                batch=bi, mask=torch.ones(N, dtype=torch.bool, device=DEV), props_context=None)
    model.zero_grad()
    loss = model.training_step(batch, t_int=t_int, noise=noise)["loss"]
    l32, l64 = float(g["loss_32"]), float(g["loss_64"])
    assert abs(loss.item() - l64) <= 4 * abs(l32 - l64) + 1e-4 * abs(l64), (loss.item(), l64)
    loss.backward()
    params = dict(model.ddpm.dynamics_network.named_parameters())
    for i, k in enumerate(shapes):
        gr = params[k].grad
        assert gr is not None and torch.isfinite(gr).all(), k
        for stat, fn in (("grad_norm", lambda v: float(v.double().norm())), ("grad_absmax", lambda v: float(v.double().abs().max()))):
            w32, w64 = float(g[f"{stat}_32"][i]), float(g[f"{stat}_64"][i])
            assert abs(fn(gr) - w64) <= 4 * abs(w32 - w64) + 1e-4 * w64, (k, stat, fn(gr), w64)
    for k in [k[len("grad_64::"):] for k in g.files if k.startswith("grad_64::")]:
        w32, w64 = torch.tensor(g[f"grad_32::{k}"]).double(), torch.tensor(g[f"grad_64::{k}"])
        bar = 4 * (w32 - w64).abs().max().item() + 1e-4 * w64.abs().max().item()
        assert (params[k].grad.double().cpu() - w64).abs().max().item() <= bar, k
