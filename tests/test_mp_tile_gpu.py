"""The "tiled" message path (ops.message_layer(path="tiled"), include/gcdm_mp_tile.h) through the modules on an MI355X: one GCPMessagePassing
against the operator path and fp64 on a ragged masked batch, the whole training step against the reference's recorded autograd, and the
tape's lifetime -- at the bars tests/test_mp_train_gpu.py holds the "fused" path to."""
import importlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mp_train_ref as R
import synth
import test_mp_train_gpu as F          # its layer, inputs and runner
from oracle import gcdm_oracle as O

pkg = importlib.import_module("bio-diffusion_amd")
DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu


def test_tiled_message_layer_matches_operator_path_and_fp64_on_a_ragged_masked_batch():
    mp, P, d = F._layer("qm9")
    h, chi, e, xi, frames, row, col = F._inputs(d)          # [1, 2, 7, 13, 9, 3]: E = 313
    N = h.shape[0]
    mask = torch.ones(N, dtype=torch.bool)
    mask[[0, 4, 11, N - 1]] = False
    mask = mask.to(DEV)
    ei = torch.stack((row, col)).to(DEV)
    r = F._rand_r(N)
    mp.set_path("operators")
    op = F._run(mp, h, chi, e, xi, frames, ei, node_mask=mask, r=r)
    mp.set_path("tiled")
    assert mp.path == "tiled"
    ti = F._run(mp, h, chi, e, xi, frames, ei, node_mask=mask, r=r)
    assert set(ti[3]) == set(P) and all(v is not None for v in ti[3].values())
    for a, b in ((ti[0], op[0]), (ti[1], op[1])):
        assert (a - b).abs().max().item() <= 1e-5 * max(1.0, b.abs().max().item())
    for a, b in list(zip(ti[2], op[2])) + [(ti[3][k], op[3][k]) for k in op[3]]:
        assert (a - b).abs().max().item() <= 1e-4 * max(b.abs().max().item(), 1e-12)
    # and against fp64: the oracle on frames zeroed where an end point is masked, under the measured bar
    g = R.make_graph("fc", N, row, col)
    edge_mask = mask.cpu()[row] & mask.cpu()[col]
    rr = torch.cat((r[0].cpu(), r[1].cpu().reshape(-1, 96)), dim=1)
    ref64, ref32 = R.references(P, d, SimpleNamespace(h=h, chi=chi, e=e, xi=xi, frames=frames), g, rr, edge_mask)
    failures, _ = R.compare(F._named(*ti), ref64, ref32)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("node_path", ["operators", "fused"])
def test_training_step_on_tiled_message_path_matches_reference_autograd(node_path, golden_dir):
    """test_mp_train_gpu.py::test_training_step_on_fused_message_path_matches_reference_autograd with set_message_path("tiled"), same bars; on
    its own and next to set_node_path("fused")."""
    case = "qm9"
    g = np.load(os.path.join(golden_dir, f"train_full_{case}.npz"), allow_pickle=False)
    d = synth.DATASET_DIMS[case]
    model = pkg.QM9MoleculeGenerationDDPM(**pkg.default_cfgs(case))
    shapes = synth.dynamics_shapes(d["S"], d["V"], d["Se"], d["Ve"], d["L"], synth.dims_h_in(d))
    net = model.ddpm.dynamics_network
    net.load_state_dict(synth.make_weights(shapes, seed=int(g["weight_seed"]), scale_2d=float(g["weight_scale"])))
    model = model.to(DEV).train()
    net.set_message_path("tiled")
    net.set_node_path(node_path)
    assert net.message_path == "tiled" and net.node_path == node_path
    nn_ = torch.tensor(g["num_nodes"])
    bi = torch.repeat_interleave(torch.arange(len(nn_)), nn_).to(DEV)
    N, Fd = int(nn_.sum()), synth.dims_feat(d)
    tape = O.TapeNoise(int(g["noise_seed"]))
    noise = [torch.cat((tape(N, 3), tape(N, Fd)), dim=-1)]
    t_int = torch.tensor(g["t_int"]).view(-1, 1)
    batch = pkg.config.AttrDict(x=torch.tensor(g["x"]).to(DEV), one_hot=torch.tensor(g["one_hot"]).to(DEV), charges=torch.tensor(g["charges"]).to(DEV),
                                batch=bi, mask=torch.ones(N, dtype=torch.bool, device=DEV), props_context=None)
    model.zero_grad()
    loss = model.training_step(batch, t_int=t_int, noise=noise)["loss"]
    l32, l64 = float(g["loss_32"]), float(g["loss_64"])
    assert abs(loss.item() - l64) <= 4 * abs(l32 - l64) + 1e-4 * abs(l64), (loss.item(), l64)
    loss.backward()
    params = dict(net.named_parameters())
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


def test_second_backward_through_a_freed_tape_raises_and_double_backward_is_refused():
    mp, P, d = F._layer("qm9")
    h, chi, e, xi, frames, row, col = F._inputs(d)
    ei = torch.stack((row, col)).to(DEV)
    mp.set_path("tiled")
    hh = h.to(DEV).requires_grad_(True)
    rest = (chi.to(DEV), e.to(DEV), xi.to(DEV), frames.to(DEV))
    a_s, _ = mp((hh, rest[0]), (rest[1], rest[2]), ei, rest[3])
    loss = a_s.sum()
    loss.backward(retain_graph=True)          # the node drops its tape whatever autograd retains
    with pytest.raises(RuntimeError, match="tape of this forward is gone"):
        loss.backward()
    a_s, _ = mp((hh, rest[0]), (rest[1], rest[2]), ei, rest[3])
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(a_s.sum(), hh, create_graph=True)
