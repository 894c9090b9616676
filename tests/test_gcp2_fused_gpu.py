"""GCPNetDynamics.set_node_path("fused") and ops.gcp2_fused on an MI355X: the whole network with every stand-alone GCP2 on the fused kernels
(with and without the fused message path) against the operator path of the same network and against the reference's training fixture; the
autograd node's contracts (tape, frozen weights, double backward, non-contiguous inputs, refusals)."""
import importlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gcp2_ref as R  # noqa: E402
import synth  # noqa: E402
from oracle import gcdm_oracle as O  # noqa: E402

pkg = importlib.import_module("bio-diffusion_amd")
ops = pkg.ops
GCP2 = pkg.gcp_modules.GCP2
pytestmark = pytest.mark.gpu
DEV = "cuda"


def _net(case="qm9"):
    d = synth.DATASET_DIMS[case]
    net = pkg.GCPNetDynamics(**pkg.default_cfgs(case))
    W = synth.make_weights(synth.dynamics_shapes(d["S"], d["V"], d["Se"], d["Ve"], d["L"], synth.dims_h_in(d)), seed=3, scale_2d=0.5)
    net.load_state_dict(W)
    return net.to(DEV).eval(), W, d


@pytest.mark.parametrize("message_path", ["operators", "fused"])
@pytest.mark.parametrize("case", ["qm9", "geom"])
def test_forward_modules_matches_the_operator_path(case, message_path):
    """A 3-molecule ragged batch with one masked node in the middle molecule.  Bar, as the variant tests': 4 |ref32 - ref64| + 1e-5 max|out|,
    ref32 / ref64 the CPU oracle's fp32 / fp64 outputs on the same inputs."""
    net, W, d = _net(case)
    xh, t, bi, nn_, _ = synth.make_inputs([7, 19, 4], synth.dims_feat(d), seed=2)
    mask = torch.ones(len(bi), dtype=torch.bool)
    mask[10] = False
    ocfg = O.OracleConfig(num_atom_types=d["num_atom_types"], include_charges=d["include_charges"], num_layers=d["L"])
    r32 = O.dynamics_forward(W, ocfg, xh, t, bi, mask).double()
    r64 = O.dynamics_forward({k: v.double() for k, v in W.items()}, ocfg, xh.double(), t.double(), bi, mask)
    bound = 4.0 * (r32 - r64).abs().max().item() + 1e-5 * r64.abs().max().item()
    batch = dict(batch=bi.to(DEV), mask=mask.to(DEV), props_context=None)
    net.set_message_path(message_path)
    with torch.no_grad():
        out_o = net.forward_modules(batch, xh.to(DEV), t.to(DEV))
        net.set_node_path("fused")
        assert net.node_path == "fused" and net.message_path == message_path
        out_f = net.forward_modules(batch, xh.to(DEV), t.to(DEV))
    err = (out_f - out_o).abs().max().item()
    print(f"\nMEASURED {case} message={message_path}: |fused - operators| = {err:.3e}, bound {bound:.3e}")
    assert torch.isfinite(out_f).all() and err <= bound
    assert (out_f.cpu().double() - r64).abs().max().item() <= bound + (out_o.cpu().double() - r64).abs().max().item()


@pytest.mark.parametrize("with_message", [False, True])
def test_training_step_matches_reference_autograd(with_message, golden_dir, monkeypatch):
    """The loss and every parameter gradient against tests/golden/train_full_qm9.npz under the bars of the existing training test of that
    fixture: that test's own body runs, with the network's path switch widened to the node path (the bars are read there, not restated)."""
    import test_mp_train_gpu as T
    orig = pkg.GCPNetDynamics.set_message_path
    seen = []

    def both(self, path):
        orig(self, path if with_message else "operators")
        self.set_node_path("fused")
        seen.append((self.message_path, self.node_path))

    monkeypatch.setattr(pkg.GCPNetDynamics, "set_message_path", both)
    T.test_training_step_on_fused_message_path_matches_reference_autograd("qm9", golden_dir)
    assert seen == [("fused" if with_message else "operators", "fused")]


@pytest.mark.parametrize("variant,word", [("frame_gate", "frame_gate"), ("no_vector_gate", "vector_gate"), ("ablate_frames", "ablate_frame_updates"),
                                          ("gcp1", "not GCP2"), ("relu_widths", "nonlinearities"), ("gcp1_sigma_gate", "not GCP2")])
def test_why_not_fused_names_the_reason_per_variant(variant, word):
    net = pkg.GCPNetDynamics(**synth.apply_variant(pkg.default_cfgs("qm9"), variant))
    with pytest.raises(NotImplementedError, match=word):
        net.set_node_path("fused")
    assert net.node_path == "operators"


def _module(inst="pos"):
    d = R.instances("qm9")[inst]
    m = GCP2((d["SI"], d["VI"]), (d["SO"], d["VO"]), bottleneck=4, nonlinearities=("silu", "silu"))
    assert m.hidden_dim == d["H"]
    W = R.make_weights(d)
    m.load_state_dict(W)
    return m.to(DEV), W, d


def _call(m, s, v, F):
    M = s.shape[0]
    ei = torch.stack((torch.arange(M), torch.arange(M))).to(DEV)          # edge rows: the frame of row m is F[m]
    return m((s, v), ei, F, node_inputs=False)


def test_module_matches_fp64_autograd_and_the_operator_path():
    m, W, d = _module()
    M = 131
    s, v, F, rs, rv = R.make_rows(d, M, seed=3)
    ref64, ref32 = R.references(W, d, s, v, F, rs, rv)
    got = {}
    for path in ("operators", "fused"):
        m.set_path(path)
        m.zero_grad()
        sd, vd = s.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
        so, vo = _call(m, sd, vd, F.to(DEV))
        ((so * rs.to(DEV)).sum() + (vo * rv.to(DEV)).sum()).backward()
        g = {"s_out": so, "v_out": vo, "ds": sd.grad, "dv": vd.grad}
        g.update({k: p.grad for k, p in m.named_parameters()})
        got[path] = {k: t.detach().cpu() for k, t in g.items()}
    failures, ratios = R.compare(got["fused"], ref64, ref32, what="module pos: ")
    print("\nMEASURED module pos: worst factor %.3g (%s)" % R.worst_ratio(ratios)[::-1])
    assert not failures, "\n".join(failures)
    for k in got["fused"]:
        scale = max(1.0, ref64[k].abs().max().item())
        assert (got["fused"][k] - got["operators"][k]).abs().max().item() <= 1e-4 * scale, k


def test_tape_only_when_recording_and_freed_by_the_backward():
    m, W, d = _module()
    m.set_path("fused")
    M = 200
    s, v, F, rs, rv = [x.to(DEV) for x in R.make_rows(d, M, seed=4)]
    _call(m, s, v, F)
    torch.cuda.synchronize()
    cd = pkg._native.Gcp2Dims(d["SI"], d["VI"], d["SO"], d["VO"], d["H"], d["ff"], d["a0"], d["a1"])
    tape = ops.gcp2_workspace_bytes(1, M, cd)
    assert tape > ops.gcp2_workspace_bytes(0, M, cd)
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        n_s, n_v = _call(m, s, v, F)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() - base <= 4 * M * (d["SO"] + 3 * d["VO"]) + 4096          # the workspace went back on return
    del n_s, n_v
    g_s, g_v = _call(m, s, v, F)
    assert torch.cuda.memory_allocated() - base >= tape                                            # the recording forward keeps its tape
    loss = (g_s * rs).sum() + (g_v * rv).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="tape"):
        loss.backward()                                                                            # a second backward: the tape is gone
    del g_s, g_v, loss
    m.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() <= base


def test_double_backward_raises():
    m, W, d = _module()
    m.set_path("fused")
    s, v, F, rs, rv = [x.to(DEV) for x in R.make_rows(d, 9, seed=4)]
    s.requires_grad_(True)
    so, _ = _call(m, s, v, F)
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(so.sum(), s, create_graph=True)


def test_frozen_weights_and_inputs_get_no_gradient():
    m, W, d = _module()
    m.set_path("fused")
    s, v, F, rs, rv = [x.to(DEV) for x in R.make_rows(d, 70, seed=4)]
    frozen = ("vector_down.weight", "scalar_out.bias", "vector_out_scale.weight")
    for k, p in m.named_parameters():
        p.requires_grad_(k not in frozen)
    v.requires_grad_(True)
    so, vo = _call(m, s, v, F)
    ((so * rs).sum() + (vo * rv).sum()).backward()
    for k, p in m.named_parameters():
        assert (p.grad is None) == (k in frozen), k
    assert s.grad is None and v.grad is not None and torch.isfinite(v.grad).all()


def test_non_contiguous_inputs_and_refusals():
    m, W, d = _module()
    m.set_path("fused")
    M = 67
    s, v, F, rs, rv = [x.to(DEV) for x in R.make_rows(d, M, seed=4)]
    with torch.no_grad():
        want_s, want_v = _call(m, s, v, F)
        s_nc = torch.empty((d["SI"], M), device=DEV).t()
        s_nc.copy_(s)
        v_nc = torch.empty((M, 3, d["VI"]), device=DEV).transpose(1, 2)
        v_nc.copy_(v)
        assert not s_nc.is_contiguous() and not v_nc.is_contiguous()
        got_s, got_v = _call(m, s_nc, v_nc, F)
        assert torch.equal(got_s, want_s) and torch.equal(got_v, want_v)
        with pytest.raises(TypeError, match="fp32"):
            _call(m, s.double(), v.double(), F.double())
        with pytest.raises(ValueError):
            _call(m, s[:, :-1], v, F)
        with pytest.raises(ValueError):
            _call(m, s, v, F[:-1])
        with pytest.raises(RuntimeError):
            ops.gcp2_fused(s.cpu(), v.cpu(), F.cpu(), [w.cpu() for w in m.fused_weights()], d["SO"], d["VO"], d["H"], act_scalar="silu", act_vector="silu")
        with pytest.raises(ValueError, match="nonlinearity"):
            ops.gcp2_fused(s, v, F, m.fused_weights(), d["SO"], d["VO"], d["H"], act_scalar="relu")
