"""ops.matrix_mode("bf16x6") on an MI355X through the Python layer: a whole training step against the reference's recorded autograd, on the
operator path and on the fused message + fused node path, and the module forward on a ragged masked batch against fp32 mode.

The training bars are not restated here: the body of the existing training test of tests/golden/train_full_qm9.npz runs
(tests/test_mp_train_gpu.py), inside the mode, with the network's path switch widened as tests/test_gcp2_fused_gpu.py widens it."""
import importlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import synth  # noqa: E402
from oracle import gcdm_oracle as O  # noqa: E402

pkg = importlib.import_module("bio-diffusion_amd")
ops = pkg.ops
pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def back_to_f32():
    """Whatever a test does to the switch, the process leaves it in fp32 mode."""
    assert ops.get_matrix_mode() == "f32"
    try:
        yield
    finally:
        ops.set_matrix_mode("f32")


@pytest.mark.parametrize("paths", [("operators", "operators"), ("fused", "fused")], ids=["operators", "fused_message_fused_node"])
def test_training_step_matches_reference_autograd_in_bf16x6(paths, golden_dir, monkeypatch):
    """Loss and every parameter gradient of a training step in bf16x6 mode -- forward and backward inside the block, so the gradients run in
    it too -- under the bars of the fp32-mode training test."""
    import test_mp_train_gpu as T
    orig = pkg.GCPNetDynamics.set_message_path
    seen = []

    def both(self, path):
        orig(self, paths[0])
        self.set_node_path(paths[1])
        seen.append((self.message_path, self.node_path, ops.get_matrix_mode()))

    monkeypatch.setattr(pkg.GCPNetDynamics, "set_message_path", both)
    with ops.matrix_mode("bf16x6"):
        T.test_training_step_on_fused_message_path_matches_reference_autograd("qm9", golden_dir)
        assert ops.get_matrix_mode() == "bf16x6"
    assert seen == [(paths[0], paths[1], "bf16x6")]
    assert ops.get_matrix_mode() == "f32"


@pytest.mark.parametrize("paths", [("operators", "operators"), ("fused", "fused")], ids=["operators", "fused_message_fused_node"])
def test_ragged_masked_forward_against_fp32_mode(paths):
    """Three molecules [7, 19, 4], one masked node in the middle one: bf16x6 against fp32 mode under 4 |ref32 - ref64| + 1e-5 max|out| of the
    existing path tests (ref32 / ref64: the CPU oracle in fp32 / fp64)."""
    d = synth.DATASET_DIMS["qm9"]
    net = pkg.GCPNetDynamics(**pkg.default_cfgs("qm9"))
    W = synth.make_weights(synth.dynamics_shapes(d["S"], d["V"], d["Se"], d["Ve"], d["L"], synth.dims_h_in(d)), seed=3, scale_2d=0.5)
    net.load_state_dict(W)
    net = net.to(DEV).eval()
    xh, t, bi, _, _ = synth.make_inputs([7, 19, 4], synth.dims_feat(d), seed=2)
    mask = torch.ones(len(bi), dtype=torch.bool)
    mask[10] = False
    ocfg = O.OracleConfig(num_atom_types=d["num_atom_types"], include_charges=d["include_charges"], num_layers=d["L"])
    r32 = O.dynamics_forward(W, ocfg, xh, t, bi, mask).double()
    r64 = O.dynamics_forward({k: v.double() for k, v in W.items()}, ocfg, xh.double(), t.double(), bi, mask)
    bound = 4.0 * (r32 - r64).abs().max().item() + 1e-5 * r64.abs().max().item()
    batch = dict(batch=bi.to(DEV), mask=mask.to(DEV), props_context=None)
    net.set_message_path(paths[0])
    net.set_node_path(paths[1])
    with torch.no_grad():
        out32 = net.forward_modules(batch, xh.to(DEV), t.to(DEV))
        with ops.matrix_mode("bf16x6"):
            out6 = net.forward_modules(batch, xh.to(DEV), t.to(DEV))
        again = net.forward_modules(batch, xh.to(DEV), t.to(DEV))
    assert ops.get_matrix_mode() == "f32"
    assert torch.equal(out32, again), "fp32 mode gives other bits after a bf16x6 block"
    err = (out6 - out32).abs().max().item()
    print(f"\nMEASURED message={paths[0]} node={paths[1]}: |bf16x6 - fp32 mode| = {err:.3e}, bound {bound:.3e}; "
          f"|bf16x6 - ref64| = {(out6.cpu().double() - r64).abs().max().item():.3e}, |fp32 mode - ref64| = {(out32.cpu().double() - r64).abs().max().item():.3e}")
    assert torch.isfinite(out6).all() and err <= bound
    assert not torch.equal(out6, out32), "the two modes gave the same bits: the switch does nothing?"


def test_the_mode_is_f32_afterwards():
    assert ops.get_matrix_mode() == "f32"
