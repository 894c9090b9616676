"""Golden fixtures of the TRAINING objective and its gradients, produced by the REFERENCE itself (build container only):

    python tests/golden/make_training_golden.py [name ...]   ->  tests/golden/train_full_<name>.npz   (no name: every VARIANT below)

The unmodified ``EquivariantVariationalDiffusion.forward`` in TRAINING mode (variational_diffusion.py:948-1160: one evaluation of the network at
t >= 0, the t = 0 terms masked in) runs on a data-like ragged batch with full-width seed-recreated weights, its two sources of randomness pinned
(``torch.randint`` returns the stored t_int -- which includes a 0 -- and ``torch.randn`` draws from ref_harness.NoiseTape); the terms are
assembled into the L2 training loss exactly as ``QM9MoleculeGenerationDDPM.forward`` does (qm9_mol_gen_ddpm.py:222-262, loss_type "l2",
norm_training_by_max_nodes false) and ``loss = nll.mean(0)`` (``training_step`` :352) is back-propagated by torch autograd through the
reference's modules.  Once in fp32 and once in fp64.  Stored: the batch, t_int, seeds, every term, nll, loss, the gradient NORM and absolute
maximum of every parameter tensor, and a handful of full gradients.

VARIANTS are the other ways the reference trains, same method and keys (plus ``context`` per molecule, ``mask``, ``n_draws`` where they apply):
  qm9cond     conditional model (one context value per molecule, broadcast to its nodes), norm_training_by_max_nodes true
  qm9sc       diffusion_cfg.self_condition, the reference module's ``random`` patched to return 0.0 so that the branch (:1017-1039) is taken;
              t_int holds no T, a 0 and a 999 (whose jump starts at T); the tape must record six draws: z_t, z_t_self_cond, the jump, x then h
  qm9sc_skip  the same model on the t_int of train_full_qm9 (holds T): the branch is skipped, xh_self_cond=None, two draws
  geomsc      GEOM dims, the branch taken
  qm9vlb      loss_type "vlb": loss_t = T/2 SNR_weight error_t, loss_0 with its constants (qm9_mol_gen_ddpm.py:246-250)
  qm9mask     the last two nodes of molecule 1 and the first of molecule 3 masked out (x, one_hot, charges zero there; x CoM-free over the
              unmasked nodes; num_nodes_present = the unmasked counts)
train_full_{qm9,geom}.npz themselves are not rewritten unless named.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import ref_harness as rh  # noqa: E402
import synth  # noqa: E402
from make_golden import cfgs_for  # noqa: E402

torch.set_num_threads(4)
NAMES = ("delta_log_px", "error_t", "SNR_weight", "loss_0_x", "loss_0_h", "neg_log_constants", "kl_prior", "log_pN", "t_int")
FULL_GRADS = ("gcp_embedding.edge_embedding.scalar_out.weight", "gcp_embedding.node_embedding.vector_down.weight",
              "interaction_layers.0.interaction.message_fusion.0.vector_down_frames.weight", "interaction_layers.0.interaction.message_fusion.2.vector_up.weight",
              "interaction_layers.1.interaction.scalar_message_attention.0.weight", "interaction_layers.1.feedforward_network.0.scalar_out.2.bias",
              "interaction_layers.2.node_position_update_gcp.vector_up.weight", "scalar_node_projection_gcp.scalar_out.weight")


VARIANTS = {
    "qm9cond": dict(case="qm9cond", by_max=True, context=True),
    "qm9sc": dict(case="qm9", self_cond=True, t_int=[0, 517, 999, 36, 1, 250], n_draws=6),
    "qm9sc_skip": dict(case="qm9", self_cond=True, n_draws=2),
    "geomsc": dict(case="geom", self_cond=True, t_int=[0, 517, 999, 36], n_draws=6),
    "qm9vlb": dict(case="qm9", loss_type="vlb"),
    "qm9mask": dict(case="qm9", masked=((1, -2), (1, -1), (3, 0))),
}


def make_case(case, weight_seed=31, noise_seed=2468, name=None, self_cond=False, loss_type="l2", by_max=False, context=False, masked=(),
              t_int=None, n_draws=2):
    out_name = name or case
    ds, cond, cfgs = cfgs_for(case)
    d = synth.DATASET_DIMS[case]
    cfgs["diffusion_cfg"]["self_condition"] = self_cond          # (False is the value both configs have)
    cfgs["diffusion_cfg"]["loss_type"] = loss_type
    cfgs["diffusion_cfg"]["norm_training_by_max_nodes"] = by_max
    shapes = synth.dynamics_shapes(d["S"], d["V"], d["Se"], d["Ve"], d["L"], synth.dims_h_in(d), self_cond_feats=synth.dims_feat(d) if self_cond else 0)
    include_charges = bool(cfgs["dataloader_cfg"]["include_charges"])
    nt = int(cfgs["dataloader_cfg"]["num_atom_types"])
    sizes = [5, 19, 3, 11, 16, 9] if case != "geom" else [5, 44, 3, 30]
    nn_ = torch.tensor(sizes)
    B, N = len(sizes), sum(sizes)
    bi = torch.repeat_interleave(torch.arange(B), nn_)
    g = torch.Generator().manual_seed(67)
    x = torch.randn((N, 3), generator=g) * 1.5
    for b in range(B):
        x[bi == b] -= x[bi == b].mean(0, keepdim=True)
    one_hot = torch.nn.functional.one_hot(torch.randint(0, nt, (N,), generator=g), nt).float()
    charges = (torch.randint(1, 10, (N,), generator=g).float() if include_charges else torch.zeros((N, 0)))
    t_int = torch.tensor([[0], [517], [1000], [36], [1], [250]][:B]) if t_int is None else torch.tensor(t_int).view(B, 1)
    mask = torch.ones(N, dtype=torch.bool)
    F = nt + int(include_charges)
    starts = torch.cat([torch.zeros(1, dtype=torch.long), nn_.cumsum(0)])
    for b, k in masked:
        mask[(starts[b + 1] if k < 0 else starts[b]) + k] = False
    nn_present = torch.zeros(B, dtype=torch.long).index_add_(0, bi, mask.long())
    if masked:
        mf = mask.float().unsqueeze(-1)
        for b in range(B):
            x[bi == b] -= (x[bi == b] * mf[bi == b]).sum(0, keepdim=True) / nn_present[b]
        x, one_hot = x * mf, one_hot * mf
        charges = charges * (mask.float() if charges.dim() == 1 else mf)
    ctx = torch.randn(B, generator=torch.Generator().manual_seed(71)) if context else None          # normalised property values, one per molecule

    def run(dtype):
        prev = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        orig_randint = torch.randint
        _, vd, _ = rh.import_reference()
        orig_random = vd.random
        try:
            net = rh.build_reference_dynamics(cfgs, seed=0)
            assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == shapes
            net.load_state_dict(synth.make_weights(shapes, seed=weight_seed, scale_2d=0.5))
            ddpm = rh.build_reference_ddpm(cfgs, net, ds).to(dtype)
            ddpm.train()
            batch = rh.make_batch(bi, mask, None if ctx is None else ctx.to(dtype)[bi].unsqueeze(-1))
            batch.x = x.to(dtype).clone()
            batch.h = {"categorical": one_hot.to(dtype).clone(), "integer": charges.to(dtype).clone()}
            batch.num_graphs = B
            batch.num_nodes_present = nn_present.clone()
            torch.randint = lambda *a, **k: t_int.clone()
            vd.random = lambda: 0.0                                             # "random() < self_conditioning_prob" holds: the branch is taken if it can be
            with rh.NoiseTape(noise_seed) as tape:
                terms = ddpm(batch, return_loss_info=True)
            # x / h noise of z_t: ONE evaluation in training mode; with the self-conditioning branch taken, of z_t_self_cond and of the jump too
            assert tape.calls == [(N, 3), (N, F)] * (n_draws // 2), tape.calls
            delta_log_px, error_t, SNR_weight, loss_0_x, loss_0_h, neg_log_const_0, kl_prior, log_pN, _, _ = terms
            # qm9_mol_gen_ddpm.py:222-262 (training)
            if loss_type == "l2":
                denom = (3 + F) * (nn_present.max() if by_max else nn_present)
                loss_t = 0.5 * (error_t / denom)
                loss_0 = loss_0_x / denom + loss_0_h
            else:
                loss_t = ddpm.T * 0.5 * SNR_weight * error_t
                loss_0 = loss_0_x + loss_0_h + neg_log_const_0
            nll = loss_t + loss_0 + kl_prior - delta_log_px - log_pN
            loss = nll.mean(0)
            loss.backward()
            grads = {k: p.grad.detach().clone() for k, p in ddpm.dynamics_network.named_parameters()}
            return terms, nll.detach(), loss.detach(), grads
        finally:
            torch.randint = orig_randint
            vd.random = orig_random
            torch.set_default_dtype(prev)

    arrs = dict(num_nodes=nn_.numpy(), x=x.numpy(), one_hot=one_hot.numpy(), charges=charges.numpy(), t_int=t_int.flatten().numpy(),
                weight_seed=weight_seed, weight_scale=0.5, noise_seed=noise_seed, keys=np.array(list(shapes)))
    if out_name in VARIANTS:
        arrs.update(n_draws=n_draws, self_condition=self_cond, loss_type=loss_type, by_max=by_max, num_nodes_present=nn_present.numpy())
    if ctx is not None:
        arrs["context"] = ctx.numpy()
    if masked:
        arrs["mask"] = mask.numpy()
    res = {}
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        terms, nll, loss, grads = run(dtype)
        res[tag] = (loss, grads)
        cast = (lambda v: v.detach().double().numpy()) if tag == "64" else (lambda v: v.detach().float().numpy())
        for name, v in zip(NAMES, terms[:9]):
            arrs[f"{name}_{tag}"] = cast(v)
        arrs[f"nll_{tag}"], arrs[f"loss_{tag}"] = cast(nll), cast(loss)
        arrs[f"grad_norm_{tag}"] = np.array([float(grads[k].double().norm()) for k in shapes])
        arrs[f"grad_absmax_{tag}"] = np.array([float(grads[k].double().abs().max()) for k in shapes])
        for k in FULL_GRADS:
            if k in grads:
                arrs[f"grad_{tag}::{k}"] = cast(grads[k])
    l32, g32 = res["32"]
    l64, g64 = res["64"]
    worst = max(float((g32[k].double() - g64[k]).norm() / max(float(g64[k].norm()), 1e-30)) for k in shapes)
    print(f"{out_name}: loss {float(l32):.6f} / {float(l64):.6f}; worst relative fp32-vs-fp64 gradient gap = {worst:.2e}; "
          f"zero-gradient tensors: {sum(1 for k in shapes if float(g64[k].norm()) == 0.0)}", flush=True)
    np.savez_compressed(os.path.join(HERE, f"train_full_{out_name}.npz"), **arrs)


if __name__ == "__main__":
    assert rh.reference_available(), "reference checkout not found"
    for name in sys.argv[1:] or list(VARIANTS):
        make_case(**(dict(VARIANTS[name], name=name) if name in VARIANTS else dict(case=name)))
