"""Where a training step of the module path spends its time (GPU box): wall clock per step against the GPU-side kernel time of the same steps.

    python tools/train_step_probe.py [steps] [--message-path operators|fused|tiled] [--node-path operators|fused] [--matrix-mode f32|bf16x6]   -> wall ms / step, host enqueue ms / step, HIP-event ms / step
    rocprofv3 --kernel-trace --stats -- python tools/train_step_probe.py 5      (sum of kernel durations / steps = GPU busy time per step)

--update torch|fused adds the update after backward(): `torch` the reference's recipe in stock torch (adaptive clipping with two host
syncs, AdamW amsgrad, the per-entry EMA), `fused` optim.TrainingUpdate (three launches); the default `none` is the bare forward + backward.

--message-path fused runs every interaction layer's message function as one autograd node on the fused message kernels
(GCPNetDynamics.set_message_path, include/gcdm_mp_train.h), --message-path tiled the same node on one tile kernel per message GCP
(include/gcdm_mp_tile.h: 29 launches per layer instead of 49); the default is the operator path bench.py times.

--node-path fused runs every stand-alone GCP2 (the embedding GCPs, the feed-forward and position GCPs of each layer, the scalar projection) as
one autograd node on the fused GCP2 kernels (GCPNetDynamics.set_node_path, include/gcdm_gcp2_train.h); independent of --message-path.

--objective-path fused runs everything around the network evaluation -- noising, loss terms, their backward -- on the fused objective
(EquivariantVariationalDiffusion.set_objective_path, include/gcdm_objective.h): four launches forward, one backward; independent of the others.

--matrix-mode bf16x6 runs every training GEMM (the plain GEMM, the grouped weight gradients, the fused GCP2's GEMM kernels) on the six-product
bf16 split instead of fp32 MFMA (ops.set_matrix_mode, include/gcdm_matrix_mode.h); the default f32 is what bench.py times.

The step is bench.py's `training_step`: forward in training mode + loss + backward of one 64-molecule QM9 batch through libgcdm_ops.so's operators."""
import importlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _torch_update(params):
    """The reference's recipe in stock torch: adaptive clipping (Queue + get_grad_norm + clip_grad_norm_), AdamW(amsgrad), per-entry EMA."""
    import numpy as np
    opt = torch.optim.AdamW(params, lr=1e-4, weight_decay=1e-12, amsgrad=True)
    ema = [p.detach().clone() for p in params]
    queue = [3000.0]

    def step():
        ps = [p for p in params if p.grad is not None]
        max_norm = 1.5 * np.mean(queue) + 2 * np.std(queue)
        norm = torch.norm(torch.stack([torch.norm(p.grad.detach(), 2.0) for p in ps]), 2.0)
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
        queue.insert(0, float(max_norm) if float(norm) > max_norm else float(norm))
        del queue[50:]
        opt.step()
        with torch.no_grad():
            for e, p in zip(ema, params):
                diff = e - p
                diff.mul_(1.0 - 0.9999)
                e.sub_(diff)
    return step


def build_step(message_path="operators", update="none", node_path="operators", objective_path="operators"):
    import synth
    pkg = importlib.import_module("bio-diffusion_amd")
    dev = torch.device("cuda", 0)
    d = synth.DATASET_DIMS["qm9"]
    cfgs = pkg.default_cfgs("qm9", ())
    torch.manual_seed(0)
    net = pkg.GCPNetDynamics(**cfgs)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 2:
                p.mul_(0.25)
    net = net.to(dev)
    net.set_message_path(message_path)
    net.set_node_path(node_path)
    info = pkg.dataset_info("qm9")
    ddpm = pkg.EquivariantVariationalDiffusion(net, cfgs["diffusion_cfg"], cfgs["dataloader_cfg"], info).to(dev)
    ddpm._native(dev)
    ddpm.set_objective_path(objective_path)
    Bt, n = 64, 19
    nt_ = torch.full((Bt,), n, dtype=torch.long, device=dev)
    Nt = Bt * n
    bt = torch.repeat_interleave(torch.arange(Bt, device=dev), nt_)
    g = torch.Generator().manual_seed(5)
    types = torch.randint(0, d["num_atom_types"], (Nt,), generator=g)
    tb = pkg.config.AttrDict(x=torch.randn((Nt, 3), generator=g).to(dev), batch=bt, mask=torch.ones(Nt, dtype=torch.bool, device=dev), props_context=None,
                             h={"categorical": torch.nn.functional.one_hot(types, d["num_atom_types"]).float().to(dev),
                                "integer": (torch.randint(1, 10, (Nt,), generator=g).float().to(dev) if d["include_charges"] else torch.zeros((Nt, 0), device=dev))},
                             num_graphs=Bt, num_nodes_present=nt_)
    ddpm.train()

    params = list(ddpm.parameters())
    upd = None
    if update == "torch":
        upd = _torch_update(params)
    elif update == "fused":
        upd = pkg.TrainingUpdate(params).step

    def once():
        for p_ in params:
            p_.grad = None
        terms = ddpm(tb)
        (terms[1] + terms[3] + terms[4]).mean().backward()
        if upd is not None:
            upd()

    return once, dev


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=10)
    ap.add_argument("--message-path", choices=("operators", "fused", "tiled"), default="operators")
    ap.add_argument("--node-path", choices=("operators", "fused"), default="operators")
    ap.add_argument("--objective-path", choices=("operators", "fused"), default="operators")
    ap.add_argument("--update", choices=("none", "torch", "fused"), default="none")
    ap.add_argument("--matrix-mode", choices=("f32", "bf16x6"), default="f32")
    args = ap.parse_args()
    steps = args.steps
    once, dev = build_step(args.message_path, args.update, args.node_path, args.objective_path)
    importlib.import_module("bio-diffusion_amd").ops.set_matrix_mode(args.matrix_mode)
    for _ in range(3):
        once()
    torch.cuda.synchronize(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t0 = time.perf_counter()
    ev[0].record()
    for _ in range(steps):
        once()
    ev[1].record()
    t_host = (time.perf_counter() - t0) / steps * 1e3          # host done enqueueing
    torch.cuda.synchronize(dev)
    wall = (time.perf_counter() - t0) / steps * 1e3
    print(f"training step, 64 x 19, message path {args.message_path}, node path {args.node_path}, objective path {args.objective_path}, update {args.update}, matrix mode {args.matrix_mode}: wall {wall:.2f} ms / step, host enqueue {t_host:.2f} ms / step, HIP events {ev[0].elapsed_time(ev[1]) / steps:.2f} ms / step")


if __name__ == "__main__":
    main()
