#!/usr/bin/env python3
"""Times gcdm_grad_bucket_pack + gcdm_grad_bucket_check (include/gcdm_grad_bucket.h) on the QM9 model's parameter table against the composition
a user would otherwise write -- torch._foreach_mul of the gradients by the scale, then one torch.cat into a flat buffer -- with HIP events,
in alternating windows on one device:

    python tools/grad_bucket_probe.py [--windows 9] [--iters 200] [--out profiles/grad_bucket_probe.txt]

Needs an MI355X; there is no CPU path.  Each window is `iters` back-to-back calls between two events; the figure of a window is its time over
`iters` (host enqueue included where the host is the slower side, as a training loop would see it).  The spread of a side is max - min over
its windows.  The requirement the text file states: median(kernel) <= median(composition) + spread(composition)."""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grad_bucket_probe needs an MI355X")
    pkg = importlib.import_module("bio-diffusion_amd")
    dev = torch.device("cuda:0")
    model = pkg.QM9MoleculeGenerationDDPM(**pkg.default_cfgs("qm9")).to(dev)
    upd = model.configure_data_parallel()
    u = upd.update
    g = torch.Generator(device=dev).manual_seed(1)
    for p in model.parameters():
        if p.requires_grad:
            p.grad = torch.randn(p.shape, generator=g, device=dev) * 0.05
    upd.accumulate()                                       # allocates the bucket, writes the pointer table, first launch
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    values = sum(x.numel() for x in grads)
    flat = torch.empty(values, device=dev)
    lib, st = u._lib, u._stream()
    ws, tab, bucket, q = C.c_void_p(u._ws.data_ptr()), C.c_void_p(upd._gtab.data_ptr()), C.c_void_p(upd.bucket.data_ptr()), u.param_groups[0]["queue_len"]
    scale = 1.0 / 3

    def kernel():
        a = lib.gcdm_grad_bucket_pack(ws, tab, bucket, u._total, u._T, u._C, q, scale, 1, st)
        b = lib.gcdm_grad_bucket_check(ws, bucket, u._total, u._T, u._C, q, 1, st)
        assert a == 0 and b == 0

    def pack_only():
        assert lib.gcdm_grad_bucket_pack(ws, tab, bucket, u._total, u._T, u._C, q, scale, 1, st) == 0

    def add_only():
        assert lib.gcdm_grad_bucket_pack(ws, tab, bucket, u._total, u._T, u._C, q, scale, 0, st) == 0

    def composition():
        torch.cat([x.view(-1) for x in torch._foreach_mul(grads, scale)], out=flat)

    # do the two sides compute the same numbers?
    kernel()
    composition()
    got = torch.cat([upd.bucket[o: o + n] for o, n, p in zip(u._offset, u._numel, model.parameters()) if p.grad is not None])
    same = bool(torch.equal(got, flat))

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters          # microseconds per call

    for _ in range(2):
        window(kernel)
        window(composition)
    window(pack_only)
    window(add_only)
    k, c, p1, p0 = [], [], [], []
    for _ in range(args.windows):
        k.append(window(kernel))
        c.append(window(composition))
        p1.append(window(pack_only))
        p0.append(window(add_only))
    mk, mc = statistics.median(k), statistics.median(c)
    sk, sc = max(k) - min(k), max(c) - min(c)
    moved = 8 * values / 1e6
    lines = [
        "Gradient bucket (include/gcdm_grad_bucket.h): pack + check against torch._foreach_mul + torch.cat on the QM9 parameter table",
        "=" * 120,
        f"device: {torch.cuda.get_device_name(0)}; tensors T = {u._T} ({len(grads)} with a gradient), chunks C = {u._C}, values = {values} "
        f"({moved:.1f} MB read + written by the pack)",
        f"HIP events, {args.windows} alternating windows of {args.iters} calls each, microseconds per call, scale = 1/3, first = 1",
        "",
        "kernel (1 pack launch + 1 check launch)   windows: " + " ".join(f"{x:.1f}" for x in k),
        f"    median {mk:.1f} us   min {min(k):.1f}   max {max(k):.1f}   spread {sk:.1f}   -> {moved / mk:.2f} TB/s of the {moved:.1f} MB",
        f"    the pack alone, first = 1: median {statistics.median(p1):.1f} us (spread {max(p1) - min(p1):.1f}); first = 0 (reads the bucket too, "
        f"{12 * values / 1e6:.1f} MB): median {statistics.median(p0):.1f} us (spread {max(p0) - min(p0):.1f})",
        "composition (_foreach_mul + cat)          windows: " + " ".join(f"{x:.1f}" for x in c),
        f"    median {mc:.1f} us   min {min(c):.1f}   max {max(c):.1f}   spread {sc:.1f}",
        "",
        f"requirement: median(kernel) <= median(composition) + spread(composition): {mk:.1f} <= {mc + sc:.1f}: {'MET' if mk <= mc + sc else 'NOT MET'}",
        f"the two sides' values are bit-identical: {'yes' if same else 'NO'} (compared before timing).  One GPU, one rank: this says nothing about multi-GPU scaling, which has not",
        "been measured; the all-reduce is not part of either side.",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
