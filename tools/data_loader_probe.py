"""What the device-resident data set buys on one MI355X, measured in alternating windows of one job (GPU box):

    python tools/data_loader_probe.py [--out profiles/data_loader_probe.txt] [--molecules 100000] [--windows 4] [--steps 10]

A synthetic QM9-shaped set (sizes drawn from dataset_info's histogram, 29 rows per molecule in the padded layout), B = 64 and B = 1024:
 1. a batch from the loader (HIP events around the two launches, and wall clock) against a host collation written for this probe: the
    molecules' pre-featurised tensors concatenated with torch on the job's CPUs, then copied to the device (wall clock, synchronised);
 2. the fused / fused / fused training step (forward + backward) of the QM9 model on loader batches against hand-built ones (x, one_hot,
    charges, batch, mask and nothing else), B = 64;
 3. the device-to-host synchronisations torch reports per step in set_sync_debug_mode("warn"), both ways.
Every figure is the median of a window's steps; the line gives the median and the range of the windows.  A gain counts only where it exceeds
the spread of the baseline's own windows."""
import argparse
import importlib
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
SPECIES = (1, 6, 7, 8, 9)


def synthetic_qm9(pkg, M, seed=0):
    info = pkg.dataset_info("qm9")
    hist = {int(k): int(v) for k, v in info["n_nodes"].items()}
    sizes_, weights = np.array(sorted(hist)), np.array([hist[k] for k in sorted(hist)], dtype=np.float64)
    rng = np.random.default_rng(seed)
    n = rng.choice(sizes_, size=M, p=weights / weights.sum())
    a_max = int(sizes_.max())
    present = np.arange(a_max)[None, :] < n[:, None]
    charges = np.where(present, rng.choice(SPECIES, size=(M, a_max)), 0).astype(np.int64)
    positions = (rng.standard_normal((M, a_max, 3)).astype(np.float32) * 1.5) * present[..., None]
    return dict(num_atoms=torch.from_numpy(n.astype(np.int64)), charges=torch.from_numpy(charges), positions=torch.from_numpy(positions),
                alpha=torch.from_numpy((rng.standard_normal(M) * 8 + 75).astype(np.float32)))


def host_items(raw):
    """Per-molecule tensors as the reference's data set hands them to its collate function (already featurised: generous to the baseline)."""
    sp = torch.tensor(SPECIES)
    one_hot = (raw["charges"].unsqueeze(-1) == sp).float()
    mask = raw["charges"] > 0
    ch = raw["charges"].float()
    return [(raw["positions"][m], one_hot[m], ch[m], mask[m]) for m in range(raw["charges"].shape[0])]


def host_collate(items, idx, dev):
    xs, ohs, chs, mks = zip(*(items[i] for i in idx))
    a_max = xs[0].shape[0]
    batch = dict(x=torch.cat(xs), one_hot=torch.cat(ohs), charges=torch.cat(chs), mask=torch.cat(mks),
                 batch=torch.repeat_interleave(torch.arange(len(idx)), a_max))
    return pkg_attr({k: v.to(dev) for k, v in batch.items()})


def pkg_attr(d):
    return importlib.import_module("bio-diffusion_amd").AttrDict(d)


def windows(fns, nwin, steps, sync):
    """Alternates the callables window by window; per callable the list of window medians (ms per call, wall clock, synchronised)."""
    out = {name: [] for name in fns}
    for _ in range(nwin):
        for name, fn in fns.items():
            ts = []
            for _ in range(steps):
                sync()
                t0 = time.perf_counter()
                fn()
                sync()
                ts.append((time.perf_counter() - t0) * 1e3)
            out[name].append(statistics.median(ts))
    return out


def fmt(ws):
    return f"{statistics.median(ws):9.3f} ms  (windows {min(ws):.3f} .. {max(ws):.3f})"


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message) for w in rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_loader_probe.txt"))
    ap.add_argument("--molecules", type=int, default=100000)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    pkg = importlib.import_module("bio-diffusion_amd")
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    lines = [f"data_loader_probe: {args.molecules} synthetic QM9-shaped molecules, padded layout (29 rows per molecule), {args.windows} alternating "
             f"windows of {args.steps} calls, median per window; {torch.cuda.get_device_name(0)}, {torch.get_num_threads()} torch CPU threads"]
    raw = synthetic_qm9(pkg, args.molecules)
    t0 = time.perf_counter()
    ds = pkg.MoleculeDataset(raw, dev)
    sync()
    lines.append(f"upload (filters, statistics, ragged layout, copy): {time.perf_counter() - t0:.2f} s once; "
                 f"{sum(t.numel() * t.element_size() for t in (ds.atom_ptr, ds.z, ds.pos, ds.props, ds.index)) / 1e6:.1f} MB in HBM")
    items = host_items(raw)
    for B in (64, 1024):
        loader = ds.loader(B, seed=1)
        it = iter(loader)
        idx = loader.indices.tolist()
        cursor = [0]

        def from_loader():
            return next(it)

        def from_host():
            cursor[0] = (cursor[0] + B) % (len(idx) - B)
            return host_collate(items, idx[cursor[0]:cursor[0] + B], dev)

        for _ in range(3):
            from_loader(), from_host()
        res = windows({"loader": from_loader, "host": from_host}, args.windows, args.steps, sync)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        sync()
        ev[0].record()
        for _ in range(args.steps):
            from_loader()
        ev[1].record()
        sync()
        lines.append(f"B = {B:4d}  one batch, wall clock: loader {fmt(res['loader'])}   host collation + copy {fmt(res['host'])}")
        lines.append(f"B = {B:4d}  one batch, HIP events around {args.steps} loader batches back to back: {ev[0].elapsed_time(ev[1]) / args.steps:.3f} ms / batch")
    ds.check()

    # the training step, B = 64
    torch.manual_seed(0)
    model = pkg.QM9MoleculeGenerationDDPM(**pkg.default_cfgs("qm9"))
    with torch.no_grad():
        for p in model.ddpm.dynamics_network.parameters():
            if p.dim() == 2:
                p.mul_(0.25)
    model = model.to(dev).train()
    model.ddpm.dynamics_network.set_message_path("fused")
    model.ddpm.dynamics_network.set_node_path("fused")
    model.set_objective_path("fused")
    B = 64
    loader = ds.loader(B, seed=2)
    it = iter(loader)
    idx = loader.indices.tolist()
    cursor = [0]

    def step(batch):
        model.zero_grad(set_to_none=True)
        model.training_step(batch)["loss"].backward()

    def step_loader():
        step(next(it))

    def step_stripped():                                  # the loader's tensors without fc_graph / all_present / num_graphs: the hints alone
        b = next(it)
        step(pkg.AttrDict({k: v for k, v in b.items() if k not in ("fc_graph", "all_present", "num_graphs")}))

    def step_hand():
        cursor[0] = (cursor[0] + B) % (len(idx) - B)
        step(host_collate(items, idx[cursor[0]:cursor[0] + B], dev))

    for _ in range(3):
        step_loader(), step_stripped(), step_hand()
    res = windows({"loader": step_loader, "stripped": step_stripped, "hand": step_hand}, args.windows, args.steps, sync)
    lines.append(f"B = {B:4d}  batch + fused / fused / fused training step (forward + backward), wall clock: loader batches {fmt(res['loader'])}   "
                 f"loader batches stripped of the hints {fmt(res['stripped'])}   hand-built batches (host collation + copy) {fmt(res['hand'])}")
    lines.append(f"B = {B:4d}  synchronising calls torch reports per step (batch included): loader batches {count_syncs(step_loader)}, stripped of the hints {count_syncs(step_stripped)}, "
                 f"hand-built batches {count_syncs(step_hand)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
