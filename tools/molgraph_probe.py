"""What validity, uniqueness and novelty on the device cost on one MI355X, measured in one job (GPU box):

    python tools/molgraph_probe.py [--out profiles/molgraph_probe.txt] [--windows 5] [--repeats 20]

 1. gcdm_molgraph_keys (include/gcdm_molgraph.h), device events around the launch, over 10 000 QM9-sized molecules (sizes from
    dataset_info("qm9")'s histogram) and over 500 GEOM-sized ones (44 .. 181 atoms, uniform): synthetic clouds on a jittered 1.3 A lattice, so
    that the molecules bond and fragment; median and range of ``--repeats`` launches after a warm-up.
 2. MoleculeDataset.graph_keys over 100 000 QM9-shaped molecules (the 10 000 above and 10 000 straight C / N / O chains of the same sizes,
    which are valid and in one fragment, five times each): launch, filter and torch.unique, wall clock, synchronised.
 3. sample_and_analyze, ten batches of 100 molecules at T = 100 on the synthetic QM9 model, with metrics attached and without -- the
    un-attached call is the path the driver had before there were metrics -- in alternating windows of one call each.  The difference of the
    medians stands beside the spread of the baseline's own windows; "no measurable cost" is claimed only if the difference is inside it."""
import argparse
import ctypes
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def clouds(sizes, num_types, seed, spacing=1.3, jitter=0.12):
    """Flat positions [N, 3] fp32 and types [N] of jittered-lattice molecules, about six cells in ten taken."""
    rng = np.random.default_rng(seed)
    xs, ts = [], []
    for n in sizes:
        side = max(2, int(np.ceil((1.7 * n) ** (1.0 / 3.0))))
        cells = rng.choice(side ** 3, size=int(n), replace=False)
        x = np.stack([cells // (side * side), (cells // side) % side, cells % side], 1).astype(np.float64) * spacing
        xs.append((x + rng.uniform(-jitter, jitter, size=x.shape)).astype(np.float32))
        ts.append(rng.integers(0, num_types, size=int(n)).astype(np.int32))
    return np.concatenate(xs), np.concatenate(ts)


def chains(sizes, seed, spacing=1.45):
    """Flat [z, x, y, z] rows of straight chains of C / N / O atoms `spacing` Angstrom apart: every neighbour pair bonds singly and nothing
    else does, so each molecule is valid and in one fragment."""
    rng = np.random.default_rng(seed)
    n = int(np.sum(sizes))
    rows = np.zeros((n, 4), np.float32)
    rows[:, 0] = rng.choice(np.array([6, 7, 8], np.float32), size=n)
    rows[:, 1] = np.concatenate([np.arange(int(k), dtype=np.float32) for k in sizes]) * np.float32(spacing)
    return torch.from_numpy(rows)


def fmt_us(v):
    return f"{statistics.median(v) * 1e3:9.1f} us  (range {min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f})"


def fmt_s(v):
    return f"{statistics.median(v):8.4f} s  (windows {min(v):.4f} .. {max(v):.4f})"


def kernel_times(pkg, ds, sizes, repeats, dev):
    info = pkg.dataset_info(ds)
    x, t = clouds(sizes, len(info["atom_decoder"]), seed=len(sizes))
    x, t, nn_ = torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev), torch.as_tensor(sizes)
    tb = pkg.metrics.graph_tables(info)
    off = torch.zeros(len(sizes) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(nn_.to(torch.int64), 0)
    off = off.to(dev)
    keys = torch.empty(len(sizes), dtype=torch.int64, device=dev)
    out = torch.empty((len(sizes), 4), dtype=torch.int32, device=dev)
    lib = pkg._native.load_ops()
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    call = lambda: lib.gcdm_molgraph_keys(tb, p(x), 3, p(t), p(off), len(sizes), p(keys), p(out), stream)
    for _ in range(3):
        assert call() == 0
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert call() == 0
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    k2, i2 = pkg.molecule_graph_keys(x, t, nn_, info)
    assert torch.equal(k2, keys) and torch.equal(i2, out)
    h = out.cpu().numpy()
    return ms, (f"{int(nn_.sum())} atoms, {float((h[:, 0] == 1).mean()) * 100:.1f} % valid, {h[:, 1].mean():.1f} fragments and "
                f"{h[:, 2].mean():.1f} atoms in the largest on average, {len(torch.unique(keys))} distinct keys"), (x, t, nn_)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "molgraph_probe.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    pkg = importlib.import_module("bio-diffusion_amd")
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    lines = [f"molgraph_probe: {torch.cuda.get_device_name(0)}, {torch.get_num_threads()} torch CPU threads"]

    rng = np.random.default_rng(1)
    hist = {int(k): int(v) for k, v in pkg.dataset_info("qm9")["n_nodes"].items()}
    ks, w = np.array(sorted(hist)), np.array([hist[k] for k in sorted(hist)], np.float64)
    qm9_sizes = rng.choice(ks, size=10_000, p=w / w.sum())
    geom_sizes = rng.integers(44, 182, size=500)
    ms, what, (x, t, nn_) = kernel_times(pkg, "qm9", qm9_sizes, args.repeats, dev)
    lines.append(f"gcdm_molgraph_keys, 10000 QM9-sized molecules ({what}): {fmt_us(ms)} per launch, device events, {args.repeats} launches")
    ms, what, _ = kernel_times(pkg, "geom", geom_sizes, args.repeats, dev)
    lines.append(f"gcdm_molgraph_keys, 500 GEOM-sized molecules of 44 .. 181 atoms ({what}): {fmt_us(ms)} per launch, device events, {args.repeats} launches")

    z = torch.tensor(pkg.metrics.graph_tables(pkg.dataset_info("qm9")).atomic_number[:5])[t.cpu().long()].to(torch.float32)
    rows = torch.cat([z[:, None], x.cpu()], 1)
    off = np.r_[0, np.cumsum(qm9_sizes)]
    crow = chains(qm9_sizes, seed=3)
    confs = ([rows[a:b] for a, b in zip(off[:-1], off[1:])] + [crow[a:b] for a, b in zip(off[:-1], off[1:])]) * 5
    data = pkg.MoleculeDataset.from_conformers(confs, dev, included_species=[1, 6, 7, 8, 9])
    data.graph_keys(pkg.dataset_info("qm9"))
    sync()
    wall = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        got = data.graph_keys(pkg.dataset_info("qm9"))
        sync()
        wall.append(time.perf_counter() - t0)
    lines.append(f"MoleculeDataset.graph_keys, {data.M} QM9-shaped molecules, {data.A} atoms -> {got.numel()} keys: {fmt_s(wall)} wall clock, tables, launch, "
                 f"filter and torch.unique")

    cfgs = pkg.default_cfgs("qm9")
    torch.manual_seed(0)
    model = pkg.QM9MoleculeGenerationDDPM(**cfgs)
    with torch.no_grad():
        for prm in model.ddpm.dynamics_network.parameters():
            if prm.dim() == 2:
                prm.mul_(0.25)
    model = model.cuda()
    metrics = pkg.GraphMolecularMetrics(model.dataset_info, dataset_keys=got)

    def run(attached):
        model.molecular_metrics = metrics if attached else None
        torch.manual_seed(5)
        sync()
        t0 = time.perf_counter()
        r = model.sample_and_analyze(num_samples=1000, batch_size=100, num_timesteps=100)
        sync()
        return time.perf_counter() - t0, r

    run(True), run(False)                                            # warm: libraries loaded, plans built
    res = {False: [], True: []}
    for wnd in range(args.windows):
        for attached in (False, True):
            dt, r = run(attached)
            res[attached].append(dt)
            print(f"window {wnd + 1} attached={attached}: {dt:.4f} s", flush=True)
            if attached:
                last = r
    model.molecular_metrics = None
    diff = statistics.median(res[True]) - statistics.median(res[False])
    spread = max(res[False]) - min(res[False])
    lines.append(f"sample_and_analyze, 10 batches of 100, T = 100, {args.windows} alternating windows of one call each: without metrics {fmt_s(res[False])}   "
                 f"with metrics {fmt_s(res[True])}")
    lines.append(f"difference of the medians {diff * 1e3:+.2f} ms against a spread of the baseline's windows of {spread * 1e3:.2f} ms: "
                 + ("inside the spread, no measurable cost" if abs(diff) <= spread else "outside the spread, a measurable cost")
                 + f"; the attached run reports validity {last['validity']:.3f}, uniqueness {last['uniqueness']:.3f}, novelty {last['novelty']:.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
