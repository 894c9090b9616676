"""What segmenting the GEOM-Drugs conformer file on the device buys on one MI355X, measured in alternating windows of one job (GPU box):

    python tools/geom_ingest_probe.py [--out profiles/geom_ingest_probe.txt] [--rows 20000000] [--windows 3] [--chunk-rows 4194304]

A synthetic conformer array of ``--rows`` float64 rows [rows, 5] (molecule id, atomic number, x, y, z; 20 M rows are 0.8 GB of host memory; the
real GEOM_drugs_30.npy has about 292 M), molecule sizes drawn from dataset_info("geom")'s histogram, with a random permutation.
 1. MoleculeDataset.geom_splits on the array: chunked upload through one pinned buffer, segmentation, split, size sort and gather in HBM, the
    three data sets ready (wall clock, synchronised);
 2. the host route on the same array, as the reference's load_split_data and GeomDrugsDataset go about it: np.split into one array per
    conformer, the permutation, the three cuts, np.argsort of the sizes per split, then MoleculeDataset.from_conformers per split (wall clock,
    synchronised).
Both run once per window, alternating; the line gives the median and the range of the windows.  A gain counts only where it exceeds the spread
of the baseline's own windows.  The two routes are checked to give the same three data sets."""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def synthetic_file(pkg, rows, seed=0):
    info = pkg.dataset_info("geom")
    hist = {int(k): int(v) for k, v in info["n_nodes"].items()}
    sizes_, weights = np.array(sorted(hist)), np.array([hist[k] for k in sorted(hist)], dtype=np.float64)
    rng = np.random.default_rng(seed)
    n = np.zeros(0, dtype=np.int64)
    while n.sum() < rows:
        n = np.concatenate((n, rng.choice(sizes_, size=int(rows / (sizes_ * weights).sum() * weights.sum()) + 8, p=weights / weights.sum())))
    n = n[:int(np.searchsorted(np.cumsum(n), rows)) + 1]
    counts = np.array([info["atom_types"][t] for t in range(len(pkg.data.GEOM_ATOMIC_NUMBERS))], dtype=np.float64)
    out = np.empty((rows, 5), dtype=np.float64)
    out[:, 0] = np.repeat(np.arange(len(n), dtype=np.float64), n)[:rows]
    out[:, 1] = rng.choice(np.array(pkg.data.GEOM_ATOMIC_NUMBERS, dtype=np.float64), size=rows, p=counts / counts.sum())
    out[:, 2:] = rng.standard_normal((rows, 3)) * 3
    M = int(out[-1, 0]) + 1
    return out, rng.permutation(M).astype("int32")


def host_route(pkg, all_data, perm, dev):
    mol_id = all_data[:, 0].astype(int)
    conformers = all_data[:, 1:]
    data_list = np.split(conformers, np.nonzero(mol_id[:-1] - mol_id[1:])[0] + 1)
    data_list = [data_list[i] for i in perm]
    val_index = int(len(data_list) * 0.1)
    test_index = val_index + int(len(data_list) * 0.1)
    out = {}
    for name, part in (("valid", data_list[:val_index]), ("test", data_list[val_index:test_index]), ("train", data_list[test_index:])):
        argsort = np.argsort([s.shape[0] for s in part])
        out[name] = pkg.MoleculeDataset.from_conformers([part[i] for i in argsort], dev, included_species=list(pkg.data.GEOM_ATOMIC_NUMBERS))
    return out


def fmt(ws):
    return f"{statistics.median(ws):9.3f} s  (windows {min(ws):.3f} .. {max(ws):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geom_ingest_probe.txt"))
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--chunk-rows", type=int, default=1 << 22)
    args = ap.parse_args()
    pkg = importlib.import_module("bio-diffusion_amd")
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    all_data, perm = synthetic_file(pkg, args.rows)
    lines = [f"geom_ingest_probe: {args.rows} synthetic rows ({all_data.nbytes / 1e9:.2f} GB float64), {len(perm)} conformers, chunks of {args.chunk_rows} rows, "
             f"{args.windows} alternating windows of one call each; {torch.cuda.get_device_name(0)}, {torch.get_num_threads()} torch CPU threads"]
    routes = {"device": lambda: pkg.MoleculeDataset.geom_splits(all_data, dev, permutation=perm, chunk_rows=args.chunk_rows),
              "host": lambda: host_route(pkg, all_data, perm, dev)}
    routes["device"]()                                        # the library is loaded, the allocator warm
    res, last = {name: [] for name in routes}, {}
    for _ in range(args.windows):
        for name, fn in routes.items():
            last.pop(name, None)
            sync()
            t0 = time.perf_counter()
            last[name] = fn()
            sync()
            res[name].append(time.perf_counter() - t0)
            print(f"window {len(res[name])} {name}: {res[name][-1]:.3f} s", flush=True)
    for split in ("train", "valid", "test"):
        a, b = last["device"][split], last["host"][split]
        same = all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("atom_ptr", "z", "pos", "index"))
        lines.append(f"{split:5s}: {a.M} molecules, {a.A} atoms, the two routes give {'the same' if same else 'DIFFERENT'} atom_ptr, z, pos and index")
    lines.append(f"file to three device-resident, size-sorted splits, wall clock: geom_splits {fmt(res['device'])}   "
                 f"host route (np.split, permutation, argsort, from_conformers) {fmt(res['host'])}")
    lines.append(f"geom_splits: {args.rows / statistics.median(res['device']) / 1e6:.1f} M rows / s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
