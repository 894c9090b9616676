"""What the sanitize / largest-fragment filters on the device cost on one MI355X, measured in one job (GPU box):

    python tools/postprocess_probe.py [--out profiles/postprocess_probe.txt] [--windows 5] [--repeats 20]

Workloads: 10 000 QM9-sized molecules (sizes from dataset_info("qm9")'s histogram) and 500 GEOM-sized ones (44 .. 181 atoms, uniform); one
half jittered-lattice clouds, which bond and fragment and mostly fail the valence caps, the other half straight C / N / O chains, which are
valid and in one fragment (the builders of tools/molgraph_probe.py).  Every step runs in a child process of its own under a time limit; the
first one that fails ends the job.

 kernels   gcdm_molproc_select (the select launch and the three scan launches) next to gcdm_molgraph_keys on the same input, device events
           around the call; median and range of ``--repeats`` calls after a warm-up.  The select launch alone is read from a kernel trace of
           this step (rocprofv3 --kernel-trace -- python tools/postprocess_probe.py --step kernels).
 qm9/geom  alternating windows, wall clock, synchronised, of
             (a) process_molecules(..., largest_frag=True, sanitize=True).molecules(), end to end;
             (b) the host route on the same input: sdf.build_molecules, then scipy's connected components, the valence-cap verdict and the
                 cut per molecule;
             (c) the per-molecule copy loop of generate_molecules' unflagged branch, for scale (it filters nothing).
           (a) and (b) must give the same molecules.  A gain is claimed only if the difference of the medians exceeds the spread of the
           baseline's own windows."""
import argparse
import ctypes
import gc
import importlib
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
STEPS = {"kernels": 240, "qm9": 420, "geom": 240}                    # seconds each child may take


def workload(pkg, ds):
    import molgraph_probe as mp
    info = pkg.dataset_info(ds)
    rng = np.random.default_rng(1)
    if ds == "qm9":
        hist = {int(k): int(v) for k, v in info["n_nodes"].items()}
        ks, w = np.array(sorted(hist)), np.array([hist[k] for k in sorted(hist)], np.float64)
        sizes = rng.choice(ks, size=10_000, p=w / w.sum())
    else:
        sizes = rng.integers(44, 182, size=500)
    half = len(sizes) // 2
    x, t = mp.clouds(sizes[:half], len(info["atom_decoder"]), seed=len(sizes))
    rows = mp.chains(sizes[half:], seed=3).numpy()
    dec = [pkg.metrics.ATOMIC_NUMBERS[s] for s in info["atom_decoder"]]
    x = np.concatenate([x, np.stack([rows[:, 1], rows[:, 2], rows[:, 3]], 1)]).astype(np.float32)
    t = np.concatenate([t, np.array([dec.index(int(z)) for z in rows[:, 0]], np.int32)])
    return info, torch.from_numpy(x), torch.from_numpy(t.astype(np.int64)), torch.as_tensor(sizes, dtype=torch.int64)


def host_route(pkg, x, t, nn_, info, caps):
    """(b): whole molecules from sdf.build_molecules, then the two filters per molecule on the host."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    dec = info["atom_decoder"]
    out = []
    for mol in pkg.build_molecules(x, t, nn_, info):
        n = len(mol.symbols)
        if n == 0:
            out.append(mol)
            continue
        b = np.array(mol.bonds, np.int64).reshape(-1, 3)
        val = np.bincount(b[:, 0], b[:, 2], n) + np.bincount(b[:, 1], b[:, 2], n)
        cap = np.array([caps[dec.index(s)] for s in mol.symbols])
        if ((cap >= 0) & (val > cap)).any():
            continue
        k, lab = connected_components(coo_matrix((np.ones(len(b)), (b[:, 0], b[:, 1])), shape=(n, n)), directed=False)
        size = np.bincount(lab, minlength=k)
        first = np.array([np.flatnonzero(lab == c)[0] for c in range(k)])
        best = min(range(k), key=lambda c: (-size[c], first[c]))
        atoms = np.flatnonzero(lab == best)
        new = -np.ones(n, np.int64)
        new[atoms] = np.arange(len(atoms))
        out.append(pkg.Molecule([mol.symbols[a] for a in atoms], mol.positions[atoms],
                                [(int(new[i]), int(new[j]), int(o)) for i, j, o in mol.bonds if new[i] >= 0 and new[j] >= 0], None))
    return out


def copy_loop(x, t, counts):
    """(c): generate_molecules' unflagged branch, mol_gen_ddpm.py."""
    mols, o = [], 0
    for n in counts:
        mols.append((x[o:o + n].cpu(), t[o:o + n].cpu(), None))
        o += n
    return mols


def fmt_s(v):
    return f"{statistics.median(v):8.4f} s  (windows {min(v):.4f} .. {max(v):.4f})"


def fmt_us(v):
    return f"{statistics.median(v) * 1e3:9.1f} us  (range {min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f})"


def step_windows(pkg, ds, windows, dev):
    info, x, t, nn_ = workload(pkg, ds)
    x, t = x.to(dev), t.to(dev)
    tb = pkg.metrics.graph_tables(info)
    caps = list(tb.valence_cap[:len(info["atom_decoder"])])
    counts = nn_.tolist()
    sync = lambda: torch.cuda.synchronize(dev)
    variants = {"a": lambda: pkg.process_molecules(x, t, nn_, info, sanitize=True, largest_frag=True).molecules(),
                "b": lambda: host_route(pkg, x, t, nn_, info, caps), "c": lambda: copy_loop(x, t, counts)}
    first = {k: f() for k, f in variants.items()}                    # warm, and (a) against (b)
    assert len(first["a"]) == len(first["b"]), (len(first["a"]), len(first["b"]))
    for a, b in zip(first["a"], first["b"]):
        assert a.symbols == b.symbols and a.bonds == b.bonds and np.array_equal(a.positions, b.positions)
    kept, atoms, bonds = len(first["a"]), sum(len(m.symbols) for m in first["a"]), sum(len(m.bonds) for m in first["a"])
    del first, a, b                                                  # no long-lived host objects under the windows: a full collection walks them all
    gc.collect()
    res = {k: [] for k in variants}
    for wnd in range(windows):
        for k, f in variants.items():
            sync()
            t0 = time.perf_counter()
            f()
            sync()
            res[k].append(time.perf_counter() - t0)
            print(f"{ds} window {wnd + 1} ({k}): {res[k][-1]:.4f} s", flush=True)
    lines = [f"{ds}: {len(counts)} molecules, {int(nn_.sum())} atoms -> {kept} survive sanitize + largest_frag with {atoms} "
             f"atoms and {bonds} bonds; (a) and (b) give the same molecules; {windows} alternating windows of one call each",
             f"  (a) process_molecules(...).molecules(), end to end: {fmt_s(res['a'])}",
             f"  (b) sdf.build_molecules + scipy components and the filters per molecule: {fmt_s(res['b'])}",
             f"  (c) the per-molecule copy loop of the unflagged generate_molecules branch (filters nothing): {fmt_s(res['c'])}"]
    for base in ("b", "c"):
        diff = statistics.median(res[base]) - statistics.median(res["a"])
        spread = max(res[base]) - min(res[base])
        lines.append(f"  ({base}) - (a), medians: {diff * 1e3:+.1f} ms against a spread of ({base})'s windows of {spread * 1e3:.1f} ms: "
                     + ("a gain outside the spread" if diff > spread else "a loss outside the spread" if -diff > spread else "inside the spread, no claim")
                     + (f", (a) takes {statistics.median(res['a']) / statistics.median(res[base]) * 100:.1f} % of ({base})" if abs(diff) > spread else ""))
    return lines


def step_kernels(pkg, repeats, dev):
    lib = pkg._native.load_ops()
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    lines = []
    for ds in ("qm9", "geom"):
        info, x, t, nn_ = workload(pkg, ds)
        x, t = x.to(dev), t.to(device=dev, dtype=torch.int32)
        M, N = len(nn_), int(nn_.sum())
        tb = pkg.metrics.graph_tables(info)
        off = torch.zeros(M + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(nn_, 0)
        off = off.to(dev)
        e = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        keys, out, out2 = e(M, torch.int64), e((M, 4), torch.int32), e((M, 4), torch.int32)
        keep, new_index, counts, totals = e(N, torch.uint8), e(N, torch.int32), e((M, 3), torch.int32), e(3, torch.int64)
        ws = e(lib.gcdm_molproc_workspace_bytes(M) // 8, torch.int64)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        calls = {"gcdm_molgraph_keys": lambda: lib.gcdm_molgraph_keys(tb, p(x), 3, p(t), p(off), M, p(keys), p(out), stream),
                 "gcdm_molproc_select (select launch + three scan launches)":
                     lambda: lib.gcdm_molproc_select(tb, p(x), 3, p(t), p(off), M, None, None, 3, p(out2), p(keep), p(new_index), p(counts), p(totals),
                                                     p(ws), stream)}
        for name, call in calls.items():
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
            lines.append(f"{name}, {M} {ds.upper()}-sized molecules, {N} atoms: {fmt_us(ms)} per call, device events, {repeats} calls")
        assert torch.equal(out, out2)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postprocess_probe.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process (what the parent starts)")
    args = ap.parse_args()
    if args.step is None:                                            # the parent never opens the GPU: one child per step, each under its limit
        parts = []
        for step, limit in STEPS.items():
            part = f"{args.out}.{step}.part"
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--out", part, "--windows", str(args.windows),
                                "--repeats", str(args.repeats)], timeout=limit)
            if r.returncode != 0:
                sys.exit(f"postprocess_probe: step {step} ended with status {r.returncode}; nothing further is started")
            parts.append(part)
        text = "".join(open(p_).read() for p_ in parts)
        for p_ in parts:
            os.remove(p_)
        with open(args.out, "w") as f:
            f.write(text)
        print(text, end="")
        return
    pkg = importlib.import_module("bio-diffusion_amd")
    dev = torch.device("cuda", 0)
    if args.step == "kernels":
        lines = [f"postprocess_probe: {torch.cuda.get_device_name(0)}, {torch.get_num_threads()} torch CPU threads"] + step_kernels(pkg, args.repeats, dev)
    else:
        lines = step_windows(pkg, args.step, args.windows, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
