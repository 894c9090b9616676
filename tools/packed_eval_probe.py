"""Times the paper's evaluation workload -- flat batches of 100 molecules -- three ways on the same GPU in the same run and writes the table.

Workload: ten ragged batches of 100 molecules, sizes from the QM9 histogram (fixed generator), T = 100 denoise steps + the decode per batch,
QM9 production widths, default (split-precision) mode.  Variants, on the same size lists and seeds (their samples are compared bitwise first):
    (a) one batch at a time             ten mol_gen_sample calls
    (b) concurrent_batches = 4          mol_gen_sample_concurrent on chunks of 4, 4, 2 (one lane handle + stream per batch)
    (c) packed_batches = 10             one mol_gen_sample_packed call: ten sub-batches in one plan on the primary handle
Timing: host clock around whole windows (all ten batches, synchronised), the variants alternating a, b, c, a, b, c, ... so that clock drift does
not favour whichever runs last; engine clock and socket power of each window from bench.ClockSampler, as the bench line reports them.  (a) and (b)
are the yardstick measured here, not figures from another box.  The packed plan counts as a gain when the median of (c) exceeds the median of (b)
by more than the spread (max - min) of (b)'s own windows; the table says which it is.

One process; the whole run is under its own time limit (--time-limit seconds, enforced from a watchdog thread) and stops at the first error.

    python tools/packed_eval_probe.py [--windows 3] [--steps 100] [--out profiles/packed_eval_probe.txt]
"""
import argparse
import faulthandler
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench          # noqa: E402  (ClockSampler, NET_EVALS_PER_SAMPLE)

BATCHES, PER_BATCH, IN_FLIGHT = 10, 100, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--time-limit", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_eval_probe.txt"))
    args = ap.parse_args()
    if args.windows < 3:
        raise SystemExit("at least three windows per variant")
    if not torch.cuda.is_available():
        raise SystemExit("packed_eval_probe needs an MI355X: a CPU run measures nothing")
    faulthandler.dump_traceback_later(args.time_limit, exit=True)          # the run's own time limit: ends the process even inside a blocked device call
    pkg = importlib.import_module("bio-diffusion_amd")
    dev = torch.device("cuda:0")
    cfgs = pkg.default_cfgs("qm9", ())
    torch.manual_seed(0)
    net = pkg.GCPNetDynamics(**cfgs)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 2:
                p.mul_(0.25)
    net = net.to(dev).eval()
    ddpm = pkg.EquivariantVariationalDiffusion(net, cfgs["diffusion_cfg"], cfgs["dataloader_cfg"], pkg.dataset_info("qm9")).to(dev).eval()
    nd = ddpm.num_nodes_distribution
    g = torch.Generator().manual_seed(2024)
    prob, sizes_of = nd.prob.cpu().float(), nd.num_nodes.cpu()
    lists = [sizes_of[torch.multinomial(prob, PER_BATCH, replacement=True, generator=g)] for _ in range(BATCHES)]
    seeds = [1234 + b for b in range(BATCHES)]
    T = args.steps

    def one_at_a_time(T_):
        return [ddpm.mol_gen_sample(PER_BATCH, lists[b], dev, num_timesteps=T_, seed=seeds[b])[0] for b in range(BATCHES)]

    def concurrent(T_):
        out = []
        for i in range(0, BATCHES, IN_FLIGHT):
            out += [r[0] for r in ddpm.mol_gen_sample_concurrent(lists[i:i + IN_FLIGHT], dev, num_timesteps=T_, seeds=seeds[i:i + IN_FLIGHT])]
        return out

    def packed(T_):
        return [r[0] for r in ddpm.mol_gen_sample_packed(lists, dev, num_timesteps=T_, seeds=seeds)]

    variants = [("a", "one batch at a time", one_at_a_time), ("b", f"concurrent_batches = {IN_FLIGHT}", concurrent), ("c", f"packed_batches = {BATCHES}", packed)]
    # warm-up (handles, lanes, captured steps) and the check that the three variants draw the same samples
    ref = None
    for key, _, fn in variants:
        res = [r.clone() for r in fn(10)]
        torch.cuda.synchronize(dev)
        if ddpm.last_flags:
            raise SystemExit(f"variant ({key}) raised device flags {ddpm.last_flags:#x} in the warm-up")
        if ref is None:
            ref = res
        elif not all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(ref, res)):
            raise SystemExit(f"variant ({key}) does not reproduce the samples of (a)")
    clocks = bench.ClockSampler(0).start()
    t_end = time.perf_counter() + 1.0
    while time.perf_counter() < t_end:          # >= 1 s of work before the first window: the clock settles after the idle set-up
        packed(10)
    torch.cuda.synchronize(dev)
    rows = []
    for w in range(args.windows):
        for key, label, fn in variants:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn(T)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            if ddpm.last_flags:
                raise SystemExit(f"variant ({key}) raised device flags {ddpm.last_flags:#x}")
            ck = clocks.stats(t0, t1)
            rows.append(dict(variant=key, label=label, window=w, seconds=t1 - t0, molecules_per_s=BATCHES * PER_BATCH / (t1 - t0),
                             ms_per_evaluation_of_all_batches=(t1 - t0) / (T + 1) * 1e3, sclk_mhz=ck.get("sclk_mhz"), power_w=ck.get("power_w")))
    clocks.stop()
    ddpm.release_lanes()
    faulthandler.cancel_dump_traceback_later()

    def med(v):
        return sorted(v)[len(v) // 2]

    summary = {}
    for key, label, _ in variants:
        v = [r["molecules_per_s"] for r in rows if r["variant"] == key]
        summary[key] = dict(label=label, median=med(v), min=min(v), max=max(v), spread=max(v) - min(v))
    gain = summary["c"]["median"] - summary["b"]["median"]
    is_gain = gain > summary["b"]["spread"]
    full = (T + 1) / bench.NET_EVALS_PER_SAMPLE          # the same batches at the full 1000 steps + decode: per-evaluation time unchanged
    fmt = lambda x, n=1: "n/a" if x is None else f"{x:.{n}f}"          # noqa: E731
    lines = [f"packed_eval_probe: {BATCHES} ragged batches of {PER_BATCH} molecules (QM9 histogram, fixed generator; {sum(int(x.sum()) for x in lists)} atoms), T = {T} steps + decode,",
             f"split-precision mode, {torch.cuda.get_device_name(0)}; clock source: {clocks.source}.  molecules/s = {BATCHES * PER_BATCH} / window seconds at T = {T};",
             f"'at 1000 steps' = the same x {full:.4f} (time per network evaluation unchanged).  The three variants gave bit-identical samples in the warm-up.", "",
             f"{'variant':<32}{'window':>7}{'seconds':>10}{'molecules/s':>13}{'at 1000 steps':>15}{'ms / evaluation':>17}{'sclk MHz':>10}{'power W':>9}"]
    for r in rows:
        lines.append(f"({r['variant']}) {r['label']:<28}{r['window']:>7}{r['seconds']:>10.3f}{r['molecules_per_s']:>13.1f}{r['molecules_per_s'] * full:>15.1f}"
                     f"{r['ms_per_evaluation_of_all_batches']:>17.3f}{fmt(r['sclk_mhz'], 0):>10}{fmt(r['power_w'], 0):>9}")
    lines.append("")
    for key in ("a", "b", "c"):
        s = summary[key]
        lines.append(f"({key}) {s['label']:<28} median {s['median']:.1f} molecules/s (at 1000 steps {s['median'] * full:.1f}), windows {s['min']:.1f} .. {s['max']:.1f}, spread {s['spread']:.1f}")
    lines.append("")
    lines.append(f"(c) - (b) = {gain:+.1f} molecules/s ({gain / summary['b']['median'] * 100:+.1f} %) against a spread of (b)'s own windows of {summary['b']['spread']:.1f}: "
                 + ("the packed plan is a gain by the stated rule." if is_gain else "NOT a gain by the stated rule (the difference is within (b)'s own spread, or negative)."))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    print(json.dumps(dict(workload="qm9_eval_packed_probe", steps=T, rows=rows, summary=summary, gain_molecules_per_s=gain, packed_is_a_gain=is_gain)), flush=True)


if __name__ == "__main__":
    main()
