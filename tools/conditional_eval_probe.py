"""Times the conditional-evaluation driver -- evaluate_conditional on batches of 100 molecules -- three ways on the same GPU in the same run and
writes the table.

Workload: the alpha-conditional QM9 model at production widths (2-D weights x 0.25), default (split-precision) mode, an EGNN property classifier of
the reference's shape (hidden 128, 7 layers, attention) with its initial weights, ten batches of 100 molecules (iterations = 9), sizes from the
QM9 histogram and contexts from a seeded stand-in for PropertiesDistribution -- both re-seeded before every window, so every window draws the same
batches -- T = 100 denoise steps + the decode per batch, one classifier forward per batch or chunk.  Variants:
    (a) the default call                 one sample() per batch (two slices on two handles at this batch size), one seed for all batches
    (b) concurrent_batches = 4           mol_gen_sample_concurrent on chunks of 4, 4, 2, seeds 1234 + i
    (c) packed_batches = 10              one mol_gen_sample_packed call, seeds 1234 + i
(a) is the driver as it was before the chunked modes existed: its code path is untouched.  (b) and (c) are compared bitwise with each other in the
warm-up; (a) draws other noise (one seed) and slices its batches, so it is compared only by count and shape.
Timing: host clock around whole calls (all ten batches, synchronised), the variants alternating a, b, c, a, b, c, ...; engine clock and socket
power of each window from bench.ClockSampler.  A chunked mode counts as a gain when its median exceeds the median of (a) by more than the spread
(max - min) of (a)'s own windows; the table says which it is.

One process; the whole run is under its own time limit (--time-limit seconds, enforced from a watchdog thread) and stops at the first error.

    python tools/conditional_eval_probe.py [--windows 3] [--steps 100] [--out profiles/conditional_eval_probe.txt]
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

ITERATIONS, PER_BATCH, IN_FLIGHT, PACKED = 9, 100, 4, 10
MEAN, MAD = 75.0, 6.5


class SeededProps:
    """Stand-in for PropertiesDistribution: one property, a seeded normalised context per molecule."""
    properties = ["alpha"]
    normalizer = {"alpha": {"mean": MEAN, "mad": MAD}}

    def __init__(self):
        self.g = torch.Generator().manual_seed(0)

    def sample_batch(self, num_nodes):
        return torch.randn((len(num_nodes), 1), generator=self.g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--time-limit", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conditional_eval_probe.txt"))
    args = ap.parse_args()
    if args.windows < 3:
        raise SystemExit("at least three windows per variant")
    if not torch.cuda.is_available():
        raise SystemExit("conditional_eval_probe needs an MI355X: a CPU run measures nothing")
    faulthandler.dump_traceback_later(args.time_limit, exit=True)          # the run's own time limit: ends the process even inside a blocked device call
    pkg = importlib.import_module("bio-diffusion_amd")
    dev = torch.device("cuda:0")
    cfgs = pkg.default_cfgs("qm9", conditioning=("alpha",))
    torch.manual_seed(0)
    model = pkg.QM9MoleculeGenerationDDPM(**cfgs)
    with torch.no_grad():
        for p in model.ddpm.dynamics_network.parameters():
            if p.dim() == 2:
                p.mul_(0.25)
    model = model.to(dev).eval()
    net = pkg.classifier.EGNN(in_node_nf=5, in_edge_nf=0, hidden_nf=128, device=dev, n_layers=7, attention=1, node_attr=0).to(dev).eval()
    ddpm = model.ddpm
    T, batches = args.steps, ITERATIONS + 1

    def call(T_, **kw):
        torch.manual_seed(0)
        mae, records = model.evaluate_conditional(net, "alpha", MEAN, MAD, iterations=ITERATIONS, batch_size=PER_BATCH, props_distr=SeededProps(),
                                                  num_timesteps=T_, **kw)
        return mae, records, ddpm.last_flags

    variants = [("a", "the default call", {}), ("b", f"concurrent_batches = {IN_FLIGHT}", dict(concurrent_batches=IN_FLIGHT)),
                ("c", f"packed_batches = {PACKED}", dict(packed_batches=PACKED))]
    # warm-up (handles, lanes, captured steps) and the check that the chunked variants agree with each other
    warm = {}
    for key, _, kw in variants:
        mae, records, fl = call(10, **kw)
        torch.cuda.synchronize(dev)
        if fl:
            raise SystemExit(f"variant ({key}) raised device flags {fl:#x} in the warm-up")
        warm[key] = (mae, [(r["num_nodes"].clone(), r["x"].clone(), r["pred"].clone()) for r in records])
    if not all(len(v[1]) == batches for v in warm.values()):
        raise SystemExit("a variant did not return one record per batch")
    for (na, xa, pa), (nb, xb, pb), (nc, xc, pc) in zip(warm["a"][1], warm["b"][1], warm["c"][1]):
        if not (torch.equal(na, nb) and torch.equal(nb, nc) and xa.shape == xb.shape):
            raise SystemExit("the variants did not draw the same batch sizes")
        if not (torch.equal(xb.view(torch.int32), xc.view(torch.int32)) and torch.equal(pb.view(torch.int32), pc.view(torch.int32))):
            raise SystemExit("(b) and (c) do not give the same samples and predictions")
    if warm["b"][0] != warm["c"][0]:
        raise SystemExit("(b) and (c) do not give the same MAE")
    atoms = sum(int(n.sum()) for n, _, _ in warm["a"][1])
    clocks = bench.ClockSampler(0).start()
    t_end = time.perf_counter() + 1.0
    while time.perf_counter() < t_end:          # >= 1 s of work before the first window: the clock settles after the idle set-up
        call(10, packed_batches=PACKED)
    torch.cuda.synchronize(dev)
    rows = []
    for w in range(args.windows):
        for key, label, kw in variants:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            _, _, fl = call(T, **kw)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            if fl:
                raise SystemExit(f"variant ({key}) raised device flags {fl:#x}")
            ck = clocks.stats(t0, t1)
            rows.append(dict(variant=key, label=label, window=w, seconds=t1 - t0, molecules_per_s=batches * PER_BATCH / (t1 - t0),
                             sclk_mhz=ck.get("sclk_mhz"), power_w=ck.get("power_w")))
    clocks.stop()
    ddpm.release_lanes()
    faulthandler.cancel_dump_traceback_later()

    def med(v):
        return sorted(v)[len(v) // 2]

    summary = {}
    for key, label, _ in variants:
        v = [r["molecules_per_s"] for r in rows if r["variant"] == key]
        summary[key] = dict(label=label, median=med(v), min=min(v), max=max(v), spread=max(v) - min(v))
    base = summary["a"]
    full = (T + 1) / bench.NET_EVALS_PER_SAMPLE          # the same batches at the full 1000 steps + decode: per-evaluation time unchanged
    fmt = lambda x, n=1: "n/a" if x is None else f"{x:.{n}f}"          # noqa: E731
    lines = [f"conditional_eval_probe: evaluate_conditional, {batches} ragged batches of {PER_BATCH} molecules (QM9 histogram, re-seeded per window; {atoms} atoms),",
             f"T = {T} steps + decode + the classifier, split-precision mode, {torch.cuda.get_device_name(0)}; clock source: {clocks.source}.",
             f"molecules/s = {batches * PER_BATCH} / window seconds at T = {T}; 'at 1000 steps' = the same x {full:.4f} (sampling dominates; time per network",
             "evaluation unchanged).  (b) and (c) gave bit-identical samples, predictions and MAE in the warm-up; (a) keeps one seed for all batches.", "",
             f"{'variant':<32}{'window':>7}{'seconds':>10}{'molecules/s':>13}{'at 1000 steps':>15}{'sclk MHz':>10}{'power W':>9}"]
    for r in rows:
        lines.append(f"({r['variant']}) {r['label']:<28}{r['window']:>7}{r['seconds']:>10.3f}{r['molecules_per_s']:>13.1f}{r['molecules_per_s'] * full:>15.1f}"
                     f"{fmt(r['sclk_mhz'], 0):>10}{fmt(r['power_w'], 0):>9}")
    lines.append("")
    for key in ("a", "b", "c"):
        s = summary[key]
        lines.append(f"({key}) {s['label']:<28} median {s['median']:.1f} molecules/s (at 1000 steps {s['median'] * full:.1f}), windows {s['min']:.1f} .. {s['max']:.1f}, spread {s['spread']:.1f}")
    lines.append("")
    gains = {}
    for key in ("b", "c"):
        gain = summary[key]["median"] - base["median"]
        gains[key] = dict(gain_molecules_per_s=gain, is_a_gain=gain > base["spread"])
        lines.append(f"({key}) - (a) = {gain:+.1f} molecules/s ({gain / base['median'] * 100:+.1f} %) against a spread of (a)'s own windows of {base['spread']:.1f}: "
                     + ("a gain by the stated rule." if gains[key]["is_a_gain"] else "NOT a gain by the stated rule (the difference is within (a)'s own spread, or negative)."))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    print(json.dumps(dict(workload="qm9_conditional_eval_probe", steps=T, rows=rows, summary=summary, gains=gains)), flush=True)


if __name__ == "__main__":
    main()
