"""Times one forward of the EGNN dynamics network (bio-diffusion_amd/egnn_dynamics.py) under torch.no_grad() on its two paths -- "fused"
(include/gcdm_egnn_dynamics.h: column-split edge_mlp.0, one edge kernel per layer) against "operators" (the reference's formulation on the
autograd operators, the [E, D] concatenation included) -- in alternating windows of one job, and records the result.

Workloads: "qm9" = 1024 molecules of 19 atoms (19 456 atoms, 369 664 edges), "geom" = 256 molecules of 44 atoms (11 264 atoms, 495 616
edges); both H = 256, L = 9, time-conditioned, seeded weights and inputs; Eh = 64 (qm9) / 16 (geom) as the GCPNet configurations of the two
data sets.  Time: device events around a window of at least `--seconds` after warm-up.  "operators" is the baseline: the spread of its own
windows stands beside the difference, and a gain is claimed only if the difference exceeds it.

One case per process, so that each GPU step runs under its own time limit:

    timeout -k 10 600 python tools/egnn_dynamics_probe.py --case qm9 && timeout -k 10 600 python tools/egnn_dynamics_probe.py --case geom --append
"""
import argparse
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import egnn_dynamics_ref as er          # noqa: E402

CASES = {"qm9": dict(molecules=1024, atoms=19, Eh=64, types=5, charges=True), "geom": dict(molecules=256, atoms=44, Eh=16, types=16, charges=True)}
H, L = 256, 9
VARIANTS = (("operators", "(a) operators: cat + ops.linear"), ("fused", "(b) fused: gcdm_egnn_dyn_layer"))


def window(step, min_seconds):
    """ms per call of step() from device events over a window of at least `min_seconds`."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls, total, reps = 0, 0.0, 1
    while total < min_seconds * 1e3:
        a.record()
        for _ in range(reps):
            step()
        b.record()
        b.synchronize()
        total += a.elapsed_time(b)
        calls += reps
        reps = min(reps * 2, 64)
    return total / calls, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), required=True)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "egnn_dynamics_probe.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("egnn_dynamics_probe needs an MI355X: a CPU run measures nothing")
    pkg = importlib.import_module("bio-diffusion_amd")
    dev = torch.device("cuda:0")
    c = CASES[args.case]
    cfg = dict(H=H, Eh=c["Eh"], L=L, num_atom_types=c["types"], include_charges=c["charges"], condition_on_time=True, num_context=0, self_condition=False)
    sizes = [c["atoms"]] * c["molecules"]
    net = pkg.EGNNDynamics(**er.reference_cfgs(cfg))
    net.load_state_dict(er.make_weights(cfg, seed=11, coors_scale=1e-2))
    net = net.to(dev).eval()
    xh, t, bi, _, _ = er.make_inputs(cfg, sizes, seed=12)
    batch = pkg.AttrDict(batch=bi.to(dev), mask=torch.ones(len(bi), dtype=torch.bool, device=dev), props_context=None)
    xh, t = xh.to(dev), t.to(dev)

    def step():
        with torch.no_grad():
            return net(batch, xh, t)[1]

    outs = {}
    for mode, _ in VARIANTS:                       # warm-up of both paths: code objects, the plan, the packed weights, the graph
        net.set_path(mode)
        outs[mode] = step().clone()
        step()
    torch.cuda.synchronize()
    diff_paths = float((outs["fused"] - outs["operators"]).abs().max())
    ms = {mode: [] for mode, _ in VARIANTS}
    rows = []
    for w in range(args.windows):
        for mode, label in VARIANTS:
            net.set_path(mode)
            torch.cuda.synchronize()
            tm, calls = window(step, args.seconds)
            ms[mode].append(tm)
            rows.append(f"{label:<40}{w:>6}{calls:>8}{tm:>12.4f}")
    N, E = sum(sizes), sum(n * n for n in sizes)
    lines = [f"egnn_dynamics_probe [{args.case}]: one forward of EGNNDynamics under no_grad, {c['molecules']} molecules of {c['atoms']} atoms ({N} atoms, {E} edges),",
             f"H = {H}, Eh = {c['Eh']}, L = {L}, {torch.cuda.get_device_name(0)}.  Windows of at least {args.seconds} s, the two paths alternating.",
             f"max|fused - operators| of the output = {diff_paths:.3e} (max|out| = {float(outs['operators'].abs().max()):.3e}).", "",
             f"{'path':<40}{'window':>6}{'calls':>8}{'ms / call':>12}"] + rows + [""]
    for mode, label in VARIANTS:
        v = ms[mode]
        lines.append(f"{label:<40} median {statistics.median(v):.4f} ms / forward, windows {min(v):.4f} .. {max(v):.4f}, spread {max(v) - min(v):.4f}")
    base, new = statistics.median(ms["operators"]), statistics.median(ms["fused"])
    spread = max(ms["operators"]) - min(ms["operators"])
    diff = base - new
    verdict = "a gain by the stated rule" if diff > spread else ("a loss by the stated rule" if -diff > spread else "no difference by the stated rule")
    lines += ["", f"(a) - (b) = {diff:+.4f} ms / forward ({100 * diff / base:+.1f} %, x{base / new:.2f}) against a spread of (a)'s own windows of {spread:.4f}: {verdict}.", ""]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
