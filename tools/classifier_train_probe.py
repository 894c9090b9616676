"""Times one training step of the EGNN property classifier on the "operators" path -- forward, backward and an Adam step -- with the first
per-edge layer split by columns ("split", ops.classifier_edge_pre) against the reference's formulation on torch.cat ("concat"), in alternating
windows of one job, and records the result.

Workload: the batch shape of tools/classifier_probe.py -- 100 molecules, sizes from the QM9 histogram (fixed seed), H = 128, L = 7, attention
on -- trained against seeded N(0, 1) targets with the L1 loss of train_epoch.  Both variants start every window from the same weights and
optimiser state, so a window times the same arithmetic each time.  Time: device events around a window of at least `--seconds` after warm-up.
"concat" is the baseline: the spread of its own windows stands beside the difference, and a gain is claimed only if the difference exceeds it.

    python tools/classifier_train_probe.py [--windows 5] [--seconds 1.0] [--out profiles/classifier_train_probe.txt]
"""
import argparse
import copy
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import classifier_ref as cr          # noqa: E402
import synth                         # noqa: E402

F, H, L = 5, 128, 7
MOLECULES = 100
VARIANTS = (("concat", "(a) concat: torch.cat + ops.linear"), ("split", "(b) split: ops.classifier_edge_pre"))


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
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classifier_train_probe.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("classifier_train_probe needs an MI355X: a CPU run measures nothing")
    pkg = importlib.import_module("bio-diffusion_amd")
    dev = torch.device("cuda:0")
    W = synth.make_weights(cr.state_dict_shapes(F, H, L, True, False), seed=11)
    sizes = cr.qm9_sizes(MOLECULES, seed=1)
    x, h0 = cr.make_batch(sizes, F, seed=100)
    x, h0, nn_ = x.to(dev), h0.to(dev), torch.tensor(sizes)
    target = torch.randn(MOLECULES, generator=torch.Generator().manual_seed(5)).to(dev)
    model = pkg.EGNN(in_node_nf=F, in_edge_nf=0, hidden_nf=H, device=dev, n_layers=L, attention=1, node_attr=0)
    model.load_state_dict(W)
    model.train().set_path("operators")
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)

    def step():
        opt.zero_grad()
        loss = (model.predict(x, h0, num_nodes=nn_) - target).abs().mean()
        loss.backward()
        opt.step()
        return loss

    # warm-up of both variants (code objects, the edge tables, Adam's state), then the state every window starts from
    first = {}
    for mode, _ in VARIANTS:
        model.load_state_dict(W)
        model.set_edge_input(mode)
        first[mode] = float(step().detach())
        step()
    model.load_state_dict(W)
    state0 = copy.deepcopy(opt.state_dict())

    ms = {mode: [] for mode, _ in VARIANTS}
    rows = []
    for w in range(args.windows):
        for mode, label in VARIANTS:
            model.load_state_dict(W)
            opt.load_state_dict(copy.deepcopy(state0))
            model.set_edge_input(mode)
            torch.cuda.synchronize()
            t, calls = window(step, args.seconds)
            ms[mode].append(t)
            rows.append(f"{label:<40}{w:>6}{calls:>8}{t:>12.4f}")
    atoms, edges = sum(sizes), sum(n * (n - 1) for n in sizes)
    lines = [f"classifier_train_probe: one training step (forward + backward + Adam) of the EGNN classifier on the operators path, {MOLECULES} molecules",
             f"(QM9 histogram, seed 1; {atoms} atoms, {edges} edges), H = {H}, L = {L}, attention on, {torch.cuda.get_device_name(0)}.",
             f"Windows of at least {args.seconds} s, the two variants alternating; each window restarts from the same weights and Adam state.",
             f"First loss of the warm-up: concat {first['concat']:.7f}, split {first['split']:.7f}.", "",
             f"{'variant':<40}{'window':>6}{'steps':>8}{'ms / step':>12}"] + rows + [""]
    for mode, label in VARIANTS:
        v = ms[mode]
        lines.append(f"{label:<40} median {statistics.median(v):.4f} ms / step, windows {min(v):.4f} .. {max(v):.4f}, spread {max(v) - min(v):.4f}")
    base, new = statistics.median(ms["concat"]), statistics.median(ms["split"])
    spread = max(ms["concat"]) - min(ms["concat"])
    diff = base - new
    verdict = "a gain by the stated rule" if diff > spread else ("a loss by the stated rule" if -diff > spread else "no difference by the stated rule")
    lines += ["", f"(a) - (b) = {diff:+.4f} ms / step ({100 * diff / base:+.1f} %) against a spread of (a)'s own windows of {spread:.4f}: {verdict}."]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
