"""Times one training step of a model whose dynamics network is the EGNN (bio-diffusion_amd/egnn_dynamics.py) -- training_step, backward and the
fused update of configure_optimizers() -- with the network's training path on "operators" (the reference's formulation on the autograd
operators, the [E, D] concatenation included) against "fused" (ops.egnn_edge_block per layer, include/gcdm_egnn_train.h), in alternating windows
of one job, and records the result.

Workloads: "qm9" = 64 molecules of 19 atoms (1 216 atoms, 23 104 edges), "geom" = 32 molecules of 44 atoms (1 408 atoms, 61 952 edges); both
H = 256, L = 9, seeded weights, fixed t and noise; Eh = 64 (qm9) / 16 (geom) as the GCPNet configurations of the two data sets.  Time: device
events around a window of at least `--seconds` after warm-up.  "operators" is the baseline: the spread of its own windows stands beside the
difference, and a gain is claimed only if the difference exceeds it.

One case per process, so that each GPU step runs under its own time limit:

    timeout -k 10 600 python tools/egnn_train_probe.py --case qm9 && timeout -k 10 600 python tools/egnn_train_probe.py --case geom --append
"""
import argparse
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from egnn_dynamics_probe import window          # noqa: E402

CASES = {"qm9": dict(dataset="qm9", model="QM9MoleculeGenerationDDPM", molecules=64, atoms=19, Eh=64),
         "geom": dict(dataset="geom", model="GEOMMoleculeGenerationDDPM", molecules=32, atoms=44, Eh=16)}
H, L = 256, 9
VARIANTS = (("operators", "(a) operators: cat + ops.linear"), ("fused", "(b) fused: ops.egnn_edge_block"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), required=True)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "egnn_train_probe.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("egnn_train_probe needs an MI355X: a CPU run measures nothing")
    pkg = importlib.import_module("bio-diffusion_amd")
    dev = torch.device("cuda:0")
    c = CASES[args.case]
    cfgs = pkg.default_cfgs(c["dataset"])
    cfgs["diffusion_cfg"]["dynamics_network"] = "egnn"
    cfgs["model_cfg"].update(num_encoder_layers=L, h_hidden_dim=H, e_hidden_dim=c["Eh"])
    torch.manual_seed(11)
    model = getattr(pkg, c["model"])(**cfgs).to(dev).train()
    dyn = model.ddpm.dynamics_network
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    upd = model.configure_optimizers()
    g = torch.Generator().manual_seed(12)
    sizes = [c["atoms"]] * c["molecules"]
    N, B, T = sum(sizes), len(sizes), dyn.num_atom_types
    bi = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    data = dict(x=1.5 * torch.randn(N, 3, generator=g), one_hot=torch.nn.functional.one_hot(torch.randint(0, T, (N,), generator=g), T).float(),
                charges=torch.randint(1, 9, (N,), generator=g).float(), batch=bi, mask=torch.ones(N, dtype=torch.bool))
    data = {k: v.to(dev) for k, v in data.items()}
    t_int = torch.randint(1, 1000, (B, 1), generator=g).to(dev)
    noise = [torch.randn(N, 3 + T + int(dyn.include_charges), generator=g).to(dev)]
    last = {}

    def step():
        upd.zero_grad()
        loss = model.training_step(pkg.AttrDict(num_graphs=B, **data), t_int=t_int, noise=noise)["loss"]
        loss.backward()
        upd.step()
        last["loss"] = loss.detach()

    first = {}
    for mode, _ in VARIANTS:                       # warm-up of both paths from the same weights: code objects, the plan, the update's state
        model.load_state_dict(start)
        dyn.set_train_path(mode)
        step()
        first[mode] = float(last["loss"])
        step()
    torch.cuda.synchronize()
    ms = {mode: [] for mode, _ in VARIANTS}
    rows = []
    for w in range(args.windows):
        for mode, label in VARIANTS:
            dyn.set_train_path(mode)
            torch.cuda.synchronize()
            tm, calls = window(step, args.seconds)
            ms[mode].append(tm)
            rows.append(f"{label:<40}{w:>6}{calls:>8}{tm:>12.4f}")
    E = sum(n * n for n in sizes)
    lines = [f"egnn_train_probe [{args.case}]: one training step (training_step, backward, fused update) of an EGNN model, {c['molecules']} molecules of "
             f"{c['atoms']} atoms ({N} atoms, {E} edges),",
             f"H = {H}, Eh = {c['Eh']}, L = {L}, {torch.cuda.get_device_name(0)}.  Windows of at least {args.seconds} s, the two paths alternating.",
             f"loss of the first step from the same weights: operators {first['operators']:.9g}, fused {first['fused']:.9g}; loss after the last window "
             f"{float(last['loss']):.6g}.", "",
             f"{'path':<40}{'window':>6}{'calls':>8}{'ms / call':>12}"] + rows + [""]
    for mode, label in VARIANTS:
        v = ms[mode]
        lines.append(f"{label:<40} median {statistics.median(v):.4f} ms / step, windows {min(v):.4f} .. {max(v):.4f}, spread {max(v) - min(v):.4f}")
    base, new = statistics.median(ms["operators"]), statistics.median(ms["fused"])
    spread = max(ms["operators"]) - min(ms["operators"])
    diff = base - new
    verdict = "a gain by the stated rule" if diff > spread else ("a loss by the stated rule" if -diff > spread else "no difference by the stated rule")
    lines += ["", f"(a) - (b) = {diff:+.4f} ms / step ({100 * diff / base:+.1f} %, x{base / new:.2f}) against a spread of (a)'s own windows of {spread:.4f}: {verdict}.", ""]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
