"""Bits of every sampling driver, one line per case: case name, sha256 of every returned tensor, last_flags / last_range_rewinds /
last_range_resume_step, and the texts of the warnings and log records the call raised.  Run it from the root of two checkouts on the same GPU
and compare the tables (the last line is the sha256 of the table itself):

    python tools/sampler_driver_bits.py > table.txt

The package is imported from the current directory, so one copy of this script serves both checkouts."""
import hashlib
import importlib
import logging
import os
import sys
import warnings

import torch

sys.path.insert(0, os.getcwd())
pkg = importlib.import_module("bio-diffusion_amd")
F16 = pkg._native.FLAG_F16_RANGE
DEV = "cuda"
LINES = []


class _Records(logging.Handler):
    def __init__(self):
        super().__init__(logging.WARNING)
        self.texts = []

    def emit(self, record):
        self.texts.append(record.getMessage())


def digest(obj) -> str:
    if isinstance(obj, torch.Tensor):
        t = obj.detach().cpu().contiguous()
        return hashlib.sha256(repr((str(t.dtype), tuple(t.shape))).encode() + t.view(torch.uint8).numpy().tobytes()).hexdigest()[:16]
    if isinstance(obj, (list, tuple)):
        return "[" + " ".join(digest(o) for o in obj) + "]"
    if isinstance(obj, dict):
        return hashlib.sha256(repr(sorted((k, repr(v)) for k, v in obj.items())).encode()).hexdigest()[:16]
    return repr(obj)


def case(name, ddpm, fn, counts_if=None):
    """One table line.  ``counts_if(ddpm)``: the condition under which the case exercises what it is meant to (printed as ``counts=``)."""
    rec = _Records()
    root = logging.getLogger()
    root.addHandler(rec)
    ddpm.last_flags, ddpm.last_range_rewinds, ddpm.last_range_resume_step = 0, 0, None
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        try:
            out = digest(fn())
        except (ValueError, NotImplementedError, AssertionError, pkg.F16RangeError) as e:     # a refusal is behaviour too: type and text go into the table
            out = f"{type(e).__name__}: {e}"
    root.removeHandler(rec)
    torch.cuda.synchronize()
    state = f"flags={ddpm.last_flags} rewinds={ddpm.last_range_rewinds} resume={ddpm.last_range_resume_step}"
    extra = "" if counts_if is None else f" counts={bool(counts_if(ddpm))}"
    line = f"{name} | {out} | {state}{extra} | logs={rec.texts + [str(w.message) for w in caught]}"
    LINES.append(line)
    print(line, flush=True)


def build(conditioning=(), self_condition=False):
    cfgs = pkg.default_cfgs("qm9", conditioning)
    cfgs["diffusion_cfg"]["self_condition"] = self_condition
    torch.manual_seed(0)
    model = pkg.QM9MoleculeGenerationDDPM(**cfgs)
    with torch.no_grad():
        for p in model.ddpm.dynamics_network.parameters():
            if p.dim() == 2:
                p.mul_(0.25)
    return model.cuda().eval()


def tape(N, D, count, seed):
    g = torch.Generator().manual_seed(seed)
    draws = [torch.randn((N, D), generator=g).to(DEV) for _ in range(count)]
    return lambda k: draws[k]


def main():
    T = 6
    nn4 = torch.tensor([7, 19, 4, 12])
    nn5 = torch.tensor([3, 19, 8, 11, 5])
    lists = [torch.tensor([7, 19, 4, 12]), torch.tensor([3, 9, 16]), torch.tensor([5, 18, 6, 11, 13])]
    N4 = int(nn4.sum())

    model = build()
    ddpm, dyn = model.ddpm, model.ddpm.dynamics_network
    D = ddpm.num_x_dims + ddpm.num_node_scalar_features
    sample = lambda nn_=nn4, **kw: ddpm.mol_gen_sample(num_samples=len(nn_), num_nodes=nn_, device=DEV, **kw)          # noqa: E731
    case("sample_philox", ddpm, lambda: sample(num_timesteps=T, seed=5))
    case("sample_tape", ddpm, lambda: sample(num_timesteps=T, noise_fn=tape(N4, D, T + 2, 1)))
    case("sample_frames3", ddpm, lambda: sample(num_timesteps=T, seed=5, return_frames=3))
    case("sample_frames3_tape", ddpm, lambda: sample(num_timesteps=T, return_frames=3, noise_fn=tape(N4, D, T + 2, 2)))
    case("sample_fix_noise", ddpm, lambda: sample(num_timesteps=T, seed=5, fix_noise=True))
    case("sample_lanes2", ddpm, lambda: sample(num_timesteps=T, seed=5, lanes=2))
    case("sample_T60_clean", ddpm, lambda: sample(nn5, num_timesteps=60, seed=11))

    def poke(s, z):
        if s == 20:
            z[1, 5] = 3.0e8
    case("sample_T60_poked", ddpm, lambda: sample(nn5, num_timesteps=60, seed=11, step_callback=poke),
         counts_if=lambda d: d.last_flags & F16 and d.last_range_rewinds == 1)
    dyn.set_mfma_mode(0)
    case("sample_T60_poked_fp32", ddpm, lambda: sample(nn5, num_timesteps=60, seed=11, step_callback=poke))
    dyn.set_mfma_mode(1)
    mask = torch.ones(N4, dtype=torch.bool, device=DEV)
    mask[9] = False
    case("sample_masked", ddpm, lambda: sample(num_timesteps=T, seed=5, node_mask=mask))
    dyn.path = "modules"
    case("sample_modules", ddpm, lambda: sample(num_timesteps=T, seed=5))
    case("sample_modules_tape_frames2", ddpm, lambda: sample(num_timesteps=T, return_frames=2, noise_fn=tape(N4, D, T + 2, 3)))
    dyn.path = "auto"

    # inpainting (the QM9 model has charges)
    g = torch.Generator().manual_seed(21)
    x = (torch.randn((N4, 3), generator=g) * 1.5 + torch.tensor([0.3, -2.0, 1.0])).to(DEV)
    oh = torch.nn.functional.one_hot(torch.randint(0, ddpm.num_atom_types, (N4,), generator=g), ddpm.num_atom_types).float().to(DEV)
    ch = torch.randint(0, 9, (N4, 1), generator=g).float().to(DEV)
    fixed = (torch.rand(N4, generator=g) < 0.4).to(DEV)
    fixed[0] = True
    mol = dict(x=x, one_hot=oh, charges=ch, num_nodes=nn4)
    inpaint = lambda m=mol, **kw: ddpm.inpaint(m, fixed, num_timesteps=T, seed=9, **kw)                                  # noqa: E731
    for r, j in ((1, 1), (2, 1), (2, 2)):
        case(f"inpaint_r{r}_j{j}", ddpm, lambda: inpaint(num_resamplings=r, jump_length=j))
    case("inpaint_frames3", ddpm, lambda: inpaint(num_resamplings=2, jump_length=1, return_frames=3))
    case("inpaint_tape", ddpm, lambda: ddpm.inpaint(mol, fixed, num_resamplings=2, jump_length=2, num_timesteps=T, noise_fn=tape(N4, D, 64, 4)))
    for scale in (1e7, 3e9):
        case(f"inpaint_range_{scale:g}", ddpm, lambda: inpaint(dict(mol, one_hot=oh * scale), num_resamplings=1), counts_if=lambda d: d.last_flags & F16)
    dyn.path = "modules"
    case("inpaint_modules", ddpm, lambda: inpaint(num_resamplings=2, jump_length=2))
    dyn.path = "auto"

    # several batches at once
    for name, fn in (("concurrent", ddpm.mol_gen_sample_concurrent), ("packed", ddpm.mol_gen_sample_packed)):
        case(f"{name}_default_seeds", ddpm, lambda: fn(lists, DEV, num_timesteps=T))
        case(f"{name}_seeds", ddpm, lambda: fn(lists, DEV, num_timesteps=T, seeds=[77, 78, 79]))
        ddpm.release_lanes()
    for kw in (dict(concurrent_batches=3), dict(packed_batches=3)):
        torch.manual_seed(3)
        case(f"sample_and_analyze_{next(iter(kw))}", ddpm, lambda: model.sample_and_analyze(num_samples=36, batch_size=12, num_timesteps=T, **kw))
        ddpm.release_lanes()

    # the conditional model (no charges): context, the optimisation loop, and a context far outside the f16 range for the several-batches drivers
    cm = build(("alpha",))
    cd = cm.ddpm
    gq = torch.Generator().manual_seed(9)
    ctx = torch.randn((len(nn4), 1), generator=gq).to(DEV)
    ctxs = [torch.randn((len(s), 1), generator=gq).to(DEV) for s in lists]
    case("cond_sample", cd, lambda: cd.mol_gen_sample(num_samples=len(nn4), num_nodes=nn4, device=DEV, num_timesteps=T, seed=5, context=ctx))
    case("cond_sample_no_context", cd, lambda: cd.mol_gen_sample(num_samples=len(nn4), num_nodes=nn4, device=DEV, num_timesteps=T, seed=5))
    samples = []
    for n in nn4.tolist():
        xs = torch.randn((n, 3), generator=gq) * 1.2
        hs = torch.nn.functional.one_hot(torch.randint(0, cd.num_atom_types, (n,), generator=gq), cd.num_atom_types).float()
        samples.append(((xs - xs.mean(0, keepdim=True)).to(DEV), hs.to(DEV)))
    for frames in (1, 2):
        case(f"cond_optimize_frames{frames}", cd, lambda: cd.mol_gen_optimize(samples=samples, num_nodes=nn4, device=DEV, num_timesteps=T, context=ctx,
                                                                           return_frames=frames, seed=5))
    for name, fn in (("concurrent", cd.mol_gen_sample_concurrent), ("packed", cd.mol_gen_sample_packed)):
        case(f"cond_{name}", cd, lambda: fn(lists, DEV, num_timesteps=T, contexts=ctxs, seeds=[77, 78, 79]))
        case(f"cond_{name}_no_context", cd, lambda: fn(lists, DEV, num_timesteps=T))
        huge = [ctxs[0], ctxs[1] * 3.0e8, ctxs[2]]
        case(f"cond_{name}_huge_context", cd, lambda: fn(lists, DEV, num_timesteps=T, contexts=huge, seeds=[77, 78, 79]), counts_if=lambda d: d.last_flags & F16)
        cd.release_lanes()

    # the self-conditioned model
    sm = build(self_condition=True)
    sd = sm.ddpm
    case("selfcond_sample", sd, lambda: sd.mol_gen_sample(num_samples=len(nn4), num_nodes=nn4, device=DEV, num_timesteps=T, seed=5))
    case("selfcond_sample_tape", sd, lambda: sd.mol_gen_sample(num_samples=len(nn4), num_nodes=nn4, device=DEV, num_timesteps=T,
                                                                noise_fn=tape(N4, D, 2 * T + 2, 6)))
    case("selfcond_inpaint", sd, lambda: sd.inpaint(mol, fixed, num_resamplings=2, jump_length=2, num_timesteps=T, seed=9))
    case("selfcond_packed", sd, lambda: sd.mol_gen_sample_packed(lists, DEV, num_timesteps=T))
    print("table sha256", hashlib.sha256("\n".join(LINES).encode()).hexdigest())


if __name__ == "__main__":
    main()
