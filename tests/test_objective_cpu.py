"""tests/objective_ref.py -- the restatement the GPU tests of the fused diffusion objective (include/gcdm_objective.h) measure against -- held
to three sources on the CPU: the reference's own training terms and loss (tests/golden/train_full_{qm9,geom}.npz, under the bars of
test_training_loss_and_gradients_match_reference_autograd), oracle.gcdm_oracle.nll_terms in evaluation mode, and the package's own
EquivariantVariationalDiffusion._loss_terms, which runs on CPU tensors once the dynamics network is replaced by a stub that returns a fixed
net_out (everything else in it is plain torch).  The closed-form d net_out of the kernel is checked against autograd through the restatement,
and each of objective_ref.MUTANTS, applied to the fp32 run, is shown to be rejected by the bar of tests/test_objective_cabi_gpu.py."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import objective_ref as R  # noqa: E402
import synth  # noqa: E402
from oracle import gcdm_oracle as O  # noqa: E402

pkg = importlib.import_module("bio-diffusion_amd")
assert hasattr(pkg.ops, "diffusion_objective") and hasattr(pkg.EquivariantVariationalDiffusion, "set_objective_path")
TRAIN_TERMS = ("delta_log_px", "error_t", "SNR_weight", "loss_0_x", "loss_0_h", "neg_log_constants", "kl_prior", "log_pN")


def _ddpm(case, net=None, **diffusion):
    cfgs = pkg.default_cfgs(case)
    cfgs["diffusion_cfg"].update(diffusion)
    ds = pkg.dataset_info(case)
    return pkg.EquivariantVariationalDiffusion(net if net is not None else torch.nn.Identity(), cfgs["diffusion_cfg"], cfgs["dataloader_cfg"], ds), cfgs


def _tables(ddpm):
    nd = ddpm.num_nodes_distribution
    tab = torch.full((max(nd.keys) + 2,), float("nan"))
    tab[nd.num_nodes] = torch.log(nd.prob + nd.eps)
    nv, nb = ddpm.diffusion_cfg["norm_values"], ddpm.diffusion_cfg["norm_biases"]
    return ddpm.gamma.gamma.detach().clone(), tab, [float(v) for v in nv], [0.0 if v is None else float(v) for v in nb]


def make_inputs(case, num_nodes, t_int, mode, seed=0, mask=None, center_x=False, ddpm=None):
    """One input dictionary of objective_ref.prepare: data-like x / one-hot / charges, raw draws from a seeded generator."""
    d = synth.DATASET_DIMS[case]
    ddpm = ddpm if ddpm is not None else _ddpm(case)[0]
    gamma, tab, nv, nb = _tables(ddpm)
    g = torch.Generator().manual_seed(seed)
    off = R.offsets_of(num_nodes)
    N, nf, ic = int(off[-1]), d["num_atom_types"], int(d["include_charges"])
    D = 3 + nf + ic
    x = torch.randn((N, 3), generator=g)
    if not center_x:
        bi = R._bi(off)
        m = torch.ones(N) if mask is None else (mask != 0).float()
        x = x - (R._seg(x, bi, len(off) - 1) / R._seg(m, bi, len(off) - 1).unsqueeze(-1))[bi] * m.unsqueeze(-1)
    types = torch.randint(0, nf, (N,), generator=g)
    return dict(x=x, one_hot=torch.nn.functional.one_hot(types, nf).float(), charges=torch.randint(1, 10, (N,), generator=g).float() if ic else None,
                mask=mask, off=off, t_int=torch.as_tensor(t_int, dtype=torch.int32), gamma=gamma, log_pn=tab, nv=nv, nb=nb,
                eps_raw=torch.randn((N, D), generator=g), eps_raw_0=torch.randn((N, D), generator=g) if mode == R.EVAL else None, nf=nf, ic=ic,
                T=ddpm.T, mode=mode, center_x=center_x)


@pytest.mark.parametrize("case", ["qm9", "geom"])
def test_restatement_matches_the_references_training_terms(case, golden_dir):
    g = np.load(os.path.join(golden_dir, f"train_full_{case}.npz"), allow_pickle=False)
    d = synth.DATASET_DIMS[case]
    ddpm, _ = _ddpm(case)
    gamma, tab, nv, nb = _tables(ddpm)
    shapes = synth.dynamics_shapes(d["S"], d["V"], d["Se"], d["Ve"], d["L"], synth.dims_h_in(d))
    W = synth.make_weights(shapes, seed=int(g["weight_seed"]), scale_2d=float(g["weight_scale"]))
    ocfg = O.OracleConfig(num_atom_types=d["num_atom_types"], include_charges=d["include_charges"], num_context=d["n_ctx"], num_layers=d["L"],
                          norm_values=d["norm_values"])
    nn_ = torch.tensor(g["num_nodes"])
    off, bi = R.offsets_of(nn_), O.num_nodes_to_batch_index(nn_)
    N, F = int(nn_.sum()), synth.dims_feat(d)
    tape = O.TapeNoise(int(g["noise_seed"]))
    raw = torch.cat((tape(N, 3), tape(N, F)), dim=-1)
    nf, ic = d["num_atom_types"], int(d["include_charges"])
    inp = dict(x=torch.tensor(g["x"]), one_hot=torch.tensor(g["one_hot"]), charges=torch.tensor(g["charges"]), mask=None, off=off,
               t_int=torch.tensor(g["t_int"]).int(), gamma=gamma, log_pn=tab, nv=nv, nb=nb, eps_raw=raw, eps_raw_0=None, nf=nf, ic=ic, T=ddpm.T,
               mode=R.TRAIN_L2, center_x=False)
    assert (inp["t_int"] == 0).any()
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        prep, _ = R.prepare(**inp, dtype=dtype)
        with torch.no_grad():
            net = O.dynamics_forward({k: v.to(dtype) for k, v in W.items()}, ocfg, prep["z_t"], prep["t_node"].reshape(-1, 1), bi)
        tr, _ = R.terms(net, None, prep, None, off, gamma, nv, nb, nf, ic, ddpm.T, R.TRAIN_L2, dtype)
        nll, means, _, _ = R.reduce(prep["mol"], tr, 3 + nf + ic, ddpm.T, R.TRAIN_L2, False, dtype)
        for i, name in enumerate(TRAIN_TERMS):
            w32, w64 = torch.tensor(g[f"{name}_32"]).double(), torch.tensor(g[f"{name}_64"]).double()
            bar = 4 * (w32 - w64).abs() + 1e-4 * w64.abs().clamp(min=1.0)
            assert ((tr[:, i].double() - w64).abs() <= bar).all(), (name, tag)
        l32, l64 = float(g["loss_32"]), float(g["loss_64"])
        assert abs(float(means[0]) - l64) <= 4 * abs(l32 - l64) + 1e-4 * abs(l64), (tag, float(means[0]), l64)
        assert (nll.double() - torch.tensor(g["nll_64"]).double()).abs().max().item() <= 4 * np.abs(g["nll_32"] - g["nll_64"]).max() + 1e-4 * np.abs(g["nll_64"]).max()


def test_restatement_matches_the_oracles_evaluation_terms():
    d = synth.DATASET_DIMS["qm9"]
    ddpm, _ = _ddpm("qm9")
    nn_ = torch.tensor([3, 5, 2])
    inp = make_inputs("qm9", nn_, [1, 700, 1000], R.EVAL, seed=3, ddpm=ddpm)
    W = synth.make_weights(synth.dynamics_shapes(d["S"], d["V"], d["Se"], d["Ve"], d["L"], synth.dims_h_in(d)), seed=3, scale_2d=0.5)
    W = {k: v.double() for k, v in W.items()}
    ocfg = O.OracleConfig(num_atom_types=d["num_atom_types"], include_charges=d["include_charges"], num_context=d["n_ctx"], num_layers=d["L"],
                          norm_values=d["norm_values"])
    draws = [inp["eps_raw"][:, :3], inp["eps_raw"][:, 3:], inp["eps_raw_0"][:, :3], inp["eps_raw_0"][:, 3:]]
    noise = lambda n, k, dtype=torch.float32: draws.pop(0).to(dtype)          # noqa: E731
    with torch.no_grad():
        want = O.nll_terms(W, ocfg, inp["x"], inp["one_hot"], inp["charges"], nn_, inp["t_int"].long(), noise, dtype=torch.float64)
        prep, _ = R.prepare(**inp, dtype=torch.float64)
        bi = O.num_nodes_to_batch_index(nn_)
        net = O.dynamics_forward(W, ocfg, prep["z_t"], prep["t_node"].reshape(-1, 1), bi)
        net0 = O.dynamics_forward(W, ocfg, prep["z_0"], torch.zeros(len(bi), 1, dtype=torch.float64), bi)
    tr, _ = R.terms(net, net0, prep, None, inp["off"], inp["gamma"], inp["nv"], inp["nb"], inp["nf"], inp["ic"], ddpm.T, R.EVAL)
    _, means, _, _ = R.reduce(prep["mol"], tr, 3 + inp["nf"] + inp["ic"], ddpm.T, R.EVAL, False)
    for i, name in enumerate(R.TERMS[:7]):
        assert (tr[:, i] - want[name]).abs().max().item() <= 1e-9 * max(1.0, want[name].abs().max().item()), name
    for k, name in ((8, "eps_hat_x"), (9, "eps_hat_h")):
        assert abs(float(means[k]) - float(want[name])) <= 1e-9


class _Stub(torch.nn.Module):
    """A dynamics network that returns what it is told to: the rest of _loss_terms is plain torch and runs on CPU tensors."""

    def __init__(self, outs):
        super().__init__()
        self.outs = list(outs)

    def forward(self, batch, z, t, **kw):
        return None, self.outs.pop(0)


@pytest.mark.parametrize("case,mode,by_max", [("qm9", R.TRAIN_L2, False), ("qm9", R.TRAIN_L2, True), ("qm9", R.TRAIN_VLB, False), ("qm9", R.EVAL, False),
                                              ("geom", R.TRAIN_L2, False), ("geom", R.EVAL, False), ("qm9", R.TRAIN_VLB, True), ("geom", R.TRAIN_VLB, True)])
def test_restatement_matches_the_packages_own_loss_terms_on_cpu_tensors(case, mode, by_max):
    """_loss_terms + the tail of _forward_impl in fp32 on the CPU (a stub network) against the fp32 restatement: 2e-5 relative, and the
    restatement's fp64 run within the same of both.  A mask with absent nodes; t_int holds 0, 1 and T."""
    ddpm, cfgs = _ddpm(case, loss_type="vlb" if mode == R.TRAIN_VLB else "l2", norm_training_by_max_nodes=by_max)
    nn_ = torch.tensor([5, 3, 9, 4])
    N = int(nn_.sum())
    mask = torch.ones(N, dtype=torch.bool)
    mask[[1, 9, 11]] = False
    t_int = [0, 1, ddpm.T, 431] if mode != R.EVAL else [1, 2, ddpm.T, 431]
    inp = make_inputs(case, nn_, t_int, mode, seed=11, mask=mask, ddpm=ddpm)
    D = 3 + inp["nf"] + inp["ic"]
    g = torch.Generator().manual_seed(5)
    keep = torch.ones(N, D)          # as the real network on masked rows: x columns zero, the other columns not (gcpnet.py:1190)
    keep[:, :3] = mask.float().unsqueeze(-1)
    net = torch.randn((N, D), generator=g) * keep
    net0 = torch.randn((N, D), generator=g) * keep if mode == R.EVAL else None
    ddpm.dynamics_network = _Stub([net] if net0 is None else [net, net0])
    ddpm.train(mode != R.EVAL)
    bi = R._bi(inp["off"])
    cnt = R._seg(mask.long(), bi, len(nn_))
    batch = pkg.config.AttrDict(x=inp["x"], h={"categorical": inp["one_hot"], "integer": inp["charges"] if inp["ic"] else torch.zeros(N)}, batch=bi,
                                mask=mask, num_graphs=len(nn_), num_nodes_present=cnt, props_context=None)
    out = ddpm(batch, return_loss_info=True, t_int=inp["t_int"].long().view(-1, 1), noise=[inp["eps_raw"], inp["eps_raw_0"]])
    r32, _ = R.run(inp, net, net0, by_max, torch.float32)
    r64, _ = R.run(inp, net, net0, by_max, torch.float64)
    over_unmasked, _ = R.run(inp, net * mask.float().unsqueeze(-1), net0, by_max, torch.float64)
    moved = (r64["terms"][:, 1] - over_unmasked["terms"][:, 1]).abs()
    assert moved.max().item() > 1e-2 * r64["terms"][:, 1].abs().max().item(), "the masked rows must carry weight in error_t"
    for i, name in enumerate(TRAIN_TERMS):
        for r in (r32, r64):
            err = (out[i].detach().double() - r["terms"][:, i].double()).abs().max().item()
            assert err <= 2e-5 * max(1.0, r64["terms"][:, i].abs().max().item()), (name, err)
    # the tail of _MoleculeGenerationDDPM._forward_impl
    T, (dl, et, sw, l0x, l0h, nlc, kl, lpn) = ddpm.T, [o.detach() for o in out[:8]]
    if mode == R.TRAIN_L2:
        den = D * (cnt.max() if by_max else cnt)
        nll = 0.5 * (et / den) + (l0x / den + l0h) + kl - dl - lpn
    else:
        nll = T * 0.5 * sw * et + (l0x + l0h + nlc) + kl - dl - lpn
    assert (nll.double() - r64["nll"]).abs().max().item() <= 2e-5 * r64["nll"].abs().max().item()
    assert abs(float(nll.mean()) - float(r64["means"][0])) <= 2e-5 * abs(float(r64["means"][0]))
    for k, name in ((8, "eps_hat_x"), (9, "eps_hat_h")):
        assert abs(float(out[9][name]) - float(r64["means"][k])) <= 2e-5


@pytest.mark.parametrize("mode,by_max", [(R.TRAIN_L2, True), (R.TRAIN_L2, False), (R.TRAIN_VLB, False)])
def test_closed_form_gradient_equals_autograd_through_the_restatement(mode, by_max):
    nn_ = torch.tensor([5, 3, 9, 4])
    N = int(nn_.sum())
    mask = torch.ones(N, dtype=torch.bool)
    mask[[1, 9, 11]] = False
    inp = make_inputs("qm9", nn_, [0, 1, 1000, 431], mode, seed=2, mask=mask)
    D = 3 + inp["nf"] + inp["ic"]
    net = torch.randn((N, D), generator=torch.Generator().manual_seed(1), dtype=torch.float64).requires_grad_(True)
    prep, _ = R.prepare(**inp)
    tr, _ = R.terms(net, None, prep, mask, inp["off"], inp["gamma"], inp["nv"], inp["nb"], inp["nf"], inp["ic"], inp["T"], mode)
    nll, means, coef, _ = R.reduce(prep["mol"], tr, D, inp["T"], mode, by_max)
    B = len(nn_)
    g = torch.Generator().manual_seed(9)
    ge, g0, gn = (torch.randn(B, generator=g, dtype=torch.float64) for _ in range(3))
    gl = torch.randn((), generator=g, dtype=torch.float64)
    ((tr[:, 1] * ge).sum() + (tr[:, 3] * g0).sum() + (nll * gn).sum() + means[0] * gl).backward()
    want = R.bwd(ge, g0, gn, gl, net.detach(), prep["eps_t"], mask, inp["off"], prep["mol"], coef.detach())
    assert (net.grad - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    # masked rows carry the error_t part (the reference sums error_t over all rows), never the loss_0_x part
    t0 = prep["mol"][:, 4][R._bi(inp["off"])]
    assert (want[~mask][t0[~mask] == 1] == 0).all() and want[~mask].abs().max().item() > 0 and want[mask].abs().max().item() > 0


def _mutant_case(mutant):
    """Inputs on which the wrong reading shows: a t = 0 molecule, absent nodes with noise on them, sizes that differ."""
    mode = {"denominator_without_max_nodes": R.TRAIN_L2, "integer_mass_ignores_mask": R.EVAL, "epsilon_inside_erf": R.EVAL}.get(mutant, R.TRAIN_VLB)
    nn_ = torch.tensor([5, 3, 9, 4])
    N = int(nn_.sum())
    mask = torch.ones(N, dtype=torch.bool)
    mask[[1, 9, 11]] = False
    inp = make_inputs("qm9", nn_, [0, 1, 1000, 431] if mode != R.EVAL else [1, 2, 1000, 431], mode, seed=4, mask=mask)
    # a schedule whose sigma at t = 0 is wide enough for the masses to differ from 0 and 1 (the entries take any gamma table)
    # -- but the data set's own narrow one where the epsilon is what keeps the log finite
    if mutant != "epsilon_inside_erf":
        inp["gamma"] = torch.linspace(-2.5, 7.0, inp["T"] + 1)
    g = torch.Generator().manual_seed(6)
    net = torch.randn((N, 3 + inp["nf"] + inp["ic"]), generator=g)
    return inp, net, (torch.randn(net.shape, generator=g) if mode == R.EVAL else None)


def _rejected(inp, net, net0, mutant):
    r32, _ = R.run(inp, net, net0, True, torch.float32)
    r64, mag = R.run(inp, net, net0, True, torch.float64)
    got, _ = R.run(inp, net, net0, True, torch.float32, mutant=mutant)
    checks = [(got["prep"][k], r32["prep"][k], r64["prep"][k], mag["prep"][k]) for k in ("eps_t", "z_t", "mol")]
    checks += [(got[k], r32[k], r64[k], mag[k]) for k in ("terms", "nll", "means")]
    return [not R.bar_ok(*c)[0] for c in checks]


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_bar_rejects_each_mutant_of_the_fp32_emulation(mutant):
    inp, net, net0 = _mutant_case(mutant)
    assert not any(_rejected(inp, net, net0, None)), "the unmutated fp32 run must pass its own bar"
    assert any(_rejected(inp, net, net0, mutant)), mutant


class _Recorder(torch.nn.Module):
    """A stub network with one parameter that records what it is called with."""

    def __init__(self, N, D):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(()))
        self.calls, self.N, self.D = [], N, D

    def forward(self, batch, z, t, **kw):
        self.calls.append(dict(z=z, t=t, grad=torch.is_grad_enabled(), **kw))
        return None, self.w * torch.full((self.N, self.D), 0.25)


@pytest.mark.parametrize("entries", [3, 1, 0])
def test_three_entry_noise_list_reaches_both_self_conditioning_draws(entries, monkeypatch):
    """noise[1] is the eps= of the compute_noised_representation call that makes z_sc, noise[2] the raw noise= of sample_p_zs_given_zt; with
    one entry or none the torch.randn calls are those of the code before the extension: (x, h) per missing draw, in order."""
    ddpm, _ = _ddpm("qm9", self_condition=True)
    nn_ = torch.tensor([4, 3])
    N, D = int(nn_.sum()), 9
    inp = make_inputs("qm9", nn_, [7, 999], R.TRAIN_L2, seed=1, ddpm=ddpm)
    bi = R._bi(inp["off"])
    mask = torch.ones(N, dtype=torch.bool)
    net = _Recorder(N, D)
    ddpm.dynamics_network = net
    ddpm.train()
    g = torch.Generator().manual_seed(8)
    draws = [torch.randn((N, D), generator=g) for _ in range(3)]
    seen = {}

    def fake_jump(s, t, z, batch_index, node_mask, **kw):
        seen.update(s=s, t=t, z=z, grad=torch.is_grad_enabled(), **kw)
        return torch.full((N, D), 0.5)
    eps_calls = []
    orig_noised = ddpm.compute_noised_representation

    def noised(xh, batch_index, node_mask, gamma_t, generate_x_only=False, eps=None):
        eps_calls.append(eps)
        return orig_noised(xh, batch_index, node_mask, gamma_t, generate_x_only=generate_x_only, eps=eps)
    randn_calls = []
    orig_randn = torch.randn

    def randn(*a, **k):
        randn_calls.append(tuple(a[0]))
        return orig_randn(*a, **k)
    monkeypatch.setattr(ddpm, "sample_p_zs_given_zt", fake_jump)
    monkeypatch.setattr(ddpm, "compute_noised_representation", noised)
    monkeypatch.setattr(torch, "randn", randn)
    batch = pkg.config.AttrDict(x=inp["x"], h={"categorical": inp["one_hot"], "integer": inp["charges"]}, batch=bi, mask=mask, num_graphs=2,
                                num_nodes_present=nn_, props_context=None)
    noise = draws[:entries] if entries else None
    out = ddpm(batch, t_int=inp["t_int"].long().view(-1, 1), noise=noise, self_conditioning_prob=1.0)
    assert len(eps_calls) == 2 and len(net.calls) == 1
    if entries == 3:
        assert eps_calls[0] is draws[0] and eps_calls[1] is draws[1] and seen["noise"] is draws[2] and randn_calls == []
    elif entries == 1:
        assert eps_calls[0] is draws[0] and eps_calls[1] is None and seen["noise"] is None and randn_calls == [(N, 3), (N, D - 3)]          # z_sc; the jump is the stub's
    else:
        assert eps_calls == [None, None] and seen["noise"] is None and randn_calls == [(N, 3), (N, D - 3)] * 2
    # the jump goes from t + 1 to 0 under no_grad, the estimate reaches the one evaluation that carries the tape
    assert torch.equal(seen["t"], (inp["t_int"].long().view(-1, 1) + 1) / ddpm.T) and not seen["s"].any() and not seen["grad"] and seen["self_condition"]
    assert net.calls[0]["grad"] and torch.equal(net.calls[0]["xh_self_cond"], torch.full((N, D), 0.5)) and not net.calls[0]["xh_self_cond"].requires_grad
    assert out[1].requires_grad
    # a T in t_int suppresses the branch whatever the probability
    eps_calls.clear(), net.calls.clear()
    ddpm(batch, t_int=torch.tensor([[7], [ddpm.T]]), noise=draws, self_conditioning_prob=1.0)
    assert len(eps_calls) == 1 and net.calls[0]["xh_self_cond"] is None


def test_training_step_forwards_self_conditioning_prob(monkeypatch):
    model = pkg.QM9MoleculeGenerationDDPM(**pkg.default_cfgs("qm9")).train()
    got = {}

    def fake(batch, **kw):
        got.update(kw)
        z = torch.zeros(2, requires_grad=True)
        return (z, z, z, z, z, z, z, z, torch.zeros(2), {})
    monkeypatch.setattr(model.ddpm, "forward", fake)
    b = pkg.config.AttrDict(x=torch.zeros(4, 3), one_hot=torch.zeros(4, 5), charges=torch.zeros(4), batch=torch.tensor([0, 0, 1, 1]), mask=torch.ones(4, dtype=torch.bool))
    model.training_step(b, self_conditioning_prob=1.0)
    assert got["self_conditioning_prob"] == 1.0
    model.training_step(b)
    assert got["self_conditioning_prob"] == 0.5


def test_paths_and_reasons_without_a_gpu():
    ddpm, _ = _ddpm("qm9")
    assert ddpm.objective_path == "operators" and ddpm.why_not_fused_objective() is None
    with pytest.raises(ValueError):
        ddpm.set_objective_path("eager")
    ddpm.set_objective_path("fused")
    assert ddpm.objective_path == "fused"
    why = ddpm.why_not_fused_objective(pkg.config.AttrDict(x=torch.zeros(2, 3), batch=torch.zeros(2, dtype=torch.long), mask=torch.ones(2, dtype=torch.bool)))
    assert why is not None and "CPU tensor" in why
    with pytest.raises(NotImplementedError, match="CPU tensor"):
        ddpm(pkg.config.AttrDict(x=torch.zeros(2, 3), batch=torch.zeros(2, dtype=torch.long), mask=torch.ones(2, dtype=torch.bool)))
    for key, val, word in (("diffusion_target", "atom_types", "diffusion_target"), ("generate_x_only", True, "generate_x_only")):
        other, _ = _ddpm("qm9", **{key: val})
        assert word in other.why_not_fused_objective()
        with pytest.raises(NotImplementedError, match=word):
            other.set_objective_path("fused")
    model = pkg.QM9MoleculeGenerationDDPM(**pkg.default_cfgs("qm9"))
    assert model.objective_path == "operators"
    model.set_objective_path("fused")
    assert model.ddpm.objective_path == "fused" and model.objective_path == "fused"
