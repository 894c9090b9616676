"""The fused training update (optim.TrainingUpdate, include/gcdm_optim.h) on an MI355X: the 433 QM9 parameter tensors plus edge sizes against
the fp64 restatement of tests/optim_ref.py within its running fp32 error bound (derivation in optim_ref's docstring), the clip queue over 60
steps, bitwise determinism, the non-finite skip, five training steps of the 64 x 19 QM9 model against stock torch (AdamW + the restated
clip and EMA) with the sampler and the EMA swap seeing the update, and the state round trips."""
import importlib
import os

import pytest
import torch

import optim_ref
import synth

pkg = importlib.import_module("bio-diffusion_amd")
optim = pkg.optim
DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu

EXTRA = [(40000,), (1,), (3,), (5,)]          # more than two chunks, and sizes below one float4


def _shapes():
    model = pkg.QM9MoleculeGenerationDDPM(**pkg.default_cfgs("qm9"))
    return [(tuple(p.shape), p.requires_grad) for p in model.parameters()]


def _params(seed=1):
    shapes = _shapes() + [(s, True) for s in EXTRA]
    assert len(shapes) == 433 + len(EXTRA) and sum(not r for _, r in shapes) == 1
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.1).to(DEV), requires_grad=r) for s, r in shapes]
    return ps


def _grads(ps, step, scale, seed=7):
    g = torch.Generator().manual_seed(seed + 1000 * step)
    return [(torch.randn(p.shape, generator=g) * scale).to(DEV) if p.requires_grad else None for p in ps]


def _set(ps, grads):
    for p, gr in zip(ps, grads):
        p.grad = None if gr is None else gr.clone()


def _check_within(fused, ref, err, what):
    d = (fused.double() - ref).abs()
    bar = 2 * err + 1e-30
    bad = (d > bar)
    assert not bad.any(), (what, d.max().item(), (d / bar).max().item())


def _compare(opt, ref, ps, amsgrad):
    for t, p in enumerate(ps):
        _check_within(p.detach(), ref.p[t], ref.err_p[t], ("p", t))
        if not p.requires_grad:
            continue
        _check_within(opt._param_view(0, t), ref.m[t], ref.err_m[t], ("m", t))
        _check_within(opt._param_view(1, t), ref.v[t], ref.err_v[t], ("v", t))
        if amsgrad:
            _check_within(opt._param_view(2, t), ref.vmax[t], ref.err_vmax[t], ("vmax", t))
        if ref.ema is not None:
            _check_within(opt._param_view(3, t), ref.ema[t], ref.err_ema[t], ("ema", t))
    assert opt.steps() == ref.steps
    assert opt.queue() == pytest.approx(ref.queue.items, rel=1e-6)


@pytest.mark.parametrize("amsgrad,scale", [(True, 1e-3), (True, 0.05), (False, 0.05)])
def test_full_size_update_matches_fp64_oracle(amsgrad, scale):
    """Three steps over the 433 QM9 tensors + EXTRA, EMA on.  scale 1e-3: norm ~2.5 against the seeded threshold 4500, clipping inactive.
    scale 0.05: norm ~125, and a queue of length 1 seeded with 10 puts the threshold at 15, so every step clips (coef 0.12, 0.18, 0.27: each push raises it by 1.5)."""
    ps = _params()
    kw = dict(lr=1e-3, weight_decay=1e-2, amsgrad=amsgrad, ema_decay=0.9)
    opt = optim.TrainingUpdate(ps, queue_len=1 if scale > 0.01 else 50, **kw)
    ref = optim_ref.RefUpdate(ps, queue_len=1 if scale > 0.01 else 50, **kw)
    if scale > 0.01:
        opt._reset_queue([10.0])
        ref.queue.items = [10.0]
    for k in range(3):
        grads = _grads(ps, k, scale)
        _set(ps, grads)
        opt.step()
        assert ref.step(grads)
    torch.cuda.synchronize()
    assert opt.read_flags() == 0
    if scale > 0.01:
        assert all(c < 0.5 for c in ref.coefs), ref.coefs
        assert opt.last_clip_coef() == pytest.approx(ref.coefs[-1], rel=1e-6)
    else:
        assert ref.coefs == [1.0, 1.0, 1.0]
    assert opt.last_grad_norm() == pytest.approx(ref.norms[-1], rel=1e-6)
    _compare(opt, ref, ps, amsgrad)
    gamma = [t for t, p in enumerate(ps) if not p.requires_grad][0]
    assert opt.steps()[gamma] == 0


def test_clip_queue_over_60_steps_matches_oracle():
    g0 = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g0).to(DEV)) for s in [(20000,), (7, 5), (1,), (3,)]]
    opt = optim.TrainingUpdate(ps, lr=1e-3, ema_decay=None)
    ref = optim_ref.RefUpdate(ps, lr=1e-3, ema_decay=None)
    coefs = []
    for k in range(60):
        scale = 1.0 + 0.5 * (k % 7)
        if k == 3:
            scale = 80.0
        if k in (52, 54, 56, 58):
            scale = 20.0
        grads = _grads(ps, k, scale)
        _set(ps, grads)
        opt.step()
        coefs.append(opt.last_clip_coef())
        assert ref.step(grads)
    assert sum(c < 1.0 for c in ref.coefs) >= 3 and 3000.0 not in ref.queue.items
    assert coefs == pytest.approx(ref.coefs, rel=1e-6)
    assert opt.queue() == pytest.approx(ref.queue.items, rel=1e-6)


def _run(seed_params=1, steps=3):
    ps = _params(seed_params)
    opt = optim.TrainingUpdate(ps, lr=1e-3)
    for k in range(steps):
        _set(ps, _grads(ps, k, 0.05))
        opt.step()
    torch.cuda.synchronize()
    return ps, opt


def test_two_runs_give_the_same_bits():
    a, oa = _run()
    b, ob = _run()
    for x, y in zip(a, b):
        assert torch.equal(x.detach(), y.detach())
    assert torch.equal(oa._state, ob._state)
    dev_a = oa._ws.view(torch.uint8)[oa._off[optim._STEPS]:]
    dev_b = ob._ws.view(torch.uint8)[ob._off[optim._STEPS]:]
    assert torch.equal(dev_a, dev_b)


def test_nonfinite_gradient_skips_the_step_and_raises_the_flag():
    ps, opt = _run(steps=2)
    before_p = [p.detach().clone() for p in ps]
    before_state = opt._state.clone()
    ws = opt._ws.view(torch.uint8)
    o = opt._off
    keep = [(o[optim._STEPS], o[optim._TSCAL]), (o[optim._QUEUE], o[optim._SCAL]), (o[optim._SCAL] + 24, o[optim._SCAL] + 40)]
    before_ws = [ws[a:b].clone() for a, b in keep]
    grads = _grads(ps, 5, 0.05)
    grads[17].view(-1)[-1] = float("nan")
    _set(ps, grads)
    opt.step()
    torch.cuda.synchronize()
    assert opt.read_flags() & optim.FLAG_NONFINITE
    for p, q in zip(ps, before_p):
        assert torch.equal(p.detach(), q)
    assert torch.equal(opt._state, before_state)
    for (a, b), w in zip(keep, before_ws):
        assert torch.equal(ws[a:b], w)
    assert opt.read_flags() == 0
    _set(ps, _grads(ps, 6, 0.05))
    opt.step()
    assert opt.read_flags() == 0 and opt.steps()[0] == 3


# ---- end to end --------------------------------------------------------------------------------------------------------------------

def _model():
    d = synth.DATASET_DIMS["qm9"]
    cfgs = pkg.default_cfgs("qm9")
    torch.manual_seed(0)
    model = pkg.QM9MoleculeGenerationDDPM(**cfgs)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 2:
                p.mul_(0.25)
    model = model.to(DEV).train()
    model.ddpm.dynamics_network.set_message_path("fused")
    Bt, n = 64, 19
    Nt = Bt * n
    g = torch.Generator().manual_seed(5)
    types = torch.randint(0, d["num_atom_types"], (Nt,), generator=g)

    def batch():
        return pkg.config.AttrDict(x=torch.randn((Nt, 3), generator=g).to(DEV), batch=torch.repeat_interleave(torch.arange(Bt), n).to(DEV),
                                   mask=torch.ones(Nt, dtype=torch.bool, device=DEV), props_context=None,
                                   one_hot=torch.nn.functional.one_hot(types, d["num_atom_types"]).float().to(DEV),
                                   charges=torch.randint(1, 10, (Nt,), generator=g).float().to(DEV))
    return model, cfgs, batch


def _sampler_forward(net):
    d = synth.DATASET_DIMS["qm9"]
    xh, t, bi, _, _ = synth.make_inputs([7, 19, 4], synth.dims_feat(d), seed=2)
    b = dict(batch=bi.to(DEV), mask=torch.ones(len(bi), dtype=torch.bool, device=DEV), props_context=None)
    with torch.no_grad():
        _, out = net(b, xh.to(DEV), t.to(DEV))
    return out.clone()


def test_five_training_steps_match_stock_torch_and_the_sampler_sees_them():
    model, cfgs, batch = _model()
    net = model.ddpm.dynamics_network
    net.eval()
    out0 = _sampler_forward(net)
    net.train()
    opt = model.configure_optimizers()
    assert isinstance(opt, optim.TrainingUpdate)
    g = opt.param_groups[0]
    g["lr"], g["ema_decay"] = 1e-3, 0.9                 # large enough that five steps move every output visibly
    ps = list(model.parameters())
    ref = optim_ref.RefUpdate(ps, lr=1e-3, ema_decay=0.9)
    tp = [p.detach().clone().requires_grad_(p.requires_grad) for p in ps]
    topt = torch.optim.AdamW(tp, lr=1e-3, weight_decay=1e-12, amsgrad=True)
    tema = [p.detach().clone() for p in tp]
    queue = optim_ref.Queue()
    queue.add(3000)
    for k in range(5):
        opt.zero_grad()
        torch.manual_seed(100 + k)
        model.training_step(batch())["loss"].backward()
        grads = [None if p.grad is None else p.grad.detach().clone() for p in ps]
        assert grads[[i for i, p in enumerate(ps) if not p.requires_grad][0]] is None
        for q, gr in zip(tp, grads):
            q.grad = gr
        opt.step()
        max_norm = 1.5 * queue.mean() + 2 * queue.std()
        norm = float(torch.nn.utils.clip_grad_norm_([q for q in tp if q.grad is not None], max_norm))
        queue.add(float(max_norm) if norm > max_norm else norm)
        topt.step()
        with torch.no_grad():
            for e, q in zip(tema, tp):
                e.sub_((e - q).mul_(1.0 - 0.9))
        assert ref.step(grads)
    torch.cuda.synchronize()
    assert opt.read_flags() == 0
    ema = opt.ema_tensors()
    for t, (p, q) in enumerate(zip(ps, tp)):
        # each of fused and torch lies within 2 err of the fp64 run on the same gradients
        _check_within(p.detach(), q.detach().double(), 2 * ref.err_p[t], ("p vs torch", t))
        _check_within(ema[t], tema[t].double(), 2 * ref.err_ema[t], ("ema vs torch", t))
    assert opt.queue() == pytest.approx(queue.items, rel=1e-6)

    # the sampler (evaluation mode, fused kernels) sees the update: it equals the module path on the trained weights
    net.train()
    mod = _sampler_forward(net)
    net.eval()
    out1 = _sampler_forward(net)
    tol = 1e-4 * max(1.0, mod.abs().max().item())
    assert (out1 - mod).abs().max().item() <= tol
    assert (out1 - out0).abs().max().item() > 10 * tol
    # evaluate_ema_weights_instead: inside the context the forward is the EMA model's
    twin = pkg.QM9MoleculeGenerationDDPM(**cfgs)
    twin.load_state_dict(opt.ema_state_dict(model))
    twin = twin.to(DEV).eval()
    want = _sampler_forward(twin.ddpm.dynamics_network)
    with opt.ema_weights():
        got = _sampler_forward(net)
    assert (got - want).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())
    assert (got - out1).abs().max().item() > 10 * tol
    after = _sampler_forward(net)
    assert (after - out1).abs().max().item() <= 1e-6 * max(1.0, out1.abs().max().item())


def test_torch_adamw_state_resumes_on_the_fused_update_and_back(tmp_path):
    g0 = torch.Generator().manual_seed(4)
    shapes = [(20000,), (33, 7), (1,), (5,)]
    init = [torch.randn(s, generator=g0).to(DEV) for s in shapes]
    tp = [torch.nn.Parameter(x.clone()) for x in init]
    topt = torch.optim.AdamW(tp, lr=1e-3, weight_decay=1e-2, amsgrad=True)
    for k in range(3):
        _set(tp, _grads(tp, k, 0.1))
        topt.step()
    sd = topt.state_dict()
    fp = [torch.nn.Parameter(q.detach().clone()) for q in tp]
    opt = optim.TrainingUpdate(fp, lr=0.5, clip_gradients=False, ema_decay=None)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == 1e-3 and opt.steps() == [3, 3, 3, 3]
    ref = optim_ref.RefUpdate(fp, lr=1e-3, weight_decay=1e-2, clip_gradients=False, ema_decay=None)
    for t, q in enumerate(tp):
        st = topt.state[q]
        ref.m[t], ref.v[t], ref.vmax[t] = st["exp_avg"].double().clone(), st["exp_avg_sq"].double().clone(), st["max_exp_avg_sq"].double().clone()
        ref.steps[t] = 3
    for k in range(3, 5):
        grads = _grads(tp, k, 0.1)
        _set(tp, grads)
        _set(fp, grads)
        topt.step()
        opt.step()
        assert ref.step(grads)
    torch.cuda.synchronize()
    for t, (p, q) in enumerate(zip(fp, tp)):
        _check_within(p.detach(), q.detach().double(), 2 * ref.err_p[t], ("p", t))
    # and back: torch continues from the fused update's state dict
    back = [torch.nn.Parameter(p.detach().clone()) for p in fp]
    topt2 = torch.optim.AdamW(back, lr=1e-3, weight_decay=1e-2, amsgrad=True)
    topt2.load_state_dict(opt.state_dict())
    for t, q in enumerate(back):
        st = topt2.state[q]
        assert int(st["step"]) == 5
        assert torch.equal(st["exp_avg"], opt._param_view(0, t)) and torch.equal(st["max_exp_avg_sq"], opt._param_view(2, t))
    _set(back, _grads(back, 9, 0.1))
    topt2.step()


def test_ema_state_dict_saves_as_an_ema_checkpoint(tmp_path):
    model, cfgs, batch = _model()
    opt = model.configure_optimizers()
    opt.param_groups[0]["ema_decay"] = 0.5
    for k in range(2):
        opt.zero_grad()
        torch.manual_seed(7 + k)
        model.training_step(batch())["loss"].backward()
        opt.step()
    sd = opt.ema_state_dict(model)
    assert len(sd) == len(model.state_dict())
    path = os.path.join(tmp_path, "last-EMA.ckpt")
    torch.save({"state_dict": sd}, path)
    loaded = model.load_from_checkpoint(path)
    ema = opt.ema_tensors()
    names = [n for n, _ in model.named_parameters()]
    lp = dict(loaded.named_parameters())
    moved = 0
    for n, e, p in zip(names, ema, model.parameters()):
        if n.startswith("ddpm.dynamics_network."):
            assert torch.equal(lp[n].detach().cpu(), e.cpu()), n
            moved += not torch.equal(e, p.detach())
    assert moved > 0
