"""The reference's other ways of training on the GPU -- conditional, self-conditioned (taken and skipped), VLB, a partial node mask -- against
the reference's own terms, loss and gradients (tests/golden/train_full_{qm9cond,qm9sc,qm9sc_skip,geomsc,qm9vlb,qm9mask}.npz) on two path
sets: every operator path, and the fused message, node and objective paths together.  The body and the bars are those of
test_training_loss_and_gradients_match_reference_autograd (tests/train_cases.py); the three draws of a self-conditioned step are pinned
through the three-entry ``noise`` list."""
import pytest
import torch

import train_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATHS = ("operators", "fused")


def _step(model, c, prob=1.0, noise="fixture", backward=True):
    model.zero_grad()
    loss = model.training_step(TC.batch_of(c, DEV), t_int=c.t_int, noise=c.noise if noise == "fixture" else noise, self_conditioning_prob=prob)["loss"]
    if backward:
        loss.backward()
    return loss


@pytest.mark.parametrize("paths", PATHS)
@pytest.mark.parametrize("name", TC.VARIANTS)
def test_training_step_matches_reference_autograd(name, paths, golden_dir):
    """self_conditioning_prob is 1.0 everywhere: on qm9sc_skip it is the T in t_int that must suppress the branch."""
    c = TC.load(golden_dir, name)
    model, why = TC.model_for(c, DEV, paths)
    assert why is None, f"{name}: the fused paths refuse this fixture ({why})"
    loss, (fac, what) = TC.check_training_step(c, model, DEV, self_conditioning_prob=1.0)
    if paths == "fused":
        assert model.ddpm.read_objective_flags() == 0
    print(f"MEASURED {name} / {paths}: loss {loss.item():.6f} (reference fp64 {float(c.g['loss_64']):.6f}); worst factor of |ref32 - ref64| beyond "
          f"the 1e-4 part: {fac:.2f} ({what})")


@pytest.mark.parametrize("name", ["qm9sc", "geomsc", "qm9mask"])
def test_fused_against_operators_on_the_same_draws(name, golden_dir):
    """Loss and d net_out (captured by a hook on the evaluation that carries the tape) of both path sets against the fp64 pipeline of
    tests/train_cases.py.  Bar: the fused distance <= 4 x the operators distance + 1e-6 relative."""
    c = TC.load(golden_dir, name)
    want = TC.pipeline(c)
    l64, d64 = float(want["loss"]), want["d_net_out"]
    dist = {}
    for paths in PATHS:
        model, why = TC.model_for(c, DEV, paths)
        assert why is None, why
        seen = {}

        def hook(mod, args, out):
            if out[1].requires_grad:
                out[1].register_hook(lambda gr: seen.__setitem__("d", gr.detach().clone()))
        h = model.ddpm.dynamics_network.register_forward_hook(hook)
        loss = _step(model, c)
        h.remove()
        dist[paths] = (abs(loss.item() - l64), (seen["d"].double().cpu() - d64).abs().max().item())
    (lo, do), (lf, df) = dist["operators"], dist["fused"]
    print(f"MEASURED {name}: distance from the fp64 pipeline, loss: operators {lo:.3e} fused {lf:.3e} (|loss| {abs(l64):.3e}); "
          f"d net_out: operators {do:.3e} fused {df:.3e} (max |d| {d64.abs().max().item():.3e})")
    assert lf <= 4 * lo + 1e-6 * abs(l64) and df <= 4 * do + 1e-6 * d64.abs().max().item()


def test_self_conditioned_step_is_bitwise_repeatable(golden_dir):
    c = TC.load(golden_dir, "qm9sc")
    model, why = TC.model_for(c, DEV, "fused")
    assert why is None, why
    runs = []
    for _ in range(2):
        loss = _step(model, c)
        runs.append((loss.detach().clone(), {k: p.grad.clone() for k, p in model.ddpm.dynamics_network.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


def test_the_estimate_keeps_no_tape(golden_dir):
    """After the step's backward the bytes allocated are those of a step whose branch was skipped, and no more than before the step: the
    no_grad estimate left no workspace.  The accounting of test_tape_is_freed_after_backward_and_double_backward_refused: gradients stay
    allocated, one set of batch tensors serves every step (the sampler's plan cache keeps the batch index and mask it last saw alive, so
    tensors made afresh per step would be counted with whichever step the cache saw last: measured 1024 bytes)."""
    c = TC.load(golden_dir, "qm9sc")
    model, why = TC.model_for(c, DEV, "fused")
    assert why is None, why
    b0 = TC.batch_of(c, DEV)
    t_int, noise = c.t_int.to(DEV), [e.to(DEV) for e in c.noise]

    def step(prob):
        model.zero_grad(set_to_none=False)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        loss = model.training_step(TC.pkg.config.AttrDict(**b0), t_int=t_int, noise=noise, self_conditioning_prob=prob)["loss"]
        loss.backward()
        del loss
        torch.cuda.synchronize()
        return base, torch.cuda.memory_allocated()
    for prob in (0.0, 1.0):          # warm: gradients of the parameters exist, caches built
        step(prob)
    (base0, held0), (base1, held1) = step(0.0), step(1.0)
    print(f"MEASURED bytes allocated before / after a step: skipped {base0} / {held0}, taken {base1} / {held1}")
    assert held1 == held0 and held1 <= base1 and held0 <= base0


def test_unpinned_draws(golden_dir):
    c = TC.load(golden_dir, "qm9sc")
    model, why = TC.model_for(c, DEV, "fused")
    assert why is None, why
    on, off = _step(model, c, 1.0, backward=False).item(), _step(model, c, 0.0, backward=False).item()
    want = float(TC.pipeline(c, self_conditioning_prob=0.0)["loss"])          # the network with xh_self_cond=None
    assert abs(on - off) > 1e-3 * abs(on) and abs(off - want) <= 1e-4 * abs(want), (on, off, want)
    one = _step(model, c, 1.0, noise=c.noise[:1], backward=False)             # one entry: the two other draws are torch.randn's
    assert torch.isfinite(one) and abs(one.item() - on) > 0
    loss = _step(model, c, 1.0, noise=None)
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in model.ddpm.dynamics_network.parameters())
    assert model.ddpm.read_objective_flags() == 0
