"""CPU checks of what the several-batches drivers do with their flag words (fused_sampler.redo_in_fp32): which batches are sampled again
on the primary handle, with which arguments, and what ``last_flags`` reports.  A fake dynamics network records ``disable_fused_layer``;
``mol_gen_sample`` is a stub that records its arguments and leaves the flag word of the repeated run in ``last_flags``."""
import importlib
import logging

import pytest
import torch
from torch import nn

pkg = importlib.import_module("bio-diffusion_amd")
FS = importlib.import_module("bio-diffusion_amd.fused_sampler")
F16, TAIL, NAN, COG = pkg._native.FLAG_F16_RANGE, pkg._native.FLAG_TAIL, pkg._native.FLAG_NAN_VEL, pkg._native.FLAG_COG_DRIFT
WARNING = "An activation left the f16 range in a test run; re-running with fp32 MFMA."
SIZES = [torch.tensor([4, 5]), torch.tensor([3]), torch.tensor([6, 7, 8])]
CONTEXTS = [torch.full((len(s), 1), float(b)) for b, s in enumerate(SIZES)]
SEEDS = [11, 22, 33]
T = 7


class FakeDyn(nn.Module):
    def __init__(self):
        super().__init__()
        self.disabled = []

    def disable_fused_layer(self, where):
        self.disabled.append(where)


@pytest.fixture
def ddpm(monkeypatch):
    cfgs = pkg.default_cfgs("qm9")
    d = pkg.EquivariantVariationalDiffusion(FakeDyn(), cfgs["diffusion_cfg"], cfgs["dataloader_cfg"], pkg.dataset_info("qm9"))
    d.calls, d.rerun_flags = [], {}

    def mol_gen_sample(num_samples, num_nodes, device, **kw):
        b = next(i for i, s in enumerate(SIZES) if s is num_nodes)
        d.calls.append((b, num_samples, device, kw))
        d.last_flags = F16 | d.rerun_flags.get(b, 0)            # what a run that fell back to fp32 MFMA reports
        return ("redone", b)
    monkeypatch.setattr(d, "mol_gen_sample", mol_gen_sample)
    return d


def redo(ddpm, words, plan_wide, where="the_driver"):
    return FS.redo_in_fp32(ddpm, where, WARNING, words, SIZES, CONTEXTS, SEEDS, "cuda", T, plan_wide=plan_wide)


@pytest.mark.parametrize("plan_wide", [False, True])
def test_clean_words_are_folded_and_nothing_is_redone(ddpm, caplog, plan_wide):
    with caplog.at_level(logging.WARNING):
        assert redo(ddpm, [0, NAN, COG], plan_wide) == [None, None, None]
    assert ddpm.calls == [] and ddpm.last_flags == NAN | COG and ddpm.dynamics_network.disabled == []
    assert WARNING not in caplog.text and "Detected NaN in `vel`" in caplog.text and "CoG drift above 5e-2" in caplog.text


def test_per_batch_policy_redoes_exactly_the_dirty_batch_with_its_own_arguments(ddpm, caplog):
    ddpm.rerun_flags = {1: COG}
    with caplog.at_level(logging.WARNING):
        assert redo(ddpm, [NAN, F16, 0], plan_wide=False) == [None, ("redone", 1), None]
    (b, num_samples, device, kw), = ddpm.calls
    assert (b, num_samples, device) == (1, len(SIZES[1]), "cuda")
    assert sorted(kw) == ["context", "num_timesteps", "seed"]
    assert kw["num_timesteps"] == T and kw["context"] is CONTEXTS[1] and kw["seed"] == SEEDS[1]
    assert ddpm.last_flags == NAN | F16 | COG                   # the redone run's flags OR the clean words
    assert caplog.text.count(WARNING) == 1 and ddpm.dynamics_network.disabled == []


def test_plan_wide_policy_redoes_every_batch(ddpm, caplog):
    ddpm.rerun_flags = {0: NAN, 2: COG}
    with caplog.at_level(logging.WARNING):
        assert redo(ddpm, [NAN, F16, 0], plan_wide=True) == [("redone", 0), ("redone", 1), ("redone", 2)]
    assert [(c[0], c[1]) for c in ddpm.calls] == [(b, len(s)) for b, s in enumerate(SIZES)]
    for b, _, _, kw in ddpm.calls:
        assert kw["num_timesteps"] == T and kw["context"] is CONTEXTS[b] and kw["seed"] == SEEDS[b]
    assert ddpm.last_flags == F16 | NAN | COG and caplog.text.count(WARNING) == 1
    assert "Detected NaN in `vel`" not in caplog.text          # the discarded words are not reported: the repeated runs report their own


@pytest.mark.parametrize("plan_wide", [False, True])
def test_range_and_tail_turn_the_fused_layer_off_once_under_the_drivers_name(ddpm, plan_wide):
    words = [0, F16 | TAIL, 0] if not plan_wide else [TAIL, F16, 0]          # plan-wide: the bits of the whole plan count
    redo(ddpm, words, plan_wide, where="mol_gen_sample_packed")
    assert ddpm.dynamics_network.disabled == ["mol_gen_sample_packed"]
    assert len(ddpm.calls) == (3 if plan_wide else 1) and ddpm.last_flags == F16


def test_tail_without_range_goes_through_the_flag_reporter(ddpm, monkeypatch):
    seen = []
    report = ddpm._report_flags
    monkeypatch.setattr(ddpm, "_report_flags", lambda fl, where, guard=None: seen.append((fl, where)) or report(fl, where, guard))
    assert redo(ddpm, [0, TAIL, NAN], plan_wide=False, where="mol_gen_sample_concurrent") == [None, None, None]
    assert seen == [(0, "mol_gen_sample_concurrent"), (TAIL, "mol_gen_sample_concurrent"), (NAN, "mol_gen_sample_concurrent")]
    assert ddpm.calls == [] and ddpm.dynamics_network.disabled == ["mol_gen_sample_concurrent"] and ddpm.last_flags == TAIL | NAN
