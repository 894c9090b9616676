"""The evaluation drivers without a GPU: what evaluate_conditional's chunked modes refuse (by name, before a size or a context is drawn and before
anything is launched), the batch plan -- chunks and per-batch seeds -- against a table, and evaluate_optimization's argument checks."""
import importlib

import pytest
import torch

pkg = importlib.import_module("bio-diffusion_amd")
plan = pkg.mol_gen_ddpm.conditional_eval_plan


class _Untouchable:
    """props_distr / classifier of a call that must be refused first: any use fails the test."""
    properties = ["alpha"]
    normalizer = {"alpha": {"mean": 75.0, "mad": 6.5}}

    def sample_batch(self, num_nodes):
        raise AssertionError("a context was drawn before the call was refused")

    def predict(self, *a, **k):
        raise AssertionError("the classifier ran before the call was refused")


def _cpu_model(self_condition=False, conditioning=("alpha",), include_charges=None):
    cfgs = pkg.default_cfgs("qm9", conditioning=conditioning)
    cfgs["diffusion_cfg"]["num_timesteps"] = 8
    if self_condition:
        cfgs["diffusion_cfg"]["self_condition"] = True
    if include_charges is not None:
        cfgs["dataloader_cfg"]["include_charges"] = include_charges
    model = pkg.QM9MoleculeGenerationDDPM(**cfgs).eval()          # stays on the CPU: a device call would fail

    def no_sizes(n):
        raise AssertionError("sizes were drawn before the call was refused")

    model.ddpm.num_nodes_distribution.sample = no_sizes
    return model


@pytest.fixture(scope="module")
def model():
    return _cpu_model()


def _call(model, **kw):
    u = _Untouchable()
    return model.evaluate_conditional(u, "alpha", 75.0, 6.5, iterations=3, batch_size=4, props_distr=u, **kw)


def test_packed_and_concurrent_exclude_each_other_in_sample_and_analyze_s_words(model):
    with pytest.raises(ValueError) as e:
        _call(model, packed_batches=2, concurrent_batches=2)
    with pytest.raises(ValueError) as e0:
        model.sample_and_analyze(4, packed_batches=2, concurrent_batches=2)
    assert str(e.value) == str(e0.value) and "exclude each other" in str(e.value)
    with pytest.raises(ValueError, match="packed_batches must be >= 1"):
        _call(model, packed_batches=0)


@pytest.mark.parametrize("mode", [dict(packed_batches=2), dict(concurrent_batches=2)])
@pytest.mark.parametrize("name, value", [("node_mask", torch.ones(3, dtype=torch.bool)), ("fix_noise", True), ("lanes", 1),
                                         ("noise_fn", lambda k: None), ("step_callback", lambda s, z: None), ("return_frames", 2)])
def test_chunked_modes_refuse_by_name_what_they_cannot_honour(model, mode, name, value):
    with pytest.raises(ValueError, match=rf"\b{name}\b") as e:
        _call(model, num_timesteps=4, **mode, **{name: value})
    assert next(iter(mode)) in str(e.value)


def test_chunked_modes_refuse_any_other_sample_keyword_too(model):
    with pytest.raises(ValueError, match="norm_with_original_timesteps"):
        _call(model, packed_batches=2, norm_with_original_timesteps=True)


def test_packed_refuses_a_self_conditioned_model_before_any_work():
    sc = _cpu_model(self_condition=True)
    with pytest.raises(NotImplementedError, match="packed_batches.*self-conditioned"):
        _call(sc, packed_batches=2)
    with pytest.raises(NotImplementedError, match="packed_batches.*self-conditioned"):
        _call(sc, packed_batches=2, lanes=1)                 # the model comes first, as in mol_gen_sample_packed


def test_the_sequential_call_still_takes_those_keywords(model):
    """No refusal without a chunked mode: the call gets as far as drawing the sizes."""
    with pytest.raises(AssertionError, match="sizes were drawn"):
        _call(model, lanes=1, seed=7)
    with pytest.raises(AssertionError, match="sizes were drawn"):
        _call(model)


# (iterations, K, seed, mode) -> chunks, seeds
PLAN_TABLE = [
    ((4, 2, 77, "packed"), [[0, 1], [2, 3], [4]], [77, 78, 79, 80, 81]),                     # a short last chunk
    ((4, 2, 77, "concurrent"), [[0, 1], [2, 3], [4]], [77, 78, 79, 80, 81]),
    ((2, 10, None, "packed"), [[0, 1, 2]], [1234, 1235, 1236]),                              # K larger than the batch count; the default base
    ((2, 1, None, "packed"), [[0], [1], [2]], [1234, 1235, 1236]),                           # K = 1
    ((5, 3, 0, "concurrent"), [[0, 1, 2], [3, 4, 5]], [0, 1, 2, 3, 4, 5]),                   # K divides the count; seed 0 is a seed, not "none"
    ((0, 4, 9, "packed"), [[0]], [9]),                                                       # iterations = 0 is one batch
    ((2, 4, None, "sequential"), [[0], [1], [2]], [None, None, None]),                       # the default call: the sampler's own seed, every batch
    ((2, 4, 5, "sequential"), [[0], [1], [2]], [5, 6, 7]),                                   # K is ignored
    ((100, 10, None, "packed"), [list(range(i, min(i + 10, 101))) for i in range(0, 101, 10)], [1234 + i for i in range(101)]),   # the paper's setting
]


@pytest.mark.parametrize("args, chunks, seeds", PLAN_TABLE)
def test_batch_plan_table(args, chunks, seeds):
    got_chunks, got_seeds = plan(*args)
    assert got_chunks == chunks and got_seeds == seeds
    assert [i for c in got_chunks for i in c] == list(range(args[0] + 1))          # every batch once, in order


def test_batch_plan_refuses_nonsense():
    with pytest.raises(ValueError, match="mode"):
        plan(1, 1, None, "tiled")
    with pytest.raises(ValueError, match="K"):
        plan(1, 0, None, "packed")
    with pytest.raises(ValueError, match="iterations"):
        plan(-1, 1, None, "packed")


def _flat(sizes, F=5):
    n = sum(sizes)
    return torch.zeros(n, 3), torch.zeros(n, F), torch.tensor(sizes)


def test_evaluate_optimization_argument_checks(model):
    u = _Untouchable()
    x, oh, nn_ = _flat([3, 4])
    ctx = torch.zeros(2, 1)
    with pytest.raises(ValueError, match="num_iterations"):
        model.evaluate_optimization(u, "alpha", 75.0, 6.5, (x, oh), nn_, num_iterations=0, num_timesteps=2, context=ctx)
    with pytest.raises(ValueError, match="rows"):
        model.evaluate_optimization(u, "alpha", 75.0, 6.5, (x[:-1], oh[:-1]), nn_, num_iterations=1, num_timesteps=2, context=ctx)
    with pytest.raises(ValueError, match="rows"):
        model.evaluate_optimization(u, "alpha", 75.0, 6.5, (x, oh[:-1]), nn_, num_iterations=1, num_timesteps=2, context=ctx)
    with pytest.raises(ValueError, match="pairs"):
        model.evaluate_optimization(u, "alpha", 75.0, 6.5, [(x[:3], oh[:3]), (x[3:5], oh[3:5]), (x[5:], oh[5:])], nn_, num_iterations=1,
                                    num_timesteps=2, context=ctx)
    with pytest.raises(ValueError, match="context or props_distr"):
        model.evaluate_optimization(u, "alpha", 75.0, 6.5, (x, oh), nn_, num_iterations=1, num_timesteps=2)
    with pytest.raises(ValueError, match="conditions on 'alpha'"):
        model.evaluate_optimization(u, "mu", 75.0, 6.5, (x, oh), nn_, num_iterations=1, num_timesteps=2, props_distr=u)


def test_evaluate_optimization_raises_what_optimize_raises():
    u = _Untouchable()
    x, oh, nn_ = _flat([3, 4])
    ctx = torch.zeros(2, 1)
    plain = _cpu_model(conditioning=())
    with pytest.raises(Exception, match="Optimization requires a context conditional") as e:
        plain.evaluate_optimization(u, "alpha", 75.0, 6.5, (x, oh), nn_, num_iterations=1, num_timesteps=2, context=ctx)
    with pytest.raises(Exception) as e0:
        plain.optimize([(x[:3], oh[:3]), (x[3:], oh[3:])], num_timesteps=2, num_nodes=nn_, context=ctx)
    assert type(e.value) is type(e0.value) and str(e.value) == str(e0.value)
    charged = _cpu_model(include_charges=True)
    with pytest.raises(NotImplementedError, match="include_charges") as e:
        charged.evaluate_optimization(u, "alpha", 75.0, 6.5, (x, oh), nn_, num_iterations=1, num_timesteps=2, context=ctx)
    with pytest.raises(NotImplementedError) as e0:
        charged.optimize([(x[:3], oh[:3]), (x[3:], oh[3:])], num_timesteps=2, num_nodes=nn_, context=ctx)
    assert str(e.value) == str(e0.value)


def test_flat_samples_are_checked_against_num_nodes_by_the_sampler_too(model):
    x, oh, nn_ = _flat([3, 4])
    with pytest.raises(ValueError, match="rows"):
        model.ddpm.mol_gen_optimize((x[:-1], oh[:-1]), nn_, "cpu", num_timesteps=2, context=torch.zeros(2, 1))
    with pytest.raises(ValueError, match="one .x, h. pair per molecule"):
        model.ddpm.mol_gen_optimize([(x, oh)], nn_, "cpu", num_timesteps=2, context=torch.zeros(2, 1))
