"""The conditional and optimisation evaluation drivers on the MI355X: sequential, concurrent and packed evaluate_conditional give one result bit for
bit, batch i runs with seed base + i, the default call is today's loop, a chunk is classified in one launch with the bits of per-batch launches,
the chunked modes write the sequential call's files, and evaluate_optimization is the hand loop of optimize / stability / classifier.  Small
throughout: alpha-conditional QM9 widths, 8-step schedule, 2-D weights x 0.25, a synthetic classifier, batches of 6, 3-4 sampling steps."""
import filecmp
import importlib
import os

import pytest
import torch

import classifier_ref as cr
import synth

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("bio-diffusion_amd")
clf = pkg.classifier
MEAN, MAD = 75.0, 6.5
ITER, BS, T, SEED = 4, 6, 4, 77


class _StubProps:
    """Duck-typed PropertiesDistribution: one property, a seeded normalised context per molecule; keeps what it handed out."""
    properties = ["alpha"]
    normalizer = {"alpha": {"mean": 75.0, "mad": 6.5}}

    def __init__(self, constant=None):
        self.g, self.constant, self.drawn = torch.Generator().manual_seed(0), constant, []

    def sample_batch(self, num_nodes):
        c = torch.randn((len(num_nodes), 1), generator=self.g) if self.constant is None else torch.full((len(num_nodes), 1), self.constant)
        self.drawn.append(c)
        return c


@pytest.fixture(scope="module")
def env():
    cfgs = pkg.default_cfgs("qm9", conditioning=("alpha",))
    cfgs["diffusion_cfg"]["num_timesteps"] = 8
    torch.manual_seed(0)
    model = pkg.QM9MoleculeGenerationDDPM(**cfgs)
    with torch.no_grad():
        for p in model.ddpm.dynamics_network.parameters():
            if p.dim() == 2:
                p.mul_(0.25)
    model = model.cuda().eval()
    W = synth.make_weights(cr.state_dict_shapes(5, 128, 7, True, False), seed=11)
    net = clf.EGNN(in_node_nf=5, in_edge_nf=0, hidden_nf=128, device="cuda", n_layers=7, attention=1, node_attr=0)
    net.load_state_dict(W)
    yield model, net.eval()
    model.ddpm.release_lanes()


def _run(env, iterations=ITER, props=None, **kw):
    model, net = env
    props = _StubProps() if props is None else props
    torch.manual_seed(0)
    before = net.launches
    mae, records = model.evaluate_conditional(net, "alpha", MEAN, MAD, iterations=iterations, batch_size=BS, props_distr=props, num_timesteps=T, **kw)
    torch.cuda.synchronize()
    return dict(mae=mae, records=records, contexts=props.drawn, launches=net.launches - before)


@pytest.fixture(scope="module")
def three_modes(env):
    """The same evaluation three ways, run once and only read afterwards."""
    return dict(sequential=_run(env, seed=SEED, lanes=1), concurrent=_run(env, seed=SEED, concurrent_batches=2), packed=_run(env, seed=SEED, packed_batches=2))


def test_three_modes_one_result(three_modes):
    seq = three_modes["sequential"]
    assert len(seq["records"]) == ITER + 1
    sizes = [[int(v) for v in r["num_nodes"]] for r in seq["records"]]
    assert all(len(set(s)) > 1 for s in sizes) and len({tuple(s) for s in sizes}) > 1, f"the sizes are not ragged: {sizes}"
    for name in ("concurrent", "packed"):
        got = three_modes[name]
        assert len(got["records"]) == ITER + 1
        for i, (a, b) in enumerate(zip(seq["records"], got["records"])):
            assert sorted(a) == sorted(b) == ["label", "loss", "num_nodes", "one_hot", "pred", "x"]
            for key in ("num_nodes", "label", "x", "one_hot", "pred"):
                assert torch.equal(a[key], b[key]), (name, i, key)
            assert a["loss"] == b["loss"], (name, i)
        print(f"{name}: MAE = {got['mae']!r}  sequential: {seq['mae']!r}")
        assert got["mae"] == seq["mae"]
    # 5 batches in chunks of 2, 2, 1: one classifier launch per chunk, one per batch in the sequential call
    assert seq["launches"] == (ITER + 1) * clf.LAUNCHES_PER_FORWARD
    assert three_modes["packed"]["launches"] == three_modes["concurrent"]["launches"] == 3 * clf.LAUNCHES_PER_FORWARD


def test_batch_i_of_the_packed_run_is_mol_gen_sample_with_seed_base_plus_i(env, three_modes):
    model, _ = env
    got = three_modes["packed"]
    xs = []
    for i, (r, ctx) in enumerate(zip(got["records"], got["contexts"])):
        xh, _, _ = model.ddpm.mol_gen_sample(BS, r["num_nodes"], model.device, num_timesteps=T, context=ctx.to(model.device), seed=SEED + i)
        assert torch.equal(xh[:, :3], r["x"]) and torch.equal(xh[:, 3:], r["one_hot"]), i
        xs.append(xh)
    # and not with one seed for all of them
    xh, _, _ = model.ddpm.mol_gen_sample(BS, got["records"][1]["num_nodes"], model.device, num_timesteps=T, context=got["contexts"][1].to(model.device), seed=SEED)
    assert not torch.equal(xh, xs[1])


def test_chunked_modes_without_a_seed_start_at_1234(env):
    model, _ = env
    got = _run(env, iterations=1, packed_batches=2)
    for i, (r, ctx) in enumerate(zip(got["records"], got["contexts"])):
        xh, _, _ = model.ddpm.mol_gen_sample(BS, r["num_nodes"], model.device, num_timesteps=T, context=ctx.to(model.device), seed=1234 + i)
        assert torch.equal(xh[:, :3], r["x"]), i


def test_identical_batches_differ_with_per_batch_seeds_and_coincide_in_the_default_call(env, monkeypatch):
    model, _ = env
    fixed = torch.tensor([5, 9, 3, 7, 9, 4])
    monkeypatch.setattr(model.ddpm.num_nodes_distribution, "sample", lambda n: fixed.clone())
    for kw in (dict(packed_batches=2, seed=SEED), dict(concurrent_batches=2, seed=SEED), dict(seed=SEED)):
        a, b = _run(env, iterations=1, props=_StubProps(constant=0.3), **kw)["records"]
        assert torch.equal(a["num_nodes"], b["num_nodes"]) and torch.equal(a["label"], b["label"])
        assert not torch.equal(a["x"], b["x"]), kw
    a, b = _run(env, iterations=1, props=_StubProps(constant=0.3))["records"]        # the documented default: one seed, one noise tape
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["one_hot"], b["one_hot"])


def test_default_call_is_the_loop_it_was(env):
    model, net = env
    got = _run(env, iterations=2)
    torch.manual_seed(0)
    props, total = _StubProps(), 0.0
    for i in range(3):
        num_nodes = model.ddpm.num_nodes_distribution.sample(BS)
        context = props.sample_batch(num_nodes).to(model.device)
        x, one_hot, charges, batch_index = model.sample(num_samples=BS, num_nodes=num_nodes, context=context, num_timesteps=T)
        label = context.reshape(BS, -1)[:, 0].to(torch.float32) * 6.5 + 75.0
        pred = net.predict(x, one_hot, num_nodes=num_nodes)
        loss = (MAD * pred + MEAN - label).abs().mean().item()
        total += loss * BS
        r = got["records"][i]
        for key, want in (("num_nodes", num_nodes), ("label", label), ("x", x), ("one_hot", one_hot), ("pred", pred)):
            assert torch.equal(r[key], want), (i, key)
        assert r["loss"] == loss
    assert got["mae"] == total / (3 * BS)


def test_a_chunk_scored_in_one_launch_has_the_bits_of_per_batch_launches(env, three_modes):
    _, net = env
    recs = three_modes["packed"]["records"]
    for chunk in ([0, 1], [2, 3], [4]):
        x, oh = torch.cat([recs[i]["x"] for i in chunk]), torch.cat([recs[i]["one_hot"] for i in chunk])
        whole = net.predict(x, oh, num_nodes=torch.cat([recs[i]["num_nodes"] for i in chunk]))
        each = torch.cat([net.predict(recs[i]["x"], recs[i]["one_hot"], num_nodes=recs[i]["num_nodes"]) for i in chunk])
        assert torch.equal(whole, each) and torch.equal(whole, torch.cat([recs[i]["pred"] for i in chunk]))


def test_chunked_modes_write_the_files_of_the_sequential_call(env, tmp_path):
    dirs = {}
    for name, kw in (("sequential", dict(lanes=1)), ("packed", dict(packed_batches=2))):
        dirs[name] = str(tmp_path / name)
        _run(env, iterations=2, seed=SEED, save_molecules=True, sampling_output_dir=dirs[name], **kw)
    runs = sorted(os.listdir(dirs["sequential"]))
    assert runs == ["run0", "run1", "run2"] == sorted(os.listdir(dirs["packed"]))
    for i, run in enumerate(runs):
        files = sorted(os.listdir(os.path.join(dirs["sequential"], run)))
        assert files == [f"conditional_{i * BS + m:03d}.xyz" for m in range(BS)]
        match, mismatch, errors = filecmp.cmpfiles(os.path.join(dirs["sequential"], run), os.path.join(dirs["packed"], run), files, shallow=False)
        assert match == files and not mismatch and not errors


# ---- the optimisation driver ---------------------------------------------------------------------------------------------------------------
OPT_SIZES = [3, 4, 5, 6, 7, 8, 9, 5, 7]
OPT_T, OPT_ITERS, OPT_SEED = 3, 3, 5


@pytest.fixture(scope="module")
def opt_inputs():
    x, oh = cr.make_batch(OPT_SIZES, 5, seed=31, spread=1.2)
    pairs = []
    for xm, hm in zip(x.split(OPT_SIZES), oh.split(OPT_SIZES)):
        pairs.append(((xm - xm.mean(0, keepdim=True)).cuda(), hm.cuda()))          # centred, as optimize wants its samples
    ctx = torch.randn((len(OPT_SIZES), 1), generator=torch.Generator().manual_seed(4)).cuda()
    return pairs, torch.tensor(OPT_SIZES), ctx


def _hand_loop(env, opt_inputs, seeds):
    """The loop a user wrote before the driver: optimize, check_molecular_stability_batch, classifier.predict, the list rebuilt each time."""
    model, net = env
    pairs, nn_, ctx = opt_inputs
    label = ctx[:, 0] * MAD + MEAN
    out = []
    for seed in seeds:
        x, oh, _, _ = model.optimize(pairs, num_timesteps=OPT_T, num_nodes=nn_, context=ctx, seed=seed)
        st = pkg.stability.check_molecular_stability_batch(x, oh.argmax(-1), nn_, model.dataset_info).cpu().to(torch.int64)
        pred = net.predict(x, oh, num_nodes=nn_)
        out.append(dict(mae=(MAD * pred + MEAN - label).abs().mean().item(), mol_stable=float(st[:, 0].sum()) / len(nn_),
                        atm_stable=float(st[:, 1].sum()) / float(st[:, 2].sum()), x=x, one_hot=oh))
        pairs = list(zip(x.split(OPT_SIZES), oh.split(OPT_SIZES)))
    return out


@pytest.fixture(scope="module")
def opt_driver(env, opt_inputs):
    model, net = env
    pairs, nn_, ctx = opt_inputs
    flat = (torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs]))
    kw = dict(num_iterations=OPT_ITERS, num_timesteps=OPT_T, context=ctx, seed=OPT_SEED)
    return dict(flat=model.evaluate_optimization(net, "alpha", MEAN, MAD, flat, nn_, **kw),
                pairs=model.evaluate_optimization(net, "alpha", MEAN, MAD, pairs, nn_, **kw), flat_in=flat)


def test_optimisation_driver_is_the_hand_loop(env, opt_inputs, opt_driver):
    model, net = env
    pairs, nn_, ctx = opt_inputs
    recs = opt_driver["flat"]
    assert [r["iteration"] for r in recs] == [None, 0, 1, 2]
    assert all(sorted(r) == ["atm_stable", "iteration", "mae", "mol_stable", "one_hot", "x"] for r in recs)
    # record 0: the initial samples, scored as they came
    x0, oh0 = opt_driver["flat_in"]
    st = pkg.stability.check_molecular_stability_batch(x0, oh0.argmax(-1), nn_, model.dataset_info).cpu().to(torch.int64)
    pred = net.predict(x0, oh0, num_nodes=nn_)
    assert torch.equal(recs[0]["x"], x0) and torch.equal(recs[0]["one_hot"], oh0)
    assert recs[0]["mae"] == (MAD * pred + MEAN - (ctx[:, 0] * MAD + MEAN)).abs().mean().item()
    assert recs[0]["mol_stable"] == float(st[:, 0].sum()) / 9 and recs[0]["atm_stable"] == float(st[:, 1].sum()) / float(st[:, 2].sum())
    want = _hand_loop(env, opt_inputs, [OPT_SEED + it for it in range(OPT_ITERS)])
    for it, (r, w) in enumerate(zip(recs[1:], want)):
        print(f"iteration {it}: mae = {r['mae']!r} mol_stable = {r['mol_stable']!r} atm_stable = {r['atm_stable']!r}")
        assert torch.equal(r["x"], w["x"]) and torch.equal(r["one_hot"], w["one_hot"]), it
        assert r["mae"] == w["mae"] and r["mol_stable"] == w["mol_stable"] and r["atm_stable"] == w["atm_stable"], it
    # one seed for every iteration is another experiment
    reused = _hand_loop(env, opt_inputs, [OPT_SEED] * OPT_ITERS)
    assert torch.equal(reused[0]["x"], recs[1]["x"])
    assert not torch.equal(reused[2]["x"], recs[3]["x"])


def test_optimisation_driver_takes_the_list_of_pairs_too(opt_driver):
    for a, b in zip(opt_driver["flat"], opt_driver["pairs"]):
        assert a["iteration"] == b["iteration"] and torch.equal(a["x"], b["x"]) and torch.equal(a["one_hot"], b["one_hot"])
        assert a["mae"] == b["mae"] and a["mol_stable"] == b["mol_stable"] and a["atm_stable"] == b["atm_stable"]


def test_optimisation_driver_options(env, opt_inputs, opt_driver, tmp_path):
    """unknown_labels scores against the property mean; without the initial record the list starts at iteration 0; context drawn once from
    props_distr; files under run<it + 2>."""
    model, net = env
    pairs, nn_, ctx = opt_inputs
    props = _StubProps()
    recs = model.evaluate_optimization(net, "alpha", MEAN, MAD, opt_driver["flat_in"], nn_, num_iterations=1, num_timesteps=OPT_T, props_distr=props,
                                       unknown_labels=True, score_initial_samples=False, seed=OPT_SEED, save_molecules=True,
                                       sampling_output_dir=str(tmp_path))
    assert [r["iteration"] for r in recs] == [0] and len(props.drawn) == 1
    x, oh, _, _ = model.optimize(pairs, num_timesteps=OPT_T, num_nodes=nn_, context=props.drawn[0].cuda(), seed=OPT_SEED)
    assert torch.equal(recs[0]["x"], x)
    pred = net.predict(x, oh, num_nodes=nn_)
    assert recs[0]["mae"] == (MAD * pred + MEAN - torch.full_like(pred, 75.0)).abs().mean().item()
    assert os.listdir(str(tmp_path)) == ["run2"]
    assert sorted(os.listdir(str(tmp_path / "run2"))) == [f"conditional_{m:03d}.xyz" for m in range(len(OPT_SIZES))]
