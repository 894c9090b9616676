"""The fused EGNN property classifier on the MI355X: parity with the reference's fp64 (tests/golden/classifier_*.npz, bar 20 x the fixture's own
fp32-vs-fp64 distance, the factor of tests/test_gpu_parity.py's every-row goldens), per-layer h through the debug read, every molecule size,
dense entry == ragged entry, bitwise independence of batch composition / position / run, guard words, a non-default stream, the in-place
weight update, and the conditional-evaluation driver.  Every figure is printed before it is asserted."""
import importlib
import os

import numpy as np
import pytest
import torch

import classifier_ref as cr
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("bio-diffusion_amd")
clf = pkg.classifier
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONFIGS = ["h128_l7_att", "h128_l7_attr", "h64_l2_att_attr", "h256_l1"]
FACTOR = 20.0


def _model(F, H, L, att, attr, seed=11):
    W = synth.make_weights(cr.state_dict_shapes(F, H, L, bool(att), bool(attr)), seed=seed)
    m = clf.EGNN(in_node_nf=F, in_edge_nf=0, hidden_nf=H, device="cuda", n_layers=L, attention=att, node_attr=attr)
    m.load_state_dict(W)
    return m.eval(), W


def _fixture(name):
    g = np.load(os.path.join(GOLDEN, f"classifier_{name}.npz"))
    cfg = tuple(int(v) for v in g["config"])
    return g, cfg


def _own_gap(W, x, h0, sizes):
    p64 = cr.forward(W, x, h0, sizes)
    p32 = cr.forward(W, x, h0, sizes, dtype=torch.float32)
    return p64, (p32.double() - p64).abs().max().item()


@pytest.mark.parametrize("name", CONFIGS)
def test_prediction_and_every_layer_against_the_reference_fp64(name):
    g, cfg = _fixture(name)
    model, _ = _model(*cfg)
    L = cfg[2]
    x, h0, nn_ = torch.tensor(g["x"]).cuda(), torch.tensor(g["one_hot"]).cuda(), torch.tensor(g["num_nodes"])
    before = model.launches
    pred = model.predict(x, h0, num_nodes=nn_)
    assert model.launches - before == clf.LAUNCHES_PER_FORWARD == 1
    err, gap = (pred.double().cpu() - torch.tensor(g["pred64"])).abs().max().item(), float(g["gap"])
    print(f"{name}: max|hip - ref64| = {err:.3e}  gap = {gap:.3e}  ratio = {err / gap:.2f}")
    rows, worst = int(g["layer_rows"]), 0.0
    ratios = []
    for k in range(L + 1):
        p2, h = model.predict(x, h0, num_nodes=nn_, debug_layer=k)
        assert torch.equal(p2, pred)
        e = (h[:rows].double().cpu() - torch.tensor(g["h_layers"][k])).abs().max().item()
        ratios.append(e / float(g["gap_layers"][k]))
    print(f"{name}: per-layer ratios " + " ".join(f"{r:.2f}" for r in ratios))
    assert err <= FACTOR * gap
    assert max(ratios) <= FACTOR


def test_every_molecule_size_in_one_batch():
    """Per molecule: err <= M * that molecule's own fp32-vs-fp64 gap + 2 ulp of what its final dot product sums (classifier_ref.compare)."""
    sizes = list(range(1, clf.MAX_NODES + 1))
    model, W = _model(5, 128, 7, 1, 0)
    x, h0 = cr.make_batch(sizes, 5, seed=3)
    ref = cr.references(W, x, h0, sizes)
    pred = model.predict(x.cuda(), h0.cuda(), num_nodes=torch.tensor(sizes))
    failures, ratios = cr.compare(ref, pred=pred.cpu())
    gap = (ref.pred32 - ref.pred64).abs().max().item()
    err = (pred.double().cpu() - ref.pred64).abs().max().item()
    print(f"sizes 1..{clf.MAX_NODES}: err = {err:.3e} gap = {gap:.3e} ratio = {err / gap:.2f}; worst M a molecule needs = {ratios['pred']:.2f}")
    assert not failures, failures


def test_dense_entry_is_bitwise_the_ragged_entry_and_checks_its_masks():
    sizes = [5, 1, 29, 2, 17, 11]
    model, _ = _model(5, 64, 2, 1, 1)
    x, h0 = cr.make_batch(sizes, 5, seed=8)
    ragged = model.predict(x.cuda(), h0.cuda(), num_nodes=torch.tensor(sizes))
    xp, hp, nm, em, n = cr.to_padded(x, h0, sizes)
    dense = model(h0=hp.cuda(), x=xp.cuda(), edges=[torch.zeros(1), torch.zeros(1)], edge_attr=None, node_mask=nm.cuda(), edge_mask=em.cuda(), n_nodes=n)
    assert torch.equal(dense, ragged)
    by_index = model.predict(x.cuda(), h0.cuda(), batch_index=torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).cuda())
    assert torch.equal(by_index, ragged)
    bad = em.clone()
    bad[1] = 1 - bad[1]                     # (0, 1) of the first molecule flipped
    with pytest.raises(ValueError, match="edge_mask"):
        model(h0=hp.cuda(), x=xp.cuda(), edges=None, edge_attr=None, node_mask=nm.cuda(), edge_mask=bad.cuda(), n_nodes=n)
    holes = nm.clone()
    holes[0], holes[n - 1] = 0, 1
    with pytest.raises(ValueError, match="prefix"):
        model(h0=hp.cuda(), x=xp.cuda(), edges=None, edge_attr=None, node_mask=holes.cuda(), edge_mask=None, n_nodes=n)


def test_a_molecule_is_bitwise_independent_of_its_batch():
    model, _ = _model(5, 128, 7, 1, 0)
    n = 19
    xm, hm = cr.make_batch([n], 5, seed=21)
    alone = model.predict(xm.cuda(), hm.cuda(), num_nodes=torch.tensor([n]))
    sizes = cr.qm9_sizes(2048, seed=4)

    def batch_with(pos, count):
        sz = list(sizes[:count])
        sz[pos] = n
        x, h0 = cr.make_batch(sz, 5, seed=77)
        o = int(sum(sz[:pos]))
        x[o:o + n], h0[o:o + n] = xm, hm
        return x.cuda(), h0.cuda(), torch.tensor(sz)

    for pos, count in [(0, 64), (31, 64), (63, 64), (1000, 2048), (2047, 2048)]:
        x, h0, nn_ = batch_with(pos, count)
        a = model.predict(x, h0, num_nodes=nn_)
        b = model.predict(x, h0, num_nodes=nn_)
        assert torch.equal(a, b), "two runs of the same batch differ"
        assert a[pos].item() == alone[0].item(), (pos, count, a[pos].item(), alone[0].item())


def test_guard_words_and_a_large_qm9_batch():
    model, W = _model(5, 128, 7, 1, 0)
    sizes = cr.qm9_sizes(2048, seed=6)
    x, h0 = cr.make_batch(sizes, 5, seed=12)
    p64, gap = _own_gap(W, x, h0, sizes)
    xd, hd, B, N = x.cuda(), h0.cuda(), len(sizes), int(sum(sizes))
    # the C entry on buffers with NaN guard words either side of pred and of the workspace
    import ctypes as C
    lib = pkg._native.load_ops()
    G = 64
    wsn = int(lib.gcdm_classifier_workspace_bytes(0, N, 5, 128, 7)) // 4
    predbuf = torch.full((B + 2 * G,), float("nan"), device="cuda")
    wsbuf = torch.full((wsn + 2 * G,), float("nan"), device="cuda")
    noff = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
    noff[1:] = torch.cumsum(torch.tensor(sizes), 0).cuda()
    packed = model._weights(lib, xd.device)
    st = lib.gcdm_classifier_forward(xd.data_ptr(), hd.data_ptr(), noff.data_ptr(), packed.data_ptr(), wsbuf[G:].data_ptr(), predbuf[G:].data_ptr(),
                                     None, -1, N, B, 5, 128, 7, 1, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, lib.gcdm_classifier_last_error()
    torch.cuda.synchronize()
    assert bool(predbuf[:G].isnan().all()) and bool(predbuf[G + B:].isnan().all())
    assert bool(wsbuf[:G].isnan().all()) and bool(wsbuf[G + wsn:].isnan().all())
    pred = predbuf[G:G + B]
    assert torch.equal(pred, model.predict(xd, hd, num_nodes=torch.tensor(sizes)))
    err = (pred.double().cpu() - p64).abs().max().item()
    print(f"2048 QM9 molecules: err = {err:.3e} gap = {gap:.3e} ratio = {err / gap:.2f}")
    assert err <= FACTOR * gap


def test_oversized_molecule_on_the_device_gives_nan_and_touches_nothing_else():
    model, _ = _model(5, 32, 1, 0, 0)
    sizes = [4, 3, 33, 5, 6, 7]            # 58 atoms in 6 molecules passes the host check; the third is over the limit
    x, h0 = cr.make_batch(sizes, 5, seed=2)
    pred = model.predict(x.cuda(), h0.cuda(), num_nodes=torch.tensor(sizes).cuda()).cpu()
    good = model.predict(*[t.cuda() for t in cr.make_batch(sizes, 5, seed=2)], num_nodes=torch.tensor([4, 3, 30, 3, 5, 6, 7]))  # same atoms, legal split
    assert bool(pred[2].isnan())                                    # (a large batch shares workgroups: its neighbour would be NaN too)
    assert torch.equal(pred[:2], good[:2].cpu()) and torch.equal(pred[3:], good[4:].cpu())


def test_non_default_stream_behind_a_long_kernel():
    model, _ = _model(5, 128, 7, 1, 0)
    sizes = cr.qm9_sizes(256, seed=9)
    x, h0 = cr.make_batch(sizes, 5, seed=10)
    xd, hd, nn_ = x.cuda(), h0.cuda(), torch.tensor(sizes).cuda()
    want = model.predict(xd, hd, num_nodes=nn_).clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    big = torch.randn(6144, 6144, device="cuda")
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        xs = xd.clone()
        for _ in range(12):
            big = big @ big * 1e-4        # a long queue on s
        xs2 = xs + 0                       # produced on s, behind the queue
        got = model.predict(xs2, hd, num_nodes=nn_)
        out = got.to("cpu", non_blocking=True)
        done.record(s)
    done.synchronize()                     # this stream only: no device-wide sync
    assert torch.equal(out, want.cpu())


def test_parameter_changed_in_place_is_picked_up():
    model, W = _model(5, 64, 2, 1, 1)
    sizes = [7, 12]
    x, h0 = cr.make_batch(sizes, 5, seed=5)
    a = model.predict(x.cuda(), h0.cuda(), num_nodes=torch.tensor(sizes))
    with torch.no_grad():
        model.graph_dec[2].bias.add_(1.0)
        model.gcl_1.edge_mlp[2].weight.mul_(0.5)
    b = model.predict(x.cuda(), h0.cuda(), num_nodes=torch.tensor(sizes))
    W2 = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    p64, gap = _own_gap(W2, x, h0, sizes)
    assert not torch.equal(a, b)
    assert (b.double().cpu() - p64).abs().max().item() <= FACTOR * gap


class _StubProps:
    """Duck-typed PropertiesDistribution: one property, a seeded normalised context per molecule."""
    properties = ["alpha"]
    normalizer = {"alpha": {"mean": 75.0, "mad": 6.5}}

    def __init__(self):
        self.g = torch.Generator().manual_seed(0)

    def sample_batch(self, num_nodes):
        return torch.randn((len(num_nodes), 1), generator=self.g)


def test_conditional_evaluation_driver():
    cfgs = pkg.default_cfgs("qm9", conditioning=("alpha",))
    cfgs["diffusion_cfg"]["num_timesteps"] = 8
    torch.manual_seed(0)
    model = pkg.QM9MoleculeGenerationDDPM(**cfgs)
    with torch.no_grad():
        for p in model.ddpm.dynamics_network.parameters():
            if p.dim() == 2:
                p.mul_(0.25)
    model = model.cuda().eval()
    net, W = _model(5, 128, 7, 1, 0)
    mean, mad = 75.0, 6.5
    mae, records = model.evaluate_conditional(net, "alpha", mean, mad, iterations=2, batch_size=8, props_distr=_StubProps())
    assert len(records) == 3                                    # iterations + 1, as the reference's loader
    total = 0.0
    for r in records:
        sizes = [int(v) for v in r["num_nodes"]]
        assert len(sizes) == 8 and r["x"].shape[0] == sum(sizes)
        p64 = cr.forward(W, r["x"].cpu(), r["one_hot"].cpu(), sizes)
        total += (mad * p64 + mean - r["label"].double().cpu()).abs().mean().item() * 8
    want = total / 24
    print(f"driver: MAE = {mae:.6f}  fp64 restatement on the same samples = {want:.6f}  rel = {abs(mae - want) / want:.2e}")
    assert abs(mae - want) <= 1e-5 * want
    mae_u, _ = model.evaluate_conditional(net, "alpha", mean, mad, iterations=0, batch_size=4, props_distr=_StubProps(), unknown_labels=True)
    assert np.isfinite(mae_u)
