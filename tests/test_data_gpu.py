"""The device-resident data set on an MI355X, through its C ABI (include/gcdm_data.h) and through data.py: every field of every batch against
the reference's own batches (tests/golden/data_small.npz) with torch.equal, the graph and its CSR against today's ops.fully_connected_edge_index
+ mask filter + ops.Graph + col_order(), the histograms against the reference's integers, the draw against its numpy / torch-CPU statement bit
for bit, a training step with and without the loader's hints, iteration without a device-to-host copy, and the conditional entry points after
attach_dataset.  Outputs are pre-filled with NaN / -1: an element the kernels leave unwritten fails the comparison."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import data_cases as dc
import synth

pkg = importlib.import_module("bio-diffusion_amd")
native, ops = pkg._native, pkg.ops
pytestmark = pytest.mark.gpu
DEV = "cuda"
GRAPH_FIELDS = ("edge_index", "rowptr", "colperm", "colptr")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def collate_cabi(ds, perm, first, B, pad_to, N=None, E=None):
    """gcdm_data_collate itself on pre-filled buffers; N and E from the host mirror unless given."""
    lib = native.load_ops()
    if N is None or E is None:
        n_, e_, _ = pkg.data.batch_accounting(ds.num_atoms_host[np.asarray(perm)[first:first + B]], pad_to)
        N, E = n_ if N is None else N, e_ if E is None else E
    P, T, Cn = len(ds.property_keys), ds.num_species, len(ds.conditioning)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)
    neg = lambda dt, *s: torch.full(s, -1, dtype=dt, device=DEV)
    o = dict(x=nan(N, 3), one_hot=nan(N, T), charges=nan(N, 1), batch=neg(torch.int64, N), mask=torch.full((N,), 7, dtype=torch.uint8, device=DEV),
             index=neg(torch.int64, B), num_nodes_present=neg(torch.int64, B), props=nan(P, B), props_context=nan(N, Cn),
             edge_index=neg(torch.int64, 2, E), rowptr=neg(torch.int32, N + 1), colperm=neg(torch.int64, E), colptr=neg(torch.int32, N + 1))
    out = native.DataBatch(*[o[f[0]].data_ptr() for f in native.DataBatch._fields_])
    perm_d = torch.tensor(np.array(perm), dtype=torch.int64).to(DEV)
    ws = torch.full((int(lib.gcdm_data_workspace_bytes(B)),), 0xAB, dtype=torch.uint8, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = lib.gcdm_data_collate(ctypes.byref(ds._set), _p(perm_d), len(perm_d), first, B, pad_to, _p(ds.ctx_cols), Cn, N, E, _p(ws), ctypes.byref(out),
                               _p(flags), _stream())
    assert st == 0
    torch.cuda.synchronize()
    o["flags"] = int(flags.item())
    return o


def todays_graph(batch_index, mask, sizes_rows):
    """The graph as the module path builds it without hints (gcpnet.py forward_modules): edges from the row counts, the mask filter, ops.Graph."""
    ei = ops.fully_connected_edge_index(torch.as_tensor(sizes_rows), torch.device(DEV))
    if not bool(mask.all()):
        ei = ei[:, mask[ei[0]] & mask[ei[1]]].contiguous()
    g = ops.Graph(ei, len(batch_index))
    colperm, colptr = g.col_order()
    return dict(edge_index=ei, rowptr=g.rowptr, colperm=colperm, colptr=colptr)


def assert_batch(got, want, property_keys, what):
    assert got["flags"] == 0, what
    for k in ("x", "one_hot", "charges", "batch", "index", "num_nodes_present", "props_context", "edge_index"):
        assert got[k].dtype == want[k].dtype and torch.equal(got[k].cpu(), want[k]), (what, k)
    assert torch.equal(got["mask"].cpu().bool(), want["mask"]) and int(got["mask"].max()) <= 1, (what, "mask")
    for p, k in enumerate(property_keys):
        assert torch.equal(got["props"][p].cpu(), want[k]), (what, k)
    N = len(want["batch"])
    today = todays_graph(got["batch"], got["mask"].bool(), torch.bincount(want["batch"], minlength=len(want["index"])))
    for k in GRAPH_FIELDS:
        assert got[k].dtype == today[k].dtype and torch.equal(got[k], today[k]), (what, k, "ops.Graph")
    rowptr, colperm, colptr = dc.csr_of(want["edge_index"], N)
    assert torch.equal(got["rowptr"].cpu(), rowptr) and torch.equal(got["colperm"].cpu(), colperm) and torch.equal(got["colptr"].cpu(), colptr), what


@pytest.fixture(scope="module")
def ds():
    return pkg.MoleculeDataset(dc.raw(), DEV, conditioning=dc.CONDITIONING)


@pytest.mark.parametrize("layout", ["padded", "compact"])
@pytest.mark.parametrize("name", dc.BATCHES)
def test_collate_equals_the_reference_batch_field_by_field(ds, name, layout):
    """`one`: B = 1, a one-atom molecule, a single self-loop.  `wave`: 8 and 9 atoms (64 and 81 edges), the 9-atom molecule fills pad_to.
    `tail`: first > 0 and a short last batch."""
    g = dc.fixture()
    want = dc.expected_batch(name, layout)
    got = collate_cabi(ds, g[f"{name}_perm"], int(g[f"{name}_first"]), len(want["index"]), dc.A_MAX if layout == "padded" else 0)
    assert_batch(got, want, dc.PROPERTY_KEYS, (name, layout))
    if name == "one":
        assert got["edge_index"].shape == (2, 1) and got["edge_index"].tolist() == [[0], [0]]


SHAPES = {
    "scan300": ([1 + (5 * k + k // 7) % 3 for k in range(300)], list(range(299, -1, -1)), 0, 300),       # the offset scan leaves one workgroup's width
    "big181": ([181, 2, 64], [0, 1, 2], 0, 3),                                                           # a molecule of many tiles of edges
    "repeat": ([4, 7, 1, 3], [2, 1, 1, 3, 0, 1], 1, 5),                                                  # a wrap-around stream repeats molecules
}


@pytest.mark.parametrize("layout", ["padded", "compact"])
@pytest.mark.parametrize("case", list(SHAPES))
def test_collate_on_shapes_beyond_the_fixture(case, layout):
    sizes, perm, first, B = SHAPES[case]
    rawd = dc.synthetic_raw(sizes, seed=len(sizes), props=("alpha", "mu"))
    d = pkg.MoleculeDataset(rawd, DEV, conditioning=["mu"])
    norm = {k: (d.norm[i, 0].cpu(), d.norm[i, 1].cpu()) for i, k in enumerate(d.property_keys)}
    pad_to = d.max_atoms if layout == "padded" else 0
    want = dc.torch_batch(rawd, d.included_species, perm[first:first + B], pad_to, norm, ["mu"], d.property_keys)
    got = collate_cabi(d, perm, first, B, pad_to)
    assert_batch(got, want, d.property_keys, (case, layout))


def test_sizes_that_do_not_add_up_raise_the_flag_and_stay_inside_the_buffers(ds):
    got = collate_cabi(ds, [5, 6], 0, 2, 0, E=96)               # 81 + 16 = 97 edges
    assert got["flags"] == native.DATA_FLAG_ACCOUNT and got["edge_index"].shape == (2, 96)
    got = collate_cabi(ds, [5, 9], 0, 2, 0, N=9, E=81)          # molecule 9 does not exist
    assert got["flags"] == native.DATA_FLAG_ACCOUNT


def test_loader_batches_are_the_cabi_batches(ds):
    for layout in ("padded", "compact"):
        loader = ds.loader(3, shuffle=True, seed=4, layout=layout)
        loader.set_epoch(2)
        batches = list(loader)
        assert len(batches) == len(loader) == 3 and [b.num_graphs for b in batches] == [3, 3, 2]
        perm = loader.indices.tolist()
        for k, b in enumerate(batches):
            got = collate_cabi(ds, perm, 3 * k, b.num_graphs, loader.pad_to)
            for key in ("x", "one_hot", "batch", "index", "num_nodes_present", "props_context"):
                assert torch.equal(b[key], got[key]), (layout, k, key)
            assert b.charges.shape == b.batch.shape and torch.equal(b.charges, got["charges"].reshape(-1))          # [N], as the reference's batches
            assert b.mask.dtype == torch.bool and torch.equal(b.mask, got["mask"].bool())
            for p, key in enumerate(ds.property_keys):
                assert b[key].shape == (b.num_graphs,) and torch.equal(b[key], got["props"][p])
            fc = b.fc_graph
            assert isinstance(fc, ops.Graph) and fc.N == len(b.batch) and fc.E == got["edge_index"].shape[1]
            assert torch.equal(fc.edge_index, got["edge_index"]) and torch.equal(fc.rowptr, got["rowptr"])
            assert torch.equal(fc.col_order()[0], got["colperm"]) and torch.equal(fc.col_order()[1], got["colptr"])
            assert b.all_present == bool(b.mask.all()) and isinstance(b.all_present, bool) and isinstance(b.num_graphs, int)
        ds.check()
    assert [b.num_graphs for b in ds.loader(3, shuffle=False, drop_last=True)] == [3, 3]


# ---- the property histograms and the draw ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_bins", [7, 1000])
def test_histograms_equal_the_reference_integers(ds, num_bins):
    g = dc.fixture()
    lib = native.load_ops()
    S = 10
    for p, key in enumerate(dc.CONDITIONING):
        counts = torch.full((S, num_bins), -1, dtype=torch.int32, device=DEV)
        params = torch.full((S, 2), float("nan"), dtype=torch.float32, device=DEV)
        members, flags = torch.full((S,), -1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        st = lib.gcdm_data_prop_histogram(_p(ds.atom_ptr), _p(ds.props[ds.property_keys.index(key)]), ds.M, S, num_bins, _p(counts), _p(params),
                                          _p(members), _p(flags), _stream())
        assert st == 0 and int(flags.item()) == 0
        assert torch.equal(counts.cpu(), torch.tensor(np.array(g[f"hist{num_bins}_counts"][p]))), key
        assert torch.equal(members.cpu(), torch.tensor(np.array(g[f"hist{num_bins}_members"][p]))), key
        assert torch.equal(params.cpu(), torch.tensor(np.array(g[f"hist{num_bins}_params"][p]))), key
    pd = pkg.PropertiesDistribution(ds, dc.CONDITIONING, num_bins=num_bins, normalizer=ds.mean_mad(dc.CONDITIONING))
    assert pd.properties == dc.CONDITIONING and sorted(pd.distributions["U0"]) == [1, 2, 3, 4, 5, 8, 9]
    for p, key in enumerate(dc.CONDITIONING):
        for n, d in pd.distributions[key].items():
            assert [float(d["params"][0]), float(d["params"][1])] == g[f"hist{num_bins}_params"][p, n].tolist()
            assert d["counts"].tolist() == g[f"hist{num_bins}_counts"][p, n].tolist()


def test_a_size_outside_the_tables_raises_the_flag(ds):
    lib = native.load_ops()
    S, nb = 9, 7                                                 # the nine-atom molecule has no row
    counts, params = torch.empty((S, nb), dtype=torch.int32, device=DEV), torch.empty((S, 2), dtype=torch.float32, device=DEV)
    members, flags = torch.empty(S, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    assert lib.gcdm_data_prop_histogram(_p(ds.atom_ptr), _p(ds.props[0]), ds.M, S, nb, _p(counts), _p(params), _p(members), _p(flags), _stream()) == 0
    assert int(flags.item()) == native.DATA_FLAG_ACCOUNT and int(members.sum()) == 7


@pytest.mark.parametrize("num_bins", [7, 1000])
def test_draw_equals_its_numpy_statement_bit_for_bit(ds, num_bins):
    g = dc.fixture()
    pd = pkg.PropertiesDistribution(ds, dc.CONDITIONING, num_bins=num_bins, normalizer=ds.mean_mad(dc.CONDITIONING))
    counts, params, members = g[f"hist{num_bins}_counts"], g[f"hist{num_bins}_params"], g[f"hist{num_bins}_members"]
    norm = np.stack([g["norm_alpha"], g["norm_U0"]])
    rng = np.random.default_rng(11)
    num_nodes = np.array([1, 5, 5, 9, 8, 4, 3, 2, 5] * 40, dtype=np.int64)           # 360 draws: more than one workgroup
    u = rng.random((len(num_nodes), 2, 2), dtype=np.float32)
    u[2, :, 0], u[1, :, 0], u[3, :, 1] = np.float32(0.99999994), 0.0, 0.0
    want = dc.sample_reference(counts, params, members, norm, num_nodes, u)
    got = pd.sample_batch(torch.tensor(num_nodes).to(DEV), u=torch.tensor(u))
    assert got.shape == (len(num_nodes), 2) and torch.equal(got.cpu(), torch.tensor(want))
    assert torch.equal(got.cpu(), dc.draw_torch(counts, params, members, norm, num_nodes, u))
    pd.check()
    # u1 = (k + 1/2) / count for every rank k: the drawn bins reproduce the counts
    for p in range(2):
        for n in (5, 9):
            count = int(members[p, n])
            uu = torch.zeros((count, 2, 2))
            uu[:, :, 0] = ((torch.arange(count, dtype=torch.float32) + 0.5) / count).unsqueeze(-1)
            vals = pd.sample_batch(torch.full((count,), n), u=uu)[:, p].cpu().numpy()
            c = counts[p, n]
            lefts = np.flatnonzero(c).repeat(c[c > 0]).astype(np.float32) / np.float32(num_bins) * np.float32(params[p, n, 1] - params[p, n, 0]) \
                + params[p, n, 0]
            assert np.array_equal(vals, (lefts - norm[p, 0]) / norm[p, 1]), (p, n)
    # seedable
    gen = torch.Generator(device=DEV)
    a = pd.sample_batch(torch.tensor([5, 9, 1]), generator=gen.manual_seed(3))
    b = pd.sample_batch(torch.tensor([5, 9, 1]), generator=gen.manual_seed(3))
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and pd.sample(5).shape == (2,)


def test_a_size_absent_from_the_data_raises(ds):
    pd = pkg.PropertiesDistribution(ds, ["alpha"], num_bins=7, normalizer=ds.mean_mad(["alpha"]))
    with pytest.raises(KeyError):
        pd.sample_batch(torch.tensor([5, 6]))                    # sizes on the host: at once
    with pytest.raises(KeyError):
        pd.sample(12)
    out = pd.sample_batch(torch.tensor([5, 6, 40], device=DEV))  # sizes on the device: NaN rows, raised at the next look
    assert torch.isnan(out.cpu()).reshape(-1).tolist() == [False, True, True]
    with pytest.raises(KeyError, match="no member"):
        pd.check()
    pd.check()                                                   # raised once
    assert bool(torch.isfinite(pd.sample_batch(torch.tensor([5], device=DEV))).all())
    pd.check()


# ---- the hints ------------------------------------------------------------------------------------------------------------------------------
def _qm9_model():
    d = synth.DATASET_DIMS["qm9"]
    model = pkg.QM9MoleculeGenerationDDPM(**pkg.default_cfgs("qm9"))
    shapes = synth.dynamics_shapes(d["S"], d["V"], d["Se"], d["Ve"], d["L"], synth.dims_h_in(d))
    model.ddpm.dynamics_network.load_state_dict(synth.make_weights(shapes, seed=3))
    return model.to(DEV).train(), d


@pytest.mark.parametrize("paths", ["operators", "fused"])
@pytest.mark.parametrize("layout", ["padded", "compact"])
def test_training_step_gives_the_same_bits_with_and_without_the_hints(layout, paths):
    """Loss and every parameter gradient with torch.equal.  On "operators" this also holds ops.gather_col's backward to a fixed summation order: with
    fp32 atomics there, 324 of 432 gradients differed between two runs of one batch (worst 1.1e-05 relative), with the hints or without."""
    model, d = _qm9_model()
    net = model.ddpm.dynamics_network
    if paths == "fused":
        net.set_message_path("fused")
        net.set_node_path("fused")
        model.set_objective_path("fused")
    data = pkg.MoleculeDataset(dc.synthetic_raw([3, 5, 9, 4, 8, 9, 7, 5], seed=2), DEV)          # sizes the QM9 size prior knows
    batch = next(iter(data.loader(8, shuffle=False, layout=layout)))
    assert batch.all_present == (layout == "compact")
    N, F = len(batch.batch), synth.dims_feat(d)
    gen = torch.Generator().manual_seed(5)
    noise = [torch.randn((N, 3 + F), generator=gen)]
    t_int = torch.tensor([[17], [400], [3], [999], [250], [1], [731], [88]])
    results = []
    for hints in (True, False):
        b = pkg.AttrDict({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()})
        if hints:
            b.fc_graph = batch.fc_graph
        else:
            for k in ("fc_graph", "all_present", "num_graphs"):
                del b[k]
        model.zero_grad(set_to_none=True)
        loss = model.training_step(b, t_int=t_int, noise=noise)["loss"]
        loss.backward()
        results.append((loss.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}))
    (la, ga), (lb, gb) = results
    assert bool(torch.isfinite(la)) and torch.equal(la, lb)
    assert len(ga) > 10 and sorted(ga) == sorted(gb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    data.check()


def test_iterating_and_drawing_make_no_device_to_host_copy(ds):
    pd = pkg.PropertiesDistribution(ds, dc.CONDITIONING, num_bins=7, normalizer=ds.mean_mad(dc.CONDITIONING))
    sizes = torch.tensor([5, 9, 1, 4], device=DEV)
    one = torch.ones(1, device=DEV)
    list(ds.loader(3, layout="compact"))                         # the library is loaded, the allocator warm
    pd.sample_batch(sizes)
    loaders = [ds.loader(3, seed=1, layout=layout) for layout in ("padded", "compact")]
    iterators = [iter(loader) for loader in loaders]            # the epoch's permutation goes up here, once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            one.item()
            effective = False
        except RuntimeError:
            effective = True
        if effective:
            for loader, it in zip(loaders, iterators):
                batches = [next(it) for _ in range(len(loader))]
                assert len(batches) == 3
            ctx = pd.sample_batch(sizes)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not effective:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make a bare .item() raise on this build")
    assert ctx.shape == (4, 2) and bool(torch.isfinite(ctx).all())
    pd.check()


def test_conditional_entry_points_work_after_attach_dataset():
    cfgs = pkg.default_cfgs("qm9", conditioning=("alpha",))
    cfgs["diffusion_cfg"]["num_timesteps"] = 8
    torch.manual_seed(0)
    model = pkg.QM9MoleculeGenerationDDPM(**cfgs)
    with torch.no_grad():
        for p in model.ddpm.dynamics_network.parameters():
            if p.dim() == 2:
                p.mul_(0.25)
    model = model.to(DEV).eval()
    sizes = sorted(int(n) for n in model.dataset_info["n_nodes"]) * 2
    rawd = dc.synthetic_raw(sizes, seed=8)
    confs = [torch.cat((rawd["charges"][m, :n].float().unsqueeze(-1), rawd["positions"][m, :n]), dim=-1).numpy() for m, n in enumerate(sizes)]
    data = pkg.MoleculeDataset.from_conformers(confs, DEV, properties={"alpha": rawd["alpha"]}, conditioning=["alpha"])
    num_nodes = torch.tensor([3, 9, 5, 4])
    with pytest.raises(ValueError, match="no props_distr attached"):
        model.sample(4, num_nodes=num_nodes)
    pd = model.attach_dataset(data)
    assert model.props_distr is pd and pd.properties == ["alpha"] and set(pd.normalizer["alpha"]) == {"mean", "mad"}
    assert sorted(pd.distributions["alpha"]) == sorted(set(sizes))
    x, one_hot, charges, batch_index = model.sample(4, num_nodes=num_nodes)
    assert x.shape == (21, 3) and one_hot.shape == (21, 5) and bool(torch.isfinite(x).all())
    torch.manual_seed(1)
    clf = pkg.EGNN(in_node_nf=5, in_edge_nf=0, hidden_nf=32, device=DEV, n_layers=1).to(DEV).eval()
    mm = data.mean_mad(["alpha"])["alpha"]
    mae, records = model.evaluate_conditional(clf, "alpha", float(mm["mean"]), float(mm["mad"]), iterations=0, batch_size=4)
    assert np.isfinite(mae) and len(records) == 1 and bool(torch.isfinite(records[0]["label"]).all())
    pd.check()
