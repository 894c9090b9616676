"""Validity, uniqueness and novelty on an MI355X through the package: molecule_graph_keys and MoleculeDataset.graph_keys against the definition
(tests/molgraph_ref.py), GraphMolecularMetrics fed in chunks, and sample_and_analyze with metrics attached -- in its three modes -- against the
reference's bookkeeping applied to the definition on the very batches the driver sampled."""
import importlib

import numpy as np
import pytest
import torch

import data_cases as dc
import molgraph_cases as mc
import molgraph_ref as ref
import stability_cases as sc

pkg = importlib.import_module("bio-diffusion_amd")
pytestmark = pytest.mark.gpu
DEV = "cuda"


def _flat(clouds):
    x = torch.from_numpy(np.concatenate([c.x for c in clouds])).to(DEV)
    t = torch.from_numpy(np.concatenate([c.types for c in clouds]).astype(np.int64)).to(DEV)
    return x, t, torch.tensor([len(c.types) for c in clouds])


@pytest.mark.parametrize("ds", sc.DATASETS)
def test_molecule_graph_keys_equals_the_definition(ds):
    """The clouds through the public entry: the limit the reference uses for the data set (GEOM: single bonds only), `xh` with its row stride,
    caps overridden by symbol, and the orders of sdf.bond_order_matrices fed back in."""
    clouds = mc.clouds(ds)
    x, t, sizes = _flat(clouds)
    info_ds = pkg.dataset_info(ds)
    keys, info = pkg.molecule_graph_keys(x, t, sizes, info_ds)
    assert keys.dtype == torch.int64 and info.dtype == torch.int32 and keys.is_cuda and info.shape == (len(clouds), 4)
    want = mc.cloud_expected(ds, ds == "geom")
    assert np.array_equal(keys.cpu().numpy(), np.array([w[0] for w in want], np.int64))
    assert np.array_equal(info.cpu().numpy(), np.array([w[1] for w in want], np.int32))
    xh = torch.cat([x, torch.full((len(x), 6), 1.0e30, device=DEV)], 1)
    k2, i2 = pkg.molecule_graph_keys(xh[:, :3], t, sizes, info_ds)
    assert torch.equal(k2, keys) and torch.equal(i2, info)
    tb = sc.tables(ds)
    zs, caps = mc.ds_type_tables(ds, {"C": 2, "O": -1})
    want = [ref.key_from_positions(c.x, c.types, zs, caps, tb.bonds, tb.margins, ds == "geom") for c in clouds[:4]]
    x4, t4, s4 = _flat(clouds[:4])
    k4, i4 = pkg.molecule_graph_keys(x4, t4, s4, info_ds, valence_caps={"C": 2, "O": -1})
    assert [int(v) for v in k4.tolist()] == [w[0] for w in want] and [tuple(r) for r in i4.tolist()] == [w[1] for w in want]
    small = [c for c in clouds if len(c.types) <= 65]
    xs, ts, ss = _flat(small)
    ks, is_ = pkg.molecule_graph_keys(xs, ts, ss, info_ds)
    blocks = pkg.bond_order_matrices(xs, ts, ss, info_ds)                # GEOM: single bonds only, as above
    orders = torch.cat([torch.as_tensor(b).to(DEV, torch.uint8).reshape(-1) for b in blocks]).contiguous()
    ko, io = pkg.molecule_graph_keys(xs, ts, ss, info_ds, orders=orders)
    assert torch.equal(ko, ks) and torch.equal(io, is_)


def _golden_dataset():
    return pkg.MoleculeDataset(dc.raw(), DEV)


def _dataset_reference(ds, info, caps_by_symbol=None):
    tb = sc.tables("qm9")
    zs, caps = mc.qm9_type_tables(caps_by_symbol)
    z, pos, ptr = ds.z.cpu().numpy(), ds.pos.cpu().numpy(), ds.atom_ptr.cpu().numpy()
    out = []
    for a, b in zip(ptr[:-1], ptr[1:]):
        assert b - a <= 25                                            # torch.cdist's direct path, as in the kernel
        out.append(ref.key_from_positions(pos[a:b], z[a:b], zs, caps, tb.bonds, tb.margins, False, types_are_atomic_numbers=True))
    return out


def test_dataset_graph_keys_equals_the_definition_per_molecule():
    """tests/golden/data_small.npz: the sorted distinct keys of the molecules that are valid and in one fragment; with a cap that invalidates
    every carbon-bearing molecule the set shrinks accordingly."""
    ds = _golden_dataset()
    info = pkg.dataset_info("qm9")
    for caps in (None, {"C": 1}):
        per_mol = _dataset_reference(ds, info, caps)
        assert len(per_mol) == ds.M >= 8
        want = sorted({k for k, (valid, frags, _, _) in per_mol if valid == 1 and frags == 1})
        got = ds.graph_keys(info, valence_caps=caps)
        assert got.dtype == torch.int64 and got.is_cuda and got.tolist() == want, caps
    # a molecule in two pieces and one with an element outside QM9's vocabulary stay out
    confs = [np.array([[6, 0, 0, 0], [8, 1.2, 0, 0]], np.float32), np.array([[6, 0, 0, 0], [8, 1.2, 0, 0], [1, 9, 9, 9]], np.float32),
             np.array([[6, 0, 0, 0], [16, 1.2, 0, 0]], np.float32)]
    ds3 = pkg.MoleculeDataset.from_conformers(confs, DEV, included_species=[1, 6, 8, 16])
    co = ref.graph_key([6, 8], [[0, 0], [2, 0]], [4, 2])
    assert co[1] == (1, 1, 2, 2) and ds3.graph_keys(info).tolist() == [co[0]]


def test_metrics_in_three_chunks_equal_one():
    clouds = [c for ds in sc.DATASETS for c in mc.clouds(ds) if len(c.types) <= 65][:18]
    clouds = clouds + clouds[:5]                                      # duplicates: uniqueness below 1
    info_ds = pkg.dataset_info("qm9")
    clouds = [c for c in clouds if (c.types < 5).all()] + [mc.Cloud(np.array([[0, 0, 0], [1.1, 0, 0]], np.float32), np.array([1, 0], np.int32), "C-H")] * 2
    x, t, sizes = _flat(clouds)
    keys, info = pkg.molecule_graph_keys(x, t, sizes, info_ds)
    valid_keys = keys[info[:, 0] == 1]
    assert 0 < len(valid_keys) < len(keys)
    known = valid_keys[:1]
    one = pkg.GraphMolecularMetrics(info_ds, dataset_keys=known)
    one.update(keys, info)
    three = pkg.GraphMolecularMetrics(info_ds, dataset_keys=known)
    for k, i in zip(torch.chunk(keys, 3), torch.chunk(info, 3)):
        three.update(k, i)
    want = ref.reference_metrics(keys.tolist(), info[:, 0].tolist(), known.tolist())
    assert one.compute() == three.compute() == want and 0 < want[0] < 1 and want[1] < 1
    off = np.r_[0, np.cumsum(sizes.numpy())]
    generated = [(x[a:b], t[a:b]) for a, b in zip(off[:-1], off[1:])]
    assert pkg.GraphMolecularMetrics(info_ds, dataset_keys=known).evaluate(generated) == want


# ---- the evaluation driver --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    cfgs = pkg.default_cfgs("qm9")
    torch.manual_seed(0)
    model = pkg.QM9MoleculeGenerationDDPM(**cfgs)
    with torch.no_grad():
        for p in model.ddpm.dynamics_network.parameters():
            if p.dim() == 2:
                p.mul_(0.25)
    model = model.cuda()
    yield model
    model.ddpm.release_lanes()


def _run(model, **mode):
    torch.manual_seed(5)
    return model.sample_and_analyze(num_samples=23, batch_size=10, num_timesteps=25, **mode)


def test_sample_and_analyze_fills_the_three_metrics(model):
    """Without attach_molecular_metrics the three entries are None; with it they are the reference's bookkeeping on the definition's keys of
    the captured batches, and the other statistics are untouched."""
    assert model.molecular_metrics is None
    plain = _run(model)
    assert plain["validity"] is None and plain["uniqueness"] is None and plain["novelty"] is None
    metrics = model.attach_molecular_metrics()
    assert metrics is model.molecular_metrics and isinstance(metrics, pkg.GraphMolecularMetrics)
    seen = []
    orig = pkg.mol_gen_ddpm.molecule_graph_keys

    def spy(xh, types, num_nodes, info, *a, **k):
        r = orig(xh, types, num_nodes, info, *a, **k)
        seen.append((xh.cpu().numpy().copy(), types.cpu().numpy().copy(), num_nodes.cpu().numpy().copy()))
        return r

    pkg.mol_gen_ddpm.molecule_graph_keys = spy
    try:
        res = _run(model)
    finally:
        pkg.mol_gen_ddpm.molecule_graph_keys = orig
    assert [len(s[2]) for s in seen] == [10, 10, 3]
    tb = sc.tables("qm9")
    zs, caps = mc.qm9_type_tables()
    keys, valid = [], []
    for xh, types, nn_ in seen:
        off = np.r_[0, np.cumsum(nn_)]
        for a, b in zip(off[:-1], off[1:]):
            k, info = ref.key_from_positions(np.ascontiguousarray(xh[a:b, :3]), types[a:b], zs, caps, tb.bonds, tb.margins, False, direct=True)
            keys.append(k)
            valid.append(info[0])
    want = ref.reference_metrics(keys, valid, None)
    print("sample_and_analyze metrics:", [res[k] for k in ("validity", "uniqueness", "novelty")], "definition:", want)
    assert [res["validity"], res["uniqueness"], res["novelty"]] == want and all(isinstance(res[k], float) for k in ("validity", "uniqueness", "novelty"))
    for k in ("mol_stable", "atm_stable"):
        assert res[k] == plain[k]
    assert res["kl_div_atom_types"] == plain["kl_div_atom_types"] or np.isnan(plain["kl_div_atom_types"])
    # novelty against half of what was generated: the same accumulated keys, another data set
    kept = sorted({k for k, v in zip(keys, valid) if v == 1})
    metrics.dataset_keys = torch.tensor(kept[::2] + [12345], dtype=torch.int64).sort().values
    assert metrics.compute() == ref.reference_metrics(keys, valid, kept[::2] + [12345])
    model.molecular_metrics = None
    again = _run(model)
    assert again == plain or (np.isnan(plain["kl_div_atom_types"]) and {k: v for k, v in again.items() if k != "kl_div_atom_types"} ==
                              {k: v for k, v in plain.items() if k != "kl_div_atom_types"})


def test_metrics_do_not_depend_on_the_sampling_mode(model):
    model.attach_molecular_metrics(dataset=_golden_dataset())
    try:
        seq = _run(model)
        con = _run(model, concurrent_batches=2)
        model.ddpm.release_lanes()
        pck = _run(model, packed_batches=2)
    finally:
        model.molecular_metrics = None
    for k in ("validity", "uniqueness", "novelty", "mol_stable", "atm_stable"):
        assert isinstance(seq[k], float) and seq[k] == con[k] == pck[k], k
