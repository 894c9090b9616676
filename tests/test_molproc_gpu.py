"""The sanitize / largest-fragment filters on an MI355X through Python (postprocess.process_molecules, ProcessedBatch, and
generate_molecules with the flags set) against the definition (tests/molproc_ref.py): every field of the batch under the four flag
combinations, both entries, a strided view of an xh, charges as the sampler holds them; the host objects against sdf.build_molecules of the
whole molecules reduced by the definition, an SDF round trip, the graph keys of the emitted largest fragments, and generate_molecules on a
small synthetic-weight model.  Integers and bit copies: torch.equal / array_equal, nothing excluded."""
import functools
import importlib
import warnings

import numpy as np
import pytest
import torch

import molgraph_cases as mc
import molproc_cases as pc
import molproc_ref as pr

pkg = importlib.import_module("bio-diffusion_amd")
pytestmark = pytest.mark.gpu
DEV = "cuda"


def _flat(cases):
    sizes = torch.tensor([len(c.types) for c in cases], dtype=torch.int64)
    types = torch.from_numpy(np.concatenate([c.types for c in cases]).astype(np.int64))
    return sizes, types


def assert_batch(got, want, x, types, charges, what):
    """Every field of a ProcessedBatch against a molproc_ref.Batch and the gathers it implies."""
    assert all(t.is_cuda for t in (got.positions, got.atom_types, got.num_nodes, got.mol_offsets, got.bonds, got.bond_offsets, got.src_atom,
                                   got.src_molecule, got.info, got.keep)), what
    for name in ("src_atom", "src_molecule", "mol_offsets", "bonds", "bond_offsets", "info"):
        assert np.array_equal(getattr(got, name).cpu().numpy(), getattr(want, name)), (what, name)
    assert np.array_equal(got.keep.cpu().numpy(), want.keep.astype(bool)), what
    assert np.array_equal(got.num_nodes.cpu().numpy(), np.diff(want.mol_offsets)) and len(got) == int(want.totals[2]), what
    src = torch.from_numpy(want.src_atom)
    assert torch.equal(got.positions.cpu().view(torch.int32), x[src].contiguous().view(torch.int32)), (what, "positions are bit copies")
    assert got.atom_types.dtype == types.dtype and torch.equal(got.atom_types.cpu(), types[src]), what
    if charges is None:
        assert got.charges is None, what
    else:
        assert got.charges.is_cuda and got.charges.shape[1:] == charges.shape[1:], what
        assert torch.equal(got.charges.cpu().view(torch.int32), charges[src].contiguous().view(torch.int32)), (what, "charges are bit copies")


@functools.lru_cache(maxsize=None)
def mixed_expected(flags):
    zs, caps = mc.qm9_type_tables()
    return pr.process_batch([(c.types, c.orders) for c in pc.mixed_batch(oversize=False)], zs, caps, flags)


@pytest.mark.parametrize("flags", (0, 1, 2, 3))
def test_process_molecules_from_orders_equals_the_definition(flags):
    """The mixed batch (0 .. 192 atoms, ties, interleaved fragments, singletons, atoms outside the vocabulary, caps) with the orders given,
    charges [N, 1] fp32; the tuples are slices of the same batch."""
    cases = pc.mixed_batch(oversize=False)
    sizes, types = _flat(cases)
    N = int(sizes.sum())
    g = torch.Generator().manual_seed(flags)
    x, charges = torch.randn(N, 3, generator=g), torch.randint(-2, 3, (N, 1), generator=g).float()
    orders = torch.from_numpy(np.concatenate([np.asarray(c.orders, np.uint8).reshape(-1) for c in cases])).to(DEV)
    got = pkg.process_molecules(x.to(DEV), types.to(DEV), sizes, pkg.dataset_info("qm9"), charges=charges.to(DEV), sanitize=bool(flags & 1),
                                largest_frag=bool(flags & 2), orders=orders, limit_bonds_to_one=False)
    want = mixed_expected(flags)
    assert_batch(got, want, x, types, charges, f"from orders flags={flags}")
    tuples = got.tuples()
    assert len(tuples) == len(got)
    off = want.mol_offsets
    for k, (pos, at, ch) in enumerate(tuples):
        src = torch.from_numpy(want.src_atom[off[k]:off[k + 1]])
        assert not pos.is_cuda and torch.equal(pos, x[src]) and torch.equal(at, types[src]) and torch.equal(ch, charges[src]), k
    if flags == 0:                                                    # an identity compaction
        assert torch.equal(got.positions.cpu(), x) and torch.equal(got.num_nodes.cpu(), sizes) and torch.equal(got.atom_types.cpu(), types)


def test_a_molecule_of_193_atoms_is_refused_on_the_host():
    c = {x.label: x for x in pc.mixed_batch()}["random n=193"]
    with pytest.raises(ValueError, match="193"):
        pkg.process_molecules(torch.zeros(193, 3, device=DEV), torch.from_numpy(c.types.astype(np.int64)).to(DEV), torch.tensor([193]),
                              pkg.dataset_info("qm9"), largest_frag=True)
    with pytest.raises(ValueError):
        pkg.process_molecules(torch.zeros(4, 3, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV), torch.tensor([3]), pkg.dataset_info("qm9"))


def _clouds(ds, drop_bad_type=False):
    out = [c for c in mc.clouds(ds) if len(c.types) <= pr.MAX_ATOMS]
    orders = [o for c, o in zip(mc.clouds(ds), pc.cloud_orders(ds, ds == "geom")) if len(c.types) <= pr.MAX_ATOMS]
    if drop_bad_type:
        keep = [k for k, c in enumerate(out) if "type 16" not in c.label]
        out, orders = [out[k] for k in keep], [orders[k] for k in keep]
    return out, orders


@pytest.mark.parametrize("ds", ("qm9", "geom"))
def test_process_molecules_from_positions_on_a_view_of_xh(ds):
    """The distance rule with the data set's own limit_bonds_to_one on lattice clouds (an atom outside the vocabulary among them), the
    positions a strided view of a wider xh, no charges; both flags, and largest_frag alone."""
    clouds, orders = _clouds(ds)
    sizes, types = _flat(clouds)
    x = torch.from_numpy(np.concatenate([c.x for c in clouds]))
    xh = torch.full((len(x), 9), 1.0e30, device=DEV)
    xh[:, :3] = x.to(DEV)
    zs, caps = mc.ds_type_tables(ds)
    for flags in (3, 2):
        got = pkg.process_molecules(xh[:, :3], types.to(DEV), sizes, pkg.dataset_info(ds), sanitize=bool(flags & 1), largest_frag=True)
        want = pr.process_batch([(c.types, o) for c, o in zip(clouds, orders)], zs, caps, flags)
        assert_batch(got, want, x, types, None, f"from positions {ds} flags={flags}")
        assert all(ch is None for _, _, ch in got.tuples())


def _reduce(whole, one):
    """A whole sdf.Molecule cut down to the atoms the definition keeps: the bonds keep their order."""
    new = one.new_index
    return pkg.Molecule(symbols=[whole.symbols[a] for a in one.atoms], positions=whole.positions[one.atoms],
                        bonds=[(new[i], new[j], o) for i, j, o in whole.bonds if new[i] >= 0 and new[j] >= 0],
                        charges=None if whole.charges is None else whole.charges[one.atoms])


@pytest.mark.parametrize("ds", ("qm9", "geom"))
def test_molecules_equal_build_molecules_reduced_and_round_trip_through_sdf(ds, tmp_path):
    clouds, orders = _clouds(ds, drop_bad_type=True)
    sizes, types = _flat(clouds)
    x = torch.from_numpy(np.concatenate([c.x for c in clouds])).to(DEV)
    charges = (torch.arange(len(x)) % 3 - 1).float().reshape(-1, 1).to(DEV)
    info = pkg.dataset_info(ds)
    zs, caps = mc.ds_type_tables(ds)
    whole = pkg.build_molecules(x, types.to(DEV), sizes, info, charges=charges)
    for flags in (3, 2, 1):
        ones = [pr.process_one(c.types, o, zs, caps, flags) for c, o in zip(clouds, orders)]
        want = [_reduce(w, one) for w, one in zip(whole, ones) if one.kept]
        got = pkg.process_molecules(x, types.to(DEV), sizes, info, charges=charges, sanitize=bool(flags & 1), largest_frag=bool(flags & 2)).molecules()
        assert len(got) == len(want) and 0 < len(got)
        for a, b in zip(got, want):
            assert a.symbols == b.symbols and a.bonds == b.bonds and np.array_equal(a.positions, b.positions)
            assert np.array_equal(a.charges, b.charges)
        if flags != 3:
            continue
        path = tmp_path / f"{ds}.sdf"
        pkg.write_sdf_file(path, got)
        back = pkg.sdf.read_sdf_file(path)
        assert len(back) == len(got)
        for a, b in zip(back, got):
            assert a.symbols == b.symbols and a.bonds == b.bonds
            assert len(b.symbols) == 0 or np.abs(a.positions - b.positions).max() <= 5.0e-5 + 1e-9        # %10.4f
            assert np.array_equal(np.zeros(len(b.symbols), int) if a.charges is None else a.charges, b.charges)


def test_keys_of_the_emitted_largest_fragments_are_the_keys_of_the_source():
    """The graph key is the key of the largest fragment: cutting the fragment out must not change it."""
    clouds, _ = _clouds("qm9")
    sizes, types = _flat(clouds)
    x = torch.from_numpy(np.concatenate([c.x for c in clouds])).to(DEV)
    info = pkg.dataset_info("qm9")
    keys, src_info = pkg.molecule_graph_keys(x, types.to(DEV), sizes, info)
    got = pkg.process_molecules(x, types.to(DEV), sizes, info, largest_frag=True)
    assert len(got) == len(clouds) and torch.equal(got.info, src_info)
    keys2, info2 = pkg.molecule_graph_keys(got.positions, got.atom_types, got.num_nodes, info)
    assert torch.equal(keys2, keys[got.src_molecule]) and torch.equal(info2[:, 2], src_info[:, 2]) and torch.equal(info2[:, 3], src_info[:, 2])
    assert bool((info2[:, 1] == (src_info[:, 3] > 0).to(torch.int32)).all())             # one fragment each
    a, b = pkg.GraphMolecularMetrics(info), pkg.GraphMolecularMetrics(info)
    a.update(keys, torch.ones_like(src_info))
    b.update(keys2, torch.ones_like(info2))
    assert a.compute() == b.compute()


@pytest.fixture(scope="module")
def model():
    cfgs = pkg.default_cfgs("qm9")
    cfgs["diffusion_cfg"]["num_timesteps"] = 6
    torch.manual_seed(0)
    m = pkg.QM9MoleculeGenerationDDPM(**cfgs)
    with torch.no_grad():
        for p in m.ddpm.dynamics_network.parameters():
            if p.dim() == 2:
                p.mul_(0.25)
    return m.cuda()


def _parent_tuples(model, x, one_hot, charges, batch_index):
    """What generate_molecules returns with both flags off: the per-molecule slices."""
    at = one_hot.argmax(-1)
    counts = torch.unique_consecutive(batch_index, return_counts=True)[1].tolist()
    out, o = [], 0
    for n in counts:
        out.append((x[o:o + n].cpu(), at[o:o + n].cpu(), charges[o:o + n].cpu() if model.include_charges else None))
        o += n
    return out


def _same(a, b):
    return len(a) == len(b) and all((u is None and v is None) or torch.equal(u, v) for s, t in zip(a, b) for u, v in zip(s, t))


def test_generate_molecules_with_the_flags_is_process_molecules_of_its_flat_output(model):
    nn_ = torch.tensor([9, 5, 12, 7, 3])
    kw = dict(num_nodes=nn_, num_timesteps=6, seed=11)
    x, one_hot, charges, bi = model.sample(len(nn_), **kw)
    plain = model.generate_molecules(num_samples=len(nn_), **kw)
    assert _same(plain, _parent_tuples(model, x, one_hot, charges, bi))                  # both flags off: the parent's result
    for sanitize, largest in ((True, True), (False, True), (True, False)):
        got = model.generate_molecules(num_samples=len(nn_), sanitize=sanitize, largest_frag=largest, **kw)
        want = pkg.process_molecules(x, one_hot.argmax(-1), nn_, model.dataset_info, charges=charges if model.include_charges else None,
                                     sanitize=sanitize, largest_frag=largest)
        assert _same(got, want.tuples())
        if not sanitize:
            assert len(got) == len(nn_) and [len(g[1]) for g in got] == want.info[:, 2].tolist()          # every molecule, its largest fragment
    built = model.generate_molecules(num_samples=len(nn_), largest_frag=True, molecule_builder=lambda pos, at, info: (len(at), info["name"]), **kw)
    lf = pkg.process_molecules(x, one_hot.argmax(-1), nn_, model.dataset_info, largest_frag=True)
    assert built == [(int(n), model.dataset_info["name"]) for n in lf.num_nodes.tolist()]
    # a chain: T one-molecule entries, the flags per frame
    frames = model.generate_molecules(num_samples=1, num_nodes=torch.tensor([7]), sample_chain=True, seed=3)
    cut = model.generate_molecules(num_samples=1, num_nodes=torch.tensor([7]), sample_chain=True, largest_frag=True, seed=3)
    pos = torch.cat([f[0] for f in frames]).to(DEV)
    at = torch.cat([f[1] for f in frames]).to(DEV)
    want = pkg.process_molecules(pos, at, torch.full((len(frames),), 7), model.dataset_info, largest_frag=True)
    assert len(cut) == len(frames) == 6 and all(c[2] is None for c in cut)
    assert _same([c[:2] for c in cut], [t[:2] for t in want.tuples()])


def test_relax_iter_and_add_hydrogens_warn_and_change_nothing(model):
    kw = dict(num_samples=3, num_nodes=torch.tensor([6, 4, 8]), num_timesteps=6, seed=5)
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)
        plain = model.generate_molecules(**kw)                        # no warning without them
    with pytest.warns(UserWarning, match="relax_iter"):
        relaxed = model.generate_molecules(relax_iter=200, **kw)
    with pytest.warns(UserWarning, match="add_hydrogens"):
        hydrogens = model.generate_molecules(add_hydrogens=True, largest_frag=True, **kw)
    assert _same(relaxed, plain)
    assert _same(hydrogens, model.generate_molecules(largest_frag=True, **kw))
