"""The GEOM-Drugs conformer file on an MI355X, through its C ABI (include/gcdm_geom.h) and through data.py: the ingestion against the
reference's own molecules (tests/golden/geom_small.npz) with torch.equal under every chunking, the device-wide scans at the edges of their
tile against numpy, the ragged gather, the flags, MoleculeDataset.geom_splits against the reference's sorted splits and against
from_conformers on its data_list, every batch of the sequential and of a plain loader against the concatenation of the reference's items, and
iteration without a device-to-host copy.  Outputs are pre-filled with NaN / -1 / 0xAB: an element the kernels leave unwritten fails the
comparison, and GUARD further elements behind every capacity show a store outside it."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import geom_cases as gc

pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tile():
    return int(native.load_ops().gcdm_geom_workspace_bytes(native.GEOM_WS_TILE, 0))


def ingest_cabi(rows, remove_h, chunk_rows, cap_atoms=None, cap_mols=None):
    """gcdm_geom_ingest chunk by chunk and gcdm_geom_finish on pre-filled buffers with GUARD elements behind each capacity."""
    lib = native.load_ops()
    rows = np.array(rows, dtype=np.float64)
    R = len(rows)
    cap_atoms = R if cap_atoms is None else cap_atoms
    cap_mols = R if cap_mols is None else cap_mols
    z = torch.full((cap_atoms + GUARD,), -1, dtype=torch.int32, device=DEV)
    pos = torch.full((cap_atoms + GUARD, 3), float("nan"), dtype=torch.float32, device=DEV)
    atom_ptr = torch.full((cap_mols + 1 + GUARD,), -1, dtype=torch.int64, device=DEV)
    state = torch.zeros(native.GEOM_STATE_WORDS, dtype=torch.int64, device=DEV)
    MA = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    dev_rows = torch.from_numpy(rows).to(DEV)
    for r0 in range(0, R, chunk_rows):
        r = min(chunk_rows, R - r0)
        ws = torch.full((int(lib.gcdm_geom_workspace_bytes(native.GEOM_WS_BYTES, r)),), 0xAB, dtype=torch.uint8, device=DEV)
        st = lib.gcdm_geom_ingest(_p(dev_rows[r0:r0 + r]), r, int(remove_h), _p(state), _p(z), _p(pos), _p(atom_ptr), cap_atoms, cap_mols, _p(ws),
                                  _p(flags), _stream())
        assert st == 0
    assert lib.gcdm_geom_finish(_p(state), _p(atom_ptr), cap_mols, _p(MA), _p(flags), _stream()) == 0
    torch.cuda.synchronize()
    M, A = (int(v) for v in MA.cpu())
    return dict(z=z.cpu(), pos=pos.cpu(), atom_ptr=atom_ptr.cpu(), M=M, A=A, flags=int(flags.item()), cap_atoms=cap_atoms, cap_mols=cap_mols)


def assert_ingest(got, sizes, z, pos, what):
    M, A = len(sizes), int(sizes.sum())
    assert got["flags"] == 0 and (got["M"], got["A"]) == (M, A), what
    ptr = torch.zeros(M + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.from_numpy(np.array(sizes, dtype=np.int64)), 0)
    assert torch.equal(got["atom_ptr"][:M + 1], ptr), what
    assert torch.equal(got["z"][:A], torch.from_numpy(np.array(z))), what
    assert torch.equal(got["pos"][:A].view(torch.int32), torch.from_numpy(np.array(pos)).view(torch.int32)), what          # bits
    # nothing behind what was appended
    assert bool((got["atom_ptr"][M + 1:] == -1).all()) and bool((got["z"][A:] == -1).all()) and bool(torch.isnan(got["pos"][A:]).all()), what


def _chunkings(remove_h):
    """all rows; 1; a value that cuts inside a molecule; a value that ends exactly on a boundary (of the array as the kernel sees it: with
    remove_h the rows are still the file's)."""
    g = gc.fixture()
    rows = g["rows"]
    mol_id = rows[:, 0].astype(int)
    bounds = set((np.nonzero(mol_id[:-1] - mol_id[1:])[0] + 1).tolist())
    inside = next(c for c in range(5, 40) if c not in bounds and 2 * c not in bounds)
    on = next(c for c in sorted(bounds) if c >= 7)
    return {"all": len(rows), "one": 1, "inside": inside, "boundary": on}


@pytest.mark.parametrize("chunking", ["all", "one", "inside", "boundary"])
@pytest.mark.parametrize("remove_h", [False, True])
def test_ingest_equals_the_reference_under_every_chunking(remove_h, chunking):
    """chunk_rows = 1 puts every id change, every all-hydrogen conformer and the join of the two id-9 conformers on a chunk edge."""
    g = gc.fixture()
    t = gc.tag(remove_h)
    got = ingest_cabi(g["rows"], remove_h, _chunkings(remove_h)[chunking])
    assert_ingest(got, g[f"ing_{t}_sizes"], g[f"ing_{t}_z"], g[f"ing_{t}_pos"], (remove_h, chunking))


@pytest.mark.parametrize("remove_h", [False, True])
def test_scans_at_the_edges_of_their_tile(remove_h):
    T = _tile()
    assert T == native.GEOM_TILE
    for R, long_run in ((1, 0), (T - 1, 0), (T, 0), (T + 1, 0), (3 * T + 1, T + 5)):
        rows = gc.generated_rows(R, seed=R, long_run=long_run)
        sizes, z, pos = gc.ingest_numpy(rows, remove_h)
        if long_run and not remove_h:
            assert sizes[0] > T
        assert_ingest(ingest_cabi(rows, remove_h, R), sizes, z, pos, (R, "one chunk"))
        if R > T:
            assert_ingest(ingest_cabi(rows, remove_h, T + 1), sizes, z, pos, (R, "chunks of T + 1"))
    # a chunk of hydrogens only, and a file of them
    rows = gc.generated_rows(40, seed=1)
    rows[10:30, 1] = 1.0
    sizes, z, pos = gc.ingest_numpy(rows, remove_h)
    assert_ingest(ingest_cabi(rows, remove_h, 10), sizes, z, pos, "a chunk without a kept row")
    rows[:, 1] = 1.0
    sizes, z, pos = gc.ingest_numpy(rows, remove_h)
    got = ingest_cabi(rows, remove_h, 16)
    assert_ingest(got, sizes, z, pos, "hydrogen only")
    assert got["M"] == (0 if remove_h else len(sizes)) and int(got["atom_ptr"][0]) == 0


@pytest.mark.parametrize("what", ["zero", "negative", "nan"])
def test_bad_rows_raise_the_flag_and_are_still_written(what):
    g = gc.fixture()
    rows = g["rows"].copy()
    r = 100 + int(np.flatnonzero(rows[100:, 1] != 1.0)[0])          # a row that remove_h keeps
    if what == "zero":
        rows[r, 1] = 0.25
    elif what == "negative":
        rows[r, 1] = -3.0
    else:
        rows[r, 3] = float("nan")
    for remove_h in (False, True):
        sizes, z, pos = gc.ingest_numpy(rows, remove_h)
        got = ingest_cabi(rows, remove_h, 64)
        assert got["flags"] == native.GEOM_FLAG_BAD_ROW and (got["M"], got["A"]) == (len(sizes), int(sizes.sum()))
        A = got["A"]
        assert torch.equal(got["z"][:A], torch.from_numpy(z))
        assert np.array_equal(got["pos"][:A].numpy(), pos, equal_nan=True) and int(np.isnan(pos).sum()) == (what == "nan")
        assert torch.equal(got["atom_ptr"][1:got["M"] + 1], torch.cumsum(torch.from_numpy(sizes), 0))


def test_capacity_raises_the_flag_and_nothing_is_written_behind_it():
    g = gc.fixture()
    sizes, z = g["ing_h_sizes"], g["ing_h_z"]
    M, A = len(sizes), int(sizes.sum())
    ptr = np.concatenate(([0], np.cumsum(sizes)))
    for chunk in (A, 37):
        got = ingest_cabi(g["rows"], False, chunk, cap_mols=M - 1)
        assert got["flags"] == native.GEOM_FLAG_CAPACITY and (got["M"], got["A"]) == (M, A)          # counted, not written
        assert torch.equal(got["atom_ptr"][:M - 1], torch.from_numpy(ptr[:M - 1])) and bool((got["atom_ptr"][M - 1:] == -1).all())
        assert torch.equal(got["z"][:A], torch.from_numpy(z.copy()))
        got = ingest_cabi(g["rows"], False, chunk, cap_atoms=A - 1)
        assert got["flags"] == native.GEOM_FLAG_CAPACITY and (got["M"], got["A"]) == (M, A)
        assert torch.equal(got["z"][:A - 1], torch.from_numpy(z[:A - 1].copy())) and bool((got["z"][A - 1:] == -1).all())
        assert bool(torch.isnan(got["pos"][A - 1:]).all()) and torch.equal(got["atom_ptr"][:M + 1], torch.from_numpy(ptr))
    got = ingest_cabi(g["rows"], False, A, cap_mols=M)                                              # exactly enough
    assert got["flags"] == 0 and int(got["atom_ptr"][M]) == A


# ---- the ragged gather ----------------------------------------------------------------------------------------------------------------------
def _source(remove_h):
    g = gc.fixture()
    t = gc.tag(remove_h)
    sizes = g[f"ing_{t}_sizes"]
    ptr = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    return sizes, ptr, g[f"ing_{t}_z"], g[f"ing_{t}_pos"]


def gather_cabi(remove_h, order, ptr_out=None, A_out=None, M_in=None):
    lib = native.load_ops()
    sizes, ptr, z, pos = _source(remove_h)
    order = np.array(order, dtype=np.int64)
    if ptr_out is None:
        ptr_out = np.concatenate(([0], np.cumsum(sizes[order]))).astype(np.int64)
    A_out = int(ptr_out[-1]) if A_out is None else A_out
    z_out = torch.full((A_out + GUARD,), -1, dtype=torch.int32, device=DEV)
    pos_out = torch.full((A_out + GUARD, 3), float("nan"), dtype=torch.float32, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    src = [torch.from_numpy(np.array(a)).to(DEV) for a in (ptr, z, pos)]
    o, po = torch.from_numpy(order).to(DEV), torch.from_numpy(np.array(ptr_out, dtype=np.int64)).to(DEV)
    st = lib.gcdm_geom_gather(_p(src[0]), _p(src[1]), _p(src[2]), len(sizes) if M_in is None else M_in, len(z), _p(o), _p(po), len(order), A_out,
                              _p(z_out), _p(pos_out), _p(flags), _stream())
    assert st == 0
    torch.cuda.synchronize()
    return z_out.cpu(), pos_out.cpu(), int(flags.item())


def _gathered(remove_h, order):
    sizes, ptr, z, pos = _source(remove_h)
    idx = np.concatenate([np.arange(ptr[m], ptr[m + 1]) for m in order]).astype(np.int64) if len(order) else np.zeros(0, dtype=np.int64)
    return torch.from_numpy(z[idx]), torch.from_numpy(pos[idx])


def test_gather_identity_reversal_and_the_reference_orders():
    g = gc.fixture()
    M = len(g["ing_h_sizes"])
    cases = [(False, np.arange(M)), (False, np.arange(M)[::-1].copy()), (False, np.array([], dtype=np.int64)), (False, np.array([7, 7, 0, 7]))]
    cases += [(gc.VARIANTS[v][0], g[f"{v}_{s}_order"]) for v in gc.VARIANTS for s in gc.SPLITS]
    for remove_h, order in cases:
        z_out, pos_out, flags = gather_cabi(remove_h, order)
        want_z, want_pos = _gathered(remove_h, order)
        A = len(want_z)
        assert flags == 0 and torch.equal(z_out[:A], want_z) and torch.equal(pos_out[:A].view(torch.int32), want_pos.view(torch.int32))
        assert bool((z_out[A:] == -1).all()) and bool(torch.isnan(pos_out[A:]).all())
    # the fixture's sorted splits are what the reference holds
    for v in gc.VARIANTS:
        for s in gc.SPLITS:
            want_z, want_pos = _gathered(gc.VARIANTS[v][0], g[f"{v}_{s}_order"])
            assert np.array_equal(want_z.numpy(), g[f"{v}_{s}_z"]) and np.array_equal(want_pos.numpy().view(np.uint32), g[f"{v}_{s}_x"].view(np.uint32))


def test_gather_skips_what_does_not_add_up_and_stays_inside_a_out():
    sizes, ptr, z, pos = _source(False)
    M = len(sizes)
    for bad in (M, -1):                                                      # an entry outside [0, M): its slots stay, the others are intact
        order = np.array([3, 9, bad, 5])
        ptr_out = np.concatenate(([0], np.cumsum([sizes[3], sizes[9], 4, sizes[5]])))
        z_out, pos_out, flags = gather_cabi(False, order, ptr_out=ptr_out)
        assert flags == native.GEOM_FLAG_ACCOUNT
        for k, m in ((0, 3), (1, 9), (3, 5)):
            assert torch.equal(z_out[ptr_out[k]:ptr_out[k + 1]], torch.from_numpy(z[ptr[m]:ptr[m + 1]].copy()))
            assert torch.equal(pos_out[ptr_out[k]:ptr_out[k + 1]], torch.from_numpy(pos[ptr[m]:ptr[m + 1]].copy()))
        assert bool((z_out[ptr_out[2]:ptr_out[3]] == -1).all()) and bool(torch.isnan(pos_out[ptr_out[2]:ptr_out[3]]).all())
    # a size that differs from the source's
    big = int(np.argmax(sizes))
    ptr_out = np.array([0, sizes[big] - 1])
    z_out, pos_out, flags = gather_cabi(False, np.array([big]), ptr_out=ptr_out)
    assert flags == native.GEOM_FLAG_ACCOUNT and bool((z_out == -1).all()) and bool(torch.isnan(pos_out).all())
    # A_out smaller than atom_ptr_out says: the flag, and no store at or behind A_out
    order = np.arange(M)[::-1].copy()
    ptr_out = np.concatenate(([0], np.cumsum(sizes[order])))
    A_out = int(ptr_out[-1]) - 3
    z_out, pos_out, flags = gather_cabi(False, order, ptr_out=ptr_out, A_out=A_out)
    want_z, want_pos = _gathered(False, order)
    assert flags == native.GEOM_FLAG_ACCOUNT
    assert torch.equal(z_out[:A_out], want_z[:A_out]) and torch.equal(pos_out[:A_out], want_pos[:A_out])
    assert bool((z_out[A_out:] == -1).all()) and bool(torch.isnan(pos_out[A_out:]).all())
    # M_in smaller than the order's entries
    _, _, flags = gather_cabi(False, np.array([2, 4]), M_in=4)
    assert flags == native.GEOM_FLAG_ACCOUNT


# ---- MoleculeDataset.geom_splits -------------------------------------------------------------------------------------------------------------
_SPLITS = {}


def splits(variant):
    if variant not in _SPLITS:
        g = gc.fixture()
        remove_h, filter_size = gc.VARIANTS[variant]
        _SPLITS[variant] = pkg.MoleculeDataset.geom_splits(np.array(g["rows"]), DEV, permutation=g[f"{variant}_perm"], filter_size=filter_size,
                                                           remove_h=remove_h, chunk_rows=50)
    return _SPLITS[variant]


def _reference_conformers(variant, split):
    g = gc.fixture()
    sizes, z, x = g[f"{variant}_{split}_sizes"], g[f"{variant}_{split}_z"], g[f"{variant}_{split}_x"]
    ptr = np.concatenate(([0], np.cumsum(sizes)))
    return [np.concatenate((z[a:b, None].astype(np.float32), x[a:b]), axis=1) for a, b in zip(ptr[:-1], ptr[1:])]


@pytest.mark.parametrize("variant", list(gc.VARIANTS))
def test_geom_splits_equal_the_reference_and_from_conformers(variant):
    g = gc.fixture()
    remove_h, _ = gc.VARIANTS[variant]
    dss = splits(variant)
    assert sorted(dss) == sorted(gc.SPLITS)
    species = g["atomic_nb_noh" if remove_h else "atomic_nb_h"]
    for split in gc.SPLITS:
        ds, key = dss[split], f"{variant}_{split}"
        sizes = g[f"{key}_sizes"]
        M = len(sizes)
        assert ds.M == len(ds) == M and ds.A == int(sizes.sum()) and ds.sorted_by_size is True and ds.max_atoms == int(sizes.max())
        assert np.array_equal(ds.num_atoms_host, sizes) and np.array_equal(ds.split_indices, g[f"{key}_split_indices"])
        assert torch.equal(ds.atom_ptr.cpu(), torch.from_numpy(np.concatenate(([0], np.cumsum(sizes)))))
        assert ds.z.dtype == torch.int32 and torch.equal(ds.z.cpu(), torch.from_numpy(g[f"{key}_z"].copy()))
        assert ds.pos.dtype == torch.float32 and torch.equal(ds.pos.cpu().view(torch.int32), torch.from_numpy(g[f"{key}_x"].copy()).view(torch.int32))
        assert torch.equal(ds.index.cpu(), torch.from_numpy(g[f"{key}_index"].copy())) and torch.equal(ds.index.cpu(), torch.arange(M))
        assert ds.included_species.tolist() == species.tolist() and ds.property_keys == []
        ref = pkg.MoleculeDataset.from_conformers(_reference_conformers(variant, split), DEV, included_species=species)
        for name in ("atom_ptr", "z", "pos", "index", "species"):
            assert torch.equal(getattr(ds, name), getattr(ref, name)), (split, name)
        assert ds.n_nodes_histogram() == ref.n_nodes_histogram() and ds.atom_type_histogram() == ref.atom_type_histogram()
        ds.check()


def test_geom_splits_from_the_file_with_its_permutation_next_to_it(tmp_path):
    g = gc.fixture()
    np.save(tmp_path / "GEOM_drugs_30.npy", g["rows"])
    np.save(tmp_path / "GEOM_permutation.npy", g["noh_f6_perm"])
    a = pkg.MoleculeDataset.from_geom_file(str(tmp_path / "GEOM_drugs_30.npy"), DEV, split="train", filter_size=6, remove_h=True)
    b = splits("noh_f6")["train"]                                 # chunks of 50 rows there, one chunk here
    for name in ("atom_ptr", "z", "pos", "index", "species"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(a.split_indices, b.split_indices)
    bad = g["rows"].copy()
    bad[17, 1] = 0.0
    with pytest.raises(ValueError, match="atomic number < 1"):
        pkg.MoleculeDataset.geom_splits(bad, DEV, permutation=g["h_all_perm"])
    with pytest.raises(ValueError, match="float64"):
        pkg.MoleculeDataset.geom_splits(g["rows"].astype(np.float32), DEV, permutation=g["h_all_perm"])
    with pytest.raises(ValueError, match="pass permutation"):
        pkg.MoleculeDataset.geom_splits(np.array(g["rows"]), DEV)


def _assert_batch(b, variant, split, first, B, layout_rows_present=True):
    g = gc.fixture()
    key = f"{variant}_{split}"
    ptr = np.concatenate(([0], np.cumsum(g[f"{key}_sizes"])))
    a0, a1 = int(ptr[first]), int(ptr[first + B])
    want = {k: torch.from_numpy(g[f"{key}_{k}"][a0:a1].copy()) for k in ("x", "one_hot", "mask")}
    want["index"] = torch.from_numpy(g[f"{key}_index"][first:first + B].copy())
    want["batch"] = torch.repeat_interleave(torch.arange(B), torch.from_numpy(g[f"{key}_sizes"][first:first + B].copy()))
    assert b.num_graphs == B
    for k, w in want.items():
        assert b[k].dtype == w.dtype and torch.equal(b[k].cpu(), w), (variant, split, first, k)


@pytest.mark.parametrize("variant", list(gc.VARIANTS))
def test_every_batch_equals_the_concatenation_of_the_reference_items(variant):
    g = gc.fixture()
    for split in gc.SPLITS:
        ds = splits(variant)[split]
        for layout in ("padded", "compact"):
            for bs, drop_last in ((3, False), (2, True)):
                counts = g[f"{variant}_{split}_bs{bs}_dl{int(drop_last)}_counts"]
                loader = ds.loader(bs, shuffle=False, drop_last=drop_last, layout=layout, sequential=True)
                batches = list(loader)
                assert len(batches) == len(loader) == len(counts) and [b.num_graphs for b in batches] == counts.tolist()
                first = 0
                for b in batches:
                    assert b.all_present is True
                    _assert_batch(b, variant, split, first, b.num_graphs)
                    first += b.num_graphs
        first = 0
        for b in ds.loader(4, shuffle=False, layout="compact"):             # a plain loader: batches of mixed sizes
            assert b.all_present is True
            _assert_batch(b, variant, split, first, b.num_graphs)
            first += b.num_graphs
        assert first == len(ds)
        ds.check()


def test_iterating_the_new_data_set_makes_no_device_to_host_copy():
    ds = splits("h_all")["train"]
    one = torch.ones(1, device=DEV)
    list(ds.loader(3, shuffle=False, sequential=True))          # the library is loaded, the allocator warm
    list(ds.loader(3, layout="compact"))
    loaders = [ds.loader(3, shuffle=False, sequential=True, layout=layout) for layout in ("padded", "compact")] + [ds.loader(3, seed=1, layout="compact")]
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
                assert len(batches) == len(loader) > 3
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not effective:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make a bare .item() raise on this build")
    ds.check()
