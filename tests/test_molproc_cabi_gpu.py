"""The sanitize / largest-fragment filters on an MI355X through their C ABI (gcdm_molproc_select, gcdm_molproc_emit; include/gcdm_molproc.h):
the molecules of tests/molgraph_cases.py and tests/molproc_cases.py under all four flag combinations, both entries (orders given, and the
distance rule on jittered lattice clouds), both type conventions, x_row_stride 3 and 9, charges present and absent, batches that straddle the
scan tiles, a batch of which nothing survives, a side stream.  Expected values are the definition's (tests/molproc_ref.py), compared as
integers or bits with array_equal on EVERY output; nothing is excluded.  Workspace and outputs are poisoned before each call -- 0xFF bytes,
NaN for positions; 0x7F bytes where -1 is a value the kernel may write (info, new_index, types_out) -- and every output is followed by
poisoned guard rows: an element left unwritten, or one written outside, fails."""
import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

import molgraph_cases as mc
import molproc_cases as pc
import molproc_ref as pr
import stability_cases as sc

pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype):
    a = np.ascontiguousarray(np.asarray(a, dtype))
    return torch.from_numpy(a.copy()).to(DEV) if a.size else torch.zeros(1, dtype=getattr(torch, np.dtype(dtype).name), device=DEV)


def _poisoned(rows, cols, dtype, byte=0xFF):
    """rows + GUARD rows of `byte` (NaN for floats); the kernel owns the first `rows`."""
    shape = (rows + GUARD,) + ((cols,) if cols else ())
    if dtype == torch.float32:
        return torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(byte)
    return t


def _host(t, rows, what):
    """The kernel's rows; the guard rows must still hold the poison."""
    a = t.cpu()
    guard = a[rows:].contiguous().view(torch.uint8).numpy()
    first = guard.reshape(-1)[:4].tobytes()
    assert guard.size and guard.tobytes() == first * (guard.size // 4), (what, "guard rows written")
    return a[:rows].numpy()


def tables(ds, limit, atomic_numbers=False, caps=None):
    return pkg.metrics.graph_tables(dict(sc.tables(ds).info), caps, limit_bonds_to_one=bool(limit), types_are_atomic_numbers=atomic_numbers)


def run(tb, types_list, flags, want, orders_list=None, x=None, stride=3, charges=False, what=""):
    """select, the read of totals, emit; every output against `want` (a molproc_ref.Batch).  Returns the outputs for further assertions."""
    lib = native.load_ops()
    sizes = np.array([len(t) for t in types_list], np.int64)
    M, N = len(sizes), int(sizes.sum())
    types_h = np.concatenate(types_list).astype(np.int32) if M else np.zeros(0, np.int32)
    rng = np.random.default_rng([N, M, flags])
    x_h = rng.normal(size=(N, 3)).astype(np.float32) if x is None else np.asarray(x, np.float32).reshape(N, 3)
    xd = torch.full((max(N, 1), stride), 1.0e30, dtype=torch.float32, device=DEV)          # what lies between the rows is not a coordinate
    xd[:N, :3] = torch.from_numpy(x_h).to(DEV)
    ch_h = (rng.integers(-2, 3, size=N).astype(np.float32) + 0.25) if charges else None
    chd = _dev(ch_h, np.float32) if charges else None
    td, off = _dev(types_h, np.int32), _dev(np.r_[0, np.cumsum(sizes)], np.int64)
    poff = orders = None
    if orders_list is not None:
        poff = _dev(np.r_[0, np.cumsum(sizes * sizes)][:-1], np.int64)
        orders = _dev(np.concatenate([np.asarray(o, np.uint8).reshape(-1) for o in orders_list]) if M else [], np.uint8)
    info, keep = _poisoned(M, 4, torch.int32, 0x7F), _poisoned(N, 0, torch.uint8)
    new_index, counts, totals = _poisoned(N, 0, torch.int32, 0x7F), _poisoned(M, 3, torch.int32), _poisoned(3, 0, torch.int64)
    ws_words = lib.gcdm_molproc_workspace_bytes(M) // 8
    ws = _poisoned(ws_words, 0, torch.int64)
    st = lib.gcdm_molproc_select(tb, _p(xd), stride, _p(td), _p(off), M, _p(poff), _p(orders), flags, _p(info), _p(keep), _p(new_index), _p(counts),
                                 _p(totals), _p(ws), _stream())
    assert st == 0, what
    torch.cuda.synchronize()
    got_totals = _host(totals, 3, (what, "totals"))
    print(f"{what}: totals {got_totals.tolist()} (definition {want.totals.tolist()})")
    assert np.array_equal(got_totals, want.totals), what              # before emit: the outputs are sized by the definition's totals
    assert np.array_equal(_host(info, M, (what, "info")), want.info), what
    assert np.array_equal(_host(counts, M, (what, "counts")), want.counts), what
    keep_h, new_h = _host(keep, N, (what, "keep")), _host(new_index, N, (what, "new_index"))
    assert np.array_equal(keep_h[want.written], want.keep[want.written]) and (keep_h[~want.written] == 0xFF).all(), what
    assert np.array_equal(new_h[want.written], want.new_index[want.written]) and (new_h[~want.written] == 0x7F7F7F7F).all(), what
    _host(ws, ws_words, (what, "workspace"))
    Np, nbp, Mp = (int(v) for v in want.totals)
    pos_out, types_out = _poisoned(Np, 3, torch.float32), _poisoned(Np, 0, torch.int32, 0x7F)
    ch_out = _poisoned(Np, 0, torch.float32) if charges else None
    src_atom, src_mol = _poisoned(Np, 0, torch.int64), _poisoned(Mp, 0, torch.int64)
    mol_off, bond_off, bonds = _poisoned(Mp + 1, 0, torch.int64), _poisoned(Mp + 1, 0, torch.int64), _poisoned(nbp, 3, torch.int32)
    st = lib.gcdm_molproc_emit(tb, _p(xd), stride, _p(td), _p(chd), _p(off), M, _p(poff), _p(orders), _p(keep), _p(new_index), _p(counts), _p(totals),
                               _p(ws), _p(pos_out), _p(types_out), _p(ch_out), _p(src_atom), _p(src_mol), _p(mol_off), _p(bonds), _p(bond_off),
                               _stream())
    assert st == 0, what
    torch.cuda.synchronize()
    out = dict(src_atom=_host(src_atom, Np, (what, "src_atom")), src_molecule=_host(src_mol, Mp, (what, "src_molecule")),
               mol_offsets=_host(mol_off, Mp + 1, (what, "mol_offsets")), bond_offsets=_host(bond_off, Mp + 1, (what, "bond_offsets")),
               bonds=_host(bonds, nbp, (what, "bonds")), pos=_host(pos_out, Np, (what, "pos")), types=_host(types_out, Np, (what, "types")),
               info=want.info, x=x_h, types_in=types_h, sizes=sizes)
    for name in ("src_atom", "src_molecule", "mol_offsets", "bond_offsets", "bonds"):
        assert np.array_equal(out[name], getattr(want, name)), (what, name)
    assert np.array_equal(out["pos"].view(np.int32), x_h[want.src_atom].view(np.int32).reshape(-1, 3)), (what, "positions are bit copies")
    assert np.array_equal(out["types"], types_h[want.src_atom]), (what, "types")
    if charges:
        got = _host(ch_out, Np, (what, "charges"))
        assert np.array_equal(got.view(np.int32), ch_h[want.src_atom].view(np.int32)), (what, "charges are bit copies")
    return out


@functools.lru_cache(maxsize=None)
def mixed_expected(flags, atomic_numbers):
    zs, caps = mc.qm9_type_tables()
    mols = [(mc.as_atomic_numbers(c.types) if atomic_numbers else c.types, c.orders) for c in pc.mixed_batch()]
    return pr.process_batch(mols, zs, caps, flags, atomic_numbers)


@pytest.mark.parametrize("atomic_numbers", (False, True))
@pytest.mark.parametrize("flags", (0, 1, 2, 3))
def test_mixed_batch_equals_the_definition(flags, atomic_numbers):
    """0 .. 193 atoms, ties, the largest fragment away from atom 0, interleaved fragments, singletons, atoms outside the vocabulary, caps
    overrun inside and outside the largest fragment, asymmetric order matrices; types as indices (with charges) and as atomic numbers."""
    cases = pc.mixed_batch()
    types = [mc.as_atomic_numbers(c.types) if atomic_numbers else c.types for c in cases]
    want = mixed_expected(flags, atomic_numbers)
    out = run(tables("qm9", 0, atomic_numbers), types, flags, want, [c.orders for c in cases], charges=not atomic_numbers,
              what=f"mixed batch flags={flags} atomic_numbers={atomic_numbers}")
    at = {c.label: m for m, c in enumerate(cases)}
    kept = {int(m): k for k, m in enumerate(out["src_molecule"])}
    size = lambda label: int(np.diff(out["mol_offsets"])[kept[at[label]]])
    assert tuple(want.info[at["random n=193"]]) == (-1, 0, 0, 193) and at["random n=193"] not in kept
    assert at["n=0"] in kept and size("n=0") == 0
    over_in, over_out = "CH5: C over its cap, in the largest fragment", "C5 + OH3: O over its cap, outside the largest fragment"
    assert (at[over_in] in kept) == (at[over_out] in kept) == (not flags & 1)          # the WHOLE molecule is sanitised
    if not flags & 1:
        assert size(over_out) == (5 if flags & 2 else 9)
    assert size("tie: C-O then C-N") == size("tie, interleaved: C-N holds atom 0") == (2 if flags & 2 else 4)
    a = int(out["mol_offsets"][kept[at["tie, interleaved: C-N holds atom 0"]]])
    first = int(np.r_[0, np.cumsum(out["sizes"])][at["tie, interleaved: C-N holds atom 0"]])
    assert out["src_atom"][a:a + 2].tolist() == ([first, first + 3] if flags & 2 else [first, first + 1])
    lone = "singletons, atom 0 outside the vocabulary: it is the largest fragment"
    if not flags & 1:
        assert out["types"][int(out["mol_offsets"][kept[at[lone]]])] == (16 if atomic_numbers else -1)


def test_identity_compaction_equals_its_input():
    """Both flags off: the output is the input, the bond lists what nonzero(tril(E, -1)) gives."""
    cases = pc.mixed_batch(oversize=False)
    zs, caps = mc.qm9_type_tables()
    want = pr.process_batch([(c.types, c.orders) for c in cases], zs, caps, 0)
    out = run(tables("qm9", 0), [c.types for c in cases], 0, want, [c.orders for c in cases], what="identity")
    sizes = out["sizes"]
    assert np.array_equal(out["pos"].view(np.int32), out["x"].view(np.int32)) and np.array_equal(out["types"], out["types_in"])
    assert np.array_equal(out["mol_offsets"], np.r_[0, np.cumsum(sizes)]) and np.array_equal(out["src_atom"], np.arange(sizes.sum()))
    assert np.array_equal(out["src_molecule"], np.arange(len(sizes)))
    tril = [np.tril(np.asarray(c.orders, np.int64), -1) for c in cases]
    for c, t in zip(cases, tril):                                     # an atom outside the vocabulary bonds to nothing
        bad = (c.types < 0) | (c.types >= len(zs))
        t[bad, :] = 0
        t[:, bad] = 0
    flat = [np.c_[np.nonzero(t)[0], np.nonzero(t)[1], t[np.nonzero(t)]] for t in tril]
    assert np.array_equal(out["bonds"], np.concatenate(flat).astype(np.int32))
    assert np.array_equal(out["bond_offsets"], np.r_[0, np.cumsum([len(f) for f in flat])])


def test_a_batch_of_which_nothing_survives():
    """Every molecule dropped: M' = N' = nb' = 0, both launches succeed, the offset lists are [0]."""
    by = {c.label: c for c in pc.mixed_batch()}
    cases = [by["CH5: C over its cap, in the largest fragment"], by["C5 + OH3: O over its cap, outside the largest fragment"],
             by["CO3 with two double bonds: C one over"], by["random n=193"], by["CH4 with type 99 at atom 2"]]
    zs, caps = mc.qm9_type_tables()
    for flags in (1, 3):
        want = pr.process_batch([(c.types, c.orders) for c in cases], zs, caps, flags)
        assert want.totals.tolist() == [0, 0, 0]
        out = run(tables("qm9", 0), [c.types for c in cases], flags, want, [c.orders for c in cases], charges=True, what=f"all dropped flags={flags}")
        assert out["mol_offsets"].tolist() == [0] and out["bond_offsets"].tolist() == [0]
    empty = pr.process_batch([], zs, caps, 3)
    out = run(tables("qm9", 0), [], 3, empty, [], what="no molecule at all")
    assert out["mol_offsets"].tolist() == [0] and out["bond_offsets"].tolist() == [0]


@pytest.mark.parametrize("M", pc.SCAN_SIZES)
def test_scans_across_the_tile_seams(M):
    """M = 1, T - 1, T, T + 1, 2 T + 3 molecules of 0 - 4 atoms, dropped ones among them: the offsets cross every tile seam with non-zero
    carries in all three scans (tests/test_molproc_cpu.py checks that of the cases)."""
    zs, caps = mc.qm9_type_tables()
    mols = pc.scan_batch(M)
    want = pr.process_batch(mols, zs, caps, 3)
    run(tables("qm9", 0), [t for t, _ in mols], 3, want, [o for _, o in mols], charges=True, what=f"scan M={M}")


@functools.lru_cache(maxsize=None)
def cloud_expected_batch(ds, limit, flags):
    zs, caps = mc.ds_type_tables(ds)
    return pr.process_batch([(c.types, o) for c, o in zip(mc.clouds(ds), pc.cloud_orders(ds, bool(limit)))], zs, caps, flags)


@pytest.mark.parametrize("stride", (3, 9))
@pytest.mark.parametrize("ds,limit", (("qm9", 0), ("qm9", 1), ("geom", 1), ("geom", 0)))
def test_from_positions_equals_the_definition(ds, limit, stride):
    """The distance rule on jittered lattice clouds of 0 .. 193 atoms (every pair at least 1e-3 pm from every threshold), an atom outside the
    vocabulary among them; x_row_stride 3 and that of a wider view; largest_frag with and without sanitize."""
    clouds = mc.clouds(ds)
    x = np.concatenate([c.x for c in clouds])
    for flags in (2, 3):
        want = cloud_expected_batch(ds, limit, flags)
        run(tables(ds, limit), [c.types for c in clouds], flags, want, None, x=x, stride=stride, charges=stride == 9,
            what=f"from positions {ds} limit={limit} stride={stride} flags={flags}")


def test_launch_on_a_side_stream():
    """Stream-ordered: both entries on a side stream see the buffers the stream filled before them."""
    cases = pc.fragment_cases() + tuple(mc.order_cases()[mc.HARD_FIRST:mc.HARD_FIRST + 4])
    zs, caps = mc.qm9_type_tables()
    want = pr.process_batch([(c.types, c.orders) for c in cases], zs, caps, 2)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run(tables("qm9", 0), [c.types for c in cases], 2, want, [c.orders for c in cases], charges=True, what="side stream")
