"""The graph kernel on an MI355X through its C ABI (gcdm_molgraph_keys, gcdm_molgraph_keys_from_orders; include/gcdm_molgraph.h) on the
molecules of tests/molgraph_cases.py: 0 .. 193 atoms, an empty molecule between two others, the pairs plain colour refinement cannot
separate, atoms at and over their caps inside and outside the largest fragment, ties between fragments, types outside the vocabulary, an
asymmetric order matrix, and jittered lattice clouds classified from positions.  Expected values are the definition's
(tests/molgraph_ref.py, from the oracle's bond orders), compared as integers with array_equal on keys AND info; nothing is excluded.
Outputs are pre-filled (0x7F bytes) inside guard words: an element the kernel leaves unwritten, or one it writes outside, fails.
Under 300 molecules in all."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import molgraph_cases as mc
import stability_cases as sc

pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8                                   # guard words on either side of keys, guard rows on either side of info
FILL64, FILL32 = 0x7F7F7F7F7F7F7F7F, 0x7F7F7F7F


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Outputs:
    def __init__(self, M):
        self.M = M
        self.keys_buf = torch.full((M + 2 * GUARD,), FILL64, dtype=torch.int64, device=DEV)
        self.info_buf = torch.full((M + 2 * GUARD, 4), FILL32, dtype=torch.int32, device=DEV)
        self.keys, self.info = self.keys_buf[GUARD:], self.info_buf[GUARD:]                # views that start where the kernel's block starts

    def results(self, what):
        torch.cuda.synchronize()
        keys, info = self.keys_buf.cpu().numpy(), self.info_buf.cpu().numpy()
        for buf, fill in ((keys, FILL64), (info, FILL32)):
            assert (buf[:GUARD] == fill).all() and (buf[GUARD + self.M:] == fill).all(), (what, "guard words")
        keys, info = keys[GUARD:GUARD + self.M], info[GUARD:GUARD + self.M]
        assert (info != FILL32).all() and (keys != FILL64).all(), (what, "an output element was not written")
        return keys, info


def _dev(a, dtype):
    a = np.ascontiguousarray(np.asarray(a, dtype))
    return torch.from_numpy(a.copy()).to(DEV) if a.size else torch.zeros(1, dtype=getattr(torch, np.dtype(dtype).name), device=DEV)


def tables(ds, limit, atomic_numbers=False, caps=None):
    return pkg.metrics.graph_tables(dict(sc.tables(ds).info), caps, limit_bonds_to_one=bool(limit), types_are_atomic_numbers=atomic_numbers)


def launch_orders(tb, types_list, orders_list, what=""):
    sizes = np.array([len(t) for t in types_list], np.int64)
    types = _dev(np.concatenate(types_list) if len(types_list) else [], np.int32)
    off = _dev(np.r_[0, np.cumsum(sizes)], np.int64)
    poff = _dev(np.r_[0, np.cumsum(sizes * sizes)][:-1], np.int64)
    orders = _dev(np.concatenate([np.asarray(o, np.uint8).reshape(-1) for o in orders_list]), np.uint8)
    out = Outputs(len(sizes))
    st = native.load_ops().gcdm_molgraph_keys_from_orders(tb, _p(types), _p(off), len(sizes), _p(poff), _p(orders), _p(out.keys), _p(out.info), _stream())
    assert st == 0, what
    return out.results(what)


def launch_positions(tb, x, types, sizes, stride=3, what=""):
    sizes = np.asarray(sizes, np.int64)
    N = len(types)
    xd = torch.full((max(N, 1), stride), 1.0e30, dtype=torch.float32, device=DEV)          # what lies between the rows is not a coordinate
    xd[:N, :3] = torch.from_numpy(np.array(x, np.float32).reshape(-1, 3)).to(DEV)
    td, off = _dev(types, np.int32), _dev(np.r_[0, np.cumsum(sizes)], np.int64)
    out = Outputs(len(sizes))
    st = native.load_ops().gcdm_molgraph_keys(tb, _p(xd), stride, _p(td), _p(off), len(sizes), _p(out.keys), _p(out.info), _stream())
    assert st == 0, what
    return out.results(what), (xd, td)


def assert_equal(keys, info, want, labels, what):
    wrong = [lab for k, i, (wk, wi), lab in zip(keys, info, want, labels) if int(k) != wk or tuple(i.tolist()) != wi]
    print(f"{what}: {len(wrong)} of {len(want)} molecules differ from the definition {wrong[:5]}")
    assert np.array_equal(info, np.array([w[1] for w in want], np.int32).reshape(-1, 4)), (what, wrong)
    assert np.array_equal(keys, np.array([w[0] for w in want], np.int64)), (what, wrong)


@pytest.mark.parametrize("atomic_numbers", (False, True))
def test_from_orders_equals_the_definition(atomic_numbers):
    """Every molecule of the from-orders batch, the types as vocabulary indices and as atomic numbers (one Z absent from the table)."""
    cases = mc.order_cases()
    types = [mc.as_atomic_numbers(c.types) if atomic_numbers else c.types for c in cases]
    keys, info = launch_orders(tables("qm9", 0, atomic_numbers), types, [c.orders for c in cases], what=("orders", atomic_numbers))
    want = mc.order_expected(atomic_numbers)
    assert_equal(keys, info, want, [c.label for c in cases], f"from orders, atomic_numbers={atomic_numbers}")
    by = {c.label: (int(k), tuple(i.tolist())) for c, k, i in zip(cases, keys, info)}
    # the hard pairs: a permuted copy has the key of its original, the two of a pair differ
    h = mc.HARD_FIRST
    for p in range(3):
        a, b, pa, pb = (int(keys[h + 4 * p + q]) for q in range(4))
        assert a == pa and b == pb and a != b, cases[h + 4 * p].label
    assert by["decalin, upper triangle scrambled"] == by["decalin"] == by["decalin below, bicyclopentyl above the diagonal"]
    assert by["CH4: C at its cap"][1] == (1, 1, 5, 5) and by["CH5: C over its cap, in the largest fragment"][1] == (0, 1, 6, 6)
    assert by["C5 + OH3: O over its cap, outside the largest fragment"][1] == (0, 2, 5, 9)
    assert by["C5 + OH2: O at its cap, outside the largest fragment"][1] == (1, 2, 5, 8)
    assert by["C5 + OH3: O over its cap, outside the largest fragment"][0] == by["C5 + OH2: O at its cap, outside the largest fragment"][0]
    assert by["tie: C-O then C-N"][0] != by["tie: C-N then C-O"][0] == by["tie, interleaved: C-N holds atom 0"][0]
    assert by["CH4 with type 99 at atom 2"][1] == (0, 2, 4, 5)
    assert by["n=0"] == (0, (1, 0, 0, 0)) and by["random n=193"] == (0, (-1, 0, 0, 193))
    assert by["chain n=192"][1] == (1, 1, 192, 192)


def test_from_orders_single_molecules_and_caps_override():
    """A batch of one at either end of the size range, and caps that arrive through the table: -1 lifts a cap, a lower cap invalidates."""
    cases = {c.label: c for c in mc.order_cases()}
    want = dict(zip((c.label for c in mc.order_cases()), mc.order_expected()))
    for label in ("n=0", "random n=192", "random n=193", "CH5: C over its cap, in the largest fragment"):
        c = cases[label]
        keys, info = launch_orders(tables("qm9", 0), [c.types], [c.orders], what=label)
        assert_equal(keys, info, [want[label]], [label], f"single molecule {label}")
    c = cases["CH5: C over its cap, in the largest fragment"]
    for caps, valid in (({"C": 5}, 1), ({"C": -1}, 1), ({"C": 4, "H": 0}, 0)):
        keys, info = launch_orders(tables("qm9", 0, caps=caps), [c.types], [c.orders], what=caps)
        assert int(keys[0]) == want[c.label][0] and tuple(info[0].tolist()) == (valid, 1, 6, 6), caps


@pytest.mark.parametrize("stride", (3, 9))
@pytest.mark.parametrize("ds,limit", (("qm9", 0), ("qm9", 1), ("geom", 1), ("geom", 0)))
def test_from_positions_equals_the_definition(ds, limit, stride):
    """Jittered lattice clouds of 0 .. 193 atoms, every pair at least 1e-3 pm from every threshold; x_row_stride 3 and 3 + 6.  The same input
    through gcdm_bond_orders and the from-orders entry must give the same keys and info, and the order sums of that launch the same verdict."""
    clouds = mc.clouds(ds)
    sizes = np.array([len(c.types) for c in clouds], np.int64)
    x, types = np.concatenate([c.x for c in clouds]), np.concatenate([c.types for c in clouds])
    tb = tables(ds, limit)
    (keys, info), (xd, td) = launch_positions(tb, x, types, sizes, stride, what=(ds, limit, stride))
    assert_equal(keys, info, mc.cloud_expected(ds, bool(limit)), [c.label for c in clouds], f"from positions {ds} limit={limit} stride={stride}")
    if stride != 3:
        return
    off32 = _dev(np.r_[0, np.cumsum(sizes)], np.int32)
    poff_host = np.r_[0, np.cumsum(sizes * sizes)].astype(np.int64)
    poff = _dev(poff_host[:-1], np.int64)
    orders = torch.full((int(poff_host[-1]),), 0xEE, dtype=torch.uint8, device=DEV)
    st = native.load().gcdm_bond_orders(tb.bonds, _p(xd), stride, _p(td), _p(off32), len(sizes), _p(poff), _p(orders), _stream())
    assert st == 0
    torch.cuda.synchronize()
    oh = orders.cpu().numpy()
    blocks = [oh[a:b].reshape(n, n) for a, b, n in zip(poff_host[:-1], poff_host[1:], sizes)]
    zs, caps = mc.ds_type_tables(ds)
    for m, (c, o) in enumerate(zip(clouds, blocks)):
        if len(c.types) > native.MOLGRAPH_MAX_ATOMS:
            continue
        inside = (c.types >= 0) & (c.types < len(zs))
        over = [int(o[i].sum()) > caps[int(c.types[i])] for i in range(len(c.types)) if inside[i]]
        assert int(info[m, 0]) == int(inside.all() and not any(over)), c.label
    keys2, info2 = launch_orders(tb, [c.types for c in clouds], blocks, what="orders of gcdm_bond_orders")
    assert np.array_equal(keys2, keys) and np.array_equal(info2, info)


def test_launch_on_a_side_stream():
    """Stream-ordered: the launch on a side stream sees the buffers the stream filled before it."""
    cases = mc.order_cases()[mc.HARD_FIRST:mc.HARD_FIRST + 4]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        keys, info = launch_orders(tables("qm9", 0), [c.types for c in cases], [c.orders for c in cases], what="side stream")
    assert_equal(keys, info, mc.order_expected()[mc.HARD_FIRST:mc.HARD_FIRST + 4], [c.label for c in cases], "side stream")
