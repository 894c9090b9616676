"""The stability and bond-order kernel on an MI355X through its C ABI (gcdm_check_stability, gcdm_bond_orders; include/gcdm_hip.h) on the
cases of tests/stability_cases.py: pairs one ulp either side of every threshold, on the axis and in general position, molecules of 0 .. 1025
atoms, collapsed and non-finite samples, caller-supplied non-integer thresholds, atom types outside the vocabulary.  Expected values are the
oracle's (torch.cdist on the CPU), compared as integers with array_equal; nothing is excluded.  Outputs are pre-filled (-7, 0xEE) inside
guard bands: an element the kernel leaves unwritten, or one it writes outside its block, fails."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import stability_cases as sc

pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096                    # bytes of 0xEE on either side of the orders block
OUT_FILL, ORD_FILL = -7, 0xEE
LIMITS = (0, 1)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Buffers:
    """Device arguments of one batch with pre-filled outputs: `out` [B, 3] between two guard rows, `orders` between two guard bands."""

    def __init__(self, x, types, sizes, stride=3):
        sizes = np.asarray(sizes, np.int64)
        N, self.B = len(types), len(sizes)
        xd = torch.full((max(N, 1), stride), 1.0e30, dtype=torch.float32, device=DEV)      # what lies between the rows is not a coordinate
        xd[:N, :3] = torch.from_numpy(np.array(x, np.float32).reshape(-1, 3)).to(DEV)
        self.x, self.stride = xd, stride
        self.types = torch.from_numpy(np.array(types, np.int32)).to(DEV) if N else torch.zeros(1, dtype=torch.int32, device=DEV)
        self.off = torch.from_numpy(np.r_[0, np.cumsum(sizes)].astype(np.int32)).to(DEV)
        self.poff_host = np.r_[0, np.cumsum(sizes * sizes)].astype(np.int64)
        self.poff = torch.from_numpy(self.poff_host[:-1].copy()).to(DEV) if self.B else torch.zeros(1, dtype=torch.int64, device=DEV)
        self.sizes = sizes
        self.out_buf = torch.full((self.B + 2, 3), OUT_FILL, dtype=torch.int32, device=DEV)
        self.ord_buf = torch.full((int(self.poff_host[-1]) + 2 * GUARD,), ORD_FILL, dtype=torch.uint8, device=DEV)
        self.out, self.orders = self.out_buf[1:], self.ord_buf[GUARD:]                     # views that start where the kernel's block starts

    def untouched(self):
        return bool((self.out_buf == OUT_FILL).all()) and bool((self.ord_buf == ORD_FILL).all())

    def results(self, what):
        """(out [B, 3], [orders n x n per molecule]) after checking the guards and that every element in range was written."""
        torch.cuda.synchronize()
        out, orders = self.out_buf.cpu().numpy(), self.ord_buf.cpu().numpy()
        assert (out[0] == OUT_FILL).all() and (out[-1] == OUT_FILL).all(), (what, "out guard rows")
        assert (orders[:GUARD] == ORD_FILL).all() and (orders[len(orders) - GUARD:] == ORD_FILL).all(), (what, "orders guard bands")
        out, orders = out[1:-1], orders[GUARD:len(orders) - GUARD]
        assert (out != OUT_FILL).all(), (what, "an element of out was not written")
        assert (orders <= 3).all(), (what, "an element of orders was not written")
        return out, [orders[a:b].reshape(n, n) for a, b, n in zip(self.poff_host[:-1], self.poff_host[1:], self.sizes)]


def launch(tb, limit, x, types, sizes, stride=3, stream=None, what=""):
    """Both entry points on one pre-filled set of buffers -> (out, orders per molecule)."""
    lib = native.load()
    tables = pkg.stability.bond_tables(dict(tb.info), bool(limit))
    buf = Buffers(x, types, sizes, stride)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream)
    torch.cuda.synchronize()
    assert lib.gcdm_check_stability(tables, _p(buf.x), stride, _p(buf.types), _p(buf.off), buf.B, _p(buf.out), s) == 0, what
    assert lib.gcdm_bond_orders(tables, _p(buf.x), stride, _p(buf.types), _p(buf.off), buf.B, _p(buf.poff), _p(buf.orders), s) == 0, what
    if stream is not None:
        stream.synchronize()
    return buf.results(what)


def assert_family(family, ds, limit, **kw):
    batch = getattr(sc, family)(ds)
    out, orders = launch(sc.family_tables(family, ds), limit, batch.x, batch.types, batch.sizes, what=(family, ds, limit), **kw)
    want = sc.expected(family, ds, limit)
    assert len(want) == len(batch.labels) == len(out) == len(orders)
    wrong = [label for m, ((want_order, want_triple), label) in enumerate(zip(want, batch.labels))
             if not np.array_equal(orders[m], want_order) or tuple(out[m].tolist()) != want_triple]
    print(f"{family} {ds} limit={limit}: {len(wrong)} of {len(want)} molecules differ from the oracle")
    for m, ((want_order, want_triple), label) in enumerate(zip(want, batch.labels)):
        msg = f"{family} {ds} limit={limit}: {label} ({len(wrong)} of {len(want)} molecules differ)"
        np.testing.assert_array_equal(orders[m], want_order, err_msg=msg)
        assert (orders[m] == orders[m].T).all() and (np.diag(orders[m]) == 0).all(), msg
        assert tuple(out[m].tolist()) == want_triple, msg
    return out, orders


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("ds", sc.DATASETS)
def test_boundary_axis(ds, limit):
    """Needs the correctly rounded square root: with v_sqrt_f32 (1 ulp) 1 of 150 (qm9) and 5 of 1536 (geom) molecules came out wrong."""
    assert_family("boundary_axis", ds, limit)


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("ds", sc.DATASETS)
def test_boundary_offaxis(ds, limit):
    """Pairs on which fma(dz, dz, fma(dy, dy, dx*dx)), the reference's sum, and another way to add the three squares (sequential, as a compiler
    contracted it, the chain reversed) give different bond orders."""
    assert_family("boundary_offaxis", ds, limit)


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("ds", sc.DATASETS)
def test_lattice(ds, limit):
    """n = 0 .. 1025: one and two atoms per lane, positions in LDS (n <= 1024) and read from global memory (n = 1025)."""
    assert_family("lattice", ds, limit)


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("ds", sc.DATASETS)
def test_collapsed(ds, limit):
    assert_family("collapsed", ds, limit)


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("ds", sc.DATASETS)
def test_nonfinite(ds, limit):
    assert_family("nonfinite", ds, limit)


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("ds", sc.DATASETS)
def test_custom_thresholds(ds, limit):
    assert_family("custom_thresholds", ds, limit)


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("ds", sc.DATASETS)
def test_bad_types(ds, limit):
    """An atom whose type is outside [0, T) bonds to nothing, nothing bonds to it, it counts as unstable, and every valid atom fares as in the
    molecule without it (the oracle on that molecule)."""
    assert_family("bad_types", ds, limit)


@pytest.mark.parametrize("ds", sc.DATASETS)
def test_strides_streams_repeats_and_position(ds):
    tb = sc.tables(ds)
    parts = [sc.lattice(ds), sc.boundary_offaxis(ds), sc.collapsed(ds)]
    x, types, sizes = np.concatenate([p.x for p in parts]), np.concatenate([p.types for p in parts]), np.concatenate([p.sizes for p in parts])
    base_out, base_orders = launch(tb, 0, x, types, sizes, what="base")
    runs = {"strided [N, 9] view": dict(stride=9), "non-default stream": dict(stream=torch.cuda.Stream()), "second run": {}}
    for what, kw in runs.items():
        out, orders = launch(tb, 0, x, types, sizes, what=what, **kw)
        np.testing.assert_array_equal(out, base_out, err_msg=what)
        for a, b in zip(orders, base_orders):
            np.testing.assert_array_equal(a, b, err_msg=what)
    off = np.r_[0, np.cumsum(sizes)]
    for m in (int(np.flatnonzero(sizes == 65)[0]), int(np.flatnonzero(sizes == 1025)[0]), len(sizes) - 3):      # alone == inside the batch
        out, orders = launch(tb, 0, x[off[m]:off[m + 1]], types[off[m]:off[m + 1]], sizes[m:m + 1], what=f"molecule {m} alone")
        np.testing.assert_array_equal(out[0], base_out[m], err_msg=f"molecule {m} alone")
        np.testing.assert_array_equal(orders[0], base_orders[m], err_msg=f"molecule {m} alone")


@pytest.mark.parametrize("ds", sc.DATASETS)
def test_wrappers_agree_with_the_direct_calls(ds):
    tb, batch = sc.tables(ds), sc.lattice(ds)
    x, t, sizes = torch.from_numpy(batch.x.copy()).to(DEV), torch.from_numpy(batch.types.copy()).to(DEV), torch.from_numpy(batch.sizes.copy())
    for limit in LIMITS:
        out, _ = launch(tb, limit, batch.x, batch.types, batch.sizes, what="direct")
        got = pkg.check_molecular_stability_batch(x, t, sizes, dict(tb.info), limit_bonds_to_one=bool(limit))
        assert got.dtype == torch.int32
        np.testing.assert_array_equal(got.cpu().numpy(), out)
    _, orders = launch(tb, int(ds == "geom"), batch.x, batch.types, batch.sizes, what="direct")     # make_mol_edm limits GEOM's bonds to single ones
    got = pkg.bond_order_matrices(x, t, sizes, dict(tb.info))
    assert len(got) == len(orders)
    for a, b, label in zip(got, orders, batch.labels):
        assert a.dtype == np.uint8 and a.shape == b.shape, label
        np.testing.assert_array_equal(a, b, err_msg=label)


def test_bad_arguments_leave_the_outputs_alone():
    lib = native.load()
    tb, batch = sc.tables("qm9"), sc.collapsed("qm9")
    buf = Buffers(batch.x, batch.types, batch.sizes)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def tables(num_types=None):
        t = pkg.stability.bond_tables(dict(tb.info))
        if num_types is not None:
            t.num_types = num_types
        return t

    def check(**kw):
        a = dict(tables=tables(), x=_p(buf.x), stride=3, types=_p(buf.types), off=_p(buf.off), B=buf.B, out=_p(buf.out))
        a.update(kw)
        return lib.gcdm_check_stability(a["tables"], a["x"], a["stride"], a["types"], a["off"], a["B"], a["out"], s)

    def orders(**kw):
        a = dict(tables=tables(), x=_p(buf.x), stride=3, types=_p(buf.types), off=_p(buf.off), B=buf.B, poff=_p(buf.poff), orders=_p(buf.orders))
        a.update(kw)
        return lib.gcdm_bond_orders(a["tables"], a["x"], a["stride"], a["types"], a["off"], a["B"], a["poff"], a["orders"], s)

    bad = [dict(tables=None), dict(x=None), dict(types=None), dict(off=None), dict(stride=2), dict(tables=tables(0)), dict(tables=tables(17)), dict(B=-1)]
    for kw in bad + [dict(out=None)]:
        assert check(**kw) == -1, ("gcdm_check_stability", list(kw))
    for kw in bad + [dict(poff=None), dict(orders=None)]:
        assert orders(**kw) == -1, ("gcdm_bond_orders", list(kw))
    assert check(B=0) == 0 and orders(B=0) == 0
    torch.cuda.synchronize()
    assert buf.untouched()
    assert check() == 0 and orders() == 0                           # the same buffers with good arguments: the calls above were refused, not broken
    out, _ = buf.results("good arguments")
    assert [tuple(r) for r in out.tolist()] == [tr for _, tr in sc.expected("collapsed", "qm9", 0)]
