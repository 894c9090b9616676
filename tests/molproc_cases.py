"""What tests/test_molproc_cpu.py, tests/test_molproc_cabi_gpu.py and tests/test_molproc_gpu.py share: the molecules that sit where the
select / scan / emit kernels can go wrong, on top of those of tests/molgraph_cases.py.  Builders return read-only arrays (OrderCase: types in
QM9's vocabulary, the full n x n uint8 orders); every expected value comes from tests/molproc_ref.py.  No GPU code here."""
import functools

import numpy as np

import molgraph_cases as mc
import molgraph_ref as ref
import molproc_ref as pr
import stability_cases as sc

SCAN_TILE = 256                                                      # GCDM_MOLPROC_SCAN_TILE (tests/test_molproc_cpu.py holds it to the header)
SCAN_SIZES = (1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 3)


@functools.lru_cache(maxsize=None)
def fragment_cases():
    """The largest fragment not holding atom 0; fragments interleaved in index, so the renumbering is no shift; all atoms singletons; an atom
    outside the vocabulary outside the largest fragment, and one that IS the largest fragment (it bonds to nothing: the first of singletons)."""
    out = [mc._case(mc.from_bonds([1, 6, 6, 6], [(2, 1, 1), (3, 2, 1)], "largest fragment behind a lone atom 0"))]
    ring = [(3, 1, 1), (5, 3, 1), (7, 5, 1), (9, 7, 1), (11, 9, 1), (11, 1, 1)]
    chain = [(2, 0, 1), (4, 2, 1), (6, 4, 2), (8, 6, 1)]
    out.append(mc._case(mc.from_bonds([6] * 12, ring + chain, "interleaved: ring on the odd atoms, chain on the even")))
    out.append(mc._case(mc.from_bonds([6, 1, 8, 7], [], "all singletons")))
    g = mc.cap_cases()[0]
    t = mc._types(g.Z)
    t[2] = 99
    out.append(mc._case(g._replace(label="CH4 with type 99 at atom 2: outside the largest fragment"), types=t))
    g = mc.from_bonds([6, 1, 1], [], "singletons, atom 0 outside the vocabulary: it is the largest fragment")
    t = mc._types(g.Z)
    t[0] = -1
    out.append(mc._case(g, types=t))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mixed_batch(oversize=True):
    """Every molecule of the from-orders batch of tests/molgraph_cases.py (0 .. 193 atoms, the hard pairs, caps, ties, types outside the
    vocabulary, asymmetric matrices) and the fragment cases.  `oversize=False` leaves the 193-atom molecule out (Python refuses it)."""
    cases = mc.order_cases() + fragment_cases()
    return tuple(c for c in cases if oversize or len(c.types) <= pr.MAX_ATOMS)


@functools.lru_cache(maxsize=None)
def _scan_templates():
    g = [mc.from_bonds([], [], "empty"), mc.from_bonds([6], [], "C"), mc.from_bonds([6, 8], [(1, 0, 2)], "C=O"),
         mc.from_bonds([8, 1, 1, 1], [(1, 0, 1), (2, 0, 1), (3, 0, 1)], "OH3: dropped by sanitize"),
         mc.from_bonds([1, 6, 6], [(2, 1, 3)], "H + C#C"), mc.from_bonds([6, 6, 6, 6], [(1, 0, 1), (2, 1, 1), (3, 2, 1)], "C4")]
    return tuple(mc._case(x) for x in g)


@functools.lru_cache(maxsize=None)
def scan_batch(M):
    """M molecules of 0 - 4 atoms, one in six dropped by sanitize, one in six empty: (types, orders) per molecule."""
    tp = _scan_templates()
    return tuple((tp[(m + 2) % len(tp)].types, tp[(m + 2) % len(tp)].orders) for m in range(M))


@functools.lru_cache(maxsize=None)
def cloud_orders(ds, limit):
    """The oracle's bond orders of the clouds of tests/molgraph_cases.py: the molecules of the entry that starts from positions."""
    tb = sc.tables(ds)
    zs, _ = mc.ds_type_tables(ds)
    out = []
    for c in mc.clouds(ds):
        n = len(c.types)
        out.append(np.zeros((n, n), np.int64) if n > pr.MAX_ATOMS else ref.oracle_orders(c.x, c.types, zs, tb.bonds, tb.margins, limit))
    return tuple(out)
