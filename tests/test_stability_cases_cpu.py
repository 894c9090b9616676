"""The cases of tests/stability_cases.py mean something before any kernel sees them (no GPU): `direct_rule`'s distances are torch.cdist's direct
path bit for bit, its orders and triples are the oracle's on every molecule of every case, the builders' own conditions hold, and every
mutant of the rule -- one mistake a kernel could make -- changes the expected result of at least one case.  Integers and bits only."""
import numpy as np
import pytest
import torch

import stability_cases as sc
from oracle import stability_oracle as so

LIMITS = (0, 1)


def _rule(family, ds, limit, mutant=None):
    tb = sc.family_tables(family, ds)
    return [sc.direct_rule(x, t, tb.thr, limit, tb.allowed, mutant) for x, t, _ in sc.molecules(getattr(sc, family)(ds))]


@pytest.mark.parametrize("n", [2, 20, 25])
def test_direct_rule_distances_are_cdists_direct_path(n):
    """>= 10^4 ordered pairs per size: 100 * cdist(x, x) on the path the reference takes for n <= 25, against the FMA chain, bit for bit;
    the sequential sum differs on some of them (the two rules are not the same rule)."""
    rng = np.random.default_rng(n)
    pairs, seq_equal = 0, 0
    while pairs < 10_000:
        x = (rng.normal(size=(n, 3)) * 1.5).astype(np.float32)
        want = np.float32(100.0) * torch.cdist(torch.from_numpy(x), torch.from_numpy(x), p=2.0, compute_mode="donot_use_mm_for_euclid_dist").numpy()
        np.testing.assert_array_equal(so.pair_distances(x).view(np.uint32), so.pair_distances(x, direct=True).view(np.uint32))
        got = sc.direct_distances(x)[0]
        off = ~np.eye(n, dtype=bool)
        np.testing.assert_array_equal(got[off].view(np.uint32), want[off].view(np.uint32))
        seq_equal += int((sc.direct_distances(x, "sequential")[0][off].view(np.uint32) == want[off].view(np.uint32)).sum())
        pairs += n * (n - 1)
    print(f"n={n}: {pairs} pairs equal to the FMA chain, {seq_equal} of them also to the sequential sum")
    assert seq_equal < pairs


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("ds", sc.DATASETS)
@pytest.mark.parametrize("family", sc.FAMILIES)
def test_direct_rule_equals_oracle(family, ds, limit):
    batch = getattr(sc, family)(ds)
    for (order, triple), (want_order, want_triple), label in zip(_rule(family, ds, limit), sc.expected(family, ds, limit), batch.labels):
        np.testing.assert_array_equal(order, want_order, err_msg=label)
        assert triple == want_triple, label


@pytest.mark.parametrize("ds", sc.DATASETS)
def test_oracle_limit_flag_and_direct_path(ds):
    """The oracle's orders with the limit are its orders without, capped at 1; on the lattice molecules its default and direct paths agree."""
    tb = sc.tables(ds)
    for (o0, _), (o1, _) in zip(sc.expected("boundary_axis", ds, 0), sc.expected("boundary_axis", ds, 1)):
        np.testing.assert_array_equal(np.minimum(o0, 1), o1)
    for (x, t, label), (order, triple) in zip(sc.molecules(sc.lattice(ds)), sc.expected("lattice", ds, 0)):
        np.testing.assert_array_equal(so.bond_order_matrix(x, t, tb.bonds, tb.margins, direct=True), order, err_msg=label)
        assert so.check_molecular_stability(x, t, tb.decoder, sc.oracle_tables(tb), tb.bonds, direct=True) == (bool(triple[0]), triple[1], triple[2]), label


@pytest.mark.parametrize("ds", sc.DATASETS)
def test_builders_conditions(ds):
    tb = sc.tables(ds)
    # boundary_axis: bond / no bond, alternating, on every ordered pair and threshold
    axis = sc.boundary_axis(ds)
    assert len(axis.sizes) == tb.T * tb.T * 3 * 2 and (axis.sizes == 2).all()
    for (x, t, label), (order, _) in zip(sc.molecules(axis), sc.expected("boundary_axis", ds, 0)):
        k = int(label.split("thr")[1][0])
        below = float(np.float32(100.0) * x[1, 0]) < tb.thr[k - 1][t[0], t[1]]
        assert below == label.endswith("below"), label
        assert order[0, 1] == order[1, 0] == max([j + 1 for j in range(3) if float(np.float32(100.0) * x[1, 0]) < tb.thr[j][t[0], t[1]]], default=0), label
    # boundary_offaxis: for each other sum, at least 8 pairs over at least 4 thresholds on which it and the FMA chain give different orders
    offaxis = sc.boundary_offaxis(ds)
    for rule in sc.SUMS[1:]:
        mine = [(x, t, label) for x, t, label in sc.molecules(offaxis) if label.split(" #")[0].endswith("!= " + rule)]
        assert len(mine) >= 8 and len({label.split("=")[1].split()[0] for _, _, label in mine}) >= 4, rule
        for x, t, label in mine:
            assert sc.direct_rule(x, t, tb.thr, 0)[0][0, 1] != sc.direct_rule(x, t, tb.thr, 0, mutant=rule)[0][0, 1], label
    # lattice: the sizes, the empty molecule in the middle, the gaps
    lat = sc.lattice(ds)
    assert sorted(lat.sizes.tolist()) == sorted(list(sc.LATTICE_SIZES) + [0, 1025]) and 0 not in (lat.sizes[0], lat.sizes[-1])
    for x, t, label in sc.molecules(lat):
        if len(t) > 25:
            assert so.threshold_gap(x, t, tb.bonds, tb.margins) >= 1e-3, label
    dense = sc.expected("lattice", ds, 0)[-1][0]
    assert dense.sum(axis=1).mean() > 8 * sc.expected("lattice", ds, 0)[-2][0].sum(axis=1).mean()
    # collapsed: all orders 3, row sums 0, 3, 30, 33, 117
    for (x, t, label), (order, triple) in zip(sc.molecules(sc.collapsed(ds)), sc.expected("collapsed", ds, 0)):
        n = len(t)
        np.testing.assert_array_equal(order, 3 * (1 - np.eye(n, dtype=np.int64)), err_msg=label)
        assert order.sum(axis=1).tolist() == [{1: 0, 2: 3, 11: 30, 12: 33, 40: 117}[n]] * n
        assert triple == ((1, n, n) if (n == 2 and label.startswith("collapsed N")) else (0, 0, n)), label
    # custom thresholds: fp32 roundings on both sides of the float64 values
    th = np.unique(np.concatenate([t.reshape(-1) for t in sc.tables(ds, custom=True).thr]))
    th32 = th.astype(np.float32).astype(np.float64)
    assert (th32 < th).sum() >= 2 and (th32 > th).sum() >= 2 and (th != np.round(th)).sum() >= 4
    assert sum(lab.endswith("at fl32(thr)") for lab in sc.custom_thresholds(ds).labels) >= 2
    # over all cases: both outcomes, all four orders, a row sum >= 32
    stable, orders, rowmax = set(), set(), 0
    for family in sc.FAMILIES:
        for order, triple in sc.expected(family, ds, 0):
            stable.add(triple[0])
            orders |= set(np.unique(order).tolist())
            rowmax = max(rowmax, int(order.sum(axis=1).max(initial=0)))
    assert stable == {0, 1} and orders == {0, 1, 2, 3} and rowmax >= 32
    # bad types: one to two atoms outside [0, T) per molecule, every value of the list present
    bad = sc.bad_types(ds)
    seen = {int(v) for v in bad.types if not 0 <= v < tb.T}
    assert seen == {-1, tb.T, 16, 255}
    for order, triple in sc.bad_types_expected(ds, 0):
        assert triple[0] == 0 and triple[1] < triple[2] and (order == order.T).all()


@pytest.mark.parametrize("custom", [False, True])
@pytest.mark.parametrize("ds", sc.DATASETS)
def test_host_tables_round_thresholds_up(ds, custom):
    """The packed fp32 threshold is the smallest fp32 >= the float64 `length + margin`: an fp32 distance is below the one exactly when it is
    below the other.  Integer tables are stored as they are."""
    tb = sc.tables(ds, custom)
    packed = sc.pkg.stability.bond_tables(dict(tb.info))
    for name, thr in zip(("thr1", "thr2", "thr3"), tb.thr):
        got = np.asarray(list(getattr(packed, name)), np.float32).reshape(16, 16)[:tb.T, :tb.T]
        assert (got.astype(np.float64) >= thr).all() and (np.nextafter(got, np.float32(-np.inf)).astype(np.float64) < thr).all()
        if not custom:
            np.testing.assert_array_equal(got.astype(np.float64), thr)


@pytest.mark.parametrize("mutant", sc.MUTANTS)
@pytest.mark.parametrize("ds", sc.DATASETS)
def test_every_mutant_is_caught(mutant, ds):
    """A mutant that no case catches means a case is missing."""
    caught = []
    for family in sc.FAMILIES:
        for limit in LIMITS:
            want = sc.expected(family, ds, limit)
            got = _rule(family, ds, limit, mutant)
            bad = sum(1 for (o, tr), (wo, wtr) in zip(got, want) if tr != wtr or not np.array_equal(o, wo))
            if bad:
                caught.append((family, limit, bad))
    print(f"{ds} {mutant}: caught by {caught}")
    assert caught, f"no case tells the mutant '{mutant}' from the rule"
