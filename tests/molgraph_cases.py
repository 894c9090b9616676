"""What tests/test_molgraph_cpu.py, tests/test_molgraph_cabi_gpu.py and tests/test_molgraph_gpu.py share: the seeded corpus of molecule-like
labelled graphs the key is held to networkx on, the hand-made molecules that sit where the graph kernel can go wrong, and the jittered
lattice clouds for the entry that starts from positions.  A graph is (Z [n] atomic numbers, orders [n, n] int64); builders return read-only
arrays, exclude nothing, and every expected value comes from tests/molgraph_ref.py.  No GPU code here."""
import functools
from collections import namedtuple

import numpy as np

import molgraph_ref as ref
import stability_cases as sc
from oracle import stability_oracle as so

ELEMENTS = (1, 6, 7, 8, 9)                            # QM9's vocabulary, in the order of its atom_decoder
CAPS = {1: 1, 6: 4, 7: 3, 8: 2, 9: 1}
GPU_SIZES = (0, 1, 2, 63, 64, 65, 128, 191, 192, 193)
Graph = namedtuple("Graph", "Z orders label")
# from-orders batch: `types` in the vocabulary of `ds` (indices; -1 / 99 outside it), orders per molecule as the full n x n uint8 block
OrderCase = namedtuple("OrderCase", "types orders label")
Cloud = namedtuple("Cloud", "x types label")


def _freeze(Z, o, label):
    Z, o = np.asarray(Z, np.int64), np.asarray(o, np.int64)
    Z.setflags(write=False)
    o.setflags(write=False)
    return Graph(Z, o, label)


def from_bonds(Z, bonds, label):
    n = len(Z)
    o = np.zeros((n, n), np.int64)
    for i, j, k in bonds:
        assert i != j and o[i, j] == 0
        o[i, j] = o[j, i] = k
    return _freeze(Z, o, label)


def permuted(g, rng, label=None):
    p = rng.permutation(len(g.Z))
    return _freeze(g.Z[p], g.orders[np.ix_(p, p)], label or g.label + " permuted")


def random_fragment(rng, n, strict=True):
    """A valence-capped random tree on n atoms with ring closures: (Z, bonds).  Atoms attach to a random atom that has valence left, with a
    bond order both ends can afford; closures join two non-adjacent atoms with valence left.  `strict=False` lets one closure overrun a cap."""
    Z = [int(rng.choice((6, 6, 6, 7, 8)))]
    free = [CAPS[Z[0]]]
    bonds, bonded = [], set()
    while len(Z) < n:
        open_ = [i for i, f in enumerate(free) if f > 0]
        if not open_:
            break
        p = int(rng.choice(open_))
        z = int(rng.choice((1, 1, 6, 6, 6, 7, 8, 9)))
        k = int(min(free[p], CAPS[z], rng.choice((1, 1, 1, 2, 3))))
        Z.append(z)
        free[p] -= k
        free.append(CAPS[z] - k)
        bonds.append((len(Z) - 1, p, k))
        bonded.add((len(Z) - 1, p))
    for _ in range(int(rng.integers(0, 3))):
        open_ = [i for i, f in enumerate(free) if f > 0]
        if len(open_) < 2:
            break
        i, j = sorted(int(v) for v in rng.choice(open_, 2, replace=False))
        if (j, i) in bonded:
            continue
        k = int(min(free[i], free[j], rng.choice((1, 1, 2)))) + (0 if strict else 1)
        free[i] -= k
        free[j] -= k
        bonds.append((j, i, k))
        bonded.add((j, i))
    return Z, bonds


def random_graph(rng, n, label, strict=True):
    """n atoms: a main fragment and, one time in three, detached ones."""
    parts = [n]
    if n >= 3 and rng.integers(3) == 0:
        cut = int(rng.integers(1, max(2, n // 2)))
        parts = [n - cut, cut] if cut < 3 or rng.integers(2) else [n - cut, cut - 1, 1]
    Z, bonds = [], []
    for size in parts:
        base = len(Z)
        z, b = random_fragment(rng, size, strict)
        while len(z) < size:                                        # the tree ran out of valence: the rest are lone atoms
            z.append(1)
        Z += z
        bonds += [(i + base, j + base, k) for i, j, k in b]
    g = from_bonds(Z, bonds, label)
    return permuted(g, rng, label)                                   # fragments are not laid out in order


def rewired(g, rng, label):
    """The same atoms with one leaf moved to another atom of the graph: equal composition, usually another graph."""
    o = g.orders.copy()
    deg = (o > 0).sum(1)
    leaves = [i for i in range(len(g.Z)) if deg[i] == 1]
    if not leaves:
        return None
    leaf = int(rng.choice(leaves))
    old = int(np.flatnonzero(o[leaf])[0])
    k = int(o[leaf, old])
    others = [i for i in range(len(g.Z)) if i not in (leaf, old) and deg[i] > 0]
    if not others:
        return None
    new = int(rng.choice(others))
    o[leaf, old] = o[old, leaf] = 0
    o[leaf, new] = o[new, leaf] = k
    return _freeze(g.Z, o, label)


# ---- the hard pairs -------------------------------------------------------------------------------------------------------------------------

def decalin():
    return from_bonds([6] * 10, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 5, 1), (5, 0, 1), (4, 6, 1), (6, 7, 1), (7, 8, 1), (8, 9, 1), (9, 5, 1)],
                      "decalin")


def bicyclopentyl():
    return from_bonds([6] * 10, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (4, 0, 1), (5, 6, 1), (6, 7, 1), (7, 8, 1), (8, 9, 1), (9, 5, 1), (4, 5, 1)],
                      "bicyclopentyl")


def order_pair():
    """Two chains that differ only in one bond order: C-C=C-O and C-C-C-O."""
    return (from_bonds([6, 6, 6, 8], [(0, 1, 1), (1, 2, 2), (2, 3, 1)], "C-C=C-O"), from_bonds([6, 6, 6, 8], [(0, 1, 1), (1, 2, 1), (2, 3, 1)], "C-C-C-O"))


def element_pair():
    """Two rings that differ only in one element."""
    ring = [(i, (i + 1) % 6, 1) for i in range(6)]
    return from_bonds([6, 6, 6, 6, 6, 7], ring, "ring C5N"), from_bonds([6, 6, 6, 6, 6, 8], ring, "ring C5O")


def hard_pairs():
    return ((decalin(), bicyclopentyl()), order_pair(), element_pair())


@functools.lru_cache(maxsize=None)
def corpus(seed=2024):
    """>= 500 graphs of 1 .. 29 atoms: random molecule-like graphs (one in ten overruns a cap), rewired twins of equal composition, 200
    permuted copies, the hard pairs."""
    rng = np.random.default_rng(seed)
    graphs = []
    for k in range(260):
        n = 1 + k % 29
        graphs.append(random_graph(rng, n, f"random #{k} n={n}", strict=k % 10 != 0))
    base = len(graphs)
    for k in range(base):
        if len(graphs) >= base + 90:
            break
        g = rewired(graphs[k * 3 % base], rng, f"rewired {graphs[k * 3 % base].label}")
        if g is not None:
            graphs.append(g)
    for a, b in hard_pairs():
        graphs += [a, b]
    for k in range(200):
        graphs.append(permuted(graphs[(k * 7) % (base + 96)], rng))
    assert len(graphs) >= 500 and all(1 <= len(g.Z) <= 29 for g in graphs)
    return tuple(graphs)


def caps_of(Z):
    return [CAPS.get(int(z), -1) for z in Z]


# ---- molecules for the from-orders entry -------------------------------------------------------------------------------------------------

def _types(Z):
    return np.array([ELEMENTS.index(int(z)) for z in Z], np.int32)


def _case(g, types=None, orders=None):
    t = _types(g.Z) if types is None else np.asarray(types, np.int32)
    o = (g.orders if orders is None else np.asarray(orders)).astype(np.uint8)
    t.setflags(write=False)
    o.setflags(write=False)
    return OrderCase(t, o, g.label)


def cap_cases():
    """An atom exactly at its cap and one over it, in the largest fragment and outside it."""
    ch4 = from_bonds([6, 1, 1, 1, 1], [(0, k, 1) for k in range(1, 5)], "CH4: C at its cap")
    ch5 = from_bonds([6, 1, 1, 1, 1, 1], [(0, k, 1) for k in range(1, 6)], "CH5: C over its cap, in the largest fragment")
    chain = [(k, k + 1, 1) for k in range(4)]
    small_over = from_bonds([6] * 5 + [8, 1, 1, 1], chain + [(5, 6, 1), (5, 7, 1), (5, 8, 1)], "C5 + OH3: O over its cap, outside the largest fragment")
    small_at = from_bonds([6] * 5 + [8, 1, 1], chain + [(5, 6, 1), (5, 7, 1)], "C5 + OH2: O at its cap, outside the largest fragment")
    double = from_bonds([6, 8, 8, 8], [(0, 1, 2), (0, 2, 2), (0, 3, 1)], "CO3 with two double bonds: C one over")
    return [ch4, ch5, small_over, small_at, double]


def tie_cases():
    """Two fragments of equal size in both index orders: the one holding the lowest atom index is the largest."""
    return [from_bonds([6, 8, 6, 7], [(0, 1, 1), (2, 3, 1)], "tie: C-O then C-N"), from_bonds([6, 7, 6, 8], [(0, 1, 1), (2, 3, 1)], "tie: C-N then C-O"),
            from_bonds([6, 6, 8, 7], [(0, 3, 1), (1, 2, 1)], "tie, interleaved: C-N holds atom 0")]


def big_graph(n, seed=77):
    rng = np.random.default_rng([seed, n])
    if n == 0:
        return _freeze(np.zeros(0), np.zeros((0, 0)), "n=0")
    return random_graph(rng, n, f"random n={n}")


def path_graph(n):
    """A chain: the longest hop distance an n-atom molecule can have."""
    return from_bonds([6] * n, [(k + 1, k, 1) for k in range(n - 1)], f"chain n={n}")


@functools.lru_cache(maxsize=None)
def order_cases():
    """The molecules of the from-orders batch, in batch order: the sizes, an empty molecule between two others, the hard pairs each with a
    permuted copy, caps, ties, a type outside the vocabulary, and an asymmetric matrix whose upper triangle must be ignored."""
    rng = np.random.default_rng(5)
    cases = [_case(big_graph(n)) for n in GPU_SIZES]
    cases.insert(3, _case(big_graph(0)))
    cases.append(_case(path_graph(192)))
    for a, b in hard_pairs():
        cases += [_case(a), _case(b), _case(permuted(a, rng)), _case(permuted(b, rng))]
    cases += [_case(g) for g in cap_cases() + tie_cases()]
    g = cap_cases()[0]
    for bad in (-1, 5, 99):
        t = _types(g.Z)
        t[2] = bad
        cases.append(_case(g._replace(label=f"CH4 with type {bad} at atom 2"), types=t))
    g = decalin()
    o = g.orders.copy()
    o[np.triu_indices(10, 1)] = np.random.default_rng(9).integers(0, 4, size=45)
    cases.append(_case(g._replace(label="decalin, upper triangle scrambled"), orders=o))
    o = np.tril(g.orders) + np.triu(bicyclopentyl().orders)
    cases.append(_case(g._replace(label="decalin below, bicyclopentyl above the diagonal"), orders=o))
    return tuple(cases)


HARD_FIRST = len(GPU_SIZES) + 2           # index of the first hard-pair molecule in order_cases()


def qm9_type_tables(caps_by_symbol=None):
    tb = sc.tables("qm9")
    return ref.type_tables(tb.decoder, caps_by_symbol, sc.TABLES["allowed_bonds"])


@functools.lru_cache(maxsize=None)
def order_expected(atomic_numbers=False, mutant=None):
    """(key, info) per molecule of order_cases() from the definition.  `atomic_numbers`: the types are handed over as Z, the atoms outside
    the vocabulary as Z = 16, which QM9's table does not hold."""
    zs, caps = qm9_type_tables()
    out = []
    for c in order_cases():
        t = as_atomic_numbers(c.types) if atomic_numbers else c.types
        out.append(ref.key_from_orders(t, c.orders, zs, caps, atomic_numbers, mutant))
    return tuple(out)


def as_atomic_numbers(types):
    return np.array([ELEMENTS[t] if 0 <= t < len(ELEMENTS) else 16 for t in np.asarray(types)], np.int32)


# ---- clouds for the entry that starts from positions ---------------------------------------------------------------------------------------

def cloud(ds, n, seed=3, spacing=1.3, jitter=0.12):
    """n atoms on a jittered cubic lattice of `spacing` Angstrom at about six cells in ten, every pair at least 1e-3 pm from every threshold
    (above 25 atoms torch.cdist takes its matmul path, 1 ulp off the direct one on some pairs: with the gap both decide alike)."""
    tb = sc.tables(ds)
    if n == 0:
        return Cloud(np.zeros((0, 3), np.float32), np.zeros(0, np.int32), f"{ds} cloud n=0")
    side = max(2, int(np.ceil((1.7 * n) ** (1.0 / 3.0))))
    for attempt in range(64):
        rng = np.random.default_rng([seed, n, attempt, len(tb.decoder)])
        cells = rng.choice(side ** 3, size=n, replace=False)
        x = np.stack([cells // (side * side), (cells // side) % side, cells % side], 1).astype(np.float64) * spacing
        x = (x + rng.uniform(-jitter, jitter, size=x.shape)).astype(np.float32)
        t = rng.integers(0, tb.T, size=n).astype(np.int32)
        if so.threshold_gap(x, t, tb.bonds, tb.margins) >= 1e-3:
            x.setflags(write=False)
            t.setflags(write=False)
            return Cloud(x, t, f"{ds} cloud n={n}")
    raise AssertionError(f"no cloud of {n} atoms with a threshold gap of 1e-3 pm")


@functools.lru_cache(maxsize=None)
def clouds(ds):
    out = [cloud(ds, n) for n in GPU_SIZES]
    out.insert(4, cloud(ds, 0))                                      # an empty molecule between two others
    bad = cloud(ds, 17, seed=4)
    t = bad.types.copy()
    t[5] = 16                                                        # outside every vocabulary (at most 16 types)
    out.append(Cloud(bad.x, t, f"{ds} cloud n=17, type 16 at atom 5"))
    return tuple(out)


def ds_type_tables(ds, caps_by_symbol=None):
    return ref.type_tables(sc.tables(ds).decoder, caps_by_symbol, sc.TABLES["allowed_bonds"])


@functools.lru_cache(maxsize=None)
def cloud_expected(ds, limit):
    tb = sc.tables(ds)
    zs, caps = ds_type_tables(ds)
    return tuple(ref.key_from_positions(c.x, c.types, zs, caps, tb.bonds, tb.margins, limit) for c in clouds(ds))
