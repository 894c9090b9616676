"""What tests/test_stability_cases_cpu.py and tests/test_stability_cabi_gpu.py share: the reference's direct bond-order rule stated in numpy fp32
(`direct_rule`, with the mistakes a kernel could make as named mutants), and the case builders -- flat batches of molecules placed where the
stability kernel can go wrong.  The expected value of every case is the oracle's (oracle/stability_oracle.py, which calls torch.cdist as the
reference does), never the rule's.  No GPU code here; the builders exclude nothing."""
import functools
import importlib
import json
import os
from collections import namedtuple

import numpy as np

from oracle import stability_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("bio-diffusion_amd")
with open(os.path.join(ROOT, "bio-diffusion_amd", "data", "bond_tables.json")) as _f:
    TABLES = json.load(_f)
DATASETS = ("qm9", "geom")
FAMILIES = ("boundary_axis", "boundary_offaxis", "lattice", "collapsed", "nonfinite", "custom_thresholds")
MUTANTS = ("le", "sequential", "contracted", "reversed", "sqrt_truncated", "squared", "first_wins", "diagonal", "shift_mod32", "first64", "no_limit", "nearest_thr")
LATTICE_SIZES = (1, 2, 25, 26, 64, 65, 1024, 1025)
CELL = np.float32(7.0 / 32.0)                    # lattice step in Angstrom: every dx^2 + dy^2 + dz^2 on it is exact in fp32
F100 = np.float32(100.0)

# decoder, bonds (3 x [T, T] float64 lengths in pm), margins, thr (bonds + margin, float64), allowed (a set of valences per type),
# info (the dataset_info the product's wrappers take, with bonds1..3 set)
Tables = namedtuple("Tables", "ds decoder T bonds margins thr allowed info")
# x [N, 3] fp32, types [N] int32, sizes [B] int64, labels [B]
Batch = namedtuple("Batch", "x types sizes labels")


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------

def _fma32(a, b, c):
    """fl32(a * b + c) for fp32 arrays: the product of two fp32 values is exact in fp64, and one fp64 addition rounded to fp32 models the
    single rounding (held to torch.cdist bit for bit by test_stability_cases_cpu.py)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


SUMS = ("fma", "sequential", "contracted", "reversed")


def direct_distances(x, rule="fma"):
    """[n, n] fp32 distances in pm, and d2 in A^2, every step in fp32.  "fma" is the reference's direct cdist path:
    d2 = fma(dz, dz, fma(dy, dy, dx * dx)), then 100 * sqrt(d2).  The others are sums a kernel could compute in its place: "sequential"
    (dx*dx + dy*dy) + dz*dz with every product and sum rounded; "contracted" dx*dx + fma(dz, dz, dy*dy), what a compiler that is free to
    contract made of the sequential expression; "reversed" fma(dx, dx, fma(dy, dy, dz * dz))."""
    x = np.asarray(x, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (x[:, None, c] - x[None, :, c] for c in range(3))
        d2 = {"fma": lambda: _fma32(dz, dz, _fma32(dy, dy, dx * dx)),
              "sequential": lambda: (dx * dx + dy * dy) + dz * dz,
              "contracted": lambda: dx * dx + _fma32(dz, dz, dy * dy),
              "reversed": lambda: _fma32(dx, dx, _fma32(dy, dy, dz * dz))}[rule]()
        return F100 * np.sqrt(d2), d2


def direct_rule(x, types, thr, limit, allowed=None, mutant=None):
    """The reference's bond orders and stability triple of one molecule -> (orders [n, n] int64, (stable, stable atoms, n)).
    `thr`: three [T, T] float64 arrays `length + margin`; `allowed`: a set of valences per type (None: orders only, triple None).
    `mutant=None` is the rule.  A name out of MUTANTS is one mistake a kernel could make; the cases exist to tell each from the rule."""
    assert mutant is None or mutant in MUTANTS
    t = np.asarray(types, np.int64)
    n = len(t)
    d, d2 = direct_distances(x, mutant if mutant in SUMS else "fma")
    if mutant == "sqrt_truncated":                                  # a square root that is not correctly rounded (here: rounded towards zero)
        with np.errstate(invalid="ignore"):
            r = np.sqrt(d2.astype(np.float64))
            r32 = r.astype(np.float32)
            d = F100 * np.where(r32.astype(np.float64) > r, np.nextafter(r32, np.float32(0)), r32)
    d = d.astype(np.float64)                                        # the fp32 distance, widened, against the float64 threshold
    order = np.zeros((n, n), np.int64)
    for k in (0, 1, 2) if mutant != "first_wins" else (2, 1, 0):    # later thresholds overwrite earlier ones
        th = thr[k][t][:, t]
        if mutant == "nearest_thr":
            th = th.astype(np.float32).astype(np.float64)
        with np.errstate(invalid="ignore"):
            if mutant == "le":
                hit = d <= th
            elif mutant == "squared":
                hit = d2 < ((th / 100.0) ** 2).astype(np.float32)
            else:
                hit = d < th
        order[hit] = k + 1
    if limit and mutant != "no_limit":
        order[order > 1] = 1
    if mutant != "diagonal":
        np.fill_diagonal(order, 0)
    if mutant == "first64":
        order[64:, :] = 0
    if allowed is None:
        return order, None
    nb = order.sum(axis=1)
    if mutant == "shift_mod32":
        nb = nb % 32
    ok = np.array([int(b) in allowed[int(a)] for a, b in zip(t, nb)], bool)
    if mutant == "first64":
        ok = ok[:64]
    stable = int(ok.sum())
    return order, (int(stable == n), stable, n)


# ---- tables -----------------------------------------------------------------------------------------------------------------------------

_FRACTIONS = (0.1, 0.7, 0.3, 0.9, 0.45, 0.2, 0.6, 0.85)


@functools.lru_cache(maxsize=None)
def tables(ds, custom=False):
    """The shipped tables of a data set, or (`custom`) the same with every present length moved off the integers: 119 -> 119.1, 133 -> 133.7,
    120 -> 120.3 and their like (caller-supplied `dataset_info["bonds1..3"]`)."""
    info = pkg.dataset_info(ds)
    dec = info["atom_decoder"]
    bonds = so.bond_length_arrays(TABLES, info["atom_encoder"])
    if custom:
        for k, b in enumerate(bonds):
            for i, (a, c) in enumerate(zip(*np.nonzero(np.triu(b)))):
                b[a, c] = b[c, a] = b[a, c] + _FRACTIONS[(i + 3 * k) % len(_FRACTIONS)]
    margins = tuple(TABLES["margins"])
    thr = tuple(b + m for b, m in zip(bonds, margins))
    allowed = []
    for sym in dec:
        a = TABLES["allowed_bonds"][sym]
        allowed.append(frozenset([a] if isinstance(a, int) else a))
    for a in list(bonds) + list(thr):
        a.setflags(write=False)
    info["bonds1"], info["bonds2"], info["bonds3"] = bonds
    return Tables(ds, dec, len(dec), tuple(bonds), margins, thr, tuple(allowed), info)


def oracle_tables(tb):
    """The `tables` dictionary the oracle's functions take."""
    return {"margins": list(tb.margins), "allowed_bonds": TABLES["allowed_bonds"]}


# ---- batches ----------------------------------------------------------------------------------------------------------------------------

def _batch(mols):
    """mols: (x [n, 3], types [n], label)."""
    x = np.concatenate([np.asarray(m[0], np.float32).reshape(-1, 3) for m in mols]) if mols else np.zeros((0, 3), np.float32)
    t = np.concatenate([np.asarray(m[1], np.int32).reshape(-1) for m in mols]) if mols else np.zeros(0, np.int32)
    sizes = np.array([len(m[1]) for m in mols], np.int64)
    for a in (x, t, sizes):
        a.setflags(write=False)
    return Batch(x, t, sizes, tuple(m[2] for m in mols))


def molecules(batch):
    off = np.r_[0, np.cumsum(batch.sizes)]
    return [(batch.x[a:b], batch.types[a:b], lab) for a, b, lab in zip(off[:-1], off[1:], batch.labels)]


def _up(v):
    return np.nextafter(np.float32(v), np.float32(np.inf))


def _down(v):
    return np.nextafter(np.float32(v), np.float32(-np.inf))


def last_below(thr):
    """The largest fp32 d (Angstrom) with fl32(100 * d) < thr (float64, pm).  fl32(100 * d) is non-decreasing in d, so the walk ends."""
    d = np.float32(thr / 100.0)
    while float(F100 * d) < thr:
        d = _up(d)
    while not float(F100 * d) < thr:
        d = _down(d)
    assert float(F100 * d) < thr <= float(F100 * _up(d))
    return d


def _axis_pair(d, a, b, label):
    return np.array([[0, 0, 0], [d, 0, 0]], np.float32), (a, b), label


def _boundary_axis(tb, exact=False):
    """-> (molecules, how many of them sit on an fl32(thr) that lies below thr)."""
    mols, on_lower_rounding = [], 0
    for a in range(tb.T):
        for b in range(tb.T):
            for k in range(3):
                th = float(tb.thr[k][a, b])
                d = last_below(th)
                for dd, side in ((d, "below"), (_up(d), "above")):
                    assert np.sqrt(np.float32(dd * dd)) == dd                    # the distance the rule sees is the one asked for
                    mols.append(_axis_pair(dd, a, b, f"axis {tb.decoder[a]}-{tb.decoder[b]} thr{k + 1}={th!r} {side}"))
                if exact:                                                        # 100 d == fl32(thr) exactly, where such a d exists
                    th32 = np.float32(th)
                    for dd in (_down(d), d, _up(d), _up(_up(d))):
                        if F100 * dd == th32 and np.sqrt(np.float32(dd * dd)) == dd:
                            mols.append(_axis_pair(dd, a, b, f"axis {tb.decoder[a]}-{tb.decoder[b]} thr{k + 1}={th!r} at fl32(thr)"))
                            on_lower_rounding += float(th32) < th
    return mols, on_lower_rounding


@functools.lru_cache(maxsize=None)
def boundary_axis(ds):
    """For every ordered type pair and each threshold, two atoms on the x axis at the last fp32 distance below the threshold and at the next."""
    return _batch(_boundary_axis(tables(ds))[0])


@functools.lru_cache(maxsize=None)
def custom_thresholds(ds):
    """boundary_axis against non-integer float64 thresholds, plus the pair that sits on the fp32 rounding of a threshold."""
    tb = tables(ds, custom=True)
    th = np.unique(np.concatenate([t.reshape(-1) for t in tb.thr]))
    th32 = th.astype(np.float32).astype(np.float64)
    assert (th32 < th).sum() >= 2 and (th32 > th).sum() >= 2
    mols, on_lower_rounding = _boundary_axis(tb, exact=True)
    assert on_lower_rounding >= 2, "no pair sits on a threshold whose fp32 rounding lies below it"
    return _batch(mols)


def _pair_order(x, ta, tb_, thr, rule):
    d = float(direct_distances(x, rule)[0][0, 1])
    return max([k + 1 for k in range(3) if d < thr[k][ta, tb_]], default=0)


@functools.lru_cache(maxsize=None)
def boundary_offaxis(ds, per_rule=8, min_thresholds=4):
    """Two atoms in general position whose last bit decides: a seeded unit vector scaled to a threshold, x[0] of the second atom walked by ulps
    to the crossing, kept when the FMA chain and another sum of SUMS give different bond orders there -- `per_rule` pairs over at least
    `min_thresholds` thresholds for each of the other sums."""
    tb = tables(ds)
    rng = np.random.default_rng(11)
    mols = []
    for rule in SUMS[1:]:
        kept, used = 0, set()
        for _ in range(4000):
            if kept >= per_rule and len(used) >= min_thresholds:
                break
            a, b, k = int(rng.integers(tb.T)), int(rng.integers(tb.T)), int(rng.integers(3))
            th = float(tb.thr[k][a, b])
            if kept >= per_rule and th in used:
                continue
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            x = np.zeros((2, 3), np.float32)
            x[0] = rng.uniform(-1, 1, size=3)
            x[1] = x[0] + (u * th / 100.0).astype(np.float32)
            step, back = (_up, _down) if u[0] > 0 else (_down, _up)                  # step: away from the first atom, the distance grows
            inside = lambda: float(direct_distances(x)[0][0, 1]) < th
            for _ in range(4096):
                if not inside():
                    break
                x[1, 0] = step(x[1, 0])
            for _ in range(4096 + 4):                                                # back to the last value inside, then four more
                inside_now = inside()
                x[1, 0] = back(x[1, 0])
                if inside_now:
                    break
            for _ in range(3):
                x[1, 0] = back(x[1, 0])
            for _ in range(9):                                                       # the nine values around the crossing
                if _pair_order(x, a, b, tb.thr, "fma") != _pair_order(x, a, b, tb.thr, rule):
                    mols.append((x.copy(), (a, b), f"offaxis {tb.decoder[a]}-{tb.decoder[b]} thr{k + 1}={th!r} fma != {rule} #{kept}"))
                    used.add(th)
                    kept += 1
                    break
                x[1, 0] = step(x[1, 0])
        assert kept >= per_rule and len(used) >= min_thresholds, (rule, kept, len(used))
    return _batch(mols)


def _lattice_molecule(tb, n, cells, seed, duplicates=0):
    rng = np.random.default_rng([seed, n, cells])
    x = (rng.integers(0, cells, size=(n, 3)).astype(np.float32) * CELL).astype(np.float32)
    for i in range(duplicates):
        x[n - 1 - i] = x[i * 7]
    t = rng.integers(0, tb.T, size=n)
    return x, t


@functools.lru_cache(maxsize=None)
def lattice(ds, seed=5):
    """Molecules of 1 .. 1025 atoms on a 7/32 A lattice (box of 40 cells), an empty one between two others, and a dense 1025-atom one (box of
    12 cells, eight duplicated points).  Above 25 atoms the reference's cdist takes the matmul expansion, 1 ulp off the direct path on some
    pairs, so every such molecule is held at least 1e-3 pm away from every threshold: the two paths then decide alike."""
    tb = tables(ds)
    mols = []
    for n in LATTICE_SIZES:
        if n == 25:
            mols.append((np.zeros((0, 3), np.float32), np.zeros(0, np.int64), "lattice n=0"))
        x, t = _lattice_molecule(tb, n, 40, seed)
        mols.append((x, t, f"lattice n={n}"))
    x, t = _lattice_molecule(tb, 1025, 12, seed, duplicates=8)
    mols.append((x, t, "lattice n=1025 dense"))
    for x, t, lab in mols:
        if len(t) > 25:
            assert so.threshold_gap(x, t, tb.bonds, tb.margins) >= 1e-3, lab
    return _batch(mols)


@functools.lru_cache(maxsize=None)
def collapsed(ds):
    """1, 2, 11, 12 and 40 atoms at one point, and spread over 2 pm: every order is 3 (the reference's "0 + margin" quirk), the row sums are
    0, 3, 30, 33 and 117.  N is stable with 3 bonds, H with 1 -- which 33 is, modulo 32."""
    tb = tables(ds)
    rng = np.random.default_rng(7)
    mols = []
    for sym in ("N", "H"):
        a = tb.decoder.index(sym)
        for n in (1, 2, 11, 12, 40):
            p = np.tile(np.array([0.5, -0.25, 1.0], np.float32), (n, 1))
            mols.append((p, [a] * n, f"collapsed {sym} n={n} coincident"))
            q = (p + rng.uniform(0, 0.02 / np.sqrt(3.0), size=(n, 3))).astype(np.float32)
            mols.append((q, [a] * n, f"collapsed {sym} n={n} within 2 pm"))
    return _batch(mols)


@functools.lru_cache(maxsize=None)
def stable_molecule(ds):
    """A molecule of the golden fixture that the reference found stable, 4 <= n <= 25 (the direct cdist path with one atom more or less)."""
    with np.load(os.path.join(ROOT, "tests", "golden", "stability.npz")) as g:
        sizes, res = g[f"{ds}_sizes"], g[f"{ds}_result"]
        off = np.r_[0, np.cumsum(sizes)]
        m = next(i for i in range(len(sizes)) if res[i, 0] == 1 and 4 <= sizes[i] <= 24)
        return g[f"{ds}_x"][off[m]:off[m + 1]].astype(np.float32), g[f"{ds}_types"][off[m]:off[m + 1]].astype(np.int64)


@functools.lru_cache(maxsize=None)
def nonfinite(ds):
    """A stable molecule, and the same with one atom at NaN and with one atom at +Inf."""
    x, t = stable_molecule(ds)
    mols = [(x, t, "stable molecule")]
    for val, name in ((np.nan, "NaN"), (np.inf, "+Inf")):
        for atom, coord in ((0, 0), (len(t) - 1, 2)):
            y = x.copy()
            y[atom, coord] = val
            mols.append((y, t, f"{name} in atom {atom} coordinate {coord}"))
    return _batch(mols)


BAD_TYPES = (-1, "T", 16, 255)


@functools.lru_cache(maxsize=None)
def bad_types(ds):
    """A stable molecule with one atom's type outside [0, T).  The reference has no answer for it; the kernel's contract is that such an atom
    bonds to nothing and is unstable, and every other atom fares as in the molecule without it (`bad_types_expected`)."""
    tb = tables(ds)
    x, t = stable_molecule(ds)
    mols = []
    for bad in BAD_TYPES:
        for atom in (0, len(t) // 2, len(t) - 1):
            u = t.copy()
            u[atom] = tb.T if bad == "T" else bad
            mols.append((x, u, f"type {u[atom]} at atom {atom}"))
    u = t.copy()
    u[0], u[1] = -1, 255
    mols.append((x, u, "types -1 and 255 at atoms 0 and 1"))
    return _batch(mols)


# ---- expected values --------------------------------------------------------------------------------------------------------------------

def oracle_molecule(tb, x, t, limit):
    """(orders [n, n] int64, (stable, stable atoms, n)) of one molecule from the oracle, torch.cdist on its default path as the reference."""
    order = so.bond_order_matrix(x, t, tb.bonds, tb.margins, bool(limit))
    s, k, n = so.check_molecular_stability(x, t, tb.decoder, oracle_tables(tb), tb.bonds, limit_bonds_to_one=bool(limit))
    return order, (int(s), k, n)


def family_tables(family, ds):
    return tables(ds, custom=family == "custom_thresholds")


@functools.lru_cache(maxsize=None)
def expected(family, ds, limit):
    """Per molecule of the family's batch: (orders, triple), from the oracle.  Computed once, shared by the tests, never written to."""
    tb = family_tables(family, ds)
    if family == "bad_types":
        return bad_types_expected(ds, limit)
    out = []
    for x, t, _ in molecules(globals()[family](ds)):
        o, tr = oracle_molecule(tb, x, t, limit)
        o.setflags(write=False)
        out.append((o, tr))
    return tuple(out)


def bad_types_expected(ds, limit):
    tb = tables(ds)
    out = []
    for x, t, _ in molecules(bad_types(ds)):
        keep = (t >= 0) & (t < tb.T)
        o, (s, k, _) = oracle_molecule(tb, x[keep], t[keep], limit)
        full = np.zeros((len(t), len(t)), np.int64)
        full[np.ix_(keep, keep)] = o
        full.setflags(write=False)
        out.append((full, (0, k, len(t))))
    return tuple(out)
