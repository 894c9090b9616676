"""The definition of include/gcdm_molgraph.h in Python integers -- TEST INFRASTRUCTURE ONLY: validity by valence caps, fragments, and the
permutation-invariant 64-bit key of the largest fragment, per molecule, from (Z, order matrix) or from positions (bond orders of
oracle.stability_oracle, torch.cdist as the reference calls it).  `reference_metrics` is BasicMolecularMetrics.evaluate_rdmols
(rdkit_functions.py:168-185) on keys.  `mutant=None` is the definition; a name out of MUTANTS is one mistake a kernel could make, and the
cases of tests/molgraph_cases.py exist to tell each from the definition (tests/test_molgraph_cpu.py)."""
from collections import deque

import numpy as np

from oracle import stability_oracle as so

MASK = (1 << 64) - 1
K1, K2, K3, K4, K5 = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0xD6E8FEB86659FD93, 0xA0761D6478BD642F
ROUNDS, MAX_ATOMS = 16, 192
MUTANTS = ("caps_on_fragment", "lt_at_cap", "tie_last", "no_order", "no_distance", "upper_triangle", "one_round_fewer")
SYMBOL_Z = {"H": 1, "B": 5, "C": 6, "N": 7, "O": 8, "F": 9, "Al": 13, "Si": 14, "P": 15, "S": 16, "Cl": 17, "As": 33, "Br": 35, "I": 53,
            "Hg": 80, "Bi": 83}


def mix(v):
    v &= MASK
    v ^= v >> 30
    v = (v * 0xBF58476D1CE4E5B9) & MASK
    v ^= v >> 27
    v = (v * 0x94D049BB133111EB) & MASK
    v ^= v >> 31
    return v


def signed(v):
    """The uint64 key as the int64 the device stores."""
    return v - (1 << 64) if v >> 63 else v


def symmetric_orders(orders, in_vocab=None, mutant=None):
    """The n x n matrix the graph phases see: the strict lower triangle of `orders` mirrored (the upper one is never read), rows and columns
    of atoms outside the vocabulary cleared."""
    o = np.asarray(orders, np.int64)
    n = o.shape[0]
    o = o.reshape(n, n)
    low = np.triu(o, 1).T if mutant == "upper_triangle" else np.tril(o, -1)
    full = low + low.T
    if in_vocab is not None:
        keep = np.asarray(in_vocab, bool)
        full[~keep, :] = 0
        full[:, ~keep] = 0
    return full


def components(o):
    """Connected components over pairs of order > 0, as lists of ascending atom indices, ordered by their lowest atom."""
    n = len(o)
    seen, out = [False] * n, []
    for s in range(n):
        if seen[s]:
            continue
        seen[s], comp, queue = True, [s], deque([s])
        while queue:
            i = queue.popleft()
            for j in np.flatnonzero(o[i]):
                if not seen[j]:
                    seen[j] = True
                    comp.append(int(j))
                    queue.append(int(j))
        out.append(sorted(comp))
    return out


def hop_distances(o, frag):
    """{i: {j: hops}} inside the fragment."""
    dist = {}
    for s in frag:
        d, queue = {s: 0}, deque([s])
        while queue:
            i = queue.popleft()
            for j in np.flatnonzero(o[i]):
                if int(j) not in d:
                    d[int(j)] = d[i] + 1
                    queue.append(int(j))
        dist[s] = d
    return dist


def graph_key(Z, orders, caps=None, in_vocab=None, mutant=None):
    """-> (key as int64, (valid, n_fragments, n_largest, n)).  `Z` atomic numbers [n] (0 for an atom outside the vocabulary), `orders` [n, n]
    (only i > j is read), `caps` per atom (None or < 0: no cap), `in_vocab` per atom (None: all inside)."""
    assert mutant is None or mutant in MUTANTS
    Z = [int(z) for z in Z]
    n = len(Z)
    if n > MAX_ATOMS:
        return 0, (-1, 0, 0, n)
    inside = [True] * n if in_vocab is None else [bool(v) for v in in_vocab]
    o = symmetric_orders(np.zeros((0, 0)) if n == 0 else orders, inside if n else None, mutant)
    frags = components(o)
    if mutant == "tie_last":
        frag = max(reversed(frags), key=len, default=[])
    else:
        frag = max(frags, key=len, default=[])                       # the first of the largest: the one holding the lowest atom index
    valid = all(inside)
    for i in (frag if mutant == "caps_on_fragment" else range(n)):
        cap = -1 if caps is None else int(caps[i])
        total = int(o[i].sum())
        if cap >= 0 and (total >= cap if mutant == "lt_at_cap" else total > cap):
            valid = False
    dist = hop_distances(o, frag)
    c = {}
    for i in frag:
        acc = 0
        if mutant != "no_distance":
            for j in frag:
                if j != i:
                    acc += mix(((dist[i][j] << 8) | Z[j]) + K2)
        c[i] = mix(Z[i] * K1 + acc)
    for _ in range(ROUNDS - (1 if mutant == "one_round_fewer" else 0)):
        nxt = {}
        for i in frag:
            acc = c[i] * K3
            for j in np.flatnonzero(o[i]):
                acc += mix(c[int(j)] + (0 if mutant == "no_order" else int(o[i, j])) * K4)
            nxt[i] = mix(acc)
        c = nxt
    key = mix(len(frag) * K5 + sum(mix(v) for v in c.values()))
    return signed(key), (int(valid), len(frags), len(frag), n)


def type_tables(decoder, caps_by_symbol=None, allowed_bonds=None):
    """(atomic numbers, caps) per vocabulary type; the default cap is the largest valence `allowed_bonds` gives the element."""
    zs = [SYMBOL_Z[s] for s in decoder]
    caps = []
    for s in decoder:
        a = allowed_bonds[s]
        caps.append(a if isinstance(a, int) else max(a))
    for s, v in (caps_by_symbol or {}).items():
        caps[list(decoder).index(s)] = int(v)
    return zs, caps


def resolve_types(types, zs, types_are_atomic_numbers=False):
    """Vocabulary index per atom, -1 outside the vocabulary."""
    out = []
    for t in np.asarray(types, np.int64).reshape(-1):
        if types_are_atomic_numbers:
            out.append(zs.index(int(t)) if int(t) in zs else -1)
        else:
            out.append(int(t) if 0 <= int(t) < len(zs) else -1)
    return out


def key_from_orders(types, orders, zs, caps, types_are_atomic_numbers=False, mutant=None):
    k = resolve_types(types, zs, types_are_atomic_numbers)
    return graph_key([zs[i] if i >= 0 else 0 for i in k], orders, [caps[i] if i >= 0 else -1 for i in k], [i >= 0 for i in k], mutant)


def oracle_orders(x, types, zs, bonds, margins, limit, types_are_atomic_numbers=False, direct=False):
    """The bond orders of one molecule from the oracle; an atom outside the vocabulary is classified as type 0 and then cleared.  `direct`:
    torch.cdist on its direct path at every size -- the rule the kernels keep -- where the default switches to the matmul expansion above 25
    atoms, 1 ulp off on some pairs (the case builders keep every pair 1e-3 pm from the thresholds; samples of a model cannot be)."""
    k = np.array(resolve_types(types, zs, types_are_atomic_numbers), np.int64)
    n = len(k)
    if n == 0:
        return np.zeros((0, 0), np.int64)
    o = so.bond_order_matrix(np.asarray(x, np.float32).reshape(n, 3), np.where(k >= 0, k, 0), bonds, margins, bool(limit), direct)
    o[k < 0, :] = 0
    o[:, k < 0] = 0
    return o


def key_from_positions(x, types, zs, caps, bonds, margins, limit, types_are_atomic_numbers=False, mutant=None, direct=False):
    if len(np.asarray(types).reshape(-1)) > MAX_ATOMS:
        return 0, (-1, 0, 0, len(np.asarray(types).reshape(-1)))
    return key_from_orders(types, oracle_orders(x, types, zs, bonds, margins, limit, types_are_atomic_numbers, direct), zs, caps, types_are_atomic_numbers, mutant)


def reference_metrics(keys, valid, dataset_keys=None):
    """BasicMolecularMetrics.evaluate_rdmols (rdkit_functions.py:168-185) with keys for SMILES -> [validity, uniqueness, novelty]."""
    kept = [int(k) for k, v in zip(keys, valid) if int(v) == 1]
    validity = len(kept) / len(keys)
    if validity > 0:
        unique = list(set(kept))
        uniqueness = len(unique) / len(kept)
        if dataset_keys is not None:
            known = set(int(k) for k in dataset_keys)
            novelty = sum(1 for k in unique if k not in known) / len(unique)
        else:
            novelty = 0.0
    else:
        uniqueness, novelty = 0.0, 0.0
    return [validity, uniqueness, novelty]
