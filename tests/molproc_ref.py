"""The definition of include/gcdm_molproc.h in plain Python -- TEST INFRASTRUCTURE ONLY: which molecules and atoms survive `sanitize` and
`largest_frag`, the renumbering of the survivors and the order of their bond list.  The molecule, its orders and its validity are those of
tests/molgraph_ref.py (symmetric_orders, resolve_types); the components here are found another way (union-find against its breadth-first
search) and tests/test_molproc_cpu.py holds both to networkx and scipy.  `mutant=None` is the definition; a name out of MUTANTS is one mistake
the kernels could make, and the cases of the GPU files exist to tell each from the definition."""
from collections import namedtuple

import numpy as np

import molgraph_ref as ref

MAX_ATOMS = ref.MAX_ATOMS
SANITIZE, LARGEST_FRAG = 1, 2
MUTANTS = ("tie_last", "sanitize_fragment_only", "bonds_column_major", "not_renumbered", "dropped_as_empty")
# one molecule: info (valid, n_fragments, n_largest, n); kept False = dropped (atoms / bonds then empty); atoms = the surviving original
# indices, ascending; new_index per original atom (-1: does not survive; None for a molecule that is too large); bonds (new_i, new_j, order)
One = namedtuple("One", "info kept atoms new_index bonds")
Batch = namedtuple("Batch", "info keep new_index counts totals src_atom src_molecule mol_offsets bonds bond_offsets written")


def components(o):
    """Connected components over pairs of order > 0 by union-find, as ascending lists ordered by their lowest atom."""
    n = len(o)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i in range(n):
        for j in range(i):
            if o[i][j] > 0:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)                    # the root is the lowest atom of the component
    groups = {}
    for i in range(n):
        groups.setdefault(find(i), []).append(i)
    return [groups[r] for r in sorted(groups)]


def largest_fragment(frags, mutant=None):
    """Among the largest the one holding the lowest atom index: the first, in the order of `components`."""
    if mutant == "tie_last":
        return max(reversed(frags), key=len, default=[])
    return max(frags, key=len, default=[])


def process_one(types, orders, zs, caps, flags, atomic_numbers=False, mutant=None):
    """`types` [n] as handed to the kernel, `orders` [n, n] (only i > j is read), `zs` / `caps` per vocabulary type."""
    assert mutant is None or mutant in MUTANTS
    n = len(types)
    if n > MAX_ATOMS:
        return One((-1, 0, 0, n), False, [], None, [])
    k = ref.resolve_types(types, zs, atomic_numbers)
    inside = [t >= 0 for t in k]
    o = ref.symmetric_orders(np.zeros((0, 0)) if n == 0 else orders, inside if n else None)
    frags = components(o)
    big = largest_fragment(frags, mutant)
    valid = all(inside)
    for i in range(n):
        if k[i] >= 0 and caps[k[i]] >= 0 and int(o[i].sum()) > caps[k[i]]:
            valid = False
    info = (int(valid), len(frags), len(largest_fragment(frags)), n)
    verdict = valid
    if mutant == "sanitize_fragment_only":
        verdict = all(inside[i] and not (caps[k[i]] >= 0 and int(o[i].sum()) > caps[k[i]]) for i in big)
    if (flags & SANITIZE) and not verdict:
        if mutant == "dropped_as_empty":
            return One(info, True, [], [-1] * n, [])
        return One(info, False, [], [-1] * n, [])
    atoms = sorted(big) if flags & LARGEST_FRAG else list(range(n))
    new_index = [-1] * n
    for r, a in enumerate(atoms):
        new_index[a] = a if mutant == "not_renumbered" else r
    pairs = [(i, j) for i in atoms for j in atoms if j < i and o[i][j] > 0]             # row-major over the lower triangle
    if mutant == "bonds_column_major":
        pairs.sort(key=lambda p: (p[1], p[0]))
    return One(info, True, atoms, new_index, [(new_index[i], new_index[j], int(o[i][j])) for i, j in pairs])


def process_batch(mols, zs, caps, flags, atomic_numbers=False, mutant=None):
    """`mols`: (types, orders) per molecule.  Everything select and emit write, as arrays; `written` marks the atoms whose keep and new_index
    are written (those of a molecule that is too large are not)."""
    ones = [process_one(t, o, zs, caps, flags, atomic_numbers, mutant) for t, o in mols]
    N = sum(len(t) for t, _ in mols)
    keep, new_index, written = np.zeros(N, np.uint8), np.full(N, -1, np.int32), np.zeros(N, bool)
    counts, src_atom, src_mol, bonds, mol_off, bond_off = [], [], [], [], [0], [0]
    a0 = 0
    for m, ((t, _), one) in enumerate(zip(mols, ones)):
        if one.new_index is not None:
            written[a0:a0 + len(t)] = True
            new_index[a0:a0 + len(t)] = one.new_index
            keep[a0:a0 + len(t)] = [v >= 0 for v in one.new_index]
        counts.append((len(one.atoms), len(one.bonds), int(one.kept)))
        if one.kept:
            src_mol.append(m)
            src_atom += [a0 + a for a in one.atoms]
            bonds += one.bonds
            mol_off.append(len(src_atom))
            bond_off.append(len(bonds))
        a0 += len(t)
    i32, i64 = np.int32, np.int64
    return Batch(np.array([o.info for o in ones], i32).reshape(-1, 4), keep, new_index, np.array(counts, i32).reshape(-1, 3),
                 np.array([len(src_atom), len(bonds), len(src_mol)], i64), np.array(src_atom, i64), np.array(src_mol, i64), np.array(mol_off, i64),
                 np.array(bonds, i32).reshape(-1, 3), np.array(bond_off, i64), written)
