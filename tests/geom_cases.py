"""What tests/test_geom_data_cpu.py and tests/test_geom_data_gpu.py share: the fixture of tests/golden/make_geom_data_golden.py, the variants it
holds, and a numpy statement of the ingestion for generated arrays the fixture does not hold."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geom_small.npz")
VARIANTS = {"h_all": (False, None), "h_f6": (False, 6), "noh_all": (True, None), "noh_f6": (True, 6)}          # name: (remove_h, filter_size)
SPLITS = ("train", "valid", "test")
BATCH_SIZES = (1, 2, 3, 64)
_FIXTURE = None


def fixture():
    """The fixture as a dict of numpy arrays, loaded once and never written to."""
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(GOLDEN) as g:
            _FIXTURE = {k: g[k] for k in g.files}
        for v in _FIXTURE.values():
            v.setflags(write=False)
    return _FIXTURE


def tag(remove_h):
    return "noh" if remove_h else "h"


def ingest_numpy(rows, remove_h):
    """(sizes, z int32, pos fp32) of a conformer array as numpy states it: the rows of atomic number == 1.0 deleted, then load_split_data's
    ``np.nonzero(mol_id[:-1] - mol_id[1:])`` on the truncated ids, ``astype(int)`` and the fp32 cast."""
    rows = np.asarray(rows, dtype=np.float64)
    if remove_h:
        rows = rows[rows[:, 1] != 1.0]
    mol_id = rows[:, 0].astype(int)
    cuts = np.nonzero(mol_id[:-1] - mol_id[1:])[0] + 1
    sizes = np.diff(np.concatenate(([0], cuts, [len(rows)]))) if len(rows) else np.zeros(0, dtype=np.int64)
    return sizes.astype(np.int64), rows[:, 1].astype(int).astype(np.int32), rows[:, 2:5].astype(np.float32)


def generated_rows(R, seed, long_run=0):
    """R rows of molecules of 1 .. 12 atoms with ids that go up and down, a third of the atoms hydrogen, some molecules all hydrogen; with
    ``long_run`` the array starts with one molecule of that many rows."""
    rng = np.random.default_rng(seed)
    ids = [77] * min(long_run, R)
    while len(ids) < R:
        ids += [int(rng.integers(1, 9))] * int(rng.integers(1, 13))          # neighbours may share an id: they are one molecule
    rows = np.empty((R, 5), dtype=np.float64)
    rows[:, 0] = ids[:R]
    rows[:, 1] = rng.choice([1.0, 1.0, 6.0, 7.0, 8.0, 16.0], size=R)
    rows[:, 2:] = rng.standard_normal((R, 3)) * 3
    k = 0
    while k < R:                                                             # every seventh run of an id: all hydrogen
        e = k
        while e < R and rows[e, 0] == rows[k, 0]:
            e += 1
        if (k // 3) % 7 == 0 and e - k <= 12:
            rows[k:e, 1] = 1.0
        k = e
    return rows
