"""Writes tests/golden/geom_small.npz: the unmodified reference GEOM-Drugs data path (build_geom_dataset.load_split_data, GeomDrugsDataset,
GeomDrugsTransform, CustomBatchSampler; imported under ref_harness.install_stubs() plus the stubs made here for msgpack and
torch_geometric.loader.dataloader) on a synthetic conformer array written to a temporary directory with a permutation of its own.

The fixture holds data only: the array (``rows``), the reference's atomic-number lists, and per variant -- ``h`` / ``noh`` (the array with the
rows of atomic number == 1.0 removed by numpy) x ``all`` / ``f6`` (filter_size 6) -- the permutation and, per split, what the reference makes:
the molecules of the sorted data set (their indices in the file, sizes, atomic numbers, fp32 positions), ``split_indices``, the concatenation of
the data set's items (x, one_hot, mask, index) and CustomBatchSampler's batch sizes and ``len`` for batch sizes 1, 2, 3 and 64 with and without
drop_last.  ``ing_<h|noh>_*`` is the whole file in file order (load_split_data with no validation or test part and the identity permutation).

The array (MOLECULES below): sizes 1 .. 9 with repeats; ids that go up and down; a one-atom conformer first and last; an all-hydrogen conformer
at the start, in the middle (between two conformers of one id, which therefore join when it disappears) and at the end; one row of atomic
number 1.5 (kept by the == 1.0 comparison, hydrogen after truncation); bismuth once; coordinates drawn in float64.

The order among molecules of one size is numpy's argsort (not a stable sort); at these sizes its AVX2 and AVX-512 builds agree.

    python tests/golden/make_geom_data_golden.py
"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh                      # noqa: E402

FILTER = 6
VARIANTS = {"h_all": (False, None), "h_f6": (False, FILTER), "noh_all": (True, None), "noh_f6": (True, FILTER)}
SPLITS = ("train", "valid", "test")
BATCH_SIZES = (1, 2, 3, 64)
HEAVY = [6, 6, 6, 7, 8, 6, 9, 16, 17, 6, 7, 8, 35, 6, 15]


def molecules():
    """[(id, [atomic numbers])]"""
    rng = np.random.default_rng(7)
    mols = [(5, [1.0]), (3, [6.0])]                                  # all-hydrogen and one atom; one heavy atom
    sizes = [2, 3, 3, 5, 9, 4, 4, 7, 1, 6, 8, 2, 5, 5, 3, 9, 6, 7, 4, 2, 8, 3, 5, 1, 6, 4, 9, 7, 2, 3, 6, 5, 8, 4, 3, 7, 5, 2, 6, 4, 9, 3, 8, 5]
    ids = rng.permutation(np.arange(10, 10 + len(sizes)))
    for k, (n, i) in enumerate(zip(sizes, ids)):
        z = rng.choice(HEAVY, size=n).astype(np.float64)
        z[rng.random(n) < 0.45] = 1.0
        if not (z != 1.0).any():
            z[0] = 6.0                                               # the all-hydrogen conformers are the ones placed by hand
        mols.append((int(i), list(z)))
        if k == 20:                                                  # id 9, all-H id 4, id 9: with the middle one gone the two join
            mols += [(9, [6.0, 1.0, 8.0]), (4, [1.0, 1.0]), (9, [7.0, 1.0])]
        if k == 30:
            mols.append((3, [1.5, 6.0, 1.0]))                        # 1.5: not == 1.0
        if k == 35:
            mols.append((2, [83.0, 1.0, 6.0, 6.0]))                  # bismuth, once
    mols += [(7, [8.0]), (1, [1.0])]                                 # one heavy atom; all-hydrogen and one atom
    return mols


def conformer_array():
    rng = np.random.default_rng(11)
    rows = []
    for i, zs in molecules():
        for z in zs:
            rows.append([float(i), z] + list(rng.standard_normal(3) * 2.5))
    return np.array(rows, dtype=np.float64)


def main():
    assert rh.reference_available(), "reference checkout not found"
    rh.install_stubs()
    sys.modules.setdefault("msgpack", types.ModuleType("msgpack"))
    tgl = types.ModuleType("torch_geometric.loader.dataloader")
    tgl.DataLoader = type("DataLoader", (), {})
    sys.modules["torch_geometric.loader.dataloader"] = tgl
    sys.modules["torch_geometric.loader"].__path__ = []
    geom = importlib.import_module("src.datamodules.components.edm.build_geom_dataset")
    config = importlib.import_module("src.datamodules.components.edm.datasets_config")
    from torch.utils.data import SequentialSampler

    rows = conformer_array()
    assert 200 <= len(rows) <= 400 and (rows[:, 1:].astype(np.float32).astype(np.float64) != rows[:, 1:]).any()
    out = {"rows": rows, "atomic_nb_h": np.array(config.GEOM_WITH_H["atomic_nb"], dtype=np.int64),
           "atomic_nb_noh": np.array(config.GEOM_NO_H["atomic_nb"], dtype=np.int64), "filter_size": np.int64(FILTER)}
    rng = np.random.default_rng(3)

    def run(array, perm, filter_size, val, test, directory):
        path = os.path.join(directory, "GEOM_drugs_30.npy")
        np.save(path, array)
        np.save(os.path.join(directory, "GEOM_permutation.npy"), perm)
        return geom.load_split_data(path, val_proportion=val, test_proportion=test, filter_size=filter_size)

    def file_index(array):
        """data pointer of a molecule's view -> its index in the file"""
        mol_id = array[:, 0].astype(int)
        starts = np.concatenate(([0], np.nonzero(mol_id[:-1] - mol_id[1:])[0] + 1))
        return starts

    for remove_h, tag in ((False, "h"), (True, "noh")):
        array = rows[rows[:, 1] != 1.0] if remove_h else rows
        starts = file_index(array)
        M = len(starts)
        with tempfile.TemporaryDirectory() as d:
            whole, _, _ = run(array, np.arange(M), None, 0.0, 0.0, d)
        assert len(whole) == M
        out[f"ing_{tag}_sizes"] = np.array([m.shape[0] for m in whole], dtype=np.int64)
        out[f"ing_{tag}_z"] = np.concatenate([m[:, 0].astype(int) for m in whole]).astype(np.int32)
        out[f"ing_{tag}_pos"] = torch.cat([torch.from_numpy(m[:, -3:].copy()).type(torch.float32) for m in whole]).numpy()
        sizes = out[f"ing_{tag}_sizes"]
        info = config.GEOM_NO_H if remove_h else config.GEOM_WITH_H
        transform = geom.GeomDrugsTransform(info, include_charges=False, device="cpu", sequential=False)
        for name, (rh_, filter_size) in VARIANTS.items():
            if rh_ != remove_h:
                continue
            kept = np.arange(M) if filter_size is None else np.flatnonzero(sizes <= filter_size)
            assert filter_size is None or 0 < len(kept) < M
            perm = rng.permutation(len(kept)).astype("int32")
            out[f"{name}_perm"] = perm
            with tempfile.TemporaryDirectory() as d:
                parts = dict(zip(SPLITS, run(array, perm, filter_size, 0.1, 0.1, d)))
                # the molecules are views of the loaded array: the offset of a view's first element names its molecule
                for split in SPLITS:
                    ds = geom.GeomDrugsDataset(parts[split], transform=transform)
                    base = ds.data_list[0].base
                    offs = [(m.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // (5 * 8) for m in ds.data_list]
                    order = np.searchsorted(starts, offs)
                    assert (starts[order] == offs).all() and len(set(order.tolist())) == len(order)
                    key = f"{name}_{split}"
                    out[f"{key}_order"] = order.astype(np.int64)
                    out[f"{key}_split_indices"] = np.asarray(ds.split_indices, dtype=np.int64)
                    out[f"{key}_sizes"] = np.array([m.shape[0] for m in ds.data_list], dtype=np.int64)
                    assert (out[f"{key}_sizes"] == sizes[order]).all() and (np.diff(out[f"{key}_sizes"]) >= 0).all()
                    out[f"{key}_z"] = np.concatenate([m[:, 0].astype(int) for m in ds.data_list]).astype(np.int32)
                    items = [ds[i] for i in range(len(ds))]
                    out[f"{key}_x"] = torch.cat([it.x for it in items]).numpy()
                    out[f"{key}_one_hot"] = torch.cat([it.one_hot for it in items]).numpy()
                    out[f"{key}_mask"] = torch.cat([it.mask for it in items]).numpy()
                    out[f"{key}_index"] = torch.cat([it.index for it in items]).numpy()
                    assert out[f"{key}_x"].dtype == np.float32 and out[f"{key}_one_hot"].dtype == np.float32 and out[f"{key}_index"].dtype == np.int64
                    for bs in BATCH_SIZES:
                        for drop_last in (False, True):
                            sampler = geom.CustomBatchSampler(SequentialSampler(ds), bs, drop_last, ds.split_indices)
                            batches = list(sampler)
                            flat = [i for b in batches for i in b]
                            assert flat == list(range(len(flat)))
                            out[f"{key}_bs{bs}_dl{int(drop_last)}_counts"] = np.array([len(b) for b in batches], dtype=np.int64)
                            out[f"{key}_bs{bs}_dl{int(drop_last)}_len"] = np.int64(len(sampler))
                assert len(out[f"{name}_train_split_indices"]) >= 3 and len(out[f"{name}_valid_split_indices"]) >= 1
    assert len(out["ing_noh_sizes"]) == len(out["ing_h_sizes"]) - 4            # three all-hydrogen conformers gone, two conformers joined
    assert (out["ing_h_z"] == 83).sum() == 1 and (rows[:, 1] == 1.5).sum() == 1
    path = os.path.join(HERE, "geom_small.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes, {len(rows)} rows, {len(out['ing_h_sizes'])} / {len(out['ing_noh_sizes'])} molecules")


if __name__ == "__main__":
    main()
