"""The GEOM-Drugs conformer file path without a GPU: include/gcdm_geom.h <-> libgcdm_ops.so exports <-> native.GEOM_SIGNATURES, the header as C99
linked from plain C, argument refusal before any HIP call, the split orders and ``split_indices`` against the reference's own
(tests/golden/geom_small.npz: load_split_data + GeomDrugsDataset), the sequential batches against its CustomBatchSampler, and the loader's
three refusals."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import geom_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
HEADER = os.path.join(ROOT, "include", "gcdm_geom.h")
TABLES = ("OPS_SIGNATURES", "MP_TRAIN_SIGNATURES", "MP_TILE_SIGNATURES", "GCP2_SIGNATURES", "OPTIM_SIGNATURES", "CLASSIFIER_SIGNATURES",
          "OBJECTIVE_SIGNATURES", "GRAD_BUCKET_SIGNATURES", "MATRIX_MODE_SIGNATURES", "DATA_SIGNATURES")
Z = None


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(gcdm_geom_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
    return out


def test_header_declares_exactly_the_signature_table():
    assert _declared() == {k: len(v) for k, v in native.GEOM_SIGNATURES.items()}
    assert sorted(native.GEOM_SIGNATURES) == ["gcdm_geom_finish", "gcdm_geom_gather", "gcdm_geom_ingest", "gcdm_geom_workspace_bytes"]
    for t in TABLES:
        assert not set(native.GEOM_SIGNATURES) & set(getattr(native, t)), t
    assert not set(native.GEOM_SIGNATURES) & set(native.EXPORTS)
    text = open(HEADER).read()
    for name in ("TILE", "STATE_WORDS", "MAX_ROWS", "FLAG_BAD_ROW", "FLAG_CAPACITY", "FLAG_ACCOUNT", "WS_BYTES", "WS_LAUNCHES", "WS_TILE"):
        assert re.search(rf"#define GCDM_GEOM_{name} {getattr(native, 'GEOM_' + name)}\b", text), name
    assert len({native.GEOM_FLAG_BAD_ROW, native.GEOM_FLAG_CAPACITY, native.GEOM_FLAG_ACCOUNT}) == 3


def test_header_and_kernels_are_library_dependencies():
    assert HEADER in native.OPS_HEADERS
    assert os.path.join(ROOT, "bio-diffusion_amd", "csrc", "gcdm_ops.geom.hip.h") in native.OPS_HEADERS
    assert '#include "gcdm_ops.geom.hip.h"' in open(native.OPS_SOURCES[0]).read()


@pytest.fixture(scope="module")
def lib():
    path = native.OPS_LIB_PATH
    if not os.path.exists(path):
        pytest.skip("libgcdm_ops.so not built (run __graft_entry__.build())")
    stale = [d for d in native.OPS_SOURCES + native.OPS_HEADERS if os.path.getmtime(d) > os.path.getmtime(path)]
    if stale:
        pytest.skip(f"libgcdm_ops.so is older than {stale} (run __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    for name, sig in native.GEOM_SIGNATURES.items():
        assert hasattr(lib, name), name
        getattr(lib, name).argtypes = sig
        getattr(lib, name).restype = native.GEOM_RESTYPES.get(name, ctypes.c_int)
    return lib


def test_library_exports_the_entries_and_the_loader_binds_them(lib):
    T = lib.gcdm_geom_workspace_bytes(native.GEOM_WS_TILE, 0)
    assert T == native.GEOM_TILE and T % 64 == 0
    w = lambda R: lib.gcdm_geom_workspace_bytes(native.GEOM_WS_BYTES, R)
    assert w(0) == 0 and w(1) % 256 == 0 and w(1) > 0 and w(T) == w(1) and w(T + 1) >= w(T) and w(1 << 22) >= 2 * 4096 * 40
    assert lib.gcdm_geom_workspace_bytes(native.GEOM_WS_LAUNCHES, 0) == 0 and lib.gcdm_geom_workspace_bytes(native.GEOM_WS_LAUNCHES, 5) == 3
    for which, R in ((3, 8), (-1, 8), (0, -1), (0, native.GEOM_MAX_ROWS + 1)):
        assert lib.gcdm_geom_workspace_bytes(which, R) == -1
    bound = native.load_ops()
    for name, sig in native.GEOM_SIGNATURES.items():
        assert getattr(bound, name).argtypes == sig


def test_header_is_c99_and_links_from_plain_c(lib, tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "gcdm_geom.h"\n'
                   "int main(void) {\n"
                   "  int32_t flags = 0;\n"
                   "  long long w = (long long)gcdm_geom_workspace_bytes(GCDM_GEOM_WS_BYTES, 5000);\n"
                   "  long long t = (long long)gcdm_geom_workspace_bytes(GCDM_GEOM_WS_TILE, 0);\n"
                   "  int empty = gcdm_geom_ingest(0, 0, 1, 0, 0, 0, 0, 0, 0, 0, &flags, 0);\n"
                   "  int bad = gcdm_geom_ingest(0, 8, 0, 0, 0, 0, 0, 8, 8, 0, &flags, 0);\n"
                   "  int none = gcdm_geom_gather(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);\n"
                   '  printf("%lld %lld %d %d %d\\n", w, t, empty, bad, none);\n'
                   "  return !(w > 0 && t == GCDM_GEOM_TILE && empty == 0 && bad == -1 && none == 0 && GCDM_GEOM_FLAG_ACCOUNT == 4);\n}\n")
    exe = tmp_path / "t"
    libdir = os.path.dirname(native.OPS_LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe),
                        "-L", libdir, "-l:libgcdm_ops.so", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"], text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], text=True, capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_every_entry_refuses_bad_arguments_before_any_launch(lib):
    """Null or dangling pointers throughout: a call that got past its checks would fault, so every case must come back with -1."""
    X = ctypes.c_void_p(64)                                      # "some pointer": never dereferenced on the host

    def ingest(R=8, remove_h=0, cap_atoms=8, cap_mols=8, ptrs=(X,) * 7):
        rows, state, z, pos, atom_ptr, ws, flags = ptrs
        return lib.gcdm_geom_ingest(rows, R, remove_h, state, z, pos, atom_ptr, cap_atoms, cap_mols, ws, flags, Z)

    cases = [ingest(R=-1), ingest(R=native.GEOM_MAX_ROWS + 1), ingest(remove_h=2), ingest(remove_h=-1), ingest(cap_atoms=-1), ingest(cap_mols=-1)]
    cases += [ingest(ptrs=tuple(Z if i == j else X for i in range(7))) for j in range(7)]
    for k, status in enumerate(cases):
        assert status == -1, k
    assert ingest(R=0, ptrs=(Z,) * 7) == 0                        # nothing to do: no launch
    assert ingest(R=0, cap_atoms=-1, ptrs=(Z,) * 7) == -1

    def finish(cap_mols=8, ptrs=(X,) * 4):
        state, atom_ptr, MA, flags = ptrs
        return lib.gcdm_geom_finish(state, atom_ptr, cap_mols, MA, flags, Z)

    for k, status in enumerate([finish(cap_mols=-1)] + [finish(ptrs=tuple(Z if i == j else X for i in range(4))) for j in range(4)]):
        assert status == -1, k

    def gather(M_in=4, A_in=9, M_out=3, A_out=7, ptrs=(X,) * 8):
        pin, zin, posin, order, pout, zout, posout, flags = ptrs
        return lib.gcdm_geom_gather(pin, zin, posin, M_in, A_in, order, pout, M_out, A_out, zout, posout, flags, Z)

    cases = [gather(M_in=-1), gather(A_in=-1), gather(M_out=-1), gather(A_out=-1), gather(M_out=1 << 32)]
    cases += [gather(ptrs=tuple(Z if i == j else X for i in range(8))) for j in range(8)]
    for k, status in enumerate(cases):
        assert status == -1, k
    assert gather(M_out=0, A_out=0, ptrs=(Z,) * 8) == 0


# ---- the host side --------------------------------------------------------------------------------------------------------------------------
def test_species_lists_are_the_reference_ones():
    g = gc.fixture()
    assert list(pkg.data.GEOM_ATOMIC_NUMBERS) == g["atomic_nb_h"].tolist()
    assert [s for s in pkg.data.GEOM_ATOMIC_NUMBERS if s != 1] == g["atomic_nb_noh"].tolist()
    assert len(pkg.data.GEOM_ATOMIC_NUMBERS) == len(pkg.dataset_info("geom")["atom_decoder"]) <= native.DATA_MAX_TYPES


def test_numpy_statement_of_the_ingestion_equals_the_reference():
    """geom_cases.ingest_numpy is the expectation of the generated arrays in the GPU file: here it is held to the reference on the fixture."""
    g = gc.fixture()
    for remove_h in (False, True):
        sizes, z, pos = gc.ingest_numpy(g["rows"], remove_h)
        t = gc.tag(remove_h)
        assert np.array_equal(sizes, g[f"ing_{t}_sizes"]) and np.array_equal(z, g[f"ing_{t}_z"])
        assert pos.dtype == np.float32 and np.array_equal(pos.view(np.uint32), g[f"ing_{t}_pos"].view(np.uint32))


@pytest.mark.parametrize("variant", list(gc.VARIANTS))
def test_split_orders_and_split_indices_equal_the_reference(variant):
    g = gc.fixture()
    remove_h, filter_size = gc.VARIANTS[variant]
    sizes = g[f"ing_{gc.tag(remove_h)}_sizes"]
    orders = pkg.data.geom_split_orders(sizes, g[f"{variant}_perm"], 0.1, 0.1, filter_size)
    assert sorted(orders) == sorted(gc.SPLITS)
    seen = []
    for split in gc.SPLITS:
        order, split_indices = orders[split]
        assert order.dtype == np.int64 and split_indices.dtype == np.int64
        assert np.array_equal(order, g[f"{variant}_{split}_order"]), split
        assert np.array_equal(split_indices, g[f"{variant}_{split}_split_indices"]), split
        assert np.array_equal(sizes[order], g[f"{variant}_{split}_sizes"])
        seen += order.tolist()
    kept = np.arange(len(sizes)) if filter_size is None else np.flatnonzero(sizes <= filter_size)
    assert sorted(seen) == kept.tolist()                          # the three splits share no molecule and lose none
    assert len(orders["valid"][0]) == int(len(kept) * 0.1) == len(orders["test"][0])


def test_split_orders_refuse_what_the_reference_refuses():
    sizes = np.array([3, 4, 5])
    with pytest.raises(ValueError, match="No molecules left"):
        pkg.data.geom_split_orders(sizes, np.arange(3), filter_size=2)
    with pytest.raises(IndexError):
        pkg.data.geom_split_orders(sizes, np.array([0, 1, 2]), filter_size=4)          # the permutation of the unfiltered list
    o = pkg.data.geom_split_orders(sizes, np.array([2, 0, 1]), 0.34, 0.34)
    assert o["valid"][0].tolist() == [2] and o["test"][0].tolist() == [0] and o["train"][0].tolist() == [1]


def _sorted_cpu_dataset(variant, split):
    """A data set on the host with the fixture's sorted molecules: what geom_splits hands over, as far as the batch boundaries can see."""
    g = gc.fixture()
    sizes, z, x = g[f"{variant}_{split}_sizes"], g[f"{variant}_{split}_z"], g[f"{variant}_{split}_x"]
    ptr = np.concatenate(([0], np.cumsum(sizes)))
    confs = [np.concatenate((z[a:b, None].astype(np.float32), x[a:b]), axis=1) for a, b in zip(ptr[:-1], ptr[1:])]
    ds = pkg.MoleculeDataset.from_conformers(confs, "cpu", included_species=list(pkg.data.GEOM_ATOMIC_NUMBERS))
    assert ds.sorted_by_size is False and ds.split_indices is None
    ds.sorted_by_size, ds.split_indices = True, g[f"{variant}_{split}_split_indices"]
    return ds


@pytest.mark.parametrize("variant", list(gc.VARIANTS))
def test_sequential_batches_equal_custom_batch_sampler(variant):
    g = gc.fixture()
    for split in gc.SPLITS:
        ds = _sorted_cpu_dataset(variant, split)
        sizes = g[f"{variant}_{split}_sizes"]
        assert max(gc.BATCH_SIZES) > np.bincount(sizes).max()
        for bs in gc.BATCH_SIZES:
            for drop_last in (False, True):
                want = g[f"{variant}_{split}_bs{bs}_dl{int(drop_last)}_counts"]
                firsts, counts = pkg.data.sequential_batches(len(sizes), bs, drop_last, g[f"{variant}_{split}_split_indices"])
                assert np.array_equal(counts, want), (split, bs, drop_last)
                assert np.array_equal(firsts, np.concatenate(([0], np.cumsum(want)[:-1]))[:len(want)])
                loader = ds.loader(bs, shuffle=False, drop_last=drop_last, sequential=True)
                assert len(loader) == int(g[f"{variant}_{split}_bs{bs}_dl{int(drop_last)}_len"]) == len(want)
                for f, c in zip(firsts, counts):                 # every batch holds one size
                    assert len(set(sizes[f:f + c].tolist())) == 1


def test_sequential_batches_at_their_edges():
    sb = pkg.data.sequential_batches
    assert [a.tolist() for a in sb(0, 4, False, [])] == [[], []]
    assert sb(7, 3, False, [])[1].tolist() == [3, 3, 1] and sb(7, 3, True, [])[1].tolist() == [3, 3]
    assert sb(7, 3, True, [2, 6])[1].tolist() == [2, 3, 1]                 # short batches at size changes stay; the open end goes
    assert sb(6, 3, True, [2, 6])[1].tolist() == [2, 3, 1]                 # num_pts ends on a size change: the batch is closed, and stays
    assert sb(5, 3, True, [2, 9])[1].tolist() == [2, 3] and sb(5, 3, True, [2, 9])[0].tolist() == [0, 2]


def test_sequential_loader_names_what_is_missing():
    ds = _sorted_cpu_dataset("h_all", "valid")
    with pytest.raises(ValueError, match="shuffle=False"):
        ds.loader(2, sequential=True)                                      # shuffle defaults to True
    with pytest.raises(ValueError, match="world == 1"):
        ds.loader(2, shuffle=False, world=2, rank=1, sequential=True)
    ds.sorted_by_size = False
    with pytest.raises(ValueError, match="size-sorted"):
        ds.loader(2, shuffle=False, sequential=True)
    assert len(ds.loader(2, shuffle=False)) == -(-len(ds) // 2)           # sequential=False: today's loader


def test_geom_splits_needs_the_gpu_and_a_well_formed_array():
    g = gc.fixture()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.MoleculeDataset.geom_splits(g["rows"], "cpu", permutation=g["h_all_perm"])
    with pytest.raises(ValueError, match="split must be"):
        pkg.MoleculeDataset.from_geom_file(g["rows"], "cpu", split="validation")
