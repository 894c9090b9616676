"""The device-resident data set without a GPU: include/gcdm_data.h <-> libgcdm_ops.so exports <-> native.DATA_SIGNATURES, the header as C99 linked
from plain C, argument refusal before any HIP call, MoleculeDataset's host side (filters, species, statistics, accounting) against the
reference's values in tests/golden/data_small.npz, the loader's index stream against torch's DistributedSampler, the trusted Graph constructor's
host checks, and the numpy statement of the sampling rule against the reference's expressions in torch."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from torch.utils.data import DistributedSampler

import data_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
HEADER = os.path.join(ROOT, "include", "gcdm_data.h")
TABLES = ("OPS_SIGNATURES", "MP_TRAIN_SIGNATURES", "MP_TILE_SIGNATURES", "GCP2_SIGNATURES", "OPTIM_SIGNATURES", "CLASSIFIER_SIGNATURES",
          "OBJECTIVE_SIGNATURES", "GRAD_BUCKET_SIGNATURES", "MATRIX_MODE_SIGNATURES")
Z = None


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(gcdm_data_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
    return out


def test_header_declares_exactly_the_signature_table():
    assert _declared() == {k: len(v) for k, v in native.DATA_SIGNATURES.items()}
    assert sorted(native.DATA_SIGNATURES) == ["gcdm_data_collate", "gcdm_data_prop_histogram", "gcdm_data_prop_sample", "gcdm_data_workspace_bytes"]
    for t in TABLES:
        assert not set(native.DATA_SIGNATURES) & set(getattr(native, t)), t
    assert not set(native.DATA_SIGNATURES) & set(native.EXPORTS)
    text = open(HEADER).read()
    for name in ("MAX_TYPES", "MAX_PROPS", "MAX_SIZES", "MAX_BINS", "FLAG_ABSENT_SIZE", "FLAG_ACCOUNT"):
        assert re.search(rf"#define GCDM_DATA_{name} {getattr(native, 'DATA_' + name)}\b", text), name
    # the two structures, field for field
    for struct, cls in (("gcdm_data_set", native.DataSet), ("gcdm_data_batch", native.DataBatch)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
        names = []
        for decl in (d.replace("const", " ").strip() for d in body.split(";")):
            if decl:
                names += [n.strip(" *") for n in decl.split(None, 1)[1].split(",")]
        assert names == [f[0] for f in cls._fields_], struct


def test_header_and_kernels_are_library_dependencies():
    assert HEADER in native.OPS_HEADERS
    assert os.path.join(ROOT, "bio-diffusion_amd", "csrc", "gcdm_ops.data.hip.h") in native.OPS_HEADERS


@pytest.fixture(scope="module")
def lib():
    path = native.OPS_LIB_PATH
    if not os.path.exists(path):
        pytest.skip("libgcdm_ops.so not built (run __graft_entry__.build())")
    stale = [d for d in native.OPS_SOURCES + native.OPS_HEADERS if os.path.getmtime(d) > os.path.getmtime(path)]
    if stale:
        pytest.skip(f"libgcdm_ops.so is older than {stale} (run __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    for name, sig in native.DATA_SIGNATURES.items():
        assert hasattr(lib, name), name
        getattr(lib, name).argtypes = sig
        getattr(lib, name).restype = native.DATA_RESTYPES.get(name, ctypes.c_int)
    return lib


def test_library_exports_the_entries_and_the_loader_binds_them(lib):
    assert lib.gcdm_data_workspace_bytes(0) >= 16 and lib.gcdm_data_workspace_bytes(1000) % 256 == 0
    assert lib.gcdm_data_workspace_bytes(1000) >= 1001 * 16 + 1000 * 12
    assert lib.gcdm_data_workspace_bytes(-1) == -1
    bound = native.load_ops()
    for name, sig in native.DATA_SIGNATURES.items():
        assert getattr(bound, name).argtypes == sig


def test_header_is_c99_and_links_from_plain_c(lib, tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "gcdm_data.h"\n'
                   "int main(void) {\n"
                   "  gcdm_data_set s; gcdm_data_batch o; int32_t flags = 0;\n"
                   "  memset(&s, 0, sizeof s); memset(&o, 0, sizeof o);\n"
                   "  long long w = (long long)gcdm_data_workspace_bytes(64);\n"
                   "  int empty = gcdm_data_collate(&s, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, &o, &flags, 0);\n"
                   "  int bad = gcdm_data_collate(&s, 0, 0, 0, 4, 0, 0, 0, 9, 27, 0, &o, &flags, 0);\n"
                   '  printf("%lld %d %d\\n", w, empty, bad);\n'
                   "  return !(w > 0 && empty == 0 && bad == -1 && GCDM_DATA_FLAG_ACCOUNT == 2);\n}\n")
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

    def collate(M=8, A=37, P=3, T=5, perm_len=8, first=0, B=4, pad_to=0, C=2, N=11, E=39, set_null=(), out_null=(), perm=X, ws=X, flags=X,
                ctx=X, no_set=False, no_out=False):
        s = native.DataSet(*[None if f[0] in set_null else 64 for f in native.DataSet._fields_[:7]], M, A, P, T)
        o = native.DataBatch(*[None if f[0] in out_null else 64 for f in native.DataBatch._fields_])
        return lib.gcdm_data_collate(None if no_set else ctypes.byref(s), perm, perm_len, first, B, pad_to, ctx, C, N, E, ws,
                                     None if no_out else ctypes.byref(o), flags, Z)

    cases = [collate(no_set=True), collate(no_out=True), collate(M=-1), collate(A=-1), collate(P=-1), collate(P=33), collate(T=17), collate(T=-1),
             collate(B=-1), collate(first=-1), collate(first=6, B=4), collate(perm_len=3), collate(pad_to=-1), collate(pad_to=1 << 15),
             collate(C=-1), collate(C=4), collate(N=-1), collate(E=-1), collate(N=1 << 31), collate(E=1 << 31), collate(pad_to=9, N=35),
             collate(B=0, N=1), collate(B=0, N=0, E=1), collate(M=0), collate(perm=Z), collate(ws=Z), collate(flags=Z), collate(ctx=Z)]
    cases += [collate(set_null=(f,)) for f in ("atom_ptr", "z", "pos", "props", "species", "norm", "index")]
    cases += [collate(out_null=(f,)) for f in [f[0] for f in native.DataBatch._fields_]]
    for k, status in enumerate(cases):
        assert status == -1, k
    assert collate(B=0, N=0, E=0, perm=Z, ws=Z, flags=Z) == 0               # nothing to do: no launch

    def hist(M=8, S=10, nb=7, ptrs=(X,) * 6):
        a, v, c, p, m, f = ptrs
        return lib.gcdm_data_prop_histogram(a, v, M, S, nb, c, p, m, f, Z)

    for k, status in enumerate([hist(M=-1), hist(S=-1), hist(S=2049), hist(nb=0), hist(nb=65537), hist(S=0, M=3)] +
                               [hist(ptrs=tuple(Z if i == j else X for i in range(6))) for j in range(6)]):
        assert status == -1, k
    assert hist(S=0, M=0, ptrs=(Z,) * 6) == 0

    def sample(B=4, P=2, S=10, nb=7, ptrs=(X,) * 8):
        c, pa, me, no, nn, u, out, f = ptrs
        return lib.gcdm_data_prop_sample(c, pa, me, no, nn, u, B, P, S, nb, out, f, Z)

    for k, status in enumerate([sample(B=-1), sample(P=-1), sample(P=33), sample(S=-1), sample(S=2049), sample(nb=0)] +
                               [sample(ptrs=tuple(Z if i == j else X for i in range(8))) for j in range(8)]):
        assert status == -1, k
    assert sample(B=0, ptrs=(Z,) * 8) == 0 and sample(P=0, ptrs=(Z,) * 8) == 0


# ---- MoleculeDataset's host side ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ds():
    return pkg.MoleculeDataset(dc.raw(), "cpu", conditioning=dc.CONDITIONING)


def test_filters_species_and_statistics_equal_the_reference(ds):
    g = dc.fixture()
    assert ds.M == 8 and len(ds) == 8 and ds.max_atoms == dc.A_MAX
    assert np.array_equal(ds.num_atoms_host, g["num_atoms"]) and list(ds.num_atoms_host) == [1, 2, 3, 5, 5, 9, 4, 8]
    assert torch.equal(ds.index, torch.tensor([100, 101, 102, 103, 105, 106, 107, 108]))          # the all-zero molecule (104) is gone
    assert np.array_equal(ds.included_species.numpy(), g["included_species"]) and ds.num_species == 5 and ds.max_charge == 9
    assert ds.property_keys == dc.PROPERTY_KEYS and ds.conditioning == dc.CONDITIONING
    assert sorted(ds.stats) == sorted(dc.PROPERTY_KEYS)
    for k in dc.PROPERTY_KEYS:
        assert np.array_equal(np.array([ds.stats[k][0].item(), ds.stats[k][1].item()], dtype=np.float32), g[f"stats_{k}"]), k
    mm = ds.mean_mad(dc.CONDITIONING)
    for p, k in enumerate(dc.CONDITIONING):
        assert np.array_equal(np.array([mm[k]["mean"].item(), mm[k]["mad"].item()], dtype=np.float32), g[f"norm_{k}"]), k
        assert np.array_equal(ds.norm[ds.property_keys.index(k)].numpy(), g[f"norm_{k}"]), k
    # the thermochemical energy is subtracted once, from U0 only
    raw = dc.raw()
    keep = raw["charges"].sum(-1) > 0
    assert torch.equal(ds.data["U0"], (raw["U0"] - raw["U0_thermo"])[keep]) and torch.equal(ds.data["alpha"], raw["alpha"][keep])
    assert torch.equal(ds.props[1], ds.data["U0"]) and ds.props.dtype == torch.float32
    # ragged layout: the present atoms of the padded arrays, in order
    assert ds.A == 37 and torch.equal(ds.atom_ptr, torch.tensor([0, 1, 3, 6, 11, 16, 25, 29, 37]))
    present = raw["charges"][keep] > 0
    assert torch.equal(ds.z.long(), raw["charges"][keep][present]) and torch.equal(ds.pos, raw["positions"][keep][present])
    assert ds.n_nodes_histogram() == {1: 1, 2: 1, 3: 1, 4: 1, 5: 2, 8: 1, 9: 1}
    hist = ds.atom_type_histogram()
    assert sum(hist.values()) == 37 and all(hist[t] == int((ds.z == s).sum()) for t, s in enumerate([1, 6, 7, 8, 9]))


def test_options_of_the_constructor():
    raw = dc.raw()
    d = pkg.MoleculeDataset(raw, "cpu", included_species=[6, 8], subtract_thermo=False, remove_zero_charge_molecules=False, num_pts=3)
    assert d.M == 9 and len(d) == 3 and d.num_species == 2 and d.max_charge == 8 and torch.equal(d.data["U0"], raw["U0"])
    assert d.num_atoms_host[4] == 0
    d = pkg.MoleculeDataset(raw, "cpu", filter_n_atoms=5)
    assert d.M == 2 and list(d.num_atoms_host) == [5, 5] and sorted(d.stats) == sorted(dc.PROPERTY_KEYS)
    assert np.array_equal(np.float32(d.stats["alpha"][0].item()), dc.fixture()["stats_alpha"][0])          # taken before the size filter
    assert pkg.MoleculeDataset(raw, "cpu", num_pts=100).num_pts == 8
    with pytest.raises(KeyError, match="gap"):
        pkg.MoleculeDataset(raw, "cpu", conditioning=["gap"])
    del raw["index"]
    assert torch.equal(pkg.MoleculeDataset(raw, "cpu").index, torch.tensor([0, 1, 2, 3, 5, 6, 7, 8]))


def test_interior_zero_charge_is_refused():
    raw = dc.raw()
    raw["charges"][5, 1] = 0
    with pytest.raises(ValueError, match="zero charge in front of a non-zero one"):
        pkg.MoleculeDataset(raw, "cpu")
    raw = dc.raw()
    raw["num_atoms"][2] = 4
    with pytest.raises(ValueError, match="num_atoms differs"):
        pkg.MoleculeDataset(raw, "cpu")


def test_from_npz_and_from_conformers(tmp_path, ds):
    path = tmp_path / "train.npz"
    np.savez_compressed(path, **{k: v.numpy() for k, v in dc.raw().items()})
    d = pkg.MoleculeDataset.from_npz(str(path), "cpu", conditioning=dc.CONDITIONING)
    for name in ("atom_ptr", "z", "pos", "props", "norm", "index", "species"):
        assert torch.equal(getattr(d, name), getattr(ds, name)), name
    confs = [torch.cat((ds.z[a:b].float().unsqueeze(-1), ds.pos[a:b]), dim=-1).numpy() for a, b in zip(ds.atom_ptr[:-1], ds.atom_ptr[1:])]
    c = pkg.MoleculeDataset.from_conformers(confs, "cpu", properties={"alpha": ds.data["alpha"]}, conditioning=["alpha"])
    assert c.max_atoms == 9 and c.property_keys == ["alpha"] and torch.equal(c.index, torch.arange(8))
    for name in ("atom_ptr", "z", "pos", "species"):
        assert torch.equal(getattr(c, name), getattr(ds, name)), name
    assert torch.equal(c.norm[0], ds.norm[0])
    with pytest.raises(ValueError, match="atomic number"):
        pkg.MoleculeDataset.from_conformers([np.zeros((2, 4))], "cpu")


def test_accounting_of_rows_and_edges_matches_the_fixture(ds):
    g = dc.fixture()
    for name in dc.BATCHES:
        perm, first = g[f"{name}_perm"], int(g[f"{name}_first"])
        B = len(g[f"{name}_index"])
        sizes = ds.num_atoms_host[perm[first:first + B]]
        N, E, full = pkg.data.batch_accounting(sizes, dc.A_MAX)
        assert (N, E) == (len(g[f"{name}_x"]), g[f"{name}_fc"].shape[1]) and full == bool(g[f"{name}_mask"].all())
        N, E, full = pkg.data.batch_accounting(sizes, 0)
        assert (N, E, full) == (int(g[f"{name}_mask"].sum()), g[f"{name}_fc_compact"].shape[1], True)
    assert pkg.data.batch_accounting(np.array([9, 9]), 9) == (18, 162, True)
    assert pkg.data.batch_accounting(np.array([], dtype=np.int64), 0) == (0, 0, True)


def test_batches_need_the_gpu(ds):
    it = iter(ds.loader(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(it)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.PropertiesDistribution(ds, ["alpha"])


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("shuffle", [True, False])
def test_loader_index_stream_equals_distributed_sampler(ds, world, shuffle):
    for seed, epoch in ((0, 0), (5, 0), (5, 3)):
        for rank in range(world):
            sampler = DistributedSampler(range(len(ds)), num_replicas=world, rank=rank, shuffle=shuffle, seed=seed)
            sampler.set_epoch(epoch)
            want = list(sampler)
            for drop_last in (False, True):
                loader = ds.loader(3, shuffle=shuffle, drop_last=drop_last, seed=seed, rank=rank, world=world)
                loader.set_epoch(epoch)
                iter(loader)
                assert loader.indices.tolist() == want, (world, rank, seed, epoch)
                n = len(want)
                assert len(loader) == (n // 3 if drop_last else -(-n // 3))
    # more ranks than molecules: the wrap-around repeats the stream
    assert pkg.data.distributed_indices(2, False, 0, 0, 4, 5).tolist() == list(DistributedSampler(range(2), num_replicas=5, rank=4, shuffle=False))
    with pytest.raises(ValueError):
        pkg.data.distributed_indices(8, True, 0, 0, 2, 2)
    with pytest.raises(ValueError, match="layout"):
        ds.loader(3, layout="dense")


def test_from_parts_checks_shapes_and_dtypes_on_the_host():
    ei = torch.zeros((2, 4), dtype=torch.int64)
    ok = dict(rowptr=torch.zeros(3, dtype=torch.int32), colperm=torch.zeros(4, dtype=torch.int64), colptr=torch.zeros(3, dtype=torch.int32))
    for bad in (dict(rowptr=torch.zeros(2, dtype=torch.int32)), dict(rowptr=torch.zeros(3, dtype=torch.int64)), dict(colperm=torch.zeros(5, dtype=torch.int64)),
                dict(colptr=torch.zeros(3, dtype=torch.float32))):
        with pytest.raises(ValueError, match="must be a contiguous"):
            pkg.ops.Graph.from_parts(ei, 2, **{**ok, **bad})
    with pytest.raises(ValueError, match="int64"):
        pkg.ops.Graph.from_parts(ei.to(torch.int32), 2, **ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.ops.Graph.from_parts(ei, 2, **ok)


def test_sampling_rule_in_numpy_equals_the_reference_expressions_in_torch():
    g = dc.fixture()
    rng = np.random.default_rng(3)
    norm = np.stack([g["norm_alpha"], g["norm_U0"]])
    for nb in (7, 1000):
        counts, params, members = g[f"hist{nb}_counts"], g[f"hist{nb}_params"], g[f"hist{nb}_members"]
        assert counts.sum(-1).tolist() == members.tolist()
        num_nodes = np.array([1, 5, 5, 9, 8, 4, 3, 2, 5, 6, 7, 12, 0], dtype=np.int64)          # 6, 7, 12 and 0 have no members
        u = rng.random((len(num_nodes), 2, 2), dtype=np.float32)
        u[2, :, 0] = np.float32(0.99999994)                                                       # the last rank
        u[1, :, 0] = 0.0
        got = dc.sample_reference(counts, params, members, norm, num_nodes, u)
        want = dc.draw_torch(counts, params, members, norm, num_nodes, u).numpy()
        assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True)
        assert np.isnan(got[-4:]).all() and np.isfinite(got[:-4]).all()
        # every rank of a group lands in a bin that holds a member, each bin as often as it has members
        for p in range(2):
            for n in (5, 9):
                count = int(members[p, n])
                uu = np.zeros((count, 2, 2), dtype=np.float32)
                uu[:, :, 0] = ((np.arange(count, dtype=np.float32) + np.float32(0.5)) / np.float32(count))[:, None]
                vals = dc.sample_reference(counts, params, members, norm, np.full(count, n), uu)[:, p]
                lefts = (np.flatnonzero(counts[p, n]).repeat(counts[p, n][counts[p, n] > 0]).astype(np.float32) / np.float32(nb)
                         * np.float32(params[p, n, 1] - params[p, n, 0]) + params[p, n, 0])
                assert np.array_equal(vals, (lefts - norm[p, 0]) / norm[p, 1])
