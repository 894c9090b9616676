"""Validity, fragments and graph keys without a GPU: include/gcdm_molgraph.h <-> libgcdm_ops.so exports <-> native.MOLGRAPH_SIGNATURES, the
header as C99 linked from plain C, argument refusal before any HIP call; the definition (tests/molgraph_ref.py) against networkx isomorphism on
the seeded corpus, no pair excluded; the bookkeeping of GraphMolecularMetrics.compute against the reference's formulas; and the mutants of the
definition, each caught by a molecule the GPU files use."""
import ctypes
import importlib
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import molgraph_cases as mc
import molgraph_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
HEADER = os.path.join(ROOT, "include", "gcdm_molgraph.h")
TABLES = ("OPS_SIGNATURES", "MP_TRAIN_SIGNATURES", "MP_TILE_SIGNATURES", "GCP2_SIGNATURES", "OPTIM_SIGNATURES", "CLASSIFIER_SIGNATURES",
          "OBJECTIVE_SIGNATURES", "GRAD_BUCKET_SIGNATURES", "MATRIX_MODE_SIGNATURES", "DATA_SIGNATURES", "GEOM_SIGNATURES")
Z = None


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(gcdm_molgraph_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
    return out


def test_header_declares_exactly_the_signature_table():
    assert _declared() == {k: len(v) for k, v in native.MOLGRAPH_SIGNATURES.items()}
    assert sorted(native.MOLGRAPH_SIGNATURES) == ["gcdm_molgraph_keys", "gcdm_molgraph_keys_from_orders"]
    for t in TABLES:
        assert not set(native.MOLGRAPH_SIGNATURES) & set(getattr(native, t)), t
    assert not set(native.MOLGRAPH_SIGNATURES) & set(native.EXPORTS)
    assert not set(native.MOLGRAPH_SIGNATURES) & set(native.OPS_EXPORTS)
    text = open(HEADER).read()
    assert re.search(rf"#define GCDM_MOLGRAPH_MAX_ATOMS {native.MOLGRAPH_MAX_ATOMS}\b", text) and native.MOLGRAPH_MAX_ATOMS == ref.MAX_ATOMS
    assert re.search(rf"#define GCDM_MOLGRAPH_ROUNDS\s+{native.MOLGRAPH_ROUNDS}\b", text) and native.MOLGRAPH_ROUNDS == ref.ROUNDS
    for k, (a, b) in enumerate(zip(native.MOLGRAPH_K, (ref.K1, ref.K2, ref.K3, ref.K4, ref.K5))):
        assert a == b and a % 2 == 1 and re.search(rf"#define GCDM_MOLGRAPH_K{k + 1} 0x{a:016X}ULL", text), k


def test_tables_struct_has_the_layout_of_the_header(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gcdm_molgraph.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(GcdmMolGraphTables), offsetof(GcdmMolGraphTables, bonds),\n'
                   "  offsetof(GcdmMolGraphTables, atomic_number), offsetof(GcdmMolGraphTables, valence_cap),\n"
                   "  offsetof(GcdmMolGraphTables, types_are_atomic_numbers)); return 0; }\n")
    exe = tmp_path / "s"
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], text=True,
                       capture_output=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], text=True, capture_output=True).stdout.split()]
    T = native.GcdmMolGraphTables
    assert got == [ctypes.sizeof(T), T.bonds.offset, T.atomic_number.offset, T.valence_cap.offset, T.types_are_atomic_numbers.offset]
    assert ctypes.sizeof(T) + 9 * 8 <= 4096                           # the struct travels in the kernel arguments


def test_header_and_kernels_are_library_dependencies():
    assert HEADER in native.OPS_HEADERS
    assert os.path.join(ROOT, "bio-diffusion_amd", "csrc", "gcdm_ops.molgraph.hip.h") in native.OPS_HEADERS
    assert '#include "gcdm_ops.molgraph.hip.h"' in open(native.OPS_SOURCES[0]).read()


@pytest.fixture(scope="module")
def lib():
    path = native.OPS_LIB_PATH
    if not os.path.exists(path):
        pytest.skip("libgcdm_ops.so not built (run __graft_entry__.build())")
    stale = [d for d in native.OPS_SOURCES + native.OPS_HEADERS if os.path.getmtime(d) > os.path.getmtime(path)]
    if stale:
        pytest.skip(f"libgcdm_ops.so is older than {stale} (run __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    for name, sig in native.MOLGRAPH_SIGNATURES.items():
        assert hasattr(lib, name), name
        getattr(lib, name).argtypes = sig
        getattr(lib, name).restype = native.MOLGRAPH_RESTYPES.get(name, ctypes.c_int)
    return lib


def test_library_exports_the_entries_and_the_loader_binds_them(lib):
    bound = native.load_ops()
    for name, sig in native.MOLGRAPH_SIGNATURES.items():
        assert getattr(bound, name).argtypes == sig


def test_header_is_c99_and_links_from_plain_c(lib, tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "gcdm_molgraph.h"\n'
                   "int main(void) {\n"
                   "  GcdmMolGraphTables tb;\n"
                   "  memset(&tb, 0, sizeof tb);\n"
                   "  tb.bonds.num_types = 5;\n"
                   "  int empty = gcdm_molgraph_keys(&tb, 0, 3, 0, 0, 0, 0, 0, 0);\n"
                   "  int null_ = gcdm_molgraph_keys(&tb, 0, 3, 0, 0, 4, 0, 0, 0);\n"
                   "  int stride = gcdm_molgraph_keys(&tb, 0, 2, 0, 0, 0, 0, 0, 0);\n"
                   "  int empty2 = gcdm_molgraph_keys_from_orders(&tb, 0, 0, 0, 0, 0, 0, 0, 0);\n"
                   "  tb.bonds.num_types = 17;\n"
                   "  int types = gcdm_molgraph_keys_from_orders(&tb, 0, 0, 0, 0, 0, 0, 0, 0);\n"
                   '  printf("%d %d %d %d %d\\n", empty, null_, stride, empty2, types);\n'
                   "  return !(empty == 0 && null_ == -1 && stride == -1 && empty2 == 0 && types == -1 && GCDM_MOLGRAPH_MAX_ATOMS == 192);\n}\n")
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
    tb = native.GcdmMolGraphTables()
    tb.bonds.num_types = 5

    def keys(tables=tb, stride=3, M=4, ptrs=(X,) * 5):
        x, types, off, k, info = ptrs
        return lib.gcdm_molgraph_keys(tables, x, stride, types, off, M, k, info, Z)

    def from_orders(tables=tb, M=4, ptrs=(X,) * 6):
        types, off, poff, orders, k, info = ptrs
        return lib.gcdm_molgraph_keys_from_orders(tables, types, off, M, poff, orders, k, info, Z)

    bad_tables = []
    for T in (0, -1, 17):
        t = native.GcdmMolGraphTables()
        t.bonds.num_types = T
        bad_tables.append(t)
    cases = [keys(tables=None), keys(stride=2), keys(stride=0), keys(stride=-3), keys(M=-1)] + [keys(tables=t) for t in bad_tables]
    cases += [keys(ptrs=tuple(Z if i == j else X for i in range(5))) for j in range(5)]
    cases += [from_orders(tables=None), from_orders(M=-1)] + [from_orders(tables=t) for t in bad_tables]
    cases += [from_orders(ptrs=tuple(Z if i == j else X for i in range(6))) for j in range(6)]
    for k, status in enumerate(cases):
        assert status == -1, k
    assert keys(M=0, ptrs=(Z,) * 5) == 0 and from_orders(M=0, ptrs=(Z,) * 6) == 0          # nothing to do: no launch
    assert keys(M=0, stride=2, ptrs=(Z,) * 5) == -1 and from_orders(M=0, tables=bad_tables[2], ptrs=(Z,) * 6) == -1


def test_the_package_refuses_cpu_tensors():
    info = pkg.dataset_info("qm9")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.molecule_graph_keys(torch.zeros(3, 3), torch.zeros(3, dtype=torch.int64), torch.tensor([3]), info)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.MoleculeDataset.from_conformers([np.array([[6, 0, 0, 0], [1, 1, 0, 0]], np.float32)], "cpu").graph_keys(info)


def test_default_caps_are_the_largest_allowed_valence():
    for ds in ("qm9", "geom"):
        info = pkg.dataset_info(ds)
        tb = pkg.metrics.graph_tables(info)
        zs, caps = mc.ds_type_tables(ds)
        T = len(info["atom_decoder"])
        assert list(tb.atomic_number[:T]) == zs and list(tb.valence_cap[:T]) == caps
        assert tb.bonds.limit_bonds_to_one == int(ds == "geom") and tb.types_are_atomic_numbers == 0
        assert pkg.metrics.ATOMIC_NUMBERS == ref.SYMBOL_Z
    assert dict(zip(pkg.dataset_info("qm9")["atom_decoder"], mc.ds_type_tables("qm9")[1])) == {"H": 1, "C": 4, "N": 3, "O": 2, "F": 1}
    info = pkg.dataset_info("geom")
    tb = pkg.metrics.graph_tables(info, {"S": 6, "P": -1}, limit_bonds_to_one=False, types_are_atomic_numbers=True)
    dec = info["atom_decoder"]
    assert tb.valence_cap[dec.index("S")] == 6 and tb.valence_cap[dec.index("P")] == -1 and tb.valence_cap[dec.index("C")] == 4
    assert tb.bonds.limit_bonds_to_one == 0 and tb.types_are_atomic_numbers == 1
    with pytest.raises(ValueError, match="does not hold"):
        pkg.metrics.graph_tables(pkg.dataset_info("qm9"), {"S": 6})


# ---- the definition against networkx ----------------------------------------------------------------------------------------------------------

def _nx_graph(g):
    nx = pytest.importorskip("networkx")
    G = nx.Graph()
    for i, z in enumerate(g.Z):
        G.add_node(i, Z=int(z))
    for i, j in zip(*np.nonzero(np.tril(g.orders, -1))):
        G.add_edge(int(i), int(j), o=int(g.orders[i, j]))
    return G


@pytest.fixture(scope="module")
def corpus_results():
    nx = pytest.importorskip("networkx")
    out = []
    for g in mc.corpus():
        G = _nx_graph(g)
        comps = sorted(nx.connected_components(G), key=min)
        out.append((g, G, comps, ref.graph_key(g.Z, g.orders, mc.caps_of(g.Z))))
    return out


def test_corpus_is_what_the_issue_asks_for():
    C = mc.corpus()
    assert len(C) >= 500 and {len(g.Z) for g in C} == set(range(1, 30))
    assert sum(g.label.endswith(" permuted") for g in C) >= 200
    labels = {g.label for g in C}
    assert {"decalin", "bicyclopentyl", "C-C=C-O", "C-C-C-O", "ring C5N", "ring C5O"} <= labels
    a, b = mc.order_pair()
    assert np.array_equal(a.Z, b.Z) and (a.orders != b.orders).sum() == 2
    a, b = mc.element_pair()
    assert np.array_equal(a.orders, b.orders) and (a.Z != b.Z).sum() == 1


def test_fragments_equal_networkx_components(corpus_results):
    multi = 0
    for g, G, comps, (key, info) in corpus_results:
        assert info[1] == len(comps) and info[2] == max(len(c) for c in comps) and info[3] == len(g.Z), g.label
        multi += len(comps) > 1
        over = any(int(g.orders[i].sum()) > mc.CAPS[int(g.Z[i])] for i in range(len(g.Z)))
        assert info[0] == int(not over), g.label
    assert multi >= 50
    assert 20 <= sum(r[3][1][0] == 0 for r in corpus_results) <= len(corpus_results) - 100           # valid and invalid molecules both occur


def test_key_equality_is_isomorphism_of_the_largest_fragments(corpus_results):
    """Every pair of the corpus whose largest fragments have equal size and composition, none excluded: equal keys <=> isomorphic (elements and
    bond orders matched).  Every other pair must differ in its key."""
    nx = pytest.importorskip("networkx")
    largest = []
    for g, G, comps, _ in corpus_results:
        best = max(comps, key=len)                                   # the first of the largest in order of lowest atom
        largest.append((G.subgraph(best), tuple(sorted(int(g.Z[i]) for i in best))))
    candidates = isomorphic = 0
    for a, b in itertools.combinations(range(len(largest)), 2):
        same_key = corpus_results[a][3][0] == corpus_results[b][3][0]
        if largest[a][1] != largest[b][1]:
            assert not same_key, (corpus_results[a][0].label, corpus_results[b][0].label)
            continue
        candidates += 1
        iso = nx.is_isomorphic(largest[a][0], largest[b][0], node_match=lambda u, v: u["Z"] == v["Z"], edge_match=lambda u, v: u["o"] == v["o"])
        isomorphic += iso
        assert iso == same_key, (corpus_results[a][0].label, corpus_results[b][0].label, iso)
    assert candidates >= 400 and isomorphic >= 200 and candidates - isomorphic >= 60, (candidates, isomorphic)


def test_hard_pairs_and_the_tie_rule():
    for a, b in mc.hard_pairs():
        assert ref.graph_key(a.Z, a.orders)[0] != ref.graph_key(b.Z, b.orders)[0], (a.label, b.label)
    a, b = mc.hard_pairs()[0]
    assert ref.graph_key(a.Z, a.orders, mutant="no_distance")[0] == ref.graph_key(b.Z, b.orders, mutant="no_distance")[0]      # plain refinement cannot
    co = ref.graph_key([6, 8], [[0, 0], [1, 0]])[0]
    cn = ref.graph_key([6, 7], [[0, 0], [1, 0]])[0]
    first, second, inter = (ref.graph_key(g.Z, g.orders) for g in mc.tie_cases())
    assert co != cn and first == (co, (1, 2, 2, 4)) and second == (cn, (1, 2, 2, 4)) and inter == (cn, (1, 2, 2, 4))
    assert ref.graph_key([], np.zeros((0, 0))) == (0, (1, 0, 0, 0))
    assert ref.graph_key([6] * 193, np.zeros((193, 193))) == (0, (-1, 0, 0, 193))


# ---- bookkeeping ------------------------------------------------------------------------------------------------------------------------------

def _compute(keys, valid, dataset_keys, chunks=1):
    m = pkg.GraphMolecularMetrics(pkg.dataset_info("qm9"), dataset_keys=None if dataset_keys is None else torch.tensor(dataset_keys, dtype=torch.int64))
    keys, valid = torch.tensor(keys, dtype=torch.int64), torch.tensor(valid, dtype=torch.int32)
    for k, v in zip(torch.chunk(keys, chunks), torch.chunk(valid, chunks)):
        info = torch.zeros((len(k), 4), dtype=torch.int32)
        info[:, 0] = v
        m.update(k, info)
    return m.compute()


BOOKKEEPING = {
    "nothing valid": ([5, 5, 7], [0, 0, 0], [5]),
    "no dataset keys": ([5, 5, 7, -3], [1, 1, 1, 0], None),
    "empty dataset keys": ([5, 5, 7, -3], [1, 1, 1, 0], []),
    "all duplicates": ([9, 9, 9, 9], [1, 1, 1, 1], [1, 9]),
    "an invalid duplicate of a valid key": ([4, 4, 8, -2 ** 63, 2 ** 63 - 1], [1, 0, 1, 1, 1], [8, 8, 2 ** 63 - 1, 11]),
    "all novel": ([1, 2, 3], [1, 1, 1], [0, 4]),
    "too large a molecule is not valid": ([0, 6], [-1, 1], [6]),
}


@pytest.mark.parametrize("name", list(BOOKKEEPING))
def test_compute_is_the_reference_bookkeeping(name):
    keys, valid, dataset_keys = BOOKKEEPING[name]
    want = ref.reference_metrics(keys, valid, dataset_keys)
    for chunks in (1, 3):
        got = _compute(keys, valid, dataset_keys, chunks)
        assert got == want and all(isinstance(v, float) for v in got), (name, chunks, got, want)
    assert {"nothing valid": [0.0, 0.0, 0.0], "no dataset keys": [0.75, 2 / 3, 0.0], "all duplicates": [1.0, 0.25, 0.0],
            "an invalid duplicate of a valid key": [0.8, 1.0, 0.5]}.get(name, want) == want


def test_compute_refuses_nothing():
    m = pkg.GraphMolecularMetrics(pkg.dataset_info("qm9"))
    with pytest.raises(ValueError):
        m.compute()
    with pytest.raises(ValueError):
        m.update(torch.zeros(3, dtype=torch.int64), torch.zeros((3, 3), dtype=torch.int32))


# ---- mutants ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_each_mutant_is_caught_by_a_gpu_case(mutant):
    """The molecules of the from-orders batch of tests/test_molgraph_cabi_gpu.py tell every mutant from the definition; the cases named here
    are the ones built for it."""
    want, got = mc.order_expected(), mc.order_expected(mutant=mutant)
    caught = {c.label for c, w, g in zip(mc.order_cases(), want, got) if w != g}
    assert caught, mutant
    built_for = {"caps_on_fragment": "C5 + OH3: O over its cap, outside the largest fragment", "lt_at_cap": "CH4: C at its cap",
                 "tie_last": "tie: C-O then C-N", "no_order": "C-C=C-O", "no_distance": "decalin", "upper_triangle": "decalin, upper triangle scrambled",
                 "one_round_fewer": "bicyclopentyl"}[mutant]
    assert built_for in caught, (mutant, sorted(caught)[:6])
    if mutant in ("caps_on_fragment", "lt_at_cap"):                  # these change the verdict and leave the key alone
        assert all(w[0] == g[0] for w, g in zip(want, got))
    if mutant == "no_distance":                                       # without the distance term the hard pair collides
        keys = {c.label: g[0] for c, g in zip(mc.order_cases(), got)}
        assert keys["decalin"] == keys["bicyclopentyl"]
