"""The sanitize / largest-fragment filters without a GPU: the definition (tests/molproc_ref.py) against networkx and scipy components on the
seeded corpus and against the largest fragment tests/molgraph_ref.py keys; the mutants of the definition, each caught by a case the GPU files
use; include/gcdm_molproc.h <-> libgcdm_ops.so exports <-> native.MOLPROC_SIGNATURES, the header as C99 linked from plain C, argument
refusal before any HIP call; the package's refusals on the host."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import molgraph_cases as mc
import molgraph_ref as ref
import molproc_cases as pc
import molproc_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
HEADER = os.path.join(ROOT, "include", "gcdm_molproc.h")
Z = None


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------

def test_components_equal_networkx_on_the_corpus():
    nx = pytest.importorskip("networkx")
    multi = 0
    for g in mc.corpus():
        G = nx.Graph()
        G.add_nodes_from(range(len(g.Z)))
        G.add_edges_from((int(i), int(j)) for i, j in zip(*np.nonzero(np.tril(g.orders, -1))))
        want = sorted((sorted(c) for c in nx.connected_components(G)), key=min)
        assert pr.components(ref.symmetric_orders(g.orders)) == want, g.label
        multi += len(want) > 1
    assert multi >= 50


def test_components_equal_scipy_on_the_corpus():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    for g in mc.corpus():
        k, labels = csgraph.connected_components(np.asarray(g.orders) > 0, directed=False)
        groups = [sorted(int(i) for i in np.flatnonzero(labels == c)) for c in range(k)]
        assert pr.components(ref.symmetric_orders(g.orders)) == sorted(groups, key=min), g.label


def test_largest_fragment_is_the_one_the_key_is_taken_of():
    """molgraph_ref.graph_key keys its largest fragment: the key of the whole molecule must be the key of the definition's largest fragment
    cut out as a molecule of its own.  The ties of tie_cases() have fragments of different keys, so the tie rule is held too."""
    ties = 0
    for g in list(mc.corpus()) + mc.tie_cases() + mc.cap_cases():
        frags = pr.components(ref.symmetric_orders(g.orders))
        big = pr.largest_fragment(frags)
        ties += sum(len(f) == len(big) for f in frags) > 1
        key, info = ref.graph_key(g.Z, g.orders)
        assert info[1:] == (len(frags), len(big), len(g.Z)), g.label
        assert ref.graph_key(g.Z[big], g.orders[np.ix_(big, big)])[0] == key, g.label
        assert frags == ref.components(ref.symmetric_orders(g.orders)), g.label
    assert ties >= 3                                                  # the three tie cases at the least
    first, second, inter = (pr.largest_fragment(pr.components(ref.symmetric_orders(g.orders))) for g in mc.tie_cases())
    assert first == [0, 1] and second == [0, 1] and inter == [0, 3]
    assert pr.largest_fragment([]) == []


def test_the_edge_cases_of_the_definition():
    zs, caps = mc.qm9_type_tables()
    empty = pr.process_one(np.zeros(0, np.int32), np.zeros((0, 0)), zs, caps, 3)
    assert empty == pr.One((1, 0, 0, 0), True, [], [], [])                      # n == 0 is kept as an empty molecule
    big = pr.process_one(np.zeros(193, np.int32), np.zeros((193, 193)), zs, caps, 0)
    assert big == pr.One((-1, 0, 0, 193), False, [], None, [])
    c = {x.label: x for x in pc.fragment_cases()}["interleaved: ring on the odd atoms, chain on the even"]
    one = pr.process_one(c.types, c.orders, zs, caps, pr.LARGEST_FRAG)
    assert one.atoms == [1, 3, 5, 7, 9, 11] and one.new_index[:4] == [-1, 0, -1, 1]
    assert one.bonds == [(1, 0, 1), (2, 1, 1), (3, 2, 1), (4, 3, 1), (5, 0, 1), (5, 4, 1)]
    same = pr.process_one(c.types, c.orders, zs, caps, 0)
    assert same.atoms == list(range(len(c.types))) and same.new_index == same.atoms
    assert same.bonds == [(int(i), int(j), int(c.orders[i, j])) for i, j in zip(*np.nonzero(np.tril(c.orders, -1)))]


@pytest.mark.parametrize("mutant", pr.MUTANTS)
def test_each_mutant_is_caught_by_a_gpu_case(mutant):
    """The mixed batch of the GPU files under the four flag combinations tells every mutant from the definition; the case named here is the
    one built for it."""
    zs, caps = mc.qm9_type_tables()
    cases = pc.mixed_batch()
    mols = [(c.types, c.orders) for c in cases]
    caught = set()
    for flags in range(4):
        want, got = pr.process_batch(mols, zs, caps, flags), pr.process_batch(mols, zs, caps, flags, mutant=mutant)
        if any(not np.array_equal(a, b) for a, b in zip(want, got)):
            for c in cases:
                one = [pr.process_one(c.types, c.orders, zs, caps, flags, mutant=mu) for mu in (None, mutant)]
                if one[0] != one[1]:
                    caught.add(c.label)
    built_for = {"tie_last": "tie: C-O then C-N", "sanitize_fragment_only": "C5 + OH3: O over its cap, outside the largest fragment",
                 "bonds_column_major": "decalin", "not_renumbered": "interleaved: ring on the odd atoms, chain on the even",
                 "dropped_as_empty": "CH5: C over its cap, in the largest fragment"}[mutant]
    assert built_for in caught, (mutant, sorted(caught)[:6])


def test_scan_batches_carry_across_every_tile_seam():
    """The scan cases: all three running sums are non-zero at every tile seam, molecules of 0-4 atoms, dropped ones among them."""
    zs, caps = mc.qm9_type_tables()
    T = native.MOLPROC_SCAN_TILE
    assert pc.SCAN_SIZES == (1, T - 1, T, T + 1, 2 * T + 3)
    for M in pc.SCAN_SIZES:
        mols = pc.scan_batch(M)
        assert len(mols) == M and {len(t) for t, _ in mols} <= {0, 1, 2, 3, 4}
        want = pr.process_batch(mols, zs, caps, 3)
        if M > 4:
            assert (want.counts[:, 2] == 0).any() and (want.counts[:, 2] == 1).any()
        run = np.cumsum(want.counts, 0)
        for seam in range(T, M, T):
            assert (run[seam - 1] > 0).all() and run[-1, 2] > run[seam - 1, 2], (M, seam)      # a carry in every scan, a molecule behind the seam


# ---- header, library, binding --------------------------------------------------------------------------------------------------------------------

def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
            for m in re.finditer(r"\b(gcdm_molproc_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_header_declares_exactly_the_signature_table():
    assert _declared() == {k: len(v) for k, v in native.MOLPROC_SIGNATURES.items()}
    assert sorted(native.MOLPROC_SIGNATURES) == ["gcdm_molproc_emit", "gcdm_molproc_select", "gcdm_molproc_workspace_bytes"]
    text = open(HEADER).read()
    for name, value in (("SANITIZE", native.MOLPROC_SANITIZE), ("LARGEST_FRAG", native.MOLPROC_LARGEST_FRAG), ("SCAN_TILE", native.MOLPROC_SCAN_TILE)):
        assert re.search(rf"#define GCDM_MOLPROC_{name}\s+{value}\b", text), name
    assert (native.MOLPROC_SANITIZE, native.MOLPROC_LARGEST_FRAG) == (pr.SANITIZE, pr.LARGEST_FRAG)
    assert HEADER in native.OPS_HEADERS
    assert os.path.join(ROOT, "bio-diffusion_amd", "csrc", "gcdm_ops.molproc.hip.h") in native.OPS_HEADERS
    assert '#include "gcdm_ops.molproc.hip.h"' in open(native.OPS_SOURCES[0]).read()


@pytest.fixture(scope="module")
def lib():
    path = native.OPS_LIB_PATH
    if not os.path.exists(path):
        pytest.skip("libgcdm_ops.so not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    for name, sig in native.MOLPROC_SIGNATURES.items():
        assert hasattr(lib, name), name
        getattr(lib, name).argtypes = sig
        getattr(lib, name).restype = native.MOLPROC_RESTYPES.get(name, ctypes.c_int)
    return lib


def test_library_exports_the_entries_and_the_loader_binds_them(lib):
    bound = native.load_ops()
    for name, sig in native.MOLPROC_SIGNATURES.items():
        assert getattr(bound, name).argtypes == sig
    T = native.MOLPROC_SCAN_TILE
    for M, tiles in ((0, 0), (1, 1), (T, 1), (T + 1, 2), (10000, -(-10000 // T))):
        assert lib.gcdm_molproc_workspace_bytes(M) == 24 * (M + 2 * tiles)
    assert lib.gcdm_molproc_workspace_bytes(-1) < 0


def test_header_is_c99_and_links_from_plain_c(lib, tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "gcdm_molproc.h"\n'
                   "int main(void) {\n"
                   "  GcdmMolGraphTables tb;\n"
                   "  int64_t totals[3];\n"
                   "  memset(&tb, 0, sizeof tb);\n"
                   "  tb.bonds.num_types = 5;\n"
                   "  int flags = gcdm_molproc_select(&tb, 0, 3, 0, 0, 0, 0, 0, 4, 0, 0, 0, 0, totals, 0, 0);\n"
                   "  int null_ = gcdm_molproc_select(&tb, 0, 3, 0, 0, 4, 0, 0, 3, 0, 0, 0, 0, totals, 0, 0);\n"
                   "  int stride = gcdm_molproc_select(&tb, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, totals, 0, 0);\n"
                   "  int emit = gcdm_molproc_emit(&tb, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, totals, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);\n"
                   "  long long ws = (long long)gcdm_molproc_workspace_bytes(GCDM_MOLPROC_SCAN_TILE + 1);\n"
                   '  printf("%d %d %d %d %lld\\n", flags, null_, stride, emit, ws);\n'
                   "  return !(flags == -1 && null_ == -1 && stride == -1 && emit == -1 && ws == 24 * (GCDM_MOLPROC_SCAN_TILE + 1 + 4));\n}\n")
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
    bad = native.GcdmMolGraphTables()
    bad.bonds.num_types = 17

    def select(tables=tb, x=X, stride=3, types=X, off=X, M=4, poff=Z, orders=Z, flags=3, outs=(X,) * 6):
        info, keep, new_index, counts, totals, ws = outs
        return lib.gcdm_molproc_select(tables, x, stride, types, off, M, poff, orders, flags, info, keep, new_index, counts, totals, ws, Z)

    def emit(tables=tb, x=X, stride=3, types=X, charges=Z, off=X, M=4, poff=Z, orders=Z, ins=(X,) * 5, charges_out=Z, outs=(X,) * 7):
        keep, new_index, counts, totals, ws = ins
        pos, types_out, src_atom, src_mol, mol_off, bonds, bond_off = outs
        return lib.gcdm_molproc_emit(tables, x, stride, types, charges, off, M, poff, orders, keep, new_index, counts, totals, ws, pos, types_out,
                                     charges_out, src_atom, src_mol, mol_off, bonds, bond_off, Z)

    cases = [select(tables=None), select(tables=bad), select(M=-1), select(stride=2), select(flags=4), select(flags=-1), select(flags=8 | 1),
             select(x=Z), select(types=Z), select(off=Z), select(orders=X, poff=Z), select(M=0, outs=(Z,) * 6)]
    cases += [select(outs=tuple(Z if i == j else X for i in range(6))) for j in range(6)]
    cases += [emit(tables=None), emit(tables=bad), emit(M=-1), emit(stride=2), emit(x=Z), emit(types=Z), emit(off=Z), emit(orders=X, poff=Z),
              emit(charges=X), emit(charges_out=X)]
    cases += [emit(ins=tuple(Z if i == j else X for i in range(5))) for j in range(5)]
    cases += [emit(outs=tuple(Z if i == j else X for i in range(7))) for j in range(7)]
    cases += [emit(M=0, ins=(Z,) * 5), emit(M=0, outs=(X, X, X, X, Z, X, X)), emit(M=0, outs=(X, X, X, X, X, X, Z))]
    for k, status in enumerate(cases):
        assert status == -1, k


def test_the_package_refuses_on_the_host():
    info = pkg.dataset_info("qm9")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.process_molecules(torch.zeros(3, 3), torch.zeros(3, dtype=torch.int64), torch.tensor([3]), info)
    assert pkg.postprocess.process_molecules is pkg.process_molecules and pkg.ProcessedBatch is pkg.postprocess.ProcessedBatch
