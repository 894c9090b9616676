"""The fused message layer's C ABI and switch, without a GPU: include/gcdm_mp_train.h <-> libgcdm_ops.so exports <-> native.MP_TRAIN_SIGNATURES,
the header as C99, argument refusal before any HIP call, the workspace sizes, and GCPNetDynamics.set_message_path on CPU-built networks.

The argument cases call the library with null pointers; as in test_ops_cabi_cpu.py the `lib` fixture runs them only on a library at least as
new as its sources that refuses a bad argument in a launch-free probe first."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest
import torch

import mp_train_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
HEADER = os.path.join(ROOT, "include", "gcdm_mp_train.h")
Z = None


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(gcdm_mp_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip()])
    return out


def test_header_declares_exactly_the_signature_table():
    decl = _declared()
    assert decl == {k: len(v) for k, v in native.MP_TRAIN_SIGNATURES.items()}
    assert not set(decl) & set(native.OPS_EXPORTS)


def test_library_exports_every_declared_entry():
    if not os.path.exists(native.OPS_LIB_PATH):
        pytest.skip("libgcdm_ops.so not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(native.OPS_LIB_PATH)
    for name in native.MP_TRAIN_SIGNATURES:
        assert hasattr(lib, name), name


def test_header_is_c99():
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = '#include "gcdm_mp_train.h"\nint main(void) { return (int)gcdm_mp_workspace_bytes(0, 0, 0, 64, 16) != 0; }\n'
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.dirname(HEADER), "-x", "c", "-"],
                       input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr


@pytest.fixture(scope="module")
def lib():
    path = native.OPS_LIB_PATH
    if not os.path.exists(path):
        pytest.skip("libgcdm_ops.so not built (run __graft_entry__.build())")
    stale = [d for d in native.OPS_SOURCES + native.OPS_HEADERS if os.path.getmtime(d) > os.path.getmtime(path)]
    if stale:
        pytest.skip(f"libgcdm_ops.so is older than {stale} (run __graft_entry__.build()): it may lack the argument checks under test")
    lib = ctypes.CDLL(path)
    for name, sig in native.MP_TRAIN_SIGNATURES.items():
        getattr(lib, name).argtypes = sig
        getattr(lib, name).restype = native.MP_TRAIN_RESTYPES.get(name, ctypes.c_int)
    # launch-free probe: bad edge dims with no work at all must be refused
    status = lib.gcdm_mp_fwd(Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, 0, 0, 0, 65, 16, Z)
    if status != -1:
        pytest.fail(f"{path}: gcdm_mp_fwd accepts SE = 65 (status {status}); the null-pointer cases would not be safe")
    return lib


def _weights(ok=True):
    arr = (ctypes.c_void_p * 30)(*([8] * 30))          # never dereferenced on the device: every case below is refused or empty
    if not ok:
        arr[17] = None
    return arr


def _fwd(N, E, SE=64, VE=16, tape=1, ptr=Z, w=Z):
    return (ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, Z, w, ptr, ptr, tape, N, E, SE, VE, Z)


def _bwd(N, E, SE=64, VE=16, ptr=Z, w=Z):
    return (ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, Z, w, ptr, ptr, ptr, ptr, ptr, ptr, ptr, N, E, SE, VE, Z)


def test_every_entry_refuses_bad_arguments_and_skips_empty_work(lib):
    cases = []
    for name, mk in (("gcdm_mp_fwd", _fwd), ("gcdm_mp_bwd", _bwd)):
        cases += [(name, mk(-1, 4), -1), (name, mk(4, -1), -1), (name, mk(0, 4), -1), (name, mk(4, 16, SE=32, VE=16), -1),
                  (name, mk(4, 16, SE=16, VE=16), -1), (name, mk(4, 16), -1), (name, mk(4, 16, w=_weights(False)), -1),
                  (name, mk(0, 0), 0), (name, mk(4, 0), 0), (name, mk(5, 0, SE=16, VE=8), 0), (name, mk(0, 0, SE=1, VE=1), -1)]
    cases += [("gcdm_mp_fwd", _fwd(4, 16, tape=2), -1), ("gcdm_mp_fwd", _fwd(4, 16, tape=-1), -1), ("gcdm_mp_fwd", _fwd(4, 0, tape=3), -1)]
    for which in (-1, 4):
        cases.append(("gcdm_mp_workspace_bytes", (which, 4, 16, 64, 16), -1))
    cases += [("gcdm_mp_workspace_bytes", (0, -1, 16, 64, 16), -1), ("gcdm_mp_workspace_bytes", (1, 4, -2, 64, 16), -1),
              ("gcdm_mp_workspace_bytes", (2, 4, 16, 64, 8), -1), ("gcdm_mp_workspace_bytes", (3, 0, 1, 16, 8), -1)]
    bad = [(n, a, want, getattr(lib, n)(*a)) for n, a, want in cases]
    assert [b for b in bad if b[2] != b[3]] == []


def _a4(n):
    return (n + 63) // 64 * 64


def _sizes(N, E, SE, VE):
    """The workspace formula of csrc/gcdm_ops.mp_train.hip.h restated (floats, every buffer rounded up to 64)."""
    S, V, H, X = 256, 32, 8, 256 + 8 + 9
    vin0 = 2 * V + VE
    h0 = vin0 // 4
    k0 = SE + h0 + 9
    common = _a4(2 * S * S) + _a4(S * k0) + _a4(N * 2 * S) + _a4(E * k0)
    tail = _a4(E * S) + _a4(E) + _a4(E * S) + _a4(E * 3 * V)          # silu buffer, attention, final scalar and vector states
    fwd0 = common + _a4(E * X) + _a4(E * 3 * V) + _a4(E * 3 * h0) + _a4(E * S) + _a4(E * V) + tail
    fwd1 = (common + _a4(E * 3 * vin0) + 3 * _a4(E * X) + 3 * _a4(E * 3 * V) + _a4(E * 3 * h0) + 3 * _a4(E * 3 * H) + 4 * _a4(E * S)
            + 4 * _a4(E * V) + tail)
    wsz = []
    for k in range(4):
        hk, vin, kin = (h0, vin0, 2 * S + k0) if k == 0 else (H, V, X)
        wsz += [hk * vin, 3 * vin, S * kin, S, V * hk, V * S, V]
    wsz += [S, 1]
    wt = sum(wsz)
    bwd = (_a4(1) + _a4(E * S) + _a4(E * 3 * V) + _a4(E * S) + _a4(E * max(X, k0))
           + sum(_a4(E * S) * 2 + _a4(E * V) + _a4(E * 3 * V) + _a4(E * 3 * (h0 if k == 0 else H)) + _a4(E * 9) for k in range(4))
           + _a4(E) + 2 * _a4(E * 3 * V) + _a4(N * 2 * S) + _a4(16 * wt))
    return [4 * fwd0, 4 * fwd1, 4 * bwd, 4 * wt]


@pytest.mark.parametrize("N,E,SE,VE", [(1, 1, 64, 16), (40, 313, 64, 16), (1216, 23104, 64, 16), (29, 451, 16, 8), (0, 0, 16, 8)])
def test_workspace_query_matches_the_formula(lib, N, E, SE, VE):
    got = [lib.gcdm_mp_workspace_bytes(w, N, E, SE, VE) for w in range(4)]
    assert got == _sizes(N, E, SE, VE)
    assert got[1] > got[0] or E == 0


def _net(**over):
    cfgs = pkg.default_cfgs("qm9")
    for group, kv in over.items():
        for k, v in kv.items():
            cfgs[group][k] = v
    return pkg.GCPNetDynamics(**cfgs)


def test_default_message_path_is_operators_and_production_config_accepts_fused():
    net = _net()
    assert net.message_path == "operators"
    assert all(l.interaction.path == "operators" for l in net.interaction_layers)
    net.set_message_path("fused")
    assert net.message_path == "fused"
    net.set_message_path("operators")
    assert net.message_path == "operators"
    with pytest.raises(ValueError):
        net.set_message_path("modules")
    g = pkg.GCPNetDynamics(**pkg.default_cfgs("geom"))
    g.set_message_path("fused")
    assert g.message_path == "fused"


@pytest.mark.parametrize("over,reason", [
    (dict(module_cfg=dict(frame_gate=True)), "vector_gate / frame_gate"),
    (dict(module_cfg=dict(selected_GCP="GCP")), "GCP2"),
    (dict(module_cfg=dict(bottleneck=2, default_bottleneck=2)), "bottleneck"),
    (dict(model_cfg=dict(h_hidden_dim=128)), "hidden sizes"),
    (dict(model_cfg=dict(e_hidden_dim=32, xi_hidden_dim=16)), "hidden sizes"),
    (dict(module_cfg=dict(nonlinearities=["relu", "silu"])), "silu"),
])
def test_set_message_path_fused_refuses_configurations_outside_the_kernels(over, reason):
    net = _net(**over)
    with pytest.raises(NotImplementedError, match=re.escape(reason)):
        net.set_message_path("fused")
    assert net.message_path == "operators"


def test_random_sparse_has_the_properties_it_is_there_for():
    """The graph of tests/test_mp_train_cabi_gpu.py that separates colptr from rowptr: a change of seed must not quietly lose what it is for."""
    g = mp_train_ref.random_sparse()
    outdeg, indeg = torch.bincount(g.row, minlength=g.N), torch.bincount(g.col, minlength=g.N)
    assert g.N == 300 and 1900 <= g.E <= 2100
    assert bool((g.row[1:] >= g.row[:-1]).all())
    assert int(((outdeg == 0) & (indeg > 0)).sum()) >= 10 and int(((indeg == 0) & (outdeg > 0)).sum()) >= 10
    assert outdeg[0] == 0 and indeg[0] == 0 and outdeg[-1] == 0 and indeg[-1] == 0
    assert (g.row * g.N + g.col).unique().numel() < g.E      # an edge appears twice
    assert bool((g.row == g.col).any())                      # a self-loop
    assert not torch.equal(g.rowptr, g.colptr)
