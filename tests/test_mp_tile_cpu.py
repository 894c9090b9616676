"""The tiled message layer's C ABI and switch, without a GPU: include/gcdm_mp_tile.h <-> libgcdm_ops.so exports <-> native.MP_TILE_SIGNATURES,
the header from plain C (compiled, linked and run), argument refusal before any HIP call, the workspace sizes against
gcdm_mp_workspace_bytes, and set_message_path("tiled") on CPU-built networks.

The argument cases call the library with null pointers: every one of them is refused or is empty work, so nothing is launched."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
HEADER = os.path.join(ROOT, "include", "gcdm_mp_tile.h")
Z = None
TABLES = ("OPS_SIGNATURES", "MP_TRAIN_SIGNATURES", "GCP2_SIGNATURES", "OPTIM_SIGNATURES", "CLASSIFIER_SIGNATURES", "OBJECTIVE_SIGNATURES",
          "GRAD_BUCKET_SIGNATURES", "MATRIX_MODE_SIGNATURES")


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()]) for m in re.finditer(r"\b(gcdm_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_header_declares_exactly_the_signature_table():
    assert _declared() == {k: len(v) for k, v in native.MP_TILE_SIGNATURES.items()}
    assert sorted(native.MP_TILE_SIGNATURES) == ["gcdm_mp_tile_bwd", "gcdm_mp_tile_fwd", "gcdm_mp_tile_workspace_bytes"]
    # the argument lists of gcdm_mp_train.h's three entries
    for tile, old in (("gcdm_mp_tile_workspace_bytes", "gcdm_mp_workspace_bytes"), ("gcdm_mp_tile_fwd", "gcdm_mp_fwd"), ("gcdm_mp_tile_bwd", "gcdm_mp_bwd")):
        assert native.MP_TILE_SIGNATURES[tile] == native.MP_TRAIN_SIGNATURES[old]
    assert native.MP_TILE_RESTYPES == {"gcdm_mp_tile_workspace_bytes": ctypes.c_int64}


def test_names_are_disjoint_from_every_other_table():
    for t in TABLES:
        assert not set(native.MP_TILE_SIGNATURES) & set(getattr(native, t)), t
    assert not set(native.MP_TILE_SIGNATURES) & set(native.EXPORTS)


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(native.OPS_LIB_PATH), "libgcdm_ops.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(native.OPS_LIB_PATH)
    for table, res in ((native.MP_TILE_SIGNATURES, native.MP_TILE_RESTYPES), (native.MP_TRAIN_SIGNATURES, native.MP_TRAIN_RESTYPES)):
        for name, sig in table.items():
            assert hasattr(lib, name), f"libgcdm_ops.so does not export {name}"
            getattr(lib, name).argtypes = sig
            getattr(lib, name).restype = res.get(name, ctypes.c_int)
    # launch-free probe: bad edge dims with no work at all must be refused, or the null-pointer cases below would not be safe
    status = lib.gcdm_mp_tile_fwd(Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, 0, 0, 0, 65, 16, Z)
    assert status == -1, f"gcdm_mp_tile_fwd accepts SE = 65 (status {status})"
    return lib


def test_library_exports_the_entries_and_the_loader_binds_them(lib):
    assert "gcdm_ops.mp_tile.hip.h" in {os.path.basename(p) for p in native.OPS_HEADERS}
    assert "gcdm_mp_tile.h" in {os.path.basename(p) for p in native.OPS_HEADERS}
    bound = native.load_ops()
    for name, sig in native.MP_TILE_SIGNATURES.items():
        assert getattr(bound, name).argtypes == sig
    assert bound.gcdm_mp_tile_workspace_bytes.restype is ctypes.c_int64


def test_header_compiles_and_links_from_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc is not None, "no gcc"
    src = tmp_path / "t.c"
    src.write_text('#include "gcdm_mp_train.h"\n#include "gcdm_mp_tile.h"\n'
                   'int main(void) {\n'
                   '  if (gcdm_mp_tile_workspace_bytes(1, 40, 313, 64, 16) != gcdm_mp_workspace_bytes(1, 40, 313, 64, 16)) return 1;\n'
                   '  if (gcdm_mp_tile_workspace_bytes(3, 40, 313, 16, 8) != gcdm_mp_workspace_bytes(3, 40, 313, 16, 8)) return 2;\n'
                   '  if (gcdm_mp_tile_fwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 4, 0, 64, 16, 0) != 0) return 3;\n'
                   '  if (gcdm_mp_tile_bwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 16, 64, 16, 0) != -1) return 4;\n'
                   '  return 0; }\n')
    exe = tmp_path / "t"
    libdir = os.path.dirname(native.OPS_LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe), "-L", libdir,
                        "-l:libgcdm_ops.so", f"-Wl,-rpath,{libdir}", "-Wl,--unresolved-symbols=ignore-in-shared-libs"], text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)


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
    """The rules of include/gcdm_mp_train.h, case by case as tests/test_mp_train_cpu.py holds gcdm_mp_fwd / gcdm_mp_bwd to them."""
    cases = []
    for name, mk in (("gcdm_mp_tile_fwd", _fwd), ("gcdm_mp_tile_bwd", _bwd)):
        cases += [(name, mk(-1, 4), -1), (name, mk(4, -1), -1), (name, mk(0, 4), -1), (name, mk(4, 16, SE=32, VE=16), -1),
                  (name, mk(4, 16, SE=16, VE=16), -1), (name, mk(4, 16), -1), (name, mk(4, 16, w=_weights(False)), -1),
                  (name, mk(0, 0), 0), (name, mk(4, 0), 0), (name, mk(5, 0, SE=16, VE=8), 0), (name, mk(0, 0, SE=1, VE=1), -1)]
    cases += [("gcdm_mp_tile_fwd", _fwd(4, 16, tape=2), -1), ("gcdm_mp_tile_fwd", _fwd(4, 16, tape=-1), -1), ("gcdm_mp_tile_fwd", _fwd(4, 0, tape=3), -1)]
    for which in (-1, 4):
        cases.append(("gcdm_mp_tile_workspace_bytes", (which, 4, 16, 64, 16), -1))
    cases += [("gcdm_mp_tile_workspace_bytes", (0, -1, 16, 64, 16), -1), ("gcdm_mp_tile_workspace_bytes", (1, 4, -2, 64, 16), -1),
              ("gcdm_mp_tile_workspace_bytes", (2, 4, 16, 64, 8), -1), ("gcdm_mp_tile_workspace_bytes", (3, 0, 1, 16, 8), -1)]
    bad = [(n, a, want, getattr(lib, n)(*a)) for n, a, want in cases]
    assert [b for b in bad if b[2] != b[3]] == []


def _a4(n):
    return (n + 63) // 64 * 64


@pytest.mark.parametrize("N,E,SE,VE", [(1, 1, 64, 16), (9, 65, 64, 16), (40, 313, 64, 16), (1216, 23104, 64, 16), (29, 451, 16, 8), (0, 0, 16, 8)])
def test_workspace_sizes_against_the_fused_entries(lib, N, E, SE, VE):
    """which = 1 (the tape) and which = 3 (dweights) are gcdm_mp_workspace_bytes'; which = 0 drops S_pre and the silu buffer and adds a second X
    buffer; which = 2 drops the d gate_in buffer.  Neither is ever larger."""
    S, X = 256, 256 + 8 + 9
    old = [lib.gcdm_mp_workspace_bytes(w, N, E, SE, VE) for w in range(4)]
    got = [lib.gcdm_mp_tile_workspace_bytes(w, N, E, SE, VE) for w in range(4)]
    assert all(g >= 0 and g % 4 == 0 for g in got)
    assert got[1] == old[1] and got[3] == old[3]
    assert got[0] == old[0] - 4 * (2 * _a4(E * S) - _a4(E * X))
    assert got[2] == old[2] - 4 * _a4(E * S)
    assert got[0] <= old[0] and got[2] <= old[2]
    if E:
        assert got[0] < old[0] and got[2] < old[2] and got[1] > got[0]


def _net(case="qm9", **over):
    cfgs = pkg.default_cfgs(case)
    for group, kv in over.items():
        for k, v in kv.items():
            cfgs[group][k] = v
    return pkg.GCPNetDynamics(**cfgs)


@pytest.mark.parametrize("case", ["qm9", "geom"])
def test_set_message_path_tiled_round_trips(case):
    net = _net(case)
    assert net.message_path == "operators"
    net.set_message_path("tiled")
    assert net.message_path == "tiled" and all(l.interaction.path == "tiled" for l in net.interaction_layers)
    net.set_message_path("fused")
    assert net.message_path == "fused"
    net.set_message_path("tiled")
    net.set_message_path("operators")
    assert net.message_path == "operators" and all(l.interaction.path == "operators" for l in net.interaction_layers)
    with pytest.raises(ValueError):
        net.set_message_path("tile")
    mp = net.interaction_layers[0].interaction
    mp.set_path("tiled")
    assert mp.path == "tiled" and net.message_path == "mixed"
    with pytest.raises(ValueError):
        mp.set_path("Tiled")
    assert mp.path == "tiled"


@pytest.mark.parametrize("over,reason", [
    (dict(module_cfg=dict(frame_gate=True)), "vector_gate / frame_gate"),
    (dict(module_cfg=dict(selected_GCP="GCP")), "GCP2"),
    (dict(module_cfg=dict(bottleneck=2, default_bottleneck=2)), "bottleneck"),
    (dict(model_cfg=dict(h_hidden_dim=128)), "hidden sizes"),
    (dict(module_cfg=dict(nonlinearities=["relu", "silu"])), "silu"),
])
def test_set_message_path_tiled_refuses_configurations_outside_the_kernels(over, reason):
    """The scope is why_not_fused()'s; the error names the path and the reason."""
    net = _net(**over)
    with pytest.raises(NotImplementedError, match=re.escape(reason)) as err:
        net.set_message_path("tiled")
    assert "'tiled'" in str(err.value)
    assert net.message_path == "operators"
    with pytest.raises(NotImplementedError, match=re.escape(reason)) as err:
        net.interaction_layers[0].interaction.set_path("tiled")
    assert "'tiled'" in str(err.value)


def test_message_layer_refuses_an_unknown_path_before_anything_else():
    with pytest.raises(ValueError, match="path"):
        pkg.ops.message_layer(None, None, None, None, None, None, [], path="tile")
