"""The fused stand-alone GCP2's C ABI and switches, without a GPU: include/gcdm_gcp2_train.h as C99 linked against libgcdm_ops.so, the three
exports, the host-only workspace query, GCP2.why_not_fused / set_path and GCPNetDynamics.set_node_path on CPU-built modules, and the yardstick
of the GPU tests (tests/gcp2_ref.py: oracle.gcdm_oracle.gcp2 in fp64 and fp32) against the reference's recorded tests/golden/fn_gcp2.npz."""
import ctypes
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gcp2_ref as R
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
HEADER = os.path.join(ROOT, "include", "gcdm_gcp2_train.h")
GCP2 = pkg.gcp_modules.GCP2
Z = None


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(native.OPS_LIB_PATH), "libgcdm_ops.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(native.OPS_LIB_PATH)
    for name, sig in native.GCP2_SIGNATURES.items():
        assert hasattr(lib, name), f"libgcdm_ops.so does not export {name}"
        getattr(lib, name).argtypes = sig
        getattr(lib, name).restype = native.GCP2_RESTYPES.get(name, ctypes.c_int)
    return lib


def _cd(d):
    return native.Gcp2Dims(d["SI"], d["VI"], d["SO"], d["VO"], d["H"], d["ff"], d["a0"], d["a1"])


def test_three_symbols_exported(lib):
    assert sorted(native.GCP2_SIGNATURES) == ["gcdm_gcp2_bwd", "gcdm_gcp2_fwd", "gcdm_gcp2_workspace_bytes"]


def test_header_compiles_and_links_from_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc is not None, "no gcc"
    src = tmp_path / "t.c"
    d = R.instances("qm9")["ff"]
    n = sum(int(np.prod(s)) for s in R.weight_shapes(d).values())
    src.write_text('#include "gcdm_gcp2_train.h"\n'
                   f'int main(void) {{ gcdm_gcp2_dims d = {{{d["SI"]}, {d["VI"]}, {d["SO"]}, {d["VO"]}, {d["H"]}, 1, 0, 0}};\n'
                   f'  if (gcdm_gcp2_workspace_bytes(3, 7, &d) != (int64_t)4 * {n}) return 1;\n'
                   '  if (gcdm_gcp2_fwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, &d, 0) != 0) return 2;\n'
                   '  if (gcdm_gcp2_bwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1, &d, 0) != -1) return 3;\n  return 0; }\n')
    exe = tmp_path / "t"
    libdir = os.path.dirname(native.OPS_LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe), "-L", libdir,
                        "-l:libgcdm_ops.so", f"-Wl,-rpath,{libdir}", "-Wl,--unresolved-symbols=ignore-in-shared-libs"], text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)


@pytest.mark.parametrize("case", ["qm9", "geom"])
def test_workspace_query_is_host_only_and_monotone(lib, case):
    for sc in (False, True):
        for name, d in R.instances(case, sc).items():
            cd = _cd(d)
            n_w = sum(int(np.prod(s)) for s in R.weight_shapes(d).values())
            prev = [-1, -1, -1]
            for M in (0, 1, 63, 64, 65, 1216, 64 * 19 * 18):
                got = [lib.gcdm_gcp2_workspace_bytes(w, M, ctypes.byref(cd)) for w in range(4)]
                assert all(g >= 0 and g % 4 == 0 for g in got), (name, M, got)
                assert got[3] == 4 * n_w
                assert got[1] >= got[0]
                assert all(g >= p for g, p in zip(got[:3], prev)), (name, M)
                prev = got[:3]
            K = d["SI"] + d["H"] + 9
            tape = d["H"] * 3 + K + d["SO"] * (1 + d["ff"]) + d["VO"]
            assert lib.gcdm_gcp2_workspace_bytes(1, 64, ctypes.byref(cd)) == 4 * 64 * tape          # 64 rows: every block is 256-byte aligned


def test_workspace_query_refuses_bad_arguments(lib):
    d = R.instances("qm9")["pos"]
    ok = _cd(d)
    assert lib.gcdm_gcp2_workspace_bytes(0, 5, ctypes.byref(ok)) > 0
    assert lib.gcdm_gcp2_workspace_bytes(4, 5, ctypes.byref(ok)) == -1
    assert lib.gcdm_gcp2_workspace_bytes(-1, 5, ctypes.byref(ok)) == -1
    assert lib.gcdm_gcp2_workspace_bytes(0, -1, ctypes.byref(ok)) == -1
    assert lib.gcdm_gcp2_workspace_bytes(0, 5, None) == -1
    for field, bad in (("SI", 0), ("SI", 2049), ("VI", 0), ("VI", 129), ("SO", 0), ("SO", 1025), ("VO", -1), ("VO", 65), ("H", 0), ("H", 65),
                       ("feedforward_out", 2), ("act_scalar", 2), ("act_vector", -1)):
        cd = _cd(d)
        setattr(cd, field, bad)
        assert lib.gcdm_gcp2_workspace_bytes(0, 5, ctypes.byref(cd)) == -1, (field, bad)
        # refused before any HIP call, with nothing to touch
        assert lib.gcdm_gcp2_fwd(Z, Z, Z, Z, Z, Z, Z, Z, 0, 5, ctypes.byref(cd), Z) == -1
        assert lib.gcdm_gcp2_bwd(Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, 5, ctypes.byref(cd), Z) == -1
    # null pointers with work to do; empty work is 0
    assert lib.gcdm_gcp2_fwd(Z, Z, Z, Z, Z, Z, Z, Z, 0, 5, ctypes.byref(ok), Z) == -1
    assert lib.gcdm_gcp2_fwd(Z, Z, Z, Z, Z, Z, Z, Z, 2, 0, ctypes.byref(ok), Z) == -1
    assert lib.gcdm_gcp2_fwd(Z, Z, Z, Z, Z, Z, Z, Z, 1, 0, ctypes.byref(ok), Z) == 0
    assert lib.gcdm_gcp2_bwd(Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, 0, ctypes.byref(ok), Z) == 0


# ---- the module switch on CPU-constructed modules ---------------------------------------------------------------------------------------------
def test_gcp2_path_default_and_switch():
    m = GCP2((256, 32), (256, 1), bottleneck=4)
    assert m.path == "operators" and m.why_not_fused() is None
    m.set_path("fused")
    assert m.path == "fused"
    m.set_path("operators")
    with pytest.raises(ValueError):
        m.set_path("eager")
    ws = m.fused_weights()
    assert [tuple(w.shape) for w in ws] == list(R.weight_shapes(R.instances("qm9")["pos"]).values())
    ff = GCP2((512, 64), (256, 32), bottleneck=4, feedforward_out=True, nonlinearities=(None, None))
    assert [tuple(w.shape) for w in ff.fused_weights()] == list(R.weight_shapes(R.instances("qm9")["ff"]).values())
    proj = GCP2((256, 32), (7, 0), nonlinearities=(None, None))
    assert proj.why_not_fused() is None and len(proj.fused_weights()) == 4


@pytest.mark.parametrize("kwargs,word", [
    (dict(frame_gate=True), "frame_gate"), (dict(sigma_frame_gate=True), "sigma_frame_gate"), (dict(vector_gate=False), "vector_gate"),
    (dict(scalar_gate=1), "scalar_gate"), (dict(vector_residual=True), "vector_residual"), (dict(vector_frame_residual=True), "vector_frame_residual"),
    (dict(ablate_frame_updates=True), "ablate_frame_updates"), (dict(ablate_scalars=True), "ablate_scalars"), (dict(ablate_vectors=True), "ablate_vectors"),
    (dict(scalarization_vectorization_output_dim=2), "scalarization_vectorization_output_dim"), (dict(nonlinearities=("relu", "silu")), "nonlinearities"),
    (dict(feedforward_out=True, scalar_out_nonlinearity="relu"), "scalar_out_nonlinearity"),
])
def test_gcp2_out_of_scope_names_the_reason(kwargs, word):
    m = GCP2((32, 8), (32, 8), **kwargs)
    why = m.why_not_fused()
    assert why is not None and word in why
    with pytest.raises(NotImplementedError, match=word):
        m.set_path("fused")
    assert m.path == "operators"


def test_gcp2_out_of_bounds_dims_name_the_dim():
    assert "VO" in GCP2((32, 8), (32, 65)).why_not_fused()
    assert "H" in GCP2((32, 128), (32, 8), bottleneck=1).why_not_fused()
    assert "vector inputs" in GCP2((32, 0), (32, 0)).why_not_fused()


@pytest.mark.parametrize("case", ["qm9", "geom"])
def test_set_node_path_switches_every_standalone_gcp2(case):
    net = pkg.GCPNetDynamics(**pkg.default_cfgs(case))
    L = synth.DATASET_DIMS[case]["L"]
    mods = net.standalone_gcps()
    assert len(mods) == 2 + 2 * L + 1
    assert net.node_path == "operators" and net.message_path == "operators"
    net.set_node_path("fused")
    assert net.node_path == "fused" and all(m.path == "fused" for m in mods)
    assert net.message_path == "operators"                                      # the two switches are independent
    assert all(m.path == "operators" for layer in net.interaction_layers for m in layer.interaction.message_fusion)
    net.set_message_path("fused")
    net.set_node_path("operators")
    assert net.node_path == "operators" and net.message_path == "fused"
    with pytest.raises(ValueError):
        net.set_node_path("eager")
    got = {(m.scalar_input_dim, m.vector_input_dim, m.scalar_output_dim, m.vector_output_dim, m.hidden_dim) for m in mods}
    want = {(d["SI"], d["VI"], d["SO"], d["VO"], d["H"]) for d in R.instances(case).values()}
    assert got == want


def test_set_node_path_refuses_an_out_of_scope_network():
    cfgs = synth.apply_variant(pkg.default_cfgs("qm9"), "frame_gate")
    net = pkg.GCPNetDynamics(**cfgs)
    with pytest.raises(NotImplementedError, match="frame_gate"):
        net.set_node_path("fused")
    assert net.node_path == "operators"


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,node", [("edge", False), ("node", True), ("nodeff", True), ("proj", True)])
def test_reference_reproduces_the_recorded_fixture(golden_dir, name, node):
    g = {k: torch.tensor(v) for k, v in np.load(os.path.join(golden_dir, "fn_gcp2.npz")).items()}
    d, W, s, v, F, _, want_s, want_v = R.golden_case(g, name, node)
    rs, rv = torch.zeros((s.shape[0], d["SO"])), torch.zeros((s.shape[0], d["VO"], 3))
    ref64, ref32 = R.references(W, d, s, v, F, rs, rv, grads=False)
    for ref in (ref64, ref32):
        assert (ref["s_out"] - want_s.double()).abs().max().item() <= 2e-6
        if want_v is not None:
            assert (ref["v_out"] - want_v.double()).abs().max().item() <= 2e-6
