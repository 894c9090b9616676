"""The EGNN dynamics network without a GPU: the fp64 restatement (tests/egnn_dynamics_ref.py) against the golden fixtures recorded from the
reference (tests/golden/make_egnn_dynamics_golden.py), state-dict names / shapes / order, the C header and its export list, the workspace
contracts and refusals, the column-split identity the fused kernel rests on, and the model's construction with dynamics_network="egnn"."""
import ctypes
import importlib
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import egnn_dynamics_ref as er  # noqa: E402
import ref_harness as rh  # noqa: E402

pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
HEADER = os.path.join(ROOT, "include", "gcdm_egnn_dynamics.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRIES = sorted(["gcdm_egnn_dyn_last_error", "gcdm_egnn_dyn_workspace_bytes", "gcdm_egnn_dyn_launches", "gcdm_egnn_dyn_pack", "gcdm_egnn_dyn_layer"])
OTHER_TABLES = ["OPS_SIGNATURES", "MP_TRAIN_SIGNATURES", "MP_TILE_SIGNATURES", "GCP2_SIGNATURES", "OPTIM_SIGNATURES", "CLASSIFIER_SIGNATURES",
                "OBJECTIVE_SIGNATURES", "GRAD_BUCKET_SIGNATURES", "MATRIX_MODE_SIGNATURES", "DATA_SIGNATURES", "GEOM_SIGNATURES", "MOLGRAPH_SIGNATURES",
                "MOLPROC_SIGNATURES", "CLASSIFIER_TRAIN_SIGNATURES"]


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, f"egnn_dynamics_{name}.npz"))
    W = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("W::")}
    get = lambda k: torch.from_numpy(z[k]) if k in z.files else None
    return W, get("xh"), get("t"), get("batch_index"), get("mask"), get("context"), get("xh_self_cond"), get("out")


# ---- the restatement is the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(er.GOLDEN_CONFIGS))
def test_restatement_matches_the_recorded_reference(name):
    W, xh, t, bi, mask, ctx, sc, out = load_golden(name)
    cfg = er.GOLDEN_CONFIGS[name]
    got = er.forward(W, cfg, xh, t, bi, mask, ctx, sc)
    assert got.dtype == torch.float64 and got.shape == out.shape
    scale = float(out.abs().max())
    assert float((got - out).abs().max()) <= 1e-11 * scale          # both fp64: association order only
    if name == "masked":
        assert not bool(mask.all()) and float(got[~mask].abs().max()) == 0.0
    # the fp32 run of the restatement is a usable yardstick: finite and close
    g32 = er.forward(W, cfg, xh, t, bi, mask, ctx, sc, dtype=torch.float32)
    assert g32.dtype == torch.float32 and float((g32.double() - out).abs().max()) <= 1e-3 * scale


def test_state_dict_names_shapes_and_order():
    want = json.load(open(os.path.join(GOLDEN, "egnn_dynamics_state_dict.json")))
    assert sorted(want) == sorted(er.GOLDEN_CONFIGS)
    for name, cfg in er.GOLDEN_CONFIGS.items():
        net = pkg.EGNNDynamics(**er.reference_cfgs(cfg))
        mine = [[k, list(v.shape)] for k, v in net.state_dict().items()]
        assert mine == want[name], name
        assert mine == [[k, list(s)] for k, s in er.state_dict_shapes(cfg).items()], name
        assert [k for k, _ in net.named_parameters()] == [k for k, _ in mine]
        assert net.self_condition == cfg["self_condition"] and net.num_atom_types == 5 and net.include_charges == cfg["include_charges"]
        assert net.fused_unsupported == "egnn" and net.path == "fused"
        for k, v in net.state_dict().items():                        # init_: zero biases inside the layers, non-zero matrices
            if k.startswith("egnn.") and k.endswith(".bias"):
                assert float(v.abs().max()) == 0.0, k
            if k.endswith("coors_norm.scale"):
                assert float(v) == pytest.approx(1e-2)
        with net.fp32_mfma():
            pass
        with pytest.raises(ValueError):
            net.set_path("eager")
        assert net.set_path("operators").path == "operators"


@pytest.mark.skipif(not rh.reference_available(), reason="the reference checkout is not on this machine")
def test_state_dict_against_the_imported_reference():
    import make_egnn_dynamics_golden as mk
    for k, (name, cfg) in enumerate(er.GOLDEN_CONFIGS.items()):
        ref = mk.build_reference(cfg, seed=40 + k)
        net = pkg.EGNNDynamics(**er.reference_cfgs(cfg))
        assert [(n, tuple(v.shape)) for n, v in ref.state_dict().items()] == [(n, tuple(v.shape)) for n, v in net.state_dict().items()]
        assert [n for n, _ in ref.named_parameters()] == [n for n, _ in net.named_parameters()]
        net.load_state_dict(ref.state_dict())                       # strict


# ---- header, exports, contracts -----------------------------------------------------------------------------------------------------------
def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(gcdm_egnn_dyn_\w+)\s*\(([^;{]*)\)\s*;", text):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
    return out


def test_header_declares_exactly_the_signature_table():
    assert _declared() == {k: len(v) for k, v in native.EGNN_DYN_SIGNATURES.items()}
    assert sorted(native.EGNN_DYN_SIGNATURES) == ENTRIES
    for t in OTHER_TABLES:
        assert not set(native.EGNN_DYN_SIGNATURES) & set(getattr(native, t)), t
    assert not set(native.EGNN_DYN_SIGNATURES) & set(native.EXPORTS)
    text = open(HEADER).read()
    for name in ("MAX_H", "MAX_EH", "M_DIM", "COORS_HIDDEN", "LAYER_TENSORS", "LAUNCHES_PER_LAYER"):
        assert re.search(rf"#define GCDM_EGNN_DYN_{name} {getattr(native, 'EGNN_DYN_' + name)}\b", text), name
    assert HEADER in native.OPS_HEADERS
    assert os.path.join(ROOT, "bio-diffusion_amd", "csrc", "gcdm_ops.egnn_dynamics.hip.h") in native.OPS_HEADERS
    assert '#include "gcdm_ops.egnn_dynamics.hip.h"' in open(native.OPS_SOURCES[0]).read()


@pytest.fixture(scope="module")
def lib():
    path = native.OPS_LIB_PATH
    if not os.path.exists(path):
        pytest.skip("libgcdm_ops.so not built (run __graft_entry__.build())")
    stale = [d for d in native.OPS_SOURCES + native.OPS_HEADERS if os.path.getmtime(d) > os.path.getmtime(path)]
    if stale:
        pytest.skip(f"libgcdm_ops.so is older than {stale} (run __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    for name, sig in native.EGNN_DYN_SIGNATURES.items():
        assert hasattr(lib, name), name
        getattr(lib, name).argtypes = sig
        getattr(lib, name).restype = native.EGNN_DYN_RESTYPES.get(name, ctypes.c_int)
    return lib


def test_library_exports_exactly_the_entries_and_the_loader_binds_them(lib):
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", native.OPS_LIB_PATH], text=True, capture_output=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(gcdm_egnn_dyn_\w+)", out))) == ENTRIES
    bound = native.load_ops()
    for name, sig in native.EGNN_DYN_SIGNATURES.items():
        assert getattr(bound, name).argtypes == sig


def test_workspace_bytes_contracts_and_refusals(lib):
    w = lib.gcdm_egnn_dyn_workspace_bytes
    for H, Eh in er.DIMS + [(256, 64), (256, 16)]:
        D = 2 * H + Eh + 1
        Kp = w(3, 0, H, Eh, 1, 2)
        assert Kp % 16 == 0 and 2 * D <= Kp < 2 * D + 16
        per_layer = 2 * H * Kp + 4 * Kp + 16 * Kp + 16 + 16 * 64 + 64 + 64 + 16 + 2 * H + (H + 16) * 2 * H + 2 * H + 2 * H * H + H
        assert w(1, 0, H, Eh, 1, 3) == 3 * per_layer * 4 == w(1, 7, H, Eh, 2, 3)
        for N in (0, 1, 126, 19456):
            need = (2 * N * Kp + N * (H + 16) + 2 * N * 2 * H + N * H + 3 * N) * 4
            assert need <= w(0, N, H, Eh, 1, 2) <= need + 7 * 256 + 256 and w(0, N, H, Eh, 1, 2) % 256 == 0
        assert w(2, 0, H, Eh, 1, 1) == native.EGNN_DYN_LAUNCHES_PER_LAYER
        assert 0 < w(4, 0, H, Eh, 1, 1) <= 64 * 1024 and w(5, 0, H, Eh, 1, 1) == 32
    assert w(3, 0, 32, 8, 1, 2) == 160                                  # 2 D = 146: K is padded
    bad = [(-1, 0, 32, 8, 1, 2), (6, 0, 32, 8, 1, 2), (0, -1, 32, 8, 1, 2), (0, 1 << 40, 32, 8, 1, 2), (0, 5, 0, 8, 1, 2), (0, 5, 48, 8, 1, 2),
           (0, 5, 288, 8, 1, 2), (0, 5, -32, 8, 1, 2), (0, 5, 32, 0, 1, 2), (0, 5, 32, -4, 1, 2), (0, 5, 32, 1 << 20, 1, 2), (0, 5, 32, 8, 0, 2),
           (0, 5, 32, 8, 3, 2), (0, 5, 32, 8, 1, 0)]
    for args in bad:
        assert w(*args) == -1, args
        assert lib.gcdm_egnn_dyn_last_error()
    assert lib.gcdm_egnn_dyn_launches() >= 0


def test_entries_refuse_bad_arguments_before_any_launch(lib):
    """Null or dangling pointers throughout: a call that got past its checks would fault, so every case must come back with -1."""
    X, Z = ctypes.c_void_p(64), ctypes.c_void_p(0)
    before = lib.gcdm_egnn_dyn_launches()
    T1 = (ctypes.c_void_p * 17)(*[64] * 17)

    def pack(count=17, H=32, Eh=8, e_in=1, L=1, table=T1, packed=X):
        return lib.gcdm_egnn_dyn_pack(table, count, H, Eh, e_in, L, packed, Z)

    holes = (ctypes.c_void_p * 17)(*[64] * 9 + [None] + [64] * 7)
    for k, st in enumerate([pack(count=16), pack(H=48), pack(H=0), pack(H=288), pack(Eh=0), pack(e_in=0), pack(e_in=3), pack(L=0), pack(L=2),
                            pack(table=None), pack(packed=Z), pack(table=holes)]):
        assert st == -1, k

    distinct = [ctypes.c_void_p(64 * (i + 1)) for i in range(9)]          # h_in x_in x0 | node_offsets node_mol packed workspace h_out x_out

    def layer(l=0, N=5, B=1, H=32, Eh=8, e_in=1, L=2, ptrs=None, xsc=Z):
        p = distinct if ptrs is None else ptrs
        return lib.gcdm_egnn_dyn_layer(l, p[0], p[1], p[2], xsc, p[3], p[4], p[5], p[6], p[7], p[8], Z, Z, Z, N, B, H, Eh, e_in, L, Z)

    cases = [layer(l=-1), layer(l=2), layer(N=-1), layer(B=-1), layer(N=5, B=0), layer(N=5, B=6), layer(N=1 << 30), layer(H=48), layer(H=0),
             layer(Eh=0), layer(e_in=0), layer(e_in=2), layer(e_in=1, xsc=X), layer(L=0)]
    cases += [layer(ptrs=[Z if i == j else distinct[i] for i in range(9)]) for j in range(9)]
    aliased = list(distinct)
    aliased[7] = distinct[0]
    cases.append(layer(ptrs=aliased))
    for k, st in enumerate(cases):
        assert st == -1, k
    assert layer(N=0, B=0, ptrs=[Z] * 9) == 0                              # nothing to do: no launch
    assert lib.gcdm_egnn_dyn_launches() == before


def test_header_is_c99_and_links_from_plain_c(lib, tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "gcdm_egnn_dynamics.h"\n'
                   "int main(void) {\n"
                   "  long long k = (long long)gcdm_egnn_dyn_workspace_bytes(3, 0, 256, 64, 1, 9);\n"
                   "  long long bad = (long long)gcdm_egnn_dyn_workspace_bytes(0, 5, 40, 64, 1, 9);\n"
                   "  int none = gcdm_egnn_dyn_layer(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 32, 8, 1, GCDM_EGNN_DYN_M_DIM / 16, 0);\n"
                   "  int refused = gcdm_egnn_dyn_layer(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 1, 32, 8, 1, 1, 0);\n"
                   '  printf("%lld %lld %d %d %s\\n", k, bad, none, refused, gcdm_egnn_dyn_last_error());\n'
                   "  return !(k == 1168 && bad == -1 && none == 0 && refused == -1 && gcdm_egnn_dyn_launches() == 0);\n}\n")
    exe = tmp_path / "t"
    libdir = os.path.dirname(native.OPS_LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe),
                        "-L", libdir, "-l:libgcdm_ops.so", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"], text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], text=True, capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- the identity the fused kernel rests on ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "selfcond", "masked"])
def test_column_split_identity_in_fp64(name):
    """A_i + B_j + r0 u (+ r0sc u') + c + r w_r equals edge_mlp.0 on the concatenation [h_i | h_j | edge_embedding(r0 (, r0sc)) | r]."""
    W, xh, t, bi, mask, ctx, sc, _ = load_golden(name)
    cfg = er.GOLDEN_CONFIGS[name]
    W = {k: v.double() for k, v in W.items()}
    probe = {}
    er.forward(W, cfg, xh, t, bi, mask, ctx, sc, probe=probe)
    ei = er.edge_index_of(bi, mask.bool())
    x0 = probe["x_init"]
    r0 = ((x0[ei[0]] - x0[ei[1]]) ** 2).sum(-1, keepdim=True)
    e, r0sc = r0, None
    if cfg["self_condition"]:
        s = sc.double()[:, :3]
        r0sc = ((s[ei[0]] - s[ei[1]]) ** 2).sum(-1, keepdim=True)
        e = torch.cat([r0, r0sc], -1)
    e_attr = e @ W["edge_embedding.weight"].T + W["edge_embedding.bias"]
    for l, (h, x) in enumerate(zip([probe["h_in"]] + probe["h"][:-1], [probe["x_in"]] + probe["x"][:-1])):
        p = f"egnn.mpnn_layers.{l}."
        r = ((x[ei[0]] - x[ei[1]]) ** 2).sum(-1, keepdim=True)
        concat = torch.cat([h[ei[1]], h[ei[0]], e_attr, r], -1) @ W[p + "edge_mlp.0.weight"].T + W[p + "edge_mlp.0.bias"]
        split = er.column_split_pre(W, p, W["edge_embedding.weight"], W["edge_embedding.bias"], h, x, r0, ei, r0sc)
        assert float((split - concat).abs().max()) <= 1e-12 * float(concat.abs().max()), l


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def test_model_constructs_with_the_egnn_dynamics_network_on_the_cpu():
    """Fails before this network existed: the constructor raised NotImplementedError for dynamics_network="egnn"."""
    cfgs = pkg.default_cfgs("qm9")
    cfgs["diffusion_cfg"]["dynamics_network"] = "egnn"
    cfgs["model_cfg"]["num_encoder_layers"] = 2
    model = pkg.QM9MoleculeGenerationDDPM(**cfgs)
    dyn = model.ddpm.dynamics_network
    assert isinstance(dyn, pkg.EGNNDynamics) and dyn.fused_unsupported == "egnn"
    H, Eh = dyn.node_dims[0], dyn.edge_dims[0]
    cfg = dict(H=H, Eh=Eh, L=2, num_atom_types=dyn.num_atom_types, include_charges=dyn.include_charges, condition_on_time=dyn.condition_on_time,
               num_context=dyn.num_context_node_features, self_condition=dyn.self_condition)
    want = ["ddpm.dynamics_network." + k for k in er.state_dict_shapes(cfg)]
    got = [k for k in model.state_dict() if k.startswith("ddpm.dynamics_network.")]
    assert got == want
    assert {k: tuple(v.shape) for k, v in dyn.state_dict().items()} == er.state_dict_shapes(cfg)
    assert model.ddpm.runs_generic_loop_only()
    for call in (lambda: model.ddpm.mol_gen_sample_packed([torch.tensor([3])], "cpu"), lambda: model.ddpm.mol_gen_sample_concurrent([torch.tensor([3])], "cpu"),
                 lambda: model.ddpm.mol_gen_sample(1, torch.tensor([3]), "cpu", lanes=2),
                 lambda: model.sample_and_analyze(4, packed_batches=2), lambda: model.sample_and_analyze(4, concurrent_batches=2)):
        with pytest.raises(NotImplementedError, match="EGNN"):
            call()
    cfgs["diffusion_cfg"]["dynamics_network"] = "transformer"
    with pytest.raises(NotImplementedError):
        pkg.QM9MoleculeGenerationDDPM(**cfgs)
    # a GCPNet model is what it was
    assert isinstance(pkg.QM9MoleculeGenerationDDPM(**pkg.default_cfgs("qm9")).ddpm.dynamics_network, pkg.GCPNetDynamics)


def test_load_from_checkpoint_takes_reference_keys(tmp_path):
    cfgs = pkg.default_cfgs("qm9")
    cfgs["diffusion_cfg"]["dynamics_network"] = "egnn"
    cfgs["model_cfg"].update(num_encoder_layers=1, h_hidden_dim=32, e_hidden_dim=8)
    model = pkg.QM9MoleculeGenerationDDPM(**cfgs)
    sd = {k: torch.randn_like(v) if v.is_floating_point() else v.clone() for k, v in model.state_dict().items()}
    path = str(tmp_path / "egnn.ckpt")
    torch.save({"state_dict": sd}, path)
    loaded = model.load_from_checkpoint(path)
    for k, v in loaded.state_dict().items():
        if k.startswith("ddpm.dynamics_network."):
            assert torch.equal(v, sd[k]), k
    del sd["ddpm.dynamics_network.egnn.mpnn_layers.0.coors_norm.scale"]
    torch.save({"state_dict": sd}, path)
    with pytest.raises(RuntimeError, match="does not match the dynamics network"):
        model.load_from_checkpoint(path)
