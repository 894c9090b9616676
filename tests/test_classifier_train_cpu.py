"""The classifier's training path without a GPU: include/gcdm_classifier_train.h <-> libgcdm_ops.so exports <-> native.CLASSIFIER_TRAIN_SIGNATURES,
the header as C99 linked from plain C, argument refusal before any HIP call; the fp64 autograd of the restatement (tests/classifier_ref.py)
against the autograd of the imported reference; the fp32-vs-fp64 gaps that scale the GPU bars; the pure-Python backward of the new operator
against torch autograd of the concatenated form, and its mutants; save_classifier -> get_classifier's files; train_epoch's refusals; and the
condition of the GPU trajectory test."""
import ctypes
import importlib
import os
import pickle
import re
import shutil
import subprocess

import pytest
import torch

import classifier_ref as cr
import classifier_train_ref as ct
import ref_harness as rh
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
clf = pkg.classifier
HEADER = os.path.join(ROOT, "include", "gcdm_classifier_train.h")
ENTRIES = ["gcdm_classifier_train_edge_pre_bwd", "gcdm_classifier_train_edge_pre_fwd", "gcdm_classifier_train_workspace_bytes"]
TABLES = ("OPS_SIGNATURES", "MP_TRAIN_SIGNATURES", "MP_TILE_SIGNATURES", "GCP2_SIGNATURES", "OPTIM_SIGNATURES", "CLASSIFIER_SIGNATURES",
          "OBJECTIVE_SIGNATURES", "GRAD_BUCKET_SIGNATURES", "MATRIX_MODE_SIGNATURES", "DATA_SIGNATURES", "GEOM_SIGNATURES", "MOLGRAPH_SIGNATURES")
Z = None
# the cases of tests/test_classifier_train_gpu.py: every small one, and the large batch once
NET_CASES = [(r, cfg, fl, s) for r in ("init", "hot") for cfg in ct.NET_CONFIGS for fl in ct.NET_FLAGS for s in ct.SIZE_SETS]
OP_SIZE_SETS = [cr.INSTANTIATION_SIZES, [32], [1], [0]]


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(gcdm_classifier_train_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
    return out


# ---- header, exports, refusals ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_signature_table():
    assert _declared() == {k: len(v) for k, v in native.CLASSIFIER_TRAIN_SIGNATURES.items()}
    assert sorted(native.CLASSIFIER_TRAIN_SIGNATURES) == ENTRIES
    for t in TABLES:
        assert not set(native.CLASSIFIER_TRAIN_SIGNATURES) & set(getattr(native, t)), t
    assert not set(native.CLASSIFIER_TRAIN_SIGNATURES) & set(native.EXPORTS)
    text = open(HEADER).read()
    for name in ("MAX_H", "TWO_STAGE_EDGES", "SLICE_EDGES", "MAX_SLICES"):
        assert re.search(rf"#define GCDM_CLASSIFIER_TRAIN_{name} {getattr(native, 'CLASSIFIER_TRAIN_' + name)}\b", text), name


def test_header_and_kernels_are_library_dependencies():
    assert HEADER in native.OPS_HEADERS
    assert os.path.join(ROOT, "bio-diffusion_amd", "csrc", "gcdm_ops.classifier_train.hip.h") in native.OPS_HEADERS
    assert '#include "gcdm_ops.classifier_train.hip.h"' in open(native.OPS_SOURCES[0]).read()


@pytest.fixture(scope="module")
def lib():
    path = native.OPS_LIB_PATH
    if not os.path.exists(path):
        pytest.skip("libgcdm_ops.so not built (run __graft_entry__.build())")
    stale = [d for d in native.OPS_SOURCES + native.OPS_HEADERS if os.path.getmtime(d) > os.path.getmtime(path)]
    if stale:
        pytest.skip(f"libgcdm_ops.so is older than {stale} (run __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    for name, sig in native.CLASSIFIER_TRAIN_SIGNATURES.items():
        assert hasattr(lib, name), name
        getattr(lib, name).argtypes = sig
        getattr(lib, name).restype = native.CLASSIFIER_TRAIN_RESTYPES.get(name, ctypes.c_int)
    return lib


def test_library_exports_exactly_the_entries_and_the_loader_binds_them(lib):
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", native.OPS_LIB_PATH], text=True, capture_output=True, check=True).stdout
        assert sorted(set(re.findall(r"\b(gcdm_classifier_train_\w+)", out))) == ENTRIES
    two, per, cap = native.CLASSIFIER_TRAIN_TWO_STAGE_EDGES, native.CLASSIFIER_TRAIN_SLICE_EDGES, native.CLASSIFIER_TRAIN_MAX_SLICES
    w = lib.gcdm_classifier_train_workspace_bytes
    assert w(0, 32) == 0 and w(two - 1, 96) == 0                              # one stage: dw_r is written directly
    assert w(two, 96) == -(-two // per) * 96 * 4 and w(two, 96) % 256 == 0    # two stages from that count on
    assert w(two, 33) % 256 == 0 and w(two, 33) >= -(-two // per) * 33 * 4
    assert w(1 << 40, 32) == cap * 32 * 4
    for E, H in ((-1, 32), (8, 0), (8, -1), (8, native.CLASSIFIER_TRAIN_MAX_H + 1), (1 << 60, 32)):
        assert w(E, H) == -1, (E, H)
    bound = native.load_ops()
    for name, sig in native.CLASSIFIER_TRAIN_SIGNATURES.items():
        assert getattr(bound, name).argtypes == sig


def test_header_is_c99_and_links_from_plain_c(lib, tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "gcdm_classifier_train.h"\n'
                   "int main(void) {\n"
                   "  long long w = (long long)gcdm_classifier_train_workspace_bytes(GCDM_CLASSIFIER_TRAIN_TWO_STAGE_EDGES, 64);\n"
                   "  long long z = (long long)gcdm_classifier_train_workspace_bytes(GCDM_CLASSIFIER_TRAIN_TWO_STAGE_EDGES - 1, 64);\n"
                   "  int empty = gcdm_classifier_train_edge_pre_fwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 5, 0, 32, 0);\n"
                   "  int bad = gcdm_classifier_train_edge_pre_fwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 1, 20, 32, 0);\n"
                   "  int none = gcdm_classifier_train_edge_pre_bwd(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0);\n"
                   '  printf("%lld %lld %d %d %d\\n", w, z, empty, bad, none);\n'
                   "  return !(w > 0 && z == 0 && empty == 0 && bad == -1 && none == 0);\n}\n")
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
    two = native.CLASSIFIER_TRAIN_TWO_STAGE_EDGES

    def fwd(N=5, nmol=1, E=20, H=32, ptrs=(X,) * 9):
        return lib.gcdm_classifier_train_edge_pre_fwd(*ptrs, N, nmol, E, H, Z)

    cases = [fwd(N=-1), fwd(N=1 << 31), fwd(nmol=-1), fwd(nmol=1 << 31), fwd(nmol=0), fwd(N=1), fwd(E=-1), fwd(H=0), fwd(H=-3),
             fwd(H=native.CLASSIFIER_TRAIN_MAX_H + 1), fwd(E=1 << 60)]
    cases += [fwd(ptrs=tuple(Z if i == j else X for i in range(9))) for j in range(9)]
    for k, status in enumerate(cases):
        assert status == -1, k
    assert fwd(E=0, ptrs=(Z,) * 9) == 0 and fwd(N=0, nmol=0, E=0, ptrs=(Z,) * 9) == 0          # nothing to do: no launch
    assert fwd(E=0, H=0, ptrs=(Z,) * 9) == -1

    def bwd(N=5, nmol=1, E=20, H=32, ptrs=(X,) * 9):
        return lib.gcdm_classifier_train_edge_pre_bwd(*ptrs, N, nmol, E, H, Z)

    cases = [bwd(N=-1), bwd(N=1 << 31), bwd(nmol=-1), bwd(nmol=0), bwd(N=1), bwd(E=-1), bwd(H=0), bwd(H=native.CLASSIFIER_TRAIN_MAX_H + 1), bwd(E=1 << 60)]
    cases += [bwd(ptrs=tuple(Z if i == j else X for i in range(9))) for j in range(8)]          # below the two-stage count the workspace may be null
    cases += [bwd(N=200, nmol=7, E=two, ptrs=tuple(Z if i == j else X for i in range(9))) for j in range(9)]      # from it on it may not
    for k, status in enumerate(cases):
        assert status == -1, k
    assert bwd(E=0, ptrs=(Z,) * 9) == 0
    assert bwd(E=0, N=-1, ptrs=(Z,) * 9) == -1


# ---- autograd of the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not rh.reference_available(), reason="the reference checkout is not on this machine")
@pytest.mark.parametrize("att,attr", [(1, 1), (0, 0)])
def test_autograd_of_the_restatement_against_the_imported_reference(att, attr):
    rh.install_stubs()
    src = importlib.import_module("src")
    sizes = [9, 1, 14, 2, 21]
    W = synth.make_weights(cr.state_dict_shapes(5, 64, 3, bool(att), bool(attr)), seed=23)
    x, h0 = cr.make_batch(sizes, 5, seed=31)
    t = ct.targets(len(sizes))
    model = src.EGNN(in_node_nf=5, in_edge_nf=0, hidden_nf=64, device="cpu", n_layers=3, coords_weight=1.0, attention=att, node_attr=attr)
    model.load_state_dict(W)
    model = model.double().train()
    xp, hp, nm, em, n = cr.to_padded(x, h0, sizes)
    pred = model(h0=hp.double(), x=xp.double(), edges=src.get_classifier_adj_matrix(n, len(sizes), "cpu", edges_dic={}), edge_attr=None,
                 node_mask=nm.double(), edge_mask=em.double(), n_nodes=n)
    loss = torch.nn.L1Loss()(pred, t.double())
    loss.backward()
    l64, g64, _ = ct.loss_and_grads(W, x, h0, sizes, t)
    assert abs(l64 - loss.item()) <= 1e-12
    named = dict(model.named_parameters())
    assert set(named) == set(g64) == set(model.state_dict())
    for k, p in named.items():
        assert (g64[k] - p.grad).abs().max().item() <= 1e-12, k


def test_chunked_accumulation_is_the_whole_batch():
    sizes = [3, 0, 5, 1, 4, 2, 6]
    W = synth.make_weights(cr.state_dict_shapes(5, 32, 2, True, True), seed=4)
    x, h0 = cr.make_batch(sizes, 5, seed=6)
    t = ct.targets(len(sizes))
    la, ga, pa = ct.loss_and_grads(W, x, h0, sizes, t, chunk=128)
    lb, gb, pb = ct.loss_and_grads(W, x, h0, sizes, t, chunk=2)
    assert abs(la - lb) <= 1e-14 and (pa - pb).abs().max().item() <= 1e-14
    for k in ga:
        assert (ga[k] - gb[k]).abs().max().item() <= 1e-13, k


# ---- the gaps that scale the GPU bars --------------------------------------------------------------------------------------------------------------
def _check_gaps(c):
    """Per parameter tensor: the fp32 autograd's distance to the fp64 autograd is a real rounding distance, non-zero and below 1e-4 of the
    tensor's largest entry -- wherever the tensor has a gradient at all (a molecule without edges leaves the edge layers' gradients exactly 0
    in both precisions, an empty molecule every gradient but the last biases').  A gap of exactly 0 is admitted only for a tensor whose fp64
    gradient is itself made of fp32 numbers (the last bias of a one-molecule batch: +-1), which an fp32 run can land on; the floor of the
    GPU bar exists for that tensor."""
    assert set(c.grads64) == set(c.W) and set(c.grads32) == set(c.W)
    assert float((c.pred64 - c.target.double()).abs().min()) > 1e-3 if len(c.sizes) else True          # no |.| of the loss sits on its kink
    for k, g in c.grads64.items():
        top, gap = float(g.abs().max()), float((c.grads32[k] - g).abs().max())
        if top == 0.0:
            assert gap == 0.0, k
            continue
        assert gap < 1e-4 * top, (k, gap, top)
        assert gap > 0.0 or torch.equal(g, g.float().double()), (k, gap, top)
    assert 0.0 <= abs(c.loss32 - c.loss64) < 1e-4 * abs(c.loss64)


@pytest.mark.parametrize("regime,cfg,flags,sizes", NET_CASES, ids=[f"{r}-F{c[0]}H{c[1]}L{c[2]}-a{f[0]}n{f[1]}-{s}" for r, c, f, s in NET_CASES])
def test_fp32_gap_of_every_parameter_is_a_rounding_distance(regime, cfg, flags, sizes):
    _check_gaps(ct.case(regime, cfg, flags, sizes))


@pytest.mark.parametrize("regime", ["init", "hot"])
def test_fp32_gap_of_every_parameter_on_the_large_batch(regime):
    name, cfg, flags = ct.BIG
    _check_gaps(ct.case(regime, cfg, flags, name))


# ---- the new operator: definition, backward, mutants ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", OP_SIZE_SETS + [[3, 1, 0, 4]], ids=lambda s: f"B{len(s)}N{sum(s)}")
@pytest.mark.parametrize("H", [4, 32])
def test_python_backward_equals_autograd_of_the_concatenated_form(sizes, H):
    """edge_mlp.0 as the reference writes it, cat([h[row], h[col], radial]) W^T + b, differentiated by torch in fp64; the split form's
    gradients chain to the same dh, dW and db through the two node-level linears."""
    inp = ct.op_inputs(sizes, H)
    g = torch.Generator().manual_seed(7)
    h = torch.randn(inp.N, H, generator=g, dtype=torch.float64, requires_grad=True)
    W = torch.randn(H, 2 * H + 1, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(H, generator=g, dtype=torch.float64, requires_grad=True)
    row, col = ct.edge_list(sizes)
    x = inp.x.double()
    pre_cat = torch.cat([h[row], h[col], ct.radial_of(x, row, col)[:, None]], 1) @ W.T + b
    dpre = inp.dpre.double()
    pre_cat.backward(dpre)
    hd, Wd, bd = h.detach(), W.detach(), b.detach()
    A, B = hd @ Wd[:, :H].T + bd, hd @ Wd[:, H:2 * H].T
    pre, _ = ct.edge_pre(A, B, x, Wd[:, 2 * H], sizes)
    top = lambda t: float(t.abs().max()) if t.numel() else 0.0
    assert pre.shape == (inp.E, H) and top(pre - pre_cat.detach()) <= 1e-12
    dA, dB, dw = ct.edge_pre_bwd(dpre, x, sizes, inp.N)
    scale = max(1.0, top(W.grad))
    assert top(torch.cat([dA.T @ hd, dB.T @ hd, dw[:, None]], 1) - W.grad) <= 1e-12 * scale
    assert top(dA.sum(0) - b.grad) <= 1e-12 * scale
    assert top(dA @ Wd[:, :H] + dB @ Wd[:, H:2 * H] - h.grad) <= 1e-12 * scale


@pytest.mark.parametrize("sizes", OP_SIZE_SETS, ids=lambda s: f"B{len(s)}N{sum(s)}")
@pytest.mark.parametrize("H", ct.OP_H)
def test_no_mutant_of_the_backward_survives_the_gpu_cases(sizes, H):
    """On every case of tests/test_classifier_train_cabi_gpu.py that has an edge, each mutant is further from the definition than the bar that
    test allows (4 gap + floor per tensor, gap = the fp32 evaluation of the definition): the test would see it.  A case without edges cannot
    tell them apart and is not asked to."""
    inp = ct.op_inputs(sizes, H)
    if inp.E == 0:
        for m in ct.MUTANTS:
            assert all(float(t.abs().max()) == 0.0 if t.numel() else True for t in ct.edge_pre_bwd(inp.dpre, inp.x, sizes, inp.N, mutant=m))
        return
    names = ("dA", "dB", "dw_r")
    want = dict(zip(names, ct.edge_pre_bwd(inp.dpre, inp.x, sizes, inp.N)))
    ref32 = dict(zip(names, ct.edge_pre_bwd(inp.dpre, inp.x, sizes, inp.N, dtype=torch.float32)))
    failures, _, count = ct.judge(ref32, want, ref32)
    assert not failures and count == 3                                             # the definition itself passes its bar
    for m in ct.MUTANTS:
        got = dict(zip(names, ct.edge_pre_bwd(inp.dpre, inp.x, sizes, inp.N, mutant=m)))
        failures, ratios, _ = ct.judge(got, want, ref32)
        assert failures, f"mutant {m} survives: ratios {ratios}"


def test_edge_tables_and_sizes_with_edges():
    mol, noff, eoff = ct.edge_tables([3, 0, 1, 4])
    assert mol.tolist() == [0, 0, 0, 2, 3, 3, 3, 3] and noff.tolist() == [0, 3, 3, 4, 8] and eoff.tolist() == [0, 6, 6, 6, 18]
    two = native.CLASSIFIER_TRAIN_TWO_STAGE_EDGES
    for E in (two - 2, two):
        s = ct.sizes_with_edges(E)
        assert sum(n * (n - 1) for n in s) == E and max(s) <= 32


# ---- files and the loop ---------------------------------------------------------------------------------------------------------------------------
class _Holder:
    """What save_classifier reads of a model, without a device."""

    def __init__(self, F, H, L, att, attr, W):
        self.in_node_nf, self.hidden_nf, self.n_layers, self.attention, self.node_attr, self._W = F, H, L, bool(att), bool(attr), W

    def state_dict(self):
        return self._W


def test_save_classifier_writes_what_get_classifier_reads(tmp_path):
    W = synth.make_weights(cr.state_dict_shapes(5, 64, 2, True, False), seed=3)
    clf.save_classifier(_Holder(5, 64, 2, 1, 0, W), str(tmp_path / "m"), property="alpha", lr=1e-3)
    args = clf.load_classifier_args(str(tmp_path / "m" / "args.pickle"))
    assert (args.nf, args.n_layers, args.attention, args.node_attr, args.property, args.lr) == (64, 2, 1, 0, "alpha", 1e-3)
    with open(tmp_path / "m" / "args.pickle", "rb") as f:
        assert vars(pickle.load(f)) == vars(args)                                             # plain pickle reads it too, as the reference does
    sd = torch.load(str(tmp_path / "m" / "best_checkpoint.npy"), map_location="cpu", weights_only=True)
    assert list(sd) == list(W) and all(torch.equal(sd[k], W[k]) for k in W)
    with pytest.raises(ValueError, match="contradicts"):
        clf.save_classifier(_Holder(5, 64, 2, 1, 0, W), str(tmp_path / "n"), nf=128)
    with pytest.raises(ValueError, match="in_node_nf = 5"):
        clf.save_classifier(_Holder(6, 64, 2, 1, 0, W), str(tmp_path / "n"))
    with pytest.raises(pickle.UnpicklingError):
        clf.save_classifier(_Holder(5, 64, 2, 1, 0, W), str(tmp_path / "n"), device=torch.device("cpu"))


def test_train_epoch_refuses_what_cannot_train():
    class M:
        path = "fused"
    with pytest.raises(ValueError, match="optimizer"):
        clf.train_epoch(M(), [], 0.0, 1.0, "alpha")
    with pytest.raises(ValueError, match="operators"):
        clf.train_epoch(M(), [], 0.0, 1.0, "alpha", optimizer=object())
    with pytest.raises(ValueError, match="no batch"):
        clf.train_epoch(M(), [], 0.0, 1.0, "alpha", partition="test")


def test_paths_and_edge_inputs_are_named():
    assert clf.PATHS == ("fused", "operators") and clf.EDGE_INPUTS == ("split", "concat")
    for name in ("set_path", "path", "set_edge_input", "edge_input"):
        assert hasattr(clf.EGNN, name)
    assert isinstance(clf.EGNN.path, property) and clf.EGNN.path.fset is None


# ---- the condition of the trajectory test ---------------------------------------------------------------------------------------------------------
def sgd_trajectory(dtype):
    """Loss before each of the steps and after the last, plain SGD on the restatement: steps + 1 numbers, and the final weights."""
    T = ct.TRAJECTORY
    (F, H, L), (att, attr) = T["cfg"], T["flags"]
    W, x, h0 = cr.make_regime(T["regime"], F, H, L, att, attr, cr.INSTANTIATION_SIZES)
    return ct.trajectory(W, x, h0, cr.INSTANTIATION_SIZES, ct.targets(len(cr.INSTANTIATION_SIZES)), T["steps"], T["lr"], dtype)


def test_condition_of_the_trajectory_test_training_reduces_the_loss():
    losses, _ = sgd_trajectory(torch.float64)
    print("fp64 SGD trajectory:", [f"{v:.6f}" for v in losses])
    assert len(losses) == ct.TRAJECTORY["steps"] + 1 and losses[-1] < losses[0]
    l32, _ = ct._one_thread(lambda: sgd_trajectory(torch.float32))
    gaps = [abs(a - b) for a, b in zip(l32, losses)]
    print("fp32 - fp64 per step:", [f"{v:.2e}" for v in gaps])
    assert all(g < 1e-4 * abs(v) for g, v in zip(gaps, losses))
