"""The EGNN property classifier without a GPU: include/gcdm_classifier.h <-> libgcdm_ops.so exports <-> native.CLASSIFIER_SIGNATURES, the header
as C99 linked from plain C, argument refusal before any HIP call, the module's state dict against the reference's (fixture lists), the loader
and its restricted unpickler, property_mae's bookkeeping, and the fp64 restatement the GPU tests use (tests/classifier_ref.py) against the
reference's fp64 predictions and per-layer h stored by tests/golden/make_classifier_golden.py."""
import argparse
import ctypes
import importlib
import json
import os
import pickle
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import classifier_ref as cr
import ref_harness as rh
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
clf = pkg.classifier
HEADER = os.path.join(ROOT, "include", "gcdm_classifier.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONFIGS = ["h128_l7_att", "h128_l7_attr", "h64_l2_att_attr", "h256_l1"]
Z = None


def _fixture(name):
    g = np.load(os.path.join(GOLDEN, f"classifier_{name}.npz"))
    F, H, L, att, attr = (int(v) for v in g["config"])
    W = synth.make_weights(cr.state_dict_shapes(F, H, L, bool(att), bool(attr)), seed=11)
    return g, (F, H, L, att, attr), W


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(gcdm_classifier_\w+)\s*\(([^)]*)\)\s*;", text):
        args = [a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
        out[m.group(1)] = len(args)
    return out


def test_header_declares_exactly_the_signature_table():
    decl = _declared()
    assert decl == {k: len(v) for k, v in native.CLASSIFIER_SIGNATURES.items()}
    assert not set(decl) & (set(native.OPS_EXPORTS) | set(native.MP_TRAIN_SIGNATURES) | set(native.OPTIM_SIGNATURES))
    text = open(HEADER).read()
    assert re.search(rf"#define GCDM_CLASSIFIER_MAX_NODES {native.CLASSIFIER_MAX_NODES}\b", text)
    assert re.search(rf"#define GCDM_CLASSIFIER_MAX_IN_NODE_NF {native.CLASSIFIER_MAX_IN_NODE_NF}\b", text)
    assert re.search(rf"#define GCDM_CLASSIFIER_MAX_HIDDEN_NF {native.CLASSIFIER_MAX_HIDDEN_NF}\b", text)
    assert native.CLASSIFIER_MAX_NODES >= 29            # QM9 with hydrogens


def test_header_and_kernels_are_library_dependencies():
    assert HEADER in native.OPS_HEADERS
    assert os.path.join(ROOT, "bio-diffusion_amd", "csrc", "gcdm_ops.classifier.hip.h") in native.OPS_HEADERS
    assert not [h for h in native.HEADERS if "classifier" in os.path.basename(h)]


@pytest.fixture(scope="module")
def lib():
    path = native.OPS_LIB_PATH
    if not os.path.exists(path):
        pytest.skip("libgcdm_ops.so not built (run __graft_entry__.build())")
    stale = [d for d in native.OPS_SOURCES + native.OPS_HEADERS if os.path.getmtime(d) > os.path.getmtime(path)]
    if stale:
        pytest.skip(f"libgcdm_ops.so is older than {stale} (run __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    for name, sig in native.CLASSIFIER_SIGNATURES.items():
        assert hasattr(lib, name), name
        getattr(lib, name).argtypes = sig
        getattr(lib, name).restype = native.CLASSIFIER_RESTYPES.get(name, ctypes.c_int)
    return lib


def test_library_exports_every_declared_entry(lib):
    assert lib.gcdm_classifier_workspace_bytes(2, 0, 5, 128, 7) == clf.LAUNCHES_PER_FORWARD


def test_header_is_c99_and_links_from_plain_c(lib, tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "gcdm_classifier.h"\n'
                   "int main(void) {\n"
                   "  long long a = (long long)gcdm_classifier_workspace_bytes(1, 0, 5, 128, 7);\n"
                   "  long long b = (long long)gcdm_classifier_workspace_bytes(1, 0, 5, 100, 7);\n"
                   '  printf("%lld %lld %s\\n", a, b, gcdm_classifier_last_error());\n'
                   "  return !(a > 0 && b == -1 && GCDM_CLASSIFIER_MAX_NODES >= 29);\n}\n")
    exe = tmp_path / "t"
    libdir = os.path.dirname(native.OPS_LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe),
                        "-L", libdir, "-l:libgcdm_ops.so", f"-Wl,-rpath,{libdir}", "-Wl,--allow-shlib-undefined"], text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], text=True, capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "multiple of 32" in r.stdout


def test_every_entry_refuses_bad_arguments_before_any_launch(lib):
    """Null pointers throughout: a call that got past its checks would fault, so every case must come back with -1 and a message."""
    ws, fw, pk = lib.gcdm_classifier_workspace_bytes, lib.gcdm_classifier_forward, lib.gcdm_classifier_pack

    def fwd(N=10, B=2, F=5, H=128, L=7, att=1, dbg=-1):
        return fw(Z, Z, Z, Z, Z, Z, Z, dbg, N, B, F, H, L, att, Z)

    cases = [(ws(0, 10, 5, 100, 7), "multiple of 32"), (ws(0, 10, 5, 288, 7), "256"), (ws(0, 10, 17, 128, 7), "16"), (ws(0, 10, 0, 128, 7), "16"),
             (ws(0, 10, 5, 128, 0), ">= 1"), (ws(5, 10, 5, 128, 7), "which"), (ws(0, -1, 5, 128, 7), "negative"),
             (fwd(H=96 + 1), "multiple of 32"), (fwd(F=17), "16"), (fwd(L=0), ">= 1"), (fwd(att=2), "0 or 1"), (fwd(N=-1), "negative"),
             (fwd(N=65, B=2), "32 atoms per molecule"), (fwd(dbg=8), "debug_layer"), (fwd(dbg=1), "h_debug"), (fwd(), "null"),
             (pk(Z, 80, 5, 128, 7, 1, 0, Z, Z), "null"), (pk(Z, 79, 5, 128, 7, 1, 0, Z, Z), "expected 80"), (pk(Z, 80, 5, 128, 7, 2, 0, Z, Z), "0 or 1"),
             (pk(Z, 80, 5, 64 + 8, 7, 1, 0, Z, Z), "multiple of 32")]
    for k, (status, word) in enumerate(cases):
        assert status == -1, k
    # the message names the limit (the last failing call's)
    assert ws(0, 10, 5, 288, 7) == -1 and "256" in lib.gcdm_classifier_last_error().decode()
    assert fwd(N=65, B=2) == -1 and "32 atoms per molecule" in lib.gcdm_classifier_last_error().decode()
    assert fwd(B=0, N=0) == 0                                # nothing to do: no launch
    assert ws(0, 1000, 5, 128, 7) >= 1000 * 128 * 4 and ws(0, 1000, 5, 128, 7) % 256 == 0
    assert ws(3, 0, 5, 128, 7) <= 160 * 1024 and ws(3, 0, 5, 256, 1) <= 160 * 1024         # LDS of a workgroup fits the CU
    assert ws(4, 0, 5, 128, 7) >= 2                           # a weight pass serves several molecules


@pytest.mark.parametrize("name", CONFIGS)
def test_state_dict_keys_and_shapes_equal_the_reference(name):
    g, (F, H, L, att, attr), W = _fixture(name)
    want = [(k, tuple(s)) for k, s in json.loads(str(g["state_dict"]))]
    model = clf.EGNN(in_node_nf=F, in_edge_nf=0, hidden_nf=H, device="cpu", act_fn=torch.nn.SiLU(), n_layers=L, coords_weight=1.0,
                     attention=att, node_attr=attr)
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == want
    assert not [k for k in model.state_dict() if "coord_mlp" in k]
    model.load_state_dict(W)                                 # synth weights are keyed by the same names


def test_constructor_refusals_name_the_limit():
    with pytest.raises(ValueError, match="multiple of 32 up to 256"):
        clf.EGNN(5, 0, 100, device="cpu")
    with pytest.raises(ValueError, match="multiple of 32 up to 256"):
        clf.EGNN(5, 0, 288, device="cpu")
    with pytest.raises(ValueError, match=r"1 \.\. 16"):
        clf.EGNN(17, 0, 128, device="cpu")
    with pytest.raises(ValueError, match="at least 1"):
        clf.EGNN(5, 0, 128, device="cpu", n_layers=0)
    with pytest.raises(NotImplementedError, match="in_edge_nf"):
        clf.EGNN(5, 2, 128, device="cpu")
    with pytest.raises(NotImplementedError, match="SiLU"):
        clf.EGNN(5, 0, 128, device="cpu", act_fn=torch.nn.ReLU())


def test_cpu_tensors_and_oversized_molecules_raise():
    model = clf.EGNN(5, 0, 32, device="cpu", n_layers=1)
    x, h0 = cr.make_batch([4, 3], 5, seed=1)
    with pytest.raises(ValueError, match="GPU only"):
        model.predict(x, h0, num_nodes=torch.tensor([4, 3]))
    xp, hp, nm, em, n = cr.to_padded(x, h0, [4, 3])
    with pytest.raises(ValueError, match="GPU only"):
        model(h0=hp, x=xp, edges=None, edge_attr=None, node_mask=nm, edge_mask=em, n_nodes=n)
    with pytest.raises(NotImplementedError, match="edge_attr"):
        model(h0=hp, x=xp, edges=None, edge_attr=torch.zeros(1), node_mask=nm, edge_mask=em, n_nodes=n)

    class FakeCuda(torch.Tensor):
        @property
        def is_cuda(self):
            return True
    big = torch.zeros(40, 3).as_subclass(FakeCuda)
    with pytest.raises(ValueError, match="up to 32 atoms"):
        model.predict(big, torch.zeros(40, 5).as_subclass(FakeCuda), num_nodes=torch.tensor([40]))
    with pytest.raises(ValueError, match="up to 32 atoms"):
        model(h0=torch.zeros(66, 5).as_subclass(FakeCuda), x=torch.zeros(66, 3).as_subclass(FakeCuda), node_mask=torch.ones(66, 1), n_nodes=33)


def test_get_classifier_round_trips_a_directory(tmp_path):
    shapes = cr.state_dict_shapes(5, 64, 2, True, True)
    W = synth.make_weights(shapes, seed=4)
    with open(tmp_path / "args.pickle", "wb") as f:
        pickle.dump(argparse.Namespace(nf=64, n_layers=2, attention=1, node_attr=1, lr=1e-3, property="alpha", exp_name="x", extra=[1, 2]), f)
    torch.save(W, tmp_path / "best_checkpoint.npy")
    model = clf.get_classifier(str(tmp_path), device="cpu")
    assert (model.hidden_nf, model.n_layers, model.attention, model.node_attr, model.in_node_nf) == (64, 2, True, True, 5)
    assert not model.training
    sd = model.state_dict()
    assert list(sd) == list(W) and all(torch.equal(sd[k], W[k]) for k in W)


class _Evil:
    def __reduce__(self):
        return (os.getcwd, ())


def test_unpickler_refuses_any_other_class(tmp_path):
    for k, obj in enumerate([_Evil(), argparse.Namespace(nf=_Evil()), {"a": torch.Size([1])}, argparse.ArgumentParser]):
        p = tmp_path / f"a{k}.pickle"
        with open(p, "wb") as f:
            pickle.dump(obj, f)
        with pytest.raises(pickle.UnpicklingError, match="only argparse.Namespace"):
            clf.load_classifier_args(str(p))
    p = tmp_path / "plain.pickle"
    with open(p, "wb") as f:
        pickle.dump({"nf": 64}, f)
    with pytest.raises(pickle.UnpicklingError, match="does not hold"):
        clf.load_classifier_args(str(p))


@pytest.mark.parametrize("name", CONFIGS)
def test_restatement_matches_the_reference_fp64(name):
    g, (F, H, L, att, attr), W = _fixture(name)
    sizes = [int(v) for v in g["num_nodes"]]
    pred, layers = cr.forward(W, torch.tensor(g["x"]), torch.tensor(g["one_hot"]), sizes, return_layers=True)
    assert (pred - torch.tensor(g["pred64"])).abs().max().item() <= 1e-12
    rows = int(g["layer_rows"])
    assert g["h_layers"].shape == (L + 1, rows, H)
    for k in range(L + 1):
        assert (layers[k][:rows] - torch.tensor(g["h_layers"][k])).abs().max().item() <= 1e-12, k
    # the fixture's own fp32-vs-fp64 distance is what the GPU bar scales: it must be a real fp32 rounding distance
    assert 1e-8 < float(g["gap"]) < 1e-5 and (torch.tensor(g["pred32"]).double() - torch.tensor(g["pred64"])).abs().max().item() == float(g["gap"])


@pytest.mark.parametrize("sizes", [[1, 2, 3, 29, 7], [5], [1], list(range(1, 33))])
@pytest.mark.parametrize("att,attr", [(1, 0), (0, 1)])
def test_ragged_restatement_equals_padded_restatement(sizes, att, attr):
    W = synth.make_weights(cr.state_dict_shapes(5, 32, 3, bool(att), bool(attr)), seed=2)
    x, h0 = cr.make_batch(sizes, 5, seed=9)
    a = cr.forward(W, x, h0, sizes)
    xp, hp, nm, em, n = cr.to_padded(x, h0, sizes, n_max=max(sizes) + 2)
    b = cr.forward_padded(W, xp, hp, nm, em, n)
    assert (a - b).abs().max().item() <= 1e-12


@pytest.mark.skipif(not rh.reference_available(), reason="the reference checkout is not on this machine")
@pytest.mark.parametrize("att,attr", [(1, 1), (0, 0)])
def test_restatement_against_the_imported_reference_on_fresh_inputs(att, attr):
    rh.install_stubs()
    src = importlib.import_module("src")
    sizes = [9, 1, 14, 2, 21]
    W = synth.make_weights(cr.state_dict_shapes(5, 64, 3, bool(att), bool(attr)), seed=23)
    x, h0 = cr.make_batch(sizes, 5, seed=31)
    model = src.EGNN(in_node_nf=5, in_edge_nf=0, hidden_nf=64, device="cpu", n_layers=3, coords_weight=1.0, attention=att, node_attr=attr)
    model.load_state_dict(W)
    model = model.double().eval()
    xp, hp, nm, em, n = cr.to_padded(x, h0, sizes)
    with torch.no_grad():
        ref = model(h0=hp.double(), x=xp.double(), edges=src.get_classifier_adj_matrix(n, len(sizes), "cpu", edges_dic={}), edge_attr=None,
                    node_mask=nm.double(), edge_mask=em.double(), n_nodes=n)
    assert (cr.forward(W, x, h0, sizes) - ref).abs().max().item() <= 1e-12


# ---- the inputs and the bar of tests/test_classifier_cabi_gpu.py ------------------------------------------------------------------------------
HOT_CASES = [(H, cr.INSTANTIATION_SIZES) for H in range(32, 257, 32)] + [(96, cr.group_sizes(1025))]


@pytest.mark.parametrize("H,sizes", HOT_CASES, ids=[f"H{H}-B{len(s)}" for H, s in HOT_CASES])
def test_hot_regime_leaves_the_linear_range_and_stays_representable(H, sizes):
    """Conditions on the inputs, not measurements of the kernel: every configuration the GPU tests run "hot"."""
    W, x, h0 = cr.make_regime("hot", 16, H, 2, 1, 1, sizes)
    assert not bool(((h0 == 0) | (h0 == 1)).any()) and W["gcl_0.att_mlp.0.weight"].abs().max() > 8 / np.sqrt(H)
    probe = {}
    p64 = cr.forward(W, x, h0, sizes, probe=probe)
    p32 = cr.forward(W, x, h0, sizes, dtype=torch.float32)
    assert bool(torch.isfinite(p32).all())
    stds = [float(g.std()) for g in probe["gate"]]
    beyond = [float((torch.cat((a, b)).abs() > 4).double().mean()) for a, b in zip(probe["pre0"], probe["pre2"])]
    rel = float((p32.double() - p64).abs().max() / p64.abs().max())
    print(f"hot H={H}: gate std per layer {stds}, share of edge_mlp pre-activations beyond 4 {beyond}, relative fp32 gap {rel:.2e}")
    assert len(stds) == 2 and min(stds) >= 0.1
    assert min(beyond) >= 0.05
    assert rel < 1e-4


def test_init_regime_is_the_near_linear_one():
    W, x, h0 = cr.make_regime("init", 16, 96, 2, 1, 1, cr.INSTANTIATION_SIZES)
    assert bool(((h0 == 0) | (h0 == 1)).all()) and all(torch.equal(v, w) for v, w in zip(W.values(), synth.make_weights(
        cr.state_dict_shapes(16, 96, 2, True, True), seed=11).values()))
    probe = {}
    cr.forward(W, x, h0, cr.INSTANTIATION_SIZES, probe=probe)
    assert max(float(g.std()) for g in probe["gate"]) < 0.05             # why "hot" exists: the gate is one number here


def test_size_lists_hold_the_named_pairs_and_edges():
    assert cr.INSTANTIATION_SIZES == [1, 2, 3, 4, 5, 8, 9, 16, 31, 32, 0, 7]
    s = cr.group_sizes(1025)
    assert len(s) == 1025 and len(s) % 2 == 1 and s == cr.group_sizes(1025)
    pairs = [(s[2 * k], s[2 * k + 1]) for k in range(len(s) // 2)]
    assert pairs[:7] == [(32, 32), (0, 32), (32, 0), (0, 0), (1, 1), (1, 32), (4, 5)] == cr.GROUP_PAIRS
    assert set(s) == set(range(33)) and sum(s) <= 32 * len(s)
    assert cr.offsets_of([3, 0, 2]) == [0, 3, 3, 5]


def test_the_bar_is_per_molecule_and_per_row():
    """A defect confined to the two-atom molecule that the batch-wide bar (20 x the batch's gap) lets through fails the per-molecule bar; the
    restatement's own fp32 run needs M <= 1; an entry left NaN fails."""
    sizes = list(range(1, 33))
    W, x, h0 = cr.make_regime("init", 5, 64, 2, 1, 0, sizes)
    ref = cr.references(W, x, h0, sizes)
    assert ref.pred64.dtype == torch.float64 and len(ref.layers64) == 3 and ref.layers32[2].shape == (sum(sizes), 64)
    assert torch.get_num_threads() >= 1 and bool((ref.pred_scale >= ref.pred64.abs() - 1e-12).all())
    failures, ratios = cr.compare(ref, pred=ref.pred32, layers=dict(enumerate(ref.layers32)))
    assert not failures and max(ratios.values()) <= 1.0 and set(ratios) == {"pred", "h0", "h1", "h2"}
    batch_gap = float((ref.pred32 - ref.pred64).abs().max())
    wrong = ref.pred32.clone()
    wrong[1] += 10 * batch_gap                                            # half the batch-wide bar of tests/test_classifier_gpu.py
    assert float((wrong - ref.pred64).abs().max()) <= 20 * batch_gap
    failures, ratios = cr.compare(ref, pred=wrong)
    assert len(failures) == 1 and "molecule 1 " in failures[0] and ratios["pred"] > cr.M_MAX
    h = ref.layers32[2].clone()
    h[2, 5] += 20 * float((ref.layers32[2] - ref.layers64[2]).abs()[2].max()) + 1e-5
    failures, ratios = cr.compare(ref, layers={2: h})
    assert len(failures) == 1 and "row 2 " in failures[0]
    h = ref.layers32[0].clone()
    h[7, 0] = float("nan")
    failures, ratios = cr.compare(ref, layers={0: h})
    assert failures and ratios["h0"] == float("inf")
    assert cr.compare(ref, pred=torch.full_like(ref.pred32, float("nan")))[0]
    assert set(cr.MARGINS) == {"init", "hot"} and cr.MARGINS["init"] == {}
    assert all(cr.M_DEFAULT <= m <= cr.M_MAX for reg in cr.MARGINS.values() for m in reg.values())


class _StubClassifier:
    """predict() returns a fixed table: property_mae's bookkeeping does not depend on the network."""

    def __init__(self, table):
        self.table, self.calls = table, 0

    def predict(self, x, one_hot, num_nodes=None):
        self.calls += 1
        return torch.tensor(self.table[self.calls - 1], dtype=torch.float32)


def test_property_mae_bookkeeping_against_a_hand_computed_case():
    # mean 10, mad 2.  batch 1 (3 molecules): pred (0, 1, -1) -> 10, 12, 8 vs labels 11, 12, 5: errors 1, 0, 3 -> 4/3
    #                  batch 2 (1 molecule):  pred 0.5 -> 11 vs label 9: error 2
    # weighted: (4/3 * 3 + 2 * 1) / 4 = 1.5  (the plain mean of the two batch losses would be 5/3)
    stub = _StubClassifier([[0.0, 1.0, -1.0], [0.5]])
    z = torch.zeros(1, 3)
    batches = [(z, z, torch.tensor([1, 1, 1]), torch.tensor([11.0, 12.0, 5.0])), (z, z, torch.tensor([1]), torch.tensor([[9.0]]))]
    mae, per = clf.property_mae(stub, batches, mean=10.0, mad=2.0, property="alpha", return_per_batch=True)
    assert mae == pytest.approx(1.5, abs=1e-6) and per == pytest.approx([4.0 / 3.0, 2.0], abs=1e-6)
    with pytest.raises(ValueError, match="no batch"):
        clf.property_mae(stub, [], 0.0, 1.0)


def test_model_has_the_conditional_evaluation_driver():
    model = pkg.QM9MoleculeGenerationDDPM(**pkg.default_cfgs("qm9"))
    with pytest.raises(Exception, match="conditional model"):
        model.evaluate_conditional(None, "alpha", 0.0, 1.0, iterations=1, batch_size=2, props_distr=object())
