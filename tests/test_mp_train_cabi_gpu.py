"""gcdm_mp_fwd / gcdm_mp_bwd (include/gcdm_mp_train.h) called directly through the C ABI on an MI355X, against oracle.message_passing under
fp64 autograd, on the graphs, shapes and values where the fused message layer could be wrong without tests/test_mp_train_gpu.py noticing.

Harness (run_fwd / run_bwd): every output sits in an `_Out` (NaN inside, sentinel guard words around it), the forward workspace, the tape and
the backward scratch are exactly gcdm_mp_workspace_bytes(which, ...) bytes inside a larger buffer, NaN-filled, with sentinel guards; rowptr,
colperm and colptr are built here on the CPU in plain torch (mp_train_ref.make_graph), not taken from ops.Graph.  A read of workspace no kernel
wrote poisons the result, a write past the advertised size breaks a guard.

The bar (mp_train_ref.compare) is measured, not fixed: per tensor and per row (nodes for agg / dh / dchi, edges for de / dxi),
max|got - ref64| <= M * max|ref32 - ref64| + 8 U max|ref64|, ref32 being the same oracle run in float32 on the CPU, on ONE thread (torch's fp32
sums split their work by thread count; with the thread count fixed the gap does not move with the host's cores).  M = 4 for 26 of the 36
tensors; the exceptions (mp_train_ref.MARGINS, none above 16; this table is their only rationale):

    tensor                                   M    measured (tensor / worst row)   reason
    dh                                       16   5.7 / 8.6                       the kernel sums dS0 over a node's edges first, then ONE K = 512
                                                                                  chain [row sums | column sums] . [W_i ; W_j]; the oracle does a
                                                                                  K = 256 product per edge and adds edges afterwards.  The two orders
                                                                                  emulated in fp32 on the CPU differ by 1.6x - 2.8x per tensor.
    message_fusion.k.scalar_out.bias,        16   5.3 (E = 40 870), 2.4 (E = 23 104)  column sums over all E edges: 16 split-K slices, each one
    message_fusion.k.vector_out_scale.bias                                        sequential chain of E / 16 terms; torch's fp32 column sum is blocked.
    scalar_message_attention.0.bias          16   6.5                             one number: its gap is a single draw, not a maximum over entries.

Every other tensor measured at most 2.7 (de, worst row; message_fusion.1.vector_down.weight 2.6).  Worst M needed per case on an MI355X, QM9 /
GEOM dims: fully connected [1] 1.2 / 1.4, [1, 1, 1] 0.6 / 0.9, [3] 0.3 / 1.8, [8] 3.9 / 2.7 (dh), [8, 8] 6.3 (attention bias) / 3.9 (dh),
[8, 1] 4.8 / 3.2 (dh), [1, 2, 7, 13, 9, 3] 4.3 / 2.4 (dh), [19] * 64 6.2 / 7.8 (dh), [181, 3, 90] 6.5 (attention bias); star_out 1.5 / 3.8,
star_in 0.6 / 0.4, random_sparse 5.2 / 3.4 (dh), chain 2.7 / 1.2 (dh); edge masks on [1, 2, 7, 13, 9, 3] 5.5 / 3.9 and on random_sparse
6.0 / 8.6 (dh); chi = xi = 0 2.5 / 4.3 (dh), with h x 100 1.0 / 2.5, their |vh| column blocks 0.7.

What a deliberately wrong library does to this file (arithmetic-only changes): colptr read as rowptr in k_mp_node_sum fails every
asymmetric graph; edge_mask ignored in k_mp_down_bwd fails every masked case; the first edge of every segment scaled by 0.999999 in k_mp_agg
fails the row check on the degree-1 graphs (chain, star_in, [1]); the norm's outer + 1e-8 dropped fails the |vh| column blocks of the
chi = xi = 0 case (M needed 424 - 729) and nothing else: under the whole-tensor bar it is invisible in fp32; __expf for expf in silu_f is NOT
caught: the worst ratio moves by about 1, within M.
"""
import ctypes as C
import importlib
import os
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mp_train_ref as R  # noqa: E402
import synth  # noqa: E402

pkg = importlib.import_module("bio-diffusion_amd")
ops = pkg.ops
pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U
GUARD = 64                         # guard words around every buffer the C ABI writes
CASES = ("qm9", "geom")            # edge dims (64, 16) and (16, 8)

MARGINS = R.MARGINS                # tensor -> M for the documented exceptions of the table in the docstring


def _lib():
    return pkg._native.load_ops()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Out:
    """`n` floats inside a larger device buffer: NaN inside (an entry the kernel does not write shows, and so does a read of a workspace entry
    nobody wrote), a finite sentinel in the GUARD words before and after (a stray write shows).  As test_ops_gpu._Out, with the guards
    compared on the device: the tapes here reach hundreds of MB."""
    SENTINEL = 12345.5

    def __init__(self, n):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * GUARD,), self.SENTINEL, dtype=torch.float32, device=DEV)
        self.inner = self.buf[GUARD:GUARD + self.n]
        self.inner.fill_(float("nan"))
        self.p = C.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def check(self):
        assert bool((self.buf[:GUARD] == self.SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == self.SENTINEL).all()), "write outside the buffer"

    def get(self):
        self.check()
        return self.inner.cpu()

    def bits(self):
        return self.inner.view(torch.int32).clone()


def _bytes(which, g, d):
    n = int(_lib().gcdm_mp_workspace_bytes(which, g.N, g.E, d["Se"], d["Ve"]))
    assert n >= 0 and n % 4 == 0
    return n // 4


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _dev_graph(g):
    if not hasattr(g, "dev"):
        g.dev = {k: getattr(g, k).to(DEV) for k in ("row", "col", "rowptr", "colperm", "colptr")}
    return g.dev


def _dev_weights(weights):
    ws = [weights[k].to(DEV).contiguous() for k in R.weight_keys()]
    return ws, (C.c_void_p * 30)(*[w.data_ptr() for w in ws])


def _mask_ptr(edge_mask):
    if edge_mask is None:
        return None, None
    mk = edge_mask.to(torch.uint8).to(DEV).contiguous()
    return mk, _ptr(mk)


def run_fwd(case, graph, inputs, weights, edge_mask, tape):
    """gcdm_mp_fwd -> (status, agg as an _Out of N * 352 floats, workspace as an _Out of exactly the advertised size)."""
    d = synth.DATASET_DIMS[case]
    gd = _dev_graph(graph)
    ws, wp = _dev_weights(weights)
    mk, mp = _mask_ptr(edge_mask)
    t = [x.to(DEV).contiguous() for x in (inputs.h, inputs.chi, inputs.e, inputs.xi, inputs.frames.reshape(-1, 9))]
    agg, work = _Out(graph.N * 352), _Out(_bytes(int(tape), graph, d))
    status = _lib().gcdm_mp_fwd(_ptr(t[0]), _ptr(t[1]), _ptr(t[2]), _ptr(t[3]), _ptr(gd["row"]), _ptr(gd["col"]), _ptr(gd["rowptr"]), _ptr(t[4]), mp, wp,
                                agg.p, work.p, int(tape), graph.N, graph.E, d["Se"], d["Ve"], _stream())
    torch.cuda.synchronize()
    agg.check()
    work.check()
    del ws, mk
    return status, agg, work


BWD_OUTS = ("dh", "dvnode", "de", "dxi", "dweights")


def run_bwd(case, graph, inputs, weights, edge_mask, tape, dagg):
    """gcdm_mp_bwd on the tape of run_fwd(..., tape=1) -> (status, name -> _Out for dh, dvnode, de, dxi, dweights, scratch)."""
    d = synth.DATASET_DIMS[case]
    gd = _dev_graph(graph)
    ws, wp = _dev_weights(weights)
    mk, mp = _mask_ptr(edge_mask)
    h, fr, dg = inputs.h.to(DEV).contiguous(), inputs.frames.reshape(-1, 9).to(DEV).contiguous(), dagg.to(torch.float32).to(DEV).contiguous()
    N, E = graph.N, graph.E
    outs = dict(dh=_Out(N * 256), dvnode=_Out(N * 96), de=_Out(E * d["Se"]), dxi=_Out(E * d["Ve"] * 3), dweights=_Out(_bytes(3, graph, d)),
                scratch=_Out(_bytes(2, graph, d)))
    status = _lib().gcdm_mp_bwd(_ptr(dg), _ptr(h), _ptr(gd["row"]), _ptr(gd["col"]), _ptr(gd["rowptr"]), _ptr(gd["colptr"]), _ptr(gd["colperm"]), _ptr(fr),
                                mp, wp, tape.p, outs["scratch"].p, outs["dh"].p, outs["dvnode"].p, outs["de"].p, outs["dxi"].p, outs["dweights"].p,
                                N, E, d["Se"], d["Ve"], _stream())
    torch.cuda.synchronize()
    for o in outs.values():
        o.check()
    tape.check()
    del ws, mk
    return status, outs


def _named(case, graph, weights, agg, outs):
    """The 36 tensors by name from the raw outputs."""
    d = synth.DATASET_DIMS[case]
    N, E = graph.N, graph.E
    a = agg.get().view(N, 352)
    got = {"agg_s": a[:, :256], "agg_v": a[:, 256:].reshape(N, 32, 3), "dh": outs["dh"].get().view(N, 256), "dchi": outs["dvnode"].get().view(N, 32, 3),
           "de": outs["de"].get().view(E, d["Se"]), "dxi": outs["dxi"].get().view(E, d["Ve"], 3)}
    dw, o = outs["dweights"].get(), 0
    for k in R.weight_keys():
        n = weights[k].numel()
        got[k] = dw[o:o + n].view(weights[k].shape)
        o += n
    assert o == dw.numel()
    return got


def _fwd_bwd(case, graph, inputs, weights, r, edge_mask=None):
    st, agg, tape = run_fwd(case, graph, inputs, weights, edge_mask, 1)
    assert st == 0
    st, outs = run_bwd(case, graph, inputs, weights, edge_mask, tape, r)
    assert st == 0
    return agg, tape, outs


def _check_case(case, graph, inputs=None, edge_mask=None, ref_mask="same", seed=5):
    """Forward with a tape + backward against fp64 under the measured bar, and the tape-free forward bitwise against the taped one."""
    weights, d = R.layer_weights(case)
    inputs = inputs if inputs is not None else R.make_inputs(d, graph, seed=seed)
    r = R.make_r(graph.N)
    ref64, ref32 = R.references(weights, d, inputs, graph, r, edge_mask if ref_mask == "same" else ref_mask)
    agg, tape, outs = _fwd_bwd(case, graph, inputs, weights, r, edge_mask)
    got = _named(case, graph, weights, agg, outs)
    st, agg0, _ = run_fwd(case, graph, inputs, weights, edge_mask, 0)
    assert st == 0
    assert torch.equal(agg0.bits(), agg.bits()), "the tape-free forward differs from the taped one"
    what = f"{case} {graph.name} N={graph.N} E={graph.E}: "
    failures, ratios = R.compare(got, ref64, ref32, MARGINS, what)
    name, worst = R.worst_ratio(ratios)
    print(f"\nMEASURED {what}worst M needed {worst:.3g} ({name}); tensor / row: " +
          ", ".join(f"{k}={v[0]:.2f}/{v[1]:.2f}" for k, v in ratios.items() if max(v) > 1))
    assert not failures, "\n".join(failures)
    return got, ref64, ref32


# ---- C. graphs and shapes ----------------------------------------------------------------------------------------------------------------
FC_SIZES = [[1], [1, 1, 1], [3], [8], [8, 8], [8, 1], [1, 2, 7, 13, 9, 3], [19] * 64]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("sizes", FC_SIZES, ids=lambda s: "x".join(map(str, s)) if len(s) < 8 else f"{s[0]}x{len(s)}")
def test_fully_connected_against_fp64(case, sizes):
    """E = 1, E % 4 = 3 and 1, one GEMM tile, a tile multiple, a tile + 1, the ragged case, the training batch (N >= 256: every split-K slice
    of the W_i / W_j gradients holds rows)."""
    g = R.fc_graph(sizes)
    assert g.E == sum(n * n for n in sizes)
    _check_case(case, g)


def test_geom_largest_molecule_against_fp64():
    """181-edge segments (GEOM's largest molecule) next to 3- and 90-edge ones; N = 274, E = 40 870."""
    g = R.fc_graph([181, 3, 90])
    assert (g.N, g.E) == (274, 40870)
    _check_case("geom", g)


def _asym(name):
    return dict(star_out=R.star_out, star_in=R.star_in, random_sparse=R.random_sparse, chain=R.chain)[name]()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", ["star_out", "star_in", "random_sparse", "chain"])
def test_asymmetric_graph_against_fp64(case, name):
    """rowptr != colptr: nodes without outgoing edges, without incoming edges, without any; duplicate edges; a 69-edge column segment."""
    g = _asym(name)
    assert not torch.equal(g.rowptr, g.colptr)
    got, _, _ = _check_case(case, g)
    if name == "star_out":
        assert g.rowptr[1:].eq(g.E).all() and not bool(got["agg_s"][1:].any()) and not bool(got["agg_v"][1:].any())      # exactly 0
    if name == "chain":
        assert g.E == 129 and not bool(got["agg_s"][-1].any())


def _masks(g):
    gen = torch.Generator().manual_seed(23)
    return {"random": torch.rand(g.E, generator=gen) < 0.5, "one_way": g.row >= g.col, "all_off": torch.zeros(g.E, dtype=torch.bool)}


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("which", ["random", "one_way", "all_off"])
@pytest.mark.parametrize("name", ["fc", "random_sparse"])
def test_edge_mask_through_the_c_abi_against_fp64(case, which, name):
    """edge_mask is per edge: about half off at random, off for (i, j) but on for (j, i), all off (fp64 with zero frames)."""
    g = R.fc_graph([1, 2, 7, 13, 9, 3]) if name == "fc" else R.random_sparse()
    mask = _masks(g)[which]
    if which == "random":
        assert 0.35 * g.E < int(mask.sum()) < 0.65 * g.E
    if which == "one_way":
        assert bool((~mask).any()) and bool(mask.any())
    _check_case(case, g, edge_mask=mask)


@pytest.mark.parametrize("case", CASES)
def test_all_on_mask_equals_null_mask_bitwise(case):
    g = R.random_sparse()
    weights, d = R.layer_weights(case)
    inputs, r = R.make_inputs(d, g), R.make_r(g.N)
    on = torch.ones(g.E, dtype=torch.bool)
    a_agg, _, a = _fwd_bwd(case, g, inputs, weights, r, None)
    b_agg, _, b = _fwd_bwd(case, g, inputs, weights, r, on)
    assert torch.equal(a_agg.bits(), b_agg.bits())
    for k in BWD_OUTS:
        assert torch.equal(a[k].bits(), b[k].bits()), k
    _check_case(case, g, edge_mask=on, ref_mask=None)


def _spre0(weights, d, g, inp):
    """S_pre of msg0 in fp64 for chi = 0 and xi = 0, restated: vh = 0, so |vh| = sqrt(1e-8) + 1e-8 and the frame scalars are 0."""
    W, b = weights["message_fusion.0.scalar_out.weight"].double(), weights["message_fusion.0.scalar_out.bias"].double()
    H0 = (2 * 32 + d["Ve"]) // 4
    merged = torch.cat((inp.h[g.row].double(), inp.e.double(), inp.h[g.col].double(), torch.full((g.E, H0), 1e-8 ** 0.5 + 1e-8, dtype=torch.float64),
                        torch.zeros(g.E, 9, dtype=torch.float64)), dim=1)
    return merged @ W.T + b


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("h_scale", [1.0, 100.0], ids=["unit_h", "saturating_h"])
def test_degenerate_vectors_and_saturated_activations(case, h_scale):
    """[5, 4] fully connected with chi = 0 and xi = 0: every vector norm of all four GCPs sits at its regularised minimum sqrt(1e-8) + 1e-8 and
    the backward's t / sqrt(. + 1e-8) is at its largest.  With h x 100, msg0's S_pre passes +-30 and +-90 as well: silu and sigmoid saturated,
    expf(-x) overflowing to inf on the negative side.  The |vh| columns of every scalar_out.weight gradient are sum_e dS_pre * |vh| with
    |vh| = 1.0001e-4 throughout: they are 1e-4 of their tensor's largest entry, so they are also compared on their own, as a block -- the only
    place where the outer + 1e-8 of the norm (1e-4 of these columns) is visible in fp32."""
    weights, d = R.layer_weights(case)
    g = R.fc_graph([5, 4])
    inp = R.make_inputs(d, g, seed=17)
    inp.chi.zero_()
    inp.xi.zero_()
    inp.h.mul_(h_scale)
    if h_scale > 1:
        spre = _spre0(weights, d, g, inp)
        assert float(spre.max()) > 90 and float(spre.min()) < -90
        assert int(((spre.abs() > 30) & (spre.abs() < 90)).sum()) > 100
    got, ref64, ref32 = _check_case(case, g, inputs=inp)                      # the references are asserted finite inside
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    # Column layout of scalar_out.weight (include/gcdm_mp_train.h, checked shape by shape in ops._mp_shapes): msg0 [h_i 256 | e Se | h_j 256 | |vh| H0 | q 9]
    # with H0 = (2 * 32 + Ve) / 4 (bottleneck 4); msg1-3 [s 256 | |vh| 8 | q 9].  The asserts on the widths keep the block on the |vh| columns.
    H0 = (2 * 32 + d["Ve"]) // 4
    assert weights["message_fusion.0.scalar_out.weight"].shape[1] == 2 * 256 + d["Se"] + H0 + 9 and weights["message_fusion.0.vector_down.weight"].shape[0] == H0
    assert weights["message_fusion.1.scalar_out.weight"].shape[1] == 256 + 8 + 9 and weights["message_fusion.1.vector_down.weight"].shape[0] == 8
    failures = []
    for k in range(4):
        name = f"message_fusion.{k}.scalar_out.weight"
        lo, hk = (2 * 256 + d["Se"], H0) if k == 0 else (256, 8)
        blk = [{name: t[name][:, lo:lo + hk]} for t in (got, ref64, ref32)]
        assert float(blk[1][name].abs().max()) > 0
        f, ratio = R.compare(blk[0], blk[1], blk[2], what=f"{case} |vh| columns of ", names=(name,))
        print(f"MEASURED {case} h x {h_scale:g} |vh| columns of {name}: M needed {ratio[name][0]:.3g}")
        failures += f
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N", [0, 5])
def test_empty_work_writes_nothing(case, N):
    weights, d = R.layer_weights(case)
    g = R.make_graph("empty", N, torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    inp = R.make_inputs(d, g)
    for tape in (0, 1):
        st, agg, work = run_fwd(case, g, inp, weights, None, tape)
        assert st == 0 and bool(torch.isnan(agg.get()).all()) and bool(torch.isnan(work.inner).all())
    st, outs = run_bwd(case, g, inp, weights, None, work, torch.zeros(N, 352))
    assert st == 0
    for k, o in outs.items():
        assert bool(torch.isnan(o.get()).all()), k
    # through the wrapper: the zero sum and zero gradients of the right shapes
    graph = ops.Graph(torch.zeros(2, 0, dtype=torch.int64, device=DEV), N)
    leaves = [t.to(DEV).requires_grad_(True) for t in (inp.h, inp.chi, inp.e, inp.xi)]
    ws = [weights[k].to(DEV).requires_grad_(True) for k in R.weight_keys()]
    a_s, a_v = ops.message_layer(*leaves, inp.frames.to(DEV), graph, ws)
    assert tuple(a_s.shape) == (N, 256) and tuple(a_v.shape) == (N, 32, 3) and not bool(a_s.any()) and not bool(a_v.any())
    (a_s.sum() + a_v.sum()).backward()
    for t in leaves + ws:
        assert t.grad is not None and t.grad.shape == t.shape and not bool(t.grad.any())


# ---- D. contracts of the header ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random_sparse", "batch"])
def test_backward_leaves_the_tape_alone_and_repeats_bitwise(name):
    """The tape is read-only in the backward; a second backward on the same tape, fresh NaN-filled outputs and scratch, gives the same bits;
    so does a second forward (dweights included: the split-K reduction order is fixed)."""
    case = "qm9"
    g = R.random_sparse() if name == "random_sparse" else R.fc_graph([19] * 64)
    weights, d = R.layer_weights(case)
    inputs, r = R.make_inputs(d, g), R.make_r(g.N)
    agg, tape, first = _fwd_bwd(case, g, inputs, weights, r)
    before = tape.bits()
    st, second = run_bwd(case, g, inputs, weights, None, tape, r)
    assert st == 0
    assert torch.equal(tape.bits(), before), "gcdm_mp_bwd wrote to the tape"
    for k in BWD_OUTS:
        assert not bool(torch.isnan(first[k].inner).any()), k
        assert torch.equal(first[k].bits(), second[k].bits()), k
    del second, before
    st, agg2, tape2 = run_fwd(case, g, inputs, weights, None, 1)
    assert st == 0 and torch.equal(agg.bits(), agg2.bits())
    st, third = run_bwd(case, g, inputs, weights, None, tape2, r)
    assert st == 0
    for k in BWD_OUTS:
        assert torch.equal(first[k].bits(), third[k].bits()), k


@pytest.mark.parametrize("case", CASES)
def test_a_molecule_computes_the_same_bits_alone_and_inside_a_batch(case):
    """The rows of agg, dh, dchi, de, dxi of the molecule [13]: alone, and as the fourth molecule of [1, 2, 7, 13, 9, 3] (node offset 10, edge
    offset 54, so its rows sit elsewhere in every 64-row GEMM tile and 4-edge workgroup).  Every one of them is a GEMM row (accumulation over K
    only) or a fixed-order segment sum, and a stable argsort keeps a molecule's relative column order."""
    weights, d = R.layer_weights(case)
    big = R.fc_graph([1, 2, 7, 13, 9, 3])
    inp, r = R.make_inputs(d, big), R.make_r(big.N)
    n0, n1, e0, e1 = 10, 23, 54, 54 + 169
    assert bool((big.row[e0:e1] >= n0).all()) and bool((big.row[e0:e1] < n1).all()) and int(big.rowptr[n0]) == e0 and int(big.rowptr[n1]) == e1
    small = R.make_graph("fc[13]", 13, big.row[e0:e1] - n0, big.col[e0:e1] - n0)
    sub = SimpleNamespace(h=inp.h[n0:n1], chi=inp.chi[n0:n1], e=inp.e[e0:e1], xi=inp.xi[e0:e1], frames=inp.frames[e0:e1])
    agg_b, _, out_b = _fwd_bwd(case, big, inp, weights, r)
    agg_s, _, out_s = _fwd_bwd(case, small, sub, weights, r[n0:n1])
    nd = dict(dh=256, dvnode=96)
    assert torch.equal(agg_b.bits().view(big.N, 352)[n0:n1], agg_s.bits().view(13, 352))
    for k, w in nd.items():
        assert torch.equal(out_b[k].bits().view(big.N, w)[n0:n1], out_s[k].bits().view(13, w)), k
    for k, w in dict(de=d["Se"], dxi=3 * d["Ve"]).items():
        assert torch.equal(out_b[k].bits().view(big.E, w)[e0:e1], out_s[k].bits().view(169, w)), k


@pytest.mark.parametrize("name", ["random_sparse", "star_in"])
def test_graph_col_order_equals_the_cpu_construction(name):
    g = _asym(name)
    G = ops.Graph(torch.stack((g.row, g.col)).to(DEV), g.N)
    perm, colptr = G.col_order()
    assert colptr.dtype == torch.int32 and G.rowptr.dtype == torch.int32
    assert torch.equal(G.rowptr.cpu(), g.rowptr) and torch.equal(perm.cpu(), g.colperm) and torch.equal(colptr.cpu(), g.colptr)


def _ops_operands(g, inp, weights, r, grad_inputs=(True, True, True, True), grad_weights=True, views=False):
    """Every operand of ops.message_layer on the device: leaves, frames, the Graph with its column order built, weights, r."""
    if views:      # h a column slice of a wider tensor, chi a permuted view, e every second row of a taller tensor
        wide = torch.zeros(g.N, 300)
        wide[:, 20:276] = inp.h
        tall = torch.zeros(2 * g.E, inp.e.shape[1])
        tall[::2] = inp.e
        leaves = [wide.to(DEV)[:, 20:276], inp.chi.permute(2, 0, 1).contiguous().to(DEV).permute(1, 2, 0), tall.to(DEV)[::2], inp.xi.to(DEV)]
        assert not leaves[0].is_contiguous() and not leaves[1].is_contiguous() and not leaves[2].is_contiguous()
        leaves = [t.detach() for t in leaves]
    else:
        leaves = [t.to(DEV).clone() for t in (inp.h, inp.chi, inp.e, inp.xi)]
    for t, need in zip(leaves, grad_inputs):
        t.requires_grad_(need)
    ws = [weights[k].to(DEV).clone().requires_grad_(grad_weights) for k in R.weight_keys()]
    G = ops.Graph(torch.stack((g.row, g.col)).to(DEV), g.N)
    G.col_order()
    return SimpleNamespace(leaves=leaves, frames=inp.frames.to(DEV), G=G, ws=ws, r=r.to(DEV))


def _call_ops(o):
    """ops.message_layer forward + backward of sum(agg . r) on operands already on the device: no host-to-device copy, no synchronisation.
    -> (agg_s, agg_v, input grads, weight grads)."""
    a_s, a_v = ops.message_layer(*o.leaves, o.frames, o.G, o.ws)
    ((a_s * o.r[:, :256]).sum() + (a_v * o.r[:, 256:].reshape(-1, 32, 3)).sum()).backward()
    return a_s.detach(), a_v.detach(), [t.grad for t in o.leaves], [w.grad for w in o.ws]


def _via_ops(case, g, inp, weights, r, **kw):
    return _call_ops(_ops_operands(g, inp, weights, r, **kw))


def _setup_ops(case="qm9"):
    weights, d = R.layer_weights(case)
    g = R.random_sparse()
    return weights, d, g, R.make_inputs(d, g), R.make_r(g.N)


def test_wrapper_agrees_bitwise_with_the_direct_calls():
    """ops.message_layer is the same two C calls: on an asymmetric graph its results are the direct calls' bits (so its column order is right)."""
    weights, d, g, inp, r = _setup_ops()
    agg, _, outs = _fwd_bwd("qm9", g, inp, weights, r)
    got = _named("qm9", g, weights, agg, outs)
    a_s, a_v, gi, gw = _via_ops("qm9", g, inp, weights, r)
    assert torch.equal(a_s.cpu(), got["agg_s"]) and torch.equal(a_v.cpu(), got["agg_v"])
    for k, t in zip(("dh", "dchi", "de", "dxi"), gi):
        assert torch.equal(t.cpu(), got[k]), k
    for k, t in zip(R.weight_keys(), gw):
        assert torch.equal(t.cpu(), got[k]), k


def test_frozen_weights_and_h_only_gradients():
    weights, d, g, inp, r = _setup_ops()
    full = _via_ops("qm9", g, inp, weights, r)
    frozen = _via_ops("qm9", g, inp, weights, r, grad_weights=False)
    assert all(w is None for w in frozen[3])
    for a, b in zip(full[2], frozen[2]):
        assert torch.equal(a, b)
    h_only = _via_ops("qm9", g, inp, weights, r, grad_inputs=(True, False, False, False), grad_weights=False)
    assert torch.equal(h_only[2][0], full[2][0]) and all(t is None for t in h_only[2][1:]) and all(w is None for w in h_only[3])
    assert torch.equal(h_only[0], full[0]) and torch.equal(h_only[1], full[1])


def test_non_contiguous_inputs_give_the_bits_of_their_contiguous_copies():
    weights, d, g, inp, r = _setup_ops("geom")
    a = _via_ops("geom", g, inp, weights, r)
    b = _via_ops("geom", g, inp, weights, r, views=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for x, y in zip(a[2] + a[3], b[2] + b[3]):
        assert x.shape == y.shape and torch.equal(x, y)


def test_non_default_stream_behind_a_long_kernel():
    """Every operand is on the device before the side stream is entered, so nothing inside the block waits on the host: the two C calls are
    enqueued while the matmuls still run, and h does not exist until the stream reaches it.  A launch on another stream would read it early."""
    weights, d, g, inp, r = _setup_ops()
    want = _via_ops("qm9", g, inp, weights, r)
    want = [t.cpu() for t in (want[0], want[1], *want[2], *want[3])]
    o = _ops_operands(g, inp, weights, r)
    hd = o.leaves[0].detach()
    big = torch.randn(6144, 6144, device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(s):
        for _ in range(12):
            big = big @ big * 1e-4        # a long queue on s
        o.leaves[0] = (hd + 0).requires_grad_(True)      # h produced on s, behind the queue
        got = _call_ops(o)
        out = [t.to("cpu", non_blocking=True) for t in (got[0], got[1], *got[2], *got[3])]
        done.record(s)
    done.synchronize()                     # this stream only: no device-wide sync
    assert len(out) == len(want) == 36
    for a, b in zip(out, want):
        assert torch.equal(a, b)
