"""gcdm_mp_tile_fwd / gcdm_mp_tile_bwd (include/gcdm_mp_tile.h) called directly through the C ABI on an MI355X, against oracle.message_passing
under fp64 autograd, with the discipline of tests/test_mp_train_cabi_gpu.py: every output, the forward workspace, the tape and the backward
scratch are NaN-filled at exactly the size gcdm_mp_tile_workspace_bytes advertises, between guard words that must be intact afterwards
(that file's `_Out`), and the CSR / column order comes from mp_train_ref.make_graph on the CPU.

The bar is mp_train_ref.compare's, unchanged: per tensor and per row max|got - ref64| <= M max|ref32 - ref64| + 8 * 2^-24 max|ref64|, M from
mp_train_ref.MARGINS / M_DEFAULT (in bf16x6 mode M = 4 for every tensor, as tests/test_matrix_mode_cabi_gpu.py holds the fused entries).  No
exception is added here.  A problem (graph, inputs, fp64 and fp32 references) is built once per process (_problem) and never modified.

Cases: the smallest that reach every branch of the two tile kernels -- E = 1, 9, 64 (exactly one 64-row tile), 65 (tile + 1), 313 (five tiles,
ragged), both edge-dim cases (msg0's K = 93 / 43: a partial last k-block and a partial last quadruple of WR0's rows), asymmetric graphs (nodes
without edges, duplicate edges, colptr != rowptr), a per-edge mask, chi = xi = 0 with saturated activations.

Crossed entries: the tape of gcdm_mp_tile_fwd handed to gcdm_mp_bwd and the tape of gcdm_mp_fwd handed to gcdm_mp_tile_bwd are held to the same
bar, so a defect shows in one kernel's half only.

Bits against the "fused" entries in fp32 mode (test_bits_against_the_fused_entries prints every comparison), as measured on an MI355X:
  * forward: agg and every field of the tape (S_pre, gate, X, the vector states, the final states, ...) carry gcdm_mp_fwd's bits -- asserted.
  * backward: dh, dvnode, de, dxi and dweights do NOT.  The first tensor that differs is dgate (about 11 % of its entries, 1 - 32 ulp at msg3;
    dup and silu(S_pre) of the same GCP are equal): dgate = (g0 u0 + g1 u1 + g2 u2) sg (1 - sg), and the compiler contracts the three-term sum
    differently where it stands in k_mp_vout_bwd and where it is inlined into the tile body's operand load (which of the two packed products
    is fused into the FMA with the third: (g2 u2 + g1 u1) + g0 u0 there, (g2 u2 + g0 u0) + g1 u1 here).  Both are roundings of the same
    expression; everything downstream inherits the last-place difference.  The kernel is not bent to force equality: the backward is held to
    the fp64 bar, on its own and crossed with the other path's forward.
"""
import functools
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
import test_mp_train_cabi_gpu as H  # noqa: E402  (its harness: _Out, the device copies, _named)

pkg = importlib.import_module("bio-diffusion_amd")
ops = pkg.ops
pytestmark = pytest.mark.gpu
CASES = H.CASES
BWD_OUTS = H.BWD_OUTS
ENTRIES = {"fused": ("gcdm_mp_workspace_bytes", "gcdm_mp_fwd", "gcdm_mp_bwd"),
           "tiled": ("gcdm_mp_tile_workspace_bytes", "gcdm_mp_tile_fwd", "gcdm_mp_tile_bwd")}


def _bytes(path, which, g, d):
    n = int(getattr(H._lib(), ENTRIES[path][0])(which, g.N, g.E, d["Se"], d["Ve"]))
    assert n >= 0 and n % 4 == 0
    return n // 4


def run_fwd(path, case, graph, inputs, weights, edge_mask, tape):
    """The forward entry of `path` -> (status, agg as an _Out of N * 352 floats, workspace as an _Out of exactly the advertised size)."""
    d = synth.DATASET_DIMS[case]
    gd = H._dev_graph(graph)
    ws, wp = H._dev_weights(weights)
    mk, mp = H._mask_ptr(edge_mask)
    t = [x.to(H.DEV).contiguous() for x in (inputs.h, inputs.chi, inputs.e, inputs.xi, inputs.frames.reshape(-1, 9))]
    agg, work = H._Out(graph.N * 352), H._Out(_bytes(path, int(tape), graph, d))
    p = H._ptr
    status = getattr(H._lib(), ENTRIES[path][1])(p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(gd["row"]), p(gd["col"]), p(gd["rowptr"]), p(t[4]), mp, wp, agg.p,
                                                 work.p, int(tape), graph.N, graph.E, d["Se"], d["Ve"], H._stream())
    torch.cuda.synchronize()
    agg.check()
    work.check()
    del ws, mk
    return status, agg, work


def run_bwd(path, case, graph, inputs, weights, edge_mask, tape, dagg):
    """The backward entry of `path` on a tape -> (status, name -> _Out for dh, dvnode, de, dxi, dweights, scratch)."""
    d = synth.DATASET_DIMS[case]
    gd = H._dev_graph(graph)
    ws, wp = H._dev_weights(weights)
    mk, mp = H._mask_ptr(edge_mask)
    h, fr = inputs.h.to(H.DEV).contiguous(), inputs.frames.reshape(-1, 9).to(H.DEV).contiguous()
    dg = dagg.to(torch.float32).to(H.DEV).contiguous()
    N, E = graph.N, graph.E
    outs = dict(dh=H._Out(N * 256), dvnode=H._Out(N * 96), de=H._Out(E * d["Se"]), dxi=H._Out(E * d["Ve"] * 3), dweights=H._Out(_bytes(path, 3, graph, d)),
                scratch=H._Out(_bytes(path, 2, graph, d)))
    p = H._ptr
    status = getattr(H._lib(), ENTRIES[path][2])(p(dg), p(h), p(gd["row"]), p(gd["col"]), p(gd["rowptr"]), p(gd["colptr"]), p(gd["colperm"]), p(fr), mp, wp,
                                                 tape.p, outs["scratch"].p, outs["dh"].p, outs["dvnode"].p, outs["de"].p, outs["dxi"].p,
                                                 outs["dweights"].p, N, E, d["Se"], d["Ve"], H._stream())
    torch.cuda.synchronize()
    for o in outs.values():
        o.check()
    tape.check()
    del ws, mk
    return status, outs


def _fwd_bwd(P, fwd="tiled", bwd="tiled", edge_mask="own"):
    mask = P.mask if isinstance(edge_mask, str) else edge_mask
    st, agg, tape = run_fwd(fwd, P.case, P.g, P.inp, P.weights, mask, 1)
    assert st == 0
    st, outs = run_bwd(bwd, P.case, P.g, P.inp, P.weights, mask, tape, P.r)
    assert st == 0
    return agg, tape, outs


# ---- the problems: built once, shared, never modified --------------------------------------------------------------------------------------
GRAPHS = {"1": lambda: R.fc_graph([1]), "3": lambda: R.fc_graph([3]), "8": lambda: R.fc_graph([8]), "8x1": lambda: R.fc_graph([8, 1]),
          "ragged": lambda: R.fc_graph([1, 2, 7, 13, 9, 3]), "5x4": lambda: R.fc_graph([5, 4]), "star_in": R.star_in, "star_out": R.star_out,
          "random_sparse": R.random_sparse}
EDGES = {"1": 1, "3": 9, "8": 64, "8x1": 65, "ragged": 313, "5x4": 41, "star_in": 69, "star_out": 69, "random_sparse": 2000}


@functools.lru_cache(maxsize=None)
def _graph(name):
    g = GRAPHS[name]()
    assert g.E == EDGES[name]
    return g


@functools.lru_cache(maxsize=None)
def _problem(case, gname, variant="plain"):
    """variant: plain | masked (about half of the edges off, per edge) | saturated (chi = xi = 0, h x 100: every vector norm at its regularised
    minimum, silu and sigmoid saturated on both sides)."""
    weights, d = R.layer_weights(case)
    g = _graph(gname)
    inp = R.make_inputs(d, g, seed=17 if variant == "saturated" else 5)
    mask = None
    if variant == "masked":
        mask = torch.rand(g.E, generator=torch.Generator().manual_seed(23)) < 0.5
        assert 0.35 * g.E < int(mask.sum()) < 0.65 * g.E
    if variant == "saturated":
        inp.chi.zero_()
        inp.xi.zero_()
        inp.h.mul_(100.0)
    r = R.make_r(g.N)
    ref64, ref32 = R.references(weights, d, inp, g, r, mask)
    return SimpleNamespace(case=case, d=d, g=g, weights=weights, inp=inp, mask=mask, r=r, ref64=ref64, ref32=ref32,
                           what=f"{case} {g.name} {variant} N={g.N} E={g.E}: ")


def _hold_to_the_bar(P, agg, outs, margins=None, tag=""):
    got = H._named(P.case, P.g, P.weights, agg, outs)
    failures, ratios = R.compare(got, P.ref64, P.ref32, R.MARGINS if margins is None else margins, P.what + tag)
    name, worst = R.worst_ratio(ratios)
    print(f"\nMEASURED {P.what}{tag}worst M needed {worst:.3g} ({name}); tensor / row: " +
          ", ".join(f"{k}={v[0]:.2f}/{v[1]:.2f}" for k, v in ratios.items() if max(v) > 1))
    assert not failures, "\n".join(failures)
    return got


def _check(P, margins=None):
    """Tiled forward with a tape + tiled backward against fp64 under the bar; the tape-free forward bitwise against the taped one on agg."""
    agg, tape, outs = _fwd_bwd(P)
    got = _hold_to_the_bar(P, agg, outs, margins)
    st, agg0, _ = run_fwd("tiled", P.case, P.g, P.inp, P.weights, P.mask, 0)
    assert st == 0
    assert torch.equal(agg0.bits(), agg.bits()), "the tape-free forward differs from the taped one"
    return got


# ---- against fp64 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("gname", ["1", "3", "8", "8x1", "ragged"])
def test_fully_connected_against_fp64(case, gname):
    """E = 1, 9, 64 (exactly one row tile), 65 (tile + 1), 313; msg0's K = 93 (qm9) and 43 (geom)."""
    _check(_problem(case, gname))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("gname", ["star_in", "star_out", "random_sparse"])
def test_asymmetric_graph_against_fp64(case, gname):
    P = _problem(case, gname)
    assert not torch.equal(P.g.rowptr, P.g.colptr)
    got = _check(P)
    if gname == "star_out":
        assert not bool(got["agg_s"][1:].any()) and not bool(got["agg_v"][1:].any())      # nodes without outgoing edges: exactly 0


@pytest.mark.parametrize("case", CASES)
def test_per_edge_mask_against_fp64(case):
    _check(_problem(case, "ragged", "masked"))


@pytest.mark.parametrize("case", CASES)
def test_degenerate_vectors_and_saturated_activations(case):
    P = _problem(case, "5x4", "saturated")
    got = _check(P)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k


@pytest.mark.parametrize("gname", ["8x1", "random_sparse"])
@pytest.mark.parametrize("fwd,bwd", [("tiled", "fused"), ("fused", "tiled")])
def test_crossed_entries_against_fp64(fwd, bwd, gname):
    """The tape is interchangeable: either forward's tape under either backward, at the same bar."""
    P = _problem("qm9", gname)
    assert _bytes("tiled", 1, P.g, P.d) == _bytes("fused", 1, P.g, P.d)
    agg, _, outs = _fwd_bwd(P, fwd, bwd)
    _hold_to_the_bar(P, agg, outs, tag=f"{fwd} forward -> {bwd} backward: ")


@pytest.fixture
def bf16x6():
    ops.set_matrix_mode("bf16x6")
    try:
        yield
    finally:
        ops.set_matrix_mode("f32")
        assert ops.get_matrix_mode() == "f32"


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("gname", ["8x1", "ragged", "star_in"])
def test_bf16x6_mode_against_fp64(case, gname, bf16x6):
    """M = 4 for every tensor (no exceptions), as the fused entries are held in this mode."""
    _check(_problem(case, gname), margins={})


# ---- hard contracts ----------------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_and_the_backward_leaves_the_tape_alone():
    P = _problem("qm9", "random_sparse")
    agg, tape, first = _fwd_bwd(P)
    before = tape.bits()
    st, second = run_bwd("tiled", P.case, P.g, P.inp, P.weights, None, tape, P.r)
    assert st == 0
    assert torch.equal(tape.bits(), before), "gcdm_mp_tile_bwd wrote to the tape"
    for k in BWD_OUTS:
        assert not bool(torch.isnan(first[k].inner).any()), k
        assert torch.equal(first[k].bits(), second[k].bits()), k
    del second
    agg2, tape2, third = _fwd_bwd(P)
    assert torch.equal(agg.bits(), agg2.bits()) and torch.equal(before, tape2.bits())
    for k in BWD_OUTS:
        assert torch.equal(first[k].bits(), third[k].bits()), k


@pytest.mark.parametrize("case", CASES)
def test_all_on_mask_equals_null_mask_bitwise(case):
    P = _problem(case, "random_sparse")
    on = torch.ones(P.g.E, dtype=torch.bool)
    a_agg, _, a = _fwd_bwd(P, edge_mask=None)
    b_agg, _, b = _fwd_bwd(P, edge_mask=on)
    assert torch.equal(a_agg.bits(), b_agg.bits())
    for k in BWD_OUTS:
        assert torch.equal(a[k].bits(), b[k].bits()), k


@pytest.mark.parametrize("case", CASES)
def test_a_molecule_computes_the_same_bits_alone_and_inside_a_batch(case):
    """The molecule [13] alone and as the fourth of [1, 2, 7, 13, 9, 3] (node offset 10, edge offset 54: its edges sit at other rows of the
    64-row tiles, in other workgroups): a row's result depends on that row alone."""
    P = _problem(case, "ragged")
    big, inp, r = P.g, P.inp, P.r
    n0, n1, e0, e1 = 10, 23, 54, 54 + 169
    assert int(big.rowptr[n0]) == e0 and int(big.rowptr[n1]) == e1
    small = R.make_graph("fc[13]", 13, big.row[e0:e1] - n0, big.col[e0:e1] - n0)
    sub = SimpleNamespace(case=case, g=small, weights=P.weights, mask=None, r=r[n0:n1],
                          inp=SimpleNamespace(h=inp.h[n0:n1], chi=inp.chi[n0:n1], e=inp.e[e0:e1], xi=inp.xi[e0:e1], frames=inp.frames[e0:e1]))
    agg_b, _, out_b = _fwd_bwd(P)
    agg_s, _, out_s = _fwd_bwd(sub)
    assert torch.equal(agg_b.bits().view(big.N, 352)[n0:n1], agg_s.bits().view(13, 352))
    for k, w in dict(dh=256, dvnode=96).items():
        assert torch.equal(out_b[k].bits().view(big.N, w)[n0:n1], out_s[k].bits().view(13, w)), k
    for k, w in dict(de=P.d["Se"], dxi=3 * P.d["Ve"]).items():
        assert torch.equal(out_b[k].bits().view(big.E, w)[e0:e1], out_s[k].bits().view(169, w)), k


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N", [0, 5])
def test_empty_work_writes_nothing(case, N):
    weights, d = R.layer_weights(case)
    g = R.make_graph("empty", N, torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    inp = R.make_inputs(d, g)
    for tape in (0, 1):
        st, agg, work = run_fwd("tiled", case, g, inp, weights, None, tape)
        assert st == 0 and bool(torch.isnan(agg.get()).all()) and bool(torch.isnan(work.inner).all())
    st, outs = run_bwd("tiled", case, g, inp, weights, None, work, torch.zeros(N, 352))
    assert st == 0
    for k, o in outs.items():
        assert bool(torch.isnan(o.get()).all()), k
    # through the wrapper: the zero sum and zero gradients of the right shapes
    graph = ops.Graph(torch.zeros(2, 0, dtype=torch.int64, device=H.DEV), N)
    leaves = [t.to(H.DEV).requires_grad_(True) for t in (inp.h, inp.chi, inp.e, inp.xi)]
    ws = [weights[k].to(H.DEV).requires_grad_(True) for k in R.weight_keys()]
    a_s, a_v = ops.message_layer(*leaves, inp.frames.to(H.DEV), graph, ws, path="tiled")
    assert tuple(a_s.shape) == (N, 256) and tuple(a_v.shape) == (N, 32, 3) and not bool(a_s.any()) and not bool(a_v.any())
    (a_s.sum() + a_v.sum()).backward()
    for t in leaves + ws:
        assert t.grad is not None and t.grad.shape == t.shape and not bool(t.grad.any())


def test_wrapper_agrees_bitwise_with_the_direct_calls():
    """ops.message_layer(path="tiled") is the same two C calls."""
    P = _problem("qm9", "random_sparse")
    agg, _, outs = _fwd_bwd(P)
    got = H._named(P.case, P.g, P.weights, agg, outs)
    o = H._ops_operands(P.g, P.inp, P.weights, P.r)
    a_s, a_v = ops.message_layer(*o.leaves, o.frames, o.G, o.ws, path="tiled")
    ((a_s * o.r[:, :256]).sum() + (a_v * o.r[:, 256:].reshape(-1, 32, 3)).sum()).backward()
    assert torch.equal(a_s.detach().cpu(), got["agg_s"]) and torch.equal(a_v.detach().cpu(), got["agg_v"])
    for k, t in zip(("dh", "dchi", "de", "dxi"), o.leaves):
        assert torch.equal(t.grad.cpu(), got[k]), k
    for k, t in zip(R.weight_keys(), o.ws):
        assert torch.equal(t.grad.cpu(), got[k]), k


# ---- bits against the "fused" entries, fp32 mode ---------------------------------------------------------------------------------------------
def _tape_fields(N, E, d):
    """The tape (fwd_layout(d, 1) of csrc/gcdm_ops.mp_train.hip.h, then the final states) restated: name -> (offset, floats); every buffer
    starts at a multiple of 64 floats."""
    S, V, Hk, X = 256, 32, 8, 256 + 8 + 9
    vin0 = 2 * V + d["Ve"]
    h0 = vin0 // 4
    k0 = d["Se"] + h0 + 9
    sizes = [("wij", 2 * S * S), ("wr0", S * k0), ("aij", N * 2 * S), ("vpre0", E * 3 * vin0), ("x0", E * k0)]
    sizes += [(f"x{k}", E * X) for k in (1, 2, 3)] + [(f"vst{k}", E * 3 * V) for k in (1, 2, 3)]
    sizes += [(f"vh{k}", E * 3 * (Hk if k else h0)) for k in range(4)] + [(f"spre{k}", E * S) for k in range(4)]
    sizes += [(f"gate{k}", E * V) for k in range(4)] + [("g", E * S), ("att", E), ("sfin", E * S), ("vfin", E * 3 * V)]
    fields, o = {}, 0
    for name, n in sizes:
        fields[name] = (o, n)
        o += (n + 63) // 64 * 64
    return fields, o


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("gname", ["8x1", "ragged", "random_sparse"])
def test_bits_against_the_fused_entries(case, gname):
    P = _problem(case, gname)
    f_agg, f_tape, f_out = _fwd_bwd(P, "fused", "fused")
    t_agg, t_tape, t_out = _fwd_bwd(P, "tiled", "tiled")
    fields, total = _tape_fields(P.g.N, P.g.E, P.d)
    assert total == f_tape.n == t_tape.n
    fb, tb = f_tape.bits(), t_tape.bits()
    o, n = fields.pop("g")
    assert bool(torch.isnan(t_tape.inner[o:o + n]).all()), "gcdm_mp_tile_fwd wrote the silu buffer it documents as unwritten"
    same = {"agg": torch.equal(f_agg.bits(), t_agg.bits())}
    for name, (o, n) in fields.items():
        same[f"tape.{name}"] = torch.equal(fb[o:o + n], tb[o:o + n])
    for k in BWD_OUTS:
        same[k] = torch.equal(f_out[k].bits(), t_out[k].bits())
    print(f"\nBITS {P.what}equal to the fused entries: " + ", ".join(k for k, v in same.items() if v) + " | DIFFERENT: " +
          (", ".join(k for k, v in same.items() if not v) or "none"))
    # the forward is bit for bit the fused forward; the backward outputs are printed only (docstring)
    assert [k for k, v in same.items() if not v and k not in BWD_OUTS] == []
