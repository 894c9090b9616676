"""CPU reference of one stand-alone GCP2 for the tests of the fused GCP2 (include/gcdm_gcp2_train.h): oracle.gcdm_oracle.gcp2 in fp64 (the
reference) and in fp32 on one thread (the yardstick of the measured bar), with autograd for ds, dv and every weight gradient.  Never the
operator path, never the code under test.  No GPU in this file.

The oracle's gcp2 takes ONE nonlinearity for both places; a module with two different ones is two oracle calls (s_out from the first, v_out
from the second): the two outputs do not interact."""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import synth  # noqa: E402
from oracle import gcdm_oracle as O  # noqa: E402

U = 2.0 ** -24                     # unit roundoff of fp32
M_DEFAULT = 4                      # the margin the project uses against fp32-vs-fp64 gaps
M_MAX = 16                         # no documented exception may go beyond this
ROWWISE = ("s_out", "v_out", "ds", "dv")
ACT = {0: None, 1: "silu"}


def weight_keys(ff, VO):
    """The module's tensors in the order of include/gcdm_gcp2_train.h (state-dict order)."""
    keys = ["vector_down.weight", "vector_down_frames.weight"]
    keys += ["scalar_out.0.weight", "scalar_out.0.bias", "scalar_out.2.weight", "scalar_out.2.bias"] if ff else ["scalar_out.weight", "scalar_out.bias"]
    if VO:
        keys += ["vector_up.weight", "vector_out_scale.weight", "vector_out_scale.bias"]
    return keys


def dims(SI, VI, SO, VO, H, ff=0, a0=0, a1=0):
    return dict(SI=SI, VI=VI, SO=SO, VO=VO, H=H, ff=int(ff), a0=int(a0), a1=int(a1))


def weight_shapes(d):
    K = d["SI"] + d["H"] + 9
    sh = {"vector_down.weight": (d["H"], d["VI"]), "vector_down_frames.weight": (3, d["VI"])}
    if d["ff"]:
        sh.update({"scalar_out.0.weight": (d["SO"], K), "scalar_out.0.bias": (d["SO"],), "scalar_out.2.weight": (d["SO"], d["SO"]),
                   "scalar_out.2.bias": (d["SO"],)})
    else:
        sh.update({"scalar_out.weight": (d["SO"], K), "scalar_out.bias": (d["SO"],)})
    if d["VO"]:
        sh.update({"vector_up.weight": (d["VO"], d["H"]), "vector_out_scale.weight": (d["VO"], d["SO"]), "vector_out_scale.bias": (d["VO"],)})
    return {k: sh[k] for k in weight_keys(d["ff"], d["VO"])}


def instances(case, self_cond=False):
    """The five stand-alone GCP2 instances of a forward at the dims of config.py's QM9 / GEOM models (gcpnet.py:74-79, gcp_modules.py:527-535):
    edge embedding (bottleneck 1, silu / silu), node embedding (bottleneck 1, identity), feed-forward (2s, 2v) -> (s, v) with feedforward_out
    (bottleneck 4, identity), position (s, v) -> (s, 1) (bottleneck 4, silu / silu), projection (s, v) -> (h_in, 0) (bottleneck 1, identity)."""
    c = synth.DATASET_DIMS[case]
    S, V, Se, Ve = c["S"], c["V"], c["Se"], c["Ve"]
    h_in = synth.dims_h_in(c)
    h_diff = c["num_atom_types"] + int(c["include_charges"])
    m = 2 if self_cond else 1
    return {
        "edge": dims(m, m, Se, Ve, max(m, Ve), 0, 1, 1),
        "node": dims(h_in + (h_diff if self_cond else 0), 2 * m, S, V, max(2 * m, V), 0, 0, 0),
        "ff": dims(2 * S, 2 * V, S, V, 2 * V // 4, 1, 0, 0),
        "pos": dims(S, V, S, 1, V // 4, 0, 1, 1),
        "proj": dims(S, V, h_in, 0, V, 0, 0, 0),
    }


def make_weights(d, seed=3):
    g = torch.Generator().manual_seed(seed)
    W = {}
    for k, shp in weight_shapes(d).items():
        if len(shp) == 2:
            W[k] = torch.randn(shp, generator=g) / math.sqrt(shp[1])
        else:
            W[k] = 0.1 * torch.randn(shp, generator=g)
    return W


def make_rows(d, M, seed=5):
    """s, v, F (unit-length frame rows, as localize produces), and the cotangents rs, rv of the loss sum(rs s_out) + sum(rv v_out)."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn((M, d["SI"]), generator=g)
    v = torch.randn((M, d["VI"], 3), generator=g)
    F = torch.randn((M, 3, 3), generator=g)
    F = F / F.norm(dim=-1, keepdim=True).clamp(min=1e-6)
    rs = torch.randn((M, d["SO"]), generator=g)
    rv = torch.randn((M, d["VO"], 3), generator=g)
    return s, v, F, rs, rv


def _run(W, d, s, v, F, rs, rv, dtype, grads=True):
    P = {k: w.detach().to(dtype).clone().requires_grad_(grads) for k, w in W.items()}
    s_, v_ = s.detach().to(dtype).clone().requires_grad_(grads), v.detach().to(dtype).clone().requires_grad_(grads)
    F_ = F.to(dtype)
    row = torch.arange(s.shape[0])
    out = {}
    if d["VO"]:
        s_out, v_out = O.gcp2(P, "", s_, v_, row, F_, False, ACT[d["a1"]], True, feedforward_out=bool(d["ff"]))
        if d["a0"] != d["a1"]:
            s_out = O.gcp2(P, "", s_, v_, row, F_, False, ACT[d["a0"]], False, feedforward_out=bool(d["ff"]))
        out["v_out"] = v_out
    else:
        s_out = O.gcp2(P, "", s_, v_, row, F_, False, ACT[d["a0"]], False, feedforward_out=bool(d["ff"]))
        out["v_out"] = torch.zeros((s.shape[0], 0, 3), dtype=dtype)
    out["s_out"] = s_out
    if grads:
        loss = (s_out * rs.to(dtype)).sum()
        if d["VO"]:
            loss = loss + (out["v_out"] * rv.to(dtype)).sum()
        loss.backward()
        out["ds"], out["dv"] = s_.grad, v_.grad
        for k in P:
            out[k] = P[k].grad
    return {k: t.detach().double() for k, t in out.items()}


def references(W, d, s, v, F, rs, rv, row_mask=None, grads=True):
    """(ref64, ref32): name -> fp64 tensor.  ref32 is the fp32 run on ONE thread (torch's fp32 sums split by thread count)."""
    if row_mask is not None:
        F = F * row_mask.to(F.dtype).reshape(-1, 1, 1)
    ref64 = _run(W, d, s, v, F, rs, rv, torch.float64, grads)
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        ref32 = _run(W, d, s, v, F, rs, rv, torch.float32, grads)
    finally:
        torch.set_num_threads(n)
    return ref64, ref32


def _needed(err, gap, floor):
    err, gap = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(gap, dtype=torch.float64)
    over = (err - floor).clamp(min=0)
    need = torch.where(over > 0, over / gap.clamp(min=1e-300), torch.zeros_like(over))
    return float(need.max())


def compare(got, ref64, ref32, margins=None, what="", names=None):
    """-> (failures, ratios): failures lists every tensor (and, for the row-wise ones, row) outside M * max|ref32 - ref64| + 8 U max|ref64|;
    ratios[name] = (the M the whole tensor needs, the M its worst row needs)."""
    margins = margins or {}
    assert all(M_DEFAULT <= m <= M_MAX for m in margins.values())
    failures, ratios = [], {}
    for name in (names or list(ref64)):
        want = ref64[name]
        if not want.numel():
            ratios[name] = (0.0, 0.0)
            continue
        g = got[name].detach().double().cpu().reshape(want.shape)
        M = margins.get(name, M_DEFAULT)
        err, gap = (g - want).abs().nan_to_num(nan=math.inf), (ref32[name] - want).abs()
        floor = 8 * U * float(want.abs().max())
        need = _needed(err.max(), gap.max(), floor)
        need_row = 0.0
        if name in ROWWISE:
            e2, g2 = err.reshape(err.shape[0], -1), gap.reshape(gap.shape[0], -1)
            need_row = _needed(e2.max(dim=1).values, g2.max(dim=1).values, floor)
        ratios[name] = (need, need_row)
        if not need <= M:
            failures.append(f"{what}{name}: max|got - ref64| = {float(err.max()):.3e} needs M = {need:.3g} > {M} (gap {float(gap.max()):.3e}, floor {floor:.3e})")
        if not need_row <= M:
            failures.append(f"{what}{name}: a row needs M = {need_row:.3g} > {M} against its own fp32 gap (floor {floor:.3e})")
    return failures, ratios


def worst_ratio(ratios):
    name = max(ratios, key=lambda k: max(ratios[k]))
    return name, max(ratios[name])


def golden_case(g, name, node):
    """Inputs of one fixture of tests/golden/fn_gcp2.npz: (dims, weights, s, v, F per entity, recorded s_out, recorded v_out or None)."""
    bi = O.num_nodes_to_batch_index(g["num_nodes"])
    mask = torch.ones(len(bi), dtype=torch.bool)
    row, col = O.fully_connected_edges(bi, mask)
    fr = O.localize(O.centralize(g["x"], bi, len(g["num_nodes"]), mask), row, col).reshape(-1, 3, 3)
    if node:                                              # the mean of the frames of the node's edges (scalarize is linear in the frame)
        N = len(bi)
        tot = torch.zeros(N, 3, 3).index_add_(0, row, fr)
        cnt = torch.zeros(N).index_add_(0, row, torch.ones(len(row)))
        fr = tot / cnt.clamp(min=1).reshape(-1, 1, 1)
    W = {k[len(name) + 3:]: v for k, v in g.items() if k.startswith(name + "_w_")}
    ff = "scalar_out.0.weight" in W
    s, v = g[name + "_s"], g[name + "_v"]
    ov = g.get(name + "_ov")
    act = 1 if name == "edge" else 0
    d = dims(s.shape[1], v.shape[1], g[name + "_os"].shape[1], 0 if ov is None else ov.shape[1], W["vector_down.weight"].shape[0], ff, act, act)
    W = {k: W[k] for k in weight_keys(ff, d["VO"])}
    return d, W, s, v, fr, row, g[name + "_os"], ov
