"""References for the training path of the EGNN dynamics network (include/gcdm_egnn_train.h, EGNNDynamics.set_train_path), CPU torch.

(a) The autograd reference: egnn_dynamics_ref.layer / forward restated with ONE change -- the diagonal edges i = j are left out of the
    coordinate sum.  Their terms are exactly zero, so the forward value is the same; their derivative is w_ii scale / 1e-8, which autograd adds to
    grad x_i through one gather and subtracts through the other, inside two separate sums next to O(1) terms.  In fp64 that pair still leaves
    about scale / 1e-8 * 2^-53 * n of rounding, comparable to the fp32 gaps the bars are built from, so fp64 autograd with the diagonal left in
    is not a usable reference for a gradient.  ``keep_diagonal=True`` gives that variant, for the test that documents the effect.
    ``block_autograd`` is the same at the level of the operator (inputs A, B, V, ...).
(b) The hand-written reference: ``block_backward``, the backward of the edge block in plain tensor algebra, in either dtype.  Its fp32 run on one
    thread is the "gap" of every bar."""
import contextlib
from typing import Dict, Optional, Sequence

import torch

import egnn_dynamics_ref as er

M_DIM, COORS_HIDDEN = er.M_DIM, er.COORS_HIDDEN
GRADS = ("gA", "gB", "gx", "gV", "gW2", "gb2", "gC1", "gc1b", "gc2", "gc2b", "gscale")
INPUTS = ("A", "B", "V", "W2", "b2", "C1", "c1b", "c2", "c2b", "scale", "x")
# The documented exceptions of the C-ABI test: tensor -> M (whole tensor) and tensor -> M (a row against its own gap).  Measured values and
# reasons: tests/test_egnn_train_cabi_gpu.py's docstring and DESIGN.md 3.10.
MARGINS: Dict[str, int] = {}
ROW_MARGINS: Dict[str, int] = {"dx": 16}                   # the forward is k_edge's arithmetic: egnn_dynamics_ref.ROW_MARGINS["dx"]
# The documented exception of the model-level test (tests/test_egnn_train_gpu.py's docstring): parameter-name suffix -> M.
GRAD_MARGINS: Dict[str, int] = {"coors_norm.scale": 16}


def grad_margins(names) -> Dict[str, int]:
    """GRAD_MARGINS spelt out for the parameter names of a network."""
    return {k: m for k in names for suffix, m in GRAD_MARGINS.items() if k.endswith(suffix)}


# ---- (a) the network -----------------------------------------------------------------------------------------------------------------------
def layer(W, p, h, x, e_attr, ei, bi, B, keep_diagonal: bool = False):
    """egnn_dynamics_ref.layer with the diagonal edges left out of the coordinate sum (unless keep_diagonal)."""
    j, i = ei[0], ei[1]
    rel = x[j] - x[i]
    rel_dist = (rel ** 2).sum(-1, keepdim=True)
    m_ij = er._silu(er._lin(W, p + "edge_mlp.3", er._silu(er._lin(W, p + "edge_mlp.0", torch.cat([h[i], h[j], e_attr, rel_dist], -1)))))
    w_ij = torch.tanh(er._lin(W, p + "coors_mlp.3", er._silu(er._lin(W, p + "coors_mlp.0", m_ij))))
    off = torch.ones_like(i, dtype=torch.bool) if keep_diagonal else i != j
    relo = rel[off]
    normed = relo / relo.norm(dim=-1, keepdim=True).clamp(min=1e-8) * W[p + "coors_norm.scale"]
    dx = torch.zeros_like(x).index_add(0, i[off], w_ij[off] * normed)
    m_i = torch.zeros((h.shape[0], M_DIM), dtype=h.dtype).index_add(0, i, m_ij)
    ln = er.layer_norm_graph(h, bi, B, W[p + "node_norm.weight"], W[p + "node_norm.bias"])
    h_out = h + er._lin(W, p + "node_mlp.3", er._silu(er._lin(W, p + "node_mlp.0", torch.cat([ln, m_i], -1))))
    return h_out, x + dx


def forward(W, cfg, xh, t, batch_index, mask=None, context=None, xh_self_cond=None, dtype=torch.float64, keep_diagonal: bool = False):
    """egnn_dynamics_ref.forward on `layer` above."""
    W = {k: v.to(dtype) for k, v in W.items()}
    bi = batch_index
    B = int(bi.max()) + 1 if bi.numel() else 0
    N = xh.shape[0]
    mask = torch.ones(N, dtype=torch.bool) if mask is None else mask.bool()
    mf = mask.to(dtype)[:, None]
    xh = xh.to(dtype) * mf
    x_init, h = xh[:, :3], xh[:, 3:]
    ei = er.edge_index_of(bi, mask)
    d0 = x_init[ei[0]] - x_init[ei[1]]
    e = torch.nan_to_num((d0 ** 2).sum(1, keepdim=True))
    if cfg["self_condition"]:
        sc = torch.zeros_like(xh) if xh_self_cond is None else xh_self_cond.to(dtype)
        ds = sc[ei[0], :3] - sc[ei[1], :3]
        h = torch.cat([h, sc[:, 3:]], -1)
        e = torch.cat([e, torch.nan_to_num((ds ** 2).sum(1, keepdim=True))], -1)
    if cfg["condition_on_time"]:
        tt = t.to(dtype).reshape(-1, 1)
        h = torch.cat([h, tt.expand(N, 1) if tt.numel() == 1 else tt], -1)
    if cfg["num_context"]:
        h = torch.cat([h, context.to(dtype).reshape(N, cfg["num_context"])], -1)
    x = er._center(x_init, bi, mask, B)
    h = er._lin(W, "node_embedding", h) * mf
    e_attr = er._lin(W, "edge_embedding", e)
    for l in range(er.n_layers_of(W)):
        h, x = layer(W, f"egnn.mpnn_layers.{l}.", h, x, e_attr, ei, bi, B, keep_diagonal)
    x, h = x * mf, h * mf
    h = er._lin(W, "scalar_node_projection", h) * mf
    vel = (x - x_init) * mf
    if cfg["num_context"]:
        h = h[:, :-cfg["num_context"]]
    if cfg["condition_on_time"]:
        h = h[:, :-1]
    if bool(vel.isnan().any()):
        vel = torch.zeros_like(vel)
    vel = er._center(vel, bi, mask, B)
    return torch.cat([vel, h], -1)


class RestatedDynamics(er.RestatedDynamics):
    """egnn_dynamics_ref.RestatedDynamics on `forward` above: what a model's objective runs on to give reference (a) of a training step."""

    def __init__(self, state_dict, cfg, dtype=torch.float64, keep_diagonal: bool = False):
        super().__init__(state_dict, cfg, dtype)
        self.keep_diagonal = keep_diagonal

    def forward(self, batch, xh, t, **kw):
        W = {k.replace("/", "."): v for k, v in self.P.items()}
        get = lambda k: batch[k] if isinstance(batch, dict) else getattr(batch, k, None)
        return batch, forward(W, self.cfg, xh, t, get("batch"), get("mask"), get("props_context"), kw.get("xh_self_cond"), dtype=self.dtype,
                              keep_diagonal=self.keep_diagonal)


# ---- the operator ---------------------------------------------------------------------------------------------------------------------------
def edges_of(sizes: Sequence[int]):
    """(i, j) of every ordered pair of one molecule, sorted by receiver i, senders ascending."""
    bi = torch.repeat_interleave(torch.arange(len(sizes)), torch.as_tensor(list(sizes), dtype=torch.long))
    i, j = torch.where(bi[:, None] == bi[None, :])
    return i, j


def make_block(H: int, Eh: int, e_in: int, sizes: Sequence[int], seed: int, coincident=()):
    """The operator's inputs (fp32 tensors, the same for every precision of the references) and upstream gradients, from a layer of
    egnn_dynamics_ref.make_weights by the column split.  `coincident`: pairs (a, b) of atoms put at one point."""
    cfg = dict(H=H, Eh=Eh, L=1, num_atom_types=5, include_charges=True, condition_on_time=True, num_context=0, self_condition=e_in == 2)
    W = {k: v.double() for k, v in er.make_weights(cfg, seed=seed).items()}
    g = torch.Generator().manual_seed(seed + 1)
    N = int(sum(sizes))
    D = 2 * H + Eh + 1
    p = "egnn.mpnn_layers.0."
    W1, b1 = W[p + "edge_mlp.0.weight"], W[p + "edge_mlp.0.bias"]
    we, be = W["edge_embedding.weight"], W["edge_embedding.bias"]
    h = torch.randn((N, H), generator=g).double()
    x0 = 1.5 * torch.randn((N, 3), generator=g)
    x = x0 + 0.3 * torch.randn((N, 3), generator=g)
    for a, b in coincident:
        x[b] = x[a]
    xsc = 1.5 * torch.randn((N, 3), generator=g) if e_in == 2 else None
    We = W1[:, 2 * H:2 * H + Eh]
    u = We @ we
    V = torch.stack([u[:, 0], u[:, 1] if e_in == 2 else torch.zeros(2 * D, dtype=torch.float64), W1[:, 2 * H + Eh]])
    blk = dict(A=h @ W1[:, :H].T + b1 + We @ be, B=h @ W1[:, H:2 * H].T, V=V, W2=W[p + "edge_mlp.3.weight"], b2=W[p + "edge_mlp.3.bias"],
               C1=W[p + "coors_mlp.0.weight"], c1b=W[p + "coors_mlp.0.bias"], c2=W[p + "coors_mlp.3.weight"].reshape(-1),
               c2b=W[p + "coors_mlp.3.bias"], scale=W[p + "coors_norm.scale"], x=x, x0=x0, xsc=xsc)
    blk = {k: (None if v is None else v.float().contiguous()) for k, v in blk.items()}
    blk["gM"] = torch.randn((N, M_DIM), generator=g)
    blk["gdx"] = torch.randn((N, 3), generator=g)
    blk["sizes"], blk["e_in"], blk["H"], blk["Eh"] = list(sizes), e_in, H, Eh
    return blk


def _pre(b, i, j, dtype):
    x, x0 = b["x"].to(dtype), b["x0"].to(dtype)
    r0 = ((x0[j] - x0[i]) ** 2).sum(-1, keepdim=True)
    r0sc = torch.zeros_like(r0)
    if b["e_in"] == 2:
        xs = b["xsc"].to(dtype)
        r0sc = ((xs[j] - xs[i]) ** 2).sum(-1, keepdim=True)
    return r0, r0sc


def block_forward(b, t: Dict[str, torch.Tensor], keep_diagonal: bool = False):
    """The forward of the operator on the tensors `t` (INPUTS, any dtype, possibly requiring gradients) -> (M, dx).  The diagonal edges are left
    out of the coordinate sum unless keep_diagonal."""
    i, j = edges_of(b["sizes"])
    dtype = t["A"].dtype
    r0, r0sc = _pre(b, i, j, dtype)
    x = t["x"]
    d = x[j] - x[i]
    r = (d ** 2).sum(-1, keepdim=True)
    z1 = t["A"][i] + t["B"][j] + r0 * t["V"][0] + r * t["V"][2]
    if b["e_in"] == 2:
        z1 = z1 + r0sc * t["V"][1]
    m = er._silu(er._silu(z1) @ t["W2"].T + t["b2"])
    w = torch.tanh(er._silu(m @ t["C1"].T + t["c1b"]) @ t["c2"][:, None] + t["c2b"])
    off = torch.ones_like(i, dtype=torch.bool) if keep_diagonal else i != j
    do = d[off]
    term = w[off] * (do / do.norm(dim=-1, keepdim=True).clamp(min=1e-8) * t["scale"])
    N = x.shape[0]
    return torch.zeros((N, M_DIM), dtype=dtype).index_add(0, i, m), torch.zeros((N, 3), dtype=dtype).index_add(0, i[off], term)


def block_autograd(b, dtype=torch.float64, keep_diagonal: bool = False):
    """(a) at the level of the operator: M, dx and every gradient by torch autograd."""
    t = {k: b[k].to(dtype).clone().requires_grad_(True) for k in INPUTS}
    M, dx = block_forward(b, t, keep_diagonal)
    ((M * b["gM"].to(dtype)).sum() + (dx * b["gdx"].to(dtype)).sum()).backward()
    out = {"M": M.detach(), "dx": dx.detach()}
    for k in INPUTS:
        out["g" + k] = t[k].grad if t[k].grad is not None else torch.zeros_like(t[k])
    return out


def _dsilu(v):
    s = torch.sigmoid(v)
    return s * (1 + v * (1 - s))


def block_backward(b, dtype=torch.float64):
    """(b): the forward and the backward of the operator written out (include/gcdm_egnn_train.h), in `dtype`."""
    t = {k: b[k].to(dtype) for k in INPUTS}
    gM, gdx = b["gM"].to(dtype), b["gdx"].to(dtype)
    i, j = edges_of(b["sizes"])
    N = t["x"].shape[0]
    r0, r0sc = _pre(b, i, j, dtype)
    d = t["x"][j] - t["x"][i]
    r = (d ** 2).sum(-1, keepdim=True)
    u, u2, wr = t["V"][0], t["V"][1], t["V"][2]
    z1 = t["A"][i] + t["B"][j] + r0 * u + r * wr
    if b["e_in"] == 2:
        z1 = z1 + r0sc * u2
    a1 = er._silu(z1)
    z2 = a1 @ t["W2"].T + t["b2"]
    m = er._silu(z2)
    v = m @ t["C1"].T + t["c1b"]
    sv = er._silu(v)
    w = torch.tanh(sv @ t["c2"][:, None] + t["c2b"])
    nv = r.sqrt()
    n = nv.clamp(min=1e-8)
    scale = t["scale"]
    zeros = lambda c: torch.zeros((N, c), dtype=dtype)
    out = {"M": zeros(M_DIM).index_add(0, i, m), "dx": zeros(3).index_add(0, i, w * (d / n * scale))}
    gt = gdx[i]
    dot = (gt * d).sum(-1, keepdim=True) / n
    out["gscale"] = (w * dot).sum().reshape(1)
    gc = scale * dot * (1 - w * w)
    out["gc2"], out["gc2b"] = (gc * sv).sum(0), gc.sum().reshape(1)
    gv = gc * t["c2"] * _dsilu(v)
    out["gC1"], out["gc1b"] = gv.T @ m, gv.sum(0)
    gz2 = (gM[i] + gv @ t["C1"]) * _dsilu(z2)
    out["gW2"], out["gb2"] = gz2.T @ a1, gz2.sum(0)
    gz1 = (gz2 @ t["W2"]) * _dsilu(z1)
    out["gA"] = zeros(z1.shape[1]).index_add(0, i, gz1)
    out["gB"] = zeros(z1.shape[1]).index_add(0, j, gz1)
    out["gV"] = torch.cat([r0, r0sc, r], 1).T @ gz1
    q = gz1 @ wr[:, None]
    coord = torch.where(nv > 1e-8, gt / n - d * (d * gt).sum(-1, keepdim=True) / n ** 3, gt / 1e-8)
    gd = 2 * d * q + w * scale * coord
    off = i != j                                         # the diagonal contributes nothing to gx: its g_d is never formed
    out["gx"] = zeros(3).index_add(0, j[off], gd[off]) - zeros(3).index_add(0, i[off], gd[off])
    return out


@contextlib.contextmanager
def one_thread():
    """torch's fp32 sums split their work by thread count: one thread, so that the gap does not move with the host."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def block_references(b):
    """(b) in fp64 and in fp32 (one thread), as float64 tensors: (ref64, ref32)."""
    r64 = block_backward(b, torch.float64)
    with one_thread():
        r32 = block_backward(b, torch.float32)
    return r64, {k: v.double() for k, v in r32.items()}


def rel_diff(a: torch.Tensor, b: torch.Tensor) -> float:
    """max|a - b| / max|b| (0 for two all-zero tensors)."""
    s = float(b.abs().max())
    dlt = float((a - b).abs().max())
    return dlt / s if s > 0 else dlt
