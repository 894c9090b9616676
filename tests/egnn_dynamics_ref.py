"""The EGNN dynamics network restated on the CPU (fp64 by default), for the tests of bio-diffusion_amd/egnn_dynamics.py.

Written from the reference's text (src/models/components/egnn.py:227-400 EGNN_Sparse, :573-823 EGNNDynamics; PyG's MessagePassing with the
default flow source_to_target: i = edge_index[1] receives, j = edge_index[0] sends, sum aggregation at edge_index[1]; PyG's LayerNorm in graph
mode).  Weights: a dict with the reference's state-dict names.  ``dtype=torch.float32`` gives the fp32 run that sets the bar of the GPU tests.
Test support, not an oracle of the sampler."""
import contextlib
import math
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import torch

M_DIM, COORS_HIDDEN = 16, 64
U = 2.0 ** -24
M_DEFAULT = 4                      # the margin the project uses against fp32-vs-fp64 gaps (mp_train_ref.M_DEFAULT)
M_MAX = 16                         # no documented exception may go beyond this
# The documented exceptions: tensor -> M.  Measured ratios and reasons: tests/test_egnn_dynamics_cabi_gpu.py's docstring and DESIGN.md 3.10.
MARGINS: Dict[str, int] = {}                               # the whole-tensor bar: no exception
ROW_MARGINS: Dict[str, int] = {"dx": 16, "x": 16}          # a row against its own gap: the two coordinate tensors, whose rows are three numbers
GUARD = 64                         # NaN guard words either side of every device buffer the C ABI writes
SIZES = [1, 2, 3, 17, 33, 70]      # one slot, a 2 x 2 list, receivers whose slot lists cross a 16-, a 64- and a 256-edge boundary, tiles inside a molecule
DIMS = [(32, 8), (64, 64)]         # (H, Eh): 2 D = 146 (K padded to 160) and 2 D = 386 (padded to 400)


def dims_of(cfg) -> Tuple[int, int, int, int]:
    """(h_in, h_out, e_in, D) of a configuration dict: H, Eh, L, num_atom_types, include_charges, condition_on_time, num_context, self_condition."""
    hd = cfg["num_atom_types"] + int(cfg["include_charges"])
    cond = int(cfg["condition_on_time"]) + cfg["num_context"]
    h_in = (2 * hd if cfg["self_condition"] else hd) + cond
    return h_in, hd + cond, 2 if cfg["self_condition"] else 1, 2 * cfg["H"] + cfg["Eh"] + 1


def state_dict_shapes(cfg) -> Dict[str, Tuple[int, ...]]:
    """Names and shapes of EGNNDynamics's state dict, in registration order."""
    H, Eh = cfg["H"], cfg["Eh"]
    h_in, h_out, e_in, D = dims_of(cfg)
    sh = {"node_embedding.weight": (H, h_in), "node_embedding.bias": (H,), "edge_embedding.weight": (Eh, e_in), "edge_embedding.bias": (Eh,)}
    for l in range(cfg["L"]):
        p = f"egnn.mpnn_layers.{l}."
        sh[p + "edge_mlp.0.weight"], sh[p + "edge_mlp.0.bias"] = (2 * D, D), (2 * D,)
        sh[p + "edge_mlp.3.weight"], sh[p + "edge_mlp.3.bias"] = (M_DIM, 2 * D), (M_DIM,)
        sh[p + "node_norm.weight"], sh[p + "node_norm.bias"] = (H,), (H,)
        sh[p + "coors_norm.scale"] = (1,)
        sh[p + "node_mlp.0.weight"], sh[p + "node_mlp.0.bias"] = (2 * H, H + M_DIM), (2 * H,)
        sh[p + "node_mlp.3.weight"], sh[p + "node_mlp.3.bias"] = (H, 2 * H), (H,)
        sh[p + "coors_mlp.0.weight"], sh[p + "coors_mlp.0.bias"] = (COORS_HIDDEN, M_DIM), (COORS_HIDDEN,)
        sh[p + "coors_mlp.3.weight"], sh[p + "coors_mlp.3.bias"] = (1, COORS_HIDDEN), (1,)
    sh["scalar_node_projection.weight"], sh["scalar_node_projection.bias"] = (h_out, H), (h_out,)
    return sh


def make_weights(cfg, seed: int, bias_scale: float = 0.1, coors_scale: float = 0.5) -> Dict[str, torch.Tensor]:
    """Xavier-normal matrices as the reference's init_, but biases ~ bias_scale N(0, 1) (the reference zeroes them: a zero bias would hide a
    bias the kernel drops), LayerNorm weight 1 + 0.1 N(0, 1), coors_norm.scale = coors_scale (the reference: 1e-2; larger, so that the
    coordinate update is well above the rounding of x)."""
    g = torch.Generator().manual_seed(seed)
    W = {}
    for k, s in state_dict_shapes(cfg).items():
        if k.endswith("coors_norm.scale"):
            W[k] = torch.full(s, coors_scale)
        elif k.endswith("node_norm.weight"):
            W[k] = 1 + 0.1 * torch.randn(s, generator=g)
        elif len(s) == 2:
            W[k] = torch.randn(s, generator=g) * math.sqrt(2.0 / (s[0] + s[1]))
        else:
            W[k] = bias_scale * torch.randn(s, generator=g)
    return W


def make_inputs(cfg, sizes: Sequence[int], seed: int, spread: float = 1.5):
    """(xh [N, 3 + F], t [N, 1], batch_index [N], context [N, C] or None, xh_self_cond or None), fp32."""
    g = torch.Generator().manual_seed(seed)
    N = int(sum(sizes))
    F = cfg["num_atom_types"] + int(cfg["include_charges"])
    bi = torch.repeat_interleave(torch.arange(len(sizes)), torch.as_tensor(list(sizes), dtype=torch.long))
    xh = torch.cat([spread * torch.randn((N, 3), generator=g), torch.randn((N, F), generator=g)], 1)
    t = torch.rand((len(sizes), 1), generator=g)[bi]
    ctx = torch.randn((len(sizes), cfg["num_context"]), generator=g)[bi] if cfg["num_context"] else None
    sc = torch.cat([spread * torch.randn((N, 3), generator=g), torch.randn((N, F), generator=g)], 1) if cfg["self_condition"] else None
    return xh, t, bi, ctx, sc


def _lin(W, name, v):
    return v @ W[name + ".weight"].T + W[name + ".bias"]


def _silu(v):
    return v * torch.sigmoid(v)


def edge_index_of(batch_index: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """get_fully_connected_edge_index (gcpnet.py:1056-1066): every ordered pair of one molecule, the diagonal included, without masked nodes."""
    ei = torch.stack(torch.where(batch_index[:, None] == batch_index[None, :]), 0)
    return ei[:, mask[ei[0]] & mask[ei[1]]]


def _center(x, bi, mask, B):
    """centralize(..., edm=True): x - centroid over the molecule's unmasked rows, on unmasked rows (masked rows are zero already)."""
    m = mask.to(x.dtype)[:, None]
    num = torch.zeros((B, 1), dtype=x.dtype).index_add_(0, bi, m)
    s = torch.zeros((B, x.shape[1]), dtype=x.dtype).index_add_(0, bi, x)
    return x - (s / num)[bi] * m


def layer_norm_graph(h, bi, B, weight, bias, eps: float = 1e-5):
    """torch_geometric.nn.norm.LayerNorm(mode="graph"): statistics per graph over all of its rows and all features."""
    norm = (torch.zeros(B, dtype=h.dtype).index_add_(0, bi, torch.ones(h.shape[0], dtype=h.dtype)).clamp(min=1) * h.shape[1])[:, None]
    mean = torch.zeros((B, h.shape[1]), dtype=h.dtype).index_add_(0, bi, h).sum(1, keepdim=True) / norm
    c = h - mean[bi]
    var = torch.zeros((B, h.shape[1]), dtype=h.dtype).index_add_(0, bi, c * c).sum(1, keepdim=True) / norm
    return c / (var + eps).sqrt()[bi] * weight + bias


def layer(W, p, h, x, e_attr, ei, bi, B, probe: Optional[dict] = None):
    """EGNN_Sparse.forward / propagate on (coors x, feats h): -> (h_out, x_out)."""
    j, i = ei[0], ei[1]
    rel = x[j] - x[i]
    rel_dist = (rel ** 2).sum(-1, keepdim=True)
    m_ij = _silu(_lin(W, p + "edge_mlp.3", _silu(_lin(W, p + "edge_mlp.0", torch.cat([h[i], h[j], e_attr, rel_dist], -1)))))
    w_ij = torch.tanh(_lin(W, p + "coors_mlp.3", _silu(_lin(W, p + "coors_mlp.0", m_ij))))
    normed = rel / rel.norm(dim=-1, keepdim=True).clamp(min=1e-8) * W[p + "coors_norm.scale"]
    dx = torch.zeros_like(x).index_add_(0, i, w_ij * normed)
    m_i = torch.zeros((h.shape[0], M_DIM), dtype=h.dtype).index_add_(0, i, m_ij)
    ln = layer_norm_graph(h, bi, B, W[p + "node_norm.weight"], W[p + "node_norm.bias"])
    if probe is not None:
        probe.setdefault("m", []).append(m_i)
        probe.setdefault("dx", []).append(dx)
        probe.setdefault("ln", []).append(ln)
    h_out = h + _lin(W, p + "node_mlp.3", _silu(_lin(W, p + "node_mlp.0", torch.cat([ln, m_i], -1))))
    if probe is not None:
        probe.setdefault("h", []).append(h_out)
        probe.setdefault("x", []).append(x + dx)
    return h_out, x + dx


def n_layers_of(W) -> int:
    return 1 + max(int(k.split(".")[2]) for k in W if k.startswith("egnn.mpnn_layers."))


def forward(W: Dict[str, torch.Tensor], cfg, xh: torch.Tensor, t: torch.Tensor, batch_index: torch.Tensor, mask: Optional[torch.Tensor] = None,
            context: Optional[torch.Tensor] = None, xh_self_cond: Optional[torch.Tensor] = None, dtype=torch.float64, probe: Optional[dict] = None):
    """atom_types_and_coords_forward (egnn.py:672-823): net_out [N, 3 + F].  A `probe` dict receives, per layer, the receiver sums "m" [N, 16] and
    "dx" [N, 3], the LayerNorm output "ln" [N, H] and the layer's outputs "h", "x"; plus "h_in", "x_in" (the layers' input) and "x_init"."""
    W = {k: v.to(dtype) for k, v in W.items()}
    bi = batch_index
    B = int(bi.max()) + 1 if bi.numel() else 0
    N = xh.shape[0]
    mask = torch.ones(N, dtype=torch.bool) if mask is None else mask.bool()
    mf = mask.to(dtype)[:, None]
    xh = xh.to(dtype) * mf
    x_init, h = xh[:, :3], xh[:, 3:]
    ei = edge_index_of(bi, mask)
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
    x = _center(x_init, bi, mask, B)
    h = _lin(W, "node_embedding", h) * mf
    e_attr = _lin(W, "edge_embedding", e)
    if probe is not None:
        probe["h_in"], probe["x_in"], probe["x_init"] = h, x, x_init
    for l in range(n_layers_of(W)):
        h, x = layer(W, f"egnn.mpnn_layers.{l}.", h, x, e_attr, ei, bi, B, probe)
    x, h = x * mf, h * mf
    h = _lin(W, "scalar_node_projection", h) * mf
    vel = (x - x_init) * mf
    if cfg["num_context"]:
        h = h[:, :-cfg["num_context"]]
    if cfg["condition_on_time"]:
        h = h[:, :-1]
    if bool(vel.isnan().any()):
        vel = torch.zeros_like(vel)
    vel = _center(vel, bi, mask, B)
    return torch.cat([vel, h], -1)


def column_split_pre(W, p, we, be, h, x, r0, ei, r0sc=None):
    """The pre-activation of edge_mlp.0 as the fused kernel forms it: A_i + B_j + r0 u (+ r0sc u') + r w_r with the edge embedding folded in."""
    W1, b1 = W[p + "edge_mlp.0.weight"], W[p + "edge_mlp.0.bias"]
    H, Eh = h.shape[1], we.shape[0]
    Wi, Wj, We, wr = W1[:, :H], W1[:, H:2 * H], W1[:, 2 * H:2 * H + Eh], W1[:, 2 * H + Eh]
    A = h @ Wi.T + b1 + We @ be
    Bm = h @ Wj.T
    u = We @ we
    j, i = ei[0], ei[1]
    r = ((x[j] - x[i]) ** 2).sum(-1, keepdim=True)
    pre = A[i] + Bm[j] + r0 * u[:, 0] + r * wr
    return pre if r0sc is None else pre + r0sc * u[:, 1]


def references(W, cfg, xh, t, bi, mask=None, context=None, xh_self_cond=None):
    """The fp64 and the fp32 restatement with every layer's tensors, as float64 CPU tensors: .out64 / .out32 and .probe64 / .probe32."""
    p64, p32 = {}, {}
    o64 = forward(W, cfg, xh, t, bi, mask, context, xh_self_cond, torch.float64, p64)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)          # torch's fp32 sums split their work by thread count: one thread, so that the gap does not move with the host
    try:
        o32 = forward(W, cfg, xh, t, bi, mask, context, xh_self_cond, torch.float32, p32)
    finally:
        torch.set_num_threads(threads)
    dbl = lambda v: [u.double() for u in v] if isinstance(v, list) else v.double()
    return SimpleNamespace(out64=o64, out32=o32.double(), probe64=p64, probe32={k: dbl(v) for k, v in p32.items()})


def _needed(err, gap, floor):
    over = (err - floor).clamp(min=0)
    need = torch.where(over > 0, over / gap, torch.zeros_like(over))
    return torch.where(torch.isnan(err) | torch.isnan(need), torch.full_like(need, float("inf")), need)


def compare(name: str, got: torch.Tensor, want64: torch.Tensor, want32: torch.Tensor, margins: Optional[Dict[str, int]] = None, what: str = "",
            row_margins: Optional[Dict[str, int]] = None):
    """mp_train_ref.compare's bar for one row-wise tensor: the whole tensor within M * (max gap) + floor, and every row within M_row * (its own
    fp32-vs-fp64 gap) + floor, floor = 8 U max|want64|.  M = MARGINS.get(name, 4), M_row = ROW_MARGINS.get(name, M).
    -> (failures, (M the tensor needs, M its worst row needs))."""
    margins = MARGINS if margins is None else margins
    row_margins = ROW_MARGINS if row_margins is None else row_margins
    assert all(M_DEFAULT <= m <= M_MAX for m in list(margins.values()) + list(row_margins.values()))
    M = margins.get(name, M_DEFAULT)
    M_row = row_margins.get(name, M)
    g = got.detach().double().cpu().reshape(want64.shape)
    if not want64.numel():
        return [], (0.0, 0.0)
    err = (g - want64).abs().nan_to_num(nan=math.inf)          # an entry the kernel left unwritten (NaN) fails any bar
    gap = (want32 - want64).abs()
    floor = 8 * U * float(want64.abs().max())
    need = float(_needed(err.max(), gap.max(), floor))
    e2, g2 = err.reshape(err.shape[0], -1), gap.reshape(gap.shape[0], -1)
    need_row = float(_needed(e2.max(1).values, g2.max(1).values, floor).max())
    failures = []
    if not need <= M:
        failures.append(f"{what}{name}: max|got - ref64| = {float(err.max()):.3e} needs M = {need:.3g} > {M} (gap {float(gap.max()):.3e}, floor {floor:.3e})")
    if not need_row <= M_row:
        failures.append(f"{what}{name}: a row needs M = {need_row:.3g} > {M_row} against its own fp32 gap (floor {floor:.3e})")
    return failures, (need, need_row)


def ordered_tensors(W, n_layers: int) -> List[torch.Tensor]:
    """The state dict in the order gcdm_egnn_dyn_pack takes it (include/gcdm_egnn_dynamics.h)."""
    out = [W["edge_embedding.weight"], W["edge_embedding.bias"]]
    for l in range(n_layers):
        p = f"egnn.mpnn_layers.{l}."
        out += [W[p + n] for n in ("edge_mlp.0.weight", "edge_mlp.0.bias", "edge_mlp.3.weight", "edge_mlp.3.bias", "node_norm.weight", "node_norm.bias",
                                   "coors_norm.scale", "node_mlp.0.weight", "node_mlp.0.bias", "node_mlp.3.weight", "node_mlp.3.bias",
                                   "coors_mlp.0.weight", "coors_mlp.0.bias", "coors_mlp.3.weight", "coors_mlp.3.bias")]
    return out


GOLDEN_CONFIGS = {                 # tests/golden/egnn_dynamics_<name>.npz (make_egnn_dynamics_golden.py)
    "plain": dict(H=32, Eh=8, L=2, num_atom_types=5, include_charges=True, condition_on_time=False, num_context=0, self_condition=False),
    "time_context": dict(H=32, Eh=8, L=2, num_atom_types=5, include_charges=False, condition_on_time=True, num_context=2, self_condition=False),
    "selfcond": dict(H=32, Eh=8, L=2, num_atom_types=5, include_charges=True, condition_on_time=True, num_context=0, self_condition=True),
    "masked": dict(H=32, Eh=8, L=2, num_atom_types=5, include_charges=True, condition_on_time=True, num_context=0, self_condition=False),
}
GOLDEN_SIZES = [1, 2, 3, 17, 33, 70]


def golden_mask(name: str, sizes: Sequence[int]) -> Optional[torch.Tensor]:
    """The node mask of a golden configuration: "masked" drops the last atom of every molecule of more than two atoms (a molecule without a present atom
    has no centre: the reference divides by its count)."""
    if name != "masked":
        return None
    parts = []
    for n in sizes:
        m = torch.ones(n, dtype=torch.bool)
        if n > 2:
            m[-1] = False
        parts.append(m)
    return torch.cat(parts)


def reference_cfgs(cfg, conditioning_names=("alpha", "gap", "homo")):
    """The four configuration dicts of the constructor for a test configuration (plain dicts; config.cfg_get reads them)."""
    model_cfg = dict(h_input_dim=cfg["num_atom_types"] + int(cfg["include_charges"]), chi_input_dim=2, e_input_dim=1, xi_input_dim=1,
                     h_hidden_dim=cfg["H"], chi_hidden_dim=8, e_hidden_dim=cfg["Eh"], xi_hidden_dim=4, num_encoder_layers=cfg["L"], dropout=0.0)
    module_cfg = dict(conditioning=list(conditioning_names[:cfg["num_context"]]), norm_x_diff=True)
    diffusion_cfg = dict(diffusion_target="atom_types_and_coords", self_condition=cfg["self_condition"], condition_on_time=cfg["condition_on_time"],
                         dynamics_network="egnn")
    dataloader_cfg = dict(num_atom_types=cfg["num_atom_types"], include_charges=cfg["include_charges"], num_x_dims=3, num_radials=1)
    return dict(model_cfg=model_cfg, module_cfg=module_cfg, diffusion_cfg=diffusion_cfg, dataloader_cfg=dataloader_cfg)


class RestatedDynamics(torch.nn.Module):
    """``forward`` above as a dynamics network (CPU, ``dtype``) holding copies of a state dict as parameters: what a model's objective runs on
    to give the fp64 (and the fp32) autograd reference of a training step.  ``grads()``: reference name -> gradient."""

    def __init__(self, state_dict, cfg, dtype=torch.float64):
        super().__init__()
        self.cfg, self.dtype = cfg, dtype
        self.P = torch.nn.ParameterDict({k.replace(".", "/"): torch.nn.Parameter(v.detach().cpu().to(dtype).clone()) for k, v in state_dict.items()})
        self.self_condition, self.num_atom_types, self.include_charges = cfg["self_condition"], cfg["num_atom_types"], cfg["include_charges"]
        self.fused_unsupported = "egnn"

    @contextlib.contextmanager
    def fp32_mfma(self):
        yield

    def forward(self, batch, xh, t, **kw):
        W = {k.replace("/", "."): v for k, v in self.P.items()}
        get = lambda k: batch[k] if isinstance(batch, dict) else getattr(batch, k, None)
        return batch, forward(W, self.cfg, xh, t, get("batch"), get("mask"), get("props_context"), kw.get("xh_self_cond"), dtype=self.dtype)

    def grads(self):
        return {k.replace("/", "."): v.grad for k, v in self.P.items()}
