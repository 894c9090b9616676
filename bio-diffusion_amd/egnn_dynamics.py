"""The reference's EGNN dynamics network (src/models/components/egnn.py: EGNN_Sparse :227-400, EGNN_Sparse_Network :406-570, EGNNDynamics
:573-823; ``diffusion_cfg.dynamics_network: egnn``, the EDM-style baseline of the paper's tables) on the MI355X.

Two paths (``set_path``), switched like the classifier's:

* ``"operators"``: the network as the reference writes it -- the ``[E, D]`` concatenation included -- on the autograd operators of
  libgcdm_ops.so (ops.linear / act / gather_row / gather_col / scatter_rows / centralize / fully_connected_edge_index / edge_features) plus
  torch element-wise ops.  Differentiable with respect to every parameter; serves masked nodes; the GPU-side cross-check of the other one.
* ``"fused"`` (the default): under ``torch.no_grad()`` / inference mode and with every node present, each layer is one call of
  include/gcdm_egnn_dynamics.h -- edge_mlp.0 split by columns with the edge embedding folded in, one edge kernel on fp32 MFMA that writes
  nothing of size [E, .], one node kernel for the graph-mode LayerNorm.  Forward only: when a gradient is being recorded or the mask has a
  False entry the call runs ``"operators"`` instead, silently.

Training (a forward that records a gradient) has two paths of its own (``set_train_path``): ``"operators"`` (the default) as above, and
``"fused"``: with every node present, everything of a layer that is per edge -- edge_mlp, coors_mlp, the coordinate term and the two receiver
sums -- is one differentiable operator, ``ops.egnn_edge_block`` (include/gcdm_egnn_train.h), fed by the column split of edge_mlp.0 written in
operators so that the gradients reach edge_mlp.0 and edge_embedding through the fold; LayerNorm, node_mlp and the residual stay on the operators.
Its gradient of the coordinates never forms the diagonal edges' cancelling pair, so it differs from the ``"operators"`` gradient by more than
rounding in x-dependent terms and is the closer one to the true gradient.

Dropout (the reference constructs the layers with dropout = 0), Fourier features, soft edges, global attention and ``recalc`` are not built.
There is no CPU / eager path: CPU tensors raise.  The module itself constructs on the CPU (state dicts, checkpoints)."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Any, List, Optional, Tuple

import torch
from torch import nn

from . import _native, ops
from .config import cfg_get

PATHS = ("fused", "operators")
TRAIN_PATHS = ("operators", "fused")
M_DIM = _native.EGNN_DYN_M_DIM
COORS_HIDDEN = _native.EGNN_DYN_COORS_HIDDEN
NODE_FEATURE_DIFFUSION_TARGETS = ("atom_types_and_coords",)


class CoorsNorm(nn.Module):
    """egnn.py:42-52: coors / clamp(|coors|, eps) * scale."""

    def __init__(self, eps: float = 1e-8, scale_init: float = 1.0):
        super().__init__()
        self.eps = eps
        self.scale = nn.Parameter(torch.zeros(1).fill_(scale_init))

    def forward(self, coors: torch.Tensor) -> torch.Tensor:
        return coors / coors.norm(dim=-1, keepdim=True).clamp(min=self.eps) * self.scale


class GraphLayerNorm(nn.Module):
    """torch_geometric.nn.norm.LayerNorm(dim) in its default graph mode: mean and variance per graph over all of its rows and all features
    (masked rows count, as in the reference), eps 1e-5, affine."""

    def __init__(self, in_channels: int, eps: float = 1e-5):
        super().__init__()
        self.in_channels, self.eps = in_channels, eps
        self.weight = nn.Parameter(torch.ones(in_channels))
        self.bias = nn.Parameter(torch.zeros(in_channels))

    def forward(self, x: torch.Tensor, batch: torch.Tensor, num_graphs: int) -> torch.Tensor:
        norm = torch.zeros(num_graphs, dtype=x.dtype, device=x.device).index_add(0, batch, torch.ones_like(x[:, 0])).clamp(min=1) * x.shape[1]
        mean = torch.zeros(num_graphs, dtype=x.dtype, device=x.device).index_add(0, batch, x.sum(1)) / norm
        c = x - mean[batch][:, None]
        var = torch.zeros(num_graphs, dtype=x.dtype, device=x.device).index_add(0, batch, (c * c).sum(1)) / norm
        return c / (var + self.eps).sqrt()[batch][:, None] * self.weight + self.bias


class EGNNSparse(nn.Module):
    """Parameter holder with EGNN_Sparse's state-dict names and registration order (edge_mlp.{0,3}, node_norm, coors_norm, node_mlp.{0,3},
    coors_mlp.{0,3}; index 1 of each Sequential is the reference's dropout slot, an Identity at dropout = 0)."""

    def __init__(self, feats_dim: int, edge_attr_dim: int, m_dim: int = M_DIM, norm_coors_scale_init: float = 1e-2):
        super().__init__()
        self.feats_dim, self.m_dim = feats_dim, m_dim
        self.edge_input_dim = edge_attr_dim + 1 + feats_dim * 2
        D = self.edge_input_dim
        self.edge_mlp = nn.Sequential(nn.Linear(D, D * 2), nn.Identity(), nn.SiLU(), nn.Linear(D * 2, m_dim), nn.SiLU())
        self.node_norm = GraphLayerNorm(feats_dim)
        self.coors_norm = CoorsNorm(scale_init=norm_coors_scale_init)
        self.node_mlp = nn.Sequential(nn.Linear(feats_dim + m_dim, feats_dim * 2), nn.Identity(), nn.SiLU(), nn.Linear(feats_dim * 2, feats_dim))
        self.coors_mlp = nn.Sequential(nn.Linear(m_dim, m_dim * 4), nn.Identity(), nn.SiLU(), nn.Linear(m_dim * 4, 1), nn.Tanh())
        self.apply(self.init_)

    @staticmethod
    def init_(module: nn.Module) -> None:
        if type(module) in {nn.Linear}:
            nn.init.xavier_normal_(module.weight)
            nn.init.zeros_(module.bias)


class EGNNSparseNetwork(nn.Module):
    def __init__(self, n_layers: int, feats_dim: int, edge_attr_dim: int):
        super().__init__()
        self.n_layers = n_layers
        self.mpnn_layers = nn.ModuleList(EGNNSparse(feats_dim, edge_attr_dim) for _ in range(n_layers))


class _Plan:
    """What a batch topology needs on the device, built once per (batch_index, mask): the molecule sizes (read on the host), node_offsets
    [B + 1] and node_mol [N] int32 for the fused layers, whether every node is present."""

    def __init__(self, batch_index: torch.Tensor, mask: Optional[torch.Tensor]):
        dev = batch_index.device
        counts = torch.unique_consecutive(batch_index, return_counts=True)[1]
        self.sizes = [int(v) for v in counts.cpu().tolist()]
        self.B, self.N = len(self.sizes), int(batch_index.shape[0])
        self.all_present = mask is None or bool(mask.all())
        noff = torch.zeros(self.B + 1, dtype=torch.int64)
        noff[1:] = torch.cumsum(torch.tensor(self.sizes, dtype=torch.int64), 0)
        with torch.inference_mode(False):          # normal tensors: the plan outlives the inference-mode call that made it
            self.node_offsets = noff.to(torch.int32).to(dev)
            self.node_mol = torch.repeat_interleave(torch.arange(self.B, dtype=torch.int32), torch.tensor(self.sizes, dtype=torch.int64)).to(dev)
            self.graph_index = torch.repeat_interleave(torch.arange(self.B), torch.tensor(self.sizes, dtype=torch.int64)).to(dev)
        self.edge_index: Optional[torch.Tensor] = None


class EGNNDynamics(nn.Module):
    """Drop-in for the reference ``dynamics_networks["egnn"]``: same constructor, ``forward(batch, xh [N, 3 + F], t [N, 1], **kwargs) ->
    (batch, net_out [N, 3 + F])``, same parameter names, shapes and registration order.  ``batch`` needs ``.batch`` (sorted molecule index
    per node), ``.mask`` and, for a property-conditional model, ``.props_context`` [N, C]."""

    def __init__(self, model_cfg, module_cfg, diffusion_cfg, dataloader_cfg, **kwargs):
        super().__init__()
        target = cfg_get(diffusion_cfg, "diffusion_target", "atom_types_and_coords")
        if target not in NODE_FEATURE_DIFFUSION_TARGETS:
            raise NotImplementedError("only diffusion_target=atom_types_and_coords is built")
        self.num_atom_types = int(cfg_get(dataloader_cfg, "num_atom_types"))
        self.include_charges = bool(cfg_get(dataloader_cfg, "include_charges"))
        self.num_x_dims = int(cfg_get(dataloader_cfg, "num_x_dims", 3))
        self.num_radials = int(cfg_get(dataloader_cfg, "num_radials", 1))
        self.norm_x_diff = bool(cfg_get(module_cfg, "norm_x_diff", True))
        self.self_condition = bool(cfg_get(diffusion_cfg, "self_condition", False))
        self.condition_on_time = bool(cfg_get(diffusion_cfg, "condition_on_time", True))
        self.num_context_node_features = len(cfg_get(module_cfg, "conditioning", []) or [])
        self.condition_on_context = self.num_context_node_features > 0
        if self.num_x_dims != 3:
            raise NotImplementedError("num_x_dims = 3 is what the kernels are built for")
        h_input_dim_ = self.num_atom_types + int(self.include_charges)
        cond = int(self.condition_on_time) + self.num_context_node_features
        h_input_dim = h_input_dim_ * 2 if self.self_condition else h_input_dim_
        e_in = int(cfg_get(model_cfg, "e_input_dim", 1))
        if e_in != 1:
            raise NotImplementedError("e_input_dim = 1 is what the featuriser of the dynamics produces (the squared distance)")
        self.edge_input_dims = (e_in * 2 if self.self_condition else e_in, int(cfg_get(model_cfg, "xi_input_dim", 1)) * (2 if self.self_condition else 1))
        self.node_input_dims = (h_input_dim + cond, int(cfg_get(model_cfg, "chi_input_dim", 2)) * (2 if self.self_condition else 1))
        self.edge_dims = (int(cfg_get(model_cfg, "e_hidden_dim")), int(cfg_get(model_cfg, "xi_hidden_dim", 0) or 0))
        self.node_dims = (int(cfg_get(model_cfg, "h_hidden_dim")), int(cfg_get(model_cfg, "chi_hidden_dim", 0) or 0))
        self.num_layers = int(cfg_get(model_cfg, "num_encoder_layers"))
        if self.node_dims[0] < 1 or self.edge_dims[0] < 1 or self.num_layers < 1:
            raise ValueError("h_hidden_dim, e_hidden_dim and num_encoder_layers must be positive")

        self.node_embedding = nn.Linear(self.node_input_dims[0], self.node_dims[0])
        self.edge_embedding = nn.Linear(self.edge_input_dims[0], self.edge_dims[0])
        self.egnn = EGNNSparseNetwork(self.num_layers, self.node_dims[0], self.edge_dims[0])
        self.scalar_node_projection = nn.Linear(self.node_dims[0], h_input_dim_ + cond)

        # every sampling entry point routes to the generic loop (EquivariantVariationalDiffusion._mol_gen_sample_modules): the fused sampling
        # kernels of libgcdm_hip.so are GCPNet's
        self.fused_unsupported = "egnn"
        self._path = "fused"
        H, Eh = self.node_dims[0], self.edge_dims[0]
        self.fused_layers_unsupported = None
        if H % 32 or H > _native.EGNN_DYN_MAX_H:
            self.fused_layers_unsupported = f"h_hidden_dim = {H}: the fused layers take a multiple of 32 up to {_native.EGNN_DYN_MAX_H}"
        elif Eh > _native.EGNN_DYN_MAX_EH:
            self.fused_layers_unsupported = f"e_hidden_dim = {Eh}: the fused layers take up to {_native.EGNN_DYN_MAX_EH}"
        self.launches = 0                       # fused edge-kernel launches of this module so far (one per layer per fused forward)
        self.fused_forwards = 0
        self._train_path = "operators"
        self.train_fused_forwards = 0           # forwards that recorded a gradient on the fused training path
        self.train_edge_blocks = 0              # ops.egnn_edge_block calls of this module so far (one per layer per such forward)
        self._packed: Optional[torch.Tensor] = None
        self._packed_key: Any = None
        self._plan: Optional[_Plan] = None
        self._plan_src: Any = None
        self._plan_keep: Any = None

    # ---- the two paths ---------------------------------------------------------------------------------------------------------------------
    @property
    def path(self) -> str:
        return self._path

    def set_path(self, path: str) -> "EGNNDynamics":
        """"fused" (the default): the fused layers whenever no gradient is recorded and every node is present, the operators otherwise.
        "operators": the autograd operators always."""
        if path not in PATHS:
            raise ValueError(f"path must be one of {PATHS}, got {path!r}")
        self._path = path
        return self

    @property
    def train_path(self) -> str:
        return self._train_path

    def set_train_path(self, path: str) -> "EGNNDynamics":
        """The path of a forward that records a gradient.  "operators" (the default): the autograd operators.  "fused": ops.egnn_edge_block per
        layer whenever every node is present, the operators otherwise.  ``set_path`` keeps its meaning for forwards without a gradient."""
        if path not in TRAIN_PATHS:
            raise ValueError(f"train path must be one of {TRAIN_PATHS}, got {path!r}")
        if path == "fused":
            why = ops.egnn_edge_block_why_not(self.node_dims[0], self.edge_dims[0], self.edge_input_dims[0])
            if why is not None:
                raise NotImplementedError(f"the fused EGNN training path does not implement this configuration ({why})")
        self._train_path = path
        return self

    @contextlib.contextmanager
    def fp32_mfma(self):
        """Nothing to switch: both paths are exact fp32 MFMA (the drivers wrap their fp32 re-runs in this for GCPNetDynamics)."""
        yield

    # ---- plumbing --------------------------------------------------------------------------------------------------------------------------
    def _plan_of(self, batch_index: torch.Tensor, mask: Optional[torch.Tensor]) -> _Plan:
        """The plan of (batch_index, mask); consecutive calls with the same tensors (a sampling loop) share it.  The cache keeps the tensors
        alive, so that the allocator cannot hand their addresses to another batch while the key is held."""
        src = (batch_index.data_ptr(), batch_index.shape[0], _native.tensor_version(batch_index),
               None if mask is None else (mask.data_ptr(), mask.shape[0], _native.tensor_version(mask)))
        if self._plan is None or self._plan_src != src:
            self._plan, self._plan_src, self._plan_keep = _Plan(batch_index, mask), src, (batch_index, mask)
        return self._plan

    def _edge_index(self, plan: _Plan, mask: Optional[torch.Tensor], dev: torch.device) -> torch.Tensor:
        if plan.edge_index is None:
            with torch.inference_mode(False):
                ei = ops.fully_connected_edge_index(torch.tensor(plan.sizes, dtype=torch.int64), dev)
                if not plan.all_present:                               # edges of masked nodes do not exist (gcpnet.py:1062-1065)
                    mk = mask.detach().clone().bool()
                    ei = ei[:, mk[ei[0]] & mk[ei[1]]].contiguous()
                plan.edge_index = ei
        return plan.edge_index

    def _features(self, batch: Any, xh: torch.Tensor, t: torch.Tensor, sc: Optional[torch.Tensor], mf: torch.Tensor):
        """(x_init, node features, self-conditioning positions) of a call: the masked input split, with the self-conditioning, time and
        context columns appended in the reference's order."""
        nx, N = self.num_x_dims, xh.shape[0]
        xh = xh.to(torch.float32) * mf
        x_init, h = xh[:, :nx].contiguous(), xh[:, nx:]
        x_sc = None
        if self.self_condition:
            s = torch.zeros_like(xh) if sc is None else sc.to(torch.float32)
            x_sc = s[:, :nx].contiguous()
            h = torch.cat((h, s[:, nx:]), dim=-1)
        if self.condition_on_time:
            tt = t.to(torch.float32).reshape(-1, 1)
            h = torch.cat((h, tt.expand(N, 1) if tt.numel() == 1 else tt), dim=-1)
        if self.condition_on_context:
            ctx = cfg_get(batch, "props_context")
            if ctx is None:
                raise ValueError("props_context required by a context-conditioned model")
            h = torch.cat((h, ctx.to(torch.float32).reshape(N, self.num_context_node_features)), dim=-1)
        return x_init, h.contiguous(), x_sc

    def _finish(self, x: torch.Tensor, h: torch.Tensor, x_init: torch.Tensor, bi: torch.Tensor, mask: Optional[torch.Tensor], mf: torch.Tensor):
        """egnn.py:784-821: mask, projection, vel = (x - x_init) mask, all zero when any entry is NaN (decided on the device), CoM projection."""
        x, h = x * mf, h * mf
        h = ops.linear(h, self.scalar_node_projection.weight, self.scalar_node_projection.bias) * mf
        vel = (x - x_init) * mf
        if self.condition_on_context:
            h = h[:, : -self.num_context_node_features]
        if self.condition_on_time:
            h = h[:, :-1]
        vel = torch.where(vel.isnan().any(), torch.zeros_like(vel), vel)
        vel = ops.centralize(vel, bi, mask)
        return torch.cat((vel, h), dim=-1)

    # ---- the operators path ----------------------------------------------------------------------------------------------------------------
    def forward_operators(self, batch: Any, xh: torch.Tensor, t: torch.Tensor, xh_self_cond: Optional[torch.Tensor] = None,
                          probe: Optional[dict] = None) -> torch.Tensor:
        """atom_types_and_coords_forward (egnn.py:672-823) as the reference evaluates it, on the autograd operators.  ``probe``: a dict that
        receives per layer the receiver sums "m", "dx" and the LayerNorm output "ln" (detached)."""
        if torch.is_grad_enabled() and xh.requires_grad:
            raise NotImplementedError("EGNNDynamics (bio-diffusion_amd): gradients with respect to the input xh are not built (parameter gradients "
                                      "only -- the edge features of the network input have no backward); detach xh")
        bi, mask = cfg_get(batch, "batch"), cfg_get(batch, "mask")
        plan = self._plan_of(bi, mask)
        dev, N = xh.device, xh.shape[0]
        mf = torch.ones((N, 1), dtype=torch.float32, device=dev) if mask is None else mask.to(torch.float32).unsqueeze(-1)
        x_init, h, x_sc = self._features(batch, xh, t, xh_self_cond, mf)
        ei = self._edge_index(plan, mask, dev)
        g = ops.graph_of(ei, N)                                  # row = the receiver i, col = the sender j: the edge set is symmetric, and per
        # receiver the senders come in ascending order, which is the order the reference's sum at edge_index[1] adds them in
        e = ops.edge_features(x_init, ei)[0]
        if self.self_condition:
            e = torch.cat((e, ops.edge_features(x_sc, ei)[0]), dim=-1)
        x = ops.centralize(x_init, bi, mask)
        h = ops.linear(h, self.node_embedding.weight, self.node_embedding.bias) * mf
        e_attr = ops.linear(e, self.edge_embedding.weight, self.edge_embedding.bias)
        empty = g.E == 0
        for layer in self.egnn.mpnn_layers:
            if empty:
                raise ValueError("EGNNDynamics: a batch without edges (no present node)")
            rel = ops.gather_col(x, g) - ops.gather_row(x, g)                          # x_j - x_i
            rel_dist = (rel ** 2).sum(dim=-1, keepdim=True)
            pre = ops.linear(torch.cat([ops.gather_row(h, g), ops.gather_col(h, g), e_attr, rel_dist], dim=-1),
                             layer.edge_mlp[0].weight, layer.edge_mlp[0].bias)
            m_ij = ops.act(ops.linear(ops.act(pre, "silu"), layer.edge_mlp[3].weight, layer.edge_mlp[3].bias), "silu")
            w_ij = torch.tanh(ops.linear(ops.act(ops.linear(m_ij, layer.coors_mlp[0].weight, layer.coors_mlp[0].bias), "silu"),
                                         layer.coors_mlp[3].weight, layer.coors_mlp[3].bias))
            dx = ops.scatter_rows(w_ij * layer.coors_norm(rel), g)
            m_i = ops.scatter_rows(m_ij, g)
            ln = layer.node_norm(h, plan.graph_index, plan.B)
            if probe is not None:
                for k, v in (("m", m_i), ("dx", dx), ("ln", ln)):
                    probe.setdefault(k, []).append(v.detach())
            h = h + ops.linear(ops.act(ops.linear(torch.cat([ln, m_i], dim=-1), layer.node_mlp[0].weight, layer.node_mlp[0].bias), "silu"),
                               layer.node_mlp[3].weight, layer.node_mlp[3].bias)
            x = x + dx
        return self._finish(x, h, x_init, bi, mask, mf)

    # ---- the fused training path ------------------------------------------------------------------------------------------------------------
    def forward_train_fused(self, batch: Any, xh: torch.Tensor, t: torch.Tensor, xh_self_cond: Optional[torch.Tensor] = None,
                            probe: Optional[dict] = None) -> torch.Tensor:
        """forward_operators with the per-edge part of every layer on ops.egnn_edge_block; every node must be present."""
        if torch.is_grad_enabled() and xh.requires_grad:
            raise NotImplementedError("EGNNDynamics (bio-diffusion_amd): gradients with respect to the input xh are not built (parameter gradients "
                                      "only -- the edge features of the network input have no backward); detach xh")
        bi, mask = cfg_get(batch, "batch"), cfg_get(batch, "mask")
        plan = self._plan_of(bi, mask)
        if not plan.all_present:
            raise ValueError("the fused EGNN training path serves batches without masked nodes; use the operators path")
        dev, N = xh.device, xh.shape[0]
        H, Eh, e_in, _ = self._dims()
        mf = torch.ones((N, 1), dtype=torch.float32, device=dev)
        x_init, h, x_sc = self._features(batch, xh, t, xh_self_cond, mf)
        x = ops.centralize(x_init, bi, None)
        h = ops.linear(h, self.node_embedding.weight, self.node_embedding.bias)
        fold = torch.cat((self.edge_embedding.weight.t(), self.edge_embedding.bias[None, :]), dim=0)        # [e_in + 1, Eh]
        for layer in self.egnn.mpnn_layers:
            W1, b1 = layer.edge_mlp[0].weight, layer.edge_mlp[0].bias
            F = ops.linear(W1[:, 2 * H:2 * H + Eh], fold)                     # [2 D, e_in + 1]: u (, u'), W_e b_emb
            V = torch.stack((F[:, 0], F[:, 1] if e_in == 2 else torch.zeros_like(F[:, 0]), W1[:, 2 * H + Eh]), dim=0)
            A = ops.linear(h, W1[:, :H], b1 + F[:, e_in])
            B = ops.linear(h, W1[:, H:2 * H])
            m_i, dx = ops.egnn_edge_block(A, B, V, layer.edge_mlp[3].weight, layer.edge_mlp[3].bias, layer.coors_mlp[0].weight,
                                          layer.coors_mlp[0].bias, layer.coors_mlp[3].weight, layer.coors_mlp[3].bias, layer.coors_norm.scale,
                                          x, x_init, x_sc, plan.node_offsets, plan.node_mol, H, Eh)
            self.train_edge_blocks += 1
            ln = layer.node_norm(h, plan.graph_index, plan.B)
            if probe is not None:
                for k, v in (("m", m_i), ("dx", dx), ("ln", ln)):
                    probe.setdefault(k, []).append(v.detach())
            h = h + ops.linear(ops.act(ops.linear(torch.cat([ln, m_i], dim=-1), layer.node_mlp[0].weight, layer.node_mlp[0].bias), "silu"),
                               layer.node_mlp[3].weight, layer.node_mlp[3].bias)
            x = x + dx
        self.train_fused_forwards += 1
        return self._finish(x, h, x_init, bi, None, mf)

    # ---- the fused path --------------------------------------------------------------------------------------------------------------------
    def _ordered(self) -> List[torch.Tensor]:
        """The tensors in the order gcdm_egnn_dyn_pack takes them."""
        out = [self.edge_embedding.weight, self.edge_embedding.bias]
        for layer in self.egnn.mpnn_layers:
            out += [layer.edge_mlp[0].weight, layer.edge_mlp[0].bias, layer.edge_mlp[3].weight, layer.edge_mlp[3].bias, layer.node_norm.weight,
                    layer.node_norm.bias, layer.coors_norm.scale, layer.node_mlp[0].weight, layer.node_mlp[0].bias, layer.node_mlp[3].weight,
                    layer.node_mlp[3].bias, layer.coors_mlp[0].weight, layer.coors_mlp[0].bias, layer.coors_mlp[3].weight, layer.coors_mlp[3].bias]
        return out

    def _dims(self) -> Tuple[int, int, int, int]:
        return self.node_dims[0], self.edge_dims[0], self.edge_input_dims[0], self.num_layers

    def _weights(self, lib, dev: torch.device) -> torch.Tensor:
        """The packed weights, re-packed once per weight change (one small kernel per tensor: the column split and the folded edge embedding)."""
        ts = self._ordered()
        key = tuple((t.data_ptr(), _native.tensor_version(t)) for t in ts)
        if self._packed is not None and key == self._packed_key and self._packed.device == dev:
            return self._packed
        for t in ts:
            if not t.is_cuda or t.device != dev:
                raise ValueError(f"EGNNDynamics parameters live on {t.device}, the inputs on {dev}: move the module with .to(device)")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("EGNNDynamics parameters must be contiguous fp32 tensors")
        H, Eh, e_in, L = self._dims()
        nbytes = int(lib.gcdm_egnn_dyn_workspace_bytes(1, 0, H, Eh, e_in, L))
        if nbytes < 0:
            raise _native.NativeError(lib.gcdm_egnn_dyn_last_error().decode())
        with torch.inference_mode(False):
            packed = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        table = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        st = lib.gcdm_egnn_dyn_pack(table, len(ts), H, Eh, e_in, L, C.c_void_p(packed.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if st != 0:
            raise _native.NativeError(f"gcdm_egnn_dyn_pack failed: {lib.gcdm_egnn_dyn_last_error().decode()}")
        self._packed, self._packed_key = packed, key
        return packed

    @torch.no_grad()
    def forward_fused(self, batch: Any, xh: torch.Tensor, t: torch.Tensor, xh_self_cond: Optional[torch.Tensor] = None,
                      probe: Optional[dict] = None) -> torch.Tensor:
        """The same forward with every layer on include/gcdm_egnn_dynamics.h; every node must be present.  8 launches per layer."""
        if self.fused_layers_unsupported is not None:
            raise NotImplementedError(f"the fused EGNN layers do not implement this configuration ({self.fused_layers_unsupported})")
        bi, mask = cfg_get(batch, "batch"), cfg_get(batch, "mask")
        plan = self._plan_of(bi, mask)
        if not plan.all_present:
            raise ValueError("the fused EGNN layers serve batches without masked nodes; use the operators path")
        dev, N = xh.device, xh.shape[0]
        H, Eh, e_in, L = self._dims()
        mf = torch.ones((N, 1), dtype=torch.float32, device=dev)
        x_init, h, x_sc = self._features(batch, xh, t, xh_self_cond, mf)
        lib = _native.load_ops()
        with torch.cuda.device(dev):
            W = self._weights(lib, dev)
            x = ops.centralize(x_init, bi, None)
            h = ops.linear(h, self.node_embedding.weight, self.node_embedding.bias)
            ws = torch.empty(int(lib.gcdm_egnn_dyn_workspace_bytes(0, N, H, Eh, e_in, L)) // 4, dtype=torch.float32, device=dev)
            h2, x2 = torch.empty_like(h), torch.empty_like(x)
            st_ = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for l in range(L):
                dbg = [None, None, None]
                if probe is not None:
                    dbg = [torch.empty((N, M_DIM), device=dev), torch.empty((N, 3), device=dev), torch.empty((N, H), device=dev)]
                    for k, v in zip(("m", "dx", "ln"), dbg):
                        probe.setdefault(k, []).append(v)
                st = lib.gcdm_egnn_dyn_layer(l, ops._p(h), ops._p(x), ops._p(x_init), ops._p(x_sc), ops._p(plan.node_offsets), ops._p(plan.node_mol),
                                             ops._p(W), ops._p(ws), ops._p(h2), ops._p(x2), ops._p(dbg[0]), ops._p(dbg[1]), ops._p(dbg[2]),
                                             N, plan.B, H, Eh, e_in, L, st_)
                if st != 0:
                    raise _native.NativeError(f"gcdm_egnn_dyn_layer failed: {lib.gcdm_egnn_dyn_last_error().decode()}")
                h, h2, x, x2 = h2, h, x2, x
                if N:
                    self.launches += 1
            self.fused_forwards += 1
            return self._finish(x, h, x_init, bi, None, mf)

    # ----------------------------------------------------------------------------------------------------------------------------------------
    def _use_fused(self, xh: torch.Tensor, bi: torch.Tensor, mask: Optional[torch.Tensor]) -> bool:
        if self._path == "operators" or self.fused_layers_unsupported is not None:
            return False
        if torch.is_grad_enabled() and (xh.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        return self._plan_of(bi, mask).all_present

    def _use_train_fused(self, xh: torch.Tensor, bi: torch.Tensor, mask: Optional[torch.Tensor]) -> bool:
        if self._train_path != "fused" or not torch.is_grad_enabled() or not any(p.requires_grad for p in self.parameters()):
            return False
        return self._plan_of(bi, mask).all_present

    def forward(self, batch: Any, xh: torch.Tensor, t: torch.Tensor, **kwargs: Any) -> Tuple[Any, torch.Tensor]:
        sc = kwargs.get("xh_self_cond")
        if sc is not None and not self.self_condition:
            sc = None                  # as the reference: the input is ignored unless diffusion_cfg.self_condition (egnn.py:715)
        if xh.device.type != "cuda":
            raise RuntimeError("EGNNDynamics (bio-diffusion_amd) runs on an MI355X only: tensors must be on a HIP ('cuda') device; there is no CPU fallback")
        if self._use_fused(xh, cfg_get(batch, "batch"), cfg_get(batch, "mask")):
            return batch, self.forward_fused(batch, xh, t, xh_self_cond=sc)
        if self._use_train_fused(xh, cfg_get(batch, "batch"), cfg_get(batch, "mask")):
            return batch, self.forward_train_fused(batch, xh, t, xh_self_cond=sc)
        return batch, self.forward_operators(batch, xh, t, xh_self_cond=sc)
