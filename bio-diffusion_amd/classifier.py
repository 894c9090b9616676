"""The reference's EGNN property classifier (src/__init__.py: E_GCL / E_GCL_mask / EGNN :233-419, get_classifier :98,
train_with_property_classifier's evaluation arm :145-204) as one fused HIP launch per forward (include/gcdm_classifier.h), and the bookkeeping
of its two evaluation workflows: the MAE of the classifier's prediction against the property that was asked for.

The default ("fused") path is forward only, evaluation mode, fp32 on the exact fp32 MFMA, no float atomics: a molecule's prediction is
bit-identical from run to run and does not depend on what else is in the batch or where the molecule sits in it.  There is no CPU / eager
path: CPU tensors raise.

Training (train_with_property_classifier's training arm :145-204) runs on the opt-in "operators" path: the same network composed from the
autograd operators of libgcdm_ops.so (ops.linear / act / gather_row / gather_col / scatter_rows and the column-split first edge layer,
include/gcdm_classifier_train.h), so ``pred.backward()`` fills every parameter's ``.grad``.  ``train_epoch`` is the reference's loop and
``save_classifier`` writes what ``get_classifier`` reads."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import pickle
from typing import Any, Iterable, List, Optional, Tuple, Union

import torch
from torch import nn

from . import _native, ops

MAX_NODES = _native.CLASSIFIER_MAX_NODES                  # atoms per molecule
MAX_IN_NODE_NF = _native.CLASSIFIER_MAX_IN_NODE_NF
MAX_HIDDEN_NF = _native.CLASSIFIER_MAX_HIDDEN_NF
LAUNCHES_PER_FORWARD = 1                                  # gcdm_classifier_workspace_bytes(2, ...)
PATHS = ("fused", "operators")                            # one launch, forward only | autograd operators, differentiable
EDGE_INPUTS = ("split", "concat")                         # edge_mlp.0 split by columns (ops.classifier_edge_pre) | on torch.cat, as the reference


class _GCL(nn.Module):
    """Parameter holder with E_GCL_mask's state-dict names (edge_mlp.{0,2}, node_mlp.{0,2}, att_mlp.0); it is never called."""

    def __init__(self, hidden_nf: int, nodes_attr_dim: int, attention: bool):
        super().__init__()
        H = hidden_nf
        self.edge_mlp = nn.Sequential(nn.Linear(2 * H + 1, H), nn.SiLU(), nn.Linear(H, H), nn.SiLU())
        self.node_mlp = nn.Sequential(nn.Linear(2 * H + nodes_attr_dim, H), nn.SiLU(), nn.Linear(H, H))
        if attention:
            self.att_mlp = nn.Sequential(nn.Linear(H, 1), nn.Sigmoid())


def _check_sizes(in_node_nf: int, hidden_nf: int, n_layers: int) -> None:
    if not 1 <= int(in_node_nf) <= MAX_IN_NODE_NF:
        raise ValueError(f"in_node_nf = {in_node_nf}: the fused classifier takes 1 .. {MAX_IN_NODE_NF} (MAX_IN_NODE_NF)")
    if not 32 <= int(hidden_nf) <= MAX_HIDDEN_NF or int(hidden_nf) % 32:
        raise ValueError(f"hidden_nf = {hidden_nf}: the fused classifier takes a multiple of 32 up to {MAX_HIDDEN_NF} (MAX_HIDDEN_NF)")
    if int(n_layers) < 1:
        raise ValueError(f"n_layers = {n_layers}: at least 1")


def _sum_rows(v: torch.Tensor, graph: "ops.Graph") -> torch.Tensor:
    """ops.scatter_rows; a graph without rows to add (a batch of one-atom or empty molecules) gives zeros that still depend on ``v``, so
    the parameters behind it get their (zero) gradients."""
    if graph.E == 0:
        return v.new_zeros((graph.N, v.shape[1])) + v.sum(0)
    return ops.scatter_rows(v, graph)


def _take(h: torch.Tensor, graph: "ops.Graph", by_row: bool) -> torch.Tensor:
    """ops.gather_row / ops.gather_col; the empty selection of a graph without edges is taken by indexing."""
    if graph.E == 0:
        return h[graph.row if by_row else graph.col]
    return ops.gather_row(h, graph) if by_row else ops.gather_col(h, graph)


class EGNN(nn.Module):
    """``EGNN(in_node_nf, in_edge_nf, hidden_nf, device, act_fn, n_layers, coords_weight, attention, node_attr)`` with exactly the reference's
    state-dict keys and shapes (E_GCL_mask deletes ``coord_mlp``, so there is none).  ``coords_weight`` is accepted and unused, as in the
    reference (coordinates are never updated).  Limits: ``in_node_nf`` <= 16, ``hidden_nf`` a multiple of 32 up to 256, molecules of up to
    ``MAX_NODES`` = 32 atoms."""

    def __init__(self, in_node_nf: int, in_edge_nf: int = 0, hidden_nf: int = 128, device: Any = "cuda", act_fn: Optional[nn.Module] = None,
                 n_layers: int = 4, coords_weight: float = 1.0, attention: Any = False, node_attr: Any = 1):
        super().__init__()
        if in_edge_nf:
            raise NotImplementedError("in_edge_nf > 0: edge attributes are not built (no reference caller uses them)")
        if act_fn is not None and not isinstance(act_fn, nn.SiLU):
            raise NotImplementedError(f"act_fn {type(act_fn).__name__}: only SiLU is built (no reference caller uses another)")
        _check_sizes(in_node_nf, hidden_nf, n_layers)
        self.in_node_nf, self.hidden_nf, self.n_layers = int(in_node_nf), int(hidden_nf), int(n_layers)
        self.attention, self.node_attr = bool(attention), bool(node_attr)
        self.embedding = nn.Linear(self.in_node_nf, self.hidden_nf)
        for i in range(self.n_layers):
            self.add_module(f"gcl_{i}", _GCL(self.hidden_nf, self.in_node_nf if self.node_attr else 0, self.attention))
        H = self.hidden_nf
        self.node_dec = nn.Sequential(nn.Linear(H, H), nn.SiLU(), nn.Linear(H, H))
        self.graph_dec = nn.Sequential(nn.Linear(H, H), nn.SiLU(), nn.Linear(H, 1))
        self.device = device
        self._packed: Optional[torch.Tensor] = None
        self._packed_key: Any = None
        self.launches = 0                                  # kernel launches of the fused forwards so far (the pack is not counted)
        self._path, self._edge_input = "fused", "split"
        self._edges: Optional[ops.MoleculeEdges] = None
        self._edges_key: Any = None
        self.to(device)

    # ---- the two paths ---------------------------------------------------------------------------------------------------------------------
    @property
    def path(self) -> str:
        return self._path

    def set_path(self, path: str) -> "EGNN":
        """"fused" (the default): one launch per forward, no graph is recorded whatever the grad mode.  "operators": the network on the
        autograd operators of libgcdm_ops.so, differentiable with respect to every parameter."""
        if path not in PATHS:
            raise ValueError(f"path must be one of {PATHS}, got {path!r}")
        self._path = path
        return self

    @property
    def edge_input(self) -> str:
        return self._edge_input

    def set_edge_input(self, mode: str) -> "EGNN":
        """How the "operators" path evaluates edge_mlp.0.  "split" (the default): W = [W_s | W_t | w_r], two node-level GEMMs and
        ops.classifier_edge_pre.  "concat": ops.linear on torch.cat([h[row], h[col], radial]), the reference's formulation."""
        if mode not in EDGE_INPUTS:
            raise ValueError(f"edge input must be one of {EDGE_INPUTS}, got {mode!r}")
        self._edge_input = mode
        return self

    # ---- weights -------------------------------------------------------------------------------------------------------------------------
    def _ordered(self) -> List[Optional[torch.Tensor]]:
        """The tensors in the order gcdm_classifier_pack takes them."""
        out: List[Optional[torch.Tensor]] = [self.embedding.weight, self.embedding.bias]
        for i in range(self.n_layers):
            g = getattr(self, f"gcl_{i}")
            out += [g.edge_mlp[0].weight, g.edge_mlp[0].bias, g.edge_mlp[2].weight, g.edge_mlp[2].bias,
                    g.node_mlp[0].weight, g.node_mlp[0].bias, g.node_mlp[2].weight, g.node_mlp[2].bias]
            out += [g.att_mlp[0].weight, g.att_mlp[0].bias] if self.attention else [None, None]
        out += [self.node_dec[0].weight, self.node_dec[0].bias, self.node_dec[2].weight, self.node_dec[2].bias,
                self.graph_dec[0].weight, self.graph_dec[0].bias, self.graph_dec[2].weight, self.graph_dec[2].bias]
        return out

    def _weights(self, lib, dev: torch.device) -> torch.Tensor:
        ts = self._ordered()
        key = tuple((t.data_ptr(), _native.tensor_version(t)) for t in ts if t is not None)
        if self._packed is not None and key == self._packed_key and self._packed.device == dev:
            return self._packed
        for t in ts:
            if t is None:
                continue
            if not t.is_cuda or t.device != dev:
                raise ValueError(f"classifier parameters live on {t.device}, the inputs on {dev}: move the module with .to(device)")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("classifier parameters must be contiguous fp32 tensors")
        nbytes = int(lib.gcdm_classifier_workspace_bytes(1, 0, self.in_node_nf, self.hidden_nf, self.n_layers))
        if nbytes < 0:
            raise _native.NativeError(lib.gcdm_classifier_last_error().decode())
        packed = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        table = (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
        st = lib.gcdm_classifier_pack(table, len(ts), self.in_node_nf, self.hidden_nf, self.n_layers, int(self.attention), int(self.node_attr),
                                      C.c_void_p(packed.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if st != 0:
            raise _native.NativeError(f"gcdm_classifier_pack failed: {lib.gcdm_classifier_last_error().decode()}")
        self._packed, self._packed_key = packed, key
        return packed

    # ---- the ragged entry ----------------------------------------------------------------------------------------------------------------
    def predict(self, x: torch.Tensor, one_hot: torch.Tensor, num_nodes: Optional[torch.Tensor] = None,
                batch_index: Optional[torch.Tensor] = None, debug_layer: Optional[int] = None):
        """One scalar per molecule on the current path (``set_path``): the fused launch below, or the autograd operators."""
        if self._path == "operators":
            return self._predict_operators(x, one_hot, num_nodes, batch_index, debug_layer)
        return self._predict_fused(x, one_hot, num_nodes, batch_index, debug_layer)

    def _edges_of(self, num_nodes, dev: torch.device) -> "ops.MoleculeEdges":
        sizes = tuple(int(v) for v in torch.as_tensor(num_nodes).detach().reshape(-1).tolist())
        key = (sizes, dev)
        if self._edges is None or self._edges_key != key:                # consecutive steps on batches of the same sizes share the tables
            self._edges, self._edges_key = ops.MoleculeEdges(sizes, dev), key
        return self._edges

    def _predict_operators(self, x, one_hot, num_nodes, batch_index, debug_layer):
        """predict() on the autograd operators: EGNN.forward / E_GCL_mask.forward (src/__init__.py:363-419) over the real atoms and the
        ordered pairs i != j of each molecule -- the reference adds exact zeros for the masked pairs, so this is the same sum.  The molecule
        sizes are read on the host (one synchronisation when they live on the device): they size the edge buffers."""
        if not (x.is_cuda and one_hot.is_cuda):
            raise ValueError(f"the classifier runs on the GPU only: x is on {x.device}, one_hot on {one_hot.device}")
        dev, N, H = x.device, x.shape[0], self.hidden_nf
        if x.dim() != 2 or x.shape[1] != 3 or one_hot.dim() != 2 or tuple(one_hot.shape) != (N, self.in_node_nf):
            raise ValueError(f"x must be [N, 3] and one_hot [N, {self.in_node_nf}]; got {tuple(x.shape)} and {tuple(one_hot.shape)}")
        if num_nodes is None:
            if batch_index is None:
                raise ValueError("predict needs num_nodes or batch_index")
            B = int(batch_index[-1]) + 1 if N else 0
            num_nodes = torch.zeros(B, dtype=torch.long, device=dev).index_add_(0, batch_index.to(dev), torch.ones(N, dtype=torch.long, device=dev))
        edges = self._edges_of(num_nodes, dev)
        if edges.N != N:
            raise ValueError(f"num_nodes adds up to {edges.N} atoms, x holds {N}")
        if edges.sizes and max(edges.sizes) > MAX_NODES:
            raise ValueError(f"a molecule of {max(edges.sizes)} atoms: the classifier takes molecules of up to {MAX_NODES} atoms (MAX_NODES)")
        for p in self.parameters():
            if p.device != dev:
                raise ValueError(f"classifier parameters live on {p.device}, the inputs on {dev}: move the module with .to(device)")
        x = x.detach().to(torch.float32).contiguous()                    # positions are data: no gradient reaches them
        h0 = one_hot.to(torch.float32).contiguous()
        split = self._edge_input == "split"
        with torch.cuda.device(dev):
            g = edges.graph
            if not split:
                d = x[g.row] - x[g.col]
                radial = (d * d).sum(1, keepdim=True)                    # coord2radial; data, like x
            h = ops.linear(h0, self.embedding.weight, self.embedding.bias)
            kept = h if debug_layer == 0 else None
            for i in range(self.n_layers):
                gcl = getattr(self, f"gcl_{i}")
                W0, b0 = gcl.edge_mlp[0].weight, gcl.edge_mlp[0].bias
                if split:
                    pre = ops.classifier_edge_pre(ops.linear(h, W0[:, :H], b0), ops.linear(h, W0[:, H:2 * H]), x, W0[:, 2 * H], edges)
                else:
                    pre = ops.linear(torch.cat([_take(h, g, True), _take(h, g, False), radial], 1), W0, b0)
                m = ops.act(ops.linear(ops.act(pre, "silu"), gcl.edge_mlp[2].weight, gcl.edge_mlp[2].bias), "silu")
                if self.attention:
                    m = m * ops.act(ops.linear(m, gcl.att_mlp[0].weight, gcl.att_mlp[0].bias), "sigmoid")
                agg = _sum_rows(m, g)
                inp = torch.cat([h, agg, h0], 1) if self.node_attr else torch.cat([h, agg], 1)
                h = h + ops.linear(ops.act(ops.linear(inp, gcl.node_mlp[0].weight, gcl.node_mlp[0].bias), "silu"),
                                   gcl.node_mlp[2].weight, gcl.node_mlp[2].bias)
                if debug_layer == i + 1:
                    kept = h
            y = ops.linear(ops.act(ops.linear(h, self.node_dec[0].weight, self.node_dec[0].bias), "silu"), self.node_dec[2].weight, self.node_dec[2].bias)
            pooled = _sum_rows(y, edges.pool)
            a = ops.act(ops.linear(pooled, self.graph_dec[0].weight, self.graph_dec[0].bias), "silu")
            pred = ops.linear(a, self.graph_dec[2].weight, self.graph_dec[2].bias).squeeze(1)
        return (pred, kept) if debug_layer is not None else pred

    @torch.no_grad()
    def _predict_fused(self, x: torch.Tensor, one_hot: torch.Tensor, num_nodes: Optional[torch.Tensor] = None,
                       batch_index: Optional[torch.Tensor] = None, debug_layer: Optional[int] = None):
        """One scalar per molecule from what ``sample()`` / ``optimize()`` return: ``x`` [N, 3], ``one_hot`` [N, in_node_nf], atoms of a molecule
        contiguous.  With ``num_nodes`` (sizes per molecule, on any device) nothing synchronises and the samples are not copied: one launch on
        the current stream.  With ``batch_index`` alone the number of molecules is read from its last entry (one host sync).  A molecule of
        more than ``MAX_NODES`` atoms gets NaN.  ``debug_layer`` k additionally returns h [N, hidden_nf] after layer k (0: the embedding)."""
        if not (x.is_cuda and one_hot.is_cuda):
            raise ValueError(f"the classifier runs on the GPU only: x is on {x.device}, one_hot on {one_hot.device}")
        dev = x.device
        N = x.shape[0]
        if x.dim() != 2 or x.shape[1] != 3 or one_hot.dim() != 2 or tuple(one_hot.shape) != (N, self.in_node_nf):
            raise ValueError(f"x must be [N, 3] and one_hot [N, {self.in_node_nf}]; got {tuple(x.shape)} and {tuple(one_hot.shape)}")
        if num_nodes is None:
            if batch_index is None:
                raise ValueError("predict needs num_nodes or batch_index")
            B = int(batch_index[-1]) + 1 if N else 0
            num_nodes = torch.zeros(B, dtype=torch.long, device=dev).index_add_(0, batch_index.to(dev), torch.ones(N, dtype=torch.long, device=dev))
        num_nodes = torch.as_tensor(num_nodes)
        B = int(num_nodes.shape[0])
        if N > B * MAX_NODES:
            raise ValueError(f"{N} atoms in {B} molecules: the fused classifier takes molecules of up to {MAX_NODES} atoms (MAX_NODES)")
        noff = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        noff[1:] = torch.cumsum(num_nodes.to(dev, non_blocking=True), 0)
        x = x if x.dtype == torch.float32 and x.is_contiguous() else x.to(torch.float32).contiguous()
        h0 = one_hot if one_hot.dtype == torch.float32 and one_hot.is_contiguous() else one_hot.to(torch.float32).contiguous()
        lib = _native.load_ops()
        with torch.cuda.device(dev):
            W = self._weights(lib, dev)
            ws = torch.empty(int(lib.gcdm_classifier_workspace_bytes(0, N, self.in_node_nf, self.hidden_nf, self.n_layers)) // 4,
                             dtype=torch.float32, device=dev)
            pred = torch.empty(B, dtype=torch.float32, device=dev)
            dbg = -1 if debug_layer is None else int(debug_layer)
            hd = torch.empty((N, self.hidden_nf), dtype=torch.float32, device=dev) if dbg >= 0 else None
            st = lib.gcdm_classifier_forward(C.c_void_p(x.data_ptr()), C.c_void_p(h0.data_ptr()), C.c_void_p(noff.data_ptr()),
                                             C.c_void_p(W.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(pred.data_ptr()),
                                             C.c_void_p(hd.data_ptr() if hd is not None else None), dbg, N, B, self.in_node_nf, self.hidden_nf,
                                             self.n_layers, int(self.attention), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if st != 0:
            raise _native.NativeError(f"gcdm_classifier_forward failed: {lib.gcdm_classifier_last_error().decode()}")
        if B:
            self.launches += LAUNCHES_PER_FORWARD
        return (pred, hd) if hd is not None else pred

    # ---- the reference's dense entry -------------------------------------------------------------------------------------------------------
    def forward(self, h0: torch.Tensor, x: torch.Tensor, edges: Any = None, edge_attr: Any = None, node_mask: Optional[torch.Tensor] = None,
                edge_mask: Optional[torch.Tensor] = None, n_nodes: Optional[int] = None) -> torch.Tensor:
        """The reference's call: ``h0`` [B n, F], ``x`` [B n, 3], ``node_mask`` [B n, 1], ``edge_mask`` [B n n, 1], ``n_nodes`` = n; returns
        pred [B].  ``edges`` is accepted and IGNORED: the reference always passes the full n x n adjacency of every molecule, which is what the
        kernel evaluates.  ``node_mask`` must be a prefix mask per molecule (both reference data loaders build it that way); ``edge_mask``, when
        given, must be "both atoms real, off the diagonal" -- it is compared on the device and a mismatch raises.  The padded form is an entry
        point only: real atoms are gathered into the ragged layout ``predict`` runs on."""
        if edge_attr is not None:
            raise NotImplementedError("edge_attr: edge attributes are not built (no reference caller uses them)")
        if not (h0.is_cuda and x.is_cuda):
            raise ValueError(f"the classifier runs on the GPU only: h0 is on {h0.device}, x on {x.device}")
        if n_nodes is None or node_mask is None:
            raise ValueError("forward needs node_mask and n_nodes (the ragged entry is predict())")
        n = int(n_nodes)
        if n > MAX_NODES:
            raise ValueError(f"n_nodes = {n}: the fused classifier takes molecules of up to {MAX_NODES} atoms (MAX_NODES)")
        with torch.no_grad():                                  # the masks and the inputs are data on either path
            B = x.shape[0] // n
            m = node_mask.to(x.device).reshape(B, n) != 0
            num_nodes = m.sum(1)
            prefix = torch.arange(n, device=x.device)[None, :] < num_nodes[:, None]
            if not bool((m == prefix).all()):
                raise ValueError("node_mask is not a prefix mask per molecule (real atoms first, padding after)")
            if edge_mask is not None:
                want = (m[:, :, None] & m[:, None, :]) & ~torch.eye(n, dtype=torch.bool, device=x.device)[None]
                if edge_mask.numel() != want.numel() or not bool(((edge_mask.to(x.device).reshape(B, n, n) != 0) == want).all()):
                    raise ValueError("edge_mask is not 'both atoms real, off the diagonal': other edge sets are not built")
            keep = m.reshape(-1)
            xs, hs = x[keep], h0[keep]
        return self.predict(xs, hs, num_nodes=num_nodes)


# ---- the reference's on-disk format --------------------------------------------------------------------------------------------------------
class _ArgsUnpickler(pickle.Unpickler):
    """args.pickle is an argparse.Namespace of plain values: nothing else is resolvable, so a crafted file cannot reach code."""
    _ALLOWED = {("argparse", "Namespace"), ("builtins", "dict"), ("builtins", "list"), ("builtins", "tuple"), ("builtins", "set"),
                ("builtins", "frozenset"), ("builtins", "int"), ("builtins", "float"), ("builtins", "bool"), ("builtins", "str"),
                ("builtins", "bytes"), ("collections", "OrderedDict")}

    def find_class(self, module, name):
        if (module, name) in self._ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"args.pickle names {module}.{name}: only argparse.Namespace and plain containers are admitted")


def load_classifier_args(path: str) -> argparse.Namespace:
    with open(path, "rb") as f:
        args = _ArgsUnpickler(f).load()
    if not isinstance(args, argparse.Namespace):
        raise pickle.UnpicklingError(f"{path} does not hold an argparse.Namespace")
    return args


def get_classifier(model_dir: str = "", device: Union[torch.device, str] = "cuda") -> EGNN:
    """src/__init__.py:98-114: ``args.pickle`` (nf, n_layers, attention, node_attr; in_node_nf = 5 as get_classifier_model) and
    ``best_checkpoint.npy`` (a torch.save state dict, read with weights_only)."""
    args = load_classifier_args(os.path.join(model_dir, "args.pickle"))
    model = EGNN(in_node_nf=5, in_edge_nf=0, hidden_nf=args.nf, device=device, n_layers=args.n_layers, coords_weight=1.0,
                 attention=args.attention, node_attr=args.node_attr)
    sd = torch.load(os.path.join(model_dir, "best_checkpoint.npy"), map_location="cpu", weights_only=True)
    model.load_state_dict(sd)
    return model.eval()


# ---- the evaluation arm ----------------------------------------------------------------------------------------------------------------------
def _batch_pred_label(classifier: EGNN, data: Any, property: str) -> Tuple[torch.Tensor, torch.Tensor]:
    if isinstance(data, dict):                        # the reference's dense batch (train_with_property_classifier :171-182)
        B, n, _ = data["positions"].shape
        dev = next(classifier.parameters()).device
        x = data["positions"].reshape(B * n, -1).to(dev, torch.float32)
        mask = data["atom_mask"].reshape(B * n, -1).to(dev, torch.float32)
        h0 = data["one_hot"].to(dev, torch.float32).reshape(B * n, -1)
        pred = classifier(h0=h0, x=x, edges=None, edge_attr=None, node_mask=mask, edge_mask=data["edge_mask"].to(dev, torch.float32), n_nodes=n)
        return pred, data[property].to(dev, torch.float32)
    x, one_hot, num_nodes, label = data               # ragged: what sample() / optimize() return plus the sizes and the label
    return classifier.predict(x, one_hot, num_nodes=num_nodes), torch.as_tensor(label).to(x.device, torch.float32)


@torch.no_grad()
def property_mae(classifier: EGNN, batches: Iterable[Any], mean: float, mad: float, property: str = "alpha",
                 return_per_batch: bool = False):
    """The evaluation arm of train_with_property_classifier: per batch ``mean(|mad pred + mean - label|)``, accumulated with weight batch_size
    and divided by the number of molecules.  ``batches`` yields the reference's dense dicts (positions, atom_mask, edge_mask, one_hot,
    <property>) or ragged tuples ``(x, one_hot, num_nodes, label)``.  The error is reduced on the device; one scalar per batch reaches the host."""
    total, count, per_batch = 0.0, 0, []
    for data in batches:
        pred, label = _batch_pred_label(classifier, data, property)
        loss = (mad * pred + mean - label.reshape(-1)).abs().mean().item()
        bs = int(pred.shape[0])
        total += loss * bs
        count += bs
        per_batch.append(loss)
    if count == 0:
        raise ValueError("property_mae got no batch")
    return (total / count, per_batch) if return_per_batch else total / count


# ---- the training arm ------------------------------------------------------------------------------------------------------------------------
def train_epoch(model: EGNN, batches: Iterable[Any], mean: float, mad: float, property: str, optimizer: Optional[torch.optim.Optimizer] = None,
                lr_scheduler: Any = None, partition: str = "train") -> float:
    """One epoch of train_with_property_classifier / test_with_property_classifier (src/__init__.py:145-230).  ``partition`` "train": the
    scheduler is stepped once, before the first batch, as the reference does; per batch ``zero_grad``, the L1 loss of the prediction
    against ``(label - mean) / mad``, ``backward`` and ``optimizer.step()`` -- the model must be on the "operators" path and the optimiser is
    the caller's.  Any other partition: evaluation mode, no graph, the L1 loss of ``mad pred + mean`` against the label, on whichever path
    the model is set to.  ``batches`` yields what ``property_mae`` takes.  Returns the mean loss weighted by batch size; the losses are
    accumulated on the device and one scalar reaches the host per epoch."""
    train = partition == "train"
    if train:
        if optimizer is None:
            raise ValueError("train_epoch: the training partition needs an optimizer")
        if model.path != "operators":
            raise ValueError('train_epoch: the fused path records no graph; call model.set_path("operators") to train')
        if lr_scheduler is not None:
            lr_scheduler.step()
    total, count = None, 0
    for data in batches:
        if train:
            model.train()
            optimizer.zero_grad()
            pred, label = _batch_pred_label(model, data, property)
            loss = (pred - (label.reshape(-1) - mean) / mad).abs().mean()
            loss.backward()
            optimizer.step()
        else:
            model.eval()
            with torch.no_grad():
                pred, label = _batch_pred_label(model, data, property)
                loss = (mad * pred + mean - label.reshape(-1)).abs().mean()
        bs = int(pred.shape[0])
        term = loss.detach() * bs
        total = term if total is None else total + term
        count += bs
    if count == 0:
        raise ValueError("train_epoch got no batch")
    return float(total) / count


def save_classifier(model: EGNN, model_dir: str, **args: Any) -> None:
    """Writes what ``get_classifier(model_dir)`` reads: ``args.pickle``, an argparse.Namespace with nf, n_layers, attention and node_attr of
    the model plus ``args`` (plain values: property, lr, ...; they may not contradict the model), and ``best_checkpoint.npy``, the state dict on
    the CPU through torch.save.  The reference's loader fixes in_node_nf = 5, so another width is refused here, not at load time."""
    if model.in_node_nf != 5:
        raise ValueError(f"in_node_nf = {model.in_node_nf}: get_classifier builds the model with in_node_nf = 5 (get_classifier_model)")
    own = {"nf": model.hidden_nf, "n_layers": model.n_layers, "attention": int(model.attention), "node_attr": int(model.node_attr)}
    for k, v in own.items():
        if k in args and int(args[k]) != v:
            raise ValueError(f"save_classifier: {k} = {args[k]!r} contradicts the model's {v}")
    os.makedirs(model_dir, exist_ok=True)
    with open(os.path.join(model_dir, "args.pickle"), "wb") as f:
        pickle.dump(argparse.Namespace(**{**args, **own}), f)
    load_classifier_args(os.path.join(model_dir, "args.pickle"))          # a value the loader would refuse is refused now
    torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, os.path.join(model_dir, "best_checkpoint.npy"))
