"""Writes tests/golden/egnn_dynamics_<name>.npz and tests/golden/egnn_dynamics_state_dict.json: the unmodified reference EGNNDynamics
(src/models/components/egnn.py, imported under ref_harness.install_stubs() plus the further stubs made here) on four small configurations
(egnn_dynamics_ref.GOLDEN_CONFIGS: plain, time + context, self-conditioned, masked nodes), evaluated in float64.

The further stubs, written from PyG's documented behaviour and NOT pinned to an installed PyG (there is none offline):
  * torch_geometric.nn.MessagePassing: what EGNN_Sparse.propagate calls -- ``__check_input__``, ``__collect__`` (x_i = x[edge_index[1]],
    x_j = x[edge_index[0]]: the default flow source_to_target), ``__user_args__``, ``inspector.distribute``, a sum ``aggregate`` at
    edge_index[1] and an identity ``update``;
  * torch_geometric.nn.norm.LayerNorm in its default graph mode: per graph mean and variance over all of its rows and features
    (count clamped to 1, times the feature width), eps 1e-5, affine weight and bias;
  * torch_geometric.utils.unbatch (imported by the reference's data module), and einops if it is absent.

The fixtures hold data only: inputs (xh, t, batch_index, mask, context, xh_self_cond), the weights drawn from a seed (the reference's own
initialisation, then biases, LayerNorm parameters and coors_norm.scale moved off their trivial initial values so that each is exercised), the
reference's output in float64, and -- in the JSON -- the state-dict names and shapes in registration order.

    python tests/golden/make_egnn_dynamics_golden.py
"""
import json
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh                      # noqa: E402
import egnn_dynamics_ref as er                # noqa: E402


class _Inspector:
    _ARGS = {"message": ("x_i", "x_j", "edge_attr"), "aggregate": ("index", "dim_size"), "update": ()}

    def distribute(self, name, data):
        return {k: data[k] for k in self._ARGS[name]}


class MessagePassing(nn.Module):
    """The part of torch_geometric.nn.MessagePassing that EGNN_Sparse.propagate uses (flow source_to_target, sum aggregation)."""

    def __init__(self, aggr="add", flow="source_to_target", node_dim=0, **kwargs):
        super().__init__()
        assert aggr in ("add", "sum") and flow == "source_to_target" and node_dim == 0
        self.aggr, self.flow, self.node_dim = aggr, flow, node_dim
        self.inspector = _Inspector()
        self.__user_args__ = {"x_i", "x_j", "edge_attr"}

    def __check_input__(self, edge_index, size):
        assert edge_index.dim() == 2 and edge_index.shape[0] == 2
        return [None, None]

    def __collect__(self, args, edge_index, size, kwargs):
        out = dict(kwargs)
        out["x_i"], out["x_j"] = kwargs["x"][edge_index[1]], kwargs["x"][edge_index[0]]
        out["index"], out["dim_size"] = edge_index[1], kwargs["x"].shape[0]
        return out

    def aggregate(self, inputs, index, dim_size=None):
        return torch.zeros((dim_size,) + tuple(inputs.shape[1:]), dtype=inputs.dtype).index_add_(0, index, inputs)

    def update(self, inputs):
        return inputs


class LayerNorm(nn.Module):
    """torch_geometric.nn.norm.LayerNorm(in_channels, eps=1e-5, affine=True, mode="graph")."""

    def __init__(self, in_channels, eps=1e-5, affine=True, mode="graph"):
        super().__init__()
        assert affine and mode == "graph"
        self.in_channels, self.eps = in_channels, eps
        self.weight = nn.Parameter(torch.ones(in_channels))
        self.bias = nn.Parameter(torch.zeros(in_channels))

    def forward(self, x, batch=None):
        B = int(batch.max()) + 1
        norm = torch.zeros(B, dtype=x.dtype).index_add_(0, batch, torch.ones(x.shape[0], dtype=x.dtype)).clamp_(min=1)
        norm = norm.mul_(x.size(-1)).view(-1, 1)
        mean = torch.zeros((B, x.shape[1]), dtype=x.dtype).index_add_(0, batch, x).sum(dim=-1, keepdim=True) / norm
        x = x - mean.index_select(0, batch)
        var = torch.zeros((B, x.shape[1]), dtype=x.dtype).index_add_(0, batch, x * x).sum(dim=-1, keepdim=True) / norm
        out = x / (var + self.eps).sqrt().index_select(0, batch)
        return out * self.weight + self.bias


def install_more_stubs():
    rh.install_stubs()
    tgm = sys.modules["torch_geometric"]
    tgn = sys.modules["torch_geometric.nn"]
    tgn.MessagePassing = MessagePassing
    norm = types.ModuleType("torch_geometric.nn.norm")
    norm.LayerNorm = LayerNorm
    tgn.norm = norm
    tgm.nn = tgn
    sys.modules["torch_geometric.nn.norm"] = norm
    tgu = types.ModuleType("torch_geometric.utils")
    tgu.unbatch = lambda src, batch, dim=0: src.split(torch.bincount(batch).tolist(), dim)
    sys.modules["torch_geometric.utils"] = tgu
    tgm.utils = tgu
    try:
        import einops  # noqa: F401
    except ImportError:
        eo = types.ModuleType("einops")
        eo.rearrange = lambda *a, **k: (_ for _ in ()).throw(NotImplementedError("einops.rearrange: not used by EGNNDynamics"))
        sys.modules["einops"] = eo


def import_reference_egnn():
    install_more_stubs()
    import importlib
    return importlib.import_module("src.models.components.egnn")


def build_reference(cfg, seed: int):
    """The reference's EGNNDynamics for a test configuration, its parameters moved off their trivial initial values (seeded)."""
    egnn = import_reference_egnn()
    torch.manual_seed(seed)
    net = egnn.EGNNDynamics(**{k: rh.to_dictconfig(v) for k, v in er.reference_cfgs(cfg).items()})
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k.endswith("coors_norm.scale"):
                p.fill_(0.5)
            elif k.endswith("node_norm.weight"):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return net.eval()


def main():
    assert rh.reference_available(), "reference checkout not found"
    names = {}
    for k, (name, cfg) in enumerate(er.GOLDEN_CONFIGS.items()):
        net = build_reference(cfg, seed=40 + k)
        sd = {n: v.detach().clone() for n, v in net.state_dict().items()}
        names[name] = [[n, list(v.shape)] for n, v in sd.items()]
        assert names[name] == [[n, list(s)] for n, s in er.state_dict_shapes(cfg).items()], name
        xh, t, bi, ctx, sc = er.make_inputs(cfg, er.GOLDEN_SIZES, seed=60 + k)
        mask = er.golden_mask(name, er.GOLDEN_SIZES)
        mk = torch.ones(len(bi), dtype=torch.bool) if mask is None else mask
        batch = rh.make_batch(bi, mk, None if ctx is None else ctx.double())
        batch.num_graphs = len(er.GOLDEN_SIZES)
        with torch.no_grad():
            _, out = net.double()(batch, xh.double(), t.double(), xh_self_cond=None if sc is None else sc.double())
        assert bool(torch.isfinite(out).all())
        mine = er.forward(sd, cfg, xh, t, bi, mk, ctx, sc)
        print(f"{name}: N = {len(bi)}, max|restatement - reference| = {float((mine - out).abs().max()):.3e}, max|out| = {float(out.abs().max()):.3e}")
        arrays = {"xh": xh.numpy(), "t": t.numpy(), "batch_index": bi.numpy(), "mask": mk.numpy(), "out": out.numpy()}
        if ctx is not None:
            arrays["context"] = ctx.numpy()
        if sc is not None:
            arrays["xh_self_cond"] = sc.numpy()
        for n, v in sd.items():
            arrays["W::" + n] = v.numpy()
        np.savez_compressed(os.path.join(HERE, f"egnn_dynamics_{name}.npz"), **arrays)
    with open(os.path.join(HERE, "egnn_dynamics_state_dict.json"), "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
