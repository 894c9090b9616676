"""The EGNN property classifier restated on the CPU (fp64 by default), for the tests of bio-diffusion_amd/classifier.py.

Two forms of the same network: `forward` on the ragged flat layout the package uses (`num_nodes`, atoms of a molecule contiguous), and
`forward_padded` on the reference's dense layout ([B, n_max] rows, a node mask, an edge mask over all n_max^2 pairs), which exists to show
that the two give the same numbers.  Weights: a dict with the reference's state-dict names.  Test support, not an oracle of the sampler."""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

QM9_SIZES = {22: 3393, 17: 13025, 23: 4848, 21: 9970, 19: 13832, 20: 9482, 16: 10644, 13: 3060, 15: 7796, 25: 1506, 18: 13364, 12: 1689,
             11: 807, 24: 539, 14: 5136, 26: 48, 7: 16, 10: 362, 8: 49, 9: 124, 27: 266, 4: 4, 29: 25, 6: 9, 5: 5, 3: 1}


def state_dict_shapes(in_node_nf: int, hidden_nf: int, n_layers: int, attention: bool, node_attr: bool) -> Dict[str, Tuple[int, ...]]:
    """Names and shapes of the classifier's state dict, in registration order."""
    F, H = in_node_nf, hidden_nf
    sh = {"embedding.weight": (H, F), "embedding.bias": (H,)}
    for k in range(n_layers):
        p = f"gcl_{k}."
        sh[p + "edge_mlp.0.weight"] = (H, 2 * H + 1)
        sh[p + "edge_mlp.0.bias"] = (H,)
        sh[p + "edge_mlp.2.weight"] = (H, H)
        sh[p + "edge_mlp.2.bias"] = (H,)
        sh[p + "node_mlp.0.weight"] = (H, 2 * H + (F if node_attr else 0))
        sh[p + "node_mlp.0.bias"] = (H,)
        sh[p + "node_mlp.2.weight"] = (H, H)
        sh[p + "node_mlp.2.bias"] = (H,)
        if attention:
            sh[p + "att_mlp.0.weight"] = (1, H)
            sh[p + "att_mlp.0.bias"] = (1,)
    for name in ("node_dec", "graph_dec"):
        sh[name + ".0.weight"] = (H, H)
        sh[name + ".0.bias"] = (H,)
        sh[name + ".2.weight"] = (H if name == "node_dec" else 1, H)
        sh[name + ".2.bias"] = (H if name == "node_dec" else 1,)
    return sh


def make_batch(sizes: Sequence[int], in_node_nf: int, seed: int, spread: float = 1.5):
    """x ~ spread N(0, 1) [N, 3] and one-hot atom types [N, F], fp32, for molecules of the given sizes."""
    g = torch.Generator().manual_seed(seed)
    N = int(sum(sizes))
    x = spread * torch.randn((N, 3), generator=g, dtype=torch.float32)
    t = torch.randint(0, in_node_nf, (N,), generator=g)
    return x, torch.nn.functional.one_hot(t, in_node_nf).to(torch.float32)


def qm9_sizes(count: int, seed: int) -> List[int]:
    keys = sorted(QM9_SIZES)
    p = np.array([QM9_SIZES[k] for k in keys], dtype=np.float64)
    rng = np.random.Generator(np.random.PCG64(seed))
    return [int(v) for v in rng.choice(keys, size=count, p=p / p.sum())]


def _lin(W, name, v):
    return v @ W[name + ".weight"].T + W[name + ".bias"]


def _silu(v):
    return v * torch.sigmoid(v)


def _cast(W, dtype):
    return {k: v.to(dtype) for k, v in W.items()}


def n_layers_of(W) -> int:
    return 1 + max(int(k.split(".")[0][4:]) for k in W if k.startswith("gcl_"))


def forward(W: Dict[str, torch.Tensor], x: torch.Tensor, h0: torch.Tensor, num_nodes: Sequence[int], dtype=torch.float64,
            return_layers: bool = False):
    """pred [B] (and the list [h after the embedding, h after layer 1, ...]) on the ragged layout."""
    W, x, h0 = _cast(W, dtype), x.to(dtype), h0.to(dtype)
    L = n_layers_of(W)
    att, attr = "gcl_0.att_mlp.0.weight" in W, W["gcl_0.node_mlp.0.weight"].shape[1] > 2 * W["embedding.weight"].shape[0]
    rows, cols, o = [], [], 0
    for n in num_nodes:                                       # all ordered pairs i != j of one molecule
        i, j = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
        keep = i != j
        rows.append(i[keep] + o)
        cols.append(j[keep] + o)
        o += n
    row = torch.cat(rows) if rows else torch.zeros(0, dtype=torch.long)
    col = torch.cat(cols) if cols else torch.zeros(0, dtype=torch.long)
    radial = ((x[row] - x[col]) ** 2).sum(1, keepdim=True)
    h = _lin(W, "embedding", h0)
    layers = [h]
    for k in range(L):
        p = f"gcl_{k}."
        m = _silu(_lin(W, p + "edge_mlp.0", torch.cat([h[row], h[col], radial], 1)))
        m = _silu(_lin(W, p + "edge_mlp.2", m))
        if att:
            m = m * torch.sigmoid(_lin(W, p + "att_mlp.0", m))
        agg = torch.zeros_like(h).index_add_(0, row, m)
        inp = torch.cat([h, agg, h0], 1) if attr else torch.cat([h, agg], 1)
        h = h + _lin(W, p + "node_mlp.2", _silu(_lin(W, p + "node_mlp.0", inp)))
        layers.append(h)
    y = _lin(W, "node_dec.2", _silu(_lin(W, "node_dec.0", h)))
    bi = torch.repeat_interleave(torch.arange(len(num_nodes)), torch.as_tensor(list(num_nodes), dtype=torch.long))
    g = torch.zeros((len(num_nodes), y.shape[1]), dtype=dtype).index_add_(0, bi, y)
    pred = _lin(W, "graph_dec.2", _silu(_lin(W, "graph_dec.0", g))).squeeze(1)
    return (pred, layers) if return_layers else pred


def to_padded(x: torch.Tensor, h0: torch.Tensor, num_nodes: Sequence[int], n_max: Optional[int] = None):
    """The reference's dense batch: x [B n, 3], h0 [B n, F], node_mask [B n, 1], edge_mask [B n n, 1], n."""
    B, n = len(num_nodes), int(n_max or max(num_nodes))
    xp, hp = torch.zeros((B, n, 3), dtype=x.dtype), torch.zeros((B, n, h0.shape[1]), dtype=h0.dtype)
    mask = torch.zeros((B, n), dtype=x.dtype)
    o = 0
    for b, k in enumerate(num_nodes):
        xp[b, :k], hp[b, :k], mask[b, :k] = x[o:o + k], h0[o:o + k], 1
        o += k
    em = mask[:, :, None] * mask[:, None, :] * (1 - torch.eye(n, dtype=x.dtype))[None]
    return xp.reshape(B * n, 3), hp.reshape(B * n, -1), mask.reshape(B * n, 1), em.reshape(B * n * n, 1), n


def forward_padded(W, x, h0, node_mask, edge_mask, n_nodes: int, dtype=torch.float64):
    """The same network over every pair of padded rows, masked: what the reference's dense call computes."""
    W, x, h0, node_mask, edge_mask = _cast(W, dtype), x.to(dtype), h0.to(dtype), node_mask.to(dtype), edge_mask.to(dtype)
    L = n_layers_of(W)
    att, attr = "gcl_0.att_mlp.0.weight" in W, W["gcl_0.node_mlp.0.weight"].shape[1] > 2 * W["embedding.weight"].shape[0]
    B, n = x.shape[0] // n_nodes, n_nodes
    base = (torch.arange(B) * n)[:, None, None]
    row = (base + torch.arange(n)[None, :, None]).expand(B, n, n).reshape(-1)
    col = (base + torch.arange(n)[None, None, :]).expand(B, n, n).reshape(-1)
    radial = ((x[row] - x[col]) ** 2).sum(1, keepdim=True)
    h = _lin(W, "embedding", h0)
    for k in range(L):
        p = f"gcl_{k}."
        m = _silu(_lin(W, p + "edge_mlp.0", torch.cat([h[row], h[col], radial], 1)))
        m = _silu(_lin(W, p + "edge_mlp.2", m))
        if att:
            m = m * torch.sigmoid(_lin(W, p + "att_mlp.0", m))
        agg = torch.zeros_like(h).index_add_(0, row, m * edge_mask)
        inp = torch.cat([h, agg, h0], 1) if attr else torch.cat([h, agg], 1)
        h = h + _lin(W, p + "node_mlp.2", _silu(_lin(W, p + "node_mlp.0", inp)))
    y = _lin(W, "node_dec.2", _silu(_lin(W, "node_dec.0", h))) * node_mask
    g = y.view(B, n, -1).sum(1)
    return _lin(W, "graph_dec.2", _silu(_lin(W, "graph_dec.0", g))).squeeze(1)
