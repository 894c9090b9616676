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
            return_layers: bool = False, probe: Optional[dict] = None):
    """pred [B] (and the list [h after the embedding, h after layer 1, ...]) on the ragged layout.  A `probe` dict receives what the
    conditions on the inputs are stated in: per layer the pre-activations of edge_mlp.0 / edge_mlp.2 ("pre0", "pre2") and the attention gate
    ("gate"), and "pred_scale" [B] = sum_n |w_n a_n| + |b|, the magnitudes the final dot product adds up."""
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
        pre0 = _lin(W, p + "edge_mlp.0", torch.cat([h[row], h[col], radial], 1))
        pre2 = _lin(W, p + "edge_mlp.2", _silu(pre0))
        m = _silu(pre2)
        if att:
            gate = torch.sigmoid(_lin(W, p + "att_mlp.0", m))
            m = m * gate
        if probe is not None:
            probe.setdefault("pre0", []).append(pre0)
            probe.setdefault("pre2", []).append(pre2)
            if att:
                probe.setdefault("gate", []).append(gate)
        agg = torch.zeros_like(h).index_add_(0, row, m)
        inp = torch.cat([h, agg, h0], 1) if attr else torch.cat([h, agg], 1)
        h = h + _lin(W, p + "node_mlp.2", _silu(_lin(W, p + "node_mlp.0", inp)))
        layers.append(h)
    y = _lin(W, "node_dec.2", _silu(_lin(W, "node_dec.0", h)))
    bi = torch.repeat_interleave(torch.arange(len(num_nodes)), torch.as_tensor(list(num_nodes), dtype=torch.long))
    g = torch.zeros((len(num_nodes), y.shape[1]), dtype=dtype).index_add_(0, bi, y)
    a = _silu(_lin(W, "graph_dec.0", g))
    pred = _lin(W, "graph_dec.2", a).squeeze(1)
    if probe is not None:
        probe["pred_scale"] = (a * W["graph_dec.2.weight"]).abs().sum(1) + W["graph_dec.2.bias"].abs()
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


# ---- the C ABI called directly, per molecule and per row (tests/test_classifier_cabi_gpu.py) ------------------------------------------------
U = 2.0 ** -24                     # unit roundoff of fp32
M_DEFAULT = 4                      # the margin the project uses against fp32-vs-fp64 gaps (mp_train_ref.M_DEFAULT)
M_MAX = 16                         # no documented exception may go beyond this
# The floor covers a molecule or row whose own fp32 draw happens to land on the fp64 value (gap ~ 0; a prediction is ONE number).  A correctly
# rounded fp32 result is within U of its magnitude, and each of the last additions of a sum rounds by up to U of a partial sum that the sum of the
# |terms| bounds: 2 ulp of that sum admits the final roundings of the kernel and of the restatement and no more.  On the CPU the restatement's
# own gap is 0.05 (median) to 0.5 (worst) of 8 ulp of the prediction's scale and 0.2 to 1.1 of 8 ulp of a row's largest |h|, so the 8 ulp of
# mp_train_ref.compare would be most of the bar here; 2 ulp leaves the bar to the gap.
FLOOR_ULPS = 2
HOT_SEED = 23
# The documented exceptions: regime -> tensor ("pred" / "h") -> M.  Measured ratios and reasons: the table in tests/test_classifier_cabi_gpu.py's
# docstring (only there).
MARGINS: Dict[str, Dict[str, int]] = {"init": {}, "hot": {"h": 16}}
GUARD = 64                         # NaN guard words either side of every device buffer the C ABI writes

INSTANTIATION_SIZES = [1, 2, 3, 4, 5, 8, 9, 16, 31, 32, 0, 7]
# what a batch of more than 1 024 molecules opens with: both LDS halves full, an empty molecule first / second / both, the smallest pair, a
# one-atom molecule before a full one, and the two sides of the quad padding's step (P = 4 -> 8)
GROUP_PAIRS = [(32, 32), (0, 32), (32, 0), (0, 0), (1, 1), (1, 32), (4, 5)]


def group_sizes(count: int = 1025, seed: int = 17) -> List[int]:
    """GROUP_PAIRS, then seeded sizes 0 .. 32; an odd count leaves the last workgroup of a grouped launch one molecule."""
    head = [n for pair in GROUP_PAIRS for n in pair]
    rng = np.random.Generator(np.random.PCG64(seed))
    return head + [int(v) for v in rng.integers(0, 33, size=count - len(head))]


def make_regime(name: str, in_node_nf: int, hidden_nf: int, n_layers: int, attention, node_attr, sizes: Sequence[int], seed: Optional[int] = None,
                dense_h0: Optional[bool] = None):
    """(W, x, h0) of an input regime.  "init": synth.make_weights as drawn, x ~ 1.5 N(0, 1), one-hot h0 (randn with dense_h0): the network
    stays near-linear (seed 11, the weights of the golden fixtures).  "hot": 2-D weights x 2, attention weights x 16 on top of that,
    x ~ 2.5 N(0, 1), dense randn h0: gates spread over (0, 1), SiLU saturated on both sides.  The conditions on "hot" are asserted by
    tests/test_classifier_cpu.py for every configuration the GPU tests use; seed 23 is the first of 20 .. 31 under which they hold at every
    hidden_nf (a gate that saturates to one side in some layer fails them), chosen on the CPU from the fp64 restatement alone."""
    import synth
    seed = (HOT_SEED if name == "hot" else 11) if seed is None else seed
    shapes = state_dict_shapes(in_node_nf, hidden_nf, n_layers, bool(attention), bool(node_attr))
    if name == "init":
        W, spread, dense = synth.make_weights(shapes, seed=seed), 1.5, bool(dense_h0)
    elif name == "hot":
        W, spread, dense = synth.make_weights(shapes, seed=seed, scale_2d=2.0), 2.5, True if dense_h0 is None else bool(dense_h0)
        for k in W:
            if "att_mlp.0.weight" in k:
                W[k] = W[k] * 16.0
    else:
        raise ValueError(name)
    x, h0 = make_batch(sizes, in_node_nf, seed=seed + 1, spread=spread)
    if dense:
        h0 = torch.randn(h0.shape, generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float32)
    return W, x, h0


def _forward_chunked(W, x, h0, sizes, dtype, chunk):
    """forward over `chunk` molecules at a time (a molecule does not depend on its batch): bounds the [E, 2H + 1] intermediates."""
    preds, layers, scales, o, L = [], None, [], 0, n_layers_of(W)
    layers = [[] for _ in range(L + 1)]
    for b in range(0, len(sizes), chunk):
        sz = list(sizes[b:b + chunk])
        n = int(sum(sz))
        probe = {}
        p, ls = forward(W, x[o:o + n], h0[o:o + n], sz, dtype=dtype, return_layers=True, probe=probe)
        preds.append(p.double())
        scales.append(probe["pred_scale"].double())
        for k in range(L + 1):
            layers[k].append(ls[k].double())
        o += n
    H = W["embedding.weight"].shape[0]
    cat = lambda ts, shape: torch.cat(ts) if ts else torch.zeros(shape, dtype=torch.float64)
    return cat(preds, (0,)), [cat(l, (0, H)) for l in layers], cat(scales, (0,))


def references(W, x, h0, sizes, chunk: int = 128):
    """The fp64 and the fp32 restatement with every layer, as float64 CPU tensors: .pred64 / .pred32 [B], .layers64 / .layers32 (L + 1 of
    [N, H]), .pred_scale [B] (fp64 run).  Both finite."""
    from types import SimpleNamespace
    p64, l64, scale = _forward_chunked(W, x, h0, sizes, torch.float64, chunk)
    # the fp32 run sets the bar, and torch's fp32 sums on the CPU split their work by thread count: one thread, so that the gap does not move
    # with the number of cores of the host that runs the test (as mp_train_ref.references)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        p32, l32, _ = _forward_chunked(W, x, h0, sizes, torch.float32, chunk)
    finally:
        torch.set_num_threads(threads)
    for t in [p64, p32] + l64 + l32:
        assert bool(torch.isfinite(t).all()), "a reference is not finite"
    return SimpleNamespace(pred64=p64, pred32=p32, layers64=l64, layers32=l32, pred_scale=scale, sizes=list(sizes))


def _needed(err, gap, floor):
    """The M every entry would need: (err - floor) / gap, 0 where err <= floor, inf where the gap is 0 and the floor is exceeded or err is NaN."""
    over = (err - floor).clamp(min=0)
    need = torch.where(over > 0, over / gap, torch.zeros_like(over))
    return torch.where(torch.isnan(err) | torch.isnan(need), torch.full_like(need, float("inf")), need)


def compare(ref, pred=None, layers=None, margins: Optional[Dict[str, int]] = None, what: str = "", molecules=None, rows=None):
    """err <= M * gap + floor, per molecule for `pred` [B] and per atom row for every h in `layers` (layer index -> [N, H]).  gap: that
    molecule's |pred32 - pred64|, that row's max|h32 - h64|.  floor: FLOOR_ULPS * U times the magnitudes that were summed, from the fp64 run
    alone: a row's largest |h64|; for pred sum_n |w_n a_n| + |b| (the terms of the final dot product cancel, so |pred| is not the scale).
    `molecules` / `rows` (index tensors) restrict the comparison.  -> (failures, ratios): ratios["pred"] / ratios["h<k>"] = the worst M needed."""
    margins = {} if margins is None else margins
    assert all(M_DEFAULT <= m <= M_MAX for m in margins.values()) and set(margins) <= {"pred", "h"}
    failures, ratios = [], {}

    def judge(name, key, need, err, gap, floor, unit):
        M = margins.get(key, M_DEFAULT)
        if not need.numel():
            ratios[name] = 0.0
            return
        k = int(need.argmax())
        ratios[name] = float(need[k])
        if not ratios[name] <= M:
            bad = int((need > M).sum())
            failures.append(f"{what}{name}: {unit} {k} needs M = {ratios[name]:.3g} > {M} (err {float(err[k]):.3e}, its gap {float(gap[k]):.3e}, "
                            f"floor {float(floor[k]):.3e}); {bad} of {need.numel()} {unit}s over the bar")

    if pred is not None:
        sel = torch.arange(len(ref.sizes)) if molecules is None else torch.as_tensor(molecules, dtype=torch.long)
        got = pred.detach().double().cpu().reshape(-1)
        assert got.numel() == len(ref.sizes)
        err, gap = (got - ref.pred64).abs()[sel], (ref.pred32 - ref.pred64).abs()[sel]
        floor = FLOOR_ULPS * U * ref.pred_scale[sel]
        judge("pred", "pred", _needed(err, gap, floor), err, gap, floor, "molecule")
    for k, h in sorted((layers or {}).items()):
        want, w32 = ref.layers64[k], ref.layers32[k]
        got = h.detach().double().cpu().reshape(want.shape)
        sel = torch.arange(want.shape[0]) if rows is None else torch.as_tensor(rows, dtype=torch.long)
        if not sel.numel():
            ratios[f"h{k}"] = 0.0
            continue
        err, gap = (got - want).abs()[sel].max(1).values, (w32 - want).abs()[sel].max(1).values
        err = torch.where(torch.isnan((got - want)[sel]).any(1), torch.full_like(err, float("nan")), err)
        floor = FLOOR_ULPS * U * want.abs()[sel].max(1).values
        judge(f"h{k}", "h", _needed(err, gap, floor), err, gap, floor, "row")
    return failures, ratios


def ordered_tensors(W, n_layers: int, attention) -> List[Optional[torch.Tensor]]:
    """The state dict in the order gcdm_classifier_pack takes it (include/gcdm_classifier.h); None for the attention slots without attention."""
    out = [W["embedding.weight"], W["embedding.bias"]]
    for k in range(n_layers):
        p = f"gcl_{k}."
        out += [W[p + f"{m}.{i}.{n}"] for m in ("edge_mlp", "node_mlp") for i in (0, 2) for n in ("weight", "bias")]
        out += [W[p + "att_mlp.0.weight"], W[p + "att_mlp.0.bias"]] if attention else [None, None]
    return out + [W[f"{m}.{i}.{n}"] for m in ("node_dec", "graph_dec") for i in (0, 2) for n in ("weight", "bias")]


class Guarded:
    """`n` floats at their advertised size inside a larger device buffer, everything NaN: an entry nobody wrote shows, a read of one poisons
    the result, and a write into the GUARD words either side clears a NaN there."""

    def __init__(self, n: int, device="cuda"):
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=device)
        self.inner = self.buf[GUARD:GUARD + self.n]

    @property
    def ptr(self):
        import ctypes
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def guards_intact(self) -> bool:
        return bool(self.buf[:GUARD].isnan().all()) and bool(self.buf[GUARD + self.n:].isnan().all())

    def bits(self):
        return self.inner.view(torch.int32).clone()


def _ops_lib():
    import importlib
    return importlib.import_module("bio-diffusion_amd")._native.load_ops()


def _stream_ptr(stream=None):
    import ctypes
    return ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


def cabi_pack(W, cfg, stream=None, into: Optional[Guarded] = None):
    """gcdm_classifier_pack on a NaN-filled, guarded buffer of exactly the advertised size.  cfg = (F, H, L, attention, node_attr).
    -> (status, Guarded, the device tensors the table points to)."""
    import ctypes
    F, H, L, att, attr = (int(v) for v in cfg)
    lib = _ops_lib()
    nbytes = int(lib.gcdm_classifier_workspace_bytes(1, 0, F, H, L))
    assert nbytes > 0 and nbytes % 4 == 0
    packed = into if into is not None else Guarded(nbytes // 4)
    assert packed.n == nbytes // 4
    ts = [None if t is None else t.to(torch.float32).cuda().contiguous() for t in ordered_tensors(W, L, att)]
    table = (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    st = lib.gcdm_classifier_pack(table, len(ts), F, H, L, att, attr, packed.ptr, _stream_ptr(stream))
    return st, packed, ts


def cabi_forward(packed: Guarded, cfg, x, h0, offsets, debug_layer: int = -1, num_nodes: Optional[int] = None, stream=None,
                 null_inputs: bool = False):
    """gcdm_classifier_forward called directly.  pred [B], the workspace and h_debug [N, H] sit at their advertised sizes, NaN-filled, between
    NaN guard words.  `offsets`: the B + 1 node offsets as given (they may be illegal on purpose).  -> a namespace: status, pred / hdbg /
    workspace (Guarded; hdbg None without debug_layer), guards (name -> intact), inputs (the device tensors and their bytes before the call),
    unchanged() -> whether x, h0, node_offsets and packed still hold the bytes they held before the call."""
    from types import SimpleNamespace
    import ctypes
    F, H, L, att, _ = (int(v) for v in cfg)
    lib = _ops_lib()
    off = torch.as_tensor(offsets, dtype=torch.int32)
    B = off.numel() - 1
    N = int(x.shape[0]) if num_nodes is None else int(num_nodes)
    wsn = int(lib.gcdm_classifier_workspace_bytes(0, N, F, H, L))
    assert wsn >= N * H * 4 and wsn % 256 == 0
    pred, ws = Guarded(B), Guarded(wsn // 4)
    hdbg = Guarded(N * H) if debug_layer >= 0 else None
    xd, hd, od = x.to(torch.float32).cuda().contiguous(), h0.to(torch.float32).cuda().contiguous(), off.cuda()
    before = [t.view(torch.uint8).clone() if t.numel() else t.clone() for t in (xd, hd, od.view(torch.uint8), packed.buf.view(torch.uint8))]
    null = ctypes.c_void_p(None)
    st = lib.gcdm_classifier_forward(null if null_inputs else ctypes.c_void_p(xd.data_ptr()), null if null_inputs else ctypes.c_void_p(hd.data_ptr()),
                                     ctypes.c_void_p(od.data_ptr()), packed.ptr, ws.ptr, pred.ptr, hdbg.ptr if hdbg is not None else null,
                                     int(debug_layer), N, B, F, H, L, att, _stream_ptr(stream))
    (stream or torch.cuda.current_stream()).synchronize()

    def unchanged():
        now = [xd.view(torch.uint8) if xd.numel() else xd, hd.view(torch.uint8) if hd.numel() else hd, od.view(torch.uint8), packed.buf.view(torch.uint8)]
        return all(torch.equal(a, b) for a, b in zip(before, now))

    guards = {"pred": pred.guards_intact(), "workspace": ws.guards_intact(), "packed": packed.guards_intact()}
    if hdbg is not None:
        guards["h_debug"] = hdbg.guards_intact()
    return SimpleNamespace(status=st, pred=pred, workspace=ws, hdbg=hdbg, guards=guards, inputs=(xd, hd, od), unchanged=unchanged, N=N, B=B, H=H)


def offsets_of(sizes: Sequence[int]) -> List[int]:
    out = [0]
    for n in sizes:
        out.append(out[-1] + int(n))
    return out
