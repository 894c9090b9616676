"""Shared by the fused-message-layer tests (test_mp_train_cabi_gpu.py, test_mp_train_gpu.py): the layer's weights in the order of
include/gcdm_mp_train.h, graphs (fully connected and hand-built asymmetric ones) with their CSR built in plain torch on the CPU, inputs, the
oracle as fp64 / fp32 reference with autograd, and the measured bar.

The bar: the oracle run in float32 on the CPU differs from its float64 run by gap = max|ref32 - ref64| per tensor (and per row).  A kernel in
"exact fp32" must sit within a small multiple M of that gap: max|got - ref64| <= M * gap + 8 * U * max|ref64|.  Nothing in the bar comes from
the code under test."""
import math
from types import SimpleNamespace

import torch

import synth
from oracle import gcdm_oracle as O

U = 2.0 ** -24                     # unit roundoff of fp32
M_DEFAULT = 4                      # the margin the project uses against fp32-vs-fp64 gaps (README, test_training_step_*)
M_MAX = 16                         # no documented exception may go beyond this
# The documented exceptions: tensor -> M.  Measured ratios and reasons: the table in tests/test_mp_train_cabi_gpu.py's docstring (only there).
MARGINS = {"dh": 16, "scalar_message_attention.0.bias": 16,
           **{f"message_fusion.{k}.{n}.bias": 16 for k in range(4) for n in ("scalar_out", "vector_out_scale")}}
PRE = "interaction_layers.0.interaction."
ROWWISE = ("agg_s", "agg_v", "dh", "dchi", "de", "dxi")          # rows = nodes for the first four, edges for de / dxi


def weight_keys():
    """The 30 tensors of the layer in the order of include/gcdm_mp_train.h."""
    keys = []
    for k in range(4):
        keys += [f"message_fusion.{k}.{n}" for n in ("vector_down.weight", "vector_down_frames.weight", "scalar_out.weight", "scalar_out.bias",
                                                     "vector_up.weight", "vector_out_scale.weight", "vector_out_scale.bias")]
    return keys + ["scalar_message_attention.0.weight", "scalar_message_attention.0.bias"]


TENSORS = ROWWISE + tuple(weight_keys())                          # the 36 tensors every comparison covers


def layer_weights(case, seed=3):
    """name -> fp32 CPU tensor: layer 0's message weights of the network test_mp_train_gpu._layer() builds (synth.make_weights draws per key)."""
    d = synth.DATASET_DIMS[case]
    W = synth.make_weights(synth.dynamics_shapes(d["S"], d["V"], d["Se"], d["Ve"], d["L"], synth.dims_h_in(d)), seed=seed, scale_2d=0.5)
    P = {k[len(PRE):]: v for k, v in W.items() if k.startswith(PRE)}
    assert set(P) == set(weight_keys())
    return P, d


# ---- graphs ----------------------------------------------------------------------------------------------------------------------------
def csr(index, N):
    """CSR pointers [N + 1] (int32) of a sorted index list: bincount + cumsum."""
    ptr = torch.zeros(N + 1, dtype=torch.int64)
    if index.numel():
        ptr[1:] = torch.cumsum(torch.bincount(index, minlength=N), 0)
    return ptr.to(torch.int32)


def make_graph(name, N, row, col):
    """A row-sorted edge list with rowptr, colperm (stable argsort of col) and colptr, all built on the CPU in plain torch."""
    row, col = row.to(torch.int64).contiguous(), col.to(torch.int64).contiguous()
    assert row.numel() == 0 or bool((row[1:] >= row[:-1]).all()), "edge list must be sorted by row"
    srt = torch.sort(col, stable=True)
    return SimpleNamespace(name=name, N=int(N), E=int(row.numel()), row=row, col=col, rowptr=csr(row, N), colperm=srt.indices.contiguous(),
                           colptr=csr(srt.values, N))


def fc_graph(sizes):
    bi = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.int64))
    row, col = O.fully_connected_edges(bi)
    return make_graph(f"fc{list(sizes) if len(sizes) < 8 else [sizes[0], 'x', len(sizes)]}", int(bi.numel()), row, col)


def star_out(N=70):
    """node 0 -> every other node: rowptr constant after row 0, every column segment of length <= 1."""
    return make_graph("star_out", N, torch.zeros(N - 1, dtype=torch.int64), torch.arange(1, N))


def star_in(N=70):
    """every other node -> node 0: row segments of length 1, one column segment of length N - 1."""
    return make_graph("star_in", N, torch.arange(1, N), torch.zeros(N - 1, dtype=torch.int64))


def chain(N=130):
    return make_graph("chain", N, torch.arange(0, N - 1), torch.arange(1, N))


def random_sparse(N=300, E=2000, seed=11):
    """Independent seeded draws, sorted by row, duplicates kept, self-loops allowed.  Sources avoid 15 nodes and targets another 15, and nobody
    touches the first or the last node.  tests/test_mp_train_cpu.py asserts the properties (no GPU needed)."""
    g = torch.Generator().manual_seed(seed)
    inner = torch.arange(1, N - 1)
    shuffled = inner[torch.randperm(inner.numel(), generator=g)]
    no_out, no_in = shuffled[:15], shuffled[15:30]
    src = inner[~torch.isin(inner, no_out)]
    dst = inner[~torch.isin(inner, no_in)]
    row = src[torch.randint(0, src.numel(), (E,), generator=g)]
    col = dst[torch.randint(0, dst.numel(), (E,), generator=g)]
    order = torch.sort(row, stable=True).indices
    return make_graph("random_sparse", N, row[order], col[order])


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def make_inputs(d, graph, seed=5):
    """h, chi, e, xi, frames (fp32, CPU) for a graph.  Frames: O.localize(x, row, col); on a hand-built graph a self-loop gets a seeded random
    3 x 3 instead of localize's zero frame (the layer takes frames as data).  The fully connected graphs keep localize's frames throughout,
    as test_mp_train_gpu._inputs() does."""
    g = torch.Generator().manual_seed(seed)
    N, E = graph.N, graph.E
    x = torch.randn(N, 3, generator=g)
    frames = O.localize(x, graph.row, graph.col)
    h = torch.randn(N, d["S"], generator=g)
    chi = torch.randn(N, d["V"], 3, generator=g)
    e = torch.rand(E, d["Se"], generator=g) * 2
    xi = torch.randn(E, d["Ve"], 3, generator=g)
    if not graph.name.startswith("fc"):
        loops = graph.row == graph.col
        frames[loops] = torch.randn(E, 3, 3, generator=g)[loops]
    return SimpleNamespace(h=h, chi=chi, e=e, xi=xi, frames=frames)


def make_r(N, seed=7):
    """The cotangent of the aggregate, [N, 352] = [r_s (256) | r_v (32 x 3)]."""
    g = torch.Generator().manual_seed(seed)
    return torch.cat((torch.randn(N, 256, generator=g), torch.randn(N, 32, 3, generator=g).reshape(N, 96)), dim=1)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def reference(P, d, inp, graph, r, dtype, edge_mask=None):
    """O.message_passing on `dtype` leaves with autograd of sum(agg . r); a masked edge has its frame multiplied by 0 before the call.
    -> name -> float64 CPU tensor for the 36 tensors."""
    Pd = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in P.items()}
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (inp.h, inp.chi, inp.e, inp.xi)]
    frames = inp.frames.to(dtype)
    if edge_mask is not None:
        frames = frames * edge_mask.to(dtype).reshape(-1, 1, 1)
    o_s, o_v = O.message_passing(Pd, "", leaves[0], leaves[1], leaves[2], leaves[3], graph.row, graph.col, frames, O.OracleConfig(num_layers=d["L"]))
    rr = r.to(dtype)
    ((o_s * rr[:, :256]).sum() + (o_v * rr[:, 256:].reshape(-1, 32, 3)).sum()).backward()
    out = {"agg_s": o_s.detach(), "agg_v": o_v.detach()}
    for name, t in zip(("dh", "dchi", "de", "dxi"), leaves):
        out[name] = t.grad if t.grad is not None else torch.zeros_like(t)
    for k, v in Pd.items():
        out[k] = v.grad if v.grad is not None else torch.zeros_like(v)
    return {k: v.detach().double() for k, v in out.items()}


def references(P, d, inp, graph, r, edge_mask=None):
    """(ref64, ref32), both finite."""
    r64 = reference(P, d, inp, graph, r, torch.float64, edge_mask)
    # ref32 sets the bar, and torch's fp32 sums on the CPU split their work by thread count: one thread, so that the gap does not move with the
    # number of cores of the host that runs the test
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        r32 = reference(P, d, inp, graph, r, torch.float32, edge_mask)
    finally:
        torch.set_num_threads(threads)
    for ref in (r64, r32):
        for k, v in ref.items():
            assert bool(torch.isfinite(v).all()), f"reference {k} is not finite"
    return r64, r32


# ---- the bar ---------------------------------------------------------------------------------------------------------------------------
def _needed(err, gap, floor):
    """The M an entry would need: (err - floor) / gap, 0 where err <= floor, inf where the gap is 0 and the floor is exceeded or err is NaN."""
    over = (err - floor).clamp(min=0)
    need = torch.where(over > 0, over / gap, torch.zeros_like(over))
    need = torch.where(torch.isnan(err), torch.full_like(need, math.inf), need)
    return float(need.max()) if need.numel() else 0.0


def compare(got, ref64, ref32, margins=None, what="", names=None):
    """got: name -> tensor for the 36 tensors.  -> (failures, ratios): failures lists every tensor (and row) outside
    M * gap + 8 U max|ref64|; ratios[name] = (the M the whole tensor needs, the M its worst row needs).  `names` restricts the comparison (a block
    of a tensor passed under the tensor's name is then held to the bar of the block alone)."""
    margins = MARGINS if margins is None else margins
    assert all(M_DEFAULT <= m <= M_MAX for m in margins.values())
    failures, ratios = [], {}
    for name in (names or TENSORS):
        want, g = ref64[name], got[name].detach().double().cpu().reshape(ref64[name].shape)
        M = margins.get(name, M_DEFAULT)
        err, gap = (g - want).abs(), (ref32[name] - want).abs()
        floor = 8 * U * float(want.abs().max()) if want.numel() else 0.0
        if not want.numel():
            ratios[name] = (0.0, 0.0)
            continue
        err = err.nan_to_num(nan=math.inf)                      # an entry the kernel left unwritten (NaN) fails any bar
        worst = float(err.max())
        need = _needed(err.max(), gap.max(), floor)
        need_row = 0.0
        if name in ROWWISE:
            e2, g2 = err.reshape(err.shape[0], -1), gap.reshape(gap.shape[0], -1)
            need_row = _needed(e2.max(dim=1).values, g2.max(dim=1).values, floor)
        ratios[name] = (need, need_row)
        if not need <= M:
            failures.append(f"{what}{name}: max|got - ref64| = {worst:.3e} needs M = {need:.3g} > {M} (gap {float(gap.max()):.3e}, floor {floor:.3e})")
        if not need_row <= M:
            failures.append(f"{what}{name}: a row needs M = {need_row:.3g} > {M} against its own fp32 gap (floor {floor:.3e})")
    return failures, ratios


def worst_ratio(ratios):
    name = max(ratios, key=lambda k: max(ratios[k]))
    return name, max(ratios[name])
