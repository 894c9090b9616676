"""Gradients of the EGNN property classifier restated on the CPU, for the tests of the classifier's training path.

The network is tests/classifier_ref.py's `forward`; this file differentiates it with torch autograd (fp64 the reference, fp32 on one thread the
gap that scales every bar), states the new operator -- the column-split first edge layer, include/gcdm_classifier_train.h -- and its backward in
pure Python with the mutants a test of it has to tell apart, and holds the bar `err <= M gap + floor` per tensor.  Test support only."""
import ctypes
import functools
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import torch

import classifier_ref as cr

ULPS_FLOOR = 16                    # fp32 ulps of a tensor's largest fp64 entry: a tensor whose fp32 run happens to land on the fp64 value
# Documented exceptions to cr.M_DEFAULT, at most cr.M_MAX: regime -> tensor name ("loss" for the loss) -> M.  Beside each: the largest ratio
# measured on the MI355X over the cases of tests/test_classifier_train_gpu.py, against fp64 or between the two edge inputs (also DESIGN.md
# 3.9).  Every one is a tensor whose gap is a single draw or the maximum of a few (one-element biases, the loss, the decoders' first layers on
# a one-molecule batch), or a bias gradient that the operator library sums over all edges four strided partial sums deep where torch's CPU sum
# is pairwise.
MARGINS: Dict[str, Dict[str, int]] = {
    "init": {"gcl_0.att_mlp.0.bias": 16,      # 8.93 (split against concat, F16 H96 L2 attention)
             "gcl_1.att_mlp.0.bias": 8},      # 4.66
    "hot": {"gcl_0.att_mlp.0.bias": 16,       # 10.7
            "node_dec.0.weight": 8,           # 5.13
            "node_dec.0.bias": 8,             # 5.66
            "graph_dec.0.weight": 8,          # 6.06
            "graph_dec.0.bias": 8,            # 4.85
            "loss": 8},                       # 4.44
}

NET_CONFIGS = [(5, 32, 1), (5, 32, 2), (16, 96, 2)]                     # (F, H, L)
NET_FLAGS = [(1, 1), (0, 0), (1, 0)]                                    # (attention, node_attr)
SIZE_SETS = {"inst": cr.INSTANTIATION_SIZES, "one32": [32], "one1": [1], "one0": [0]}
BIG = ("big", (16, 96, 2), (1, 1))                                      # cr.group_sizes(1025) at H = 96, once
OP_H = [32, 96]
TRAJECTORY = dict(cfg=(5, 32, 2), flags=(1, 1), steps=8, lr=0.01, regime="init")


def sizes_of(name: str) -> List[int]:
    return cr.group_sizes(1025) if name == "big" else list(SIZE_SETS[name])


def targets(count: int, seed: int = 5) -> torch.Tensor:
    """What the predictions are trained against, (label - mean) / mad of a batch: N(0, 1), fp32."""
    return torch.randn(count, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def edge_list(sizes: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(row, col) of the ordered pairs i != j of each molecule, row-major: the classifier's edge set (as classifier_ref.forward)."""
    rows, cols, o = [], [], 0
    for n in sizes:
        i, j = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
        keep = i != j
        rows.append(i[keep] + o)
        cols.append(j[keep] + o)
        o += n
    z = torch.zeros(0, dtype=torch.long)
    return (torch.cat(rows) if rows else z), (torch.cat(cols) if cols else z)


# ---- loss and parameter gradients of the restatement ----------------------------------------------------------------------------------------------
def loss_and_grads(W, x, h0, sizes, target, dtype=torch.float64, chunk: int = 128):
    """L1 loss mean_b |pred_b - target_b| of classifier_ref.forward and its gradient for every tensor of W, as float64 CPU tensors.  Molecules do
    not interact, so the loss is accumulated `chunk` molecules at a time (bounds the [E, 2H + 1] intermediates of the backward)."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in W.items()}
    B = len(sizes)
    loss, o, preds = 0.0, 0, []
    for b in range(0, B, chunk):
        sz = list(sizes[b:b + chunk])
        n = int(sum(sz))
        pred = cr.forward(leaves, x[o:o + n], h0[o:o + n], sz, dtype=dtype)
        part = (pred - target[b:b + chunk].to(dtype)).abs().sum() / B
        part.backward()
        loss += float(part.detach().double())
        preds.append(pred.detach().double())
        o += n
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double() for k, v in leaves.items()}
    return loss, grads, torch.cat(preds) if preds else torch.zeros(0, dtype=torch.float64)


def _one_thread(fn):
    """torch's fp32 sums on the CPU split their work by thread count: one thread, so the gap does not move with the host (cr.references)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn()
    finally:
        torch.set_num_threads(threads)


@functools.lru_cache(maxsize=None)
def case(regime: str, cfg: Tuple[int, int, int], flags: Tuple[int, int], sizes_name: str):
    """Everything a network test needs of one case, computed once: the inputs, the target, loss and gradients in fp64 and fp32, and
    cr.references for the predictions.  Treat as read-only."""
    (F, H, L), (att, attr) = cfg, flags
    sizes = sizes_of(sizes_name)
    W, x, h0 = cr.make_regime(regime, F, H, L, att, attr, sizes)
    t = targets(len(sizes))
    l64, g64, p64 = loss_and_grads(W, x, h0, sizes, t, torch.float64)
    l32, g32, _ = _one_thread(lambda: loss_and_grads(W, x, h0, sizes, t, torch.float32))
    assert all(bool(torch.isfinite(g).all()) for g in list(g64.values()) + list(g32.values()))
    return SimpleNamespace(W=W, x=x, h0=h0, sizes=sizes, target=t, loss64=l64, loss32=l32, grads64=g64, grads32=g32, pred64=p64,
                           cfg=(F, H, L, att, attr), regime=regime)


def trajectory(W, x, h0, sizes, target, steps: int, lr: float, dtype=torch.float64):
    """Plain SGD on the restatement, w <- w - lr dL/dw for `steps` steps on one batch: the loss before every step and after the last
    (steps + 1 numbers) and the final weights."""
    Wc = {k: v.detach().to(dtype).clone() for k, v in W.items()}
    losses = []
    for _ in range(steps):
        loss, grads, _ = loss_and_grads(Wc, x, h0, sizes, target, dtype)
        losses.append(loss)
        Wc = {k: Wc[k] - lr * grads[k].to(dtype) for k in Wc}
    losses.append(loss_and_grads(Wc, x, h0, sizes, target, dtype)[0])
    return losses, Wc


def ulp32(v: float) -> float:
    """The spacing of fp32 at |v| (0 for 0)."""
    a = torch.tensor(abs(float(v)), dtype=torch.float32)
    return float(torch.nextafter(a, torch.tensor(float("inf"))).double() - a.double()) if float(a) > 0 else 0.0


def needed(err: float, gap: float, floor: float) -> float:
    """The M an error needs: (err - floor) / gap, 0 at or below the floor, inf for NaN or for a zero gap with the floor exceeded."""
    if err != err:
        return float("inf")
    over = err - floor
    if over <= 0:
        return 0.0
    return over / gap if gap > 0 else float("inf")


def judge(got: Dict[str, torch.Tensor], want: Dict[str, torch.Tensor], ref32: Dict[str, torch.Tensor], margins: Optional[Dict[str, int]] = None,
          what: str = ""):
    """err <= M gap + floor per tensor: err = max|got - want|, gap = max|ref32 - want| (the restatement's own fp32 distance for that tensor on
    that case), floor = ULPS_FLOOR fp32 ulps of max|want|.  -> (failures, ratios, number of tensors compared); no tensor of `want` is skipped."""
    margins = {} if margins is None else margins
    assert all(cr.M_DEFAULT <= m <= cr.M_MAX for m in margins.values())
    assert set(got) == set(want) == set(ref32), sorted(set(got) ^ set(want))
    failures, ratios = [], {}
    for k in want:
        w, g, r = want[k].double(), got[k].detach().double().cpu().reshape(want[k].shape), ref32[k].double()
        err = float((g - w).abs().max()) if w.numel() else 0.0
        if w.numel() and bool(torch.isnan(g).any()):
            err = float("nan")
        gap = float((r - w).abs().max()) if w.numel() else 0.0
        floor = ULPS_FLOOR * ulp32(float(w.abs().max())) if w.numel() else 0.0
        ratios[k] = needed(err, gap, floor)
        M = margins.get(k, cr.M_DEFAULT)
        if not ratios[k] <= M:
            failures.append(f"{what}{k}: needs M = {ratios[k]:.3g} > {M} (err {err:.3e}, gap {gap:.3e}, floor {floor:.3e})")
    return failures, ratios, len(want)


def scalar(v) -> Dict[str, torch.Tensor]:
    return {"loss": torch.as_tensor(float(v), dtype=torch.float64).reshape(1)}


# ---- the new operator in pure Python --------------------------------------------------------------------------------------------------------------
def radial_of(x: torch.Tensor, row: torch.Tensor, col: torch.Tensor) -> torch.Tensor:
    d = x[row] - x[col]
    return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]


def edge_pre(A, B, x, w_r, sizes, dtype=torch.float64):
    """pre[(i, j)] = A[i] + B[j] + |x_i - x_j|^2 w_r and the radial, the definition of include/gcdm_classifier_train.h."""
    row, col = edge_list(sizes)
    A, B, x, w_r = A.to(dtype), B.to(dtype), x.to(dtype), w_r.to(dtype).reshape(-1)
    r = radial_of(x, row, col)
    return A[row] + B[col] + r[:, None] * w_r[None, :], r


def edge_pre_bwd(dpre, x, sizes, N: int, mutant: Optional[str] = None, dtype=torch.float64):
    """(dA, dB, dw_r) written out by hand: dA[i] = sum_j dpre[(i, j)], dB[j] = sum_i dpre[(i, j)], dw_r = sum_e r(e) dpre[e].  `mutant` names
    one wrong version of it (MUTANTS); a test of the operator must tell every one from the definition."""
    assert mutant is None or mutant in MUTANTS
    dpre, x = dpre.to(dtype), x.to(dtype)
    H = dpre.shape[1]
    dA, dB, dw = torch.zeros((N, H), dtype=dtype), torch.zeros((N, H), dtype=dtype), torch.zeros(H, dtype=dtype)
    e, o, E = 0, 0, dpre.shape[0]
    for n in sizes:
        eo = e                                                            # the molecule's first edge
        for i in range(n):
            for j in range(n):
                if i == j:
                    # the pair (i, i) put through the index formula eo + i (n - 1) + j - (j > i): a neighbouring edge's row, added to both sums
                    if mutant == "diagonal_included" and E:
                        k = min(eo + i * (n - 1) + i, E - 1)
                        dA[o + i] += dpre[k]
                        dB[o + i] += dpre[k]
                    continue
                g = dpre[e]
                a, b = (o + j, o + i) if mutant == "rows_and_columns_swapped" else (o + i, o + j)
                dA[a] += g
                dB[b] += g
                d = x[o + i] - x[o + j]
                r = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
                if mutant == "radial_dropped":
                    r = r * 0
                if mutant == "w_r_gradient_without_radial":
                    r = r * 0 + 1
                dw += r * g
                e += 1
        o += n
    return dA, dB, dw


MUTANTS = ("rows_and_columns_swapped", "radial_dropped", "diagonal_included", "w_r_gradient_without_radial")


def op_inputs(sizes: Sequence[int], H: int, seed: int = 3):
    """A, B [N, H], x [N, 3], w_r [H] and an upstream gradient dpre [E, H], fp32, seeded."""
    g = torch.Generator().manual_seed(seed + 1000 * H + len(sizes))
    N = int(sum(sizes))
    E = int(sum(n * (n - 1) for n in sizes))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    return SimpleNamespace(A=r(N, H), B=r(N, H), x=1.5 * r(N, 3), w_r=r(H), dpre=r(E, H), N=N, E=E, H=H, sizes=list(sizes))


def edge_tables(sizes: Sequence[int]):
    """node_mol [N] int32, node_offsets [B + 1] int32, edge_offsets [B + 1] int64 of include/gcdm_classifier_train.h (CPU tensors)."""
    n = torch.as_tensor(list(sizes), dtype=torch.int64)
    noff, eoff = torch.zeros(len(sizes) + 1, dtype=torch.int64), torch.zeros(len(sizes) + 1, dtype=torch.int64)
    noff[1:], eoff[1:] = torch.cumsum(n, 0), torch.cumsum(n * (n - 1), 0)
    mol = torch.repeat_interleave(torch.arange(len(sizes)), n).to(torch.int32)
    return mol, noff.to(torch.int32), eoff


def sizes_with_edges(E: int) -> List[int]:
    """Molecule sizes whose edge count is exactly E (E even): full 32-atom molecules, then one molecule per remaining n (n - 1) term."""
    assert E >= 0 and E % 2 == 0
    out = []
    while E > 0:
        n = 32
        while n * (n - 1) > E:
            n -= 1
        out.append(n)
        E -= n * (n - 1)
    return out


# ---- the operator through its C ABI -----------------------------------------------------------------------------------------------------------------
def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def cabi_edge_pre(inp, stream=None):
    """gcdm_classifier_train_edge_pre_fwd and _bwd called directly on NaN-filled, guarded outputs of exactly the advertised sizes.
    -> namespace: st_fwd / st_bwd, pre / radial / dA / dB / dw / ws (cr.Guarded; ws None below the two-stage count), ws_bytes."""
    lib = cr._ops_lib()
    dev = "cuda"
    mol, noff, eoff = (t.to(dev) for t in edge_tables(inp.sizes))
    A, B, x, w, dpre = (t.to(dev).contiguous() for t in (inp.A, inp.B, inp.x, inp.w_r, inp.dpre))
    N, E, H, nmol = inp.N, inp.E, inp.H, len(inp.sizes)
    pre, radial = cr.Guarded(E * H), cr.Guarded(E)
    st = cr._stream_ptr(stream)
    st_fwd = lib.gcdm_classifier_train_edge_pre_fwd(_ptr(A), _ptr(B), _ptr(x), _ptr(w), _ptr(mol), _ptr(noff), _ptr(eoff), pre.ptr, radial.ptr, N, nmol,
                                                    E, H, st)
    nbytes = int(lib.gcdm_classifier_train_workspace_bytes(E, H))
    assert nbytes >= 0 and nbytes % 256 == 0
    ws = cr.Guarded(nbytes // 4) if nbytes else None
    dA, dB, dw = cr.Guarded(N * H), cr.Guarded(N * H), cr.Guarded(H)
    st_bwd = lib.gcdm_classifier_train_edge_pre_bwd(_ptr(dpre), radial.ptr, _ptr(mol), _ptr(noff), _ptr(eoff), dA.ptr, dB.ptr, dw.ptr,
                                                    ws.ptr if ws is not None else ctypes.c_void_p(None), N, nmol, E, H, st)
    (stream or torch.cuda.current_stream()).synchronize()
    return SimpleNamespace(st_fwd=st_fwd, st_bwd=st_bwd, pre=pre, radial=radial, dA=dA, dB=dB, dw=dw, ws=ws, ws_bytes=nbytes, keep=(A, B, x, w, dpre, mol, noff, eoff))
