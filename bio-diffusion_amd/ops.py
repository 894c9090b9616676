"""Module-level operators of the GCPNet block on MI355X: thin autograd wrappers around libgcdm_ops.so (include/gcdm_ops.h).

Every function here launches HIP kernels -- forward in ``forward``, the backward twin in ``backward`` -- on the tensors' device and the
current stream; there is no torch / CPU fallback (a CPU tensor raises).  The Python mirrors in ``gcpnet.py`` compose these exactly where
the reference composes torch ops (src/models/components/gcpnet.py:33-491, 618-930; components/__init__.py:123-286), which is what makes
``selected_GCP(...)(s_maybe_v, edge_index, frames, ...)`` callable (plug point 3), the non-production configurations loadable, and the
training objective differentiable.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional, Tuple

import torch

from . import _native

ACT_KINDS = {None: 0, "none": 0, "identity": 0, "silu": 1, "swish": 1, "relu": 2, "sigmoid": 3, "leakyrelu": 4, "selu": 5}


def _lib():
    return _native.load_ops()


def _chk(status: int, what: str) -> None:
    if status != 0:
        raise _native.NativeError(f"{what} failed with status {status} (libgcdm_ops.so)")


def set_matrix_mode(mode: str) -> None:
    """Chooses the matrix instruction under every training GEMM of libgcdm_ops.so (include/gcdm_matrix_mode.h): ``"f32"``, the default, is
    exact fp32 MFMA; ``"bf16x6"`` is the six-product bf16 split (fp32-class accuracy, not fp32's bits, no range guard).  The switch is
    process-wide, not per thread, and each operator call reads it once when it is made: linear(), message_layer() and the fused GCP2, forward
    and backward, and nothing else."""
    if mode not in _native.MATRIX_MODES:
        raise ValueError(f"matrix mode must be one of {sorted(_native.MATRIX_MODES)}, got {mode!r}")
    _chk(_lib().gcdm_ops_set_matrix_mode(_native.MATRIX_MODES[mode]), "gcdm_ops_set_matrix_mode")


def get_matrix_mode() -> str:
    code = int(_lib().gcdm_ops_get_matrix_mode())
    return next(name for name, c in _native.MATRIX_MODES.items() if c == code)


@contextlib.contextmanager
def matrix_mode(mode: str):
    """``with ops.matrix_mode("bf16x6"):`` runs the block in that mode and restores the previous one on any exit.  A backward pass called
    after the block has exited runs in the mode current at that moment, not in the one its forward ran in: keep ``loss.backward()`` inside
    the block (or use set_matrix_mode) when the gradients are meant to run in it."""
    previous = get_matrix_mode()
    set_matrix_mode(mode)
    try:
        yield
    finally:
        set_matrix_mode(previous)


def _dev(t: torch.Tensor) -> None:
    if t.device.type != "cuda":
        raise RuntimeError("bio-diffusion_amd operators run on an MI355X only: tensors must be on a HIP ('cuda') device; there is no CPU fallback")


def _shape(ok: bool, what: str) -> None:
    """Shape checks run before the device check and before any launch: a mismatched shape would make a kernel read or write out of bounds."""
    if not ok:
        raise ValueError(what)


def _f(t: torch.Tensor) -> torch.Tensor:
    _dev(t)
    return t.detach().to(torch.float32).contiguous()


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st(t: torch.Tensor):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _gemm(A: torch.Tensor, sam: int, sak: int, B: torch.Tensor, sbk: int, sbn: int, M: int, N: int, K: int, bias: Optional[torch.Tensor] = None,
          split: bool = False) -> torch.Tensor:
    out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    if M == 0 or N == 0:
        return out
    if K == 0:
        out.zero_()
        if bias is not None:
            out += bias
        return out
    slices = 1
    if split:                       # contraction over the entities (dW): enough slices to fill the chip, reduced in slice order
        tiles = ((M + 63) // 64) * ((N + 63) // 64)
        slices = max(1, min(64, 1024 // max(tiles, 1), (K + 511) // 512))
    if slices == 1:
        _chk(_lib().gcdm_op_gemm(_p(A), sam, sak, _p(B), sbk, sbn, _p(out), _p(bias), M, N, K, 1, _st(A)), "gcdm_op_gemm")
        return out
    part = torch.empty((slices, M, N), dtype=torch.float32, device=A.device)
    _chk(_lib().gcdm_op_gemm(_p(A), sam, sak, _p(B), sbk, sbn, _p(part), _p(bias), M, N, K, slices, _st(A)), "gcdm_op_gemm")
    _chk(_lib().gcdm_op_reduce_slices(_p(part), _p(out), M * N, slices, _st(A)), "gcdm_op_reduce_slices")
    return out


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        _shape(w.dim() == 2 and x.dim() >= 1 and x.shape[-1] == w.shape[1],
               f"linear: input {tuple(x.shape)} does not match weight {tuple(w.shape)} (last axis must equal weight.shape[1])")
        _shape(b is None or (b.dim() == 1 and b.shape[0] == w.shape[0]), f"linear: bias {None if b is None else tuple(b.shape)} for weight {tuple(w.shape)}")
        xs = _f(x).reshape(-1, x.shape[-1])
        ws = _f(w)
        bs = None if b is None else _f(b)
        M, K, N = xs.shape[0], xs.shape[1], ws.shape[0]
        y = _gemm(xs, K, 1, ws, 1, K, M, N, K, bs)                       # B(k, n) = W[n][k]
        ctx.save_for_backward(xs, ws)
        ctx.has_bias = b is not None
        ctx.lead = x.shape[:-1]
        return y.reshape(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        xs, ws = ctx.saved_tensors
        M, K, N = xs.shape[0], xs.shape[1], ws.shape[0]
        g = _f(dy).reshape(M, N)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _gemm(g, N, 1, ws, K, 1, M, K, N).reshape(*ctx.lead, K)                 # dx = dy W
        if ctx.needs_input_grad[1]:
            dw = _gemm(g, 1, N, xs, K, 1, N, K, M, split=True)                            # dW = dy^T x  (A(n, m) = dy[m][n])
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = torch.empty(N, dtype=torch.float32, device=g.device)
            if M >= 4096:                # many rows: partial sums over row slices on the whole chip, then a fixed-order reduction
                slices = int(min(256, (M + 511) // 512))
                part = torch.empty((slices, N), dtype=torch.float32, device=g.device)
                _chk(_lib().gcdm_op_colsum_slices(_p(g), _p(part), M, N, slices, _st(g)), "gcdm_op_colsum_slices")
                _chk(_lib().gcdm_op_reduce_slices(_p(part), _p(db), N, slices, _st(g)), "gcdm_op_reduce_slices")
            else:
                _chk(_lib().gcdm_op_colsum(_p(g), _p(db), M, N, _st(g)), "gcdm_op_colsum")
        return dx, dw, db


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``nn.Linear`` on the last axis: y = x W^T + b (fp32 MFMA)."""
    return _Linear.apply(x, weight, bias)


class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind):
        xs = _f(x)
        y = torch.empty_like(xs)
        _chk(_lib().gcdm_op_act(kind, _p(xs), _p(y), xs.numel(), _st(xs)), "gcdm_op_act")
        ctx.save_for_backward(xs)
        ctx.kind = kind
        return y

    @staticmethod
    def backward(ctx, dy):
        (xs,) = ctx.saved_tensors
        g = _f(dy)
        dx = torch.empty_like(xs)
        _chk(_lib().gcdm_op_act_bwd(ctx.kind, _p(xs), _p(g), _p(dx), xs.numel(), _st(xs)), "gcdm_op_act_bwd")
        return dx, None


def act(x: torch.Tensor, name) -> torch.Tensor:
    """get_nonlinearity(name) of the reference (relu / leakyrelu / selu / silu / swish), 'sigmoid', or None = identity."""
    key = name.lower() if isinstance(name, str) else name
    if key not in ACT_KINDS:
        raise NotImplementedError(f"nonlinearity {name!r}")
    kind = ACT_KINDS[key]
    return x if kind == 0 else _Act.apply(x, kind)


class _Norm3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, rep_layout):
        _shape(v.dim() == 3 and v.shape[2 if rep_layout else 1] == 3,
               f"safe_norm: vectors {tuple(v.shape)} must be [M, C, 3] (rep) / [M, 3, C] (pre)")
        vs = _f(v)
        M = vs.shape[0]
        Cn = vs.shape[1] if rep_layout else vs.shape[2]
        out = torch.empty((M, Cn), dtype=torch.float32, device=vs.device)
        _chk(_lib().gcdm_op_norm3(_p(vs), _p(out), M, Cn, int(rep_layout), _st(vs)), "gcdm_op_norm3")
        ctx.save_for_backward(vs, out)
        ctx.rep = int(rep_layout)
        return out

    @staticmethod
    def backward(ctx, dout):
        vs, out = ctx.saved_tensors
        g = _f(dout)
        dv = torch.empty_like(vs)
        M, Cn = out.shape
        _chk(_lib().gcdm_op_norm3_bwd(_p(vs), _p(out), _p(g), _p(dv), M, Cn, ctx.rep, _st(vs)), "gcdm_op_norm3_bwd")
        return dv, None


def safe_norm_pre(v_pre: torch.Tensor) -> torch.Tensor:
    """safe_norm(v, dim=-2) of a vector tensor in the "pre" layout [M, 3, C] -> [M, C]."""
    return _Norm3.apply(v_pre, False)


def safe_norm_rep(v_rep: torch.Tensor) -> torch.Tensor:
    """safe_norm(v, dim=-1) of a vector tensor in the "rep" layout [M, C, 3] -> [M, C]."""
    return _Norm3.apply(v_rep, True)


class _Scalarize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u_pre, F):
        _shape(u_pre.dim() == 3 and u_pre.shape[1] == 3, f"scalarize: u {tuple(u_pre.shape)} must be [M, 3, CH]")
        _shape(F.numel() == 9 * u_pre.shape[0] and F.shape[0] == u_pre.shape[0], f"scalarize: frames {tuple(F.shape)} for {u_pre.shape[0]} rows")
        us, Fs = _f(u_pre), _f(F).reshape(-1, 9)
        M, CH = us.shape[0], us.shape[2]
        out = torch.empty((M, 3 * CH), dtype=torch.float32, device=us.device)
        _chk(_lib().gcdm_op_scalarize(_p(us), _p(Fs), _p(out), M, CH, _st(us)), "gcdm_op_scalarize")
        ctx.save_for_backward(Fs)
        ctx.CH = CH
        return out

    @staticmethod
    def backward(ctx, dout):
        (Fs,) = ctx.saved_tensors
        g = _f(dout)
        M = g.shape[0]
        du = torch.empty((M, 3, ctx.CH), dtype=torch.float32, device=g.device)
        _chk(_lib().gcdm_op_scalarize_bwd(_p(g), _p(Fs), _p(du), M, ctx.CH, _st(g)), "gcdm_op_scalarize_bwd")
        return du, None


def scalarize(u_pre: torch.Tensor, entity_frames: torch.Tensor) -> torch.Tensor:
    """u_pre [M, 3, CH] against one frame per entity [M, 3, 3] -> [M, 3 CH] in the reference's order (3 c + r).  Edge mode: the edge's
    frame; node mode: the mean of the frames of the node's edges (``mean_frames``)."""
    return _Scalarize.apply(u_pre, entity_frames)


class _Vectorize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gate, F):
        _shape(gate.dim() == 2 and gate.shape[1] % 3 == 0, f"vectorize: gate {tuple(gate.shape)} must be [M, 3 K]")
        _shape(F.numel() == 9 * gate.shape[0] and F.shape[0] == gate.shape[0], f"vectorize: frames {tuple(F.shape)} for {gate.shape[0]} rows")
        gs, Fs = _f(gate), _f(F).reshape(-1, 9)
        M, KC = gs.shape[0], gs.shape[1] // 3
        out = torch.empty((M, KC, 3), dtype=torch.float32, device=gs.device)
        _chk(_lib().gcdm_op_vectorize(_p(gs), _p(Fs), _p(out), M, KC, _st(gs)), "gcdm_op_vectorize")
        ctx.save_for_backward(Fs)
        ctx.KC = KC
        return out

    @staticmethod
    def backward(ctx, dout):
        (Fs,) = ctx.saved_tensors
        g = _f(dout)
        M = g.shape[0]
        dgate = torch.empty((M, 3 * ctx.KC), dtype=torch.float32, device=g.device)
        _chk(_lib().gcdm_op_vectorize_bwd(_p(g), _p(Fs), _p(dgate), M, ctx.KC, _st(g)), "gcdm_op_vectorize_bwd")
        return dgate, None


def vectorize(gate: torch.Tensor, entity_frames: torch.Tensor) -> torch.Tensor:
    """gate [M, 3 K] -> vectors [M, K, 3]: gate[3k] a + gate[3k+1] b + gate[3k+2] c with (a, b, c) the rows of the entity's frame."""
    return _Vectorize.apply(gate, entity_frames)


class _RowScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v_rep, g):
        _shape(v_rep.dim() == 3 and v_rep.shape[2] == 3, f"rowscale: vectors {tuple(v_rep.shape)} must be [M, C, 3]")
        _shape(g.shape[0] == v_rep.shape[0] and g.numel() == v_rep.shape[0] * v_rep.shape[1],
               f"rowscale: gate {tuple(g.shape)} for vectors {tuple(v_rep.shape)}")
        vs, gs = _f(v_rep), _f(g)
        M, Cn = vs.shape[0], vs.shape[1]
        out = torch.empty_like(vs)
        _chk(_lib().gcdm_op_rowscale(_p(vs), _p(gs), _p(out), M, Cn, _st(vs)), "gcdm_op_rowscale")
        ctx.save_for_backward(vs, gs)
        return out

    @staticmethod
    def backward(ctx, dout):
        vs, gs = ctx.saved_tensors
        d = _f(dout)
        dv, dg = torch.empty_like(vs), torch.empty_like(gs)
        _chk(_lib().gcdm_op_rowscale_bwd(_p(vs), _p(gs), _p(d), _p(dv), _p(dg), vs.shape[0], vs.shape[1], _st(vs)), "gcdm_op_rowscale_bwd")
        return dv, dg


def rowscale(v_rep: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """v_rep [M, C, 3] * g [M, C] (or [M, C, 1])."""
    _shape(g.dim() >= 1, "rowscale: the gate must have a row axis")
    return _RowScale.apply(v_rep, g.reshape(g.shape[0], -1))


# ---- graph plumbing ---------------------------------------------------------------------------------------------------------------------
class Graph:
    """CSR view of a row-sorted edge list (what get_fully_connected_edge_index produces): rowptr on the device, built once per edge_index."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int):
        _shape(edge_index.dim() == 2 and edge_index.shape[0] == 2, f"edge_index {tuple(edge_index.shape)} must be [2, E]")
        _shape(int(num_nodes) >= 0, f"num_nodes = {num_nodes}")
        N = int(num_nodes)
        # an index outside [0, N) would make the gathers / scatters read or write out of bounds: bit 1 of the flag, read back together with the
        # sortedness bit (one device-to-host read, as before)
        bad = ((edge_index < 0) | (edge_index >= N)).any()
        if edge_index.device.type != "cuda" and bool(bad):
            raise IndexError(f"edge_index holds a node index outside [0, {N})")
        _dev(edge_index)
        self.row = edge_index[0].to(torch.int64).contiguous()
        self.col = edge_index[1].to(torch.int64).contiguous()
        self.N, self.E = N, int(self.row.shape[0])
        self.rowptr = torch.empty(self.N + 1, dtype=torch.int32, device=self.row.device)
        flag = torch.zeros(1, dtype=torch.int32, device=self.row.device)
        _chk(_lib().gcdm_op_rowptr(_p(self.row), self.E, self.N, _p(self.rowptr), _p(flag), _st(self.row)), "gcdm_op_rowptr")
        flag |= bad.to(torch.int32) << 1
        f = int(flag.item())
        if f & 2:
            raise IndexError(f"edge_index holds a node index outside [0, {N})")
        if f & 1:
            raise ValueError("edge_index must be sorted by its first row (source node), as get_fully_connected_edge_index produces it")
        self._col_order = None

    @classmethod
    def from_parts(cls, edge_index: torch.Tensor, num_nodes: int, rowptr: torch.Tensor, colperm: torch.Tensor, colptr: torch.Tensor) -> "Graph":
        """Trusted constructor: the caller (the data loader's collation kernel, include/gcdm_data.h) vouches that ``edge_index`` [2, E] int64 is
        sorted by row with every index in [0, num_nodes), and that rowptr / (colperm, colptr) are what ``Graph(edge_index, num_nodes)`` and
        ``col_order()`` would compute.  Shapes and dtypes are checked on the host; no launch, no device-to-host copy."""
        _shape(edge_index.dim() == 2 and edge_index.shape[0] == 2 and edge_index.dtype == torch.int64 and edge_index.is_contiguous(),
               f"edge_index {tuple(edge_index.shape)} {edge_index.dtype} must be a contiguous int64 [2, E]")
        N, E = int(num_nodes), int(edge_index.shape[1])
        _shape(N >= 0, f"num_nodes = {num_nodes}")
        for name, t, n, dt in (("rowptr", rowptr, N + 1, torch.int32), ("colperm", colperm, E, torch.int64), ("colptr", colptr, N + 1, torch.int32)):
            _shape(t.dim() == 1 and t.shape[0] == n and t.dtype == dt and t.is_contiguous() and t.device == edge_index.device,
                   f"{name} {tuple(t.shape)} {t.dtype} must be a contiguous {dt} [{n}] on {edge_index.device}")
        _dev(edge_index)
        g = cls.__new__(cls)
        g.edge_index, g.row, g.col = edge_index, edge_index[0], edge_index[1]
        g.N, g.E = N, E
        g.rowptr = rowptr
        g._col_order = (colperm, colptr)
        return g

    def col_order(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(colperm, colptr): a stable argsort of col and the CSR pointers of col[colperm] -- the fixed order of every column sum of the fused
        message layer's backward.  Computed once per graph."""
        if self._col_order is None:
            perm = torch.sort(self.col, stable=True).indices
            colptr = torch.empty(self.N + 1, dtype=torch.int32, device=self.col.device)
            flag = torch.zeros(1, dtype=torch.int32, device=self.col.device)
            csorted = self.col[perm].contiguous()
            _chk(_lib().gcdm_op_rowptr(_p(csorted), self.E, self.N, _p(colptr), _p(flag), _st(csorted)), "gcdm_op_rowptr")
            self._col_order = (perm.contiguous(), colptr)
        return self._col_order


_GRAPH_CACHE = {}


def graph_of(edge_index: torch.Tensor, num_nodes: int) -> Graph:
    key = (edge_index.data_ptr(), tuple(edge_index.shape), _native.tensor_version(edge_index), int(num_nodes))
    g = _GRAPH_CACHE.get("g")
    if g is None or _GRAPH_CACHE.get("key") != key:
        g = Graph(edge_index, num_nodes)
        _GRAPH_CACHE["g"], _GRAPH_CACHE["key"], _GRAPH_CACHE["keep"] = g, key, edge_index
    return g


def register_graph(graph: Graph, edge_index: torch.Tensor) -> None:
    """Makes ``graph_of(edge_index, graph.N)`` return ``graph`` (a Graph.from_parts of that very tensor) instead of building one."""
    _shape(edge_index.dim() == 2 and edge_index.shape[0] == 2 and edge_index.shape[1] == graph.E and edge_index[0].data_ptr() == graph.row.data_ptr(),
           "register_graph: the graph was not made from this edge_index")
    key = (edge_index.data_ptr(), tuple(edge_index.shape), _native.tensor_version(edge_index), int(graph.N))
    _GRAPH_CACHE["g"], _GRAPH_CACHE["key"], _GRAPH_CACHE["keep"] = graph, key, edge_index


class _Gather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, graph, by_row):
        _shape(x.dim() >= 1 and x.shape[0] == graph.N, f"gather: x {tuple(x.shape)} for a graph of {graph.N} nodes")
        xs = _f(x).reshape(x.shape[0], -1)
        idx = graph.row if by_row else graph.col
        out = torch.empty((graph.E, xs.shape[1]), dtype=torch.float32, device=xs.device)
        _chk(_lib().gcdm_op_gather(_p(xs), _p(idx), _p(out), graph.E, xs.shape[1], _st(xs)), "gcdm_op_gather")
        ctx.graph, ctx.by_row, ctx.shape = graph, by_row, x.shape
        if not by_row and ctx.needs_input_grad[0]:
            graph.col_order()          # the backward's fixed summation order, made here: once per graph, on the forward's stream
        return out.reshape(graph.E, *x.shape[1:])

    @staticmethod
    def backward(ctx, dout):
        g = _f(dout).reshape(ctx.graph.E, -1)
        Cn = g.shape[1]
        if ctx.by_row:           # sorted index: a deterministic segment sum
            dx = torch.empty((ctx.graph.N, Cn), dtype=torch.float32, device=g.device)
            _chk(_lib().gcdm_op_segment_sum(_p(g), _p(ctx.graph.rowptr), _p(dx), ctx.graph.N, Cn, 0, _st(g)), "gcdm_op_segment_sum")
        else:                    # column index: the rows in the graph's stable column order, then the same segment sum -- no atomics, so the
            # gradient has the same bits from run to run (the order is the one the fused message layer's backward sums in)
            colperm, colptr = ctx.graph.col_order()
            by_col = torch.empty_like(g)
            _chk(_lib().gcdm_op_gather(_p(g), _p(colperm), _p(by_col), ctx.graph.E, Cn, _st(g)), "gcdm_op_gather")
            dx = torch.empty((ctx.graph.N, Cn), dtype=torch.float32, device=g.device)
            _chk(_lib().gcdm_op_segment_sum(_p(by_col), _p(colptr), _p(dx), ctx.graph.N, Cn, 0, _st(g)), "gcdm_op_segment_sum")
        return dx.reshape(ctx.shape), None, None


class _Embedding(torch.autograd.Function):
    """rows of a table by integer index (nn.Embedding's forward; backward: fp32 atomic adds onto the table's gradient)."""

    @staticmethod
    def forward(ctx, weight, index):
        _shape(weight.dim() == 2, f"embedding: table {tuple(weight.shape)} must be [num, dim]")
        idx = index.reshape(-1).to(torch.int64).contiguous()
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= weight.shape[0]):
            raise IndexError(f"embedding index out of range [0, {weight.shape[0]})")
        w = _f(weight)
        _dev(idx)
        out = torch.empty((idx.numel(), w.shape[1]), dtype=torch.float32, device=w.device)
        _chk(_lib().gcdm_op_gather(_p(w), _p(idx), _p(out), idx.numel(), w.shape[1], _st(w)), "gcdm_op_gather")
        ctx.idx, ctx.rows = idx, w.shape[0]
        return out.reshape(*index.shape, w.shape[1])

    @staticmethod
    def backward(ctx, dout):
        g = _f(dout).reshape(ctx.idx.numel(), -1)
        dw = torch.zeros((ctx.rows, g.shape[1]), dtype=torch.float32, device=g.device)
        _chk(_lib().gcdm_op_scatter_add(_p(g), _p(ctx.idx), _p(dw), ctx.idx.numel(), g.shape[1], _st(g)), "gcdm_op_scatter_add")
        return dw, None


def embedding(weight: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """`nn.Embedding(num, dim)(index)` (gcpnet.py:540-549, 569-570: the atom-type table of `GCPEmbedding`)."""
    return _Embedding.apply(weight, index)


def gather_row(x: torch.Tensor, graph: Graph) -> torch.Tensor:
    return _Gather.apply(x, graph, True)


def gather_col(x: torch.Tensor, graph: Graph) -> torch.Tensor:
    return _Gather.apply(x, graph, False)


class _SegmentReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, graph, mean):
        _shape(x.dim() >= 1 and x.shape[0] == graph.E, f"scatter_rows: x {tuple(x.shape)} for a graph of {graph.E} edges")
        xs = _f(x).reshape(x.shape[0], -1)
        out = torch.empty((graph.N, xs.shape[1]), dtype=torch.float32, device=xs.device)
        _chk(_lib().gcdm_op_segment_sum(_p(xs), _p(graph.rowptr), _p(out), graph.N, xs.shape[1], int(mean), _st(xs)), "gcdm_op_segment_sum")
        ctx.graph, ctx.mean, ctx.shape = graph, int(mean), x.shape
        return out.reshape(graph.N, *x.shape[1:])

    @staticmethod
    def backward(ctx, dout):
        g = _f(dout).reshape(ctx.graph.N, -1)
        dx = torch.empty((ctx.graph.E, g.shape[1]), dtype=torch.float32, device=g.device)
        _chk(_lib().gcdm_op_segment_bwd(_p(g), _p(ctx.graph.row), _p(ctx.graph.rowptr), _p(dx), ctx.graph.E, g.shape[1], ctx.mean, _st(g)),
             "gcdm_op_segment_bwd")
        return dx.reshape(ctx.shape), None, None


def scatter_rows(x: torch.Tensor, graph: Graph, reduce: str = "sum") -> torch.Tensor:
    """torch_scatter.scatter(x, row, dim=0, dim_size=N, reduce=sum | mean) for a row-sorted edge list (summation in edge order)."""
    if reduce not in ("sum", "mean"):
        raise NotImplementedError(f"reduce={reduce!r}")
    return _SegmentReduce.apply(x, graph, reduce == "mean")


def mean_frames(frames: torch.Tensor, graph: Graph, edge_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-node mean of the frames of its edges [N, 3, 3] (masked edges contribute zeros but count, as in the reference's scatter-mean)."""
    _shape(frames.numel() == 9 * graph.E and frames.shape[0] == graph.E, f"mean_frames: frames {tuple(frames.shape)} for {graph.E} edges")
    _shape(edge_mask is None or edge_mask.numel() == graph.E, f"mean_frames: edge_mask of {None if edge_mask is None else edge_mask.numel()} entries")
    f = _f(frames).reshape(-1, 9)
    if edge_mask is not None:
        f = f * edge_mask.to(f.dtype).unsqueeze(-1)
    out = torch.empty((graph.N, 9), dtype=torch.float32, device=f.device)
    _chk(_lib().gcdm_op_segment_sum(_p(f), _p(graph.rowptr), _p(out), graph.N, 9, 1, _st(f)), "gcdm_op_segment_sum")
    return out.reshape(graph.N, 3, 3)


# ---- geometry of the network input (no gradients) -----------------------------------------------------------------------------------------
def _geometry_shapes(x: torch.Tensor, edge_index: Optional[torch.Tensor], what: str) -> None:
    _shape(x.dim() == 2 and x.shape[1] == 3, f"{what}: positions {tuple(x.shape)} must be [N, 3]")
    _shape(edge_index is None or (edge_index.dim() == 2 and edge_index.shape[0] == 2), f"{what}: edge_index must be [2, E]")


_RANGE_CACHE = {}


def _node_range(edge_index: torch.Tensor, num_nodes: int, what: str) -> None:
    """Refuses node indices outside [0, N) on the host before a kernel reads positions at them.  One device-to-host read per edge_index:
    the last one that passed is remembered under the same key as graph_of (localize and edge_features of a forward share it)."""
    key = (edge_index.data_ptr(), tuple(edge_index.shape), _native.tensor_version(edge_index), str(edge_index.device), int(num_nodes))
    if _RANGE_CACHE.get("key") == key:
        return
    if edge_index.numel() and bool(((edge_index < 0) | (edge_index >= num_nodes)).any()):
        raise IndexError(f"{what}: edge_index holds a node index outside [0, {num_nodes})")
    _RANGE_CACHE["key"], _RANGE_CACHE["keep"] = key, edge_index


def localize(x: torch.Tensor, edge_index: torch.Tensor, norm_x_diff: bool = True) -> torch.Tensor:
    _geometry_shapes(x, edge_index, "localize")
    _node_range(edge_index, x.shape[0], "localize")
    xs = _f(x)
    row, col = edge_index[0].to(torch.int64).contiguous(), edge_index[1].to(torch.int64).contiguous()
    E = int(row.shape[0])
    F = torch.empty((E, 3, 3), dtype=torch.float32, device=xs.device)
    _chk(_lib().gcdm_op_localize(_p(xs), _p(row), _p(col), _p(F), E, int(norm_x_diff), _st(xs)), "gcdm_op_localize")
    return F


def edge_features(x: torch.Tensor, edge_index: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    _geometry_shapes(x, edge_index, "edge_features")
    _node_range(edge_index, x.shape[0], "edge_features")
    xs = _f(x)
    row, col = edge_index[0].to(torch.int64).contiguous(), edge_index[1].to(torch.int64).contiguous()
    E = int(row.shape[0])
    e = torch.empty((E, 1), dtype=torch.float32, device=xs.device)
    xi = torch.empty((E, 1, 3), dtype=torch.float32, device=xs.device)
    _chk(_lib().gcdm_op_edge_features(_p(xs), _p(row), _p(col), _p(e), _p(xi), E, _st(xs)), "gcdm_op_edge_features")
    return e, xi


def orientations(x: torch.Tensor) -> torch.Tensor:
    _geometry_shapes(x, None, "orientations")
    xs = _f(x)
    out = torch.empty((xs.shape[0], 2, 3), dtype=torch.float32, device=xs.device)
    _chk(_lib().gcdm_op_orientations(_p(xs), _p(out), xs.shape[0], _st(xs)), "gcdm_op_orientations")
    return out


class _Centralize(torch.autograd.Function):
    """x -> (x - mean over the molecule's unmasked nodes) on unmasked rows, 0 on masked rows: a symmetric projection, so the backward is
    the same kernel applied to the incoming gradient."""

    @staticmethod
    def _run(xs, bi, mk):
        out = torch.empty_like(xs)
        _chk(_lib().gcdm_op_centralize(_p(xs), _p(bi), _p(mk), _p(out), xs.shape[0], xs.shape[1], _st(xs)), "gcdm_op_centralize")
        return out

    @staticmethod
    def forward(ctx, x, bi, mk):
        ctx.bi, ctx.mk = bi, mk
        return _Centralize._run(_f(x), bi, mk)

    @staticmethod
    def backward(ctx, dout):
        return _Centralize._run(_f(dout), ctx.bi, ctx.mk), None, None


def centralize(x: torch.Tensor, batch_index: torch.Tensor, node_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    _shape(x.dim() == 2, f"centralize: x {tuple(x.shape)} must be [N, D]")
    _shape(batch_index.numel() == x.shape[0], f"centralize: batch_index of {batch_index.numel()} entries for {x.shape[0]} rows")
    _shape(node_mask is None or node_mask.numel() == x.shape[0], f"centralize: node_mask of {None if node_mask is None else node_mask.numel()} entries")
    bi = batch_index.to(torch.int64).contiguous()
    mk = None if node_mask is None else node_mask.to(torch.uint8).contiguous()
    return _Centralize.apply(x, bi, mk)


def fully_connected_edge_index(num_nodes: torch.Tensor, device) -> torch.Tensor:
    """get_fully_connected_edge_index (gcpnet.py:1054-1066) from the molecule sizes: [2, sum n^2] int64, self-loops included, sorted."""
    nn_ = torch.as_tensor(num_nodes, dtype=torch.int64, device="cpu")
    _shape(nn_.dim() == 1 and bool((nn_ >= 0).all()), f"fully_connected_edge_index: molecule sizes must be a list of counts >= 0, got {nn_.tolist()}")
    noff = torch.zeros(len(nn_) + 1, dtype=torch.int32)
    noff[1:] = torch.cumsum(nn_, 0).to(torch.int32)
    eoff = torch.zeros(len(nn_) + 1, dtype=torch.int64)
    eoff[1:] = torch.cumsum(nn_ * nn_, 0)
    E = int(eoff[-1])
    dev = torch.device(device)
    noff_d, eoff_d = noff.to(dev), eoff.to(dev)
    ei = torch.empty((2, E), dtype=torch.int64, device=dev)
    _chk(_lib().gcdm_op_fc_edges(_p(noff_d), _p(eoff_d), len(nn_), C.c_void_p(ei.data_ptr()), C.c_void_p(ei.data_ptr() + 8 * E), E,
                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "gcdm_op_fc_edges")
    return ei


# ---- the message function of one interaction layer as one autograd node (include/gcdm_mp_train.h) -------------------------------------------
MP_NODE_DIMS = (256, 32)
MP_EDGE_DIMS = ((64, 16), (16, 8))
MP_NUM_WEIGHTS = 30


MP_PATHS = ("fused", "tiled")          # include/gcdm_mp_train.h | include/gcdm_mp_tile.h (one tile kernel per message GCP): same arguments, same tape
_MP_ENTRIES = {"fused": ("gcdm_mp_workspace_bytes", "gcdm_mp_fwd", "gcdm_mp_bwd"),
               "tiled": ("gcdm_mp_tile_workspace_bytes", "gcdm_mp_tile_fwd", "gcdm_mp_tile_bwd")}


def mp_workspace_bytes(which: int, N: int, E: int, SE: int, VE: int, path: str = "fused") -> int:
    name = _MP_ENTRIES[path][0]
    n = int(getattr(_lib(), name)(int(which), int(N), int(E), int(SE), int(VE)))
    if n < 0:
        raise ValueError(f"{name}({which}, N={N}, E={E}, SE={SE}, VE={VE}): bad argument")
    return n


def _mp_shapes(h, chi, e, xi, frames, graph, weights):
    N, E = graph.N, graph.E
    _shape(len(weights) == MP_NUM_WEIGHTS, f"message_layer: {len(weights)} weight tensors, expected {MP_NUM_WEIGHTS}")
    _shape(tuple(h.shape) == (N, MP_NODE_DIMS[0]), f"message_layer: h {tuple(h.shape)} must be [{N}, {MP_NODE_DIMS[0]}]")
    _shape(tuple(chi.shape) == (N, MP_NODE_DIMS[1], 3), f"message_layer: chi {tuple(chi.shape)} must be [{N}, {MP_NODE_DIMS[1]}, 3]")
    _shape(e.dim() == 2 and e.shape[0] == E and xi.dim() == 3 and tuple(xi.shape[::2]) == (E, 3) and (e.shape[1], xi.shape[1]) in MP_EDGE_DIMS,
           f"message_layer: edge features {tuple(e.shape)} / {tuple(xi.shape)}: edge dims must be one of {MP_EDGE_DIMS} for {E} edges")
    _shape(frames.shape[0] == E and frames.numel() == 9 * E, f"message_layer: frames {tuple(frames.shape)} for {E} edges")
    SE, VE = int(e.shape[1]), int(xi.shape[1])
    vin0, h0 = 2 * MP_NODE_DIMS[1] + VE, (2 * MP_NODE_DIMS[1] + VE) // 4
    want = []
    for k in range(4):
        hk, vin, kin = (h0, vin0, 2 * 256 + SE + h0 + 9) if k == 0 else (8, 32, 256 + 8 + 9)
        want += [(hk, vin), (3, vin), (256, kin), (256,), (32, hk), (32, 256), (32,)]
    want += [(1, 256), (1,)]
    for i, (w, s) in enumerate(zip(weights, want)):
        _shape(tuple(w.shape) == s, f"message_layer: weight {i} has shape {tuple(w.shape)}, expected {s}")
    for t in (h, chi, e, xi, frames, *weights):
        if t.dtype != torch.float32:
            raise TypeError(f"message_layer: the fused message layer computes in fp32; got a {t.dtype} tensor")
        _dev(t)
    return SE, VE


class _MessageLayer(torch.autograd.Function):
    """GCPMessagePassing.forward of the production message configuration: two C calls (gcdm_mp_fwd / gcdm_mp_bwd, or the two tiled entries
    of include/gcdm_mp_tile.h when ``path`` is "tiled").  The tape -- what the backward reads -- is one workspace tensor held by the context
    and dropped by the backward; under no_grad the forward writes none."""

    @staticmethod
    def forward(ctx, h, chi, e, xi, frames, graph, edge_mask, record, path, *weights):
        _, fwd_name, _ = _MP_ENTRIES[path]
        SE, VE = _mp_shapes(h, chi, e, xi, frames, graph, weights)
        N, E = graph.N, graph.E
        hs, cs, es, xs = h.detach().contiguous(), chi.detach().contiguous(), e.detach().contiguous(), xi.detach().contiguous()
        fs = frames.detach().reshape(E, 9).contiguous()
        ws = [w.detach().contiguous() for w in weights]
        mk = None if edge_mask is None else edge_mask.reshape(-1).to(torch.uint8).contiguous()
        _shape(mk is None or mk.numel() == E, "message_layer: edge_mask must have one entry per edge")
        alloc = torch.zeros if E == 0 else torch.empty          # no edges: the library writes nothing, the sums are zero
        agg = alloc((N, 256 + 3 * 32), dtype=torch.float32, device=h.device)
        tape = bool(record)                 # (grad mode is off inside forward: the caller says whether a graph is being recorded)
        ws_t = torch.empty(mp_workspace_bytes(int(tape), N, E, SE, VE, path) // 4, dtype=torch.float32, device=h.device)
        wp = (C.c_void_p * MP_NUM_WEIGHTS)(*[w.data_ptr() for w in ws])
        _chk(getattr(_lib(), fwd_name)(_p(hs), _p(cs), _p(es), _p(xs), _p(graph.row), _p(graph.col), _p(graph.rowptr), _p(fs), _p(mk), wp, _p(agg),
                                       _p(ws_t), int(tape), N, E, SE, VE, _st(hs)), fwd_name)
        ctx.tape = ws_t if tape else None
        del ws_t
        ctx.graph, ctx.frames, ctx.mask, ctx.dims, ctx.path = graph, fs, mk, (N, E, SE, VE), path
        ctx.save_for_backward(hs, *weights)
        ctx.ws = ws
        return agg

    @staticmethod
    def backward(ctx, dagg):
        if torch.is_grad_enabled():
            raise RuntimeError("message_layer (fused message path): double backward (create_graph=True) is not supported; use the operator path")
        if ctx.tape is None:
            raise RuntimeError("message_layer: the tape of this forward is gone (a second backward through the same graph is not supported)")
        saved = ctx.saved_tensors
        hs = saved[0]
        N, E, SE, VE = ctx.dims
        g = _f(dagg).reshape(N, 256 + 3 * 32)
        dev = g.device
        colperm, colptr = ctx.graph.col_order()
        alloc = torch.zeros if E == 0 else torch.empty
        dh = alloc((N, 256), dtype=torch.float32, device=dev)
        dchi = alloc((N, 32, 3), dtype=torch.float32, device=dev)
        de = alloc((E, SE), dtype=torch.float32, device=dev)
        dxi = alloc((E, VE, 3), dtype=torch.float32, device=dev)
        bwd_name = _MP_ENTRIES[ctx.path][2]
        dw = alloc(mp_workspace_bytes(3, N, E, SE, VE, ctx.path) // 4, dtype=torch.float32, device=dev)
        scratch = torch.empty(mp_workspace_bytes(2, N, E, SE, VE, ctx.path) // 4, dtype=torch.float32, device=dev)
        wp = (C.c_void_p * MP_NUM_WEIGHTS)(*[w.data_ptr() for w in ctx.ws])
        _chk(getattr(_lib(), bwd_name)(_p(g), _p(hs), _p(ctx.graph.row), _p(ctx.graph.col), _p(ctx.graph.rowptr), _p(colptr), _p(colperm),
                                       _p(ctx.frames), _p(ctx.mask), wp, _p(ctx.tape), _p(scratch), _p(dh), _p(dchi), _p(de), _p(dxi), _p(dw), N, E, SE,
                                       VE, _st(g)), bwd_name)
        ctx.tape = None
        del scratch
        grads, o = [], 0
        for w in ctx.ws:
            grads.append(dw[o: o + w.numel()].view(w.shape))
            o += w.numel()
        ctx.ws = None
        need = ctx.needs_input_grad
        return ((dh if need[0] else None), (dchi if need[1] else None), (de if need[2] else None), (dxi if need[3] else None), None, None, None, None,
                None, *[gr if need[9 + i] else None for i, gr in enumerate(grads)])


def message_layer(h: torch.Tensor, chi: torch.Tensor, e: torch.Tensor, xi: torch.Tensor, frames: torch.Tensor, graph: Graph, weights,
                  edge_mask: Optional[torch.Tensor] = None, path: str = "fused") -> Tuple[torch.Tensor, torch.Tensor]:
    """The message function + sum aggregation of one interaction layer (GCPMessagePassing.forward, production configuration) as one autograd
    node on libgcdm_ops.so's fused kernels.  ``weights``: the 30 tensors in the order of include/gcdm_mp_train.h.  -> (agg_s [N, 256],
    agg_v [N, 32, 3]).  Raises (no fallback) for shapes, dims or dtypes the kernels do not take; the edge list must be row-sorted (``graph``).
    ``path``: "fused" (include/gcdm_mp_train.h) or "tiled" (include/gcdm_mp_tile.h: each message GCP's GEMMs and element-wise kernels in one
    tile kernel, 12 + 17 launches instead of 24 + 25)."""
    if path not in MP_PATHS:
        raise ValueError(f"message_layer: path must be one of {MP_PATHS}, got {path!r}")
    record = torch.is_grad_enabled() and any(t.requires_grad for t in (h, chi, e, xi, *weights))
    agg = _MessageLayer.apply(h, chi, e, xi, frames, graph, edge_mask, record, path, *weights)
    return agg[:, :256], agg[:, 256:].reshape(graph.N, 32, 3)


# ---- one stand-alone GCP2 module as one autograd node (include/gcdm_gcp2_train.h) -----------------------------------------------------------
GCP2_MAX = _native.GCP2_MAX
_GCP2_ACTS = {None: 0, "none": 0, "identity": 0, "silu": 1, "swish": 1}


def gcp2_act_code(name) -> int:
    """0 identity | 1 silu, the two nonlinearities the fused GCP2 takes; raises ValueError for another one."""
    key = name.lower() if isinstance(name, str) else name
    if key not in _GCP2_ACTS:
        raise ValueError(f"gcp2_fused: nonlinearity {name!r} (identity or silu)")
    return _GCP2_ACTS[key]


def gcp2_why_not_dims(SI: int, VI: int, SO: int, VO: int, H: int) -> Optional[str]:
    """None if the dims are inside the bounds of include/gcdm_gcp2_train.h, else the first one that is not."""
    for name, val, lo in (("SI", SI, 1), ("VI", VI, 1), ("SO", SO, 1), ("VO", VO, 0), ("H", H, 1)):
        if not lo <= int(val) <= GCP2_MAX[name]:
            return f"{name} = {val} outside [{lo}, {GCP2_MAX[name]}]"
    return None


def _gcp2_dims(SI, VI, SO, VO, H, feedforward_out, act_scalar, act_vector) -> "_native.Gcp2Dims":
    return _native.Gcp2Dims(int(SI), int(VI), int(SO), int(VO), int(H), int(bool(feedforward_out)), int(act_scalar), int(act_vector))


def gcp2_workspace_bytes(which: int, M: int, dims) -> int:
    n = int(_lib().gcdm_gcp2_workspace_bytes(int(which), int(M), C.byref(dims)))
    if n < 0:
        raise ValueError(f"gcdm_gcp2_workspace_bytes({which}, M={M}, dims={[getattr(dims, f) for f, _ in dims._fields_]}): bad argument")
    return n


def _gcp2_weight_shapes(SI, VI, SO, VO, H, ff):
    K = SI + H + 9
    want = [(H, VI), (3, VI), (SO, K), (SO,)]
    if ff:
        want += [(SO, SO), (SO,)]
    if VO:
        want += [(VO, H), (VO, SO), (VO,)]
    return want


class _GCP2Fused(torch.autograd.Function):
    """GCP2.forward of one stand-alone module: two C calls (gcdm_gcp2_fwd / gcdm_gcp2_bwd).  The tape -- what the backward reads beyond s, v and
    the weights -- is one workspace tensor held by the context and dropped by the backward; under no_grad the forward writes none."""

    @staticmethod
    def forward(ctx, s, v, F, row_mask, dims, record, *weights):
        SI, VI, SO, VO, H, ff, a0, a1 = dims
        M = int(s.shape[0])
        _shape(s.dim() == 2 and s.shape[1] == SI, f"gcp2_fused: s {tuple(s.shape)} must be [M, {SI}]")
        _shape(tuple(v.shape) == (M, VI, 3), f"gcp2_fused: v {tuple(v.shape)} must be [{M}, {VI}, 3]")
        _shape(F.shape[0] == M and F.numel() == 9 * M, f"gcp2_fused: frames {tuple(F.shape)} for {M} rows")
        why = gcp2_why_not_dims(SI, VI, SO, VO, H)
        _shape(why is None, f"gcp2_fused: {why}")
        want = _gcp2_weight_shapes(SI, VI, SO, VO, H, ff)
        _shape(len(weights) == len(want), f"gcp2_fused: {len(weights)} weight tensors, expected {len(want)}")
        for i, (w, shp) in enumerate(zip(weights, want)):
            _shape(tuple(w.shape) == shp, f"gcp2_fused: weight {i} has shape {tuple(w.shape)}, expected {shp}")
        for t in (s, v, F, *weights):
            if t.dtype != torch.float32:
                raise TypeError(f"gcp2_fused: the fused GCP2 computes in fp32; got a {t.dtype} tensor")
            _dev(t)
        ss, vs, fs = s.detach().contiguous(), v.detach().contiguous(), F.detach().reshape(M, 9).contiguous()
        ws = [w.detach().contiguous() for w in weights]
        mk = None if row_mask is None else row_mask.reshape(-1).to(torch.uint8).contiguous()
        _shape(mk is None or mk.numel() == M, "gcp2_fused: row_mask must have one entry per row")
        cd = _gcp2_dims(SI, VI, SO, VO, H, ff, a0, a1)
        s_out = torch.empty((M, SO), dtype=torch.float32, device=s.device)
        v_out = torch.empty((M, VO, 3), dtype=torch.float32, device=s.device)
        tape = bool(record)                 # (grad mode is off inside forward: the caller says whether a graph is being recorded)
        ws_t = torch.empty(gcp2_workspace_bytes(int(tape), M, cd) // 4, dtype=torch.float32, device=s.device)
        wp = (C.c_void_p * len(ws))(*[w.data_ptr() for w in ws])
        _chk(_lib().gcdm_gcp2_fwd(_p(ss), _p(vs), _p(fs), _p(mk), wp, _p(s_out), _p(v_out) if VO else None, _p(ws_t), int(tape), M, C.byref(cd),
                                  _st(ss)), "gcdm_gcp2_fwd")
        ctx.tape = ws_t if tape else None
        del ws_t
        ctx.frames, ctx.mask, ctx.cd, ctx.M, ctx.VO = fs, mk, cd, M, VO
        ctx.save_for_backward(ss, vs, *weights)
        ctx.ws = ws
        if not VO:
            ctx.mark_non_differentiable(v_out)
        return s_out, v_out

    @staticmethod
    def backward(ctx, ds_out, dv_out):
        if torch.is_grad_enabled():
            raise RuntimeError("gcp2_fused (fused node path): double backward (create_graph=True) is not supported; use the operator path")
        if ctx.tape is None:
            raise RuntimeError("gcp2_fused: the tape of this forward is gone (a second backward through the same graph is not supported)")
        saved = ctx.saved_tensors
        ss, vs = saved[0], saved[1]
        M, cd, VO = ctx.M, ctx.cd, ctx.VO
        dev = ss.device
        gs = _f(ds_out).reshape(M, cd.SO)
        gv = _f(dv_out).reshape(M, VO, 3) if VO else None
        alloc = torch.zeros if M == 0 else torch.empty          # no rows: the library writes nothing, the gradients are zero
        ds = alloc((M, cd.SI), dtype=torch.float32, device=dev)
        dv = alloc((M, cd.VI, 3), dtype=torch.float32, device=dev)
        dw = alloc(gcp2_workspace_bytes(3, M, cd) // 4, dtype=torch.float32, device=dev)
        scratch = torch.empty(gcp2_workspace_bytes(2, M, cd) // 4, dtype=torch.float32, device=dev)
        wp = (C.c_void_p * len(ctx.ws))(*[w.data_ptr() for w in ctx.ws])
        _chk(_lib().gcdm_gcp2_bwd(_p(gs), _p(gv), _p(ss), _p(vs), _p(ctx.frames), _p(ctx.mask), wp, _p(ctx.tape), _p(scratch), _p(ds), _p(dv), _p(dw),
                                  M, C.byref(cd), _st(gs)), "gcdm_gcp2_bwd")
        ctx.tape = None
        del scratch
        grads, o = [], 0
        for w in ctx.ws:
            grads.append(dw[o: o + w.numel()].view(w.shape))
            o += w.numel()
        ctx.ws = None
        need = ctx.needs_input_grad
        return ((ds if need[0] else None), (dv if need[1] else None), None, None, None, None,
                *[gr if need[6 + i] else None for i, gr in enumerate(grads)])


def gcp2_fused(s: torch.Tensor, v: torch.Tensor, F: torch.Tensor, weights, SO: int, VO: int, H: int, feedforward_out: bool = False,
               act_scalar=None, act_vector=None, row_mask: Optional[torch.Tensor] = None):
    """One stand-alone GCP2 (vector_gate, no frame gate, no residuals, no ablations) as one autograd node on libgcdm_ops.so's fused kernels.
    ``s`` [M, SI], ``v`` [M, VI, 3], ``F`` [M, 3, 3] the entity frames (constant: no gradient), ``weights`` the module's Linear tensors in
    state-dict order (include/gcdm_gcp2_train.h), ``H`` its hidden_dim, the nonlinearities None / "silu"; ``row_mask`` [M]: False zeroes the
    row's frame.  -> (s_out [M, SO], v_out [M, VO, 3]).  Raises (no fallback) for shapes, dims or dtypes the kernels do not take."""
    _shape(s.dim() == 2 and v.dim() == 3, f"gcp2_fused: s {tuple(s.shape)} / v {tuple(v.shape)} must be [M, SI] / [M, VI, 3]")
    dims = (int(s.shape[1]), int(v.shape[1]), int(SO), int(VO), int(H), bool(feedforward_out), gcp2_act_code(act_scalar), gcp2_act_code(act_vector))
    weights = list(weights)
    record = torch.is_grad_enabled() and any(t.requires_grad for t in (s, v, *weights))
    return _GCP2Fused.apply(s, v, F, row_mask, dims, record, *weights)


# ---- the diffusion objective around the network evaluation (include/gcdm_objective.h) ----------------------------------------------------------
OBJECTIVE_TERMS = ("delta_log_px", "error_t", "SNR_weight", "loss_0_x", "loss_0_h", "neg_log_constants", "kl_prior", "log_pN", "eps_hat_x", "eps_hat_h")
OBJECTIVE_MEANS = ("loss", "loss_t", "SNR_weight", "loss_0", "kl_prior", "delta_log_px", "neg_log_const_0", "log_pN", "eps_hat_x", "eps_hat_h")


def objective_workspace_bytes(N: int, B: int, D: int, mode: int) -> int:
    n = int(_lib().gcdm_objective_workspace_bytes(int(N), int(B), int(D), int(mode)))
    if n < 0:
        raise ValueError(f"gcdm_objective_workspace_bytes({N}, {B}, {D}, {mode}): bad argument")
    return n


class ObjectiveState:
    """What gcdm_objective_prepare wrote for one batch (xh, eps_t, z_t, t_node, mol [B, 8]; eps_0, z_0 in evaluation mode) together with
    the inputs the later entries read again.  ``read_flags()`` copies the device flag word to the host (the one sync; call it when convenient),
    clears it and raises for what it says."""

    def read_flags(self) -> int:
        fl = int(self.flags.item())
        if fl:
            self.flags.zero_()
        if fl & _native.OBJECTIVE_FLAG_UNSORTED:
            raise ValueError("diffusion_objective: batch_index must be non-decreasing (molecules contiguous in node order)")
        if fl & _native.OBJECTIVE_FLAG_T_RANGE:
            raise ValueError(f"diffusion_objective: t_int outside 0 .. {self.T}")
        if fl & _native.OBJECTIVE_FLAG_EMPTY:
            raise ValueError("diffusion_objective: a molecule has no unmasked node")
        if fl & _native.OBJECTIVE_FLAG_SIZE:
            raise KeyError("diffusion_objective: a molecule's size is missing from the histogram of NumNodesDistribution (its log_pN is NaN)")
        return fl


def objective_prepare(x: torch.Tensor, one_hot: torch.Tensor, charges: Optional[torch.Tensor], mask: Optional[torch.Tensor],
                      batch_index: torch.Tensor, num_graphs: int, t_int: torch.Tensor, gamma: torch.Tensor, log_pn: torch.Tensor, norm_values,
                      norm_biases, eps_raw: torch.Tensor, eps_raw_0: Optional[torch.Tensor], num_atom_types: int, include_charges: bool, T: int,
                      mode: int, flags: torch.Tensor, center_x: bool = False) -> ObjectiveState:
    """Two launches: gcdm_op_rowptr (node_offsets from ``batch_index``) and gcdm_objective_prepare; plus one conversion launch when ``t_int``
    is not int32 already.  ``flags``: an int32 [1] device tensor the caller keeps (OR-ed into, read lazily with ``state.read_flags()``)."""
    nf, ic, B = int(num_atom_types), int(bool(include_charges)), int(num_graphs)
    D = 3 + nf + ic
    N = int(x.shape[0])
    _shape(x.dim() == 2 and x.shape[1] == 3 and N >= 1 and 1 <= B <= N, f"diffusion_objective: x {tuple(x.shape)} must be [N, 3] with 1 <= B = {B} <= N")
    _shape(1 <= nf <= _native.OBJECTIVE_MAX_TYPES and N * D < 2 ** 31, f"diffusion_objective: {nf} atom types (1 .. {_native.OBJECTIVE_MAX_TYPES}), N * D < 2^31")
    _shape(tuple(one_hot.shape) == (N, nf), f"diffusion_objective: one_hot {tuple(one_hot.shape)} must be [{N}, {nf}]")
    _shape(not ic or (charges is not None and charges.numel() == N), "diffusion_objective: charges must have one entry per node")
    _shape(batch_index.numel() == N and (mask is None or mask.numel() == N), "diffusion_objective: batch_index / mask must have one entry per node")
    _shape(t_int.numel() == B and gamma.numel() == int(T) + 1 and log_pn.numel() >= 1, "diffusion_objective: t_int [B], gamma [T + 1], log_pn")
    _shape(tuple(eps_raw.shape) == (N, D) and (eps_raw_0 is None or tuple(eps_raw_0.shape) == (N, D)), f"diffusion_objective: the raw draws must be [{N}, {D}]")
    _shape(mode in (0, 1, 2) and (mode != _native.OBJECTIVE_EVAL or eps_raw_0 is not None), "diffusion_objective: mode / second draw")
    _shape(flags.dtype == torch.int32 and flags.numel() == 1, "diffusion_objective: flags must be int32 [1]")
    st = ObjectiveState()
    xs, oh, er = _f(x), _f(one_hot), _f(eps_raw)
    for t in (batch_index, t_int, gamma, log_pn, flags):
        _dev(t)
    ch = _f(charges).reshape(-1) if ic else None
    e0 = _f(eps_raw_0) if mode == _native.OBJECTIVE_EVAL else None
    bi = batch_index.reshape(-1).to(torch.int64).contiguous()
    mk = None
    if mask is not None:
        _dev(mask)
        mk = mask.reshape(-1).contiguous()
        mk = mk.view(torch.uint8) if mk.dtype == torch.bool else mk.ne(0).view(torch.uint8)
    ti = t_int.reshape(-1).to(torch.int32).contiguous()            # the conversion launch (torch.randint draws int64)
    dev = xs.device
    off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    _chk(_lib().gcdm_op_rowptr(_p(bi), N, B, _p(off), _p(flags), _st(xs)), "gcdm_op_rowptr")
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)          # noqa: E731
    st.xh, st.eps_t, st.z_t, st.t_node, st.mol = new(N, D), new(N, D), new(N, D), new(N), new(B, 8)
    st.eps_0, st.z_0 = (new(N, D), new(N, D)) if e0 is not None else (None, None)
    st.nv, st.nb = (C.c_float * 3)(*[float(v) for v in norm_values]), (C.c_float * 3)(*[float(v) for v in norm_biases])
    st.gamma, st.log_pn = _f(gamma).reshape(-1), _f(log_pn).reshape(-1)
    _chk(_lib().gcdm_objective_prepare(_p(xs), _p(oh), _p(ch), _p(mk), _p(off), _p(ti), _p(st.gamma), _p(st.log_pn), st.log_pn.numel(), st.nv, st.nb,
                                       _p(er), _p(e0), _p(st.xh), _p(st.eps_t), _p(st.z_t), _p(st.eps_0), _p(st.z_0), _p(st.t_node), _p(st.mol),
                                       _p(flags), N, B, nf, ic, int(T), int(mode), int(bool(center_x)), _st(xs)), "gcdm_objective_prepare")
    st.off, st.mask, st.flags, st.t_int = off, mk, flags, ti
    st.N, st.B, st.D, st.nf, st.ic, st.T, st.mode = N, B, D, nf, ic, int(T), int(mode)
    st.keep = (xs, oh, ch, er, e0, bi)
    return st


class _DiffusionObjective(torch.autograd.Function):
    """gcdm_objective_terms + gcdm_objective_reduce forward, gcdm_objective_bwd backward; the only differentiable input is net_out."""

    @staticmethod
    def forward(ctx, net_out, st, net_out_0, norm_by_max_nodes):
        N, B, D = st.N, st.B, st.D
        _shape(tuple(net_out.shape) == (N, D) and (net_out_0 is None or tuple(net_out_0.shape) == (N, D)), f"diffusion_objective: net_out must be [{N}, {D}]")
        _shape(st.mode != _native.OBJECTIVE_EVAL or net_out_0 is not None, "diffusion_objective: evaluation mode needs net_out_0")
        no = _f(net_out)
        n0 = _f(net_out_0) if st.mode == _native.OBJECTIVE_EVAL else None
        dev = no.device
        terms = torch.empty((B, 10), dtype=torch.float32, device=dev)
        nll = torch.empty(B, dtype=torch.float32, device=dev)
        means = torch.empty(16, dtype=torch.float32, device=dev)
        ws = torch.empty(objective_workspace_bytes(N, B, D, st.mode), dtype=torch.uint8, device=dev)
        _chk(_lib().gcdm_objective_terms(_p(no), _p(n0), _p(st.xh), _p(st.eps_t), _p(st.z_t), _p(st.eps_0), _p(st.z_0), _p(st.mask), _p(st.off),
                                         _p(st.mol), _p(st.gamma), st.nv, st.nb, _p(terms), N, B, st.nf, st.ic, st.T, st.mode, _st(no)),
             "gcdm_objective_terms")
        _chk(_lib().gcdm_objective_reduce(_p(st.mol), _p(terms), _p(ws), _p(nll), _p(means), B, D, st.T, st.mode, int(bool(norm_by_max_nodes)), _st(no)),
             "gcdm_objective_reduce")
        ctx.st, ctx.no, ctx.ws = st, no, ws
        ctx.set_materialize_grads(False)
        st.terms_block, st.means_block = terms, means            # the columns without a gradient are read from here
        return terms[:, 1], terms[:, 3], nll, means[0]

    @staticmethod
    def backward(ctx, g_err, g_l0x, g_nll, g_loss):
        if torch.is_grad_enabled():
            raise RuntimeError("diffusion_objective (fused objective path): double backward (create_graph=True) is not supported; use the operator path")
        st = ctx.st
        if st.mode == _native.OBJECTIVE_EVAL:
            raise RuntimeError("diffusion_objective: the evaluation-mode objective has no backward")
        if not ctx.needs_input_grad[0]:
            return None, None, None, None

        def vec(g):
            if g is None:
                return None, 0
            g = g.detach()
            if g.dtype != torch.float32 or g.dim() != 1 or g.stride(0) < 0:
                g = g.to(torch.float32).reshape(-1).contiguous()
            return g, int(g.stride(0))

        (ge, se), (g0, s0), (gn, sn) = vec(g_err), vec(g_l0x), vec(g_nll)
        gl = None if g_loss is None else g_loss.detach().to(torch.float32).reshape(1)
        d = torch.empty((st.N, st.D), dtype=torch.float32, device=ctx.no.device)
        _chk(_lib().gcdm_objective_bwd(_p(ge), se, _p(g0), s0, _p(gn), sn, _p(gl), _p(ctx.no), _p(st.eps_t), _p(st.mask), _p(st.off), _p(st.mol),
                                       _p(ctx.ws), _p(d), st.N, st.B, st.D, st.mode, _st(d)), "gcdm_objective_bwd")
        return d, None, None, None


def diffusion_objective(net_out: torch.Tensor, state: ObjectiveState, net_out_0: Optional[torch.Tensor] = None, norm_by_max_nodes: bool = False):
    """The loss terms of one batch from the network's output as one autograd node (two launches forward, one backward; d net_out is the only
    gradient).  -> (terms, nll [B], loss, means): ``terms`` maps OBJECTIVE_TERMS to [B] tensors (error_t and loss_0_x carry the graph),
    ``loss`` = mean(nll) carries it too, ``means`` maps OBJECTIVE_MEANS to detached scalars (the batch means ``loss_info`` reports)."""
    error_t, loss_0_x, nll, loss = _DiffusionObjective.apply(net_out, state, net_out_0, bool(norm_by_max_nodes))
    tb, mb = state.terms_block, state.means_block
    terms = {k: tb[:, i] for i, k in enumerate(OBJECTIVE_TERMS)}
    terms["error_t"], terms["loss_0_x"] = error_t, loss_0_x
    return terms, nll, loss, {k: mb[i] for i, k in enumerate(OBJECTIVE_MEANS)}


# ---- the classifier's column-split first edge layer (include/gcdm_classifier_train.h) ------------------------------------------------------------
class MoleculeEdges:
    """The classifier's edge set from the molecule sizes alone: the ordered pairs i != j of each molecule, row-major.  Holds the three device
    tables gcdm_classifier_train_edge_pre_* read (node_mol [N], node_offsets [B + 1] int32, edge_offsets [B + 1] int64) and, made on first
    use, the two ``Graph`` views the other operators take: ``graph`` (nodes x edges, with its column order in closed form -- nothing is
    sorted) and ``pool`` (molecules x nodes, for the per-molecule sum).  ``sizes`` is read on the host: E and N size the buffers."""

    def __init__(self, sizes, device):
        n = torch.as_tensor(sizes).detach().to("cpu", torch.int64).reshape(-1)
        _shape(bool((n >= 0).all()), f"MoleculeEdges: molecule sizes must be counts >= 0, got {n.tolist()}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("bio-diffusion_amd operators run on an MI355X only: MoleculeEdges needs a HIP ('cuda') device; there is no CPU fallback")
        self.sizes, self.device = [int(v) for v in n], dev
        self.B, self.N, self.E = int(n.numel()), int(n.sum()), int((n * (n - 1)).clamp(min=0).sum())
        _shape(self.N < 2 ** 31 - 1, f"MoleculeEdges: {self.N} nodes")
        noff = torch.zeros(self.B + 1, dtype=torch.int64)
        noff[1:] = torch.cumsum(n, 0)
        eoff = torch.zeros(self.B + 1, dtype=torch.int64)
        eoff[1:] = torch.cumsum((n * (n - 1)).clamp(min=0), 0)
        self.node_offsets = noff.to(torch.int32).to(dev)
        self.edge_offsets = eoff.to(dev)
        self._n = n.to(dev)
        self.node_mol = torch.repeat_interleave(torch.arange(self.B, device=dev), self._n, output_size=self.N).to(torch.int32)
        self._graph = self._pool = None

    @property
    def graph(self) -> Graph:
        if self._graph is None:
            dev, N, E = self.device, self.N, self.E
            mol = self.node_mol.to(torch.int64)
            n_of, o_of, eo_of = self._n[mol], self.node_offsets.to(torch.int64)[mol], self.edge_offsets[mol]      # per node: its molecule's
            deg = (n_of - 1).clamp(min=0)
            rowptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
            rowptr[1:] = torch.cumsum(deg, 0)
            node = torch.repeat_interleave(torch.arange(N, device=dev), deg, output_size=E)      # the row of edge e; also the column of slot e
            k = torch.arange(E, device=dev) - rowptr[node]                                      # position among the node's n - 1 partners
            li = node - o_of[node]
            other = k + (k >= li).to(torch.int64)                                               # the partner's local index, ascending
            ei = torch.stack([node, o_of[node] + other]).contiguous()
            # slot e of the column order is the edge (other, li) of the node's molecule: the block walked with stride n - 1
            colperm = (eo_of[node] + other * (n_of[node] - 1) + li - (li > other).to(torch.int64)).contiguous()
            ptr = rowptr.to(torch.int32)
            self._graph = Graph.from_parts(ei, N, ptr, colperm, ptr.clone())
        return self._graph

    @property
    def pool(self) -> Graph:
        if self._pool is None:
            mol = self.node_mol.to(torch.int64)
            ei = torch.stack([mol, mol]).contiguous()
            self._pool = Graph.from_parts(ei, self.B, self.node_offsets, torch.arange(self.N, device=self.device), self.node_offsets.clone())
        return self._pool


class _ClassifierEdgePre(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, x, w_r, edges):
        N, E = edges.N, edges.E
        _shape(A.dim() == 2 and A.shape[0] == N and A.shape[1] >= 1 and tuple(B.shape) == tuple(A.shape),
               f"classifier_edge_pre: A {tuple(A.shape)} and B {tuple(B.shape)} must both be [{N}, H]")
        H = int(A.shape[1])
        _shape(H <= _native.CLASSIFIER_TRAIN_MAX_H, f"classifier_edge_pre: H = {H} > {_native.CLASSIFIER_TRAIN_MAX_H}")
        _shape(tuple(x.shape) == (N, 3), f"classifier_edge_pre: x {tuple(x.shape)} must be [{N}, 3]")
        _shape(w_r.numel() == H, f"classifier_edge_pre: w_r {tuple(w_r.shape)} must hold {H} entries")
        As, Bs, xs, ws = _f(A), _f(B), _f(x), _f(w_r).reshape(-1)
        pre = torch.empty((E, H), dtype=torch.float32, device=As.device)
        radial = torch.empty(E, dtype=torch.float32, device=As.device)
        _chk(_lib().gcdm_classifier_train_edge_pre_fwd(_p(As), _p(Bs), _p(xs), _p(ws), _p(edges.node_mol), _p(edges.node_offsets), _p(edges.edge_offsets),
                                                       _p(pre), _p(radial), N, edges.B, E, H, _st(As)), "gcdm_classifier_train_edge_pre_fwd")
        ctx.edges, ctx.radial, ctx.H, ctx.w_shape = edges, radial, H, w_r.shape
        return pre

    @staticmethod
    def backward(ctx, dpre):
        edges, H = ctx.edges, ctx.H
        N, E = edges.N, edges.E
        g = _f(dpre).reshape(E, H)
        alloc = torch.zeros if E == 0 else torch.empty          # no edges: the library writes nothing, the sums are zero
        dA, dB = alloc((N, H), dtype=torch.float32, device=g.device), alloc((N, H), dtype=torch.float32, device=g.device)
        dw = alloc(H, dtype=torch.float32, device=g.device)
        nbytes = int(_lib().gcdm_classifier_train_workspace_bytes(E, H))
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=g.device) if nbytes > 0 else None
        _chk(_lib().gcdm_classifier_train_edge_pre_bwd(_p(g), _p(ctx.radial), _p(edges.node_mol), _p(edges.node_offsets), _p(edges.edge_offsets), _p(dA),
                                                       _p(dB), _p(dw), _p(ws), N, edges.B, E, H, _st(g)), "gcdm_classifier_train_edge_pre_bwd")
        need = ctx.needs_input_grad
        return (dA if need[0] else None), (dB if need[1] else None), None, (dw.reshape(ctx.w_shape) if need[3] else None), None


def classifier_edge_pre(A: torch.Tensor, B: torch.Tensor, x: torch.Tensor, w_r: torch.Tensor, edges: MoleculeEdges) -> torch.Tensor:
    """The classifier's first per-edge layer with its weight split by columns, W = [W_s | W_t | w_r]: with A = linear(h, W_s, b) and
    B = linear(h, W_t), ``pre[(i, j)] = A[i] + B[j] + |x_i - x_j|^2 w_r`` over the ordered pairs i != j of each molecule [E, H].  The radial
    is computed in the same kernel.  Gradients to A, B and w_r (fixed summation order, no atomics); none to x: positions are data."""
    return _ClassifierEdgePre.apply(A, B, x, w_r, edges)


# ---- the per-edge block of an EGNN dynamics layer (include/gcdm_egnn_train.h) -----------------------------------------------------------------
def egnn_edge_block_why_not(H: int, Eh: int, e_in: int) -> Optional[str]:
    """None when the kernels of include/gcdm_egnn_train.h serve these widths, else the reason."""
    if H < 32 or H % 32 or H > _native.EGNN_DYN_MAX_H:
        return f"h_hidden_dim = {H}: the fused edge block takes a multiple of 32 up to {_native.EGNN_DYN_MAX_H}"
    if Eh < 1 or Eh > _native.EGNN_DYN_MAX_EH:
        return f"e_hidden_dim = {Eh}: the fused edge block takes 1 .. {_native.EGNN_DYN_MAX_EH}"
    if e_in not in (1, 2):
        return f"e_in = {e_in}: the fused edge block takes 1 or 2 edge input scalars"
    return None


def _egnn_err(what: str) -> "_native.NativeError":
    return _native.NativeError(f"{what} failed: {_lib().gcdm_egnn_train_last_error().decode()}")


class _EgnnEdgeBlock(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, V, W2, b2, C1, c1b, c2, c2b, scale, x, x0, xsc, node_offsets, node_mol, H, Eh):
        N, K = int(A.shape[0]) if A.dim() == 2 else -1, 2 * (2 * H + Eh + 1)
        e_in = 1 if xsc is None else 2
        why = egnn_edge_block_why_not(H, Eh, e_in)
        _shape(why is None, f"egnn_edge_block: {why}")
        _shape(tuple(A.shape) == (N, K) and tuple(B.shape) == (N, K), f"egnn_edge_block: A {tuple(A.shape)} and B {tuple(B.shape)} must both be [N, {K}]")
        _shape(tuple(V.shape) == (3, K) and tuple(W2.shape) == (_native.EGNN_DYN_M_DIM, K) and b2.numel() == _native.EGNN_DYN_M_DIM,
               f"egnn_edge_block: V {tuple(V.shape)}, W2 {tuple(W2.shape)}, b2 {tuple(b2.shape)} must be [3, {K}], [16, {K}], [16]")
        CHn, MDn = _native.EGNN_DYN_COORS_HIDDEN, _native.EGNN_DYN_M_DIM
        _shape(tuple(C1.shape) == (CHn, MDn) and c1b.numel() == CHn and c2.numel() == CHn and c2b.numel() == 1 and scale.numel() == 1,
               "egnn_edge_block: C1 [64, 16], c1b [64], c2 [64], c2b [1], scale [1]")
        _shape(tuple(x.shape) == (N, 3) and tuple(x0.shape) == (N, 3) and (xsc is None or tuple(xsc.shape) == (N, 3)),
               f"egnn_edge_block: x, x0 (and xsc) must be [{N}, 3]")
        _shape(node_mol.dtype == torch.int32 and node_offsets.dtype == torch.int32 and node_mol.numel() == N and node_offsets.numel() >= 1,
               "egnn_edge_block: node_offsets int32 [B + 1], node_mol int32 [N]")
        ts = [_f(t) for t in (A, B, V, W2, b2, C1, c1b, c2, c2b, scale, x, x0)]
        xs = None if xsc is None else _f(xsc)
        nB = int(node_offsets.numel()) - 1
        M = torch.zeros((N, MDn), dtype=torch.float32, device=ts[0].device)
        dx = torch.zeros((N, 3), dtype=torch.float32, device=ts[0].device)
        st = _lib().gcdm_egnn_train_edge_fwd(*[_p(t) for t in ts], _p(xs), _p(node_offsets), _p(node_mol), _p(M), _p(dx), N, nB, H, Eh, e_in, _st(ts[0]))
        if st != 0:
            raise _egnn_err("gcdm_egnn_train_edge_fwd")
        ctx.save_for_backward(*ts, *([] if xs is None else [xs]), node_offsets, node_mol)        # its inputs only: nothing per edge is kept
        ctx.dims, ctx.shapes = (N, nB, H, Eh, e_in, K), [t.shape for t in (A, B, V, W2, b2, C1, c1b, c2, c2b, scale, x)]
        return M, dx

    @staticmethod
    def backward(ctx, gM, gdx):
        N, nB, H, Eh, e_in, K = ctx.dims
        saved = ctx.saved_tensors
        ts, xs = saved[:12], (saved[12] if e_in == 2 else None)
        node_offsets, node_mol = saved[-2], saved[-1]
        dev = ts[0].device
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        CHn, MDn = _native.EGNN_DYN_COORS_HIDDEN, _native.EGNN_DYN_M_DIM
        outs = [new(N, K), new(N, K), new(N, 3), new(3, K), new(MDn, K), new(MDn), new(CHn, MDn), new(CHn), new(CHn), new(1), new(1)]
        nbytes = int(_lib().gcdm_egnn_train_workspace_bytes(N, H, Eh, e_in))
        if nbytes < 0:
            raise _egnn_err("gcdm_egnn_train_workspace_bytes")
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        st = _lib().gcdm_egnn_train_edge_bwd(*[_p(t) for t in ts], _p(xs), _p(node_offsets), _p(node_mol), _p(_f(gM)), _p(_f(gdx)), _p(ws),
                                             *[_p(t) for t in outs], N, nB, H, Eh, e_in, _st(ts[0]))
        if st != 0:
            raise _egnn_err("gcdm_egnn_train_edge_bwd")
        gA, gB, gx, gV, gW2, gb2, gC1, gc1b, gc2, gc2b, gscale = outs
        order = [gA, gB, gV, gW2, gb2, gC1, gc1b, gc2, gc2b, gscale, gx]
        need = ctx.needs_input_grad
        grads = [(g.reshape(s) if need[k] else None) for k, (g, s) in enumerate(zip(order, ctx.shapes))]
        return (*grads, None, None, None, None, None, None)


def egnn_edge_block(A: torch.Tensor, B: torch.Tensor, V: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor, C1: torch.Tensor, c1b: torch.Tensor,
                    c2: torch.Tensor, c2b: torch.Tensor, scale: torch.Tensor, x: torch.Tensor, x0: torch.Tensor, xsc: Optional[torch.Tensor],
                    node_offsets: torch.Tensor, node_mol: torch.Tensor, H: int, Eh: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Everything of an EGNN dynamics layer that is per edge, as one operator over the fully connected edges of each molecule (the diagonal
    included), none of which is materialised: with A = linear(h, W_i, b1 + W_e b_emb), B = linear(h, W_j) [N, K], V = (u, u', w_r) [3, K],
    ``z1 = A_i + B_j + r0 u + r0sc u' + r w_r``, ``m = silu(W2 silu(z1) + b2)``, ``w = tanh(c2 . silu(C1 m + c1b) + c2b)`` ->
    (sum_j m_ij [N, 16], sum_j w_ij (x_j - x_i) / max(|x_j - x_i|, 1e-8) scale [N, 3]).  Differentiable in A, B, V, W2, b2, C1, c1b, c2, c2b,
    scale and x (x0 and xsc are data); the backward recomputes every edge, saves only its inputs, uses no float atomics and never forms the
    diagonal's cancelling pair in the gradient of x (include/gcdm_egnn_train.h).  ``xsc`` is None with one edge input scalar."""
    return _EgnnEdgeBlock.apply(A, B, V, W2, b2, C1, c1b, c2, c2b, scale, x, x0, xsc, node_offsets, node_mol, int(H), int(Eh))
