"""Argument checks of the module-level operators, without a GPU.

* The C ABI of libgcdm_ops.so (include/gcdm_ops.h): every entry returns -1 for a bad argument BEFORE any HIP call, and 0 without a
  launch for empty work.  All pointers here are null, so a call that got past its checks would launch a kernel on nothing.  These tests
  carry no gpu mark and also run on GPU machines, so the `lib` fixture keeps them away from a library without the checks (where such a
  launch would fault the card): it skips unless the library is at least as new as its sources (the rule native.build_ops() rebuilds by),
  and it then probes the library with gcdm_op_act(kind = 9, n = 0) -- a call that returns 0 before any launch in a library without the
  checks, and -1 in one with them -- and errors out unless the answer is -1.  No case runs before both have passed.
* ops.py: every shape check raises ValueError (IndexError for an index out of range) before the device check, so host tensors reach it.
"""
import ctypes
import importlib
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
pkg = importlib.import_module("bio-diffusion_amd")
ops = pkg.ops
native = pkg._native

NULL = None


@pytest.fixture(scope="module")
def lib():
    path = native.OPS_LIB_PATH
    if not os.path.exists(path):
        pytest.skip("libgcdm_ops.so not built (run __graft_entry__.build())")
    stale = [d for d in native.OPS_SOURCES + native.OPS_HEADERS if os.path.getmtime(d) > os.path.getmtime(path)]
    if stale:
        pytest.skip(f"libgcdm_ops.so is older than {stale} (run __graft_entry__.build()): it may lack the argument checks under test")
    lib = ctypes.CDLL(path)
    for name, sig in native.OPS_SIGNATURES.items():
        getattr(lib, name).argtypes = sig
        getattr(lib, name).restype = ctypes.c_int
    # launch-free in every version of the library: without the checks, n = 0 returns 0 before the kind is looked at
    status = lib.gcdm_op_act(9, None, None, 0, None)
    if status != -1:
        pytest.fail(f"{path} accepts kind = 9 (status {status}): it lacks the argument checks, so the null-pointer cases would launch")
    return lib


# (entry, args with null pointers) -> expected status.  -1: refused; 0: empty work, no launch.
def _cases():
    Z = NULL
    c = []
    # gemm(A, sam, sak, B, sbk, sbn, C, bias, M, N, K, slices, stream)
    c += [("gcdm_op_gemm", (Z, 1, 1, Z, 1, 1, Z, Z, -1, 4, 4, 1, Z), -1), ("gcdm_op_gemm", (Z, 1, 1, Z, 1, 1, Z, Z, 4, -1, 4, 1, Z), -1),
          ("gcdm_op_gemm", (Z, 1, 1, Z, 1, 1, Z, Z, 4, 4, -1, 1, Z), -1), ("gcdm_op_gemm", (Z, 1, 1, Z, 1, 1, Z, Z, 4, 4, 4, 0, Z), -1),
          ("gcdm_op_gemm", (Z, 1, 1, Z, 1, 1, Z, Z, 4, 4, 4, -3, Z), -1), ("gcdm_op_gemm", (Z, 1, 1, Z, 1, 1, Z, Z, 4, 4, 4, 1, Z), -1),
          ("gcdm_op_gemm", (Z, 1, 1, Z, 1, 1, Z, Z, 0, 4, 4, 1, Z), 0), ("gcdm_op_gemm", (Z, 1, 1, Z, 1, 1, Z, Z, 4, 0, 4, 2, Z), 0),
          ("gcdm_op_gemm", (Z, 1, 1, Z, 1, 1, Z, Z, 0, 4, 4, 0, Z), -1)]
    c += [("gcdm_op_reduce_slices", (Z, Z, -1, 1, Z), -1), ("gcdm_op_reduce_slices", (Z, Z, 4, 0, Z), -1),
          ("gcdm_op_reduce_slices", (Z, Z, 4, 2, Z), -1), ("gcdm_op_reduce_slices", (Z, Z, 0, 2, Z), 0)]
    c += [("gcdm_op_colsum", (Z, Z, -1, 4, Z), -1), ("gcdm_op_colsum", (Z, Z, 4, -1, Z), -1), ("gcdm_op_colsum", (Z, Z, 4, 4, Z), -1),
          ("gcdm_op_colsum", (Z, Z, 0, 4, Z), -1), ("gcdm_op_colsum", (Z, Z, 4, 0, Z), 0)]
    c += [("gcdm_op_colsum_slices", (Z, Z, -1, 4, 2, Z), -1), ("gcdm_op_colsum_slices", (Z, Z, 4, -1, 2, Z), -1),
          ("gcdm_op_colsum_slices", (Z, Z, 4, 4, 0, Z), -1), ("gcdm_op_colsum_slices", (Z, Z, 4, 4, 2, Z), -1),
          ("gcdm_op_colsum_slices", (Z, Z, 4, 0, 2, Z), 0)]
    for kind in (-1, 6, 99):
        c += [("gcdm_op_act", (kind, Z, Z, 4, Z), -1), ("gcdm_op_act", (kind, Z, Z, 0, Z), -1),
              ("gcdm_op_act_bwd", (kind, Z, Z, Z, 4, Z), -1), ("gcdm_op_act_bwd", (kind, Z, Z, Z, 0, Z), -1)]
    c += [("gcdm_op_act", (1, Z, Z, -1, Z), -1), ("gcdm_op_act", (1, Z, Z, 4, Z), -1), ("gcdm_op_act", (5, Z, Z, 0, Z), 0),
          ("gcdm_op_act_bwd", (1, Z, Z, Z, -1, Z), -1), ("gcdm_op_act_bwd", (2, Z, Z, Z, 4, Z), -1), ("gcdm_op_act_bwd", (0, Z, Z, Z, 0, Z), 0)]
    # the issue's example: M * C = 5 > 0 from two negative sizes
    c += [("gcdm_op_norm3", (Z, Z, -1, -5, 0, Z), -1), ("gcdm_op_norm3", (Z, Z, -1, 4, 1, Z), -1), ("gcdm_op_norm3", (Z, Z, 4, 4, 2, Z), -1),
          ("gcdm_op_norm3", (Z, Z, 0, 4, -1, Z), -1), ("gcdm_op_norm3", (Z, Z, 4, 4, 1, Z), -1), ("gcdm_op_norm3", (Z, Z, 0, 4, 1, Z), 0),
          ("gcdm_op_norm3_bwd", (Z, Z, Z, Z, -1, -5, 1, Z), -1), ("gcdm_op_norm3_bwd", (Z, Z, Z, Z, 4, 4, 3, Z), -1),
          ("gcdm_op_norm3_bwd", (Z, Z, Z, Z, 4, 4, 0, Z), -1), ("gcdm_op_norm3_bwd", (Z, Z, Z, Z, 4, 0, 0, Z), 0)]
    for name in ("gcdm_op_scalarize", "gcdm_op_scalarize_bwd", "gcdm_op_vectorize", "gcdm_op_vectorize_bwd", "gcdm_op_rowscale",
                 "gcdm_op_gather", "gcdm_op_scatter_add"):
        c += [(name, (Z, Z, Z, -1, -5, Z), -1), (name, (Z, Z, Z, -1, 4, Z), -1), (name, (Z, Z, Z, 4, -1, Z), -1),
              (name, (Z, Z, Z, 4, 4, Z), -1), (name, (Z, Z, Z, 0, 4, Z), 0), (name, (Z, Z, Z, 4, 0, Z), 0)]
    c += [("gcdm_op_rowscale_bwd", (Z, Z, Z, Z, Z, -1, -5, Z), -1), ("gcdm_op_rowscale_bwd", (Z, Z, Z, Z, Z, 4, 4, Z), -1),
          ("gcdm_op_rowscale_bwd", (Z, Z, Z, Z, Z, 0, 4, Z), 0)]
    # rowptr(row, E, N, rowptr, flag): never empty (N + 1 entries)
    c += [("gcdm_op_rowptr", (Z, -1, 4, Z, Z, Z), -1), ("gcdm_op_rowptr", (Z, 4, -1, Z, Z, Z), -1), ("gcdm_op_rowptr", (Z, 0, 0, Z, Z, Z), -1),
          ("gcdm_op_rowptr", (Z, 4, 4, Z, Z, Z), -1)]
    c += [("gcdm_op_segment_sum", (Z, Z, Z, -1, 4, 0, Z), -1), ("gcdm_op_segment_sum", (Z, Z, Z, 4, -1, 0, Z), -1),
          ("gcdm_op_segment_sum", (Z, Z, Z, 4, 4, 2, Z), -1), ("gcdm_op_segment_sum", (Z, Z, Z, 0, 4, -1, Z), -1),
          ("gcdm_op_segment_sum", (Z, Z, Z, 4, 4, 1, Z), -1), ("gcdm_op_segment_sum", (Z, Z, Z, 0, 4, 1, Z), 0),
          ("gcdm_op_segment_bwd", (Z, Z, Z, Z, -1, 4, 0, Z), -1), ("gcdm_op_segment_bwd", (Z, Z, Z, Z, 4, -1, 0, Z), -1),
          ("gcdm_op_segment_bwd", (Z, Z, Z, Z, 4, 4, 2, Z), -1), ("gcdm_op_segment_bwd", (Z, Z, Z, Z, 4, 4, 0, Z), -1),
          ("gcdm_op_segment_bwd", (Z, Z, Z, Z, 4, 0, 1, Z), 0)]
    c += [("gcdm_op_localize", (Z, Z, Z, Z, -1, 1, Z), -1), ("gcdm_op_localize", (Z, Z, Z, Z, 4, 2, Z), -1),
          ("gcdm_op_localize", (Z, Z, Z, Z, 0, -1, Z), -1), ("gcdm_op_localize", (Z, Z, Z, Z, 4, 1, Z), -1),
          ("gcdm_op_localize", (Z, Z, Z, Z, 0, 0, Z), 0),
          ("gcdm_op_edge_features", (Z, Z, Z, Z, Z, -1, Z), -1), ("gcdm_op_edge_features", (Z, Z, Z, Z, Z, 4, Z), -1),
          ("gcdm_op_edge_features", (Z, Z, Z, Z, Z, 0, Z), 0),
          ("gcdm_op_orientations", (Z, Z, -1, Z), -1), ("gcdm_op_orientations", (Z, Z, 4, Z), -1), ("gcdm_op_orientations", (Z, Z, 0, Z), 0),
          ("gcdm_op_centralize", (Z, Z, Z, Z, -1, 3, Z), -1), ("gcdm_op_centralize", (Z, Z, Z, Z, 4, -1, Z), -1),
          ("gcdm_op_centralize", (Z, Z, Z, Z, 4, 3, Z), -1), ("gcdm_op_centralize", (Z, Z, Z, Z, 0, 3, Z), 0),
          ("gcdm_op_fc_edges", (Z, Z, -1, Z, Z, 4, Z), -1), ("gcdm_op_fc_edges", (Z, Z, 2, Z, Z, -1, Z), -1),
          ("gcdm_op_fc_edges", (Z, Z, 0, Z, Z, 4, Z), -1), ("gcdm_op_fc_edges", (Z, Z, 2, Z, Z, 4, Z), -1),
          ("gcdm_op_fc_edges", (Z, Z, 0, Z, Z, 0, Z), 0), ("gcdm_op_fc_edges", (Z, Z, 3, Z, Z, 0, Z), 0)]
    return c


CASES = _cases()


@pytest.mark.parametrize("name,args,want", CASES, ids=[f"{n[8:]}-{i}" for i, (n, _, _) in enumerate(CASES)])
def test_ops_cabi_refuses_bad_arguments_before_any_hip_call(lib, name, args, want):
    assert getattr(lib, name)(*args) == want


def test_ops_cabi_rejection_cases_cover_every_entry():
    assert {n for n, _, _ in CASES} == set(native.OPS_EXPORTS)


# ---- ops.py: shapes are checked on the host, before the device check ----------------------------------------------------------------------
def _z(*shape):
    return torch.zeros(*shape)


def _graph(N, E):
    """Stands in for ops.Graph (which needs a device) where only its sizes are read before the device check."""
    return types.SimpleNamespace(N=N, E=E)


BAD_SHAPES = {
    "linear_K_mismatch": lambda: ops.linear(_z(2, 5, 4), _z(3, 3)),            # K1 > K2: would read past the end of W
    "linear_K_smaller": lambda: ops.linear(_z(2, 3), _z(3, 4)),
    "linear_weight_1d": lambda: ops.linear(_z(2, 3), _z(3)),
    "linear_bias_len": lambda: ops.linear(_z(2, 3), _z(4, 3), _z(5)),
    "linear_bias_2d": lambda: ops.linear(_z(2, 3), _z(4, 3), _z(1, 4)),
    "safe_norm_pre_axis": lambda: ops.safe_norm_pre(_z(4, 2, 5)),
    "safe_norm_rep_axis": lambda: ops.safe_norm_rep(_z(4, 5, 2)),
    "safe_norm_rank": lambda: ops.safe_norm_rep(_z(4, 3)),
    "scalarize_frames_rows": lambda: ops.scalarize(_z(4, 3, 2), _z(5, 3, 3)),
    "scalarize_frames_short": lambda: ops.scalarize(_z(4, 3, 2), _z(4, 3, 2)),
    "scalarize_u_layout": lambda: ops.scalarize(_z(4, 2, 3), _z(4, 3, 3)),
    "vectorize_frames_rows": lambda: ops.vectorize(_z(4, 6), _z(3, 3, 3)),
    "vectorize_gate_width": lambda: ops.vectorize(_z(4, 7), _z(4, 3, 3)),
    "rowscale_gate_numel": lambda: ops.rowscale(_z(4, 5, 3), _z(4, 4)),
    "rowscale_gate_rows": lambda: ops.rowscale(_z(4, 5, 3), _z(5, 4)),
    "rowscale_vector_axis": lambda: ops.rowscale(_z(4, 5, 2), _z(4, 5)),
    "gather_row_nodes": lambda: ops.gather_row(_z(6, 3), _graph(5, 9)),
    "gather_col_nodes": lambda: ops.gather_col(_z(4, 3, 3), _graph(5, 9)),
    "scatter_rows_edges": lambda: ops.scatter_rows(_z(8, 3), _graph(5, 9)),
    "scatter_rows_mean_edges": lambda: ops.scatter_rows(_z(10, 3), _graph(5, 9), "mean"),
    "mean_frames_edges": lambda: ops.mean_frames(_z(8, 3, 3), _graph(5, 9)),
    "mean_frames_mask": lambda: ops.mean_frames(_z(9, 3, 3), _graph(5, 9), torch.ones(8, dtype=torch.bool)),
    "graph_edge_index_rank": lambda: ops.Graph(torch.zeros(6, dtype=torch.int64), 3),
    "graph_edge_index_rows": lambda: ops.Graph(torch.zeros(3, 4, dtype=torch.int64), 3),
    "graph_num_nodes": lambda: ops.Graph(torch.zeros(2, 0, dtype=torch.int64), -1),
    "embedding_table_rank": lambda: ops.embedding(_z(5), torch.zeros(3, dtype=torch.int64)),
    "localize_positions": lambda: ops.localize(_z(4, 2), torch.zeros(2, 3, dtype=torch.int64)),
    "localize_edge_index": lambda: ops.localize(_z(4, 3), torch.zeros(3, dtype=torch.int64)),
    "localize_edge_index_rows": lambda: ops.localize(_z(4, 3), torch.zeros(3, 2, dtype=torch.int64)),
    "edge_features_positions": lambda: ops.edge_features(_z(4, 4), torch.zeros(2, 3, dtype=torch.int64)),
    "orientations_positions": lambda: ops.orientations(_z(4, 3, 1)),
    "centralize_batch_index": lambda: ops.centralize(_z(4, 3), torch.zeros(5, dtype=torch.int64)),
    "centralize_mask": lambda: ops.centralize(_z(4, 3), torch.zeros(4, dtype=torch.int64), torch.ones(3, dtype=torch.bool)),
    "centralize_rank": lambda: ops.centralize(_z(4), torch.zeros(4, dtype=torch.int64)),
    "fc_edges_negative_size": lambda: ops.fully_connected_edge_index(torch.tensor([3, -1, 2]), "cpu"),
}


@pytest.mark.parametrize("case", sorted(BAD_SHAPES))
def test_ops_shape_checks_raise_before_the_device_check(case):
    with pytest.raises(ValueError):
        BAD_SHAPES[case]()


BAD_INDICES = {
    "graph_row_negative": lambda: ops.Graph(torch.tensor([[-1, 0, 1], [0, 1, 2]]), 3),
    "graph_row_too_large": lambda: ops.Graph(torch.tensor([[0, 1, 3], [0, 1, 2]]), 3),
    "graph_col_too_large": lambda: ops.Graph(torch.tensor([[0, 1, 2], [0, 3, 2]]), 3),
    "graph_col_negative": lambda: ops.Graph(torch.tensor([[0, 1, 2], [0, -2, 2]]), 3),
    "graph_no_nodes": lambda: ops.Graph(torch.tensor([[0], [0]]), 0),
    "embedding_too_large": lambda: ops.embedding(_z(5, 2), torch.tensor([0, 5])),
    "embedding_negative": lambda: ops.embedding(_z(5, 2), torch.tensor([[-1, 0]])),
    "localize_col_too_large": lambda: ops.localize(_z(4, 3), torch.tensor([[0, 1, 3], [0, 4, 2]])),
    "localize_row_negative": lambda: ops.localize(_z(4, 3), torch.tensor([[-1, 1, 3], [0, 1, 2]])),
    "edge_features_col_too_large": lambda: ops.edge_features(_z(4, 3), torch.tensor([[0, 1, 3], [0, 1, 7]])),
    "edge_features_row_negative": lambda: ops.edge_features(_z(4, 3), torch.tensor([[0, -3], [0, 1]])),
    "localize_no_positions": lambda: ops.localize(_z(0, 3), torch.tensor([[0], [0]])),
}


@pytest.mark.parametrize("case", sorted(BAD_INDICES))
def test_ops_index_checks_raise_before_the_device_check(case):
    with pytest.raises(IndexError):
        BAD_INDICES[case]()


def test_ops_valid_shapes_on_the_host_still_reach_the_device_check():
    """The checks refuse bad shapes only: well-formed host tensors still fail at the device check (no CPU fallback)."""
    g = torch.tensor([[0, 0, 1, 2], [0, 1, 1, 2]])
    for call in (lambda: ops.linear(_z(2, 5, 3), _z(4, 3), _z(4)), lambda: ops.safe_norm_rep(_z(4, 5, 3)),
                 lambda: ops.scalarize(_z(4, 3, 2), _z(4, 3, 3)), lambda: ops.vectorize(_z(4, 6), _z(4, 9)),
                 lambda: ops.rowscale(_z(4, 5, 3), _z(4, 5, 1)), lambda: ops.gather_row(_z(5, 3), _graph(5, 9)),
                 lambda: ops.scatter_rows(_z(9, 3), _graph(5, 9), "mean"), lambda: ops.mean_frames(_z(9, 3, 3), _graph(5, 9)),
                 lambda: ops.Graph(g, 3), lambda: ops.embedding(_z(5, 2), torch.tensor([0, 4])), lambda: ops.localize(_z(4, 3), g),
                 lambda: ops.edge_features(_z(4, 3), g), lambda: ops.orientations(_z(4, 3)),
                 lambda: ops.centralize(_z(4, 3), torch.zeros(4, dtype=torch.int64), torch.ones(4, dtype=torch.bool))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
