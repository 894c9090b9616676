"""The column-split first edge layer of the classifier through its C ABI on the MI355X (include/gcdm_classifier_train.h), forward and backward,
against the fp64 definition of tests/classifier_train_ref.py: every molecule size, a batch of one full / one-atom / empty molecule, H = 32 and
96, one case on each side of the edge count at which the dw_r sum takes two stages, outputs NaN-poisoned between guard words, and two calls
bit for bit.  Bar per tensor: err <= 4 gap + floor, gap = the fp32 evaluation of the same definition on the CPU, floor = 16 fp32 ulps of the
tensor's largest entry.  Every figure is printed before it is asserted."""
import importlib

import pytest
import torch

import classifier_ref as cr
import classifier_train_ref as ct

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
TWO = native.CLASSIFIER_TRAIN_TWO_STAGE_EDGES
SIZE_SETS = {"inst": cr.INSTANTIATION_SIZES, "one32": [32], "one1": [1], "one0": [0],
             "below_two_stage": ct.sizes_with_edges(TWO - 2), "at_two_stage": ct.sizes_with_edges(TWO)}


def _check(name, H):
    sizes = SIZE_SETS[name]
    inp = ct.op_inputs(sizes, H)
    a = ct.cabi_edge_pre(inp)
    assert a.st_fwd == 0 and a.st_bwd == 0
    outs = {"pre": a.pre, "radial": a.radial, "dA": a.dA, "dB": a.dB, "dw_r": a.dw}
    for k, g in outs.items():
        assert g.guards_intact(), f"{k}: a guard word was written"
    assert a.ws is None or a.ws.guards_intact()
    assert (a.ws is not None) == (inp.E >= TWO) and a.ws_bytes == (0 if inp.E < TWO else a.ws.n * 4)
    if inp.E == 0:                                             # E = 0 returns 0 without a launch: nothing is written
        for k, g in outs.items():
            assert bool(g.inner.isnan().all()), k
        return a
    for k, g in outs.items():
        assert not bool(g.inner.isnan().any()), f"{k}: an entry was not written"
    # forward: the radial is rounded as torch rounds it, bit for bit; pre against the fp64 definition
    row, col = ct.edge_list(sizes)
    assert torch.equal(a.radial.inner.cpu(), ct.radial_of(inp.x, row, col))
    pre64, _ = ct.edge_pre(inp.A, inp.B, inp.x, inp.w_r, sizes)
    pre32, _ = ct.edge_pre(inp.A, inp.B, inp.x, inp.w_r, sizes, dtype=torch.float32)
    names = ("dA", "dB", "dw_r")
    want = dict(zip(names, ct.edge_pre_bwd(inp.dpre, inp.x, sizes, inp.N)), pre=pre64)
    ref32 = dict(zip(names, ct.edge_pre_bwd(inp.dpre, inp.x, sizes, inp.N, dtype=torch.float32)), pre=pre32)
    got = {"pre": a.pre.inner, "dA": a.dA.inner, "dB": a.dB.inner, "dw_r": a.dw.inner}
    failures, ratios, count = ct.judge(got, want, ref32, what=f"{name} H={H}: ")
    print(f"{name} H={H} E={inp.E}: M needed " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    assert count == 4 and not failures, failures
    return a


@pytest.mark.parametrize("H", ct.OP_H)
@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_forward_and_backward_against_the_fp64_definition(name, H):
    _check(name, H)


@pytest.mark.parametrize("name,H", [("inst", 32), ("at_two_stage", 96), ("below_two_stage", 32)])
def test_two_calls_give_the_same_bits(name, H):
    inp = ct.op_inputs(SIZE_SETS[name], H)
    a, b = ct.cabi_edge_pre(inp), ct.cabi_edge_pre(inp)
    for k in ("pre", "radial", "dA", "dB", "dw"):
        assert torch.equal(getattr(a, k).bits(), getattr(b, k).bits()), k


def test_the_two_stage_count_is_where_the_workspace_starts():
    below, at = ct.op_inputs(SIZE_SETS["below_two_stage"], 32), ct.op_inputs(SIZE_SETS["at_two_stage"], 32)
    assert below.E == TWO - 2 and at.E == TWO
    lib = cr._ops_lib()
    assert lib.gcdm_classifier_train_workspace_bytes(below.E, 32) == 0 < lib.gcdm_classifier_train_workspace_bytes(at.E, 32)


def test_tables_that_disagree_write_nothing_out_of_bounds():
    """A molecule index past the table, a node outside its molecule and an edge offset past E: the node is skipped in the forward and gets zeros
    in the backward; the guards stay intact."""
    import ctypes
    sizes, H = [3, 4], 32
    inp = ct.op_inputs(sizes, H)
    lib = cr._ops_lib()
    mol, noff, eoff = ct.edge_tables(sizes)
    mol[0], mol[3] = 7, 0                                       # out of range; node 3 is not inside molecule 0
    eoff[1] = inp.E                                             # molecule 1's edges would start at the end of the buffer
    mol, noff, eoff = mol.cuda(), noff.cuda(), eoff.cuda()
    A, B, x, w, dpre = (t.cuda() for t in (inp.A, inp.B, inp.x, inp.w_r, inp.dpre))
    pre, radial, dA, dB, dw = cr.Guarded(inp.E * H), cr.Guarded(inp.E), cr.Guarded(inp.N * H), cr.Guarded(inp.N * H), cr.Guarded(H)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = cr._stream_ptr()
    assert lib.gcdm_classifier_train_edge_pre_fwd(p(A), p(B), p(x), p(w), p(mol), p(noff), p(eoff), pre.ptr, radial.ptr, inp.N, 2, inp.E, H, st) == 0
    radial.inner.nan_to_num_(0.0)
    assert lib.gcdm_classifier_train_edge_pre_bwd(p(dpre), radial.ptr, p(mol), p(noff), p(eoff), dA.ptr, dB.ptr, dw.ptr, None, inp.N, 2, inp.E, H, st) == 0
    torch.cuda.synchronize()
    for g in (pre, radial, dA, dB, dw):
        assert g.guards_intact()
    rows = pre.inner.reshape(inp.E, H)
    assert bool(rows[:2].isnan().all()) and not bool(rows[2:6].isnan().any()) and bool(rows[6:].isnan().all())      # nodes 1, 2 of molecule 0 only
    dAm = dA.inner.reshape(inp.N, H)
    assert not bool(dAm.isnan().any()) and float(dAm[0].abs().max()) == 0.0 and float(dAm[3:].abs().max()) == 0.0
