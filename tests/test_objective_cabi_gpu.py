"""gcdm_objective_workspace_bytes / _prepare / _terms / _reduce / _bwd (include/gcdm_objective.h) called directly through ctypes on an MI355X,
against tests/objective_ref.py in fp64 -- never through ops.diffusion_objective.

Harness (_call): every input, every output and the workspace lie inside larger device buffers between GUARD guard words (a quiet NaN with a
payload); outputs and the workspace are filled with another NaN at exactly the advertised size.  After the calls the guards and every input
must be bitwise as they were and no output element may still hold the fill.  node_offsets come from gcdm_op_rowptr on the device.

Bar, per element: |got - ref64| <= M |ref32 - ref64| + 8 * 2^-24 * Sigma |terms summed|, ref32 = the restatement's own fp32 run, M = 4
(objective_ref.bar_ok; the same function rejects every mutant in tests/test_objective_cpu.py).  Inputs stay clear of the 1e-10 epsilon of
`mass` wherever a mass carries weight (checked on the CPU, _clear_of_epsilon).  Every case prints its worst factor per tensor ("MEASURED").
Figures measured so far: DESIGN.md 3.6, "Fused diffusion objective"."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import objective_ref as R
from test_objective_cpu import make_inputs

pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
GUARD_BITS, FILL_BITS = 0x7FC0BEEF, 0x7FC00A11
SIZES = [1, 2, 7, 13, 9, 3]
T_MIX = [0, 1, 1000, 5, 500, 999]


def _lib():
    lib = native.load_ops()
    assert set(native.OBJECTIVE_SIGNATURES) == {"gcdm_objective_workspace_bytes", "gcdm_objective_prepare", "gcdm_objective_terms", "gcdm_objective_reduce",
                                                "gcdm_objective_bwd"}
    return lib


class _Buf:
    """n 32-bit words between guards; `host` (any 4-byte dtype, or uint8 with a multiple of 4 bytes) = an input, None = an output to fill."""

    def __init__(self, n=None, host=None, partial=False):
        self.partial = partial            # an output the entries need not write to its end (the workspace is advertised in 256-byte steps)
        if host is not None:
            raw = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
            raw = np.concatenate([raw, np.zeros((-raw.size) % 4, dtype=np.uint8)])
            words = raw.view(np.uint32)
            n = words.size
        self.n, self.is_input = n, host is not None
        full = np.full(n + 2 * GUARD, GUARD_BITS, dtype=np.uint32)
        full[GUARD:GUARD + n] = words if host is not None else FILL_BITS
        self.host = full
        self.dev = torch.from_numpy(full.view(np.int32)).to(DEV)
        self.ptr = C.c_void_p(self.dev.data_ptr() + 4 * GUARD)

    def read(self, dtype=np.float32, what=""):
        got = self.dev.cpu().numpy().view(np.uint32)
        assert (got[:GUARD] == GUARD_BITS).all() and (got[GUARD + self.n:] == GUARD_BITS).all(), f"write outside {what}"
        body = got[GUARD:GUARD + self.n]
        if self.is_input:
            assert (body == self.host[GUARD:GUARD + self.n]).all(), f"input {what} changed"
        elif not self.partial:
            assert not (body == FILL_BITS).any(), f"output {what} not fully written"
        return body.view(dtype).copy()


def _call(inp, net, net0=None, by_max=False, grads=None, stream=None):
    """The four entries on one input dictionary -> dict of numpy outputs (flags included)."""
    lib = _lib()
    off, nf, ic, T, mode = inp["off"], inp["nf"], inp["ic"], inp["T"], inp["mode"]
    B, N, D = len(off) - 1, int(off[-1]), 3 + nf + ic
    f32 = lambda t: None if t is None else _Buf(host=t.detach().float().numpy())          # noqa: E731
    bufs = dict(x=f32(inp["x"]), one_hot=f32(inp["one_hot"]), charges=f32(inp["charges"]) if ic else None, gamma=f32(inp["gamma"]), log_pn=f32(inp["log_pn"]),
                eps_raw=f32(inp["eps_raw"]), eps_raw_0=f32(inp["eps_raw_0"]), net=f32(net), net0=f32(net0),
                t_int=_Buf(host=inp["t_int"].numpy().astype(np.int32)), bi=_Buf(host=R._bi(off).numpy().astype(np.int64)))
    mask = inp["mask"]
    if mask is not None:
        mk = np.zeros((N + 3) // 4 * 4, dtype=np.uint8)
        mk[:N] = mask.numpy().astype(np.uint8)
        bufs["mask"] = _Buf(host=mk)
    ws_bytes = int(lib.gcdm_objective_workspace_bytes(N, B, D, mode))
    assert ws_bytes >= 8 * B and ws_bytes % 256 == 0
    ev = mode == R.EVAL
    outs = dict(off=_Buf(B + 1), xh=_Buf(N * D), eps_t=_Buf(N * D), z_t=_Buf(N * D), t_node=_Buf(N), mol=_Buf(B * 8), terms=_Buf(B * 10), nll=_Buf(B),
                means=_Buf(16), ws=_Buf(ws_bytes // 4, partial=True))
    if ev:
        outs.update(eps_0=_Buf(N * D), z_0=_Buf(N * D))
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    nv, nb = (C.c_float * 3)(*inp["nv"]), (C.c_float * 3)(*inp["nb"])
    p = lambda k: bufs[k].ptr if bufs.get(k) is not None else None          # noqa: E731
    o = lambda k: outs[k].ptr if k in outs else None          # noqa: E731
    s = torch.cuda.current_stream() if stream is None else stream
    st = C.c_void_p(s.cuda_stream)
    fp = C.c_void_p(flags.data_ptr())
    with torch.cuda.stream(s):
        assert lib.gcdm_op_rowptr(p("bi"), N, B, o("off"), fp, st) == 0
        assert lib.gcdm_objective_prepare(p("x"), p("one_hot"), p("charges"), p("mask"), o("off"), p("t_int"), p("gamma"), p("log_pn"), len(inp["log_pn"]),
                                          nv, nb, p("eps_raw"), p("eps_raw_0"), o("xh"), o("eps_t"), o("z_t"), o("eps_0"), o("z_0"), o("t_node"), o("mol"),
                                          fp, N, B, nf, ic, T, mode, int(inp["center_x"]), st) == 0
        assert lib.gcdm_objective_terms(p("net"), p("net0"), o("xh"), o("eps_t"), o("z_t"), o("eps_0"), o("z_0"), p("mask"), o("off"), o("mol"),
                                        p("gamma"), nv, nb, o("terms"), N, B, nf, ic, T, mode, st) == 0
        assert lib.gcdm_objective_reduce(o("mol"), o("terms"), o("ws"), o("nll"), o("means"), B, D, T, mode, int(by_max), st) == 0
        if grads is not None:
            gb = [None if g is None else _Buf(host=g.float().numpy()) for g in grads]
            gp = [None if g is None else g.ptr for g in gb]
            outs["d"] = _Buf(N * D)
            assert lib.gcdm_objective_bwd(gp[0], 1, gp[1], 1, gp[2], 1, gp[3], p("net"), o("eps_t"), p("mask"), o("off"), o("mol"), o("ws"), o("d"),
                                          N, B, D, mode, st) == 0
            for i, g in enumerate(gb):
                if g is not None:
                    bufs[f"g{i}"] = g
    s.synchronize()
    torch.cuda.synchronize()
    for k, b in bufs.items():
        if b is not None:
            b.read(np.uint32, k)
    res = {k: b.read(np.int32 if k == "off" else np.float32, k) for k, b in outs.items()}
    assert (res["off"] == off.numpy()).all()
    res["flags"] = int(flags.item())
    shp = dict(xh=(N, D), eps_t=(N, D), z_t=(N, D), eps_0=(N, D), z_0=(N, D), mol=(B, 8), terms=(B, 10), d=(N, D))
    return {k: (v.reshape(shp[k]) if k in shp else v) for k, v in res.items()}


def _clear_of_epsilon(inp, r32):
    """Every mass that carries weight in the fp32 restatement is far above the 1e-10 epsilon."""
    d = R.mass_argument(r32["prep"], inp["off"], inp["gamma"], inp["nv"], inp["nb"], inp["nf"], inp["ic"], inp["mode"])
    bi = R._bi(inp["off"])
    w = [(r32["prep"]["xh"][:, 3:3 + inp["nf"]] * inp["nv"][1] + inp["nb"][1]).abs() > 0.5]
    if inp["ic"]:
        w.append(torch.ones(len(bi), 1, dtype=torch.bool))
    w = torch.cat(w, dim=-1)
    counts = torch.ones(len(bi), dtype=torch.bool) if inp["mode"] == R.EVAL else r32["prep"]["mol"][:, 4][bi] > 0
    present = torch.ones(len(bi), dtype=torch.bool) if inp["mask"] is None else inp["mask"] != 0
    sel = w & (counts & present).unsqueeze(-1)
    assert not sel.any() or d[sel].min().item() > 1e-4


def _net(inp, seed=1):
    """As the real network on masked rows: the x columns zero, the other columns not (the scalar projection's bias, gcpnet.py:1190)."""
    N, D = int(inp["off"][-1]), 3 + inp["nf"] + inp["ic"]
    g = torch.Generator().manual_seed(seed)
    m = torch.ones(N, D)
    if inp["mask"] is not None:
        m[:, :3] = (inp["mask"] != 0).float().unsqueeze(-1)
    return torch.randn((N, D), generator=g) * m, (torch.randn((N, D), generator=g) * m if inp["mode"] == R.EVAL else None)


def _synthetic_table(inp, missing=()):
    g = torch.Generator().manual_seed(77)
    tab = torch.log(torch.rand(200, generator=g) * 0.1 + 1e-3)
    for n in missing:
        tab[n] = float("nan")
    inp["log_pn"] = tab
    return inp


def _check(inp, by_max=False, label="", with_bwd=True, M=4.0):
    net, net0 = _net(inp)
    r32, _ = R.run(inp, net, net0, by_max, torch.float32)
    r64, mag = R.run(inp, net, net0, by_max, torch.float64)
    _clear_of_epsilon(inp, r32)
    B = len(inp["off"]) - 1
    grads = None
    if with_bwd and inp["mode"] != R.EVAL:
        g = torch.Generator().manual_seed(3)
        grads = [torch.randn(B, generator=g) for _ in range(3)] + [torch.randn(1, generator=g)]
    got = _call(inp, net, net0, by_max, grads)
    assert got["flags"] == r64["prep"]["flags"]
    worst = {}
    keys = ["xh", "eps_t", "z_t", "t_node", "mol"] + (["eps_0", "z_0"] if inp["mode"] == R.EVAL else [])
    checks = [(k, got[k], r32["prep"][k], r64["prep"][k], mag["prep"][k]) for k in keys]
    checks += [(k, got[k], r32[k], r64[k], mag[k]) for k in ("terms", "nll")]
    checks.append(("means", got["means"][:10], r32["means"][:10], r64["means"][:10], mag["means"][:10]))
    if grads is not None:
        a = lambda r, dt: R.bwd(grads[0], grads[1], grads[2], grads[3][0], net, r["prep"]["eps_t"], inp["mask"], inp["off"], r["prep"]["mol"], r["coef"], dt)  # noqa: E731
        d32, d64 = a(r32, torch.float32), a(r64, torch.float64)
        checks.append(("d_net_out", got["d"], d32, d64, 2 * d64.abs()))
        if inp["mask"] is not None:
            # masked rows get the error_t part only: exactly 0 where t = 0 selects loss_0_x, and elsewhere what a kernel that skips them
            # (d = 0) would miss by far more than the bar below allows
            gone, t0 = ~(inp["mask"] != 0), r64["prep"]["mol"][:, 4][R._bi(inp["off"])] == 1
            assert (got["d"][(gone & t0).numpy()] == 0).all(), "masked rows of a t = 0 molecule must get exactly 0"
            live = (gone & ~t0).numpy()
            assert live.any() and (got["d"][live, :3] == 0).all()
            want = d64[torch.from_numpy(live)][:, 3:]
            assert want.abs().min().item() > 0 and np.abs(got["d"][live, 3:] - want.numpy()).max() <= 1e-4 * want.abs().max().item()
    if inp["mask"] is not None:          # error_t over ALL rows: the sum over unmasked rows is far from what the device gives
        skipped, _ = R.terms(net * (inp["mask"] != 0).float().unsqueeze(-1), net0, r64["prep"], inp["mask"], inp["off"], inp["gamma"], inp["nv"], inp["nb"],
                             inp["nf"], inp["ic"], inp["T"], inp["mode"])
        moved = (r64["terms"][:, 1] - skipped[:, 1]).abs()
        sel = moved > 0
        assert sel.any() and (np.abs(got["terms"][:, 1] - r64["terms"][:, 1].numpy())[sel.numpy()] <= 1e-3 * moved[sel].numpy()).all()
    bad = []
    for k, g_, a32, a64, mg in checks:
        ok, fac = R.bar_ok(torch.from_numpy(np.asarray(g_)).reshape(a64.shape), a32, a64, mg, M)
        worst[k] = fac
        if not ok:
            bad.append(k)
    print(f"MEASURED {label}: worst factor (err - slack) / |ref32 - ref64| per tensor: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert not bad, (label, bad, worst)
    assert (got["means"][10:] == 0).all()
    return got


def _case(case, sizes, t_int, mode, mask=None, center_x=False, seed=0):
    return _synthetic_table(make_inputs(case, torch.tensor(sizes), t_int, mode, seed=seed, mask=mask, center_x=center_x))


@pytest.mark.parametrize("n", [1, 2, 3])
def test_one_molecule_of_one_two_three_atoms(n):
    for mode, t in ((R.TRAIN_L2, 0), (R.TRAIN_VLB, 7), (R.EVAL, 1)):
        _check(_case("qm9", [n], [t], mode), label=f"B=1 n={n} mode={mode}")


@pytest.mark.parametrize("case,mode,by_max", [("qm9", R.TRAIN_L2, False), ("qm9", R.TRAIN_L2, True), ("qm9", R.TRAIN_VLB, False), ("qm9", R.EVAL, False),
                                              ("geom", R.TRAIN_L2, True), ("geom", R.TRAIN_VLB, False), ("geom", R.EVAL, False)])
def test_ragged_batch_both_widths_every_mode(case, mode, by_max):
    t = T_MIX if mode != R.EVAL else [1, 2, 1000, 5, 500, 999]
    _check(_case(case, SIZES, t, mode, center_x=(mode == R.TRAIN_VLB)), by_max, label=f"{case} ragged mode={mode} by_max={by_max}")


def test_one_181_atom_molecule_among_small_ones():
    _check(_case("geom", [3, 181, 2], [0, 1000, 1], R.TRAIN_VLB), label="geom 181")
    _check(_case("geom", [3, 181, 2], [3, 1, 1000], R.EVAL), label="geom 181 eval")


def test_more_molecules_than_waves_of_a_workgroup():
    _check(_case("qm9", [1] * 65, [i % 3 * 500 for i in range(65)], R.TRAIN_L2), True, label="65 x 1")


@pytest.mark.parametrize("t", [0, 1000])
def test_all_t_zero_and_all_t_T(t):
    _check(_case("qm9", SIZES, [t] * 6, R.TRAIN_VLB), label=f"all t={t}")
    _check(_case("qm9", SIZES, [t] * 6, R.TRAIN_L2), label=f"all t={t} l2")


@pytest.mark.parametrize("mode", [R.TRAIN_L2, R.TRAIN_VLB, R.EVAL])
def test_mask_without_first_last_and_every_second_node(mode):
    """The first and the last molecule keep one node each."""
    sizes = [2, 7, 13, 9, 3]
    N = sum(sizes)
    mask = torch.ones(N, dtype=torch.bool)
    mask[::2] = False
    mask[0] = mask[-1] = False
    inp = _case("qm9", sizes, [0, 1, 1000, 5, 500] if mode != R.EVAL else [1, 2, 1000, 5, 500], mode, mask=mask, center_x=True)
    got = _check(inp, by_max=True, label=f"mask mode={mode}")
    assert got["mol"][0, 5] == 1 and got["mol"][-1, 5] == 1


def test_size_missing_from_the_histogram_raises_the_flag_and_nothing_else():
    inp = _case("qm9", SIZES, T_MIX, R.TRAIN_L2)
    net, _ = _net(inp)
    clean = _call(inp, net)
    inp2 = dict(inp)
    inp2["log_pn"] = inp["log_pn"].clone()
    inp2["log_pn"][7] = float("nan")
    got = _call(inp2, net)
    assert clean["flags"] == 0 and got["flags"] == native.OBJECTIVE_FLAG_SIZE
    assert np.isnan(got["mol"][2, 6]) and np.isnan(got["terms"][2, 7]) and np.isnan(got["nll"][2]) and np.isnan(got["means"][0]) and np.isnan(got["means"][7])
    for k in ("xh", "eps_t", "z_t", "t_node"):
        assert (got[k].view(np.uint32) == clean[k].view(np.uint32)).all()
    keep = np.ones_like(got["terms"], dtype=bool)
    keep[2, 7] = False
    assert (got["terms"].view(np.uint32)[keep] == clean["terms"].view(np.uint32)[keep]).all()
    assert (np.delete(got["nll"], 2).view(np.uint32) == np.delete(clean["nll"], 2).view(np.uint32)).all()
    assert (got["means"][[1, 2, 3, 4, 5, 6, 8, 9]].view(np.uint32) == clean["means"][[1, 2, 3, 4, 5, 6, 8, 9]].view(np.uint32)).all()


def test_non_default_stream_and_two_runs_bitwise_equal():
    inp = _case("qm9", SIZES, T_MIX, R.TRAIN_VLB)
    net, _ = _net(inp)
    g = [torch.ones(6), None, torch.full((6,), 0.5), torch.ones(1)]
    a = _call(inp, net, grads=g)
    b = _call(inp, net, grads=g)
    c = _call(inp, net, grads=g, stream=torch.cuda.Stream())
    for k in a:
        if k != "flags":
            assert (a[k].view(np.uint32) == b[k].view(np.uint32)).all() and (a[k].view(np.uint32) == c[k].view(np.uint32)).all(), k


@pytest.mark.parametrize("mode", [R.TRAIN_VLB, R.EVAL])
def test_a_molecule_is_the_same_bits_alone_and_at_any_position(mode):
    """Rows and terms of a 13-atom molecule: alone, and first / middle / last in a batch with other molecules."""
    n, t = 13, 5
    solo = _case("geom", [n], [t], mode, seed=21)
    net_s, net0_s = _net(solo, seed=8)
    ref = _call(solo, net_s, net0_s)
    other = _case("geom", [7, 64, 3], [0, 1000, 2], mode, seed=22)
    net_o, net0_o = _net(other, seed=9)
    oo = other["off"].long()
    segs = [(int(oo[i]), int(oo[i + 1])) for i in range(3)]
    for pos in (0, 1, 3):
        order = list(range(3))
        order.insert(pos, "solo")
        cat = lambda key, a_, b_: torch.cat([(a_ if o == "solo" else b_[segs[o][0]:segs[o][1]]) for o in order])          # noqa: E731
        inp = dict(solo)
        for key in ("x", "one_hot", "eps_raw") + (("eps_raw_0",) if mode == R.EVAL else ()):
            inp[key] = cat(key, solo[key], other[key])
        inp["t_int"] = torch.tensor([t if o == "solo" else int(other["t_int"][o]) for o in order], dtype=torch.int32)
        inp["off"] = R.offsets_of([n if o == "solo" else segs[o][1] - segs[o][0] for o in order])
        net = cat("net", net_s, net_o)
        net0 = cat("net0", net0_s, net0_o) if mode == R.EVAL else None
        got = _call(inp, net, net0)
        a = int(inp["off"][pos])
        for k in ("xh", "eps_t", "z_t", "t_node") + (("eps_0", "z_0") if mode == R.EVAL else ()):
            assert (got[k][a:a + n].view(np.uint32) == ref[k].view(np.uint32)).all(), (k, pos)
        assert (got["mol"][pos].view(np.uint32) == ref["mol"][0].view(np.uint32)).all() and (got["terms"][pos].view(np.uint32) == ref["terms"][0].view(np.uint32)).all()
        assert got["nll"][pos].view(np.uint32) == ref["nll"][0].view(np.uint32)


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib()
    assert lib.gcdm_objective_workspace_bytes(10, 0, 9, 0) == -1 and lib.gcdm_objective_workspace_bytes(10, 2, 9, 3) == -1
    assert lib.gcdm_objective_reduce(None, None, None, None, None, 2, 9, 1000, 0, 0, None) == -1
    assert lib.gcdm_objective_bwd(None, 1, None, 1, None, 1, None, None, None, None, None, None, None, None, 10, 2, 9, 1, None) == -1
