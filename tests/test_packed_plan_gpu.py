"""Packed plans (gcdm_plan_batches / gcdm_set_batch_seeds): K independent flat batches laid end to end in one plan on one handle.  MI355X only.

The yardstick is the single-batch path: sub-batch k of a packed run must be BIT-identical to the same batch planned with gcdm_plan_batch on the same
handle and run with seed = seeds[k] (what mol_gen_sample_concurrent promises per lane).  Every comparison below is torch.equal on the int32 view of the
fp32 tensors -- no tolerance, and stricter than torch.equal on the floats (it tells -0 from +0 and compares NaN payloads, which the NaN case needs).
Synthetic weights at the production widths, both MFMA modes, T = 6 free-running steps (init, 6 steps, final decode) unless a test says otherwise.
"""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
MODES = [pytest.param(1, id="f16x3"), pytest.param(0, id="f32")]
T_STEPS = 6
PLAN_WIDE = native.FLAG_F16_RANGE | native.FLAG_TAIL


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _model(case):
    """One handle per configuration for the whole file (weights are packed once); every test plans afresh."""
    d = synth.DATASET_DIMS[case]
    ds = "geom" if case == "geom" else "qm9"
    cfgs = pkg.default_cfgs(ds, ("alpha",) if d["n_ctx"] else ())
    net = pkg.GCPNetDynamics(**cfgs)
    net.load_state_dict(synth.make_weights(synth.dynamics_shapes(d["S"], d["V"], d["Se"], d["Ve"], d["L"], synth.dims_h_in(d)), seed=23, scale_2d=0.25))
    net = net.cuda().eval()
    ddpm = pkg.EquivariantVariationalDiffusion(net, cfgs["diffusion_cfg"], cfgs["dataloader_cfg"], pkg.dataset_info(ds)).cuda()
    dyn, lib, h = ddpm._native(torch.device("cuda"))
    return ddpm, dyn, lib, h, 3 + synth.dims_feat(d)


class _H:
    """The handle of one configuration in one MFMA mode, with the few C-ABI calls the tests repeat."""

    def __init__(self, case, mode):
        self.ddpm, self.dyn, self.lib, self.h, self.D = _model(case)
        self.dyn.set_mfma_mode(mode)
        assert self.dyn.mfma_mode == mode
        self.dev = torch.device("cuda")
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert self.lib.gcdm_set_option(self.h, b"step_graph", 1) == 0

    def ok(self, st):
        assert st == 0, self.lib.gcdm_last_error(self.h)

    def plan(self, sizes):
        self.dyn._plan_key = None
        nn_ = torch.tensor(sizes, dtype=torch.int32)
        self.ok(self.lib.gcdm_plan_batch(self.h, len(nn_), _ptr(nn_)))
        return int(nn_.sum())

    def plan_packed(self, batches, seeds=None):
        self.dyn._plan_key = None
        per = torch.tensor([len(b) for b in batches], dtype=torch.int32)
        nn_ = torch.tensor([n for b in batches for n in b], dtype=torch.int32)
        self.ok(self.lib.gcdm_plan_batches(self.h, len(batches), _ptr(per), _ptr(nn_)))
        assert self.lib.gcdm_get_option(self.h, b"num_batches") == len(batches)
        if seeds is not None:
            self.ok(self.lib.gcdm_set_batch_seeds(self.h, len(seeds), (C.c_uint64 * len(seeds))(*seeds)))
        return int(nn_.sum())

    def run(self, N, words, seed, ctx=None, T=T_STEPS):
        """init, T steps, final decode with Philox noise -> z_T, the latent after every step, the decoded output, the flag words."""
        lib, h = self.lib, self.h
        z = torch.empty((N, self.D), device=self.dev)
        out = torch.empty((N, self.D), device=self.dev)
        fl = torch.zeros(words, dtype=torch.int32, device=self.dev)
        sd = C.c_uint64(seed)
        self.ok(lib.gcdm_sample_init(h, _ptr(z), None, sd, self.stream))
        lat = [z.clone()]
        for s in reversed(range(T)):
            self.ok(lib.gcdm_sample_step(h, _ptr(z), _ptr(ctx), s, T, None, sd, _ptr(fl), self.stream))
            lat.append(z.clone())
        self.ok(lib.gcdm_sample_final(h, _ptr(z), _ptr(ctx), None, sd, _ptr(out), _ptr(fl), self.stream))
        torch.cuda.synchronize()
        return lat, out, fl.cpu().tolist()

    def forward(self, xh, t, ctx, words):
        out = torch.empty_like(xh)
        fl = torch.zeros(words, dtype=torch.int32, device=self.dev)
        self.ok(self.lib.gcdm_forward(self.h, _ptr(xh), _ptr(t), _ptr(ctx), _ptr(out), _ptr(fl), self.stream))
        torch.cuda.synchronize()
        return out, fl.cpu().tolist()

    def chi0(self, N):
        buf = np.empty(6 * N, dtype=np.float32)
        assert self.lib.gcdm_debug_read(self.h, b"chi0", buf.ctypes.data_as(C.c_void_p), buf.size) == buf.size, self.lib.gcdm_last_error(self.h)
        return torch.from_numpy(buf).reshape(6, N)


def _offsets(batches):
    off = [0]
    for b in batches:
        off.append(off[-1] + sum(b))
    return off


SEEDS = [77, 5, 2 ** 40 + 3, 11]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case,batches", [
    ("qm9", [[5, 1, 7], [3], [2, 9, 4, 4]]),       # a one-atom molecule, a one-molecule sub-batch, seams inside a node tile and inside an edge tile
    ("qm9", [[8] * 8, [6, 5]]),                    # sub-batch 0: 64 nodes, 512 edges -- its seam on a 32- / 64-node tile boundary and on a 64-edge tile boundary
    ("qm9", [[1], [1], [4]]),                      # one-atom sub-batches: one self edge each, both orientations zero
    ("geom", [[44, 3], [181]]),
], ids=["ragged", "tile_seams", "one_atom", "geom"])
def test_packed_run_equals_the_single_runs(case, batches, mode):
    """z_T, the latent after each of the 6 steps, the decoded output and each sub-batch's flag word against the K single runs with the same seeds."""
    H = _H(case, mode)
    K, off = len(batches), _offsets(batches)
    seeds = SEEDS[:K]
    N = H.plan_packed(batches, seeds)
    assert N == off[-1]
    lat, out, words = H.run(N, K, seed=999)            # (the scalar seed is ignored under a packed plan)
    for k, b in enumerate(batches):
        n = H.plan(b)
        lat1, out1, w1 = H.run(n, 1, seeds[k])
        assert torch.isfinite(out1).all()
        for i, (a, a1) in enumerate(zip(lat, lat1)):
            assert _same(a[off[k]:off[k + 1]], a1), f"sub-batch {k}, latent {i}"
        assert _same(out[off[k]:off[k + 1]], out1), f"sub-batch {k}, decoded output"
        assert words[k] == w1[0], f"sub-batch {k}: flag word {words[k]} against {w1[0]}"


@pytest.mark.parametrize("mode", MODES)
def test_forward_under_a_packed_plan_cuts_the_orientations_at_the_seams(mode):
    """gcdm_forward with random xh, per-node t and a context on the conditional configuration: output rows and CHI0 (orientations, [6][N]) equal the
    separate forwards, seam rows included.  Control: the same concatenation planned with plain gcdm_plan_batch differs from the separate forwards at
    a seam row of CHI0 -- a missing cut would be seen."""
    H = _H("qm9cond", mode)
    batches = [[5, 1, 7], [3], [2, 9, 4, 4]]
    K, off = len(batches), _offsets(batches)
    N = off[-1]
    g = torch.Generator().manual_seed(31)
    xh = torch.randn((N, H.D), generator=g).to(H.dev)
    t = torch.rand(N, generator=g).to(H.dev)
    ctx = torch.randn((N, 1), generator=g).to(H.dev)
    assert H.plan_packed(batches) == N
    out, words = H.forward(xh, t, ctx, K)
    chi = H.chi0(N)
    assert words == [0] * K and torch.isfinite(out).all()
    assert H.plan([n for b in batches for n in b]) == N
    H.forward(xh, t, ctx, 1)
    chi_flat = H.chi0(N)
    seam_differs = False
    for k, b in enumerate(batches):
        n, sl = H.plan(b), slice(off[k], off[k + 1])
        o1, w1 = H.forward(xh[sl].contiguous(), t[sl].contiguous(), ctx[sl].contiguous(), 1)
        c1 = H.chi0(n)
        assert _same(out[sl], o1) and w1 == [0], f"sub-batch {k}"
        assert _same(chi[:, sl], c1), f"sub-batch {k}: orientations"
        assert torch.equal(c1[:3, -1], torch.zeros(3)) and torch.equal(c1[3:, 0], torch.zeros(3))        # zero padded at the batch's two ends
        seam_differs |= not _same(chi_flat[:, sl][:, [0, -1]], c1[:, [0, -1]])
    assert seam_differs


@pytest.mark.parametrize("mode", MODES)
def test_one_sub_batch_equals_gcdm_plan_batch(mode):
    """num_batches == 1: the same bits as gcdm_plan_batch, for a forward (output, orientations, final node scalars) and a 6-step run."""
    H = _H("qm9", mode)
    sizes = [5, 1, 7, 19, 3]
    N = sum(sizes)
    g = torch.Generator().manual_seed(37)
    xh = torch.randn((N, H.D), generator=g).to(H.dev)
    t = torch.rand(N, generator=g).to(H.dev)

    def both(planner):
        planner()
        o, w = H.forward(xh, t, None, 1)
        c = H.chi0(N)
        return (o, c) + H.run(N, 1, seed=123 if planner is plain else 0) + (w,)

    plain = lambda: H.plan(sizes)                                    # noqa: E731
    packed = lambda: H.plan_packed([sizes], [123])                   # noqa: E731
    o0, c0, lat0, out0, w0, fw0 = both(plain)
    o1, c1, lat1, out1, w1, fw1 = both(packed)
    assert _same(o0, o1) and _same(c0, c1) and fw0 == fw1
    assert len(lat0) == T_STEPS + 1 and all(_same(a, b) for a, b in zip(lat0, lat1))
    assert _same(out0, out1) and w0 == w1


@pytest.mark.parametrize("mode", MODES)
def test_captured_step_equals_direct_launches_under_a_packed_plan(mode):
    """The step graph serves a packed plan (seeds and tables are device-resident): same latents as direct launches, and new seeds need no re-capture."""
    H = _H("qm9", mode)
    batches = [[5, 1, 7], [3], [2, 9, 4, 4]]
    K = len(batches)
    N = H.plan_packed(batches, SEEDS[:K])
    res = {}
    for graph in (0, 1):
        assert H.lib.gcdm_set_option(H.h, b"step_graph", graph) == 0
        before = H.lib.gcdm_get_option(H.h, b"graph_launches")
        res[graph] = H.run(N, K, seed=graph)                          # (different scalar seeds: ignored)
        assert H.lib.gcdm_get_option(H.h, b"graph_launches") - before == (T_STEPS if graph else 0), H.lib.gcdm_last_error(H.h)
    assert all(_same(a, b) for a, b in zip(res[0][0], res[1][0])) and _same(res[0][1], res[1][1]) and res[0][2] == res[1][2]
    # other seeds through the SAME captured step: the table changed, the graph did not
    H.ok(H.lib.gcdm_set_batch_seeds(H.h, K, (C.c_uint64 * K)(*[s + 1 for s in SEEDS[:K]])))
    other = H.run(N, K, seed=1)
    assert not _same(other[0][0], res[1][0][0])
    assert H.lib.gcdm_set_option(H.h, b"step_graph", 0) == 0
    direct = H.run(N, K, seed=1)
    assert all(_same(a, b) for a, b in zip(other[0], direct[0])) and _same(other[1], direct[1])
    assert H.lib.gcdm_set_option(H.h, b"step_graph", 1) == 0


def _step_once(H, z, words, seed, s=3, T=T_STEPS):
    z = z.clone()
    fl = torch.zeros(words, dtype=torch.int32, device=H.dev)
    H.ok(H.lib.gcdm_sample_step(H.h, _ptr(z), None, s, T, None, C.c_uint64(seed), _ptr(fl), H.stream))
    torch.cuda.synchronize()
    return z, fl.cpu().tolist()


@pytest.mark.parametrize("mode", MODES)
def test_nan_in_vel_stays_inside_its_sub_batch(mode):
    """One NaN in the latent row of ONE molecule of sub-batch 1 (an input value) before a single gcdm_sample_step: that sub-batch equals its single run on the
    same poisoned latent -- vel zeroed for all its molecules, FLAG_NAN_VEL in its word -- and the others equal their clean single runs with a clean word.
    fp32 MFMA: the words are exactly FLAG_NAN_VEL and 0.  Split-precision mode: a non-finite value also raises FLAG_F16_RANGE, which is plan-wide by
    definition (it asks for the fp32 re-run of the whole plan), so there the poisoned sub-batch carries FLAG_NAN_VEL | FLAG_F16_RANGE as its single run does and
    the clean ones carry FLAG_F16_RANGE alone; the latents are compared bitwise in both modes."""
    H = _H("qm9", mode)
    batches = [[5, 7], [6, 3, 4], [2, 9]]
    K, off = len(batches), _offsets(batches)
    seeds = SEEDS[:K]
    N = off[-1]
    clean = (0.5 * torch.randn((N, H.D), generator=torch.Generator().manual_seed(41))).to(H.dev)
    bad = clean.clone()
    bad[off[1] + 2, 0] = float("nan")                                # an atom of molecule 0 of sub-batch 1
    H.plan_packed(batches, seeds)
    z, words = _step_once(H, bad, K, 0)
    singles = []
    for k, b in enumerate(batches):
        H.plan(b)
        singles.append(_step_once(H, bad[off[k]:off[k + 1]], 1, seeds[k]))
    H.plan(batches[1])
    z1_clean, w1_clean = _step_once(H, clean[off[1]:off[2]], 1, seeds[1])
    range_bit = native.FLAG_F16_RANGE if mode == 1 else 0
    assert w1_clean == [0] and singles[1][1] == [native.FLAG_NAN_VEL | range_bit]
    assert words[1] == native.FLAG_NAN_VEL | range_bit
    for k in range(K):
        assert _same(z[off[k]:off[k + 1]], singles[k][0]), f"sub-batch {k}"
        if k != 1:
            assert singles[k][1] == [0] and words[k] == range_bit and torch.isfinite(z[off[k]:off[k + 1]]).all()
    # vel was zeroed for ALL molecules of sub-batch 1: its NaN-free molecules moved differently than in the clean run
    rest = slice(batches[1][0], None)
    assert torch.isfinite(singles[1][0][rest]).all() and not _same(singles[1][0][rest, :3], z1_clean[rest, :3])


@pytest.mark.parametrize("mode", MODES)
def test_cog_drift_is_reprojected_in_its_sub_batch_only(mode):
    """A z_0 whose centroid is off in one molecule of sub-batch 1 (as test_final_decode_cog_drift_flag_and_reprojection shifts it): FLAG_COG_DRIFT and the
    re-projection appear in that sub-batch only -- all of its molecules re-centred, as its single run does -- the others are bit-equal to their single runs."""
    H = _H("qm9", mode)
    batches = [[5, 19, 8], [4, 12, 6], [7, 3]]
    K, off = len(batches), _offsets(batches)
    seeds = SEEDS[:K]
    N = off[-1]
    sizes = torch.tensor([n for b in batches for n in b])
    bi = torch.repeat_interleave(torch.arange(len(sizes)), sizes)
    z = 0.3 * torch.randn((N, H.D), generator=torch.Generator().manual_seed(9))
    mean = torch.zeros(len(sizes), 3).index_add_(0, bi, z[:, :3]) / sizes[:, None]
    z[:, :3] -= mean[bi]
    z[off[1] + 4:off[1] + 16, 0] += 0.75                             # molecule 1 of sub-batch 1 drifts along x
    z = z.to(H.dev)

    def final(rows, words, seed):
        out = torch.empty((rows.shape[0], H.D), device=H.dev)
        fl = torch.zeros(words, dtype=torch.int32, device=H.dev)
        assert H.lib.gcdm_get_option(H.h, b"cog_fix") == 1
        H.ok(H.lib.gcdm_sample_final(H.h, _ptr(rows), None, None, C.c_uint64(seed), _ptr(out), _ptr(fl), H.stream))
        torch.cuda.synchronize()
        return out, fl.cpu().tolist()

    H.plan_packed(batches, seeds)
    out, words = final(z, K, 0)
    assert words == [0, native.FLAG_COG_DRIFT, 0]
    for k, b in enumerate(batches):
        H.plan(b)
        o1, w1 = final(z[off[k]:off[k + 1]].contiguous(), 1, seeds[k])
        assert _same(out[off[k]:off[k + 1]], o1) and w1 == [words[k]], f"sub-batch {k}"
    cog = torch.zeros(len(sizes), 3).index_add_(0, bi, out[:, :3].cpu()).abs().max(dim=1).values
    lo, hi = len(batches[0]), len(batches[0]) + len(batches[1])
    assert cog[lo:hi].max().item() < 1e-4                            # every molecule of sub-batch 1 re-centred, not only the one that drifted


def _qm9_model():
    cfgs = pkg.default_cfgs("qm9")
    torch.manual_seed(0)
    model = pkg.QM9MoleculeGenerationDDPM(**cfgs)
    with torch.no_grad():
        for p in model.ddpm.dynamics_network.parameters():
            if p.dim() == 2:
                p.mul_(0.25)
    return model.cuda()


def test_python_drivers_equal_the_concurrent_ones():
    """mol_gen_sample_packed against mol_gen_sample_concurrent on the same lists and seeds (3 batches of 12 molecules, sizes from the QM9 histogram with a
    fixed generator, T = 6), and sample_and_analyze(packed_batches=3) against concurrent_batches=3."""
    model = _qm9_model()
    ddpm = model.ddpm
    nd = ddpm.num_nodes_distribution
    g = torch.Generator().manual_seed(12)
    lists = [nd.num_nodes.cpu()[torch.multinomial(nd.prob.cpu().float(), 12, replacement=True, generator=g)] for _ in range(3)]
    assert len({int(n) for nn_ in lists for n in nn_}) > 3           # ragged
    seeds = [77, 78, 79]
    con = [(xh.clone(), bi.clone(), m.clone()) for xh, bi, m in ddpm.mol_gen_sample_concurrent(lists, "cuda", num_timesteps=T_STEPS, seeds=seeds)]
    fl_con = ddpm.last_flags
    ddpm.release_lanes()
    ddpm.last_flags = -1
    before = ddpm.dynamics_network._lib.gcdm_get_option(ddpm.dynamics_network._handle, b"graph_launches")
    pck = ddpm.mol_gen_sample_packed(lists, "cuda", num_timesteps=T_STEPS, seeds=seeds)
    assert ddpm.dynamics_network._lib.gcdm_get_option(ddpm.dynamics_network._handle, b"graph_launches") - before == T_STEPS      # the captured step, on the primary handle
    assert not getattr(ddpm, "_lanes", None)                         # no lane handles
    assert len(pck) == 3 and ddpm.last_flags == fl_con == 0
    for (a, abi, am), (b, bbi, bm) in zip(con, pck):
        assert _same(a, b) and torch.equal(abi, bbi) and torch.equal(am, bm)
    # defaults: seeds[b] = 1234 + b, as the concurrent driver has them
    d_con = [xh.clone() for xh, _, _ in ddpm.mol_gen_sample_concurrent(lists[:2], "cuda", num_timesteps=2)]
    ddpm.release_lanes()
    d_pck = ddpm.mol_gen_sample_packed(lists[:2], "cuda", num_timesteps=2)
    assert all(_same(a, b[0]) for a, b in zip(d_con, d_pck))
    # the module-level call plans for itself again after a packed run
    one = ddpm.mol_gen_sample(len(lists[0]), lists[0], "cuda", num_timesteps=T_STEPS, seed=77)[0]
    assert _same(one, con[0][0])
    torch.manual_seed(3)
    r_con = model.sample_and_analyze(num_samples=36, batch_size=12, num_timesteps=T_STEPS, concurrent_batches=3)
    ddpm.release_lanes()
    torch.manual_seed(3)
    r_pck = model.sample_and_analyze(num_samples=36, batch_size=12, num_timesteps=T_STEPS, packed_batches=3)
    assert r_con.keys() == r_pck.keys()
    for key in r_con:
        a, b = r_con[key], r_pck[key]
        assert a == b or (isinstance(a, float) and np.isnan(a) and np.isnan(b)), key


def test_out_of_scope_calls_are_refused_and_leave_the_handle_usable():
    """The _sc and inpaint entry points, gcdm_encode_samples, gcdm_plan_batch_masked and the options fix_noise / flat_prev / flat_next / node_base return non-zero
    with a message under a packed plan and leave it in place; an ordinary gcdm_plan_batch + forward afterwards gives the bits it gave before."""
    H = _H("qm9", 1)
    lib, h, st = H.lib, H.h, H.stream
    sizes = [4, 5]
    N = sum(sizes)
    g = torch.Generator().manual_seed(43)
    xh = torch.randn((N, H.D), generator=g).to(H.dev)
    t = torch.rand(N, generator=g).to(H.dev)
    H.plan(sizes)
    want, _ = H.forward(xh, t, None, 1)
    batches = [sizes, [3]]
    Np = H.plan_packed(batches, [1, 2])
    z = torch.zeros((Np, H.D), device=H.dev)
    z2 = torch.zeros_like(z)
    fixed = torch.zeros(Np, dtype=torch.uint8, device=H.dev)
    fl = torch.zeros(2, dtype=torch.int32, device=H.dev)
    tp = torch.rand(Np, device=H.dev)
    sd = C.c_uint64(1)
    nn_ = torch.tensor(sizes + [3], dtype=torch.int32)
    mask = torch.ones(Np, dtype=torch.uint8)
    mask[1] = 0
    calls = {
        "gcdm_forward_sc": lambda: lib.gcdm_forward_sc(h, _ptr(z), None, _ptr(tp), None, _ptr(z2), _ptr(fl), st),
        "gcdm_sample_step_sc": lambda: lib.gcdm_sample_step_sc(h, _ptr(z), _ptr(z2), 0, None, 2, T_STEPS, None, None, sd, _ptr(fl), st),
        "gcdm_sample_final_sc": lambda: lib.gcdm_sample_final_sc(h, _ptr(z), None, None, None, sd, _ptr(z2), _ptr(fl), st),
        "gcdm_inpaint_center": lambda: lib.gcdm_inpaint_center(h, _ptr(z), _ptr(fixed), _ptr(z2), st),
        "gcdm_inpaint_step": lambda: lib.gcdm_inpaint_step(h, _ptr(z), _ptr(z2), _ptr(fixed), None, 0, None, 2, T_STEPS, None, None, None, sd, 0, _ptr(fl), st),
        "gcdm_inpaint_jump": lambda: lib.gcdm_inpaint_jump(h, _ptr(z), 1, 2, T_STEPS, None, sd, 0, st),
        "gcdm_encode_samples": lambda: lib.gcdm_encode_samples(h, _ptr(z), _ptr(z2), _ptr(fl), st),
        "gcdm_plan_batch_masked": lambda: lib.gcdm_plan_batch_masked(h, len(nn_), _ptr(nn_), _ptr(mask)),
    }
    for name in ("fix_noise", "flat_prev", "flat_next", "node_base"):
        calls[f"option {name}"] = lambda name=name: lib.gcdm_set_option(h, name.encode(), 1)
    for name, call in calls.items():
        assert lib.gcdm_set_option(h, b"cog_fix", 1) == 0             # (a successful call in between: the message below is the refusal's own)
        status = call()
        msg = lib.gcdm_last_error(h)
        assert status != 0 and msg and b"packed" in msg, (name, status, msg)
        assert lib.gcdm_get_option(h, b"num_batches") == 2 and lib.gcdm_num_nodes(h) == Np, name
    for name in ("fix_noise", "flat_prev", "flat_next", "node_base"):
        assert lib.gcdm_get_option(h, name.encode()) == 0
    # misuse of the two new entry points themselves
    assert lib.gcdm_set_batch_seeds(h, 3, (C.c_uint64 * 3)(1, 2, 3)) != 0 and lib.gcdm_last_error(h)
    per_bad = torch.tensor([2, 0], dtype=torch.int32)
    assert lib.gcdm_plan_batches(h, 2, _ptr(per_bad), _ptr(nn_)) != 0 and lib.gcdm_last_error(h)
    assert lib.gcdm_get_option(h, b"num_batches") == 2                # an argument error leaves the plan in place
    # the packed plan still runs, and an ordinary plan afterwards gives the old bits
    torch.cuda.synchronize()
    lat, out, words = H.run(Np, 2, seed=0, T=2)
    assert torch.isfinite(out).all() and words == [0, 0]
    H.plan(sizes)
    assert lib.gcdm_get_option(h, b"num_batches") == 0
    assert lib.gcdm_set_batch_seeds(h, 1, (C.c_uint64 * 1)(1)) != 0   # no packed plan any more
    got, w = H.forward(xh, t, None, 1)
    assert _same(got, want) and w == [0]
    # and a handle on which a slice option is set cannot be given a packed plan
    assert lib.gcdm_set_option(h, b"flat_next", 1) == 0
    per = torch.tensor([2, 1], dtype=torch.int32)
    assert lib.gcdm_plan_batches(h, 2, _ptr(per), _ptr(nn_)) != 0 and b"flat_next" in lib.gcdm_last_error(h)
    assert lib.gcdm_set_option(h, b"flat_next", 0) == 0
    got, w = H.forward(xh, t, None, 1)
    assert _same(got, want)
