"""The sampler's small kernels and host-side coefficient code, pinned through the C ABI to tests/sampler_ref.py.  MI355X only.

Subjects: k_sample (modes 0-4), k_noise_mean, k_encode, k_unnormalize, k_cog_fix, k_inpaint_center, k_inpaint_combine, the step_row / coefficient code of
gcdm_api.hip (direct launches and the captured step's device table) and the Philox generator.  The network is taken OUT of every comparison: its own
output (h columns from gcdm_forward on the same input, x columns from the velocities of the very forward under test) is fed to the fp64 formula, so what
is left is a handful of fp32 operations per element and the bars are those of that arithmetic, not the network's 1e-4.

Bars (none taken from the code under test):
  * network-free entries: derived, k * 2^-24 * sum|terms| per element, k written out where the bar is formed;
  * step / final decode / x of the inpaint step: 4 * max|ref32 - ref64| + 4 * 2^-24 * scale per case, ref32 and ref64 both from sampler_ref on the same
    z, eps and noise (the reference's own fp32-vs-fp64 gap; part of it is the cancellation softplus(gamma_s) - softplus(gamma_t) between neighbouring
    steps, hence per case);
  * Philox normals: measured (fast log / sincos, fp32 angle on the device), PHILOX_BAR below.
Every test prints its figures ("PIN ..." lines, `pytest -s`); profiles/sampler_pins.txt is one such run.
"""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import sampler_ref as R
import synth

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native

U = 2.0 ** -24
SIZES = [1, 2, 6, 19, 63, 64, 65]       # one node (CoM-free x-noise exactly 0), the 64-lane stride on both sides, n * D across 64
# max |device normal - fp64 reference| over every Philox draw of this file on the MI355X: 1.684e-6, in the 2^20-element draw (profiles/sampler_pins.txt); the
# constant is 4x that.  (|r| <= 5.9 and the fp32 angle is off by <= 3.7e-7, so a correct generator sits within a few 1e-6; a counter / key / lane bug gives
# errors of order 1)
PHILOX_BAR = 4 * 1.7e-6
SEEDS = [77, (0x9E3779B9 << 32) | 5]    # the second one has a non-zero high word
TOL_TODAY = 1e-4                        # the bar the network-bearing tests use, for the ratios in the record


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _report(name, err, bar, scale=1.0):
    print(f"PIN {name}: err {err:.3e} bar {bar:.3e} | err / 1e-4 scale {err / (TOL_TODAY * scale):.2e}, bar / 1e-4 scale {bar / (TOL_TODAY * scale):.2e}")


class _H:
    """One handle of one configuration (synthetic weights at the production widths, scale 0.25) with the few C-ABI calls the tests repeat."""

    def __init__(self, case, self_condition=False):
        d = synth.DATASET_DIMS[case]
        ds = "geom" if case == "geom" else "qm9"
        cfgs = pkg.default_cfgs(ds, ("alpha",) if d["n_ctx"] else ())
        self.F = synth.dims_feat(d)
        if self_condition:
            cfgs["diffusion_cfg"]["self_condition"] = True
        net = pkg.GCPNetDynamics(**cfgs)
        net.load_state_dict(synth.make_weights(synth.dynamics_shapes(d["S"], d["V"], d["Se"], d["Ve"], d["L"], synth.dims_h_in(d),
                                                                     **(dict(self_cond_feats=self.F) if self_condition else {})), seed=41, scale_2d=0.25))
        net = net.cuda().eval()
        self.ddpm = pkg.EquivariantVariationalDiffusion(net, cfgs["diffusion_cfg"], cfgs["dataloader_cfg"], pkg.dataset_info(ds)).cuda()
        self.dyn, self.lib, self.h = self.ddpm._native(torch.device("cuda"))
        self.case, self.D, self.n_ctx = case, 3 + self.F, d["n_ctx"]
        nb = [0.0 if v is None else float(v) for v in cfgs["diffusion_cfg"]["norm_biases"]]
        self.norm = R.Norm(d["num_atom_types"], bool(d["include_charges"]), tuple(float(v) for v in cfgs["diffusion_cfg"]["norm_values"]), tuple(nb))
        self.gamma = self.ddpm.gamma.gamma.detach().to("cpu", torch.float32).numpy().copy()       # the fp32 table the handle was given
        assert len(self.gamma) == 1001
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ok(self, st):
        assert st == 0, self.lib.gcdm_last_error(self.h)

    def opt(self, name, value):
        self.ok(self.lib.gcdm_set_option(self.h, name.encode(), value))

    def plan(self, sizes):
        self.dyn._plan_key = None
        nn_ = torch.tensor(sizes, dtype=torch.int32)
        self.ok(self.lib.gcdm_plan_batch(self.h, len(nn_), _ptr(nn_)))
        assert self.lib.gcdm_num_nodes(self.h) == int(nn_.sum())
        return R.offsets(sizes)

    def plan_packed(self, batches, seeds):
        self.dyn._plan_key = None
        per = torch.tensor([len(b) for b in batches], dtype=torch.int32)
        nn_ = torch.tensor([n for b in batches for n in b], dtype=torch.int32)
        self.ok(self.lib.gcdm_plan_batches(self.h, len(batches), _ptr(per), _ptr(nn_)))
        self.ok(self.lib.gcdm_set_batch_seeds(self.h, len(seeds), (C.c_uint64 * len(seeds))(*seeds)))
        return R.offsets(nn_.tolist())

    def flags(self, words=1):
        return torch.zeros(words, dtype=torch.int32, device="cuda")

    def context(self, noff, seed=3):
        """per-node context [N, 1] of a conditional configuration, else None"""
        if not self.n_ctx:
            return None
        per_mol = torch.randn((len(noff) - 1, 1), generator=torch.Generator().manual_seed(seed))
        return per_mol[np.repeat(np.arange(len(noff) - 1), np.diff(noff))].contiguous().cuda()

    def init(self, N, noise, seed):
        z = torch.full((N, self.D), float("nan"), device="cuda")
        self.ok(self.lib.gcdm_sample_init(self.h, _ptr(z), _ptr(noise), C.c_uint64(seed), self.stream))
        torch.cuda.synchronize()
        return z.cpu().numpy()

    def eps_h(self, z, t, ctx, words=1):
        """h columns of the network's eps at time t (fp32 scalar) on z: gcdm_forward's own output"""
        zd = _dev(z)
        td = torch.full((len(z),), float(np.float32(t)), device="cuda")
        out, fl = torch.empty_like(zd), self.flags(words)
        self.ok(self.lib.gcdm_forward(self.h, _ptr(zd), _ptr(td), _ptr(ctx), _ptr(out), _ptr(fl), self.stream))
        torch.cuda.synchronize()
        assert fl.cpu().tolist() == [0] * words
        return out.cpu().numpy()[:, 3:]

    def vel(self, N):
        """velocities [3, N] of the LAST forward (before the CoM projection that makes them eps's x columns)"""
        buf = np.empty(3 * N, dtype=np.float32)
        assert self.lib.gcdm_debug_read(self.h, b"vel", buf.ctypes.data_as(C.c_void_p), buf.size) == buf.size, self.lib.gcdm_last_error(self.h)
        return buf.reshape(3, N)

    def eps(self, eps_h, noff, dtype):
        return np.concatenate((R.eps_from_vel(self.vel(len(eps_h)), noff, dtype), eps_h.astype(dtype)), axis=1)

    def step_to(self, z_in, z_out, ctx, s, n, noise, seed, fl):
        self.ok(self.lib.gcdm_sample_step_to(self.h, _ptr(z_in), _ptr(z_out), _ptr(ctx), s, n, _ptr(noise), C.c_uint64(seed), _ptr(fl), self.stream))
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def qm9():
    return _H("qm9")


@pytest.fixture(scope="module")
def geom():
    return _H("geom")


@pytest.fixture(scope="module")
def qm9cond():
    return _H("qm9cond")


@pytest.fixture(scope="module")
def qm9sc():
    return _H("qm9", self_condition=True)


def _tape(seed, N, F):
    """One raw draw in the reference's randn order: x-part [N,3], then h-part [N,F]."""
    g = torch.Generator().manual_seed(seed)
    return torch.cat((torch.randn((N, 3), generator=g), torch.randn((N, F), generator=g)), dim=-1).numpy()


def _latent(seed, noff, D, scale):
    z = torch.randn((int(noff[-1]), D), generator=torch.Generator().manual_seed(seed)).numpy() * np.float32(scale)
    z[:, :3] -= R.mol_mean(z[:, :3], noff, np.float32)
    return z


def _gap_bar(ref32, ref64):
    """the project's rule: the reference's own fp32-vs-fp64 gap on these inputs (x4: another legitimate operation order, libm against torch)"""
    scale = max(1.0, float(np.abs(ref64).max()))
    return 4 * float(np.abs(ref32.astype(np.float64) - ref64).max()) + 4 * U * scale, scale


def _mean_terms(a, noff):
    """per-node copy of its molecule's mean |a| (the sum|terms| / n of a mean over the molecule)"""
    return R.mol_mean(np.abs(a), noff)


def _serial_n(noff):
    return np.repeat(np.diff(noff), np.diff(noff)).astype(np.float64)[:, None]


def _philox_noise_bar(raw64, noff):
    """|device CoM-free noise - fp64| per element: the generator's measured bar on the element and on its molecule's mean, plus the serial fp32 mean
    (n additions and a division over sum|x_i| / n) and the subtraction."""
    e = R.combined_noise(raw64, noff)
    bar = np.full(raw64.shape, PHILOX_BAR)
    bar[:, :3] = 2 * PHILOX_BAR + U * ((_serial_n(noff) + 1) * _mean_terms(raw64[:, :3], noff) + np.abs(e[:, :3]))
    return e, bar


# ================================================================================================================================================
# (a) Philox, every element
# ================================================================================================================================================
@pytest.mark.parametrize("seed", SEEDS, ids=["low", "high_word"])
@pytest.mark.parametrize("case", ["qm9", "geom"])
def test_philox_init_equals_the_reference_in_every_element(case, seed, request):
    H = request.getfixturevalue(case)
    noff = H.plan(SIZES)
    N = int(noff[-1])
    z = H.init(N, None, seed)
    raw = R.philox_table(seed, R.DRAW_INIT, N, H.D)
    want, bar = _philox_noise_bar(raw, noff)
    err = np.abs(z - want)
    _report(f"philox init {case} seed {seed:#x} h columns", err[:, 3:].max(), PHILOX_BAR)
    _report(f"philox init {case} seed {seed:#x} x columns", err[:, :3].max(), bar[:, :3].max())
    assert (err <= bar).all(), f"worst {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"
    assert np.array_equal(z[0, :3], np.zeros(3, dtype=np.float32))                 # one node: exactly 0
    # option node_base on a second plan: the rows of the flat reference from 37 on
    sub = [6, 19, 63]
    noff2 = H.plan(sub)
    H.opt("node_base", 37)
    try:
        z2 = H.init(int(noff2[-1]), None, seed)
    finally:
        H.opt("node_base", 0)
    want2, bar2 = _philox_noise_bar(R.philox_table(seed, R.DRAW_INIT, N, H.D)[37:37 + int(noff2[-1])], noff2)
    assert np.array_equal(R.philox_table(seed, R.DRAW_INIT, int(noff2[-1]), H.D, node_base=37), R.philox_table(seed, R.DRAW_INIT, N, H.D)[37:37 + int(noff2[-1])])
    err2 = np.abs(z2 - want2)
    _report(f"philox init {case} seed {seed:#x} node_base 37", err2.max(), bar2.max())
    assert (err2 <= bar2).all()


@pytest.mark.parametrize("N", [700, 1024, 1140])
def test_fix_noise_centres_by_the_whole_batch_mean(N, qm9):
    """k_noise_mean: thread i sums nodes i, i + 1024, ... (<= 2 additions for N <= 2048), a 10-level tree, one division: k = 13 on sum|x_i| / N; k_sample subtracts it
    (1 on |result|).  Tape noise: that bar alone; Philox: plus the generator's bar on the element and on the mean."""
    H = qm9
    sizes = [19] * (N // 19) + ([N % 19] if N % 19 else [])
    noff = H.plan(sizes)
    H.opt("fix_noise", 1)
    try:
        raw = _tape(N, N, H.F)
        z = H.init(N, _dev(raw), 0)
        zp = H.init(N, None, SEEDS[1])
    finally:
        H.opt("fix_noise", 0)
    for name, got, r64, gen in (("tape", z, raw.astype(np.float64), 0.0), ("philox", zp, R.philox_table(SEEDS[1], R.DRAW_INIT, N, H.D), PHILOX_BAR)):
        want = R.mode_init(None, None, r64, noff, gmean=R.noise_mean(r64))
        bar = np.full(want.shape, gen)
        bar[:, :3] = 2 * gen + U * (13 * np.abs(r64[:, :3]).mean(axis=0)[None, :] + np.abs(want[:, :3]))
        err = np.abs(got - want)
        _report(f"fix_noise N={N} {name} x columns", err[:, :3].max(), bar[:, :3].max())
        assert (err <= bar).all()
        per_mol = R.mode_init(None, None, r64, noff)
        assert np.abs(per_mol[:, :3] - want[:, :3]).max() > 1e-2               # the two centrings are far apart: the test tells them from each other
    assert np.array_equal(z[:, 3:], raw[:, 3:])


def test_packed_plan_draws_each_sub_batch_with_its_own_seed_from_node_zero(qm9):
    H = qm9
    batches = [[1, 2, 6], [19, 63], [64, 65]]
    seeds = [SEEDS[1], 5, (7 << 32) | 11]
    noff = H.plan_packed(batches, seeds)
    z = H.init(int(noff[-1]), None, 999)                                       # (the scalar seed is ignored under a packed plan)
    o = 0
    for k, b in enumerate(batches):
        n = sum(b)
        want, bar = _philox_noise_bar(R.philox_table(seeds[k], R.DRAW_INIT, n, H.D), R.offsets(b))
        err = np.abs(z[o:o + n] - want)
        _report(f"philox init packed sub-batch {k}", err.max(), bar.max())
        assert (err <= bar).all(), f"sub-batch {k}"
        o += n


def test_a_million_philox_normals_are_finite(geom):
    H = geom
    sizes = [2] * 27595                                                         # 55190 nodes x 19 columns >= 2^20 elements
    noff = H.plan(sizes)
    N = int(noff[-1])
    assert N * H.D >= 2 ** 20
    z = H.init(N, None, SEEDS[1])
    assert np.isfinite(z).all() and np.abs(z[:, 3:]).max() <= 5.9 and np.abs(z[:, :3]).max() <= 5.9 * 2
    # and every one of them equals the reference (two-node molecules: the mean is one addition and one halving, both within the generator's bar already)
    raw = R.philox_table(SEEDS[1], R.DRAW_INIT, N, H.D)
    want = raw.copy()
    want[:, :3] -= np.repeat(raw[:, :3].reshape(-1, 2, 3).mean(axis=1), 2, axis=0)
    err = np.abs(z - want)
    _report("philox 2^20 draw h columns", err[:, 3:].max(), PHILOX_BAR)
    _report("philox 2^20 draw x columns", err[:, :3].max(), 2 * PHILOX_BAR)
    assert (err[:, 3:] <= PHILOX_BAR).all() and (err[:, :3] <= 2 * PHILOX_BAR + 4 * U * np.abs(raw[:, :3])).all()


# ================================================================================================================================================
# (b) one ancestral step with the network taken out
# ================================================================================================================================================
STEPS = [(0, 1000), (1, 1000), (499, 1000), (999, 1000), (0, 400), (1, 400), (399, 400), (3, 7), (0, 1)]


def _step_refs(H, noff, z, eps_h, raw64, s_pair, n):
    """fp64 and fp32 reference of the transition s_pair = (index of s, index of t) out of n on the GPU's own eps; also sigma (fp64)"""
    g = R.gamma_pair(H.gamma, s_pair[0], s_pair[1], n)
    c64, c32 = R.step_coeffs(*g), R.step_coeffs(*g, dtype=np.float32)
    ref64 = R.mode_step(z, H.eps(eps_h, noff, np.float64), raw64, noff, c64)
    ref32 = R.mode_step(z, H.eps(eps_h, noff, np.float32), raw64, noff, c32, dtype=np.float32)
    return ref64, ref32, float(c64[2])


def _check_step(H, name, noff, z, ctx, s, n, seed=None, tape_seed=0, words=1, raw64=None):
    """gcdm_sample_step_to from z (out of place, direct launches) with tape noise (seed None) or Philox noise, against the fp64 formula."""
    N = len(z)
    t = R.step_times(s, n)[1]
    eps_h = H.eps_h(z, t, ctx, words)
    if seed is None:
        raw = _tape(tape_seed, N, H.F)
        noise, raw64, gen = _dev(raw), raw.astype(np.float64), 0.0
    else:
        noise, gen = None, 3 * PHILOX_BAR                  # the element, its molecule's noise mean, the projection's mean
        raw64 = R.philox_table(seed, R.draw_step(s), N, H.D) if raw64 is None else raw64
    z_in, z_out, fl = _dev(z), torch.full((N, H.D), float("nan"), device="cuda"), H.flags(words)
    H.step_to(z_in, z_out, ctx, s, n, noise, 0 if seed is None else seed, fl)
    ref64, ref32, sigma = _step_refs(H, noff, z, eps_h, raw64, (s, s + 1), n)
    bar, scale = _gap_bar(ref32, ref64)
    bar += sigma * gen
    err = float(np.abs(z_out.cpu().numpy() - ref64).max())
    _report(f"step {name} s={s}/{n} {'tape' if seed is None else 'philox'}", err, bar, scale)
    assert fl.cpu().tolist() == [0] * words
    assert np.array_equal(z_in.cpu().numpy(), z)          # out of place: the input is left alone
    assert err <= bar
    return z_out.cpu().numpy()


@pytest.mark.parametrize("s,n", STEPS)
@pytest.mark.parametrize("case", ["qm9", "geom"])
def test_step_arithmetic_on_the_gpus_own_eps(case, s, n, request):
    H = request.getfixturevalue(case)
    noff = H.plan(SIZES)
    z = _latent(100 + s, noff, H.D, 1.0 if s / n > 0.1 else 0.3)
    _check_step(H, case, noff, z, None, s, n, tape_seed=300 + s)
    _check_step(H, case, noff, z, None, s, n, seed=SEEDS[1])


@pytest.mark.parametrize("s,n", [(1, 400), (999, 1000)])
def test_step_arithmetic_with_a_context(s, n, qm9cond):
    H = qm9cond
    noff = H.plan(SIZES)
    z = _latent(100 + s, noff, H.D, 1.0 if s / n > 0.1 else 0.3)
    _check_step(H, "qm9cond", noff, z, H.context(noff), s, n, tape_seed=300 + s)


@pytest.mark.parametrize("case", ["qm9", "geom"])
def test_captured_step_reads_the_right_row_of_its_table(case, request):
    """In place with Philox noise = the captured step graph: s = 5, 4, 3 (the cursor steps down by itself), then a jump to s = 9 (k_cursor_set), each against the
    fp64 formula with the coefficients and the draw number of ITS step."""
    H = request.getfixturevalue(case)
    noff = H.plan(SIZES)
    N, n, seed = int(noff[-1]), 10, SEEDS[1]
    H.opt("step_graph", 1)
    before = H.lib.gcdm_get_option(H.h, b"graph_launches")
    zd, fl = _dev(_latent(7, noff, H.D, 1.0)), H.flags()
    for s in (5, 4, 3, 9):
        z = zd.cpu().numpy()
        eps_h = H.eps_h(z, R.step_times(s, n)[1], None)
        H.ok(H.lib.gcdm_sample_step(H.h, _ptr(zd), None, s, n, None, C.c_uint64(seed), _ptr(fl), H.stream))
        torch.cuda.synchronize()
        ref64, ref32, sigma = _step_refs(H, noff, z, eps_h, R.philox_table(seed, R.draw_step(s), N, H.D), (s, s + 1), n)
        bar, scale = _gap_bar(ref32, ref64)
        bar += 3 * sigma * PHILOX_BAR
        err = float(np.abs(zd.cpu().numpy() - ref64).max())
        _report(f"captured step {case} s={s}/{n}", err, bar, scale)
        assert err <= bar, f"s={s}"
    assert fl.item() == 0
    assert H.lib.gcdm_get_option(H.h, b"step_graph") == 1 and H.lib.gcdm_get_option(H.h, b"graph_launches") == before + 4, H.lib.gcdm_last_error(H.h)


def test_step_under_a_packed_plan(qm9):
    H = qm9
    batches, seeds = [[1, 2, 6, 19], [63, 64, 65]], [SEEDS[1], 5]
    noff = H.plan_packed(batches, seeds)
    N, s, n = int(noff[-1]), 499, 1000
    z = _latent(11, noff, H.D, 1.0)
    _check_step(H, "packed K=2", noff, z, None, s, n, tape_seed=12, words=2)
    raw64 = np.concatenate([R.philox_table(seeds[k], R.draw_step(s), sum(b), H.D) for k, b in enumerate(batches)])
    _check_step(H, "packed K=2", noff, z, None, s, n, seed=999, words=2, raw64=raw64)


# ================================================================================================================================================
# (c) final decode
# ================================================================================================================================================
def _final(H, noff, z, ctx, raw, cog_fix, words=1, subs=None, seed=None):
    """gcdm_sample_final on z with the tape draw `raw` -> (out, flag words, per sub-batch [(slice, fp64 Decoded, fp32 Decoded)])"""
    N = len(z)
    eps_h = H.eps_h(z, np.float32(0), ctx, words)
    H.opt("cog_fix", int(cog_fix))
    try:
        out, fl, zd, rd = torch.full((N, H.D), float("nan"), device="cuda"), H.flags(words), _dev(z), _dev(raw)
        H.ok(H.lib.gcdm_sample_final(H.h, _ptr(zd), _ptr(ctx), _ptr(rd), C.c_uint64(0), _ptr(out), _ptr(fl), H.stream))
        torch.cuda.synchronize()
    finally:
        H.opt("cog_fix", 1)
    g0 = H.gamma[R.timestep_index(np.float32(0), len(H.gamma) - 1)]
    eps64, eps32 = H.eps(eps_h, noff, np.float64), H.eps(eps_h, noff, np.float32)
    refs = []
    for sl, mol in (subs or [(slice(0, N), list(np.diff(noff)))]):                 # the drift decision is a sub-batch's own
        o = R.offsets(mol)
        refs.append((sl, R.mode_final(z[sl], eps64[sl], raw[sl].astype(np.float64), o, R.final_coeffs(g0), H.norm, cog_fix=cog_fix),
                     R.mode_final(z[sl], eps32[sl], raw[sl], o, R.final_coeffs(g0, dtype=np.float32), H.norm, dtype=np.float32, cog_fix=cog_fix)))
    return out.cpu().numpy(), fl.cpu().tolist(), refs


def _check_decoded(H, name, out, sl, r64, r32):
    """x within the gap bar; one-hot and charge identical on every row whose fp64 top-2 margin and distance to a half-integer exceed the bar of the continuous values
    (at most one row per case may be left out).  Returns the x bar."""
    T = H.norm.num_atom_types
    bar, scale = _gap_bar(r32.x, r64.x)
    bar_c, _ = _gap_bar(r32.cont, r64.cont)
    err = float(np.abs(out[sl, :3] - r64.x).max())
    _report(f"final {name} x", err, bar, scale)
    assert err <= bar
    top2 = np.sort(r64.cont[:, 3:3 + T], axis=1)
    safe = (top2[:, -1] - top2[:, -2]) > 2 * bar_c
    if H.norm.include_charges:
        safe &= np.abs(np.abs(r64.cont[:, 3 + T] - np.floor(r64.cont[:, 3 + T])) - 0.5) > bar_c
    left_out = int((~safe).sum())
    print(f"PIN final {name}: rows left out of the discrete comparison {left_out} of {len(safe)}")
    assert left_out <= 1
    assert np.array_equal(out[sl, 3:3 + T][safe], r64.one_hot[safe])
    assert (out[sl, 3:3 + T].sum(axis=1) == 1).all()
    if H.norm.include_charges:
        assert np.array_equal(out[sl, 3 + T][safe], r64.charge[safe])
    return bar


@pytest.mark.parametrize("case", ["qm9", "geom", "qm9cond"])
def test_final_decode_on_the_gpus_own_eps(case, request):
    H = request.getfixturevalue(case)
    noff = H.plan(SIZES)
    ctx = H.context(noff)
    z = _latent(9, noff, H.D, 0.3)
    out, fl, [(sl, r64, r32)] = _final(H, noff, z, ctx, _tape(77, len(z), H.F), cog_fix=True)
    assert not r64.drift and fl == [0]
    _check_decoded(H, case, out, sl, r64, r32)


# molecule 2 has 6 nodes, molecule 1 has 2: +0.01 per node puts sum x at 0.06 / alpha_0 and 0.02 / alpha_0 -- just above and below 5e-2
@pytest.mark.parametrize("cog_fix", [True, False], ids=["cog_fix", "frames"])
@pytest.mark.parametrize("mol,shift,drifts", [(3, 0.75, True), (2, 0.01, True), (1, 0.01, False)])
def test_final_decode_drift_decision_follows_the_reference(mol, shift, drifts, cog_fix, qm9):
    H = qm9
    noff = H.plan(SIZES)
    z = _latent(9, noff, H.D, 0.3)
    z[noff[mol]:noff[mol + 1], 0] += np.float32(shift)
    out, fl, [(sl, r64, r32)] = _final(H, noff, z, None, _tape(77, len(z), H.F), cog_fix=cog_fix)
    assert r64.drift == drifts and r32.drift == drifts
    bar = _check_decoded(H, f"drift mol {mol} +{shift} cog_fix={int(cog_fix)}", out, sl, r64, r32)
    assert (np.abs(r64.cog - 5e-2) > 65 * bar).all()                           # (condition) no molecule's sum of <= 65 positions sits on the threshold
    # the flag is k_cog_fix's report; with cog_fix off (chain frames) nothing is re-projected and nothing reported
    assert fl == [native.FLAG_COG_DRIFT if (drifts and cog_fix) else 0]
    sums = np.array([np.abs(out[noff[b]:noff[b + 1], :3].astype(np.float64).sum(axis=0)).max() for b in range(len(noff) - 1)])
    if drifts and cog_fix:
        assert sums.max() <= 65 * bar                                          # EVERY molecule re-centred
    else:
        assert np.abs(sums - r64.cog).max() <= 65 * bar and (sums.max() > 5e-2) == drifts


def test_final_decode_drift_is_a_sub_batchs_own_decision(qm9):
    H = qm9
    batches = [[1, 2, 6, 19], [63, 6, 65]]
    noff = H.plan_packed(batches, [1, 2])
    z = _latent(9, noff, H.D, 0.3)
    z[noff[5]:noff[6], 0] += np.float32(0.75)                                  # a molecule of sub-batch 1
    subs = [(slice(0, 28), batches[0]), (slice(28, 28 + 134), batches[1])]
    out, fl, refs = _final(H, noff, z, None, _tape(78, len(z), H.F), cog_fix=True, words=2, subs=subs)
    assert [r[1].drift for r in refs] == [False, True] and fl == [0, native.FLAG_COG_DRIFT]
    bars = [_check_decoded(H, f"packed sub-batch {k}", out, sl, r64, r32) for k, (sl, r64, r32) in enumerate(refs)]
    assert np.abs(out[28:28 + 63, :3].astype(np.float64).sum(axis=0)).max() <= 63 * bars[1]            # sub-batch 1: every molecule re-centred ...
    assert abs(np.abs(out[9:28, :3].astype(np.float64).sum(axis=0)).max() - refs[0][1].cog[3]) <= 19 * bars[0]      # ... sub-batch 0 left as decoded


# ================================================================================================================================================
# (d) the network-free entry points
# ================================================================================================================================================
def _molecule(H, noff, seed):
    """[x | one-hot | charge] of a made-up molecule, positions centred per molecule (fp32)"""
    N, T = int(noff[-1]), H.norm.num_atom_types
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((N, 3), generator=g) * 1.5).numpy()
    x -= R.mol_mean(x, noff, np.float32)
    oh = torch.nn.functional.one_hot(torch.randint(0, T, (N,), generator=g), T).float().numpy()
    parts = [x, oh] + ([torch.randint(0, 9, (N, 1), generator=g).float().numpy()] if H.norm.include_charges else [])
    return np.concatenate(parts, axis=1)


@pytest.mark.parametrize("case", ["qm9", "geom", "qm9cond"])
def test_encode_and_unnormalize(case, request):
    """k_encode: x / nv0 is one division (k = 1 on |x / nv0|), (h - nb) / nv a subtraction and a division (k = 2 on (|h| + |nb|) / nv).
    k_unnormalize: x * nv0 (k = 1), h * nv + nb (k = 2 on |h nv| + |nb|)."""
    H = request.getfixturevalue(case)
    noff = H.plan(SIZES)
    nv, nb, T = H.norm.values, H.norm.biases, H.norm.num_atom_types
    col_nv = np.array([nv[0]] * 3 + [nv[1]] * T + [nv[2]] * (H.D - 3 - T))
    col_nb = np.array([0.0] * 3 + [nb[1]] * T + [nb[2]] * (H.D - 3 - T))
    for shift, flag in ((0.0, 0), (0.5, native.FLAG_MEAN_NOT_ZERO)):
        xh = _molecule(H, noff, 21)
        xh[noff[3]:noff[4], 1] += np.float32(shift)
        z, fl, xd = torch.full(xh.shape, float("nan"), device="cuda"), H.flags(), _dev(xh)
        H.ok(H.lib.gcdm_encode_samples(H.h, _ptr(xd), _ptr(z), _ptr(fl), H.stream))
        torch.cuda.synchronize()
        want = R.encode(xh, H.norm)
        bar = U * 2 * (np.abs(xh) + np.abs(col_nb)[None, :]) / col_nv[None, :]
        bar[:, :3] /= 2
        err = np.abs(z.cpu().numpy() - want)
        _report(f"encode {case} shift {shift}", err.max(), bar.max())
        assert (err <= bar).all()
        assert (R.mean_zero_error(want[:, :3], noff) >= 1e-2) == bool(flag) and fl.item() == flag
    zl = _latent(5, noff, H.D, 1.0)
    out, zd = torch.full(zl.shape, float("nan"), device="cuda"), _dev(zl)
    H.ok(H.lib.gcdm_unnormalize_z(H.h, _ptr(zd), _ptr(out), H.stream))
    torch.cuda.synchronize()
    want = R.unnormalize(zl, H.norm)
    bar = U * 2 * (np.abs(zl) * col_nv[None, :] + np.abs(col_nb)[None, :])
    bar[:, :3] /= 2
    err = np.abs(out.cpu().numpy() - want)
    _report(f"unnormalize {case}", err.max(), bar.max())
    assert (err <= bar).all()


def _fixed_patterns(noff):
    N = int(noff[-1])
    mixed = torch.rand(N, generator=torch.Generator().manual_seed(4)) < 0.4
    mixed = mixed.numpy()
    mixed[noff[3]:noff[4]] = False                # a molecule generated freely
    mixed[noff[4]:noff[5]] = True                 # a molecule kept whole
    mixed[0] = True
    return dict(none=np.zeros(N, dtype=bool), all=np.ones(N, dtype=bool), mixed=mixed)


@pytest.mark.parametrize("pattern", ["none", "all", "mixed"])
def test_inpaint_center(pattern, qm9):
    """k_inpaint_center: the mean over a molecule's m fixed nodes is m - 1 additions (per-lane partial sums, then a shuffle tree: never more than the serial sum's),
    one reciprocal and one product: k = m + 1 on sum|x_i| / m; the subtraction is 1 on |result|."""
    H = qm9
    noff = H.plan(SIZES)
    fixed = _fixed_patterns(noff)[pattern]
    xh = _molecule(H, noff, 22)
    xh[:, :3] += np.array([0.3, -2.0, 1.0], dtype=np.float32)
    out, xd, fd = torch.full(xh.shape, float("nan"), device="cuda"), _dev(xh), torch.from_numpy(fixed.astype(np.uint8)).cuda()
    H.ok(H.lib.gcdm_inpaint_center(H.h, _ptr(xd), _ptr(fd), _ptr(out), H.stream))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    want = R.inpaint_center(xh, fixed, noff)
    m = np.repeat([max(1, int(fixed[noff[b]:noff[b + 1]].sum())) for b in range(len(noff) - 1)], np.diff(noff)).astype(np.float64)[:, None]
    bar = U * ((m + 1) * R.fixed_mean(np.abs(xh[:, :3]).astype(np.float64), fixed, noff) + np.abs(want[:, :3]))
    err = np.abs(out[:, :3] - want[:, :3])
    _report(f"inpaint_center fixed={pattern}", err.max(), bar.max())
    assert (err <= bar).all() and np.array_equal(out[:, 3:], xh[:, 3:])
    if pattern == "none":
        assert np.array_equal(out, xh)


def _coef_rel(c32, c64):
    """relative uncertainty of host-side fp32 coefficients: the project's rule applied to the coefficient alone"""
    return [4 * abs(float(a) - float(b)) / abs(float(b)) + 4 * U if b != 0 else 0.0 for a, b in zip(c32, c64)]


@pytest.mark.parametrize("s,t,n", [(0, 1, 6), (2, 4, 6), (5, 6, 6), (1, 400, 400)])
def test_inpaint_jump(s, t, n, qm9):
    """k_sample mode 4, v = alpha z + sigma e, then the projection.  Before the projection, per element: the subtraction that makes e, two products and a sum (k = 3 on
    |alpha z| + |sigma e|); alpha and sigma are fp32 host values with a relative uncertainty of 4 |c32 - c64| / |c64| + 4 * 2^-24 each (the reference's own gap) on
    their terms; e's x columns carry the serial noise mean over n nodes (k = n + 1 on sigma sum|raw_i| / n).  The projection adds the molecule's mean of those
    element bars, its own serial mean (k = n + 1 on sum|v_i| / n) and a subtraction (1 on |result|).  Philox: sigma * the generator's bar on the element and on
    the noise mean."""
    H = qm9
    noff = H.plan(SIZES)
    N = int(noff[-1])
    g = R.gamma_pair(H.gamma, s, t, n)
    c64, c32 = R.jump_coeffs(*g), R.jump_coeffs(*g, dtype=np.float32)
    ra, rs = _coef_rel(c32, c64)
    z = _latent(31 + s, noff, H.D, 0.7)
    nser = _serial_n(noff)
    for seed in (None, SEEDS[1]):
        raw64 = _tape(32 + s, N, H.F).astype(np.float64) if seed is None else R.philox_table(seed, 12345, N, H.D)
        zd, rd = _dev(z), None if seed is not None else _dev(raw64)
        H.ok(H.lib.gcdm_inpaint_jump(H.h, _ptr(zd), s, t, n, _ptr(rd), C.c_uint64(seed or 0), C.c_uint32(12345), H.stream))
        torch.cuda.synchronize()
        want = R.mode_jump(z, None, raw64, noff, c64)
        v64 = R.mode_noising(z, None, raw64, noff, c64)
        gen = 0.0 if seed is None else float(c64[1]) * PHILOX_BAR
        ta, ts = np.abs(c64[0] * z), np.abs(c64[1] * R.combined_noise(raw64, noff))
        eb = U * 3 * (ta + ts) + ra * ta + rs * ts + gen
        eb[:, :3] += float(c64[1]) * U * (nser + 1) * _mean_terms(raw64[:, :3], noff) + gen
        bar = eb.copy()
        bar[:, :3] += _mean_terms(eb[:, :3], noff) + U * ((nser + 1) * _mean_terms(v64[:, :3], noff) + np.abs(want[:, :3]))
        err = np.abs(zd.cpu().numpy() - want)
        _report(f"inpaint_jump {s}->{t}/{n} {'tape' if seed is None else 'philox'}", err.max(), bar.max())
        assert (err <= bar).all(), f"worst {err.max():.3e} against {bar[np.unravel_index(err.argmax(), err.shape)]:.3e}"


# ================================================================================================================================================
# (e) gcdm_inpaint_step
# ================================================================================================================================================
def _inpaint_step(H, z, xh0, fixed, s, n, nk, nu, seed, draw_base):
    zd, fl, xd, fd = _dev(z), H.flags(), _dev(xh0), torch.from_numpy(fixed.astype(np.uint8)).cuda()
    H.ok(H.lib.gcdm_inpaint_step(H.h, _ptr(zd), _ptr(xd), _ptr(fd), None, 0, None, s, n,
                                 _ptr(nk), _ptr(nu), None, C.c_uint64(seed), C.c_uint32(draw_base), _ptr(fl), H.stream))
    torch.cuda.synchronize()
    assert fl.item() == 0
    return zd.cpu().numpy()


@pytest.mark.parametrize("s,n", [(2, 6), (399, 400)])
def test_inpaint_step_three_ways(s, n, qm9):
    """fixed all true: h columns = alpha_s xh0 + sigma_s noise_known -- alpha_s, sigma_s = sqrt(sigmoid(-+gamma_s)) are exp, sum, quotient, root on the host (k = 4, relative),
    the kernel adds two products and a sum: k = 7 on |alpha_s xh0| + |sigma_s noise|; x columns = the noised known part moved by CoM(z_unknown) - CoM(z_known), within the
    gap bar.  fixed all false: bitwise gcdm_sample_step_to with the same noise_unknown.  Mixed: the combine formula on the two."""
    H = qm9
    noff = H.plan(SIZES)
    N = int(noff[-1])
    pats = _fixed_patterns(noff)
    z = _latent(41, noff, H.D, 0.8)
    xh0 = _molecule(H, noff, 42)
    rk, ru = _tape(43, N, H.F), _tape(44, N, H.F)
    nk, nu = _dev(rk), _dev(ru)
    t = R.step_times(s, n)[1]
    # the model step alone (the unknown part), and its references on the GPU's own eps
    eps_h = H.eps_h(z, t, None)
    zu_gpu, fl = torch.full((N, H.D), float("nan"), device="cuda"), H.flags()
    H.step_to(_dev(z), zu_gpu, None, s, n, nu, 0, fl)
    zu_gpu = zu_gpu.cpu().numpy()
    zu64, zu32, _ = _step_refs(H, noff, z, eps_h, ru.astype(np.float64), (s, s + 1), n)
    gs = R.gamma_pair(H.gamma, s, s, n)[0]
    a64, a32 = R.noising_coeffs(gs), R.noising_coeffs(gs, dtype=np.float32)
    zk64, zk32 = R.mode_noising(xh0, None, rk.astype(np.float64), noff, a64), R.mode_noising(xh0, None, rk, noff, a32, dtype=np.float32)
    h_bar = 7 * U * (np.abs(a64[0] * xh0[:, 3:]) + np.abs(a64[1] * rk[:, 3:].astype(np.float64)))
    for name in ("all", "none", "mixed"):
        fixed = pats[name]
        got = _inpaint_step(H, z, xh0, fixed, s, n, nk, nu, 0, 100)
        assert np.array_equal(got[~fixed].view(np.int32), zu_gpu[~fixed].view(np.int32)), name          # free nodes: the model step's bits
        want64, want32 = R.inpaint_combine(zk64, zu64, fixed, noff), R.inpaint_combine(zk32, zu32, fixed, noff, dtype=np.float32)
        err_h = np.abs(got[fixed, 3:] - want64[fixed, 3:])
        if fixed.any():
            _report(f"inpaint_step s={s}/{n} fixed={name} h columns", err_h.max(), h_bar[fixed].max())
            assert (err_h <= h_bar[fixed]).all()
        bar, scale = _gap_bar(want32[:, :3], want64[:, :3])
        err = float(np.abs(got[:, :3] - want64[:, :3]).max())
        _report(f"inpaint_step s={s}/{n} fixed={name} x columns", err, bar, scale)
        assert err <= bar
    # Philox: draw_base serves the known part, draw_base + 1 the model step
    seed, base = SEEDS[1], s - 1
    got = _inpaint_step(H, z, xh0, pats["all"], s, n, None, None, seed, base)
    known = a64[1] * R.philox_table(seed, R.draws_inpaint(base)[0], N, H.D)[:, 3:]
    want_h = a64[0] * xh0[:, 3:] + known
    bar_h = 7 * U * (np.abs(a64[0] * xh0[:, 3:]) + np.abs(known)) + float(a64[1]) * PHILOX_BAR
    err_h = np.abs(got[:, 3:] - want_h)
    _report(f"inpaint_step s={s}/{n} philox known part h columns", err_h.max(), bar_h.max())
    assert (err_h <= bar_h).all()
    # draw_base + 1 == s: the free-running step's own draw
    free = _inpaint_step(H, z, xh0, pats["none"], s, n, None, None, seed, base)
    direct, fl = torch.full((N, H.D), float("nan"), device="cuda"), H.flags()
    H.step_to(_dev(z), direct, None, s, n, None, seed, fl)
    assert np.array_equal(free.view(np.int32), direct.cpu().numpy().view(np.int32))


# ================================================================================================================================================
# (f) self-conditioned step: the second transition is a jump from s to 0 with its own draw number
# ================================================================================================================================================
@pytest.mark.parametrize("s,n", [(5, 10), (999, 1000), (0, 10)])
def test_self_conditioning_estimate_of_a_step(s, n, qm9sc):
    """gcdm_sample_step_sc leaves z_s in z and p(z_0 | z_s) in self_cond; the estimate's network call has no self-conditioning input, which is what gcdm_forward gives on a
    self-conditioning handle, and its velocities are those of the handle's last forward."""
    H = qm9sc
    noff = H.plan(SIZES)
    N, seed = int(noff[-1]), SEEDS[1]
    z0 = _latent(51 + s, noff, H.D, 1.0 if s / n > 0.1 else 0.3)
    raw = _dev(_tape(52, N, H.F))
    for philox in (False, True):
        zd, sc, fl = _dev(z0), torch.full((N, H.D), float("nan"), device="cuda"), H.flags()
        raw_sc = _tape(53, N, H.F)
        rd = None if philox else _dev(raw_sc)
        H.ok(H.lib.gcdm_sample_step_sc(H.h, _ptr(zd), _ptr(sc), 0, None, s, n, _ptr(raw), _ptr(rd), C.c_uint64(seed), _ptr(fl), H.stream))
        torch.cuda.synchronize()
        vel = H.vel(N)
        z_s = zd.cpu().numpy()
        eps_h = H.eps_h(z_s, R.step_times(s, n)[0], None)
        raw64 = R.philox_table(seed, R.draw_self_cond(s), N, H.D) if philox else raw_sc.astype(np.float64)
        g = R.gamma_pair(H.gamma, 0, s, n)
        c64, c32 = R.step_coeffs(*g), R.step_coeffs(*g, dtype=np.float32)
        e64 = np.concatenate((R.eps_from_vel(vel, noff), eps_h.astype(np.float64)), axis=1)
        e32 = np.concatenate((R.eps_from_vel(vel, noff, np.float32), eps_h), axis=1)
        ref64, ref32 = R.mode_step(z_s, e64, raw64, noff, c64), R.mode_step(z_s, e32, raw64, noff, c32, dtype=np.float32)
        bar, scale = _gap_bar(ref32, ref64)
        bar += 3 * float(c64[2]) * PHILOX_BAR if philox else 0.0
        err = float(np.abs(sc.cpu().numpy() - ref64).max())
        _report(f"self-conditioning estimate s={s}/{n} {'philox' if philox else 'tape'}", err, bar, scale)
        assert fl.item() == 0 and err <= bar
