"""Plain numpy reference of the sampler's noise and step arithmetic (no torch, no kernel code).

Written from the reference's formulas (src/models/components/variational_diffusion.py: gamma lookup :252-255, sigma / alpha :318-367,
CoM-free noise :396-420 and :795-819, normalize / unnormalize :702-792, sample_p_xh_given_z0 :840-907, compute_noised_representation :910-931,
sample_p_zt_given_zs :1163-1201, sample_p_zs_given_zt :1204-1278, CoG re-projection :1389-1402, inpaint :1625-1702) and from the generator contract
documented in include/gcdm_hip.h (Philox4x32-10 as published by Salmon et al. / Random123, Box-Muller on two 24-bit uniforms).

Every arithmetic function takes ``dtype``: np.float64 is the truth; np.float32 evaluates the reference's torch order of operations in fp32 (softplus
with threshold 20, logsigmoid, expm1; sequential sums), so that |ref32 - ref64| is the reference's own rounding gap for the very inputs of a test.
"""
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

# ---- draw numbers of the entry points (include/gcdm_hip.h, "On-device noise") ------------------------------------------------------------------
DRAW_INIT = 0x7FFFFFFF
DRAW_FINAL = 0x7FFFFFFE
DRAW_SELF_COND = 0x20000000          # | s_index
COUNTER_TAG = 0x6C078965             # word 3 of every counter


def draw_step(s_index: int) -> int:
    return s_index


def draw_self_cond(s_index: int) -> int:
    return DRAW_SELF_COND | s_index


def draws_inpaint(draw_base: int):
    """(known part, model step, self-conditioning estimate)"""
    return draw_base, draw_base + 1, draw_base + 2


# ---- Philox4x32-10 -----------------------------------------------------------------------------------------------------------------------------
_M0, _M1 = 0xD2511F53, 0xCD9E8D57        # multipliers
_W0, _W1 = 0x9E3779B9, 0xBB67AE85        # Weyl increments of the key (golden ratio, sqrt(3) - 1)
_MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Ten rounds on counter[4], key[2]: Python integers, or uint64 numpy arrays holding 32-bit values (broadcast against each other).  Returns four words
    in counter order."""
    if all(isinstance(v, int) for v in (*counter, *key)):
        cast = int
    else:
        cast = lambda v: np.asarray(v, dtype=np.uint64)              # noqa: E731
    c0, c1, c2, c3 = (cast(v) for v in counter)
    k0, k1 = (cast(v) for v in key)
    m0, m1, w0, w1, mask, sh = (cast(v) for v in (_M0, _M1, _W0, _W1, _MASK, 32))
    for rnd in range(10):
        if rnd:
            k0, k1 = (k0 + w0) & mask, (k1 + w1) & mask
        p0, p1 = m0 * c0, m1 * c2                        # 32 x 32 -> 64 bit products
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & mask, (p0 >> sh) ^ c3 ^ k1, p0 & mask
    return c0, c1, c2, c3


def uniform24(w):
    """((w >> 8) + 0.5) * 2^-24 EVALUATED IN fp32 -- part of the generator's definition: from w >> 8 = 2^23 on the + 0.5 rounds away (ties to even), and
    w >> 8 = 2^24 - 1 gives exactly 1.0."""
    m = np.asarray(w, dtype=np.uint64) >> np.uint64(8)
    return (m.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def box_muller(w0, w1, col):
    """Standard normal from two output words: fp32 uniforms, then fp64 throughout; even col takes the cosine lane, odd col the sine lane."""
    u1, u2 = uniform24(w0).astype(np.float64), uniform24(w1).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return np.where(np.asarray(col, dtype=np.uint64) & np.uint64(1), r * np.sin(ang), r * np.cos(ang))


def philox_normal(seed, draw, node, col):
    """Entry (node, col) of draw `draw` under `seed`; node and col may be arrays (broadcast).  fp64."""
    node = np.asarray(node, dtype=np.uint64) & np.uint64(_MASK)
    col = np.asarray(col, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = (node, np.uint64(int(draw) & _MASK), col >> np.uint64(1), np.uint64(COUNTER_TAG))
    key = (np.uint64(seed & _MASK), np.uint64(seed >> 32))
    w = philox4x32_10(ctr, key)
    return box_muller(w[0], w[1], col)


def philox_table(seed, draw, N, D, node_base=0):
    """[N, D] raw draw: row i is node node_base + i."""
    return philox_normal(seed, draw, (np.arange(N, dtype=np.uint64) + np.uint64(node_base))[:, None], np.arange(D, dtype=np.uint64)[None, :])


# ---- schedule -----------------------------------------------------------------------------------------------------------------------------------
def timestep_index(t, T):
    """round-half-even(float32(t) * T) in fp32, clamped to [0, T] (torch.round(t * timesteps).long(), :252-255)."""
    v = np.rint(np.float32(t) * np.float32(T))
    return int(min(max(v, 0), T))


def step_times(s_index, num_steps):
    """(s, t) of the step at s_index, as fp32 quotients of fp32 integers."""
    n = np.float32(num_steps)
    return np.float32(s_index) / n, np.float32(s_index + 1) / n


def gamma_pair(gamma, s_index, t_index, num_steps):
    """gamma at s_index / num_steps and t_index / num_steps from the fp32 table the handle was given (T = len - 1)."""
    T = len(gamma) - 1
    n = np.float32(num_steps)
    return (gamma[timestep_index(np.float32(s_index) / n, T)], gamma[timestep_index(np.float32(t_index) / n, T)])


def _softplus(x, dt):
    x = dt(x)
    return x if x > 20 else np.log1p(np.exp(x))          # torch F.softplus, threshold 20


def _logsigmoid(x, dt):
    x = dt(x)
    return min(x, dt(0)) - np.log1p(np.exp(-abs(x)))     # torch F.logsigmoid


def _sigmoid(x, dt):
    return dt(1) / (dt(1) + np.exp(-dt(x)))


def _sigma2_alpha_ts(gs, gt, dt):
    """sigma_and_alpha_t_given_s (:342-367)."""
    s2 = -np.expm1(_softplus(gs, dt) - _softplus(gt, dt))
    a = np.exp(dt(0.5) * (_logsigmoid(-dt(gt), dt) - _logsigmoid(-dt(gs), dt)))
    return s2, a


def step_coeffs(gs, gt, dtype=np.float64):
    """(alpha_ts, c_eps, sigma) of z_s = z_t / alpha_ts - c_eps * eps + sigma * noise (:1247-1263)."""
    dt = dtype
    s2, a = _sigma2_alpha_ts(gs, gt, dt)
    sig_s, sig_t = np.sqrt(_sigmoid(gs, dt)), np.sqrt(_sigmoid(gt, dt))
    return a, s2 / a / sig_t, np.sqrt(s2) * sig_s / sig_t


def final_coeffs(g0, dtype=np.float64):
    """(1 / alpha_0, sigma_0, sigma_x) of xh = 1 / alpha_0 * (z_0 - sigma_0 * eps) + sigma_x * noise (:855-886); sigma_x = SNR(-0.5 gamma_0)."""
    dt = dtype
    return dt(1) / np.sqrt(_sigmoid(-dt(g0), dt)), np.sqrt(_sigmoid(g0, dt)), np.exp(dt(0.5) * dt(g0))


def noising_coeffs(gs, dtype=np.float64):
    """(alpha_s, sigma_s) of q(z_s | x, h) (:910-931)."""
    dt = dtype
    return np.sqrt(_sigmoid(-dt(gs), dt)), np.sqrt(_sigmoid(gs, dt))


def jump_coeffs(gs, gt, dtype=np.float64):
    """(alpha_ts, sigma_ts) of q(z_t | z_s) (:1163-1201)."""
    s2, a = _sigma2_alpha_ts(gs, gt, dtype)
    return a, np.sqrt(s2)


# ---- per-molecule means ---------------------------------------------------------------------------------------------------------------------------
def offsets(num_nodes: Sequence[int]) -> np.ndarray:
    return np.concatenate(([0], np.cumsum(np.asarray(num_nodes, dtype=np.int64))))


def _colsum(a, dt):
    """Column sums of a [n, k] block: sequential in fp32 (what a scatter-add does), numpy's in fp64."""
    a = a.astype(dt)
    return a.sum(axis=0) if dt is np.float64 else np.cumsum(a, axis=0, dtype=dt)[-1]


def mol_mean(x, noff, dtype=np.float64):
    """Per-node copy of its molecule's mean of x [N, k]."""
    out = np.empty(x.shape, dtype=dtype)
    for b in range(len(noff) - 1):
        o, e = noff[b], noff[b + 1]
        out[o:e] = _colsum(x[o:e], dtype) / dtype(e - o)
    return out


def noise_mean(raw, dtype=np.float64):
    """fix_noise (:832-834, 1323-1325): the mean of the x-part of one raw draw over the WHOLE flat batch, [3]."""
    return _colsum(raw[:, :3], dtype) / dtype(raw.shape[0])


def combined_noise(raw, noff, gmean=None, dtype=np.float64):
    """sample_combined_gaussian noise (:795-819): x-part CoM-free per molecule (or by `gmean`, the whole-batch mean), h-part as drawn."""
    e = raw.astype(dtype).copy()
    e[:, :3] -= mol_mean(e[:, :3], noff, dtype) if gmean is None else np.asarray(gmean, dtype=dtype)[None, :]
    return e


def project(v, noff, dtype=np.float64):
    """x columns back to zero CoM per molecule."""
    v = v.copy()
    v[:, :3] -= mol_mean(v[:, :3], noff, dtype)
    return v


def eps_from_vel(vel, noff, dtype=np.float64):
    """x columns of eps from the network's velocities [3, N]: vel minus its molecule's mean (gcpnet.py:1206-1211)."""
    v = np.ascontiguousarray(vel.T).astype(dtype)
    return v - mol_mean(v, noff, dtype)


# ---- the five modes ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Norm:
    """normalisation constants of a configuration (diffusion_cfg.norm_values / norm_biases)."""
    num_atom_types: int
    include_charges: bool
    values: Sequence[float] = (1.0, 4.0, 10.0)
    biases: Sequence[float] = (0.0, 0.0, 0.0)


def mode_init(z, eps, raw_noise, noff, coeffs=None, gmean=None, dtype=np.float64):
    """z_T: CoM-free noise."""
    return combined_noise(raw_noise, noff, gmean, dtype)


def mode_step(z, eps, raw_noise, noff, coeffs, gmean=None, dtype=np.float64):
    """z / alpha - c * eps + sigma * e, x projected to zero CoM."""
    dt = dtype
    a, c, sg = (dt(v) for v in coeffs)
    e = combined_noise(raw_noise, noff, gmean, dt)
    return project(z.astype(dt) / a - c * eps.astype(dt) + sg * e, noff, dt)


def mode_noising(z, eps, raw_noise, noff, coeffs, gmean=None, dtype=np.float64):
    """alpha * z + sigma * e (forward noising of a given molecule)."""
    dt = dtype
    a, sg = (dt(v) for v in coeffs)
    return a * z.astype(dt) + sg * combined_noise(raw_noise, noff, gmean, dt)


def mode_jump(z, eps, raw_noise, noff, coeffs, gmean=None, dtype=np.float64):
    """forward noising z_s -> z_t, x projected to zero CoM."""
    return project(mode_noising(z, eps, raw_noise, noff, coeffs, gmean, dtype), noff, dtype)


def unnormalize(z, norm: Norm, dtype=np.float64):
    """[x * nv0 | h_cat * nv1 + nb1 | h_int * nv2 + nb2], continuous."""
    dt = dtype
    z = z.astype(dt)
    F = norm.num_atom_types
    out = np.empty_like(z)
    out[:, :3] = z[:, :3] * dt(norm.values[0])
    out[:, 3:3 + F] = z[:, 3:3 + F] * dt(norm.values[1]) + dt(norm.biases[1])
    out[:, 3 + F:] = z[:, 3 + F:] * dt(norm.values[2]) + dt(norm.biases[2])
    return out


def encode(xh, norm: Norm, dtype=np.float64):
    """normalize (:702-732): [x / nv0 | (one_hot - nb1) / nv1 | (charge - nb2) / nv2]."""
    dt = dtype
    xh = xh.astype(dt)
    F = norm.num_atom_types
    out = np.empty_like(xh)
    out[:, :3] = xh[:, :3] / dt(norm.values[0])
    out[:, 3:3 + F] = (xh[:, 3:3 + F] - dt(norm.biases[1])) / dt(norm.values[1])
    out[:, 3 + F:] = (xh[:, 3 + F:] - dt(norm.biases[2])) / dt(norm.values[2])
    return out


def mean_zero_error(zx, noff):
    """assert_mean_zero_with_mask (:465-474): max_b |sum_i x| / (max |x| + 1e-10); the reference asserts < 1e-2."""
    zx = zx.astype(np.float64)
    sums = np.stack([zx[noff[b]:noff[b + 1]].sum(axis=0) for b in range(len(noff) - 1)])
    return np.abs(sums).max() / (np.abs(zx).max() + 1e-10)


@dataclass
class Decoded:
    x: np.ndarray            # [N,3] un-normalised positions, re-projected where the decision says so
    cont: np.ndarray         # [N,3+F] un-normalised continuous values before argmax / rounding / re-projection
    one_hot: np.ndarray      # [N,T]
    charge: Optional[np.ndarray]   # [N] rounded (half to even), or None
    drift: bool              # any molecule with max |sum_i x| > 5e-2
    cog: np.ndarray          # [B] max |sum_i x| per molecule


def mode_final(z, eps, raw_noise, noff, coeffs, norm: Norm, gmean=None, dtype=np.float64, cog_fix=True) -> Decoded:
    """alpha (z - c eps) + sigma e, unnormalize, argmax one-hot, rounded charge; drift decision per molecule, re-projection of the whole batch if any drifted."""
    dt = dtype
    a, c, sg = (dt(v) for v in coeffs)
    xh = a * (z.astype(dt) - c * eps.astype(dt)) + sg * combined_noise(raw_noise, noff, gmean, dt)
    cont = unnormalize(xh, norm, dt)
    T = norm.num_atom_types
    one_hot = np.zeros((len(cont), T), dtype=dt)
    one_hot[np.arange(len(cont)), np.argmax(cont[:, 3:3 + T], axis=1)] = 1
    charge = np.rint(cont[:, 3 + T]) if norm.include_charges else None
    cog = np.array([np.abs(_colsum(cont[noff[b]:noff[b + 1], :3], dt)).max() for b in range(len(noff) - 1)])
    drift = bool((cog > 5e-2).any())
    x = cont[:, :3].copy()
    if drift and cog_fix:
        x -= mol_mean(x, noff, dt)
    return Decoded(x, cont, one_hot, charge, drift, cog)


# ---- inpainting -------------------------------------------------------------------------------------------------------------------------------------
def fixed_mean(x, fixed, noff, dtype=np.float64):
    """Per-node copy of the mean of x over its molecule's FIXED nodes (0 where it has none)."""
    out = np.zeros(x.shape, dtype=dtype)
    for b in range(len(noff) - 1):
        o, e = noff[b], noff[b + 1]
        sel = np.asarray(fixed[o:e], dtype=bool)
        if sel.any():
            out[o:e] = _colsum(x[o:e][sel], dtype) / dtype(sel.sum())
    return out


def inpaint_center(xh, fixed, noff, dtype=np.float64):
    """The given molecule shifted so that its fixed nodes have zero CoM (:1625-1633); features untouched."""
    out = xh.astype(dtype).copy()
    out[:, :3] -= fixed_mean(out[:, :3], fixed, noff, dtype)
    return out


def inpaint_combine(zk, zu, fixed, noff, dtype=np.float64):
    """fixed ? z_known + CoM_fixed(z_unknown) - CoM_fixed(z_known) : z_unknown (:1678-1702)."""
    zk, zu = zk.astype(dtype), zu.astype(dtype)
    moved = zk.copy()
    moved[:, :3] += fixed_mean(zu[:, :3], fixed, noff, dtype) - fixed_mean(zk[:, :3], fixed, noff, dtype)
    return np.where(np.asarray(fixed, dtype=bool)[:, None], moved, zu)
