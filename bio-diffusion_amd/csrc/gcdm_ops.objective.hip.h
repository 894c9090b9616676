// gcdm_ops.objective.hip.h -- the diffusion objective around the network evaluation (variational_diffusion.py:948-1160 and the tail of
// qm9_mol_gen_ddpm.py:184-252) as three launches forward and one backward.  C ABI and every formula: include/gcdm_objective.h.
//
//   k_obj_prepare  one wave per molecule: normalise, gamma look-ups, CoM projection of the noise, z_t (z_0), the terms that need no network
//   k_obj_terms    one wave per molecule: error_t, loss_0_x, loss_0_h (four erff per atom type, logsumexp), the eps_hat statistics
//   k_obj_reduce   one workgroup: nll per molecule, the batch means, d nll / d (error_t, loss_0_x) for the backward
//   k_obj_bwd      one wave per molecule, element-wise: d net_out
//
// Plain fp32, contraction off so that every operation rounds as the torch expression it restates; no float atomics and no scratch (the
// per-type log masses live in a fully unrolled register array).  Per-molecule sums: lane l adds rows l, l + 64, ... in order, then a fixed
// butterfly -- the order depends on the molecule's size alone.
#pragma once

namespace gobj {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAXF = 16;                 // GCDM_OBJECTIVE_MAX_TYPES

struct Norm { float nv0, nv1, nv2, nb1, nb2, log_nv0; };

__device__ inline float wave_sum(float x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ inline float sigmoidf(float g) {
#pragma clang fp contract(off)
    return 1.f / (1.f + expf(-g));
}
__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// rint(t / T * T) in fp32 as PredefinedNoiseSchedule.forward computes it; a negative index wraps as Python's does
__device__ inline int gamma_index(int t, int T) {
#pragma clang fp contract(off)
    const float f = (float)t / (float)T;
    int i = (int)rintf(f * (float)T);
    if (i < 0) i += T + 1;
    return clampi(i, 0, T);
}

struct PrepArgs {
    const float* x; const float* one_hot; const float* charges; const uint8_t* mask; const int32_t* off; const int32_t* t_int;
    const float* gamma; const float* log_pn; const float* eps_raw; const float* eps_raw0;
    float* xh; float* eps_t; float* z_t; float* eps_0; float* z_0; float* t_node; float* mol; int32_t* flags;
    int32_t N, B, D, nf, ic, T, pn_len, eval, center_x;
    Norm nm;
};

__global__ void __launch_bounds__(THREADS) k_obj_prepare(PrepArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const int o0 = clampi(a.off[b], 0, a.N), o1 = clampi(a.off[b + 1], 0, a.N);
    const int D = a.D, nf = a.nf;
    int fl = 0;
    int t = a.t_int[b];
    if (t < 0 || t > a.T) { fl |= 4; t = clampi(t, 0, a.T); }
    const float g_t = a.gamma[gamma_index(t, a.T)], g_s = a.gamma[gamma_index(t - 1, a.T)];
    const float g_T = a.gamma[a.T], g_0 = a.gamma[0];
    const float al_t = sqrtf(sigmoidf(-g_t)), si_t = sqrtf(sigmoidf(g_t));
    const float al_0 = sqrtf(sigmoidf(-g_0)), si_0 = sqrtf(sigmoidf(g_0));
    const float al_T = sqrtf(sigmoidf(-g_T)), si_T = sqrtf(sigmoidf(g_T));
    const float tf = (float)t / (float)a.T;

    // pass 1: the molecule's sums
    float cnt = 0.f, sx[3] = {0.f, 0.f, 0.f}, se[3] = {0.f, 0.f, 0.f}, s0[3] = {0.f, 0.f, 0.f};
    for (int r = o0 + lane; r < o1; r += 64) {
        const float mf = (a.mask == nullptr || a.mask[r] != 0) ? 1.f : 0.f;
        cnt += mf;
        for (int j = 0; j < 3; ++j) {
            if (a.center_x) sx[j] += a.x[(int64_t)r * 3 + j];
            se[j] += a.eps_raw[(int64_t)r * D + j] * mf;
            if (a.eval) s0[j] += a.eps_raw0[(int64_t)r * D + j] * mf;
        }
    }
    cnt = wave_sum(cnt);
    float mx[3], me[3], m0[3];
    for (int j = 0; j < 3; ++j) {
        mx[j] = a.center_x ? wave_sum(sx[j]) / cnt : 0.f;
        me[j] = wave_sum(se[j]) / cnt;
        m0[j] = a.eval ? wave_sum(s0[j]) / cnt : 0.f;
    }

    // pass 2: the rows
    float qx = 0.f, qh = 0.f;
    for (int r = o0 + lane; r < o1; r += 64) {
        const float mf = (a.mask == nullptr || a.mask[r] != 0) ? 1.f : 0.f;
        const int64_t base = (int64_t)r * D;
        float rx = 0.f, rh = 0.f;
        for (int j = 0; j < D; ++j) {
            float v, e = a.eps_raw[base + j] * mf, e0 = a.eval ? a.eps_raw0[base + j] * mf : 0.f;
            if (j < 3) {
                float xc = a.x[(int64_t)r * 3 + j];
                if (a.center_x) xc = xc - mx[j] * mf;
                v = xc / a.nm.nv0;
                e = e - me[j] * mf;
                e0 = e0 - m0[j] * mf;
            } else if (j < 3 + nf) {
                v = (a.one_hot[(int64_t)r * nf + (j - 3)] - a.nm.nb1) / a.nm.nv1 * mf;
            } else {
                v = (a.charges[r] - a.nm.nb2) / a.nm.nv2 * mf;
            }
            a.xh[base + j] = v;
            a.eps_t[base + j] = e;
            a.z_t[base + j] = al_t * v + si_t * e;
            if (a.eval) {
                a.eps_0[base + j] = e0;
                a.z_0[base + j] = al_0 * v + si_0 * e0;
            }
            const float mu = al_T * v;
            if (j < 3) rx += mu * mu; else rh += mu * mu * mf;
        }
        qx += rx;
        qh += rh;
        a.t_node[r] = tf;
    }
    qx = wave_sum(qx);
    qh = wave_sum(qh);
    if (lane != 0) return;

    const int np = (int)cnt;
    const float sub = (float)((np - 1) * 3);
    float* m = a.mol + (int64_t)b * 8;
    m[0] = (-sub) * a.nm.log_nv0;
    m[1] = -(sub * (-0.5f * g_0 - 0.918938533204672742f));             // 0.5 log(2 pi)
    const float lg = logf(1.f / si_T), s2 = si_T * si_T;
    const float klx = sub * lg + 0.5f * (sub * s2 + qx) - 0.5f * sub;
    const float klh = lg + 0.5f * (s2 + qh) - 0.5f;
    m[2] = klx + klh;
    m[3] = expf(-(g_s - g_t)) - 1.f;
    m[4] = t == 0 ? 1.f : 0.f;
    m[5] = cnt;
    float lp = __builtin_nanf("");
    if (np >= 0 && np < a.pn_len) lp = a.log_pn[np];
    if (lp != lp) fl |= 2;
    m[6] = lp;
    m[7] = g_t;
    if (np < 1) fl |= 8;
    if (fl) atomicOr(a.flags, fl);
}

struct TermArgs {
    const float* net; const float* net0; const float* xh; const float* eps_t; const float* z_t; const float* eps_0; const float* z_0;
    const uint8_t* mask; const int32_t* off; const float* mol; const float* gamma; float* terms;
    int32_t N, B, D, nf, ic, T, eval, l2;
    Norm nm;
};

// log of the probability of [c - 0.5, c + 0.5] under N(0, w), with the torch code's epsilon outside the difference of the two cdfs
__device__ inline float log_mass(float c, float w) {
#pragma clang fp contract(off)
    const float rs2 = 0.707106781186547524f;                             // 0.5 ** 0.5
    const float hi = 0.5f * (1.f + erff((c + 0.5f) / w * rs2));
    const float lo = 0.5f * (1.f + erff((c - 0.5f) / w * rs2));
    return logf(hi - lo + 1e-10f);
}

__global__ void __launch_bounds__(THREADS) k_obj_terms(TermArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const int o0 = clampi(a.off[b], 0, a.N), o1 = clampi(a.off[b + 1], 0, a.N);
    const int D = a.D, nf = a.nf;
    const float* m = a.mol + (int64_t)b * 8;
    const float t0 = m[4];
    const float sig0 = sqrtf(sigmoidf(a.eval ? a.gamma[0] : m[7]));
    const float* eps = a.eval ? a.eps_0 : a.eps_t;
    const float* net = a.eval ? a.net0 : a.net;
    const float* z = a.eval ? a.z_0 : a.z_t;
    const float w1 = sig0 * a.nm.nv1, w2 = sig0 * a.nm.nv2;

    float err = 0.f, l0x = 0.f, lph = 0.f, ax = 0.f, ah = 0.f;
    for (int r = o0 + lane; r < o1; r += 64) {
        const bool present = a.mask == nullptr || a.mask[r] != 0;
        const int64_t base = (int64_t)r * D;
        float sa_x = 0.f, sa_h = 0.f, re = 0.f;
        for (int j = 0; j < D; ++j) {
            const float n = a.net[base + j];
            if (j < 3) sa_x += fabsf(n); else sa_h += fabsf(n);
            const float d = a.eps_t[base + j] - n;
            re += d * d;
        }
        ax += sa_x / 3.f;
        ah += sa_h / (float)(D - 3);
        err += re;                  // error_t sums over ALL rows as the reference does: the projection's output on a masked row is not zero
        if (!present) continue;
        float r0 = 0.f;
        for (int j = 0; j < 3; ++j) { const float d = eps[base + j] - net[base + j]; r0 += d * d; }
        l0x += r0;
        float lp[MAXF], mxl = -INFINITY;
#pragma unroll
        for (int k = 0; k < MAXF; ++k) {
            lp[k] = -INFINITY;
            if (k < nf) {
                lp[k] = log_mass(z[base + 3 + k] * a.nm.nv1 + a.nm.nb1 - 1.0f, w1);
                mxl = fmaxf(mxl, lp[k]);
            }
        }
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < MAXF; ++k)
            if (k < nf) se += expf(lp[k] - mxl);
        const float lse = mxl + logf(se);
        float rp = 0.f;
#pragma unroll
        for (int k = 0; k < MAXF; ++k)
            if (k < nf) rp += (lp[k] - lse) * (a.xh[base + 3 + k] * a.nm.nv1 + a.nm.nb1);
        lph += rp;
        if (a.ic) {
            const float hi = rintf(a.xh[base + 3 + nf] * a.nm.nv2 + a.nm.nb2);
            lph += log_mass(hi - (z[base + 3 + nf] * a.nm.nv2 + a.nm.nb2), w2);
        }
    }
    err = wave_sum(err);
    l0x = wave_sum(l0x);
    lph = wave_sum(lph);
    ax = wave_sum(ax);
    ah = wave_sum(ah);
    if (lane != 0) return;
    float loss_0_x = 0.5f * l0x, loss_0_h = -lph;
    if (!a.eval) {
        err = err * (1.f - t0);
        loss_0_x = loss_0_x * t0;
        loss_0_h = loss_0_h * t0;
    }
    const int rows = o1 - o0;
    const float cnt = (float)(rows > 1 ? rows : 1);
    float* o = a.terms + (int64_t)b * 10;
    o[0] = a.l2 ? 0.f : m[0];
    o[1] = err;
    o[2] = a.l2 ? 1.f : m[3];
    o[3] = loss_0_x;
    o[4] = loss_0_h;
    o[5] = a.l2 ? 0.f : m[1];
    o[6] = m[2];
    o[7] = m[6];
    o[8] = ax / cnt;
    o[9] = ah / cnt;
}

// fixed-order block sum: butterfly per wave, then the wave totals in order; the result is valid in every thread
__device__ inline float block_sum(float x, float* lds) {
    x = wave_sum(x);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < WAVES; ++i) s += lds[i];
    return s;
}

__global__ void __launch_bounds__(THREADS) k_obj_reduce(const float* __restrict__ mol, const float* __restrict__ terms, float* __restrict__ coef,
                                                        float* __restrict__ nll, float* __restrict__ means, int B, int D, int T, int l2, int by_max) {
#pragma clang fp contract(off)
    __shared__ float lds[WAVES];
    __shared__ float ldm[WAVES];
    float mxn = 0.f;
    if (l2 && by_max) {
        for (int b = threadIdx.x; b < B; b += THREADS) mxn = fmaxf(mxn, mol[(int64_t)b * 8 + 5]);
        for (int o = 32; o > 0; o >>= 1) mxn = fmaxf(mxn, __shfl_xor(mxn, o, 64));
        if ((threadIdx.x & 63) == 0) ldm[threadIdx.x >> 6] = mxn;
        __syncthreads();
        mxn = ldm[0];
        for (int i = 1; i < WAVES; ++i) mxn = fmaxf(mxn, ldm[i]);
    }
    float acc[10];
    for (int k = 0; k < 10; ++k) acc[k] = 0.f;
    for (int b = threadIdx.x; b < B; b += THREADS) {
        const float* t = terms + (int64_t)b * 10;
        float loss_t, loss_0, ct, c0;
        if (l2) {
            const float den = (float)D * (by_max ? mxn : mol[(int64_t)b * 8 + 5]);
            loss_t = 0.5f * (t[1] / den);
            loss_0 = t[3] / den + t[4];
            ct = 0.5f / den;
            c0 = 1.f / den;
        } else {
            ct = (float)T * 0.5f * t[2];
            loss_t = ct * t[1];
            loss_0 = t[3] + t[4] + t[5];
            c0 = 1.f;
        }
        const float v = loss_t + loss_0 + t[6] - t[0] - t[7];
        nll[b] = v;
        coef[2 * b] = ct;
        coef[2 * b + 1] = c0;
        acc[0] += v; acc[1] += loss_t; acc[2] += t[2]; acc[3] += loss_0; acc[4] += t[6];
        acc[5] += t[0]; acc[6] += t[5]; acc[7] += t[7]; acc[8] += t[8]; acc[9] += t[9];
    }
    for (int k = 0; k < 10; ++k) {
        const float s = block_sum(acc[k], lds);
        if (threadIdx.x == 0) means[k] = s / (float)B;
    }
    if (threadIdx.x >= 10 && threadIdx.x < 16) means[threadIdx.x] = 0.f;
}

struct BwdArgs {
    const float* g_err; const float* g_l0x; const float* g_nll; const float* g_loss; const float* net; const float* eps_t;
    const uint8_t* mask; const int32_t* off; const float* mol; const float* coef; float* d_net;
    int64_t s_err, s_l0x, s_nll;
    int32_t N, B, D;
};

__global__ void __launch_bounds__(THREADS) k_obj_bwd(BwdArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const int o0 = clampi(a.off[b], 0, a.N), o1 = clampi(a.off[b + 1], 0, a.N);
    const int D = a.D;
    const float t0 = a.mol[(int64_t)b * 8 + 4];
    float G = a.g_nll ? a.g_nll[b * a.s_nll] : 0.f;
    if (a.g_loss) G += a.g_loss[0] / (float)a.B;
    const float Gt = (a.g_err ? a.g_err[b * a.s_err] : 0.f) + G * a.coef[2 * b];
    const float G0 = (a.g_l0x ? a.g_l0x[b * a.s_l0x] : 0.f) + G * a.coef[2 * b + 1];
    const float kt = -2.f * (1.f - t0) * Gt, k0 = -(t0 * G0);
    const int n = (o1 - o0) * D;
    for (int i = lane; i < n; i += 64) {
        const int r = o0 + i / D, j = i - (i / D) * D;
        const int64_t at = (int64_t)o0 * D + i;
        const float df = a.eps_t[at] - a.net[at];
        float d = kt * df;
        if (j < 3 && (a.mask == nullptr || a.mask[r] != 0)) d = d + k0 * df;
        a.d_net[at] = d;
    }
}

inline bool mode_ok(int32_t mode) { return mode == 0 || mode == 1 || mode == 2; }
inline bool dims_ok(int64_t N, int64_t B, int32_t nf, int32_t ic) {
    return N >= 1 && B >= 1 && nf >= 1 && nf <= MAXF && gops_flag(ic) && N * (int64_t)(3 + nf + ic) < ((int64_t)1 << 31) && B <= N;
}
inline Norm make_norm(const float* nv, const float* nb) {
    Norm n;
    n.nv0 = nv[0]; n.nv1 = nv[1]; n.nv2 = nv[2]; n.nb1 = nb[1]; n.nb2 = nb[2];
    n.log_nv0 = (float)log((double)nv[0]);
    return n;
}
inline unsigned grid_of(int64_t B) { return (unsigned)((B + WAVES - 1) / WAVES); }

}  // namespace gobj

extern "C" {

int64_t gcdm_objective_workspace_bytes(int64_t N, int64_t B, int32_t D, int32_t mode) {
    GOPS_REQUIRE(N >= 1 && B >= 1 && D >= 4 && D <= 3 + gobj::MAXF + 1 && gobj::mode_ok(mode));
    return (8 * B + 255) & ~(int64_t)255;
}

int gcdm_objective_prepare(const float* x, const float* one_hot, const float* charges, const uint8_t* mask, const int32_t* node_offsets,
                           const int32_t* t_int, const float* gamma, const float* log_pn, int32_t pn_len, const float* norm_values,
                           const float* norm_biases, const float* eps_raw, const float* eps_raw_0, float* xh, float* eps_t, float* z_t,
                           float* eps_0, float* z_0, float* t_node, float* mol, int32_t* flags, int64_t N, int64_t B, int32_t num_atom_types,
                           int32_t include_charges, int32_t T, int32_t mode, int32_t center_x, void* stream) {
    GOPS_REQUIRE(gobj::dims_ok(N, B, num_atom_types, include_charges) && T >= 1 && gobj::mode_ok(mode) && gops_flag(center_x) && pn_len >= 1);
    GOPS_REQUIRE(x && one_hot && (charges || !include_charges) && node_offsets && t_int && gamma && log_pn && norm_values && norm_biases && eps_raw);
    GOPS_REQUIRE(xh && eps_t && z_t && t_node && mol && flags);
    const int eval = mode == GCDM_OBJECTIVE_EVAL;
    GOPS_REQUIRE(!eval || (eps_raw_0 && eps_0 && z_0));
    gobj::PrepArgs a{};
    a.x = x; a.one_hot = one_hot; a.charges = charges; a.mask = mask; a.off = node_offsets; a.t_int = t_int; a.gamma = gamma; a.log_pn = log_pn;
    a.eps_raw = eps_raw; a.eps_raw0 = eps_raw_0; a.xh = xh; a.eps_t = eps_t; a.z_t = z_t; a.eps_0 = eps_0; a.z_0 = z_0; a.t_node = t_node;
    a.mol = mol; a.flags = flags;
    a.N = (int32_t)N; a.B = (int32_t)B; a.nf = num_atom_types; a.ic = include_charges; a.D = 3 + num_atom_types + include_charges; a.T = T;
    a.pn_len = pn_len; a.eval = eval; a.center_x = center_x;
    a.nm = gobj::make_norm(norm_values, norm_biases);
    hipLaunchKernelGGL(gobj::k_obj_prepare, dim3(gobj::grid_of(B)), dim3(gobj::THREADS), 0, (hipStream_t)stream, a);
    return GOPS_LAUNCH_OK();
}

int gcdm_objective_terms(const float* net_out, const float* net_out_0, const float* xh, const float* eps_t, const float* z_t, const float* eps_0,
                         const float* z_0, const uint8_t* mask, const int32_t* node_offsets, const float* mol, const float* gamma,
                         const float* norm_values, const float* norm_biases, float* terms, int64_t N, int64_t B, int32_t num_atom_types,
                         int32_t include_charges, int32_t T, int32_t mode, void* stream) {
    GOPS_REQUIRE(gobj::dims_ok(N, B, num_atom_types, include_charges) && T >= 1 && gobj::mode_ok(mode));
    GOPS_REQUIRE(net_out && xh && eps_t && z_t && node_offsets && mol && gamma && norm_values && norm_biases && terms);
    const int eval = mode == GCDM_OBJECTIVE_EVAL;
    GOPS_REQUIRE(!eval || (net_out_0 && eps_0 && z_0));
    gobj::TermArgs a{};
    a.net = net_out; a.net0 = net_out_0; a.xh = xh; a.eps_t = eps_t; a.z_t = z_t; a.eps_0 = eps_0; a.z_0 = z_0; a.mask = mask;
    a.off = node_offsets; a.mol = mol; a.gamma = gamma; a.terms = terms;
    a.N = (int32_t)N; a.B = (int32_t)B; a.nf = num_atom_types; a.ic = include_charges; a.D = 3 + num_atom_types + include_charges; a.T = T;
    a.eval = eval; a.l2 = mode == GCDM_OBJECTIVE_TRAIN_L2;
    a.nm = gobj::make_norm(norm_values, norm_biases);
    hipLaunchKernelGGL(gobj::k_obj_terms, dim3(gobj::grid_of(B)), dim3(gobj::THREADS), 0, (hipStream_t)stream, a);
    return GOPS_LAUNCH_OK();
}

int gcdm_objective_reduce(const float* mol, const float* terms, void* workspace, float* nll, float* means, int64_t B, int32_t D, int32_t T,
                          int32_t mode, int32_t norm_by_max_nodes, void* stream) {
    GOPS_REQUIRE(B >= 1 && B < ((int64_t)1 << 28) && D >= 4 && D <= 3 + gobj::MAXF + 1 && T >= 1 && gobj::mode_ok(mode) && gops_flag(norm_by_max_nodes));
    GOPS_REQUIRE(mol && terms && workspace && nll && means);
    hipLaunchKernelGGL(gobj::k_obj_reduce, dim3(1), dim3(gobj::THREADS), 0, (hipStream_t)stream, mol, terms, (float*)workspace, nll, means, (int)B,
                       (int)D, (int)T, (int)(mode == GCDM_OBJECTIVE_TRAIN_L2), (int)norm_by_max_nodes);
    return GOPS_LAUNCH_OK();
}

int gcdm_objective_bwd(const float* g_error_t, int64_t stride_error_t, const float* g_loss_0_x, int64_t stride_loss_0_x, const float* g_nll,
                       int64_t stride_nll, const float* g_loss, const float* net_out, const float* eps_t, const uint8_t* mask, const int32_t* node_offsets, const float* mol, const void* workspace,
                       float* d_net_out, int64_t N, int64_t B, int32_t D, int32_t mode, void* stream) {
    GOPS_REQUIRE(N >= 1 && B >= 1 && B <= N && D >= 4 && D <= 3 + gobj::MAXF + 1 && N * (int64_t)D < ((int64_t)1 << 31));
    GOPS_REQUIRE(mode == GCDM_OBJECTIVE_TRAIN_VLB || mode == GCDM_OBJECTIVE_TRAIN_L2);
    GOPS_REQUIRE(net_out && eps_t && node_offsets && mol && workspace && d_net_out && stride_error_t >= 0 && stride_loss_0_x >= 0 && stride_nll >= 0);
    gobj::BwdArgs a{};
    a.s_err = stride_error_t; a.s_l0x = stride_loss_0_x; a.s_nll = stride_nll;
    a.g_err = g_error_t; a.g_l0x = g_loss_0_x; a.g_nll = g_nll; a.g_loss = g_loss; a.net = net_out; a.eps_t = eps_t; a.mask = mask;
    a.off = node_offsets; a.mol = mol; a.coef = (const float*)workspace; a.d_net = d_net_out;
    a.N = (int32_t)N; a.B = (int32_t)B; a.D = D;
    hipLaunchKernelGGL(gobj::k_obj_bwd, dim3(gobj::grid_of(B)), dim3(gobj::THREADS), 0, (hipStream_t)stream, a);
    return GOPS_LAUNCH_OK();
}

}  // extern "C"
