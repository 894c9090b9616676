// gcdm_ops.egnn_train.hip.h -- the per-edge block of an EGNN dynamics layer as one differentiable operator, forward and backward, on gfx950.
// C ABI: include/gcdm_egnn_train.h.  DESIGN.md 3.10.
//
// The edge list is never materialised (as in gcdm_ops.egnn_dynamics.hip.h): a workgroup (256 threads, 4 waves) owns up to RB = 32 consecutive nodes (fewer in a small batch: owners_of) and
// walks their slots "owner o, slot s -> node_offsets[mol(o)] + s" as one flat list in rounds.
//
// Forward (k_fwd, rounds of 256 edges): k_edge's plan on the unpacked operands A, B [N, K], V [3, K], W2 [16, K].
//
// Backward (k_bwd<ROLE>, rounds of 128 edges), one kernel compiled for two roles.  ROLE 0: the owner is the receiver i, the slots are the senders;
// it produces gA, the -g_d half of gx and every weight / vector gradient.  ROLE 1: the owner is the sender j, the slots are the receivers (the same
// list: the edge set is symmetric); it produces gB and adds the +g_d half of gx.  Each role recomputes the edge; per round:
//   1. sweep 1, edges split over the waves: z2 = W2 silu(z1) + b2 by 16-wide k-block on v_mfma_f32_16x16x4_f32 -> LDS stage;
//   2. one lane per edge: m, coors_mlp forward and backward -> g_z2, w, g_c; ROLE 0 stages g_v by halves of the 64 hidden units and 256 threads
//      add g_v (x) m, g_v, g_c silu(v) over the round's edges in edge order into registers they keep for the whole launch;
//   3. sweep 2, k-blocks split over the waves (a wave walks all edges of the round for its k-blocks, so that a k-block's gW2 / gV tile has one
//      owner): recomputes z1 at (edge 4 q + r, k = lane & 15), forms W2^T g_z2 (MFMA, contraction over m), g_z1, g_z2 (x) a1 and
//      (r0, r0sc, r) (x) g_z1 (MFMA, contraction over edges), stages g_z1 and adds it per owner in slot order to gA / gB;
//   4. one lane per edge: g_d from w_r . g_z1 and the coordinate term; per owner the sum in slot order, THE DIAGONAL SLOT SKIPPED, to gx.
// Weight and vector gradients of a workgroup go to its own partial block in the workspace (read-modify-write by the one lane that owns the
// address, or a plain store at the end); k_reduce adds the blocks in workgroup order.  The grid is capped at GROUPS workgroups, which loop over
// the owner blocks.  No float atomics; the same bits from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdarg.h>
#include <stdio.h>
#include <math.h>
#include <atomic>

namespace gegt {

using gegd::f32x4;
using gegd::silu;
constexpr int MD = gegd::MD, CH = gegd::CH, THREADS = gegd::THREADS, RB = gegd::RB, NC = gegd::NC, SS = gegd::SS;
constexpr int RNDF = 256;           // edges per round, forward
constexpr int RNDB = 128;           // edges per round, backward
constexpr int GS = 17;              // g_z1 stage row stride
constexpr int HC = 32;              // hidden units of coors_mlp per staged half
constexpr int GROUPS = 256;         // GCDM_EGNN_TRAIN_MAX_GROUPS
constexpr int SMALL = MD + CH * MD + CH + CH + 2;          // gb2 | gC1 | gc1b | gc2 | gc2b | gscale

__host__ __device__ inline int64_t partial_floats(int K) { return (int64_t)19 * K + SMALL; }

struct Args {
    const float *A, *B, *V, *W2, *b2, *C1, *c1b, *c2, *c2b, *scale, *x, *x0, *xsc;
    const int32_t *noff, *nmol;
    int64_t N;
    int nB, K, Kp, e_in, rb;          // rb: owners per owner block, 1 .. RB
};

// d silu(v) / dv
__device__ __forceinline__ float dsilu(float v) {
    const float s = 1.f / (1.f + expf(-v));
    return s * (1.f + v * (1.f - s));
}

// s += v with the rounding error carried in c (Kahan): the sums over all edges of a launch are a round's plain sum added this way
__device__ __forceinline__ void kadd(float& s, float& c, float v) {
    const float y = v - c, t = s + y;
    c = (t - s) - y;
    s = t;
}

// the slot lists of the owner block that starts at node i0: mo / cnt per owner, lp the prefix sums.  Ends with a barrier.
__device__ __forceinline__ void setup_block(const Args& p, int64_t i0, int nr, int* lp, int* mo, int* cnt) {
    const int tid = threadIdx.x;
    if (tid < RB) {
        int start = 0, n = 0;
        if (tid < nr) {
            const int64_t i = i0 + tid;
            const int m = p.nmol[i];
            if (m >= 0 && m < p.nB) {
                const int64_t a = p.noff[m], b = p.noff[m + 1];
                if (a >= 0 && b <= p.N && a <= i && i < b) { start = (int)a; n = (int)(b - a); }
            }
        }
        mo[tid] = start;
        cnt[tid] = n;
    }
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int r = 0; r < RB; ++r) { lp[r] = s; s += cnt[r]; }
        lp[RB] = s;
    }
    __syncthreads();
}

// (receiver, sender) of local edge q of the owner block; a slot past the end computes on node i0 and is never summed
template <int ROLE>
__device__ __forceinline__ void edge_nodes(const int* lp, const int* mo, int64_t i0, int q, int total, int64_t& i, int64_t& j) {
    i = i0; j = i0;
    if (q < total) {
        const int r = gegd::locate(lp, q);
        const int64_t own = i0 + r, oth = (int64_t)mo[r] + (q - lp[r]);
        i = ROLE == 0 ? own : oth;
        j = ROLE == 0 ? oth : own;
    }
}

__device__ __forceinline__ float sqdist(const float* __restrict__ x, int64_t i, int64_t j) {
    const float dx = x[j * 3] - x[i * 3], dy = x[j * 3 + 1] - x[i * 3 + 1], dz = x[j * 3 + 2] - x[i * 3 + 2];
    return dx * dx + dy * dy + dz * dz;
}

// z2 (without the bias) of TW 16-edge tiles: lane (e, q) = (lane & 15, lane >> 4) forms k = kc + 4 q .. + 3 of edge e of each tile
template <int TW>
__device__ __forceinline__ void sweep1(const Args& p, int lane, const int64_t* ei, const int64_t* ej, const float* r0, const float* r0s,
                                       const float* rad, f32x4* c) {
    const int e16 = lane & 15, kq = lane >> 4, K = p.K;
#pragma unroll
    for (int t = 0; t < TW; ++t) c[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < p.Kp; kc += 16) {
        float uv[4], sv[4], wv[4], w2v[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = kc + 4 * kq + s;
            const bool in = k < K;
            uv[s] = in ? p.V[k] : 0.f;
            sv[s] = (in && p.e_in == 2) ? p.V[K + k] : 0.f;
            wv[s] = in ? p.V[2 * K + k] : 0.f;
            w2v[s] = in ? p.W2[e16 * K + k] : 0.f;
        }
        float act[TW][4];
#pragma unroll
        for (int t = 0; t < TW; ++t)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = kc + 4 * kq + s;
                float v = 0.f;
                if (k < K) {
                    v = p.A[ei[t] * K + k] + p.B[ej[t] * K + k];
                    v = fmaf(r0[t], uv[s], v);
                    v = fmaf(r0s[t], sv[s], v);
                    v = fmaf(rad[t], wv[s], v);
                }
                act[t][s] = silu(v);
            }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < TW; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(act[t][s], w2v[s], c[t], 0, 0, 0);
    }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_fwd(Args p, float* __restrict__ Mout, float* __restrict__ dxout) {
    __shared__ float stage[RNDF * SS];
    __shared__ float acc[RB * NC];
    __shared__ int lp[RB + 1];
    __shared__ int mo[RB];
    __shared__ int cnt[RB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e16 = lane & 15, kq = lane >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * p.rb;
    const int nr = p.N - i0 < p.rb ? (int)(p.N - i0) : p.rb;
    for (int idx = tid; idx < RB * NC; idx += THREADS) acc[idx] = 0.f;
    setup_block(p, i0, nr, lp, mo, cnt);
    const int total = lp[RB];
    const float b2v = p.b2[e16];
    for (int q0 = 0; q0 < total; q0 += RNDF) {
        const int tile0 = q0 + wave * 64;
        if (tile0 < total) {
            int64_t ei[4], ej[4];
            float r0[4], r0s[4], rad[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                edge_nodes<0>(lp, mo, i0, tile0 + 16 * t + e16, total, ei[t], ej[t]);
                rad[t] = sqdist(p.x, ei[t], ej[t]);
                r0[t] = sqdist(p.x0, ei[t], ej[t]);
                r0s[t] = p.xsc ? sqdist(p.xsc, ei[t], ej[t]) : 0.f;
            }
            f32x4 c[4];
            sweep1<4>(p, lane, ei, ej, r0, r0s, rad, c);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) stage[(wave * 64 + 16 * t + 4 * kq + r) * SS + e16] = silu(c[t][r] + b2v);
        }
        __syncthreads();
        {
            const int q = tile0 + lane;
            if (q < total) {
                int64_t i, j;
                edge_nodes<0>(lp, mo, i0, q, total, i, j);
                float* row = stage + (wave * 64 + lane) * SS;
                float m[MD];
#pragma unroll
                for (int k = 0; k < MD; ++k) m[k] = row[k];
                float w = p.c2b[0];
                for (int h = 0; h < CH; ++h) {
                    float v = p.c1b[h];
#pragma unroll
                    for (int k = 0; k < MD; ++k) v = fmaf(m[k], p.C1[h * MD + k], v);
                    w = fmaf(silu(v), p.c2[h], w);
                }
                w = tanhf(w);
                const float scale = p.scale[0];
                const float dx = p.x[j * 3] - p.x[i * 3], dy = p.x[j * 3 + 1] - p.x[i * 3 + 1], dz = p.x[j * 3 + 2] - p.x[i * 3 + 2];
                const float nrm = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-8f);
                row[MD] = w * (dx / nrm * scale);
                row[MD + 1] = w * (dy / nrm * scale);
                row[MD + 2] = w * (dz / nrm * scale);
            }
        }
        __syncthreads();
        {
            const int qe = q0 + RNDF < total ? q0 + RNDF : total;
            const int rf = gegd::locate(lp, q0), rl = gegd::locate(lp, qe - 1);
            for (int task = tid; task < (rl - rf + 1) * NC; task += THREADS) {
                const int r = rf + task / NC, col = task % NC;
                const int s0 = lp[r] > q0 ? lp[r] : q0, s1 = lp[r + 1] < qe ? lp[r + 1] : qe;
                float a = acc[r * NC + col];
                for (int q = s0; q < s1; ++q) a += stage[(q - q0) * SS + col];
                acc[r * NC + col] = a;
            }
        }
        __syncthreads();
    }
    for (int idx = tid; idx < nr * MD; idx += THREADS) Mout[(i0 + idx / MD) * MD + idx % MD] = acc[(idx / MD) * NC + idx % MD];
    for (int idx = tid; idx < nr * 3; idx += THREADS) dxout[(i0 + idx / 3) * 3 + idx % 3] = acc[(idx / 3) * NC + MD + idx % 3];
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------------
// gown: gA (ROLE 0) or gB (ROLE 1), zero on entry.  gx: zero on entry of ROLE 0, ROLE 1 adds to it.  part: this launch's partial blocks, zero on
// entry (ROLE 0 only).
template <int ROLE>
__global__ __launch_bounds__(THREADS) void k_bwd(Args p, const float* __restrict__ gM, const float* __restrict__ gdx, float* __restrict__ gown,
                                                 float* __restrict__ gx, float* __restrict__ part, int64_t nblocks) {
    __shared__ float stage[RNDB * SS];          // z2 -> m -> g_z2 in 0 .. 15 (g_d in 0 .. 2 at the end), w, g_c, the gscale term in 16 .. 18
    __shared__ float rst[RNDB * 4];             // r0, r0sc, r
    __shared__ int sei[RNDB], sej[RNDB], sval[RNDB];
    __shared__ float big[4 * RNDB * GS];        // per wave the g_z1 of its k-block | the two g_v stages of phase 2 | the four partial w_r . g_z1
    __shared__ int lp[RB + 1];
    __shared__ int mo[RB];
    __shared__ int cnt[RB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e16 = lane & 15, kq = lane >> 4;
    const int K = p.K, nkb = p.Kp / 16, nit = (nkb + 3) / 4;
    const float b2v = p.b2[e16];
    const float scale = p.scale[0];
    float* gvst = big;
    float* gsvst = big + RNDB * (HC + 1);
    float* pw = part + (int64_t)blockIdx.x * partial_floats(K);
    float accC1[CH / HC][2] = {{0.f, 0.f}, {0.f, 0.f}}, accH[CH / HC] = {0.f, 0.f}, accS = 0.f;
    float cmpC1[CH / HC][2] = {{0.f, 0.f}, {0.f, 0.f}}, cmpH[CH / HC] = {0.f, 0.f}, cmpS = 0.f;

    for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const int64_t i0 = blk * p.rb;
        const int nr = p.N - i0 < p.rb ? (int)(p.N - i0) : p.rb;
        __syncthreads();
        setup_block(p, i0, nr, lp, mo, cnt);
        const int total = lp[RB];
        for (int q0 = 0; q0 < total; q0 += RNDB) {
            const int nE = total - q0 < RNDB ? total - q0 : RNDB;
            // ---- phase 1: z2 of the wave's 32 edges ---------------------------------------------------------------------------------------
            const int tile0 = q0 + wave * 32;
            if (tile0 < total) {
                int64_t ei[2], ej[2];
                float r0[2], r0s[2], rad[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    edge_nodes<ROLE>(lp, mo, i0, tile0 + 16 * t + e16, total, ei[t], ej[t]);
                    rad[t] = sqdist(p.x, ei[t], ej[t]);
                    r0[t] = sqdist(p.x0, ei[t], ej[t]);
                    r0s[t] = p.xsc ? sqdist(p.xsc, ei[t], ej[t]) : 0.f;
                }
                f32x4 c[2];
                sweep1<2>(p, lane, ei, ej, r0, r0s, rad, c);
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) stage[(wave * 32 + 16 * t + 4 * kq + r) * SS + e16] = c[t][r] + b2v;
            }
            __syncthreads();
            // ---- phase 2: one lane per edge, coors_mlp forward and backward ---------------------------------------------------------------
            float z2[MD], gm[MD], gc = 0.f;
            int64_t pi = i0, pj = i0;
            const bool mine = tid < RNDB;
            const bool valid = mine && tid < nE;
            if (mine) {
                edge_nodes<ROLE>(lp, mo, i0, q0 + tid, total, pi, pj);
                sei[tid] = (int)pi; sej[tid] = (int)pj; sval[tid] = valid ? 1 : 0;
                float* row = stage + tid * SS;
                float m[MD];
                if (valid) {
#pragma unroll
                    for (int k = 0; k < MD; ++k) { z2[k] = row[k]; m[k] = silu(z2[k]); }
                } else {
#pragma unroll
                    for (int k = 0; k < MD; ++k) { z2[k] = 0.f; m[k] = 0.f; }
                }
#pragma unroll
                for (int k = 0; k < MD; ++k) { row[k] = m[k]; gm[k] = valid ? gM[pi * MD + k] : 0.f; }
                float w = p.c2b[0];
                for (int h = 0; h < CH; ++h) {
                    float v = p.c1b[h];
#pragma unroll
                    for (int k = 0; k < MD; ++k) v = fmaf(m[k], p.C1[h * MD + k], v);
                    w = fmaf(silu(v), p.c2[h], w);
                }
                w = tanhf(w);
                const float dx = p.x[pj * 3] - p.x[pi * 3], dy = p.x[pj * 3 + 1] - p.x[pi * 3 + 1], dz = p.x[pj * 3 + 2] - p.x[pi * 3 + 2];
                const float rr = dx * dx + dy * dy + dz * dz;
                const float nrm = fmaxf(sqrtf(rr), 1e-8f);
                const float dot = (gdx[pi * 3] * dx + gdx[pi * 3 + 1] * dy + gdx[pi * 3 + 2] * dz) / nrm;
                float gs = 0.f;
                if (valid) { gs = w * dot; gc = scale * dot * (1.f - w * w); }
                rst[tid * 4] = sqdist(p.x0, pi, pj);
                rst[tid * 4 + 1] = p.xsc ? sqdist(p.xsc, pi, pj) : 0.f;
                rst[tid * 4 + 2] = rr;
                rst[tid * 4 + 3] = 0.f;
                row[MD] = w; row[MD + 1] = gc; row[MD + 2] = gs;
            }
#pragma unroll
            for (int ch = 0; ch < CH / HC; ++ch) {
                if (mine) {
                    const float* row = stage + tid * SS;
                    float m[MD];
#pragma unroll
                    for (int k = 0; k < MD; ++k) m[k] = row[k];
                    for (int hl = 0; hl < HC; ++hl) {
                        const int h = ch * HC + hl;
                        float v = p.c1b[h];
#pragma unroll
                        for (int k = 0; k < MD; ++k) v = fmaf(m[k], p.C1[h * MD + k], v);
                        const float gv = gc * p.c2[h] * dsilu(v);
#pragma unroll
                        for (int k = 0; k < MD; ++k) gm[k] = fmaf(p.C1[h * MD + k], gv, gm[k]);
                        if (ROLE == 0) { gvst[tid * (HC + 1) + hl] = gv; gsvst[tid * (HC + 1) + hl] = gc * silu(v); }
                    }
                }
                if (ROLE == 0) {
                    __syncthreads();
#pragma unroll
                    for (int pp = 0; pp < 2; ++pp) {
                        const int pr = tid + THREADS * pp, hl = pr >> 4, k = pr & 15;
                        float a = 0.f;
                        for (int e = 0; e < nE; ++e) a = fmaf(gvst[e * (HC + 1) + hl], stage[e * SS + k], a);
                        kadd(accC1[ch][pp], cmpC1[ch][pp], a);
                    }
                    if (tid < 2 * HC) {
                        const float* src = tid < HC ? gvst + tid : gsvst + (tid - HC);
                        float a = 0.f;
                        for (int e = 0; e < nE; ++e) a += src[e * (HC + 1)];
                        kadd(accH[ch], cmpH[ch], a);
                    }
                    __syncthreads();
                }
            }
            if (mine) {
                float* row = stage + tid * SS;
#pragma unroll
                for (int k = 0; k < MD; ++k) row[k] = valid ? gm[k] * dsilu(z2[k]) : 0.f;
            }
            __syncthreads();
            if (ROLE == 0 && tid < MD + 2) {                         // gb2 | gc2b | gscale
                const int col = tid < MD ? tid : tid + 1;
                float a = 0.f;
                for (int e = 0; e < nE; ++e) a += stage[e * SS + col];
                kadd(accS, cmpS, a);
            }
            // ---- phase 3: sweep 2, the wave's k-blocks over all edges of the round ----------------------------------------------------------
            float qacc[RNDB / 16][4];
#pragma unroll
            for (int t = 0; t < RNDB / 16; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) qacc[t][r] = 0.f;
            float* gz = big + wave * RNDB * GS;
            const int qe = q0 + nE;
            const int rf = gegd::locate(lp, q0), rl = gegd::locate(lp, qe - 1);
            for (int it = 0; it < nit; ++it) {
                const int kb = it * 4 + wave;
                const int k = kb * 16 + e16;
                const bool kin = kb < nkb && k < K;
                if (kb < nkb) {
                    const float uu = kin ? p.V[k] : 0.f, us = (kin && p.e_in == 2) ? p.V[K + k] : 0.f, ww = kin ? p.V[2 * K + k] : 0.f;
                    float w2b[4];
#pragma unroll
                    for (int s = 0; s < 4; ++s) w2b[s] = kin ? p.W2[(4 * kq + s) * K + k] : 0.f;
                    f32x4 accW = {0.f, 0.f, 0.f, 0.f}, accV = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int t = 0; t < RNDB / 16; ++t) {
                        if (16 * t < nE) {
                            const int eb = 16 * t + 4 * kq;
                            f32x4 g1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                            for (int s = 0; s < 4; ++s) g1 = __builtin_amdgcn_mfma_f32_16x16x4f32(stage[(16 * t + e16) * SS + 4 * kq + s], w2b[s], g1, 0, 0, 0);
                            float a1[4], gz1[4];
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int e = eb + r;
                                a1[r] = 0.f; gz1[r] = 0.f;
                                if (kin && sval[e]) {
                                    float v = p.A[(int64_t)sei[e] * K + k] + p.B[(int64_t)sej[e] * K + k];
                                    v = fmaf(rst[e * 4], uu, v);
                                    v = fmaf(rst[e * 4 + 1], us, v);
                                    v = fmaf(rst[e * 4 + 2], ww, v);
                                    const float sg = 1.f / (1.f + expf(-v));
                                    a1[r] = v * sg;
                                    gz1[r] = g1[r] * (sg * (1.f + v * (1.f - sg)));
                                }
                                qacc[t][r] = fmaf(ww, gz1[r], qacc[t][r]);
                                gz[e * GS + e16] = gz1[r];
                            }
                            if (ROLE == 0) {
#pragma unroll
                                for (int s = 0; s < 4; ++s) {
                                    accW = __builtin_amdgcn_mfma_f32_16x16x4f32(stage[(eb + s) * SS + e16], a1[s], accW, 0, 0, 0);
                                    accV = __builtin_amdgcn_mfma_f32_16x16x4f32(e16 < 3 ? rst[(eb + s) * 4 + e16] : 0.f, gz1[s], accV, 0, 0, 0);
                                }
                            }
                        }
                    }
                    if (ROLE == 0 && kin) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) pw[(int64_t)(4 * kq + r) * K + k] += accW[r];
                        if (kq == 0) {
#pragma unroll
                            for (int r = 0; r < 3; ++r) pw[(int64_t)(MD + r) * K + k] += accV[r];
                        }
                    }
                }
                __syncthreads();
                if (kb < nkb) {
                    for (int task = lane; task < (rl - rf + 1) * 16; task += 64) {
                        const int r = rf + (task >> 4), kk = kb * 16 + (task & 15);
                        if (kk < K) {
                            const int s0 = lp[r] > q0 ? lp[r] : q0, s1 = lp[r + 1] < qe ? lp[r + 1] : qe;
                            float* dst = gown + (i0 + r) * K + kk;
                            float a = *dst;
                            for (int q = s0; q < s1; ++q) a += gz[(q - q0) * GS + (task & 15)];
                            *dst = a;
                        }
                    }
                }
                __syncthreads();
            }
            // ---- phase 4: g_d and the owner's sum, the diagonal skipped -------------------------------------------------------------------
#pragma unroll
            for (int t = 0; t < RNDB / 16; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = qacc[t][r];
                    v += __shfl_xor(v, 1, 16);
                    v += __shfl_xor(v, 2, 16);
                    v += __shfl_xor(v, 4, 16);
                    v += __shfl_xor(v, 8, 16);
                    if (e16 == 0) big[wave * RNDB + 16 * t + 4 * kq + r] = v;
                }
            __syncthreads();
            if (valid && pi != pj) {
                const float q = ((big[tid] + big[RNDB + tid]) + big[2 * RNDB + tid]) + big[3 * RNDB + tid];
                float* row = stage + tid * SS;
                const float w = row[MD];
                const float dx = p.x[pj * 3] - p.x[pi * 3], dy = p.x[pj * 3 + 1] - p.x[pi * 3 + 1], dz = p.x[pj * 3 + 2] - p.x[pi * 3 + 2];
                const float nv = sqrtf(dx * dx + dy * dy + dz * dz);
                const float gtx = gdx[pi * 3], gty = gdx[pi * 3 + 1], gtz = gdx[pi * 3 + 2];
                const float ws = w * scale;
                float cx, cy, cz;
                if (nv > 1e-8f) {
                    const float dn = (gtx * dx + gty * dy + gtz * dz) / (nv * nv * nv);
                    cx = ws * (gtx / nv - dx * dn); cy = ws * (gty / nv - dy * dn); cz = ws * (gtz / nv - dz * dn);
                } else {
                    cx = ws * (gtx / 1e-8f); cy = ws * (gty / 1e-8f); cz = ws * (gtz / 1e-8f);
                }
                row[0] = fmaf(2.f * dx, q, cx);
                row[1] = fmaf(2.f * dy, q, cy);
                row[2] = fmaf(2.f * dz, q, cz);
            }
            __syncthreads();
            if (tid < (rl - rf + 1) * 3) {
                const int r = rf + tid / 3, c = tid % 3;
                const int s0 = lp[r] > q0 ? lp[r] : q0, s1 = lp[r + 1] < qe ? lp[r + 1] : qe;
                const int64_t own = i0 + r;
                float a = gx[own * 3 + c];
                for (int q = s0; q < s1; ++q) {
                    if ((int64_t)mo[r] + (q - lp[r]) == own) continue;          // the diagonal: g_d is never formed, added or subtracted
                    const float g = stage[(q - q0) * SS + c];
                    a = ROLE == 0 ? a - g : a + g;
                }
                gx[own * 3 + c] = a;
            }
            __syncthreads();
        }
    }
    if (ROLE == 0) {
        float* ps = pw + (int64_t)19 * K;
        if (tid < MD) ps[tid] = accS - cmpS;
        else if (tid == MD) ps[MD + CH * MD + 2 * CH] = accS - cmpS;
        else if (tid == MD + 1) ps[MD + CH * MD + 2 * CH + 1] = accS - cmpS;
#pragma unroll
        for (int ch = 0; ch < CH / HC; ++ch) {
#pragma unroll
            for (int pp = 0; pp < 2; ++pp) ps[MD + ch * HC * MD + tid + THREADS * pp] = accC1[ch][pp] - cmpC1[ch][pp];
            if (tid < HC) ps[MD + CH * MD + ch * HC + tid] = accH[ch] - cmpH[ch];
            else if (tid < 2 * HC) ps[MD + CH * MD + CH + ch * HC + (tid - HC)] = accH[ch] - cmpH[ch];
        }
    }
}

struct Grads { float *gV, *gW2, *gb2, *gC1, *gc1b, *gc2, *gc2b, *gscale; };

// the partial blocks added in workgroup order
__global__ void k_reduce(const float* __restrict__ part, int groups, int K, Grads g) {
    const int64_t P = partial_floats(K);
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P) return;
    float s = 0.f, c = 0.f;
    for (int w = 0; w < groups; ++w) kadd(s, c, part[(int64_t)w * P + idx]);
    s -= c;
    int64_t o = idx;
    if (o < (int64_t)MD * K) { g.gW2[o] = s; return; }
    o -= (int64_t)MD * K;
    if (o < (int64_t)3 * K) { g.gV[o] = s; return; }
    o -= (int64_t)3 * K;
    if (o < MD) { g.gb2[o] = s; return; }
    o -= MD;
    if (o < CH * MD) { g.gC1[o] = s; return; }
    o -= CH * MD;
    if (o < CH) { g.gc1b[o] = s; return; }
    o -= CH;
    if (o < CH) { g.gc2[o] = s; return; }
    o -= CH;
    if (o == 0) g.gc2b[0] = s; else g.gscale[0] = s;
}

static thread_local char g_err[256] = "";
static std::atomic<int64_t> g_bwd_launches{0};
__attribute__((format(printf, 2, 3))) static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

static int check(int64_t N, int64_t nB, int H, int Eh, int e_in) {
    if (H < 32 || H > gegd::MAX_H || H % 32) return fail(-1, "h_hidden = %d: the limit is a multiple of 32 up to %d", H, gegd::MAX_H);
    if (Eh < 1 || Eh > gegd::MAX_EH) return fail(-1, "e_hidden = %d: the limit is 1 .. %d", Eh, gegd::MAX_EH);
    if (e_in != 1 && e_in != 2) return fail(-1, "e_in = %d: 1 or 2", e_in);
    if (N < 0 || nB < 0) return fail(-1, "negative size");
    if (N > gegd::MAX_NODES || nB > N) return fail(-1, "%lld atoms in %lld molecules: at most %lld atoms and no more molecules than atoms",
                                                   (long long)N, (long long)nB, (long long)gegd::MAX_NODES);
    if (N > 0 && nB == 0) return fail(-1, "%lld atoms in no molecule", (long long)N);
    return 0;
}

// owners per owner block: as few as fill GROUPS workgroups, so that a training batch of a thousand atoms still covers the chip; what a
// receiver's or a sender's sums are does not depend on it (one owner, slot order), only the association of the weight gradients' partial sums does
static int owners_of(int64_t N) {
    const int64_t rb = (N + GROUPS - 1) / GROUPS;
    return rb < 1 ? 1 : rb > RB ? RB : (int)rb;
}

static int groups_of(int64_t N) {
    const int64_t nb = (N + owners_of(N) - 1) / owners_of(N);
    return nb < 1 ? 1 : nb > GROUPS ? GROUPS : (int)nb;
}

}  // namespace gegt

extern "C" {

const char* gcdm_egnn_train_last_error(void) { return gegt::g_err; }

int64_t gcdm_egnn_train_launches(void) { return gegt::g_bwd_launches.load(std::memory_order_relaxed); }

int64_t gcdm_egnn_train_workspace_bytes(int64_t num_nodes, int32_t h_hidden, int32_t e_hidden, int32_t e_in) {
    using namespace gegt;
    if (num_nodes < 0 || num_nodes > gegd::MAX_NODES) return fail(-1, "num_nodes = %lld: 0 .. %lld", (long long)num_nodes, (long long)gegd::MAX_NODES);
    if (check(0, 0, h_hidden, e_hidden, e_in)) return -1;
    const int K = 2 * (2 * h_hidden + e_hidden + 1);
    const int64_t blocks = num_nodes < 1 ? 1 : num_nodes > GROUPS ? GROUPS : num_nodes;          // >= groups_of(num_nodes), monotone
    return blocks * partial_floats(K) * 4 + 256;
}

int gcdm_egnn_train_edge_fwd(const float* A, const float* B, const float* V, const float* W2, const float* b2, const float* C1, const float* c1b,
                             const float* c2, const float* c2b, const float* scale, const float* x, const float* x0, const float* xsc,
                             const int32_t* node_offsets, const int32_t* node_mol, float* M, float* dx, int64_t num_nodes, int64_t num_molecules,
                             int32_t h_hidden, int32_t e_hidden, int32_t e_in, void* stream) {
    using namespace gegt;
    if (check(num_nodes, num_molecules, h_hidden, e_hidden, e_in)) return -1;
    if ((e_in == 2) != (xsc != nullptr)) return fail(-1, "xsc goes with e_in = 2 and only with it");
    if (num_nodes == 0) return 0;
    if (!A || !B || !V || !W2 || !b2 || !C1 || !c1b || !c2 || !c2b || !scale || !x || !x0 || !node_offsets || !node_mol || !M || !dx)
        return fail(-1, "null pointer");
    const int K = 2 * (2 * h_hidden + e_hidden + 1);
    const Args p{A, B, V, W2, b2, C1, c1b, c2, c2b, scale, x, x0, xsc, node_offsets, node_mol, num_nodes, (int)num_molecules, K, (K + 15) / 16 * 16, e_in, owners_of(num_nodes)};
    hipLaunchKernelGGL(k_fwd, dim3((unsigned)((num_nodes + p.rb - 1) / p.rb)), dim3(THREADS), 0, (hipStream_t)stream, p, M, dx);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(-2, "egnn train forward launch failed: %s", hipGetErrorString(e));
}

int gcdm_egnn_train_edge_bwd(const float* A, const float* B, const float* V, const float* W2, const float* b2, const float* C1, const float* c1b,
                             const float* c2, const float* c2b, const float* scale, const float* x, const float* x0, const float* xsc,
                             const int32_t* node_offsets, const int32_t* node_mol, const float* gM, const float* gdx, void* workspace, float* gA,
                             float* gB, float* gx, float* gV, float* gW2, float* gb2, float* gC1, float* gc1b, float* gc2, float* gc2b,
                             float* gscale, int64_t num_nodes, int64_t num_molecules, int32_t h_hidden, int32_t e_hidden, int32_t e_in,
                             void* stream) {
    using namespace gegt;
    const int64_t N = num_nodes;
    if (check(N, num_molecules, h_hidden, e_hidden, e_in)) return -1;
    if ((e_in == 2) != (xsc != nullptr)) return fail(-1, "xsc goes with e_in = 2 and only with it");
    if (!gV || !gW2 || !gb2 || !gC1 || !gc1b || !gc2 || !gc2b || !gscale) return fail(-1, "null pointer");
    if (N > 0 && (!A || !B || !V || !W2 || !b2 || !C1 || !c1b || !c2 || !c2b || !scale || !x || !x0 || !node_offsets || !node_mol || !gM || !gdx ||
                  !workspace || !gA || !gB || !gx))
        return fail(-1, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int K = 2 * (2 * h_hidden + e_hidden + 1);
    const Grads g{gV, gW2, gb2, gC1, gc1b, gc2, gc2b, gscale};
    if (N == 0) {
        (void)hipMemsetAsync(gV, 0, (size_t)3 * K * 4, st); (void)hipMemsetAsync(gW2, 0, (size_t)MD * K * 4, st); (void)hipMemsetAsync(gb2, 0, MD * 4, st);
        (void)hipMemsetAsync(gC1, 0, CH * MD * 4, st); (void)hipMemsetAsync(gc1b, 0, CH * 4, st); (void)hipMemsetAsync(gc2, 0, CH * 4, st);
        (void)hipMemsetAsync(gc2b, 0, 4, st); (void)hipMemsetAsync(gscale, 0, 4, st);
        const hipError_t e0 = hipGetLastError();
        return e0 == hipSuccess ? 0 : fail(-2, "egnn train backward memset failed: %s", hipGetErrorString(e0));
    }
    const Args p{A, B, V, W2, b2, C1, c1b, c2, c2b, scale, x, x0, xsc, node_offsets, node_mol, N, (int)num_molecules, K, (K + 15) / 16 * 16, e_in, owners_of(N)};
    const int groups = groups_of(N);
    const int64_t nblocks = (N + p.rb - 1) / p.rb, P = partial_floats(K);
    float* part = (float*)(((uintptr_t)workspace + 255) / 256 * 256);
    (void)hipMemsetAsync(part, 0, (size_t)groups * P * 4, st);
    (void)hipMemsetAsync(gA, 0, (size_t)N * K * 4, st);
    (void)hipMemsetAsync(gB, 0, (size_t)N * K * 4, st);
    (void)hipMemsetAsync(gx, 0, (size_t)N * 3 * 4, st);
    hipLaunchKernelGGL(k_bwd<0>, dim3((unsigned)groups), dim3(THREADS), 0, st, p, gM, gdx, gA, gx, part, nblocks);
    hipLaunchKernelGGL(k_bwd<1>, dim3((unsigned)groups), dim3(THREADS), 0, st, p, gM, gdx, gB, gx, part, nblocks);
    hipLaunchKernelGGL(k_reduce, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, (const float*)part, groups, K, g);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-2, "egnn train backward launch failed: %s", hipGetErrorString(e));
    g_bwd_launches.fetch_add(2, std::memory_order_relaxed);
    return 0;
}

}  // extern "C"
