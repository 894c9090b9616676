// gcdm_ops.mp_tile.hip.h -- the "tiled" message path: the fused message layer of gcdm_ops.mp_train.hip.h with each message GCP's scalar GEMM,
// activation, gate GEMM and gated vector update in ONE tile kernel (forward), and its gate backward, d gate_in GEMM and activation backward in
// ONE tile kernel (backward) -- the pattern of k_gcp2_scalar / k_gcp2_gate_bwd (gcdm_ops.gcp2.hip.h) at M = E.  C ABI: include/gcdm_mp_tile.h.
// Everything else (pack, down projections, attention, aggregation, node sums, weight gradients, the layouts) is gcdm_ops.mp_train.hip.h's, as
// it is.  Same tile body, same k order, no float atomics: a row's result depends on that row alone and is the same bits from run to run.
//
// Forward, 12 launches:  k_mp_pack, gops::gemm (aij), 4 x (k_mp_down, k_mp_tile), k_mp_att, k_mp_agg.
// Backward, 17 launches: k_mp_att_bwd, 4 x (k_mp_tile_bwd, gops::gemm (dX), k_mp_down_bwd), k_mp_node_sum, gops::gemm (dh), k_wgrad_grouped,
//                        k_reduce_slices.
// The tape is gcdm_mp_fwd's (fwd_layout(d, 1)) except that `g` is never written: either forward's tape serves either backward.
#pragma once

namespace gmp {

// Workspace of gcdm_mp_tile_fwd.  With a tape: fwd_layout(d, 1).  Without: no spre and no g, and TWO X buffers -- k_mp_tile writes its rows'
// next scalar state while later column tiles of the same rows still read X, so X[k + 1] must not be X[k] (x: 1 -> 2 -> 1).
inline FwdLayout tile_fwd_layout(const Dims& d, int tape) {
    if (tape) return fwd_layout(d, 1);
    FwdLayout L;
    Arena ar;
    const int64_t E = d.E;
    L.wij = ar.take((int64_t)2 * S * S);
    L.wr0 = ar.take((int64_t)S * d.K0);
    L.aij = ar.take(d.N * 2 * S);
    L.vpre0 = -1;
    L.x0 = ar.take(E * d.K0);
    L.x[0] = -1;
    L.x[1] = ar.take(E * KX);
    L.x[2] = ar.take(E * KX);
    L.x[3] = L.x[1];
    L.vst[0] = -1;
    L.vst[1] = L.vst[2] = L.vst[3] = ar.take(E * 3 * V);
    L.vh[0] = L.vh[1] = L.vh[2] = L.vh[3] = ar.take(E * 3 * d.H0);
    L.gate[0] = L.gate[1] = L.gate[2] = L.gate[3] = ar.take(E * V);
    for (int k = 0; k < 4; ++k) L.spre[k] = -1;
    L.g = -1;
    L.att = ar.take(E);
    L.total = ar.o;
    return L;
}
inline int64_t tile_fwd_floats(const Dims& d, int tape) { const FwdLayout L = tile_fwd_layout(d, tape); return fwd_vfin(d, L) + a4(d.E * 3 * V); }

// Scratch of gcdm_mp_tile_bwd: bwd_layout(d) without dg (d gate_in never leaves the tile)
inline BwdLayout tile_bwd_layout(const Dims& d) {
    BwdLayout L;
    Arena ar;
    const int64_t E = d.E;
    L.one = ar.take(1);
    L.ds = ar.take(E * S);
    L.dv = ar.take(E * 3 * V);
    L.dg = -1;
    L.dx = ar.take(E * (KX > d.K0 ? KX : d.K0));
    for (int k = 0; k < 4; ++k) {
        L.dspre[k] = ar.take(E * S); L.gk[k] = ar.take(E * S); L.dgate[k] = ar.take(E * V); L.dup[k] = ar.take(E * 3 * V);
        L.dvh[k] = ar.take(E * 3 * (k ? H : d.H0)); L.du[k] = ar.take(E * 3 * SV);
    }
    L.dlog = ar.take(E);
    L.dvrow = ar.take(E * 3 * V);
    L.dvcol = ar.take(E * 3 * V);
    L.rscs = ar.take(d.N * 2 * S);
    L.part = ar.take((int64_t)WG_SLICES * weight_total(d));
    L.total = ar.o;
    return L;
}

// silu(S_pre) of the current column tile as the A operand of the gate contraction (bf16x6 mode: a second pass of the tile body)
struct PsTileA {
    const float (*Ps)[GM + 1];
    int64_t m0;
    int n0;
    __device__ __forceinline__ float operator()(int64_t r, int64_t k) const { return Ps[k - n0][r - m0]; }
};

// ---- forward of message GCP k: one workgroup per 64 edges, the 256 scalar columns in 64-wide tiles ------------------------------------------
// S_pre = X W^T (+ the gathered node halves + b0 for K0, + bias otherwise), a = silu(S_pre), s_out = (K0 ? 0 : X[:, :S]) + a; a goes through LDS
// as [column][row] into the gate contraction of the same rows; then gate = gacc + b_g, v_out = (K0 ? 0 : v_in) + vector_up(vh) sigmoid(gate).
// K0: X = X0 [E][d.K0] against WR0 [S][d.K0]; otherwise X [E][KX] against scalar_out.weight [S][KX].  s_out must not be X (later column tiles
// still read it); v_out may be v_in (each element is read and written by one thread).  spre_out is null without a tape.
template <int K0, int MODE>
__global__ __launch_bounds__(256) void k_mp_tile(Dims d, const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias,
                                                 const float* __restrict__ aij, const int64_t* __restrict__ row, const int64_t* __restrict__ col,
                                                 const float* __restrict__ Wg, const float* __restrict__ bg, const float* __restrict__ wup,
                                                 const float* __restrict__ vh, float* __restrict__ spre_out, float* __restrict__ s_out, int ld_out,
                                                 float* __restrict__ gate_out, const float* v_in, float* v_out) {
    __shared__ typename TileLds<MODE>::type As[2], Bs[2];
    __shared__ float Ps[GN][GM + 1];                       // silu(S_pre) of the current column tile, [column][row]; at the end the gate, [channel][row]
    __shared__ int64_t ri[K0 ? GM : 1], ci[K0 ? GM : 1];   // K0: the tile's end points (row >= E: unused)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int64_t m0 = (int64_t)blockIdx.x * GM;
    const int cl = wn * 32 + (lane & 31);                  // this lane's column inside a tile
    const int Kd = K0 ? d.K0 : KX, hk = K0 ? d.H0 : H;
    if (K0 && tid < GM) {
        const bool on = m0 + tid < d.E;
        ri[tid] = on ? row[m0 + tid] : 0;
        ci[tid] = on ? col[m0 + tid] : 0;
    }                                                      // (read after the barriers of the first tile_body)
    f32x16 gacc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < S; n0 += GN) {
        const int c = n0 + cl;
        const float bv = bias[c];
        // what the epilogue adds, requested in one burst: the residual state before the tile's MFMAs (X is not written here), msg0's node
        // halves behind them (ri / ci are complete after the tile body's first barrier)
        float res[16], ai[K0 ? 16 : 1], aj[K0 ? 16 : 1];
        if (!K0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t e = m0 + tile_row(wm, lane, r);
                res[r] = e < d.E ? X[e * KX + c] : 0.f;
            }
        }
        const f32x16 acc = tile_body<MODE>(StridedA{X, Kd, 1}, W, 1, Kd, m0, n0, d.E, S, 0, Kd, As, Bs);
        if (K0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rl = tile_row(wm, lane, r);
                const bool on = m0 + rl < d.E;
                res[r] = 0.f;
                ai[r] = on ? aij[ri[rl] * 2 * S + c] : 0.f;
                aj[r] = on ? aij[ci[rl] * 2 * S + S + c] : 0.f;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = tile_row(wm, lane, r);
            const int64_t e = m0 + rl;
            float a = 0.f;
            if (e < d.E) {
                float v;
                if (K0) v = acc[r] + ai[r] + aj[r] + bv;
                else v = acc[r] + bv;
                if (spre_out) spre_out[e * S + c] = v;
                a = act_f(ACT_SILU, v);
                s_out[e * ld_out + c] = res[r] + a;
            }
            Ps[cl][rl] = a;
        }
        __syncthreads();
        if constexpr (MODE == MM_BF16X6) {
            // gate[e][ch] += sum_k Ps[k][e] W_g[ch][n0 + k]: B(k, n = ch) = W_g[ch * S + k], k in [n0, n0 + GN)
            gacc += tile_body<MODE>(FunctorA<PsTileA>{{Ps, m0, n0}}, Wg, 1, S, m0, 0, d.E, V, n0, n0 + GN, As, Bs);
        } else if (wn == 0) {                              // V = 32 gate channels: the waves of the first 32 columns
            const float* wg = Wg + (int64_t)cl * S + n0;
#pragma unroll 8
            for (int kk = 0; kk < GN; kk += 2) {
                const int kq = kk + (lane >> 5);
                gacc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ps[kq][wm * 32 + (lane & 31)], wg[kq], gacc, 0, 0, 0);
            }
            // the next tile's tile_mma passes a barrier before Ps is written again
        }
    }
    __syncthreads();                                       // the last gate contraction has read Ps
    if (wn == 0) {
        const float bgv = bg[cl];
#pragma unroll
        for (int r = 0; r < 16; ++r) Ps[cl][tile_row(wm, lane, r)] = gacc[r] + bgv;
    }
    __syncthreads();
    // one thread per (edge, channel), 8 edges each: vector_up in k_mp_vout's order (h ascending), the sigmoid, the residual
    const int ch = tid & 31, r0 = tid >> 5;
    float u[8][3];
    const float* p[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        u[j][0] = u[j][1] = u[j][2] = 0.f;
        const int64_t e = m0 + r0 + 8 * j;
        p[j] = e < d.E ? vh + e * 3 * hk : nullptr;
    }
#pragma unroll 1
    for (int h = 0; h < hk; ++h) {
        const float w = wup[ch * hk + h];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (p[j]) { u[j][0] += w * p[j][h]; u[j][1] += w * p[j][hk + h]; u[j][2] += w * p[j][2 * hk + h]; }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int rl = r0 + 8 * j;
        const int64_t e = m0 + rl;
        if (e >= d.E) continue;
        const float g = Ps[ch][rl];
        gate_out[e * V + ch] = g;
        const float sg = sigm_f(g);
        const int64_t o = e * 3 * V + ch;
        v_out[o] = (K0 ? 0.f : v_in[o]) + u[j][0] * sg;
        v_out[o + V] = (K0 ? 0.f : v_in[o + V]) + u[j][1] * sg;
        v_out[o + 2 * V] = (K0 ? 0.f : v_in[o + 2 * V]) + u[j][2] * sg;
    }
}

// ---- backward of message GCP k: dS_pre = (ds + dgate W_g) silu'(S_pre), gk = silu(S_pre) ---------------------------------------------------------
// dgate[e][c] = (dv[e][:][c] . up[e][:][c]) sg (1 - sg), dup[e][x][c] = dv[e][x][c] sg, with up = vector_up(vh) and sg = sigmoid(gate) recomputed
// where the GEMM loads its A operand (k_mp_vout_bwd's arithmetic; dv in the pre layout [E][3][V]); the workgroups of the first column tile keep
// dup and dgate for the weight gradients.
struct MpDgateA {
    const float* __restrict__ vh; const float* __restrict__ wup; const float* __restrict__ gate; const float* __restrict__ dv;
    float* __restrict__ dup; float* __restrict__ dgate;
    int hk;
    bool keep;
    __device__ __forceinline__ float operator()(int64_t e, int64_t c) const {
        const float* p = vh + e * 3 * hk;
        float u0 = 0.f, u1 = 0.f, u2 = 0.f;
#pragma unroll 4                                   // 16 loads in flight per wait instead of 4: the operand load is a chain of L1 round trips
        for (int h = 0; h < hk; ++h) {
            const float w = wup[c * hk + h];
            u0 += w * p[h]; u1 += w * p[hk + h]; u2 += w * p[2 * hk + h];
        }
        const float sg = sigm_f(gate[e * V + c]);
        const int64_t o = e * 3 * V + c;
        const float g0 = dv[o], g1 = dv[o + V], g2 = dv[o + 2 * V];
        const float dg = (g0 * u0 + g1 * u1 + g2 * u2) * sg * (1.f - sg);
        if (keep) {
            dup[o] = g0 * sg; dup[o + V] = g1 * sg; dup[o + 2 * V] = g2 * sg;
            dgate[e * V + c] = dg;
        }
        return dg;
    }
};
template <int MODE>
__global__ __launch_bounds__(256) void k_mp_tile_bwd(Dims d, int hk, const float* __restrict__ ds, const float* __restrict__ dv, const float* __restrict__ spre,
                                                     const float* __restrict__ vh, const float* __restrict__ gate, const float* __restrict__ wup,
                                                     const float* __restrict__ Wg, float* __restrict__ dup, float* __restrict__ dgate,
                                                     float* __restrict__ dspre, float* __restrict__ gk) {
    __shared__ typename TileLds<MODE>::type As[2], Bs[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int64_t m0 = (int64_t)blockIdx.x * GM;
    const int n0 = blockIdx.y * GN;
    const FunctorA<MpDgateA> aload{{vh, wup, gate, dv, dup, dgate, hk, blockIdx.y == 0}};
    // the epilogue's operands, requested in one burst before the tile: their latency runs under the operand load and the MFMAs
    const int c = n0 + wn * 32 + (lane & 31);
    float xs[16], dsv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t e = m0 + tile_row(wm, lane, r);
        xs[r] = e < d.E ? spre[e * S + c] : 0.f;
        dsv[r] = e < d.E ? ds[e * S + c] : 0.f;
    }
    const f32x16 acc = tile_body<MODE>(aload, Wg, S, 1, m0, n0, d.E, S, 0, V, As, Bs);                // B(k = c, n) = W_g[c][n]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t e = m0 + tile_row(wm, lane, r);
        if (e < d.E) {
            const int64_t i = e * S + c;
            gk[i] = act_f(ACT_SILU, xs[r]);
            dspre[i] = (dsv[r] + acc[r]) * act_df(ACT_SILU, xs[r]);
        }
    }
}

}  // namespace gmp

// ------------------------------------------------------------------------------------------------------------------------------------------
// C ABI (include/gcdm_mp_tile.h)
// ------------------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int64_t gcdm_mp_tile_workspace_bytes(int32_t which, int64_t N, int64_t E, int32_t SE, int32_t VE) {
    GOPS_REQUIRE(which >= 0 && which <= 3 && gmp_dims_ok(N, E, SE, VE));
    const gmp::Dims d = gmp::make_dims(N, E, SE, VE);
    if (which <= 1) return 4 * gmp::tile_fwd_floats(d, which);
    if (which == 2) return 4 * gmp::tile_bwd_layout(d).total;
    return 4 * gmp::weight_total(d);
}

int gcdm_mp_tile_fwd(const float* h, const float* vnode, const float* e, const float* xi, const int64_t* row, const int64_t* col, const int32_t* rowptr,
                     const float* frames, const uint8_t* edge_mask, const float* const* weights, float* agg, float* workspace, int32_t tape, int64_t N,
                     int64_t E, int32_t SE, int32_t VE, void* stream) {
    using namespace gmp;
    GOPS_REQUIRE(gmp_dims_ok(N, E, SE, VE) && gops_flag(tape));
    if (N == 0 || E == 0) return 0;
    GOPS_REQUIRE(h && vnode && e && xi && row && col && rowptr && frames && agg && workspace && gmp_weights_ok(weights));
    const float* const* W = weights;
    const hipStream_t st = (hipStream_t)stream;
    const Dims d = make_dims(N, E, SE, VE);
    const int mode = gops_matrix_mode();         // read once: every launch of this call runs in it
    const FwdLayout L = tile_fwd_layout(d, tape);
    float* ws = workspace;
    float* sfin = ws + fwd_sfin(L);
    float* vfin = ws + fwd_vfin(d, L);
    const int64_t npack = (int64_t)2 * S * S + (int64_t)S * d.K0;
    hipLaunchKernelGGL(k_mp_pack, dim3(gops_blocks(npack)), dim3(256), 0, st, W[2], ws + L.wij, ws + L.wr0, d);
    gops::gemm(h, S, 1, ws + L.wij, 1, S, ws + L.aij, nullptr, N, 2 * S, S, st, 1, mode);        // [A_i | A_j] = h [W_i ; W_j]^T
    const unsigned eb = (unsigned)((E + 3) / 4);
    const dim3 tiles((unsigned)((E + GM - 1) / GM));
    for (int k = 0; k < 4; ++k) {
        const float* const* Wk = W + 7 * k;
        float* X = ws + (k ? L.x[k] : L.x0);
        const float* vin = k ? ws + L.vst[k] : nullptr;
        float* vout = k < 3 ? ws + L.vst[k + 1] : vfin;
        float* spre = tape ? ws + L.spre[k] : nullptr;
        float* s_out = k < 3 ? ws + L.x[k + 1] : sfin;
        const int ld_out = k < 3 ? (int)KX : (int)S;
        const float* vh = ws + L.vh[k];
        hipLaunchKernelGGL(k_mp_down, dim3(eb), dim3(256), 0, st, k, d, vnode, xi, e, row, col, frames, edge_mask, vin, Wk[0], Wk[1],
                           (k == 0 && tape) ? ws + L.vpre0 : nullptr, ws + L.vh[k], X);
        if (k == 0)
            GOPS_LAUNCH_MODE2(mode, k_mp_tile, 1, tiles, dim3(256), 0, st, d, (const float*)X, (const float*)(ws + L.wr0), W[3], (const float*)(ws + L.aij), row,
                              col, Wk[5], Wk[6], Wk[4], vh, spre, s_out, ld_out, ws + L.gate[k], vin, vout);
        else
            GOPS_LAUNCH_MODE2(mode, k_mp_tile, 0, tiles, dim3(256), 0, st, d, (const float*)X, Wk[2], Wk[3], (const float*)nullptr, row, col, Wk[5], Wk[6],
                              Wk[4], vh, spre, s_out, ld_out, ws + L.gate[k], vin, vout);
    }
    hipLaunchKernelGGL(k_mp_att, dim3(eb), dim3(256), 0, st, d, sfin, W[28], W[29], ws + L.att);
    hipLaunchKernelGGL(k_mp_agg, dim3(gops_blocks(N * (S + 3 * V))), dim3(256), 0, st, d, rowptr, sfin, ws + L.att, vfin, agg);
    return GOPS_LAUNCH_OK();
}

int gcdm_mp_tile_bwd(const float* dagg, const float* h, const int64_t* row, const int64_t* col, const int32_t* rowptr, const int32_t* colptr,
                     const int64_t* colperm, const float* frames, const uint8_t* edge_mask, const float* const* weights, const float* tape,
                     float* workspace, float* dh, float* dvnode, float* de, float* dxi, float* dweights, int64_t N, int64_t E, int32_t SE, int32_t VE,
                     void* stream) {
    using namespace gmp;
    GOPS_REQUIRE(gmp_dims_ok(N, E, SE, VE));
    if (N == 0 || E == 0) return 0;
    GOPS_REQUIRE(dagg && h && row && col && rowptr && colptr && colperm && frames && tape && workspace && dh && dvnode && de && dxi && dweights &&
                 gmp_weights_ok(weights));
    (void)col;
    const float* const* W = weights;
    const hipStream_t st = (hipStream_t)stream;
    const Dims d = make_dims(N, E, SE, VE);
    const int mode = gops_matrix_mode();         // read once: every launch of this call runs in it
    auto gemm = [&](auto... a) { gops::gemm(a..., 1, mode); };
    const FwdLayout F = fwd_layout(d, 1);
    const BwdLayout L = tile_bwd_layout(d);
    const float* t = tape;
    float* ws = workspace;
    const unsigned eb = (unsigned)((E + 3) / 4);
    const dim3 tiles((unsigned)((E + GM - 1) / GM), S / GN);
    hipLaunchKernelGGL(k_mp_att_bwd, dim3(eb), dim3(256), 0, st, d, dagg, row, t + fwd_sfin(F), t + F.att, W[28], ws + L.ds, ws + L.dv, ws + L.dlog,
                       ws + L.one);
    for (int k = 3; k >= 0; --k) {
        const float* const* Wk = W + 7 * k;
        GOPS_LAUNCH_MODE(mode, k_mp_tile_bwd, tiles, dim3(256), 0, st, d, k ? (int)H : d.H0, (const float*)(ws + L.ds), (const float*)(ws + L.dv),
                         t + F.spre[k], t + F.vh[k], t + F.gate[k], Wk[4], Wk[5], ws + L.dup[k], ws + L.dgate[k], ws + L.dspre[k], ws + L.gk[k]);
        if (k) gemm(ws + L.dspre[k], S, 1, Wk[2], KX, 1, ws + L.dx, nullptr, E, KX, S, st);          // dX = dS_pre . W_s
        else gemm(ws + L.dspre[0], S, 1, t + F.wr0, d.K0, 1, ws + L.dx, nullptr, E, d.K0, S, st);
        hipLaunchKernelGGL(k_mp_down_bwd, dim3(eb), dim3(256), 0, st, k, d, ws + L.dx, ws + L.dup[k], t + F.vh[k], Wk[4], Wk[0], Wk[1], frames, edge_mask,
                           ws + L.dvh[k], ws + L.du[k], ws + L.ds, ws + L.dv, de, dxi, ws + L.dvrow, ws + L.dvcol);
    }
    hipLaunchKernelGGL(k_mp_node_sum, dim3(gops_blocks(N * (S + 3 * V))), dim3(256), 0, st, d, rowptr, colptr, colperm, ws + L.dspre[0], ws + L.dvrow,
                       ws + L.dvcol, ws + L.rscs, dvnode);
    gemm(ws + L.rscs, 2 * S, 1, t + F.wij, S, 1, dh, nullptr, N, S, 2 * S, st);                    // dh = [RS | CS] . [W_i ; W_j]
    wgrad_all(d, F, L, t, ws, h, dweights, st, mode);
    return GOPS_LAUNCH_OK();
}

}  // extern "C"
