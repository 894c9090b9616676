// gcdm_ops.gcp2.hip.h -- one stand-alone GCP2 module (GCP2.forward, reference gcpnet.py:418-491 + process_vector_with_frames :378-415) as one
// training operator, forward and backward: the embedding GCPs, the feed-forward GCP and the position GCP of an interaction layer, the scalar
// projection.  C ABI: include/gcdm_gcp2_train.h.  Exact fp32 (every GEMM on gops::tile_mma, gcdm_ops.tile.hip.h, its A operand computed on
// load where the kernels below say so); no float atomics; a row's results depend on that row alone (the MFMA accumulates each row over k in a
// fixed order), so they are the same bits whatever M is.
//
// Forward, 2 launches (3 with feedforward_out):
//   k_gcp2_down     one wave per row: vh = vector_down(v), X = [s | |vh| | q] (q: the frame scalars of vector_down_frames(v)), and
//                   vector_up(vh) written straight into v_out;
//   (gops::gemm     hid = X W0^T + b0 when feedforward_out;)
//   k_gcp2_scalar   one workgroup per 64 rows, all SO columns in 64-wide tiles: p = A W^T + b (A = X, or silu(hid) applied on load), s_out =
//                   act0(p); act1(p) goes through LDS into the gate GEMM of the same rows, whose epilogue scales v_out by sigmoid(gate).
// Backward, 5 launches (6 with feedforward_out):
//   k_gcp2_gate_bwd dp = ds_out act0'(p) + (dgate W_g) act1'(p); the A operand dgate is computed on load (vector_up and the sigmoid are
//                   recomputed from vh and the gate pre-activation), dup / dgate are kept for the weight gradients;
//   (k_gcp2_ff_bwd  dhid = (dp W2) silu'(hid) when feedforward_out;)
//   gops::gemm      dX = dp W_s (dhid W0);
//   k_gcp2_down_bwd one wave per row: norms, frame scalars and the two down projections -> ds, dv, and dvh / du / v in the "pre" layout for
//   gops::wgrad_launch: every weight gradient, biases included, in one grouped split-K launch and one slice reduction.
#pragma once

namespace ggcp {

using namespace gops;

struct Dims {
    int64_t M;
    int SI, VI, SO, VO, H, K, ff, a0, a1;
};

// positions in the weight table (include/gcdm_gcp2_train.h)
struct WIdx {
    int wd, wdf, ws, bs, w2, b2, wup, wg, bg, n;
};
inline WIdx weight_index(const Dims& d) {
    WIdx w;
    int i = 0;
    w.wd = i++; w.wdf = i++; w.ws = i++; w.bs = i++;
    w.w2 = w.b2 = -1;
    if (d.ff) { w.w2 = i++; w.b2 = i++; }
    w.wup = w.wg = w.bg = -1;
    if (d.VO) { w.wup = i++; w.wg = i++; w.bg = i++; }
    w.n = i;
    return w;
}
constexpr int MAXW = 9;
inline void weight_sizes(const Dims& d, int64_t* n) {
    const WIdx w = weight_index(d);
    n[w.wd] = (int64_t)d.H * d.VI; n[w.wdf] = (int64_t)3 * d.VI; n[w.ws] = (int64_t)d.SO * d.K; n[w.bs] = d.SO;
    if (d.ff) { n[w.w2] = (int64_t)d.SO * d.SO; n[w.b2] = d.SO; }
    if (d.VO) { n[w.wup] = (int64_t)d.VO * d.H; n[w.wg] = (int64_t)d.VO * d.SO; n[w.bg] = d.VO; }
}
inline int64_t weight_total(const Dims& d) {
    int64_t n[MAXW], t = 0;
    weight_sizes(d, n);
    for (int i = 0; i < weight_index(d).n; ++i) t += n[i];
    return t;
}

// Workspace of gcdm_gcp2_fwd, offsets in floats (-1: not kept).  tape = 1: everything the backward reads beyond s, v and the weights.
struct FwdLayout {
    int64_t x, hid, vh, p, gate, total;
};
inline FwdLayout fwd_layout(const Dims& d, int tape) {
    FwdLayout L;
    Arena ar;
    L.x = ar.take(d.M * d.K);
    L.hid = d.ff ? ar.take(d.M * d.SO) : -1;
    L.vh = tape ? ar.take(d.M * 3 * d.H) : -1;
    L.p = tape ? ar.take(d.M * d.SO) : -1;
    L.gate = (tape && d.VO) ? ar.take(d.M * d.VO) : -1;
    L.total = ar.o;
    return L;
}
struct BwdLayout {
    int64_t one, vpre, dvh, du, dup, dgate, dp, ga, dhid, a2, dx, part, total;
};
inline BwdLayout bwd_layout(const Dims& d) {
    BwdLayout L;
    Arena ar;
    L.one = ar.take(1);                         // 1.0f: the B operand of the bias gradients (stride 0)
    L.vpre = ar.take(d.M * 3 * d.VI);           // v in the "pre" layout [M][3][VI]
    L.dvh = ar.take(d.M * 3 * d.H);
    L.du = ar.take(d.M * 9);
    L.dup = d.VO ? ar.take(d.M * 3 * d.VO) : -1;
    L.dgate = d.VO ? ar.take(d.M * d.VO) : -1;
    L.dp = ar.take(d.M * d.SO);
    L.ga = d.VO ? ar.take(d.M * d.SO) : -1;     // act1(p): the input of the gate GEMM, recomputed
    L.dhid = d.ff ? ar.take(d.M * d.SO) : -1;
    L.a2 = d.ff ? ar.take(d.M * d.SO) : -1;     // silu(hid), recomputed
    L.dx = ar.take(d.M * d.K);
    L.part = ar.take((int64_t)WG_SLICES * weight_total(d));
    L.total = ar.o;
    return L;
}

// the module's activation flags (Dims a0, a1: silu or none) as a gops::ACT_* kind; the two-way choice stays visible to the compiler
__device__ __forceinline__ int act_kind(int silu) { return silu ? ACT_SILU : ACT_NONE; }

// ---- A operands computed on load (gops::FunctorA) ------------------------------------------------------------------------------------------------
template <int SILU>
struct RowMajorA {
    const float* A;
    int64_t lda;
    __device__ __forceinline__ float operator()(int64_t r, int64_t k) const {
        return act_f(act_kind(SILU), A[r * lda + k]);
    }
};

// ---- forward: down projections, norms, frame scalars, vector_up (one 64-lane wave per row, 4 rows per workgroup) -------------------------------
__global__ __launch_bounds__(256) void k_gcp2_down(Dims d, const float* __restrict__ s, const float* __restrict__ v, const float* __restrict__ F,
                                                   const uint8_t* __restrict__ mask, const float* __restrict__ wd, const float* __restrict__ wdf,
                                                   const float* __restrict__ wup, float* __restrict__ X, float* __restrict__ vh_out,
                                                   float* __restrict__ v_out) {
    __shared__ float vp[4][3][GCDM_GCP2_MAX_VI];
    __shared__ float vhs[4][3][GCDM_GCP2_MAX_H];
    __shared__ float fr[4][9];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + w;
    const bool on = m < d.M;
    const int VI = d.VI, H = d.H;
    if (on) {
        for (int j = lane; j < 3 * VI; j += 64) vp[w][j % 3][j / 3] = v[m * 3 * VI + j];          // rep [VI][3] -> pre [3][VI]
        if (lane < 9) fr[w][lane] = (mask && !mask[m]) ? 0.f : F[m * 9 + lane];
        for (int c = lane; c < d.SI; c += 64) X[m * d.K + c] = s[m * d.SI + c];
    }
    __syncthreads();
    if (on) {
        for (int j = lane; j < H + 3; j += 64) {
            const bool isv = j < H;
            const float* wrow = isv ? wd + (int64_t)j * VI : wdf + (int64_t)(j - H) * VI;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
            for (int c = 0; c < VI; ++c) {
                const float wv = wrow[c];
                a0 += wv * vp[w][0][c]; a1 += wv * vp[w][1][c]; a2 += wv * vp[w][2][c];
            }
            if (isv) {
                vhs[w][0][j] = a0; vhs[w][1][j] = a1; vhs[w][2][j] = a2;
                if (vh_out) {
                    float* o = vh_out + m * 3 * H;
                    o[j] = a0; o[H + j] = a1; o[2 * H + j] = a2;
                }
                X[m * d.K + d.SI + j] = sqrtf(a0 * a0 + a1 * a1 + a2 * a2 + 1e-8f) + 1e-8f;
            } else {
                const int c = j - H;
                const float* f = fr[w];
#pragma unroll
                for (int r = 0; r < 3; ++r) X[m * d.K + d.SI + H + 3 * c + r] = f[3 * r] * a0 + f[3 * r + 1] * a1 + f[3 * r + 2] * a2;
            }
        }
    }
    __syncthreads();
    if (!on) return;
    for (int c = lane; c < d.VO; c += 64) {
        float u0 = 0.f, u1 = 0.f, u2 = 0.f;
        for (int h = 0; h < H; ++h) {
            const float wv = wup[c * H + h];
            u0 += wv * vhs[w][0][h]; u1 += wv * vhs[w][1][h]; u2 += wv * vhs[w][2][h];
        }
        float* o = v_out + (m * d.VO + c) * 3;
        o[0] = u0; o[1] = u1; o[2] = u2;
    }
}

// ---- forward: p = A W^T + b over all SO columns of 64 rows, s_out = act0(p), gate = act1(p) W_g^T + b_g, v_out *= sigmoid(gate) ----------------
// A = X (lda = K) or, with ASILU, silu(hid) (lda = SO).  v_out holds vector_up(vh) on entry (k_gcp2_down).
// In bf16x6 mode (MODE, gcdm_ops.tile.hip.h) the gate contraction is a second pass of the tile body over Ps, so its operands are split like any other's.
struct PsA {
    const float (*Ps)[GM + 1];
    int64_t m0;
    int n0;
    __device__ __forceinline__ float operator()(int64_t r, int64_t k) const { return Ps[k - n0][r - m0]; }
};
template <int ASILU, int MODE>
__global__ __launch_bounds__(256) void k_gcp2_scalar(Dims d, const float* __restrict__ A, int64_t Kd, const float* __restrict__ W, const float* __restrict__ bias,
                                                     const float* __restrict__ Wg, const float* __restrict__ bg, float* __restrict__ p_out,
                                                     float* __restrict__ s_out, float* __restrict__ gate_out, float* __restrict__ v_out) {
    __shared__ typename TileLds<MODE>::type As[2], Bs[2];
    __shared__ float Ps[GN][GM + 1];                       // act1(p) of the current column tile, [column][row]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int64_t m0 = (int64_t)blockIdx.x * GM;
    const int cl = wn * 32 + (lane & 31);                  // this lane's column inside a tile (of p, and of the gate)
    const FunctorA<RowMajorA<ASILU>> aload{{A, Kd}};
    f32x16 gacc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < d.SO; n0 += GN) {
        const f32x16 acc = tile_body<MODE>(aload, W, 1, Kd, m0, n0, d.M, d.SO, 0, Kd, As, Bs);
        const int col = n0 + cl;
        const bool cv = col < d.SO;
        const float bv = cv ? bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = tile_row(wm, lane, r);
            const int64_t row = m0 + rl;
            const bool ok = cv && row < d.M;
            const float pv = acc[r] + bv;
            if (ok) {
                if (p_out) p_out[row * d.SO + col] = pv;
                s_out[row * d.SO + col] = act_f(act_kind(d.a0), pv);
            }
            if (d.VO) Ps[cl][rl] = ok ? act_f(act_kind(d.a1), pv) : 0.f;
        }
        if constexpr (MODE == MM_BF16X6) {
            if (d.VO) {
                __syncthreads();
                // gate[m][c] += sum_k Ps[k][m] W_g[c][n0 + k]: B(k, n = c) = W_g[c * SO + k], k in [n0, min(n0 + GN, SO))
                const int k1 = n0 + GN < d.SO ? n0 + GN : d.SO;
                gacc += tile_body<MODE>(FunctorA<PsA>{{Ps, m0, n0}}, Wg, 1, d.SO, m0, 0, d.M, d.VO, n0, k1, As, Bs);
            }
        } else if (d.VO) {
            __syncthreads();
            const bool gv = cl < d.VO;
            const float* wg = Wg + (int64_t)(gv ? cl : 0) * d.SO + n0;
#pragma unroll 8
            for (int kk = 0; kk < GN; kk += 2) {
                const int kq = kk + (lane >> 5);
                const float a = Ps[kq][wm * 32 + (lane & 31)];
                const float b = (gv && n0 + kq < d.SO) ? wg[kq] : 0.f;
                gacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, gacc, 0, 0, 0);
            }
            // the next tile's tile_mma passes a barrier before Ps is written again
        }
    }
    if (d.VO && cl < d.VO) {
        const float bgv = bg[cl];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = m0 + tile_row(wm, lane, r);
            if (row < d.M) {
                const float g = gacc[r] + bgv;
                if (gate_out) gate_out[row * d.VO + cl] = g;
                const float sg = sigm_f(g);
                float* o = v_out + (row * d.VO + cl) * 3;
                o[0] *= sg; o[1] *= sg; o[2] *= sg;
            }
        }
    }
}

// ---- backward: dp = ds_out act0'(p) + (dgate W_g) act1'(p), ga = act1(p) ------------------------------------------------------------------------
// dgate[m][c] = (dv_out[m][c] . up[m][c]) sg (1 - sg), dup[m][x][c] = dv_out[m][c][x] sg, with up = vector_up(vh) and sg = sigmoid(gate)
// recomputed where the GEMM loads its A operand; the workgroups of the first column tile keep dup and dgate for the weight gradients.
struct DgateA {
    const float* vh; const float* wup; const float* gate; const float* dv_out;
    float* dup; float* dgate;
    int H, VO;
    bool keep;
    __device__ __forceinline__ float operator()(int64_t r, int64_t c) const {
        const float* p = vh + r * 3 * H;
        const float* w = wup + c * H;
        float u0 = 0.f, u1 = 0.f, u2 = 0.f;
        for (int h = 0; h < H; ++h) {
            const float wv = w[h];
            u0 += wv * p[h]; u1 += wv * p[H + h]; u2 += wv * p[2 * H + h];
        }
        const float sg = sigm_f(gate[r * VO + c]);
        const float* g = dv_out + (r * VO + c) * 3;
        const float g0 = g[0], g1 = g[1], g2 = g[2];
        const float dg = (g0 * u0 + g1 * u1 + g2 * u2) * sg * (1.f - sg);
        if (keep) {
            float* o = dup + r * 3 * VO + c;
            o[0] = g0 * sg; o[VO] = g1 * sg; o[2 * VO] = g2 * sg;
            dgate[r * VO + c] = dg;
        }
        return dg;
    }
};
template <int MODE>
__global__ __launch_bounds__(256) void k_gcp2_gate_bwd(Dims d, const float* __restrict__ ds_out, const float* __restrict__ dv_out, const float* __restrict__ p,
                                                       const float* __restrict__ vh, const float* __restrict__ gate, const float* __restrict__ wup,
                                                       const float* __restrict__ Wg, float* __restrict__ dup, float* __restrict__ dgate,
                                                       float* __restrict__ dp, float* __restrict__ ga, float* __restrict__ one) {
    __shared__ typename TileLds<MODE>::type As[2], Bs[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int64_t m0 = (int64_t)blockIdx.x * GM;
    const int n0 = blockIdx.y * GN;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *one = 1.f;
    const FunctorA<DgateA> aload{{vh, wup, gate, dv_out, dup, dgate, d.H, d.VO, blockIdx.y == 0}};
    const f32x16 acc = tile_body<MODE>(aload, Wg, d.SO, 1, m0, n0, d.M, d.SO, 0, d.VO, As, Bs);      // B(k = c, n) = W_g[c][n]
    const int col = n0 + wn * 32 + (lane & 31);
    if (col >= d.SO) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t row = m0 + tile_row(wm, lane, r);
        if (row < d.M) {
            const int64_t i = row * d.SO + col;
            const float pv = p[i];
            float g = ds_out[i] * act_df(act_kind(d.a0), pv);
            if (d.VO) {
                g += acc[r] * act_df(act_kind(d.a1), pv);
                ga[i] = act_f(act_kind(d.a1), pv);
            }
            dp[i] = g;
        }
    }
}

// ---- backward, feedforward_out: dhid = (dp W2) silu'(hid), a2 = silu(hid) -----------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void k_gcp2_ff_bwd(Dims d, const float* __restrict__ dp, const float* __restrict__ W2, const float* __restrict__ hid,
                                                     float* __restrict__ dhid, float* __restrict__ a2) {
    __shared__ typename TileLds<MODE>::type As[2], Bs[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int64_t m0 = (int64_t)blockIdx.x * GM;
    const int n0 = blockIdx.y * GN;
    const FunctorA<RowMajorA<0>> aload{{dp, d.SO}};
    const f32x16 acc = tile_body<MODE>(aload, W2, d.SO, 1, m0, n0, d.M, d.SO, 0, d.SO, As, Bs);       // B(k, n) = W2[k][n]
    const int col = n0 + wn * 32 + (lane & 31);
    if (col >= d.SO) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t row = m0 + tile_row(wm, lane, r);
        if (row < d.M) {
            const int64_t i = row * d.SO + col;
            const float hv = hid[i];
            dhid[i] = acc[r] * act_df(ACT_SILU, hv);
            a2[i] = act_f(ACT_SILU, hv);
        }
    }
}

// ---- backward: norms, frame scalars and down projections (one wave per row, 4 rows per workgroup) -----------------------------------------------
// in: dX, dup, the tape's vh.  out: ds = dX[:, :SI], dv (rep layout), and for the weight gradients dvh [M][3][H], du [M][3][3], vpre [M][3][VI].
__global__ __launch_bounds__(256) void k_gcp2_down_bwd(Dims d, const float* __restrict__ dX, const float* __restrict__ dup, const float* __restrict__ vh,
                                                       const float* __restrict__ v, const float* __restrict__ wup, const float* __restrict__ wd,
                                                       const float* __restrict__ wdf, const float* __restrict__ F, const uint8_t* __restrict__ mask,
                                                       float* __restrict__ dvh_out, float* __restrict__ du_out, float* __restrict__ vpre,
                                                       float* __restrict__ ds, float* __restrict__ dv) {
    __shared__ float gv[4][3][GCDM_GCP2_MAX_H + 3];        // dvh (H) then du (3)
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + w;
    const bool on = m < d.M;
    const int VI = d.VI, H = d.H, VO = d.VO;
    if (on) {
        const float* gx = dX + m * d.K + d.SI;
        for (int j = lane; j < H + 3; j += 64) {
            float g0, g1, g2;
            if (j < H) {
                const float* p = vh + m * 3 * H;
                const float a0 = p[j], a1 = p[H + j], a2 = p[2 * H + j];
                const float t = gx[j] / sqrtf(a0 * a0 + a1 * a1 + a2 * a2 + 1e-8f);
                g0 = t * a0; g1 = t * a1; g2 = t * a2;
                if (VO) {
                    const float* q = dup + m * 3 * VO;
                    for (int c = 0; c < VO; ++c) {
                        const float wv = wup[c * H + j];
                        g0 += q[c] * wv; g1 += q[VO + c] * wv; g2 += q[2 * VO + c] * wv;
                    }
                }
                float* o = dvh_out + m * 3 * H;
                o[j] = g0; o[H + j] = g1; o[2 * H + j] = g2;
            } else {
                const int c = j - H;
                float f[9];
                const bool off = mask && !mask[m];
#pragma unroll
                for (int i = 0; i < 9; ++i) f[i] = off ? 0.f : F[m * 9 + i];
                const float q0 = gx[H + 3 * c], q1 = gx[H + 3 * c + 1], q2 = gx[H + 3 * c + 2];
                g0 = f[0] * q0 + f[3] * q1 + f[6] * q2;
                g1 = f[1] * q0 + f[4] * q1 + f[7] * q2;
                g2 = f[2] * q0 + f[5] * q1 + f[8] * q2;
                float* o = du_out + m * 9;
                o[c] = g0; o[3 + c] = g1; o[6 + c] = g2;
            }
            gv[w][0][j] = g0; gv[w][1][j] = g1; gv[w][2][j] = g2;
        }
    }
    __syncthreads();
    if (!on) return;
    for (int j = lane; j < VI; j += 64) {
        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
        for (int h = 0; h < H; ++h) {
            const float wv = wd[(int64_t)h * VI + j];
            r0 += gv[w][0][h] * wv; r1 += gv[w][1][h] * wv; r2 += gv[w][2][h] * wv;
        }
        for (int c = 0; c < 3; ++c) {
            const float wv = wdf[(int64_t)c * VI + j];
            r0 += gv[w][0][H + c] * wv; r1 += gv[w][1][H + c] * wv; r2 += gv[w][2][H + c] * wv;
        }
        float* o = dv + (m * VI + j) * 3;
        o[0] = r0; o[1] = r1; o[2] = r2;
        const float* vi = v + (m * VI + j) * 3;
        float* t = vpre + m * 3 * VI + j;
        t[0] = vi[0]; t[VI] = vi[1]; t[2 * VI] = vi[2];
    }
    for (int c = lane; c < d.SI; c += 64) ds[m * d.SI + c] = dX[m * d.K + c];
}

}  // namespace ggcp

// ------------------------------------------------------------------------------------------------------------------------------------------
// C ABI (include/gcdm_gcp2_train.h)
// ------------------------------------------------------------------------------------------------------------------------------------------
static inline bool ggcp_dims_ok(int64_t M, const gcdm_gcp2_dims* q) {
    return q && M >= 0 && M <= GCDM_GCP2_MAX_ROWS && q->SI >= 1 && q->SI <= GCDM_GCP2_MAX_SI && q->VI >= 1 && q->VI <= GCDM_GCP2_MAX_VI && q->SO >= 1 &&
           q->SO <= GCDM_GCP2_MAX_SO && q->VO >= 0 && q->VO <= GCDM_GCP2_MAX_VO && q->H >= 1 && q->H <= GCDM_GCP2_MAX_H && gops_flag(q->feedforward_out) &&
           gops_flag(q->act_scalar) && gops_flag(q->act_vector);
}
static inline ggcp::Dims ggcp_make_dims(int64_t M, const gcdm_gcp2_dims* q) {
    ggcp::Dims d;
    d.M = M; d.SI = q->SI; d.VI = q->VI; d.SO = q->SO; d.VO = q->VO; d.H = q->H; d.K = q->SI + q->H + 9;
    d.ff = q->feedforward_out; d.a0 = q->act_scalar; d.a1 = q->act_vector;
    return d;
}
static inline bool ggcp_weights_ok(const float* const* w, int n) {
    if (!w) return false;
    for (int i = 0; i < n; ++i)
        if (!w[i]) return false;
    return true;
}

extern "C" {

int64_t gcdm_gcp2_workspace_bytes(int32_t which, int64_t M, const gcdm_gcp2_dims* dims) {
    GOPS_REQUIRE(which >= 0 && which <= 3 && ggcp_dims_ok(M, dims));
    const ggcp::Dims d = ggcp_make_dims(M, dims);
    if (which <= 1) return 4 * ggcp::fwd_layout(d, which).total;
    if (which == 2) return 4 * ggcp::bwd_layout(d).total;
    return 4 * ggcp::weight_total(d);
}

int gcdm_gcp2_fwd(const float* s, const float* v, const float* F, const uint8_t* row_mask, const float* const* weights, float* s_out, float* v_out,
                  float* workspace, int32_t tape, int64_t M, const gcdm_gcp2_dims* dims, void* stream) {
    using namespace ggcp;
    GOPS_REQUIRE(ggcp_dims_ok(M, dims) && gops_flag(tape));
    if (M == 0) return 0;
    const Dims d = ggcp_make_dims(M, dims);
    const WIdx wi = weight_index(d);
    GOPS_REQUIRE(s && v && F && s_out && workspace && (v_out || !d.VO) && ggcp_weights_ok(weights, wi.n));
    const float* const* W = weights;
    const hipStream_t st = (hipStream_t)stream;
    const int mode = gops_matrix_mode();         // read once: every GEMM launch of this call runs in it
    auto gemm = [&](auto... a) { gops::gemm(a..., 1, mode); };
    const FwdLayout L = fwd_layout(d, tape);
    float* ws = workspace;
    float* X = ws + L.x;
    float* vh = tape ? ws + L.vh : nullptr;
    float* p = tape ? ws + L.p : nullptr;
    float* gate = (tape && d.VO) ? ws + L.gate : nullptr;
    const float* wup = d.VO ? W[wi.wup] : nullptr;
    const float* wg = d.VO ? W[wi.wg] : nullptr;
    const float* bg = d.VO ? W[wi.bg] : nullptr;
    hipLaunchKernelGGL(k_gcp2_down, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, d, s, v, F, row_mask, W[wi.wd], W[wi.wdf], wup, X, vh, v_out);
    const dim3 rows((unsigned)((M + GM - 1) / GM));
    if (d.ff) {
        float* hid = ws + L.hid;
        gemm(X, d.K, 1, W[wi.ws], 1, d.K, hid, W[wi.bs], M, d.SO, d.K, st);                         // hid = X W0^T + b0
        GOPS_LAUNCH_MODE2(mode, k_gcp2_scalar, 1, rows, dim3(256), 0, st, d, (const float*)hid, (int64_t)d.SO, W[wi.w2], W[wi.b2], wg, bg, p, s_out, gate, v_out);
    } else {
        GOPS_LAUNCH_MODE2(mode, k_gcp2_scalar, 0, rows, dim3(256), 0, st, d, (const float*)X, (int64_t)d.K, W[wi.ws], W[wi.bs], wg, bg, p, s_out, gate, v_out);
    }
    return GOPS_LAUNCH_OK();
}

int gcdm_gcp2_bwd(const float* ds_out, const float* dv_out, const float* s, const float* v, const float* F, const uint8_t* row_mask,
                  const float* const* weights, const float* tape, float* workspace, float* ds, float* dv, float* dweights, int64_t M,
                  const gcdm_gcp2_dims* dims, void* stream) {
    using namespace ggcp;
    GOPS_REQUIRE(ggcp_dims_ok(M, dims));
    if (M == 0) return 0;
    const Dims d = ggcp_make_dims(M, dims);
    const WIdx wi = weight_index(d);
    GOPS_REQUIRE(ds_out && (dv_out || !d.VO) && s && v && F && tape && workspace && ds && dv && dweights && ggcp_weights_ok(weights, wi.n));
    (void)s;                                   // the merged row on the tape holds it
    const float* const* W = weights;
    const hipStream_t st = (hipStream_t)stream;
    const int mode = gops_matrix_mode();         // read once: every GEMM launch of this call runs in it
    auto gemm = [&](auto... a) { gops::gemm(a..., 1, mode); };
    const FwdLayout T = fwd_layout(d, 1);
    const BwdLayout L = bwd_layout(d);
    const float* t = tape;
    float* ws = workspace;
    const float* vh = t + T.vh;
    const float* wup = d.VO ? W[wi.wup] : nullptr;
    float* dup = d.VO ? ws + L.dup : nullptr;
    float* dgate = d.VO ? ws + L.dgate : nullptr;
    float* ga = d.VO ? ws + L.ga : nullptr;
    const dim3 tiles((unsigned)((M + GM - 1) / GM), (unsigned)((d.SO + GN - 1) / GN));
    GOPS_LAUNCH_MODE(mode, k_gcp2_gate_bwd, tiles, dim3(256), 0, st, d, ds_out, dv_out, t + T.p, vh, d.VO ? t + T.gate : nullptr, wup,
                       d.VO ? W[wi.wg] : nullptr, dup, dgate, ws + L.dp, ga, ws + L.one);
    const float* dpre = ws + L.dp;             // the gradient of what scalar_out's first Linear produced
    if (d.ff) {
        GOPS_LAUNCH_MODE(mode, k_gcp2_ff_bwd, tiles, dim3(256), 0, st, d, (const float*)(ws + L.dp), W[wi.w2], t + T.hid, ws + L.dhid, ws + L.a2);
        dpre = ws + L.dhid;
    }
    gemm(dpre, d.SO, 1, W[wi.ws], d.K, 1, ws + L.dx, nullptr, M, d.K, d.SO, st);                       // dX = dpre . W_s
    hipLaunchKernelGGL(k_gcp2_down_bwd, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, d, (const float*)(ws + L.dx), (const float*)dup, vh, v, wup,
                       W[wi.wd], W[wi.wdf], F, row_mask, ws + L.dvh, ws + L.du, ws + L.vpre, ds, dv);

    // every weight gradient of the module: one grouped split-K launch, one fixed-order slice reduction
    int64_t sz[MAXW], off[MAXW];
    weight_sizes(d, sz);
    WgTable G;
    G.total = wgrad_offsets(sz, wi.n, off);
    const float* one = ws + L.one;
    const float* vpre = ws + L.vpre;
    G.add(ws + L.dvh, 1, d.H, vpre, d.VI, 1, d.H, d.VI, 3 * M, off[wi.wd], d.VI);                            // dW_down = sum_(m,x) dvh^T v_pre
    G.add(ws + L.du, 1, 3, vpre, d.VI, 1, 3, d.VI, 3 * M, off[wi.wdf], d.VI);                                // dW_down_frames
    G.add(dpre, 1, d.SO, t + T.x, d.K, 1, d.SO, d.K, M, off[wi.ws], d.K);                                    // dW_s = dpre^T X
    G.add(dpre, 1, d.SO, one, 0, 0, d.SO, 1, M, off[wi.bs], 1);
    if (d.ff) {
        G.add(ws + L.dp, 1, d.SO, ws + L.a2, d.SO, 1, d.SO, d.SO, M, off[wi.w2], d.SO);                      // dW_2 = dp^T silu(hid)
        G.add(ws + L.dp, 1, d.SO, one, 0, 0, d.SO, 1, M, off[wi.b2], 1);
    }
    if (d.VO) {
        G.add(dup, 1, d.VO, vh, d.H, 1, d.VO, d.H, 3 * M, off[wi.wup], d.H);                                 // dW_up = sum dup^T vh
        G.add(dgate, 1, d.VO, ga, d.SO, 1, d.VO, d.SO, M, off[wi.wg], d.SO);                                 // dW_gate = dgate^T act1(p)
        G.add(dgate, 1, d.VO, one, 0, 0, d.VO, 1, M, off[wi.bg], 1);
    }
    wgrad_launch(G, ws + L.part, dweights, st, mode);
    return GOPS_LAUNCH_OK();
}

}  // extern "C"
