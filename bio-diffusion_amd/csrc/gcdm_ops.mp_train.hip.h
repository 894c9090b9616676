// gcdm_ops.mp_train.hip.h -- the message function of one interaction layer (GCPMessagePassing.forward, reference gcpnet.py:676-737) as one
// training operator, forward and backward, for the configuration the fused sampling kernels take at the message layer: GCP2 with vector_gate,
// silu / silu, bottleneck 4, four residual message GCPs, scalar attention, sum aggregation, node dims (256, 32), edge dims (SE, VE) in
// {(64, 16), (16, 8)}.  C ABI: include/gcdm_mp_train.h.  Exact fp32 throughout (every GEMM is gops::gemm, every weight gradient one
// gops::wgrad_launch: gcdm_ops.tile.hip.h);
// no float atomics: every sum over edges runs in a fixed order, so two backward passes give the same bits.
//
// msg0 column split: W_s [h_i | e | h_j | |vh| | q] = W_i h_i + W_j h_j + W_r [e | |vh| | q] + b.  The node halves are one
// N-row GEMM (h against WIJ = [W_i ; W_j], packed once per call), gathered per edge; per edge only K0 = SE + H0 + 9 columns remain.  In the
// backward the node halves of dW and dh come from the row sums and column sums of dS0 (column order: a stable argsort of col + colptr).
//
// Layouts: scalars [E][C]; vector states in the "pre" layout [E][3][C] (what the down projections contract over); node vectors and the
// aggregate in the reference's "rep" layout.  Tape (grad mode): what the backward and the weight gradients read -- see fwd_layout().
#pragma once

namespace gmp {

using namespace gops;

constexpr int S = 256, V = 32, H = 8, SV = 3, KX = S + H + 3 * SV;       // message state width, vector channels, hidden of msg1-3, X width
constexpr int NW = 30;                                                 // weight tensors of the layer (include/gcdm_mp_train.h)

struct Dims {
    int64_t N, E;
    int SE, VE, VIN0, H0, K0, KIN0;
};
__host__ __device__ inline Dims make_dims(int64_t N, int64_t E, int SE, int VE) {
    Dims d;
    d.N = N; d.E = E; d.SE = SE; d.VE = VE;
    d.VIN0 = 2 * V + VE; d.H0 = d.VIN0 / 4; d.K0 = SE + d.H0 + 3 * SV; d.KIN0 = 2 * S + d.K0;
    return d;
}

// Workspace of gcdm_mp_fwd (tape = 1: everything the backward reads; tape = 0: the same buffers shared across the four GCPs) and of
// gcdm_mp_bwd.  Offsets in floats.
struct FwdLayout {
    int64_t wij, wr0, aij, vpre0, x0, x[4], vst[4], vh[4], spre[4], gate[4], g, att, total;
};
inline FwdLayout fwd_layout(const Dims& d, int tape) {
    FwdLayout L;
    Arena ar;
    const int64_t E = d.E;
    L.wij = ar.take((int64_t)2 * S * S);
    L.wr0 = ar.take((int64_t)S * d.K0);
    L.aij = ar.take(d.N * 2 * S);
    L.vpre0 = tape ? ar.take(E * 3 * d.VIN0) : -1;
    L.x0 = ar.take(E * d.K0);
    for (int k = 1; k < 4; ++k) L.x[k] = (tape || k == 1) ? ar.take(E * KX) : L.x[1];
    L.x[0] = -1;
    L.vst[0] = -1;
    for (int k = 1; k < 4; ++k) L.vst[k] = (tape || k == 1) ? ar.take(E * 3 * V) : L.vst[1];
    for (int k = 0; k < 4; ++k) L.vh[k] = (tape || k == 0) ? ar.take(E * 3 * (k ? H : d.H0)) : L.vh[0];
    for (int k = 0; k < 4; ++k) L.spre[k] = (tape || k == 0) ? ar.take(E * S) : L.spre[0];
    for (int k = 0; k < 4; ++k) L.gate[k] = (tape || k == 0) ? ar.take(E * V) : L.gate[0];
    L.g = ar.take(E * S);                       // silu(S_pre): input of the gate GEMM (recomputed in the backward)
    L.att = ar.take(E);
    L.total = ar.o;
    return L;
}
// the final message state: X[3]'s scalar columns are not it (msg3 adds a residual) -- it lives in `sfin`, after the layout above
inline int64_t fwd_sfin(const FwdLayout& L) { return L.total; }
inline int64_t fwd_vfin(const Dims& d, const FwdLayout& L) { return L.total + a4(d.E * S); }
inline int64_t fwd_floats(const Dims& d, int tape) { const FwdLayout L = fwd_layout(d, tape); return fwd_vfin(d, L) + a4(d.E * 3 * V); }

// weight-gradient sizes in the order of the weight table
inline void weight_sizes(const Dims& d, int64_t* n) {
    for (int k = 0; k < 4; ++k) {
        const int hk = k ? H : d.H0, vin = k ? V : d.VIN0, kin = k ? KX : d.KIN0;
        n[7 * k + 0] = (int64_t)hk * vin; n[7 * k + 1] = (int64_t)SV * vin; n[7 * k + 2] = (int64_t)S * kin; n[7 * k + 3] = S;
        n[7 * k + 4] = (int64_t)V * hk; n[7 * k + 5] = (int64_t)V * S; n[7 * k + 6] = V;
    }
    n[28] = S; n[29] = 1;
}
inline int64_t weight_total(const Dims& d) { int64_t n[NW], t = 0; weight_sizes(d, n); for (int i = 0; i < NW; ++i) t += n[i]; return t; }

struct BwdLayout {
    int64_t one, ds, dv, dg, dx, dspre[4], gk[4], dgate[4], dup[4], dvh[4], du[4], dlog, dvrow, dvcol, rscs, part, total;
};
inline BwdLayout bwd_layout(const Dims& d) {
    BwdLayout L;
    Arena ar;
    const int64_t E = d.E;
    L.one = ar.take(1);                         // 1.0f: the B operand of the bias gradients (stride 0)
    L.ds = ar.take(E * S);
    L.dv = ar.take(E * 3 * V);
    L.dg = ar.take(E * S);
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

// ---- pack: WIJ [2S][S] = [W_i ; W_j] (rows: output channel of the node half), WR0 [S][K0] = W_s0 columns [e | |vh| | q] ----------------------
__global__ void k_mp_pack(const float* __restrict__ ws0, float* __restrict__ wij, float* __restrict__ wr0, Dims d) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nij = (int64_t)2 * S * S;
    if (i < nij) {
        const int r = (int)(i / S), c = (int)(i % S);
        wij[i] = r < S ? ws0[(int64_t)r * d.KIN0 + c] : ws0[(int64_t)(r - S) * d.KIN0 + S + d.SE + c];
    } else if (i < nij + (int64_t)S * d.K0) {
        const int64_t j = i - nij;
        const int o = (int)(j / d.K0), c = (int)(j % d.K0);
        wr0[j] = ws0[(int64_t)o * d.KIN0 + (c < d.SE ? S + c : 2 * S + c)];
    }
}

// ---- forward: down projections, norms and frame scalars of GCP k (one 64-lane wave per edge, 4 edges per workgroup) -----------------------
// k = 0: v_pre = [V_i | xi | V_j] gathered (written to the tape when vpre0_out != null), X0 = [e | |vh| | q];
// k > 0: v_pre = the vector state [E][3][V], X = [s | |vh| | q] (s already in X's first S columns).
__global__ __launch_bounds__(256) void k_mp_down(int k, Dims d, const float* __restrict__ vnode, const float* __restrict__ xi, const float* __restrict__ e_in,
                                                 const int64_t* __restrict__ row, const int64_t* __restrict__ col, const float* __restrict__ F,
                                                 const uint8_t* __restrict__ emask, const float* __restrict__ vst, const float* __restrict__ wd,
                                                 const float* __restrict__ wdf, float* __restrict__ vpre0_out, float* __restrict__ vh_out,
                                                 float* __restrict__ X) {
    __shared__ float vp[4][3][2 * V + 16];
    __shared__ float fr[4][9];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 4 + w;
    const bool on = e < d.E;
    const int vin = k ? V : d.VIN0, hk = k ? H : d.H0, ldx = k ? KX : d.K0, off = k ? S : d.SE;
    if (on) {
        for (int j = lane; j < 3 * vin; j += 64) {
            const int x = j / vin, c = j % vin;
            float val;
            if (k) val = vst[e * 3 * V + j];
            else if (c < V) val = vnode[row[e] * 3 * V + c * 3 + x];
            else if (c < V + d.VE) val = xi[e * 3 * d.VE + (c - V) * 3 + x];
            else val = vnode[col[e] * 3 * V + (c - V - d.VE) * 3 + x];
            vp[w][x][c] = val;
            if (!k && vpre0_out) vpre0_out[e * 3 * vin + j] = val;
        }
        if (lane < 9) fr[w][lane] = (emask && !emask[e]) ? 0.f : F[e * 9 + lane];
        if (!k)
            for (int c = lane; c < d.SE; c += 64) X[e * ldx + c] = e_in[e * d.SE + c];
    }
    __syncthreads();
    if (!on || lane >= hk + SV) return;
    const bool isv = lane < hk;
    const float* wrow = isv ? wd + (int64_t)lane * vin : wdf + (int64_t)(lane - hk) * vin;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int c = 0; c < vin; ++c) {
        const float wv = wrow[c];
        a0 += wv * vp[w][0][c]; a1 += wv * vp[w][1][c]; a2 += wv * vp[w][2][c];
    }
    if (isv) {
        float* o = vh_out + e * 3 * hk;
        o[lane] = a0; o[hk + lane] = a1; o[2 * hk + lane] = a2;
        X[e * ldx + off + lane] = sqrtf(a0 * a0 + a1 * a1 + a2 * a2 + 1e-8f) + 1e-8f;
    } else {
        const int c = lane - hk;
        const float* f = fr[w];
#pragma unroll
        for (int r = 0; r < 3; ++r) X[e * ldx + off + hk + 3 * c + r] = f[3 * r] * a0 + f[3 * r + 1] * a1 + f[3 * r + 2] * a2;
    }
}

// ---- forward: S_pre (+ the node halves and bias for k = 0), silu, residual state update ------------------------------------------------------
__global__ void k_mp_act(int k, Dims d, float* __restrict__ spre, const float* __restrict__ aij, const float* __restrict__ b0, const int64_t* __restrict__ row,
                         const int64_t* __restrict__ col, float* __restrict__ g, const float* __restrict__ s_in, int ld_in, float* __restrict__ s_out, int ld_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.E * S) return;
    const int64_t e = i / S;
    const int c = (int)(i - e * S);
    float v = spre[i];
    if (!k) v = v + aij[row[e] * 2 * S + c] + aij[col[e] * 2 * S + S + c] + b0[c];
    spre[i] = v;
    const float a = act_f(ACT_SILU, v);
    g[i] = a;
    s_out[e * ld_out + c] = (k ? s_in[e * ld_in + c] : 0.f) + a;
}

// ---- forward: vector_up, sigmoid gate, residual vector update (one thread per edge and output channel) --------------------------------------
__global__ void k_mp_vout(int k, Dims d, const float* __restrict__ vh, const float* __restrict__ wup, const float* __restrict__ gate,
                          const float* __restrict__ v_in, float* __restrict__ v_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.E * V) return;
    const int64_t e = i / V;
    const int c = (int)(i - e * V), hk = k ? H : d.H0;
    const float* p = vh + e * 3 * hk;
    float u0 = 0.f, u1 = 0.f, u2 = 0.f;
    for (int h = 0; h < hk; ++h) {
        const float w = wup[c * hk + h];
        u0 += w * p[h]; u1 += w * p[hk + h]; u2 += w * p[2 * hk + h];
    }
    const float sg = sigm_f(gate[i]);
    const int64_t o = e * 3 * V + c;
    v_out[o] = (k ? v_in[o] : 0.f) + u0 * sg;
    v_out[o + V] = (k ? v_in[o + V] : 0.f) + u1 * sg;
    v_out[o + 2 * V] = (k ? v_in[o + 2 * V] : 0.f) + u2 * sg;
}

// deterministic sum over a 64-lane wave (fixed butterfly)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// ---- forward: scalar attention sigmoid(s . w_a + b_a), one wave per edge ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mp_att(Dims d, const float* __restrict__ s, const float* __restrict__ wa, const float* __restrict__ ba, float* __restrict__ att) {
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (e >= d.E) return;
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < S / 64; ++j) a += s[e * S + lane + 64 * j] * wa[lane + 64 * j];
    a = wave_sum(a);
    if (lane == 0) att[e] = sigm_f(a + ba[0]);
}

// ---- forward: agg[n] = sum over the node's edges, in edge order (index_add_ order), of [s * att | v (rep layout)] -----------------------------
__global__ void k_mp_agg(Dims d, const int32_t* __restrict__ rowptr, const float* __restrict__ s, const float* __restrict__ att, const float* __restrict__ v,
                         float* __restrict__ agg) {
    constexpr int W = S + 3 * V;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.N * W) return;
    const int64_t n = i / W;
    const int c = (int)(i - n * W);
    const int b = rowptr[n], en = rowptr[n + 1];
    float acc = 0.f;
    if (c < S) {
        for (int e = b; e < en; ++e) acc += s[(int64_t)e * S + c] * att[e];
    } else {
        const int ch = (c - S) / 3, x = (c - S) % 3;
        for (int e = b; e < en; ++e) acc += v[(int64_t)e * 3 * V + x * V + ch];
    }
    agg[i] = acc;
}

// ---- backward: attention and the incoming aggregate gradient, one wave per edge --------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mp_att_bwd(Dims d, const float* __restrict__ dagg, const int64_t* __restrict__ row, const float* __restrict__ s,
                                                    const float* __restrict__ att, const float* __restrict__ wa, float* __restrict__ ds, float* __restrict__ dv,
                                                    float* __restrict__ dlog, float* __restrict__ one) {
    constexpr int W = S + 3 * V;
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) *one = 1.f;
    if (e >= d.E) return;
    const float* g = dagg + row[e] * W;
    const float a = att[e];
    float da = 0.f, gv[S / 64];
#pragma unroll
    for (int j = 0; j < S / 64; ++j) { gv[j] = g[lane + 64 * j]; da += gv[j] * s[e * S + lane + 64 * j]; }
    da = wave_sum(da);
    const float dl = da * a * (1.f - a);
#pragma unroll
    for (int j = 0; j < S / 64; ++j) ds[e * S + lane + 64 * j] = gv[j] * a + dl * wa[lane + 64 * j];
    for (int j = lane; j < 3 * V; j += 64) {           // rep (ch, x) -> pre (x, ch)
        const int ch = j / 3, x = j % 3;
        dv[e * 3 * V + x * V + ch] = g[S + j];
    }
    if (lane == 0) dlog[e] = dl;
}

// ---- backward: gate and vector_up of GCP k (one thread per edge and output channel); d nv = dv (the gradient of the next vector state) -----
__global__ void k_mp_vout_bwd(int k, Dims d, const float* __restrict__ vh, const float* __restrict__ wup, const float* __restrict__ gate,
                              const float* __restrict__ dv, float* __restrict__ dup, float* __restrict__ dgate) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.E * V) return;
    const int64_t e = i / V;
    const int c = (int)(i - e * V), hk = k ? H : d.H0;
    const float* p = vh + e * 3 * hk;
    float u0 = 0.f, u1 = 0.f, u2 = 0.f;
    for (int h = 0; h < hk; ++h) {
        const float w = wup[c * hk + h];
        u0 += w * p[h]; u1 += w * p[hk + h]; u2 += w * p[2 * hk + h];
    }
    const float sg = sigm_f(gate[i]);
    const int64_t o = e * 3 * V + c;
    const float g0 = dv[o], g1 = dv[o + V], g2 = dv[o + 2 * V];
    dup[o] = g0 * sg; dup[o + V] = g1 * sg; dup[o + 2 * V] = g2 * sg;
    dgate[i] = (g0 * u0 + g1 * u1 + g2 * u2) * sg * (1.f - sg);
}

// ---- backward: silu of GCP k: dS_pre = (d ns + d gate_in) * silu'(S_pre); silu(S_pre) recomputed for dW_gate ---------------------------------
__global__ void k_mp_act_bwd(Dims d, const float* __restrict__ spre, const float* __restrict__ ds, const float* __restrict__ dgin, float* __restrict__ dspre,
                             float* __restrict__ g) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.E * S) return;
    const float x = spre[i];
    g[i] = act_f(ACT_SILU, x);
    dspre[i] = (ds[i] + dgin[i]) * act_df(ACT_SILU, x);
}

// ---- backward: norms, frame scalars and down projections of GCP k (one wave per edge, 4 per workgroup) -------------------------------------
// in: dX (gradient of X), dup, the tape's v_pre and vh.  out: dvh, du (for the weight gradients); k > 0: ds += dX[:, :S], dv += d v_pre;
// k = 0: de, dxi, and the per-edge pieces of the node gradient dvrow / dvcol ([E][3][V]).
__global__ __launch_bounds__(256) void k_mp_down_bwd(int k, Dims d, const float* __restrict__ dX, const float* __restrict__ dup, const float* __restrict__ vh,
                                                     const float* __restrict__ wup, const float* __restrict__ wd, const float* __restrict__ wdf,
                                                     const float* __restrict__ F, const uint8_t* __restrict__ emask, float* __restrict__ dvh_out,
                                                     float* __restrict__ du_out, float* __restrict__ ds, float* __restrict__ dv, float* __restrict__ de,
                                                     float* __restrict__ dxi, float* __restrict__ dvrow, float* __restrict__ dvcol) {
    __shared__ float gv[4][3][24];         // dvh (hk <= 20) then du (3)
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 4 + w;
    const bool on = e < d.E;
    const int vin = k ? V : d.VIN0, hk = k ? H : d.H0, ldx = k ? KX : d.K0, off = k ? S : d.SE;
    if (on && lane < hk + SV) {
        const float* gx = dX + e * ldx + off;
        float g0, g1, g2;
        if (lane < hk) {
            const float* p = vh + e * 3 * hk;
            const float a0 = p[lane], a1 = p[hk + lane], a2 = p[2 * hk + lane];
            const float t = gx[lane] / sqrtf(a0 * a0 + a1 * a1 + a2 * a2 + 1e-8f);
            g0 = t * a0; g1 = t * a1; g2 = t * a2;
            const float* q = dup + e * 3 * V;
            for (int c = 0; c < V; ++c) {
                const float wv = wup[c * hk + lane];
                g0 += q[c] * wv; g1 += q[V + c] * wv; g2 += q[2 * V + c] * wv;
            }
            float* o = dvh_out + e * 3 * hk;
            o[lane] = g0; o[hk + lane] = g1; o[2 * hk + lane] = g2;
        } else {
            const int c = lane - hk;
            float f[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) f[j] = (emask && !emask[e]) ? 0.f : F[e * 9 + j];
            const float q0 = gx[hk + 3 * c], q1 = gx[hk + 3 * c + 1], q2 = gx[hk + 3 * c + 2];
            g0 = f[0] * q0 + f[3] * q1 + f[6] * q2;
            g1 = f[1] * q0 + f[4] * q1 + f[7] * q2;
            g2 = f[2] * q0 + f[5] * q1 + f[8] * q2;
            float* o = du_out + e * 3 * SV;
            o[c] = g0; o[SV + c] = g1; o[2 * SV + c] = g2;
        }
        gv[w][0][lane] = g0; gv[w][1][lane] = g1; gv[w][2][lane] = g2;
    }
    __syncthreads();
    if (!on) return;
    for (int j = lane; j < vin; j += 64) {
        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
        for (int h = 0; h < hk; ++h) {
            const float wv = wd[(int64_t)h * vin + j];
            r0 += gv[w][0][h] * wv; r1 += gv[w][1][h] * wv; r2 += gv[w][2][h] * wv;
        }
        for (int c = 0; c < SV; ++c) {
            const float wv = wdf[(int64_t)c * vin + j];
            r0 += gv[w][0][hk + c] * wv; r1 += gv[w][1][hk + c] * wv; r2 += gv[w][2][hk + c] * wv;
        }
        if (k) {
            float* o = dv + e * 3 * V + j;
            o[0] += r0; o[V] += r1; o[2 * V] += r2;
        } else if (j < V) {
            float* o = dvrow + e * 3 * V + j;
            o[0] = r0; o[V] = r1; o[2 * V] = r2;
        } else if (j < V + d.VE) {
            float* o = dxi + (e * d.VE + (j - V)) * 3;
            o[0] = r0; o[1] = r1; o[2] = r2;
        } else {
            float* o = dvcol + e * 3 * V + (j - V - d.VE);
            o[0] = r0; o[V] = r1; o[2 * V] = r2;
        }
    }
    if (k) {
        for (int c = lane; c < S; c += 64) ds[e * S + c] += dX[e * ldx + c];
    } else {
        for (int c = lane; c < d.SE; c += 64) de[e * d.SE + c] = dX[e * ldx + c];
    }
}

// ---- backward: node sums in fixed order: RSCS[n] = [sum_{row = n} dS0 | sum_{col = n} dS0], dV_node (rep) = sum_row dvrow + sum_col dvcol -----
__global__ void k_mp_node_sum(Dims d, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colptr, const int64_t* __restrict__ colperm,
                              const float* __restrict__ ds0, const float* __restrict__ dvrow, const float* __restrict__ dvcol, float* __restrict__ rscs,
                              float* __restrict__ dvnode) {
    constexpr int W = S + 3 * V;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.N * W) return;
    const int64_t n = i / W;
    const int c = (int)(i - n * W);
    const int rb = rowptr[n], re = rowptr[n + 1], cb = colptr[n], ce = colptr[n + 1];
    if (c < S) {
        float a = 0.f, b = 0.f;
        for (int e = rb; e < re; ++e) a += ds0[(int64_t)e * S + c];
        for (int p = cb; p < ce; ++p) b += ds0[colperm[p] * S + c];
        rscs[n * 2 * S + c] = a;
        rscs[n * 2 * S + S + c] = b;
    } else {
        const int j = c - S, x = j / V, ch = j % V;          // pre (x, ch) -> rep (ch, x)
        float a = 0.f, b = 0.f;
        for (int e = rb; e < re; ++e) a += dvrow[(int64_t)e * 3 * V + j];
        for (int p = cb; p < ce; ++p) b += dvcol[colperm[p] * 3 * V + j];
        dvnode[n * 3 * V + ch * 3 + x] = a + b;
    }
}

// ---- backward: every weight gradient of the layer (one grouped split-K launch, one fixed-order slice reduction), from the tape `t` (layout F)
// and the backward's scratch `ws` (layout L: dspre, gk, dgate, dup, dvh, du, dlog, rscs filled) -- shared by gcdm_mp_bwd and gcdm_mp_tile_bwd ---------
static inline void wgrad_all(const Dims& d, const FwdLayout& F, const BwdLayout& L, const float* t, float* ws, const float* h, float* dweights,
                             hipStream_t st, int mode) {
    const int64_t N = d.N, E = d.E;
    int64_t sz[NW], off[NW];
    weight_sizes(d, sz);
    WgTable T;
    T.total = wgrad_offsets(sz, NW, off);
    const float* one = ws + L.one;
    for (int k = 0; k < 4; ++k) {
        const int hk = k ? H : d.H0, vin = k ? V : d.VIN0;
        const float* vpre = k ? t + F.vst[k] : t + F.vpre0;
        const float* dsp = ws + L.dspre[k];
        const int64_t ow = off[7 * k + 2];
        T.add(ws + L.dvh[k], 1, hk, vpre, vin, 1, hk, vin, 3 * E, off[7 * k + 0], vin);                     // dW_down = sum_(e,x) dvh^T v_pre
        T.add(ws + L.du[k], 1, SV, vpre, vin, 1, SV, vin, 3 * E, off[7 * k + 1], vin);                       // dW_down_frames
        if (k) {
            T.add(dsp, 1, S, t + F.x[k], KX, 1, S, KX, E, ow, KX);                                           // dW_s = dS_pre^T X
        } else {
            const float* rscs = ws + L.rscs;
            const float* x0 = t + F.x0;
            T.add(rscs, 1, 2 * S, h, S, 1, S, S, N, ow, d.KIN0);                                              // W_i: (row sums)^T h
            T.add(dsp, 1, S, x0, d.K0, 1, S, d.SE, E, ow + S, d.KIN0);                                         // W_e
            T.add(rscs + S, 1, 2 * S, h, S, 1, S, S, N, ow + S + d.SE, d.KIN0);                                 // W_j: (column sums)^T h
            T.add(dsp, 1, S, x0 + d.SE, d.K0, 1, S, d.H0 + 3 * SV, E, ow + 2 * S + d.SE, d.KIN0);               // [|vh| | q] columns
        }
        T.add(dsp, 1, S, one, 0, 0, S, 1, E, off[7 * k + 3], 1);                                             // b_s
        T.add(ws + L.dup[k], 1, V, t + F.vh[k], hk, 1, V, hk, 3 * E, off[7 * k + 4], hk);                    // dW_up = sum dup^T vh
        T.add(ws + L.dgate[k], 1, V, ws + L.gk[k], S, 1, V, S, E, off[7 * k + 5], S);                        // dW_gate = dgate^T silu(S_pre)
        T.add(ws + L.dgate[k], 1, V, one, 0, 0, V, 1, E, off[7 * k + 6], 1);                                // b_gate
    }
    T.add(ws + L.dlog, 0, 1, t + fwd_sfin(F), S, 1, 1, S, E, off[28], S);                                     // attention weight
    T.add(ws + L.dlog, 0, 1, one, 0, 0, 1, 1, E, off[29], 1);                                                 // attention bias
    wgrad_launch(T, ws + L.part, dweights, st, mode);
}

}  // namespace gmp

// ------------------------------------------------------------------------------------------------------------------------------------------
// C ABI (include/gcdm_mp_train.h)
// ------------------------------------------------------------------------------------------------------------------------------------------
static inline bool gmp_dims_ok(int64_t N, int64_t E, int32_t SE, int32_t VE) {
    return N >= 0 && E >= 0 && ((SE == 64 && VE == 16) || (SE == 16 && VE == 8)) && (N > 0 || E == 0);
}
static inline bool gmp_weights_ok(const float* const* w) {
    if (!w) return false;
    for (int i = 0; i < gmp::NW; ++i)
        if (!w[i]) return false;
    return true;
}
extern "C" {

int64_t gcdm_mp_workspace_bytes(int32_t which, int64_t N, int64_t E, int32_t SE, int32_t VE) {
    GOPS_REQUIRE(which >= 0 && which <= 3 && gmp_dims_ok(N, E, SE, VE));
    const gmp::Dims d = gmp::make_dims(N, E, SE, VE);
    if (which <= 1) return 4 * gmp::fwd_floats(d, which);
    if (which == 2) return 4 * gmp::bwd_layout(d).total;
    return 4 * gmp::weight_total(d);
}

int gcdm_mp_fwd(const float* h, const float* vnode, const float* e, const float* xi, const int64_t* row, const int64_t* col, const int32_t* rowptr,
                const float* frames, const uint8_t* edge_mask, const float* const* weights, float* agg, float* workspace, int32_t tape, int64_t N,
                int64_t E, int32_t SE, int32_t VE, void* stream) {
    using namespace gmp;
    GOPS_REQUIRE(gmp_dims_ok(N, E, SE, VE) && gops_flag(tape));
    if (N == 0 || E == 0) return 0;
    GOPS_REQUIRE(h && vnode && e && xi && row && col && rowptr && frames && agg && workspace && gmp_weights_ok(weights));
    const float* const* W = weights;
    const hipStream_t st = (hipStream_t)stream;
    const Dims d = make_dims(N, E, SE, VE);
    const int mode = gops_matrix_mode();         // read once: every GEMM launch of this call runs in it
    auto gemm = [&](auto... a) { gops::gemm(a..., 1, mode); };
    const FwdLayout L = fwd_layout(d, tape);
    float* ws = workspace;
    float* sfin = ws + fwd_sfin(L);
    float* vfin = ws + fwd_vfin(d, L);
    const int64_t npack = (int64_t)2 * S * S + (int64_t)S * d.K0;
    hipLaunchKernelGGL(k_mp_pack, dim3(gops_blocks(npack)), dim3(256), 0, st, W[2], ws + L.wij, ws + L.wr0, d);
    gemm(h, S, 1, ws + L.wij, 1, S, ws + L.aij, nullptr, N, 2 * S, S, st);                  // [A_i | A_j] = h [W_i ; W_j]^T
    const unsigned eb = (unsigned)((E + 3) / 4);
    for (int k = 0; k < 4; ++k) {
        const float* const* Wk = W + 7 * k;
        float* X = ws + (k ? L.x[k] : L.x0);
        const float* vin = k ? ws + L.vst[k] : nullptr;
        float* vout = k < 3 ? ws + L.vst[k + 1] : vfin;
        float* spre = ws + L.spre[k];
        float* gate = ws + L.gate[k];
        hipLaunchKernelGGL(k_mp_down, dim3(eb), dim3(256), 0, st, k, d, vnode, xi, e, row, col, frames, edge_mask, vin, Wk[0], Wk[1],
                           (k == 0 && tape) ? ws + L.vpre0 : nullptr, ws + L.vh[k], X);
        if (k == 0) gemm(X, d.K0, 1, ws + L.wr0, 1, d.K0, spre, nullptr, E, S, d.K0, st);
        else gemm(X, KX, 1, Wk[2], 1, KX, spre, Wk[3], E, S, KX, st);
        float* s_out = k < 3 ? ws + L.x[k + 1] : sfin;
        hipLaunchKernelGGL(k_mp_act, dim3(gops_blocks(E * S)), dim3(256), 0, st, k, d, spre, ws + L.aij, W[3], row, col, ws + L.g, X, (int)KX, s_out,
                           k < 3 ? (int)KX : (int)S);
        gemm(ws + L.g, S, 1, Wk[5], 1, S, gate, Wk[6], E, V, S, st);
        hipLaunchKernelGGL(k_mp_vout, dim3(gops_blocks(E * V)), dim3(256), 0, st, k, d, ws + L.vh[k], Wk[4], gate, vin, vout);
    }
    hipLaunchKernelGGL(k_mp_att, dim3(eb), dim3(256), 0, st, d, sfin, W[28], W[29], ws + L.att);
    hipLaunchKernelGGL(k_mp_agg, dim3(gops_blocks(N * (S + 3 * V))), dim3(256), 0, st, d, rowptr, sfin, ws + L.att, vfin, agg);
    return GOPS_LAUNCH_OK();
}

int gcdm_mp_bwd(const float* dagg, const float* h, const int64_t* row, const int64_t* col, const int32_t* rowptr, const int32_t* colptr,
                const int64_t* colperm, const float* frames, const uint8_t* edge_mask, const float* const* weights, const float* tape, float* workspace,
                float* dh, float* dvnode, float* de, float* dxi, float* dweights, int64_t N, int64_t E, int32_t SE, int32_t VE, void* stream) {
    using namespace gmp;
    GOPS_REQUIRE(gmp_dims_ok(N, E, SE, VE));
    if (N == 0 || E == 0) return 0;
    GOPS_REQUIRE(dagg && h && row && col && rowptr && colptr && colperm && frames && tape && workspace && dh && dvnode && de && dxi && dweights &&
                 gmp_weights_ok(weights));
    (void)col;
    const float* const* W = weights;
    const hipStream_t st = (hipStream_t)stream;
    const Dims d = make_dims(N, E, SE, VE);
    const int mode = gops_matrix_mode();         // read once: every GEMM launch of this call runs in it
    auto gemm = [&](auto... a) { gops::gemm(a..., 1, mode); };
    const FwdLayout F = fwd_layout(d, 1);
    const BwdLayout L = bwd_layout(d);
    const float* t = tape;
    float* ws = workspace;
    const unsigned eb = (unsigned)((E + 3) / 4);
    hipLaunchKernelGGL(k_mp_att_bwd, dim3(eb), dim3(256), 0, st, d, dagg, row, t + fwd_sfin(F), t + F.att, W[28], ws + L.ds, ws + L.dv, ws + L.dlog,
                       ws + L.one);
    for (int k = 3; k >= 0; --k) {
        const float* const* Wk = W + 7 * k;
        hipLaunchKernelGGL(k_mp_vout_bwd, dim3(gops_blocks(E * V)), dim3(256), 0, st, k, d, t + F.vh[k], Wk[4], t + F.gate[k], ws + L.dv, ws + L.dup[k],
                           ws + L.dgate[k]);
        gemm(ws + L.dgate[k], V, 1, Wk[5], S, 1, ws + L.dg, nullptr, E, S, V, st);                 // d gate_in = d gate . W_g
        hipLaunchKernelGGL(k_mp_act_bwd, dim3(gops_blocks(E * S)), dim3(256), 0, st, d, t + F.spre[k], ws + L.ds, ws + L.dg, ws + L.dspre[k], ws + L.gk[k]);
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
