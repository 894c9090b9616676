// gcdm_ops.egnn_dynamics.hip.h -- the layers of the EGNN dynamics network (src/models/components/egnn.py EGNN_Sparse / EGNNDynamics of the
// reference), forward only, on gfx950.  C ABI: include/gcdm_egnn_dynamics.h.  DESIGN.md 3.10.
//
// One layer is 8 launches: two node-level GEMMs (A = h W_i^T + b1 + W_e b_emb, B = h W_j^T, [N, Kp] with Kp = 2 D rounded up to 16 and zero
// columns behind 2 D), the edge kernel, the node kernel, node_mlp.0, SiLU, node_mlp.3, the residual.  The GEMMs are gops::gemm in exact fp32.
//
// Edge kernel.  The edges are never materialised: the fully connected edge list sorted by receiver is "node i, slot s -> sender
// node_offsets[mol(i)] + s", so a workgroup (256 threads, 4 waves) that owns RB = 32 consecutive receivers walks their slots as one flat
// list in rounds of 256 edges, a wave taking 64 of them as four 16-edge MFMA tiles that share the weight operand:
//   * lane (e, q) = (lane & 15, lane >> 4) forms, per 16-wide k-block, the four pre-activations k = 4 q .. 4 q + 3 of its edges from one
//     16-byte read of A_i, one of B_j and the three per-layer vectors u, u', w_r, applies SiLU and issues v_mfma_f32_16x16x4_f32 four times;
//     MFMA step s of a block contracts k = {s, 4 + s, 8 + s, 12 + s}: a fixed order, the same for every edge; the weights are packed in it;
//   * the 16 outputs of an edge take bias and SiLU in the accumulators and go to an LDS stage ([256][21], odd stride), where one lane per
//     edge runs coors_mlp (16 -> 64 -> 1, tanh) as an fmaf chain and adds w_ij (x_j - x_i) / max(|x_j - x_i|, 1e-8) * scale to its row;
//   * one thread per (receiver, column) adds the staged rows of its receiver to a running sum in slot order: m_i = ((0 + m_i0) + m_i1) + ...
//     across rounds, whatever the tile boundaries and whatever else is in the batch.  No atomics.
// Node kernel: one workgroup per molecule, graph-mode LayerNorm in two passes (strided partial sums, a fixed LDS tree) and x + dx.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdarg.h>
#include <stdio.h>
#include <math.h>
#include <atomic>

namespace gegd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MAX_H = 256;          // GCDM_EGNN_DYN_MAX_H
constexpr int MAX_EH = 1024;        // GCDM_EGNN_DYN_MAX_EH
constexpr int MD = 16;              // GCDM_EGNN_DYN_M_DIM
constexpr int CH = 64;              // GCDM_EGNN_DYN_COORS_HIDDEN
constexpr int LAYER_TENSORS = 15;   // GCDM_EGNN_DYN_LAYER_TENSORS
constexpr int HEAD_TENSORS = 2;
constexpr int LAUNCHES = 8;         // GCDM_EGNN_DYN_LAUNCHES_PER_LAYER
constexpr int THREADS = 256;
constexpr int RB = 32;              // receivers per workgroup
constexpr int ROUND = 256;          // edges per round: 4 waves x 64
constexpr int NC = MD + 3;          // summed columns per receiver: m | dx
constexpr int SS = 21;              // stage row stride, odd
constexpr int64_t MAX_NODES = 1LL << 24;

__host__ __device__ inline int kpad(int H, int Eh) { return (2 * (2 * H + Eh + 1) + 15) / 16 * 16; }

// offsets (floats) inside one layer's packed block; every block a multiple of 16 floats
struct LayerOff { int64_t wi, wj, b1c, u, u2, wr, w2p, b2, c1t, c1b, c2, misc, lnw, lnb, n1t, n1b, n2t, n2b, total; };
__host__ __device__ inline LayerOff layer_off(int H, int Eh) {
    LayerOff o;
    const int64_t Kp = kpad(H, Eh);
    int64_t p = 0;
    o.wi = p; p += (int64_t)H * Kp; o.wj = p; p += (int64_t)H * Kp;
    o.b1c = p; p += Kp; o.u = p; p += Kp; o.u2 = p; p += Kp; o.wr = p; p += Kp;
    o.w2p = p; p += Kp * MD; o.b2 = p; p += MD;
    o.c1t = p; p += MD * CH; o.c1b = p; p += CH; o.c2 = p; p += CH; o.misc = p; p += 16;      // misc[0] = coors_mlp.3.bias, misc[1] = coors_norm.scale
    o.lnw = p; p += H; o.lnb = p; p += H;
    o.n1t = p; p += (int64_t)(H + MD) * 2 * H; o.n1b = p; p += 2 * H; o.n2t = p; p += (int64_t)2 * H * H; o.n2b = p; p += H;
    o.total = p;
    return o;
}

struct WsOff { int64_t A, B, cat, mid, mid2, y, dx, total; };
__host__ inline WsOff ws_off(int64_t N, int H, int Eh) {
    WsOff w;
    const int64_t Kp = kpad(H, Eh);
    auto up = [](int64_t n) { return (n + 63) / 64 * 64; };
    int64_t p = 0;
    w.A = p; p += up(N * Kp); w.B = p; p += up(N * Kp); w.cat = p; p += up(N * (H + MD)); w.mid = p; p += up(N * 2 * H);
    w.mid2 = p; p += up(N * 2 * H); w.y = p; p += up(N * H); w.dx = p; p += up(N * 3);
    w.total = p;
    return w;
}

__device__ __forceinline__ float silu(float v) { return v / (1.f + expf(-v)); }

// ---- packing ---------------------------------------------------------------------------------------------------------------------------------
// dst[k * n_out + n] = src[n * ld + col0 + k] for k < K and n < n_real, else 0
__global__ void k_pack_t(const float* __restrict__ src, float* __restrict__ dst, int n_real, int n_out, int ld, int col0, int K, int Kpad) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)Kpad * n_out) return;
    const int k = (int)(idx / n_out), n = (int)(idx % n_out);
    dst[idx] = (k < K && n < n_real) ? src[(int64_t)n * ld + col0 + k] : 0.f;
}

// the folded edge embedding: b1c = b1 + W_e b_emb, u = W_e w_emb[:, 0], u2 = W_e w_emb[:, 1] (0 with e_in = 1), wr = W1[:, D - 1]; zero behind 2 D
__global__ void k_fold(const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ we, const float* __restrict__ be,
                       float* __restrict__ b1c, float* __restrict__ u, float* __restrict__ u2, float* __restrict__ wr, int H, int Eh, int e_in, int Kp) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Kp) return;
    const int D = 2 * H + Eh + 1;
    float c = 0.f, a = 0.f, b = 0.f, r = 0.f;
    if (k < 2 * D) {
        const float* row = W1 + (int64_t)k * D + 2 * H;
        for (int e = 0; e < Eh; ++e) {
            c = fmaf(row[e], be[e], c);
            a = fmaf(row[e], we[e * e_in], a);
            if (e_in == 2) b = fmaf(row[e], we[e * 2 + 1], b);
        }
        c = b1[k] + c;
        r = row[Eh];
    }
    b1c[k] = c; u[k] = a; u2[k] = b; wr[k] = r;
}

// edge_mlp.3.weight [16, 2 D] in the order the MFMA steps read it: w2p[(block * 64 + lane) * 4 + s] = W2[lane & 15][16 block + 4 (lane >> 4) + s]
__global__ void k_pack_w2(const float* __restrict__ W2, float* __restrict__ w2p, int K2, int Kp) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= Kp * MD) return;
    const int s = idx & 3, lane = (idx >> 2) & 63, blk = idx >> 8;
    const int k = blk * 16 + 4 * (lane >> 4) + s;
    w2p[idx] = k < K2 ? W2[(int64_t)(lane & 15) * K2 + k] : 0.f;
}

// ---- the edge kernel ---------------------------------------------------------------------------------------------------------------------------
// largest r in [0, RB) with lp[r] <= q (q < lp[RB]): the receiver of local edge q; receivers without edges are skipped
__device__ __forceinline__ int locate(const int* lp, int q) {
    int lo = 0, hi = RB;                       // invariant: lp[lo] <= q < lp[hi]
#pragma unroll
    for (int it = 0; it < 5; ++it) {
        const int mid = (lo + hi) >> 1;
        if (lp[mid] <= q) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(THREADS) void k_edge(const float* __restrict__ A, const float* __restrict__ Bm, const float* __restrict__ x,
                                                  const float* __restrict__ x0, const float* __restrict__ xsc, const int32_t* __restrict__ noff,
                                                  const int32_t* __restrict__ nmol, const float* __restrict__ Wl, LayerOff o, float* __restrict__ cat,
                                                  int ldcat, int col0, float* __restrict__ dxout, int64_t N, int B, int Kp) {
    __shared__ float stage[ROUND * SS];
    __shared__ float acc[RB * NC];
    __shared__ int lp[RB + 1];
    __shared__ int mo[RB];
    __shared__ int cnt[RB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * RB;
    const int nr = N - i0 < RB ? (int)(N - i0) : RB;
    if (tid < RB) {
        int start = 0, n = 0;
        if (tid < nr) {
            const int64_t i = i0 + tid;
            const int m = nmol[i];
            if (m >= 0 && m < B) {
                const int64_t a = noff[m], b = noff[m + 1];
                if (a >= 0 && b <= N && a <= i && i < b) { start = (int)a; n = (int)(b - a); }
            }
        }
        mo[tid] = start;
        cnt[tid] = n;
    }
    for (int idx = tid; idx < RB * NC; idx += THREADS) acc[idx] = 0.f;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int r = 0; r < RB; ++r) { lp[r] = s; s += cnt[r]; }
        lp[RB] = s;
    }
    __syncthreads();
    const int total = lp[RB];
    const float* u = Wl + o.u;
    const float* u2 = Wl + o.u2;
    const float* wr = Wl + o.wr;
    const float* w2p = Wl + o.w2p;
    const int e16 = lane & 15, kq = lane >> 4;
    const float b2v = Wl[o.b2 + e16];

    for (int q0 = 0; q0 < total; q0 += ROUND) {
        const int tile0 = q0 + wave * 64;
        // ---- phase 1: m_ij of the wave's 64 edges ------------------------------------------------------------------------------------------
        if (tile0 < total) {
            const float* pa[4];
            const float* pb[4];
            float r0[4], r0s[4], rad[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int q = tile0 + 16 * t + e16;
                int64_t i = i0, j = i0;                              // a slot past the end computes on node i0 and is never summed
                if (q < total) {
                    const int r = locate(lp, q);
                    i = i0 + r;
                    j = (int64_t)mo[r] + (q - lp[r]);
                }
                pa[t] = A + i * Kp + 4 * kq;
                pb[t] = Bm + j * Kp + 4 * kq;
                float dx = x[j * 3] - x[i * 3], dy = x[j * 3 + 1] - x[i * 3 + 1], dz = x[j * 3 + 2] - x[i * 3 + 2];
                rad[t] = dx * dx + dy * dy + dz * dz;
                dx = x0[j * 3] - x0[i * 3]; dy = x0[j * 3 + 1] - x0[i * 3 + 1]; dz = x0[j * 3 + 2] - x0[i * 3 + 2];
                r0[t] = dx * dx + dy * dy + dz * dz;
                r0s[t] = 0.f;
                if (xsc) {
                    dx = xsc[j * 3] - xsc[i * 3]; dy = xsc[j * 3 + 1] - xsc[i * 3 + 1]; dz = xsc[j * 3 + 2] - xsc[i * 3 + 2];
                    r0s[t] = dx * dx + dy * dy + dz * dz;
                }
            }
            f32x4 c[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) c[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int kc = 0; kc < Kp; kc += 16) {
                const float4 uu = *(const float4*)(u + kc + 4 * kq);
                const float4 us = *(const float4*)(u2 + kc + 4 * kq);
                const float4 ww = *(const float4*)(wr + kc + 4 * kq);
                const float4 w2 = *(const float4*)(w2p + ((int64_t)(kc >> 4) * 64 + lane) * 4);
                const float uv[4] = {uu.x, uu.y, uu.z, uu.w}, sv[4] = {us.x, us.y, us.z, us.w}, wv[4] = {ww.x, ww.y, ww.z, ww.w};
                const float w2v[4] = {w2.x, w2.y, w2.z, w2.w};
                float act[4][4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float4 a4 = *(const float4*)(pa[t] + kc);
                    const float4 b4 = *(const float4*)(pb[t] + kc);
                    const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        float p = av[s] + bv[s];
                        p = fmaf(r0[t], uv[s], p);
                        p = fmaf(r0s[t], sv[s], p);
                        p = fmaf(rad[t], wv[s], p);
                        act[t][s] = silu(p);
                    }
                }
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int t = 0; t < 4; ++t) c[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(act[t][s], w2v[s], c[t], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) stage[(wave * 64 + 16 * t + 4 * kq + r) * SS + e16] = silu(c[t][r] + b2v);
        }
        __syncthreads();
        // ---- phase 2: coors_mlp and the coordinate term, one lane per edge ---------------------------------------------------------------------
        {
            const int q = tile0 + lane;
            if (q < total) {
                const int r = locate(lp, q);
                const int64_t i = i0 + r, j = (int64_t)mo[r] + (q - lp[r]);
                float* row = stage + (wave * 64 + lane) * SS;
                float m[MD];
#pragma unroll
                for (int k = 0; k < MD; ++k) m[k] = row[k];
                const float* c1t = Wl + o.c1t;
                float w = Wl[o.misc];
                for (int h = 0; h < CH; ++h) {
                    float v = Wl[o.c1b + h];
#pragma unroll
                    for (int k = 0; k < MD; ++k) v = fmaf(m[k], c1t[k * CH + h], v);
                    w = fmaf(silu(v), Wl[o.c2 + h], w);
                }
                w = tanhf(w);
                const float scale = Wl[o.misc + 1];
                const float dx = x[j * 3] - x[i * 3], dy = x[j * 3 + 1] - x[i * 3 + 1], dz = x[j * 3 + 2] - x[i * 3 + 2];
                const float nrm = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-8f);
                row[MD] = w * (dx / nrm * scale);
                row[MD + 1] = w * (dy / nrm * scale);
                row[MD + 2] = w * (dz / nrm * scale);
            }
        }
        __syncthreads();
        // ---- phase 3: the receiver sums, in slot order, one owner per (receiver, column) ---------------------------------------------------------
        {
            const int qe = q0 + ROUND < total ? q0 + ROUND : total;
            const int rf = locate(lp, q0), rl = locate(lp, qe - 1);
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
    for (int idx = tid; idx < nr * MD; idx += THREADS) cat[(i0 + idx / MD) * ldcat + col0 + idx % MD] = acc[(idx / MD) * NC + idx % MD];
    for (int idx = tid; idx < nr * 3; idx += THREADS) dxout[(i0 + idx / 3) * 3 + idx % 3] = acc[(idx / 3) * NC + MD + idx % 3];
}

// ---- the node kernel: graph-mode LayerNorm of h into cat[:, :H], x_out = x + dx ------------------------------------------------------------------
__device__ __forceinline__ float block_sum(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const float out = red[0];
    __syncthreads();
    return out;
}

__global__ __launch_bounds__(THREADS) void k_node(const float* __restrict__ h, const float* __restrict__ x, const float* __restrict__ dx,
                                                  const int32_t* __restrict__ noff, const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                  float* __restrict__ cat, int ldcat, float* __restrict__ xout, int64_t N, int H) {
    __shared__ float red[THREADS];
    const int tid = threadIdx.x;
    const int64_t a = noff[blockIdx.x], b = noff[blockIdx.x + 1];
    if (a < 0 || b > N || b <= a) return;                       // (uniform over the workgroup)
    const int64_t cnt = (b - a) * H;
    const float* hg = h + a * H;
    float s = 0.f;
    for (int64_t idx = tid; idx < cnt; idx += THREADS) s += hg[idx];
    const float norm = (float)(b - a) * (float)H;
    const float mean = block_sum(s, red) / norm;
    float v = 0.f;
    for (int64_t idx = tid; idx < cnt; idx += THREADS) { const float d = hg[idx] - mean; v += d * d; }
    const float sd = sqrtf(block_sum(v, red) / norm + 1e-5f);
    for (int64_t idx = tid; idx < cnt; idx += THREADS) {
        const int col = (int)(idx % H);
        cat[(a + idx / H) * ldcat + col] = (hg[idx] - mean) / sd * lnw[col] + lnb[col];
    }
    for (int64_t idx = tid; idx < (b - a) * 3; idx += THREADS) xout[a * 3 + idx] = x[a * 3 + idx] + dx[a * 3 + idx];
}

__global__ void k_residual(const float* __restrict__ h, const float* __restrict__ y, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = h[i] + y[i];
}

__global__ void k_copy_cols(const float* __restrict__ src, int ld, int col0, float* __restrict__ dst, int64_t N, int Cn) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N * Cn) dst[i] = src[(i / Cn) * ld + col0 + i % Cn];
}

static thread_local char g_err[256] = "";
static std::atomic<int64_t> g_edge_launches{0};
__attribute__((format(printf, 2, 3))) static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

static int check_dims(int H, int Eh, int e_in, int L) {
    if (H < 32 || H > MAX_H || H % 32) return fail(-1, "h_hidden = %d: the limit is a multiple of 32 up to %d", H, MAX_H);
    if (Eh < 1 || Eh > MAX_EH) return fail(-1, "e_hidden = %d: the limit is 1 .. %d", Eh, MAX_EH);
    if (e_in != 1 && e_in != 2) return fail(-1, "e_in = %d: 1 or 2", e_in);
    if (L < 1) return fail(-1, "n_layers = %d: the limit is >= 1", L);
    return 0;
}

}  // namespace gegd

extern "C" {

const char* gcdm_egnn_dyn_last_error(void) { return gegd::g_err; }

int64_t gcdm_egnn_dyn_launches(void) { return gegd::g_edge_launches.load(std::memory_order_relaxed); }

int64_t gcdm_egnn_dyn_workspace_bytes(int32_t which, int64_t num_nodes, int32_t h_hidden, int32_t e_hidden, int32_t e_in, int32_t n_layers) {
    using namespace gegd;
    if (which < 0 || which > 5) return fail(-1, "which = %d: 0 .. 5", which);
    if (num_nodes < 0 || num_nodes > MAX_NODES) return fail(-1, "num_nodes = %lld: 0 .. %lld", (long long)num_nodes, (long long)MAX_NODES);
    if (check_dims(h_hidden, e_hidden, e_in, n_layers)) return -1;
    switch (which) {
        case 0: return ws_off(num_nodes, h_hidden, e_hidden).total * 4 + 256;
        case 1: return layer_off(h_hidden, e_hidden).total * 4 * n_layers;
        case 2: return LAUNCHES;
        case 3: return kpad(h_hidden, e_hidden);
        case 4: return (int64_t)(ROUND * SS + RB * NC + 3 * RB + 1) * 4;
        default: return RB;
    }
}

int gcdm_egnn_dyn_pack(const void* const* tensors, int32_t count, int32_t h_hidden, int32_t e_hidden, int32_t e_in, int32_t n_layers,
                       float* packed, void* stream) {
    using namespace gegd;
    const int H = h_hidden, Eh = e_hidden, L = n_layers;
    if (check_dims(H, Eh, e_in, L)) return -1;
    if (count != HEAD_TENSORS + LAYER_TENSORS * L) return fail(-1, "count = %d tensors: expected %d", count, HEAD_TENSORS + LAYER_TENSORS * L);
    if (!tensors || !packed) return fail(-1, "null tensor table or packed buffer");
    for (int i = 0; i < count; ++i)
        if (!tensors[i]) return fail(-1, "tensor %d is null", i);
    const LayerOff o = layer_off(H, Eh);
    const int D = 2 * H + Eh + 1, K2 = 2 * D, Kp = kpad(H, Eh);
    hipStream_t st = (hipStream_t)stream;
    auto T = [&](int i) { return (const float*)tensors[i]; };
    auto put = [&](const float* src, float* dst, int n_real, int n_out, int ld, int col0, int K, int Kpad) {
        const int64_t n = (int64_t)Kpad * n_out;
        hipLaunchKernelGGL(k_pack_t, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, dst, n_real, n_out, ld, col0, K, Kpad);
    };
    auto vec = [&](const float* src, float* dst, int n, int npad) { put(src, dst, 1, 1, 1, 0, n, npad); };
    for (int l = 0; l < L; ++l) {
        const int t = HEAD_TENSORS + LAYER_TENSORS * l;
        float* b = packed + o.total * l;
        put(T(t), b + o.wi, K2, Kp, D, 0, H, H);
        put(T(t), b + o.wj, K2, Kp, D, H, H, H);
        hipLaunchKernelGGL(k_fold, dim3((unsigned)((Kp + 255) / 256)), dim3(256), 0, st, T(t), T(t + 1), T(0), T(1), b + o.b1c, b + o.u, b + o.u2,
                           b + o.wr, H, Eh, e_in, Kp);
        hipLaunchKernelGGL(k_pack_w2, dim3((unsigned)((Kp * MD + 255) / 256)), dim3(256), 0, st, T(t + 2), b + o.w2p, K2, Kp);
        vec(T(t + 3), b + o.b2, MD, MD);
        vec(T(t + 4), b + o.lnw, H, H);
        vec(T(t + 5), b + o.lnb, H, H);
        vec(T(t + 6), b + o.misc + 1, 1, 1);
        put(T(t + 7), b + o.n1t, 2 * H, 2 * H, H + MD, 0, H + MD, H + MD);
        vec(T(t + 8), b + o.n1b, 2 * H, 2 * H);
        put(T(t + 9), b + o.n2t, H, H, 2 * H, 0, 2 * H, 2 * H);
        vec(T(t + 10), b + o.n2b, H, H);
        put(T(t + 11), b + o.c1t, CH, CH, MD, 0, MD, MD);
        vec(T(t + 12), b + o.c1b, CH, CH);
        vec(T(t + 13), b + o.c2, CH, CH);
        vec(T(t + 14), b + o.misc, 1, 1);
        vec(nullptr, b + o.misc + 2, 0, 14);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(-2, "egnn dynamics pack launch failed: %s", hipGetErrorString(e));
}

int gcdm_egnn_dyn_layer(int32_t layer, const float* h_in, const float* x_in, const float* x0, const float* xsc, const int32_t* node_offsets,
                        const int32_t* node_mol, const float* packed, void* workspace, float* h_out, float* x_out, float* dbg_m, float* dbg_dx,
                        float* dbg_ln, int64_t num_nodes, int64_t num_molecules, int32_t h_hidden, int32_t e_hidden, int32_t e_in,
                        int32_t n_layers, void* stream) {
    using namespace gegd;
    const int H = h_hidden, Eh = e_hidden;
    const int64_t N = num_nodes;
    if (check_dims(H, Eh, e_in, n_layers)) return -1;
    if (layer < 0 || layer >= n_layers) return fail(-1, "layer = %d: 0 .. n_layers - 1", layer);
    if (N < 0 || num_molecules < 0) return fail(-1, "negative size");
    if (N > MAX_NODES || num_molecules > N) return fail(-1, "%lld atoms in %lld molecules: at most %lld atoms and no more molecules than atoms",
                                                         (long long)N, (long long)num_molecules, (long long)MAX_NODES);
    if (N > 0 && num_molecules == 0) return fail(-1, "%lld atoms in no molecule", (long long)N);
    if ((e_in == 2) != (xsc != nullptr)) return fail(-1, "xsc goes with e_in = 2 and only with it");
    if (N == 0) return 0;
    if (!h_in || !x_in || !x0 || !node_offsets || !node_mol || !packed || !workspace || !h_out || !x_out) return fail(-1, "null pointer");
    if (h_out == h_in || x_out == x_in) return fail(-1, "h_out / x_out alias the inputs");
    hipStream_t st = (hipStream_t)stream;
    const int B = (int)num_molecules, Kp = kpad(H, Eh), ldcat = H + MD;
    const LayerOff o = layer_off(H, Eh);
    const WsOff w = ws_off(N, H, Eh);
    const float* Wl = packed + o.total * layer;
    float* ws = (float*)(((uintptr_t)workspace + 255) / 256 * 256);
    gops::gemm(h_in, H, 1, Wl + o.wi, Kp, 1, ws + w.A, Wl + o.b1c, N, Kp, H, st, 1, gops::MM_F32);
    gops::gemm(h_in, H, 1, Wl + o.wj, Kp, 1, ws + w.B, nullptr, N, Kp, H, st, 1, gops::MM_F32);
    hipLaunchKernelGGL(k_edge, dim3((unsigned)((N + RB - 1) / RB)), dim3(THREADS), 0, st, (const float*)(ws + w.A), (const float*)(ws + w.B), x_in, x0,
                       xsc, node_offsets, node_mol, Wl, o, ws + w.cat, ldcat, H, ws + w.dx, N, B, Kp);
    hipLaunchKernelGGL(k_node, dim3((unsigned)B), dim3(THREADS), 0, st, h_in, x_in, (const float*)(ws + w.dx), node_offsets, Wl + o.lnw, Wl + o.lnb,
                       ws + w.cat, ldcat, x_out, N, H);
    gops::gemm(ws + w.cat, ldcat, 1, Wl + o.n1t, 2 * H, 1, ws + w.mid, Wl + o.n1b, N, 2 * H, ldcat, st, 1, gops::MM_F32);
    hipLaunchKernelGGL(gops::k_act, dim3(gops_blocks(N * 2 * H)), dim3(256), 0, st, 1, (const float*)(ws + w.mid), ws + w.mid2, N * 2 * H);
    gops::gemm(ws + w.mid2, 2 * H, 1, Wl + o.n2t, H, 1, ws + w.y, Wl + o.n2b, N, H, 2 * H, st, 1, gops::MM_F32);
    hipLaunchKernelGGL(k_residual, dim3(gops_blocks(N * H)), dim3(256), 0, st, h_in, (const float*)(ws + w.y), h_out, N * H);
    if (dbg_m) hipLaunchKernelGGL(k_copy_cols, dim3(gops_blocks(N * MD)), dim3(256), 0, st, (const float*)(ws + w.cat), ldcat, H, dbg_m, N, MD);
    if (dbg_dx) hipLaunchKernelGGL(k_copy_cols, dim3(gops_blocks(N * 3)), dim3(256), 0, st, (const float*)(ws + w.dx), 3, 0, dbg_dx, N, 3);
    if (dbg_ln) hipLaunchKernelGGL(k_copy_cols, dim3(gops_blocks(N * H)), dim3(256), 0, st, (const float*)(ws + w.cat), ldcat, 0, dbg_ln, N, H);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-2, "egnn dynamics layer launch failed: %s", hipGetErrorString(e));
    g_edge_launches.fetch_add(1, std::memory_order_relaxed);
    return 0;
}

}  // extern "C"
