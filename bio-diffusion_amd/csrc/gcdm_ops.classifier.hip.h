// gcdm_ops.classifier.hip.h -- the EGNN property classifier (src/__init__.py EGNN / E_GCL_mask of the reference), forward only, evaluation
// mode, as ONE launch per forward on gfx950.  C ABI: include/gcdm_classifier.h.  DESIGN.md 3.9.
//
// A workgroup (256 threads, 4 waves) owns up to ROWS / 32 consecutive molecules (one in batches of up to SMALL_BATCH molecules, which are
// latency-bound) for the whole network: embedding, every layer, read-out.
// Node rows live in LDS ([ROWS][H + 1] buffers, ROWS = 64 for H <= 128 and 32 above); h is mirrored in a [N][H] workspace (node-level, L2-hot).
// Nothing of size [E, .] leaves the chip or even reaches LDS as a whole:
//   * edge_mlp.0 is column-split, W1 = [W_s | W_t | w_r]: A = h W_s^T + b1 and B = h W_t^T are node-level GEMMs; the pre-activation of edge
//     (i, j) is A_i + B_j + |x_i - x_j|^2 w_r, formed per lane as the A operand of the only per-edge GEMM, the H x H edge_mlp.2;
//   * that GEMM's accumulators ([32 edges][H] per wave, v_mfma_f32_32x32x2_f32) take SiLU, the attention dot product (in-lane over column
//     blocks, then a 32-lane xor butterfly), the gate and the mask in registers;
//   * a node's neighbour slots are padded to a multiple of 4 and aligned to 4, so a "quad" (4 accumulator registers of one lane half) always
//     belongs to one node: the quad is summed in the lane, staged ([32 quads][H] per round of 4 tiles) and added to agg_i in slot order by one
//     thread per column.  agg_i = (((0 + q_0) + q_1) + ...) whatever else is in the batch: no atomics, bit-identical, position-independent.
// All arithmetic fp32; every GEMM (node-level ones included, also the tiny graph_dec.0) is a k-ordered fmaf chain on the exact fp32 MFMA, rows
// independent of each other.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdarg.h>
#include <stdio.h>
#include <math.h>

namespace gcls {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MAX_N = 32;        // atoms per molecule (GCDM_CLASSIFIER_MAX_NODES)
constexpr int MAX_F = 16;        // in_node_nf (GCDM_CLASSIFIER_MAX_IN_NODE_NF); the packed K of every h0 product
constexpr int MAX_H = 256;       // hidden_nf, a multiple of 32
constexpr int THREADS = 256;
constexpr int SMALL_BATCH = 1024; // molecules: up to here one molecule per workgroup
constexpr int PER_LAYER_TENSORS = 10, HEAD_TENSORS = 2, TAIL_TENSORS = 8;

__host__ __device__ constexpr int rows_cap(int H) { return H <= 128 ? 64 : 32; }

// ---- packed weights: every matrix k-major ([k][n] = W[n][k]) so that a B operand is two coalesced 128-byte reads per wave ------------------
struct LayerOff { int64_t ws, wt, wr, b1, w2, b2, wa, ba, n1h, n1a, n1f, n1b, n2, n2b; };
struct Offsets {
    int64_t emb_w, emb_b, layer0, layer_stride, d1, d1b, d2, d2b, g1, g1b, g2, g2b, total;
    LayerOff lo;                  // relative to a layer's base
};
__host__ __device__ inline Offsets offsets(int H, int L) {
    Offsets o;
    const int64_t HH = (int64_t)H * H, FH = (int64_t)MAX_F * H;
    int64_t p = 0;
    o.emb_w = p; p += FH; o.emb_b = p; p += H;
    int64_t q = 0;
    o.lo.ws = q; q += HH; o.lo.wt = q; q += HH; o.lo.wr = q; q += H; o.lo.b1 = q; q += H; o.lo.w2 = q; q += HH; o.lo.b2 = q; q += H;
    o.lo.wa = q; q += H; o.lo.ba = q; q += 32; o.lo.n1h = q; q += HH; o.lo.n1a = q; q += HH; o.lo.n1f = q; q += FH; o.lo.n1b = q; q += H;
    o.lo.n2 = q; q += HH; o.lo.n2b = q; q += H;
    o.layer0 = p; o.layer_stride = q; p += q * L;
    o.d1 = p; p += HH; o.d1b = p; p += H; o.d2 = p; p += HH; o.d2b = p; p += H; o.g1 = p; p += HH; o.g1b = p; p += H; o.g2 = p; p += H;
    o.g2b = p; p += 32;
    o.total = p;
    return o;
}

// dst[k * n_out + n] = src[n * ld + col0 + k] for k < K, 0 for K <= k < Kpad; src == nullptr writes zeros
__global__ void k_pack_t(const float* __restrict__ src, float* __restrict__ dst, int n_out, int ld, int col0, int K, int Kpad) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)Kpad * n_out) return;
    const int k = (int)(idx / n_out), n = (int)(idx % n_out);
    dst[idx] = (src && k < K) ? src[(int64_t)n * ld + col0 + k] : 0.f;
}

__device__ __forceinline__ float silu(float v) { return v / (1.f + expf(-v)); }

__device__ __forceinline__ void seg_mma(f32x16& acc, const float* in, int ld, const float* __restrict__ w, int K, int H, int m0, int n0, int lane) {
    const float* pa = in + (m0 + (lane & 31)) * ld + (lane >> 5);
    const float* pb = w + (int64_t)(lane >> 5) * H + n0 + (lane & 31);
#pragma unroll 4
    for (int k = 0; k < K; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[k], pb[(int64_t)k * H], acc, 0, 0, 0);
}

// out[rows][H] = act(sum_s in_s . w_s + bias) (+ resid), rows of LDS buffers; the (row tile, column block) pairs go round the 4 waves.  Input
// rows past `rows` are read (inside the buffers) and their results dropped: GEMM rows are independent.  `out` aliases no input.
__device__ void gemm(float* out, int old, const float* in0, int ld0, const float* w0, int K0, const float* in1, int ld1, const float* w1, int K1,
                     const float* in2, int ld2, const float* w2, int K2, const float* __restrict__ bias, int rows, int H, bool act,
                     const float* resid, int rld, float* gout) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mt = (rows + 31) >> 5, nb = H >> 5;
    for (int t = wave; t < mt * nb; t += 4) {
        const int m0 = (t / nb) * 32, n0 = (t % nb) * 32;
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        seg_mma(acc, in0, ld0, w0, K0, H, m0, n0, lane);
        if (in1) seg_mma(acc, in1, ld1, w1, K1, H, m0, n0, lane);
        if (in2) seg_mma(acc, in2, ld2, w2, K2, H, m0, n0, lane);
        const int col = n0 + (lane & 31);
        const float bv = bias ? bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (row < rows) {
                float v = acc[r] + bv;
                if (act) v = silu(v);
                if (resid) v = resid[row * rld + col] + v;
                out[row * old + col] = v;
                if (gout) gout[(int64_t)row * H + col] = v;
            }
        }
    }
}

__host__ __device__ inline int64_t lds_floats(int H) {
    const int R = rows_cap(H);
    return 3LL * R * (H + 1) + 32LL * H + (int64_t)R * (MAX_F + 1) + R * 3 + H + (int64_t)R * MAX_N + 16;
}

template <int NB>
__global__ __launch_bounds__(THREADS) void k_forward(const float* __restrict__ x, const float* __restrict__ h0, const int32_t* __restrict__ noff,
                                                     const float* __restrict__ W, float* __restrict__ hbuf, float* __restrict__ pred,
                                                     float* __restrict__ hdbg, int dbg_layer, int64_t N, int B, int F, int L, int attention, int group) {
    constexpr int H = NB * 32, S = H + 1, R = H <= 128 ? 64 : 32, FS = MAX_F + 1;
    extern __shared__ float lds[];
    float* b0 = lds;
    float* b1 = b0 + R * S;
    float* b2 = b1 + R * S;
    float* Q = b2 + R * S;                        // [32 quads][H]
    float* h0s = Q + 32 * H;                      // [R][FS], columns F .. 15 zero
    float* xs = h0s + R * FS;                     // [R][3]
    float* wrs = xs + R * 3;                      // [H] the radial column of edge_mlp.0 of the current layer
    uint32_t* table = (uint32_t*)(wrs + H);       // [R * 32] slot -> row i | row j << 8 | valid << 16
    int* meta = (int*)(table + R * MAX_N);        // [0 .. group] local row starts, [8] ok
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mol0 = blockIdx.x * group;                 // group <= R / MAX_N molecules per workgroup (the host's choice; results do not depend on it)
    const int nmol = B - mol0 < group ? B - mol0 : group;
    const Offsets o = offsets(H, L);

    // ---- sizes: every molecule 0 .. MAX_N atoms, offsets inside [0, N]; anything else gives NaN predictions and touches nothing -----------
    if (tid == 0) {
        bool ok = true;
        const int64_t base = noff[mol0];
        ok = base >= 0 && base <= N;
        meta[0] = 0;
        for (int m = 0; m < nmol; ++m) {
            const int64_t a = noff[mol0 + m], b = noff[mol0 + m + 1];
            if (b < a || b - a > MAX_N || b > N || a < 0) ok = false;
            meta[m + 1] = ok ? (int)(b - base) : 0;
        }
        meta[8] = ok ? 1 : 0;
    }
    __syncthreads();
    if (!meta[8]) {
        if (tid < nmol) pred[mol0 + tid] = __builtin_nanf("");
        return;
    }
    const int64_t row0 = noff[mol0];
    const int rows = meta[nmol];
    float* hg = hbuf + row0 * H;

    // ---- inputs and the slot table -----------------------------------------------------------------------------------------------------
    for (int idx = tid; idx < R * FS; idx += THREADS) {
        const int r = idx / FS, c = idx % FS;
        h0s[idx] = (r < rows && c < F) ? h0[(row0 + r) * F + c] : 0.f;
    }
    for (int idx = tid; idx < R * 3; idx += THREADS) xs[idx] = idx < rows * 3 ? x[row0 * 3 + idx] : 0.f;
    int T = 0;                                    // slots of the group: per atom 4 ceil(n / 4), slot s = neighbour s of its molecule
    for (int m = 0; m < nmol; ++m) {
        const int s0 = meta[m], n = meta[m + 1] - s0, P = (n + 3) & ~3;
        for (int idx = tid; idx < n * P; idx += THREADS) {
            const int i = idx / P, s = idx % P;
            const bool valid = s < n && s != i;
            table[T + idx] = (uint32_t)(s0 + i) | (uint32_t)(s0 + (s < n ? s : i)) << 8 | (valid ? 1u << 16 : 0u);
        }
        T += n * P;
    }
    for (int idx = T + tid; idx < ((T + 31) & ~31); idx += THREADS) table[idx] = 0u;
    __syncthreads();

    // ---- embedding -----------------------------------------------------------------------------------------------------------------------
    gemm(b0, S, h0s, FS, W + o.emb_w, MAX_F, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, W + o.emb_b, rows, H, false, nullptr, 0, hg);
    __syncthreads();
    if (hdbg && dbg_layer == 0)
        for (int idx = tid; idx < rows * H; idx += THREADS) hdbg[row0 * H + idx] = b0[(idx / H) * S + idx % H];

    for (int l = 0; l < L; ++l) {
        const float* Wl = W + o.layer0 + o.layer_stride * l;
        // A = h W_s^T + b1 -> b1, B = h W_t^T -> b2
        gemm(b1, S, b0, S, Wl + o.lo.ws, H, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, Wl + o.lo.b1, rows, H, false, nullptr, 0, nullptr);
        gemm(b2, S, b0, S, Wl + o.lo.wt, H, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, rows, H, false, nullptr, 0, nullptr);
        if (tid < H) wrs[tid] = Wl[o.lo.wr + tid];
        __syncthreads();
        for (int idx = tid; idx < rows * S; idx += THREADS) b0[idx] = 0.f;          // agg
        __syncthreads();

        // ---- edges: rounds of 4 tiles of 32 slots -----------------------------------------------------------------------------------
        const float* W2 = Wl + o.lo.w2;
        for (int round = 0; round * 128 < T; ++round) {
            const int tile = round * 128 + wave * 32;
            if (tile < T) {
                const uint32_t ent = table[tile + (lane & 31)];
                const int i = ent & 0xff, j = (ent >> 8) & 0xff;
                const uint32_t vmask = (uint32_t)__ballot((ent >> 16) & 1);
                const float dx = xs[i * 3] - xs[j * 3], dy = xs[i * 3 + 1] - xs[j * 3 + 1], dz = xs[i * 3 + 2] - xs[j * 3 + 2];
                const float rad = dx * dx + dy * dy + dz * dz;
                f32x16 acc[NB];
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
                const float* pA = b1 + i * S + (lane >> 5);
                const float* pB = b2 + j * S + (lane >> 5);
                const float* pr = wrs + (lane >> 5);
                const float* pW = W2 + (lane >> 5) * H + (lane & 31);
#pragma unroll 2
                for (int k = 0; k < H; k += 2) {
                    const float t = silu(pA[k] + pB[k] + rad * pr[k]);
#pragma unroll
                    for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(t, pW[k * H + b * 32], acc[b], 0, 0, 0);
                }
                float b2v[NB], wav[NB];
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    b2v[b] = Wl[o.lo.b2 + b * 32 + (lane & 31)];
                    wav[b] = attention ? Wl[o.lo.wa + b * 32 + (lane & 31)] : 0.f;
                }
                const float ba = attention ? Wl[o.lo.ba] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int e = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    float p = 0.f;
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        acc[b][r] = silu(acc[b][r] + b2v[b]);
                        p = fmaf(wav[b], acc[b][r], p);
                    }
                    float g = 1.f;
                    if (attention) {
#pragma unroll
                        for (int off = 16; off >= 1; off >>= 1) p += __shfl_xor(p, off);
                        g = 1.f / (1.f + expf(-(p + ba)));
                    }
                    const bool valid = (vmask >> e) & 1u;
#pragma unroll
                    for (int b = 0; b < NB; ++b) acc[b][r] = valid ? acc[b][r] * g : 0.f;
                }
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const int quad = wave * 8 + 2 * g4 + (lane >> 5);
#pragma unroll
                    for (int b = 0; b < NB; ++b)
                        Q[quad * H + b * 32 + (lane & 31)] = ((acc[b][4 * g4] + acc[b][4 * g4 + 1]) + acc[b][4 * g4 + 2]) + acc[b][4 * g4 + 3];
                }
            }
            __syncthreads();
            if (tid < H) {
                const int left = T / 4 - round * 32, nq = left < 32 ? left : 32;
                for (int qq = 0; qq < nq; ++qq) {
                    const int node = table[(round * 32 + qq) * 4] & 0xff;
                    b0[node * S + tid] += Q[qq * H + tid];
                }
            }
            __syncthreads();
        }

        // ---- nodes: h += node_mlp([h | agg | h0]) -------------------------------------------------------------------------------------
        for (int idx = tid; idx < rows * H; idx += THREADS) b1[(idx / H) * S + idx % H] = hg[idx];
        __syncthreads();
        gemm(b2, S, b1, S, Wl + o.lo.n1h, H, b0, S, Wl + o.lo.n1a, H, h0s, FS, Wl + o.lo.n1f, MAX_F, Wl + o.lo.n1b, rows, H, true, nullptr, 0, nullptr);
        __syncthreads();
        gemm(b0, S, b2, S, Wl + o.lo.n2, H, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, Wl + o.lo.n2b, rows, H, false, b1, S, hg);
        __syncthreads();
        if (hdbg && dbg_layer == l + 1)
            for (int idx = tid; idx < rows * H; idx += THREADS) hdbg[row0 * H + idx] = b0[(idx / H) * S + idx % H];
    }

    // ---- read-out: node_dec, sum over the atoms of a molecule in index order, graph_dec ---------------------------------------------------
    gemm(b1, S, b0, S, W + o.d1, H, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, W + o.d1b, rows, H, true, nullptr, 0, nullptr);
    __syncthreads();
    gemm(b2, S, b1, S, W + o.d2, H, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, W + o.d2b, rows, H, false, nullptr, 0, nullptr);
    __syncthreads();
    if (tid < H)
        for (int m = 0; m < nmol; ++m) {
            float s = 0.f;
            for (int r = meta[m]; r < meta[m + 1]; ++r) s += b2[r * S + tid];
            b0[m * S + tid] = s;
        }
    __syncthreads();
    gemm(b1, S, b0, S, W + o.g1, H, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, W + o.g1b, nmol, H, true, nullptr, 0, nullptr);
    __syncthreads();
    if (wave < nmol) {
        float s = 0.f;
        for (int n = lane; n < H; n += 64) s = fmaf(b1[wave * S + n], W[o.g2 + n], s);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0) pred[mol0 + wave] = s + W[o.g2b];
    }
}

static thread_local char g_err[256] = "";
__attribute__((format(printf, 2, 3))) static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

static int check_dims(int F, int H, int L) {
    if (F < 1 || F > MAX_F) return fail(-1, "in_node_nf = %d: the limit is 1 .. %d", F, MAX_F);
    if (H < 32 || H > MAX_H || H % 32) return fail(-1, "hidden_nf = %d: the limit is a multiple of 32 up to %d", H, MAX_H);
    if (L < 1) return fail(-1, "n_layers = %d: the limit is >= 1", L);
    return 0;
}

template <int NB>
static int launch(const float* x, const float* h0, const int32_t* noff, const float* W, float* hbuf, float* pred, float* hdbg, int dbg, int64_t N,
                  int B, int F, int L, int att, hipStream_t st) {
    constexpr int H = NB * 32;
    // a weight pass serves rows_cap / MAX_N molecules when there are enough of them to fill the chip; a small batch (the evaluation driver's 100)
    // is latency-bound on too few workgroups, so it gets one molecule per workgroup
    const int GROUP = B <= SMALL_BATCH ? 1 : rows_cap(H) / MAX_N;
    const size_t bytes = (size_t)lds_floats(H) * 4;
    if (hipFuncSetAttribute((const void*)k_forward<NB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
        return fail(-2, "hipFuncSetAttribute(%zu bytes of LDS) failed", bytes);
    hipLaunchKernelGGL(k_forward<NB>, dim3((B + GROUP - 1) / GROUP), dim3(THREADS), bytes, st, x, h0, noff, W, hbuf, pred, hdbg, dbg, N, B, F, L, att, GROUP);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(-2, "classifier forward launch failed: %s", hipGetErrorString(e));
}

}  // namespace gcls

extern "C" {

const char* gcdm_classifier_last_error(void) { return gcls::g_err; }

int64_t gcdm_classifier_workspace_bytes(int32_t which, int64_t num_nodes, int32_t in_node_nf, int32_t hidden_nf, int32_t n_layers) {
    using namespace gcls;
    if (which < 0 || which > 4) return fail(-1, "which = %d: 0 .. 4", which);
    if (num_nodes < 0) return fail(-1, "num_nodes = %lld is negative", (long long)num_nodes);
    if (check_dims(in_node_nf, hidden_nf, n_layers)) return -1;
    switch (which) {
        case 0: return (num_nodes * hidden_nf * 4 + 255) / 256 * 256 + 256;
        case 1: return offsets(hidden_nf, n_layers).total * 4;
        case 2: return 1;                                     // launches per forward
        case 3: return lds_floats(hidden_nf) * 4;
        default: return rows_cap(hidden_nf) / MAX_N;          // molecules per workgroup
    }
}

int gcdm_classifier_pack(const void* const* tensors, int32_t count, int32_t in_node_nf, int32_t hidden_nf, int32_t n_layers, int32_t attention,
                         int32_t node_attr, float* packed, void* stream) {
    using namespace gcls;
    const int F = in_node_nf, H = hidden_nf, L = n_layers;
    if (check_dims(F, H, L)) return -1;
    if ((attention | 1) != 1 || (node_attr | 1) != 1) return fail(-1, "attention and node_attr are 0 or 1");
    if (count != HEAD_TENSORS + PER_LAYER_TENSORS * L + TAIL_TENSORS) return fail(-1, "count = %d tensors: expected %d", count, HEAD_TENSORS + PER_LAYER_TENSORS * L + TAIL_TENSORS);
    if (!tensors || !packed) return fail(-1, "null tensor table or packed buffer");
    for (int i = 0; i < count; ++i) {
        const int k = i < HEAD_TENSORS ? -1 : (i - HEAD_TENSORS) % PER_LAYER_TENSORS;
        const bool att_slot = i >= HEAD_TENSORS && i < HEAD_TENSORS + PER_LAYER_TENSORS * L && (k == 8 || k == 9);
        if (!tensors[i] && !(att_slot && !attention)) return fail(-1, "tensor %d is null", i);
    }
    const Offsets o = offsets(H, L);
    hipStream_t st = (hipStream_t)stream;
    auto T = [&](int i) { return (const float*)tensors[i]; };
    auto put = [&](const float* src, int64_t dst, int n_out, int ld, int col0, int K, int Kpad) {
        const int64_t n = (int64_t)Kpad * n_out;
        hipLaunchKernelGGL(k_pack_t, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, packed + dst, n_out, ld, col0, K, Kpad);
    };
    auto vec = [&](const float* src, int64_t dst, int n, int npad) { put(src, dst, 1, 1, 0, src ? n : 0, npad); };
    put(T(0), o.emb_w, H, F, 0, F, MAX_F);
    vec(T(1), o.emb_b, H, H);
    const int in1 = 2 * H + 1, in2 = 2 * H + (node_attr ? F : 0);
    for (int l = 0; l < L; ++l) {
        const int t = HEAD_TENSORS + PER_LAYER_TENSORS * l;
        const int64_t b = o.layer0 + o.layer_stride * l;
        put(T(t), b + o.lo.ws, H, in1, 0, H, H);
        put(T(t), b + o.lo.wt, H, in1, H, H, H);
        put(T(t), b + o.lo.wr, H, in1, 2 * H, 1, 1);
        vec(T(t + 1), b + o.lo.b1, H, H);
        put(T(t + 2), b + o.lo.w2, H, H, 0, H, H);
        vec(T(t + 3), b + o.lo.b2, H, H);
        put(T(t + 4), b + o.lo.n1h, H, in2, 0, H, H);
        put(T(t + 4), b + o.lo.n1a, H, in2, H, H, H);
        put(node_attr ? T(t + 4) : nullptr, b + o.lo.n1f, H, in2, 2 * H, F, MAX_F);
        vec(T(t + 5), b + o.lo.n1b, H, H);
        put(T(t + 6), b + o.lo.n2, H, H, 0, H, H);
        vec(T(t + 7), b + o.lo.n2b, H, H);
        vec(attention ? T(t + 8) : nullptr, b + o.lo.wa, H, H);
        vec(attention ? T(t + 9) : nullptr, b + o.lo.ba, 1, 32);
    }
    const int t = HEAD_TENSORS + PER_LAYER_TENSORS * L;
    put(T(t), o.d1, H, H, 0, H, H);     vec(T(t + 1), o.d1b, H, H);
    put(T(t + 2), o.d2, H, H, 0, H, H); vec(T(t + 3), o.d2b, H, H);
    put(T(t + 4), o.g1, H, H, 0, H, H); vec(T(t + 5), o.g1b, H, H);
    vec(T(t + 6), o.g2, H, H);          vec(T(t + 7), o.g2b, 1, 32);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(-2, "classifier pack launch failed: %s", hipGetErrorString(e));
}

int gcdm_classifier_forward(const float* x, const float* h0, const int32_t* node_offsets, const float* packed, void* workspace, float* pred,
                            float* h_debug, int32_t debug_layer, int64_t num_nodes, int64_t num_molecules, int32_t in_node_nf, int32_t hidden_nf,
                            int32_t n_layers, int32_t attention, void* stream) {
    using namespace gcls;
    if (check_dims(in_node_nf, hidden_nf, n_layers)) return -1;
    if ((attention | 1) != 1) return fail(-1, "attention is 0 or 1");
    if (num_nodes < 0 || num_molecules < 0) return fail(-1, "negative size");
    if (num_molecules > (1LL << 30) || num_nodes > (1LL << 31) - 1) return fail(-1, "batch too large: at most 2^30 molecules and 2^31 - 1 atoms");
    if (num_nodes > num_molecules * MAX_N) return fail(-1, "%lld atoms in %lld molecules: the limit is %d atoms per molecule", (long long)num_nodes, (long long)num_molecules, MAX_N);
    if (debug_layer < -1 || debug_layer > n_layers) return fail(-1, "debug_layer = %d: -1 .. n_layers", debug_layer);
    if (debug_layer >= 0 && !h_debug) return fail(-1, "debug_layer without h_debug");
    if (num_molecules == 0) return 0;
    if (!node_offsets || !packed || !pred || !workspace) return fail(-1, "null pointer");
    if (num_nodes > 0 && (!x || !h0)) return fail(-1, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    float* hd = debug_layer >= 0 ? h_debug : nullptr;
    const int B = (int)num_molecules;
#define GCLS_CASE(NB) case NB: return launch<NB>(x, h0, node_offsets, packed, (float*)workspace, pred, hd, debug_layer, num_nodes, B, in_node_nf, n_layers, attention, st);
    switch (hidden_nf / 32) {
        GCLS_CASE(1) GCLS_CASE(2) GCLS_CASE(3) GCLS_CASE(4) GCLS_CASE(5) GCLS_CASE(6) GCLS_CASE(7) GCLS_CASE(8)
    }
#undef GCLS_CASE
    return fail(-1, "hidden_nf = %d", hidden_nf);
}

}  // extern "C"
