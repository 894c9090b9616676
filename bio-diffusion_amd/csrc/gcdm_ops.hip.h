// gcdm_ops.hip.h -- the MODULE-LEVEL operators of the GCPNet block as stand-alone HIP kernels (gfx950), forward and backward.
//
// The fused kernels (gcdm_kernels.hip.h, gcdm_edge_x3.hip.h, gcdm_node_x3.hip.h) evaluate the production configuration of
// GCPNetDynamics.forward in ~25 launches; this file is the other end of the trade: every arithmetic step the reference's modules take
// (src/models/components/gcpnet.py GCP :33-262, GCP2 :265-491, GCPMessagePassing :618-737, GCPInteractions :740-930;
// src/models/components/__init__.py localize :123-171, scalarize :174-224, vectorize :227-272, safe_norm :275-286, GCPLayerNorm :779-808)
// as one small kernel with its backward twin, for ANY dimension and flag.  The Python mirrors (bio-diffusion_amd/gcpnet.py) compose them
// exactly where the reference composes torch ops, which gives
//   * plug point 3: `module_cfg.selected_GCP(in, out, ...)(s_maybe_v, edge_index, frames, ...)` is callable (GCP and GCP2, every flag);
//   * the non-production settings of the path's Hydra surface (frame_gate, GCP v1, residuals, ablations, gcp norm, vector-sum position
//     updates, any hidden size / number of message layers) -- slower than the fused path, same results;
//   * the training objective: each operator is a torch.autograd.Function whose backward is the kernel below (ops.py).
// Layouts: scalars [M][C] row-major; vectors in the reference's two layouts, "rep" [M][C][3] and "pre" [M][3][C] (its transpose(-1,-2));
// frames [M][9] = rows a, b, c of f_ij.  All fp32.  No fallback: a launch failure is reported through the int status.
#pragma once
#include "gcdm_ops.tile.hip.h"
#include "../../include/gcdm_matrix_mode.h"
#include <atomic>

namespace gops {

// column sums of dy [M][N] (bias gradient): one workgroup per 64 columns, fixed summation order (rows strided over the threads, then a tree)
__global__ __launch_bounds__(256) void k_colsum(const float* __restrict__ dy, float* __restrict__ db, int64_t M, int N) {
    __shared__ float red[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
    float s = 0.f;
    if (c < N)
        for (int64_t m = g; m < M; m += 4) s += dy[m * N + c];
    red[g][threadIdx.x & 63] = s;
    __syncthreads();
    if (g == 0 && c < N) db[c] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// the same over `slices` contiguous row ranges (grid.y), partial sums to part[slice][N]: with M = #edges one workgroup per 64 columns leaves 252 of
// 256 CUs idle (260 us per call, 58 % of a training step); gcdm_op_reduce_slices adds the partials in slice order (deterministic)
__global__ __launch_bounds__(256) void k_colsum_slices(const float* __restrict__ dy, float* __restrict__ part, int64_t M, int N, int64_t rows) {
    __shared__ float red[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
    const int64_t m0 = (int64_t)blockIdx.y * rows, m1 = m0 + rows < M ? m0 + rows : M;
    float s = 0.f;
    if (c < N)
        for (int64_t m = m0 + g; m < m1; m += 4) s += dy[m * N + c];
    red[g][threadIdx.x & 63] = s;
    __syncthreads();
    if (g == 0 && c < N) part[(int64_t)blockIdx.y * N + c] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// ---- element-wise nonlinearities (act_f / act_df: gcdm_ops.tile.hip.h) -----------------------------------------------------------------------
__global__ void k_act(int kind, const float* __restrict__ x, float* __restrict__ y, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = act_f(kind, x[i]);
}
__global__ void k_act_bwd(int kind, const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dx[i] = dy[i] * act_df(kind, x[i]);
}

// ---- safe_norm over the spatial axis (components/__init__.py:275-286: sqrt(sum x^2 + eps) + eps) -----------------------------------------
// element (m, c, x) of v at m * 3C + c * sc + x * sx:  "pre" layout [M][3][C]: sc = 1, sx = C;   "rep" layout [M][C][3]: sc = 3, sx = 1
__global__ void k_norm3(const float* __restrict__ v, float* __restrict__ out, int64_t MC, int C, int sc, int sx, float eps) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= MC) return;
    const int64_t m = i / C;
    const int c = (int)(i - m * C);
    const float* p = v + m * 3 * C + (int64_t)c * sc;
    const float a = p[0], b = p[sx], d = p[2 * sx];
    out[i] = sqrtf(a * a + b * b + d * d + eps) + eps;
}
__global__ void k_norm3_bwd(const float* __restrict__ v, const float* __restrict__ out, const float* __restrict__ dout, float* __restrict__ dv,
                            int64_t MC, int C, int sc, int sx, float eps) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= MC) return;
    const int64_t m = i / C;
    const int c = (int)(i - m * C);
    const int64_t o = m * 3 * C + (int64_t)c * sc;
    const float g = dout[i] / (out[i] - eps);           // d/dv sqrt(s + eps) = v / sqrt(s + eps)
    dv[o] = g * v[o];
    dv[o + sx] = g * v[o + sx];
    dv[o + 2 * sx] = g * v[o + 2 * sx];
}

// ---- scalarize / vectorize against per-entity frames F[m] = rows (a, b, c) (components/__init__.py:174-272) ----------------------------------
// scalarize: u in "pre" layout [M][3 xyz][CH]; out[m][CH * ... ] follows the reference: out[m][3 c + r] = F[m][r][:] . u[m][:][c]
__global__ void k_scalarize(const float* __restrict__ u, const float* __restrict__ F, float* __restrict__ out, int64_t M, int CH) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;        // one thread per (m, c)
    if (i >= M * CH) return;
    const int64_t m = i / CH;
    const int c = (int)(i - m * CH);
    const float* f = F + m * 9;
    const float* p = u + m * 3 * CH + c;
    const float x = p[0], y = p[CH], z = p[2 * CH];
#pragma unroll
    for (int r = 0; r < 3; ++r) out[m * 3 * CH + 3 * c + r] = f[3 * r] * x + f[3 * r + 1] * y + f[3 * r + 2] * z;
}
__global__ void k_scalarize_bwd(const float* __restrict__ dout, const float* __restrict__ F, float* __restrict__ du, int64_t M, int CH) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * CH) return;
    const int64_t m = i / CH;
    const int c = (int)(i - m * CH);
    const float* f = F + m * 9;
    const float* d = dout + m * 3 * CH + 3 * c;
#pragma unroll
    for (int x = 0; x < 3; ++x) du[m * 3 * CH + (int64_t)x * CH + c] = f[x] * d[0] + f[3 + x] * d[1] + f[6 + x] * d[2];
}
// vectorize: gate [M][3 K], out "rep" layout [M][K][3]: out[m][k][:] = gate[3k] a + gate[3k+1] b + gate[3k+2] c
__global__ void k_vectorize(const float* __restrict__ gate, const float* __restrict__ F, float* __restrict__ out, int64_t M, int KC) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * KC) return;
    const int64_t m = i / KC;
    const float* f = F + m * 9;
    const float* g = gate + i * 3;
#pragma unroll
    for (int x = 0; x < 3; ++x) out[i * 3 + x] = g[0] * f[x] + g[1] * f[3 + x] + g[2] * f[6 + x];
}
__global__ void k_vectorize_bwd(const float* __restrict__ dout, const float* __restrict__ F, float* __restrict__ dgate, int64_t M, int KC) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * KC) return;
    const int64_t m = i / KC;
    const float* f = F + m * 9;
    const float* d = dout + i * 3;
#pragma unroll
    for (int r = 0; r < 3; ++r) dgate[i * 3 + r] = d[0] * f[3 * r] + d[1] * f[3 * r + 1] + d[2] * f[3 * r + 2];
}

// ---- row-wise gating of vectors: out[m][c][:] = v[m][c][:] * g[m][c]   ("rep" layout) --------------------------------------------------------
__global__ void k_rowscale(const float* __restrict__ v, const float* __restrict__ g, float* __restrict__ out, int64_t MC) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= MC) return;
    const float s = g[i];
    out[3 * i] = v[3 * i] * s; out[3 * i + 1] = v[3 * i + 1] * s; out[3 * i + 2] = v[3 * i + 2] * s;
}
__global__ void k_rowscale_bwd(const float* __restrict__ v, const float* __restrict__ g, const float* __restrict__ dout, float* __restrict__ dv,
                               float* __restrict__ dg, int64_t MC) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= MC) return;
    const float s = g[i];
    const float a = dout[3 * i], b = dout[3 * i + 1], c = dout[3 * i + 2];
    dv[3 * i] = a * s; dv[3 * i + 1] = b * s; dv[3 * i + 2] = c * s;
    dg[i] = a * v[3 * i] + b * v[3 * i + 1] + c * v[3 * i + 2];
}

// ---- graph plumbing: CSR of a row-sorted edge list, gather, segment sum / mean, scatter-add ---------------------------------------------------
// rowptr[i] = first edge with row >= i (binary search: the edge list of get_fully_connected_edge_index is sorted by row, gcpnet.py:1054-1066);
// bit 0 of *flag is raised if the list is not sorted
__global__ void k_rowptr(const int64_t* __restrict__ row, int64_t E, int64_t N, int32_t* __restrict__ rowptr, int32_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= N) {
        int64_t lo = 0, hi = E;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (row[mid] < i) lo = mid + 1; else hi = mid; }
        rowptr[i] = (int32_t)lo;
    }
    for (int64_t e = i; e + 1 < E; e += (int64_t)gridDim.x * blockDim.x)
        if (row[e] > row[e + 1]) atomicOr(flag, 1);
}
__global__ void k_gather(const float* __restrict__ x, const int64_t* __restrict__ idx, float* __restrict__ out, int64_t E, int C) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E * C) return;
    const int64_t e = i / C;
    out[i] = x[idx[e] * C + (i - e * C)];
}
// out[n][c] = sum (mean) over the edges rowptr[n] .. rowptr[n+1]-1, in edge order (= the index_add_ order of torch_scatter): deterministic
__global__ void k_segment_sum(const float* __restrict__ x, const int32_t* __restrict__ rowptr, float* __restrict__ out, int64_t N, int C, int mean) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * C) return;
    const int64_t n = i / C;
    const int c = (int)(i - n * C);
    const int b = rowptr[n], e = rowptr[n + 1];
    float s = 0.f;
    for (int k = b; k < e; ++k) s += x[(int64_t)k * C + c];
    if (mean) s /= (float)(e - b > 1 ? e - b : 1);            // torch_scatter: counts clamped to >= 1
    out[i] = s;
}
// backward of segment sum / mean: every edge receives its row's gradient (/ count)
__global__ void k_segment_bwd(const float* __restrict__ dout, const int64_t* __restrict__ row, const int32_t* __restrict__ rowptr, float* __restrict__ dx,
                              int64_t E, int C, int mean) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E * C) return;
    const int64_t e = i / C;
    const int64_t n = row[e];
    float g = dout[n * C + (i - e * C)];
    if (mean) { const int cnt = rowptr[n + 1] - rowptr[n]; g /= (float)(cnt > 1 ? cnt : 1); }
    dx[i] = g;
}
// backward of a gather by an UNSORTED index (ops.embedding's table gradient): fp32 atomics, summation order not fixed.  (The gather by an edge
// list's column index is summed in the graph's column order instead: gcdm_op_gather + gcdm_op_segment_sum, ops.py)
__global__ void k_scatter_add(const float* __restrict__ dy, const int64_t* __restrict__ idx, float* __restrict__ out, int64_t E, int C) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E * C) return;
    const int64_t e = i / C;
    atomicAdd(out + idx[e] * C + (i - e * C), dy[i]);
}

// ---- geometry of the input graph (no gradients: functions of the network INPUT only) -------------------------------------------------------------
// localize (components/__init__.py:123-171, norm_x_diff): a = d / (|d| + 1), b = (x_i x x_j) / (|x_i x x_j| + 1), c = a x b
__global__ void k_localize(const float* __restrict__ x, const int64_t* __restrict__ row, const int64_t* __restrict__ col, float* __restrict__ F, int64_t E,
                           int norm_x_diff) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const float* xi = x + row[e] * 3;
    const float* xj = x + col[e] * 3;
    float a0 = xi[0] - xj[0], a1 = xi[1] - xj[1], a2 = xi[2] - xj[2];
    float b0 = xi[1] * xj[2] - xi[2] * xj[1], b1 = xi[2] * xj[0] - xi[0] * xj[2], b2 = xi[0] * xj[1] - xi[1] * xj[0];
    if (norm_x_diff) {
        const float na = 1.f / (sqrtf(a0 * a0 + a1 * a1 + a2 * a2) + 1.f), nb = 1.f / (sqrtf(b0 * b0 + b1 * b1 + b2 * b2) + 1.f);
        a0 *= na; a1 *= na; a2 *= na;
        b0 *= nb; b1 *= nb; b2 *= nb;
    }
    float* f = F + e * 9;
    f[0] = a0; f[1] = a1; f[2] = a2;
    f[3] = b0; f[4] = b1; f[5] = b2;
    f[6] = a1 * b2 - a2 * b1; f[7] = a2 * b0 - a0 * b2; f[8] = a0 * b1 - a1 * b0;
}
// _edge_features (src/datamodules/components/protein_graph_dataset.py via gcpnet.py:1109): e = |x_i - x_j|^2, xi = normalize(x_i - x_j) (NaN -> 0)
__global__ void k_edge_features(const float* __restrict__ x, const int64_t* __restrict__ row, const int64_t* __restrict__ col, float* __restrict__ e_out,
                                float* __restrict__ xi_out, int64_t E) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const float* xi = x + row[e] * 3;
    const float* xj = x + col[e] * 3;
    const float d0 = xi[0] - xj[0], d1 = xi[1] - xj[1], d2 = xi[2] - xj[2];
    const float r2 = d0 * d0 + d1 * d1 + d2 * d2;
    e_out[e] = r2;
    const float n = sqrtf(r2);
    const float inv = n > 0.f ? 1.f / n : 0.f;               // nan_to_num(v / |v|): 0 / 0 -> 0
    xi_out[3 * e] = d0 * inv; xi_out[3 * e + 1] = d1 * inv; xi_out[3 * e + 2] = d2 * inv;
}
// _orientations over the FLAT batch (protein_graph_dataset.py:217-225): [normalize(x[i+1] - x[i]) (0 for the last), normalize(x[i-1] - x[i]) (0 for the first)]
__global__ void k_orientations(const float* __restrict__ x, float* __restrict__ out, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int64_t j = s == 0 ? i + 1 : i - 1;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
        if (j >= 0 && j < N) {
            d0 = x[3 * j] - x[3 * i]; d1 = x[3 * j + 1] - x[3 * i + 1]; d2 = x[3 * j + 2] - x[3 * i + 2];
            const float n = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
            const float inv = n > 0.f ? 1.f / n : 0.f;
            d0 *= inv; d1 *= inv; d2 *= inv;
        }
        out[i * 6 + 3 * s] = d0; out[i * 6 + 3 * s + 1] = d1; out[i * 6 + 3 * s + 2] = d2;
    }
}
// per-molecule mean over the unmasked nodes subtracted (centralize, components/__init__.py:45-92; batch_index sorted): each node walks its molecule
__global__ void k_centralize(const float* __restrict__ x, const int64_t* __restrict__ bi, const uint8_t* __restrict__ mask, float* __restrict__ out, int64_t N,
                             int D) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int64_t b = bi[i];
    int64_t lo = i, hi = i;
    while (lo > 0 && bi[lo - 1] == b) --lo;
    while (hi + 1 < N && bi[hi + 1] == b) ++hi;
    float cnt = 0.f;
    for (int64_t j = lo; j <= hi; ++j) cnt += (!mask || mask[j]) ? 1.f : 0.f;
    const bool on = !mask || mask[i];
    for (int d = 0; d < D; ++d) {
        float s = 0.f;
        for (int64_t j = lo; j <= hi; ++j) s += (!mask || mask[j]) ? x[j * D + d] : 0.f;
        out[i * D + d] = on ? x[i * D + d] - s / (cnt > 0.f ? cnt : 1.f) : 0.f;      // masked rows: 0, as `x * mask` in the reference
    }
}
// get_fully_connected_edge_index (gcpnet.py:1054-1066): all (i, j) of a molecule INCLUDING i == j, sorted by i then j; eoff[b] = first edge of molecule b
__global__ void k_fc_edges(const int32_t* __restrict__ noff, const int64_t* __restrict__ eoff, int B, int64_t* __restrict__ row, int64_t* __restrict__ col,
                           int64_t E) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    int lo = 0, hi = B - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (eoff[mid] <= e) lo = mid; else hi = mid - 1; }
    const int n = noff[lo + 1] - noff[lo];
    const int64_t r = e - eoff[lo];
    row[e] = noff[lo] + r / n;
    col[e] = noff[lo] + r % n;
}

}  // namespace gops

// ------------------------------------------------------------------------------------------------------------------------------------------
// C ABI (include/gcdm_ops.h).  Handle-less: device pointers, sizes, a hipStream_t as void*; returns 0 or a negative status.
// ------------------------------------------------------------------------------------------------------------------------------------------
#define GOPS_LAUNCH_OK() (hipGetLastError() == hipSuccess ? 0 : -2)
static inline unsigned gops_blocks(int64_t n, int t = 256) { return (unsigned)((n + t - 1) / t); }
// argument checks, all before any HIP call: a negative size, a flag outside its range or a null pointer the (non-empty) work needs is -1;
// empty work is 0 without a launch
#define GOPS_REQUIRE(cond) do { if (!(cond)) return -1; } while (0)
static inline bool gops_flag(int32_t v) { return v == 0 || v == 1; }
// the process-wide matrix mode (include/gcdm_matrix_mode.h): one atomic word, so the autograd thread sees what the caller's thread set
static std::atomic<int32_t> g_gops_matrix_mode{gops::MM_F32};
static inline int gops_matrix_mode() { return g_gops_matrix_mode.load(std::memory_order_acquire); }

extern "C" {

int gcdm_op_gemm(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn, float* C, const float* bias, int64_t M, int32_t N,
                 int64_t K, int32_t slices, void* stream) {
    GOPS_REQUIRE(M >= 0 && N >= 0 && K >= 0 && slices >= 1);
    if (M == 0 || N == 0) return 0;
    GOPS_REQUIRE(A && B && C);
    gops::gemm(A, sam, sak, B, sbk, sbn, C, bias, M, N, K, (hipStream_t)stream, slices, gops_matrix_mode());
    return GOPS_LAUNCH_OK();
}
int gcdm_ops_set_matrix_mode(int32_t mode) {
    GOPS_REQUIRE(mode == gops::MM_F32 || mode == gops::MM_BF16X6);
    g_gops_matrix_mode.store(mode, std::memory_order_release);
    return 0;
}
int32_t gcdm_ops_get_matrix_mode(void) { return gops_matrix_mode(); }
int gcdm_op_reduce_slices(const float* part, float* out, int64_t n, int32_t slices, void* stream) {
    GOPS_REQUIRE(n >= 0 && slices >= 1);
    if (n == 0) return 0;
    GOPS_REQUIRE(part && out);
    hipLaunchKernelGGL(gops::k_reduce_slices, dim3(gops_blocks(n)), dim3(256), 0, (hipStream_t)stream, part, out, n, slices);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_colsum(const float* dy, float* db, int64_t M, int32_t N, void* stream) {
    GOPS_REQUIRE(M >= 0 && N >= 0);
    if (N == 0) return 0;
    GOPS_REQUIRE(db && (M == 0 || dy));
    hipLaunchKernelGGL(gops::k_colsum, dim3((N + 63) / 64), dim3(256), 0, (hipStream_t)stream, dy, db, M, N);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_colsum_slices(const float* dy, float* part, int64_t M, int32_t N, int32_t slices, void* stream) {
    GOPS_REQUIRE(M >= 0 && N >= 0 && slices >= 1);
    if (N == 0) return 0;
    GOPS_REQUIRE(part && (M == 0 || dy));
    const int64_t rows = (M + slices - 1) / slices;
    hipLaunchKernelGGL(gops::k_colsum_slices, dim3((N + 63) / 64, slices), dim3(256), 0, (hipStream_t)stream, dy, part, M, N, rows);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_act(int32_t kind, const float* x, float* y, int64_t n, void* stream) {
    GOPS_REQUIRE(kind >= 0 && kind <= 5 && n >= 0);
    if (n == 0) return 0;
    GOPS_REQUIRE(x && y);
    hipLaunchKernelGGL(gops::k_act, dim3(gops_blocks(n)), dim3(256), 0, (hipStream_t)stream, kind, x, y, n);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_act_bwd(int32_t kind, const float* x, const float* dy, float* dx, int64_t n, void* stream) {
    GOPS_REQUIRE(kind >= 0 && kind <= 5 && n >= 0);
    if (n == 0) return 0;
    GOPS_REQUIRE(x && dy && dx);
    hipLaunchKernelGGL(gops::k_act_bwd, dim3(gops_blocks(n)), dim3(256), 0, (hipStream_t)stream, kind, x, dy, dx, n);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_norm3(const float* v, float* out, int64_t M, int32_t C, int32_t rep_layout, void* stream) {
    GOPS_REQUIRE(M >= 0 && C >= 0 && gops_flag(rep_layout));
    if (M == 0 || C == 0) return 0;
    GOPS_REQUIRE(v && out);
    hipLaunchKernelGGL(gops::k_norm3, dim3(gops_blocks(M * C)), dim3(256), 0, (hipStream_t)stream, v, out, M * C, C, rep_layout ? 3 : 1, rep_layout ? 1 : C, 1e-8f);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_norm3_bwd(const float* v, const float* out, const float* dout, float* dv, int64_t M, int32_t C, int32_t rep_layout, void* stream) {
    GOPS_REQUIRE(M >= 0 && C >= 0 && gops_flag(rep_layout));
    if (M == 0 || C == 0) return 0;
    GOPS_REQUIRE(v && out && dout && dv);
    hipLaunchKernelGGL(gops::k_norm3_bwd, dim3(gops_blocks(M * C)), dim3(256), 0, (hipStream_t)stream, v, out, dout, dv, M * C, C, rep_layout ? 3 : 1,
                       rep_layout ? 1 : C, 1e-8f);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_scalarize(const float* u, const float* F, float* out, int64_t M, int32_t CH, void* stream) {
    GOPS_REQUIRE(M >= 0 && CH >= 0);
    if (M == 0 || CH == 0) return 0;
    GOPS_REQUIRE(u && F && out);
    hipLaunchKernelGGL(gops::k_scalarize, dim3(gops_blocks(M * CH)), dim3(256), 0, (hipStream_t)stream, u, F, out, M, CH);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_scalarize_bwd(const float* dout, const float* F, float* du, int64_t M, int32_t CH, void* stream) {
    GOPS_REQUIRE(M >= 0 && CH >= 0);
    if (M == 0 || CH == 0) return 0;
    GOPS_REQUIRE(dout && F && du);
    hipLaunchKernelGGL(gops::k_scalarize_bwd, dim3(gops_blocks(M * CH)), dim3(256), 0, (hipStream_t)stream, dout, F, du, M, CH);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_vectorize(const float* gate, const float* F, float* out, int64_t M, int32_t KC, void* stream) {
    GOPS_REQUIRE(M >= 0 && KC >= 0);
    if (M == 0 || KC == 0) return 0;
    GOPS_REQUIRE(gate && F && out);
    hipLaunchKernelGGL(gops::k_vectorize, dim3(gops_blocks(M * KC)), dim3(256), 0, (hipStream_t)stream, gate, F, out, M, KC);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_vectorize_bwd(const float* dout, const float* F, float* dgate, int64_t M, int32_t KC, void* stream) {
    GOPS_REQUIRE(M >= 0 && KC >= 0);
    if (M == 0 || KC == 0) return 0;
    GOPS_REQUIRE(dout && F && dgate);
    hipLaunchKernelGGL(gops::k_vectorize_bwd, dim3(gops_blocks(M * KC)), dim3(256), 0, (hipStream_t)stream, dout, F, dgate, M, KC);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_rowscale(const float* v, const float* g, float* out, int64_t M, int32_t C, void* stream) {
    GOPS_REQUIRE(M >= 0 && C >= 0);
    if (M == 0 || C == 0) return 0;
    GOPS_REQUIRE(v && g && out);
    hipLaunchKernelGGL(gops::k_rowscale, dim3(gops_blocks(M * C)), dim3(256), 0, (hipStream_t)stream, v, g, out, M * C);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_rowscale_bwd(const float* v, const float* g, const float* dout, float* dv, float* dg, int64_t M, int32_t C, void* stream) {
    GOPS_REQUIRE(M >= 0 && C >= 0);
    if (M == 0 || C == 0) return 0;
    GOPS_REQUIRE(v && g && dout && dv && dg);
    hipLaunchKernelGGL(gops::k_rowscale_bwd, dim3(gops_blocks(M * C)), dim3(256), 0, (hipStream_t)stream, v, g, dout, dv, dg, M * C);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_rowptr(const int64_t* row, int64_t E, int64_t N, int32_t* rowptr, int32_t* flag, void* stream) {
    GOPS_REQUIRE(E >= 0 && N >= 0);
    GOPS_REQUIRE(rowptr && flag && (E == 0 || row));          // never empty: rowptr has N + 1 entries
    const int64_t n = (N + 1 > E ? N + 1 : E);
    hipLaunchKernelGGL(gops::k_rowptr, dim3(gops_blocks(n)), dim3(256), 0, (hipStream_t)stream, row, E, N, rowptr, flag);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_gather(const float* x, const int64_t* idx, float* out, int64_t E, int32_t C, void* stream) {
    GOPS_REQUIRE(E >= 0 && C >= 0);
    if (E == 0 || C == 0) return 0;
    GOPS_REQUIRE(x && idx && out);
    hipLaunchKernelGGL(gops::k_gather, dim3(gops_blocks(E * C)), dim3(256), 0, (hipStream_t)stream, x, idx, out, E, C);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_segment_sum(const float* x, const int32_t* rowptr, float* out, int64_t N, int32_t C, int32_t mean, void* stream) {
    GOPS_REQUIRE(N >= 0 && C >= 0 && gops_flag(mean));
    if (N == 0 || C == 0) return 0;
    GOPS_REQUIRE(x && rowptr && out);
    hipLaunchKernelGGL(gops::k_segment_sum, dim3(gops_blocks(N * C)), dim3(256), 0, (hipStream_t)stream, x, rowptr, out, N, C, mean);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_segment_bwd(const float* dout, const int64_t* row, const int32_t* rowptr, float* dx, int64_t E, int32_t C, int32_t mean, void* stream) {
    GOPS_REQUIRE(E >= 0 && C >= 0 && gops_flag(mean));
    if (E == 0 || C == 0) return 0;
    GOPS_REQUIRE(dout && row && rowptr && dx);
    hipLaunchKernelGGL(gops::k_segment_bwd, dim3(gops_blocks(E * C)), dim3(256), 0, (hipStream_t)stream, dout, row, rowptr, dx, E, C, mean);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_scatter_add(const float* dy, const int64_t* idx, float* out, int64_t E, int32_t C, void* stream) {
    GOPS_REQUIRE(E >= 0 && C >= 0);
    if (E == 0 || C == 0) return 0;
    GOPS_REQUIRE(dy && idx && out);
    hipLaunchKernelGGL(gops::k_scatter_add, dim3(gops_blocks(E * C)), dim3(256), 0, (hipStream_t)stream, dy, idx, out, E, C);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_localize(const float* x, const int64_t* row, const int64_t* col, float* F, int64_t E, int32_t norm_x_diff, void* stream) {
    GOPS_REQUIRE(E >= 0 && gops_flag(norm_x_diff));
    if (E == 0) return 0;
    GOPS_REQUIRE(x && row && col && F);
    hipLaunchKernelGGL(gops::k_localize, dim3(gops_blocks(E)), dim3(256), 0, (hipStream_t)stream, x, row, col, F, E, norm_x_diff);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_edge_features(const float* x, const int64_t* row, const int64_t* col, float* e_out, float* xi_out, int64_t E, void* stream) {
    GOPS_REQUIRE(E >= 0);
    if (E == 0) return 0;
    GOPS_REQUIRE(x && row && col && e_out && xi_out);
    hipLaunchKernelGGL(gops::k_edge_features, dim3(gops_blocks(E)), dim3(256), 0, (hipStream_t)stream, x, row, col, e_out, xi_out, E);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_orientations(const float* x, float* out, int64_t N, void* stream) {
    GOPS_REQUIRE(N >= 0);
    if (N == 0) return 0;
    GOPS_REQUIRE(x && out);
    hipLaunchKernelGGL(gops::k_orientations, dim3(gops_blocks(N)), dim3(256), 0, (hipStream_t)stream, x, out, N);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_centralize(const float* x, const int64_t* batch_index, const uint8_t* mask, float* out, int64_t N, int32_t D, void* stream) {
    GOPS_REQUIRE(N >= 0 && D >= 0);
    if (N == 0 || D == 0) return 0;
    GOPS_REQUIRE(x && batch_index && out);                     // mask may be null: every node counts
    hipLaunchKernelGGL(gops::k_centralize, dim3(gops_blocks(N)), dim3(256), 0, (hipStream_t)stream, x, batch_index, mask, out, N, D);
    return GOPS_LAUNCH_OK();
}
int gcdm_op_fc_edges(const int32_t* noff, const int64_t* eoff, int32_t B, int64_t* row, int64_t* col, int64_t E, void* stream) {
    GOPS_REQUIRE(B >= 0 && E >= 0);
    if (E == 0) return 0;
    GOPS_REQUIRE(B >= 1 && noff && eoff && row && col);
    hipLaunchKernelGGL(gops::k_fc_edges, dim3(gops_blocks(E)), dim3(256), 0, (hipStream_t)stream, noff, eoff, B, row, col, E);
    return GOPS_LAUNCH_OK();
}

}  // extern "C"
