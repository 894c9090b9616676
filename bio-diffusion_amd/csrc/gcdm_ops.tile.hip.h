// gcdm_ops.tile.hip.h -- the shared floor of libgcdm_ops.so's GEMM kernels: ONE 64 x 64 x 16 fp32 tile body on v_mfma_f32_32x32x2_f32 (exact
// fp32 products, fp32 accumulate), the accumulator-to-row mapping of its result, the plain GEMM (k_gemm + gops::gemm), the grouped split-K GEMM
// every training operator computes its weight gradients with (WgTable, k_wgrad_grouped, wgrad_launch), and the small helpers the operators
// share (the 256-byte arena of the workspace layouts, the activations).  Included first by gcdm_ops.hip; everything in namespace gops.
//
// A kernel on the tile body is index setup, one tile_mma() call, its own epilogue.  The MFMAs of a tile run over k in ascending order, two k
// per instruction, whoever calls: that fixed order is what makes every operator's result independent of the row count and the same bits from
// run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gops {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// 64 x 64 tile per 256-thread workgroup (4 waves, 32 x 32 each), K in steps of 16 through LDS
constexpr int GM = 64, GN = 64, GK = 16;

// ---- the A operand of a tile: where element i (of 4 per thread and K step) comes from ---------------------------------------------------------
// Strided: A[row * sam + k * sak].  The element address is set up once and advanced by GK * sak per K step (round 3: a pointer += stride
// instead of two 64-bit multiplies per element and step); the thread-to-element coordinates follow the fast axis (coalesced either way).
struct StridedA {
    const float* A;
    int64_t sam, sak;
    const float* p[4];
    __device__ __forceinline__ bool kfast() const { return sak == 1; }
    __device__ __forceinline__ void start(int i, bool valid, int64_t row, int64_t k) { p[i] = A + (valid ? row * sam : 0) + k * sak; }
    __device__ __forceinline__ float get(int i, bool ok, int64_t, int64_t) {
        const float x = ok ? *p[i] : 0.f;
        p[i] += GK * sak;
        return x;
    }
};
// Computed: f(row, k), addressed k-fast.  f is called exactly once per element of a K step, by exactly one thread, and never outside
// [0, M) x [k_begin, k_end) -- it may write what it computed as a side effect.
template <class F>
struct FunctorA {
    F f;
    __device__ __forceinline__ bool kfast() const { return true; }
    __device__ __forceinline__ void start(int, bool, int64_t, int64_t) {}
    __device__ __forceinline__ float get(int, bool ok, int64_t row, int64_t k) { return ok ? f(row, k) : 0.f; }
};

// ---- one 64 x 64 tile of A[M,K] . B[K,N] over k in [k_begin, k_end) -----------------------------------------------------------------------------
// B is strided (B[k * sbk + n * sbn]).  The next K step's 4 + 4 elements are requested into registers before the current step's MFMAs and
// stored into the OTHER half of the double-buffered LDS tile behind them: one barrier per step, global latency under the MFMAs.  Rows >= M,
// columns >= N and k >= k_end read as 0 and are never dereferenced, so an empty K range touches no memory and returns zeros.  All 256 threads
// call it together; on return nobody reads As / Bs any more.
template <class ASrc>
__device__ __forceinline__ f32x16 tile_mma(ASrc a, const float* __restrict__ B, int64_t sbk, int64_t sbn, int64_t m0, int n0, int64_t M, int N,
                                           int64_t k_begin, int64_t k_end, float (*As)[GK][GM + 1], float (*Bs)[GK][GN + 1]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bool a_kfast = a.kfast(), b_nfast = sbn == 1;
    // this thread's 4 + 4 elements of a K step: tile coordinates, running global pointers, row / column validity
    int am[4], ak[4], bn[4], bk[4];
    const float* pb[4];
    bool va[4], vb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i;
        am[i] = a_kfast ? idx / GK : idx % GM; ak[i] = a_kfast ? idx % GK : idx / GM;
        bn[i] = b_nfast ? idx % GN : idx / GK; bk[i] = b_nfast ? idx / GN : idx % GK;
        va[i] = m0 + am[i] < M; vb[i] = n0 + bn[i] < N;
        a.start(i, va[i], m0 + am[i], k_begin + ak[i]);
        pb[i] = B + (k_begin + bk[i]) * sbk + (vb[i] ? (int64_t)(n0 + bn[i]) * sbn : 0);
    }
    const int64_t db_ = GK * sbk;
    float ra[4], rb[4];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[i] = a.get(i, va[i] && k0 + ak[i] < k_end, m0 + am[i], k0 + ak[i]);
            rb[i] = (vb[i] && k0 + bk[i] < k_end) ? *pb[i] : 0.f;
            pb[i] += db_;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { As[buf][ak[i]][am[i]] = ra[i]; Bs[buf][bk[i]][bn[i]] = rb[i]; }
    };
    fetch(k_begin);
    stash(0);
    __syncthreads();
    int buf = 0;
    for (int64_t k0 = k_begin; k0 < k_end; k0 += GK) {
        const bool more = k0 + GK < k_end;
        if (more) fetch(k0 + GK);                     // in flight during the MFMAs below
#pragma unroll
        for (int kk = 0; kk < GK; kk += 2) {
            const float x = As[buf][kk + (lane >> 5)][wm * 32 + (lane & 31)];
            const float y = Bs[buf][kk + (lane >> 5)][wn * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, acc, 0, 0, 0);
        }
        if (more) stash(buf ^ 1);                     // the other half: nobody reads it before the barrier
        __syncthreads();
        buf ^= 1;
    }
    return acc;
}
// element r of a lane's accumulator is row tile_row(wm, lane, r) of the tile (wm = wave & 1), column (wave >> 1) * 32 + (lane & 31)
__device__ __forceinline__ int tile_row(int wm, int lane, int r) { return wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// ---- C[M,N] = A[M,K] . B[K,N] (+ bias[N]) ------------------------------------------------------------------------------------------------------
// General strides, so one kernel serves y = x W^T (A = x, B = W^T), dx = dy W (A = dy, B = W) and dW = dy^T x (A = dy^T, B = x).
// grid.z = split-K slices writing C + z * M * N (reduced in fixed order by k_reduce_slices: deterministic).
__global__ __launch_bounds__(256) void k_gemm(const float* __restrict__ A, int64_t sam, int64_t sak, const float* __restrict__ B, int64_t sbk,
                                              int64_t sbn, float* __restrict__ C, const float* __restrict__ bias, int64_t M, int N, int64_t K,
                                              int64_t kslice) {
    __shared__ float As[2][GK][GM + 1];
    __shared__ float Bs[2][GK][GN + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int64_t m0 = (int64_t)blockIdx.x * GM;
    const int n0 = blockIdx.y * GN;
    const int64_t k_begin = (int64_t)blockIdx.z * kslice, k_end = k_begin + kslice < K ? k_begin + kslice : K;
    const f32x16 acc = tile_mma(StridedA{A, sam, sak}, B, sbk, sbn, m0, n0, M, N, k_begin, k_end, As, Bs);
    float* Cz = C + (int64_t)blockIdx.z * M * N;
    const int col = n0 + wn * 32 + (lane & 31);
    if (col < N) {
        const float bv = (bias && blockIdx.z == 0) ? bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = m0 + tile_row(wm, lane, r);
            if (row < M) Cz[row * N + col] = acc[r] + bv;
        }
    }
}
// the launch: `slices` K slices of a multiple of GK each (trailing ones may be empty: they write 0); 1 slice is the finished product
static inline void gemm(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn, float* C, const float* bias, int64_t M, int N,
                        int64_t K, hipStream_t st, int slices = 1) {
    const int64_t kslice = ((K + slices - 1) / slices + GK - 1) / GK * GK;
    const dim3 grid((unsigned)((M + GM - 1) / GM), (unsigned)((N + GN - 1) / GN), (unsigned)slices);
    hipLaunchKernelGGL(k_gemm, grid, dim3(256), 0, st, A, sam, sak, B, sbk, sbn, C, bias, M, N, K, kslice > 0 ? kslice : GK);
}

__global__ void k_reduce_slices(const float* __restrict__ part, float* __restrict__ out, int64_t n, int slices) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int z = 0; z < slices; ++z) s += part[(int64_t)z * n + i];
    out[i] = s;
}

// ---- grouped split-K GEMM for every weight gradient of an operator: C_g = A_g . B_g into part[z] + off_g (row stride ldc_g) ---------------------
// One workgroup per (64 x 64 tile of some group, K slice z); slice z of every group covers the same fraction of that group's K, the slices are
// added in slice order by k_reduce_slices (deterministic).  A bias gradient is a group whose B is a single 1.0f with strides 0.
constexpr int MAXG = 36;
constexpr int WG_SLICES = 16;            // fixed: the reduction order never changes
struct WgDesc {
    const float* A; const float* B;
    int64_t sam, sak, sbk, sbn, K, off;
    int M, N, ldc, tile0;
};
struct WgTable {
    WgDesc g[MAXG];
    int n = 0, tiles = 0;
    int64_t total = 0;                   // floats of all gradients together = the stride between two slices of `part`
    void add(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbk, int64_t sbn, int M, int N, int64_t K, int64_t off, int ldc) {
        WgDesc& d = g[n++];
        d.A = A; d.B = B; d.sam = sam; d.sak = sak; d.sbk = sbk; d.sbn = sbn; d.K = K; d.off = off; d.M = M; d.N = N; d.ldc = ldc; d.tile0 = tiles;
        tiles += ((M + GM - 1) / GM) * ((N + GN - 1) / GN);
    }
};
// off[i] = where gradient i starts among the n gradients of sizes sz[]; returns their total
static inline int64_t wgrad_offsets(const int64_t* sz, int n, int64_t* off) {
    int64_t t = 0;
    for (int i = 0; i < n; ++i) { off[i] = t; t += sz[i]; }
    return t;
}

__global__ __launch_bounds__(256) void k_wgrad_grouped(WgTable T, float* __restrict__ part) {
    __shared__ float As[2][GK][GM + 1];
    __shared__ float Bs[2][GK][GN + 1];
    int gi = 0;
    while (gi + 1 < T.n && T.g[gi + 1].tile0 <= (int)blockIdx.x) ++gi;
    const WgDesc& D = T.g[gi];
    const int t = blockIdx.x - D.tile0, tn_count = (D.N + GN - 1) / GN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int64_t m0 = (int64_t)(t / tn_count) * GM;
    const int n0 = (t % tn_count) * GN;
    const int64_t kslice = ((D.K + WG_SLICES - 1) / WG_SLICES + GK - 1) / GK * GK;
    const int64_t k_begin = (int64_t)blockIdx.z * kslice, k_end = k_begin + kslice < D.K ? k_begin + kslice : D.K;
    const f32x16 acc = tile_mma(StridedA{D.A, D.sam, D.sak}, D.B, D.sbk, D.sbn, m0, n0, D.M, D.N, k_begin, k_end, As, Bs);
    float* Cz = part + (int64_t)blockIdx.z * T.total + D.off;
    const int col = n0 + wn * 32 + (lane & 31);
    if (col < D.N) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = m0 + tile_row(wm, lane, r);
            if (row < D.M) Cz[row * D.ldc + col] = acc[r];
        }
    }
}
// dweights[T.total] = the groups of T, through part[WG_SLICES][T.total]
static inline void wgrad_launch(const WgTable& T, float* part, float* dweights, hipStream_t st) {
    hipLaunchKernelGGL(k_wgrad_grouped, dim3((unsigned)T.tiles, 1, WG_SLICES), dim3(256), 0, st, T, part);
    hipLaunchKernelGGL(k_reduce_slices, dim3((unsigned)((T.total + 255) / 256)), dim3(256), 0, st, (const float*)part, dweights, T.total, (int)WG_SLICES);
}

// ---- workspace layouts: offsets in floats, every buffer 256-byte aligned ------------------------------------------------------------------------
inline int64_t a4(int64_t n) { return (n + 63) & ~(int64_t)63; }
struct Arena {
    int64_t o = 0;
    int64_t take(int64_t n) { const int64_t r = o; o += a4(n); return r; }
};

// ---- element-wise nonlinearities (get_nonlinearity, components/__init__.py: relu / leakyrelu / selu / silu; + sigmoid) --------------------
enum { ACT_NONE = 0, ACT_SILU = 1, ACT_RELU = 2, ACT_SIGMOID = 3, ACT_LEAKYRELU = 4, ACT_SELU = 5 };
// expf / expm1f, not __expf: the fast exp2-based form loses relative accuracy at large negative x (SiLU, sigmoid) and `__expf(x) - 1`
// cancels completely near 0- (SELU); the kernels are memory-bound, the accurate forms cost nothing measurable.  ReLU keeps NaN (x < 0 is
// false for it), as torch.relu does.
__device__ __forceinline__ float sigm_f(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float act_f(int kind, float x) {
    switch (kind) {
        case ACT_SILU: return x / (1.f + expf(-x));
        case ACT_RELU: return x < 0.f ? 0.f : x;
        case ACT_SIGMOID: return sigm_f(x);
        case ACT_LEAKYRELU: return x > 0.f ? x : 0.01f * x;
        case ACT_SELU: return 1.0507009873554804934193349852946f * (x > 0.f ? x : 1.6732632423543772848170429916717f * expm1f(x));
        default: return x;
    }
}
__device__ __forceinline__ float act_df(int kind, float x) {
    switch (kind) {
        case ACT_SILU: { const float s = sigm_f(x); return s * (1.f + x * (1.f - s)); }
        case ACT_RELU: return x > 0.f ? 1.f : 0.f;
        case ACT_SIGMOID: { const float s = sigm_f(x); return s * (1.f - s); }
        case ACT_LEAKYRELU: return x > 0.f ? 1.f : 0.01f;
        case ACT_SELU: return 1.0507009873554804934193349852946f * (x > 0.f ? 1.f : 1.6732632423543772848170429916717f * expf(x));
        default: return 1.f;
    }
}

}  // namespace gops
