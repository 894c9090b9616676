// gcdm_ops.tile.hip.h -- the shared floor of libgcdm_ops.so's GEMM kernels: ONE 64 x 64 x 16 fp32 tile body on v_mfma_f32_32x32x2_f32 (exact
// fp32 products, fp32 accumulate), the accumulator-to-row mapping of its result, the plain GEMM (k_gemm + gops::gemm), the grouped split-K GEMM
// every training operator computes its weight gradients with (WgTable, k_wgrad_grouped, wgrad_launch), and the small helpers the operators
// share (the 256-byte arena of the workspace layouts, the activations).  Included first by gcdm_ops.hip; everything in namespace gops.
//
// A kernel on the tile body is index setup, one tile_mma() call, its own epilogue.  The MFMAs of a tile run over k in ascending order, two k
// per instruction, whoever calls: that fixed order is what makes every operator's result independent of the row count and the same bits from
// run to run.  A second body with the same contract, tile_mma_bf16x6 (six v_mfma_f32_32x32x16_bf16 per 16-deep block on three bf16 images of
// every fp32 element), serves the opt-in bf16x6 matrix mode (include/gcdm_matrix_mode.h); the kernels take the mode as a template parameter
// and reach either body through tile_body<MODE>, the fp32 instantiation being the kernel as it was before the mode existed.
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
// (start4 / get4: the same operand for the bf16x6 body below, which takes 4 consecutive k of one row per thread and K step.)
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
// x[i] = element k + i of one row or column of a strided operand, p at its element k, k stride sk: 0 and not dereferenced where the row
// is invalid or k + i >= k_end.  A k-contiguous quadruple that lies inside the range is ONE 16-byte load, which needs dword alignment
// only, so odd row strides (K = 273) and bases off by one float take it too.
__device__ __forceinline__ void strided_load4(const float* p, int64_t sk, bool valid, int64_t k, int64_t k_end, float (&x)[4]) {
    if (valid && k + 3 < k_end) {
        if (sk == 1) {
            const f32x4u v = *reinterpret_cast<const f32x4u*>(p);
            x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; x[3] = v[3];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = p[i * sk];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = (valid && k + i < k_end) ? p[i * sk] : 0.f;
    }
}
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
    __device__ __forceinline__ void start4(bool valid, int64_t row, int64_t k) { start(0, valid, row, k); }
    __device__ __forceinline__ void get4(bool valid, int64_t, int64_t k, int64_t k_end, float (&x)[4]) {
        strided_load4(p[0], sak, valid, k, k_end, x);
        p[0] += GK * sak;
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
    __device__ __forceinline__ void start4(bool, int64_t, int64_t) {}
    __device__ __forceinline__ void get4(bool valid, int64_t row, int64_t k, int64_t k_end, float (&x)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = (valid && k + i < k_end) ? f(row, k + i) : 0.f;
    }
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

// ---- the same tile in bf16x6 mode (include/gcdm_matrix_mode.h): six v_mfma_f32_32x32x16_bf16 per 16-deep block ----------------------------------
// Every fp32 element is the exact sum of three bf16 images, x = x0 + x1 + x2 (x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1), round to
// nearest even: 3 x 8 significand bits, both subtractions exact), and
//     x y ~ x0 y0 + (x0 y1 + x1 y0) + (x1 y1 + x0 y2 + x2 y0)                       (dropped: x1 y2, x2 y1, x2 y2 <= 2^-24 relative)
// Products of bf16 values are exact in fp32 and the MFMA accumulates in fp32, in three accumulators (one per bracket) that are merged once at
// the end, smallest first.  bf16 has fp32's exponent range, so there is no prescale, no range guard and no flag: an operand that is not
// finite or is >= 2^127 in magnitude becomes NaN in all three images (below 2^127 no image can round up to Inf) and so does every output
// element that depends on it.
// The split happens once per workgroup where the element is stashed: a thread takes 4 consecutive k of one row (A) / column (B) per K step,
// splits them and writes 8 bytes per image; the images are k-contiguous in LDS, [image][k / 8][row][k % 8] (16-byte chunks: the ds_read_b128 of
// a wave's 32 rows x 2 k-halves falls on 16 distinct chunks per 16-lane group), so an MFMA operand is one ds_read_b128 per image and the
// conversion results reach the MFMAs through LDS only.  Same contract as tile_mma otherwise: k ascending in steps of GK, rows >= M, columns
// >= N and k outside [k_begin, k_end) read as 0 and are never dereferenced, a row's bits depend on that row alone, f32x16 result in
// tile_row()'s layout.
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
struct alignas(16) X6Tile {
    u32x2 c[3][GK / 8][GM][2];             // [image][k / 8][row][(k / 4) & 1]: 4 bf16 each
};
__device__ __forceinline__ void x6_split4(const float (&x)[4], u32x2 (&img)[3]) {
    bf16x4 b0, b1, b2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float v = __builtin_fabsf(x[i]) < 0x1p127f ? x[i] : __builtin_nanf("");
        b0[i] = (__bf16)v;
        const float r1 = v - (float)b0[i];
        b1[i] = (__bf16)r1;
        b2[i] = (__bf16)(r1 - (float)b1[i]);
    }
    img[0] = __builtin_bit_cast(u32x2, b0); img[1] = __builtin_bit_cast(u32x2, b1); img[2] = __builtin_bit_cast(u32x2, b2);
}
template <class ASrc>
__device__ __forceinline__ f32x16 tile_mma_bf16x6(ASrc a, const float* __restrict__ B, int64_t sbk, int64_t sbn, int64_t m0, int n0, int64_t M,
                                                  int N, int64_t k_begin, int64_t k_end, X6Tile* As, X6Tile* Bs) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    f32x16 a00 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, a01 = a00, a11 = a00;
    const bool a_kfast = a.kfast(), b_kfast = sbk == 1;
    // this thread's quadruple of A and of B in a K step: k-fast operands 4 threads per row, the others 64 rows per wave (coalesced either way)
    const int ar = a_kfast ? tid >> 2 : tid & 63, ac = a_kfast ? tid & 3 : tid >> 6;
    const int br = b_kfast ? tid >> 2 : tid & 63, bc = b_kfast ? tid & 3 : tid >> 6;
    const bool va = m0 + ar < M, vb = n0 + br < N;
    a.start4(va, m0 + ar, k_begin + 4 * ac);
    const float* pb = B + (k_begin + 4 * bc) * sbk + (vb ? (int64_t)(n0 + br) * sbn : 0);
    const int64_t db_ = GK * sbk;
    float ra[4], rb[4];
    auto fetch = [&](int64_t k0) {
        a.get4(va, m0 + ar, k0 + 4 * ac, k_end, ra);
        strided_load4(pb, sbk, vb, k0 + 4 * bc, k_end, rb);
        pb += db_;
    };
    auto stash = [&](int buf) {
        u32x2 ia[3], ib[3];
        x6_split4(ra, ia);
        x6_split4(rb, ib);
#pragma unroll
        for (int i = 0; i < 3; ++i) { As[buf].c[i][ac >> 1][ar][ac & 1] = ia[i]; Bs[buf].c[i][bc >> 1][br][bc & 1] = ib[i]; }
    };
    fetch(k_begin);
    stash(0);
    __syncthreads();
    int buf = 0;
    for (int64_t k0 = k_begin; k0 < k_end; k0 += GK) {
        const bool more = k0 + GK < k_end;
        if (more) fetch(k0 + GK);                     // in flight during the MFMAs below
        bf16x8 x[3], y[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            x[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(&As[buf].c[i][lane >> 5][wm * 32 + (lane & 31)][0]));
            y[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(&Bs[buf].c[i][lane >> 5][wn * 32 + (lane & 31)][0]));
        }
        a00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[0], y[0], a00, 0, 0, 0);
        a01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[0], y[1], a01, 0, 0, 0);
        a11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[1], y[1], a11, 0, 0, 0);
        a01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[1], y[0], a01, 0, 0, 0);
        a11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[0], y[2], a11, 0, 0, 0);
        a11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[2], y[0], a11, 0, 0, 0);
        if (more) stash(buf ^ 1);                     // the other half: nobody reads it before the barrier
        __syncthreads();
        buf ^= 1;
    }
    return a00 + (a01 + a11);
}

// ---- the matrix mode of a kernel: which body its tiles run on, and the LDS tile that body stages through -------------------------------------
enum { MM_F32 = 0, MM_BF16X6 = 1 };        // GCDM_OPS_MATRIX_F32 / GCDM_OPS_MATRIX_BF16X6
template <int MODE> struct TileLds { typedef float type[GK][GM + 1]; };
template <> struct TileLds<MM_BF16X6> { typedef X6Tile type; };
template <int MODE, class ASrc, class L>
__device__ __forceinline__ f32x16 tile_body(ASrc a, const float* __restrict__ B, int64_t sbk, int64_t sbn, int64_t m0, int n0, int64_t M, int N,
                                            int64_t k_begin, int64_t k_end, L* As, L* Bs) {
    if constexpr (MODE == MM_BF16X6) return tile_mma_bf16x6(a, B, sbk, sbn, m0, n0, M, N, k_begin, k_end, As, Bs);
    else return tile_mma(a, B, sbk, sbn, m0, n0, M, N, k_begin, k_end, As, Bs);
}
// a launch in the mode the C entry read: the fp32 instantiation is the kernel as it always was
#define GOPS_LAUNCH_MODE(mode, K, ...) \
    do { if ((mode) == gops::MM_BF16X6) hipLaunchKernelGGL((K<gops::MM_BF16X6>), __VA_ARGS__); else hipLaunchKernelGGL((K<gops::MM_F32>), __VA_ARGS__); } while (0)
// the same for a kernel whose mode is its second template parameter, behind T1
#define GOPS_LAUNCH_MODE2(mode, K, T1, ...) \
    do { if ((mode) == gops::MM_BF16X6) hipLaunchKernelGGL((K<T1, gops::MM_BF16X6>), __VA_ARGS__); else hipLaunchKernelGGL((K<T1, gops::MM_F32>), __VA_ARGS__); } while (0)

// ---- C[M,N] = A[M,K] . B[K,N] (+ bias[N]) ------------------------------------------------------------------------------------------------------
// General strides, so one kernel serves y = x W^T (A = x, B = W^T), dx = dy W (A = dy, B = W) and dW = dy^T x (A = dy^T, B = x).
// grid.z = split-K slices writing C + z * M * N (reduced in fixed order by k_reduce_slices: deterministic).
template <int MODE>
__global__ __launch_bounds__(256) void k_gemm(const float* __restrict__ A, int64_t sam, int64_t sak, const float* __restrict__ B, int64_t sbk,
                                              int64_t sbn, float* __restrict__ C, const float* __restrict__ bias, int64_t M, int N, int64_t K,
                                              int64_t kslice) {
    __shared__ typename TileLds<MODE>::type As[2], Bs[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int64_t m0 = (int64_t)blockIdx.x * GM;
    const int n0 = blockIdx.y * GN;
    const int64_t k_begin = (int64_t)blockIdx.z * kslice, k_end = k_begin + kslice < K ? k_begin + kslice : K;
    const f32x16 acc = tile_body<MODE>(StridedA{A, sam, sak}, B, sbk, sbn, m0, n0, M, N, k_begin, k_end, As, Bs);
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
                        int64_t K, hipStream_t st, int slices = 1, int mode = MM_F32) {
    const int64_t kslice = ((K + slices - 1) / slices + GK - 1) / GK * GK;
    const dim3 grid((unsigned)((M + GM - 1) / GM), (unsigned)((N + GN - 1) / GN), (unsigned)slices);
    GOPS_LAUNCH_MODE(mode, k_gemm, grid, dim3(256), 0, st, A, sam, sak, B, sbk, sbn, C, bias, M, N, K, kslice > 0 ? kslice : GK);
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

template <int MODE>
__global__ __launch_bounds__(256) void k_wgrad_grouped(WgTable T, float* __restrict__ part) {
    __shared__ typename TileLds<MODE>::type As[2], Bs[2];
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
    const f32x16 acc = tile_body<MODE>(StridedA{D.A, D.sam, D.sak}, D.B, D.sbk, D.sbn, m0, n0, D.M, D.N, k_begin, k_end, As, Bs);
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
static inline void wgrad_launch(const WgTable& T, float* part, float* dweights, hipStream_t st, int mode = MM_F32) {
    GOPS_LAUNCH_MODE(mode, k_wgrad_grouped, dim3((unsigned)T.tiles, 1, WG_SLICES), dim3(256), 0, st, T, part);
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
