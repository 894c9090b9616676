// gcdm_ops.bucket.hip.h -- the flat gradient bucket of data-parallel and accumulated training steps.  C ABI: include/gcdm_grad_bucket.h.
// The bucket is laid out like a state quarter of the fused training update (gcdm_ops.optim.hip.h, whose workspace layout gopt::layout this
// file reads): tensor t at otab[t], cut into the chunks of ctab; after the `total` values a presence tail of one float per tensor.
//
//   k_bucket_pack   blocks 0 .. SPLIT C - 1, SPLIT per chunk (a chunk of the optimiser's table has up to 16384 values; a quarter of it per
//                   workgroup keeps four 128-bit loads per lane in flight and gives the QM9 table 3000 workgroups instead of 757):
//                   bucket = fl32(s g) (first) or fl32(bucket + fl32(s g)), an absent tensor +0.0 (first) or untouched; the blocks after
//                   them, one thread per tensor: the presence tail and, on a first pass, the padding behind the tensor.
//                   Streaming, 128-bit on the bucket side; a gradient at an odd alignment is read in dwords into the same lanes, so the
//                   bits do not depend on it.  No atomics, nothing is summed across lanes.
//   k_bucket_check  one workgroup: a presence other than 0 or `world` raises GCDM_GRAD_BUCKET_FLAG_MISMATCH and poisons the first value of
//                   every tensor with a NaN, which the next gcdm_optim_step turns into a skipped step.
#pragma once

namespace gbkt {

constexpr int THREADS = 256;
constexpr int SPLIT = 4;          // workgroups per chunk
constexpr int TILE = 1024;        // offsets in LDS at a time (8 KB)

struct Args {
    const int64_t* gptr;     // the caller's gradient table of this pass (not section 2 of the workspace)
    const int64_t* otab;
    const int64_t* ntab;
    const int64_t* ctab;
    float* bucket;
    int64_t total, T, C, tail;          // tail = T rounded up to 64
    float s;
    int first;
};

inline int64_t tail_floats(int64_t T) { return (T + 63) & ~(int64_t)63; }

__device__ inline float4 scale4(float s, float4 x) {
#pragma clang fp contract(off)
    return float4{s * x.x, s * x.y, s * x.z, s * x.w};
}
__device__ inline float4 add4(float4 y, float4 x) {
#pragma clang fp contract(off)
    return float4{y.x + x.x, y.y + x.y, y.z + x.z, y.w + x.w};
}

// the float4 body of one chunk; ALIGNED: the gradient can be read 128 bits at a time
template <bool ALIGNED, bool FIRST>
__device__ inline void pack4(const float* __restrict__ g, float* __restrict__ d, int64_t n4, float s) {
#pragma unroll 4
    for (int64_t i = threadIdx.x; i < n4; i += THREADS) {
        float4 x;
        if (ALIGNED) x = ((const float4*)g)[i];
        else x = float4{g[4 * i], g[4 * i + 1], g[4 * i + 2], g[4 * i + 3]};
        x = scale4(s, x);
        if (!FIRST) x = add4(((const float4*)d)[i], x);
        ((float4*)d)[i] = x;
    }
}

__global__ void __launch_bounds__(THREADS) k_bucket_pack(Args a) {
#pragma clang fp contract(off)
    const int64_t b = blockIdx.x;
    if (b >= SPLIT * a.C) {
        // one thread per tensor: presence, and on a first pass the padding between this tensor's end and the next tensor's offset (in
        // (offset, index) order; `total` after the last one) and the padding of the tail.  The offsets pass through LDS a tile at a time:
        // every thread looks at every offset
        __shared__ int64_t so[TILE];
        const int64_t t = (b - SPLIT * a.C) * THREADS + threadIdx.x;
        float* pres = a.bucket + a.total;
        const bool live = t < a.T;
        const float here = live && a.gptr[t] != 0 ? 1.f : 0.f;
        if (!a.first) {
            if (live) pres[t] = fmaxf(pres[t], here);
            return;
        }
        if (t < a.tail) pres[t] = here;
        const int64_t o = live ? a.otab[t] : 0, end = live ? o + a.ntab[t] : 0;
        int64_t next = a.total, lowest = a.total;
        for (int64_t base = 0; base < a.T; base += TILE) {
            const int64_t n = a.T - base < TILE ? a.T - base : TILE;
            __syncthreads();
            for (int64_t j = threadIdx.x; j < n; j += THREADS) so[j] = a.otab[base + j];
            __syncthreads();
            for (int64_t j = 0; j < n; ++j) {
                const int64_t ou = so[j], u = base + j;
                if (ou >= end && (ou > o || u > t) && ou < next) next = ou;
                if (ou < lowest) lowest = ou;
            }
        }
        if (!live) return;
        for (int64_t i = end; i < next; ++i) a.bucket[i] = 0.f;
        if (t == 0)
            for (int64_t i = 0; i < lowest; ++i) a.bucket[i] = 0.f;          // before the first tensor
        return;
    }
    const int64_t c = b / SPLIT, part = b % SPLIT;
    const int64_t t = a.ctab[3 * c], clen = a.ctab[3 * c + 2];
    const int64_t per = (clen + 4 * SPLIT - 1) / (4 * SPLIT) * 4;          // values per workgroup, a multiple of 4: the last one takes the tail
    const int64_t lo = part * per, len = (lo + per < clen ? lo + per : clen) - lo;
    const float* g = (const float*)a.gptr[t];
    if (len <= 0 || (g == nullptr && !a.first)) return;
    const int64_t start = a.ctab[3 * c + 1] + lo;
    float* d = a.bucket + a.otab[t] + start;
    const int64_t n4 = gopt::aligned16(d) ? len >> 2 : 0;          // offsets and chunk starts are multiples of 4 floats, the bucket is aligned
    if (g == nullptr) {
        for (int64_t i = threadIdx.x; i < n4; i += THREADS) ((float4*)d)[i] = float4{0.f, 0.f, 0.f, 0.f};
        for (int64_t i = (n4 << 2) + threadIdx.x; i < len; i += THREADS) d[i] = 0.f;
        return;
    }
    g += start;
    if (gopt::aligned16(g)) {
        if (a.first) pack4<true, true>(g, d, n4, a.s);
        else pack4<true, false>(g, d, n4, a.s);
    } else {
        if (a.first) pack4<false, true>(g, d, n4, a.s);
        else pack4<false, false>(g, d, n4, a.s);
    }
    for (int64_t i = (n4 << 2) + threadIdx.x; i < len; i += THREADS) {
        float x = a.s * g[i];
        if (!a.first) x = d[i] + x;
        d[i] = x;
    }
}

__global__ void __launch_bounds__(THREADS) k_bucket_check(const int64_t* otab, const int64_t* ntab, gopt::Scal* scal, float* bucket, int64_t total,
                                                           int64_t T, float world) {
    const float* pres = bucket + total;
    int bad = 0;
    for (int64_t t = threadIdx.x; t < T; t += THREADS) {
        const float p = pres[t];
        bad |= !(p == 0.f || p == world);          // a NaN tail is a mismatch too
    }
    if (!__syncthreads_or(bad)) return;
    if (threadIdx.x == 0) scal->flags |= GCDM_GRAD_BUCKET_FLAG_MISMATCH;
    for (int64_t t = threadIdx.x; t < T; t += THREADS)
        if (ntab[t] > 0) bucket[otab[t]] = __builtin_nanf("");
}

}  // namespace gbkt

extern "C" {

int64_t gcdm_grad_bucket_floats(int64_t total, int64_t num_tensors) {
    GOPS_REQUIRE(total >= 0 && num_tensors >= 0 && total % 4 == 0);
    return total + gbkt::tail_floats(num_tensors);
}

int gcdm_grad_bucket_pack(const void* optim_workspace, const int64_t* grad_ptrs, float* bucket, int64_t total, int64_t num_tensors,
                          int64_t num_chunks, int32_t queue_len, double scale, int32_t first, void* stream) {
    GOPS_REQUIRE(total >= 0 && total % 4 == 0 && num_tensors >= 0 && num_chunks >= 0 && queue_len >= 1 && queue_len <= GCDM_OPTIM_QUEUE_MAX);
    GOPS_REQUIRE(gops_flag(first) && scale - scale == 0.0);          // NaN and +-Inf fail x - x == 0
    if (num_tensors == 0 || num_chunks == 0) return 0;
    GOPS_REQUIRE(optim_workspace && grad_ptrs && bucket && total > 0);
    const gopt::Layout L = gopt::layout(num_tensors, num_chunks, queue_len);
    const char* w = (const char*)optim_workspace;
    gbkt::Args a{};
    a.gptr = grad_ptrs;
    a.otab = (const int64_t*)(w + L.otab);
    a.ntab = (const int64_t*)(w + L.ntab);
    a.ctab = (const int64_t*)(w + L.ctab);
    a.bucket = bucket;
    a.total = total;
    a.T = num_tensors;
    a.C = num_chunks;
    a.tail = gbkt::tail_floats(num_tensors);
    a.s = (float)scale;
    a.first = first;
    const int64_t blocks = gbkt::SPLIT * num_chunks + (a.tail + gbkt::THREADS - 1) / gbkt::THREADS;
    GOPS_REQUIRE(blocks < ((int64_t)1 << 31));
    hipLaunchKernelGGL(gbkt::k_bucket_pack, dim3((unsigned)blocks), dim3(gbkt::THREADS), 0, (hipStream_t)stream, a);
    return GOPS_LAUNCH_OK();
}

int gcdm_grad_bucket_check(void* optim_workspace, float* bucket, int64_t total, int64_t num_tensors, int64_t num_chunks, int32_t queue_len,
                           int32_t world, void* stream) {
    GOPS_REQUIRE(total >= 0 && total % 4 == 0 && num_tensors >= 0 && num_chunks >= 0 && queue_len >= 1 && queue_len <= GCDM_OPTIM_QUEUE_MAX);
    GOPS_REQUIRE(world >= 1);
    if (num_tensors == 0 || num_chunks == 0) return 0;
    GOPS_REQUIRE(optim_workspace && bucket && total > 0);
    const gopt::Layout L = gopt::layout(num_tensors, num_chunks, queue_len);
    char* w = (char*)optim_workspace;
    hipLaunchKernelGGL(gbkt::k_bucket_check, dim3(1), dim3(gbkt::THREADS), 0, (hipStream_t)stream, (const int64_t*)(w + L.otab),
                       (const int64_t*)(w + L.ntab), (gopt::Scal*)(w + L.scal), bucket, total, num_tensors, (float)world);
    return GOPS_LAUNCH_OK();
}

}  // extern "C"
