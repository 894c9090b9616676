// gcdm_ops.optim.hip.h -- the reference's training update after backward() as three launches: adaptive gradient clipping (the queue of the
// last clipped norms, qm9_mol_gen_ddpm.py configure_gradient_clipping + models/__init__.py Queue / get_grad_norm), AdamW with optional
// AMSGrad (torch.optim.AdamW, single-tensor formulas) and the EMA of the weights (utils/__init__.py EMA.apply_ema).  C ABI:
// include/gcdm_optim.h.  Plain fp32 streaming; no float atomics: every sum runs in a fixed order, so a step gives the same bits every run.
//
// Launches of gcdm_optim_step, all on the caller's stream, no host sync:
//   k_opt_sqnorm    one workgroup per chunk: fp32 sum of g^2 over the chunk -> part[chunk]
//   k_opt_finalize  one workgroup: fp64 sum of the partials in a fixed order -> norm; queue mean / population std -> max_norm -> coef;
//                   push min(norm, max_norm); per tensor with a grad: step += 1, lr / bc1 and sqrt(bc2) in fp64.  A non-finite norm sets
//                   GCDM_OPTIM_FLAG_NONFINITE and `skip`: nothing below (and nothing above but the flag) changes.
//   k_opt_update    one workgroup per chunk: g' = coef g, decoupled weight decay, moments, AMSGrad max, parameter, then the EMA.
#pragma once

namespace gopt {

constexpr int THREADS = 256;

// the byte layout of the workspace (include/gcdm_optim.h): host-written table first, device-owned state after it; every section starts
// on a 256-byte boundary
struct Layout {
    int64_t ptab, gtab, otab, ntab, ctab, host_end, steps, tscal, part, queue, scal, total;
};
inline int64_t a256(int64_t n) { return (n + 255) & ~(int64_t)255; }
inline Layout layout(int64_t T, int64_t C, int32_t Q) {
    Layout L;
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t r = o; o += a256(bytes); return r; };
    L.ptab = take(8 * T);
    L.gtab = take(8 * T);
    L.otab = take(8 * T);
    L.ntab = take(8 * T);
    L.ctab = take(24 * C);
    L.host_end = o;
    L.steps = take(8 * T);
    L.tscal = take(16 * T);
    L.part = take(4 * C);
    L.queue = take(8 * (int64_t)Q);
    L.scal = take(64);
    L.total = o;
    return L;
}

// the scalar block (64 bytes at Layout::scal)
struct Scal {
    double norm;         // the last step's gradient norm (fp32 value widened)
    double max_norm;     // the last step's clip threshold (fp64, as numpy computes it)
    float coef;          // min(1, max_norm / (norm + 1e-6)) in fp32; 1 without clipping
    int32_t flags;       // OR of GCDM_OPTIM_FLAG_* since the caller last cleared it
    int32_t qhead;       // ring slot of the next push
    int32_t qcount;      // values in the queue (<= queue_len)
    int64_t gstep;       // completed (not skipped) steps
    int32_t skip;        // this step was skipped (non-finite norm)
    int32_t ema_now;     // this step applies the EMA
    int32_t pad[4];
};
static_assert(sizeof(Scal) == 64, "scalar block is 64 bytes");

struct Args {
    const int64_t* ptab;
    const int64_t* gtab;
    const int64_t* otab;
    const int64_t* ntab;
    const int64_t* ctab;
    int64_t* steps;
    double* tscal;
    float* part;
    double* queue;
    Scal* scal;
    float* state;        // m | v | vmax | ema, each `total` floats
    int64_t total, T, C;
    double lr, beta1, beta2, eps, wd, ema_decay;
    int64_t ema_every, ema_start;
    int32_t amsgrad, clip, queue_len, ema;
};

__device__ inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// fixed-order block sum (wave64 shuffles, then the four wave totals in order)
template <typename Tv>
__device__ inline Tv block_sum(Tv x, Tv* lds) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[w] = x;
    __syncthreads();
    Tv s = 0;
    if (threadIdx.x == 0)
        for (int i = 0; i < THREADS / 64; ++i) s += lds[i];
    return s;          // valid in thread 0
}

__global__ void __launch_bounds__(THREADS) k_opt_sqnorm(Args a) {
    __shared__ float lds[THREADS / 64];
    const int64_t c = blockIdx.x;
    const int64_t t = a.ctab[3 * c], start = a.ctab[3 * c + 1], len = a.ctab[3 * c + 2];
    const float* g = (const float*)a.gtab[t];
    float acc = 0.f;
    if (g != nullptr) {
        g += start;
        int64_t i0 = 0;
        if (aligned16(g)) {
            const int64_t n4 = len >> 2;
            for (int64_t i = threadIdx.x; i < n4; i += THREADS) {
                const float4 x = ((const float4*)g)[i];
                acc += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
            }
            i0 = n4 << 2;
        }
        for (int64_t i = i0 + threadIdx.x; i < len; i += THREADS) acc += g[i] * g[i];
    }
    const float s = block_sum(acc, lds);
    if (threadIdx.x == 0) a.part[c] = s;
}

__global__ void __launch_bounds__(THREADS) k_opt_finalize(Args a) {
#pragma clang fp contract(off)
    __shared__ double lds[THREADS / 64];
    __shared__ int skip_s;
    double acc = 0.0;
    for (int64_t c = threadIdx.x; c < a.C; c += THREADS) acc += (double)a.part[c];
    const double sq = block_sum(acc, lds);
    Scal* s = a.scal;
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(sq);
        s->norm = (double)norm;
        int skip = !isfinite(norm);
        s->skip = skip;
        s->ema_now = 0;
        if (skip) {
            s->flags |= 1;                                                   // GCDM_OPTIM_FLAG_NONFINITE
        } else {
            float coef = 1.f;
            if (a.clip) {
                const int n = s->qcount;
                double mean = 0.0, var = 0.0;
                for (int i = 0; i < n; ++i) mean += a.queue[i];
                mean /= n;
                for (int i = 0; i < n; ++i) { const double d = a.queue[i] - mean; var += d * d; }
                const double max_norm = 1.5 * mean + 2.0 * sqrt(var / n);
                s->max_norm = max_norm;
                // torch.nn.utils.clip_grad_norm_: max_norm / (total_norm + 1e-6) is Tensor.__rtruediv__ = reciprocal() * max_norm, in fp32
                const float inv = 1.f / (norm + 1e-6f);
                coef = fminf(1.f, inv * (float)max_norm);
                a.queue[s->qhead] = fmin((double)norm, max_norm);
                s->qhead = (s->qhead + 1) % a.queue_len;
                if (s->qcount < a.queue_len) s->qcount += 1;
            }
            s->coef = coef;
            const int64_t k = s->gstep + 1;
            s->gstep = k;
            s->ema_now = a.ema && k >= a.ema_start && k % a.ema_every == 0;
        }
        skip_s = skip;
    }
    __syncthreads();
    if (skip_s) return;
    for (int64_t t = threadIdx.x; t < a.T; t += THREADS) {
        if (a.gtab[t] == 0) continue;
        const int64_t k = a.steps[t] + 1;
        a.steps[t] = k;
        // torch's single-tensor AdamW: step_size = lr / (1 - beta1**step), bias_correction2_sqrt = sqrt(1 - beta2**step), Python floats
        a.tscal[2 * t] = a.lr / (1.0 - pow(a.beta1, (double)k));
        a.tscal[2 * t + 1] = sqrt(1.0 - pow(a.beta2, (double)k));
    }
}

struct Hyp {
    float coef, decay_mul, omb1, b2, omb2, step_size, sbc2, eps, ema_w;
    int amsgrad, ema;
};

// one element: every operation rounded in fp32 as torch's kernels round it (no contraction)
__device__ inline void upd1(float& p, float g, float& m, float& v, float& vm, float& e, const Hyp& h, bool has_grad) {
#pragma clang fp contract(off)
    if (has_grad) {
        g = g * h.coef;
        p = p * h.decay_mul;
        m = m + h.omb1 * (g - m);                                             // torch.lerp with weight < 0.5
        v = v * h.b2 + g * g * h.omb2;
        float den;
        if (h.amsgrad) {
            vm = fmaxf(vm, v);
            den = sqrtf(vm) / h.sbc2 + h.eps;
        } else {
            den = sqrtf(v) / h.sbc2 + h.eps;
        }
        p = p + (-h.step_size) * (m / den);
    }
    if (h.ema) e = e - (e - p) * h.ema_w;
}

__global__ void __launch_bounds__(THREADS) k_opt_update(Args a) {
    const Scal* s = a.scal;
    if (s->skip) return;
    const int64_t c = blockIdx.x;
    const int64_t t = a.ctab[3 * c], start = a.ctab[3 * c + 1], len = a.ctab[3 * c + 2];
    const float* g = (const float*)a.gtab[t];
    const bool has_grad = g != nullptr;
    Hyp h;
    h.ema = s->ema_now;
    if (!has_grad && !h.ema) return;
    h.coef = s->coef;
    h.decay_mul = (float)(1.0 - a.lr * a.wd);
    h.omb1 = (float)(1.0 - a.beta1);
    h.b2 = (float)a.beta2;
    h.omb2 = (float)(1.0 - a.beta2);
    h.step_size = has_grad ? (float)a.tscal[2 * t] : 0.f;
    h.sbc2 = has_grad ? (float)a.tscal[2 * t + 1] : 1.f;
    h.eps = (float)a.eps;
    h.ema_w = (float)(1.0 - a.ema_decay);
    h.amsgrad = a.amsgrad;
    const int64_t off = a.otab[t] + start;
    float* p = (float*)a.ptab[t] + start;
    float* m = a.state + off;
    float* v = a.state + a.total + off;
    float* vm = a.state + 2 * a.total + off;
    float* e = a.state + 3 * a.total + off;
    if (has_grad) g += start;
    float dummy = 0.f;
    int64_t i0 = 0;
    // state offsets and chunk starts are multiples of 4 floats: the float4 body needs p and g on 16 bytes too
    if (aligned16(p) && (!has_grad || aligned16(g)) && aligned16(m)) {
        const int64_t n4 = len >> 2;
        for (int64_t i = threadIdx.x; i < n4; i += THREADS) {
            float4 P = ((float4*)p)[i], E = h.ema ? ((float4*)e)[i] : float4{0.f, 0.f, 0.f, 0.f};
            float4 G{0.f, 0.f, 0.f, 0.f}, M{0.f, 0.f, 0.f, 0.f}, Vv{0.f, 0.f, 0.f, 0.f}, VM{0.f, 0.f, 0.f, 0.f};
            if (has_grad) {
                G = ((const float4*)g)[i];
                M = ((float4*)m)[i];
                Vv = ((float4*)v)[i];
                if (h.amsgrad) VM = ((float4*)vm)[i];
            }
            upd1(P.x, G.x, M.x, Vv.x, VM.x, E.x, h, has_grad);
            upd1(P.y, G.y, M.y, Vv.y, VM.y, E.y, h, has_grad);
            upd1(P.z, G.z, M.z, Vv.z, VM.z, E.z, h, has_grad);
            upd1(P.w, G.w, M.w, Vv.w, VM.w, E.w, h, has_grad);
            if (has_grad) {
                ((float4*)p)[i] = P;
                ((float4*)m)[i] = M;
                ((float4*)v)[i] = Vv;
                if (h.amsgrad) ((float4*)vm)[i] = VM;
            }
            if (h.ema) ((float4*)e)[i] = E;
        }
        i0 = n4 << 2;
    }
    for (int64_t i = i0 + threadIdx.x; i < len; i += THREADS) {
        float P = p[i], E = h.ema ? e[i] : 0.f;
        float G = has_grad ? g[i] : 0.f, M = has_grad ? m[i] : 0.f, Vv = has_grad ? v[i] : 0.f;
        float VM = (has_grad && h.amsgrad) ? vm[i] : 0.f;
        upd1(P, G, M, Vv, h.amsgrad ? VM : dummy, E, h, has_grad);
        if (has_grad) {
            p[i] = P;
            m[i] = M;
            v[i] = Vv;
            if (h.amsgrad) vm[i] = VM;
        }
        if (h.ema) e[i] = E;
    }
}

// mode 0: swap p <-> ema; 1: ema = p; 2: p = ema
__global__ void __launch_bounds__(THREADS) k_opt_ema_swap(Args a, int mode) {
    const int64_t c = blockIdx.x;
    const int64_t t = a.ctab[3 * c], start = a.ctab[3 * c + 1], len = a.ctab[3 * c + 2];
    float* p = (float*)a.ptab[t] + start;
    float* e = a.state + 3 * a.total + a.otab[t] + start;
    for (int64_t i = threadIdx.x; i < len; i += THREADS) {
        const float x = p[i], y = e[i];
        if (mode != 1) p[i] = y;
        if (mode != 2) e[i] = x;
    }
}

inline Args make_args(void* workspace, float* state, int64_t total, int64_t T, int64_t C, int32_t Q) {
    const Layout L = layout(T, C, Q);
    char* w = (char*)workspace;
    Args a{};
    a.ptab = (const int64_t*)(w + L.ptab);
    a.gtab = (const int64_t*)(w + L.gtab);
    a.otab = (const int64_t*)(w + L.otab);
    a.ntab = (const int64_t*)(w + L.ntab);
    a.ctab = (const int64_t*)(w + L.ctab);
    a.steps = (int64_t*)(w + L.steps);
    a.tscal = (double*)(w + L.tscal);
    a.part = (float*)(w + L.part);
    a.queue = (double*)(w + L.queue);
    a.scal = (Scal*)(w + L.scal);
    a.state = state;
    a.total = total;
    a.T = T;
    a.C = C;
    a.queue_len = Q;
    return a;
}

}  // namespace gopt

extern "C" {

int64_t gcdm_optim_workspace_bytes(int32_t which, int64_t num_tensors, int64_t num_chunks, int32_t queue_len) {
    GOPS_REQUIRE(which >= 0 && which <= 11 && num_tensors >= 0 && num_chunks >= 0 && queue_len >= 1 && queue_len <= GCDM_OPTIM_QUEUE_MAX);
    const gopt::Layout L = gopt::layout(num_tensors, num_chunks, queue_len);
    const int64_t v[12] = {L.total, L.ptab, L.gtab, L.otab, L.ntab, L.ctab, L.host_end, L.steps, L.tscal, L.part, L.queue, L.scal};
    return v[which];
}

int gcdm_optim_step(void* workspace, float* state, int64_t total, int64_t num_tensors, int64_t num_chunks, double lr, double beta1, double beta2,
                    double eps, double weight_decay, int32_t amsgrad, int32_t clip, int32_t queue_len, int32_t ema, double ema_decay,
                    int64_t ema_every, int64_t ema_start, void* stream) {
    GOPS_REQUIRE(total >= 0 && num_tensors >= 0 && num_chunks >= 0 && queue_len >= 1 && queue_len <= GCDM_OPTIM_QUEUE_MAX);
    GOPS_REQUIRE(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && weight_decay >= 0.0);
    GOPS_REQUIRE(gops_flag(amsgrad) && gops_flag(clip) && gops_flag(ema) && ema_decay >= 0.0 && ema_decay <= 1.0 && ema_every >= 1 && ema_start >= 0);
    if (num_tensors == 0 || num_chunks == 0) return 0;
    GOPS_REQUIRE(workspace && state && total > 0);
    gopt::Args a = gopt::make_args(workspace, state, total, num_tensors, num_chunks, queue_len);
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay; a.ema_decay = ema_decay;
    a.ema_every = ema_every; a.ema_start = ema_start; a.amsgrad = amsgrad; a.clip = clip; a.ema = ema;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gopt::k_opt_sqnorm, dim3((unsigned)num_chunks), dim3(gopt::THREADS), 0, st, a);
    hipLaunchKernelGGL(gopt::k_opt_finalize, dim3(1), dim3(gopt::THREADS), 0, st, a);
    hipLaunchKernelGGL(gopt::k_opt_update, dim3((unsigned)num_chunks), dim3(gopt::THREADS), 0, st, a);
    return GOPS_LAUNCH_OK();
}

int gcdm_optim_ema_swap(void* workspace, float* state, int64_t total, int64_t num_tensors, int64_t num_chunks, int32_t queue_len, int32_t mode,
                        void* stream) {
    GOPS_REQUIRE(total >= 0 && num_tensors >= 0 && num_chunks >= 0 && queue_len >= 1 && queue_len <= GCDM_OPTIM_QUEUE_MAX && mode >= 0 && mode <= 2);
    if (num_tensors == 0 || num_chunks == 0) return 0;
    GOPS_REQUIRE(workspace && state && total > 0);
    const gopt::Args a = gopt::make_args(workspace, state, total, num_tensors, num_chunks, queue_len);
    hipLaunchKernelGGL(gopt::k_opt_ema_swap, dim3((unsigned)num_chunks), dim3(gopt::THREADS), 0, (hipStream_t)stream, a, (int)mode);
    return GOPS_LAUNCH_OK();
}

}  // extern "C"
