/* gcdm_optim.h -- C ABI of the fused training update, exported from libgcdm_ops.so (gfx950 / MI355X).  Plain C99.
 *
 * One call does what the reference's training step does after backward(): adaptive gradient clipping (max_norm = 1.5 mean(Q) + 2 std(Q)
 * over a queue Q of the last `queue_len` clipped gradient norms, qm9_mol_gen_ddpm.py configure_gradient_clipping), AdamW with optional
 * AMSGrad (torch.optim.AdamW), and an EMA of the weights, ema -= (1 - decay) (ema - p) (utils/__init__.py EMA).  Three launches, no host
 * sync, no float atomics: a step gives the same bits from run to run.  A non-finite gradient norm skips the whole step -- parameters,
 * moments, step counts, EMA and queue stay as they are -- and raises GCDM_OPTIM_FLAG_NONFINITE in the flag word (the reference would
 * write NaN into every weight).
 *
 * Conventions as include/gcdm_ops.h: device pointers, a hipStream_t passed as void*; caller-owned buffers; nothing is allocated, nothing
 * synchronises.  0 on success, -1 for a bad argument (checked before any HIP call; nothing is touched), -2 if a launch failed.
 * Bad arguments: a negative size; queue_len outside 1 .. GCDM_OPTIM_QUEUE_MAX; lr, eps or weight_decay negative or NaN; beta1 or beta2
 * outside [0, 1); amsgrad, clip or ema outside {0, 1}; ema_decay outside [0, 1]; ema_every < 1; ema_start < 0; mode outside 0 .. 2;
 * a null workspace or state, or total = 0, with work to do.  num_tensors = 0 or num_chunks = 0 returns 0 without a launch.
 *
 * Buffers:
 *   state     fp32, 4 * total floats: m | v | vmax | ema, each `total` floats (total a multiple of 4).  Tensor t's values start at offset[t]
 *             within each quarter (a multiple of 4).  vmax is used with amsgrad, ema with ema = 1.
 *   workspace 256-byte aligned, gcdm_optim_workspace_bytes(0, ...) bytes.  Sections (byte offset = gcdm_optim_workspace_bytes(which, ...)):
 *      which  1  int64 [T]     parameter pointers (fp32, device)                         written by the caller once
 *             2  int64 [T]     gradient pointers, 0 = no gradient this step (skipped)     written by the caller when one changes
 *             3  int64 [T]     offset of tensor t in each state quarter                   written by the caller once
 *             4  int64 [T]     numel of tensor t                                          written by the caller once
 *             5  int64 [C][3]  chunks (tensor, start, length): start a multiple of 4, the chunks of a tensor cover it exactly once
 *             6  end of the caller-written part
 *             7  int64 [T]     AdamW step count of tensor t                               set by the caller at the start, then owned here
 *             8  double [T][2] lr / (1 - beta1^step), sqrt(1 - beta2^step) of the last step (scratch)
 *             9  float [C]     partial sums of g^2 (scratch)
 *            10  double [queue_len] the queue, a ring                                     seeded by the caller
 *            11  the 64-byte scalar block: double norm @0, double max_norm @8, float coef @16, int32 flags @20, int32 qhead @24 (slot of
 *                the next push), int32 qcount @28 (values in the ring, slots 0 .. qcount-1 until it is full), int64 steps done @32,
 *                int32 skipped @40, int32 ema applied @44.  The caller seeds it and clears `flags` after reading it.
 *   T = num_tensors, C = num_chunks.  which = 0 is the total size.
 *
 * gcdm_optim_step, for each tensor t with a gradient g (coef = min(1, max_norm / (norm + 1e-6)) with clip = 1, else 1; every operation
 * rounded in fp32 as torch's kernels round it):
 *   g' = coef g;  p *= 1 - lr wd;  m = lerp(m, g', 1 - beta1);  v = beta2 v + (1 - beta2) g'^2;  vmax = max(vmax, v) (amsgrad);
 *   p -= lr / (1 - beta1^step) * m / (sqrt(vmax or v) / sqrt(1 - beta2^step) + eps)
 * and then, when ema = 1 and the k-th completed step has k >= ema_start and k % ema_every == 0, for every tensor (with a gradient or not):
 *   ema -= (1 - ema_decay) (ema - p).
 * With clip = 1 the step pushes min(norm, max_norm) onto the queue.  With clip = 1 the caller seeds at least one queue value (qcount >= 1):
 * the mean and the deviation divide by qcount, and the result with an empty queue is unspecified.
 *
 * gcdm_optim_ema_swap: mode 0 swaps p and ema, 1 copies p into ema, 2 copies ema into p (every tensor of the table). */
#ifndef GCDM_OPTIM_H
#define GCDM_OPTIM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GCDM_OPTIM_QUEUE_MAX 1024
#define GCDM_OPTIM_FLAG_NONFINITE 1

int64_t gcdm_optim_workspace_bytes(int32_t which, int64_t num_tensors, int64_t num_chunks, int32_t queue_len);

int gcdm_optim_step(void* workspace, float* state, int64_t total, int64_t num_tensors, int64_t num_chunks, double lr, double beta1, double beta2,
                    double eps, double weight_decay, int32_t amsgrad, int32_t clip, int32_t queue_len, int32_t ema, double ema_decay,
                    int64_t ema_every, int64_t ema_start, void* stream);

int gcdm_optim_ema_swap(void* workspace, float* state, int64_t total, int64_t num_tensors, int64_t num_chunks, int32_t queue_len, int32_t mode,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
