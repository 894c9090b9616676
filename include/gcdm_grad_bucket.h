/* gcdm_grad_bucket.h -- C ABI of the flat gradient bucket for data-parallel and accumulated training steps, exported from libgcdm_ops.so
 * (gfx950 / MI355X).  Plain C99.
 *
 * The bucket is one flat fp32 buffer laid out exactly like a state quarter of the fused training update (include/gcdm_optim.h): tensor t at
 * offset[t], the offsets, numels and chunk table being sections 3, 4 and 5 of the optimiser workspace, which these entries read and never
 * write.  gcdm_grad_bucket_pack fills it from the per-tensor gradients of one backward pass, or adds such a pass to it, in one launch; the
 * caller sums it over the ranks with one all-reduce; gcdm_grad_bucket_check looks at the reduced bucket; and gcdm_optim_step, its gradient
 * table (section 2) pointing at bucket + offset[t], consumes it unchanged.  Gradient accumulation is the same with one rank.  No float
 * atomics and no host sync: the same gradients give the same bits, on every rank.
 *
 * Conventions as include/gcdm_optim.h: device pointers, a hipStream_t passed as void*; caller-owned buffers; nothing is allocated, nothing
 * synchronises.  0 on success, -1 for a bad argument (checked before any HIP call; nothing is touched), -2 if a launch failed.
 * Bad arguments: a negative size; total no multiple of 4; queue_len outside 1 .. GCDM_OPTIM_QUEUE_MAX (it places the workspace sections);
 * first outside {0, 1}; scale NaN or infinite; world < 1; a null workspace, bucket or gradient table, or total = 0, with work to do.
 * num_tensors = 0 or num_chunks = 0 returns 0 without a launch.
 *
 * The bucket: gcdm_grad_bucket_floats(total, T) floats, 256-byte aligned.
 *   value part     `total` floats; tensor t's values at offset[t] .. offset[t] + numel[t]; the rest is padding
 *   presence tail  T floats, rounded up to a multiple of 64: presence[t] counts the passes' verdicts on tensor t (below)
 *
 * gcdm_grad_bucket_pack: grad_ptrs is a device table of T gradient pointers (fp32, dense, numel[t] values each, at any 4-byte alignment),
 * separate from section 2 of the workspace; 0 = tensor t has no gradient in this pass.  s = (float)scale.
 *   first = 1   every float of the bucket becomes defined, whatever it held: a present tensor's values are fl32(s g); an absent tensor's
 *               values, all padding and the padding of the tail are +0.0; presence[t] = 1.0 if present, else 0.0.
 *   first = 0   a present tensor's values become fl32(bucket + fl32(s g)); absent tensors and the padding are untouched;
 *               presence[t] = max(presence[t], present).
 * The product and the sum are two separately rounded fp32 operations (no fused multiply-add), so s = 1 copies the bits of g (-0.0 and
 * denormals included) and a numpy float32 evaluation gives the same bits for any scale.  The result does not depend on the alignment of a
 * gradient pointer.  One launch.
 *
 * gcdm_grad_bucket_check runs after the all-reduce (sum) over `world` ranks.  Every presence[t] must then be 0 (no rank had a gradient) or
 * `world` (every rank had one).  If one is not, it ORs GCDM_GRAD_BUCKET_FLAG_MISMATCH into the flag word of the optimiser's scalar block
 * (section 11) and writes a NaN into the first value of every tensor's segment of the bucket, so that the following gcdm_optim_step, reading
 * its gradients from the bucket, finds a non-finite norm and skips as a whole (raising GCDM_OPTIM_FLAG_NONFINITE as well).  A consistent tail
 * changes nothing.  One launch of one workgroup. */
#ifndef GCDM_GRAD_BUCKET_H
#define GCDM_GRAD_BUCKET_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GCDM_GRAD_BUCKET_FLAG_MISMATCH 2

int64_t gcdm_grad_bucket_floats(int64_t total, int64_t num_tensors);

int gcdm_grad_bucket_pack(const void* optim_workspace, const int64_t* grad_ptrs, float* bucket, int64_t total, int64_t num_tensors,
                          int64_t num_chunks, int32_t queue_len, double scale, int32_t first, void* stream);

int gcdm_grad_bucket_check(void* optim_workspace, float* bucket, int64_t total, int64_t num_tensors, int64_t num_chunks, int32_t queue_len,
                           int32_t world, void* stream);

#ifdef __cplusplus
}
#endif
#endif
