/* gcdm_matrix_mode.h -- the matrix mode of libgcdm_ops.so's training GEMMs (gfx950 / MI355X).  Plain C99.
 *
 * Every GEMM of the training path runs on one 64 x 64 tile body (the plain GEMM, the grouped split-K weight gradients, and the GEMM kernels of
 * the fused stand-alone GCP2).  The mode chooses the matrix instruction under it:
 *   GCDM_OPS_MATRIX_F32     the default: v_mfma_f32_32x32x2_f32, exact fp32 products, fp32 accumulate.
 *   GCDM_OPS_MATRIX_BF16X6  every fp32 operand element is the exact sum of three bf16 images, x = x0 + x1 + x2, and a product is the six
 *                           largest of the nine cross terms on v_mfma_f32_32x32x16_bf16,
 *                               x y ~ x0 y0 + (x0 y1 + x1 y0) + (x1 y1 + x0 y2 + x2 y0),
 *                           the brackets in fp32 accumulators of their own, merged once per tile, smallest first.  The dropped terms are
 *                           <= 2^-24 relative: fp32-class accuracy (the tests hold it to the bars of fp32 mode), not fp32's bits.
 *
 * The switch is process-wide and atomic, not per thread: autograd runs a backward pass on another thread, which has to see it.
 * gcdm_op_gemm, gcdm_mp_fwd, gcdm_mp_bwd, gcdm_gcp2_fwd and gcdm_gcp2_bwd read it once on entry, so all launches of one call run in one mode;
 * a call that is already enqueued is not affected by a later change.  No other entry of the library depends on it, and no signature changes
 * with it: same arguments, same workspaces, same split-K slice counts and slice reduction order, same launches.  In either mode a result
 * does not depend on the row count or on neighbouring rows, and repeats bitwise from run to run.
 *
 * gcdm_ops_set_matrix_mode returns 0, or -1 for any other value (the mode is then unchanged).  gcdm_ops_get_matrix_mode returns the current
 * mode.  Neither makes a HIP call.
 *
 * bf16x6 at the edges.  bf16 has fp32's exponent range, so the mode needs no range guard, prescale or flag for finite operands with
 * |x| < 2^127.  An operand that is +-Inf, NaN, or at or above 2^127 in magnitude gives a non-finite result (NaN or Inf) in every output
 * element that depends on it, never a finite one; elements that do not depend on it are unaffected.  The second and third image of an
 * operand below about 2^-109 in magnitude are fp32 denormals and may be flushed to zero, as may a denormal operand itself: such an operand
 * then enters with 8 or 16 significant bits, an error of at most 2^-126 times the other factor per product, which the absolute term of the
 * tolerances this library is tested with covers. */
#ifndef GCDM_MATRIX_MODE_H
#define GCDM_MATRIX_MODE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GCDM_OPS_MATRIX_F32 0
#define GCDM_OPS_MATRIX_BF16X6 1

int gcdm_ops_set_matrix_mode(int32_t mode);
int32_t gcdm_ops_get_matrix_mode(void);

#ifdef __cplusplus
}
#endif
#endif
