/* gcdm_gcp2_train.h -- C ABI of one stand-alone GCP2 module for training, forward and backward, exported from libgcdm_ops.so (gfx950 / MI355X).
 * Plain C99.
 *
 * One call evaluates GCP2.forward (reference gcpnet.py:418-491 with process_vector_with_frames :378-415) of one module on M entities (edge
 * rows or node rows); one call back-propagates through it.  Configuration: vector_gate, no frame_gate / sigma_frame_gate, scalar_gate = 0, no
 * vector or frame residual, no ablation flag, scalarization_vectorization_output_dim = 3, vector inputs present (VI > 0); each of the two
 * nonlinearities identity or silu; scalar_out a Linear or (feedforward_out) Linear - SiLU - Linear.  Exact fp32 (the GEMMs run on
 * v_mfma_f32_32x32x2_f32).  No float atomics: outputs and gradients are the same bits from run to run, and a row's outputs are the same bits
 * whatever M is and whichever rows surround it.
 *
 * Conventions as include/gcdm_mp_train.h: device pointers, sizes, a hipStream_t passed as void*; caller-owned buffers; nothing is allocated,
 * nothing synchronises.  0 on success, -1 for a bad argument (checked before any HIP call; nothing is touched), -2 if a launch failed.
 * Bad arguments: a null `dims`, dims outside the bounds below, M negative or above GCDM_GCP2_MAX_ROWS, `tape` / `which` out of range, a null
 * pointer the call needs (row_mask may be null; v_out / dv_out may be null when VO = 0), a null entry of `weights`.  Empty work (M = 0)
 * returns 0 without a launch and writes nothing.
 *
 * Bounds: 1 <= SI <= 2048, 1 <= VI <= 128, 1 <= SO <= 1024, 0 <= VO <= 64, 1 <= H <= 64, feedforward_out in {0, 1}, act_scalar and
 * act_vector in {0 identity, 1 silu}.  H is the module's hidden_dim (VI / bottleneck, or max(VI, VO) for bottleneck 1); K = SI + H + 9 is
 * the width of the merged row [s | |vh| | q].
 *
 * Tensors (fp32 row-major):
 *   s [M][SI], v [M][VI][3], F [M][3][3] the entity's frame (rows a, b, c; the edge's own frame for edge rows, the mean of the frames of the
 *   node's edges for node rows; a constant: it gets no gradient), row_mask [M] (uint8, may be null): 0 zeroes that row's frame;
 *   s_out [M][SO] = act_scalar(p), v_out [M][VO][3] = vector_up(vh) * sigmoid(vector_out_scale(act_vector(p))) (absent when VO = 0).
 *   weights: a HOST array of device pointers, the module's nn.Linear tensors in state-dict order --
 *     vector_down.weight [H][VI], vector_down_frames.weight [3][VI],
 *     scalar_out.weight [SO][K], scalar_out.bias [SO]      (feedforward_out: scalar_out.0.weight [SO][K], .0.bias, .2.weight [SO][SO], .2.bias),
 *     and when VO > 0: vector_up.weight [VO][H], vector_out_scale.weight [VO][SO], vector_out_scale.bias [VO]
 *     (4 + 2 feedforward_out + 3 (VO > 0) entries).
 *   dweights: the gradients of those tensors, concatenated in the same order (gcdm_gcp2_workspace_bytes(3, ...) bytes).
 *
 * Workspace: gcdm_gcp2_workspace_bytes(which, M, dims), a host-only query: which = 0 the forward without a tape, 1 the forward with a tape
 * (the workspace then IS the tape: vh, the merged row, p, the feed-forward hidden pre-activation and the gate pre-activation; keep it
 * unchanged until the backward, which only reads it), 2 the backward's scratch, 3 the size of dweights.  Returns -1 for a bad argument.
 *
 * Launches: the forward 2 (3 with feedforward_out), the backward 5 (6 with feedforward_out): all weight gradients, biases included, come from
 * one grouped split-K launch with a fixed slice count and one slice reduction. */
#ifndef GCDM_GCP2_TRAIN_H
#define GCDM_GCP2_TRAIN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GCDM_GCP2_MAX_SI 2048
#define GCDM_GCP2_MAX_VI 128
#define GCDM_GCP2_MAX_SO 1024
#define GCDM_GCP2_MAX_VO 64
#define GCDM_GCP2_MAX_H 64
#define GCDM_GCP2_MAX_ROWS 268435456 /* 2^28 */

typedef struct gcdm_gcp2_dims {
    int32_t SI, VI, SO, VO, H;
    int32_t feedforward_out;
    int32_t act_scalar, act_vector; /* 0 identity, 1 silu */
} gcdm_gcp2_dims;

int64_t gcdm_gcp2_workspace_bytes(int32_t which, int64_t M, const gcdm_gcp2_dims* dims);

int gcdm_gcp2_fwd(const float* s, const float* v, const float* F, const uint8_t* row_mask, const float* const* weights, float* s_out, float* v_out,
                  float* workspace, int32_t tape, int64_t M, const gcdm_gcp2_dims* dims, void* stream);

/* ds_out [M][SO], dv_out [M][VO][3] in; ds [M][SI], dv [M][VI][3], dweights out (all written, none accumulated) */
int gcdm_gcp2_bwd(const float* ds_out, const float* dv_out, const float* s, const float* v, const float* F, const uint8_t* row_mask,
                  const float* const* weights, const float* tape, float* workspace, float* ds, float* dv, float* dweights, int64_t M,
                  const gcdm_gcp2_dims* dims, void* stream);

#ifdef __cplusplus
}
#endif
#endif
