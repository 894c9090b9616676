/* gcdm_mp_train.h -- C ABI of the fused message layer for training, exported from libgcdm_ops.so (gfx950 / MI355X).  Plain C99.
 *
 * One call evaluates GCPMessagePassing.forward of one interaction layer (reference gcpnet.py:676-737: gather -> msg0 -> residual msg1-3 ->
 * scalar attention -> row sum); one call back-propagates through it.  Configuration: GCP2 with vector_gate, silu / silu, bottleneck 4, four
 * residual message GCPs, scalar attention, sum aggregation, node dims (256, 32), edge dims (SE, VE) = (64, 16) or (16, 8).  Exact fp32.
 * No float atomics: the results, gradients included, are the same bits from run to run.
 *
 * Conventions as include/gcdm_ops.h: device pointers, sizes, a hipStream_t passed as void*; caller-owned buffers; nothing is allocated,
 * nothing synchronises.  0 on success, -1 for a bad argument (checked before any HIP call; nothing is touched), -2 if a launch failed.
 * Bad arguments: N or E negative, E > 0 with N = 0, (SE, VE) not one of the two pairs, `tape` / `which` out of range, a null pointer the
 * call needs (edge_mask may be null), a null entry of `weights`.  Empty work (N = 0 or E = 0) returns 0 without a launch and writes
 * nothing: the caller's aggregate is the zero sum, its gradients are zero.
 *
 * Tensors (fp32 row-major, index tensors int64, CSR pointers int32):
 *   h [N][256], vnode [N][32][3], e [E][SE], xi [E][VE][3], frames [E][3][3]; row / col [E] with row sorted (rowptr [N+1] its CSR);
 *   colperm [E] a stable argsort of col and colptr [N+1] the CSR of col[colperm] (the fixed order of every column sum);
 *   edge_mask [E] (uint8, may be null): 0 zeroes the edge's frame (an edge with a masked end point, gcp_modules._entity_frames);
 *   agg [N][352] = [sum of attended scalar messages (256) | sum of vector messages (32 x 3)].
 *   weights: a HOST array of 30 device pointers, the nn.Linear tensors of the layer's `interaction` module in this order --
 *     for k = 0..3 (message_fusion.k.): vector_down.weight, vector_down_frames.weight, scalar_out.weight, scalar_out.bias,
 *                                       vector_up.weight, vector_out_scale.weight, vector_out_scale.bias;
 *     then scalar_message_attention.0.weight, scalar_message_attention.0.bias.
 *   dweights: the gradients of those 30 tensors, concatenated in the same order (gcdm_mp_workspace_bytes(3, ...) bytes).
 *
 * Workspace: gcdm_mp_workspace_bytes(which, N, E, SE, VE), a host-only query: which = 0 the forward without a tape, 1 the forward with a
 * tape (the workspace then IS the tape: what gcdm_mp_bwd reads; keep it unchanged until the backward), 2 the backward's scratch, 3 the
 * size of dweights.  Returns -1 for a bad argument. */
#ifndef GCDM_MP_TRAIN_H
#define GCDM_MP_TRAIN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int64_t gcdm_mp_workspace_bytes(int32_t which, int64_t N, int64_t E, int32_t SE, int32_t VE);

int gcdm_mp_fwd(const float* h, const float* vnode, const float* e, const float* xi, const int64_t* row, const int64_t* col, const int32_t* rowptr,
                const float* frames, const uint8_t* edge_mask, const float* const* weights, float* agg, float* workspace, int32_t tape, int64_t N,
                int64_t E, int32_t SE, int32_t VE, void* stream);

/* dagg [N][352] in; dh [N][256], dvnode [N][32][3], de [E][SE], dxi [E][VE][3], dweights out (all written, none accumulated) */
int gcdm_mp_bwd(const float* dagg, const float* h, const int64_t* row, const int64_t* col, const int32_t* rowptr, const int32_t* colptr,
                const int64_t* colperm, const float* frames, const uint8_t* edge_mask, const float* const* weights, const float* tape, float* workspace,
                float* dh, float* dvnode, float* de, float* dxi, float* dweights, int64_t N, int64_t E, int32_t SE, int32_t VE, void* stream);

#ifdef __cplusplus
}
#endif
#endif
