/* gcdm_mp_tile.h -- C ABI of the "tiled" message layer for training, exported from libgcdm_ops.so (gfx950 / MI355X).  Plain C99.
 *
 * The same function as include/gcdm_mp_train.h (one interaction layer's GCPMessagePassing.forward and its backward, same configuration,
 * same tensors, same weight table, same conventions, bad-argument rules, empty-work rule and return codes -- read that header), on other
 * kernels: each message GCP's scalar GEMM, silu, gate GEMM and gated vector update are ONE tile kernel in the forward (64 edges per
 * workgroup), and its gate backward, d gate_in GEMM and silu backward ONE tile kernel in the backward.  12 launches forward and 17 backward
 * instead of 24 and 25; silu(S_pre) and the d gate_in product never reach memory.  The matrix mode (include/gcdm_matrix_mode.h) is read once
 * per call.  No float atomics: the results, gradients included, are the same bits from run to run, and a row's result does not depend on
 * the other rows.
 *
 * Workspace: gcdm_mp_tile_workspace_bytes(which, N, E, SE, VE), `which` as gcdm_mp_workspace_bytes: 0 the forward without a tape, 1 the
 * forward with a tape, 2 the backward's scratch, 3 the size of dweights.  Never larger than gcdm_mp_workspace_bytes(which, ...); which = 1
 * and which = 3 are equal to it.
 *
 * The tape is interchangeable with gcdm_mp_fwd's: same size, same layout, and every field a backward reads holds what gcdm_mp_fwd puts
 * there, so a tape written by either forward may be handed to either backward.  The one field no backward reads, the buffer of
 * silu(S_pre) that gcdm_mp_fwd's gate GEMM goes through, is left UNWRITTEN by gcdm_mp_tile_fwd. */
#ifndef GCDM_MP_TILE_H
#define GCDM_MP_TILE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int64_t gcdm_mp_tile_workspace_bytes(int32_t which, int64_t N, int64_t E, int32_t SE, int32_t VE);

int gcdm_mp_tile_fwd(const float* h, const float* vnode, const float* e, const float* xi, const int64_t* row, const int64_t* col,
                     const int32_t* rowptr, const float* frames, const uint8_t* edge_mask, const float* const* weights, float* agg, float* workspace,
                     int32_t tape, int64_t N, int64_t E, int32_t SE, int32_t VE, void* stream);

/* dagg [N][352] in; dh [N][256], dvnode [N][32][3], de [E][SE], dxi [E][VE][3], dweights out (all written, none accumulated) */
int gcdm_mp_tile_bwd(const float* dagg, const float* h, const int64_t* row, const int64_t* col, const int32_t* rowptr, const int32_t* colptr,
                     const int64_t* colperm, const float* frames, const uint8_t* edge_mask, const float* const* weights, const float* tape,
                     float* workspace, float* dh, float* dvnode, float* de, float* dxi, float* dweights, int64_t N, int64_t E, int32_t SE, int32_t VE,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
