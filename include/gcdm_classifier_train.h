/* gcdm_classifier_train.h -- C ABI of the one operator the EGNN property classifier's training path adds to the module-level operators: the first
 * per-edge layer (edge_mlp.0 of E_GCL_mask, src/__init__.py:286-291) with its weight split by columns, forward and backward.  Exported from
 * libgcdm_ops.so (gfx950 / MI355X).  Plain C99.
 *
 * Conventions as include/gcdm_geom.h: device pointers, a hipStream_t passed as void*; caller-owned buffers; nothing is allocated, nothing
 * synchronises.  0 on success, -1 for a bad argument (checked before any HIP call; nothing is touched), -2 if a launch failed.  E = 0 returns 0
 * without a launch and writes nothing.  All fp32.  No float atomics: every sum has a fixed order, so two calls on the same input give the
 * same bits.
 *
 * The edge set is the one the classifier evaluates: the ordered pairs i != j of each molecule, row-major.  Molecule m owns the nodes
 * node_offsets[m] .. node_offsets[m + 1] - 1 (n of them) and the edges edge_offsets[m] .. edge_offsets[m] + n (n - 1) - 1; the edge of local
 * atoms (i, j) is edge_offsets[m] + i (n - 1) + j - (j > i).  node_mol[v] is the molecule of node v.  The three tables are read on the device
 * and checked there: a node whose tables disagree (molecule out of range, the node outside its molecule, nodes beyond N, edges beyond E)
 * gets no edge written in the forward and zeros in the backward, and every load and store stays inside the sizes given.
 *
 * With W = [W_s | W_t | w_r] the weight of edge_mlp.0, A = h W_s^T + b and B = h W_t^T are node-level GEMMs (gcdm_op_gemm); then
 *
 * gcdm_classifier_train_edge_pre_fwd (one launch, one workgroup per node i):
 *   radial[e] = (dx dx + dy dy) + dz dz with d = x[i] - x[j], each product and sum rounded once (coord2radial, :318-321);
 *   pre[e][c] = (A[i][c] + B[j][c]) + radial[e] w_r[c]                                   for e = (i, j).
 *   A, B [N][H], x [N][3], w_r [H], pre [E][H], radial [E] (the backward reads it).
 *
 * gcdm_classifier_train_edge_pre_bwd (two or three launches):
 *   dA[i][c] = sum_j dpre[(i, j)][c], j ascending: the node's own contiguous rows;
 *   dB[j][c] = sum_i dpre[(i, j)][c], i ascending: the molecule's block walked with stride n - 1, no sorted copy of the edge list;
 *   dw_r[c]  = sum_e radial[e] dpre[e][c]: rows strided over the four waves of a workgroup, then a fixed tree.  From
 *              GCDM_CLASSIFIER_TRAIN_TWO_STAGE_EDGES edges on the sum has two stages: min(GCDM_CLASSIFIER_TRAIN_MAX_SLICES,
 *              ceil(E / GCDM_CLASSIFIER_TRAIN_SLICE_EDGES)) contiguous slices of edges write partial sums to `workspace`, which a second launch
 *              adds in slice order; below that count `workspace` is not read and may be null.
 *   There is no gradient to x: positions are data.  dA, dB [N][H] are written for every node (zeros for a molecule of one atom).
 *
 * gcdm_classifier_train_workspace_bytes(E, H): the bytes of `workspace` for the backward (0 below the two-stage count), 256-byte aligned; -1
 * for a bad argument.
 *
 * Bounds: 0 <= N, num_molecules < 2^31; 1 <= H <= GCDM_CLASSIFIER_TRAIN_MAX_H; 0 <= E, E H < 2^62. */
#ifndef GCDM_CLASSIFIER_TRAIN_H
#define GCDM_CLASSIFIER_TRAIN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GCDM_CLASSIFIER_TRAIN_MAX_H 4096
#define GCDM_CLASSIFIER_TRAIN_TWO_STAGE_EDGES 4096
#define GCDM_CLASSIFIER_TRAIN_SLICE_EDGES 512
#define GCDM_CLASSIFIER_TRAIN_MAX_SLICES 256

int64_t gcdm_classifier_train_workspace_bytes(int64_t E, int32_t H);

int gcdm_classifier_train_edge_pre_fwd(const float* A, const float* B, const float* x, const float* w_r, const int32_t* node_mol,
                                       const int32_t* node_offsets, const int64_t* edge_offsets, float* pre, float* radial, int64_t N,
                                       int64_t num_molecules, int64_t E, int32_t H, void* stream);

int gcdm_classifier_train_edge_pre_bwd(const float* dpre, const float* radial, const int32_t* node_mol, const int32_t* node_offsets,
                                       const int64_t* edge_offsets, float* dA, float* dB, float* dw_r, void* workspace, int64_t N,
                                       int64_t num_molecules, int64_t E, int32_t H, void* stream);

#ifdef __cplusplus
}
#endif
#endif
