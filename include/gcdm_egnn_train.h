/* gcdm_egnn_train.h -- C ABI of the per-edge block of an EGNN dynamics layer as one differentiable operator, forward and backward, exported
 * from libgcdm_ops.so (gfx950 / MI355X).  Plain C99.  DESIGN.md 3.10.
 *
 * Notation as include/gcdm_egnn_dynamics.h: H = h_hidden, Eh = e_hidden, D = 2 H + Eh + 1, K = 2 D; i receives, j sends; the edges are all
 * ordered pairs of one molecule, the diagonal included, and are never materialised (slot s of node i is node_offsets[mol(i)] + s).
 *
 * Inputs (device pointers, fp32, contiguous): A [N, K] (= h W_i^T + b1 + W_e b_emb), B [N, K] (= h W_j^T), V [3, K] (rows u = W_e w_emb[:, 0],
 * u' = W_e w_emb[:, 1] -- ignored with e_in = 1 -- and w_r), W2 [16, K], b2 [16], C1 [64, 16], c1b [64], c2 [64], c2b [1], scale [1],
 * x [N, 3] the current coordinates, x0 [N, 3] the network's input coordinates, xsc [N, 3] (e_in = 2; null with e_in = 1), node_offsets int32
 * [B + 1], node_mol int32 [N].
 *
 * Forward, per edge: d = x_j - x_i, r = |d|^2, r0 / r0sc the same of x0 / xsc; z1 = A_i + B_j + r0 u + r0sc u' + r w_r; z2 = W2 silu(z1) + b2;
 * m = silu(z2); w = tanh(c2 . silu(C1 m + c1b) + c2b); t = w d / max(|d|, 1e-8) scale.  Outputs M [N, 16] = sum_j m_ij and dx [N, 3] =
 * sum_j t_ij, summed per receiver in slot order by one owner: the same bits from run to run and for a molecule whatever else is in the batch.
 *
 * Backward: given gM [N, 16] and gdx [N, 3] it writes gA [N, K], gB [N, K], gx [N, 3], gV [3, K] (the row of u' zero with e_in = 1), gW2
 * [16, K], gb2 [16], gC1 [64, 16], gc1b [64], gc2 [64], gc2b [1], gscale [1].  Nothing per edge is saved by the forward: the backward
 * recomputes every edge from A, B, x, twice (once with the receiver as the owner of the sums, once with the sender).  x0 and xsc get no gradient.
 * The diagonal edge i = j contributes to gA, gB, gV and the weight gradients like any other edge and NOTHING to gx: its coordinate term is
 * identically zero, and its derivative scale w_ii / 1e-8 would enter gx_i once with each sign; it is never formed.  For a coincident pair of
 * distinct atoms the clamp branch applies, as in torch: g_d = 2 d (w_r . g_z1) + w scale g_t / 1e-8.
 * No float atomics; every output has the same bits from run to run.  The weight and vector gradients go through one partial block per workgroup
 * in the workspace ((19 K + 1170) floats each, at most GCDM_EGNN_TRAIN_MAX_GROUPS of them: the grid is capped and the workgroups loop) and a
 * fixed-order reduction launch.  The MFMAs are exact fp32; ops.matrix_mode has no influence.
 *
 * Conventions as include/gcdm_egnn_dynamics.h: a hipStream_t passed as void*; caller-owned buffers; nothing is allocated, nothing
 * synchronises.  0 on success, -1 for a bad argument (checked before any HIP call; nothing is touched; gcdm_egnn_train_last_error() says which),
 * -2 if a launch failed.  Limits: H a multiple of 32 in 32 .. 256, Eh in 1 .. 1024, e_in 1 or 2, at most 2^24 atoms, any molecule size.  A node
 * whose molecule index or offsets are inconsistent has no edges: its rows of M, dx, gA, gB, gx are zero and nothing is read out of bounds.
 *
 * gcdm_egnn_train_workspace_bytes: the workspace of gcdm_egnn_train_edge_bwd, -1 on a bad argument.  min(max(num_nodes, 1), GCDM_EGNN_TRAIN_MAX_GROUPS) partial
 *   blocks of (19 K + 1170) floats plus 256 bytes: monotone in num_nodes and never more than GCDM_EGNN_TRAIN_MAX_GROUPS blocks.
 * gcdm_egnn_train_launches: backward-kernel launches of this process so far: GCDM_EGNN_TRAIN_BWD_LAUNCHES (one per role) per successful
 *   gcdm_egnn_train_edge_bwd call with num_nodes > 0. */
#ifndef GCDM_EGNN_TRAIN_H
#define GCDM_EGNN_TRAIN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GCDM_EGNN_TRAIN_MAX_GROUPS 256
#define GCDM_EGNN_TRAIN_BWD_LAUNCHES 2

const char* gcdm_egnn_train_last_error(void);

int64_t gcdm_egnn_train_workspace_bytes(int64_t num_nodes, int32_t h_hidden, int32_t e_hidden, int32_t e_in);

int64_t gcdm_egnn_train_launches(void);

int gcdm_egnn_train_edge_fwd(const float* A, const float* B, const float* V, const float* W2, const float* b2, const float* C1, const float* c1b,
                             const float* c2, const float* c2b, const float* scale, const float* x, const float* x0, const float* xsc,
                             const int32_t* node_offsets, const int32_t* node_mol, float* M, float* dx, int64_t num_nodes, int64_t num_molecules,
                             int32_t h_hidden, int32_t e_hidden, int32_t e_in, void* stream);

int gcdm_egnn_train_edge_bwd(const float* A, const float* B, const float* V, const float* W2, const float* b2, const float* C1, const float* c1b,
                             const float* c2, const float* c2b, const float* scale, const float* x, const float* x0, const float* xsc,
                             const int32_t* node_offsets, const int32_t* node_mol, const float* gM, const float* gdx, void* workspace, float* gA,
                             float* gB, float* gx, float* gV, float* gW2, float* gb2, float* gC1, float* gc1b, float* gc2, float* gc2b,
                             float* gscale, int64_t num_nodes, int64_t num_molecules, int32_t h_hidden, int32_t e_hidden, int32_t e_in,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
