/* gcdm_egnn_dynamics.h -- C ABI of the EGNN dynamics network's layers (forward only), exported from libgcdm_ops.so (gfx950 / MI355X).
 * Plain C99.  DESIGN.md 3.10.
 *
 * The network is the reference's EGNNDynamics (src/models/components/egnn.py:227-400, 573-823): per layer and per ordered pair (i, j) of one
 * molecule (i = j included: the fully connected edge index keeps the diagonal), with H = h_hidden_dim, Eh = e_hidden_dim, D = 2 H + Eh + 1,
 *   m_ij  = silu(W2 silu(W1 [h_i | h_j | edge_attr_ij | |x_j - x_i|^2] + b1) + b2)                       edge_mlp, 2 D wide inside, 16 out
 *   w_ij  = tanh(c2 . silu(C1 m_ij + c1b) + c2b)                                                           coors_mlp, 64 wide inside
 *   x_i  += sum_j w_ij (x_j - x_i) / max(|x_j - x_i|, 1e-8) * scale                                        coors_norm
 *   h_i  += node_mlp([LayerNorm_graph(h)_i | sum_j m_ij])                                                  node_norm, node_mlp
 * edge_attr_ij = edge_embedding(r0_ij (, r0sc_ij)) with r0 the squared distance of the network's INPUT coordinates (and of the
 * self-conditioning coordinates), the same in every layer.
 *
 * W1 is split by columns, W1 = [W_i | W_j | W_e | w_r]: A = h W_i^T + b1 + W_e b_emb and B = h W_j^T are node-level GEMMs, and since
 * edge_attr is a Linear of one or two scalars its term is r0 u (+ r0sc u'), u = W_e w_emb.  The pre-activation of an edge is
 * A_i + B_j + r0 u (+ r0sc u') + r w_r: nothing of size [E, .] is read or written.  One edge kernel per layer forms it by k-block, applies SiLU
 * and feeds it to the 2 D -> 16 GEMM on the exact fp32 MFMA (K zero-padded to a multiple of 16), runs coors_mlp, and sums m_ij and the
 * coordinate terms per receiver in slot order (j ascending) by one owner: no float atomics, the same bits from run to run and for a molecule
 * whatever else is in the batch.  Molecule sizes are not limited.  One node kernel does the graph-mode LayerNorm (two passes per graph, fixed
 * order; statistics over all rows and features of the graph) and the coordinate add.  The GEMMs are libgcdm_ops.so's own, always exact fp32.
 *
 * Conventions as include/gcdm_ops.h: device pointers, a hipStream_t passed as void*; caller-owned buffers; nothing is allocated, nothing
 * synchronises.  0 on success, -1 for a bad argument (checked before any HIP call; nothing is touched; gcdm_egnn_dyn_last_error() says
 * which), -2 if a launch failed.  Limits: h_hidden (H) a multiple of 32 in 32 .. GCDM_EGNN_DYN_MAX_H, e_hidden (Eh) >= 1 and at most
 * GCDM_EGNN_DYN_MAX_EH, e_in 1 or 2, n_layers >= 1, m_dim = GCDM_EGNN_DYN_M_DIM and the coors_mlp width GCDM_EGNN_DYN_COORS_HIDDEN fixed.
 *
 * gcdm_egnn_dyn_workspace_bytes(which, ...), -1 on a bad argument: 0 the workspace of gcdm_egnn_dyn_layer (256-byte aligned), 1 the packed
 *   weights of all layers, 2 kernel launches per gcdm_egnn_dyn_layer call, 3 the padded K of the edge GEMM (2 D rounded up to 16), 4 LDS bytes
 *   of the edge kernel, 5 receivers per workgroup of the edge kernel.
 *
 * gcdm_egnn_dyn_launches(): edge-kernel launches of this process so far (one per successful gcdm_egnn_dyn_layer call with num_nodes > 0).
 *
 * gcdm_egnn_dyn_pack: `tensors` is a HOST array of `count` = 2 + 15 n_layers device pointers (fp32, contiguous, the reference's shapes):
 *   edge_embedding.weight [Eh, e_in], edge_embedding.bias [Eh]; per layer egnn.mpnn_layers.k.: edge_mlp.0.weight [2D, D], .bias,
 *   edge_mlp.3.weight [16, 2D], .bias, node_norm.weight [H], .bias, coors_norm.scale [1], node_mlp.0.weight [2H, H + 16], .bias,
 *   node_mlp.3.weight [H, 2H], .bias, coors_mlp.0.weight [64, 16], .bias, coors_mlp.3.weight [1, 64], .bias [1].
 *
 * gcdm_egnn_dyn_layer: one layer, `layer` in [0, n_layers).  h_in [N, H], x_in [N, 3] the current coordinates, x0 [N, 3] the network's input
 *   coordinates, xsc [N, 3] the self-conditioning coordinates (e_in = 2; null with e_in = 1), node_offsets int32 [B + 1] (molecule m owns
 *   atoms node_offsets[m] .. node_offsets[m+1] - 1, node_offsets[B] = N), node_mol int32 [N] (the molecule of each atom).  h_out [N, H] and
 *   x_out [N, 3] may not alias the inputs.  A node whose molecule index or offsets are inconsistent has no edges (its sums are zero) and
 *   nothing is read out of bounds for it.  dbg_m [N, 16], dbg_dx [N, 3], dbg_ln [N, H] (each may be null): the two receiver sums and the
 *   LayerNorm output of this layer. */
#ifndef GCDM_EGNN_DYNAMICS_H
#define GCDM_EGNN_DYNAMICS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GCDM_EGNN_DYN_MAX_H 256
#define GCDM_EGNN_DYN_MAX_EH 1024
#define GCDM_EGNN_DYN_M_DIM 16
#define GCDM_EGNN_DYN_COORS_HIDDEN 64
#define GCDM_EGNN_DYN_LAYER_TENSORS 15
#define GCDM_EGNN_DYN_LAUNCHES_PER_LAYER 8

const char* gcdm_egnn_dyn_last_error(void);

int64_t gcdm_egnn_dyn_workspace_bytes(int32_t which, int64_t num_nodes, int32_t h_hidden, int32_t e_hidden, int32_t e_in, int32_t n_layers);

int64_t gcdm_egnn_dyn_launches(void);

int gcdm_egnn_dyn_pack(const void* const* tensors, int32_t count, int32_t h_hidden, int32_t e_hidden, int32_t e_in, int32_t n_layers,
                       float* packed, void* stream);

int gcdm_egnn_dyn_layer(int32_t layer, const float* h_in, const float* x_in, const float* x0, const float* xsc, const int32_t* node_offsets,
                        const int32_t* node_mol, const float* packed, void* workspace, float* h_out, float* x_out, float* dbg_m, float* dbg_dx,
                        float* dbg_ln, int64_t num_nodes, int64_t num_molecules, int32_t h_hidden, int32_t e_hidden, int32_t e_in,
                        int32_t n_layers, void* stream);

#ifdef __cplusplus
}
#endif
#endif
