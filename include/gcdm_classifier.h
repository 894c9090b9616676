/* gcdm_classifier.h -- C ABI of the EGNN property classifier (forward only, evaluation mode), exported from libgcdm_ops.so (gfx950 / MI355X).
 * Plain C99.
 *
 * The network is the reference's src/__init__.py EGNN of E_GCL_mask layers: h = embedding(h0); per layer and per pair (i, j), i != j, of one
 * molecule m_ij = silu(W2 silu(W1 [h_i | h_j | |x_i - x_j|^2] + b1) + b2), with attention m_ij *= sigmoid(w_a m_ij + b_a); agg_i = sum_j m_ij;
 * h_i += node_mlp([h_i | agg_i | h0_i if node_attr]); pred = graph_dec(sum_i node_dec(h_i)).  Coordinates are never updated.
 *
 * One forward is ONE launch: a workgroup carries its molecules through the whole network.  fp32 throughout on the exact fp32 MFMA, no float
 * atomics: a molecule's prediction is bit-identical from run to run, whatever else is in the batch and wherever it sits in it.
 *
 * Conventions as include/gcdm_ops.h: device pointers, a hipStream_t passed as void*; caller-owned buffers; nothing is allocated, nothing
 * synchronises.  0 on success, -1 for a bad argument (checked before any HIP call; nothing is touched; gcdm_classifier_last_error() says
 * which), -2 if a launch failed.  Limits: in_node_nf 1 .. GCDM_CLASSIFIER_MAX_IN_NODE_NF, hidden_nf a multiple of 32 up to
 * GCDM_CLASSIFIER_MAX_HIDDEN_NF, n_layers >= 1, 0 .. GCDM_CLASSIFIER_MAX_NODES atoms per molecule.
 *
 * gcdm_classifier_workspace_bytes(which, ...): 0 the forward's workspace (256-byte aligned; h of every atom), 1 the packed weights,
 *   2 launches per forward, 3 LDS bytes per workgroup, 4 molecules per workgroup.
 *
 * gcdm_classifier_pack: `tensors` is a HOST array of `count` = 2 + 10 n_layers + 8 device pointers (fp32, contiguous, the reference's shapes):
 *   embedding.weight, embedding.bias; per layer k: gcl_k.edge_mlp.0.weight [H, 2H+1], .bias, gcl_k.edge_mlp.2.weight, .bias,
 *   gcl_k.node_mlp.0.weight [H, 2H (+F with node_attr)], .bias, gcl_k.node_mlp.2.weight, .bias, gcl_k.att_mlp.0.weight [1, H], .bias [1] (both
 *   null without attention); node_dec.0.weight, .bias, node_dec.2.weight, .bias, graph_dec.0.weight, .bias, graph_dec.2.weight [1, H], .bias [1].
 *
 * gcdm_classifier_forward: x [N, 3], h0 [N, F], node_offsets int32 [B + 1] (molecule m owns atoms node_offsets[m] .. node_offsets[m+1] - 1;
 *   node_offsets[B] <= N), pred [B].  A molecule whose offsets are out of order, out of [0, N] or more than GCDM_CLASSIFIER_MAX_NODES apart
 *   gets pred = NaN (with the other molecules of its workgroup) and nothing of it is read or written.  A molecule of one atom has no edges
 *   (agg = 0), one of zero atoms is graph_dec(0).  debug_layer = -1: none; 0: h after the embedding, k: h after layer k, copied to h_debug [N, H]. */
#ifndef GCDM_CLASSIFIER_H
#define GCDM_CLASSIFIER_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GCDM_CLASSIFIER_MAX_NODES 32
#define GCDM_CLASSIFIER_MAX_IN_NODE_NF 16
#define GCDM_CLASSIFIER_MAX_HIDDEN_NF 256

const char* gcdm_classifier_last_error(void);

int64_t gcdm_classifier_workspace_bytes(int32_t which, int64_t num_nodes, int32_t in_node_nf, int32_t hidden_nf, int32_t n_layers);

int gcdm_classifier_pack(const void* const* tensors, int32_t count, int32_t in_node_nf, int32_t hidden_nf, int32_t n_layers, int32_t attention,
                         int32_t node_attr, float* packed, void* stream);

int gcdm_classifier_forward(const float* x, const float* h0, const int32_t* node_offsets, const float* packed, void* workspace, float* pred,
                            float* h_debug, int32_t debug_layer, int64_t num_nodes, int64_t num_molecules, int32_t in_node_nf, int32_t hidden_nf,
                            int32_t n_layers, int32_t attention, void* stream);

#ifdef __cplusplus
}
#endif
#endif
