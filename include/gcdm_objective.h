/* gcdm_objective.h -- C ABI of the fused diffusion objective for training and validation, exported from libgcdm_ops.so (gfx950 / MI355X).
 * Plain C99.
 *
 * Everything EquivariantVariationalDiffusion does around its network evaluation (variational_diffusion.py:948-1160 and the tail of
 * qm9_mol_gen_ddpm.py:184-252): normalisation, the gamma look-ups, alpha / sigma, the CoM projection of the noise, z_t; the prior KL, the
 * constants, error_t, log p(x, h | z_0), the L2 / VLB weighting, the batch means; and d net_out.  Three launches forward (prepare, terms,
 * reduce) and one backward, fp32 throughout with the full-precision erff / logf / expf / sqrtf, no float atomics, no scratch.
 *
 * Conventions as include/gcdm_ops.h: device pointers unless stated, a hipStream_t passed as void*; caller-owned buffers; nothing is allocated,
 * nothing synchronises.  0 on success, -1 for a bad argument (checked before any HIP call; nothing is touched), -2 if a launch failed.
 * EVERY INPUT IS READ-ONLY.  Bad arguments: B < 1, N < 1, N * D >= 2^31, num_atom_types outside 1 .. GCDM_OBJECTIVE_MAX_TYPES,
 * include_charges outside {0, 1}, T < 1, a mode other than the three below, pn_len < 1, a null pointer that the mode needs.
 *
 * Sizes and layouts (row-major fp32 unless stated):
 *   N nodes, B >= 1 molecules, D = 3 + num_atom_types + include_charges columns.  Molecules are contiguous in node order; molecule b owns
 *   rows node_offsets[b] .. node_offsets[b+1]-1 (int32 [B+1], what gcdm_op_rowptr makes of a non-decreasing batch_index; offsets are
 *   clamped to [0, N] before use).  Every molecule has >= 1 row (sizes 1 .. 181 and beyond work) and >= 1 unmasked row; a molecule
 *   without an unmasked row raises GCDM_OBJECTIVE_FLAG_EMPTY and its projected noise is NaN as on the torch path.
 *   x [N,3]; one_hot [N,num_atom_types]; charges [N] (NULL allowed when include_charges = 0); mask uint8 [N], 0 = masked, NULL = all
 *   present; t_int int32 [B] in 0 .. T (outside: GCDM_OBJECTIVE_FLAG_T_RANGE, clamped); gamma [T+1]; log_pn [pn_len]: log p(size), NaN
 *   for a size the histogram does not have; norm_values / norm_biases: HOST float[3]; eps_raw, eps_raw_0 [N,D]: raw standard-normal draws.
 *
 * mode: GCDM_OBJECTIVE_TRAIN_VLB (0), GCDM_OBJECTIVE_EVAL (1), GCDM_OBJECTIVE_TRAIN_L2 (2).
 *
 * Determinism: one wave per molecule loops over its rows; lane l adds rows l, l + 64, ... in order, then the 64 lane sums are combined by a
 * fixed butterfly.  The order depends on the molecule's size alone, so a molecule's rows and terms are the same bits alone, at any
 * position of any batch, and from run to run.  (The batch means of gcdm_objective_reduce depend on B.)
 *
 * gcdm_objective_workspace_bytes(N, B, D, mode): bytes of `workspace` (256-byte aligned), written by gcdm_objective_reduce and read by
 *   gcdm_objective_bwd: float [B][2] = d nll_b / d error_t_b, d nll_b / d loss_0_x_b.  -1 for a bad argument.
 *
 * gcdm_objective_prepare -- one launch.  Gamma indices as PredefinedNoiseSchedule.forward: rint((float)t_int / (float)T * (float)T), ties to
 *   even; the s index of t_int = 0 is -1 and wraps to gamma[T] as Python indexing does.  center_x = 1 first subtracts from the unmasked rows
 *   of x the molecule's sum over ALL rows divided by its number of unmasked rows (centralize(..., edm=True)); center_x = 0 takes x as
 *   CoM-free.  Written in every mode:
 *     xh [N,D]      x / nv0 | (one_hot - nb1) / nv1 * m | (charges - nb2) / nv2 * m
 *     eps_t [N,D]   eps_raw * m, its x part minus the molecule's mean over unmasked rows (times m)
 *     z_t [N,D]     alpha_t xh + sigma_t eps_t
 *     t_node [N]    (float)t_int / (float)T of the row's molecule (the network's time input)
 *     mol [B][8]    0 delta_log_px, 1 neg_log_constants, 2 kl_prior (both Gaussian KLs against gamma[T]), 3 SNR_weight =
 *                   exp(-(gamma_s - gamma_t)) - 1, 4 t_is_zero, 5 num_nodes_present, 6 log_pN (NaN and GCDM_OBJECTIVE_FLAG_SIZE for a size
 *                   the table does not have), 7 gamma_t
 *     flags         int32 [1], OR-ed into (never cleared here): GCDM_OBJECTIVE_FLAG_*; bit 0 is gcdm_op_rowptr's "not sorted"
 *   and with GCDM_OBJECTIVE_EVAL only (NULL allowed otherwise, eps_raw_0 too): eps_0 [N,D] from eps_raw_0, z_0 [N,D] = alpha_0 xh + sigma_0 eps_0.
 *
 * gcdm_objective_terms -- one launch.  Reads net_out [N,D] (and net_out_0 [N,D] with GCDM_OBJECTIVE_EVAL) and what prepare wrote; writes
 *   terms [B][10] = 0 delta_log_px, 1 error_t, 2 SNR_weight, 3 loss_0_x, 4 loss_0_h, 5 neg_log_constants, 6 kl_prior, 7 log_pN,
 *   8 eps_hat_x, 9 eps_hat_h (the molecule's mean over ALL its rows of mean_j |net_out|, x columns / other columns).
 *     error_t   = sum over ALL rows and all columns of (eps_t - net_out)^2 (eps_t is zero on a masked row, net_out is not: the reference
 *                 sums the squared output of its scalar projection there too, variational_diffusion.py:1052)
 *     loss_0_x  = 0.5 sum over unmasked rows of the x columns of (eps - net)^2
 *     loss_0_h  = -log p(h | z_0): per unmasked row, log(cdf((c + .5) / w) - cdf((c - .5) / w) + 1e-10) per atom type with c = z nv1 + nb1 - 1,
 *                 w = sigma_0 nv1, minus its logsumexp over the types, weighted by xh nv1 + nb1; plus, with charges, the same mass at
 *                 c = rint(xh nv2 + nb2) - (z nv2 + nb2), w = sigma_0 nv2
 *   training modes: (eps, net, z, sigma_0) = (eps_t, net_out, z_t, sigma_t); error_t is multiplied by 1 - t_is_zero, loss_0_x and loss_0_h by
 *   t_is_zero.  GCDM_OBJECTIVE_EVAL: (eps_0, net_out_0, z_0, sigma(gamma[0])), no t_is_zero factors.  GCDM_OBJECTIVE_TRAIN_L2 writes
 *   delta_log_px = neg_log_constants = 0 and SNR_weight = 1.  (The x columns of the network's output are zero at masked rows, so loss_0_x over
 *   unmasked rows is the torch path's sum over all rows.)
 *
 * gcdm_objective_reduce -- one launch of one workgroup.  nll [B] = loss_t + loss_0 + kl_prior - delta_log_px - log_pN with
 *   GCDM_OBJECTIVE_TRAIN_L2: loss_t = 0.5 error_t / den, loss_0 = loss_0_x / den + loss_0_h, den = D * (norm_by_max_nodes ? max_b
 *   num_nodes_present : num_nodes_present_b); otherwise loss_t = T * 0.5 * SNR_weight * error_t, loss_0 = loss_0_x + loss_0_h + neg_log_constants.
 *   means [16]: 0 mean nll (the loss), 1 loss_t, 2 SNR_weight, 3 loss_0, 4 kl_prior, 5 delta_log_px, 6 neg_log_constants, 7 log_pN,
 *   8 eps_hat_x, 9 eps_hat_h (batch means), 10 .. 15 zero.  Writes `workspace`.
 *
 * gcdm_objective_bwd -- one launch, element-wise, training modes only.  g_error_t, g_loss_0_x, g_nll [B] and g_loss [1] are the upstream
 *   gradients of terms columns 1 and 3, of nll and of means[0]; each may be NULL (= zero).  The three [B] gradients are read at
 *   g[b * stride] with an element stride >= 0 (1 = dense, 0 = one value for every molecule: what the backward of a mean hands over).
 *   Rows outside every molecule (node_offsets that do not cover 0 .. N) are not written.  With G = g_nll_b + g_loss / B:
 *     d_net_out[i][j] = ( -2 (1 - t_is_zero) (g_error_t_b + G ct_b) - m_i [j < 3] t_is_zero (g_loss_0_x_b + G c0_b) ) (eps_t - net_out)[i][j]
 *   with (ct, c0) from `workspace`.  Masked rows get the error_t part only. */
#ifndef GCDM_OBJECTIVE_H
#define GCDM_OBJECTIVE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GCDM_OBJECTIVE_MAX_TYPES 16
#define GCDM_OBJECTIVE_TRAIN_VLB 0
#define GCDM_OBJECTIVE_EVAL 1
#define GCDM_OBJECTIVE_TRAIN_L2 2
#define GCDM_OBJECTIVE_FLAG_UNSORTED 1
#define GCDM_OBJECTIVE_FLAG_SIZE 2
#define GCDM_OBJECTIVE_FLAG_T_RANGE 4
#define GCDM_OBJECTIVE_FLAG_EMPTY 8

int64_t gcdm_objective_workspace_bytes(int64_t N, int64_t B, int32_t D, int32_t mode);

int gcdm_objective_prepare(const float* x, const float* one_hot, const float* charges, const uint8_t* mask, const int32_t* node_offsets,
                           const int32_t* t_int, const float* gamma, const float* log_pn, int32_t pn_len, const float* norm_values,
                           const float* norm_biases, const float* eps_raw, const float* eps_raw_0, float* xh, float* eps_t, float* z_t,
                           float* eps_0, float* z_0, float* t_node, float* mol, int32_t* flags, int64_t N, int64_t B, int32_t num_atom_types,
                           int32_t include_charges, int32_t T, int32_t mode, int32_t center_x, void* stream);

int gcdm_objective_terms(const float* net_out, const float* net_out_0, const float* xh, const float* eps_t, const float* z_t, const float* eps_0,
                         const float* z_0, const uint8_t* mask, const int32_t* node_offsets, const float* mol, const float* gamma,
                         const float* norm_values, const float* norm_biases, float* terms, int64_t N, int64_t B, int32_t num_atom_types,
                         int32_t include_charges, int32_t T, int32_t mode, void* stream);

int gcdm_objective_reduce(const float* mol, const float* terms, void* workspace, float* nll, float* means, int64_t B, int32_t D, int32_t T,
                          int32_t mode, int32_t norm_by_max_nodes, void* stream);

int gcdm_objective_bwd(const float* g_error_t, int64_t stride_error_t, const float* g_loss_0_x, int64_t stride_loss_0_x, const float* g_nll,
                       int64_t stride_nll, const float* g_loss, const float* net_out, const float* eps_t, const uint8_t* mask, const int32_t* node_offsets, const float* mol, const void* workspace,
                       float* d_net_out, int64_t N, int64_t B, int32_t D, int32_t mode, void* stream);

#ifdef __cplusplus
}
#endif
#endif
