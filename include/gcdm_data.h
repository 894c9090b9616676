/* gcdm_data.h -- C ABI of the device-resident molecule data set: training batches built in HBM, the property histograms of conditional
 * sampling and the context draw, exported from libgcdm_ops.so (gfx950 / MI355X).  Plain C99.
 *
 * Conventions as include/gcdm_ops.h: device pointers, a hipStream_t passed as void*; caller-owned buffers; nothing is allocated, nothing
 * synchronises.  0 on success, -1 for a bad argument (checked before any HIP call; nothing is touched), -2 if a launch failed.  Empty work
 * returns 0 without a launch.
 *
 * The data set on the device (ragged, written once; gcdm_data_set): molecule m owns atoms atom_ptr[m] .. atom_ptr[m+1] - 1 of z (atomic
 * numbers, present atoms only) and pos; props[p][m] is property p of molecule m; species[t] is the atomic number of one-hot column t;
 * norm[p] = (mean, mad) of property p; index[m] is the molecule's index in the source files.
 *
 * gcdm_data_collate builds batch molecules perm[first] .. perm[first + B - 1] in two launches (an offset scan, then one workgroup per
 * molecule).  pad_to = 0: the compact layout, a molecule takes its n_b rows.  pad_to > 0: every molecule takes pad_to rows, the rows behind
 * its atoms are masked (mask 0, zero positions, one-hot, charge and context).  The host supplies N (rows) and E = sum n_b^2 from its mirror
 * of the sizes; the kernels derive every offset themselves and write nothing outside [0, N) / [0, E): when the sizes on the device do not add
 * up to N and E, when a permutation entry is outside [0, M) or a molecule has more than pad_to atoms, GCDM_DATA_FLAG_ACCOUNT is raised in
 * `flags` (which the kernels only ever OR into) and the batch is not to be used.  Every element of every output is written:
 *   x [N][3], one_hot [N][T], charges [N] (the atomic number as float), batch int64 [N], mask uint8 [N], index int64 [B],
 *   num_nodes_present int64 [B], props [P][B], props_context [N][C] = mask * (props[ctx_cols[c]][m] - mean) / mad (fp32, correctly
 *   rounded, no contraction; null with C = 0),
 *   edge_index int64 [2][E]: per molecule all ordered pairs of its present atoms, self-loops included, row-major (sorted by row),
 *   rowptr int32 [N+1], colperm int64 [E] (the stable argsort of edge_index[1]), colptr int32 [N+1]: with o_b / eoff_b the first row / edge
 *   of molecule b, edge (o_b + i, o_b + j) sits at eoff_b + i n_b + j and colperm[eoff_b + j n_b + i] names it.
 * workspace: gcdm_data_workspace_bytes(B) bytes, 256-byte aligned.
 *
 * gcdm_data_prop_histogram (one launch): for molecule sizes n = 0 .. num_sizes - 1 (rows of the tables) the member count, (min, max) of the
 * members' values (0, 0 without members) and counts[n][k], k = int((v - min) / (max - min + 1e-12) * num_bins) in fp32 with num_bins folded
 * into num_bins - 1.  A molecule of num_sizes or more atoms is a bad data set: GCDM_DATA_FLAG_ACCOUNT.
 *
 * gcdm_data_prop_sample (one launch): out[b][p] for sizes num_nodes[b] from P stacked tables and uniforms u [B][P][2] in [0, 1):
 * k = min(floor(u1 count), count - 1), bin i = the first whose cumulative count exceeds k, left = i / num_bins * (max - min) + min,
 * right likewise from i + 1, value = u2 (right - left) + left, out = (value - mean) / mad.  A size outside the tables or without members:
 * out = NaN and GCDM_DATA_FLAG_ABSENT_SIZE. */
#ifndef GCDM_DATA_H
#define GCDM_DATA_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GCDM_DATA_MAX_TYPES 16
#define GCDM_DATA_MAX_PROPS 32
#define GCDM_DATA_MAX_SIZES 2048
#define GCDM_DATA_MAX_BINS 65536
#define GCDM_DATA_FLAG_ABSENT_SIZE 1
#define GCDM_DATA_FLAG_ACCOUNT 2

typedef struct gcdm_data_set {
    const int64_t* atom_ptr; /* [M + 1] */
    const int32_t* z;        /* [A] */
    const float* pos;        /* [A][3] */
    const float* props;      /* [P][M] */
    const int32_t* species;  /* [T] */
    const float* norm;       /* [P][2] */
    const int64_t* index;    /* [M] */
    int64_t M, A;
    int32_t P, T;
} gcdm_data_set;

typedef struct gcdm_data_batch {
    float* x;
    float* one_hot;
    float* charges;
    int64_t* batch;
    uint8_t* mask;
    int64_t* index;
    int64_t* num_nodes_present;
    float* props;
    float* props_context;
    int64_t* edge_index;
    int32_t* rowptr;
    int64_t* colperm;
    int32_t* colptr;
} gcdm_data_batch;

int64_t gcdm_data_workspace_bytes(int64_t B);

int gcdm_data_collate(const gcdm_data_set* set, const int64_t* perm, int64_t perm_len, int64_t first, int64_t B, int32_t pad_to,
                      const int32_t* ctx_cols, int32_t C, int64_t N, int64_t E, void* workspace, const gcdm_data_batch* out, int32_t* flags,
                      void* stream);

int gcdm_data_prop_histogram(const int64_t* atom_ptr, const float* values, int64_t M, int32_t num_sizes, int32_t num_bins, int32_t* counts,
                             float* params, int32_t* members, int32_t* flags, void* stream);

int gcdm_data_prop_sample(const int32_t* counts, const float* params, const int32_t* members, const float* norm, const int64_t* num_nodes,
                          const float* u, int64_t B, int32_t P, int32_t num_sizes, int32_t num_bins, float* out, int32_t* flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif
