/* gcdm_geom.h -- C ABI of the GEOM-Drugs conformer file on the device: the rows of GEOM_drugs_30.npy are segmented into molecules in HBM, chunk
 * by chunk, and the molecules are reordered into the size-sorted splits.  Exported from libgcdm_ops.so (gfx950 / MI355X).  Plain C99.
 *
 * Conventions as include/gcdm_data.h: device pointers, a hipStream_t passed as void*; caller-owned buffers; nothing is allocated, nothing
 * synchronises.  0 on success, -1 for a bad argument (checked before any HIP call; nothing is touched), -2 if a launch failed.  Empty work
 * returns 0 without a launch.  `flags` is a device word the kernels only ever OR into.  No float atomics; every result is independent of
 * the launch geometry and of how the file was cut into chunks.
 *
 * The file (build_geom_dataset.py: extract_conformers / load_split_data): float64 rows [R][5] = molecule id, atomic number, x, y, z.
 *
 * gcdm_geom_ingest takes one chunk of consecutive rows and appends to z int32 [cap_atoms], pos float [cap_atoms][3] and atom_ptr int64
 * [cap_mols + 1].  `state` is GCDM_GEOM_STATE_WORDS int64 on the device, zeroed by the caller before the first chunk and owned by the
 * kernels afterwards: the id of the last kept row, the atoms appended, the molecules opened (the fourth word is reserved).  Consecutive
 * chunks therefore need no host round trip.  Row for row:
 *   - a row is dropped iff remove_h and its atomic-number column == 1.0 (the float comparison, before any truncation: 1.5 is kept);
 *   - z = the column truncated toward zero, pos = the float64 coordinates rounded to nearest-even fp32;
 *   - the id is the id column truncated toward zero; a molecule starts at the first kept row and wherever the id of a kept row differs
 *     from the id of the kept row before it (ids need not increase), so a conformer that loses every atom to remove_h disappears and its
 *     neighbours join if their ids are equal, as when the rows are deleted from the file;
 *   - atom_ptr[m] = the atom slot of the first row of molecule m;
 *   - GCDM_GEOM_FLAG_BAD_ROW: z < 1 after truncation, or a value of a kept row that is not finite (z and the id are then 0).  The row is
 *     still written;
 *   - GCDM_GEOM_FLAG_CAPACITY: an atom slot >= cap_atoms or a molecule ordinal >= cap_mols.  Such an element is counted and not written.
 * Launches per chunk: tile totals (one workgroup per tile of GCDM_GEOM_TILE rows), one workgroup that scans the totals behind the state and
 * advances the state, then the tiles again to write.  No workgroup waits for another.
 * workspace: gcdm_geom_workspace_bytes(GCDM_GEOM_WS_BYTES, R) bytes, 256-byte aligned; its contents mean nothing between calls.
 *
 * gcdm_geom_finish (one launch) closes the last molecule: atom_ptr[M] = A when M <= cap_mols (GCDM_GEOM_FLAG_CAPACITY otherwise), and
 * MA[0] = M, MA[1] = A, the totals counted whether or not they fit.
 *
 * gcdm_geom_gather (one launch, one wave per molecule): molecule k of the output is molecule order[k] of the input; its atoms go to
 * atom_ptr_out[k] .. atom_ptr_out[k + 1] - 1, consecutive lanes copying consecutive atoms.  The caller scans the reordered sizes into
 * atom_ptr_out.  An order entry outside [0, M_in), source atoms outside [0, A_in) or a size that differs between atom_ptr_out and the
 * source raises GCDM_GEOM_FLAG_ACCOUNT and the molecule is skipped; a destination outside [0, A_out) raises it too, and every store is
 * guarded by A_out.
 *
 * gcdm_geom_workspace_bytes(which, R): GCDM_GEOM_WS_BYTES the workspace of an R-row chunk, GCDM_GEOM_WS_LAUNCHES the launches of such a
 * chunk (0 for R = 0), GCDM_GEOM_WS_TILE the rows per scan tile; -1 for a bad argument. */
#ifndef GCDM_GEOM_H
#define GCDM_GEOM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GCDM_GEOM_TILE 1024
#define GCDM_GEOM_STATE_WORDS 4
#define GCDM_GEOM_MAX_ROWS 2147483647
#define GCDM_GEOM_FLAG_BAD_ROW 1
#define GCDM_GEOM_FLAG_CAPACITY 2
#define GCDM_GEOM_FLAG_ACCOUNT 4
#define GCDM_GEOM_WS_BYTES 0
#define GCDM_GEOM_WS_LAUNCHES 1
#define GCDM_GEOM_WS_TILE 2

int64_t gcdm_geom_workspace_bytes(int32_t which, int64_t R);

int gcdm_geom_ingest(const double* rows, int64_t R, int32_t remove_h, int64_t* state, int32_t* z, float* pos, int64_t* atom_ptr,
                     int64_t cap_atoms, int64_t cap_mols, void* workspace, int32_t* flags, void* stream);

int gcdm_geom_finish(const int64_t* state, int64_t* atom_ptr, int64_t cap_mols, int64_t* MA, int32_t* flags, void* stream);

int gcdm_geom_gather(const int64_t* atom_ptr_in, const int32_t* z_in, const float* pos_in, int64_t M_in, int64_t A_in, const int64_t* order,
                     const int64_t* atom_ptr_out, int64_t M_out, int64_t A_out, int32_t* z_out, float* pos_out, int32_t* flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif
