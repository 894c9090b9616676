/* gcdm_molproc.h -- C ABI of the two graph filters the reference applies to every generated molecule (process_molecule,
 * rdkit_functions.py:323-379: `sanitize` and `largest_frag`), run on a whole flat batch on the device: which molecules and atoms survive, and the
 * survivors as a new flat batch with their bond lists.  Exported from libgcdm_ops.so (gfx950 / MI355X).  Plain C99.
 *
 * Conventions as include/gcdm_molgraph.h: device pointers, a hipStream_t passed as void*; caller-owned buffers; nothing is allocated, nothing
 * synchronises.  0 on success, -1 for a bad argument (checked before any HIP call; nothing is touched), -2 if a launch failed.  No workgroup
 * waits for another; integer work and bit copies only after the pair classification, no float atomics: the results do not depend on the launch
 * geometry.
 *
 * Semantics.  The molecule, its bond orders, its fragments, "largest" and "valid" are exactly those of include/gcdm_molgraph.h: the distance
 * rule with its written-out FMA chain and strict <, limit_bonds_to_one, an atom outside the vocabulary bonding to nothing, valence summed over
 * the WHOLE molecule, ties between fragments of equal size going to the one that holds the lowest atom index.  For a molecule m of n atoms and
 * the flags sanitize (GCDM_MOLPROC_SANITIZE) and largest_frag (GCDM_MOLPROC_LARGEST_FRAG):
 *   dropped      m is dropped iff sanitize is set and m is not valid, or n is outside [0, GCDM_MOLGRAPH_MAX_ATOMS].  A dropped molecule
 *                contributes no atoms, no bonds and no output molecule (the reference appends only molecules that are not None).
 *   kept atoms   a kept molecule keeps all its atoms; with largest_frag those of its largest fragment only.  The reference sanitises the
 *                fragment a second time (:358-363); under the valence-cap rule that cannot fail -- no bond leaves a component, so an atom of
 *                the fragment carries in it the order sum it carries in the molecule, which the first verdict has passed -- and there is no
 *                second verdict here.
 *   order        kept atoms stay in ascending original order and are renumbered 0 .. n' - 1 within the molecule.
 *   bonds        the pairs (i, j), i > j, of order > 0 with both atoms kept, written as (new_i, new_j, order) in row-major order of the
 *                renumbered lower triangle: the order nonzero(tril(E, -1)) gives a whole molecule.  The renumbering is monotone, so it
 *                preserves that order.
 *   n == 0       kept as an empty molecule (max(..., default=mol) in the reference).
 *   no flag      the output is the input: an identity compaction.
 *
 * gcdm_molproc_select -- one workgroup per molecule, then three scan launches (tile totals, one workgroup over the totals, apply):
 *   orders == NULL: the distance rule on x (row stride x_row_stride >= 3 floats); pair_offsets is not read.  Otherwise x is not read and the
 *   orders come in the layout of gcdm_bond_orders, as for gcdm_molgraph_keys_from_orders (only i > j is read).
 *   info      [M, 4] int32   {valid, n_fragments, n_largest, n} as gcdm_molgraph_keys writes it
 *   keep      [N] uint8      1 for a surviving atom, else 0
 *   new_index [N] int32      the atom's index within its output molecule, -1 if it does not survive
 *   counts    [M, 3] int32   {kept atoms, kept bonds, kept molecule as 0 or 1}
 *   totals    [3] int64      {N', nb', M'}: surviving atoms, bonds and molecules of the batch
 *   workspace gcdm_molproc_workspace_bytes(M) bytes, 8-byte aligned; holds the exclusive scans of counts for gcdm_molproc_emit
 *   For n outside [0, GCDM_MOLGRAPH_MAX_ATOMS]: info = {-1, 0, 0, n clamped to int32}, counts = {0, 0, 0}; no atom is read and keep and new_index
 *   of its atoms are not written.  Refused with -1: null tables / totals, num_molecules < 0, tables->bonds.num_types outside 1..16,
 *   a bit of flags beyond the two, x_row_stride < 3 with orders == NULL, and -- when there is a molecule -- any other null pointer that is read
 *   or written.  num_molecules == 0 writes totals = {0, 0, 0} in one launch.
 *
 * The caller reads totals (three integers, one copy: the only synchronisation of the path) and sizes the outputs of
 *
 * gcdm_molproc_emit -- one workgroup per source molecule (it returns at once for a dropped one) and one that closes the offset lists.  Inputs
 *   as given to select, and what select wrote (keep, new_index, counts, totals, workspace).  charges / charges_out: [N] / [N'] elements of
 *   four bytes (fp32 as the sampler holds them, or int32), copied as bits; both NULL when there are none.
 *   pos_out          [N', 3] fp32    bit copies of x[., 0..2]
 *   types_out        [N'] int32      atom_types as given (not mapped)
 *   src_atom         [N'] int64      index of the atom in the source batch
 *   src_molecule     [M'] int64      index of the molecule in the source batch
 *   mol_offsets_out  [M' + 1] int64  first atom of every output molecule; [M'] = N'
 *   bonds_out        [nb', 3] int32  (new_i, new_j, order)
 *   bond_offsets_out [M' + 1] int64  first bond of every output molecule; [M'] = nb'
 *   x is read in both entries (positions are gathered even when the orders are given): x_row_stride >= 3 always.  Every output pointer must be
 *   non-null even when its array is empty. */
#ifndef GCDM_MOLPROC_H
#define GCDM_MOLPROC_H
#include <stdint.h>
#include "gcdm_molgraph.h"
#ifdef __cplusplus
extern "C" {
#endif

#define GCDM_MOLPROC_SANITIZE     1
#define GCDM_MOLPROC_LARGEST_FRAG 2
#define GCDM_MOLPROC_SCAN_TILE    256    /* molecules per workgroup of the scan launches */

int64_t gcdm_molproc_workspace_bytes(int64_t num_molecules);   /* < 0 for num_molecules < 0 */

int gcdm_molproc_select(const GcdmMolGraphTables* tables, const float* x, int64_t x_row_stride, const int32_t* atom_types,
                        const int64_t* mol_offsets, int64_t num_molecules, const int64_t* pair_offsets, const uint8_t* orders, int32_t flags,
                        int32_t* info, uint8_t* keep, int32_t* new_index, int32_t* counts, int64_t* totals, void* workspace, void* stream);

int gcdm_molproc_emit(const GcdmMolGraphTables* tables, const float* x, int64_t x_row_stride, const int32_t* atom_types, const void* charges,
                      const int64_t* mol_offsets, int64_t num_molecules, const int64_t* pair_offsets, const uint8_t* orders,
                      const uint8_t* keep, const int32_t* new_index, const int32_t* counts, const int64_t* totals, const void* workspace,
                      float* pos_out, int32_t* types_out, void* charges_out, int64_t* src_atom, int64_t* src_molecule,
                      int64_t* mol_offsets_out, int32_t* bonds_out, int64_t* bond_offsets_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
