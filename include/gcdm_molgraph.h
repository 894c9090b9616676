/* gcdm_molgraph.h -- C ABI of the per-molecule graph kernel behind validity, uniqueness and novelty of samples without RDKit: for every
 * molecule of a flat batch the valence-cap verdict, its fragments and a permutation-invariant 64-bit key of its largest fragment.
 * Exported from libgcdm_ops.so (gfx950 / MI355X).  Plain C99.
 *
 * Conventions as include/gcdm_geom.h: device pointers, a hipStream_t passed as void*; caller-owned buffers; nothing is allocated, nothing
 * synchronises.  0 on success, -1 for a bad argument (checked before any HIP call; nothing is touched), -2 if a launch failed.  Refused with
 * -1: a null `tables`, num_molecules < 0, x_row_stride < 3, tables->bonds.num_types outside 1..16, and -- when there is a molecule -- any
 * other null pointer.  num_molecules == 0 returns 0 without a launch.  One launch (one more per 2^30 molecules), one workgroup per molecule,
 * no workgroup waits for another; integer work only after the pair classification, so the results do not depend on the launch geometry.
 *
 * The molecule is the labelled graph the reference builds in make_mol_edm (rdkit_functions.py:276-320): element per atom, bond order per pair,
 * no charges, no aromatic flags.  Molecule m owns atoms mol_offsets[m] .. mol_offsets[m + 1] - 1 (int64, ascending), n of them.
 *
 * Bond orders.  gcdm_molgraph_keys classifies the pairs (i, j), i > j, with the arithmetic of gcdm_check_stability (include/gcdm_hip.h):
 * d = 100 * sqrtf(fma(dz, dz, fma(dy, dy, dx * dx))) in fp32 with a correctly rounded root, differences taken as atom i minus atom j, order k
 * when d < thrK[type_i * 16 + type_j] strictly, later k overwriting earlier ones, limit_bonds_to_one folding 2 and 3 to 1; the order of (j, i)
 * is that of (i, j).  gcdm_molgraph_keys_from_orders reads them instead from the layout of gcdm_bond_orders: an n x n uint8 block at
 * orders[pair_offsets[m] ..]; only the entries (i, j) with i > j are read (torch.tril(E, -1) in the reference) and taken as they are.
 *
 * Types.  atom_types holds vocabulary indices, or, with types_are_atomic_numbers = 1, atomic numbers that are mapped through atomic_number[]
 * (the first match among the num_types entries).  An index outside [0, num_types), or an atomic number without a match, is an atom outside the
 * vocabulary: it bonds to nothing (in the second entry its orders are ignored), makes the molecule invalid and enters the key with Z = 0.
 *
 * Per molecule, info[m] = {valid, n_fragments, n_largest, n}:
 *   fragments   the connected components over pairs of order > 0.  The largest is chosen, among equal sizes the one holding the lowest atom
 *               index (what max(frags, key=GetNumAtoms) picks);
 *   valid       1 iff every atom is inside the vocabulary and every atom's orders, summed over the WHOLE molecule, are <= valence_cap of
 *               its type (a cap < 0 is no cap); the reference sanitises before it fragments;
 *   n == 0      valid = 1, n_fragments = 0, n_largest = 0 and the key of an empty fragment;
 *   n outside [0, GCDM_MOLGRAPH_MAX_ATOMS]   info = {-1, 0, 0, n clamped to int32}, key = 0; no atom is read.
 * The key is computed whether or not the molecule is valid.
 *
 * The key.  Arithmetic mod 2^64; mix is the splitmix64 finaliser (x ^= x >> 30, x *= 0xBF58476D1CE4E5B9, x ^= x >> 27,
 * x *= 0x94D049BB133111EB, x ^= x >> 31).  F: the largest fragment, m atoms; d(i, j): the hop distance inside F; Z: the atomic number;
 * o(i, j): the bond order.
 *   c0(i)      = mix( Z_i * K1 + sum_{j in F, j != i} mix( (d(i, j) << 8 | Z_j) + K2 ) )
 *   c_{r+1}(i) = mix( c_r(i) * K3 + sum_{j: o(i, j) > 0} mix( c_r(j) + o(i, j) * K4 ) ),   r = 0 .. GCDM_MOLGRAPH_ROUNDS - 1
 *   key        = mix( m * K5 + sum_{i in F} mix( c_ROUNDS(i) ) )
 * Every sum is commutative: the key does not depend on the order of the atoms.  It is a hash, not a canonical form: equal graphs have equal
 * keys, different graphs have different keys up to collisions of a 64-bit value. */
#ifndef GCDM_MOLGRAPH_H
#define GCDM_MOLGRAPH_H
#include <stdint.h>
#include "gcdm_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define GCDM_MOLGRAPH_MAX_ATOMS 192      /* GEOM-Drugs' max_n_nodes is 181 */
#define GCDM_MOLGRAPH_ROUNDS    16
#define GCDM_MOLGRAPH_K1 0x9E3779B97F4A7C15ULL
#define GCDM_MOLGRAPH_K2 0xC2B2AE3D27D4EB4FULL
#define GCDM_MOLGRAPH_K3 0x165667B19E3779F9ULL
#define GCDM_MOLGRAPH_K4 0xD6E8FEB86659FD93ULL
#define GCDM_MOLGRAPH_K5 0xA0761D6478BD642FULL

typedef struct GcdmMolGraphTables {
    GcdmBondTables bonds;                /* as for gcdm_check_stability (include/gcdm_hip.h) */
    int32_t atomic_number[16];           /* per type of the vocabulary */
    int32_t valence_cap[16];             /* an atom whose bond orders sum to more makes the molecule invalid; < 0 = no cap */
    int32_t types_are_atomic_numbers;    /* 1: atom_types holds Z (MoleculeDataset.z); mapped through atomic_number[], no match = outside the vocabulary */
} GcdmMolGraphTables;

int gcdm_molgraph_keys(const GcdmMolGraphTables* tables, const float* x, int64_t x_row_stride, const int32_t* atom_types,
                       const int64_t* mol_offsets, int64_t num_molecules, int64_t* keys, int32_t* info, void* stream);

int gcdm_molgraph_keys_from_orders(const GcdmMolGraphTables* tables, const int32_t* atom_types, const int64_t* mol_offsets, int64_t num_molecules,
                                   const int64_t* pair_offsets, const uint8_t* orders, int64_t* keys, int32_t* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif
