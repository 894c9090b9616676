// gcdm_ops.molproc.hip.h -- process_molecule's two graph filters on a flat batch (include/gcdm_molproc.h): select, scan, emit.
//
//   select   k_molgraph<., SELECT = true> (gcdm_ops.molgraph.hip.h): its steps 1-4, then keep bytes, new local indices and the three counts
//            per molecule in place of the key rounds.
//   scan     exclusive scans of the three counts over the molecules as plain launches, the scheme of gcdm_ops.geom.hip.h:
//              k_molproc_totals   one workgroup per tile of SCAN_TILE molecules: the tile's three sums;
//              k_molproc_scan     one workgroup: the exclusive scan of the tile sums, SCAN_TILE tiles at a time behind a running carry; the
//                                 carry at the end is totals = {N', nb', M'};
//              k_molproc_apply    one workgroup per tile: the scan inside the tile behind the tile's prefix -> one offset triple per molecule.
//            Each launch reads only what an earlier launch wrote: no workgroup waits for another.
//   emit     one workgroup per source molecule; a dropped one returns at once.  Steps 1 and 2 of k_molgraph again through the same device
//            functions (gmg::load_atoms, gmg::fill_orders -> gmg::pair_order: the orders emit writes are the orders select judged), then the
//            gather of the kept atoms to the scanned offsets and the bond triples: thread i counts the kept bonds of row i, an exclusive scan
//            of the row counts in LDS places the row, and the thread walks its row in ascending j -- row-major order of the renumbered lower
//            triangle.  ~41 KB of LDS (the order bytes are 37 KB of it), under k_molgraph's.  One more workgroup closes the two offset lists.
// Integer work and bit copies; no atomics in global memory.  Every store of emit is guarded by the counts select wrote, so the two cannot
// disagree into memory that is not theirs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/gcdm_molproc.h"
#include "gcdm_ops.molgraph.hip.h"

namespace gmp {

using gmg::MAXA;
using gmg::LD;
using gmg::THREADS;
constexpr int SCAN_TILE = GCDM_MOLPROC_SCAN_TILE;
static_assert(SCAN_TILE == THREADS, "one molecule per thread of a scan workgroup");

inline int64_t ntiles(int64_t M) { return (M + SCAN_TILE - 1) / SCAN_TILE; }

// exclusive scan of three int64 per thread over the workgroup (Hillis-Steele in LDS); total[c] = the sum over all threads.  sh is free on return.
__device__ inline void block_scan3(const int64_t v[3], int64_t ex[3], int64_t total[3], int64_t (*sh)[SCAN_TILE]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) sh[c][t] = v[c];
    __syncthreads();
    for (int d = 1; d < SCAN_TILE; d <<= 1) {
        int64_t add[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) add[c] = t >= d ? sh[c][t - d] : 0;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) sh[c][t] += add[c];
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { ex[c] = sh[c][t] - v[c]; total[c] = sh[c][SCAN_TILE - 1]; }
    __syncthreads();
}

__device__ inline void load_counts(const int32_t* __restrict__ counts, int64_t m, int64_t M, int64_t v[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = m < M ? (int64_t)counts[3 * m + c] : 0;
}

__global__ __launch_bounds__(SCAN_TILE) void k_molproc_totals(const int32_t* __restrict__ counts, int64_t M, int64_t* __restrict__ tile_total) {
    __shared__ int64_t sh[3][SCAN_TILE];
    int64_t v[3], ex[3], total[3];
    load_counts(counts, (int64_t)blockIdx.x * SCAN_TILE + threadIdx.x, M, v);
    block_scan3(v, ex, total, sh);
    if (threadIdx.x < 3) tile_total[3 * (int64_t)blockIdx.x + threadIdx.x] = total[threadIdx.x];
}

__global__ __launch_bounds__(SCAN_TILE) void k_molproc_scan(const int64_t* __restrict__ tile_total, int64_t tiles, int64_t* __restrict__ tile_prefix,
                                                            int64_t* __restrict__ totals) {
    __shared__ int64_t sh[3][SCAN_TILE];
    int64_t carry[3] = {0, 0, 0};
    for (int64_t base = 0; base < tiles; base += SCAN_TILE) {
        const int64_t t = base + threadIdx.x;
        int64_t v[3], ex[3], total[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = t < tiles ? tile_total[3 * t + c] : 0;
        block_scan3(v, ex, total, sh);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (t < tiles) tile_prefix[3 * t + c] = carry[c] + ex[c];
            carry[c] += total[c];
        }
    }
    if (threadIdx.x < 3) totals[threadIdx.x] = carry[threadIdx.x];
}

__global__ __launch_bounds__(SCAN_TILE) void k_molproc_apply(const int32_t* __restrict__ counts, int64_t M, const int64_t* __restrict__ tile_prefix,
                                                             int64_t* __restrict__ prefix) {
    __shared__ int64_t sh[3][SCAN_TILE];
    const int64_t m = (int64_t)blockIdx.x * SCAN_TILE + threadIdx.x;
    int64_t v[3], ex[3], total[3];
    load_counts(counts, m, M, v);
    block_scan3(v, ex, total, sh);
    if (m < M) {
#pragma unroll
        for (int c = 0; c < 3; ++c) prefix[3 * m + c] = tile_prefix[3 * (int64_t)blockIdx.x + c] + ex[c];
    }
}

template <bool FROM_ORDERS>
__global__ __launch_bounds__(THREADS) void k_molproc_emit(GcdmMolGraphTables tb, const float* __restrict__ x, long stride, const int32_t* __restrict__ types,
                                                          const uint32_t* __restrict__ charges, const int64_t* __restrict__ off, int64_t mol0, int64_t M,
                                                          const int64_t* __restrict__ pair_off, const uint8_t* __restrict__ orders,
                                                          const uint8_t* __restrict__ keep, const int32_t* __restrict__ new_index,
                                                          const int32_t* __restrict__ counts, const int64_t* __restrict__ totals,
                                                          const int64_t* __restrict__ prefix, uint32_t* __restrict__ pos_out, int32_t* __restrict__ types_out,
                                                          uint32_t* __restrict__ charges_out, int64_t* __restrict__ src_atom, int64_t* __restrict__ src_molecule,
                                                          int64_t* __restrict__ mol_off_out, int32_t* __restrict__ bonds_out, int64_t* __restrict__ bond_off_out) {
    __shared__ float sx[MAXA], sy[MAXA], sz[MAXA];
    __shared__ int st[MAXA], sZ[MAXA], sk[MAXA], srow[THREADS];
    __shared__ uint8_t so[MAXA * LD];
    const int64_t m = mol0 + blockIdx.x;
    const int tid = threadIdx.x;
    if (m == M) {                                                      // the workgroup behind the last molecule closes the offset lists
        if (tid == 0) { mol_off_out[totals[2]] = totals[0]; bond_off_out[totals[2]] = totals[1]; }
        return;
    }
    if (counts[3 * m + 2] == 0) return;                                // dropped: no atoms, no bonds, no molecule
    const int64_t a0 = off[m];
    const int n = (int)(off[m + 1] - a0);                              // inside [0, MAXA]: select drops every other size
    const int na = counts[3 * m + 0], nb = counts[3 * m + 1];
    const int64_t A = prefix[3 * m + 0], B = prefix[3 * m + 1], ord = prefix[3 * m + 2];
    if (n < 0 || n > MAXA || na < 0 || na > n || nb < 0 || A < 0 || A + na > totals[0] || B < 0 || B + nb > totals[1] || ord < 0 || ord >= totals[2])
        return;                                                        // not what select wrote: nothing is stored
    if (tid == 0) { mol_off_out[ord] = A; bond_off_out[ord] = B; src_molecule[ord] = m; }
    // the kept atoms to their places: bit copies
    const int i = tid;
    int ni = -1;
    if (i < n) {
        ni = keep[a0 + i] ? new_index[a0 + i] : -1;
        if (ni >= na) ni = -1;
        sk[i] = ni;
        if (ni >= 0) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(x) + (a0 + i) * stride;
            uint32_t* q = pos_out + (A + ni) * 3;
            q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
            types_out[A + ni] = types[a0 + i];
            if (charges) charges_out[A + ni] = charges[a0 + i];
            src_atom[A + ni] = a0 + i;
        }
    }
    if (nb == 0) return;                                               // the same for every thread of the workgroup
    gmg::load_atoms<FROM_ORDERS>(tb, x, stride, types, a0, n, st, sZ, sx, sy, sz);
    __syncthreads();
    gmg::fill_orders<FROM_ORDERS>(tb, n, st, sx, sy, sz, orders, FROM_ORDERS ? pair_off[m] : 0, so);
    __syncthreads();
    // the kept bonds of row i, then the row's place: an exclusive scan of the row counts
    int c = 0;
    if (ni >= 0)
        for (int j = 0; j < i; ++j) c += (sk[j] >= 0 && so[i * LD + j] != 0) ? 1 : 0;
    srow[tid] = c;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {
        const int add = tid >= d ? srow[tid - d] : 0;
        __syncthreads();
        srow[tid] += add;
        __syncthreads();
    }
    int at = srow[tid] - c;
    if (ni >= 0)
        for (int j = 0; j < i; ++j) {
            const int o = so[i * LD + j];
            if (sk[j] >= 0 && o != 0) {
                if (at < nb) {
                    int32_t* q = bonds_out + (B + at) * 3;
                    q[0] = ni; q[1] = sk[j]; q[2] = o;
                }
                ++at;
            }
        }
}

static int scan(const int32_t* counts, int64_t M, int64_t* totals, void* workspace, hipStream_t s) {
    const int64_t tiles = ntiles(M);
    int64_t* prefix = static_cast<int64_t*>(workspace);
    int64_t* tile_total = prefix + 3 * M;
    int64_t* tile_prefix = tile_total + 3 * tiles;
    if (tiles > 0) {
        hipLaunchKernelGGL(k_molproc_totals, dim3((unsigned)tiles), dim3(SCAN_TILE), 0, s, counts, M, tile_total);
        if (hipGetLastError() != hipSuccess) return -2;
    }
    hipLaunchKernelGGL(k_molproc_scan, dim3(1), dim3(SCAN_TILE), 0, s, (const int64_t*)tile_total, tiles, tile_prefix, totals);
    if (hipGetLastError() != hipSuccess) return -2;
    if (tiles > 0) {
        hipLaunchKernelGGL(k_molproc_apply, dim3((unsigned)tiles), dim3(SCAN_TILE), 0, s, counts, M, (const int64_t*)tile_prefix, prefix);
        if (hipGetLastError() != hipSuccess) return -2;
    }
    return 0;
}

template <bool FROM_ORDERS>
static int select(const GcdmMolGraphTables* tb, const float* x, int64_t stride, const int32_t* types, const int64_t* off, int64_t M,
                  const int64_t* pair_off, const uint8_t* orders, int flags, int32_t* info, uint8_t* keep, int32_t* new_index, int32_t* counts,
                  hipStream_t s) {
    for (int64_t mol0 = 0; mol0 < M; mol0 += gmg::GRID_CHUNK) {
        const int64_t blocks = M - mol0 < gmg::GRID_CHUNK ? M - mol0 : gmg::GRID_CHUNK;
        hipLaunchKernelGGL((gmg::k_molgraph<FROM_ORDERS, true>), dim3((unsigned)blocks), dim3(THREADS), 0, s, *tb, x, (long)stride, types, off, mol0,
                           pair_off, orders, (int64_t*)nullptr, info, flags, keep, new_index, counts);
        if (hipGetLastError() != hipSuccess) return -2;
    }
    return 0;
}

}  // namespace gmp

extern "C" {

int64_t gcdm_molproc_workspace_bytes(int64_t num_molecules) {
    if (num_molecules < 0) return -1;
    return (int64_t)sizeof(int64_t) * 3 * (num_molecules + 2 * gmp::ntiles(num_molecules));
}

int gcdm_molproc_select(const GcdmMolGraphTables* tables, const float* x, int64_t x_row_stride, const int32_t* atom_types,
                        const int64_t* mol_offsets, int64_t num_molecules, const int64_t* pair_offsets, const uint8_t* orders, int32_t flags,
                        int32_t* info, uint8_t* keep, int32_t* new_index, int32_t* counts, int64_t* totals, void* workspace, void* stream) {
    GOPS_REQUIRE(gmg::tables_ok(tables) && num_molecules >= 0 && totals && (flags & ~(GCDM_MOLPROC_SANITIZE | GCDM_MOLPROC_LARGEST_FRAG)) == 0);
    GOPS_REQUIRE(orders || x_row_stride >= 3);
    if (num_molecules > 0) {
        GOPS_REQUIRE(atom_types && mol_offsets && info && keep && new_index && counts && workspace && (orders ? pair_offsets != nullptr : x != nullptr));
        const int st = orders ? gmp::select<true>(tables, nullptr, 3, atom_types, mol_offsets, num_molecules, pair_offsets, orders, flags, info, keep,
                                                  new_index, counts, (hipStream_t)stream)
                              : gmp::select<false>(tables, x, x_row_stride, atom_types, mol_offsets, num_molecules, nullptr, nullptr, flags, info, keep,
                                                   new_index, counts, (hipStream_t)stream);
        if (st != 0) return st;
    }
    return gmp::scan(counts, num_molecules, totals, workspace, (hipStream_t)stream);
}

int gcdm_molproc_emit(const GcdmMolGraphTables* tables, const float* x, int64_t x_row_stride, const int32_t* atom_types, const void* charges,
                      const int64_t* mol_offsets, int64_t num_molecules, const int64_t* pair_offsets, const uint8_t* orders,
                      const uint8_t* keep, const int32_t* new_index, const int32_t* counts, const int64_t* totals, const void* workspace,
                      float* pos_out, int32_t* types_out, void* charges_out, int64_t* src_atom, int64_t* src_molecule,
                      int64_t* mol_offsets_out, int32_t* bonds_out, int64_t* bond_offsets_out, void* stream) {
    GOPS_REQUIRE(gmg::tables_ok(tables) && num_molecules >= 0 && x_row_stride >= 3 && totals && mol_offsets_out && bond_offsets_out);
    GOPS_REQUIRE((charges == nullptr) == (charges_out == nullptr));
    if (num_molecules > 0)
        GOPS_REQUIRE(x && atom_types && mol_offsets && keep && new_index && counts && workspace && pos_out && types_out && src_atom && src_molecule &&
                     bonds_out && (!orders || pair_offsets));
    const int64_t M = num_molecules;
    for (int64_t mol0 = 0; mol0 <= M; mol0 += gmg::GRID_CHUNK) {       // M + 1 workgroups: the last one closes the offset lists
        const int64_t blocks = M + 1 - mol0 < gmg::GRID_CHUNK ? M + 1 - mol0 : gmg::GRID_CHUNK;
        if (orders)
            hipLaunchKernelGGL(gmp::k_molproc_emit<true>, dim3((unsigned)blocks), dim3(gmp::THREADS), 0, (hipStream_t)stream, *tables, x, (long)x_row_stride,
                               atom_types, (const uint32_t*)charges, mol_offsets, mol0, M, pair_offsets, orders, keep, new_index, counts, totals,
                               (const int64_t*)workspace, (uint32_t*)pos_out, types_out, (uint32_t*)charges_out, src_atom, src_molecule, mol_offsets_out,
                               bonds_out, bond_offsets_out);
        else
            hipLaunchKernelGGL(gmp::k_molproc_emit<false>, dim3((unsigned)blocks), dim3(gmp::THREADS), 0, (hipStream_t)stream, *tables, x, (long)x_row_stride,
                               atom_types, (const uint32_t*)charges, mol_offsets, mol0, M, pair_offsets, orders, keep, new_index, counts, totals,
                               (const int64_t*)workspace, (uint32_t*)pos_out, types_out, (uint32_t*)charges_out, src_atom, src_molecule, mol_offsets_out,
                               bonds_out, bond_offsets_out);
        if (hipGetLastError() != hipSuccess) return -2;
    }
    return 0;
}

}  // extern "C"
