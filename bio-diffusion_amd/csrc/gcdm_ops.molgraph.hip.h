// gcdm_ops.molgraph.hip.h -- the per-molecule graph kernel behind validity, uniqueness and novelty without RDKit (include/gcdm_molgraph.h).
//
// One workgroup of 256 threads per molecule of at most 192 atoms; everything after the loads lives in LDS (~50 KB: three workgroups per CU).
//   1. types -> vocabulary index and atomic number; coordinates staged (first entry).
//   2. the n x n bond orders as bytes, every element written exactly once: the thread that owns (i, j), i > j, classifies the pair -- with the
//      arithmetic of k_stability (gcdm_stability.hip.h), restated here: written-out FMA chain, sqrtf, strict < against thr1..3 -- or reads it
//      from the gcdm_bond_orders layout, and writes (i, j) and (j, i).  Rows are 196 bytes apart: 49 dwords, so the threads of a wave that walk
//      their own rows in step 3 fall on different banks (192 would put them on two).
//   3. thread i walks row i: the 3 x 64-bit adjacency words of the atom, its order sum against the cap of its type.
//   4. thread i runs a breadth-first search from atom i on the bitsets (frontier -> OR of the adjacency rows -> minus visited).  Level by
//      level it adds the distance term of c0(i); what it has visited at the end IS the component of i: its size is a population count,
//      its label the lowest set bit.  The component leaders (label == own index) count the fragments and bid for the largest with one LDS
//      atomicMax on size << 8 | 255 - label, which prefers the larger size and then the lower label.
//      The SELECT mode (include/gcdm_molproc.h) ends here: keep bytes, new local indices and counts in place of steps 5 and 6.
//   5. GCDM_MOLGRAPH_ROUNDS refinement rounds over the neighbours, two colour arrays in turn, the threads of the largest fragment only.
//   6. the 64-bit sum of the fragment's colours through one LDS atomic per atom (the sum is commutative and exact: no order dependence).
// Integer work throughout; no float leaves step 2.  Nothing is read for a molecule whose size is outside [0, 192].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/gcdm_molgraph.h"

namespace gmg {

constexpr int MAXA = GCDM_MOLGRAPH_MAX_ATOMS, W = MAXA / 64, LD = MAXA + 4, THREADS = 256, T16 = GCDM_STABILITY_MAX_TYPES;
constexpr int64_t GRID_CHUNK = (int64_t)1 << 30;
static_assert(MAXA % 64 == 0 && MAXA <= 255 && MAXA <= THREADS, "one thread per atom, labels in 8 bits");

__device__ __forceinline__ uint64_t mix(uint64_t v) {
    v ^= v >> 30; v *= 0xBF58476D1CE4E5B9ULL;
    v ^= v >> 27; v *= 0x94D049BB133111EBULL;
    v ^= v >> 31;
    return v;
}

// Steps 1 and 2, stated once for k_molgraph and for the emit kernel of gcdm_ops.molproc.hip.h: both see the same types and the same orders.
// 1. types -> vocabulary index (-1 outside it) and atomic number; coordinates staged when the orders come from the distance rule.
template <bool FROM_ORDERS>
__device__ __forceinline__ void load_atoms(const GcdmMolGraphTables& tb, const float* __restrict__ x, long stride, const int32_t* __restrict__ types,
                                           int64_t a0, int n, int* st, int* sZ, float* sx, float* sy, float* sz) {
    const int nt = tb.bonds.num_types;
    for (int i = threadIdx.x; i < n; i += THREADS) {
        const int t = types[a0 + i];
        int k = -1;
        if (tb.types_are_atomic_numbers) {
            for (int c = nt - 1; c >= 0; --c) k = (tb.atomic_number[c] == t) ? c : k;        // the first match
        } else if ((unsigned)t < (unsigned)nt) {
            k = t;
        }
        st[i] = k;
        sZ[i] = k >= 0 ? tb.atomic_number[k] : 0;
        if (!FROM_ORDERS) {
            const float* p = x + (a0 + i) * stride;
            sx[i] = p[0]; sy[i] = p[1]; sz[i] = p[2];
        }
    }
}

// the order of the pair (i, j), i > j: THE classification, of which there is one
template <bool FROM_ORDERS>
__device__ __forceinline__ int pair_order(const GcdmMolGraphTables& tb, int i, int j, int ti, int tj, const float* sx, const float* sy, const float* sz,
                                          const uint8_t* __restrict__ orders, int64_t at) {
    int o;
    if (FROM_ORDERS) {
        o = orders[at];
    } else {
        const float dx = sx[i] - sx[j], dy = sy[i] - sy[j], dz = sz[i] - sz[j];
        const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));       // the chain of cdist's direct path, not left to contraction
        const float d = 100.0f * sqrtf(d2);                                             // sqrtf is correctly rounded
        const int k = (ti >= 0 && tj >= 0) ? ti * T16 + tj : 0;
        o = d < tb.bonds.thr1[k] ? 1 : 0;
        o = d < tb.bonds.thr2[k] ? 2 : o;
        o = d < tb.bonds.thr3[k] ? 3 : o;
        if (tb.bonds.limit_bonds_to_one && o > 1) o = 1;
    }
    if (ti < 0 || tj < 0) o = 0;                                       // an atom outside the vocabulary bonds to nothing
    return o;
}

// 2. the n x n orders as bytes, rows LD apart, every element written exactly once
template <bool FROM_ORDERS>
__device__ __forceinline__ void fill_orders(const GcdmMolGraphTables& tb, int n, const int* st, const float* sx, const float* sy, const float* sz,
                                            const uint8_t* __restrict__ orders, int64_t p0, uint8_t* so) {
    for (int idx = threadIdx.x; idx < n * n; idx += THREADS) {
        const int i = idx / n, j = idx - i * n;
        if (i == j) so[i * LD + i] = 0;
        if (i <= j) continue;
        const int o = pair_order<FROM_ORDERS>(tb, i, j, st[i], st[j], sx, sy, sz, orders, p0 + idx);
        so[i * LD + j] = (uint8_t)o;
        so[j * LD + i] = (uint8_t)o;
    }
}

// SELECT = false: the key of the largest fragment (steps 5 and 6).  SELECT = true (include/gcdm_molproc.h): in place of the key rounds, per atom
// the keep byte and its new local index under `flags` (bit 0 sanitize, bit 1 largest_frag), per molecule counts = {kept atoms, kept bonds, kept
// molecule}; `keys` is then not touched.
template <bool FROM_ORDERS, bool SELECT>
__global__ __launch_bounds__(THREADS) void k_molgraph(GcdmMolGraphTables tb, const float* __restrict__ x, long stride,
                                                      const int32_t* __restrict__ types, const int64_t* __restrict__ off, int64_t mol0,
                                                      const int64_t* __restrict__ pair_off, const uint8_t* __restrict__ orders,
                                                      int64_t* __restrict__ keys, int32_t* __restrict__ info, int flags, uint8_t* __restrict__ keep,
                                                      int32_t* __restrict__ new_index, int32_t* __restrict__ counts) {
    __shared__ float sx[MAXA], sy[MAXA], sz[MAXA];
    __shared__ int st[MAXA], sZ[MAXA];
    __shared__ uint8_t so[MAXA * LD];
    __shared__ unsigned long long adj[MAXA * W], col[SELECT ? 1 : 2][SELECT ? 1 : MAXA], s_sum;
    __shared__ int s_invalid, s_nfrag, s_wave[THREADS / 64], s_bonds;
    __shared__ unsigned s_best;
    const int64_t m = mol0 + blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t a0 = off[m], n64 = off[m + 1] - a0;
    if (n64 < 0 || n64 > MAXA) {                                       // the same for every thread of the workgroup: nothing is read, nothing computed
        if (tid == 0) {
            if (SELECT) { counts[3 * m + 0] = 0; counts[3 * m + 1] = 0; counts[3 * m + 2] = 0; }
            else keys[m] = 0;
            info[4 * m + 0] = -1; info[4 * m + 1] = 0; info[4 * m + 2] = 0;
            info[4 * m + 3] = (int32_t)(n64 > INT32_MAX ? INT32_MAX : (n64 < INT32_MIN ? INT32_MIN : n64));
        }
        return;
    }
    const int n = (int)n64;
    if (tid == 0) { s_invalid = 0; s_nfrag = 0; s_best = 0; s_sum = 0; s_bonds = 0; }
    load_atoms<FROM_ORDERS>(tb, x, stride, types, a0, n, st, sZ, sx, sy, sz);
    __syncthreads();
    fill_orders<FROM_ORDERS>(tb, n, st, sx, sy, sz, orders, FROM_ORDERS ? pair_off[m] : 0, so);
    __syncthreads();
    // 3. adjacency words and the valence of atom tid
    const int i = tid;
    const bool atom = i < n;
    uint64_t row[W];
#pragma unroll
    for (int w = 0; w < W; ++w) row[w] = 0;
    if (atom) {
        int val = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const int jn = min(64, n - w * 64);
            uint64_t bits = 0;
            for (int b = 0; b < jn; ++b) {
                const int o = so[i * LD + w * 64 + b];
                val += o;
                bits |= (uint64_t)(o != 0) << b;
            }
            row[w] = bits;
            adj[i * W + w] = bits;
        }
        const int k = st[i];
        const int cap = k >= 0 ? tb.valence_cap[k] : 0;
        if (k < 0 || (cap >= 0 && val > cap)) atomicOr(&s_invalid, 1);
    }
    __syncthreads();
    // 4. breadth-first search from atom tid: the distance term of c0, and the component of the atom
    int label = -1;
    if (atom) {
        uint64_t vis[W], fr[W];
#pragma unroll
        for (int w = 0; w < W; ++w) vis[w] = fr[w] = (w == (i >> 6)) ? (uint64_t)1 << (i & 63) : 0;
        uint64_t acc = 0;
        for (int d = 1; d < MAXA; ++d) {
            uint64_t nx[W];
#pragma unroll
            for (int w = 0; w < W; ++w) nx[w] = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                uint64_t f = fr[w];
                while (f) {
                    const int j = w * 64 + __builtin_ctzll(f);
                    f &= f - 1;
#pragma unroll
                    for (int v = 0; v < W; ++v) nx[v] |= adj[j * W + v];
                }
            }
            uint64_t any = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) { nx[w] &= ~vis[w]; any |= nx[w]; }
            if (!any) break;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                uint64_t f = nx[w];
                while (!SELECT && f) {
                    const int j = w * 64 + __builtin_ctzll(f);
                    f &= f - 1;
                    acc += mix((((uint64_t)d << 8) | (uint64_t)(int64_t)sZ[j]) + GCDM_MOLGRAPH_K2);
                }
                vis[w] |= nx[w];
                fr[w] = nx[w];
            }
        }
        if constexpr (!SELECT) col[0][i] = mix((uint64_t)(int64_t)sZ[i] * GCDM_MOLGRAPH_K1 + acc);
        int size = 0;
#pragma unroll
        for (int w = W - 1; w >= 0; --w) {
            size += __builtin_popcountll(vis[w]);
            if (vis[w]) label = w * 64 + __builtin_ctzll(vis[w]);
        }
        if (label == i) {
            atomicAdd(&s_nfrag, 1);
            atomicMax(&s_best, ((unsigned)size << 8) | (unsigned)(255 - label));
        }
    }
    __syncthreads();
    const unsigned best = s_best;
    const int msize = (int)(best >> 8);
    const bool in_f = atom && msize > 0 && label == 255 - (int)(best & 255u);
    if constexpr (SELECT) {
        // the molecule is dropped iff sanitize is set and it is not valid; a kept molecule keeps all its atoms, with largest_frag those of its
        // largest fragment.  New index = the number of kept atoms below: a ballot per wave, the wave totals through LDS.  A bond never leaves a
        // component, so every neighbour of a kept atom is kept: the kept bonds of atom i are its neighbours below i.
        const bool kept_mol = !((flags & 1) && s_invalid);
        const bool kp = atom && kept_mol && (!(flags & 2) || in_f);
        const unsigned long long ballot = __ballot(kp);
        const int lane = tid & 63, wave = tid >> 6;
        if (lane == 0) s_wave[wave] = __builtin_popcountll(ballot);
        if (kp) {
            int nb = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const int below = i - w * 64;                         // bits of word w that lie below atom i
                const uint64_t mask = below >= 64 ? ~(uint64_t)0 : (below <= 0 ? 0 : (((uint64_t)1 << below) - 1));
                nb += __builtin_popcountll(row[w] & mask);
            }
            if (nb) atomicAdd(&s_bonds, nb);
        }
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) { before += w < wave ? s_wave[w] : 0; total += s_wave[w]; }
        if (atom) {
            keep[a0 + i] = kp ? 1 : 0;
            new_index[a0 + i] = kp ? before + __builtin_popcountll(ballot & (((uint64_t)1 << lane) - 1)) : -1;
        }
        if (tid == 0) {
            counts[3 * m + 0] = total; counts[3 * m + 1] = s_bonds; counts[3 * m + 2] = kept_mol ? 1 : 0;
            info[4 * m + 0] = s_invalid ? 0 : 1; info[4 * m + 1] = s_nfrag; info[4 * m + 2] = msize; info[4 * m + 3] = n;
        }
    } else {
        // 5. refinement over the neighbours
        int cur = 0;
        for (int r = 0; r < GCDM_MOLGRAPH_ROUNDS; ++r) {
            if (in_f) {
                uint64_t acc = col[cur][i] * GCDM_MOLGRAPH_K3;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    uint64_t f = row[w];
                    while (f) {
                        const int j = w * 64 + __builtin_ctzll(f);
                        f &= f - 1;
                        acc += mix(col[cur][j] + (uint64_t)so[i * LD + j] * GCDM_MOLGRAPH_K4);
                    }
                }
                col[cur ^ 1][i] = mix(acc);
            }
            cur ^= 1;
            __syncthreads();
        }
        // 6. the key
        if (in_f) atomicAdd(&s_sum, (unsigned long long)mix(col[cur][i]));
        __syncthreads();
        if (tid == 0) {
            keys[m] = (int64_t)mix((uint64_t)msize * GCDM_MOLGRAPH_K5 + (uint64_t)s_sum);
            info[4 * m + 0] = s_invalid ? 0 : 1;
            info[4 * m + 1] = s_nfrag;
            info[4 * m + 2] = msize;
            info[4 * m + 3] = n;
        }
    }
}

static inline bool tables_ok(const GcdmMolGraphTables* tb) {
    return tb && tb->bonds.num_types >= 1 && tb->bonds.num_types <= GCDM_STABILITY_MAX_TYPES;
}

template <bool FROM_ORDERS>
static int launch(const GcdmMolGraphTables* tb, const float* x, int64_t stride, const int32_t* types, const int64_t* off, int64_t M,
                  const int64_t* pair_off, const uint8_t* orders, int64_t* keys, int32_t* info, void* stream) {
    for (int64_t mol0 = 0; mol0 < M; mol0 += GRID_CHUNK) {
        const int64_t blocks = M - mol0 < GRID_CHUNK ? M - mol0 : GRID_CHUNK;
        hipLaunchKernelGGL((k_molgraph<FROM_ORDERS, false>), dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, *tb, x, (long)stride, types, off,
                           mol0, pair_off, orders, keys, info, 0, (uint8_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
        if (hipGetLastError() != hipSuccess) return -2;
    }
    return 0;
}

}  // namespace gmg

extern "C" {

int gcdm_molgraph_keys(const GcdmMolGraphTables* tables, const float* x, int64_t x_row_stride, const int32_t* atom_types,
                       const int64_t* mol_offsets, int64_t num_molecules, int64_t* keys, int32_t* info, void* stream) {
    GOPS_REQUIRE(gmg::tables_ok(tables) && num_molecules >= 0 && x_row_stride >= 3);
    if (num_molecules == 0) return 0;
    GOPS_REQUIRE(x && atom_types && mol_offsets && keys && info);
    return gmg::launch<false>(tables, x, x_row_stride, atom_types, mol_offsets, num_molecules, nullptr, nullptr, keys, info, stream);
}

int gcdm_molgraph_keys_from_orders(const GcdmMolGraphTables* tables, const int32_t* atom_types, const int64_t* mol_offsets, int64_t num_molecules,
                                   const int64_t* pair_offsets, const uint8_t* orders, int64_t* keys, int32_t* info, void* stream) {
    GOPS_REQUIRE(gmg::tables_ok(tables) && num_molecules >= 0);
    if (num_molecules == 0) return 0;
    GOPS_REQUIRE(atom_types && mol_offsets && pair_offsets && orders && keys && info);
    return gmg::launch<true>(tables, nullptr, 3, atom_types, mol_offsets, num_molecules, pair_offsets, orders, keys, info, stream);
}

}  // extern "C"
