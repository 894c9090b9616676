// gcdm_ops.geom.hip.h -- the GEOM-Drugs conformer file on the device: rows [R][5] (molecule id, atomic number, x, y, z; float64) segmented
// into molecules chunk by chunk, and the ragged reorder that makes the size-sorted splits.  C ABI: include/gcdm_geom.h.
//
// A run of rows is summarised by a Seg: kept rows, molecule starts among them other than at its first kept row, the ids of its first and
// last kept row.  Two adjacent runs combine associatively (a start is added where the left run's last id differs from the right run's
// first), so the slot and the molecule ordinal of every row are an exclusive scan of Segs behind the carry state:
//   k_geom_totals   one workgroup per tile of TILE rows: the tile's Seg.
//   k_geom_scan     one workgroup: the exclusive scan of the tile Segs behind the state, THREADS tiles at a time with a running carry; the
//                   state advances to the total.
//   k_geom_apply    one workgroup per tile: each thread scans its ROWS consecutive rows behind the tile's prefix and writes z, pos and,
//                   at a start, atom_ptr.  Every store is guarded by cap_atoms / cap_mols.
// Each launch reads only what an earlier launch wrote: no workgroup waits for another.  A scan of Segs is exact integer work, so the
// result does not depend on the tile, the grid or where the chunks were cut.
//   k_geom_finish   one thread: atom_ptr[M] = A and the pair (M, A).
//   k_geom_gather   one wave per output molecule: consecutive lanes copy consecutive atoms (z) and consecutive floats (pos).
#pragma once

namespace ggeo {

constexpr int THREADS = 256;
constexpr int ROWS = 4;                       // consecutive rows per thread
constexpr int TILE = THREADS * ROWS;
static_assert(TILE == GCDM_GEOM_TILE, "include/gcdm_geom.h states the tile");
constexpr int GATHER_WAVES = THREADS / 64;

struct Seg {
    int64_t keep, starts, first, last;
    int64_t has;
};
inline int64_t ntiles(int64_t R) { return (R + TILE - 1) / TILE; }
inline int64_t ws_bytes(int64_t R) { return (2 * ntiles(R) * (int64_t)sizeof(Seg) + 255) & ~(int64_t)255; }

__device__ inline Seg seg_none() { return Seg{0, 0, 0, 0, 0}; }
__device__ inline Seg seg_join(const Seg& l, const Seg& r) {
    Seg o;
    o.keep = l.keep + r.keep;
    o.starts = l.starts + r.starts + ((l.has && r.has && l.last != r.first) ? 1 : 0);
    o.first = l.has ? l.first : r.first;
    o.last = r.has ? r.last : l.last;
    o.has = l.has | r.has;
    return o;
}

// the id column truncated toward zero (astype(int)); 0 and *bad for a value an int64 does not hold
__device__ inline int64_t id_of(double v, int* bad) {
    if (!(fabs(v) < 9.2e18)) {
        *bad = 1;
        return 0;
    }
    return (int64_t)v;
}
__device__ inline bool kept(const double* row, int remove_h) { return !(remove_h && row[1] == 1.0); }
__device__ inline Seg seg_row(const double* row, int remove_h) {
    if (!kept(row, remove_h)) return seg_none();
    int bad = 0;
    const int64_t id = id_of(row[0], &bad);
    return Seg{1, 0, id, id, 1};
}
__device__ inline Seg seg_thread(const double* __restrict__ rows, int64_t r0, int64_t R, int remove_h) {
    Seg v = seg_none();
    for (int j = 0; j < ROWS; ++j)
        if (r0 + j < R) v = seg_join(v, seg_row(rows + (r0 + j) * 5, remove_h));
    return v;
}

// exclusive scan of one Seg per thread; *total = the join of all.  sh [THREADS] is free again on return.
__device__ inline Seg block_scan(Seg v, Seg* sh, Seg* total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {
        const Seg a = tid >= d ? seg_join(sh[tid - d], sh[tid]) : sh[tid];
        __syncthreads();
        sh[tid] = a;
        __syncthreads();
    }
    *total = sh[THREADS - 1];
    const Seg ex = tid ? sh[tid - 1] : seg_none();
    __syncthreads();
    return ex;
}

__global__ void __launch_bounds__(THREADS) k_geom_totals(const double* __restrict__ rows, int64_t R, int remove_h, Seg* __restrict__ totals) {
    __shared__ Seg sh[THREADS];
    const int64_t r0 = (int64_t)blockIdx.x * TILE + (int64_t)threadIdx.x * ROWS;
    Seg total;
    block_scan(seg_thread(rows, r0, R, remove_h), sh, &total);
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

__global__ void __launch_bounds__(THREADS) k_geom_scan(const Seg* __restrict__ totals, int64_t tiles, Seg* __restrict__ prefix, int64_t* state) {
    __shared__ Seg sh[THREADS];
    const int tid = threadIdx.x;
    const int64_t atoms = state[1], mols = state[2];
    Seg carry;                                  // everything before this chunk, as one run
    carry.has = atoms > 0 ? 1 : 0;
    carry.keep = atoms;
    carry.starts = mols - carry.has;
    carry.first = carry.last = state[0];
    for (int64_t base = 0; base < tiles; base += THREADS) {
        const int64_t t = base + tid;
        Seg total;
        const Seg ex = block_scan(t < tiles ? totals[t] : seg_none(), sh, &total);
        if (t < tiles) prefix[t] = seg_join(carry, ex);
        carry = seg_join(carry, total);
    }
    __syncthreads();                            // every thread has read the state
    if (tid == 0) {
        state[0] = carry.has ? carry.last : 0;
        state[1] = carry.keep;
        state[2] = carry.starts + carry.has;
    }
}

__global__ void __launch_bounds__(THREADS) k_geom_apply(const double* __restrict__ rows, int64_t R, int remove_h, const Seg* __restrict__ prefix,
                                                         int32_t* __restrict__ z, float* __restrict__ pos, int64_t* __restrict__ atom_ptr,
                                                         int64_t cap_atoms, int64_t cap_mols, int32_t* flags) {
    __shared__ Seg sh[THREADS];
    const int64_t r0 = (int64_t)blockIdx.x * TILE + (int64_t)threadIdx.x * ROWS;
    Seg total;
    const Seg ex = block_scan(seg_thread(rows, r0, R, remove_h), sh, &total);
    Seg x = seg_join(prefix[blockIdx.x], ex);  // everything before row r0
    int raise = 0;
    for (int j = 0; j < ROWS; ++j) {
        if (r0 + j >= R) break;
        const double* row = rows + (r0 + j) * 5;
        if (!kept(row, remove_h)) continue;
        int bad = 0;
        const int64_t id = id_of(row[0], &bad);
        const double zc = row[1];
        int32_t zz = 0;
        if (fabs(zc) < 2147483648.0) zz = (int32_t)zc;
        else bad = 1;
        if (zz < 1 || !isfinite(row[2]) || !isfinite(row[3]) || !isfinite(row[4])) bad = 1;
        if (bad) raise |= GCDM_GEOM_FLAG_BAD_ROW;
        const int64_t slot = x.keep;
        if (slot < cap_atoms) {
            z[slot] = zz;
            pos[slot * 3 + 0] = (float)row[2];
            pos[slot * 3 + 1] = (float)row[3];
            pos[slot * 3 + 2] = (float)row[4];
        } else {
            raise |= GCDM_GEOM_FLAG_CAPACITY;
        }
        if (!x.has || x.last != id) {           // this row opens molecule x.starts + x.has
            const int64_t m = x.starts + x.has;
            if (m < cap_mols) atom_ptr[m] = slot;
            else raise |= GCDM_GEOM_FLAG_CAPACITY;
        }
        x = seg_join(x, Seg{1, 0, id, id, 1});
    }
    if (raise) atomicOr(flags, raise);
}

__global__ void k_geom_finish(const int64_t* __restrict__ state, int64_t* atom_ptr, int64_t cap_mols, int64_t* MA, int32_t* flags) {
    if (blockIdx.x || threadIdx.x) return;
    const int64_t A = state[1], M = state[2];
    if (M <= cap_mols) atom_ptr[M] = A;
    else atomicOr(flags, GCDM_GEOM_FLAG_CAPACITY);
    MA[0] = M;
    MA[1] = A;
}

__global__ void __launch_bounds__(THREADS) k_geom_gather(const int64_t* __restrict__ ptr_in, const int32_t* __restrict__ z_in,
                                                          const float* __restrict__ pos_in, int64_t M_in, int64_t A_in,
                                                          const int64_t* __restrict__ order, const int64_t* __restrict__ ptr_out, int64_t M_out,
                                                          int64_t A_out, int32_t* __restrict__ z_out, float* __restrict__ pos_out, int32_t* flags) {
    const int64_t k = (int64_t)blockIdx.x * GATHER_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (k >= M_out) return;
    const int64_t m = order[k];
    const int64_t d0 = ptr_out[k], n = ptr_out[k + 1] - d0;
    bool ok = m >= 0 && m < M_in && n >= 0;
    int64_t s0 = 0;
    if (ok) {
        s0 = ptr_in[m];
        ok = s0 >= 0 && ptr_in[m + 1] - s0 == n && s0 + n <= A_in;
    }
    if (!ok) {
        if (lane == 0) atomicOr(flags, GCDM_GEOM_FLAG_ACCOUNT);
        return;
    }
    if ((d0 < 0 || d0 + n > A_out) && lane == 0) atomicOr(flags, GCDM_GEOM_FLAG_ACCOUNT);
    for (int64_t i = lane; i < n; i += 64) {
        const int64_t d = d0 + i;
        if (d >= 0 && d < A_out) z_out[d] = z_in[s0 + i];
    }
    for (int64_t i = lane; i < n * 3; i += 64) {
        const int64_t d = d0 * 3 + i;
        if (d >= 0 && d < A_out * 3) pos_out[d] = pos_in[s0 * 3 + i];
    }
}

}  // namespace ggeo

extern "C" {

int64_t gcdm_geom_workspace_bytes(int32_t which, int64_t R) {
    GOPS_REQUIRE(R >= 0 && R <= GCDM_GEOM_MAX_ROWS);
    if (which == GCDM_GEOM_WS_BYTES) return ggeo::ws_bytes(R);
    if (which == GCDM_GEOM_WS_LAUNCHES) return R ? 3 : 0;
    if (which == GCDM_GEOM_WS_TILE) return ggeo::TILE;
    return -1;
}

int gcdm_geom_ingest(const double* rows, int64_t R, int32_t remove_h, int64_t* state, int32_t* z, float* pos, int64_t* atom_ptr,
                     int64_t cap_atoms, int64_t cap_mols, void* workspace, int32_t* flags, void* stream) {
    GOPS_REQUIRE(R >= 0 && R <= GCDM_GEOM_MAX_ROWS && gops_flag(remove_h) && cap_atoms >= 0 && cap_mols >= 0);
    if (R == 0) return 0;
    GOPS_REQUIRE(rows && state && atom_ptr && workspace && flags && (cap_atoms == 0 || (z && pos)));
    const int64_t tiles = ggeo::ntiles(R);
    ggeo::Seg* totals = (ggeo::Seg*)workspace;
    ggeo::Seg* prefix = totals + tiles;
    hipLaunchKernelGGL(ggeo::k_geom_totals, dim3((unsigned)tiles), dim3(ggeo::THREADS), 0, (hipStream_t)stream, rows, R, (int)remove_h, totals);
    if (hipGetLastError() != hipSuccess) return -2;
    hipLaunchKernelGGL(ggeo::k_geom_scan, dim3(1), dim3(ggeo::THREADS), 0, (hipStream_t)stream, totals, tiles, prefix, state);
    if (hipGetLastError() != hipSuccess) return -2;
    hipLaunchKernelGGL(ggeo::k_geom_apply, dim3((unsigned)tiles), dim3(ggeo::THREADS), 0, (hipStream_t)stream, rows, R, (int)remove_h, prefix, z, pos,
                       atom_ptr, cap_atoms, cap_mols, flags);
    return GOPS_LAUNCH_OK();
}

int gcdm_geom_finish(const int64_t* state, int64_t* atom_ptr, int64_t cap_mols, int64_t* MA, int32_t* flags, void* stream) {
    GOPS_REQUIRE(state && atom_ptr && MA && flags && cap_mols >= 0);
    hipLaunchKernelGGL(ggeo::k_geom_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, state, atom_ptr, cap_mols, MA, flags);
    return GOPS_LAUNCH_OK();
}

int gcdm_geom_gather(const int64_t* atom_ptr_in, const int32_t* z_in, const float* pos_in, int64_t M_in, int64_t A_in, const int64_t* order,
                     const int64_t* atom_ptr_out, int64_t M_out, int64_t A_out, int32_t* z_out, float* pos_out, int32_t* flags, void* stream) {
    GOPS_REQUIRE(M_in >= 0 && A_in >= 0 && M_out >= 0 && A_out >= 0 && M_out < ((int64_t)1 << 32) && A_in < ((int64_t)1 << 60) &&
                 A_out < ((int64_t)1 << 60));
    if (M_out == 0) return 0;
    GOPS_REQUIRE(order && atom_ptr_out && flags && (M_in == 0 || atom_ptr_in) && (A_in == 0 || (z_in && pos_in)) &&
                 (A_out == 0 || (z_out && pos_out)));
    hipLaunchKernelGGL(ggeo::k_geom_gather, dim3(gops_blocks(M_out, ggeo::GATHER_WAVES)), dim3(ggeo::THREADS), 0, (hipStream_t)stream, atom_ptr_in,
                       z_in, pos_in, M_in, A_in, order, atom_ptr_out, M_out, A_out, z_out, pos_out, flags);
    return GOPS_LAUNCH_OK();
}

}  // extern "C"
