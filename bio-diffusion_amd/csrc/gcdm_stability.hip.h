// gcdm_stability.hip.h -- molecular stability of a sampled batch on the device (gfx950).
//
// One wave per molecule.  Lane i owns atoms i, i+64, ...: for each it walks all atoms j of the molecule (positions and types of
// the molecule are staged in LDS for n <= STAB_LDS_ATOMS, read through L1 otherwise), classifies the pair by the three
// length + margin thresholds (later thresholds overwrite earlier ones, edm/__init__.py:76-81), sums the bond orders of the row
// (diagonal excluded, :108-109) and tests the valence against the type's allowed set (:111-117).  Integer work on 16 B per atom:
// HBM/latency bound, ~ microseconds for a whole batch; it exists so that the evaluation loop never leaves the device.
//
// Distances: d2 = fma(dz, dz, fma(dy, dy, dx * dx)), d = 100 * sqrt(d2), fp32 with a correctly rounded square root.  That is what ATen's
// cdist computes on its direct path (n <= 25): tests/test_stability_cases_cpu.py holds the chain to torch.cdist bit for bit on > 30 000
// pairs; the plain sequential sum agrees on 91 % of them only.  The FMAs are written out and the root is sqrtf: HIP's __fmul_rn / __fadd_rn
// are the plain operators (the compiler contracts them as it likes) and __fsqrt_rn is the 1-ulp v_sqrt_f32, which put pairs one ulp off
// a threshold on the wrong side of it (tests/test_stability_cabi_gpu.py::test_boundary_axis).  For n > 25 the reference switches to the
// matmul expansion, whose last bits differ from its own direct path; the kernel keeps the direct rule at every size.
// Thresholds arrive as the smallest fp32 >= the reference's float64 `length + margin` (stability.bond_tables), so `d < thr` decides as the
// reference's widened comparison does.  A type outside [0, num_types) reads no table entry: order 0 to and from that atom, atom unstable.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/gcdm_hip.h"

constexpr int STAB_LDS_ATOMS = 1024;

__global__ __launch_bounds__(64) void k_stability(GcdmBondTables tb, const float* __restrict__ x, long stride,
                                                  const int32_t* __restrict__ types, const int32_t* __restrict__ off,
                                                  int32_t* __restrict__ out, const int64_t* __restrict__ pair_off = nullptr,
                                                  uint8_t* __restrict__ orders = nullptr) {
    __shared__ float sx[STAB_LDS_ATOMS], sy[STAB_LDS_ATOMS], sz[STAB_LDS_ATOMS];
    __shared__ int st[STAB_LDS_ATOMS];
    const int m = blockIdx.x, lane = threadIdx.x;
    const int a0 = off[m], n = off[m + 1] - a0;
    const bool in_lds = n <= STAB_LDS_ATOMS;
    if (in_lds) {
        for (int i = lane; i < n; i += 64) {
            const float* p = x + (long)(a0 + i) * stride;
            sx[i] = p[0]; sy[i] = p[1]; sz[i] = p[2];
            st[i] = types[a0 + i];
        }
        __syncthreads();
    }
    int stable = 0;
    for (int i = lane; i < n; i += 64) {
        float xi, yi, zi; int ti;
        if (in_lds) { xi = sx[i]; yi = sy[i]; zi = sz[i]; ti = st[i]; }
        else { const float* p = x + (long)(a0 + i) * stride; xi = p[0]; yi = p[1]; zi = p[2]; ti = types[a0 + i]; }
        const bool vi = (unsigned)ti < (unsigned)tb.num_types;         // a type outside [0, T) reads no table entry: no bonds, unstable
        int nb = 0;
        for (int j = 0; j < n; ++j) {
            float xj, yj, zj; int tj;
            if (in_lds) { xj = sx[j]; yj = sy[j]; zj = sz[j]; tj = st[j]; }
            else { const float* p = x + (long)(a0 + j) * stride; xj = p[0]; yj = p[1]; zj = p[2]; tj = types[a0 + j]; }
            const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
            const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));   // the chain of cdist's direct path, not left to contraction
            const float d = 100.0f * sqrtf(d2);                          // "we change the metric" (:69), fp32 like the reference; sqrtf is correctly rounded
            const bool pair = vi && (unsigned)tj < (unsigned)tb.num_types;
            const int k = pair ? ti * GCDM_STABILITY_MAX_TYPES + tj : 0;
            int o = d < tb.thr1[k] ? 1 : 0;
            o = d < tb.thr2[k] ? 2 : o;
            o = d < tb.thr3[k] ? 3 : o;
            if (tb.limit_bonds_to_one && o > 1) o = 1;
            if (!pair) o = 0;
            if (orders) orders[pair_off[m] + (int64_t)i * n + j] = (uint8_t)((j == i) ? 0 : o);     // n x n bond-order matrix (get_bond_order_batch, :61-87)
            nb += (j == i) ? 0 : o;
        }
        stable += (vi && nb < 32 && ((tb.allowed_mask[vi ? ti : 0] >> nb) & 1u)) ? 1 : 0;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) stable += __shfl_xor(stable, s);
    if (lane == 0 && out) {
        out[3 * m + 0] = (stable == n) ? 1 : 0;
        out[3 * m + 1] = stable;
        out[3 * m + 2] = n;
    }
}
