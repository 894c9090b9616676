// gcdm_ops.classifier_train.hip.h -- the column-split first edge layer of the EGNN property classifier for training, forward and backward.
// C ABI: include/gcdm_classifier_train.h.
//
// edge_mlp.0 of E_GCL_mask is an [E, 2H + 1] . [2H + 1, H] GEMM on cat(h[row], h[col], radial).  Split by columns it is two node-level GEMMs
// (A = h W_s^T + b, B = h W_t^T: gcdm_op_gemm) and this element-wise kernel over the edges, which also computes the radial from x.  The
// edge set is fixed -- the ordered pairs i != j of each molecule, row-major -- so an edge's index is arithmetic on the molecule's offsets and
// neither an edge list nor a column-sorted copy of one is read:
//   k_ct_edge_pre_fwd   one workgroup per node i: its n - 1 edge rows are contiguous; consecutive threads write consecutive columns.
//   k_ct_edge_pre_bwd   one workgroup per node, one thread per column: dA = the sum of the node's own rows, dB = the sum over the molecule's
//                       block with stride n - 1, both in ascending order of the other atom.
//   k_ct_wr_slices      dw_r = sum_e radial[e] dpre[e][:] over contiguous slices of edges (grid.y), as gops::k_colsum_slices; one slice
//                       writes dw_r itself, several write partial sums that gops::k_reduce_slices adds in slice order.
// No float atomics; no workgroup waits for another.
#pragma once

namespace gct {

constexpr int THREADS = 256;

struct Where {
    int64_t o, eo;          // first node and first edge of the molecule
    int n, li;              // atoms of the molecule, the node's index among them
};

// The node's place from the three tables; false if they disagree.  After true: o + n <= N and eo + n (n - 1) <= E, so every node index
// o + j (j < n) and every edge index eo + i (n - 1) + jj (i < n, jj < n - 1) is inside the buffers.
__device__ inline bool where(int64_t v, const int32_t* __restrict__ node_mol, const int32_t* __restrict__ noff, const int64_t* __restrict__ eoff,
                             int64_t N, int64_t nmol, int64_t E, Where* w) {
    const int64_t m = node_mol[v];
    if (m < 0 || m >= nmol) return false;
    const int64_t o = noff[m], o1 = noff[m + 1], eo = eoff[m];
    if (o < 0 || o1 > N || v < o || v >= o1 || eo < 0 || eo > E) return false;
    const int64_t n = o1 - o;                                   // 1 <= n <= N < 2^31: n (n - 1) < 2^62
    if (n * (n - 1) > E - eo) return false;
    w->o = o;
    w->eo = eo;
    w->n = (int)n;
    w->li = (int)(v - o);
    return true;
}

// torch.sum((coord_diff)**2, 1) of coord2radial with every product and sum rounded once: (dx dx + dy dy) + dz dz, no contraction into FMAs, so
// the radial has the bits of the element-wise fp32 expression
__device__ inline float radial3(float dx, float dy, float dz) {
#pragma clang fp contract(off)
    const float a = dx * dx, b = dy * dy, c = dz * dz;
    return (a + b) + c;
}

__global__ __launch_bounds__(THREADS) void k_ct_edge_pre_fwd(const float* __restrict__ A, const float* __restrict__ B, const float* __restrict__ x,
                                                             const float* __restrict__ wr, const int32_t* __restrict__ node_mol,
                                                             const int32_t* __restrict__ noff, const int64_t* __restrict__ eoff,
                                                             float* __restrict__ pre, float* __restrict__ radial, int64_t N, int64_t nmol, int64_t E,
                                                             int H) {
    const int64_t i = blockIdx.x;
    Where w;
    if (i >= N || !where(i, node_mol, noff, eoff, N, nmol, E, &w) || w.n < 2) return;
    const float xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2];
    const int64_t e0 = w.eo + (int64_t)w.li * (w.n - 1);
    const int64_t total = (int64_t)(w.n - 1) * H;
    for (int64_t t = threadIdx.x; t < total; t += THREADS) {
        const int64_t jj = t / H;
        const int c = (int)(t - jj * H);
        const int64_t j = w.o + jj + (jj >= w.li ? 1 : 0);
        const float dx = xi - x[3 * j], dy = yi - x[3 * j + 1], dz = zi - x[3 * j + 2];
        const float r = radial3(dx, dy, dz);
        pre[(e0 + jj) * H + c] = (A[i * H + c] + B[j * H + c]) + r * wr[c];
        if (c == 0) radial[e0 + jj] = r;
    }
}

__global__ void k_ct_edge_pre_bwd(const float* __restrict__ dpre, const int32_t* __restrict__ node_mol, const int32_t* __restrict__ noff,
                                  const int64_t* __restrict__ eoff, float* __restrict__ dA, float* __restrict__ dB, int64_t N, int64_t nmol,
                                  int64_t E, int H) {
    const int64_t i = blockIdx.x;
    if (i >= N) return;
    Where w;
    const bool ok = where(i, node_mol, noff, eoff, N, nmol, E, &w);
    const int n = ok ? w.n : 0;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        float sa = 0.f, sb = 0.f;
        if (n >= 2) {
            const float* own = dpre + (w.eo + (int64_t)w.li * (n - 1)) * H + c;                 // edges (li, j), j ascending
            for (int jj = 0; jj < n - 1; ++jj) sa += own[(int64_t)jj * H];
            const float* blk = dpre + w.eo * H + c;                                             // edges (ii, li), ii ascending
            for (int ii = 0; ii < n; ++ii)
                if (ii != w.li) sb += blk[((int64_t)ii * (n - 1) + (w.li - (w.li > ii ? 1 : 0))) * H];
        }
        dA[i * H + c] = sa;
        dB[i * H + c] = sb;
    }
}

__global__ __launch_bounds__(THREADS) void k_ct_wr_slices(const float* __restrict__ dpre, const float* __restrict__ radial, float* __restrict__ part,
                                                          int64_t E, int H, int64_t rows) {
    __shared__ float red[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
    const int64_t m0 = (int64_t)blockIdx.y * rows, m1 = m0 + rows < E ? m0 + rows : E;
    float s = 0.f;
    if (c < H)
        for (int64_t m = m0 + g; m < m1; m += 4) s += radial[m] * dpre[m * H + c];
    red[g][threadIdx.x & 63] = s;
    __syncthreads();
    if (g == 0 && c < H) part[(int64_t)blockIdx.y * H + c] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

inline int slices_of(int64_t E) {
    if (E < GCDM_CLASSIFIER_TRAIN_TWO_STAGE_EDGES) return 1;
    const int64_t s = (E + GCDM_CLASSIFIER_TRAIN_SLICE_EDGES - 1) / GCDM_CLASSIFIER_TRAIN_SLICE_EDGES;
    return (int)(s < GCDM_CLASSIFIER_TRAIN_MAX_SLICES ? s : GCDM_CLASSIFIER_TRAIN_MAX_SLICES);
}
inline bool dims_ok(int64_t N, int64_t nmol, int64_t E, int32_t H) {
    return N >= 0 && N < ((int64_t)1 << 31) && nmol >= 0 && nmol < ((int64_t)1 << 31) && E >= 0 && H >= 1 && H <= GCDM_CLASSIFIER_TRAIN_MAX_H &&
           E < (((int64_t)1 << 62) / H);
}

}  // namespace gct

extern "C" {

int64_t gcdm_classifier_train_workspace_bytes(int64_t E, int32_t H) {
    GOPS_REQUIRE(gct::dims_ok(0, 0, E, H));
    const int s = gct::slices_of(E);
    return s == 1 ? 0 : ((int64_t)s * H * (int64_t)sizeof(float) + 255) & ~(int64_t)255;
}

int gcdm_classifier_train_edge_pre_fwd(const float* A, const float* B, const float* x, const float* w_r, const int32_t* node_mol,
                                       const int32_t* node_offsets, const int64_t* edge_offsets, float* pre, float* radial, int64_t N,
                                       int64_t num_molecules, int64_t E, int32_t H, void* stream) {
    GOPS_REQUIRE(gct::dims_ok(N, num_molecules, E, H));
    if (E == 0) return 0;
    GOPS_REQUIRE(N >= 2 && num_molecules >= 1 && A && B && x && w_r && node_mol && node_offsets && edge_offsets && pre && radial);
    hipLaunchKernelGGL(gct::k_ct_edge_pre_fwd, dim3((unsigned)N), dim3(gct::THREADS), 0, (hipStream_t)stream, A, B, x, w_r, node_mol, node_offsets,
                       edge_offsets, pre, radial, N, num_molecules, E, (int)H);
    return GOPS_LAUNCH_OK();
}

int gcdm_classifier_train_edge_pre_bwd(const float* dpre, const float* radial, const int32_t* node_mol, const int32_t* node_offsets,
                                       const int64_t* edge_offsets, float* dA, float* dB, float* dw_r, void* workspace, int64_t N,
                                       int64_t num_molecules, int64_t E, int32_t H, void* stream) {
    GOPS_REQUIRE(gct::dims_ok(N, num_molecules, E, H));
    if (E == 0) return 0;
    const int slices = gct::slices_of(E);
    GOPS_REQUIRE(N >= 2 && num_molecules >= 1 && dpre && radial && node_mol && node_offsets && edge_offsets && dA && dB && dw_r &&
                 (slices == 1 || workspace));
    const int threads = H <= 64 ? 64 : H <= 128 ? 128 : 256;
    hipLaunchKernelGGL(gct::k_ct_edge_pre_bwd, dim3((unsigned)N), dim3(threads), 0, (hipStream_t)stream, dpre, node_mol, node_offsets, edge_offsets,
                       dA, dB, N, num_molecules, E, (int)H);
    if (hipGetLastError() != hipSuccess) return -2;
    const int64_t rows = (E + slices - 1) / slices;
    float* part = slices == 1 ? dw_r : (float*)workspace;
    hipLaunchKernelGGL(gct::k_ct_wr_slices, dim3((H + 63) / 64, slices), dim3(gct::THREADS), 0, (hipStream_t)stream, dpre, radial, part, E, (int)H,
                       rows);
    if (slices == 1) return GOPS_LAUNCH_OK();
    if (hipGetLastError() != hipSuccess) return -2;
    hipLaunchKernelGGL(gops::k_reduce_slices, dim3(gops_blocks(H)), dim3(256), 0, (hipStream_t)stream, (const float*)part, dw_r, (int64_t)H, slices);
    return GOPS_LAUNCH_OK();
}

}  // extern "C"
