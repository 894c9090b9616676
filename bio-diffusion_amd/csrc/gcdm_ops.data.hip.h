// gcdm_ops.data.hip.h -- the device-resident molecule data set: a training batch collated in HBM, the property histograms of conditional
// sampling and the context draw.  C ABI: include/gcdm_data.h.
//
//   k_data_scan     one workgroup: the batch's molecules perm[first + b], their sizes n_b and the exclusive scans of rows (n_b, or pad_to)
//                   and of edges (n_b^2) into the workspace, a tile of THREADS molecules at a time with a running carry.  A permutation
//                   entry outside [0, M), atoms outside [0, A), n_b > pad_to, or totals other than the host's N and E raise
//                   GCDM_DATA_FLAG_ACCOUNT; such a molecule counts as empty.
//   k_data_collate  one workgroup per molecule: its rows (positions, one-hot, charge, batch, mask, context), its slots of index /
//                   num_nodes_present / props, and its n_b^2 edges with their CSR in closed form: edge k = i n_b + j of the molecule is
//                   (o_b + i, o_b + j), colperm[eoff_b + k] = eoff_b + (k mod n_b) n_b + k / n_b, rowptr[o_b + i] = colptr[o_b + i] =
//                   eoff_b + min(i, n_b) n_b.  Consecutive lanes write consecutive 64-bit words of row, col and colperm.  Every store is
//                   guarded by the host's N and E, so totals that do not add up cannot make it write outside the caller's buffers.
//   k_data_hist     one workgroup: per size the member count and (min, max) through integer LDS atomics on order-preserving keys, then the
//                   bin of every value with the reference's fp32 arithmetic and an integer atomic on the count table.
//   k_data_sample   one thread per (molecule, property).
// No float atomics anywhere; integer sums do not depend on their order.
#pragma once

namespace gdat {

constexpr int THREADS = 256;
constexpr int HIST_THREADS = 1024;

struct Set {
    const int64_t* atom_ptr;
    const int32_t* z;
    const float* pos;
    const float* props;
    const int32_t* species;
    const float* norm;
    const int64_t* index;
    int64_t M, A;
    int P, T;
};

struct Out {
    float* x;
    float* one_hot;
    float* charges;
    int64_t* batch;
    uint8_t* mask;
    int64_t* index;
    int64_t* num_nodes_present;
    float* props;
    float* props_context;
    int64_t* row;
    int64_t* col;
    int32_t* rowptr;
    int64_t* colperm;
    int32_t* colptr;
};

// the workspace: noff [B + 1], eoff [B + 1], mol [B] (int64), n [B] (int32)
struct Ws {
    int64_t* noff;
    int64_t* eoff;
    int64_t* mol;
    int32_t* n;
};
inline int64_t ws_bytes(int64_t B) { return ((2 * (B + 1) + B) * 8 + B * 4 + 255) & ~(int64_t)255; }
inline Ws ws_of(void* w, int64_t B) {
    Ws s;
    s.noff = (int64_t*)w;
    s.eoff = s.noff + (B + 1);
    s.mol = s.eoff + (B + 1);
    s.n = (int32_t*)(s.mol + B);
    return s;
}

__global__ void __launch_bounds__(THREADS) k_data_scan(const int64_t* __restrict__ atom_ptr, int64_t M, int64_t A, const int64_t* __restrict__ perm,
                                                        int64_t first, int64_t B, int pad_to, int64_t N, int64_t E, Ws ws, int32_t* flags) {
    __shared__ int64_t sn[THREADS], se[THREADS];
    const int tid = threadIdx.x;
    int64_t cn = 0, ce = 0;
    int bad = 0;
    for (int64_t base = 0; base < B; base += THREADS) {
        const int64_t b = base + tid;
        int64_t m = -1, n = 0, rows = 0;
        if (b < B) {
            m = perm[first + b];
            if (m < 0 || m >= M) {
                bad = 1;
                m = -1;
            } else {
                const int64_t a0 = atom_ptr[m], a1 = atom_ptr[m + 1];
                n = a1 - a0;
                if (a0 < 0 || n < 0 || a1 > A || n >= ((int64_t)1 << 15) || (pad_to > 0 && n > pad_to)) {
                    bad = 1;
                    n = 0;
                }
            }
            rows = pad_to > 0 ? pad_to : n;
        }
        const int64_t e = n * n;
        sn[tid] = rows;
        se[tid] = e;
        __syncthreads();
        for (int d = 1; d < THREADS; d <<= 1) {
            const int64_t an = tid >= d ? sn[tid - d] : 0, ae = tid >= d ? se[tid - d] : 0;
            __syncthreads();
            sn[tid] += an;
            se[tid] += ae;
            __syncthreads();
        }
        if (b < B) {
            ws.noff[b] = cn + sn[tid] - rows;
            ws.eoff[b] = ce + se[tid] - e;
            ws.mol[b] = m;
            ws.n[b] = (int32_t)n;
        }
        cn += sn[THREADS - 1];
        ce += se[THREADS - 1];
        __syncthreads();
    }
    if (tid == 0) {
        ws.noff[B] = cn;
        ws.eoff[B] = ce;
        if (cn != N || ce != E) bad = 1;
    }
    if (bad) atomicOr(flags, GCDM_DATA_FLAG_ACCOUNT);
}

__global__ void __launch_bounds__(THREADS) k_data_collate(Set s, Ws ws, Out o, const int32_t* __restrict__ ctx_cols, int C, int64_t B, int pad_to,
                                                           int64_t N, int64_t E) {
#pragma clang fp contract(off)
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t m = ws.mol[b];
    const int64_t n = ws.n[b];
    const int64_t ob = ws.noff[b], eb = ws.eoff[b];
    const int64_t rows = pad_to > 0 ? pad_to : n;
    const int64_t a0 = m >= 0 ? s.atom_ptr[m] : 0;
    // the molecule's slots
    if (tid == 0) {
        o.index[b] = m >= 0 ? s.index[m] : -1;
        o.num_nodes_present[b] = n;
        if (b == B - 1) {
            o.rowptr[N] = (int32_t)E;
            o.colptr[N] = (int32_t)E;
        }
    }
    for (int p = tid; p < s.P; p += THREADS) o.props[(int64_t)p * B + b] = m >= 0 ? s.props[(int64_t)p * s.M + m] : __builtin_nanf("");
    // its rows
    for (int64_t r = tid; r < rows; r += THREADS) {
        const int64_t v = ob + r;
        if (v >= N) break;
        const bool present = r < n;
        const int32_t zz = present ? s.z[a0 + r] : 0;
        o.charges[v] = (float)zz;
        o.batch[v] = b;
        o.mask[v] = present ? 1 : 0;
        const int32_t at = (int32_t)(eb + (r < n ? r : n) * n);
        o.rowptr[v] = at;
        o.colptr[v] = at;
    }
    for (int64_t k = tid; k < rows * 3; k += THREADS) {
        const int64_t r = k / 3, v = ob + r;
        if (v >= N) break;
        o.x[v * 3 + (k - r * 3)] = r < n ? s.pos[(a0 + r) * 3 + (k - r * 3)] : 0.f;
    }
    for (int64_t k = tid; k < rows * s.T; k += THREADS) {
        const int64_t r = k / s.T, v = ob + r;
        if (v >= N) break;
        const int t = (int)(k - r * s.T);
        o.one_hot[v * s.T + t] = (r < n && s.z[a0 + r] == s.species[t]) ? 1.f : 0.f;
    }
    for (int64_t k = tid; k < rows * C; k += THREADS) {
        const int64_t r = k / C, v = ob + r;
        if (v >= N) break;
        const int c = (int)(k - r * C);
        const int p = ctx_cols[c];
        const bool known = m >= 0 && p >= 0 && p < s.P;          // a column outside the properties reads nothing: NaN
        const float val = known ? s.props[(int64_t)p * s.M + m] : __builtin_nanf("");
        const float q = known ? (val - s.norm[2 * p]) / s.norm[2 * p + 1] : val;
        o.props_context[v * C + c] = q * (r < n ? 1.f : 0.f);
    }
    // its edges
    const int64_t ne = n * n;
    for (int64_t k = tid; k < ne; k += THREADS) {
        const int64_t e = eb + k;
        if (e >= E) break;
        const int64_t i = k / n, j = k - i * n;
        o.row[e] = ob + i;
        o.col[e] = ob + j;
        o.colperm[e] = eb + j * n + i;
    }
}

// order-preserving map of a float onto an unsigned key, and back
__device__ inline uint32_t f2key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float key2f(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ void __launch_bounds__(HIST_THREADS) k_data_hist(const int64_t* __restrict__ atom_ptr, const float* __restrict__ values, int64_t M, int S,
                                                             int nb, int32_t* counts, float* params, int32_t* members, int32_t* flags) {
#pragma clang fp contract(off)
    __shared__ uint32_t kmin[GCDM_DATA_MAX_SIZES], kmax[GCDM_DATA_MAX_SIZES];
    __shared__ int32_t cnt[GCDM_DATA_MAX_SIZES];
    const int tid = threadIdx.x;
    for (int n = tid; n < S; n += HIST_THREADS) {
        kmin[n] = 0xffffffffu;
        kmax[n] = 0u;
        cnt[n] = 0;
    }
    for (int64_t k = tid; k < (int64_t)S * nb; k += HIST_THREADS) counts[k] = 0;
    __threadfence();
    __syncthreads();
    int bad = 0;
    for (int64_t m = tid; m < M; m += HIST_THREADS) {
        const int64_t n = atom_ptr[m + 1] - atom_ptr[m];
        if (n < 0 || n >= S) {
            bad = 1;
            continue;
        }
        const uint32_t key = f2key(values[m]);
        atomicMin(&kmin[n], key);
        atomicMax(&kmax[n], key);
        atomicAdd(&cnt[n], 1);
    }
    if (bad) atomicOr(flags, GCDM_DATA_FLAG_ACCOUNT);
    __syncthreads();
    for (int n = tid; n < S; n += HIST_THREADS) {
        members[n] = cnt[n];
        params[2 * n] = cnt[n] ? key2f(kmin[n]) : 0.f;
        params[2 * n + 1] = cnt[n] ? key2f(kmax[n]) : 0.f;
    }
    const float nbf = (float)nb;
    for (int64_t m = tid; m < M; m += HIST_THREADS) {
        const int64_t n = atom_ptr[m + 1] - atom_ptr[m];
        if (n < 0 || n >= S) continue;
        const float mn = key2f(kmin[n]), mx = key2f(kmax[n]);
        const float range = (mx - mn) + 1e-12f;
        const float q = (values[m] - mn) / range * nbf;
        if (!(q >= 0.f && q <= nbf)) continue;          // a NaN value has no bin
        int i = (int)q;
        if (i == nb) i = nb - 1;
        atomicAdd(&counts[n * (int64_t)nb + i], 1);
    }
}

__global__ void __launch_bounds__(THREADS) k_data_sample(const int32_t* __restrict__ counts, const float* __restrict__ params,
                                                          const int32_t* __restrict__ members, const float* __restrict__ norm,
                                                          const int64_t* __restrict__ num_nodes, const float* __restrict__ u, int64_t B, int P, int S,
                                                          int nb, float* out, int32_t* flags) {
#pragma clang fp contract(off)
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (t >= B * P) return;
    const int64_t b = t / P;
    const int p = (int)(t - b * P);
    const int64_t n = num_nodes[b];
    const int64_t tab = n >= 0 && n < S ? (int64_t)p * S + n : -1;
    const int32_t count = tab >= 0 ? members[tab] : 0;
    if (count <= 0) {
        out[t] = __builtin_nanf("");
        atomicOr(flags, GCDM_DATA_FLAG_ABSENT_SIZE);
        return;
    }
    const float u1 = u[2 * t], u2 = u[2 * t + 1];
    int64_t k = (int64_t)floorf(u1 * (float)count);
    k = k < 0 ? 0 : (k > count - 1 ? count - 1 : k);
    const int32_t* c = counts + tab * nb;
    int64_t cum = 0;
    int i = 0;
    for (; i < nb - 1; ++i) {
        cum += c[i];
        if (cum > k) break;
    }
    const float mn = params[2 * tab], range = params[2 * tab + 1] - mn;
    const float nbf = (float)nb;
    const float left = (float)i / nbf * range + mn;
    const float right = (float)(i + 1) / nbf * range + mn;
    const float val = u2 * (right - left) + left;
    out[t] = (val - norm[2 * p]) / norm[2 * p + 1];
}

}  // namespace gdat

extern "C" {

int64_t gcdm_data_workspace_bytes(int64_t B) {
    GOPS_REQUIRE(B >= 0 && B < ((int64_t)1 << 31));
    return gdat::ws_bytes(B);
}

int gcdm_data_collate(const gcdm_data_set* set, const int64_t* perm, int64_t perm_len, int64_t first, int64_t B, int32_t pad_to,
                      const int32_t* ctx_cols, int32_t C, int64_t N, int64_t E, void* workspace, const gcdm_data_batch* out, int32_t* flags,
                      void* stream) {
    GOPS_REQUIRE(set && out);
    GOPS_REQUIRE(set->M >= 0 && set->A >= 0 && set->P >= 0 && set->P <= GCDM_DATA_MAX_PROPS && set->T >= 0 && set->T <= GCDM_DATA_MAX_TYPES);
    GOPS_REQUIRE(B >= 0 && B < ((int64_t)1 << 31) && first >= 0 && perm_len >= 0 && first <= perm_len && B <= perm_len - first);
    GOPS_REQUIRE(pad_to >= 0 && pad_to < (1 << 15) && C >= 0 && C <= set->P);
    GOPS_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) - 1 && E >= 0 && E < ((int64_t)1 << 31) - 1);
    GOPS_REQUIRE(pad_to == 0 || N == B * (int64_t)pad_to);
    if (B == 0) {
        GOPS_REQUIRE(N == 0 && E == 0);
        return 0;
    }
    GOPS_REQUIRE(set->M > 0 && set->atom_ptr && set->index && perm && workspace && flags);
    GOPS_REQUIRE(set->A == 0 || (set->z && set->pos));
    GOPS_REQUIRE(set->P == 0 || (set->props && set->norm && out->props));
    GOPS_REQUIRE(set->T == 0 || (set->species && out->one_hot) || N == 0);
    GOPS_REQUIRE(C == 0 || (ctx_cols && out->props_context) || N == 0);
    GOPS_REQUIRE(out->index && out->num_nodes_present && out->rowptr && out->colptr);
    GOPS_REQUIRE(N == 0 || (out->x && out->charges && out->batch && out->mask));
    GOPS_REQUIRE(E == 0 || (out->edge_index && out->colperm));
    gdat::Set s{set->atom_ptr, set->z, set->pos, set->props, set->species, set->norm, set->index, set->M, set->A, set->P, set->T};
    gdat::Out o{out->x, out->one_hot, out->charges, out->batch, out->mask, out->index, out->num_nodes_present, out->props, out->props_context,
                out->edge_index, out->edge_index ? out->edge_index + E : nullptr, out->rowptr, out->colperm, out->colptr};
    const gdat::Ws ws = gdat::ws_of(workspace, B);
    hipLaunchKernelGGL(gdat::k_data_scan, dim3(1), dim3(gdat::THREADS), 0, (hipStream_t)stream, set->atom_ptr, set->M, set->A, perm, first, B,
                       (int)pad_to, N, E, ws, flags);
    if (hipGetLastError() != hipSuccess) return -2;
    hipLaunchKernelGGL(gdat::k_data_collate, dim3((unsigned)B), dim3(gdat::THREADS), 0, (hipStream_t)stream, s, ws, o, ctx_cols, (int)C, B,
                       (int)pad_to, N, E);
    return GOPS_LAUNCH_OK();
}

int gcdm_data_prop_histogram(const int64_t* atom_ptr, const float* values, int64_t M, int32_t num_sizes, int32_t num_bins, int32_t* counts,
                             float* params, int32_t* members, int32_t* flags, void* stream) {
    GOPS_REQUIRE(M >= 0 && M < ((int64_t)1 << 31) && num_sizes >= 0 && num_sizes <= GCDM_DATA_MAX_SIZES && num_bins >= 1 &&
                 num_bins <= GCDM_DATA_MAX_BINS);
    if (num_sizes == 0) {
        GOPS_REQUIRE(M == 0);
        return 0;
    }
    GOPS_REQUIRE(counts && params && members && flags && (M == 0 || (atom_ptr && values)));
    hipLaunchKernelGGL(gdat::k_data_hist, dim3(1), dim3(gdat::HIST_THREADS), 0, (hipStream_t)stream, atom_ptr, values, M, (int)num_sizes,
                       (int)num_bins, counts, params, members, flags);
    return GOPS_LAUNCH_OK();
}

int gcdm_data_prop_sample(const int32_t* counts, const float* params, const int32_t* members, const float* norm, const int64_t* num_nodes,
                          const float* u, int64_t B, int32_t P, int32_t num_sizes, int32_t num_bins, float* out, int32_t* flags, void* stream) {
    GOPS_REQUIRE(B >= 0 && B < ((int64_t)1 << 31) && P >= 0 && P <= GCDM_DATA_MAX_PROPS && num_sizes >= 0 && num_sizes <= GCDM_DATA_MAX_SIZES &&
                 num_bins >= 1 && num_bins <= GCDM_DATA_MAX_BINS);
    if (B == 0 || P == 0) return 0;
    GOPS_REQUIRE(num_nodes && u && out && flags && norm && (num_sizes == 0 || (counts && params && members)));
    hipLaunchKernelGGL(gdat::k_data_sample, dim3(gops_blocks(B * P, gdat::THREADS)), dim3(gdat::THREADS), 0, (hipStream_t)stream, counts, params,
                       members, norm, num_nodes, u, B, (int)P, (int)num_sizes, (int)num_bins, out, flags);
    return GOPS_LAUNCH_OK();
}

}  // extern "C"
