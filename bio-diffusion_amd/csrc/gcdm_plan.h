// gcdm_plan.h -- the batch plan as the host builds it: every table a plan puts on the device, and the ONE table of the workspace's sub-buffers.
// Plain C++17, no HIP: gcdm_api.hip uploads what this builds (struct Plan there), tests/test_plan_host_cpu.py compiles it alone.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

// what a plan needs of the handle's dims (gcdm_create) and of the device
struct PlanDims {
    int D = 0, FinG = 0, Se = 0, Ve = 0, H0 = 0;      // 3 + F | 4-groups of node input features | edge scalar / vector channels | hidden vectors of msg0
    int sc = 0;                                       // self-conditioning
    int cus = 256;                                    // compute units (persistent edge-message workgroups: one per CU)
};

constexpr int PLAN_S = 256, PLAN_AGGW = 352;          // h_hidden_dim, width of one aggregated message row (GCDM_S, GCDM_AGGW of the kernels)

// ---- workspace: one device allocation, its sub-buffers in this order, each rounded up to 4 floats (16-byte aligned) ---------------
// X(member of Plan, name gcdm_debug_read serves the whole sub-buffer under or nullptr, floats); n = nodes, e = slots of the edge list, d = PlanDims
#define GCDM_WS_BUFFERS(X)                                                                                                                 \
    X(X0, "x0", 3 * n)          X(XC, "x", 3 * n)            X(FBAR, "fbar", 9 * n)        X(CHI0, nullptr, 12 * n)                             \
    X(HIN4, "hin", 4 * (size_t)d.FinG * n)                   X(H4, "h", PLAN_S * n)        X(CHI, "chi", 96 * n)                                \
    X(PQ4, "pq", 512 * n)       X(VDI, "vdi", (size_t)(d.H0 + 3) * 3 * n)                  X(VDJ, "vdj", (size_t)(d.H0 + 3) * 3 * n)            \
    X(AGG, nullptr, PLAN_AGGW * n)                           X(PART, nullptr, ((e + 31) / 32) * 2 * PLAN_AGGW)                                  \
    X(VEL, "vel", 3 * n)        X(EPS, nullptr, (size_t)d.D * n)                           X(EP4, "ep", (size_t)d.Se * e)                       \
    X(AL, "alpha", (size_t)d.Ve * e)                         X(U, "u", 3 * e)              X(FR, "frames", 9 * e)                               \
    X(PROF, nullptr, ((e + 31) / 32) * 192)                                                                                                \
    X(X0SC, nullptr, d.sc ? 3 * n : 0)                       X(BL, nullptr, d.sc ? (size_t)d.Ve * e : 0)   X(USC, nullptr, d.sc ? 3 * e : 0)    \
    X(ZK, nullptr, (size_t)d.D * n)                          X(ZU, nullptr, (size_t)d.D * n)                                                    \
    X(ZROW, nullptr, PLAN_AGGW)        /* never written: the workspace starts zeroed */                                                    \
    X(PQ4b, nullptr, 512 * n)   X(VDIb, nullptr, (size_t)(d.H0 + 3) * 3 * n)               X(VDJb, nullptr, (size_t)(d.H0 + 3) * 3 * n)
// (PQ4b / VDIb / VDJb: second set of the node-level msg0 halves -- layer l gathers set l & 1, its node tiles write set (l + 1) & 1)

#define GCDM_WS_ID(id, name, floats) WS_##id,
enum WsBuf { GCDM_WS_BUFFERS(GCDM_WS_ID) WS_COUNT };
#undef GCDM_WS_ID

struct WsEntry {
    const char* id;            // the member of Plan
    const char* read_as;       // gcdm_debug_read's name for the whole sub-buffer (readable count == allocated count), or nullptr
    size_t floats, off;        // count as asked for; offset in floats
};
struct WsLayout {
    WsEntry buf[WS_COUNT];
    size_t total = 0;          // floats
    std::string err;           // non-empty: refused (buffer-addressed kernels: < 4 GB)
    const WsEntry* find(const std::string& read_as) const {
        for (const WsEntry& b : buf)
            if (b.read_as && read_as == b.read_as) return &b;
        return nullptr;
    }
};

inline WsLayout ws_layout(const PlanDims& d, int64_t N, int64_t E) {
    const size_t n = (size_t)N, e = (size_t)E;
    WsLayout L{{
#define GCDM_WS_ENTRY(id, name, floats) {#id, name, (size_t)(floats), 0},
        GCDM_WS_BUFFERS(GCDM_WS_ENTRY)
#undef GCDM_WS_ENTRY
    }, 0, {}};
    for (WsEntry& b : L.buf) { b.off = L.total; L.total += (b.floats + 3) & ~size_t(3); }
    if (L.total * sizeof(float) >= ((size_t)1 << 32)) L.err = "gcdm_plan_batch: workspace exceeds 4 GB (buffer-addressed); split the batch";
    return L;
}

// ---- the plan's tables ------------------------------------------------------------------------------------------------------------
struct PlanScalars {
    int B = 0, N = 0, max_n = 0;
    int K = 0;                          // packed plan (gcdm_plan_batches): K sub-batches end to end; 0: an ordinary plan
    int64_t E = 0;                      // slots of the edge list (a packed plan pads it)
    int64_t E_real = 0;                 // edges without that padding
    int tail_tiles32 = 0;               // 32-node tiles of the fused launch's ready flags; 0: the plan is not in the fused launch's size range
};

struct PlanHost : PlanScalars {
    std::vector<int> noff, erow, ecol, ncnt, rowstart;
    std::vector<float> mask;            // 1 / 0 per node; empty when nothing is masked
    // packed plan (empty when K == 0): real edges of every 64-group of the edge list, sub-batch of every molecule, first node of every sub-batch
    std::vector<int> tvalid, mol_sub, sub_noff;
    // Fused layer launch (gcdm_layer_x3.hip.h), TailArgs::tab; empty when the plan does not qualify --
    // XCD x [8 x + 0..3]: first owned node tile, owned node tiles, edge tiles + owned node tiles (not read), rel_node_end |
    // [64 + t]: edge tiles node tile t waits for, | 1 << 16 when they reach into the next XCD's range
    std::vector<int> tail_tab;
};

// Builds the plan of B molecules of nn[b] atoms (node_mask: 1 / 0 per node or null; K > 0: packed, mols_per_batch[K] sums to B).
// 0, or -1 with the refusal in err and `out` untouched.
inline int build_plan_host(const PlanDims& d, int32_t B, const int32_t* nn, const uint8_t* node_mask, int32_t K, const int32_t* mols_per_batch,
                           PlanHost& out, std::string& err) {
    auto refuse = [&](const char* msg) { err = msg; return -1; };
    if (B <= 0 || !nn || K < 0 || (K > 0 && !mols_per_batch)) return refuse("gcdm_plan_batch: bad argument");
    PlanHost p;
    p.B = B; p.K = K;
    p.noff.assign((size_t)B + 1, 0);
    bool masked = false;
    // packed plan: first molecule of every sub-batch.  The edges of a sub-batch start on a 64-edge boundary of the flat edge list (the slots up to it repeat the last
    // edge in front of them and are no part of any row: EdgeMsgArgs::TVALID) -- tile boundaries then cut its rows exactly where they cut them in a plan of its own, which
    // is what makes its partial row sums (AggSrc), and so its results, those of the single run bit for bit.  64 covers both tile sizes.
    std::vector<char> sub_first((size_t)B, 0);
    int64_t packed_mols = 0;
    for (int k = 0; k < K; packed_mols += mols_per_batch[k], ++k) {
        if (mols_per_batch[k] <= 0 || packed_mols >= B) return refuse("gcdm_plan_batch: bad argument");
        sub_first[(size_t)packed_mols] = 1;
    }
    if (K > 0 && packed_mols != B) return refuse("gcdm_plan_batch: bad argument");
    for (int b = 0; b < B; ++b) {
        if (nn[b] <= 0) return refuse("gcdm_plan_batch: every molecule needs >= 1 atom");
        if (sub_first[b]) p.E = (p.E + 63) / 64 * 64;
        p.noff[b + 1] = p.noff[b] + nn[b];
        int64_t m = nn[b];
        if (node_mask) {            // edges only between unmasked atoms of a molecule (get_fully_connected_edge_index, gcpnet.py:1062-1065)
            m = 0;
            for (int i = 0; i < nn[b]; ++i) m += node_mask[p.noff[b] + i] ? 1 : 0;
            if (m == 0) return refuse("gcdm_plan_batch_masked: every molecule needs >= 1 unmasked atom (the reference's centroid is 0 / 0 otherwise)");
            masked |= m != nn[b];
        }
        p.E += m * m;
        p.max_n = std::max(p.max_n, (int)nn[b]);
    }
    if (!masked) node_mask = nullptr;
    if (p.E >= (int64_t)1 << 31) return refuse("gcdm_plan_batch: too many edges");
    // k_sample / k_prep stage one molecule in LDS (max_n * (3 + F) floats, 64 KB without an opt-in attribute)
    if (p.max_n > 4096 || (size_t)p.max_n * d.D * sizeof(float) > 65536)
        return refuse("gcdm_plan_batch: molecule too large (max_n * (3 + F) floats must fit 64 KB of LDS)");
    const int N = p.N = p.noff[B];
    const int64_t E = p.E;
    p.erow.resize((size_t)E); p.ecol.resize((size_t)E); p.ncnt.resize((size_t)N); p.rowstart.resize((size_t)N);
    std::vector<int>&erow = p.erow, &ecol = p.ecol, &ncnt = p.ncnt, &rowstart = p.rowstart;
    if (K > 0) p.tvalid.assign((size_t)((E + 63) / 64), 64);
    int64_t q = 0;
    for (int b = 0; b < B; ++b) {
        const int o = p.noff[b], n = nn[b];
        if (sub_first[b] && (q & 63)) {
            p.tvalid[(size_t)(q >> 6)] = (int)(q & 63);
            for (; q & 63; ++q) { erow[q] = erow[q - 1]; ecol[q] = ecol[q - 1]; }
        }
        int m = n;
        if (node_mask) { m = 0; for (int i = 0; i < n; ++i) m += node_mask[o + i] ? 1 : 0; }
        for (int i = 0; i < n; ++i) {
            const bool on = !node_mask || node_mask[o + i];
            ncnt[o + i] = on ? m : 0;           // a masked node has no edges: its aggregated row is zero (AggRow)
            rowstart[o + i] = (int)q;
            if (!on) continue;
            for (int j = 0; j < n; ++j)
                if (!node_mask || node_mask[o + j]) { erow[q] = o + i; ecol[q] = o + j; ++q; }
        }
    }
    if (K > 0 && (q & 63)) p.tvalid[(size_t)(q >> 6)] = (int)(q & 63);
    for (int i = 0; i < N; ++i) p.E_real += ncnt[i];
    if (node_mask) {
        p.mask.resize((size_t)N);
        for (int i = 0; i < N; ++i) p.mask[i] = node_mask[i] ? 1.f : 0.f;
    }
    if (K > 0) {            // the same topology, plus the sub-batch of each molecule and the first node of each sub-batch
        p.mol_sub.resize((size_t)B); p.sub_noff.assign((size_t)K + 1, 0);
        for (int k = 0, b = 0; k < K; ++k) {
            for (int j = 0; j < mols_per_batch[k]; ++j, ++b) p.mol_sub[b] = k;
            p.sub_noff[k + 1] = p.noff[b];
        }
    }
    // ---- node-tile queues of the fused layer launch (gcdm_layer_x3.hip.h): 64-edge tiles, XCD x owns the x-th contiguous eighth of the tile list (the partition of
    // k_edge_msg_x3's persistent loop); node tile t (T nodes) waits for the edge tiles first_tile(t) .. last_tile(t) of its rows and is owned by the XCD whose range
    // contains first_tile(t).  A plan qualifies when nothing is masked, the launch is persistent and no node tile spans three XCDs.
    const int wgs = d.cus / 8 * 8;
    if (!node_mask && K == 0 && E > (int64_t)64 * wgs && wgs >= 8) {          // (a packed plan runs two launches per layer: its padded edge list is not what the queues below describe)
        const int G = (int)((E + 63) / 64), base = G >> 3, rem = G & 7;
        int xs[9];
        for (int x = 0; x <= 8; ++x) xs[x] = x * base + std::min(x, rem);
        auto xcd_of_tile = [&](int g) { int x = 0; while (x < 7 && g >= xs[x + 1]) ++x; return x; };
        constexpr int T = 32;                              // nodes per node tile of the tail role (NodeTailRole<32>)
        const int NTt = (N + T - 1) / T;
        std::vector<int> tab(64 + (size_t)NTt, 0);
        std::vector<std::vector<std::pair<int, int>>> owned(8);          // per XCD: (edge tile the node item stands behind, node tile)
        bool ok = true;
        for (int t = 0; t < NTt && ok; ++t) {
            const int nf = t * T, nl = std::min(nf + T, N) - 1;
            const int ft = rowstart[nf] >> 6, lt = (rowstart[nl] + ncnt[nl] - 1) >> 6;
            const int owner = xcd_of_tile(ft), xl = xcd_of_tile(lt);
            if (xl > owner + 1 || lt - ft + 1 > 0xffff) ok = false;
            tab[64 + t] = (lt - ft + 1) | ((xl != owner ? 1 : 0) << 16);
            owned[owner].push_back({lt, t});
        }
        for (int x = 0; x < 8 && ok; ++x) {
            tab[8 * x] = owned[x].empty() ? 0 : owned[x][0].second;
            tab[8 * x + 1] = (int)owned[x].size();
            tab[8 * x + 2] = xs[x + 1] - xs[x] + (int)owned[x].size();
            if (x >= 1) {                                                // rows of XCD x's first tiles that belong to the boundary node tile owned by XCD x - 1
                const int tb = erow[(size_t)xs[x] * 64] / T;
                if ((rowstart[tb * T] >> 6) < xs[x]) tab[8 * x + 3] = std::min((tb + 1) * T, N);
            }
        }
        if (ok) p.tail_tab = std::move(tab);
        p.tail_tiles32 = (N + 31) / 32;          // (the counters exist in the size range, with or without the table)
    }
    out = std::move(p);
    return 0;
}
