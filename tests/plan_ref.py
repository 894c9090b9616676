"""The batch plan of libgcdm_hip.so written down from its rules in numpy (not from csrc/gcdm_plan.h): edge list, row tables, the packed plan's padding,
the node-tile queue table of the fused layer launch, and the workspace's sub-buffer list.  tests/test_plan_host_cpu.py holds the header to it; the GPU
suite takes the workspace size from it."""
import numpy as np

S, AGGW = 256, 352          # h_hidden_dim, width of one aggregated message row (S + 3 V)

# PlanDims of the two datasets: D = 3 + F, FinG = 4-groups of [h | (h_sc) | t | ctx], H0 = (2 V + Ve) / 4
DIMS = {
    "qm9": dict(D=9, FinG=2, Se=64, Ve=16, H0=20, sc=0),
    "qm9_sc": dict(D=9, FinG=4, Se=64, Ve=16, H0=20, sc=1),
    "geom": dict(D=19, FinG=5, Se=16, Ve=8, H0=18, sc=0),
    "geom_sc": dict(D=19, FinG=9, Se=16, Ve=8, H0=18, sc=1),
}


def ws_buffers(d, n, e):
    """(name, floats) of the workspace's sub-buffers in allocation order, as the parent commit's plan took them."""
    g32 = (e + 31) // 32
    vd = (d["H0"] + 3) * 3 * n
    sc = d["sc"]
    return [("X0", 3 * n), ("XC", 3 * n), ("FBAR", 9 * n), ("CHI0", 12 * n), ("HIN4", 4 * d["FinG"] * n), ("H4", S * n), ("CHI", 96 * n),
            ("PQ4", 512 * n), ("VDI", vd), ("VDJ", vd), ("AGG", AGGW * n), ("PART", g32 * 2 * AGGW), ("VEL", 3 * n), ("EPS", d["D"] * n),
            ("EP4", d["Se"] * e), ("AL", d["Ve"] * e), ("U", 3 * e), ("FR", 9 * e), ("PROF", g32 * 192),
            ("X0SC", 3 * n if sc else 0), ("BL", d["Ve"] * e if sc else 0), ("USC", 3 * e if sc else 0),
            ("ZK", d["D"] * n), ("ZU", d["D"] * n), ("ZROW", AGGW), ("PQ4b", 512 * n), ("VDIb", vd), ("VDJb", vd)]


def ws_offsets(d, n, e):
    """[(name, floats, offset)] and the total, every sub-buffer rounded up to 4 floats."""
    out, off = [], 0
    for name, cnt in ws_buffers(d, n, e):
        out.append((name, cnt, off))
        off += (cnt + 3) // 4 * 4
    return out, off


def first_count_over_4gb(d, atoms):
    """Smallest number of `atoms`-atom molecules whose workspace reaches 4 GB (bisection: the size grows with the count)."""
    over = lambda b: ws_offsets(d, atoms * b, atoms * atoms * b)[1] * 4 >= 1 << 32
    lo, hi = 1, 2
    while not over(hi):
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if over(mid) else (mid, hi)
    return hi


def plan(nn, mask=None, per_batch=None, cus=8):
    """dict of the plan's scalars and tables.  mask: 1 / 0 per node or None; per_batch: molecules of every sub-batch of a packed plan or None."""
    nn = [int(v) for v in nn]
    B, N = len(nn), sum(nn)
    noff = np.concatenate([[0], np.cumsum(nn)]).astype(np.int64)
    on = np.ones(N, bool) if mask is None else np.asarray(mask).astype(bool)
    if on.all():
        mask = None                                      # an all-true mask is no mask
    K = 0 if per_batch is None else len(per_batch)
    first = set(np.concatenate([[0], np.cumsum(per_batch)])[:-1].tolist()) if K else set()
    erow, ecol, real = [], [], []
    ncnt, rowstart = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for b in range(B):
        if b in first:                                   # a sub-batch starts on a 64-edge boundary: the slots up to it repeat the last edge
            pad = -len(erow) % 64
            erow += [erow[-1]] * pad if pad else []
            ecol += [ecol[-1]] * pad if pad else []
            real += [False] * pad
        o = int(noff[b])
        idx = [o + i for i in range(nn[b]) if on[o + i]]
        for i in range(o, o + nn[b]):
            rowstart[i] = len(erow)
            if on[i]:                                    # edges only between the unmasked atoms of a molecule, self edge included, row-major
                ncnt[i] = len(idx)
                erow += [i] * len(idx)
                ecol += idx
                real += [True] * len(idx)
    E = len(erow)
    p = dict(B=B, N=N, max_n=max(nn), K=K, E=E, E_real=int(ncnt.sum()), noff=noff, erow=np.array(erow), ecol=np.array(ecol), ncnt=ncnt,
             rowstart=rowstart, mask=np.zeros(0) if mask is None else on.astype(np.float32), tvalid=np.zeros(0, int), mol_sub=np.zeros(0, int),
             sub_noff=np.zeros(0, int), tail_tab=np.zeros(0, int), tail_tiles32=0)
    if K:
        r = np.zeros((E + 63) // 64 * 64, int)
        r[:E] = real
        p["tvalid"] = r.reshape(-1, 64).sum(1)           # real edges of every 64-group
        p["mol_sub"] = np.repeat(np.arange(K), per_batch)
        p["sub_noff"] = noff[np.concatenate([[0], np.cumsum(per_batch)])]
    # node-tile queues of the fused launch: unmasked, not packed, more 64-edge tiles than one round of cus/8*8 persistent workgroups
    wgs = cus // 8 * 8
    if mask is None and K == 0 and E > 64 * wgs and wgs >= 8:
        p["tail_tiles32"] = (N + 31) // 32
        G = (E + 63) // 64
        xs = [x * (G // 8) + min(x, G % 8) for x in range(9)]          # XCD x owns the edge tiles xs[x] .. xs[x + 1] - 1
        xcd = lambda g: max(x for x in range(8) if xs[x] <= g)
        NT = (N + 31) // 32
        tab = np.zeros(64 + NT, np.int64)
        owned = [[] for _ in range(8)]
        for t in range(NT):
            nf, nl = 32 * t, min(32 * t + 32, N) - 1
            ft, lt = rowstart[nf] >> 6, (rowstart[nl] + ncnt[nl] - 1) >> 6          # the edge tiles that hold the node tile's rows
            if xcd(lt) > xcd(ft) + 1:
                return p                                  # a node tile over three XCDs: no table
            tab[64 + t] = (lt - ft + 1) | ((1 << 16) if xcd(lt) != xcd(ft) else 0)
            owned[xcd(ft)].append(t)
        for x in range(8):
            tab[8 * x] = owned[x][0] if owned[x] else 0
            tab[8 * x + 1] = len(owned[x])
            tab[8 * x + 2] = xs[x + 1] - xs[x] + len(owned[x])
            if x >= 1:                                    # the node tile that XCD x's first edge tile belongs to, when XCD x - 1 owns it: its end node
                tb = p["erow"][xs[x] * 64] // 32
                if rowstart[tb * 32] >> 6 < xs[x]:
                    tab[8 * x + 3] = min((tb + 1) * 32, N)
        p["tail_tab"] = tab
    return p
