"""What tests/test_data_cpu.py and tests/test_data_gpu.py share: the fixture of tests/golden/make_data_golden.py, a plain-torch statement of a
collated batch for shapes the fixture does not hold, synthetic data sets, and the draw twice: the reference's expressions in torch on the CPU, and the kernel's rule in numpy fp32."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_small.npz")
BATCHES = ("all", "tail", "one", "wave")
CONDITIONING = ["alpha", "U0"]
PROPERTY_KEYS = ["alpha", "U0", "U0_thermo"]
A_MAX = 9
_FIXTURE = None


def fixture():
    """The fixture as a dict of numpy arrays, loaded once and never written to."""
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(GOLDEN) as g:
            _FIXTURE = {k: g[k] for k in g.files}
        for v in _FIXTURE.values():
            v.setflags(write=False)
    return _FIXTURE


def raw():
    g = fixture()
    return {k[len("raw_"):]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith("raw_")}


def expected_batch(name, layout):
    """The reference's batch `name`: as stored (padded), or its present rows (compact)."""
    g = fixture()
    keep = torch.from_numpy(g[f"{name}_mask"].copy())
    rows = keep if layout == "compact" else torch.ones_like(keep)
    out = {k: torch.from_numpy(g[f"{name}_{k}"].copy())[rows] for k in ("x", "one_hot", "charges", "mask", "batch", "props_context")}
    out["charges"] = out["charges"].reshape(-1, 1)
    for k in ("index", "alpha", "U0", "U0_thermo"):
        out[k] = torch.from_numpy(g[f"{name}_{k}"].copy())
    out["edge_index"] = torch.from_numpy(g[f"{name}_fc_compact" if layout == "compact" else f"{name}_fc"].copy())
    out["num_nodes_present"] = torch.zeros(len(out["index"]), dtype=torch.int64).index_add_(0, torch.from_numpy(g[f"{name}_batch"].copy()), keep.long())
    return out


def synthetic_raw(sizes, a_max=None, species=(1, 6, 7, 8, 9), seed=0, props=("alpha",)):
    """A processed dictionary of len(sizes) molecules (fp32 properties)."""
    rng = np.random.default_rng(seed)
    a_max = max(sizes) if a_max is None else a_max
    M = len(sizes)
    charges = np.zeros((M, a_max), dtype=np.int64)
    positions = np.zeros((M, a_max, 3), dtype=np.float32)
    for m, n in enumerate(sizes):
        charges[m, :n] = rng.choice(species, size=n)
        positions[m, :n] = rng.standard_normal((n, 3)).astype(np.float32)
    out = dict(num_atoms=torch.tensor(sizes, dtype=torch.int64), charges=torch.from_numpy(charges), positions=torch.from_numpy(positions),
               index=torch.arange(M, dtype=torch.int64) + 7)
    for p in props:
        out[p] = torch.from_numpy((rng.standard_normal(M) * 5 + 50).astype(np.float32))
    return out


def torch_batch(rawd, species, molecules, pad_to, norm, ctx_keys, prop_keys):
    """A collated batch of `molecules` (indices into rawd) stated with plain torch on the CPU, layout by pad_to (0 = compact)."""
    xs, ohs, chs, bis, mks, ctxs = [], [], [], [], [], []
    sp = torch.as_tensor(species, dtype=torch.int64)
    for b, m in enumerate(molecules):
        n = int(rawd["num_atoms"][m])
        rows = pad_to if pad_to else n
        z = torch.zeros(rows, dtype=torch.int64)
        z[:n] = rawd["charges"][m, :n]
        x = torch.zeros(rows, 3)
        x[:n] = rawd["positions"][m, :n]
        mask = torch.arange(rows) < n
        xs.append(x), chs.append(z.to(torch.float32).reshape(-1, 1)), ohs.append((z.unsqueeze(-1) == sp.unsqueeze(0)).to(torch.float32))
        bis.append(torch.full((rows,), b, dtype=torch.int64)), mks.append(mask)
        c = torch.stack([((rawd[k][m].to(torch.float32) - norm[k][0]) / norm[k][1]).expand(rows) for k in ctx_keys], dim=-1) if ctx_keys \
            else torch.zeros(rows, 0)
        ctxs.append(c * mask.unsqueeze(-1))
    mol = torch.as_tensor(molecules, dtype=torch.int64)
    out = dict(x=torch.cat(xs), one_hot=torch.cat(ohs), charges=torch.cat(chs), batch=torch.cat(bis), mask=torch.cat(mks), index=rawd["index"][mol],
               num_nodes_present=rawd["num_atoms"][mol].to(torch.int64), props_context=torch.cat(ctxs))
    for k in prop_keys:
        out[k] = rawd[k][mol].to(torch.float32)
    bi, mk = out["batch"], out["mask"]
    ei = torch.stack(torch.where(bi[:, None] == bi[None, :]))                # get_fully_connected_edge_index (gcpnet.py:1054-1066)
    out["edge_index"] = ei[:, mk[ei[0]] & mk[ei[1]]]
    return out


def csr_of(edge_index, N):
    """rowptr, colperm, colptr of a row-sorted edge list, stated with torch on the CPU."""
    row, col = edge_index
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=N), 0)
    colperm = torch.sort(col, stable=True).indices
    colptr = torch.zeros(N + 1, dtype=torch.int64)
    colptr[1:] = torch.cumsum(torch.bincount(col, minlength=N), 0)
    return rowptr.to(torch.int32), colperm, colptr.to(torch.int32)


def draw_torch(counts, params, members, norm, num_nodes, u):
    """PropertiesDistribution.sample of the reference (src/models/__init__.py:384-415) with the bin and the uniform given: torch fp32 on the CPU,
    the reference's expressions.  counts [P][S][nb], params [P][S][2], members [P][S], norm [P][2], num_nodes [B], u [B][P][2]."""
    counts, params, norm, u = (torch.tensor(np.array(v)) for v in (counts, params, norm, u))
    nb = counts.shape[-1]
    out = torch.full((len(num_nodes), counts.shape[0]), float("nan"))
    for b, n in enumerate(int(v) for v in num_nodes):
        for p in range(counts.shape[0]):
            count = int(members[p][n]) if 0 <= n < counts.shape[1] else 0
            if count <= 0:
                continue
            k = min(int(torch.floor(u[b, p, 0] * torch.tensor(count, dtype=torch.float32))), count - 1)
            idx = torch.tensor([int((torch.cumsum(counts[p, n].long(), 0) > k).nonzero()[0])])
            prop_range = params[p, n, 1] - params[p, n, 0]
            left = idx / nb * prop_range + params[p, n, 0]
            right = (idx + 1) / nb * prop_range + params[p, n, 0]
            val = u[b, p, 1:2] * (right - left) + left
            out[b, p] = ((val - norm[p, 0]) / norm[p, 1])[0]
    return out


def sample_reference(counts: np.ndarray, params: np.ndarray, members: np.ndarray, norm: np.ndarray, num_nodes: np.ndarray, u: np.ndarray) -> np.ndarray:
    """The sampling rule of gcdm_data_prop_sample (include/gcdm_data.h) in numpy fp32, operation for operation: counts [P][S][nb], params [P][S][2], members [P][S],
    norm [P][2], num_nodes [B], u [B][P][2] -> [B][P]; NaN where the size has no members."""
    f = np.float32
    Pn, S, nb = counts.shape
    B = len(num_nodes)
    out = np.full((B, Pn), np.nan, dtype=f)
    for b in range(B):
        n = int(num_nodes[b])
        for p in range(Pn):
            if not (0 <= n < S) or members[p, n] <= 0:
                continue
            count = int(members[p, n])
            k = min(max(int(np.floor(f(u[b, p, 0]) * f(count))), 0), count - 1)
            cum = np.cumsum(counts[p, n].astype(np.int64))
            i = min(int(np.searchsorted(cum, k, side="right")), nb - 1)
            mn = f(params[p, n, 0])
            rng = f(f(params[p, n, 1]) - mn)
            left = f(f(f(f(i) / f(nb)) * rng) + mn)
            right = f(f(f(f(i + 1) / f(nb)) * rng) + mn)
            val = f(f(f(u[b, p, 1]) * f(right - left)) + left)
            out[b, p] = f(f(val - f(norm[p, 0])) / f(norm[p, 1]))
    return out
