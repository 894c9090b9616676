"""Writes tests/golden/data_small.npz: the unmodified reference data path (ProcessedDataset._featurize_as_graph, prepare_context,
compute_mean_mad_from_dataloader, GCPNetDynamics.get_fully_connected_edge_index, PropertiesDistribution; imported under
ref_harness.install_stubs() plus the one further stub made here, torch_geometric.utils.unbatch) on a nine-molecule processed dictionary.

The fixture holds data only: the raw dictionary (``raw_*``), the reference's statistics, and per batch (``<name>_*``) the PyG-style
concatenation of the reference's own items, prepare_context's output and the fully connected edge index of the padded batch and of its present
rows; per num_bins (7, 1000) the reference's histograms as integer counts, (min, max) and member counts per molecule size.

The raw set: A_max = 9, sizes 1 2 3 5 5 9 4 8 and one all-zero-charge molecule (dropped by the reference's filter), species 1 6 7 8 9, properties
``alpha`` and ``U0`` (+ ``U0_thermo``) in fp32 -- the reference bins in the data's dtype, and fp32 is what lives on the device.  The two
five-atom molecules share one alpha (a size group of range 1e-12) and differ in U0 (one value equal to its group's maximum: the num_bins fold);
every other size is a single-member group.

    python tests/golden/make_data_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh                      # noqa: E402

A_MAX = 9
SIZES = [1, 2, 3, 5, 0, 5, 9, 4, 8]          # the fifth raw molecule is the all-zero one
SPECIES = [1, 6, 7, 8, 9]
CONDITIONING = ["alpha", "U0"]
BATCHES = {                                   # name: (perm over the filtered set, first, B)
    "all": ([0, 1, 2, 3, 4, 5, 6, 7], 0, 8),
    "tail": ([6, 2, 7, 0, 3, 5, 1, 4], 5, 3),
    "one": ([0], 0, 1),
    "wave": ([6, 5, 7], 0, 3),                # 4, 9 and 8 atoms: 16, 81 and 64 edges
}
NUM_BINS = (7, 1000)


def raw_data():
    rng = np.random.default_rng(20)
    M = len(SIZES)
    charges = np.zeros((M, A_MAX), dtype=np.int64)
    positions = np.zeros((M, A_MAX, 3), dtype=np.float32)
    for m, n in enumerate(SIZES):
        charges[m, :n] = rng.choice(SPECIES, size=n)
        positions[m, :n] = rng.standard_normal((n, 3)).astype(np.float32) * 1.5
        positions[m, n:] = 7.0                  # garbage behind the atoms: the reference zeroes it through the mask
    charges[6, :5] = SPECIES                    # every species occurs
    alpha = (rng.standard_normal(M) * 8 + 75).astype(np.float32)
    alpha[5] = alpha[3]                         # the two five-atom molecules: one value
    U0 = (rng.standard_normal(M) * 10 - 400).astype(np.float32)
    thermo = (rng.standard_normal(M) * 3 - 390).astype(np.float32)
    return dict(num_atoms=np.array(SIZES, dtype=np.int64), charges=charges, positions=positions, index=np.arange(100, 100 + M, dtype=np.int64),
                alpha=alpha, U0=U0, U0_thermo=thermo)


def _unbatch(src, batch, dim=0):
    sizes = torch.bincount(batch).tolist()
    return src.split(sizes, dim)


def main():
    assert rh.reference_available(), "reference checkout not found"
    rh.install_stubs()
    tgu = types.ModuleType("torch_geometric.utils")
    tgu.unbatch = _unbatch
    sys.modules["torch_geometric.utils"] = tgu
    sys.modules["torch_geometric"].utils = tgu
    import importlib
    edm_dataset = importlib.import_module("src.datamodules.components.edm_dataset")
    edm_utils = importlib.import_module("src.datamodules.components.edm.utils")
    models = importlib.import_module("src.models")
    gcpnet = importlib.import_module("src.models.components.gcpnet")

    raw = raw_data()
    out = {f"raw_{k}": v for k, v in raw.items()}
    ds = edm_dataset.ProcessedDataset({k: torch.from_numpy(v.copy()) for k, v in raw.items()}, shuffle=False)
    loader = types.SimpleNamespace(dataset=ds)
    assert ds.data["charges"].shape[0] == 8 and [int(s) for s in ds.included_species] == SPECIES
    out["included_species"] = ds.included_species.numpy()
    out["num_atoms"] = ds.data["num_atoms"].numpy()
    for k, (mean, std) in ds.stats.items():
        out[f"stats_{k}"] = np.array([mean.item(), std.item()], dtype=np.float32)
    norms = models.compute_mean_mad_from_dataloader(loader, CONDITIONING)
    norms2 = edm_utils.compute_mean_mad_from_dataloader(loader, CONDITIONING)
    for k in CONDITIONING:
        assert torch.equal(norms[k]["mean"], norms2[k]["mean"]) and torch.equal(norms[k]["mad"], norms2[k]["mad"])
        out[f"norm_{k}"] = np.array([norms[k]["mean"].item(), norms[k]["mad"].item()], dtype=np.float32)

    for name, (perm, first, B) in BATCHES.items():
        items = [ds[m] for m in perm[first:first + B]]
        cat = lambda key: torch.cat([it[key] for it in items])
        batch = rh._Batch(x=cat("x"), one_hot=cat("one_hot"), charges=cat("charges"), mask=cat("mask"), index=cat("index"),
                          batch=torch.repeat_interleave(torch.arange(B), A_MAX), alpha=cat("alpha"), U0=cat("U0"), U0_thermo=cat("U0_thermo"))
        ctx = edm_utils.prepare_context(CONDITIONING, batch, norms)
        fc = gcpnet.GCPNetDynamics.get_fully_connected_edge_index(batch.batch, batch.mask)
        fc_compact = gcpnet.GCPNetDynamics.get_fully_connected_edge_index(batch.batch[batch.mask])
        out[f"{name}_perm"], out[f"{name}_first"] = np.array(perm, dtype=np.int64), np.int64(first)
        for key in ("x", "one_hot", "charges", "mask", "index", "batch", "alpha", "U0", "U0_thermo"):
            out[f"{name}_{key}"] = batch[key].numpy()
        out[f"{name}_props_context"], out[f"{name}_fc"], out[f"{name}_fc_compact"] = ctx.numpy(), fc.numpy(), fc_compact.numpy()
        assert ctx.dtype == torch.float32 and batch.x.dtype == torch.float32

    S = int(ds.data["num_atoms"].max()) + 1
    for nb in NUM_BINS:
        pd = models.PropertiesDistribution(loader, CONDITIONING, device="cpu", num_bins=nb, normalizer=norms)
        counts, params, members = np.zeros((2, S, nb), dtype=np.int32), np.zeros((2, S, 2), dtype=np.float32), np.zeros((2, S), dtype=np.int32)
        for p, key in enumerate(CONDITIONING):
            for n, d in pd.distributions[key].items():
                k = int((ds.data["num_atoms"] == n).sum())
                c = d["probs"].probs.double() * k
                assert float((c - c.round()).abs().max()) < 1e-4
                counts[p, n], members[p, n] = c.round().to(torch.int32).numpy(), k
                params[p, n] = [d["params"][0].item(), d["params"][1].item()]
        assert counts.sum() == 2 * 8
        out[f"hist{nb}_counts"], out[f"hist{nb}_params"], out[f"hist{nb}_members"] = counts, params, members
    assert out["hist7_counts"][1, 5, 6] == 1 and out["hist7_counts"][0, 5, 0] == 2          # the fold; the range-1e-12 group
    path = os.path.join(HERE, "data_small.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
