"""Device-resident molecule data sets: the whole processed QM9 / GEOM split lives in HBM and a training batch is built from it by two launches
(include/gcdm_data.h), with no host round trip.

What it replaces in the reference (BioinfoMachineLearning/bio-diffusion): ``ProcessedDataset`` + the PyG ``DataLoader`` of
``EDMDataModule.train_dataloader()`` (src/datamodules/components/edm_dataset.py:79-226), ``prepare_context``
(src/datamodules/components/edm/utils.py:333-382), ``compute_mean_mad_from_dataloader`` and ``PropertiesDistribution``
(src/models/__init__.py:63-76, 311-415).  A batch also carries what the network would otherwise rebuild from it with device-to-host copies:
the fully connected graph with its CSR (``fc_graph``), ``all_present`` and ``num_graphs``.

GEOM-Drugs comes from the reference's own conformer file (``GEOM_drugs_30.npy`` + ``GEOM_permutation.npy``): ``MoleculeDataset.geom_splits``
uploads it in chunks and segments, strips (``remove_h``), filters, splits and size-sorts it in HBM (include/gcdm_geom.h), replacing
``load_split_data`` + ``GeomDrugsDataset`` (src/datamodules/components/edm/build_geom_dataset.py:89-212); ``loader(sequential=True)`` gives the
same-size batches of its ``CustomBatchSampler`` (:215-242).

Out of scope: downloading or pre-processing raw QM9 / GEOM (``extract_conformers`` from the msgpack), ``remove_h`` for QM9, sequential batches
under data-parallel ranks, overlapping the upload with the ingestion or the collation with the previous step on a side stream, Lightning.
There is no CPU path: the data set lives on an MI355X.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Any, Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import _native, ops
from .config import AttrDict

_NOT_PROPERTIES = ("num_atoms", "charges", "positions", "index", "one_hot", "atom_mask")          # edm_dataset.py:206


def _lib():
    return _native.load_ops()


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _chk(status: int, what: str) -> None:
    if status != 0:
        raise _native.NativeError(f"{what} failed with status {status} (libgcdm_ops.so)")


def _cpu(v: Any) -> torch.Tensor:
    return v.detach().cpu() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))


def distributed_indices(length: int, shuffle: bool, seed: int, epoch: int, rank: int, world: int) -> torch.Tensor:
    """The index stream of ``torch.utils.data.DistributedSampler(range(length), world, rank, shuffle, seed)`` after ``set_epoch(epoch)``:
    ``randperm`` from a CPU generator seeded ``seed + epoch``, padded by wrap-around to a multiple of ``world``, then ``[rank::world]``."""
    if not (0 <= rank < world):
        raise ValueError(f"rank {rank} outside [0, {world})")
    if shuffle:
        g = torch.Generator()
        g.manual_seed(int(seed) + int(epoch))
        idx = torch.randperm(length, generator=g)
    else:
        idx = torch.arange(length)
    total = math.ceil(length / world) * world
    pad = total - length
    if pad > 0 and length > 0:
        idx = torch.cat([idx] + [idx] * math.ceil(pad / length))[:total]
    return idx[rank:total:world].contiguous()


def batch_accounting(sizes: np.ndarray, pad_to: int):
    """(N, E, all_present) of a batch of molecules with ``sizes`` atoms: rows and edges (all ordered pairs, self-loops included)."""
    sizes = np.asarray(sizes, dtype=np.int64)
    N = int(len(sizes) * pad_to) if pad_to > 0 else int(sizes.sum())
    return N, int((sizes * sizes).sum()), bool(pad_to == 0 or (sizes == pad_to).all())


# the atomic numbers of dataset_info("geom")["atom_decoder"], in its order: the one-hot columns of a GEOM-Drugs batch
GEOM_ATOMIC_NUMBERS = (1, 5, 6, 7, 8, 9, 13, 14, 15, 16, 17, 33, 35, 53, 80, 83)
GEOM_SPLITS = ("train", "valid", "test")


def geom_split_orders(sizes: np.ndarray, permutation: np.ndarray, val_proportion: float = 0.1, test_proportion: float = 0.1,
                      filter_size: Optional[int] = None) -> Dict[str, Any]:
    """``{split: (order, split_indices)}`` from the atom counts of the file's molecules, as ``load_split_data`` + ``GeomDrugsDataset`` make them
    (build_geom_dataset.py:104-128, 157-161): molecules of more than ``filter_size`` atoms leave, ``permutation`` indexes what is left, the cuts
    are ``[valid | test | train]``, and each split is sorted by ``np.argsort`` of its sizes -- the reference's very call, whose order among equal
    sizes is numpy's.  ``order`` names molecules of the file, ``split_indices`` the positions in the sorted split at which the size changes."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    kept = np.arange(len(sizes)) if filter_size is None else np.flatnonzero(sizes <= filter_size)
    if filter_size is not None and len(kept) == 0:
        raise ValueError("No molecules left after filter.")
    perm = np.asarray(permutation).reshape(-1).astype(np.int64)
    if len(perm) and (int(perm.min()) < -len(kept) or int(perm.max()) >= len(kept)):
        raise IndexError(f"the permutation names molecule {int(perm.max())} (or {int(perm.min())}) of {len(kept)}")
    picked = kept[perm]
    val_index = int(len(picked) * val_proportion)
    test_index = val_index + int(len(picked) * test_proportion)
    out = {}
    for name, ids in (("valid", picked[:val_index]), ("test", picked[val_index:test_index]), ("train", picked[test_index:])):
        lengths = sizes[ids]
        out[name] = (ids[np.argsort(lengths)], np.unique(np.sort(lengths), return_index=True)[1][1:].astype(np.int64))
    return out


def sequential_batches(n: int, batch_size: int, drop_last: bool, split_indices: np.ndarray):
    """(first, count) of ``CustomBatchSampler``'s batches over ``range(n)`` (build_geom_dataset.py:215-242): consecutive indices, a batch closed
    at ``batch_size`` or where ``idx + 1`` is in ``split_indices``; what is left open at the end is dropped by ``drop_last`` only."""
    cuts = np.unique(np.asarray(split_indices, dtype=np.int64).reshape(-1))
    cuts = cuts[(cuts >= 1) & (cuts <= n)]
    edges = np.concatenate(([0], cuts, [n])).astype(np.int64)
    firsts, counts = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for a, b in zip(edges[:-1], edges[1:]):
        if b > a:
            first = np.arange(a, b, batch_size, dtype=np.int64)
            firsts.append(first)
            counts.append(np.minimum(batch_size, b - first))
    firsts, counts = np.concatenate(firsts), np.concatenate(counts)
    open_end = len(counts) > 0 and counts[-1] < batch_size and not (len(cuts) and cuts[-1] == n)
    if drop_last and open_end:
        firsts, counts = firsts[:-1], counts[:-1]
    return firsts, counts


class MoleculeDataset:
    """The reference's processed dictionary (``num_atoms [M]``, ``charges [M, A_max]``, ``positions [M, A_max, 3]``, optional ``index``, 1-D
    property arrays, ``<key>_thermo`` companions) after ProcessedDataset's filters, uploaded once in a ragged layout; the sizes stay mirrored on
    the host.  ``num_pts`` limits what a loader iterates to the first ``num_pts`` molecules (statistics and histograms see all, as in the
    reference); ``filter_n_atoms`` keeps molecules of that many atoms (edm/dataset.py:114-123; ``stats`` is computed before it, as there).
    ``conditioning``: the property keys whose normalised per-node copies make ``props_context``."""

    def __init__(self, data: Dict[str, Any], device, included_species=None, subtract_thermo: bool = True, remove_zero_charge_molecules: bool = True,
                 num_pts: int = -1, filter_n_atoms: Optional[int] = None, conditioning: Sequence[str] = ()):
        data = {k: _cpu(v) for k, v in data.items()}
        for key in ("num_atoms", "charges", "positions"):
            if key not in data:
                raise KeyError(f"the processed dictionary has no {key!r}")
        M0 = data["charges"].shape[0]
        if "index" not in data:
            data["index"] = torch.arange(M0, dtype=torch.int64)
        if remove_zero_charge_molecules:
            keep = data["charges"].sum(-1) > 0
            data = {k: v[keep] for k, v in data.items()}
        if included_species is None:
            included_species = torch.unique(data["charges"], sorted=True)
            if len(included_species) and included_species[0] == 0:
                included_species = included_species[1:]
        included_species = torch.as_tensor(included_species).reshape(-1).to(torch.int32)
        if subtract_thermo:
            for key in [k.split("_")[0] for k in data if k.endswith("_thermo")]:
                data[key] = data[key] - data[key + "_thermo"].to(data[key].dtype)
        self.stats = {k: (v.mean(), v.std()) for k, v in data.items() if v.dim() == 1 and v.is_floating_point()}          # calc_stats
        if filter_n_atoms is not None:
            keep = data["num_atoms"] == int(filter_n_atoms)
            data = {k: v[keep] for k, v in data.items()}
        charges = data["charges"].to(torch.int64)
        present = charges > 0
        n = present.sum(-1)
        if bool((present != (torch.arange(charges.shape[1]).unsqueeze(0) < n.unsqueeze(1))).any()):
            raise ValueError("a molecule has a zero charge in front of a non-zero one: the reference keeps such a row in place, this layout compacts "
                             "the present atoms to the front of the molecule")
        if bool((n != data["num_atoms"].to(torch.int64)).any()):
            raise ValueError("num_atoms differs from the number of non-zero charges of a molecule")
        props = {k: v for k, v in data.items() if k not in _NOT_PROPERTIES and v.dim() == 1 and v.shape[0] == charges.shape[0]}
        self._init_ragged(n, charges[present].to(torch.int32), data["positions"][present].to(torch.float32), props, data["index"].to(torch.int64),
                          included_species, device, num_pts, conditioning, max_atoms=int(charges.shape[1]))

    def _init_ragged(self, n, z, pos, props, index, included_species, device, num_pts, conditioning, max_atoms):
        self.device = torch.device(device)          # "cpu" prepares, filters and takes statistics only: batches and histograms need the GPU
        M = int(n.shape[0])
        if len(props) > _native.DATA_MAX_PROPS or len(included_species) > _native.DATA_MAX_TYPES:
            raise ValueError(f"at most {_native.DATA_MAX_PROPS} properties and {_native.DATA_MAX_TYPES} species")
        self.M, self.max_atoms = M, int(max_atoms)
        self.sorted_by_size, self.split_indices = False, None          # geom_splits sets them
        self.num_pts =M if num_pts is None or num_pts < 0 else min(int(num_pts), M)
        self.included_species = included_species
        self.num_species, self.max_charge = len(included_species), (int(included_species.max()) if len(included_species) else 0)
        self.parameters = {"num_species": self.num_species, "max_charge": self.max_charge}
        self.property_keys = list(props)
        self.conditioning = list(conditioning)
        for key in self.conditioning:
            if key not in props:
                raise KeyError(f"conditioning on {key!r}: the data has no such property (it has {self.property_keys})")
        self.data = dict(props)                                        # the host copies, in the data's own dtype (statistics are taken on these)
        self.data["num_atoms"] = n.clone()
        self.num_atoms_host = n.numpy().astype(np.int64)                # the host mirror of the sizes
        atom_ptr = torch.zeros(M + 1, dtype=torch.int64)
        atom_ptr[1:] = torch.cumsum(n, 0)
        self.A = int(atom_ptr[-1])
        norms = self.mean_mad(self.property_keys)
        dev = self.device
        self.atom_ptr, self.z, self.pos, self.index = atom_ptr.to(dev), z.contiguous().to(dev), pos.contiguous().to(dev), index.contiguous().to(dev)
        P = len(props)
        self.props = (torch.stack([v.to(torch.float32) for v in props.values()]) if P else torch.zeros(0, M)).contiguous().to(dev)
        self.norm = (torch.tensor([[float(norms[k]["mean"].to(torch.float32)), float(norms[k]["mad"].to(torch.float32))] for k in props],
                                  dtype=torch.float32).reshape(P, 2)).to(dev)
        self.species = included_species.contiguous().to(dev)
        self.ctx_cols = torch.tensor([self.property_keys.index(k) for k in self.conditioning], dtype=torch.int32).to(dev)
        self.flags = torch.zeros(1, dtype=torch.int32, device=dev)
        self._z_host = z
        self._set = _native.DataSet(self.atom_ptr.data_ptr(), self.z.data_ptr(), self.pos.data_ptr(), self.props.data_ptr(), self.species.data_ptr(),
                                    self.norm.data_ptr(), self.index.data_ptr(), M, self.A, P, self.num_species)

    @classmethod
    def from_npz(cls, path: str, device, **kw) -> "MoleculeDataset":
        """The reference's ``train.npz`` / ``valid.npz`` / ``test.npz`` (edm/utils.py:175-180)."""
        with np.load(path) as f:
            return cls({k: torch.from_numpy(np.asarray(f[k])) for k in f.files}, device, **kw)

    @classmethod
    def from_conformers(cls, conformers: Iterable[Any], device, properties: Optional[Dict[str, Any]] = None, included_species=None,
                        num_pts: int = -1, conditioning: Sequence[str] = ()) -> "MoleculeDataset":
        """GEOM's layout: one ``[n, 4]`` array (atomic number, x, y, z) per conformer, never padded on the host."""
        confs = [torch.as_tensor(np.asarray(c), dtype=torch.float32).reshape(-1, 4) for c in conformers]
        n = torch.tensor([c.shape[0] for c in confs], dtype=torch.int64)
        flat = torch.cat(confs) if confs else torch.zeros(0, 4)
        z = flat[:, 0].to(torch.int32)
        if bool((z <= 0).any()) or bool((n == 0).any()):
            raise ValueError("a conformer holds an atom with atomic number <= 0, or no atom at all")
        if included_species is None:
            included_species = torch.unique(z, sorted=True)
        props = {k: _cpu(v) for k, v in (properties or {}).items()}
        self = cls.__new__(cls)
        self.stats = {k: (v.mean(), v.std()) for k, v in props.items() if v.is_floating_point()}
        self._init_ragged(n, z, flat[:, 1:4].contiguous(), props, torch.arange(len(confs), dtype=torch.int64),
                          torch.as_tensor(included_species).reshape(-1).to(torch.int32), device, num_pts, conditioning,
                          max_atoms=int(n.max()) if len(confs) else 0)
        return self

    @classmethod
    def geom_splits(cls, file_or_array, device, permutation=None, val_proportion: float = 0.1, test_proportion: float = 0.1,
                    filter_size: Optional[int] = None, remove_h: bool = False, included_species=None,
                    chunk_rows: int = 1 << 22) -> Dict[str, "MoleculeDataset"]:
        """``{"train", "valid", "test"}`` from the reference's conformer file: a path to ``GEOM_drugs_30.npy`` (memory-mapped, never read whole)
        or the float64 array ``[A, 5]`` itself (molecule id, atomic number, x, y, z).  ``permutation=None`` reads ``GEOM_permutation.npy`` next
        to the file, as ``load_split_data`` does.  The rows go up ``chunk_rows`` at a time through one pinned buffer and are segmented in HBM,
        without hydrogens if ``remove_h`` (what ``extract_conformers --remove_h`` leaves); (M, A) and then the M sizes come back, the orders are
        ``geom_split_orders`` of them, and each split is one ragged gather.  A split is sorted by size (``sorted_by_size``, ``split_indices``),
        its ``index`` is the position in it, and ``included_species`` defaults to GEOM's atomic numbers (without 1 under ``remove_h``)."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("MoleculeDataset.geom_splits segments the conformer file on an MI355X: device must be a HIP ('cuda') device; there is "
                               "no CPU fallback")
        if isinstance(file_or_array, (str, os.PathLike)):
            path = os.fspath(file_or_array)
            rows = np.load(path, mmap_mode="r")
            if permutation is None:
                permutation = np.load(os.path.join(os.path.dirname(os.path.abspath(path)), "GEOM_permutation.npy"))
        else:
            rows = file_or_array if isinstance(file_or_array, np.ndarray) else np.asarray(file_or_array)
            if permutation is None:
                raise ValueError("an array has no GEOM_permutation.npy next to it: pass permutation")
        if rows.ndim != 2 or rows.shape[1] != 5 or rows.dtype != np.float64:
            raise ValueError(f"the conformer array must be float64 [A, 5] (molecule id, atomic number, x, y, z), got {rows.dtype} {rows.shape}")
        R = int(rows.shape[0])
        chunk_rows = max(1, min(int(chunk_rows), max(R, 1), _native.GEOM_MAX_ROWS))
        if included_species is None:
            included_species = [s for s in GEOM_ATOMIC_NUMBERS if not (remove_h and s == 1)]
        included_species = torch.as_tensor(included_species).reshape(-1).to(torch.int32)
        lib, stream = _lib(), _stream(dev)
        # ingestion: every row could be a molecule of its own, so the capacities are the row count
        z_all, pos_all = torch.empty(R, dtype=torch.int32, device=dev), torch.empty((R, 3), dtype=torch.float32, device=dev)
        ptr_all = torch.empty(R + 1, dtype=torch.int64, device=dev)
        state, MA = torch.zeros(_native.GEOM_STATE_WORDS, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(int(lib.gcdm_geom_workspace_bytes(_native.GEOM_WS_BYTES, chunk_rows)), dtype=torch.uint8, device=dev)
        staging = torch.empty((chunk_rows, 5), dtype=torch.float64).pin_memory()
        chunk = torch.empty((chunk_rows, 5), dtype=torch.float64, device=dev)
        staged = torch.cuda.Event()
        for r0 in range(0, R, chunk_rows):
            r = min(chunk_rows, R - r0)
            np.copyto(staging.numpy()[:r], rows[r0:r0 + r])
            chunk[:r].copy_(staging[:r], non_blocking=True)
            staged.record(torch.cuda.current_stream(dev))
            _chk(lib.gcdm_geom_ingest(_ptr(chunk), r, int(bool(remove_h)), _ptr(state), _ptr(z_all), _ptr(pos_all), _ptr(ptr_all), R, R, _ptr(ws),
                                      _ptr(flags), stream), "gcdm_geom_ingest")
            staged.synchronize()                   # the pinned buffer is free for the next chunk; the kernels run on
        _chk(lib.gcdm_geom_finish(_ptr(state), _ptr(ptr_all), R, _ptr(MA), _ptr(flags), stream), "gcdm_geom_finish")
        M, A = (int(v) for v in MA.cpu())
        sizes = (ptr_all[1:M + 1] - ptr_all[:M]).cpu().numpy()          # the host mirror of the sizes: with (M, A) the read-back of the ingestion
        del staging, chunk, ws
        orders = geom_split_orders(sizes, permutation, val_proportion, test_proportion, filter_size)
        out = {}
        for name in GEOM_SPLITS:
            order, split_indices = orders[name]
            n = torch.from_numpy(sizes[order])
            ptr_out = torch.zeros(len(order) + 1, dtype=torch.int64)
            ptr_out[1:] = torch.cumsum(n, 0)
            A_out = int(ptr_out[-1])
            z, pos = torch.empty(A_out, dtype=torch.int32, device=dev), torch.empty((A_out, 3), dtype=torch.float32, device=dev)
            order_dev, ptr_dev = torch.from_numpy(order).to(dev), ptr_out.to(dev)
            _chk(lib.gcdm_geom_gather(_ptr(ptr_all), _ptr(z_all), _ptr(pos_all), M, A, _ptr(order_dev), _ptr(ptr_dev), len(order), A_out, _ptr(z),
                                      _ptr(pos), _ptr(flags), stream), "gcdm_geom_gather")
            self = cls.__new__(cls)
            self.stats = {}
            self._init_ragged(n, z, pos, {}, torch.arange(len(order), dtype=torch.int64), included_species, dev, -1, (),
                              max_atoms=int(n.max()) if len(order) else 0)
            self.sorted_by_size, self.split_indices = True, split_indices
            out[name] = self
        f = int(flags.item())                      # also waits for the gathers before the raw buffers go
        del z_all, pos_all, ptr_all
        if f & _native.GEOM_FLAG_BAD_ROW:
            raise ValueError("the conformer file holds a row with an atomic number < 1 or a value that is not finite")
        if f:
            raise RuntimeError(f"the GEOM ingestion raised device flags {f}: the sizes on the device did not add up")
        return out

    @classmethod
    def from_geom_file(cls, file_or_array, device, split: str = "train", **kw) -> "MoleculeDataset":
        """One split of ``geom_splits`` (same arguments)."""
        if split not in GEOM_SPLITS:
            raise ValueError(f"split must be one of {GEOM_SPLITS}, got {split!r}")
        return cls.geom_splits(file_or_array, device, **kw)[split]

    def __len__(self) -> int:
        return self.num_pts

    def mean_mad(self, properties: Sequence[str]) -> Dict[str, Dict[str, torch.Tensor]]:
        """compute_mean_mad_from_dataloader (src/models/__init__.py:63-76) on the data set's own values."""
        out = {}
        for key in properties:
            v = self.data[key]
            v = v if v.is_floating_point() else v.to(torch.float32)
            mean = torch.mean(v)
            out[key] = {"mean": mean, "mad": torch.mean(torch.abs(v - mean))}
        return out

    def n_nodes_histogram(self) -> Dict[int, int]:
        """{size: molecules} in ascending size: what NumNodesDistribution takes."""
        sizes, counts = np.unique(self.num_atoms_host, return_counts=True)
        return {int(s): int(c) for s, c in zip(sizes, counts)}

    def atom_type_histogram(self) -> Dict[int, int]:
        """{one-hot column: atoms}, the ``atom_types`` entry of a dataset_info."""
        zs = self._z_host.to(torch.int64)
        return {t: int((zs == int(s)).sum()) for t, s in enumerate(self.included_species)}

    @torch.inference_mode()
    def graph_keys(self, dataset_info: Dict[str, Any], valence_caps: Optional[Dict[str, int]] = None) -> torch.Tensor:
        """The sorted distinct graph keys (metrics.molecule_graph_keys) of the split's molecules that are valid AND in one fragment: what
        novelty is taken against.  compute_qm9_smiles (rdkit_functions.py:32-76) keeps the whole-molecule SMILES of the sanitisable molecules,
        and a dotted SMILES can never equal a largest-fragment one.  One launch over ``pos`` / ``z`` / ``atom_ptr``, the atomic numbers mapped
        through the vocabulary of ``dataset_info`` on the device."""
        from . import metrics
        if self.device.type != "cuda":
            raise RuntimeError("MoleculeDataset.graph_keys runs on the GPU only (no CPU fallback)")
        tb = metrics.graph_tables(dataset_info, valence_caps, types_are_atomic_numbers=True)
        keys, info = metrics._launch(tb, self.pos, self.z, self.atom_ptr, self.M)
        keep = (info[:, 0] == 1) & (info[:, 1] == 1)
        return torch.unique(keys[keep])

    def loader(self, batch_size: int, shuffle: bool = True, drop_last: bool = False, seed: int = 0, layout: str = "padded", rank: int = 0,
               world: int = 1, sequential: bool = False) -> "DeviceLoader":
        return DeviceLoader(self, batch_size, shuffle, drop_last, seed, layout, rank, world, sequential)

    def collate(self, perm: torch.Tensor, first: int, B: int, pad_to: int, sizes: np.ndarray) -> AttrDict:
        """One batch of molecules ``perm[first : first + B]`` (``perm`` int64 on the device, ``sizes`` their atom counts from the host mirror):
        two launches on the current stream, no device-to-host copy."""
        ops._dev(self.atom_ptr)
        N, E, all_present = batch_accounting(sizes, pad_to)
        dev, P, T, Cn = self.device, len(self.property_keys), self.num_species, len(self.conditioning)
        f32 = dict(dtype=torch.float32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        x, one_hot, charges = torch.empty((N, 3), **f32), torch.empty((N, T), **f32), torch.empty((N, 1), **f32)
        bi, mask = torch.empty(N, **i64), torch.empty(N, dtype=torch.bool, device=dev)
        index, present, props = torch.empty(B, **i64), torch.empty(B, **i64), torch.empty((P, B), **f32)
        ctx = torch.empty((N, Cn), **f32) if Cn else None
        edge_index, colperm = torch.empty((2, E), **i64), torch.empty(E, **i64)
        rowptr, colptr = torch.empty(N + 1, dtype=torch.int32, device=dev), torch.empty(N + 1, dtype=torch.int32, device=dev)
        ws = torch.empty(int(_lib().gcdm_data_workspace_bytes(B)), dtype=torch.uint8, device=dev)
        out = _native.DataBatch(*[None if t is None else t.data_ptr() for t in (x, one_hot, charges, bi, mask, index, present, props, ctx, edge_index,
                                                                                rowptr, colperm, colptr)])
        _chk(_lib().gcdm_data_collate(C.byref(self._set), _ptr(perm), int(perm.shape[0]), int(first), int(B), int(pad_to), _ptr(self.ctx_cols), Cn,
                                      N, E, _ptr(ws), C.byref(out), _ptr(self.flags), _stream(dev)), "gcdm_data_collate")
        # charges leaves as [N], the shape of the reference's batches (its items' [A_max] rows concatenated), which normalize() multiplies by the mask
        batch = AttrDict(x=x, one_hot=one_hot, charges=charges.reshape(N), batch=bi, mask=mask, index=index, num_graphs=int(B), num_nodes_present=present,
                         all_present=all_present)
        for p, key in enumerate(self.property_keys):
            batch[key] = props[p]
        if Cn:
            batch["props_context"] = ctx
        batch["fc_graph"] = ops.Graph.from_parts(edge_index, N, rowptr, colperm, colptr)
        return batch

    def check(self) -> None:
        """Reads the device flag word (one device-to-host copy; not part of iterating): raises if a collation's sizes did not add up."""
        f = int(self.flags.item())
        if f & _native.DATA_FLAG_ACCOUNT:
            raise RuntimeError("a batch's sizes on the device did not add up to the host mirror's N and E (or an index was out of range): the batch "
                               "is not to be used")


class DeviceLoader:
    """Iterates a MoleculeDataset in batches; ``set_epoch(e)`` as on a DistributedSampler.  The index stream is
    ``distributed_indices(len(dataset), shuffle, seed, epoch, rank, world)``, uploaded once per epoch; ``drop_last`` drops a short last batch.
    ``layout="padded"``: every molecule takes ``dataset.max_atoms`` rows (the reference's batches); ``"compact"``: present atoms only.
    ``sequential=True`` (GEOM's ``dataloader_cfg.sequential``): the batches of ``sequential_batches`` over a size-sorted data set, every batch of
    one molecule size, so both layouts hold present atoms only and ``all_present`` is true; it needs ``shuffle=False`` and ``world == 1``."""

    def __init__(self, dataset: MoleculeDataset, batch_size: int, shuffle: bool = True, drop_last: bool = False, seed: int = 0, layout: str = "padded",
                 rank: int = 0, world: int = 1, sequential: bool = False):
        if layout not in ("padded", "compact"):
            raise ValueError(f"layout must be 'padded' or 'compact', got {layout!r}")
        if int(batch_size) < 1:
            raise ValueError(f"batch_size = {batch_size}")
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), bool(shuffle), bool(drop_last)
        self.seed, self.layout, self.rank, self.world = int(seed), layout, int(rank), int(world)
        self.pad_to = dataset.max_atoms if layout == "padded" else 0
        self.epoch, self._perm_epoch = 0, None
        self.sequential = bool(sequential)
        if self.sequential:
            if self.shuffle:
                raise ValueError("sequential batches need shuffle=False: they walk the size-sorted data set in order")
            if self.world != 1:
                raise ValueError(f"sequential batches need world == 1, got world = {self.world}: they are not built under data-parallel ranks")
            if not getattr(dataset, "sorted_by_size", False):
                raise ValueError("sequential batches need a size-sorted data set (MoleculeDataset.geom_splits / from_geom_file): this one is not")
            self._firsts, self._counts = sequential_batches(len(dataset), self.batch_size, self.drop_last, dataset.split_indices)
        self.indices = distributed_indices(len(dataset), self.shuffle, self.seed, 0, self.rank, self.world)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def __len__(self) -> int:
        if self.sequential:
            return len(self._counts)
        n = len(self.indices)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _upload(self) -> None:
        if self._perm_epoch != self.epoch:
            self.indices = distributed_indices(len(self.dataset), self.shuffle, self.seed, self.epoch, self.rank, self.world)
            self._sizes = self.dataset.num_atoms_host[self.indices.numpy()]
            self._perm = self.indices.to(self.dataset.device)
            self._perm_epoch = self.epoch

    def __iter__(self):
        self._upload()
        self._cursor = 0
        return self

    def __next__(self) -> AttrDict:
        if self.sequential:
            k = self._cursor
            if k >= len(self._counts):
                raise StopIteration
            self._cursor = k + 1
            first, B = int(self._firsts[k]), int(self._counts[k])
            sizes = self._sizes[first:first + B]
            return self.dataset.collate(self._perm, first, B, int(sizes[0]) if self.layout == "padded" else 0, sizes)
        first, n = self._cursor, len(self.indices)
        B = min(self.batch_size, n - first)
        if B <= 0 or (self.drop_last and B < self.batch_size):
            raise StopIteration
        self._cursor = first + B
        return self.dataset.collate(self._perm, first, B, self.pad_to, self._sizes[first:first + B])


class PropertiesDistribution:
    """The reference's PropertiesDistribution (src/models/__init__.py:311-415) on the device: per property and molecule size the integer
    histogram of ``num_bins`` bins over [min, max], built by one launch per property; ``sample_batch`` draws a normalised context ``[B, P]`` by
    one launch, from ``torch.rand`` on the device (seedable through ``generator``).  ``distributions[prop][n]`` holds ``params`` (min, max)
    and ``counts``.  A size without members makes ``sample_batch`` raise KeyError: at once for host sizes, at the next ``check()`` or call for
    sizes given on the device (their rows are NaN)."""

    def __init__(self, dataset: MoleculeDataset, properties: Sequence[str], num_bins: int = 1000, normalizer: Optional[Dict[str, Dict[str, Any]]] = None):
        self.dataset, self.properties, self.num_bins, self.device = dataset, list(properties), int(num_bins), dataset.device
        if not 1 <= self.num_bins <= _native.DATA_MAX_BINS:
            raise ValueError(f"num_bins must be 1 .. {_native.DATA_MAX_BINS}")
        ops._dev(dataset.atom_ptr)
        S =int(dataset.num_atoms_host.max()) + 1 if dataset.M else 0
        if S > _native.DATA_MAX_SIZES:
            raise ValueError(f"molecules of up to {_native.DATA_MAX_SIZES - 1} atoms")
        Pn, dev = len(self.properties), self.device
        self.num_sizes = S
        self.counts = torch.empty((Pn, S, self.num_bins), dtype=torch.int32, device=dev)
        self.params = torch.empty((Pn, S, 2), dtype=torch.float32, device=dev)
        self.members = torch.empty((Pn, S), dtype=torch.int32, device=dev)
        self.flags = torch.zeros(1, dtype=torch.int32, device=dev)
        for p, key in enumerate(self.properties):
            row = dataset.props[dataset.property_keys.index(key)]
            _chk(_lib().gcdm_data_prop_histogram(_ptr(dataset.atom_ptr), _ptr(row), dataset.M, S, self.num_bins, _ptr(self.counts[p]),
                                                 _ptr(self.params[p]), _ptr(self.members[p]), _ptr(self.flags), _stream(dev)),
                 "gcdm_data_prop_histogram")
        params, members, counts = self.params.cpu(), self.members.cpu(), self.counts.cpu()          # once, at construction
        if int(self.flags.item()) & _native.DATA_FLAG_ACCOUNT:
            raise RuntimeError("gcdm_data_prop_histogram: a molecule's size is outside the tables")
        self._members_host = members.numpy()
        self.distributions = {key: {n: {"params": (params[p, n, 0], params[p, n, 1]), "counts": counts[p, n]}
                                    for n in range(S) if int(members[p, n]) > 0} for p, key in enumerate(self.properties)}
        self._flags_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._event = None
        self.normalizer = None
        if normalizer is not None:
            self.set_normalizer(normalizer)

    def set_normalizer(self, normalizer: Dict[str, Dict[str, Any]]) -> None:
        self.normalizer = normalizer
        self._norm = torch.tensor([[float(torch.as_tensor(normalizer[k]["mean"]).to(torch.float32)),
                                    float(torch.as_tensor(normalizer[k]["mad"]).to(torch.float32))] for k in self.properties],
                                  dtype=torch.float32).reshape(len(self.properties), 2).to(self.device)

    def check(self, wait: bool = True) -> None:
        """Raises KeyError if an earlier ``sample_batch`` met a size without members.  ``wait=False`` looks only if the copy has arrived."""
        if self._event is None or (not wait and not self._event.query()):
            return
        self._event.synchronize()
        self._event = None
        if int(self._flags_host[0]) & _native.DATA_FLAG_ABSENT_SIZE:
            self._flags_host.zero_()
            self.flags.zero_()
            raise KeyError("PropertiesDistribution.sample_batch: a requested molecule size has no member in the data set")

    def sample_batch(self, num_nodes: torch.Tensor, generator: Optional[torch.Generator] = None, u: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Normalised context ``[B, P]`` on the device.  ``u`` ``[B, P, 2]`` replaces the uniforms (tests)."""
        if self.normalizer is None:
            raise AssertionError("To normalize properties, `normalizer` must not be null.")
        self.check(wait=False)
        num_nodes = torch.as_tensor(num_nodes)
        B, Pn, dev = int(num_nodes.numel()), len(self.properties), self.device
        if num_nodes.device.type == "cpu":
            nn_host = num_nodes.reshape(-1).to(torch.int64).numpy()
            for n in nn_host:
                if not (0 <= n < self.num_sizes) or (Pn and self._members_host[0, n] <= 0):
                    raise KeyError(int(n))
        nn_dev = num_nodes.reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
        if u is None:
            u = torch.rand((B, Pn, 2), dtype=torch.float32, device=dev, generator=generator)
        u = u.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(u.shape) != (B, Pn, 2):
            raise ValueError(f"u {tuple(u.shape)} must be [{B}, {Pn}, 2]")
        out = torch.empty((B, Pn), dtype=torch.float32, device=dev)
        _chk(_lib().gcdm_data_prop_sample(_ptr(self.counts), _ptr(self.params), _ptr(self.members), _ptr(self._norm), _ptr(nn_dev), _ptr(u), B, Pn,
                                          self.num_sizes, self.num_bins, _ptr(out), _ptr(self.flags), _stream(dev)), "gcdm_data_prop_sample")
        if num_nodes.device.type != "cpu":                      # the host could not look: the flag word follows without blocking
            self._flags_host.copy_(self.flags, non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record(torch.cuda.current_stream(dev))
        return out

    def sample(self, num_nodes: int = 19) -> torch.Tensor:
        return self.sample_batch(torch.tensor([int(num_nodes)]))[0]
