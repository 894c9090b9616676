"""Validity, uniqueness and novelty of generated molecules on the device, without RDKit.

Stand-in for the reference's BasicMolecularMetrics (src/datamodules/components/edm/rdkit_functions.py:121-197).  Its molecules are built from
the EDM distance rule (make_mol_edm, :276-320): elements and explicit bond orders, no charges, no aromatic flags.  For such a molecule
  * validity (SanitizeMol) is the question whether an atom carries more bond order than its element may,
  * the largest fragment is the largest connected component,
  * equality of canonical SMILES is isomorphism of two labelled graphs,
and `gcdm_molgraph_keys` (include/gcdm_molgraph.h) answers all three per molecule in one launch: a valence-cap verdict, the fragments, and a
permutation-invariant 64-bit key of the largest fragment.  Uniqueness and novelty are then set operations on int64 tensors.  No arithmetic
happens here: this module builds the constant tables, calls the C ABI and does the bookkeeping; CPU tensors are rejected.

Differences from RDKit: validity is the valence-cap rule and is not pinned to RDKit; two molecules that differ only in where
a ring's alternating double bonds fall are one SMILES after aromatisation and two keys here; a key is a 64-bit hash, not a canonical form.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

from . import _native
from .stability import bond_tables

ATOMIC_NUMBERS = {"H": 1, "B": 5, "C": 6, "N": 7, "O": 8, "F": 9, "Al": 13, "Si": 14, "P": 15, "S": 16, "Cl": 17, "As": 33, "Br": 35, "I": 53,
                  "Hg": 80, "Bi": 83}


def _limit_bonds_to_one(dataset_info: Dict[str, Any]) -> bool:
    """make_mol_edm (rdkit_functions.py:286)."""
    return "GEOM" in str(dataset_info.get("name", ""))


def graph_tables(dataset_info: Dict[str, Any], valence_caps: Optional[Dict[str, int]] = None, limit_bonds_to_one: Optional[bool] = None,
                 types_are_atomic_numbers: bool = False) -> "_native.GcdmMolGraphTables":
    """The ABI struct: the bond tables of the stability check, the atomic number per vocabulary type and the valence caps.  The default cap
    of an element is the largest valence `allowed_bonds` (edm/constants.py:22-25) gives it: the highest set bit of the `allowed_mask` that
    `stability.bond_tables` builds; `valence_caps={"S": 6}` overrides by symbol (a negative value lifts the cap)."""
    decoder = list(dataset_info["atom_decoder"])
    unknown = [s for s in decoder if s not in ATOMIC_NUMBERS]
    if unknown:
        raise ValueError(f"no atomic number known for {unknown}")
    for s in (valence_caps or {}):
        if s not in decoder:
            raise ValueError(f"valence_caps names {s!r}, which the vocabulary {decoder} does not hold")
    tb = _native.GcdmMolGraphTables()
    tb.bonds = bond_tables(dataset_info, _limit_bonds_to_one(dataset_info) if limit_bonds_to_one is None else bool(limit_bonds_to_one))
    tb.types_are_atomic_numbers = int(bool(types_are_atomic_numbers))
    for a, sym in enumerate(decoder):
        tb.atomic_number[a] = ATOMIC_NUMBERS[sym]
        tb.valence_cap[a] = int(tb.bonds.allowed_mask[a]).bit_length() - 1
        if valence_caps and sym in valence_caps:
            tb.valence_cap[a] = int(valence_caps[sym])
    return tb


def _offsets64(num_nodes: torch.Tensor, device) -> torch.Tensor:
    off = torch.zeros(len(num_nodes) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.as_tensor(num_nodes).to(torch.int64).cpu(), 0)
    return off.to(device)


@torch.inference_mode()
def molecule_graph_keys(positions: torch.Tensor, atom_types: torch.Tensor, num_nodes: torch.Tensor, dataset_info: Dict[str, Any],
                        valence_caps: Optional[Dict[str, int]] = None, orders: Optional[torch.Tensor] = None,
                        limit_bonds_to_one: Optional[bool] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`positions` [N, >=3] fp32 (row stride arbitrary: a view of the sampler output `xh` is fine), `atom_types` [N] vocabulary indices,
    `num_nodes` [M] atoms per molecule (flat batch order).  Returns `(keys int64 [M], info int32 [M, 4])` on the device, info rows
    (valid, n_fragments, n_largest, n); one launch.  `orders`: flat uint8 bond orders in the layout of `gcdm_bond_orders` (one n x n block
    per molecule, end to end) to use in place of the distance rule; positions are then only consulted for the device.  `limit_bonds_to_one`
    defaults to the reference's choice for the data set (GEOM: on).  A molecule of more than 192 atoms gets info (-1, 0, 0, n), key 0."""
    if not positions.is_cuda:
        raise RuntimeError("molecule_graph_keys runs on the GPU only (no CPU fallback)")
    if positions.dtype != torch.float32 or positions.dim() != 2 or positions.shape[1] < 3 or positions.stride(1) != 1:
        raise ValueError("positions must be fp32 [N, >=3] with unit column stride")
    N = positions.shape[0]
    sizes = torch.as_tensor(num_nodes).to(torch.int64).cpu()
    if int(sizes.sum()) != N or atom_types.shape[0] != N or (len(sizes) and int(sizes.min()) < 0):
        raise ValueError("num_nodes / atom_types do not match positions")
    tb = graph_tables(dataset_info, valence_caps, limit_bonds_to_one)
    return _launch(tb, positions, atom_types, _offsets64(sizes, positions.device), len(sizes), orders, sizes)


def _launch(tb, positions, atom_types, off, M, orders=None, sizes=None):
    lib = _native.load_ops()
    dev = positions.device
    types = atom_types.to(device=dev, dtype=torch.int32).contiguous()
    keys = torch.empty(M, dtype=torch.int64, device=dev)
    info = torch.empty((M, 4), dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        if orders is None:
            stride = positions.stride(0) if positions.shape[0] > 1 else max(positions.shape[1], 3)
            st = lib.gcdm_molgraph_keys(tb, p(positions), stride, p(types), p(off), M, p(keys), p(info), stream)
        else:
            if not orders.is_cuda or orders.dtype != torch.uint8 or not orders.is_contiguous() or orders.numel() != int((sizes * sizes).sum()):
                raise ValueError("orders must be a contiguous uint8 device tensor of sum(n^2) elements (the layout of gcdm_bond_orders)")
            poff = torch.zeros(M + 1, dtype=torch.int64)
            poff[1:] = torch.cumsum(sizes * sizes, 0)
            poff = poff.to(dev)
            st = lib.gcdm_molgraph_keys_from_orders(tb, p(types), p(off), M, p(poff), p(orders), p(keys), p(info), stream)
    if st != 0:
        raise _native.NativeError(f"gcdm_molgraph_keys failed with status {st} (libgcdm_ops.so)")
    return keys, info


class GraphMolecularMetrics:
    """BasicMolecularMetrics on graph keys.  `dataset_keys`: int64 keys of the training molecules (`MoleculeDataset.graph_keys`), any
    order, duplicates allowed; None: novelty is 0.0, as in the reference when it has no SMILES list (GEOM)."""

    def __init__(self, dataset_info: Dict[str, Any], dataset_keys: Optional[torch.Tensor] = None, valence_caps: Optional[Dict[str, int]] = None):
        self.dataset_info = dataset_info
        self.valence_caps = dict(valence_caps) if valence_caps else None
        self.dataset_keys = None if dataset_keys is None else torch.unique(torch.as_tensor(dataset_keys).to(torch.int64).reshape(-1))   # sorted
        self.reset()

    def reset(self) -> None:
        self._keys: List[torch.Tensor] = []
        self._valid: List[torch.Tensor] = []

    def update(self, keys: torch.Tensor, info: torch.Tensor) -> None:
        """Appends the `(keys, info)` of `molecule_graph_keys`; nothing leaves the device."""
        if keys.dim() != 1 or info.dim() != 2 or info.shape != (keys.shape[0], 4):
            raise ValueError("update takes keys [M] and info [M, 4]")
        self._keys.append(keys.to(torch.int64))
        self._valid.append(info[:, 0] == 1)

    def compute(self) -> List[float]:
        """[validity, uniqueness, novelty] with the bookkeeping of evaluate_rdmols (rdkit_functions.py:168-185): valid / generated, distinct
        valid keys / valid, distinct valid keys absent from the data set / distinct valid keys; 0.0 and 0.0 when nothing is valid.  Three
        integers reach the host, in one copy."""
        if not self._keys:
            raise ValueError("compute() before any update()")
        keys, valid = torch.cat(self._keys), torch.cat(self._valid)
        generated = keys.shape[0]
        if generated == 0:
            raise ValueError("compute() on zero molecules")
        unique = torch.unique(keys[valid])                                    # sorted
        if self.dataset_keys is not None and self.dataset_keys.numel():
            known = self.dataset_keys.to(unique.device)
            at = torch.searchsorted(known, unique).clamp_(max=known.numel() - 1)
            novel = (known[at] != unique).sum()
        else:
            novel = torch.tensor(unique.numel() if self.dataset_keys is not None else 0, device=unique.device)
        n_valid, n_unique, n_novel = torch.stack([valid.sum(), torch.tensor(unique.numel(), device=valid.device), novel.to(valid.device)]).tolist()
        validity = n_valid / generated
        if n_valid == 0:
            return [validity, 0.0, 0.0]
        return [validity, n_unique / n_valid, (n_novel / n_unique) if self.dataset_keys is not None else 0.0]

    @torch.inference_mode()
    def evaluate(self, generated: Sequence[Tuple[torch.Tensor, ...]]) -> List[float]:
        """The reference's `evaluate` (:188-197): a list of (positions [n, 3], atom_types [n]) pairs, already masked; charges, if there, are
        ignored as make_mol_edm ignores them."""
        if not len(generated):
            raise ValueError("evaluate() on zero molecules")
        x = torch.cat([g[0].reshape(-1, 3).to(torch.float32) for g in generated]).contiguous()
        t = torch.cat([g[1].reshape(-1) for g in generated])
        sizes = torch.tensor([g[1].numel() for g in generated], dtype=torch.int64)
        self.reset()
        self.update(*molecule_graph_keys(x, t, sizes, self.dataset_info, self.valence_caps))
        return self.compute()
