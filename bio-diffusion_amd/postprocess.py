"""The graph filters of the reference's post-processing of generated molecules, on the device and without RDKit.

Stand-in for ``process_molecule`` (src/datamodules/components/edm/rdkit_functions.py:323-379) as ``generate_molecules`` applies it to every
sample (qm9_mol_gen_ddpm.py:1201-1209, 1233-1241): ``sanitize`` drops a molecule that fails the valence-cap verdict of ``metrics.py``,
``largest_frag`` keeps the atoms of its largest connected component.  ``gcdm_molproc_select`` / ``gcdm_molproc_emit``
(include/gcdm_molproc.h, where the semantics are written down) do both for a whole flat batch: the survivors come back as a new flat batch on
the device with their bond lists, and the host objects are built from one copy per tensor.  No arithmetic happens here: this module builds the
tables, calls the C ABI and slices; CPU tensors are rejected.  ``add_hydrogens`` and ``relax_iter`` (AddHs, UFF) are not built.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import torch

from . import _native
from .metrics import _offsets64, graph_tables
from .sdf import Molecule


@dataclass
class ProcessedBatch:
    """The surviving molecules as a flat batch; every tensor lives on the device.  M, N: molecules and atoms given; M', N', nb': molecules,
    atoms and bonds that survive."""
    positions: torch.Tensor                 # [N', 3] fp32, bit copies
    atom_types: torch.Tensor                # [N'] in the dtype given
    charges: Optional[torch.Tensor]         # [N'] (or [N', 1], as given); None when none were given
    num_nodes: torch.Tensor                 # [M'] int64
    mol_offsets: torch.Tensor               # [M' + 1] int64
    bonds: torch.Tensor                     # [nb', 3] int32 (i, j, order), i > j within the molecule, nonzero(tril(E, -1)) order
    bond_offsets: torch.Tensor              # [M' + 1] int64
    src_atom: torch.Tensor                  # [N'] int64 index into the atoms given
    src_molecule: torch.Tensor              # [M'] int64 index into the molecules given
    info: torch.Tensor                      # [M, 4] int32 (valid, n_fragments, n_largest, n) of the molecules given
    keep: torch.Tensor                      # [N] bool over the atoms given
    dataset_info: Dict[str, Any]

    def __len__(self) -> int:
        return int(self.num_nodes.shape[0])

    def _host(self):
        """One copy per tensor."""
        off = self.mol_offsets.cpu().tolist()
        return off, self.positions.cpu(), self.atom_types.cpu(), None if self.charges is None else self.charges.cpu()

    def tuples(self) -> List[Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]]:
        """The ``(pos, at, ch)`` list ``generate_molecules`` returns: CPU tensors per molecule, ``ch`` None without charges."""
        off, pos, at, ch = self._host()
        return [(pos[a:b], at[a:b], None if ch is None else ch[a:b]) for a, b in zip(off[:-1], off[1:])]

    def molecules(self) -> List[Molecule]:
        """What ``sdf.build_molecules`` gives the whole molecules, reduced to the survivors."""
        off, pos, at, ch = self._host()
        boff, bonds = self.bond_offsets.cpu().tolist(), self.bonds.cpu().tolist()
        dec = self.dataset_info["atom_decoder"]
        pos, at = pos.numpy(), at.tolist()
        chg = None if ch is None or ch.numel() == 0 else ch.reshape(-1).round().to(torch.int64).numpy()
        out = []
        for k, (a, b) in enumerate(zip(off[:-1], off[1:])):
            out.append(Molecule(symbols=[dec[t] for t in at[a:b]], positions=pos[a:b].copy(),
                                bonds=[(i, j, o) for i, j, o in bonds[boff[k]:boff[k + 1]]], charges=None if chg is None else chg[a:b].copy()))
        return out


def _some(t: torch.Tensor) -> torch.Tensor:
    """A tensor whose pointer the ABI accepts: an empty one has none."""
    return t if t.numel() else torch.zeros(1, dtype=t.dtype, device=t.device)


@torch.inference_mode()
def process_molecules(positions: torch.Tensor, atom_types: torch.Tensor, num_nodes: torch.Tensor, dataset_info: Dict[str, Any],
                      charges: Optional[torch.Tensor] = None, sanitize: bool = False, largest_frag: bool = False,
                      valence_caps: Optional[Dict[str, int]] = None, orders: Optional[torch.Tensor] = None,
                      limit_bonds_to_one: Optional[bool] = None) -> ProcessedBatch:
    """`positions` [N, >=3] fp32 (row stride arbitrary: a view of the sampler output `xh` is fine), `atom_types` [N] vocabulary indices,
    `num_nodes` [M] atoms per molecule (flat batch order), `charges` [N] or [N, 1] fp32 / int32.  `valence_caps`, `orders` and
    `limit_bonds_to_one` as for `metrics.molecule_graph_keys`.  Two calls into the library; between them three integers reach the host (the
    sizes of the outputs), the only synchronisation.  A molecule of more than 192 atoms is a ValueError."""
    if not positions.is_cuda:
        raise RuntimeError("process_molecules runs on the GPU only (no CPU fallback)")
    if positions.dtype != torch.float32 or positions.dim() != 2 or positions.shape[1] < 3 or positions.stride(1) != 1:
        raise ValueError("positions must be fp32 [N, >=3] with unit column stride")
    dev, N = positions.device, positions.shape[0]
    sizes = torch.as_tensor(num_nodes).to(torch.int64).cpu().reshape(-1)
    M = len(sizes)
    if int(sizes.sum()) != N or atom_types.shape[0] != N or (M and int(sizes.min()) < 0):
        raise ValueError("num_nodes / atom_types do not match positions")
    if M and int(sizes.max()) > _native.MOLGRAPH_MAX_ATOMS:
        raise ValueError(f"a molecule of {int(sizes.max())} atoms: at most {_native.MOLGRAPH_MAX_ATOMS} are handled")
    ch = None
    if charges is not None and charges.numel() == 0 and N > 0:
        charges = None                                               # the sampler's placeholder for "no charges"
    if charges is not None:
        if charges.dtype not in (torch.float32, torch.int32) or charges.numel() != N:
            raise ValueError("charges must be fp32 or int32 with one element per atom")
        ch = charges.to(dev).reshape(-1).contiguous()
    lib = _native.load_ops()
    tb = graph_tables(dataset_info, valence_caps, limit_bonds_to_one)
    off = _offsets64(sizes, dev)
    types = atom_types.to(device=dev, dtype=torch.int32).contiguous()
    poff = None
    if orders is not None:
        if not orders.is_cuda or orders.dtype != torch.uint8 or not orders.is_contiguous() or orders.numel() != int((sizes * sizes).sum()):
            raise ValueError("orders must be a contiguous uint8 device tensor of sum(n^2) elements (the layout of gcdm_bond_orders)")
        poff = torch.zeros(M + 1, dtype=torch.int64)
        poff[1:] = torch.cumsum(sizes * sizes, 0)
        poff = poff.to(dev)
    flags = (_native.MOLPROC_SANITIZE if sanitize else 0) | (_native.MOLPROC_LARGEST_FRAG if largest_frag else 0)
    stride = positions.stride(0) if N > 1 else max(positions.shape[1], 3)
    e = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    info, counts, totals = e((M, 4), torch.int32), e((max(M, 1), 3), torch.int32), e(3, torch.int64)
    keep, new_index = e(max(N, 1), torch.uint8), e(max(N, 1), torch.int32)
    ws = e(max(lib.gcdm_molproc_workspace_bytes(M) // 8, 1), torch.int64)
    p = lambda t: None if t is None else C.c_void_p(_some(t).data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        st = lib.gcdm_molproc_select(tb, p(positions), stride, p(types), p(off), M, p(poff), None if orders is None else p(orders), flags, p(info),
                                     p(keep), p(new_index), p(counts), p(totals), p(ws), stream)
        if st != 0:
            raise _native.NativeError(f"gcdm_molproc_select failed with status {st} (libgcdm_ops.so)")
        Np, nbp, Mp = totals.tolist()                                # the sizes of the outputs: three integers, one copy
        pos_out, types_out = e((max(Np, 1), 3), torch.float32), e(max(Np, 1), torch.int32)
        ch_out = None if ch is None else e(max(Np, 1), ch.dtype)
        src_atom, src_mol = e(max(Np, 1), torch.int64), e(max(Mp, 1), torch.int64)
        mol_off, bond_off, bonds = e(Mp + 1, torch.int64), e(Mp + 1, torch.int64), e((max(nbp, 1), 3), torch.int32)
        st = lib.gcdm_molproc_emit(tb, p(positions), stride, p(types), p(ch), p(off), M, p(poff), None if orders is None else p(orders), p(keep),
                                   p(new_index), p(counts), p(totals), p(ws), p(pos_out), p(types_out), p(ch_out), p(src_atom), p(src_mol),
                                   p(mol_off), p(bonds), p(bond_off), stream)
        if st != 0:
            raise _native.NativeError(f"gcdm_molproc_emit failed with status {st} (libgcdm_ops.so)")
    if ch_out is not None:
        ch_out = ch_out[:Np].reshape((Np,) + tuple(charges.shape[1:])) if charges.dim() > 1 else ch_out[:Np]
    return ProcessedBatch(positions=pos_out[:Np], atom_types=types_out[:Np].to(atom_types.dtype), charges=ch_out, num_nodes=mol_off[1:] - mol_off[:-1],
                          mol_offsets=mol_off, bonds=bonds[:nbp], bond_offsets=bond_off, src_atom=src_atom[:Np], src_molecule=src_mol[:Mp], info=info,
                          keep=keep[:N].to(torch.bool), dataset_info=dataset_info)
