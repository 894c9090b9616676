"""Whole-model plug point: ``_target_`` stand-ins for the reference LightningModules.

Boundary only (plug point 2): the constructor keywords, ``load_from_checkpoint``, ``.to(device)``,
``.dataset_info``, ``.ddpm.num_nodes_distribution.sample(n)``, ``.sample(...)`` and ``.generate_molecules(...)`` that
``src/mol_gen_sample.py:81-182`` and ``src/mol_gen_eval_conditional_qm9.py:101-109`` use of
``src/models/qm9_mol_gen_ddpm.py`` / ``geom_mol_gen_ddpm.py``, plus the evaluation driver ``sample_and_analyze`` (``:747-885``)
with the stability statistics computed on the device.  Training / validation hooks, RDKit metrics and RDKit
post-processing are out of scope; ``generate_molecules`` returns raw (positions, atom-type indices, charges) per
molecule and hands them to an optional ``molecule_builder`` (the reference's ``build_molecule``) when given.
"""
from __future__ import annotations

import logging
import os
import pickle
import re
import warnings
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import nn

from .config import cfg_get, dataset_info as _dataset_info
from .gcpnet import GCPNetDynamics
from .egnn_dynamics import EGNNDynamics
from .stability import CategoricalDistribution, check_molecular_stability_batch
from .metrics import GraphMolecularMetrics, molecule_graph_keys
from .postprocess import process_molecules
from .xyz import save_xyz_file
from .variational_diffusion import EquivariantVariationalDiffusion, _segment_mean_sub

log = logging.getLogger(__name__)


DEFAULT_LANES_MIN_SAMPLES = 64     # sample(): plain batches of at least this many molecules are drawn as two slices (see sample)

class _Dummy:
    """Placeholder for globals (omegaconf containers, functools.partial(torch.optim.AdamW), ...) found in the
    ``hyper_parameters`` of a Lightning checkpoint; only ``state_dict`` is used."""

    def __init__(self, *a, **k):
        pass

    def __setstate__(self, state):
        pass

    def __call__(self, *a, **k):
        return _Dummy()


class _StateDictUnpickler(pickle.Unpickler):
    """Resolves ONLY the globals a tensor state-dict needs, by (module, name); everything else in a Lightning checkpoint (omegaconf nodes,
    callbacks, optimizer objects, ...) becomes an inert placeholder.  In particular nothing from `builtins` that can run code (eval, exec,
    getattr, __import__, ...) and no `os` / `subprocess` / `torch.*` callables beyond the tensor rebuild helpers are reachable."""
    _ALLOWED = {
        ("collections", "OrderedDict"), ("collections", "defaultdict"),
        ("builtins", "dict"), ("builtins", "list"), ("builtins", "tuple"), ("builtins", "set"), ("builtins", "frozenset"),
        ("builtins", "int"), ("builtins", "float"), ("builtins", "bool"), ("builtins", "str"), ("builtins", "bytes"), ("builtins", "complex"),
        ("builtins", "slice"), ("builtins", "range"),
        ("_codecs", "encode"),
        ("torch._utils", "_rebuild_tensor_v2"), ("torch._utils", "_rebuild_tensor"), ("torch._utils", "_rebuild_parameter"),
        ("torch._utils", "_rebuild_parameter_with_state"), ("torch._tensor", "_rebuild_from_type_v2"), ("torch", "Size"), ("torch", "device"),
        ("torch", "Tensor"), ("torch.nn.parameter", "Parameter"), ("torch.serialization", "_get_layout"),
        ("numpy.core.multiarray", "_reconstruct"), ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "_reconstruct"),
        ("numpy._core.multiarray", "scalar"), ("numpy", "ndarray"), ("numpy", "dtype"),
    }
    _TORCH_TYPED = re.compile(r"^(Float|Double|Half|BFloat16|Long|Int|Short|Char|Byte|Bool|ComplexFloat|ComplexDouble)Storage$|^(float|double|half|bfloat16|"
                              r"float16|float32|float64|int8|int16|int32|int64|uint8|bool|long|int|short|complex64|complex128|strided)$")

    def find_class(self, module, name):
        if (module, name) in self._ALLOWED or (module in ("torch", "torch.storage") and self._TORCH_TYPED.match(name)) or \
                (module == "torch.storage" and name in ("UntypedStorage", "TypedStorage")):
            # (torch.storage._load_from_bytes is NOT here: it is torch.load(BytesIO(b), weights_only=False) with the default pickle
            #  module, i.e. an unrestricted inner unpickler a crafted checkpoint can REDUCE onto a bytes payload.  Zip-format checkpoints
            #  -- everything torch >= 1.6 and Lightning write -- never reference it.)
            try:
                return super().find_class(module, name)
            except Exception:
                return _Dummy
        return _Dummy


class _PickleShim:
    Unpickler = _StateDictUnpickler
    __name__ = "pickle"

    @staticmethod
    def load(f, **kw):
        return _StateDictUnpickler(f, **kw).load()


def load_lightning_state_dict(path: str) -> Dict[str, torch.Tensor]:
    """Reads ``state_dict`` from a reference ``*.ckpt`` without needing omegaconf / lightning importable."""
    try:
        ckpt = torch.load(path, map_location="cpu", weights_only=False, pickle_module=_PickleShim)
    except TypeError:
        ckpt = torch.load(path, map_location="cpu", pickle_module=_PickleShim)
    return ckpt["state_dict"] if "state_dict" in ckpt else ckpt


CHUNKED_EVAL_BASE_SEED = 1234      # evaluate_conditional's chunked modes without `seed`: batch i runs with 1234 + i, as sample_and_analyze's batches do
_CHUNKED_EVAL_REFUSED = ("node_mask", "fix_noise", "lanes", "noise_fn", "step_callback", "return_frames")


def _chunked_eval_mode(packed_batches: Optional[int], concurrent_batches: int) -> Tuple[str, int]:
    """("sequential" | "concurrent" | "packed", K) of evaluate_conditional's two arguments; sample_and_analyze's rules and wording."""
    if packed_batches is not None:
        if int(concurrent_batches) > 1:
            raise ValueError("packed_batches and concurrent_batches > 1 exclude each other: batches are either packed into one plan or run on lane handles")
        if int(packed_batches) < 1:
            raise ValueError("packed_batches must be >= 1")
        return "packed", int(packed_batches)
    if int(concurrent_batches) > 1:
        return "concurrent", int(concurrent_batches)
    return "sequential", 1


def _refuse_for_chunked_eval(mode: str, self_conditioned: bool, sample_kw: Dict[str, Any]) -> None:
    """What mol_gen_sample_packed / mol_gen_sample_concurrent cannot honour, refused by name before anything is drawn or launched."""
    arg = "packed_batches" if mode == "packed" else "concurrent_batches"
    if mode == "packed" and self_conditioned:
        raise NotImplementedError("evaluate_conditional: packed_batches does not serve a self-conditioned model (mol_gen_sample_packed refuses it); "
                                  "leave packed_batches out")
    for name in sample_kw:
        if name in _CHUNKED_EVAL_REFUSED:
            raise ValueError(f"evaluate_conditional: {name} cannot be honoured with {arg} (the batches of a chunk are plain samples on the device's own "
                             f"noise); leave {arg} out to pass {name}")
        if name != "num_timesteps":
            raise ValueError(f"evaluate_conditional: {name} is not passed on with {arg}: only num_timesteps is")


def conditional_eval_plan(iterations: int, K: int, seed: Optional[int], mode: str) -> Tuple[List[List[int]], List[Optional[int]]]:
    """The batches of one evaluate_conditional call: (chunks, seeds).  ``chunks`` lists the batch numbers 0 .. iterations of each sampling call, in
    order (``mode`` "sequential": one batch per call whatever K; "concurrent" / "packed": K per call, the last one shorter if need be);
    ``seeds[i]`` is the seed of batch i: ``seed + i``, with 1234 for a ``seed`` of None in the two chunked modes, and None -- the sampler's own
    default, the same for every batch -- in the sequential one."""
    if mode not in ("sequential", "concurrent", "packed"):
        raise ValueError(f"unknown mode {mode!r}")
    n = int(iterations) + 1
    if n < 1:
        raise ValueError("iterations must be >= 0")
    K = 1 if mode == "sequential" else int(K)
    if K < 1:
        raise ValueError("K must be >= 1")
    if seed is None:
        seeds = [None] * n if mode == "sequential" else [CHUNKED_EVAL_BASE_SEED + i for i in range(n)]
    else:
        seeds = [int(seed) + i for i in range(n)]
    return [list(range(i0, min(i0 + K, n))) for i0 in range(0, n, K)], seeds


class _MoleculeGenerationDDPM(nn.Module):
    _DATASETS: Dict[str, str] = {}

    def __init__(self, optimizer: Any = None, scheduler: Any = None, model_cfg: Any = None, module_cfg: Any = None,
                 layer_cfg: Any = None, diffusion_cfg: Any = None, dataloader_cfg: Any = None, path_cfg: Any = None, **kwargs):
        super().__init__()
        network = cfg_get(diffusion_cfg, "dynamics_network", "gcpnet")
        if network not in ("gcpnet", "egnn"):
            raise NotImplementedError(f"dynamics_network={network!r}: 'gcpnet' and 'egnn' are built (qm9_mol_gen_ddpm.py:101-131)")
        if cfg_get(diffusion_cfg, "ddpm_mode", "unconditional") not in ("unconditional", "inpainting"):
            raise ValueError("unsupported ddpm_mode")
        self.ddpm_mode = cfg_get(diffusion_cfg, "ddpm_mode", "unconditional")
        self.T = int(cfg_get(diffusion_cfg, "num_timesteps"))
        self.num_atom_types = int(cfg_get(dataloader_cfg, "num_atom_types"))
        self.num_x_dims = int(cfg_get(dataloader_cfg, "num_x_dims", 3))
        self.include_charges = bool(cfg_get(dataloader_cfg, "include_charges"))
        self.condition_on_context = len(cfg_get(module_cfg, "conditioning", []) or []) > 0
        name = str(cfg_get(dataloader_cfg, "dataset"))
        if name not in self._DATASETS:
            raise ValueError(f"dataset {name!r} not supported by {type(self).__name__}")
        self.dataset_info = _dataset_info(self._DATASETS[name])
        if network == "egnn":               # the EDM-style baseline (egnn_dynamics.py): the generic sampling loop, training on its operators path or, after set_train_path("fused"), its fused edge block
            dynamics_network = EGNNDynamics(model_cfg=model_cfg, module_cfg=module_cfg, diffusion_cfg=diffusion_cfg, dataloader_cfg=dataloader_cfg)
        else:
            dynamics_network = GCPNetDynamics(model_cfg=model_cfg, module_cfg=module_cfg, layer_cfg=layer_cfg,
                                              diffusion_cfg=diffusion_cfg, dataloader_cfg=dataloader_cfg)
        self.ddpm = EquivariantVariationalDiffusion(dynamics_network=dynamics_network, diffusion_cfg=diffusion_cfg,
                                                    dataloader_cfg=dataloader_cfg, dataset_info=self.dataset_info)
        self.props_distr = None   # PropertiesDistribution needs training data: attach_dataset(data.MoleculeDataset) sets it
        # qm9_mol_gen_ddpm.py:196-199: node-type statistics of the training set, for the KL reported by analyze_samples
        self.node_type_distribution = CategoricalDistribution(self.dataset_info["atom_types"], self.dataset_info["atom_encoder"])
        self.molecular_metrics = None   # attach_molecular_metrics() sets it (metrics.GraphMolecularMetrics: validity etc. without RDKit)
        self._init_kwargs = dict(model_cfg=model_cfg, module_cfg=module_cfg, layer_cfg=layer_cfg, diffusion_cfg=diffusion_cfg,
                                 dataloader_cfg=dataloader_cfg, path_cfg=path_cfg)

    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    def attach_dataset(self, dataset: Any, properties: Optional[List[str]] = None, num_bins: int = 1000):
        """Sets ``props_distr`` from a device-resident training set (data.MoleculeDataset): the reference's PropertiesDistribution over
        ``properties`` (default: the data set's ``conditioning``), normalised with the data set's own mean / mad -- what the reference's
        training script builds from ``train_dataloader()``.  Returns it."""
        from .data import PropertiesDistribution
        props = list(dataset.conditioning if properties is None else properties)
        if not props:
            raise ValueError("attach_dataset: no properties to condition on (the data set was built without `conditioning`)")
        self.props_distr = PropertiesDistribution(dataset, props, num_bins=num_bins, normalizer=dataset.mean_mad(props))
        return self.props_distr

    def attach_molecular_metrics(self, dataset: Any = None, dataset_keys: Optional[torch.Tensor] = None,
                                 valence_caps: Optional[Dict[str, int]] = None):
        """Sets ``molecular_metrics`` to a metrics.GraphMolecularMetrics, the stand-in for the reference's BasicMolecularMetrics
        (qm9_mol_gen_ddpm.py:201-206): from then on ``sample_and_analyze`` fills ``validity``, ``uniqueness`` and ``novelty``.  Novelty is
        taken against ``dataset_keys`` or, with a ``dataset`` (data.MoleculeDataset, the training split), against its ``graph_keys``; with
        neither it is 0.0, as in the reference without a SMILES list.  Returns the metrics object."""
        if dataset is not None and dataset_keys is not None:
            raise ValueError("attach_molecular_metrics takes a dataset or its keys, not both")
        if dataset is not None:
            dataset_keys = dataset.graph_keys(self.dataset_info, valence_caps=valence_caps)
        self.molecular_metrics = GraphMolecularMetrics(self.dataset_info, dataset_keys=dataset_keys, valence_caps=valence_caps)
        return self.molecular_metrics

    # the reference calls ``model.load_from_checkpoint(...)`` on an instance (mol_gen_sample.py:113-122)
    def load_from_checkpoint(self, checkpoint_path: str, map_location: Any = None, strict: bool = True, **kwargs):
        init = dict(self._init_kwargs)
        init.update({k: v for k, v in kwargs.items() if k in init})
        model = type(self)(**init)
        sd = load_lightning_state_dict(checkpoint_path)
        sd = {k: v for k, v in sd.items() if k.startswith("ddpm.")}
        missing, unexpected = model.load_state_dict(sd, strict=False)
        bad = [k for k in missing if k.startswith("ddpm.dynamics_network.")]
        if strict and (bad or [k for k in unexpected if k.startswith("ddpm.dynamics_network.")]):
            raise RuntimeError(f"checkpoint does not match the dynamics network: missing {bad[:4]} unexpected {unexpected[:4]}")
        if map_location is not None:
            model = model.to(map_location)
        return model

    # ---- loss / likelihood of a data batch (training, validation, test step), qm9_mol_gen_ddpm.py:184-277, 340-360, 429-459 --------
    def forward(self, batch: Any, dtype: torch.dtype = torch.float32, t_int: Optional[torch.Tensor] = None,
                noise: Optional[List[torch.Tensor]] = None, self_conditioning_prob: float = 0.5) -> Tuple[torch.Tensor, Dict[str, Any]]:
        """Loss per molecule and the batch means of the monitored terms.  Evaluation mode: the NLL (two evaluations of the network, fused
        kernels, inference mode).  Training mode: the L2 or VLB objective of ``diffusion_cfg.loss_type`` with gradients -- the network runs on
        the module path (HIP operators with autograd).  ``batch``: x, one_hot, charges, batch, mask and -- for a conditional model -- the
        per-node ``props_context`` (the reference derives it from the training set's property statistics, qm9utils.prepare_context; a
        batch of data.MoleculeDataset's loader carries it).  ``t_int`` / ``noise`` / ``self_conditioning_prob``: see EquivariantVariationalDiffusion.forward."""
        if self.training:
            return self._forward_impl(batch, dtype, t_int, noise, self_conditioning_prob)
        with torch.inference_mode():
            return self._forward_impl(batch, dtype, t_int, noise, self_conditioning_prob)

    def set_objective_path(self, path: str) -> None:
        """"operators" (default) | "fused": EquivariantVariationalDiffusion.set_objective_path, plus the centring of x and the NLL assembled
        from the terms (the tail of ``forward``) inside the same launches."""
        self.ddpm.set_objective_path(path)

    @property
    def objective_path(self) -> str:
        return self.ddpm.objective_path

    def _forward_fused(self, batch, dtype, t_int, noise, self_conditioning_prob=0.5):
        """``_forward_impl`` on the fused objective: x is centred, the terms are weighted and averaged inside its launches.  No device-to-host
        copy when ``batch.num_graphs`` is given; ``batch.x`` is left as it came.  ``loss_info["loss"]`` = mean(nll) with the graph."""
        batch.h = {"categorical": batch.one_hot, "integer": batch.charges}
        ctx = getattr(batch, "props_context", None)
        if self.condition_on_context:
            if ctx is None:
                raise ValueError("conditional model: batch.props_context (per node, normalised like the training set's) is required")
            batch.props_context = ctx.type(dtype)
        else:
            batch.props_context = None
        by_max = bool(cfg_get(self._init_kwargs["diffusion_cfg"], "norm_training_by_max_nodes", False))
        out = self.ddpm(batch, return_loss_info=True, t_int=t_int, noise=noise, self_conditioning_prob=self_conditioning_prob,
                        _objective=dict(center_x=True, norm_by_max_nodes=by_max))
        nll, loss, means = self.ddpm.last_objective
        loss_info = dict(out[-1])
        for name in ("loss_t", "SNR_weight", "loss_0", "kl_prior", "delta_log_px", "neg_log_const_0", "log_pN"):
            loss_info[name] = means[name]
        loss_info["loss"] = loss
        return nll, loss_info

    def _forward_impl(self, batch, dtype, t_int, noise, self_conditioning_prob=0.5):
        if self.ddpm.objective_path == "fused":
            return self._forward_fused(batch, dtype, t_int, noise, self_conditioning_prob)
        bi, mask = batch.batch, batch.mask
        B = getattr(batch, "num_graphs", None)                                  # a data loader's batch (data.py) brings it: no device-to-host copy
        B = int(bi.max().item()) + 1 if B is None else int(B)
        batch.x = _segment_mean_sub(batch.x, bi, B, mask)                         # centralize(..., edm=True): translation-invariant positions
        batch.h = {"categorical": batch.one_hot, "integer": batch.charges}
        ctx = getattr(batch, "props_context", None)
        if self.condition_on_context:
            if ctx is None:
                raise ValueError("conditional model: batch.props_context (per node, normalised like the training set's) is required")
            batch.props_context = ctx.type(dtype)
        else:
            batch.props_context = None
        num_nodes = torch.zeros(B, dtype=torch.long, device=bi.device).index_add_(0, bi, mask.long())
        batch.num_nodes_present, batch.num_graphs = num_nodes, B
        (delta_log_px, error_t, SNR_weight, loss_0_x, loss_0_h, neg_log_const_0, kl_prior, log_pN, t_int, loss_info) = self.ddpm(
            batch, return_loss_info=True, t_int=t_int, noise=noise, self_conditioning_prob=self_conditioning_prob)
        if self.training and cfg_get(self._init_kwargs["diffusion_cfg"], "loss_type", "l2") == "l2":
            # L2 training objective (:222-234): the squared error per predicted number, the x part of L_0 normalised the same way
            eff = num_nodes.max() if cfg_get(self._init_kwargs["diffusion_cfg"], "norm_training_by_max_nodes", False) else num_nodes
            denom = (self.num_x_dims + self.ddpm.num_node_scalar_features) * eff
            error_t = error_t / denom
            loss_t = 0.5 * error_t
            loss_0_x = loss_0_x / denom
            loss_0 = loss_0_x + loss_0_h
        else:
            loss_t = self.T * 0.5 * SNR_weight * error_t                          # the variational bound (:236-240); evaluation always scores it
            loss_0 = loss_0_x + loss_0_h + neg_log_const_0
        nll = loss_t + loss_0 + kl_prior - delta_log_px - log_pN                  # normalisation of x undone, joint with the size prior (:243-252)
        for name, v in (("loss_t", loss_t), ("SNR_weight", SNR_weight), ("loss_0", loss_0), ("kl_prior", kl_prior), ("delta_log_px", delta_log_px),
                        ("neg_log_const_0", neg_log_const_0), ("log_pN", log_pN)):
            loss_info[name] = v.mean(0)
        return nll, loss_info

    def training_step(self, batch: Any, batch_idx: int = 0, **kw) -> Dict[str, Any]:
        """qm9_mol_gen_ddpm.py:340-360 without the Lightning metric objects: ``metrics["loss"]`` carries the graph (call ``.backward()`` on it),
        every other entry is detached.  The module must be in training mode."""
        if not self.training:
            raise RuntimeError("training_step needs .train() (evaluation mode scores the NLL without gradients)")
        nll, metrics = self.step(batch, **kw)
        loss = metrics.pop("loss", None)                       # the fused objective's own mean(nll), with the graph
        metrics = {k: v.detach() for k, v in metrics.items()}
        metrics["loss"] = nll.mean(0) if loss is None else loss
        return metrics

    def step(self, batch: Any, **kw) -> Tuple[torch.Tensor, Dict[str, Any]]:
        return self.forward(batch, **kw)

    def configure_optimizers(self):
        """The reference's update after backward() as one fused step (optim.TrainingUpdate): AdamW(lr=1e-4, weight_decay=1e-12,
        amsgrad=True) of configs/model/*_mol_gen_ddpm.yaml, the adaptive clipping of configure_gradient_clipping when
        ``module_cfg.clip_gradients``, and the EMA of configs/callbacks/ema.yaml (decay 0.9999 every step from step 0).  Move the module to
        the GPU first."""
        from .optim import TrainingUpdate
        clip = bool(cfg_get(self._init_kwargs["module_cfg"], "clip_gradients", True))
        return TrainingUpdate(self.parameters(), lr=1e-4, weight_decay=1e-12, amsgrad=True, clip_gradients=clip, queue_len=50,
                              ema_decay=0.9999, ema_every=1, ema_start=0)

    def configure_data_parallel(self, group=None, accumulate_grad_batches: int = 1):
        """Opt-in: a fresh ``configure_optimizers()`` wrapped for data-parallel and accumulated steps (optim.BucketedUpdate) -- the
        reference's ``strategy: ddp_find_unused_parameters_false`` and ``accumulate_grad_batches`` (configs/trainer/default.yaml).  Call
        ``accumulate()`` after each ``backward()`` and ``step()`` after every ``accumulate_grad_batches``-th; with a process group, bring the
        replicas to one state first (parallel.broadcast_training_state).  Without one it runs as a single rank."""
        from .optim import BucketedUpdate
        return BucketedUpdate(self.configure_optimizers(), group=group, accumulate_grad_batches=accumulate_grad_batches)

    @torch.inference_mode()
    def validation_step(self, batch: Any, batch_idx: int = 0, **kw) -> Dict[str, Any]:
        """The metrics dictionary of the reference's validation / test step (without the Lightning logging around it)."""
        nll, metrics = self.step(batch, **kw)
        if "loss" not in metrics:                              # (the fused objective brings its own mean(nll))
            metrics["loss"] = nll.mean(0)
        g = self.ddpm.gamma.gamma
        metrics["log_SNR_max"], metrics["log_SNR_min"] = -g[0], -g[-1]            # -gamma(0), -gamma(1)
        return metrics

    test_step = validation_step

    @torch.inference_mode()
    def sample(self, num_samples: int, num_nodes: Optional[torch.Tensor] = None, node_mask: Optional[torch.Tensor] = None,
               context: Optional[torch.Tensor] = None, fix_noise: bool = False, num_timesteps: Optional[int] = None,
               **kw) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """qm9_mol_gen_ddpm.py:591-633."""
        if num_nodes is None:
            num_nodes = self.ddpm.num_nodes_distribution.sample(num_samples)
            assert int(num_nodes.max()) <= self.dataset_info.get("max_n_nodes", int(num_nodes.max()))
        if self.condition_on_context:
            if context is None:
                if self.props_distr is None:
                    raise ValueError("context required (no props_distr attached)")
                context = self.props_distr.sample_batch(num_nodes)
        else:
            context = None
        plain = not any(k in kw for k in ("lanes", "noise_fn", "step_callback", "_init_xh")) and kw.get("return_frames", 1) == 1
        if plain and not fix_noise and num_samples >= DEFAULT_LANES_MIN_SAMPLES and (node_mask is None or bool(node_mask.all())) \
                and not self.ddpm.runs_generic_loop_only():
            # plain batches: two slices of the flat batch on two handles / streams (same samples up to fp summation order).  One slice's node kernels
            # and launch tails run under the other's edge kernels: +4-5 % at 1024 QM9 molecules, +17 % at the evaluation driver's 100, +23 % at 64;
            # GEOM-Drugs +-0 at 64, -5 % at 32 (tools/ab_lanes.sh) -- hence the threshold
            kw["lanes"] = 2
        xh, batch_index, _ = self.ddpm.mol_gen_sample(num_samples=num_samples, num_nodes=num_nodes, node_mask=node_mask,
                                                      context=context, fix_noise=fix_noise, fix_self_conditioning_noise=fix_noise,
                                                      device=self.device, num_timesteps=num_timesteps, **kw)
        x = xh[:, : self.num_x_dims]
        one_hot = xh[:, self.num_x_dims:-1] if self.include_charges else xh[:, self.num_x_dims:]
        charges = xh[:, -1:] if self.include_charges else torch.zeros(0, device=self.device)
        return x, one_hot, charges, batch_index

    @torch.inference_mode()
    def generate_molecules(self, ddpm_mode: str = "unconditional", num_samples: int = 1, num_nodes: Optional[torch.Tensor] = None,
                           sanitize: bool = False, largest_frag: bool = False, add_hydrogens: bool = False,
                           sample_chain: bool = False, relax_iter: int = 0, num_timesteps: Optional[int] = None,
                           node_mask: Optional[torch.Tensor] = None, context: Optional[torch.Tensor] = None,
                           num_resamplings: int = 1, jump_length: int = 1,
                           molecule_builder: Optional[Callable[[torch.Tensor, torch.Tensor, Dict[str, Any]], Any]] = None,
                           **kw) -> List[Any]:
        """qm9_mol_gen_ddpm.py:1063-1243.  ``ddpm_mode="inpainting"`` (:1130-1181): RePaint on an all-zero molecule with the nodes of
        ``node_mask`` fixed (default: the first node of the batch), then every generated molecule is moved back to the given one's centre of
        mass.  Of the post-processing (``process_molecule``, rdkit_functions.py:323-379) the two graph filters run, on the device
        (postprocess.py): ``sanitize`` drops the molecules that fail the valence-cap verdict, ``largest_frag`` keeps the largest fragment's
        atoms; only surviving molecules are returned (with ``sample_chain`` the filters apply per frame, :1194-1209).  ``add_hydrogens``
        and ``relax_iter`` (AddHs, UFF: RDKit) are not done and warn."""
        if add_hydrogens or relax_iter > 0:
            skipped = [name for name, on in (("add_hydrogens", add_hydrogens), ("relax_iter", relax_iter > 0)) if on]
            warnings.warn(f"generate_molecules: {' and '.join(skipped)} not applied (AddHs and UFF relaxation need RDKit); the molecules are "
                          "returned without", UserWarning, stacklevel=2)
        if sample_chain:
            assert num_samples == 1, "Chain sampling is only supported for single-molecule batches."
            if ddpm_mode != "unconditional":
                raise NotImplementedError("chains are built for ddpm_mode='unconditional' only")
            # every step is a frame (return_frames = num_timesteps, :1122), frames put in generation order (reverse_tensor, :1186)
            T = self.ddpm.T if num_timesteps is None else num_timesteps
            if num_nodes is None:
                num_nodes = self.ddpm.num_nodes_distribution.sample(num_samples)
            if self.condition_on_context and context is None:
                if self.props_distr is None:
                    raise ValueError("context required (no props_distr attached)")
                context = self.props_distr.sample_batch(num_nodes)
            frames, _, _ = self.ddpm.mol_gen_sample(num_samples=1, num_nodes=num_nodes, device=self.device, return_frames=T, num_timesteps=T,
                                                    node_mask=node_mask, context=context if self.condition_on_context else None, **kw)
            frames = frames.reshape(T, -1, frames.shape[-1]).flip(0)
            oh = frames[:, :, self.num_x_dims:-1] if self.include_charges else frames[:, :, self.num_x_dims:]
            if sanitize or largest_frag:                              # T one-molecule entries: the flags apply per frame
                done = process_molecules(frames[:, :, : self.num_x_dims].reshape(-1, self.num_x_dims).contiguous(), oh.argmax(-1).reshape(-1),
                                         torch.full((frames.shape[0],), frames.shape[1], dtype=torch.int64), self.dataset_info,
                                         sanitize=sanitize, largest_frag=largest_frag)
                return [molecule_builder(pos, at, self.dataset_info) if molecule_builder is not None else (pos, at, None)
                        for pos, at, _ in done.tuples()]
            mols = []
            for pos, at in zip(frames[:, :, : self.num_x_dims].cpu(), oh.argmax(-1).cpu()):
                mols.append(molecule_builder(pos, at, self.dataset_info) if molecule_builder is not None else (pos, at, None))
            return mols
        if ddpm_mode == "unconditional":
            x, one_hot, charges, batch_index = self.sample(num_samples, num_nodes=num_nodes, node_mask=node_mask, context=context,
                                                           num_timesteps=num_timesteps, **kw)
        elif ddpm_mode == "inpainting":
            if num_nodes is None:
                num_nodes = self.ddpm.num_nodes_distribution.sample(num_samples)
                assert int(num_nodes.max()) <= self.dataset_info.get("max_n_nodes", int(num_nodes.max()))
            if self.condition_on_context:
                if context is None:
                    if self.props_distr is None:
                        raise ValueError("context required (no props_distr attached)")
                    context = self.props_distr.sample_batch(num_nodes)
            else:
                context = None
            dev = self.device
            n_total = int(torch.as_tensor(num_nodes).sum())
            batch_index = torch.repeat_interleave(torch.arange(len(num_nodes), device=dev), torch.as_tensor(num_nodes).to(dev))
            molecule = {"x": torch.zeros((n_total, self.num_x_dims), device=dev), "one_hot": torch.zeros((n_total, self.num_atom_types), device=dev),
                        "charges": torch.zeros((n_total, 1), device=dev), "num_nodes": num_nodes, "batch_index": batch_index}
            if node_mask is None:                     # "largely disable inpainting": only the first node is a fixed point (:1159-1162)
                node_mask = torch.zeros(n_total, dtype=torch.bool, device=dev)
                node_mask[0] = True
            xh = self.ddpm.inpaint(molecule=molecule, node_mask_fixed=node_mask, num_resamplings=num_resamplings, jump_length=jump_length,
                                   num_timesteps=num_timesteps, context=context, **kw)
            cnt = torch.as_tensor(num_nodes).to(dev, torch.float32)[:, None]
            com_before = torch.zeros((len(cnt), self.num_x_dims), device=dev).index_add_(0, batch_index, molecule["x"]) / cnt
            com_after = torch.zeros((len(cnt), self.num_x_dims), device=dev).index_add_(0, batch_index, xh[:, : self.num_x_dims]) / cnt
            x = xh[:, : self.num_x_dims] + (com_before - com_after)[batch_index]
            one_hot = xh[:, self.num_x_dims:-1] if self.include_charges else xh[:, self.num_x_dims:]
            charges = xh[:, -1:] if self.include_charges else torch.zeros(0, device=dev)
        else:
            raise NotImplementedError(f"ddpm_mode {ddpm_mode!r} is not implemented (reference: 'unconditional' | 'inpainting')")
        atom_types = one_hot.argmax(dim=-1)
        counts = torch.unique_consecutive(batch_index, return_counts=True)[1].tolist()
        if sanitize or largest_frag:
            done = process_molecules(x, atom_types, torch.tensor(counts, dtype=torch.int64), self.dataset_info,
                                     charges=charges if self.include_charges else None, sanitize=sanitize, largest_frag=largest_frag)
            return [molecule_builder(pos, at, self.dataset_info) if molecule_builder is not None else (pos, at, ch) for pos, at, ch in done.tuples()]
        mols, o = [], 0
        for n in counts:
            pos, at = x[o:o + n].cpu(), atom_types[o:o + n].cpu()
            ch = charges[o:o + n].cpu() if self.include_charges else None
            mols.append(molecule_builder(pos, at, self.dataset_info) if molecule_builder is not None else (pos, at, ch))
            o += n
        return mols


    @torch.inference_mode()
    def sample_and_save(self, num_samples: int, num_nodes: Optional[torch.Tensor] = None, node_mask: Optional[torch.Tensor] = None,
                        context: Optional[torch.Tensor] = None, num_timesteps: Optional[int] = None, id_from: int = 0,
                        name: str = "molecule", sampling_output_dir: Optional[str] = None,
                        norm_with_original_timesteps: bool = False, **kw) -> None:
        """qm9_mol_gen_ddpm.py:887-947 without the matplotlib / wandb visualisation: sample, write one XYZ file per molecule."""
        x, one_hot, charges, batch_index = self.sample(num_samples, num_nodes=num_nodes, node_mask=node_mask, context=context,
                                                       num_timesteps=num_timesteps, norm_with_original_timesteps=norm_with_original_timesteps, **kw)
        out_dir = str(sampling_output_dir) if sampling_output_dir is not None else os.path.join("sampling_output", "epoch_0")
        save_xyz_file(path=out_dir + "/", positions=x, one_hot=one_hot, charges=charges, dataset_info=self.dataset_info,
                      id_from=id_from, name=name, batch_index=batch_index)

    @torch.inference_mode()
    def sample_chain_and_save(self, keep_frames: int, node_mask: Optional[torch.Tensor] = None, context: Optional[torch.Tensor] = None,
                              id_from: int = 0, num_tries: int = 1, name: str = os.sep + "chain", verbose: bool = True,
                              sampling_output_dir: Optional[str] = None, num_timesteps: Optional[int] = None, **kw) -> bool:
        """qm9_mol_gen_ddpm.py:957-1060 without the matplotlib / wandb visualisation: one molecule sampled with `keep_frames` intermediate
        frames (up to `num_tries` times, until the final molecule is stable -- checked on the device), frames put in generation order, the
        last one repeated 10 times, one XYZ file per frame.  Returns whether the molecule shown is stable."""
        if "QM9" in str(self.dataset_info.get("name", "")).upper():
            num_nodes = torch.tensor([19], dtype=torch.long)
        else:
            num_nodes = self.ddpm.num_nodes_distribution.sample(1)
            assert int(num_nodes.max()) <= self.dataset_info.get("max_n_nodes", int(num_nodes.max()))
        if self.condition_on_context:
            if context is None:
                if self.props_distr is None:
                    raise ValueError("context required (no props_distr attached)")
                context = self.props_distr.sample_batch(num_nodes)
        else:
            context = None
        x = one_hot = charges = None
        mol_stable = False
        for i in range(num_tries):
            chain, _, _ = self.ddpm.mol_gen_sample(num_samples=1, num_nodes=num_nodes, node_mask=node_mask, context=context,
                                                   return_frames=keep_frames, device=self.device, num_timesteps=num_timesteps,
                                                   seed=kw.get("seed", 1234) + i, **{k: v for k, v in kw.items() if k != "seed"})
            chain = chain.reshape(keep_frames, -1, chain.shape[-1]).flip(0)
            chain = torch.cat([chain, chain[-1:].repeat(10, 1, 1)], dim=0)           # repeat the last frame to see the final sample better
            oh_last = chain[-1, :, self.num_x_dims:-1] if self.include_charges else chain[-1, :, self.num_x_dims:]
            res = check_molecular_stability_batch(chain[-1].contiguous(), oh_last.argmax(-1), num_nodes, self.dataset_info)
            mol_stable = bool(int(res[0, 0]))
            x = chain[:, :, : self.num_x_dims]
            oh = chain[:, :, self.num_x_dims:-1] if self.include_charges else chain[:, :, self.num_x_dims:]
            one_hot = torch.nn.functional.one_hot(oh.argmax(-1), num_classes=self.num_atom_types)
            charges = torch.round(chain[:, :, -1:]).long() if self.include_charges else torch.zeros(0, dtype=torch.long, device=self.device)
            if mol_stable:
                break
        F_, n = x.shape[0], x.shape[1]
        out_dir = os.path.join(str(sampling_output_dir) if sampling_output_dir is not None else os.path.join("sampling_output", "epoch_0"), "chain")
        save_xyz_file(path=out_dir, positions=x.reshape(-1, x.shape[-1]), one_hot=one_hot.reshape(-1, one_hot.shape[-1]),
                      charges=charges.reshape(-1, 1) if charges.numel() > 0 else charges, dataset_info=self.dataset_info, id_from=id_from, name=name,
                      batch_index=torch.arange(F_).repeat_interleave(n))
        return mol_stable

    @torch.inference_mode()
    def optimize(self, samples: List[Tuple[torch.Tensor, torch.Tensor]], num_timesteps: int, num_nodes: torch.Tensor,
                 context: Optional[torch.Tensor], node_mask: Optional[torch.Tensor] = None, sampling_output_dir: Optional[str] = None,
                 optim_property: Optional[str] = None, iteration_index: Optional[int] = None, return_frames: int = 1, id_from: int = 0,
                 chain_viz_batch_element_idx: int = 0, name: str = os.sep + "chain", norm_with_original_timesteps: bool = False,
                 verbose: bool = True, **kw) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """qm9_mol_gen_ddpm.py:636-743: property-guided optimisation of existing samples (``samples``: the reference's list of (x, one_hot) pairs, or
        the flat pair (x [N,3], one_hot [N,F]) this method returns -- see ``mol_gen_optimize``).  ``return_frames > 1`` (:674-731): the chain of molecule
        ``chain_viz_batch_element_idx`` -- frames in generation order, the last one repeated 10 times -- goes out as one XYZ file per frame under
        ``<sampling_output_dir>/<optim_property>/<time stamp>/iteration_<i>/chain`` (the reference then renders them with matplotlib / imageio:
        visualisation, not built), and the returned x / one_hot are frame 0 = the optimised molecules."""
        if not self.condition_on_context:
            raise Exception("Optimization requires a context conditional to optimize (e.g., `alpha`).")
        if context is None:
            if self.props_distr is None:
                raise ValueError("context required (no props_distr attached)")
            context = self.props_distr.sample_batch(num_nodes)
        xh, batch_index, _ = self.ddpm.mol_gen_optimize(samples=samples, num_nodes=num_nodes, node_mask=node_mask, context=context,
                                                        device=self.device, num_timesteps=num_timesteps, return_frames=return_frames,
                                                        norm_with_original_timesteps=norm_with_original_timesteps, **kw)
        if return_frames > 1:
            assert all(p is not None for p in (sampling_output_dir, optim_property, iteration_index)), \
                "Required parameters must be provided to visualize optimized molecules."
            import time as _time
            chain = xh[:, batch_index == chain_viz_batch_element_idx, :].flip(0)              # reverse_tensor (:679-680)
            chain = torch.cat([chain, chain[-1:].repeat(10, 1, 1)], dim=0)
            xs = chain[:, :, : self.num_x_dims]
            oh = chain[:, :, self.num_x_dims:-1] if self.include_charges else chain[:, :, self.num_x_dims:]
            one_hot_c = torch.nn.functional.one_hot(oh.argmax(-1), num_classes=self.num_atom_types)
            n_sel = torch.tensor([xs.shape[1]], dtype=torch.long)
            res = check_molecular_stability_batch(chain[-1].contiguous(), oh[-1].argmax(-1), n_sel, self.dataset_info)
            if verbose:
                log.info("Found stable molecule to visualize :)" if bool(int(res[0, 0])) else "Did not find stable molecule to visualize :(")
            out_dir = os.path.join(str(sampling_output_dir), str(optim_property), _time.strftime("%Y%m%d-%H%M%S"), f"iteration_{iteration_index}", "chain")
            save_xyz_file(path=out_dir, positions=xs.reshape(-1, xs.shape[-1]), one_hot=one_hot_c.reshape(-1, one_hot_c.shape[-1]),
                          charges=torch.tensor([]), dataset_info=self.dataset_info, id_from=id_from, name=name,
                          batch_index=torch.arange(xs.shape[0]).repeat_interleave(xs.shape[1]))
            self.last_chain_dir = out_dir
            x = xh[0, :, : self.num_x_dims]
            one_hot = xh[0, :, self.num_x_dims:-1] if self.include_charges else xh[0, :, self.num_x_dims:]
            charges = torch.round(chain[:, :, -1:]).long() if self.include_charges else torch.zeros(0, dtype=torch.long, device=self.device)   # (:705-709)
            return x, one_hot, charges, batch_index
        x = xh[:, : self.num_x_dims]
        one_hot = xh[:, self.num_x_dims:-1] if self.include_charges else xh[:, self.num_x_dims:]
        charges = xh[:, -1:] if self.include_charges else torch.zeros(0, device=self.device)
        return x, one_hot, charges, batch_index

    @torch.inference_mode()
    def sample_and_analyze(self, num_samples: int, node_mask: Optional[torch.Tensor] = None, context: Optional[torch.Tensor] = None,
                           batch_size: Optional[int] = None, max_num_nodes: Optional[int] = 100, num_timesteps: Optional[int] = None,
                           concurrent_batches: int = 1, packed_batches: Optional[int] = None, **kw) -> Dict[str, Any]:
        """qm9_mol_gen_ddpm.py:747-843 -- the evaluation driver: batches of `batch_size` molecules with sizes drawn from the
        dataset histogram, one 1000-step sampling run per batch, stability statistics.  The per-molecule host loop of the
        reference (`check_molecular_stability` on CPU copies) is one device launch per batch here; only three integers per
        molecule and the atom-type histogram ever leave the GPU.  `concurrent_batches > 1` keeps that many batches in flight on
        separate handles / streams (`mol_gen_sample_concurrent`): same samples, better use of the chip at the reference's batch
        size of 100.  `packed_batches = K` instead lays K batches end to end in one packed plan on the primary handle
        (`mol_gen_sample_packed`): the same samples again, without the lane handles; it excludes `concurrent_batches > 1`.
        `save_molecules` (xyz files) is `sample_and_save`.  With `attach_molecular_metrics` each batch also gets one launch of
        `molecule_graph_keys` next to the stability launch, in every mode, and the three RDKit-free metrics are filled in."""
        if packed_batches is not None:
            if int(concurrent_batches) > 1:
                raise ValueError("packed_batches and concurrent_batches > 1 exclude each other: batches are either packed into one plan or run on lane handles")
            if int(packed_batches) < 1:
                raise ValueError("packed_batches must be >= 1")
            self.ddpm.refuse_fused_sampler_only("sample_and_analyze(packed_batches=...)")
        elif int(concurrent_batches) > 1:
            self.ddpm.refuse_fused_sampler_only("sample_and_analyze(concurrent_batches=...)")
        max_num_nodes = self.dataset_info.get("max_n_nodes", max_num_nodes)
        batch_size = int(cfg_get(self._init_kwargs["dataloader_cfg"], "batch_size", 64)) if batch_size is None else batch_size
        batch_size = min(batch_size, num_samples)
        results, type_counts = [], torch.zeros(self.num_atom_types, dtype=torch.int64)
        metrics = self.molecular_metrics
        if metrics is not None:
            metrics.reset()
        plan, done = [], 0
        while done < num_samples:                               # draw all sizes first: the same random stream as the sequential driver
            nb = min(batch_size, num_samples - done)
            num_nodes = self.ddpm.num_nodes_distribution.sample(nb)
            assert int(num_nodes.max()) <= max_num_nodes
            ctx = context
            if self.condition_on_context and ctx is None:
                if self.props_distr is None:
                    raise ValueError("context required (no props_distr attached)")
                ctx = self.props_distr.sample_batch(num_nodes)
            plan.append((nb, num_nodes, ctx if self.condition_on_context else None))
            done += nb

        def account(xh, num_nodes):
            oh = xh[:, self.num_x_dims:-1] if self.include_charges else xh[:, self.num_x_dims:]
            atom_types = oh.argmax(-1)
            results.append(check_molecular_stability_batch(xh, atom_types, num_nodes, self.dataset_info))
            if metrics is not None:
                metrics.update(*molecule_graph_keys(xh, atom_types, num_nodes, self.dataset_info, metrics.valence_caps))
            type_counts.add_(torch.bincount(atom_types, minlength=self.num_atom_types).cpu())

        K = max(1, int(concurrent_batches)) if packed_batches is None else int(packed_batches)
        for i0 in range(0, len(plan), K):
            chunk = plan[i0:i0 + K]
            if packed_batches is not None:
                outs = self.ddpm.mol_gen_sample_packed([c[1] for c in chunk], self.device, num_timesteps=num_timesteps,
                                                       contexts=[c[2] for c in chunk], seeds=[1234 + i0 + j for j in range(len(chunk))])
                for (xh, _, _), c in zip(outs, chunk):
                    account(xh, c[1])
            elif K == 1:
                nb, num_nodes, ctx = chunk[0]
                xh, _, _ = self.ddpm.mol_gen_sample(num_samples=nb, num_nodes=num_nodes, node_mask=node_mask, context=ctx, device=self.device,
                                                    num_timesteps=num_timesteps, seed=1234 + i0, **kw)
                account(xh, num_nodes)
            else:
                outs = self.ddpm.mol_gen_sample_concurrent([c[1] for c in chunk], self.device, num_timesteps=num_timesteps,
                                                           contexts=[c[2] for c in chunk], seeds=[1234 + i0 + j for j in range(len(chunk))])
                for (xh, _, _), c in zip(outs, chunk):
                    account(xh, c[1])
        return self.analyze_samples(torch.cat(results).cpu(), type_counts, metrics)

    @torch.inference_mode()
    def evaluate_conditional(self, classifier: Any, property: str, mean: float, mad: float, iterations: int, batch_size: int,
                             props_distr: Any = None, unknown_labels: bool = False, save_molecules: bool = False,
                             sampling_output_dir: Optional[str] = None, packed_batches: Optional[int] = None, concurrent_batches: int = 1,
                             seed: Optional[int] = None, **sample_kw) -> Tuple[float, List[Dict[str, Any]]]:
        """The conditional-evaluation driver, src/mol_gen_eval_conditional_qm9.py:101-156 and :303-315 on the device: per batch draw the sizes,
        draw the (normalised) context from ``props_distr.sample_batch``, ``sample``, de-normalise the label with ``props_distr.normalizer``
        (``unknown_labels``: the label is the property's mean), classify the samples (classifier.EGNN.predict: one launch, no copy of the
        samples) and accumulate ``mean(|mad pred + mean - label|)`` with weight ``batch_size``.  The reference's loader yields while
        ``i <= iterations``, i.e. ``iterations + 1`` batches; so does this.  ``props_distr`` is duck-typed (``sample_batch``, ``properties``,
        ``normalizer``) and defaults to ``self.props_distr``.  ``save_molecules`` writes each batch's XYZ files under
        ``<sampling_output_dir>/run<i>/``.  Returns the MAE and one record per batch (loss, num_nodes, label, pred and the samples x / one_hot,
        all left on the device).

        Seeds.  The default call samples EVERY batch with the sampler's default seed (1234): device noise is a pure function of (seed, node index
        within the batch, draw number), so all ``iterations + 1`` batches share one noise tape and differ only through their sizes and contexts --
        the reference's global RNG advances between batches instead.  That default is kept as it is; pass ``seed`` to give batch ``i`` the seed
        ``seed + i`` and with it noise of its own.

        ``packed_batches = K`` / ``concurrent_batches = K > 1`` (they exclude each other, as in ``sample_and_analyze``): the sizes and contexts of
        all batches are drawn first, in the sequential order (sizes of batch 0, context of batch 0, sizes of batch 1, ...), then the batches run in
        chunks of K through ``mol_gen_sample_packed`` / ``mol_gen_sample_concurrent`` with seed ``base + i`` for batch ``i`` (``base``: ``seed``,
        or 1234), a chunk is classified in one launch and its per-batch losses reach the host in one copy.  Records, files and -- with the same
        ``seed`` and ``lanes=1`` on the sequential side -- samples are those of the sequential call.  These modes take ``num_timesteps`` in
        ``sample_kw`` and nothing else, and ``packed_batches`` no self-conditioned model: refused before any work."""
        mode, K = _chunked_eval_mode(packed_batches, concurrent_batches)
        if mode != "sequential":
            self.ddpm.refuse_fused_sampler_only(f"evaluate_conditional({'packed_batches' if mode == 'packed' else 'concurrent_batches'}=...)")
            _refuse_for_chunked_eval(mode, bool(getattr(self.ddpm.dynamics_network, "self_condition", False)), sample_kw)
        if not self.condition_on_context:
            raise Exception("Conditional evaluation requires a conditional model (module_cfg.conditioning).")
        props_distr = self.props_distr if props_distr is None else props_distr
        if props_distr is None:
            raise ValueError("evaluate_conditional needs props_distr (none attached)")
        prop_key = props_distr.properties[0]
        if prop_key != property:
            raise ValueError(f"props_distr conditions on {prop_key!r}, the classifier is evaluated on {property!r}")
        norm = props_distr.normalizer[prop_key]
        if mode != "sequential":
            return self._evaluate_conditional_chunked(classifier, mean, mad, norm, props_distr, unknown_labels, int(iterations), batch_size, mode, K,
                                                      seed, sample_kw.get("num_timesteps"), save_molecules, sampling_output_dir)
        total, count, records = 0.0, 0, []
        for i in range(int(iterations) + 1):
            num_nodes = self.ddpm.num_nodes_distribution.sample(batch_size)
            assert int(num_nodes.max()) <= self.dataset_info.get("max_n_nodes", int(num_nodes.max()))
            context = props_distr.sample_batch(num_nodes).to(self.device)
            if seed is not None:
                sample_kw["seed"] = int(seed) + i                                # (seed given: batch i draws its own noise)
            x, one_hot, charges, batch_index = self.sample(num_samples=batch_size, num_nodes=num_nodes, context=context, **sample_kw)
            if save_molecules:
                out_dir = os.path.join(str(sampling_output_dir) if sampling_output_dir is not None else "sampling_output", f"run{i}")
                save_xyz_file(path=out_dir + "/", positions=x, one_hot=one_hot, charges=charges, dataset_info=self.dataset_info,
                              id_from=i * batch_size, name="conditional", batch_index=batch_index)
            label = context.reshape(batch_size, -1)[:, 0].to(torch.float32)
            if unknown_labels:
                label = torch.full_like(label, float(norm["mean"]))
            else:
                label = label * float(norm["mad"]) + float(norm["mean"])
            pred = classifier.predict(x, one_hot, num_nodes=num_nodes)
            loss = (mad * pred + mean - label).abs().mean().item()               # one scalar per batch reaches the host
            total += loss * batch_size
            count += batch_size
            records.append(dict(loss=loss, num_nodes=num_nodes, label=label, pred=pred, x=x, one_hot=one_hot))
        return total / count, records

    def _evaluate_conditional_chunked(self, classifier, mean, mad, norm, props_distr, unknown_labels, iterations, batch_size, mode, K, seed,
                                      num_timesteps, save_molecules, sampling_output_dir):
        """evaluate_conditional with K batches per sampling call: the statements of the sequential loop, per chunk where they can be."""
        chunks, seeds = conditional_eval_plan(iterations, K, seed, mode)
        plan = []
        for i in range(iterations + 1):                              # draw everything first: the same random streams as the sequential driver
            num_nodes = self.ddpm.num_nodes_distribution.sample(batch_size)
            assert int(num_nodes.max()) <= self.dataset_info.get("max_n_nodes", int(num_nodes.max()))
            plan.append((num_nodes, props_distr.sample_batch(num_nodes).to(self.device)))
        sampler = self.ddpm.mol_gen_sample_packed if mode == "packed" else self.ddpm.mol_gen_sample_concurrent
        total, count, records = 0.0, 0, []
        for chunk in chunks:
            outs = sampler([plan[i][0] for i in chunk], self.device, num_timesteps=num_timesteps, contexts=[plan[i][1] for i in chunk],
                           seeds=[seeds[i] for i in chunk])
            xh = torch.cat([o[0] for o in outs], dim=0)
            one_hot_all = xh[:, self.num_x_dims:-1] if self.include_charges else xh[:, self.num_x_dims:]
            pred_all = classifier.predict(xh[:, : self.num_x_dims], one_hot_all, num_nodes=torch.cat([plan[i][0] for i in chunk]))   # one launch
            losses, parts = [], []
            for j, (i, (xh_b, batch_index, _)) in enumerate(zip(chunk, outs)):
                num_nodes, context = plan[i]
                x = xh_b[:, : self.num_x_dims]
                one_hot = xh_b[:, self.num_x_dims:-1] if self.include_charges else xh_b[:, self.num_x_dims:]
                charges = xh_b[:, -1:] if self.include_charges else torch.zeros(0, device=self.device)
                if save_molecules:
                    out_dir = os.path.join(str(sampling_output_dir) if sampling_output_dir is not None else "sampling_output", f"run{i}")
                    save_xyz_file(path=out_dir + "/", positions=x, one_hot=one_hot, charges=charges, dataset_info=self.dataset_info,
                                  id_from=i * batch_size, name="conditional", batch_index=batch_index)
                label = context.reshape(batch_size, -1)[:, 0].to(torch.float32)
                if unknown_labels:
                    label = torch.full_like(label, float(norm["mean"]))
                else:
                    label = label * float(norm["mad"]) + float(norm["mean"])
                pred = pred_all[j * batch_size:(j + 1) * batch_size]
                losses.append((mad * pred + mean - label).abs().mean())          # the sequential statement on the same values: the same bits
                parts.append(dict(num_nodes=num_nodes, label=label, pred=pred, x=x, one_hot=one_hot))
            for loss, part in zip(torch.stack(losses).tolist(), parts):          # one copy per chunk reaches the host
                total += loss * batch_size
                count += batch_size
                records.append(dict(loss=loss, **part))
        return total / count, records

    @torch.inference_mode()
    def evaluate_optimization(self, classifier: Any, property: str, mean: float, mad: float, samples: Any, num_nodes: torch.Tensor,
                              num_iterations: int, num_timesteps: int, context: Optional[torch.Tensor] = None, props_distr: Any = None,
                              unknown_labels: bool = False, score_initial_samples: bool = True, seed: int = 1234, save_molecules: bool = False,
                              sampling_output_dir: Optional[str] = None) -> List[Dict[str, Any]]:
        """The optimisation-evaluation driver, src/mol_gen_eval_optimization_qm9.py:133-241 and :433-450 on the device: ``num_iterations`` times
        ``optimize`` the samples for ``num_timesteps`` steps (``norm_with_original_timesteps=False``, as the reference insists), count the stable
        molecules and atoms (``check_molecular_stability_batch``) and score the property classifier against the requested, de-normalised property.

        ``samples``: the flat pair ``(x [N,3], one_hot [N,F])``, rows as ``num_nodes`` [B] lays them out, or the reference's list of B
        ``(x, one_hot)`` pairs (concatenated once, up front).  ``context`` [B, 1] (normalised) is kept for all iterations, as in the reference;
        without it, it is drawn once from ``props_distr`` (default ``self.props_distr``).  The label is ``context * mad + mean`` with the mean / mad
        of ``props_distr.normalizer`` when a ``props_distr`` is there, else with the classifier's ``mean`` / ``mad`` (the reference builds both from
        the same statistics); ``unknown_labels``: the label is that mean.  Iteration ``it`` runs with ``seed + it``: with one seed for all of them
        every iteration would add the very same noise tape to its input.

        Between iterations the samples stay flat on the device -- no per-molecule masks, no list -- and per iteration the three stability integers
        per molecule and one scalar reach the host.  ``save_molecules`` writes iteration ``it`` to ``<sampling_output_dir>/run<it + 2>/`` (the
        reference's numbering: run 1 is the scoring of the initial samples, which writes nothing).

        Returns a list of records ``dict(iteration, mae, mol_stable, atm_stable, x, one_hot)``: first the initial samples (``iteration`` None) when
        ``score_initial_samples``, then iterations 0 .. num_iterations - 1; ``x`` / ``one_hot`` stay on the device."""
        if not self.condition_on_context:
            raise Exception("Optimization requires a context conditional to optimize (e.g., `alpha`).")
        if self.include_charges:
            raise NotImplementedError("mol_gen_optimize builds z without the charge column (reference :1457): include_charges must be False")
        if int(num_iterations) < 1:
            raise ValueError(f"num_iterations must be >= 1, got {num_iterations}")
        num_nodes = torch.as_tensor(num_nodes).cpu()
        if len(samples) == 2 and all(torch.is_tensor(s) for s in samples):
            x, one_hot = samples
        else:
            if len(samples) != len(num_nodes):
                raise ValueError(f"{len(samples)} (x, one_hot) pairs for {len(num_nodes)} molecules in num_nodes")
            x, one_hot = torch.cat([s[0] for s in samples], dim=0), torch.cat([s[1] for s in samples], dim=0)
        if x.shape[0] != int(num_nodes.sum()) or one_hot.shape[0] != x.shape[0]:
            raise ValueError(f"samples have {x.shape[0]} / {one_hot.shape[0]} rows (x / one_hot), num_nodes sums to {int(num_nodes.sum())}")
        props_distr = self.props_distr if props_distr is None else props_distr
        if props_distr is not None and props_distr.properties[0] != property:
            raise ValueError(f"props_distr conditions on {props_distr.properties[0]!r}, the classifier is evaluated on {property!r}")
        if context is None:
            if props_distr is None:
                raise ValueError("evaluate_optimization needs context or props_distr (none attached)")
            context = props_distr.sample_batch(num_nodes)
        norm = props_distr.normalizer[property] if props_distr is not None else {"mean": mean, "mad": mad}
        B = len(num_nodes)
        context = context.to(self.device)
        label = context.reshape(B, -1)[:, 0].to(torch.float32)
        if unknown_labels:
            label = torch.full_like(label, float(norm["mean"]))
        else:
            label = label * float(norm["mad"]) + float(norm["mean"])
        x, one_hot = x.to(self.device, torch.float32), one_hot.to(self.device, torch.float32)

        def record(iteration, x, one_hot):
            st = check_molecular_stability_batch(x, one_hot.argmax(-1), num_nodes, self.dataset_info).cpu().to(torch.int64)   # 3 integers per molecule
            pred = classifier.predict(x, one_hot, num_nodes=num_nodes)
            mae = (mad * pred + mean - label).abs().mean().item()                # one scalar
            return dict(iteration=iteration, mae=mae, mol_stable=float(st[:, 0].sum()) / float(B), atm_stable=float(st[:, 1].sum()) / float(st[:, 2].sum()),
                        x=x, one_hot=one_hot)

        records = [record(None, x, one_hot)] if score_initial_samples else []
        for it in range(int(num_iterations)):
            x, one_hot, charges, batch_index = self.optimize((x, one_hot), num_timesteps=num_timesteps, num_nodes=num_nodes, context=context,
                                                             norm_with_original_timesteps=False, seed=int(seed) + it)
            if save_molecules:
                out_dir = os.path.join(str(sampling_output_dir) if sampling_output_dir is not None else "sampling_output", f"run{it + 2}")
                save_xyz_file(path=out_dir + "/", positions=x, one_hot=one_hot, charges=charges, dataset_info=self.dataset_info,
                              id_from=0, name="conditional", batch_index=batch_index)
            records.append(record(it, x, one_hot))
        return records

    def analyze_samples(self, stability: torch.Tensor, atom_type_counts: torch.Tensor, molecular_metrics: Any = None) -> Dict[str, Any]:
        """qm9_mol_gen_ddpm.py:846-885 on the device results: `stability` int [M, 3] rows (stable, nr_stable_atoms, n).  `molecular_metrics`:
        an updated metrics.GraphMolecularMetrics, whose `compute()` fills validity, uniqueness and novelty (None without one)."""
        st = stability.to(torch.int64)
        q = atom_type_counts.to(torch.float64).numpy()
        p = self.node_type_distribution.p
        with np.errstate(divide="ignore", invalid="ignore"):
            kl = float(-np.sum(p * np.log(q / q.sum() / p + self.node_type_distribution.EPS)))
        out = {
            "kl_div_atom_types": kl,
            "mol_stable": float(st[:, 0].sum()) / float(len(st)),
            "atm_stable": float(st[:, 1].sum()) / float(st[:, 2].sum()),
            "validity": None, "uniqueness": None, "novelty": None,    # filled from attach_molecular_metrics' GraphMolecularMetrics below
        }
        if molecular_metrics is not None:
            out["validity"], out["uniqueness"], out["novelty"] = (float(v) for v in molecular_metrics.compute())
        return out


class QM9MoleculeGenerationDDPM(_MoleculeGenerationDDPM):
    """``_target_`` stand-in for src.models.qm9_mol_gen_ddpm.QM9MoleculeGenerationDDPM."""
    _DATASETS = {"QM9": "qm9", "QM9_second_half": "qm9_second_half"}


class GEOMMoleculeGenerationDDPM(_MoleculeGenerationDDPM):
    """``_target_`` stand-in for src.models.geom_mol_gen_ddpm.GEOMMoleculeGenerationDDPM."""
    _DATASETS = {"GEOM": "geom"}


def sample_sweep_conditionally(model: Any, props_distr: Any, num_nodes: int = 19, num_frames: int = 100
                               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """src/models/__init__.py:200-226: `num_frames` molecules of `num_nodes` atoms whose (normalised) property context sweeps linearly from the
    smallest to the largest value seen for that size, all drawn with the same noise (`fix_noise=True`: option "fix_noise" of the library)."""
    num_nodes_ = torch.tensor([num_nodes] * num_frames, device=model.device)
    cols = []
    for key in props_distr.distributions:
        lo, hi = props_distr.distributions[key][num_nodes]["params"]
        mean, mad = props_distr.normalizer[key]["mean"], props_distr.normalizer[key]["mad"]
        lo_n, hi_n = float((torch.as_tensor(lo) - mean) / mad), float((torch.as_tensor(hi) - mean) / mad)
        cols.append(torch.tensor(np.linspace(lo_n, hi_n, num_frames)).unsqueeze(1))
    context = torch.cat(cols, dim=-1).float().to(model.device)
    return model.sample(num_samples=num_frames, num_nodes=num_nodes_, context=context, fix_noise=True)
