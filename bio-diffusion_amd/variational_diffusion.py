"""The diffusion model around the MI355X dynamics network: schedule, objective and samplers.

Mirror of ``src/models/components/variational_diffusion.py``:
``PredefinedNoiseSchedule`` (:206-255), ``EquivariantVariationalDiffusion`` with ``sigma/alpha/SNR`` (:318-338),
``sigma_and_alpha_t_given_s`` (:342-367), ``sample_combined_position_feature_noise`` (:795-819),
``sample_normal`` (:822-837), ``sample_p_zs_given_zt`` (:1204-1278), ``sample_p_xh_given_z0`` (:840-907),
``mol_gen_sample`` (:1282-1412), RePaint inpainting (``inpaint``, :1582-1789) and the property-guided optimisation loop
(``mol_gen_optimize``, :1416-1546), plus ``NumNodesDistribution`` (src/models/__init__.py:264-308).
``forward`` (:948-1160) gives the likelihood terms of a data batch: evaluation mode with two evaluations of the network on the fused kernels,
training mode with one evaluation under autograd; the algebra around the network runs on HIP operators or (``set_objective_path("fused")``) in
the fused objective kernels.

Three ways to sample:
  * ``sample_p_zs_given_zt`` / ``sample_p_xh_given_z0`` -- the reference's method signatures, torch ops on the device for the O(N) algebra
    and the HIP dynamics forward for the network call (used by the teacher-forced parity tests);
  * the module-path loops on those methods (masked nodes, position-only diffusion, configurations off the fused sampling kernels);
  * the production loops on ``gcdm_sample_init / gcdm_sample_step / gcdm_sample_final`` (one fused HIP kernel per step after the network
    kernels; noise from a tape or on-device Philox; a device flag word read once at the end instead of host-side asserts): their drivers
    are in ``fused_sampler``; the public methods here check their arguments, choose the loop and call them.
"""
from __future__ import annotations

import logging
from itertools import count
from random import random as _random
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _native, fused_sampler, ops
from .config import AttrDict, cfg_get
from .fused_sampler import RANGE_CHECK_EVERY, _RangeCheckpoints, num_nodes_to_batch_index, slice_cuts  # noqa: F401  (also this module's names)
from .gcpnet import F16RangeError

log = logging.getLogger(__name__)


def inflate_batch_array(array: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """src/models/__init__.py:80-86."""
    return array.view((array.shape[0],) + (1,) * (len(target.shape) - 1))


def _segment_mean_sub(x: torch.Tensor, batch_index: torch.Tensor, num_graphs: int, mask: torch.Tensor) -> torch.Tensor:
    """centralize(..., edm=True) (components/__init__.py:45-98) without torch_scatter."""
    mf = mask.to(x.dtype)
    cnt = torch.zeros(num_graphs, dtype=x.dtype, device=x.device).index_add_(0, batch_index, mf).unsqueeze(-1)
    s = torch.zeros(num_graphs, x.shape[1], dtype=x.dtype, device=x.device).index_add_(0, batch_index, x)
    return x - (s / cnt)[batch_index] * mf.unsqueeze(-1)


def polynomial_gamma(num_timesteps: int, noise_precision: float, power: float) -> np.ndarray:
    """gamma table of the "polynomial_<power>" schedule in float64 (variational_diffusion.py:67-107, 237-246)."""
    steps = num_timesteps + 1
    x = np.linspace(0, steps, steps)
    a2 = (1 - np.power(x / steps, power)) ** 2
    a2 = np.concatenate([np.ones(1), a2], axis=0)
    a2 = np.cumprod(np.clip(a2[1:] / a2[:-1], a_min=0.001, a_max=1.0), axis=0)
    a2 = (1 - 2 * noise_precision) * a2 + noise_precision
    return -(np.log(a2) - np.log(1 - a2))


def cosine_gamma(num_timesteps: int, s: float = 0.008) -> np.ndarray:
    """gamma table of the "cosine" schedule in float64 (cosine_beta_schedule + PredefinedNoiseSchedule, variational_diffusion.py:37-58, 220-243)."""
    steps = num_timesteps + 2
    x = np.linspace(0, steps, steps)
    ac = np.cos(((x / steps) + s) / (1 + s) * np.pi * 0.5) ** 2
    ac = ac / ac[0]
    a2 = np.cumprod(1.0 - np.clip(1 - (ac[1:] / ac[:-1]), a_min=0, a_max=0.999), axis=0)
    return -(np.log(a2) - np.log(1 - a2))


def repaint_schedule(resamplings: int, jump_length: int, num_timesteps: int) -> List[int]:
    """RePaint schedule (variational_diffusion.py:1548-1578, `get_repaint_schedule`): the number of denoising steps to apply before each
    jump back, from t = T downwards.  T is cut into ``(T-1) // jump_length`` stretches of ``jump_length`` steps plus a remainder; every
    stretch is visited ``resamplings`` times, the last visit running on through the following stretch, and the remainder joins the last
    entry.  (With one resampling there is never a jump: the schedule is [T].)"""
    if num_timesteps <= 0:
        return []
    if jump_length <= 0:
        raise ValueError("jump_length must be positive")
    stretches = (num_timesteps - 1) // jump_length
    rest = num_timesteps - stretches * jump_length
    if stretches == 0 or resamplings <= 0:
        return [rest]
    if resamplings == 1:
        return [num_timesteps]
    low_to_high = [jump_length] * (resamplings - 1)
    low_to_high += ([2 * jump_length] + [jump_length] * (resamplings - 2)) * (stretches - 1)
    low_to_high.append(jump_length + rest)
    return low_to_high[::-1]


def _check_frames(return_frames: int, num_timesteps: int) -> None:
    assert 0 < return_frames <= num_timesteps, "Number of frames cannot be greater than number of timesteps."
    assert num_timesteps % return_frames == 0, "Number of frames must be evenly divisible by number of timesteps."


def _module_draws(noise_fn: Optional[Callable[[int], torch.Tensor]], seed: int, device) -> Tuple[Optional[torch.Generator], Callable[[], Optional[torch.Tensor]]]:
    """Noise of a module-path loop, as (generator, draw): ``draw()`` is the next raw draw of the tape (k = 0, 1, ...), or None without a tape -- the
    draws then come from the device generator seeded with ``seed``, so that a re-run after F16RangeError draws the same noise."""
    if noise_fn is None:
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed))
        return gen, lambda: None
    k = count()
    return None, lambda: noise_fn(next(k)).to(device, torch.float32)


class PredefinedNoiseSchedule(nn.Module):
    def __init__(self, noise_schedule: str, num_timesteps: int, noise_precision: float, verbose: bool = False, **kwargs):
        super().__init__()
        self.timesteps = num_timesteps
        if noise_schedule == "cosine":
            g = cosine_gamma(num_timesteps)
        elif "polynomial" in noise_schedule:
            splits = noise_schedule.split("_")
            assert len(splits) == 2
            g = polynomial_gamma(num_timesteps, float(noise_precision), float(splits[1]))
        else:
            raise ValueError(noise_schedule)
        self.gamma = nn.Parameter(torch.tensor(g).float(), requires_grad=False)

    def forward(self, t: torch.Tensor) -> torch.Tensor:
        return self.gamma[torch.round(t * self.timesteps).long()]


class NumNodesDistribution(nn.Module):
    """src/models/__init__.py:264-308."""

    def __init__(self, histogram: Dict[int, int], verbose: bool = False, eps: float = 1e-30):
        super().__init__()
        self.eps = eps
        sizes = list(histogram)                                  # insertion order = the order of the checkpoint's buffers
        counts = torch.tensor([histogram[n] for n in sizes])
        self.keys = {n: i for i, n in enumerate(sizes)}
        self.register_buffer("num_nodes", torch.tensor(sizes))
        self.register_buffer("prob", counts / counts.sum())      # same state-dict entries as the reference: sizes and normalised frequencies

    @property
    def m(self) -> torch.distributions.Categorical:
        """Built from the CURRENT `prob` buffer (a checkpoint may have replaced it after construction) and on the CPU, so that a torch seed
        draws the sizes the reference draws (its Categorical is created before the module moves to the GPU)."""
        return torch.distributions.Categorical(self.prob.detach().cpu())

    def sample(self, n_samples: int = 1) -> torch.Tensor:
        idx = self.m.sample((n_samples,))
        return self.num_nodes[idx.to(self.num_nodes.device)]

    def log_prob(self, batch_n_nodes: torch.Tensor) -> torch.Tensor:
        idcs = torch.tensor([self.keys[n] for n in batch_n_nodes.tolist()], device=batch_n_nodes.device)        # one host copy, not one per molecule
        return torch.log(self.prob + self.eps)[idcs]


class _Batch(AttrDict):
    """Attribute bag with the three fields the dynamics network reads (stand-in for torch_geometric Batch)."""


class EquivariantVariationalDiffusion(nn.Module):
    def __init__(self, dynamics_network: nn.Module, diffusion_cfg: Any, dataloader_cfg: Any, dataset_info: Dict[str, Any]):
        super().__init__()
        assert cfg_get(diffusion_cfg, "parametrization", "eps") in ["eps"], "Epsilon is currently the only supported parametrization."
        if cfg_get(diffusion_cfg, "noise_schedule") == "learned":
            raise NotImplementedError("learned noise schedule (training) is out of scope")
        self.diffusion_cfg = diffusion_cfg
        self.diffusion_target = cfg_get(diffusion_cfg, "diffusion_target", "atom_types_and_coords")
        self.num_atom_types = int(cfg_get(dataloader_cfg, "num_atom_types"))
        self.num_x_dims = int(cfg_get(dataloader_cfg, "num_x_dims", 3))
        self.include_charges = bool(cfg_get(dataloader_cfg, "include_charges"))
        self.num_node_scalar_features = self.num_atom_types + int(self.include_charges)
        self.T = int(cfg_get(diffusion_cfg, "num_timesteps"))
        self.dynamics_network = dynamics_network
        histogram = {int(k): int(v) for k, v in dataset_info["n_nodes"].items()}
        self.num_nodes_distribution = NumNodesDistribution(histogram)
        self.gamma = PredefinedNoiseSchedule(noise_schedule=cfg_get(diffusion_cfg, "noise_schedule"), num_timesteps=self.T,
                                             noise_precision=float(cfg_get(diffusion_cfg, "noise_precision")))
        self._gamma_uploaded = None
        self._objective_path = "operators"
        self._objective_flags = None          # int32 [1] on the device, OR-ed into by the fused objective, read lazily (read_objective_flags)
        self._log_pn_cache = None
        # outcome of the last sampling call: device flag word, range rewinds, step an fp32 resume started from
        self.last_flags, self.last_range_rewinds, self.last_range_resume_step = 0, 0, None

    # ---- schedule algebra (:318-367) ---------------------------------------------------------------
    @staticmethod
    def sigma(gamma, target_tensor):
        return inflate_batch_array(torch.sqrt(torch.sigmoid(gamma)), target_tensor)

    @staticmethod
    def alpha(gamma, target_tensor):
        return inflate_batch_array(torch.sqrt(torch.sigmoid(-gamma)), target_tensor)

    @staticmethod
    def SNR(gamma):
        return torch.exp(-gamma)

    @staticmethod
    def sigma_and_alpha_t_given_s(gamma_t, gamma_s, target_tensor):
        sigma2_t_given_s = inflate_batch_array(-torch.expm1(F.softplus(gamma_s) - F.softplus(gamma_t)), target_tensor)
        log_alpha2_t_given_s = F.logsigmoid(-gamma_t) - F.logsigmoid(-gamma_s)
        alpha_t_given_s = inflate_batch_array(torch.exp(0.5 * log_alpha2_t_given_s), target_tensor)
        return sigma2_t_given_s, torch.sqrt(sigma2_t_given_s), alpha_t_given_s

    # ---- noise (:396-437, 795-837) -----------------------------------------------------------------
    def sample_combined_position_feature_noise(self, batch_index, node_mask, generate_x_only: bool = False,
                                               generator: Optional[torch.Generator] = None, num_graphs: Optional[int] = None):
        # (num_graphs: the batch size when the caller knows it -- the reference's torch_scatter call derives it from batch_index.max(), a host
        #  sync per draw that leaves the GPU idle for ~0.6 ms per sampling step at the benchmark size)
        n, B = len(batch_index), (int(batch_index.max().item()) + 1 if num_graphs is None else int(num_graphs))
        dev = batch_index.device
        z_x = torch.randn((n, self.num_x_dims), device=dev, generator=generator) * node_mask.float().unsqueeze(-1)
        z_x = _segment_mean_sub(z_x, batch_index, B, node_mask)
        if generate_x_only:
            return z_x
        z_h = torch.randn((n, self.num_node_scalar_features), device=dev, generator=generator) * node_mask.float().unsqueeze(-1)
        return torch.cat([z_x, z_h], dim=-1)

    def sample_normal(self, mu, sigma, batch_index, node_mask, fix_noise: bool = False, generate_x_only: bool = False,
                      eps: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None):
        if eps is None:
            bi = torch.zeros_like(batch_index) if fix_noise else batch_index
            eps = self.sample_combined_position_feature_noise(bi, node_mask, generate_x_only=generate_x_only, generator=generator,
                                                              num_graphs=1 if fix_noise else sigma.shape[0])
        return mu + sigma[batch_index] * eps

    def compute_x_pred(self, zt, net_out, gamma_t, batch_index):
        sigma_t = self.sigma(gamma_t, target_tensor=net_out)
        alpha_t = self.alpha(gamma_t, target_tensor=net_out)
        return 1.0 / alpha_t[batch_index] * (zt - sigma_t[batch_index] * net_out)

    @staticmethod
    def assert_mean_zero_with_mask(x, node_mask, eps: float = 1e-10):
        largest_value = x.abs().max().item()
        error = torch.sum(x, dim=0, keepdim=True).abs().max().item()
        rel_error = error / (largest_value + eps)
        assert rel_error < 1e-2, f"Mean is not zero, as relative_error {rel_error}"

    # ---- likelihood terms of a data batch, evaluation mode (:371-397, 449-454, 493-557, 580-732, 910-1160) ---------------------
    @staticmethod
    def sum_node_features_except_batch(values, batch_index, num_graphs: Optional[int] = None):
        B = int(batch_index.max().item()) + 1 if num_graphs is None else num_graphs
        return torch.zeros(B, dtype=values.dtype, device=values.device).index_add_(0, batch_index, values.sum(-1))

    @staticmethod
    def gaussian_KL(q_mu_minus_p_mu_squared, q_sigma, p_sigma, d):
        return d * torch.log(p_sigma / q_sigma) + 0.5 * (d * q_sigma ** 2 + q_mu_minus_p_mu_squared) / p_sigma ** 2 - 0.5 * d

    @staticmethod
    def cdf_standard_gaussian(x):
        return 0.5 * (1.0 + torch.erf(x * (0.5 ** 0.5)))

    def subspace_dimensionality(self, num_nodes):
        return (num_nodes - 1) * self.num_x_dims

    def delta_log_px(self, num_nodes):
        return -self.subspace_dimensionality(num_nodes) * float(np.log(cfg_get(self.diffusion_cfg, "norm_values")[0]))

    def log_pN(self, num_nodes):
        return self.num_nodes_distribution.log_prob(num_nodes)

    def normalize(self, x, h, node_mask, generate_x_only: bool = False):
        nv, nb = cfg_get(self.diffusion_cfg, "norm_values"), cfg_get(self.diffusion_cfg, "norm_biases")
        x = x / nv[0]
        if generate_x_only:
            return x, (h.float() - nb[1]) / nv[1]
        m = node_mask.float()
        h_cat = (h["categorical"].float() - nb[1]) / nv[1] * m.unsqueeze(-1)
        h_int = (h["integer"].float() - nb[2]) / nv[2]
        if self.include_charges:
            h_int = h_int * m
        return x, {"categorical": h_cat, "integer": h_int}

    def compute_noised_representation(self, xh, batch_index, node_mask, gamma_t, generate_x_only: bool = False, eps: Optional[torch.Tensor] = None):
        """z_t ~ q(z_t | x, h) (:910-931).  ``eps``: optional RAW standard-normal draws [N, 3 + F] (masked and CoM-projected here)."""
        if eps is None:
            eps = self.sample_combined_position_feature_noise(batch_index, node_mask, generate_x_only=generate_x_only, num_graphs=int(gamma_t.shape[0]))
        else:
            m = node_mask.float().unsqueeze(-1)
            ex = _segment_mean_sub(eps[:, : self.num_x_dims] * m, batch_index, int(gamma_t.shape[0]), node_mask)
            eps = torch.cat([ex, eps[:, self.num_x_dims:] * m], dim=-1)
        return self.alpha(gamma_t, xh)[batch_index] * xh + self.sigma(gamma_t, xh)[batch_index] * eps, eps

    def compute_kl_prior(self, xh, batch_index, node_mask, num_nodes, device=None, generate_x_only: bool = False):
        B = len(num_nodes)
        gamma_T = self.gamma(torch.ones((B, 1), device=xh.device))
        mu_T = self.alpha(gamma_T, xh)[batch_index] * xh
        sigma_T = self.sigma(gamma_T, xh).reshape(B)
        one = torch.ones_like(sigma_T)
        nx = self.num_x_dims
        kl = self.gaussian_KL(self.sum_node_features_except_batch(mu_T[:, :nx] ** 2, batch_index, B), sigma_T, one, self.subspace_dimensionality(num_nodes))
        if generate_x_only:
            return kl
        mu_h2 = self.sum_node_features_except_batch(mu_T[:, nx:] ** 2 * node_mask.float().unsqueeze(-1), batch_index, B)
        return kl + self.gaussian_KL(mu_h2, sigma_T, one, 1)

    def log_constants_p_x_given_z0(self, num_nodes, device=None):
        B = len(num_nodes)
        gamma_0 = self.gamma(torch.zeros((B, 1), device=self.gamma.gamma.device))
        return self.subspace_dimensionality(num_nodes).to(gamma_0.device) * (-0.5 * gamma_0.view(B) - 0.5 * float(np.log(2 * np.pi)))

    def log_pxh_given_z0_without_constants(self, h, z_0, eps, net_out, gamma_0, batch_index, node_mask, device=None,
                                           generate_x_only: bool = False, epsilon: float = 1e-10):
        nv, nb = cfg_get(self.diffusion_cfg, "norm_values"), cfg_get(self.diffusion_cfg, "norm_biases")
        nx, B = self.num_x_dims, int(gamma_0.shape[0])
        psum = lambda v: self.sum_node_features_except_batch(v, batch_index, B)
        log_px = -0.5 * psum((eps[:, :nx] - net_out[:, :nx]) ** 2)
        if generate_x_only:
            return log_px, None
        m = node_mask.float().unsqueeze(-1)
        sigma_0 = self.sigma(gamma_0[batch_index], target_tensor=z_0)

        def mass(centre, width):             # probability of [centre - 0.5, centre + 0.5] under N(0, width)
            return torch.log(self.cdf_standard_gaussian((centre + 0.5) / width) - self.cdf_standard_gaussian((centre - 0.5) / width) + epsilon)

        z_cat = z_0[:, nx:-1] if self.include_charges else z_0[:, nx:]
        lp = mass(z_cat * nv[1] + nb[1] - 1.0, sigma_0 * nv[1])
        lp = lp - torch.logsumexp(lp, dim=-1, keepdim=True)
        log_ph = psum(lp * (h["categorical"] * nv[1] + nb[1]) * m)
        if self.include_charges:
            h_int = torch.round(h["integer"].reshape(h["integer"].shape[0], -1) * nv[2] + nb[2]).long()
            log_ph = log_ph + psum(mass(h_int - (z_0[:, -1:] * nv[2] + nb[2]), sigma_0 * nv[2]) * m)
        return log_px, log_ph

    # ---- how the objective around the network evaluation runs -------------------------------------------------------------------
    def why_not_fused_objective(self, batch=None) -> Optional[str]:
        """The first reason the fused objective (include/gcdm_objective.h) cannot serve this configuration / batch, or None."""
        if self.diffusion_target != "atom_types_and_coords":
            return f"diffusion_target={self.diffusion_target!r}: only 'atom_types_and_coords' is built"
        if bool(cfg_get(self.diffusion_cfg, "generate_x_only", False)):
            return "generate_x_only: the fused objective scores positions and node features together"
        if self.num_x_dims != 3 or not 1 <= self.num_atom_types <= _native.OBJECTIVE_MAX_TYPES:
            return f"num_x_dims={self.num_x_dims}, num_atom_types={self.num_atom_types}: 3 and 1 .. {_native.OBJECTIVE_MAX_TYPES} are built"
        if batch is not None:
            for name in ("x", "batch", "mask"):
                t = cfg_get(batch, name)
                if isinstance(t, torch.Tensor) and t.device.type != "cuda":
                    return f"a CPU tensor (batch.{name} is on {t.device}): the fused objective runs on an MI355X only"
        return None

    def set_objective_path(self, path: str) -> None:
        """"operators" (default) | "fused": how everything in ``forward`` outside ``dynamics_network(...)`` runs.  "fused" = the noising and
        the per-molecule terms that need no network in one launch, the loss terms and their reduction as one autograd node whose backward is
        one launch (ops.diffusion_objective, include/gcdm_objective.h); raises NotImplementedError naming the first reason when the
        configuration is outside what the kernels implement.  The raw draws stay torch's, in the operator path's order."""
        if path not in ("operators", "fused"):
            raise ValueError(f"objective path must be 'operators' or 'fused', got {path!r}")
        if path == "fused":
            why = self.why_not_fused_objective()
            if why is not None:
                raise NotImplementedError(f"objective path 'fused': the fused objective does not implement this configuration ({why})")
        self._objective_path = path

    @property
    def objective_path(self) -> str:
        return self._objective_path

    def read_objective_flags(self) -> int:
        """The device flag word of the fused objective since the last read (one host sync; call it when convenient, e.g. once per logging
        interval).  Raises what the operator path raises on the spot: ValueError for an unsorted batch index, KeyError for a molecule size
        the histogram does not have."""
        if self._objective_flags is None:
            return 0
        st = ops.ObjectiveState()
        st.flags, st.T = self._objective_flags, self.T
        return st.read_flags()

    def _log_pn_table(self, dev) -> torch.Tensor:
        """log p(N) indexed by molecule size on the device, NaN where the histogram has no entry; rebuilt when the buffer changes."""
        nd = self.num_nodes_distribution
        key = (str(dev), nd.prob.data_ptr(), _native.tensor_version(nd.prob))
        if self._log_pn_cache is None or self._log_pn_cache[0] != key:
            tab = torch.full((max(nd.keys) + 2,), float("nan"), dtype=torch.float32, device=dev)
            tab[nd.num_nodes.to(dev)] = torch.log(nd.prob + nd.eps).to(dev, torch.float32)
            self._log_pn_cache = (key, tab)
        return self._log_pn_cache[1]

    @staticmethod
    def _sc_draw(noise, k, dev):
        """Entry k of a three-entry training ``noise`` list (the two draws of the self-conditioning estimate), or None: torch.randn draws it."""
        return noise[k].to(dev) if noise is not None and len(noise) > k else None

    def _fused_loss_terms(self, batch, return_loss_info, t_int, noise, self_conditioning_prob, fix_self_conditioning_noise,
                          center_x: bool = False, norm_by_max_nodes: bool = False):
        """``_loss_terms`` on the fused objective: same draws in the same order, same tuple.  ``self.last_objective`` keeps (nll, loss, means)
        for the module that assembles the NLL (``center_x`` / ``norm_by_max_nodes`` are its two switches)."""
        training = self.training
        l2 = training and cfg_get(self.diffusion_cfg, "loss_type", "l2") == "l2"
        mode = _native.OBJECTIVE_EVAL if not training else (_native.OBJECTIVE_TRAIN_L2 if l2 else _native.OBJECTIVE_TRAIN_VLB)
        bi, mask, x = batch.batch, batch.mask, batch.x
        dev, N = x.device, int(x.shape[0])
        ng = cfg_get(batch, "num_graphs")
        B = int(bi.max().item()) + 1 if ng is None else int(ng)
        if t_int is None:
            t_int = torch.randint(0 if training else 1, self.T + 1, size=(B, 1), device=dev)
        t_int = t_int.to(dev).reshape(B, 1)
        F_ = self.num_node_scalar_features

        def raw(k):
            if noise is not None:
                return noise[k].to(dev)
            return torch.cat([torch.randn((N, self.num_x_dims), device=dev), torch.randn((N, F_), device=dev)], dim=-1)

        eps_raw = raw(0)
        eps_raw_0 = None if training else raw(1)
        if self._objective_flags is None or self._objective_flags.device != dev:
            self._objective_flags = torch.zeros(1, dtype=torch.int32, device=dev)
        nv, nb = cfg_get(self.diffusion_cfg, "norm_values"), cfg_get(self.diffusion_cfg, "norm_biases")
        st = ops.objective_prepare(x, batch.h["categorical"], batch.h["integer"] if self.include_charges else None, mask, bi, B, t_int,
                                   self.gamma.gamma, self._log_pn_table(dev), [float(v) for v in nv], [0.0 if v is None else float(v) for v in nb],
                                   eps_raw, eps_raw_0, self.num_atom_types, self.include_charges, self.T, mode, self._objective_flags,
                                   center_x=center_x)
        t_node = st.t_node.view(N, 1)
        net_out_0 = None
        if training:
            self_cond = None
            if bool(cfg_get(self.diffusion_cfg, "self_condition", False)) and not bool((t_int == self.T).any()) and _random() < self_conditioning_prob:
                with torch.no_grad():                       # the estimate: gradients off, so the network runs on the sampler's fused kernels
                    t_sc = (t_int + 1) / self.T
                    z_sc, _ = self.compute_noised_representation(st.xh, bi, mask, inflate_batch_array(self.gamma(t_sc), x), eps=self._sc_draw(noise, 1, dev))
                    self_cond = self.sample_p_zs_given_zt(s=torch.zeros_like(t_sc), t=t_sc, z=z_sc, batch_index=bi, node_mask=mask,
                                                          context=getattr(batch, "props_context", None), fix_noise=fix_self_conditioning_noise,
                                                          self_condition=True, noise=self._sc_draw(noise, 2, dev)).detach()
            _, net_out = self.dynamics_network(batch, st.z_t, t_node, xh_self_cond=self_cond)
        else:
            t_zeros = torch.zeros((N, 1), dtype=torch.float32, device=dev)

            def two_evaluations():
                a = self.dynamics_network(batch, st.z_t, t_node, xh_self_cond=None, **self._deferred())[1]
                b = self.dynamics_network(batch, st.z_0, t_zeros, xh_self_cond=None, **self._deferred())[1]
                self._final_range_check()
                return a, b
            net_out, net_out_0 = self._rerun_in_fp32(two_evaluations, "the network evaluations")
        terms, nll, loss, means = ops.diffusion_objective(net_out, st, net_out_0, norm_by_max_nodes=norm_by_max_nodes)
        self.last_objective = (nll, loss, means)
        out = tuple(terms[k] for k in ops.OBJECTIVE_TERMS[:8]) + (t_int.squeeze(-1),)
        if not return_loss_info:
            return out
        return (*out, {"eps_hat_x": means["eps_hat_x"], "eps_hat_h": means["eps_hat_h"]})

    def forward(self, batch, return_loss_info: bool = False, t_int: Optional[torch.Tensor] = None, noise: Optional[List[torch.Tensor]] = None,
                self_conditioning_prob: float = 0.5, fix_self_conditioning_noise: bool = False, _objective: Optional[Dict[str, Any]] = None):
        """Loss / NLL terms of a data batch (:948-1160): (delta_log_px, error_t, SNR_weight, loss_0_x, loss_0_h, neg_log_constants, kl_prior,
        log_pN, t_int[, loss_info]), each per molecule.  ``batch``: x (CoM-free), h = {categorical, integer}, batch, mask, num_graphs,
        num_nodes_present, props_context (per node or None).
          * evaluation mode: two evaluations of the network (t and 0) on the fused kernels, under inference mode;
          * TRAINING mode (``.train()``): one evaluation at t >= 0 on the module path (HIP operators with autograd), the t = 0 terms masked
            in as the reference does (:1078-1101); ``loss_type == "l2"`` drops the weights / constants (:978, 1050-1063).
        Extensions for reproducible runs: ``t_int`` [B, 1] instead of the torch.randint draw, ``noise`` = the raw standard-normal draws
        [N, 3 + F] (evaluation: two, for z_t and z_0; training: one, or three with self-conditioning -- ``noise[1]`` noises the z the
        estimate's jump starts from, ``noise[2]`` is the jump's own draw, masked and CoM-projected by sample_p_zs_given_zt; with one entry the
        two come from torch.randn as without the argument)."""
        if self.diffusion_target != "atom_types_and_coords":
            raise NotImplementedError(f"diffusion_target {self.diffusion_target!r}")
        fn = self._loss_terms
        if self._objective_path == "fused":
            why = self.why_not_fused_objective(batch)
            if why is not None:
                raise NotImplementedError(f"objective path 'fused': {why}")
            fn = lambda *a: self._fused_loss_terms(*a, **(_objective or {}))          # noqa: E731
        if self.training:
            return fn(batch, return_loss_info, t_int, noise, self_conditioning_prob, fix_self_conditioning_noise)
        with torch.inference_mode():
            return fn(batch, return_loss_info, t_int, noise, self_conditioning_prob, fix_self_conditioning_noise)

    def _loss_terms(self, batch, return_loss_info, t_int, noise, self_conditioning_prob, fix_self_conditioning_noise):
        training = self.training
        l2 = training and cfg_get(self.diffusion_cfg, "loss_type", "l2") == "l2"
        x, h = self.normalize(batch.x, batch.h, node_mask=batch.mask)
        bi, B, num_nodes, mask = batch.batch, int(batch.num_graphs), batch.num_nodes_present, batch.mask
        dev = x.device
        if t_int is None:
            t_int = torch.randint(0 if training else 1, self.T + 1, size=(B, 1), device=dev)     # lowest_t (:982-990)
        t_int = t_int.to(dev).reshape(B, 1)
        t_is_zero = (t_int == 0).float().squeeze(-1)
        s, t = (t_int - 1) / self.T, t_int / self.T
        gamma_s, gamma_t = inflate_batch_array(self.gamma(s), x), inflate_batch_array(self.gamma(t), x)
        xh = torch.cat([x, h["categorical"]] + ([h["integer"].reshape(-1, 1)] if self.include_charges else []), dim=-1)
        z_t, eps_t = self.compute_noised_representation(xh, bi, mask, gamma_t, eps=None if noise is None else noise[0].to(dev))
        num_nodes = num_nodes.to(dev)
        delta_log_px = self.delta_log_px(num_nodes)
        neg_log_constants = -self.log_constants_p_x_given_z0(num_nodes, dev)
        kl_prior = self.compute_kl_prior(xh, batch_index=bi, node_mask=mask, num_nodes=num_nodes, device=dev)
        if training:
            self_cond = None
            if bool(cfg_get(self.diffusion_cfg, "self_condition", False)) and not bool((t_int == self.T).any()) and _random() < self_conditioning_prob:
                with torch.no_grad():                       # the estimate the network is conditioned on: a jump from t + 1 to 0 (:1016-1035)
                    t_sc = (t_int + 1) / self.T
                    z_sc, _ = self.compute_noised_representation(xh, bi, mask, inflate_batch_array(self.gamma(t_sc), x), eps=self._sc_draw(noise, 1, dev))
                    self_cond = self.sample_p_zs_given_zt(s=torch.zeros_like(t_sc), t=t_sc, z=z_sc, batch_index=bi, node_mask=mask,
                                                          context=getattr(batch, "props_context", None), fix_noise=fix_self_conditioning_noise,
                                                          self_condition=True, noise=self._sc_draw(noise, 2, dev)).detach()
            _, net_out = self.dynamics_network(batch, z_t, t[bi], xh_self_cond=self_cond)
            error_t = self.sum_node_features_except_batch((eps_t - net_out) ** 2, bi, B)
            if l2:
                delta_log_px, neg_log_constants = torch.zeros_like(delta_log_px), torch.zeros_like(neg_log_constants)
                SNR_weight = torch.ones_like(error_t)
            else:
                SNR_weight = (self.SNR(gamma_s - gamma_t) - 1).squeeze(-1)
            log_px, log_ph = self.log_pxh_given_z0_without_constants(h=h, z_0=z_t, eps=eps_t, net_out=net_out, gamma_0=gamma_t, batch_index=bi,
                                                                     node_mask=mask, device=dev)
            loss_0_x, loss_0_h = -log_px * t_is_zero, -log_ph * t_is_zero
            error_t = error_t * (1 - t_is_zero)
        else:
            # L_0 from its own draw at t = 0 (second evaluation of the network, :1107-1128)
            t_zeros = torch.zeros_like(s)
            gamma_0 = inflate_batch_array(self.gamma(t_zeros), x)
            z_0, eps_0 = self.compute_noised_representation(xh, bi, mask, gamma_0, eps=None if noise is None else noise[1].to(dev))

            def two_evaluations():          # no host sync between them; ONE check of the range guard after both (one sync per batch)
                a = self.dynamics_network(batch, z_t, t[bi], xh_self_cond=None, **self._deferred())[1]
                b = self.dynamics_network(batch, z_0, t_zeros[bi], xh_self_cond=None, **self._deferred())[1]
                self._final_range_check()
                return a, b
            net_out, net_out_0 = self._rerun_in_fp32(two_evaluations, "the network evaluations")
            error_t = self.sum_node_features_except_batch((eps_t - net_out) ** 2, bi, B)
            SNR_weight = (self.SNR(gamma_s - gamma_t) - 1).squeeze(-1)
            log_px, log_ph = self.log_pxh_given_z0_without_constants(h=h, z_0=z_0, eps=eps_0, net_out=net_out_0, gamma_0=gamma_0, batch_index=bi,
                                                                     node_mask=mask, device=dev)
            loss_0_x, loss_0_h = -log_px, -log_ph
        terms = (delta_log_px, error_t, SNR_weight, loss_0_x, loss_0_h, neg_log_constants, kl_prior, self.log_pN(num_nodes), t_int.squeeze(-1))
        if not return_loss_info:
            return terms
        cnt = torch.zeros(B, dtype=x.dtype, device=dev).index_add_(0, bi, torch.ones_like(bi, dtype=x.dtype)).clamp(min=1)
        gmean = lambda v: (torch.zeros(B, dtype=x.dtype, device=dev).index_add_(0, bi, v) / cnt).mean()
        no = net_out.detach()
        info = {"eps_hat_x": gmean(no[:, : self.num_x_dims].abs().mean(-1)), "eps_hat_h": gmean(no[:, self.num_x_dims:].abs().mean(-1))}
        return (*terms, info)

    # ---- one step with the reference's signature (:1204-1278) --------------------------------------
    @torch.inference_mode()
    def sample_p_zs_given_zt(self, s, t, z, batch_index, node_mask, batch=None, context=None, fix_noise: bool = False,
                             generate_x_only: bool = False, self_condition: bool = False, xh_self_cond=None,
                             noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None):
        gamma_s, gamma_t = self.gamma(s), self.gamma(t)
        sigma2_t_given_s, sigma_t_given_s, alpha_t_given_s = self.sigma_and_alpha_t_given_s(gamma_t, gamma_s, z)
        sigma_s = self.sigma(gamma_s, target_tensor=z)
        sigma_t = self.sigma(gamma_t, target_tensor=z)
        if batch is None:
            batch = _Batch(batch=batch_index, mask=node_mask, props_context=context)
        # deferred range guard: the reference's loop calls this T times; call k looks at the flag word of call k-1 (no host sync), and
        # sample_p_xh_given_z0 -- the call that ends every one of the reference's loops -- checks the last one before it returns samples
        _, eps_t = self.dynamics_network(batch, z, t[batch_index], x_self_cond=xh_self_cond, xh_self_cond=xh_self_cond, **self._deferred())
        mu = z / alpha_t_given_s[batch_index] - (sigma2_t_given_s[batch_index] / alpha_t_given_s[batch_index] / sigma_t[batch_index]) * eps_t
        sigma = sigma_t_given_s * sigma_s / sigma_t
        if noise is not None:  # raw standard-normal draws [N,3+F] (x-part gets CoM-projected like the reference's sampler)
            B = int(s.shape[0])
            nx = _segment_mean_sub(noise[:, : self.num_x_dims] * node_mask.float().unsqueeze(-1), batch_index, B, node_mask)
            noise = torch.cat([nx, noise[:, self.num_x_dims:] * node_mask.float().unsqueeze(-1)], dim=-1)
        zs = self.sample_normal(mu, sigma, batch_index, node_mask, fix_noise=fix_noise, generate_x_only=generate_x_only, eps=noise, generator=generator)
        zs_x = _segment_mean_sub(zs[:, : self.num_x_dims], batch_index, int(s.shape[0]), node_mask)
        return zs_x if generate_x_only else torch.cat([zs_x, zs[:, self.num_x_dims:]], dim=-1)

    def unnormalize(self, x, node_mask, h_cat=None, h_int=None, generate_x_only: bool = False):
        """(:735-759)"""
        nv, nb = cfg_get(self.diffusion_cfg, "norm_values"), cfg_get(self.diffusion_cfg, "norm_biases")
        x = x * nv[0]
        if generate_x_only:
            return x, None, None
        m = node_mask.float().unsqueeze(-1)
        h_cat = (h_cat * nv[1] + nb[1]) * m
        h_int = h_int * nv[2] + nb[2]
        if self.include_charges:
            h_int = h_int * m
        return x, h_cat, h_int

    @torch.inference_mode()
    def sample_p_xh_given_z0(self, z_0, batch_index, node_mask, batch_size: int, batch=None, context=None, fix_noise: bool = False,
                             generate_x_only: bool = False, xh_self_cond=None, noise: Optional[torch.Tensor] = None,
                             generator: Optional[torch.Generator] = None):
        """x, h ~ p(x, h | z0) with the reference's signature (:839-907): the call that ends each of the reference's sampling loops.  One
        network evaluation at t = 0 plus O(N) torch algebra; extension: ``noise`` = the raw standard-normal draw [N, 3 + F].  Before the
        samples are returned the deferred range guard of this evaluation AND of the sample_p_zs_given_zt calls in front of it is checked
        (one host sync); F16RangeError means the trajectory has to be re-run (the handle has been switched to fp32 MFMA)."""
        t_zeros = torch.zeros(size=(batch_size, 1), device=batch_index.device)
        gamma_0 = self.gamma(t_zeros)
        sigma_x = self.SNR(-0.5 * gamma_0)
        if batch is None:
            batch = _Batch(batch=batch_index, mask=node_mask, props_context=context)
        _, net_out = self.dynamics_network(batch, z_0, t_zeros[batch_index], x_self_cond=xh_self_cond, xh_self_cond=xh_self_cond, **self._deferred())
        mu_x = self.compute_x_pred(z_0, net_out, gamma_0, batch_index)
        if noise is not None:
            m = node_mask.float().unsqueeze(-1)
            noise = torch.cat([_segment_mean_sub(noise[:, : self.num_x_dims] * m, batch_index, batch_size, node_mask), noise[:, self.num_x_dims:] * m], dim=-1)
        xh = self.sample_normal(mu=mu_x, sigma=sigma_x, batch_index=batch_index, node_mask=node_mask, fix_noise=fix_noise, generate_x_only=generate_x_only, eps=noise,
                                generator=generator)
        x = xh[:, : self.num_x_dims]
        if generate_x_only:              # positions only (:894-897): no node features to decode
            x, _, _ = self.unnormalize(x, node_mask, generate_x_only=True)
            self._final_range_check()
            return x, {}
        h_cat = xh[:, self.num_x_dims:-1] if self.include_charges else xh[:, self.num_x_dims:]
        h_int = xh[:, -1:] if self.include_charges else torch.zeros(0, device=x.device)
        x, h_cat, h_int = self.unnormalize(x, node_mask, h_cat=h_cat, h_int=h_int)
        h_cat = F.one_hot(torch.argmax(h_cat, dim=-1), self.num_atom_types) * node_mask.long().unsqueeze(-1)
        h_int = torch.round(h_int).long() * node_mask.long().unsqueeze(-1)
        self._final_range_check()
        return x, {"integer": h_int, "categorical": h_cat}

    def _deferred(self) -> Dict[str, Any]:
        """Keyword that selects the deferred range guard for one module-level call -- only for this package's GCPNetDynamics (a foreign
        dynamics network gets no extra keyword)."""
        return {"_range_check": "deferred"} if hasattr(self.dynamics_network, "check_deferred_flags") else {}

    def _final_range_check(self) -> None:
        """Deferred range guard of the module-level calls (GCPNetDynamics.check_f16_range): the flag word of the LAST network evaluation is
        looked at here, with one host sync, before a driver hands results to its caller.  Raises F16RangeError (handle switched to fp32)."""
        chk = getattr(self.dynamics_network, "check_deferred_flags", None)
        if chk is not None:
            chk(wait=True)

    def _rerun_in_fp32(self, fn: Callable[[], Any], what: str) -> Any:
        """``fn()``; on F16RangeError (an activation left the f16 range of the split-precision kernels) ``fn()`` once more with fp32 MFMA --
        ``fn`` must draw the same noise again -- after which the handle returns to its default mode and ``last_flags`` reports FLAG_F16_RANGE."""
        try:
            return fn()
        except F16RangeError:
            log.warning("An activation left the f16 range of the split-precision kernels; re-running %s with fp32 MFMA.", what)
        with self.dynamics_network.fp32_mfma():
            out = fn()
        self.last_flags |= _native.FLAG_F16_RANGE
        return out

    def _report_flags(self, fl: int, where: str, guard: Optional[_RangeCheckpoints] = None) -> int:
        """The final device flag word of a fused sampling run -> ``last_flags`` / ``last_range_rewinds`` / ``last_range_resume_step``, warnings
        and errors.  A run whose guard fell back to fp32 MFMA reports FLAG_F16_RANGE."""
        if fl & _native.FLAG_F16_RANGE:
            raise RuntimeError("f16 range flag raised in fp32 mode (internal error)")
        fell_back = guard is not None and guard.fell_back
        if fell_back:
            fl |= _native.FLAG_F16_RANGE
        self.last_range_rewinds = 0 if guard is None else guard.rewinds
        self.last_range_resume_step = guard.resume_step if fell_back else None
        if fl & _native.FLAG_TAIL or (guard is not None and guard.tail_flag):
            self.dynamics_network.disable_fused_layer(where)      # (the affected interval was repeated with two launches per layer by the range rewind)
        if fl & _native.FLAG_MEAN_NOT_ZERO:
            raise AssertionError("Mean is not zero: the supplied samples are not centred (assert_mean_zero_with_mask, relative error >= 1e-2)")
        if fl & _native.FLAG_NAN_VEL:
            log.warning("Detected NaN in `vel` -> GCPNet `vel` output was reset to zero for at least one time step.")
        if fl & _native.FLAG_COG_DRIFT:
            log.warning("CoG drift above 5e-2. Projected the positions down.")
        self.last_flags = fl
        return fl

    # ---- production loop (:1282-1412) ---------------------------------------------------------------
    def _native(self, device):
        dyn = self.dynamics_network
        if not hasattr(dyn, "_ensure_handle"):
            raise RuntimeError("mol_gen_sample needs the bio-diffusion_amd GCPNetDynamics (HIP) as dynamics_network")
        dyn._ensure_handle(torch.device(device))
        dyn.sync_weights()
        lib, h = dyn._lib, dyn._handle
        if self._gamma_uploaded is not h:
            fused_sampler.upload_gamma(self, lib, h)
            self._gamma_uploaded = h
        return dyn, lib, h

    def _mol_gen_sample_modules(self, num_samples, num_nodes, device, return_frames, num_timesteps, node_mask, context, fix_noise,
                                fix_self_conditioning_noise, norm_with_original_timesteps, noise_fn, step_callback, generate_x_only, seed, init_xh):
        """mol_gen_sample (:1282-1412) step by step through the reference-signature methods of this class -- torch algebra on the device around
        one network evaluation per step on whichever HIP path the configuration / mask selects.  Serves masked nodes inside the loop and the
        configurations the fused sampling kernels are not built for; ~10x slower per step than the fused loop.  ``noise_fn(k)``: raw draw k;
        without it the draws come from a device torch.Generator seeded with ``seed`` (reproducible per seed, in the reference's randn order,
        so that a re-run after F16RangeError draws the same noise)."""
        num_timesteps = self.T if num_timesteps is None else num_timesteps
        _check_frames(return_frames, num_timesteps)
        num_nodes = torch.as_tensor(num_nodes)
        bi = num_nodes_to_batch_index(num_samples, num_nodes.to(device), device=device)
        node_mask = torch.ones_like(bi).bool() if node_mask is None else node_mask.to(device)
        if context is not None:
            context = context.to(device)[bi] * node_mask.float().unsqueeze(-1)
        t_norm = self.T if norm_with_original_timesteps else num_timesteps
        gen, draw = _module_draws(noise_fn, seed, device)
        m = node_mask.float().unsqueeze(-1)
        raw = draw() if init_xh is None else None
        if init_xh is not None:
            # optimisation loop (mol_gen_optimize :1451-1464): z = normalize(samples), no initial draw; the reference's assert_mean_zero_with_mask
            xin = init_xh.to(device, torch.float32)
            nv, nb = cfg_get(self.diffusion_cfg, "norm_values"), cfg_get(self.diffusion_cfg, "norm_biases")
            z = torch.cat((xin[:, : self.num_x_dims] / nv[0], (xin[:, self.num_x_dims:] - nb[1]) / nv[1] * m), dim=-1)
            self.assert_mean_zero_with_mask(z[:, : self.num_x_dims], node_mask)
        elif raw is None:
            z = self.sample_combined_position_feature_noise(torch.zeros_like(bi) if fix_noise else bi, node_mask, generate_x_only=generate_x_only,
                                                            generator=gen, num_graphs=1 if fix_noise else num_samples)
        else:
            z = torch.cat((_segment_mean_sub(raw[:, : self.num_x_dims] * m, bi, num_samples, node_mask), raw[:, self.num_x_dims:] * m), dim=-1)
        self_cond_on = bool(cfg_get(self.diffusion_cfg, "self_condition", False))
        self_cond = None
        out = torch.zeros((return_frames,) + tuple(z.shape), device=device)
        for s in reversed(range(num_timesteps)):
            s_arr = torch.full((num_samples, 1), s / t_norm, device=device)
            t_arr = torch.full((num_samples, 1), (s + 1) / t_norm, device=device)
            z = self.sample_p_zs_given_zt(s=s_arr, t=t_arr, z=z, batch_index=bi, node_mask=node_mask, context=context, fix_noise=fix_noise,
                                          generate_x_only=generate_x_only, xh_self_cond=self_cond, noise=draw(), generator=gen)
            if step_callback is not None:
                step_callback(s, z)
            if (s * return_frames) % num_timesteps == 0:
                out[(s * return_frames) // num_timesteps] = self.unnormalize_z(z, node_mask, generate_x_only=generate_x_only)
            if self_cond_on:
                self_cond = self.sample_p_zs_given_zt(s=torch.zeros_like(s_arr), t=s_arr, z=z, batch_index=bi, node_mask=node_mask, context=context,
                                                      fix_noise=fix_self_conditioning_noise, self_condition=True, noise=draw(), generator=gen)
        x, h = self.sample_p_xh_given_z0(z_0=z, batch_index=bi, node_mask=node_mask, batch_size=num_samples, context=context,
                                         fix_noise=fix_self_conditioning_noise if self_cond_on else fix_noise, generate_x_only=generate_x_only,
                                         xh_self_cond=self_cond, noise=draw(), generator=gen)
        out[0] = self._decoded_frame(x, h, bi, num_samples, node_mask, return_frames, generate_x_only)
        self.last_flags = 0
        return out.squeeze(0), bi, node_mask

    def _decoded_frame(self, x, h, bi, num_graphs, node_mask, return_frames, generate_x_only):
        """Frame 0 of a module-path loop from the decode's (x, h): the positions re-centred where the centres of gravity drifted (runs without
        intermediate frames only, :1389-1402), then [x, one-hot, charges]."""
        if return_frames == 1:
            cog = torch.zeros(num_graphs, self.num_x_dims, device=x.device).index_add_(0, bi, x).abs().max().item()
            if cog > 5e-2:
                x = _segment_mean_sub(x, bi, num_graphs, node_mask)
        if generate_x_only:
            return x
        return torch.cat([x, h["categorical"].to(x.dtype)] + ([h["integer"].to(x.dtype)] if self.include_charges else []), dim=-1)

    def unnormalize_z(self, z, node_mask, generate_x_only: bool = False):
        """(:761-793)"""
        nx, nt = self.num_x_dims, self.num_atom_types
        if generate_x_only:
            return self.unnormalize(z[:, :nx], node_mask, generate_x_only=True)[0]
        x, h_cat, h_int = self.unnormalize(z[:, :nx], node_mask, h_cat=z[:, nx:nx + nt], h_int=z[:, nx + nt:])
        return torch.cat([x, h_cat] + ([h_int] if self.include_charges else []), dim=-1)

    @torch.inference_mode()
    def mol_gen_sample(self, num_samples: int, num_nodes: torch.Tensor, device: Union[torch.device, str], return_frames: int = 1,
                       num_timesteps: Optional[int] = None, node_mask: Optional[torch.Tensor] = None,
                       context: Optional[torch.Tensor] = None, fix_noise: bool = False, generate_x_only: bool = False,
                       fix_self_conditioning_noise: bool = False, norm_with_original_timesteps: bool = False,
                       noise_fn: Optional[Callable[[int], torch.Tensor]] = None, seed: int = 1234,
                       step_callback: Optional[Callable[[int, torch.Tensor], None]] = None,
                       _init_xh: Optional[torch.Tensor] = None, _t_norm: Optional[int] = None, lanes: int = 1
                       ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Draw samples.  ``noise_fn(k)`` (optional) returns the k-th raw standard-normal draw [N,3+F] on ``device``
        (k = 0 for z_T, then one per step, then one for the final decode: the reference's randn call order,
        SURVEY A.5); without it noise comes from on-device Philox(seed)."""
        self._check_x_only_network(generate_x_only)
        if lanes > 1:
            self.refuse_fused_sampler_only("mol_gen_sample(lanes > 1)")
        if self._off_fused_kernels(generate_x_only, node_mask):
            # general loop: position-only diffusion, masked nodes inside the loop, or a configuration the fused sampling kernels are not built for
            if _t_norm is not None:
                raise NotImplementedError("an explicit time normalisation runs on the fused path only")
            return self._rerun_in_fp32(lambda: self._mol_gen_sample_modules(num_samples, num_nodes, torch.device(device), return_frames, num_timesteps,
                                                                            node_mask, context, fix_noise, fix_self_conditioning_noise,
                                                                            norm_with_original_timesteps, noise_fn, step_callback, generate_x_only, seed,
                                                                            _init_xh),
                                       "the sampling loop")
        self_cond_on = bool(getattr(self.dynamics_network, "self_condition", False))
        if fix_noise or self_cond_on:
            lanes = 1                  # fix_noise: the noise is centred over the whole flat batch; self-conditioning: not sliced (yet)
        if self_cond_on and fix_self_conditioning_noise != fix_noise:
            raise NotImplementedError("fix_self_conditioning_noise must equal fix_noise")
        num_timesteps = self.T if num_timesteps is None else num_timesteps
        _check_frames(return_frames, num_timesteps)
        # time normalisation of the loop (:1333-1341): s / T_norm with T_norm = self.T if norm_with_original_timesteps else num_timesteps
        t_norm = _t_norm if _t_norm is not None else (self.T if norm_with_original_timesteps else num_timesteps)
        if num_timesteps > t_norm:
            raise ValueError("num_timesteps exceeds the normalising number of timesteps")
        if lanes > 1 and len(num_nodes) >= 2 * lanes and not (
                noise_fn is not None or return_frames != 1 or _init_xh is not None or step_callback is not None):
            # slices of the flat batch on several handles / streams: plain sampling with on-device noise; anything else runs on one handle
            return fused_sampler.sample_lanes(self, num_nodes, torch.device(device), num_timesteps, t_norm, context, seed, lanes)
        assert len(num_nodes) == num_samples
        return fused_sampler.sample(self, num_nodes, torch.device(device), return_frames, num_timesteps, t_norm, context, fix_noise, noise_fn, seed,
                                    step_callback, _init_xh)

    def _check_x_only_network(self, generate_x_only: bool) -> None:
        """Position-only diffusion (:1292, 1325-1327, 1349, 1385, 1407-1408: z = z_x, centred x-noise alone, [N, 3] out) needs a dynamics network
        built WITHOUT node features (dataloader_cfg.num_atom_types = 0, include_charges = False: xh is [N, 3] then, as in the reference)."""
        if generate_x_only and getattr(self.dynamics_network, "num_atom_types", 0) + int(getattr(self.dynamics_network, "include_charges", False)) > 0:
            raise ValueError("generate_x_only needs a dynamics network built without node features (num_atom_types = 0, include_charges = False); "
                             "the reference fails on the feature width of this one too (gcpnet.py:1093-1110)")

    def runs_generic_loop_only(self) -> bool:
        """Is the dynamics network one the fused sampling kernels are not written for at all (the EGNN dynamics network), so that every
        sampling entry point runs the generic loop?"""
        return getattr(self.dynamics_network, "fused_unsupported", None) == "egnn"

    def refuse_fused_sampler_only(self, what: str) -> None:
        """``what`` exists on the fused sampler alone (lane handles, packed plans): refused by name for the EGNN dynamics network, before
        any GPU work."""
        if self.runs_generic_loop_only():
            raise NotImplementedError(f"{what}: the EGNN dynamics network (dynamics_network=egnn) samples through the generic loop; lanes, "
                                      "concurrent batches and packed plans are drivers of GCPNet's fused sampling kernels")

    def _off_fused_kernels(self, generate_x_only: bool, node_mask: Optional[torch.Tensor] = None) -> bool:
        """Does this call run the general loop on the module path (position-only diffusion, masked nodes inside the loop, a configuration the
        fused sampling kernels are not built for, ``dynamics_network.path = "modules"``) instead of the fused kernels?"""
        return bool(generate_x_only or (node_mask is not None and not bool(node_mask.all()))
                    or getattr(self.dynamics_network, "fused_unsupported", None) is not None or getattr(self.dynamics_network, "path", "auto") == "modules")

    @torch.inference_mode()
    def inpaint(self, molecule: Dict[str, Any], node_mask_fixed: torch.Tensor, num_resamplings: int = 1, jump_length: int = 1,
                return_frames: int = 1, num_timesteps: Optional[int] = None, context: Optional[torch.Tensor] = None,
                generate_x_only: bool = False, noise_fn: Optional[Callable[[int], torch.Tensor]] = None, seed: int = 1234) -> torch.Tensor:
        """Draw samples while keeping parts of the given molecules fixed (RePaint; variational_diffusion.py:1582-1789).
        ``molecule``: dict with "x" [N,3], "one_hot" [N,F], "charges" [N,1] (if the model has charges), "num_nodes" [B] (and optionally
        "batch_index", which must be the contiguous one); ``node_mask_fixed`` [N] bool.  Returns [N,3+F], or [return_frames,N,3+F].
        The reference method raises on every call (:1650, :1177); this is that method with the two tokens repaired (include/gcdm_hip.h,
        DESIGN.md 7), pinned by tests/golden/inpaint_small_qm9.npz.  ``noise_fn(k)``: the k-th raw draw in the reference's order -- z_T, then
        per step [known part, model step, self-conditioning estimate if any], one per jump back, and the final decode."""
        num_timesteps = self.T if num_timesteps is None else num_timesteps
        _check_frames(return_frames, num_timesteps)
        assert jump_length == 1 or return_frames == 1, "Chain visualization is only implemented for `jump_length=1`"
        if self._off_fused_kernels(generate_x_only):
            # position-only diffusion (a dynamics network without node features) and configurations off the fused kernels: the general loop
            return self._rerun_in_fp32(lambda: self._inpaint_modules(molecule, node_mask_fixed, num_resamplings, jump_length, return_frames,
                                                                     num_timesteps, context, generate_x_only, noise_fn, seed),
                                       "the inpainting loop")
        schedule = repaint_schedule(num_resamplings, jump_length, num_timesteps)
        return self._rerun_in_fp32(lambda: fused_sampler.inpaint_once(self, molecule, node_mask_fixed, schedule, jump_length, return_frames,
                                                                      num_timesteps, context, noise_fn, seed),
                                   "the inpainting")

    def sample_p_zt_given_zs(self, zs, batch_index, node_mask, gamma_t, gamma_s, generate_x_only: bool = False, noise: Optional[torch.Tensor] = None,
                             generator: Optional[torch.Generator] = None):
        """The forward jump z_s -> z_t of RePaint (variational_diffusion.py:1163-1201) WITH the reference's crashing token repaired: `:1177` indexes
        a [B, 1] factor with the [N] node mask; every sibling gathers per-molecule factors with `[batch_index]`, and so does this.  ``gamma_*``:
        [B, 1] (the reference inflates them to [B, 1] as well)."""
        _, sigma_t_given_s, alpha_t_given_s = self.sigma_and_alpha_t_given_s(gamma_t, gamma_s, zs)
        B = int(gamma_t.shape[0])
        if noise is None:
            eps = self.sample_combined_position_feature_noise(batch_index, node_mask, generate_x_only=generate_x_only, generator=generator, num_graphs=B)
        else:
            m = node_mask.float().unsqueeze(-1)
            eps = torch.cat([_segment_mean_sub(noise[:, : self.num_x_dims] * m, batch_index, B, node_mask), noise[:, self.num_x_dims:] * m], dim=-1)
        zt = alpha_t_given_s[batch_index] * zs + sigma_t_given_s[batch_index] * eps
        zx = _segment_mean_sub(zt[:, : self.num_x_dims], batch_index, B, node_mask)
        return zx if generate_x_only else torch.cat([zx, zt[:, self.num_x_dims:]], dim=-1)

    def _inpaint_modules(self, molecule, node_mask_fixed, num_resamplings, jump_length, return_frames, num_timesteps, context, generate_x_only,
                              noise_fn, seed):
        """inpaint (:1582-1789, the two repairs of the fused method's docstring) step by step through the reference-signature methods of this class:
        torch algebra on the device around one network evaluation per step.  Serves ``generate_x_only`` (position-only diffusion: the molecule is
        its positions, z = z_x, [N, 3] out -- the dynamics network must be built without node features, as for mol_gen_sample) and configurations
        the fused kernels are not built for.  ``noise_fn(k)``: raw draws in the reference's order; otherwise a device generator seeded with ``seed``
        (so that a re-run after F16RangeError draws the same noise)."""
        device = torch.device(molecule["x"].device)
        nx = self.num_x_dims
        self._check_x_only_network(generate_x_only)
        num_nodes = torch.as_tensor(molecule["num_nodes"])
        B = len(num_nodes)
        bi = num_nodes_to_batch_index(B, num_nodes.to(device), device=device)
        if "batch_index" in molecule and not torch.equal(molecule["batch_index"].to(device), bi):
            raise ValueError("molecule['batch_index'] must be the contiguous index implied by molecule['num_nodes']")
        ones = torch.ones_like(bi).bool()
        fixed = node_mask_fixed.to(device).bool()
        if context is not None:
            context = context.to(device)[bi]
        if generate_x_only:
            xh0 = molecule["x"].to(device, torch.float32).clone()
        else:
            parts = [molecule["x"], molecule["one_hot"]] + ([molecule["charges"]] if self.include_charges else [])
            xh0 = torch.cat([p_.to(device, torch.float32) for p_ in parts], dim=-1)

        def fixed_mean(x):                                   # scatter(x[fixed], batch_index[fixed], reduce="mean"), one row per molecule (0 where none is fixed)
            f = fixed.float().unsqueeze(-1)
            sums = torch.zeros((B, x.shape[1]), device=device).index_add_(0, bi, x * f)
            cnt = torch.zeros(B, device=device).index_add_(0, bi, fixed.float()).clamp(min=1)
            return sums / cnt[:, None]

        xh0[:, :nx] = xh0[:, :nx] - fixed_mean(xh0[:, :nx])[bi]                    # :1625-1633
        gen, draw = _module_draws(noise_fn, seed, device)
        raw = draw()
        if raw is None:
            z = self.sample_combined_position_feature_noise(bi, ones, generate_x_only=generate_x_only, generator=gen, num_graphs=B)
        else:
            z = torch.cat((_segment_mean_sub(raw[:, :nx], bi, B, ones), raw[:, nx:]), dim=-1)
        out = torch.zeros((return_frames,) + tuple(z.shape), device=device)
        schedule = repaint_schedule(num_resamplings, jump_length, num_timesteps)
        self_cond_on = bool(cfg_get(self.diffusion_cfg, "self_condition", False))
        self_cond = None
        s = num_timesteps - 1
        fm = fixed.float().unsqueeze(-1)
        for i, num_denoise_steps in enumerate(schedule):
            for j in range(num_denoise_steps):
                s_arr = torch.full((B, 1), s / num_timesteps, device=device)
                t_arr = torch.full((B, 1), (s + 1) / num_timesteps, device=device)
                gamma_s = self.gamma(s_arr)
                rk = draw()
                if rk is None and gen is not None:
                    rk = torch.randn(xh0.shape, device=device, generator=gen)
                z_known, _ = self.compute_noised_representation(xh0, bi, ones, gamma_s, generate_x_only=generate_x_only, eps=rk)
                z_unknown = self.sample_p_zs_given_zt(s=s_arr, t=t_arr, z=z, batch_index=bi, node_mask=ones, context=context,
                                                      generate_x_only=generate_x_only, xh_self_cond=self_cond, noise=draw(), generator=gen)
                if self_cond_on:
                    self_cond = self.sample_p_zs_given_zt(s=torch.zeros_like(s_arr), t=s_arr, z=z_unknown, batch_index=bi, node_mask=ones, context=context,
                                                          generate_x_only=generate_x_only, self_condition=True, noise=draw(), generator=gen)
                shift = fixed_mean(z_unknown[:, :nx]) - fixed_mean(z_known[:, :nx])       # :1680-1697
                z_known = torch.cat((z_known[:, :nx] + shift[bi], z_known[:, nx:]), dim=-1)
                z = z_known * fm + z_unknown * (1 - fm)
                self.assert_mean_zero_with_mask(z[:, :nx], ones)
                if (num_denoise_steps > jump_length or i == len(schedule) - 1) and (s * return_frames) % num_timesteps == 0:
                    out[(s * return_frames) // num_timesteps] = self.unnormalize_z(z, ones, generate_x_only=generate_x_only)
                if j == num_denoise_steps - 1 and i < len(schedule) - 1:                  # go back `jump_length` steps (:1717-1737)
                    t = s + jump_length
                    gamma_t = self.gamma(torch.full((B, 1), t / num_timesteps, device=device))
                    z = self.sample_p_zt_given_zs(z, bi, ones, gamma_t, gamma_s, generate_x_only=generate_x_only, noise=draw(), generator=gen)
                    s = t
                s -= 1
        x, h = self.sample_p_xh_given_z0(z_0=z, batch_index=bi, node_mask=ones, batch_size=B, context=context, generate_x_only=generate_x_only,
                                         xh_self_cond=self_cond, noise=draw(), generator=gen)
        self.assert_mean_zero_with_mask(x, ones)
        out[0] = self._decoded_frame(x, h, bi, B, ones, return_frames, generate_x_only)
        # the device check word of the network evaluations of this loop (NaN in vel, ...; the range bit was handled by the deferred guard above)
        rf = getattr(self.dynamics_network, "read_flags", None)
        self.last_flags = (int(rf()) & ~_native.FLAG_F16_RANGE) if rf is not None and getattr(self.dynamics_network, "_handle", None) is not None else 0
        return out.squeeze(0)

    # ---- several independent batches in flight (evaluation driver) -------------------------------------------------------------
    _Lane = fused_sampler._Lane
    _SlicedBatch = fused_sampler._SlicedBatch

    @torch.inference_mode()
    def mol_gen_sample_concurrent(self, num_nodes_list: List[torch.Tensor], device: Union[torch.device, str],
                                  num_timesteps: Optional[int] = None, contexts: Optional[List[Optional[torch.Tensor]]] = None,
                                  seeds: Optional[List[int]] = None) -> List[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
        """`mol_gen_sample` for several independent batches at once: batch b runs on its own handle and HIP stream, the step
        launches of all batches are interleaved on the host.  Results are those of `mol_gen_sample(..., seed=seeds[b])` called one
        after the other (bit-identical); small batches (the evaluation driver's 100 molecules) no longer leave CUs idle."""
        return self._sample_batches(False, num_nodes_list, device, num_timesteps, contexts, seeds)

    @torch.inference_mode()
    def mol_gen_sample_packed(self, num_nodes_list: List[torch.Tensor], device: Union[torch.device, str],
                              num_timesteps: Optional[int] = None, contexts: Optional[List[Optional[torch.Tensor]]] = None,
                              seeds: Optional[List[int]] = None) -> List[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
        """`mol_gen_sample_concurrent` without the lane handles: the batches are laid end to end in ONE packed plan (`gcdm_plan_batches`) on the primary
        handle and sampled by one (captured) launch set per step.  Every batch stays a flat batch of its own -- orientation padding at its ends, its own
        noise stream, its own NaN-in-vel and CoG decisions -- so the results are those of `mol_gen_sample(..., seed=seeds[b])` called one after the other
        (bit-identical), at one copy of the weights and one workspace."""
        return self._sample_batches(True, num_nodes_list, device, num_timesteps, contexts, seeds)

    def _sample_batches(self, packed: bool, num_nodes_list, device, num_timesteps, contexts, seeds):
        """The two samplers above behind their defaults.  The packed one checks what needs no device first: one context and one seed per batch, no
        empty batch, no self-conditioned model."""
        self.refuse_fused_sampler_only("mol_gen_sample_packed" if packed else "mol_gen_sample_concurrent")
        K = len(num_nodes_list)
        contexts = contexts if contexts is not None else [None] * K
        seeds = seeds if seeds is not None else [1234 + b for b in range(K)]
        if packed:
            if K == 0:
                raise ValueError("num_nodes_list is empty: at least one batch is needed")
            if len(contexts) != K:
                raise ValueError(f"contexts has {len(contexts)} entries for {K} batches")
            if len(seeds) != K:
                raise ValueError(f"seeds has {len(seeds)} entries for {K} batches")
            for b, nn_ in enumerate(num_nodes_list):
                if len(nn_) == 0:
                    raise ValueError(f"batch {b} is empty: every batch needs at least one molecule")
            if bool(getattr(self.dynamics_network, "self_condition", False)):
                raise NotImplementedError("mol_gen_sample_packed: a self-conditioned model is not served by a packed plan (the self-conditioned step entry "
                                          "points refuse it); use mol_gen_sample per batch")
        return fused_sampler.sample_batches(self, num_nodes_list, torch.device(device), self.T if num_timesteps is None else num_timesteps,
                                            contexts, seeds, packed)

    def release_lanes(self):
        for ln in getattr(self, "_lanes", None) or []:
            ln.close()
        self._lanes = []

    def __del__(self):
        try:
            self.release_lanes()
        except Exception:
            pass

    def get_repaint_schedule(self, resamplings: int, jump_length: int, num_timesteps: int) -> List[int]:
        """variational_diffusion.py:1548-1578."""
        return repaint_schedule(resamplings, jump_length, num_timesteps)

    @torch.inference_mode()
    def mol_gen_optimize(self, samples: List[Tuple[torch.Tensor, torch.Tensor]], num_nodes: torch.Tensor, device: Union[torch.device, str],
                         return_frames: int = 1, num_timesteps: Optional[int] = None, node_mask: Optional[torch.Tensor] = None,
                         context: Optional[torch.Tensor] = None, generate_x_only: bool = False, norm_with_original_timesteps: bool = False,
                         noise_fn: Optional[Callable[[int], torch.Tensor]] = None, seed: int = 1234
                         ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Optimise existing samples with the generative model (variational_diffusion.py:1416-1546): the samples
        ``[(x [n,3], one_hot [n,F]), ...]`` -- or one flat pair ``(x [N,3], one_hot [N,F])`` of all molecules, rows as ``num_nodes`` lays them
        out -- are normalised and taken as z at t = num_timesteps / T_norm, denoised for ``num_timesteps``
        steps and decoded.  As in the reference z carries no charge column (``"integer": torch.tensor([])``, :1457), so the model must
        have ``include_charges=False`` (the property-conditional QM9 models).  ``noise_fn(k)``: k = 0 is the first step's draw.
        ``return_frames > 1``: [frames, N, 3 + F] -- frame (s * return_frames) // T after the step to s, frame 0 the decoded sample (:1490-1497,
        1540-1546).  Configurations off the fused path (and ``dynamics_network.path = "modules"``) run the general loop."""
        if generate_x_only:
            # nothing to mirror: the reference's own call raises -- normalize(..., generate_x_only=True) does `h.float()` on the {"categorical", "integer"}
            # dict mol_gen_optimize hands it (variational_diffusion.py:716 via :1454-1459: AttributeError)
            raise NotImplementedError("mol_gen_optimize: generate_x_only raises in the reference too (variational_diffusion.py:716 via :1454: `h.float()` on a dict)")
        if self.include_charges:
            raise NotImplementedError("mol_gen_optimize builds z without the charge column (reference :1457): include_charges must be False")
        if len(samples) == 2 and all(torch.is_tensor(s) for s in samples):
            # the flat form, what sample() / optimize() return: (x [N,3], one_hot [N,F]) of all molecules, the atoms of a molecule contiguous
            x, h = samples
            if x.shape[0] != h.shape[0] or x.shape[0] != int(torch.as_tensor(num_nodes).sum()):
                raise ValueError(f"flat samples have {x.shape[0]} / {h.shape[0]} rows, num_nodes sums to {int(torch.as_tensor(num_nodes).sum())}")
            xh = torch.cat((x.to(torch.float32), h.to(torch.float32)), dim=-1)
            n_samples = len(num_nodes)
        else:
            if len(samples) != len(num_nodes):
                raise ValueError("one (x, h) pair per molecule")
            xh = torch.cat([torch.cat((x.to(torch.float32), h.to(torch.float32)), dim=-1) for x, h in samples], dim=0)
            n_samples = len(samples)
        return self.mol_gen_sample(num_samples=n_samples, num_nodes=num_nodes, device=device, return_frames=return_frames, num_timesteps=num_timesteps,
                                   node_mask=node_mask, context=context, norm_with_original_timesteps=norm_with_original_timesteps,
                                   noise_fn=noise_fn, seed=seed, _init_xh=xh)
