"""Drivers of the fused sampling entry points (``gcdm_sample_init`` / ``gcdm_sample_step*`` / ``gcdm_sample_final*`` and the inpainting calls).

``_FusedRun`` is one flat batch, or one packed plan, on one handle and one stream: the batch index, the per-node context, the latent, the frames,
the flag word(s), the draw counter and the entry points as methods.  The drivers are written on it: ``sample`` (mol_gen_sample), ``inpaint_once``
and ``sample_batches`` (K runs on lane handles, or one packed run with K flag words); ``_SlicedBatch`` (one flat batch as K slices with a
double-buffered latent: the loop bench.py times) shares its helpers.  A result in the f16 range is recovered inside the loop by
``_RangeCheckpoints`` and, where several batches ran at once, by ``redo_in_fp32``.  EquivariantVariationalDiffusion's public methods call these."""
from __future__ import annotations

import ctypes as C
import logging
import os
from collections import deque
from functools import reduce
from itertools import accumulate
from operator import or_
from typing import Any, Callable, Dict, List, Optional, Tuple

import torch

from . import _native
from .gcpnet import F16RangeError

log = logging.getLogger(__name__.rpartition(".")[0] + ".variational_diffusion")      # the records keep the name they have always had

RANGE_CHECK_EVERY = 25          # steps between two looks at the f16-range flag inside the fused sampling loops


def num_nodes_to_batch_index(num_samples: int, num_nodes, device) -> torch.Tensor:
    """src/models/components/__init__.py:314-321."""
    assert isinstance(num_nodes, int) or len(num_nodes) == num_samples
    idx = torch.arange(num_samples, device=device)
    return torch.repeat_interleave(idx, num_nodes if isinstance(num_nodes, int) else num_nodes.to(device))


def slice_cuts(num_nodes: torch.Tensor, K: int) -> List[int]:
    """Molecule indices [c_0 = 0, c_1, ..., c_K = B] that cut a flat batch into K contiguous, non-empty slices of roughly equal work
    (edges, i.e. sum of n^2) -- used when one batch is sampled on K handles / streams."""
    nn_ = torch.as_tensor(num_nodes).long().cpu()
    Bm = len(nn_)
    if not 1 <= K <= Bm:
        raise ValueError(f"cannot cut {Bm} molecules into {K} non-empty slices")
    work_cum = (nn_ ** 2).cumsum(0)
    cuts = [0]
    # (round 5 measured unequal cuts -- the first slice's tile count a multiple of the persistent workgroup count, 0.4873 / 0.5127 / 0.45 / 0.531 of the work:
    #  6.93 / 6.92 / 6.95 / 6.85 ms per step against 6.88 for the equal cut, profiles/r05_slices.txt: the dispatcher already fills one slice's tails with the other)
    for k in range(1, K):
        c = int(torch.searchsorted(work_cum, work_cum[-1] * k // K).item()) + 1
        cuts.append(min(max(c, cuts[-1] + 1), Bm - (K - k)))
    return cuts + [Bm]


def ptr(t: Optional[torch.Tensor]) -> Optional[C.c_void_p]:
    return None if t is None else C.c_void_p(t.data_ptr())


def node_context(dyn, context: Optional[torch.Tensor], batch_index: torch.Tensor) -> Optional[torch.Tensor]:
    """The per-molecule context gathered per node (fp32, contiguous), or None for a model that takes none."""
    if context is not None:
        return context.to(batch_index.device, torch.float32)[batch_index].contiguous()
    if dyn.condition_on_context:
        raise ValueError("context required by a context-conditioned model")
    return None


def plan_flat(lib, h, sizes: torch.Tensor) -> None:
    """One flat batch of these molecule sizes (int32, host) on a handle no GCPNetDynamics.plan cache stands in front of."""
    _native.check(lib, h, lib.gcdm_plan_batch(h, len(sizes), ptr(sizes)), "gcdm_plan_batch")


def upload_gamma(ddpm, lib, h) -> None:
    g = ddpm.gamma.gamma.detach().to("cpu", torch.float32).contiguous()
    _native.check(lib, h, lib.gcdm_set_gamma(h, ptr(g), g.numel()), "gcdm_set_gamma")


def _pinned_flag_copy(flags: torch.Tensor) -> Callable[[], List[int]]:
    """Asynchronous copy of the device flag word(s) to pinned host memory, on the current stream; returns the reader that waits for it."""
    host = torch.zeros(flags.numel(), dtype=torch.int32).pin_memory()
    host.copy_(flags, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(flags.device))

    def read() -> List[int]:
        ev.synchronize()
        return [int(v) for v in host.tolist()]
    return read


class _RangeCheckpoints:
    """Range guard of the split-precision mode INSIDE a sampling loop, and the loop itself (``run``).  Every RANGE_CHECK_EVERY steps the loop
    hands over a snapshot of its state (latent + counters) together with an asynchronous copy of the device flag word; one interval later
    that copy has long arrived and is looked at without stalling the GPU: clean -> the snapshot becomes the restart point;
    GCDM_FLAG_F16_RANGE -> the loop resumes from the previous restart point with fp32 MFMA instead of re-running the whole trajectory (an
    overflow at step 900 of 1000 costs <= 1.3x a clean run; it used to cost 1 + 2.7).  ``active=False`` (the handle already runs fp32 MFMA):
    the plain loop.  ``copy_flags(flags)`` starts the flag copy and returns its reader (default: pinned copy + event)."""

    def __init__(self, active: bool = True, copy_flags: Callable[[torch.Tensor], Callable[[], List[int]]] = _pinned_flag_copy):
        self.active = active
        self.copy_flags = copy_flags
        self.good = None             # (state, tensors) verified clean
        self.pend = None             # (state, tensors, reader of the flag copy) waiting for its flag copy
        self.rewinds = 0
        self.fell_back = False       # the handle was switched to fp32 MFMA at step resume_step
        self.resume_step = None
        self.tail_flag = False       # GCDM_FLAG_TAIL in any flag word looked at (the caller disables the fused layer launch)

    def run(self, num_timesteps: int, step: Callable[[int], None], final: Callable[[], int], flags: torch.Tensor,
            save: Callable[[], Tuple[Dict[str, Any], List[torch.Tensor]]], load: Callable[[Dict[str, Any], List[torch.Tensor]], None],
            set_mode: Callable[[int], None], wait: Callable[[], None] = lambda: None, fence: Callable[[], None] = lambda: None) -> int:
        """Steps s = num_timesteps - 1 ... 0, then the final decode; returns its flag word (the caller reports it).  ``step(s)`` / ``final()``
        enqueue the work (``final`` reads the flag word: the one host sync of a clean run); ``save()`` -> (counters, latent tensors) and
        ``load(counters, copies)`` put a snapshot back; ``set_mode(m)`` switches the handle(s) between fp32 (0) and split-precision (1) MFMA;
        ``wait()`` / ``fence()`` order the caller's stream after / before the work around a snapshot or restore (several streams)."""
        def restart(point):
            st, copies = point
            wait()
            load(st, copies)
            self.restore_flags(flags, st)
            if not self.fell_back:
                log.warning("An activation left the f16 range of the split-precision kernels; resuming from step %d with fp32 MFMA.", st["s"])
                set_mode(0)
                self.fell_back, self.resume_step = True, st["s"]
            fence()
            return st["s"]

        try:
            s = num_timesteps - 1
            if self.active:
                wait()
                st, tensors = save()
                self.good = (dict(st, s=s), [t.clone() for t in tensors])
                fence()
            while True:
                while s >= 0:
                    if self.active and not self.fell_back and (num_timesteps - 1 - s) % RANGE_CHECK_EVERY == 0 and s != num_timesteps - 1:
                        wait()
                        st, tensors = save()
                        point = self.snapshot(dict(st, s=s), tensors, flags)
                        fence()
                        if point is not None:
                            s = restart(point)
                            continue
                    step(s)
                    s -= 1
                fl = final()
                point = self.resolve(fl) if (self.active and not self.fell_back) else None
                if point is None:
                    return fl
                s = restart(point)       # an overflow in the last interval (or in the decode): repeat it in fp32
        finally:
            if self.fell_back:
                set_mode(1)

    def snapshot(self, state: Dict[str, Any], tensors: List[torch.Tensor], flags: torch.Tensor):
        """Called on the stream the latent is valid on.  Returns the restart point to rewind to if the PREVIOUS snapshot's flag is dirty."""
        rewind = self.resolve()
        if rewind is not None:
            return rewind
        copies = [t.clone() for t in tensors]
        self.pend = (dict(state), copies, self.copy_flags(flags))
        return None

    def resolve(self, final_flags: Optional[int] = None):
        """Looks at the pending snapshot's flag copy (or, at the end of the run, at the final flag word).  Returns (state, tensors) to rewind
        to, or None if the trajectory so far is clean."""
        if self.pend is not None:
            st, copies, read = self.pend
            host = read()
            self.pend = None
            self.tail_flag |= any(v & _native.FLAG_TAIL for v in host)
            if any(v & _native.FLAG_F16_RANGE for v in host):
                return self._rewind()
            st["flags"] = host                                 # the flag word(s) AT the snapshot: what a rewind restores (bits raised during a
            self.good = (st, copies)                           # discarded f16 interval -- NaN in vel, CoG drift -- must not survive it)
        if final_flags is not None:
            self.tail_flag |= bool(final_flags & _native.FLAG_TAIL)
            if final_flags & _native.FLAG_F16_RANGE:
                return self._rewind()
        return None

    def _rewind(self):
        self.rewinds += 1
        return self.good

    @staticmethod
    def restore_flags(flags: torch.Tensor, state: Dict[str, Any]) -> None:
        """Device flag word(s) back to their value at the restart point.  The first restart point (start of the loop) has no copy: only the
        bits a network evaluation / decode can raise are cleared there (a mean-not-zero flag of the encode step in front of it stays)."""
        saved = state.get("flags")
        if saved is not None:
            flags.copy_(torch.tensor(saved, dtype=flags.dtype).to(flags.device, non_blocking=True))
        else:
            flags.bitwise_and_(~(_native.FLAG_F16_RANGE | _native.FLAG_NAN_VEL | _native.FLAG_COG_DRIFT | _native.FLAG_TAIL))


class _FusedRun:
    """A flat batch (one entry in ``num_nodes_list``), or a packed plan (``packed=True``: the batches laid end to end, one flag word and one seed
    each), on one handle and one stream: the primary handle and the current stream, or those of ``lane``.  Plans the handle and owns what the entry
    points read and write; the entry points are methods, in the library's names.  A flat run on the primary handle takes the self-conditioned entry
    points when the model is self-conditioned (lanes and packed plans do not serve those)."""

    def __init__(self, ddpm, device: torch.device, num_nodes_list, contexts, seeds, lane=None, packed: bool = False, frames: int = 1,
                 noise_fn: Optional[Callable[[int], torch.Tensor]] = None):
        self.device, self.noise_fn, K = device, noise_fn, len(num_nodes_list)
        self.dyn, self.lib, self.h = dyn, lib, h = ddpm._native(device) if lane is None else (ddpm.dynamics_network, lane.lib, lane.h)
        self.stream = C.c_void_p((torch.cuda.current_stream(device) if lane is None else lane.stream).cuda_stream)
        sizes = [torch.as_tensor(nn_, dtype=torch.int32, device="cpu").reshape(-1) for nn_ in num_nodes_list]
        self.bis = [num_nodes_to_batch_index(len(sz), sz.to(device), device=device) for sz in sizes]
        self.node_off = [0] + list(accumulate(int(bi.shape[0]) for bi in self.bis))
        self.N, self.D = self.node_off[-1], ddpm.num_x_dims + ddpm.num_node_scalar_features
        if packed:
            self.ctx = None                    # (a model that takes no context ignores the argument)
            if dyn.condition_on_context:
                self.ctx = torch.cat([node_context(dyn, c, bi) for c, bi in zip(contexts, self.bis)], dim=0).contiguous()
            per_batch, nn_all = torch.tensor([len(sz) for sz in sizes], dtype=torch.int32), torch.cat(sizes).contiguous()
            dyn._plan_key = None               # the handle's plan is no longer one GCPNetDynamics.plan made: the next plan() call builds its own
            dyn._plan_src = None
            self.check(lib.gcdm_plan_batches(h, K, ptr(per_batch), ptr(nn_all)), "gcdm_plan_batches")
            self.check(lib.gcdm_set_batch_seeds(h, K, (C.c_uint64 * K)(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in seeds])), "gcdm_set_batch_seeds")
            self.seed = C.c_uint64(0)          # ignored under a packed plan
        else:
            if lane is None:
                dyn.plan(sizes[0])
            else:
                plan_flat(lib, h, sizes[0])
            self.ctx = node_context(dyn, contexts[0], self.bis[0])
            self.seed = C.c_uint64(seeds[0])
        self.z = torch.empty((self.N, self.D), dtype=torch.float32, device=device)
        self.frames = torch.zeros((frames, self.N, self.D), dtype=torch.float32, device=device)     # frame 0 = the final sample (:1404-1410)
        self.out = self.frames[0]
        self.flags = torch.zeros(K, dtype=torch.int32, device=device)
        # the estimate fed back into the next step (:1363-1375)
        self.self_cond = torch.zeros_like(self.z) if lane is None and not packed and getattr(dyn, "self_condition", False) else None
        self.zp, self.cp, self.fp, self.scp = ptr(self.z), ptr(self.ctx), ptr(self.flags), ptr(self.self_cond)
        self.k = 0                             # number of the next noise draw
        self.held: deque = deque(maxlen=8)     # tape tensors of the last calls, alive until the stream (which frees in its own order) has consumed them

    def check(self, st: int, what: str) -> None:
        _native.check(self.lib, self.h, st, what)

    def draw(self) -> Optional[C.c_void_p]:
        """Tape tensor of draw number k, or None = Philox draw number k."""
        k = self.k
        self.k = k + 1
        if self.noise_fn is None:
            return None
        nz = self.noise_fn(k).to(self.device, torch.float32).contiguous()
        self.held.append(nz)
        return ptr(nz)

    def init(self) -> None:
        self.check(self.lib.gcdm_sample_init(self.h, self.zp, self.draw(), self.seed, self.stream), "gcdm_sample_init")

    def encode(self, xin: torch.Tensor) -> None:
        self.check(self.lib.gcdm_encode_samples(self.h, ptr(xin), self.zp, self.fp, self.stream), "gcdm_encode_samples")

    def step(self, s: int, t_norm: int, have_estimate: bool = False) -> None:
        p = self.draw()
        if self.self_cond is not None:
            st = self.lib.gcdm_sample_step_sc(self.h, self.zp, self.scp, int(have_estimate), self.cp, s, t_norm, p, self.draw(), self.seed, self.fp, self.stream)
        else:
            st = self.lib.gcdm_sample_step(self.h, self.zp, self.cp, s, t_norm, p, self.seed, self.fp, self.stream)
        self.check(st, "gcdm_sample_step")

    def unnormalize(self, frame: int) -> None:
        self.check(self.lib.gcdm_unnormalize_z(self.h, self.zp, ptr(self.frames[frame]), self.stream), "gcdm_unnormalize_z")

    def inpaint_center(self, xh0: torch.Tensor, fixed: torch.Tensor) -> None:
        self.check(self.lib.gcdm_inpaint_center(self.h, ptr(xh0), ptr(fixed), ptr(xh0), self.stream), "gcdm_inpaint_center")

    def inpaint_step(self, xh0: torch.Tensor, fixed: torch.Tensor, s: int, t_norm: int, have_estimate: bool) -> None:
        base = self.k
        p_known, p_unknown = self.draw(), self.draw()
        p_sc = self.draw() if self.self_cond is not None else None
        st = self.lib.gcdm_inpaint_step(self.h, self.zp, ptr(xh0), ptr(fixed), self.scp, int(have_estimate), self.cp, s, t_norm, p_known, p_unknown, p_sc,
                                        self.seed, base, self.fp, self.stream)
        self.check(st, "gcdm_inpaint_step")

    def inpaint_jump(self, s: int, t: int, t_norm: int) -> None:
        dk = self.k
        self.check(self.lib.gcdm_inpaint_jump(self.h, self.zp, s, t, t_norm, self.draw(), self.seed, dk, self.stream), "gcdm_inpaint_jump")

    def final(self, have_estimate: bool = False) -> None:
        """The decode into frame 0.  The CoG re-projection is for runs without intermediate frames only (:1389, :1767)."""
        p = self.draw()
        self.check(self.lib.gcdm_set_option(self.h, b"cog_fix", 1 if len(self.frames) == 1 else 0), "gcdm_set_option")
        if self.self_cond is not None:
            st = self.lib.gcdm_sample_final_sc(self.h, self.zp, self.scp if have_estimate else None, self.cp, p, self.seed, ptr(self.out), self.fp, self.stream)
        else:
            st = self.lib.gcdm_sample_final(self.h, self.zp, self.cp, p, self.seed, ptr(self.out), self.fp, self.stream)
        self.lib.gcdm_set_option(self.h, b"cog_fix", 1)
        self.check(st, "gcdm_sample_final")

    def read_flags(self) -> List[int]:
        """The flag word(s) on the host: a host sync (the one of a clean run)."""
        return [int(v) for v in self.flags.tolist()]

    def result(self, b: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(samples, batch index, node mask) of batch b."""
        return self.out[self.node_off[b]:self.node_off[b + 1]], self.bis[b], torch.ones_like(self.bis[b]).bool()


def sample(ddpm, num_nodes, device: torch.device, return_frames: int, num_timesteps: int, t_norm: int, context, fix_noise: bool, noise_fn, seed: int,
           step_callback, init_xh) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """mol_gen_sample / mol_gen_optimize on the fused kernels: one run on the primary handle, under the range guard."""
    run = _FusedRun(ddpm, device, [num_nodes], [context], [seed], frames=return_frames, noise_fn=noise_fn)
    latent = [run.z] if run.self_cond is None else [run.z, run.self_cond]
    run.check(run.lib.gcdm_set_option(run.h, b"fix_noise", int(bool(fix_noise))), "gcdm_set_option")

    def step(s):
        run.step(s, t_norm, s != num_timesteps - 1)
        if return_frames > 1 and (s * return_frames) % num_timesteps == 0:             # save frame (:1354-1361)
            run.unnormalize((s * return_frames) // num_timesteps)
        if step_callback is not None:
            step_callback(s, run.z)          # (fires again for the steps a resumed run repeats)

    def final():
        run.final(num_timesteps > 0)
        return run.read_flags()[0]           # the one host sync of a clean run

    def load(st, copies):
        for t_, c_ in zip(latent, copies):
            t_.copy_(c_)
        run.k = st["k"]

    guard = _RangeCheckpoints(active=run.dyn.mfma_mode == 1)
    try:
        if init_xh is None:
            run.init()
        else:                                # optimisation loop: z = normalize(samples) (:1451-1464), no initial draw
            xin = init_xh.to(device, torch.float32).contiguous()
            if xin.shape != (run.N, run.D):
                raise ValueError(f"samples have shape {tuple(xin.shape)}, expected {(run.N, run.D)}")
            run.encode(xin)
        fl = guard.run(num_timesteps, step, final, run.flags, lambda: ({"k": run.k}, latent), load, run.dyn.set_mfma_mode)
    finally:
        run.lib.gcdm_set_option(run.h, b"fix_noise", 0)
    ddpm._report_flags(fl, "mol_gen_sample", guard)
    return (run.out if return_frames == 1 else run.frames, *run.result()[1:])


def inpaint_once(ddpm, molecule, node_mask_fixed, schedule: List[int], jump_length: int, return_frames: int, num_timesteps: int, context, noise_fn,
                 seed: int) -> torch.Tensor:
    """inpaint on the fused kernels, one run over the RePaint ``schedule``.  Raises F16RangeError if an activation left the f16 range of the
    split-precision kernels."""
    device = torch.device(molecule["x"].device)
    run = _FusedRun(ddpm, device, [molecule["num_nodes"]], [context], [seed], frames=return_frames, noise_fn=noise_fn)
    if "batch_index" in molecule and not torch.equal(molecule["batch_index"].to(device), run.bis[0]):
        raise ValueError("molecule['batch_index'] must be the contiguous index implied by molecule['num_nodes']")
    parts = [molecule["x"], molecule["one_hot"]] + ([molecule["charges"]] if ddpm.include_charges else [])
    xh0 = torch.cat([p.to(device, torch.float32) for p in parts], dim=-1).contiguous()
    fixed = node_mask_fixed.to(device).bool().contiguous()
    if xh0.shape != (run.N, run.D) or fixed.shape != (run.N,):
        raise ValueError(f"molecule has shape {tuple(xh0.shape)} / mask {tuple(fixed.shape)}, expected {(run.N, run.D)} / {(run.N,)}")
    run.inpaint_center(xh0, fixed)
    run.init()
    s, first = num_timesteps - 1, True
    for i, num_denoise_steps in enumerate(schedule):
        for j in range(num_denoise_steps):
            run.inpaint_step(xh0, fixed, s, num_timesteps, not first)
            first = False
            # frame at the end of a resample cycle (:1707-1715)
            if return_frames > 1 and (num_denoise_steps > jump_length or i == len(schedule) - 1) and (s * return_frames) % num_timesteps == 0:
                run.unnormalize((s * return_frames) // num_timesteps)
            if j == num_denoise_steps - 1 and i < len(schedule) - 1:       # go back `jump_length` steps (:1717-1737)
                run.inpaint_jump(s, s + jump_length, num_timesteps)
                s += jump_length
            s -= 1
    run.final(not first)
    fl = run.read_flags()[0]                                                # the one host sync of the run
    if fl & _native.FLAG_F16_RANGE and run.dyn.mfma_mode == 1:
        if fl & _native.FLAG_TAIL:
            run.dyn.disable_fused_layer("inpaint")
        raise F16RangeError("an activation left the f16 range of the split-precision kernels during inpainting")
    ddpm._report_flags(fl, "inpaint")
    return run.out if return_frames == 1 else run.frames


def redo_in_fp32(ddpm, where: str, warning: str, words: List[int], num_nodes_list, contexts, seeds, device, num_timesteps: int,
                 plan_wide: bool) -> List[Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]]:
    """What follows the flag words of several batches that ran at once: a batch whose word has the f16-range bit (``plan_wide``: every batch, if
    any word has it -- the batches of a packed plan share their launches) is redone by mol_gen_sample on the primary handle, which falls back to
    fp32 MFMA -- with ``warning`` logged and the fused layer launch turned off on FLAG_TAIL; every other word goes through ``_report_flags``.
    Returns the redone results (None where the batch stands) and leaves the OR of all of it in ``last_flags``."""
    results, fl_all = [None] * len(words), 0
    for group in ([range(len(words))] if plan_wide else [[b] for b in range(len(words))]):
        fl = reduce(or_, (words[b] for b in group), 0)
        if fl & _native.FLAG_F16_RANGE:                        # rare
            log.warning(warning)
            if fl & _native.FLAG_TAIL:
                ddpm.dynamics_network.disable_fused_layer(where)
            for b in group:
                results[b] = ddpm.mol_gen_sample(len(num_nodes_list[b]), num_nodes_list[b], device, num_timesteps=num_timesteps, context=contexts[b],
                                                 seed=seeds[b])
                fl_all |= ddpm.last_flags
        else:
            for b in group:
                fl_all |= ddpm._report_flags(words[b], where)
    ddpm.last_flags = fl_all
    return results


def sample_batches(ddpm, num_nodes_list, device: torch.device, T: int, contexts, seeds, packed: bool) -> List[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
    """Several independent batches at once.  ``packed``: laid end to end in ONE packed plan on the primary handle, one (captured) launch set per step;
    otherwise batch b on lane b (its own handle and stream), the step launches of all batches interleaved on the host."""
    if packed:
        runs = [_FusedRun(ddpm, device, num_nodes_list, contexts, seeds, packed=True)]
    else:
        ddpm._native(device)                               # validates the dynamics network, uploads the primary handle
        runs = [_FusedRun(ddpm, device, [num_nodes_list[b]], [contexts[b]], [seeds[b]], lane=ln)
                for b, ln in zip(range(len(num_nodes_list)), get_lanes(ddpm, len(num_nodes_list), device))]
        torch.cuda.synchronize(device)
    for run in runs:
        run.init()
    for s in reversed(range(T)):
        for run in runs:
            run.step(s, T)
    for run in runs:
        run.final()
    if not packed:
        torch.cuda.synchronize(device)
    words = [fl for run in runs for fl in run.read_flags()]                 # (packed: the one host sync of a clean run)
    where, what = ("mol_gen_sample_packed", "packed run; re-running its batches") if packed else ("mol_gen_sample_concurrent", "concurrent batch; re-running it")
    redone = redo_in_fp32(ddpm, where, f"An activation left the f16 range in a {what} with fp32 MFMA.", words, num_nodes_list, contexts, seeds, device, T,
                          plan_wide=packed)
    stands = [run.result(b) for run in runs for b in range(len(run.bis))]
    return [stands[b] if r is None else r for b, r in enumerate(redone)]


# ---- lanes: extra handles that mirror the primary one ------------------------------------------------------------------------------
def lane_key(ddpm, device: torch.device):
    g = ddpm.gamma.gamma
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return (ddpm.dynamics_network._params_fingerprint(), idx, g.data_ptr(), g._version)


class _Lane:
    """One extra library handle + stream: its own packed weights (26 MB) and workspace, so that the launches of different
    batches are independent and the GPU can fill the CUs a 100-molecule batch leaves idle."""

    def __init__(self, ddpm, device: torch.device):
        dyn = ddpm.dynamics_network
        self.lib, self.h = _native.load(), C.c_void_p()
        idx = device.index if device.index is not None else torch.cuda.current_device()
        cfg = dyn._native_config(idx)
        _native.check(self.lib, self.h, self.lib.gcdm_create(C.byref(cfg), C.byref(self.h)), "gcdm_create")
        dyn.upload_weights(self.lib, self.h)
        upload_gamma(ddpm, self.lib, self.h)
        self.lib.gcdm_set_option(self.h, b"mfma_mode", dyn.mfma_mode)
        # lane handles run CONCURRENTLY with other handles (slices of one batch, batches in flight): two launches per layer there -- the fused layer launch
        # (option "fuse_node") packs a single handle's tiles better (-3 % per step), but beside another launch its node role is gated and loses (+3 %)
        # (GCDM_LANE_FUSE=1: A/B hook.  Stream priorities for the slices -- lane 0 high, lane 1 normal, so that one slice's launch would be dispatched whole before
        #  the other's -- were measured too: no effect on the dispatch interleave, 7.00 vs 7.00 ms per step un-fused, 7.21 vs 7.22 fused; profiles/r06_ab_log.txt)
        self.lib.gcdm_set_option(self.h, b"fuse_node", int(os.environ.get("GCDM_LANE_FUSE", "0")))
        self.stream = torch.cuda.Stream(device)
        self.key = lane_key(ddpm, device)

    def close(self):
        if self.h:
            self.lib.gcdm_destroy(self.h)
            self.h = None


def get_lanes(ddpm, K: int, device: torch.device) -> List[_Lane]:
    """K extra handles that mirror the primary one (kept in ``ddpm._lanes``).  A lane is a COPY of the weights: after load_state_dict / an EMA swap /
    fine-tuning / `.to(other device)` the stale ones are rebuilt (the primary handle re-uploads through sync_weights)."""
    lanes = list(getattr(ddpm, "_lanes", None) or [])
    key = lane_key(ddpm, device)
    for i, ln in enumerate(lanes):
        if ln.h is None or ln.key != key:                  # no longer a copy of the primary handle's weights / schedule / device
            ln.close()
            lanes[i] = _Lane(ddpm, device)
    lanes += [_Lane(ddpm, device) for _ in range(K - len(lanes))]
    for ln in lanes:
        ln.lib.gcdm_set_option(ln.h, b"mfma_mode", ddpm.dynamics_network.mfma_mode)
    ddpm._lanes = lanes
    return lanes


class _SlicedBatch:
    """One flat batch sampled as K contiguous slices of molecules, each on its own handle and HIP stream (same semantics and the
    same Philox noise as the single-handle run: a slice's boundary nodes read their flat neighbours from the adjacent slice,
    options "flat_prev" / "flat_next" / "node_base").  The latent is double-buffered (`gcdm_sample_step_to`) and the slices join
    once per step, so no slice ever reads a row its neighbour is writing.  Fills the round-quantisation tails of the big
    configurations (+5-6 % at 1024 QM9 / 256 GEOM molecules on MI355X)."""

    def __init__(self, ddpm, num_nodes, device: torch.device, context: Optional[torch.Tensor], seed: int, K: int):
        self.ddpm, self.device, self.K = ddpm, device, K
        self.dyn = dyn = ddpm._native(device)[0]
        nn_ = torch.as_tensor(num_nodes, dtype=torch.int32, device="cpu")
        self.cuts = cuts = slice_cuts(nn_, K)
        self.node_off = torch.cat((torch.zeros(1, dtype=torch.long), nn_.long().cumsum(0))).tolist()
        lanes = get_lanes(ddpm, K, device)
        self.batch_index = num_nodes_to_batch_index(len(nn_), nn_.to(device), device=device)
        N, D = int(self.batch_index.shape[0]), ddpm.num_x_dims + ddpm.num_node_scalar_features
        self.ctx = node_context(dyn, context, self.batch_index)
        self.bufs = [torch.empty((N, D), dtype=torch.float32, device=device) for _ in range(2)]
        self.out = torch.empty((N, D), dtype=torch.float32, device=device)
        self.flags = torch.zeros(K, dtype=torch.int32, device=device)
        self.sd = C.c_uint64(seed)
        self.sl = []
        for k in range(K):
            ln = lanes[k]
            plan_flat(ln.lib, ln.h, nn_[cuts[k]:cuts[k + 1]].contiguous())
            n0 = self.node_off[cuts[k]]
            for name, val in ((b"flat_prev", int(k > 0)), (b"flat_next", int(k < K - 1)), (b"node_base", n0), (b"mfma_mode", dyn.mfma_mode)):
                _native.check(ln.lib, ln.h, ln.lib.gcdm_set_option(ln.h, name, val), "gcdm_set_option")
            self.sl.append(dict(lane=ln, n0=n0, stream=C.c_void_p(ln.stream.cuda_stream), ev=torch.cuda.Event(),
                                fl=C.c_void_p(self.flags.data_ptr() + 4 * k)))
        self.cur = 0

    @staticmethod
    def _row(t_, n0):
        return C.c_void_p(t_.data_ptr() + 4 * n0 * t_.shape[1])

    def _cptr(self, n0):
        return None if self.ctx is None else self._row(self.ctx, n0)

    def _join(self):
        for a_ in self.sl:
            for b_ in self.sl:
                if a_ is not b_:
                    a_["lane"].stream.wait_event(b_["ev"])

    def init(self):
        start = torch.cuda.Event()
        start.record(torch.cuda.current_stream(self.device))
        for w in self.sl:
            ln = w["lane"]
            ln.stream.wait_event(start)
            _native.check(ln.lib, ln.h, ln.lib.gcdm_sample_init(ln.h, self._row(self.bufs[0], w["n0"]), None, self.sd, w["stream"]), "gcdm_sample_init")
            w["ev"].record(ln.stream)
        self.cur = 0

    def step(self, s: int, t_norm: int):
        self._join()
        cur, nxt = self.cur, 1 - self.cur
        for w in self.sl:
            ln = w["lane"]
            st = ln.lib.gcdm_sample_step_to(ln.h, self._row(self.bufs[cur], w["n0"]), self._row(self.bufs[nxt], w["n0"]), self._cptr(w["n0"]), s, t_norm,
                                            None, self.sd, w["fl"], w["stream"])
            _native.check(ln.lib, ln.h, st, "gcdm_sample_step_to")
            w["ev"].record(ln.stream)
        self.cur = nxt

    def final(self):
        self._join()
        for w in self.sl:
            ln = w["lane"]
            st = ln.lib.gcdm_sample_final(ln.h, self._row(self.bufs[self.cur], w["n0"]), self._cptr(w["n0"]), None, self.sd, self._row(self.out, w["n0"]),
                                          w["fl"], w["stream"])
            _native.check(ln.lib, ln.h, st, "gcdm_sample_final")
            w["ev"].record(ln.stream)
        self.wait()

    def wait(self):
        """The caller's current stream waits for every slice (no host sync)."""
        cs = torch.cuda.current_stream(self.device)
        for w in self.sl:
            cs.wait_event(w["ev"])

    def close(self):
        for w in self.sl:                                   # lanes go back to whole-batch behaviour
            for name in (b"flat_prev", b"flat_next", b"node_base"):
                w["lane"].lib.gcdm_set_option(w["lane"].h, name, 0)

    def recentre_undrifted(self, drift: List[bool]):
        """The reference re-projects the WHOLE batch when any molecule drifted (:1389-1402): slices that saw no drift follow."""
        for k, w in enumerate(self.sl):
            if not drift[k]:
                n0, n1 = w["n0"], self.node_off[self.cuts[k + 1]]
                bi = self.batch_index[n0:n1] - self.batch_index[n0]
                cnt = torch.bincount(bi).clamp(min=1).to(torch.float32)[:, None]
                mean = torch.zeros((int(bi.max()) + 1, 3), device=self.device).index_add_(0, bi, self.out[n0:n1, :3]) / cnt
                self.out[n0:n1, :3] -= mean[bi]


def sample_lanes(ddpm, num_nodes, device: torch.device, num_timesteps: int, t_norm: int, context, seed: int, K: int):
    """mol_gen_sample(lanes=K): plain sampling with on-device noise, the flat batch as K slices, under the range guard."""
    sb = _SlicedBatch(ddpm, num_nodes, device, context, seed, K)
    cs = torch.cuda.current_stream(device)
    fl_all: List[int] = []

    def fence():                         # the slices continue only after what the caller's stream has just done with their buffers
        ev = torch.cuda.Event()
        ev.record(cs)
        for w in sb.sl:
            w["lane"].stream.wait_event(ev)

    def final():
        sb.final()
        fl_all[:] = sb.flags.cpu().tolist()             # the one host sync of a clean run
        return reduce(or_, fl_all, 0)

    def set_mode(mode):
        for w in sb.sl:
            w["lane"].lib.gcdm_set_option(w["lane"].h, b"mfma_mode", mode)

    guard = _RangeCheckpoints(active=sb.dyn.mfma_mode == 1)
    try:
        sb.init()
        fl = guard.run(num_timesteps, lambda s: sb.step(s, t_norm), final, sb.flags, lambda: ({}, [sb.bufs[sb.cur]]),
                       lambda st, copies: sb.bufs[sb.cur].copy_(copies[0]), set_mode, wait=sb.wait, fence=fence)
    finally:
        sb.close()
    ddpm._report_flags(fl, "mol_gen_sample", guard)
    drift = [bool(int(v) & _native.FLAG_COG_DRIFT) for v in fl_all]
    if any(drift) and not all(drift):
        sb.recentre_undrifted(drift)
    return sb.out, sb.batch_index, torch.ones_like(sb.batch_index).bool()
