"""fp64 restatement of the reference's update after backward() -- what optim.TrainingUpdate computes -- with a running bound on the error of
an fp32 evaluation of the same step (tests/test_optim_cpu.py checks the restatement against torch.optim.AdamW and clip_grad_norm_ in fp64;
tests/test_optim_gpu.py and tests/test_optim_cabi_gpu.py check the HIP update against it), and Emu32, the same step in numpy float32 on
the buffers of include/gcdm_optim.h, which the CPU tests hold to the bars the device is held to.

The reference (qm9_mol_gen_ddpm.py configure_gradient_clipping, models/__init__.py Queue, utils/__init__.py EMA):
    max_norm = 1.5 * mean(Q) + 2 * std(Q)   (numpy, population std; Q seeded with 3000, the last `queue_len` values, newest first)
    clip_grad_norm_(params, max_norm); Q.add(min(norm, max_norm))
    AdamW(lr, betas, eps, weight_decay, amsgrad).step()
    ema -= (1 - decay) * (ema - p)      (every state entry, after the step)

Error bound of the fp32 step (u = 2^-24, unit roundoff).  Starting from an fp32 state that is within `err_*` of this oracle's state:
  * norm: per chunk an fp32 sum of <= 16384 squares (each thread a sequential sum of <= 64 products, then 6 shuffle levels and 4 wave
    totals), then fp64: a sum of positive terms with <= 80 roundings -> relative error <= 80u; the square root halves it, the cast adds u:
    eps_norm = 41u.  coef = (1 / (norm + 1e-6)) * max_norm, three fp32 roundings: eps_c = eps_norm + 3u (0 when coef = 1 exactly).
  * g' = coef g: |dg'| <= (eps_c + u) |g'|.
  * m = m + w (g' - m): three roundings on terms bounded by |m_old| + |g'|: |dm| <= b1 |dm_old| + (1 - b1) |dg'| + 3u (|m_old| + |g'|) + u|m|.
  * v = b2 v + (1 - b2) g'^2: positive terms, four roundings: |dv| <= b2 |dv_old| + (1 - b2) 2 |dg'| |g'| + 4u v + u v.
  * den = sqrt(vmax) / sbc2 + eps: |dden| / den <= |dvmax| / (2 vmax) + 4u (sqrt, cast of sbc2, division, addition).
  * p = p (1 - lr wd) + (-ss) (m / den): |dp| <= |dp_old| + 3u |p| + ss (|dm| / den + |m| / den (|dden| / den) + 3u |m| / den).
  * ema = ema - (ema - p) w: |dema| <= |dema_old| + w |dp| + 3u (|ema| + |p|).
Second-order terms are below u^2 relative; the tests allow twice the bound plus 1e-30."""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np
import torch

U = 2.0 ** -24


class Queue:
    """models/__init__.py Queue, restated."""

    def __init__(self, max_len=50):
        self.items, self.max_len = [], max_len

    def add(self, item):
        self.items.insert(0, item)
        if len(self.items) > self.max_len:
            self.items.pop()

    def mean(self):
        return np.mean(self.items)

    def std(self):
        return np.std(self.items)


class RefUpdate:
    """The update in float64 on the device of `params`; `err_*` the running bound of an fp32 evaluation (module docstring)."""

    def __init__(self, params: List[torch.Tensor], lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-12, amsgrad=True, clip_gradients=True,
                 queue_len=50, ema_decay: Optional[float] = 0.9999, ema_every=1, ema_start=0):
        self.p = [q.detach().double().clone() for q in params]
        self.lr, (self.b1, self.b2), self.eps, self.wd = lr, betas, eps, weight_decay
        self.amsgrad, self.clip, self.ema_decay, self.ema_every, self.ema_start = amsgrad, clip_gradients, ema_decay, ema_every, ema_start
        z = lambda: [torch.zeros_like(q) for q in self.p]          # noqa: E731
        self.m, self.v, self.vmax = z(), z(), z()
        self.ema = [q.clone() for q in self.p] if ema_decay is not None else None
        self.steps = [0] * len(self.p)
        self.gstep = 0
        self.queue = Queue(queue_len)
        self.queue.add(3000.0)
        self.err_p, self.err_m, self.err_v, self.err_vmax, self.err_ema = z(), z(), z(), z(), z()
        self.norms, self.coefs, self.max_norms = [], [], []
        self.norms64 = []          # the norm before its rounding to fp32: what the 41u bound of the docstring is relative to

    def step(self, grads: List[Optional[torch.Tensor]]) -> bool:
        gs = [None if g is None else g.detach().double() for g in grads]
        sq = sum(float((g * g).sum()) for g in gs if g is not None)
        norm = math.sqrt(sq)
        norm32 = float(np.float32(norm))
        if not math.isfinite(norm32):
            return False
        coef, eps_c = 1.0, 0.0
        if self.clip:
            max_norm = 1.5 * self.queue.mean() + 2 * self.queue.std()
            coef = min(1.0, max_norm / (norm32 + 1e-6))
            if coef < 1.0:
                eps_c = 44 * U
            self.queue.add(min(norm32, max_norm))
            self.max_norms.append(float(max_norm))
        self.norms.append(norm32)
        self.norms64.append(norm)
        self.coefs.append(coef)
        ema_now = False
        self.gstep += 1
        if self.ema is not None and self.gstep >= self.ema_start and self.gstep % self.ema_every == 0:
            ema_now = True
        for t, g in enumerate(gs):
            if g is not None:
                self._adam(t, coef * g, eps_c)
        if ema_now:
            w = 1.0 - self.ema_decay
            for t in range(len(self.p)):
                self.err_ema[t] = self.err_ema[t] + w * self.err_p[t] + 3 * U * (self.ema[t].abs() + self.p[t].abs())
                self.ema[t] = self.ema[t] - w * (self.ema[t] - self.p[t])
        return True

    def _adam(self, t, g, eps_c):
        self.steps[t] += 1
        k = self.steps[t]
        b1, b2 = self.b1, self.b2
        dg = (eps_c + U) * g.abs()
        m_old = self.m[t]
        self.p[t] = self.p[t] * (1 - self.lr * self.wd)
        self.m[t] = m_old + (1 - b1) * (g - m_old)
        self.err_m[t] = b1 * self.err_m[t] + (1 - b1) * dg + 3 * U * (m_old.abs() + g.abs()) + U * self.m[t].abs()
        self.v[t] = b2 * self.v[t] + (1 - b2) * g * g
        self.err_v[t] = b2 * self.err_v[t] + (1 - b2) * 2 * dg * g.abs() + 5 * U * self.v[t]
        if self.amsgrad:
            take = self.v[t] >= self.vmax[t]
            self.vmax[t] = torch.maximum(self.vmax[t], self.v[t])
            self.err_vmax[t] = torch.maximum(self.err_vmax[t], self.err_v[t])
            vd, evd = self.vmax[t], self.err_vmax[t]
            del take
        else:
            vd, evd = self.v[t], self.err_v[t]
        ss = self.lr / (1 - b1 ** k)
        sbc2 = math.sqrt(1 - b2 ** k)
        den = vd.sqrt() / sbc2 + self.eps
        rel_den = evd / (2 * vd.clamp_min(1e-300)) + 4 * U
        rel_den = torch.where(vd > 0, rel_den, torch.full_like(rel_den, 4 * U))
        upd = ss * self.m[t] / den
        self.err_p[t] = (self.err_p[t] + 3 * U * self.p[t].abs()
                         + ss * (self.err_m[t] / den + self.m[t].abs() / den * rel_den + 3 * U * self.m[t].abs() / den))
        self.p[t] = self.p[t] - upd


class Emu32:
    """One step of include/gcdm_optim.h restated operation by operation in numpy float32, on the header's own buffers: parameters as a list of
    fp32 arrays, the state as four quarters of `total` floats with tensor t at offsets[t], the chunk table, the ring with qhead / qcount and
    the scalars of the 64-byte block.  The norm is an fp32 sum per chunk, then an fp64 sum of the partials.  tests/test_optim_cpu.py holds it
    to the bars the GPU tests use (a correct fp32 evaluation must pass them) and, with `mutant` set to one of MUTANTS, shows that the same
    checks reject that wrong evaluation.  It assumes 16-byte aligned pointers where a mutant depends on the float4 body (a, j)."""

    MUTANTS = {"a": "the tail of the update starts at 0 after the float4 body", "b": "EMA only for tensors with a gradient",
               "c": "steps[t] advances without a gradient", "d": "ema_now tested on gstep before the increment",
               "e": "bias correction from the global step count", "f": "vmax stored with amsgrad = 0", "g": "swap mode 2 also writes ema",
               "h": "the queue push stores max_norm", "i": "the ema pointer omits the tensor's offset",
               "j": "the scalar tail of the norm starts at 0 after the vector body"}

    def __init__(self, params, offsets, total, chunks, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=True, clip=True,
                 queue_len=50, ema=True, ema_decay=0.9, ema_every=1, ema_start=0, mutant=None):
        assert mutant is None or mutant in self.MUTANTS
        self.p = [np.array(q, dtype=np.float32).reshape(-1).copy() for q in params]
        self.numel = [q.size for q in self.p]
        self.offsets, self.total, self.chunks = list(offsets), int(total), [tuple(int(x) for x in c) for c in chunks]
        self.state = np.zeros((4, self.total), dtype=np.float32)
        self.lr, (self.b1, self.b2), self.eps, self.wd = lr, betas, eps, weight_decay
        self.amsgrad, self.clip, self.queue_len = bool(amsgrad), bool(clip), int(queue_len)
        self.ema_on, self.ema_decay, self.ema_every, self.ema_start = bool(ema), ema_decay, int(ema_every), int(ema_start)
        self.mutant = mutant
        T = len(self.p)
        self.steps = np.zeros(T, dtype=np.int64)
        self.tscal = np.full((T, 2), np.nan)
        self.ring = np.zeros(self.queue_len)
        self.norm, self.max_norm, self.coef = 0.0, 0.0, np.float32(0)
        self.flags = self.qhead = self.qcount = self.gstep = self.skipped = self.ema_applied = 0

    def view(self, k, t):
        return self.state[k, self.offsets[t]: self.offsets[t] + self.numel[t]]

    def step(self, grads):
        f32 = np.float32
        gs = [None if g is None else np.asarray(g, dtype=f32).reshape(-1) for g in grads]
        sq = 0.0
        with np.errstate(all="ignore"):
            for t, s, n in self.chunks:
                if gs[t] is None:
                    continue
                x = gs[t][s:s + n]
                part = np.sum(x * x, dtype=f32)
                if self.mutant == "j" and n % 4:
                    part = f32(part + np.sum(x[: n // 4 * 4] * x[: n // 4 * 4], dtype=f32))
                sq += float(part)
            norm = f32(math.sqrt(sq)) if sq == sq and sq >= 0 else f32(np.nan)
        self.norm = float(norm)
        self.skipped, self.ema_applied = int(not np.isfinite(norm)), 0
        if self.skipped:
            self.flags |= 1
            return False
        coef = f32(1)
        if self.clip:
            n = self.qcount
            mean = 0.0
            for i in range(n):
                mean += self.ring[i]
            mean /= n
            var = 0.0
            for i in range(n):
                var += (self.ring[i] - mean) ** 2
            self.max_norm = 1.5 * mean + 2.0 * math.sqrt(var / n)
            inv = f32(1) / (norm + f32(1e-6))
            coef = min(f32(1), inv * f32(self.max_norm))
            self.ring[self.qhead] = self.max_norm if self.mutant == "h" else min(float(norm), self.max_norm)
            self.qhead = (self.qhead + 1) % self.queue_len
            self.qcount = min(self.qcount + 1, self.queue_len)
        self.coef = coef
        k_ema = self.gstep if self.mutant == "d" else self.gstep + 1
        self.gstep += 1
        self.ema_applied = int(self.ema_on and k_ema >= self.ema_start and k_ema % self.ema_every == 0)
        for t, g in enumerate(gs):
            if g is None and self.mutant != "c":
                continue
            self.steps[t] += 1
            k = self.gstep if self.mutant == "e" else int(self.steps[t])
            self.tscal[t] = (self.lr / (1.0 - self.b1 ** k), math.sqrt(1.0 - self.b2 ** k))
        hyp = dict(coef=coef, decay_mul=f32(1.0 - self.lr * self.wd), omb1=f32(1.0 - self.b1), b2=f32(self.b2), omb2=f32(1.0 - self.b2),
                   eps=f32(self.eps), ema_w=f32(1.0 - self.ema_decay))
        for t, s, n in self.chunks:
            has_grad = gs[t] is not None
            if not has_grad and not self.ema_applied:
                continue
            self._chunk(t, s, n, gs[t], hyp)
            if self.mutant == "a" and n % 4 and n >= 4:
                self._chunk(t, s, n // 4 * 4, gs[t], hyp)
        return True

    def _chunk(self, t, s, n, g, h):
        f32 = np.float32
        o = self.offsets[t] + s
        p = self.p[t][s:s + n]
        m, v, vm = (self.state[k, o:o + n] for k in range(3))
        e = self.state[3, s:s + n] if self.mutant == "i" else self.state[3, o:o + n]
        has_grad = g is not None
        if has_grad:
            ss, sbc2 = f32(self.tscal[t, 0]), f32(self.tscal[t, 1])
            gg = g[s:s + n] * h["coef"]
            p[:] = p * h["decay_mul"]
            m[:] = m + h["omb1"] * (gg - m)
            v[:] = v * h["b2"] + gg * gg * h["omb2"]
            if self.amsgrad:
                vm[:] = np.maximum(vm, v)
                den = np.sqrt(vm) / sbc2 + h["eps"]
            else:
                den = np.sqrt(v) / sbc2 + h["eps"]
                if self.mutant == "f":
                    vm[:] = 0
            p[:] = p + (-ss) * (m / den)
        if self.ema_applied and (has_grad or self.mutant != "b"):
            e[:] = e - (e - p) * h["ema_w"]

    def swap(self, mode):
        """gcdm_optim_ema_swap: 0 swaps p and ema, 1 copies p into ema, 2 copies ema into p."""
        for t in range(len(self.p)):
            x, y = self.p[t].copy(), self.view(3, t).copy()
            if mode != 1:
                self.p[t][:] = y
            if mode != 2 or self.mutant == "g":
                self.view(3, t)[:] = x
