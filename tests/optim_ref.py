"""fp64 restatement of the reference's update after backward() -- what optim.TrainingUpdate computes -- with a running bound on the error of
an fp32 evaluation of the same step (tests/test_optim_cpu.py checks the restatement against torch.optim.AdamW and clip_grad_norm_ in fp64;
tests/test_optim_gpu.py checks the HIP update against it).

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
