"""The reference's training update after backward() as one fused HIP step (include/gcdm_optim.h): adaptive gradient clipping over a queue of
the last clipped norms (qm9_mol_gen_ddpm.py configure_gradient_clipping, models/__init__.py Queue / get_grad_norm), torch.optim.AdamW with
AMSGrad (configs/model/*_mol_gen_ddpm.yaml) and the EMA of the weights (configs/callbacks/ema.yaml, utils/__init__.py EMA).

One ``step()`` is three launches on the current stream and no host sync.  Parameters stay where they are and autograd keeps ``p.grad``;
the moments, the AMSGrad maximum and the EMA live in one flat fp32 buffer.  Deliberate difference from the reference: a step whose gradient
norm is not finite is skipped as a whole (parameters, moments, step counts, EMA and queue unchanged) and raises FLAG_NONFINITE in
``read_flags()``; the reference would write NaN into every weight.

``BucketedUpdate`` (opt-in) wraps a ``TrainingUpdate`` for data-parallel and accumulated steps: every backward pass is packed into one flat
gradient bucket laid out like the update's state (include/gcdm_grad_bucket.h), one all-reduce sums it over the ranks, and the same fused
step consumes it."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Any, Dict, Iterable, List, Optional

import torch

from . import _native

FLAG_NONFINITE = _native.OPTIM_FLAG_NONFINITE
FLAG_MISMATCH = _native.GRAD_BUCKET_FLAG_MISMATCH       # BucketedUpdate: the ranks disagreed on which tensors have a gradient
QUEUE_MAX = _native.OPTIM_QUEUE_MAX
CHUNK = 16384                 # values per chunk (one workgroup each): the QM9 model gives several hundred chunks
QUEUE_SEED = 3000.0           # qm9_mol_gen_ddpm.py: gradnorm_queue.add(3000), a large value that gets flushed

# workspace sections (gcdm_optim_workspace_bytes(which, ...))
_TOTAL, _PTAB, _GTAB, _OTAB, _NTAB, _CTAB, _HOST_END, _STEPS, _TSCAL, _PART, _QUEUE, _SCAL = range(12)


class TrainingUpdate(torch.optim.Optimizer):
    """Clipping + AdamW (AMSGrad) + EMA in three launches per step.  One parameter group of CUDA fp32 dense tensors.

    ``clip_gradients``: the reference's adaptive clipping, max_norm = 1.5 mean(Q) + 2 std(Q) over the last ``queue_len`` clipped norms
    (seeded with 3000).  ``ema_decay=None`` turns the EMA off; otherwise the k-th completed step applies it when k >= ema_start and
    k % ema_every == 0.  ``state_dict()`` has torch.optim.AdamW's layout plus ``gradnorm_queue`` (newest first, as the reference's Queue)
    and ``ema``."""

    def __init__(self, params: Iterable[Any], lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-12,
                 amsgrad: bool = True, clip_gradients: bool = True, queue_len: int = 50, ema_decay: Optional[float] = 0.9999,
                 ema_every: int = 1, ema_start: int = 0):
        if not 0.0 <= lr:
            raise ValueError(f"invalid learning rate {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid betas {betas}: each must lie in [0, 1)")
        if not 0.0 <= eps or not 0.0 <= weight_decay:
            raise ValueError("eps and weight_decay must be >= 0")
        if not 1 <= int(queue_len) <= QUEUE_MAX:
            raise ValueError(f"queue_len must lie in 1 .. {QUEUE_MAX}")
        if ema_decay is not None and not 0.0 <= ema_decay <= 1.0:
            raise ValueError("EMA decay value must be between 0 and 1")
        if int(ema_every) < 1 or int(ema_start) < 0:
            raise ValueError("ema_every must be >= 1 and ema_start >= 0")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad), maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, clip_gradients=bool(clip_gradients), queue_len=int(queue_len),
                        ema_decay=ema_decay, ema_every=int(ema_every), ema_start=int(ema_start))
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("TrainingUpdate takes one parameter group")
        ps = self.param_groups[0]["params"]
        if not ps:
            raise ValueError("TrainingUpdate got no parameters")
        for i, p in enumerate(ps):
            if not p.is_cuda:
                raise ValueError(f"parameter {i} is not a CUDA tensor ({p.device}): the update runs on the GPU only")
            if p.dtype != torch.float32:
                raise ValueError(f"parameter {i} is {p.dtype}: the update takes fp32 parameters only")
            if p.layout != torch.strided or p.is_sparse:
                raise ValueError(f"parameter {i} is not a dense tensor")
            if not p.is_contiguous():
                raise ValueError(f"parameter {i} is not contiguous")
        if len({p.device for p in ps}) != 1:
            raise ValueError("all parameters must live on one device")
        self._lib = _native.load_ops()
        self._dev = ps[0].device
        self._build()

    # ---- layout ----------------------------------------------------------------------------------------------------------------
    def _build(self):
        ps = self.param_groups[0]["params"]
        T = len(ps)
        self._numel = [p.numel() for p in ps]
        self._offset, o = [], 0
        for n in self._numel:
            self._offset.append(o)
            o += (n + 63) // 64 * 64
        self._total = max(o, 64)
        chunks = []
        for t, n in enumerate(self._numel):
            for s in range(0, n, CHUNK):
                chunks.append((t, s, min(CHUNK, n - s)))
        self._C, self._T = len(chunks), T
        q = self.param_groups[0]["queue_len"]
        off = {w: int(self._lib.gcdm_optim_workspace_bytes(w, T, self._C, q)) for w in range(12)}
        assert min(off.values()) >= 0
        self._off = off
        self._ws = torch.zeros(off[_TOTAL] // 8, dtype=torch.int64, device=self._dev)
        self._state = torch.zeros(4 * self._total, dtype=torch.float32, device=self._dev)
        host = torch.zeros(off[_HOST_END] // 8, dtype=torch.int64)
        host[off[_PTAB] // 8: off[_PTAB] // 8 + T] = torch.tensor([p.data_ptr() for p in ps], dtype=torch.int64)
        host[off[_OTAB] // 8: off[_OTAB] // 8 + T] = torch.tensor(self._offset, dtype=torch.int64)
        host[off[_NTAB] // 8: off[_NTAB] // 8 + T] = torch.tensor(self._numel, dtype=torch.int64)
        host[off[_CTAB] // 8: off[_CTAB] // 8 + 3 * self._C] = torch.tensor(chunks, dtype=torch.int64).reshape(-1)
        self._ws[: off[_HOST_END] // 8].copy_(host)
        self._param_ptrs = [p.data_ptr() for p in ps]
        self._grad_ptrs: Optional[List[int]] = [0] * T
        self._scal_host = torch.zeros(8, dtype=torch.int64).pin_memory()
        self._scal_event = torch.cuda.Event()
        self._scal_pending = False
        self._reset_queue([QUEUE_SEED])
        self._ema_on = False
        if self.param_groups[0]["ema_decay"] is not None:
            self._swap(1)                     # EMA starts as a copy of the weights (EMA.on_train_start)
            self._ema_on = True

    def _view(self, which, dtype, n):
        b = self._off[which]
        return self._ws.view(torch.uint8)[b: b + n * torch.empty((), dtype=dtype).element_size()].view(dtype)

    def _quarter(self, k):
        return self._state[k * self._total: (k + 1) * self._total]

    def _param_view(self, k, t):
        o = self._offset[t]
        return self._quarter(k)[o: o + self._numel[t]].view_as(self.param_groups[0]["params"][t])

    def _scal(self):
        return self._view(_SCAL, torch.int64, 8)

    def _reset_queue(self, items_newest_first: List[float]):
        q = self.param_groups[0]["queue_len"]
        items = list(items_newest_first)[:q][::-1]          # oldest first into slots 0 .. n-1
        ring = torch.zeros(q, dtype=torch.float64)
        ring[: len(items)] = torch.tensor(items, dtype=torch.float64) if items else ring[:0]
        self._view(_QUEUE, torch.float64, q).copy_(ring)
        sc = self._view(_SCAL, torch.int32, 16)
        sc[6] = len(items) % q                               # qhead
        sc[7] = len(items)                                   # qcount

    def _check_params(self):
        ps = self.param_groups[0]["params"]
        if [p.data_ptr() for p in ps] != self._param_ptrs:
            raise RuntimeError("a parameter of TrainingUpdate was re-allocated (e.g. module.to() after construction): build the update again")

    def _grad_pointers(self) -> List[int]:
        """The device pointer of every ``p.grad`` as the kernels take it, 0 where there is none."""
        ps = self.param_groups[0]["params"]
        ptrs = []
        for i, p in enumerate(ps):
            g = p.grad
            if g is None:
                ptrs.append(0)
                continue
            if g.is_sparse or g.dtype != torch.float32 or g.device != self._dev or g.shape != p.shape or not g.is_contiguous():
                raise ValueError(f"gradient of parameter {i} is not a dense contiguous fp32 tensor on {self._dev}")
            ptrs.append(g.data_ptr())
        return ptrs

    def _refresh_grads(self):
        ptrs = self._grad_pointers()
        if ptrs != self._grad_ptrs:
            src = torch.tensor(ptrs, dtype=torch.int64).pin_memory()
            self._view(_GTAB, torch.int64, self._T).copy_(src, non_blocking=True)
            self._grad_ptrs = ptrs

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream)

    def _bump(self):
        torch.autograd.graph.increment_version(list(self.param_groups[0]["params"]))

    def _swap(self, mode: int):
        g = self.param_groups[0]
        st = self._lib.gcdm_optim_ema_swap(C.c_void_p(self._ws.data_ptr()), C.c_void_p(self._state.data_ptr()), self._total, self._T, self._C,
                                           g["queue_len"], mode, self._stream())
        if st != 0:
            raise _native.NativeError(f"gcdm_optim_ema_swap failed ({st})")

    # ---- the step --------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_params()
        self._refresh_grads()
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        ema = g["ema_decay"] is not None
        st = self._lib.gcdm_optim_step(C.c_void_p(self._ws.data_ptr()), C.c_void_p(self._state.data_ptr()), self._total, self._T, self._C,
                                       float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]), int(g["amsgrad"]),
                                       int(g["clip_gradients"]), g["queue_len"], int(ema), float(g["ema_decay"] if ema else 0.0),
                                       g["ema_every"], g["ema_start"], self._stream())
        if st != 0:
            raise _native.NativeError(f"gcdm_optim_step failed ({st})")
        self._bump()
        # the scalar block (norm, flags) follows to pinned memory; read_flags / last_grad_norm look at it when asked
        self._scal_host.copy_(self._scal(), non_blocking=True)
        self._scal_event.record(torch.cuda.current_stream(self._dev))
        self._scal_pending = True
        return loss

    def _host_scal(self):
        if self._scal_pending:
            self._scal_event.synchronize()
            self._scal_pending = False
        return self._scal_host

    def read_flags(self, reset: bool = True) -> int:
        """OR of the GCDM_OPTIM_FLAG_* words of the steps so far (FLAG_NONFINITE: a step was skipped).  Waits for the last step's copy."""
        v = int(self._host_scal().view(torch.int32)[5])
        if reset:
            self._view(_SCAL, torch.int32, 16)[5].zero_()
            self._scal_host.view(torch.int32)[5] = 0
        return v

    def last_grad_norm(self) -> float:
        """The gradient norm of the last step (before clipping).  Waits for the last step's copy."""
        return float(self._host_scal().view(torch.float64)[0])

    def last_clip_coef(self) -> float:
        return float(self._host_scal().view(torch.float32)[4])

    # ---- EMA -------------------------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def ema_weights(self):
        """Swaps the EMA weights into the parameters for the body (evaluate_ema_weights_instead) and back on exit."""
        if not self._ema_on:
            raise RuntimeError("this TrainingUpdate keeps no EMA (ema_decay=None)")
        with torch.no_grad():
            self._swap(0)
            self._bump()
        try:
            yield self
        finally:
            with torch.no_grad():
                self._swap(0)
                self._bump()

    def ema_tensors(self) -> List[torch.Tensor]:
        if not self._ema_on:
            raise RuntimeError("this TrainingUpdate keeps no EMA (ema_decay=None)")
        return [self._param_view(3, t).clone() for t in range(self._T)]

    def ema_state_dict(self, module: torch.nn.Module) -> Dict[str, torch.Tensor]:
        """``module.state_dict()`` with the EMA value of every parameter this update owns (buffers as they are): save it as
        ``{"state_dict": ...}`` to get the reference's ``*-EMA.ckpt``."""
        ema = self.ema_tensors()
        idx = {id(p): t for t, p in enumerate(self.param_groups[0]["params"])}
        out = {}
        for k, v in module.state_dict(keep_vars=True).items():
            t = idx.get(id(v))
            out[k] = ema[t].detach().clone() if t is not None else v.detach().clone()
        return out

    # ---- state (torch.optim.AdamW layout) --------------------------------------------------------------------------------------
    def queue(self) -> List[float]:
        """The gradient-norm queue, newest first (the reference's Queue.items)."""
        g = self.param_groups[0]
        sc = self._host_scal_sync()
        head, count = int(sc.view(torch.int32)[6]), int(sc.view(torch.int32)[7])
        ring = self._view(_QUEUE, torch.float64, g["queue_len"]).cpu().tolist()
        return [ring[(head - 1 - i) % g["queue_len"]] for i in range(count)]

    def _host_scal_sync(self):
        return self._scal().cpu()

    def steps(self) -> List[int]:
        return self._view(_STEPS, torch.int64, self._T).cpu().tolist()

    def state_dict(self) -> Dict[str, Any]:
        g = self.param_groups[0]
        steps = self.steps()
        state = {}
        for t in range(self._T):
            if steps[t] == 0:
                continue
            s = {"step": torch.tensor(float(steps[t]), dtype=torch.float32), "exp_avg": self._param_view(0, t).clone(),
                 "exp_avg_sq": self._param_view(1, t).clone()}
            if g["amsgrad"]:
                s["max_exp_avg_sq"] = self._param_view(2, t).clone()
            state[t] = s
        group = {k: v for k, v in g.items() if k != "params"}
        group["params"] = list(range(self._T))
        return {"state": state, "param_groups": [group], "gradnorm_queue": self.queue(), "global_step": int(self._host_scal_sync()[4]),
                "ema": self.ema_tensors() if self._ema_on else None}

    @torch.no_grad()
    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        """Takes a TrainingUpdate or torch.optim.AdamW state dict.  Without ``gradnorm_queue`` the queue is reseeded; without ``ema`` the
        EMA restarts from the current weights."""
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != self._T:
            raise ValueError("state dict does not match: TrainingUpdate has one group of "
                             f"{self._T} parameters")
        g = self.param_groups[0]
        for k in ("lr", "betas", "eps", "weight_decay", "amsgrad"):
            if k in groups[0]:
                g[k] = tuple(groups[0][k]) if k == "betas" else groups[0][k]
        g["amsgrad"] = bool(g["amsgrad"])
        ids = list(groups[0]["params"])
        steps = [0] * self._T
        for k in range(3):
            self._quarter(k).zero_()
        for t, pid in enumerate(ids):
            s = state_dict["state"].get(pid)
            if s is None:
                continue
            steps[t] = int(float(s["step"]))
            self._param_view(0, t).copy_(s["exp_avg"])
            self._param_view(1, t).copy_(s["exp_avg_sq"])
            if "max_exp_avg_sq" in s:
                self._param_view(2, t).copy_(s["max_exp_avg_sq"])
        self._view(_STEPS, torch.int64, self._T).copy_(torch.tensor(steps, dtype=torch.int64))
        self._reset_queue(state_dict.get("gradnorm_queue") or [QUEUE_SEED])
        self._scal()[4] = int(state_dict.get("global_step", max(steps)))
        ema = state_dict.get("ema")
        if self._ema_on:
            if ema is not None:
                for t in range(self._T):
                    self._param_view(3, t).copy_(ema[t])
            else:
                self._swap(1)


class BucketedUpdate:
    """Data-parallel and accumulated training steps on one flat gradient bucket (include/gcdm_grad_bucket.h), around an unchanged
    ``TrainingUpdate``.  Opt-in: nothing here runs unless it is constructed.

        upd = model.configure_data_parallel(group=None, accumulate_grad_batches=k)
        for micro_batch in ...:
            model.training_step(micro_batch)["loss"].backward(); upd.accumulate(); upd.zero_grad()
            # after every k-th micro-batch:
            upd.step()

    ``accumulate()`` adds ``p.grad / (world * accumulate_grad_batches)`` of every parameter to the bucket in one launch; ``step()`` sums the
    bucket over the ranks of ``group`` with one ``all_reduce`` (none without an initialised process group, or with one rank), checks that the
    ranks agree on which tensors have a gradient, and lets the wrapped update take its step on the bucket: the clipping norm is the norm of
    the averaged gradient, as under the reference's DDP strategy, so every rank pushes the same value onto its queue and the replicas stay
    bit-identical.  The reduce is not overlapped with the backward pass, and no multi-GPU scaling has been measured.

    Loss semantics are DDP's and Lightning's: each micro-batch of each rank contributes the gradient of its own ``nll.mean(0)``, and the
    step sees the mean of those means.  With shards or micro-batches of unequal size that is not the mean over all molecules -- exactly as
    in the reference.

    When the ranks disagree on a tensor's presence (one has a gradient, another has none) the step is skipped as a whole on every rank and
    ``read_flags()`` carries ``FLAG_MISMATCH`` (together with ``FLAG_NONFINITE``, the mechanism of the skip).  A tensor counts as present on
    this rank when any of the step's passes had a gradient for it.  Everything else -- ``zero_grad``, ``param_groups``, ``queue``,
    ``ema_weights`` ... -- is the wrapped update's."""

    def __init__(self, update: TrainingUpdate, group=None, accumulate_grad_batches: int = 1):
        if not isinstance(update, TrainingUpdate):
            raise TypeError("BucketedUpdate wraps an optim.TrainingUpdate")
        if int(accumulate_grad_batches) != accumulate_grad_batches or int(accumulate_grad_batches) < 1:
            raise ValueError(f"accumulate_grad_batches must be an integer >= 1, got {accumulate_grad_batches!r}")
        self.update = update
        self.group = group
        self.accumulate_grad_batches = int(accumulate_grad_batches)
        self._passes = 0
        self._bucket: Optional[torch.Tensor] = None

    def __getattr__(self, name):
        if name == "update":
            raise AttributeError(name)
        return getattr(self.update, name)

    # ---- the bucket ------------------------------------------------------------------------------------------------------------
    def _world(self) -> int:
        import torch.distributed as dist
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def _alloc(self):
        u = self.update
        n = int(u._lib.gcdm_grad_bucket_floats(u._total, u._T))
        assert n >= u._total + u._T
        self._bucket = torch.empty(n, dtype=torch.float32, device=u._dev)
        assert self._bucket.data_ptr() % 256 == 0
        self._gtab = torch.zeros(u._T, dtype=torch.int64, device=u._dev)
        self._ptrs: Optional[List[int]] = None
        self._have = [False] * u._T                  # tensors with a gradient in a pass of the current step
        self._views: List[Optional[torch.Tensor]] = [None] * u._T

    @property
    def bucket(self) -> torch.Tensor:
        """The flat bucket: ``total`` values laid out like a state quarter of the update, then the presence tail.  Before ``step()`` it holds
        this rank's scaled sum, after it the sum over the ranks."""
        if self._bucket is None:
            self._alloc()
        return self._bucket

    def _call(self, name, *args):
        st = getattr(self.update._lib, name)(*args)
        if st != 0:
            raise _native.NativeError(f"{name} failed ({st})")

    @torch.no_grad()
    def accumulate(self) -> None:
        """After each micro-batch's ``backward()``: one launch, no host sync."""
        if self._passes >= self.accumulate_grad_batches:
            raise RuntimeError(f"accumulate() was called {self._passes} times with accumulate_grad_batches={self.accumulate_grad_batches}: step() is due")
        u = self.update
        bucket = self.bucket
        u._check_params()
        ptrs = u._grad_pointers()
        if ptrs != self._ptrs:
            self._gtab.copy_(torch.tensor(ptrs, dtype=torch.int64).pin_memory(), non_blocking=True)
            self._ptrs = ptrs
        first = self._passes == 0
        self._have = [p != 0 or (h and not first) for p, h in zip(ptrs, self._have)]
        scale = 1.0 / (self._world() * self.accumulate_grad_batches)
        self._call("gcdm_grad_bucket_pack", C.c_void_p(u._ws.data_ptr()), C.c_void_p(self._gtab.data_ptr()), C.c_void_p(bucket.data_ptr()),
                   u._total, u._T, u._C, u.param_groups[0]["queue_len"], scale, int(first), u._stream())
        self._passes += 1

    @torch.no_grad()
    def step(self, closure=None):
        """All-reduce, presence check, then ``TrainingUpdate.step()`` reading its gradients from the bucket (``p.grad`` is left as it was)."""
        if closure is not None:
            raise ValueError("BucketedUpdate.step takes no closure: run the passes and accumulate() yourself")
        if self._passes < self.accumulate_grad_batches:
            raise RuntimeError(f"step() after {self._passes} of {self.accumulate_grad_batches} accumulate() calls")
        u = self.update
        world = self._world()
        if world > 1:
            import torch.distributed as dist
            dist.all_reduce(self._bucket, op=dist.ReduceOp.SUM, group=self.group)
        self._call("gcdm_grad_bucket_check", C.c_void_p(u._ws.data_ptr()), C.c_void_p(self._bucket.data_ptr()), u._total, u._T, u._C,
                   u.param_groups[0]["queue_len"], world, u._stream())
        # the update reads p.grad: for the length of its step that is the tensor's segment of the bucket.  Its gradient table (section 2) is
        # thereby written once, and again only when the set of present tensors changes
        ps = u.param_groups[0]["params"]
        saved = [p.grad for p in ps]
        try:
            for t, p in enumerate(ps):
                if self._have[t]:
                    if self._views[t] is None:
                        o = u._offset[t]
                        self._views[t] = self._bucket[o: o + u._numel[t]].view_as(p)
                    p.grad = self._views[t]
                else:
                    p.grad = None
            u.step()
        finally:
            for p, g in zip(ps, saved):
                p.grad = g
        self._passes = 0

    def read_flags(self, reset: bool = True) -> int:
        """The wrapped update's flag word: FLAG_NONFINITE (a step was skipped) and FLAG_MISMATCH (it was skipped because the ranks disagreed
        on which tensors have a gradient)."""
        return self.update.read_flags(reset)

    def state_dict(self) -> Dict[str, Any]:
        return self.update.state_dict()

    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        self.update.load_state_dict(state_dict)
