"""gcdm_optim_workspace_bytes / gcdm_optim_step / gcdm_optim_ema_swap (include/gcdm_optim.h) called directly through the C ABI on an MI355X,
against optim_ref.RefUpdate in fp64 -- never optim.TrainingUpdate: the workspace table is written here by hand from the header.

Harness (_Dev): every parameter, every gradient, the 4 x total state and the workspace lie inside larger device buffers whose every other word
is a guard pattern (a quiet NaN with a payload for floats, 0xA5 bytes round the workspace and in the padding of its sections); the padding
between tensors inside each state quarter and the unused ring slots carry such patterns too.  After every call all of it is read back and
the guards, the padding, the gradients and the caller-written sections 1 to 5 of the workspace must be bitwise as they were.  A read of a
guard poisons the result, a write to one no longer compares equal.  Pointers are placed 0 to 3 floats past a 16-byte boundary as the case
asks, so the scalar fallbacks of k_opt_sqnorm / k_opt_update and the tails after their float4 bodies run.

The cases, their bars and what each asserts are in tests/optim_cases.py; the same code runs on the CPU against optim_ref.Emu32, where each of
Emu32.MUTANTS is shown to be rejected (tests/test_optim_cpu.py).  Every test prints its worst d / bar per quantity ("MEASURED ...").

The mutants of the library this file is meant to catch, and the figures measured so far: DESIGN.md 3.6, "Fused training update"."""
import ctypes as C
import importlib
import struct

import numpy as np
import pytest
import torch

import optim_cases as K

pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                         # guard floats round every buffer (256 bytes round the workspace)
WS_GUARD = 0xA5
TSCAL_BITS = 0x7FF80000000BEEF5    # the caller's pattern in tscal, which the kernels write before they read


def _lib():
    lib = native.load_ops()
    assert set(native.OPTIM_SIGNATURES) == {"gcdm_optim_workspace_bytes", "gcdm_optim_step", "gcdm_optim_ema_swap"}
    assert native.OPTIM_RESTYPES["gcdm_optim_workspace_bytes"] is C.c_int64
    return lib


def _place(sizes, mis):
    """Float offsets of the items in one buffer: item i starts mis[i] floats past a 16-byte boundary, GUARD or more guard floats round each."""
    pos, starts = GUARD, []
    for n, k in zip(sizes, mis):
        pos = (pos + 3) // 4 * 4 + k
        starts.append(pos)
        pos += n + GUARD
    return starts, pos + 4


def _upload(host):
    dev = torch.from_numpy(host).to(DEV)
    assert dev.data_ptr() % 256 == 0
    return dev


class _Dev:
    """A runner of optim_cases on the device: builds the header's buffers for a Spec, calls the C entries, reads everything back."""

    def __init__(self, spec):
        self.spec, self.lib = spec, _lib()
        h = spec.hyp
        T, Cn, Q = len(spec.numels), len(spec.chunks), h["queue_len"]
        self.T, self.C, self.Q = T, Cn, Q
        off = [int(self.lib.gcdm_optim_workspace_bytes(w, T, Cn, Q)) for w in range(12)]
        assert off[1] == 0 and all(o % 256 == 0 for o in off) and sorted(off[1:]) == off[1:] and off[0] > off[11]
        self.off = off
        pad = K.pad_value()
        # parameters
        self.p_starts, n = _place(spec.numels, spec.p_mis)
        self.p_guard = np.full(n, pad, dtype=np.float32)
        host = self.p_guard.copy()
        self.p_mask = np.ones(n, dtype=bool)
        for s, p in zip(self.p_starts, spec.p0):
            host[s:s + p.size] = p
            self.p_mask[s:s + p.size] = False
        self.p_dev = _upload(host)
        # gradients: written before every step
        self.g_starts, n = _place(spec.numels, spec.g_mis)
        self.g_host = np.full(n, pad, dtype=np.float32)
        self.g_dev = _upload(self.g_host)
        # the state
        self.s_start = GUARD + spec.state_mis
        host = np.full(4 * spec.total + 2 * GUARD + 4, pad, dtype=np.float32)
        host[self.s_start: self.s_start + 4 * spec.total] = spec.state0().reshape(-1)
        self.s_mask = np.ones(host.size, dtype=bool)
        self.s_mask[self.s_start: self.s_start + 4 * spec.total] = False
        self.s_dev = _upload(host)
        # the workspace, section by section as the header lists them
        ws = np.full(off[0] + 512, WS_GUARD, dtype=np.uint8)
        self.sizes = {1: 8 * T, 2: 8 * T, 3: 8 * T, 4: 8 * T, 5: 24 * Cn, 7: 8 * T, 8: 16 * T, 9: 4 * Cn, 10: 8 * Q, 11: 64}

        def put(which, arr):
            b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
            assert b.size == self.sizes[which]
            ws[256 + off[which]: 256 + off[which] + b.size] = b

        put(1, np.array([self.p_dev.data_ptr() + 4 * s for s in self.p_starts], dtype=np.int64))
        put(2, np.zeros(T, dtype=np.int64))
        put(3, np.array(spec.offsets, dtype=np.int64))
        put(4, np.array(spec.numels, dtype=np.int64))
        put(5, np.array(spec.chunks, dtype=np.int64).reshape(-1))
        put(7, np.zeros(T, dtype=np.int64))
        put(8, np.full(2 * T, TSCAL_BITS, dtype=np.uint64))
        put(9, np.full(Cn, pad, dtype=np.float32))
        put(10, spec.ring0)
        scal = bytearray(64)
        struct.pack_into("<ii", scal, 24, spec.qhead, spec.qcount)
        put(11, np.frombuffer(bytes(scal), dtype=np.uint8))
        self.ws_host = ws                                   # kept in step with what the caller writes (the gradient pointers)
        self.ws_dev = _upload(ws)
        self.ws_mask = np.ones(ws.size, dtype=bool)         # guards and section padding
        for w, n in self.sizes.items():
            self.ws_mask[256 + off[w]: 256 + off[w] + n] = False
        self.ws_ptr = C.c_void_p(self.ws_dev.data_ptr() + 256)
        self.s_ptr = C.c_void_p(self.s_dev.data_ptr() + 4 * self.s_start)
        assert (self.s_dev.data_ptr() // 4 + self.s_start) % 4 == spec.state_mis
        for t in range(T):
            assert (self.p_dev.data_ptr() // 4 + self.p_starts[t]) % 4 == spec.p_mis[t] and (self.g_dev.data_ptr() // 4 + self.g_starts[t]) % 4 == spec.g_mis[t]

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def snap(self):
        """Reads everything back, checks every guard and returns what the header lets a caller see."""
        torch.cuda.synchronize()
        spec, off = self.spec, self.off
        p, g, s, ws = (x.cpu().numpy() for x in (self.p_dev, self.g_dev, self.s_dev, self.ws_dev))
        assert K.same_bits(p[self.p_mask], self.p_guard[self.p_mask]), "write outside a parameter"
        assert K.same_bits(g, self.g_host), "a gradient buffer or its guards changed"
        assert K.same_bits(s[self.s_mask], np.full(int(self.s_mask.sum()), K.pad_value(), dtype=np.float32)), "write outside the state"
        assert (ws[self.ws_mask] == WS_GUARD).all(), "write outside the workspace or into the padding of a section"
        host_end = 256 + off[6]
        assert (ws[256:host_end] == self.ws_host[256:host_end]).all(), "a caller-written section of the workspace changed"
        sec = lambda w, dt: ws[256 + off[w]: 256 + off[w] + self.sizes[w]].view(dt).copy()          # noqa: E731
        norm, max_norm, coef, flags, qhead, qcount, gstep, skipped, ema_applied = struct.unpack_from("<ddfiiiqii", sec(11, np.uint8).tobytes(), 0)
        out = K.Snap(spec, p=[p[a:a + n].copy() for a, n in zip(self.p_starts, spec.numels)],
                     state=s[self.s_start: self.s_start + 4 * spec.total].reshape(4, spec.total).copy(), steps=sec(7, np.int64),
                     tscal=sec(8, np.float64).reshape(self.T, 2), ring=sec(10, np.float64), norm=norm, max_norm=max_norm, coef=coef, flags=flags,
                     qhead=qhead, qcount=qcount, gstep=gstep, skipped=skipped, ema_applied=ema_applied)
        out.dev = ws[256 + off[7]: 256 + off[0]].tobytes()
        return out

    def step(self, grads):
        spec, h = self.spec, self.spec.hyp
        self.g_host[:] = K.pad_value()
        ptrs = np.zeros(self.T, dtype=np.int64)
        for t, g in enumerate(grads):
            if g is not None:
                assert g.dtype == np.float32 and g.size == spec.numels[t]
                self.g_host[self.g_starts[t]: self.g_starts[t] + g.size] = g
                ptrs[t] = self.g_dev.data_ptr() + 4 * self.g_starts[t]
        self.g_dev.copy_(torch.from_numpy(self.g_host))
        a = 256 + self.off[2]
        self.ws_host[a: a + 8 * self.T] = ptrs.view(np.uint8)
        self.ws_dev[a: a + 8 * self.T].copy_(torch.from_numpy(self.ws_host[a: a + 8 * self.T]))
        st = self.lib.gcdm_optim_step(self.ws_ptr, self.s_ptr, spec.total, self.T, self.C, h["lr"], h["betas"][0], h["betas"][1], h["eps"],
                                      h["weight_decay"], int(h["amsgrad"]), int(h["clip"]), self.Q, int(h["ema"]), h["ema_decay"], h["ema_every"],
                                      h["ema_start"], self._stream())
        assert st == 0
        return self.snap()

    def swap(self, mode):
        st = self.lib.gcdm_optim_ema_swap(self.ws_ptr, self.s_ptr, self.spec.total, self.T, self.C, self.Q, mode, self._stream())
        assert st == 0
        return self.snap()

    def clear_flags(self):
        a = 256 + self.off[11] + 20
        self.ws_dev[a: a + 4].zero_()


@pytest.mark.parametrize("clip", [False, True])
def test_alignment_and_layout_give_the_same_bits(clip):
    K.case_layouts(_Dev, clip)


def test_intermittent_gradients():
    K.case_intermittent(_Dev)


@pytest.mark.parametrize("every,start,nonfinite", [(1, 0, False), (3, 0, False), (2, 5, False), (4, 4, False), (3, 0, True)])
def test_ema_schedule(every, start, nonfinite):
    K.case_ema_schedule(_Dev, every, start, nonfinite)


@pytest.mark.parametrize("which", ["vmax", "ema"])
def test_untouched_quarters(which):
    K.case_untouched(_Dev, which)


def test_swap_modes():
    K.case_swap(_Dev)


@pytest.mark.parametrize("kind", list(K.QUEUES))
def test_queue(kind):
    K.case_queue(_Dev, kind)


@pytest.mark.parametrize("which", list(K.LIMITS))
def test_hyperparameter_limits(which):
    K.case_limits(_Dev, which)


@pytest.mark.parametrize("kind", ["nan_tail", "inf_chunk4"])
def test_nonfinite_skip_under_the_guards(kind):
    K.case_nonfinite(_Dev, kind)


def test_more_than_256_tensors_and_chunks():
    K.case_many_tensors(_Dev)


def test_two_runs_give_the_same_bits():
    a, b = K.case_intermittent(_Dev), K.case_intermittent(_Dev)
    assert all(K.same_bits(x, y) for x, y in zip(a.p, b.p)) and K.same_bits(a.state, b.state)
    assert a.dev == b.dev, "the device-owned sections of the workspace differ between two runs"
