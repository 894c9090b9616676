"""gcdm_grad_bucket_floats / gcdm_grad_bucket_pack / gcdm_grad_bucket_check (include/gcdm_grad_bucket.h) called directly through the C ABI on
an MI355X, against the numpy float32 restatement of tests/grad_bucket_cases.py bit for bit -- never optim.BucketedUpdate.

Harness: the optimiser workspace, parameters, state and gradients are those of tests/test_optim_cabi_gpu.py (_Dev: guard words round every
buffer, sections 1 to 5 of the workspace and the gradients compared bitwise after every call); the tensors are optim_cases.NUMELS with both
chunk tables and the misaligned placements of optim_cases.PLACEMENTS.  The bucket lies at exactly its advertised size between 64 guard words
and starts as quiet NaNs with the payload PAD_BITS, so a float the pack leaves undefined, or reads on a first pass, shows.

Where a step of the update is compared with a step "fed the original gradients", those are handed to it at aligned pointers: k_opt_sqnorm sums
a chunk in float4 lanes at an aligned pointer and element by element otherwise, the two orders round differently, and a gradient read from
the bucket is always aligned.  The pack's own sources take every placement."""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_bucket_cases as G
import optim_cases as K
import test_optim_cabi_gpu as OC

native = OC.native
pytestmark = pytest.mark.gpu
DEV = OC.DEV
GUARD = OC.GUARD
MISMATCH, NONFINITE = native.GRAD_BUCKET_FLAG_MISMATCH, native.OPTIM_FLAG_NONFINITE
PAD = np.uint32(K.PAD_BITS)


class _Bucket:
    """`n` floats on the device between GUARD guard words, all of it the NaN pattern."""

    def __init__(self, n):
        self.n = n
        self.dev = OC._upload(np.full(n + 2 * GUARD, K.pad_value(), dtype=np.float32))
        self.addr = self.dev.data_ptr() + 4 * GUARD
        assert self.addr % 256 == 0
        self.ptr = C.c_void_p(self.addr)

    def inner(self):
        return self.dev[GUARD: GUARD + self.n]

    def read(self):
        torch.cuda.synchronize()
        a = self.dev.cpu().numpy()
        assert (K.bits(a[:GUARD]) == PAD).all() and (K.bits(a[GUARD + self.n:]) == PAD).all(), "write outside the bucket"
        return a[GUARD: GUARD + self.n].copy()


class _BDev(OC._Dev):
    """The optimiser harness plus buckets: pack / check through the C ABI, and a step whose gradient table points into a bucket."""

    def __init__(self, spec):
        super().__init__(spec)
        for name, sig in native.GRAD_BUCKET_SIGNATURES.items():
            assert getattr(self.lib, name).argtypes == sig
        self.nb = int(self.lib.gcdm_grad_bucket_floats(spec.total, self.T))
        assert self.nb == G.bucket_floats(spec.total, self.T)
        self.gtab = torch.zeros(self.T, dtype=torch.int64, device=DEV)

    def bucket(self):
        return _Bucket(self.nb)

    def emu(self):
        return np.full(self.nb, K.pad_value(), dtype=np.float32)

    def put_grads(self, grads):
        spec = self.spec
        self.g_host[:] = K.pad_value()
        ptrs = np.zeros(self.T, dtype=np.int64)
        for t, g in enumerate(grads):
            if g is not None:
                assert g.dtype == np.float32 and g.size == spec.numels[t]
                self.g_host[self.g_starts[t]: self.g_starts[t] + g.size] = g
                ptrs[t] = self.g_dev.data_ptr() + 4 * self.g_starts[t]
        self.g_dev.copy_(torch.from_numpy(self.g_host))
        return ptrs

    def pack(self, bucket, grads, scale, first, emu=None):
        self.gtab.copy_(torch.from_numpy(self.put_grads(grads)))
        st = self.lib.gcdm_grad_bucket_pack(self.ws_ptr, C.c_void_p(self.gtab.data_ptr()), bucket.ptr, self.spec.total, self.T, self.C, self.Q,
                                            float(scale), int(first), self._stream())
        assert st == 0
        if emu is not None:
            G.emu_pack(emu, self.spec.offsets, self.spec.numels, self.spec.total, grads, scale, first)

    def check(self, bucket, world):
        st = self.lib.gcdm_grad_bucket_check(self.ws_ptr, bucket.ptr, self.spec.total, self.T, self.C, self.Q, world, self._stream())
        assert st == 0

    def step_bucket(self, bucket, have):
        """gcdm_optim_step with section 2 pointing at bucket + offset[t] for the tensors of `have`."""
        spec, h = self.spec, self.spec.hyp
        ptrs = np.array([bucket.addr + 4 * o if hv else 0 for o, hv in zip(spec.offsets, have)], dtype=np.int64)
        a = 256 + self.off[2]
        self.ws_host[a: a + 8 * self.T] = ptrs.view(np.uint8)
        self.ws_dev[a: a + 8 * self.T].copy_(torch.from_numpy(self.ws_host[a: a + 8 * self.T]))
        st = self.lib.gcdm_optim_step(self.ws_ptr, self.s_ptr, spec.total, self.T, self.C, h["lr"], h["betas"][0], h["betas"][1], h["eps"],
                                      h["weight_decay"], int(h["amsgrad"]), int(h["clip"]), self.Q, int(h["ema"]), h["ema_decay"], h["ema_every"],
                                      h["ema_start"], self._stream())
        assert st == 0
        return self.snap()


def _same(a, b, what=""):
    assert K.same_bits(a, b), (what, int((K.bits(a) != K.bits(b)).sum()), int(np.flatnonzero(K.bits(a) != K.bits(b))[0]))


def _parts(spec, bucket):
    T = len(spec.numels)
    return bucket[:spec.total], bucket[spec.total: spec.total + T], bucket[spec.total + T:]


def _snap_same(a, b):
    """Two snapshots hold the same bits: parameters, every state quarter, and the device-owned workspace (step counts, tscal, partial sums,
    the ring, the scalar block)."""
    K.same_tensors(a, b)
    assert all(K.same_bits(x, y) for x, y in zip(a.p, b.p))
    assert K.same_bits(a.steps, b.steps) and K.same_bits(a.ring, b.ring) and K.same_bits(a.tscal, b.tscal)
    sa, sb = ((s.norm, s.max_norm, s.coef, s.flags, s.qhead, s.qcount, s.gstep, s.skipped, s.ema_applied) for s in (a, b))
    assert sa == sb, (sa, sb)
    assert a.dev == b.dev


# ---- 1. first pass at scale 1: a copy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", range(len(K.PLACEMENTS)))
def test_first_pass_at_scale_one_copies_the_bits_and_defines_every_float(place):
    spec = K.Spec(**K.PLACEMENTS[place])
    r = _BDev(spec)
    before = r.snap()
    have = K.have_pattern(2)                              # tensor 3 (5 values) and tensor 6 (65 values) absent
    grads = K.grads(spec, 1, have=have)
    for g in grads:
        if g is not None:
            G.special_values(g)
    b, emu = r.bucket(), r.emu()
    r.pack(b, grads, 1.0, 1, emu)
    got = b.read()
    values, pres, tail_pad = _parts(spec, got)
    for t, (o, n) in enumerate(zip(spec.offsets, spec.numels)):
        if have[t]:
            _same(values[o:o + n], grads[t], ("tensor", t))
        else:
            assert (K.bits(values[o:o + n]) == 0).all(), ("absent tensor is not +0.0", t)
    assert (K.bits(values[spec.pad_mask()]) == 0).all(), "padding is not +0.0"
    assert pres.tolist() == [1.0 if h else 0.0 for h in have] and (K.bits(tail_pad) == 0).all()
    _same(got, emu, "emulation")
    assert any((K.bits(g) == 0x80000000).any() for g in grads if g is not None) and (K.bits(values) == 0x00000001).any()
    after = r.snap()                                      # guards, gradients, sections 1 - 5 bitwise (asserted inside), and nothing else moved
    _snap_same(before, after)


# ---- 2. accumulation at scales that round ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", [0, 3, 5, 10, 11])
@pytest.mark.parametrize("scale", [1 / 2, 1 / 3, 1 / 6])
def test_three_passes_match_the_float32_emulation_bitwise(scale, place):
    """Passes with have_pattern(4), (5), (6): tensor 8 on the first and third, tensor 6 on the second only, tensor 3 never."""
    spec = K.Spec(**K.PLACEMENTS[place])
    r = _BDev(spec)
    b, emu = r.bucket(), r.emu()
    union = [False] * len(spec.numels)
    for i, step in enumerate((4, 5, 6)):
        have = K.have_pattern(step)
        grads = K.grads(spec, step, have=have)
        if i == 1:
            for g in grads:
                if g is not None:
                    G.special_values(g)
        r.pack(b, grads, scale, int(i == 0), emu)
        union = [u or h for u, h in zip(union, have)]
        got = b.read()
        _same(got, emu, ("pass", i))
        assert _parts(spec, got)[1].tolist() == [1.0 if u else 0.0 for u in union]
    assert union[6] and union[8] and not union[3]
    o, n = spec.offsets[3], spec.numels[3]
    assert (K.bits(got[o:o + n]) == 0).all() and (K.bits(got[:spec.total][spec.pad_mask()]) == 0).all()
    r.snap()


# ---- 3. two simulated ranks --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", [0, 11])
def test_the_sum_of_two_ranks_buckets_equals_one_accumulated_bucket(place):
    spec = K.Spec(**K.PLACEMENTS[place])
    r = _BDev(spec)
    have = [t != 3 for t in range(len(spec.numels))]
    g0, g1 = K.grads(spec, 1, have=have), K.grads(spec, 2, have=have)
    A, B, acc = r.bucket(), r.bucket(), r.bucket()
    r.pack(A, g0, 0.5, 1)
    r.pack(B, g1, 0.5, 1)
    r.pack(acc, g0, 0.5, 1)
    r.pack(acc, g1, 0.5, 0)
    A.inner().copy_(A.inner() + B.inner())               # what the all-reduce leaves on every rank (torch fp32)
    summed, one = A.read(), acc.read()
    _same(summed[:spec.total], one[:spec.total], "values")
    assert _parts(spec, summed)[1].tolist() == [2.0 if h else 0.0 for h in have] == [2 * p for p in _parts(spec, one)[1].tolist()]
    before = r.snap()
    r.check(A, 2)
    _same(A.read(), summed, "check changed a consistent bucket")
    after = r.snap()
    assert after.flags == 0
    _snap_same(before, after)
    r.check(acc, 1)                                       # world 1 with its own consistent tail
    _same(acc.read(), one)
    assert r.snap().flags == 0


# ---- 4. the bucket feeds the update ------------------------------------------------------------------------------------------------------------------
CLIP = dict(clip=True, queue_len=3, ring=(10.0,))
CLIP_SCALES = [1, 3, 1]                                   # norms about 12.5, 37, 12.5 against thresholds 15, 15.x: the second step clips


@pytest.mark.parametrize("place", [0, 3, 5, 11])
def test_a_step_on_the_bucket_equals_a_step_on_the_gradients(place):
    pl = dict(K.PLACEMENTS[place])
    aligned = {k: v for k, v in pl.items() if k != "g_mis"}
    ref, r = OC._Dev(K.Spec(**aligned, **CLIP)), _BDev(K.Spec(**pl, **CLIP))
    b = r.bucket()
    coefs = []
    for step, sc in enumerate(CLIP_SCALES, 1):
        have = K.have_pattern(step)
        grads = K.grads(r.spec, step, scale=0.05 * sc, have=have)
        want = ref.step(grads)
        r.pack(b, grads, 1.0, 1)
        r.check(b, 1)
        got = r.step_bucket(b, have)
        _snap_same(want, got)
        K.check_padding(got)
        coefs.append(got.coef)
    assert coefs[1] < 1.0 and got.gstep == 3 and got.flags == 0, coefs


# ---- 5. presence mismatch ----------------------------------------------------------------------------------------------------------------------------
def test_a_presence_mismatch_skips_the_step_and_raises_the_flag():
    spec = K.Spec(chunking="B", g_mis=1, **CLIP)
    r = _BDev(spec)
    b = r.bucket()
    T = len(spec.numels)
    have = [t != 3 for t in range(T)]
    g = K.grads(spec, 1, have=have)
    r.pack(b, g, 1.0, 1)
    r.check(b, 1)
    before = r.step_bucket(b, have)                       # moments and the queue hold real values
    assert before.gstep == 1 and before.flags == 0
    # the reduced tail of two ranks: 0 for tensor 3 (neither), 1 for tensor 8 (one of them), 2 for the rest
    r.pack(b, K.grads(spec, 2, have=have), 0.5, 1)
    tail = torch.tensor([0.0 if t == 3 else 1.0 if t == 8 else 2.0 for t in range(T)], device=DEV)
    b.inner()[spec.total: spec.total + T].copy_(tail)
    r.check(b, 2)
    poisoned = b.read()
    assert all(np.isnan(poisoned[o]) for o, n in zip(spec.offsets, spec.numels)) and _parts(spec, poisoned)[1].tolist() == tail.tolist()
    assert r.snap().flags == MISMATCH
    snap = r.step_bucket(b, have)
    assert snap.flags == MISMATCH | NONFINITE and snap.skipped == 1 and snap.ema_applied == 0
    assert all(K.same_bits(x, y) for x, y in zip(snap.p, before.p)) and K.same_bits(snap.state, before.state)
    assert K.same_bits(snap.steps, before.steps) and K.same_bits(snap.ring, before.ring)
    assert (snap.qhead, snap.qcount, snap.gstep) == (before.qhead, before.qcount, before.gstep)
    K.check_padding(snap)
    # a consistent next step proceeds
    r.clear_flags()
    r.pack(b, K.grads(spec, 3, have=have), 0.5, 1)
    b.inner()[spec.total: spec.total + T].mul_(2.0)
    r.check(b, 2)
    after = r.step_bucket(b, have)
    assert after.flags == 0 and after.skipped == 0 and after.gstep == 2 and after.qcount == before.qcount + 1
    assert after.steps.tolist() == [0 if t == 3 else 2 for t in range(T)] and not K.same_bits(after.p[0], before.p[0])


# ---- 6. a non-finite gradient on one rank ------------------------------------------------------------------------------------------------------------
def test_an_inf_on_one_rank_skips_the_step_on_the_summed_bucket():
    spec = K.Spec(chunking="B", g_mis=[0, 1, 2, 3] * 3, **CLIP)
    r = _BDev(spec)
    A, B = r.bucket(), r.bucket()
    T = len(spec.numels)
    have = [True] * T
    r.pack(A, K.grads(spec, 1), 1.0, 1)
    r.check(A, 1)
    before = r.step_bucket(A, have)
    g0, g1 = K.grads(spec, 2), K.grads(spec, 3)
    g1[9][77] = np.inf
    r.pack(A, g0, 0.5, 1)
    r.pack(B, g1, 0.5, 1)
    A.inner().copy_(A.inner() + B.inner())
    r.check(A, 2)
    assert r.snap().flags == 0 and np.isinf(A.read()[spec.offsets[9] + 77])
    snap = r.step_bucket(A, have)
    assert snap.flags == NONFINITE and snap.skipped == 1
    assert all(K.same_bits(x, y) for x, y in zip(snap.p, before.p)) and K.same_bits(snap.state, before.state)
    assert K.same_bits(snap.steps, before.steps) and K.same_bits(snap.ring, before.ring)
    assert (snap.qhead, snap.qcount, snap.gstep) == (before.qhead, before.qcount, before.gstep)


# ---- 7. determinism, and another stream --------------------------------------------------------------------------------------------------------------
def _three_passes_and_a_step():
    spec = K.Spec(chunking="B", g_mis=3, p_mis=1, **CLIP)
    r = _BDev(spec)
    b = r.bucket()
    union = [False] * len(spec.numels)
    for i, step in enumerate((4, 5, 6)):
        have = K.have_pattern(step)
        r.pack(b, K.grads(spec, step, have=have), 1 / 3, int(i == 0))
        union = [u or h for u, h in zip(union, have)]
    r.check(b, 1)
    return b.read(), r.step_bucket(b, union)


def test_two_runs_and_a_side_stream_give_the_same_bits():
    a_bucket, a = _three_passes_and_a_step()
    b_bucket, b = _three_passes_and_a_step()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        c_bucket, c = _three_passes_and_a_step()
    for bucket, snap in ((b_bucket, b), (c_bucket, c)):
        _same(a_bucket, bucket)
        _snap_same(a, snap)
    assert a.gstep == 1 and a.flags == 0
