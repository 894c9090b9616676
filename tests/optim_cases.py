"""The edge cases of the fused training update (include/gcdm_optim.h), written once against a small runner interface so that the same
checks run on the CPU against optim_ref.Emu32 (tests/test_optim_cpu.py: a correct fp32 evaluation stays inside every bar, each mutant of
Emu32.MUTANTS is rejected) and on an MI355X against the library's C entries (tests/test_optim_cabi_gpu.py).

A runner is built from a Spec and has step(grads) -> Snap, swap(mode) -> Snap, snap() -> Snap and clear_flags().  A Snap is what the header
lets a caller read back: the parameters, the 4 x total state, the step counts, tscal, the ring and the fields of the scalar block.

Reference: optim_ref.RefUpdate in fp64.  Bars: per element |got - ref| <= 2 err_* + 1e-30 with RefUpdate's running bound; the norm within 41u
of the fp64 norm and a clipping coefficient within 44u of max_norm / (norm + 1e-6) (optim_ref's docstring; every chunk here has at most 16384
values, which that derivation assumes); tscal within 1e-15 of Python's lr / (1 - beta1^k), sqrt(1 - beta2^k) (fp64 pow on the device against
Python's); max_norm within 1e-12 of numpy's 1.5 mean + 2 std over the ring the step started from (both sides fp64); ring slots within 41u of
optim_ref.Queue's.  (A slot that holds a clipped max_norm inherits the errors of the slots it was computed from through 1.5 mean + 2 std,
in the worst case a few times 41u; the measured ratios, printed by every test, stay far below 1, so the 41u bar is kept.)"""
import math

import numpy as np
import torch

import optim_ref

U = optim_ref.U
F32 = np.float32
NUMELS = [1, 3, 4, 5, 63, 64, 65, 255, 1027, 4100, 16384 + 5, 40000]
CHUNK = 16384
B_LENS = [4, 8, 260, 1028, 16384]
PAD_BITS = 0x7FC12345              # a quiet NaN with a payload: read, it poisons the result; written, it no longer compares equal
HYP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=True, clip=False, queue_len=50, ema=True, ema_decay=0.9,
           ema_every=1, ema_start=0)


def pad_value():
    return np.array([PAD_BITS], dtype=np.uint32).view(F32)[0]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if np.asarray(a).dtype.itemsize == 4 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def chunks_a(numels):
    return [(t, s, min(CHUNK, n - s)) for t, n in enumerate(numels) for s in range(0, n, CHUNK)]


def chunks_b(numels, seed=5):
    """Chunk lengths 4, 8, 260, 1028, 16384 in rotation (starting at another one per tensor), the last chunk of a tensor taking the remainder;
    every start a multiple of 4; the table shuffled."""
    out = []
    for t, n in enumerate(numels):
        s, i = 0, t
        while n - s > B_LENS[i % 5]:
            out.append((t, s, B_LENS[i % 5]))
            s += B_LENS[i % 5]
            i += 1
        out.append((t, s, n - s))
    order = np.random.default_rng(seed).permutation(len(out))
    return [out[i] for i in order]


def check_chunks(numels, chunks):
    cover = [np.zeros(n, dtype=np.int64) for n in numels]
    for t, s, n in chunks:
        assert s % 4 == 0 and 0 < n <= CHUNK and s + n <= numels[t]
        cover[t][s:s + n] += 1
    assert all((c == 1).all() for c in cover)


class Spec:
    """Tensors, table, seeds and hyperparameters of one run; p_mis / g_mis / state_mis (floats past a 16-byte boundary; an int or one per
    tensor) only matter to a runner with real pointers."""

    def __init__(self, numels=None, chunking="A", ostride=64, seed=1, ring=(3000.0,), qhead=None, p_mis=0, g_mis=0, state_mis=0, chunks=None, **hyp):
        self.numels = list(NUMELS if numels is None else numels)
        T = len(self.numels)
        self.offsets, o = [], 0
        for n in self.numels:
            self.offsets.append(o)
            o += (n + ostride - 1) // ostride * ostride
        self.total = o
        assert self.total % 4 == 0 and all(x % 4 == 0 for x in self.offsets)
        self.chunks = chunks if chunks is not None else (chunks_a if chunking == "A" else chunks_b)(self.numels)
        check_chunks(self.numels, self.chunks)
        assert not (set(hyp) - set(HYP)), hyp
        self.hyp = {**HYP, **hyp}
        rng = np.random.default_rng(seed)
        self.p0 = [(rng.standard_normal(n) * 0.1).astype(F32) for n in self.numels]
        self.ema0 = [p + (rng.standard_normal(p.size) * 0.05).astype(F32) for p in self.p0]
        Q = self.hyp["queue_len"]
        self.ring0 = np.full(Q, np.array([0x7FF8000000C0FFEE], dtype=np.uint64).view(np.float64)[0])          # the caller's pattern in unused slots
        self.ring0[:len(ring)] = ring
        self.qcount = len(ring)
        self.qhead = len(ring) % Q if qhead is None else qhead
        as_list = lambda m: list(m) if isinstance(m, (list, tuple)) else [m] * T          # noqa: E731
        self.p_mis, self.g_mis, self.state_mis = as_list(p_mis), as_list(g_mis), state_mis

    def state0(self):
        st = np.full((4, self.total), pad_value(), dtype=F32)
        nanq = F32(np.nan)
        for t, (o, n) in enumerate(zip(self.offsets, self.numels)):
            st[0, o:o + n] = 0
            st[1, o:o + n] = 0
            st[2, o:o + n] = 0 if self.hyp["amsgrad"] else nanq
            st[3, o:o + n] = self.ema0[t] if self.hyp["ema"] else nanq
        return st

    def pad_mask(self):
        mask = np.ones(self.total, dtype=bool)
        for o, n in zip(self.offsets, self.numels):
            mask[o:o + n] = False
        return mask

    def items(self, ring, qhead, qcount):
        """The ring as the reference's Queue.items: newest first."""
        Q = self.hyp["queue_len"]
        return [float(ring[(qhead - 1 - i) % Q]) for i in range(qcount)]


class Snap:
    FIELDS = ("p", "state", "steps", "tscal", "ring", "norm", "max_norm", "coef", "flags", "qhead", "qcount", "gstep", "skipped", "ema_applied")

    def __init__(self, spec, **kw):
        self.spec = spec
        self.dev = None              # a runner with a device keeps the bytes of the device-owned workspace sections here
        for k in self.FIELDS:
            setattr(self, k, kw[k])

    def q(self, k, t):
        o, n = self.spec.offsets[t], self.spec.numels[t]
        return self.state[k, o:o + n]

    def tensor(self, name, t):
        return self.p[t] if name == "p" else self.q(("m", "v", "vmax", "ema").index(name), t)


class EmuRunner:
    def __init__(self, spec, mutant=None):
        h = spec.hyp
        self.spec = spec
        self.e = optim_ref.Emu32(spec.p0, spec.offsets, spec.total, spec.chunks, lr=h["lr"], betas=h["betas"], eps=h["eps"],
                                 weight_decay=h["weight_decay"], amsgrad=h["amsgrad"], clip=h["clip"], queue_len=h["queue_len"], ema=h["ema"],
                                 ema_decay=h["ema_decay"], ema_every=h["ema_every"], ema_start=h["ema_start"], mutant=mutant)
        self.e.state[:] = spec.state0()
        self.e.ring[:] = spec.ring0
        self.e.qhead, self.e.qcount = spec.qhead, spec.qcount

    def snap(self):
        e = self.e
        return Snap(self.spec, p=[x.copy() for x in e.p], state=e.state.copy(), steps=e.steps.copy(), tscal=e.tscal.copy(), ring=e.ring.copy(),
                    norm=e.norm, max_norm=e.max_norm, coef=float(e.coef), flags=e.flags, qhead=e.qhead, qcount=e.qcount, gstep=e.gstep,
                    skipped=e.skipped, ema_applied=e.ema_applied)

    def step(self, grads):
        self.e.step(grads)
        return self.snap()

    def swap(self, mode):
        self.e.swap(mode)
        return self.snap()

    def clear_flags(self):
        self.e.flags = 0


def make_ref(spec):
    h = spec.hyp
    ref = optim_ref.RefUpdate([torch.from_numpy(p) for p in spec.p0], lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["weight_decay"],
                              amsgrad=h["amsgrad"], clip_gradients=h["clip"], queue_len=h["queue_len"],
                              ema_decay=h["ema_decay"] if h["ema"] else None, ema_every=h["ema_every"], ema_start=h["ema_start"])
    if h["ema"]:
        ref.ema = [torch.from_numpy(e).double() for e in spec.ema0]
    ref.queue.items = spec.items(spec.ring0, spec.qhead, spec.qcount)
    return ref


def grads(spec, step, scale=0.05, have=None, seed=7):
    rng = np.random.default_rng(seed + 1000 * step)
    out = [(rng.standard_normal(n) * scale).astype(F32) for n in spec.numels]
    return [g if have is None or have[t] else None for t, g in enumerate(out)]


def ref_step(ref, gs):
    return ref.step([None if g is None else torch.from_numpy(g) for g in gs])


class Worst(dict):
    def add(self, name, ratio):
        self[name] = max(self.get(name, 0.0), float(ratio))

    def report(self, what):
        print(f"\nMEASURED {what}: worst d / bar " + ", ".join(f"{k}={v:.3g}" for k, v in self.items()))
        return self


def check_state(snap, ref, worst, names=("p", "m", "v", "vmax", "ema"), tensors=None):
    amsgrad, ema = snap.spec.hyp["amsgrad"], snap.spec.hyp["ema"]
    for name in names:
        if (name == "vmax" and not amsgrad) or (name == "ema" and not ema):
            continue
        for t in (range(len(snap.p)) if tensors is None else tensors):
            got = torch.from_numpy(snap.tensor(name, t).astype(np.float64))
            want, err = getattr(ref, name)[t], getattr(ref, "err_" + name)[t]
            bar = 2 * err + 1e-30
            d = (got - want).abs()
            ok = bool((d <= bar).all())
            if ok and d.numel():
                worst.add(name, (d / bar).max())
            assert ok, (name, t, snap.spec.numels[t], float(d.max()), float((d / bar).max()))


def check_padding(snap):
    spec = snap.spec
    mask = spec.pad_mask()
    want = spec.state0()
    for k in range(4):
        assert same_bits(snap.state[k][mask], want[k][mask]), ("padding of quarter", k)
    if not spec.hyp["amsgrad"]:
        assert same_bits(snap.state[2], want[2]), "vmax quarter touched with amsgrad = 0"
    if not spec.hyp["ema"]:
        assert same_bits(snap.state[3], want[3]), "ema quarter touched with ema = 0"


def check_norm(snap, ref, worst):
    """norm against the fp64 norm (41u); coef against max_norm / (norm + 1e-6) with the step's own max_norm (44u), exactly 1 when not clipping."""
    n64 = ref.norms64[-1]
    r = abs(snap.norm - n64) / (41 * U * n64)
    worst.add("norm", r)
    assert r <= 1, ("norm", snap.norm, n64, r)
    if not snap.spec.hyp["clip"]:
        assert snap.coef == 1.0
        return
    exact = snap.max_norm / (n64 + 1e-6)
    assert abs(exact - 1) > 1e-3, "the scripted gradients put a step at the clip threshold"
    if exact > 1:
        assert snap.coef == 1.0 and ref.coefs[-1] == 1.0
    else:
        r = abs(snap.coef - exact) / (44 * U * exact)
        worst.add("coef", r)
        assert r <= 1 and ref.coefs[-1] < 1.0, ("coef", snap.coef, exact, r)


def check_counts(snap, ref):
    assert snap.steps.tolist() == ref.steps, (snap.steps.tolist(), ref.steps)
    assert snap.gstep == ref.gstep, (snap.gstep, ref.gstep)


def check_tscal(snap, worst):
    h = snap.spec.hyp
    for t, k in enumerate(snap.steps.tolist()):
        if k == 0:
            continue
        want = (h["lr"] / (1.0 - h["betas"][0] ** k), math.sqrt(1.0 - h["betas"][1] ** k))
        for j in range(2):
            r = abs(snap.tscal[t, j] - want[j]) / (1e-15 * abs(want[j])) if want[j] else float(snap.tscal[t, j] != 0)
            worst.add("tscal", r)
            assert r <= 1, ("tscal", t, j, k, snap.tscal[t, j], want[j])


def check_queue(before, snap, ref, worst):
    """After a completed step with clip = 1: the ring against optim_ref.Queue slot by slot, mapped through qhead."""
    spec = snap.spec
    Q = spec.hyp["queue_len"]
    assert snap.qcount == len(ref.queue.items) and snap.qhead == (before.qhead + 1) % Q and snap.qcount == min(before.qcount + 1, Q)
    q = optim_ref.Queue(Q)
    q.items = spec.items(before.ring, before.qhead, before.qcount)
    want = 1.5 * q.mean() + 2 * q.std()
    r = abs(snap.max_norm - want) / (1e-12 * want)
    worst.add("max_norm", r)
    assert r <= 1, ("max_norm", snap.max_norm, want)
    for i, item in enumerate(ref.queue.items):
        got = snap.ring[(snap.qhead - 1 - i) % Q]
        r = abs(got - item) / (41 * U * item)
        worst.add("ring", r)
        assert r <= 1, ("ring slot", (snap.qhead - 1 - i) % Q, got, item, r)
    keep = np.ones(Q, dtype=bool)
    keep[before.qhead] = False
    assert same_bits(snap.ring[keep], before.ring[keep]), "a slot other than the pushed one changed"
    if snap.qcount < Q:
        assert same_bits(snap.ring[snap.qcount:], spec.ring0[snap.qcount:]), "a slot at or above qcount lost the caller's pattern"


def same_tensors(a, b, names=("p", "m", "v", "vmax", "ema")):
    """Bitwise equality per tensor (the two runs may place the tensors at other offsets)."""
    for name in names:
        for t in range(len(a.p)):
            assert same_bits(a.tensor(name, t), b.tensor(name, t)), (name, t, a.spec.numels[t])


# ---- 1. alignment and layout ---------------------------------------------------------------------------------------------------------------------
PLACEMENTS = [dict(), dict(p_mis=1, g_mis=1), dict(p_mis=2, g_mis=2), dict(p_mis=3, g_mis=3), dict(g_mis=1), dict(g_mis=[0, 1, 2, 3] * 3),
              dict(p_mis=3), dict(p_mis=[1, 2, 3, 0] * 3), dict(state_mis=1), dict(ostride=4), dict(chunking="B"),
              dict(chunking="B", p_mis=[2, 0, 1, 3] * 3, g_mis=[0, 3, 0, 1] * 3, ostride=4)]


def case_layouts(make, clip):
    hyp = dict(clip=clip, queue_len=50)
    ref = make_ref(Spec(**hyp))
    gs = [grads(Spec(**hyp), k) for k in range(3)]
    for g in gs:
        assert ref_step(ref, g)
    assert ref.coefs == [1.0] * 3
    worst, first = Worst(), None
    for place in PLACEMENTS:
        spec = Spec(**place, **hyp)
        r = make(spec)
        for k, g in enumerate(gs):
            snap = r.step(g)
            at_k = type("RefAtStep", (), dict(norms64=ref.norms64[:k + 1], coefs=ref.coefs[:k + 1]))          # the norm of step k, whatever the chunking
            check_norm(snap, at_k, worst)
            assert snap.coef == 1.0
        check_state(snap, ref, worst)
        check_padding(snap)
        check_counts(snap, ref)
        if first is None:
            first = snap
        same_tensors(first, snap)
    return worst.report(f"layouts clip={int(clip)}")


# ---- 2. intermittent gradients -------------------------------------------------------------------------------------------------------------------
def have_pattern(step):
    """Step 1 .. 6: tensor 8 (1027 values) on steps 1, 2, 4, 6; tensor 3 (5 values) never; tensor 6 (65 values) only on step 5; the rest always."""
    have = [True] * len(NUMELS)
    have[8] = step in (1, 2, 4, 6)
    have[3] = False
    have[6] = step == 5
    return have


def case_intermittent(make):
    spec = Spec(chunking="B", p_mis=1, g_mis=3)
    r, ref, worst = make(spec), make_ref(spec), Worst()
    prev = r.snap()
    for step in range(1, 7):
        have = have_pattern(step)
        g = grads(spec, step, have=have)
        snap = r.step(g)
        assert ref_step(ref, g)
        check_counts(snap, ref)
        check_tscal(snap, worst)
        check_state(snap, ref, worst)
        check_padding(snap)
        check_norm(snap, ref, worst)
        for t in range(len(have)):
            if not have[t]:
                for name in ("m", "v", "vmax", "p"):
                    assert same_bits(snap.tensor(name, t), prev.tensor(name, t)), (name, t, step)
                assert same_bits(snap.tscal[t], prev.tscal[t])
        prev = snap
    assert snap.steps.tolist() == [6, 6, 6, 0, 6, 6, 1, 6, 4, 6, 6, 6] and snap.gstep == 6
    worst.report("intermittent gradients")
    return snap


# ---- 3. EMA schedule -----------------------------------------------------------------------------------------------------------------------------
def case_ema_schedule(make, every, start, nonfinite=False):
    spec = Spec(chunking="B" if every % 2 == 0 else "A", p_mis=2 if every % 2 == 0 else 0, ema_every=every, ema_start=start)
    r, ref, worst = make(spec), make_ref(spec), Worst()
    have = [t != 3 for t in range(len(NUMELS))]          # tensor 3 never has a gradient: its EMA still moves
    prev, fired = r.snap(), []
    for call in range(1, 11):
        g = grads(spec, call, have=have)
        if nonfinite and call == 3:
            g[9][77] = np.inf
        snap = r.step(g)
        done = ref_step(ref, g)
        assert done == (not (nonfinite and call == 3)) and snap.skipped == int(not done)
        k = ref.gstep
        now = done and k >= start and k % every == 0
        assert snap.ema_applied == int(now) and snap.gstep == k, (call, snap.ema_applied, now, snap.gstep, k)
        if now:
            fired.append(call)
            check_state(snap, ref, worst, names=("ema",))
        else:
            assert same_bits(snap.state[3], prev.state[3]), ("the ema quarter changed without an EMA step", call)
        if done:
            assert not same_bits(snap.p[0], prev.p[0])
        else:
            assert snap.flags & 1
            r.clear_flags()
        check_state(snap, ref, worst)
        check_padding(snap)
        check_counts(snap, ref)
        prev = snap
    want = {(1, 0): list(range(1, 11)), (3, 0): [3, 6, 9], (2, 5): [6, 8, 10], (4, 4): [4, 8]}[(every, start)]
    if nonfinite:
        want = {(3, 0): [4, 7, 10]}[(every, start)]
    assert fired == want, (fired, want)
    return worst.report(f"ema schedule every={every} start={start} nonfinite={int(nonfinite)}")


# ---- 4. untouched quarters -----------------------------------------------------------------------------------------------------------------------
def case_untouched(make, which):
    spec = Spec(chunking="B", g_mis=2, **({"amsgrad": False} if which == "vmax" else {"ema": False}))
    r, ref, worst = make(spec), make_ref(spec), Worst()
    for step in range(1, 4):
        g = grads(spec, step)
        snap = r.step(g)
        assert ref_step(ref, g)
        check_padding(snap)                                # the NaN-filled quarter, bitwise
        check_state(snap, ref, worst)
    k = 2 if which == "vmax" else 3
    assert np.isnan(snap.state[k][~spec.pad_mask()]).all() and snap.ema_applied == int(which == "vmax")
    return worst.report(f"untouched {which}")


# ---- 5. swap -------------------------------------------------------------------------------------------------------------------------------------
def case_swap(make):
    spec = Spec(chunking="B", p_mis=[1, 2, 3, 1] * 3, clip=True)
    r = make(spec)
    s0 = r.step(grads(spec, 1))                            # moments and workspace hold real values

    def rest_same(a, b):
        assert same_bits(a.state[:3], b.state[:3]) and same_bits(a.steps, b.steps) and same_bits(a.tscal, b.tscal) and same_bits(a.ring, b.ring)
        assert (a.norm, a.max_norm, a.coef, a.flags, a.qhead, a.qcount, a.gstep) == (b.norm, b.max_norm, b.coef, b.flags, b.qhead, b.qcount, b.gstep)
        assert a.dev is None or a.dev == b.dev
        check_padding(b)

    T = range(len(s0.p))
    s1 = r.swap(0)
    rest_same(s0, s1)
    assert all(same_bits(s1.p[t], s0.q(3, t)) and same_bits(s1.q(3, t), s0.p[t]) for t in T)
    assert not same_bits(s1.p[0], s0.p[0])
    s2 = r.swap(0)
    rest_same(s0, s2)
    assert all(same_bits(s2.p[t], s0.p[t]) for t in T) and same_bits(s2.state, s0.state), "mode 0 twice is not the identity"
    s3 = r.swap(2)                                         # p = ema
    rest_same(s0, s3)
    assert same_bits(s3.state[3], s0.state[3]), "mode 2 wrote to ema"
    assert all(same_bits(s3.p[t], s0.q(3, t)) for t in T)
    s4 = r.step(grads(spec, 2))                            # p and ema differ again
    s5 = r.swap(1)                                         # ema = p
    rest_same(s4, s5)
    assert all(same_bits(s5.p[t], s4.p[t]) and same_bits(s5.q(3, t), s4.p[t]) for t in T)
    assert not same_bits(s4.q(3, 0), s4.p[0])


# ---- 6. queue ------------------------------------------------------------------------------------------------------------------------------------
QUEUES = {"len1": dict(queue_len=1, ring=(10.0,), scales=[1, 3, 1, 1, 2]),
          "len3": dict(queue_len=3, ring=(10.0,), scales=[1, 1, 3, 1, 1, 4, 1, 0.5, 5, 1]),
          "len1024": dict(queue_len=1024, ring=(10.0, 12.0, 11.0, 13.0, 9.0, 14.0, 12.0), scales=[1, 3, 1]),
          "resumed": dict(queue_len=3, ring=(11.0, 13.0, 12.0), qhead=2, scales=[1, 3, 0.5, 1])}


def case_queue(make, kind):
    cfg = QUEUES[kind]
    spec = Spec(clip=True, queue_len=cfg["queue_len"], ring=cfg["ring"], qhead=cfg.get("qhead"), chunking="B" if kind == "len3" else "A")
    r, ref, worst = make(spec), make_ref(spec), Worst()
    prev = r.snap()
    for step, scale in enumerate(cfg["scales"], 1):
        g = grads(spec, step, scale=0.05 * scale)
        snap = r.step(g)
        assert ref_step(ref, g)
        check_norm(snap, ref, worst)
        check_queue(prev, snap, ref, worst)
        check_counts(snap, ref)
        check_padding(snap)
        prev = snap
    clipped = sum(c < 1.0 for c in ref.coefs)
    assert 0 < clipped < len(ref.coefs), ref.coefs
    if kind == "len3":
        assert clipped >= 2 and snap.qhead == (1 + 10) % 3 and snap.qcount == 3
    if kind == "resumed":
        assert snap.qhead == (2 + 4) % 3 and snap.qcount == 3
    if kind == "len1024":
        assert snap.qhead == 10 and snap.qcount == 10
    return worst.report(f"queue {kind}")


# ---- 7. hyperparameter limits --------------------------------------------------------------------------------------------------------------------
LIMITS = {"beta1=0": dict(betas=(0.0, 0.999)), "beta2=0": dict(betas=(0.9, 0.0), eps=1e-8), "lr=0": dict(lr=0.0), "weight_decay=0": dict(weight_decay=0.0),
          "ema_decay=1": dict(ema_decay=1.0), "ema_decay=0": dict(ema_decay=0.0), "clip=0,ema=1": dict(clip=False, ema=True)}
ZERO_GRAD = 7                       # the 255-value tensor gets an all-zero gradient in every limit run


def case_limits(make, which):
    spec = Spec(chunking="B", p_mis=3, g_mis=1, **LIMITS[which])
    r, ref, worst = make(spec), make_ref(spec), Worst()
    s0 = r.snap()
    for step in range(1, 4):
        g = grads(spec, step)
        g[ZERO_GRAD][:] = 0
        snap = r.step(g)
        assert ref_step(ref, g)
        check_state(snap, ref, worst)
        check_padding(snap)
        check_counts(snap, ref)
        check_tscal(snap, worst)
        check_norm(snap, ref, worst)
    T = range(len(snap.p))
    # the all-zero gradient: v and m stay 0, p moves by the decoupled decay alone
    h = spec.hyp
    want = s0.p[ZERO_GRAD].copy()
    for _ in range(3):
        want = want * F32(1.0 - h["lr"] * h["weight_decay"])
    assert not snap.q(1, ZERO_GRAD).any() and not snap.q(0, ZERO_GRAD).any() and same_bits(snap.p[ZERO_GRAD], want)
    moved = [t for t in T if t != ZERO_GRAD]
    assert all(snap.q(0, t).any() and snap.q(1, t).any() for t in moved)
    if which == "lr=0":
        assert all(same_bits(snap.p[t], s0.p[t]) for t in T), "lr = 0 moved a parameter"
    else:
        assert not any(same_bits(snap.p[t], s0.p[t]) for t in moved)
    if which == "ema_decay=1":
        assert same_bits(snap.state[3], s0.state[3]), "ema_decay = 1 moved the EMA"
    if which == "ema_decay=0":                         # e - (e - p) rounds: within the bar of p (check_state above; the oracle's ema is its p), not its bits
        assert all((ref.ema[t] - ref.p[t]).abs().max().item() <= 1e-15 for t in T)
    return worst.report(f"limit {which}")


# ---- 8. non-finite skip --------------------------------------------------------------------------------------------------------------------------
def case_nonfinite(make, kind):
    spec = Spec(chunking="B", p_mis=1, g_mis=1, clip=True, ring=(10.0, 12.0))
    r, ref, worst = make(spec), make_ref(spec), Worst()
    for step in (1, 2):
        g = grads(spec, step)
        before = r.step(g)
        assert ref_step(ref, g)
    g = grads(spec, 3)
    if kind == "nan_tail":
        g[1][2] = np.nan                                   # the last of 3 values at an unaligned pointer: the scalar tail alone reaches it
    else:
        t, s, n = [c for c in spec.chunks if c[2] == 4 and spec.numels[c[0]] > 4][0]
        g[t][s + 1] = np.inf                               # inside a chunk of 4 values
    snap = r.step(g)
    assert not ref_step(ref, g)
    assert snap.flags & 1 and snap.skipped == 1 and snap.ema_applied == 0
    assert all(same_bits(a, b) for a, b in zip(snap.p, before.p)) and same_bits(snap.state, before.state)
    assert same_bits(snap.steps, before.steps) and same_bits(snap.ring, before.ring)
    assert (snap.qhead, snap.qcount, snap.gstep) == (before.qhead, before.qcount, before.gstep)
    check_padding(snap)
    r.clear_flags()
    g = grads(spec, 4)
    after = r.step(g)
    assert ref_step(ref, g)
    assert after.flags == 0 and after.skipped == 0 and after.steps.tolist() == [3] * len(NUMELS) and after.gstep == 3
    check_state(after, ref, worst)
    check_queue(snap, after, ref, worst)
    check_norm(after, ref, worst)
    check_tscal(after, worst)
    return worst.report(f"non-finite {kind}")


# ---- more than 256 tensors and chunks: the strided loops of the finalize kernel -------------------------------------------------------------------
def many_tensors_spec():
    rng = np.random.default_rng(3)
    numels = [int(n) for n in rng.integers(4, 9, size=300)]
    chunks = []
    for t, n in enumerate(numels):
        chunks += [(t, 0, 4), (t, 4, 4)] if n == 8 else [(t, 0, n)]
    chunks = [chunks[i] for i in rng.permutation(len(chunks))]
    assert len(chunks) > 300
    return Spec(numels=numels, chunks=chunks, ostride=4, clip=True, p_mis=[0, 1, 2, 3] * 75, g_mis=[1, 0] * 150)


def case_many_tensors(make):
    spec = many_tensors_spec()
    r, ref, worst = make(spec), make_ref(spec), Worst()
    for step in range(1, 4):
        have = [not (t % 7 == step or t == 299 - step) for t in range(300)]          # some tensors past index 255 skip a step
        g = grads(spec, step, scale=1.0, have=have)
        snap = r.step(g)
        assert ref_step(ref, g)
        check_counts(snap, ref)
        check_tscal(snap, worst)
        check_norm(snap, ref, worst)
        check_state(snap, ref, worst)
        check_padding(snap)
    assert snap.steps.max() == 3 and snap.steps[256:].min() < 3 and snap.steps[:256].min() < 3
    return worst.report("300 tensors")
