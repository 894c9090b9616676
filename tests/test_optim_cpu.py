"""The fused training update without a GPU: include/gcdm_optim.h <-> libgcdm_ops.so exports <-> native.OPTIM_SIGNATURES, the header as C99,
argument refusal before any HIP call, the workspace layout, the Python refusals of optim.TrainingUpdate, and the fp64 restatement the GPU tests
use (tests/optim_ref.py) against torch.optim.AdamW(amsgrad=True) + torch.nn.utils.clip_grad_norm_ + the reference's EMA.

The argument cases call the library with null pointers; as in test_ops_cabi_cpu.py the `lib` fixture runs them only on a library at least as
new as its sources that refuses a bad argument in a launch-free probe first."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest
import torch

import optim_cases as K
import optim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
optim = pkg.optim
HEADER = os.path.join(ROOT, "include", "gcdm_optim.h")
Z = None


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(gcdm_optim_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip()])
    return out


def test_header_declares_exactly_the_signature_table():
    decl = _declared()
    assert decl == {k: len(v) for k, v in native.OPTIM_SIGNATURES.items()}
    assert not set(decl) & (set(native.OPS_EXPORTS) | set(native.MP_TRAIN_SIGNATURES))
    text = open(HEADER).read()
    assert re.search(rf"#define GCDM_OPTIM_QUEUE_MAX {native.OPTIM_QUEUE_MAX}\b", text)
    assert re.search(rf"#define GCDM_OPTIM_FLAG_NONFINITE {native.OPTIM_FLAG_NONFINITE}\b", text)


def test_header_and_kernels_are_library_dependencies():
    assert HEADER in native.OPS_HEADERS
    assert os.path.join(ROOT, "bio-diffusion_amd", "csrc", "gcdm_ops.optim.hip.h") in native.OPS_HEADERS
    assert not [h for h in native.HEADERS if "optim" in os.path.basename(h)]


def test_library_exports_every_declared_entry():
    if not os.path.exists(native.OPS_LIB_PATH):
        pytest.skip("libgcdm_ops.so not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(native.OPS_LIB_PATH)
    for name in native.OPTIM_SIGNATURES:
        assert hasattr(lib, name), name


def test_header_is_c99():
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = '#include "gcdm_optim.h"\nint main(void) { return (int)gcdm_optim_workspace_bytes(0, 1, 1, GCDM_OPTIM_QUEUE_MAX) < 0; }\n'
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.dirname(HEADER), "-x", "c", "-"],
                       input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr


@pytest.fixture(scope="module")
def lib():
    path = native.OPS_LIB_PATH
    if not os.path.exists(path):
        pytest.skip("libgcdm_ops.so not built (run __graft_entry__.build())")
    stale = [d for d in native.OPS_SOURCES + native.OPS_HEADERS if os.path.getmtime(d) > os.path.getmtime(path)]
    if stale:
        pytest.skip(f"libgcdm_ops.so is older than {stale} (run __graft_entry__.build()): it may lack the argument checks under test")
    lib = ctypes.CDLL(path)
    for name, sig in native.OPTIM_SIGNATURES.items():
        getattr(lib, name).argtypes = sig
        getattr(lib, name).restype = native.OPTIM_RESTYPES.get(name, ctypes.c_int)
    # launch-free probe: a queue length of 0 with no work at all must be refused
    status = lib.gcdm_optim_step(Z, Z, 0, 0, 0, 1e-4, 0.9, 0.999, 1e-8, 0.0, 1, 1, 0, 1, 0.9999, 1, 0, Z)
    if status != -1:
        pytest.fail(f"{path}: gcdm_optim_step accepts queue_len = 0 (status {status}); the null-pointer cases would not be safe")
    return lib


def _step(ws=Z, state=Z, total=64, T=4, C=4, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, wd=1e-12, ams=1, clip=1, q=50, ema=1, decay=0.9999, every=1,
          start=0):
    return (ws, state, total, T, C, lr, b1, b2, eps, wd, ams, clip, q, ema, decay, every, start, Z)


def _swap(ws=Z, state=Z, total=64, T=4, C=4, q=50, mode=0):
    return (ws, state, total, T, C, q, mode, Z)


def test_every_entry_refuses_bad_arguments_and_skips_empty_work(lib):
    nan = float("nan")
    qmax = native.OPTIM_QUEUE_MAX
    S, W = "gcdm_optim_step", "gcdm_optim_ema_swap"
    cases = [
        (S, _step(), -1), (S, _step(total=-1), -1), (S, _step(T=-1), -1), (S, _step(C=-1), -1),
        (S, _step(q=0), -1), (S, _step(q=qmax + 1), -1), (S, _step(q=-5), -1),
        (S, _step(lr=-1e-4), -1), (S, _step(lr=nan), -1), (S, _step(eps=-1.0), -1), (S, _step(wd=-1e-3), -1), (S, _step(wd=nan), -1),
        (S, _step(b1=1.0), -1), (S, _step(b1=-0.1), -1), (S, _step(b2=1.0), -1), (S, _step(b2=nan), -1),
        (S, _step(ams=2), -1), (S, _step(clip=-1), -1), (S, _step(ema=2), -1),
        (S, _step(decay=1.5), -1), (S, _step(decay=-0.1), -1), (S, _step(decay=nan), -1), (S, _step(every=0), -1), (S, _step(start=-1), -1),
        (S, _step(ws=8, state=8, total=0), -1),
        (S, _step(T=0), 0), (S, _step(C=0), 0), (S, _step(T=0, C=0, total=0), 0), (S, _step(T=0, q=0), -1),
        (S, _step(T=0, decay=2.0), -1), (S, _step(T=0, ema=0, decay=0.0), 0), (S, _step(T=0, decay=1.0), 0), (S, _step(T=0, b1=0.0, b2=0.0), 0),
        (W, _swap(), -1), (W, _swap(mode=3), -1), (W, _swap(mode=-1), -1), (W, _swap(q=0), -1), (W, _swap(total=-1), -1),
        (W, _swap(T=0), 0), (W, _swap(C=0, mode=2), 0), (W, _swap(T=0, mode=3), -1), (W, _swap(ws=8, state=8, total=0), -1),
    ]
    for which in (-1, 12):
        cases.append(("gcdm_optim_workspace_bytes", (which, 4, 4, 50), -1))
    cases += [("gcdm_optim_workspace_bytes", (0, -1, 4, 50), -1), ("gcdm_optim_workspace_bytes", (0, 4, -1, 50), -1),
              ("gcdm_optim_workspace_bytes", (0, 4, 4, 0), -1), ("gcdm_optim_workspace_bytes", (0, 4, 4, qmax + 1), -1)]
    bad = [(n, a, want, getattr(lib, n)(*a)) for n, a, want in cases]
    assert [b for b in bad if b[2] != b[3]] == []


def _a(n):
    return (n + 255) // 256 * 256


def _layout(T, C, Q):
    """The workspace layout of include/gcdm_optim.h restated (bytes, every section rounded up to 256)."""
    sizes = [8 * T, 8 * T, 8 * T, 8 * T, 24 * C, None, 8 * T, 16 * T, 4 * C, 8 * Q, 64]
    off, o = [], 0
    for s in sizes:
        off.append(o)
        if s is not None:
            o += _a(s)
    return [o] + off


@pytest.mark.parametrize("T,C,Q", [(1, 1, 1), (433, 757, 50), (3, 1000, 1024), (0, 0, 7), (17, 33, 3)])
def test_workspace_query_matches_the_layout(lib, T, C, Q):
    got = [lib.gcdm_optim_workspace_bytes(w, T, C, Q) for w in range(12)]
    assert got == _layout(T, C, Q)
    assert all(g % 256 == 0 for g in got)


def test_python_refusals():
    cpu = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="not a CUDA tensor"):
        optim.TrainingUpdate([cpu])
    a, b = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="one parameter group"):
        optim.TrainingUpdate([{"params": [a]}, {"params": [b]}])
    with pytest.raises(ValueError, match="betas"):
        optim.TrainingUpdate([a], betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="queue_len"):
        optim.TrainingUpdate([a], queue_len=0)
    with pytest.raises(ValueError, match="EMA decay"):
        optim.TrainingUpdate([a], ema_decay=1.5)


def test_python_refuses_fp16_before_the_device():
    class FakeCuda(torch.Tensor):
        @property
        def is_cuda(self):
            return True
    p = torch.zeros(4, dtype=torch.float16).as_subclass(FakeCuda)
    with pytest.raises(ValueError, match="float16"):
        optim.TrainingUpdate([p])


def _scripted_grads(shapes, steps, seed=11):
    """Gradients whose norm crosses the clip threshold: a spike above the seeded 4500 at step 3, small norms until the 3000 is flushed
    (after 50 pushes), then spikes that the recent-history threshold clips."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(steps):
        scale = 1.0 + 0.5 * (k % 7)
        if k == 3:
            scale = 5e3
        if k in (52, 54, 56, 58):
            scale = 60.0
        out.append([None if s is None else torch.randn(s, generator=g, dtype=torch.float64) * scale / 8 for s in shapes])
    return out


def test_fp64_oracle_matches_torch_adamw_clip_and_ema_over_60_steps():
    shapes = [(7, 5), (3,), None, (1,), (4, 4, 2)]
    g0 = torch.Generator().manual_seed(3)
    init = [torch.randn(s if s else (2,), generator=g0, dtype=torch.float64) for s in shapes]
    ref = optim_ref.RefUpdate(init, lr=1e-2, weight_decay=1e-2, ema_decay=0.99)
    params = [torch.nn.Parameter(p.clone()) for p in init]
    opt = torch.optim.AdamW(params, lr=1e-2, weight_decay=1e-2, amsgrad=True, foreach=False)
    ema = [p.detach().clone() for p in params]
    queue = optim_ref.Queue()
    queue.add(3000)
    clipped = 0
    for grads in _scripted_grads(shapes, 60):
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.clone()
        # qm9_mol_gen_ddpm.py configure_gradient_clipping, then the optimizer, then EMA.on_train_batch_end
        max_norm = 1.5 * queue.mean() + 2 * queue.std()
        norm = float(torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], max_norm))
        queue.add(float(max_norm) if norm > max_norm else norm)
        clipped += norm > max_norm
        opt.step()
        for e, p in zip(ema, params):
            diff = e - p.detach()
            diff.mul_(1.0 - 0.99)
            e.sub_(diff)
        assert ref.step(grads)
    assert clipped >= 3 and 3000.0 not in queue.items
    assert ref.queue.items == pytest.approx(queue.items, rel=1e-6)       # the oracle pushes the fp32-rounded norm
    assert ref.gstep == 60 and ref.steps == [60, 60, 0, 60, 60]
    for t, p in enumerate(params):
        scale = max(1.0, float(p.detach().abs().max()))
        assert (ref.p[t] - p.detach()).abs().max().item() <= 1e-6 * scale, t
        assert (ref.ema[t] - ema[t]).abs().max().item() <= 1e-6 * scale, t
        if shapes[t] is None:
            assert torch.equal(ref.p[t], init[t])
            continue
        st = opt.state[p]
        assert int(st["step"]) == 60
        for mine, theirs in ((ref.m[t], st["exp_avg"]), (ref.v[t], st["exp_avg_sq"]), (ref.vmax[t], st["max_exp_avg_sq"])):
            assert (mine - theirs).abs().max().item() <= 1e-6 * theirs.abs().max().item(), t


@pytest.mark.parametrize("every,start", [(1, 0), (3, 0), (2, 5), (4, 4)])
def test_fp64_oracle_matches_torch_with_an_ema_schedule_and_intermittent_gradients(every, start):
    """torch.optim.AdamW keeps a step count per parameter and passes over a parameter whose grad is None, as the oracle does; the EMA is
    applied in the torch loop on the k-th step only when k >= ema_start and k % ema_every == 0."""
    shapes = [(7, 5), (3,), (1,), (4, 4, 2)]
    have = lambda t, k: {0: True, 1: k in (1, 2, 4, 6, 11), 2: False, 3: k == 5}[t]          # noqa: E731
    g0 = torch.Generator().manual_seed(5)
    init = [torch.randn(s, generator=g0, dtype=torch.float64) for s in shapes]
    kw = dict(lr=1e-2, weight_decay=1e-2, ema_decay=0.9)
    ref = optim_ref.RefUpdate(init, ema_every=every, ema_start=start, **kw)
    params = [torch.nn.Parameter(p.clone()) for p in init]
    opt = torch.optim.AdamW(params, lr=1e-2, weight_decay=1e-2, amsgrad=True, foreach=False)
    ema = [p.detach().clone() + 0.5 for p in params]
    ref.ema = [e.clone() for e in ema]
    queue = optim_ref.Queue()
    queue.add(3000)
    applied = []
    for k in range(1, 13):
        grads = [torch.randn(s, generator=g0, dtype=torch.float64) * (40.0 if k == 9 else 1.0) if have(t, k) else None for t, s in enumerate(shapes)]
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.clone()
        max_norm = 1.5 * queue.mean() + 2 * queue.std()
        norm = float(torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], max_norm))
        queue.add(float(max_norm) if norm > max_norm else norm)
        opt.step()
        if k >= start and k % every == 0:
            applied.append(k)
            for e, p in zip(ema, params):
                e.sub_((e - p.detach()).mul_(1.0 - 0.9))
        assert ref.step(grads)
    assert applied == [k for k in range(1, 13) if k >= start and k % every == 0] and 0 < len(applied)
    assert ref.gstep == 12 and ref.steps == [12, 5, 0, 1]
    assert ref.queue.items == pytest.approx(queue.items, rel=1e-6)
    for t, p in enumerate(params):
        scale = max(1.0, float(p.detach().abs().max()))
        assert (ref.p[t] - p.detach()).abs().max().item() <= 1e-6 * scale, t
        assert (ref.ema[t] - ema[t]).abs().max().item() <= 1e-6 * scale, t
        if ref.steps[t] == 0:
            assert torch.equal(ref.p[t], init[t]) and p not in opt.state
            continue
        st = opt.state[p]
        assert int(st["step"]) == ref.steps[t]
        for mine, theirs in ((ref.m[t], st["exp_avg"]), (ref.v[t], st["exp_avg_sq"]), (ref.vmax[t], st["max_exp_avg_sq"])):
            assert (mine - theirs).abs().max().item() <= 1e-6 * theirs.abs().max().item(), t


# ---- the fp32 restatement (optim_ref.Emu32) through the cases of the GPU file (tests/optim_cases.py) ----------------------------------------------
def test_the_tables_hold_the_shapes_the_cases_rely_on():
    """Chunking B has short chunks, chunks whose float4 count is no multiple of 256, several chunks in one small tensor and a shuffled table;
    the 300-tensor table has more than 256 tensors and chunks; no chunk exceeds the 16384 values the norm's error bound assumes."""
    b = K.chunks_b(K.NUMELS)
    K.check_chunks(K.NUMELS, b)
    assert {4, 8, 260, 1028, 16384} <= {n for _, _, n in b} and [t for t, _, _ in b] != sorted(t for t, _, _ in b)
    assert sum(1 for t, _, _ in b if K.NUMELS[t] == 64) >= 3 and any(n % 4 for _, _, n in b)
    many = K.many_tensors_spec()
    assert len(many.numels) == 300 and len(many.chunks) > 300 and all(4 <= n <= 8 for n in many.numels)
    assert max(n for _, _, n in K.chunks_a(K.NUMELS)) == K.CHUNK


EMU_CASES = {
    "layouts": lambda make: K.case_layouts(make, False),
    "layouts clip": lambda make: K.case_layouts(make, True),
    "intermittent": K.case_intermittent,
    "ema 1/0": lambda make: K.case_ema_schedule(make, 1, 0),
    "ema 3/0": lambda make: K.case_ema_schedule(make, 3, 0),
    "ema 2/5": lambda make: K.case_ema_schedule(make, 2, 5),
    "ema 4/4": lambda make: K.case_ema_schedule(make, 4, 4),
    "ema 3/0 nonfinite": lambda make: K.case_ema_schedule(make, 3, 0, True),
    "untouched vmax": lambda make: K.case_untouched(make, "vmax"),
    "untouched ema": lambda make: K.case_untouched(make, "ema"),
    "swap": K.case_swap,
    "nonfinite nan": lambda make: K.case_nonfinite(make, "nan_tail"),
    "nonfinite inf": lambda make: K.case_nonfinite(make, "inf_chunk4"),
    "300 tensors": K.case_many_tensors,
}
EMU_CASES.update({f"queue {k}": (lambda make, k=k: K.case_queue(make, k)) for k in K.QUEUES})
EMU_CASES.update({f"limit {k}": (lambda make, k=k: K.case_limits(make, k)) for k in K.LIMITS})


@pytest.mark.parametrize("case", list(EMU_CASES))
def test_a_correct_fp32_evaluation_meets_every_bar(case):
    """Emu32 follows the header's formulas in numpy float32: it must pass every check the device is held to, at the same bars."""
    EMU_CASES[case](K.EmuRunner)


# mutant of Emu32 -> one case whose checks must reject it (the mutants of the library the GPU file is run against: DESIGN.md 3.6)
MUTANT_CASES = {"a": "layouts", "b": "ema 1/0", "c": "intermittent", "d": "ema 3/0", "e": "intermittent", "f": "untouched vmax", "g": "swap",
                "h": "queue len3", "i": "ema 2/5", "j": "layouts"}


@pytest.mark.parametrize("mutant", sorted(optim_ref.Emu32.MUTANTS))
def test_the_bars_reject_each_mutant(mutant):
    assert sorted(MUTANT_CASES) == sorted(optim_ref.Emu32.MUTANTS)
    with pytest.raises(AssertionError):
        EMU_CASES[MUTANT_CASES[mutant]](lambda spec: K.EmuRunner(spec, mutant=mutant))


def test_module_configure_optimizers_is_the_fused_update_and_needs_the_gpu():
    model = pkg.QM9MoleculeGenerationDDPM(**pkg.default_cfgs("qm9"))
    with pytest.raises(ValueError, match="not a CUDA tensor"):
        model.configure_optimizers()
