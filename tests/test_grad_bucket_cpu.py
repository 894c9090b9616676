"""The flat gradient bucket without a GPU: include/gcdm_grad_bucket.h <-> libgcdm_ops.so exports <-> native.GRAD_BUCKET_SIGNATURES, the header as
C99, argument refusal before any HIP call, the bucket's size, parallel.shard_batch, the Python refusals of optim.BucketedUpdate, and the numpy
float32 restatement of the pack arithmetic (tests/grad_bucket_cases.py) against a float64 evaluation.

The argument cases call the library with null pointers; as in test_optim_cpu.py the `lib` fixture runs them only on a library at least as new
as its sources that refuses a bad argument in a launch-free probe first."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import grad_bucket_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
optim = pkg.optim
par = importlib.import_module("bio-diffusion_amd.parallel")
HEADER = os.path.join(ROOT, "include", "gcdm_grad_bucket.h")
Z = None


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(gcdm_grad_bucket_\w+)\s*\(([^)]*)\)\s*;", text):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip()])
    return out


def test_header_declares_exactly_the_signature_table():
    decl = _declared()
    assert decl == {k: len(v) for k, v in native.GRAD_BUCKET_SIGNATURES.items()}
    assert sorted(decl) == ["gcdm_grad_bucket_check", "gcdm_grad_bucket_floats", "gcdm_grad_bucket_pack"]
    assert not set(decl) & (set(native.OPS_EXPORTS) | set(native.OPTIM_SIGNATURES) | set(native.MP_TRAIN_SIGNATURES))
    assert re.search(rf"#define GCDM_GRAD_BUCKET_FLAG_MISMATCH {native.GRAD_BUCKET_FLAG_MISMATCH}\b", open(HEADER).read())
    assert native.GRAD_BUCKET_FLAG_MISMATCH == 2 == optim.FLAG_MISMATCH and not native.GRAD_BUCKET_FLAG_MISMATCH & native.OPTIM_FLAG_NONFINITE
    assert native.GRAD_BUCKET_RESTYPES == {"gcdm_grad_bucket_floats": ctypes.c_int64}


def test_header_and_kernels_are_library_dependencies():
    assert HEADER in native.OPS_HEADERS
    assert os.path.join(ROOT, "bio-diffusion_amd", "csrc", "gcdm_ops.bucket.hip.h") in native.OPS_HEADERS
    assert not [h for h in native.HEADERS if "bucket" in os.path.basename(h)]


def test_library_exports_every_declared_entry():
    if not os.path.exists(native.OPS_LIB_PATH):
        pytest.skip("libgcdm_ops.so not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(native.OPS_LIB_PATH)
    for name in native.GRAD_BUCKET_SIGNATURES:
        assert hasattr(lib, name), name


def test_header_is_c99():
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = ('#include "gcdm_grad_bucket.h"\nint main(void) { return (int)gcdm_grad_bucket_floats(64, 1) < 0 || '
           'gcdm_grad_bucket_pack(0, 0, 0, 0, 0, 0, 1, 1.0, 1, 0) || gcdm_grad_bucket_check(0, 0, 0, 0, 0, 1, GCDM_GRAD_BUCKET_FLAG_MISMATCH, 0); }\n')
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
    for name, sig in native.GRAD_BUCKET_SIGNATURES.items():
        getattr(lib, name).argtypes = sig
        getattr(lib, name).restype = native.GRAD_BUCKET_RESTYPES.get(name, ctypes.c_int)
    # launch-free probe: `first` = 2 with no work at all must be refused
    status = lib.gcdm_grad_bucket_pack(Z, Z, Z, 0, 0, 0, 50, 1.0, 2, Z)
    if status != -1:
        pytest.fail(f"{path}: gcdm_grad_bucket_pack accepts first = 2 (status {status}); the null-pointer cases would not be safe")
    return lib


def _pack(ws=Z, grads=Z, bucket=Z, total=64, T=4, C=4, q=50, scale=0.5, first=1):
    return (ws, grads, bucket, total, T, C, q, scale, first, Z)


def _check(ws=Z, bucket=Z, total=64, T=4, C=4, q=50, world=2):
    return (ws, bucket, total, T, C, q, world, Z)


def test_every_entry_refuses_bad_arguments_and_skips_empty_work(lib):
    nan, inf = float("nan"), float("inf")
    qmax = native.OPTIM_QUEUE_MAX
    P, K, F = "gcdm_grad_bucket_pack", "gcdm_grad_bucket_check", "gcdm_grad_bucket_floats"
    cases = [
        (P, _pack(), -1), (P, _pack(ws=8, grads=8), -1), (P, _pack(ws=8, bucket=8), -1), (P, _pack(grads=8, bucket=8), -1),
        (P, _pack(total=-4), -1), (P, _pack(T=-1), -1), (P, _pack(C=-1), -1), (P, _pack(total=66), -1), (P, _pack(total=2, T=0), -1),
        (P, _pack(q=0), -1), (P, _pack(q=qmax + 1), -1), (P, _pack(first=2), -1), (P, _pack(first=-1), -1),
        (P, _pack(scale=nan), -1), (P, _pack(scale=inf), -1), (P, _pack(scale=-inf), -1),
        (P, _pack(ws=8, grads=8, bucket=8, total=0), -1),
        (P, _pack(T=0), 0), (P, _pack(C=0), 0), (P, _pack(T=0, C=0, total=0), 0), (P, _pack(T=0, scale=nan), -1), (P, _pack(C=0, first=3), -1),
        (P, _pack(T=0, scale=0.0, first=0), 0), (P, _pack(C=0, scale=-1.0 / 3), 0),
        (K, _check(), -1), (K, _check(ws=8), -1), (K, _check(bucket=8), -1), (K, _check(total=-4), -1), (K, _check(T=-1), -1),
        (K, _check(C=-1), -1), (K, _check(total=62), -1), (K, _check(q=0), -1), (K, _check(q=qmax + 1), -1),
        (K, _check(world=0), -1), (K, _check(world=-2), -1), (K, _check(ws=8, bucket=8, total=0), -1),
        (K, _check(T=0), 0), (K, _check(C=0), 0), (K, _check(T=0, world=0), -1), (K, _check(C=0, world=1), 0), (K, _check(T=0, C=0, total=0), 0),
        (F, (-4, 1), -1), (F, (64, -1), -1), (F, (66, 1), -1), (F, (0, 0), 0),
    ]
    bad = [(n, a, want, getattr(lib, n)(*a)) for n, a, want in cases]
    assert [b for b in bad if b[2] != b[3]] == []


@pytest.mark.parametrize("T", [1, 63, 64, 65, 432])
def test_bucket_size_matches_the_layout(lib, T):
    """`total` values, then T presence floats rounded up to a multiple of 64."""
    want_tail = {1: 64, 63: 64, 64: 64, 65: 128, 432: 448}[T]
    for total in (0, 4, 64, 6_200_000):
        got = lib.gcdm_grad_bucket_floats(total, T)
        assert got == total + want_tail == G.bucket_floats(total, T)


# ---- parallel.shard_batch ------------------------------------------------------------------------------------------------------------------------
def _ragged_batch(with_counts):
    nn = torch.tensor([3, 1, 5, 2])                       # world 3 gives rank 2 the 1-molecule shard [2]; world 2 gives [3, 1] and [5, 2]
    N = int(nn.sum())
    g = torch.Generator().manual_seed(1)
    bi = torch.repeat_interleave(torch.arange(len(nn)), nn)
    b = pkg.config.AttrDict(x=torch.randn((N, 3), generator=g), one_hot=torch.randn((N, 5), generator=g), charges=torch.randn((N, 1), generator=g),
                            batch=bi, mask=torch.rand(N, generator=g) > 0.2, props_context=None, note="kept")
    if with_counts:
        b.num_graphs, b.num_nodes_present, b.context_per_molecule = len(nn), nn.clone(), torch.randn((len(nn), 2), generator=g)
        b.h = {"categorical": b.one_hot, "integer": b.charges}
    return b, nn


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("with_counts", [False, True])
def test_shard_batch_equals_slicing_by_shard_range(world, with_counts):
    b, nn = _ragged_batch(with_counts)
    starts = torch.cat((torch.zeros(1, dtype=torch.long), nn.cumsum(0)))
    sizes = []
    for rank in range(world):
        lo, hi = par.shard_range(len(nn), rank, world)
        a, e = int(starts[lo]), int(starts[hi])
        s = par.shard_batch(b, rank, world)
        assert type(s) is type(b) and set(s) == set(b) and s.note == "kept" and s.props_context is None
        for k in ("x", "one_hot", "charges", "mask"):
            assert torch.equal(s[k], b[k][a:e]), k
        assert torch.equal(s.batch, b.batch[a:e] - lo) and (hi == lo or (s.batch[0] == 0 and s.batch[-1] == hi - lo - 1))
        if with_counts:
            assert s.num_graphs == hi - lo and torch.equal(s.num_nodes_present, nn[lo:hi])
            assert torch.equal(s.context_per_molecule, b.context_per_molecule[lo:hi])
            assert torch.equal(s.h["categorical"], b.one_hot[a:e]) and torch.equal(s.h["integer"], b.charges[a:e])
        sizes.append(hi - lo)
    assert sum(sizes) == len(nn) and (world != 3 or 1 in sizes)
    assert torch.equal(b.batch, torch.repeat_interleave(torch.arange(len(nn)), nn)), "the batch itself was changed"


# ---- optim.BucketedUpdate: what it refuses before it touches a device ------------------------------------------------------------------------------
def test_python_refusals():
    stub = optim.TrainingUpdate.__new__(optim.TrainingUpdate)          # never initialised: a refusal must come before any use of it
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="accumulate_grad_batches"):
            optim.BucketedUpdate(stub, accumulate_grad_batches=bad)
    with pytest.raises(TypeError, match="TrainingUpdate"):
        optim.BucketedUpdate(torch.optim.SGD([torch.nn.Parameter(torch.zeros(2))], lr=0.1))
    w = optim.BucketedUpdate(stub, accumulate_grad_batches=2)
    with pytest.raises(RuntimeError, match="0 of 2"):
        w.step()
    w._passes = 1
    with pytest.raises(RuntimeError, match="1 of 2"):
        w.step()
    with pytest.raises(ValueError, match="closure"):
        w.step(lambda: None)


def test_module_configure_data_parallel_wraps_a_fresh_update_and_needs_the_gpu():
    model = pkg.QM9MoleculeGenerationDDPM(**pkg.default_cfgs("qm9"))
    with pytest.raises(ValueError, match="not a CUDA tensor"):
        model.configure_data_parallel()


# ---- the float32 restatement of the pack arithmetic ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3, 1.0 / 6])
def test_the_float32_emulation_is_two_roundings_of_the_float64_evaluation(scale):
    """float64 holds the product of two float32 exactly (24 + 24 bits), and the sum of two float32 whose exponents differ by less than 29; the
    data here stay inside that, so rounding each float64 result to float32 once is the stated arithmetic, and the emulation must give those
    bits.  A single rounding of s g + b (what a fused multiply-add computes) differs from it somewhere for a scale that is no power of two."""
    rng = np.random.default_rng(4)
    numels = [1, 5, 1027, 40000]
    offsets, o = [], 0
    for n in numels:
        offsets.append(o)
        o += (n + 63) // 64 * 64
    total = o
    mk = lambda: [(rng.standard_normal(n) * 0.05).astype(np.float32) for n in numels]          # noqa: E731
    g1, g2, g3 = mk(), mk(), mk()
    g2[1] = None
    bucket = np.full(G.bucket_floats(total, 4), np.float32(np.nan))
    G.emu_pack(bucket, offsets, numels, total, g1, scale, True)
    G.emu_pack(bucket, offsets, numels, total, g2, scale, False)
    G.emu_pack(bucket, offsets, numels, total, g3, scale, False)
    s64 = np.float64(np.float32(scale))
    fused_differs = False
    for t, (o, n) in enumerate(zip(offsets, numels)):
        want = (s64 * g1[t].astype(np.float64)).astype(np.float32)
        for g in (g2[t], g3[t]):
            if g is None:
                continue
            prod64 = s64 * g.astype(np.float64)
            two = (want.astype(np.float64) + prod64.astype(np.float32).astype(np.float64)).astype(np.float32)
            one = (want.astype(np.float64) + prod64).astype(np.float32)
            fused_differs |= bool((two.view(np.uint32) != one.view(np.uint32)).any())
            want = two
        assert (bucket[o:o + n].view(np.uint32) == want.view(np.uint32)).all(), t
    assert fused_differs == (scale not in (1.0, 0.5))
    pad = np.ones(bucket.size, dtype=bool)
    for o, n in zip(offsets, numels):
        pad[o:o + n] = False
    pad[total:total + 4] = False
    assert (bucket[pad].view(np.uint32) == 0).all() and bucket[total:total + 4].tolist() == [1.0, 1.0, 1.0, 1.0]
    absent = [None, None, g1[2], None]
    G.emu_pack(bucket, offsets, numels, total, absent, scale, True)
    assert bucket[total:total + 4].tolist() == [0.0, 0.0, 1.0, 0.0] and not bucket[:offsets[2]].any() and bucket[offsets[2]:offsets[2] + 1027].any()
