"""optim.BucketedUpdate, parallel.broadcast_training_state / shard_batch and model.configure_data_parallel on an MI355X: gradient accumulation
against stock fp32 arithmetic, the wrapper's transparency at one rank, and two ranks on GPU 0 over gloo staying bit-identical.

The single-process tests compute each gradient set once, clone it and feed the clones to both sides, so they do not depend on a backward pass
being bit-repeatable.  The model is the `qm9` training fixture's (train_cases.model_for); the 8-molecule batch is drawn here, ragged."""
import datetime
import importlib
import os
import socket

import numpy as np
import pytest
import torch

import synth
import train_cases as TC

pkg = importlib.import_module("bio-diffusion_amd")
optim = pkg.optim
par = importlib.import_module("bio-diffusion_amd.parallel")
pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [5, 19, 3, 11, 16, 9, 7, 12]


def _batch8(dev=DEV):
    d = synth.DATASET_DIMS["qm9"]
    g = torch.Generator().manual_seed(5)
    nn = torch.tensor(SIZES)
    N = int(nn.sum())
    types = torch.randint(0, d["num_atom_types"], (N,), generator=g)
    return pkg.config.AttrDict(x=torch.randn((N, 3), generator=g).to(dev), batch=torch.repeat_interleave(torch.arange(len(nn)), nn).to(dev),
                               mask=torch.ones(N, dtype=torch.bool, device=dev), props_context=None,
                               one_hot=torch.nn.functional.one_hot(types, d["num_atom_types"]).float().to(dev),
                               charges=torch.randint(1, 10, (N,), generator=g).float().to(dev))


def _twins(golden_dir):
    c = TC.load(golden_dir, "qm9")
    model, _ = TC.model_for(c)
    twin, _ = TC.model_for(c)
    twin.load_state_dict(model.state_dict())
    for p, q in zip(model.parameters(), twin.parameters()):
        assert torch.equal(p.detach(), q.detach())
    return c, model, twin


def _grads_of(model, batch, seed):
    model.zero_grad()
    torch.manual_seed(seed)
    model.training_step(pkg.config.AttrDict(batch))["loss"].backward()          # (the step writes into the batch it is given)
    return [None if p.grad is None else p.grad.detach().clone() for p in model.parameters()]


def _feed(model, grads):
    for p, g in zip(model.parameters(), grads):
        p.grad = None if g is None else g.clone()


def _same_everywhere(a_model, a, b_model, b, step):
    torch.cuda.synchronize()
    for t, (p, q) in enumerate(zip(a_model.parameters(), b_model.parameters())):
        assert torch.equal(p.detach(), q.detach()), ("parameter", t, step)
    for t, (x, y) in enumerate(zip(a.ema_tensors(), b.ema_tensors())):
        assert torch.equal(x, y), ("ema", t, step)
    assert a.queue() == b.queue() and a.steps() == b.steps() and a.last_grad_norm() == b.last_grad_norm(), step
    assert a.read_flags() == 0 and b.read_flags() == 0


def test_accumulation_equals_one_step_on_the_stock_fp32_mean(golden_dir):
    c, model, twin = _twins(golden_dir)
    batch = _batch8()
    micro = [par.shard_batch(batch, r, 2) for r in range(2)]
    assert [int(m.batch.max()) + 1 for m in micro] == [4, 4] and sum(m.x.shape[0] for m in micro) == sum(SIZES)
    upd = optim.BucketedUpdate(model.configure_optimizers(), accumulate_grad_batches=2)
    plain = twin.configure_optimizers()
    norms = []
    for step in range(3):
        g1, g2 = _grads_of(model, micro[0], 10 + step), _grads_of(model, micro[1], 20 + step)
        absent = sum(g is None for g in g1)
        assert 1 <= absent < len(g1) // 2 and [g is None for g in g1] == [g is None for g in g2] and all(torch.isfinite(g).all() for g in g1 + g2 if g is not None)
        _feed(model, g1)
        upd.accumulate()
        _feed(model, g2)
        upd.accumulate()
        with pytest.raises(RuntimeError, match="step\\(\\) is due"):
            upd.accumulate()
        mine = [p.grad for p in model.parameters()]
        upd.step()
        assert all(a is b for a, b in zip(mine, (p.grad for p in model.parameters()))), "step() did not leave p.grad as it was"
        _feed(twin, [None if a is None else a * 0.5 + b * 0.5 for a, b in zip(g1, g2)])
        plain.step()
        _same_everywhere(model, upd, twin, plain, step)
        norms.append(upd.last_grad_norm())
    assert len(set(norms)) == 3 and upd.steps().count(3) == len(upd.steps()) - absent
    with pytest.raises(RuntimeError, match="0 of 2"):
        upd.step()


def test_configure_data_parallel_is_transparent_at_one_rank(golden_dir):
    c, model, twin = _twins(golden_dir)
    batch = TC.batch_of(c)
    upd = model.configure_data_parallel()
    assert isinstance(upd, optim.BucketedUpdate) and isinstance(upd.update, optim.TrainingUpdate) and upd.accumulate_grad_batches == 1
    plain = twin.configure_optimizers()
    par.broadcast_training_state(model, upd)              # no process group: nothing to do
    for step in range(3):
        grads = _grads_of(model, batch, 30 + step)
        _feed(model, grads)
        upd.accumulate()
        upd.step()
        _feed(twin, grads)
        plain.step()
        _same_everywhere(model, upd, twin, plain, step)
    sd = upd.state_dict()
    assert sd["global_step"] == 3 and sd["gradnorm_queue"] == plain.queue()
    upd.load_state_dict(sd)
    assert upd.queue() == plain.queue() and upd.steps() == plain.steps()


# ---- two ranks on GPU 0 --------------------------------------------------------------------------------------------------------------------------
def _rank(rank, world, port, golden_dir, out_dir, q):
    try:
        _rank_body(rank, world, port, golden_dir, out_dir, q)
    except BaseException:                                  # the parent must not wait out its limit for a rank that has died
        import traceback
        q.put((rank, "failed", traceback.format_exc()))
        raise


def _rank_body(rank, world, port, golden_dir, out_dir, q):
    """One rank of three data-parallel training steps, both ranks on GPU 0 (this pool has one-GPU boxes), the all-reduce over gloo."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    c = TC.load(golden_dir, "qm9")
    torch.manual_seed(0)
    model, _ = TC.model_for(c)
    upd = model.configure_data_parallel()
    if rank != 0:                                          # so that the broadcast has something to do
        with torch.no_grad():
            next(model.parameters()).mul_(1.5)
        upd.update._reset_queue([7.0, 8.0])
    par.broadcast_training_state(model, upd, src=0)
    local = par.shard_batch(_batch8(), rank, world)
    pre = post = None
    for step in range(3):
        upd.zero_grad()
        torch.manual_seed(100 + step + 10 * rank)
        model.training_step(pkg.config.AttrDict(local))["loss"].backward()
        upd.accumulate()
        if step == 0:
            pre = upd.bucket.clone()
        upd.step()
        if step == 0:
            post = upd.bucket.clone()
    torch.cuda.synchronize()
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).cpu().numpy()          # noqa: E731
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), pre=pre.cpu().numpy(), post=post.cpu().numpy(), params=flat(model.parameters()),
             ema=flat(upd.ema_tensors()), final=upd.bucket.cpu().numpy(), queue=np.array(upd.queue()), steps=np.array(upd.steps()))
    q.put((rank, upd.read_flags(), int(local.batch.max()) + 1, "libgcdm_ops.so" in open("/proc/self/maps").read()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_stay_bit_identical(golden_dir, tmp_path):
    """2 processes, spawn, a free port; every wait has a limit, the children are killed on any failure, nothing is retried."""
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, golden_dir, str(tmp_path), q)) for r in range(2)]
    try:
        for p in procs:
            p.start()
        res = []
        for _ in range(2):
            res.append(q.get(timeout=600))
            assert res[-1][1] != "failed", res[-1][2]
        res.sort(key=lambda t: t[0])
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(timeout=30)
    bits = lambda a: a.view(np.uint32 if a.dtype == np.float32 else np.uint64)          # noqa: E731
    out = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2)]
    for r in range(2):
        assert res[r][0] == r and res[r][1] == 0, ("flags", res[r])
        assert res[r][2] == 4 and res[r][3], "the rank did not get its 4 molecules or did not load the HIP library"
    pre0, pre1 = torch.from_numpy(out[0]["pre"]), torch.from_numpy(out[1]["pre"])
    assert not np.array_equal(bits(out[0]["pre"]), bits(out[1]["pre"])), "the two ranks packed the same gradients"
    want = (pre0 + pre1).numpy()                          # torch fp32: one rounded sum per value
    assert np.isfinite(want).all() and np.count_nonzero(want) > want.size // 2
    for r in range(2):
        assert np.array_equal(bits(out[r]["post"]), bits(want)), ("post-reduce bucket", r)
    for k in ("post", "final", "params", "ema", "queue", "steps"):
        assert np.array_equal(bits(out[0][k]), bits(out[1][k])) if out[0][k].dtype.kind == "f" else np.array_equal(out[0][k], out[1][k]), k
    assert len(out[0]["queue"]) == 4 and 3000.0 in out[0]["queue"].tolist() and 7.0 not in out[1]["queue"].tolist()
    assert out[0]["steps"].max() == 3
