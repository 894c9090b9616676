"""What the gradient-bucket tests share (include/gcdm_grad_bucket.h): the bucket's layout restated, and the pack arithmetic in numpy float32 --
fl32(s g) on a first pass, fl32(bucket + fl32(s g)) on a later one, two roundings -- which tests/test_grad_bucket_cpu.py holds to a float64
evaluation and tests/test_grad_bucket_cabi_gpu.py holds the device to, bit for bit."""
import numpy as np

F32 = np.float32


def tail_floats(T):
    return (T + 63) // 64 * 64


def bucket_floats(total, T):
    """`total` values, then one presence float per tensor rounded up to a multiple of 64."""
    return total + tail_floats(T)


def emu_pack(bucket, offsets, numels, total, grads, scale, first):
    """One gcdm_grad_bucket_pack on a numpy float32 bucket, in place.  ``grads``: one float32 array or None per tensor."""
    assert bucket.dtype == F32 and bucket.size == bucket_floats(total, len(numels))
    s = F32(scale)
    if first:
        bucket[:] = 0.0                                   # absent tensors, padding, tail
    pres = bucket[total: total + len(numels)]
    for t, (o, n) in enumerate(zip(offsets, numels)):
        g = grads[t]
        if g is None:
            continue
        assert g.dtype == F32 and g.size == n
        prod = s * g                                      # float32 * float32 array: one rounding
        assert prod.dtype == F32
        bucket[o:o + n] = prod if first else bucket[o:o + n] + prod          # the second rounding
        pres[t] = 1.0
    return bucket


def special_values(g):
    """Puts -0.0, the smallest denormal, a denormal with several bits and the largest denormal (and their negatives) into a gradient."""
    vals = np.array([0x80000000, 0x00000001, 0x80000001, 0x00012345, 0x007FFFFF, 0x807FFFFF], dtype=np.uint32).view(F32)
    n = min(g.size, vals.size)
    g[g.size - n:] = vals[:n]
    return g
