"""The training step's own GEMM shapes in both matrix modes (include/gcdm_matrix_mode.h), timed on the GPU in alternating windows (GPU box).

    python tools/gemm_mode_probe.py [--windows 5] [--reps 50] [--edges 23104] [--nodes 1216]

Shapes (64 x 19 QM9: E = 23 104 edges, 1 216 nodes), all through gcdm_op_gemm as the operators call it:
    message scalar_out     [E x 273] . [273 x 256]     y = x W^T + b   (A k-fast, B k-fast, odd row stride)
    message gate           [E x 256] . [256 x 32]
    message dX             [E x 256] . [256 x 273]     dx = dy W       (A k-fast, B n-fast)
    weight gradient        [256 x E] . [E x 273]       dW = dy^T x in 16 K slices + the slice reduction (A m-fast, B n-fast: the operand
                                                       layout and slice count of the grouped weight-gradient kernel, which has no entry of
                                                       its own and runs on the same tile body)
    node scalar_out        [1 216 x 537] . [537 x 256]

Per shape: `windows` pairs of windows, fp32 mode then bf16x6 mode, `reps` calls each between two HIP events after 5 untimed calls; printed are
every window's us per call, the median of each mode, the spread (max - min) of the fp32 windows, and the ratio of the medians.  A difference
counts when it exceeds that spread."""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--edges", type=int, default=64 * 19 * 19)
    ap.add_argument("--nodes", type=int, default=64 * 19)
    args = ap.parse_args()
    pkg = importlib.import_module("bio-diffusion_amd")
    ops, lib = pkg.ops, pkg._native.load_ops()
    dev = torch.device("cuda", 0)
    E, Nn = args.edges, args.nodes
    g = torch.Generator().manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dev)

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    # name, M, N, K, (A, sam, sak), (B, sbk, sbn), bias, slices
    shapes = [
        ("message scalar_out [E x 273].[273 x 256]", E, 256, 273, (rnd(E, 273), 273, 1), (rnd(256, 273), 1, 273), rnd(256), 1),
        ("message gate       [E x 256].[256 x 32] ", E, 32, 256, (rnd(E, 256), 256, 1), (rnd(32, 256), 1, 256), rnd(32), 1),
        ("message dX         [E x 256].[256 x 273]", E, 273, 256, (rnd(E, 256), 256, 1), (rnd(256, 273), 273, 1), None, 1),
        ("weight gradient    [256 x E].[E x 273] /16", 256, 273, E, (rnd(E, 256), 1, 256), (rnd(E, 273), 273, 1), None, 16),
        (f"node scalar_out    [{Nn} x 537].[537 x 256]", Nn, 256, 537, (rnd(Nn, 537), 537, 1), (rnd(256, 537), 1, 537), rnd(256), 1),
    ]
    print(f"gemm_mode_probe: E = {E}, nodes = {Nn}, {args.windows} window pairs of {args.reps} calls, {torch.cuda.get_device_name(dev)}")
    try:
        for name, M, N, K, (A, sam, sak), (B, sbk, sbn), bias, slices in shapes:
            part = torch.empty(slices * M * N, device=dev)
            out = torch.empty(M * N, device=dev)

            def call():
                assert lib.gcdm_op_gemm(ptr(A), sam, sak, ptr(B), sbk, sbn, ptr(part), None if bias is None else ptr(bias), M, N, K, slices, st) == 0
                if slices > 1:
                    assert lib.gcdm_op_reduce_slices(ptr(part), ptr(out), M * N, slices, st) == 0

            us = {"f32": [], "bf16x6": []}
            for _ in range(args.windows):
                for mode in ("f32", "bf16x6"):
                    ops.set_matrix_mode(mode)
                    for _ in range(5):
                        call()
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record()
                    for _ in range(args.reps):
                        call()
                    ev[1].record()
                    torch.cuda.synchronize(dev)
                    us[mode].append(ev[0].elapsed_time(ev[1]) / args.reps * 1e3)
            m32, m6 = statistics.median(us["f32"]), statistics.median(us["bf16x6"])
            tf = 2.0 * M * N * K / 1e6
            print(f"{name}: f32 {m32:8.1f} us ({tf / m32:6.1f} TFLOP/s) windows [{', '.join(f'{u:.1f}' for u in us['f32'])}] spread {max(us['f32']) - min(us['f32']):.1f}"
                  f" | bf16x6 {m6:8.1f} us ({tf / m6:6.1f} TFLOP/s) windows [{', '.join(f'{u:.1f}' for u in us['bf16x6'])}] | f32 / bf16x6 = {m32 / m6:.2f}")
    finally:
        ops.set_matrix_mode("f32")


if __name__ == "__main__":
    main()
