"""A-factor build of Conv3d layers (curv_kfac_conv3d_accumulate) at five 3-D U-Net / video shapes, N as listed:
HIP-event times, the candidates run in turn inside every round (so drift and neighbours hit all alike), of
  - the Conv3d build (gather pass + the plain build of the depth-unfolded stack),
  - baseline (i): the same stack made by torch (F.pad + unfold + permute + contiguous), then `ops.kfac_accumulate`,
  - baseline (ii): a torch fp32 3-D im2col (pad + three unfolds + reshape) and one mm,
  - the plain build of a ready-made stack alone: the Conv3d build minus this is the gather pass,
  - a device-to-device copy_ that moves as many bytes as the gather pass (source read once + stack written once),
with the median and the spread (min .. max) over the rounds, the launch form of the stack's build, whether the Conv3d build
and baseline (i) give the same bits, and the relative error against baseline (ii).

    python tools/bench_conv3d.py [--rounds 7] [--reps 5]

The gather pass alone: run the tool under ``rocprofv3 --kernel-trace --stats`` (a run of its own, --rounds 2) and read
`conv3d_gather_kernel`.
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from curvature_amd import _lib, ops

# ((N, C, D, H, W), kernel, padding), stride 1
SHAPES = [((2, 32, 32, 64, 64), (3, 3, 3), (1, 1, 1)), ((2, 64, 16, 32, 32), (3, 3, 3), (1, 1, 1)),
          ((2, 128, 8, 16, 16), (3, 3, 3), (1, 1, 1)), ((8, 64, 8, 56, 56), (1, 3, 3), (0, 1, 1)),
          ((8, 64, 8, 56, 56), (3, 1, 1), (1, 0, 0))]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def launch_form(job):
    """What curv_kfac_plan_info / curv_kfac_path_for say about a plain build of `job` alone."""
    arr = ops._factor_descs([job], check_tensors=False)
    out = (ctypes.c_longlong * ops.PLAN_INFO_FIELDS)()
    _lib.check(_lib.lib().curv_kfac_plan_info(arr, 1, out), "curv_kfac_plan_info")
    path = {_lib.PATH_SMALL: "small", _lib.PATH_GROUPED: "grouped"}[int(_lib.lib().curv_kfac_path_for(arr, 1))]
    kind = {0: "implicit im2col", 1: "flat LDS-DMA", 2: "shifted correlations"}[int(out[23])]
    return dict(path=path, kind=kind, tile=int(out[16]), k_slices=int(out[13]), flops_G=round(out[24] / 1e9, 2))


def torch_stack(x, k, p):
    u = F.pad(x, (0, 0, 0, 0, p[0], p[0])).unfold(2, k[0], 1)                      # (N, C, Do, H, W, kd)
    return u.permute(0, 2, 1, 5, 3, 4).reshape(x.shape[0] * u.shape[2], x.shape[1] * k[0], *x.shape[3:]).contiguous()


def torch_im2col(x, k, p):
    u = F.pad(x, (p[2], p[2], p[1], p[1], p[0], p[0])).unfold(2, k[0], 1).unfold(3, k[1], 1).unfold(4, k[2], 1)
    return u.permute(1, 5, 6, 7, 0, 2, 3, 4).reshape(x.shape[1] * math.prod(k), -1)


def spread(values):
    return dict(median=round(statistics.median(values), 4), min=round(min(values), 4), max=round(max(values), 4))


def bench(shape, k, p, rounds, reps):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = torch.randn(*shape, device=dev)
    N, C, D, H, W = shape
    n = C * math.prod(k) + 1
    Do, Ho, Wo = (shape[2 + d] + 2 * p[d] - k[d] + 1 for d in range(3))
    scale = 1.0 / (N * Do * Ho * Wo)
    A, B, S = (torch.empty(n, n, device=dev) for _ in range(3))
    job = ops.Conv3dFactorJob(x, A, k, (1, 1, 1), p, True, scale, True)
    stack = torch_stack(x, k, p)
    ready = ops.FactorJob(stack, S, k[1:], (1, 1), p[1:], True, scale, True)

    def new():
        ops.kfac_accumulate_conv3d([job])

    def base_i():
        ops.kfac_accumulate([ops.FactorJob(torch_stack(x, k, p), B, k[1:], (1, 1), p[1:], True, scale, True)])

    def base_ii():
        U = torch_im2col(x, k, p)
        U = torch.cat([U, U.new_ones(1, U.shape[1])])
        return torch.mm(U, U.t()).mul_(scale)

    moved = x.numel() + stack.numel()                                             # floats the gather pass reads + writes
    a, b = torch.empty(moved // 2, device=dev), torch.empty(moved // 2, device=dev)
    candidates = dict(conv3d_build=new, torch_stack_then_build=base_i, torch_im2col_mm=base_ii,
                      ready_stack_build=lambda: ops.kfac_accumulate([ready]), copy=lambda: b.copy_(a))
    for fn in candidates.values():                                                 # warm up every shape the window uses
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in candidates}
    for _ in range(rounds):
        for name, fn in candidates.items():
            times[name].append(timed(fn, reps))
    same_bits = bool(torch.equal(A, B)) and bool(torch.equal(A, S))
    ref = base_ii()
    err = float((A - ref).norm() / ref.norm())
    del ref
    med = {name: statistics.median(v) for name, v in times.items()}
    gather_ms = med["conv3d_build"] - med["ready_stack_build"]
    nbytes = 4 * moved
    return dict(shape=dict(N=N, C=C, D=D, H=H, W=W, kernel=k, padding=p), dim=n, stack=list(stack.shape),
                stack_MB=round(4 * stack.numel() / 1e6, 1), ms={name: spread(v) for name, v in times.items()},
                speedup_vs_torch_stack=round(med["torch_stack_then_build"] / med["conv3d_build"], 3),
                speedup_vs_torch_im2col_mm=round(med["torch_im2col_mm"] / med["conv3d_build"], 3),
                gather_by_difference_ms=round(gather_ms, 4),
                gather_by_difference_GBps=round(nbytes / max(gather_ms, 1e-6) / 1e6, 1),
                copy_GBps=round(nbytes / med["copy"] / 1e6, 1),
                stack_form=launch_form(ops.FactorJob(tuple(stack.shape), None, k[1:], (1, 1), p[1:], True)),
                same_bits_as_torch_stack_build=same_bits, rel_err_vs_torch_im2col_mm=float(f"{err:.2e}"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for shape, k, p in SHAPES:
        print(json.dumps(bench(shape, k, p, a.rounds, a.reps)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
