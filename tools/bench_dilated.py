"""A-factor build of dilated convolutions (curv_kfac_dilated_accumulate) at the two DeepLab layer shapes of DESIGN.md K16,
N = 32: HIP-event times of
  - the dilated build (gather pass + the plain build of the class stack),
  - the plain build of the class stack alone (the stack gathered by torch beforehand): the difference is the gather pass,
  - the same layer with dilation 1 and padding 1 through curv_kfac_accumulate (the same multiply-adds),
  - torch: F.unfold(..., dilation) and one fp32 mm,
  - a device-to-device copy of the source (the bandwidth the gather pass is held against),
with the launch form each build takes and the relative error of the dilated factor against the torch one.

    python tools/bench_dilated.py [--reps 20] [--batch 32]

The gather pass alone: run the tool under ``rocprofv3 --kernel-trace --stats`` (a run of its own, --reps 3) and read
`dilated_gather_kernel`.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from curvature_amd import _lib, ops

# (C, H, W, kernel, dilation)
SHAPES = [(256, 28, 28, 3, 2), (512, 28, 28, 3, 4)]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
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
    return dict(path=path, kind=kind, tile=int(out[16]), k_slices=int(out[13]), pretiled=int(out[22]), flops_G=round(out[24] / 1e9, 2))


def bench(shape, batch, reps):
    dev = torch.device("cuda:0")
    C, H, W, k, d = shape
    torch.manual_seed(0)
    x = torch.randn(batch, C, H, W, device=dev)
    n = C * k * k + 1
    scale = 1.0 / (batch * H * W)
    A = torch.empty(n, n, device=dev)
    dilated = ops.DilatedFactorJob(x, A, (k, k), (1, 1), (d, d), (d, d), True, scale, True)
    t_dilated = timed(lambda: ops.kfac_accumulate_dilated([dilated]), reps)

    # the class stack as the gather pass lays it out (class-major), gathered by torch: the plain build of it alone
    stack = torch.cat([x[:, :, rh::d, rw::d] for rh in range(d) for rw in range(d)]).contiguous()
    B = torch.empty(n, n, device=dev)
    stack_job = ops.FactorJob(stack, B, (k, k), (1, 1), (1, 1), True, scale, True)
    t_stack = timed(lambda: ops.kfac_accumulate([stack_job]), reps)
    same_bits = bool(torch.equal(A, B))

    P = torch.empty(n, n, device=dev)
    plain_job = ops.FactorJob(x, P, (k, k), (1, 1), (1, 1), True, scale, True)
    t_plain = timed(lambda: ops.kfac_accumulate([plain_job]), reps)

    def yardstick():
        U = F.unfold(x, (k, k), dilation=(d, d), padding=(d, d)).transpose(0, 1).reshape(C * k * k, -1)
        U = torch.cat([U, U.new_ones(1, U.shape[1])])
        return torch.mm(U, U.t()).mul_(scale)
    t_torch = timed(yardstick, max(2, reps // 4))
    ref = yardstick()
    err = float((A - ref).norm() / ref.norm())
    del ref

    y = torch.empty_like(x)
    t_copy = timed(lambda: y.copy_(x), reps)
    nbytes = 2 * x.numel() * 4                                  # read + write, of the copy and of the gather pass alike
    gather_ms = t_dilated - t_stack
    return dict(shape=dict(N=batch, C=C, H=H, W=W, kernel=k, dilation=d, padding=d), dim=n,
                dilated_build_ms=round(t_dilated, 4), class_stack_build_ms=round(t_stack, 4),
                gather_by_difference_ms=round(gather_ms, 4),
                gather_by_difference_GBps=round(nbytes / max(gather_ms, 1e-6) / 1e6, 1),
                copy_ms=round(t_copy, 4), copy_GBps=round(nbytes / t_copy / 1e6, 1),
                dilation1_build_ms=round(t_plain, 4), torch_unfold_mm_ms=round(t_torch, 4),
                dilated_vs_dilation1=round(t_dilated / t_plain, 3), speedup_vs_torch=round(t_torch / t_dilated, 2),
                class_stack_form=launch_form(ops.FactorJob(tuple(stack.shape), None, (k, k), (1, 1), (1, 1), True)),
                dilation1_form=launch_form(ops.FactorJob(tuple(x.shape), None, (k, k), (1, 1), (1, 1), True)),
                stack_build_same_bits=same_bits, rel_err_vs_torch=float(f"{err:.2e}"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    for shape in SHAPES:
        print(json.dumps(bench(shape, a.batch, a.reps)), flush=True)


if __name__ == "__main__":
    main()
