"""KFAC.update() on a bf16-autocast ResNet-50 (N=32, 224²): (a) the native half-precision build (curv_kfac16_accumulate for
every bf16 side, the fp32 build for the stem's A side) against (b) `.float()` copies of the records plus today's fp32
build, the casts included.  HIP-event times, executed GFLOP, fraction of the 2.5 PF dense bf16 roof, and the bytes the
half-precision build moves against HBM.

    python tools/bench_half_update.py [--batch 32] [--size 224] [--reps 10] [--model resnet50] [--dtype bf16]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from curvature_amd import models, ops
from curvature_amd.curvatures import KFAC

HBM_BPS = 8.0e12            # MI355X HBM3E, datasheet
BF16_FLOPS = 2.5e15         # MI355X dense bf16 / fp16 MFMA, datasheet


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


def half_bytes(kfac):
    """Bytes the half-precision build moves: source reads, packed image written once and read by the MFMA kernel
    (L2 reuse aside: each 128-row panel once per tile of its row / column), slabs written and read, dst written."""
    import ctypes
    from curvature_amd import _lib
    total = 0
    for layer, (x, g) in kfac.record.items():
        for side, t in enumerate((x, g)):
            if t.dtype == torch.float32 or (isinstance(layer, torch.nn.Conv2d) and layer.groups > 1):
                continue
            conv = isinstance(layer, torch.nn.Conv2d)
            kernel = layer.kernel_size if conv and side == 0 else (1, 1)
            stride = layer.stride if conv and side == 0 else (1, 1)
            padding = layer.padding if conv and side == 0 else (0, 0)
            src = t if conv else t.reshape(-1, t.shape[-1])
            job = ops.HalfFactorJob(tuple(src.shape), None, kernel, stride, padding, side == 0 and layer.bias is not None,
                                    dtype=t.dtype)
            arr = ops._half_descs([job], check_tensors=False)
            ws = _lib.lib().curv_kfac16_workspace_bytes(arr, 1)
            dim = kfac.state[layer][side].shape[0]
            total += t.numel() * 2 + 2 * ws + dim * dim * 4        # image + slabs: written once, read once
    return total


def bench(name, batch, size, reps, dtype):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = getattr(models, name)().to(dev)
    kfac = KFAC(model)
    x = torch.randn(batch, 3, size, size, device=dev)
    with torch.autocast("cuda", dtype=dtype):
        loss = F.cross_entropy(model(x), torch.randint(0, 1000, (batch,), device=dev))
    model.zero_grad()
    loss.backward()
    sides = [t.dtype for pair in kfac.record.values() for t in pair]
    kfac._count_flops = True
    kfac.update(batch_size=batch)
    flops = kfac._last_flops
    t_native = timed(lambda: kfac.update(batch_size=batch), reps)

    ref = KFAC(model)
    records = dict(kfac.record)

    def cast_and_build():
        ref.record = {l: [t.detach().float() for t in v] for l, v in records.items()}
        ref.update(batch_size=batch)

    ref._count_flops = True
    cast_and_build()
    flops32 = ref._last_flops
    t_cast = timed(cast_and_build, reps)
    kfac.restart_accumulation()
    ref.restart_accumulation()
    kfac.update(batch_size=batch)
    cast_and_build()
    torch.cuda.synchronize()
    err = max(float((a.double() - b.double()).norm() / b.double().norm())
              for l in kfac.state for a, b in zip(kfac.state[l], ref.state[l]))
    nbytes = half_bytes(kfac)
    return dict(model=name, batch=batch, size=size, dtype=str(dtype).replace("torch.", ""),
                half_sides=sum(d != torch.float32 for d in sides), fp32_sides=sum(d == torch.float32 for d in sides),
                native_update_ms=round(t_native, 4), cast_fp32_update_ms=round(t_cast, 4),
                ratio_native_over_cast=round(t_native / t_cast, 3),
                native_exec_GFLOP=round(flops / 1e9, 1), fp32_exec_GFLOP=round(flops32 / 1e9, 1),
                native_roof_fraction_bf16=round(flops / (t_native * 1e-3) / BF16_FLOPS, 3),
                native_TFLOPs=round(flops / (t_native * 1e-3) / 1e12, 1),
                half_build_bytes_GB=round(nbytes / 1e9, 3), half_build_hbm_ms=round(nbytes / HBM_BPS * 1e3, 3),
                max_rel_err_vs_fp32_path=float(f"{err:.2e}"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    a = ap.parse_args()
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    print(json.dumps(bench(a.model, a.batch, a.size, a.reps, dtype)), flush=True)


if __name__ == "__main__":
    main()
