"""A-factor build of every ConvTranspose2d of the DCGAN generator (N = 64) and the U-Net (N = 8, 256x256): HIP-event
times of the phase-split build (curv_kfac_convt_accumulate) per layer, next to a torch yardstick on the same GPU
(zero-stuffing, F.unfold and one fp32 mm of the dense patch matrix), with bytes, executed FLOPs and the roof: the larger
of the HBM time of (source read + factor write) and the executed-FLOP time at the fp32 MFMA rate.

    python tools/bench_convt.py [--reps 10] [--models dcgan_generator,unet]
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

HBM_BPS = 8.0e12          # MI355X HBM3E, datasheet
FP32_FLOPS = 157.3e12     # MI355X dense fp32 MFMA, datasheet

SETUPS = {
    "dcgan_generator": dict(batch=64, input=lambda n: (n, 100, 1, 1)),
    "unet": dict(batch=8, input=lambda n: (n, 3, 256, 256)),
}


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


def yardstick(layer, x, out_size):
    """torch on the GPU: zero-stuffed input padded by k - 1 - p (and the output padding), F.unfold, taps flipped, one mm."""
    N, C, H, W = x.shape
    (kh, kw), (sh, sw), (ph, pw) = layer.kernel_size, layer.stride, layer.padding
    Ho, Wo = out_size
    xs = x.new_zeros(N, C, (H - 1) * sh + 1, (W - 1) * sw + 1)
    xs[:, :, ::sh, ::sw] = x
    oph, opw = Ho - ((H - 1) * sh - 2 * ph + kh), Wo - ((W - 1) * sw - 2 * pw + kw)
    eh, ew = kh - 1 - ph, kw - 1 - pw
    xs = F.pad(xs, (ew, ew + opw, eh, eh + oph))          # (every benchmarked layer has p <= k - 1)
    U = F.unfold(xs, (kh, kw)).view(N, C, kh, kw, -1).flip(2).flip(3)
    U = U.permute(1, 2, 3, 0, 4).reshape(C * kh * kw, -1)
    if layer.bias is not None:
        U = torch.cat([U, U.new_ones(1, U.shape[1])])
    return torch.mm(U, U.t()).mul_(1.0 / (N * Ho * Wo))


def bench(name, reps):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    setup = SETUPS[name]
    batch = setup["batch"]
    model = getattr(models, name)().to(dev)
    kfac = KFAC(model, ['ConvTranspose2d'])
    out = model(torch.randn(*setup["input"](batch), device=dev))
    model.zero_grad()
    out.square().mean().backward()
    layers = kfac._layers()
    rows, total = [], dict(build=0.0, yard=0.0, roof=0.0)
    for i, layer in enumerate(layers):
        x, g = (t.detach().contiguous() for t in kfac.record[layer])
        out_size = tuple(g.shape[2:])
        N, L = x.shape[0], out_size[0] * out_size[1]
        n = layer.in_channels * layer.kernel_size[0] * layer.kernel_size[1] + int(layer.bias is not None)
        A = torch.empty(n, n, device=dev)
        job = ops.ConvTFactorJob(x, A, layer.kernel_size, layer.stride, layer.padding, out_size,
                                 layer.bias is not None, 1.0 / (N * L), True)
        flops_exec = ops.kfac_convt_plan_flops([job])[0]
        flops_dense = n * (n + 1) * N * L
        nbytes = x.numel() * 4 + n * n * 4
        t_build = timed(lambda: ops.kfac_accumulate_convt([job]), reps)
        t_yard = timed(lambda: yardstick(layer, x, out_size), reps)
        ref = yardstick(layer, x, out_size)
        err = float((A - ref).norm() / ref.norm())
        roof = max(nbytes / HBM_BPS, flops_exec / FP32_FLOPS) * 1e3
        bound = "HBM" if nbytes / HBM_BPS >= flops_exec / FP32_FLOPS else "MFMA"
        rows.append(dict(model=name, layer=i, input=list(x.shape), kernel=list(layer.kernel_size),
                         stride=list(layer.stride), padding=list(layer.padding), dim=n,
                         build_ms=round(t_build, 4), torch_yardstick_ms=round(t_yard, 4),
                         speedup_vs_torch=round(t_yard / t_build, 2), bytes_MB=round(nbytes / 1e6, 2),
                         flops_exec_G=round(flops_exec / 1e9, 3), flops_dense_G=round(flops_dense / 1e9, 3),
                         roof_ms=round(roof, 4), roof_bound=bound, roof_fraction=round(roof / t_build, 3),
                         rel_err_vs_torch=float(f"{err:.2e}")))
        total["build"] += t_build
        total["yard"] += t_yard
        total["roof"] += roof
    summary = dict(model=name, batch=batch, layers=len(rows), build_ms=round(total["build"], 4),
                   torch_yardstick_ms=round(total["yard"], 4), speedup_vs_torch=round(total["yard"] / total["build"], 2),
                   roof_ms=round(total["roof"], 4), roof_fraction=round(total["roof"] / total["build"], 3))
    return rows, summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--models", default="dcgan_generator,unet")
    a = ap.parse_args()
    for name in a.models.split(","):
        rows, summary = bench(name, a.reps)
        for r in rows:
            print(json.dumps(r), flush=True)
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
