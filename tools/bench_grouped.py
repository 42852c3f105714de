"""KFAC on models with grouped convolutions (MobileNetV2: 17 depthwise 3x3 layers; ResNeXt-50 32x4d: 16 grouped 3x3 layers):
HIP-event times of update / invert / sample_and_replace, the grouped factor build on its own (curv_kfac_group_accumulate)
next to a torch yardstick on the same GPU (group-major F.unfold + torch.bmm per layer), with bytes, FLOPs and roof fractions.

    python tools/bench_grouped.py [--batch 32] [--size 224] [--reps 10] [--models mobilenet_v2,resnext50_32x4d]
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
FP32_FLOPS = 157.3e12     # MI355X dense fp32 (vector = matrix), datasheet


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


def grouped_jobs(kfac, layers, first=True):
    jobs = []
    for layer in layers:
        x, g = (t.detach().contiguous() for t in kfac.record[layer])
        N, L = g.shape[0], g.shape[2] * g.shape[3]
        A, G = kfac.state[layer]
        jobs.append(ops.GroupFactorJob(x, A, layer.groups, layer.kernel_size, layer.stride, layer.padding,
                                       layer.bias is not None, 1.0 / (N * L), first))
        jobs.append(ops.GroupFactorJob(g, G, layer.groups, scale=float(N) / L, first=first))
    return jobs


def yardstick(kfac, layers):
    """torch: group-major im2col (F.unfold, then a copy to (G, P, N L)) and one batched GEMM per factor."""
    out = []
    for layer in layers:
        x, g = (t.detach() for t in kfac.record[layer])
        G = layer.groups
        N, L = g.shape[0], g.shape[2] * g.shape[3]
        U = F.unfold(x, layer.kernel_size, padding=layer.padding, stride=layer.stride)
        U = U.view(N, G, -1, L).permute(1, 2, 0, 3).reshape(G, -1, N * L)
        out.append(torch.bmm(U, U.transpose(1, 2)).mul_(1.0 / (N * L)))
        V = g.reshape(N, G, -1, L).permute(1, 2, 0, 3).reshape(G, -1, N * L)
        out.append(torch.bmm(V, V.transpose(1, 2)).mul_(float(N) / L))
    return out


def bench(name, batch, size, reps):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = getattr(models, name)().to(dev)
    kfac = KFAC(model)
    x = torch.randn(batch, 3, size, size, device=dev)
    loss = F.cross_entropy(model(x), torch.randint(0, 1000, (batch,), device=dev))
    model.zero_grad()
    loss.backward()
    kfac.update(batch_size=batch)
    layers = [l for l in kfac._layers() if isinstance(l, torch.nn.Conv2d) and l.groups > 1]
    jobs = grouped_jobs(kfac, layers)
    flops_exec = sum(ops.kfac_group_plan_flops(jobs))
    flops_sym, nbytes = 0, 0
    for j in jobs:
        N, C, H, W = j.src.shape
        n = j.dst.shape[1]
        Ho = (H + 2 * j.padding[0] - j.kernel[0]) // j.stride[0] + 1
        Wo = (W + 2 * j.padding[1] - j.kernel[1]) // j.stride[1] + 1
        flops_sym += j.groups * n * (n + 1) * N * Ho * Wo
        nbytes += j.src.numel() * 4 + j.dst.numel() * 4
    t_group = timed(lambda: ops.kfac_accumulate_groups(jobs), reps)
    t_yard = timed(lambda: yardstick(kfac, layers), reps)
    got = [t for l in layers for t in kfac.state[l]]
    want = yardstick(kfac, layers)
    err = max(float((a - b).norm() / b.norm()) for a, b in zip(got, want))
    t_update = timed(lambda: kfac.update(batch_size=batch), reps)
    kfac.restart_accumulation()
    kfac.update(batch_size=batch)
    t_invert = timed(lambda: kfac.invert(add=0.5, multiply=1.0), reps)
    t_sample = timed(lambda: kfac.sample_and_replace(), reps)
    n_desc = sum(2 * getattr(l, "groups", 1) for l in kfac.state)
    roof = max(nbytes / HBM_BPS, flops_sym / FP32_FLOPS) * 1e3
    return dict(model=name, batch=batch, size=size, grouped_layers=len(layers),
                grouped_groups=sum(l.groups for l in layers), invert_descriptors=n_desc,
                grouped_build_ms=round(t_group, 4), torch_yardstick_ms=round(t_yard, 4),
                speedup_vs_torch=round(t_yard / t_group, 2),
                grouped_bytes_GB=round(nbytes / 1e9, 4), grouped_flops_sym_G=round(flops_sym / 1e9, 2),
                grouped_flops_exec_G=round(flops_exec / 1e9, 2), grouped_roof_ms=round(roof, 4),
                roof_fraction=round(roof / t_group, 3), max_rel_err_vs_torch=float(f"{err:.2e}"),
                update_ms=round(t_update, 4), invert_ms=round(t_invert, 4), sample_and_replace_ms=round(t_sample, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--models", default="mobilenet_v2,resnext50_32x4d")
    a = ap.parse_args()
    for name in a.models.split(","):
        print(json.dumps(bench(name, a.batch, a.size, a.reps)), flush=True)


if __name__ == "__main__":
    main()
