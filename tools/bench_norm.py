"""The fused normalisation-layer passes (csrc/norm_factor.hip) on two layer sets, N = 32:
  - resnet50_bn: the 53 BatchNorm2d layers of a ResNet-50 at 224 x 224, eval mode (given statistics);
  - vit_b_ln:    the 25 LayerNorms of a ViT-B/16 (T = 197, D = 768).
HIP-event times, the candidates run in turn inside every round (so drift and neighbours hit all alike), of
  - per_sample_sq: `ops.per_sample_norm_sq_accumulate`, every layer of the set in one call (the exact Fisher diagonal),
  - kfac_build:    `ops.kfac_accumulate_norm`, the A and G factors of every layer in one call,
  - torch:         per layer ``xh = F.*_norm(x, no affine); p = (g * xh).sum(positions); (p ** 2).sum(0)`` and the same for
                   the bias column - what the per-sample pass replaces; it writes two activation-sized temporaries,
with the median and the spread over the rounds, the bytes the algorithm needs (curv_persample_norm_plan_info: x twice -
once with given statistics - and g once; the factor build: x twice / once, then g once) and the fraction of the HBM peak
(`--peak-gbps`, 8000 for an MI355X) they amount to, and the error of the fused pass against the torch expression.

    python tools/bench_norm.py [--rounds 5] [--reps 3] [--channels-last] [--sets resnet50_bn vit_b_ln]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn as nn
import torch.nn.functional as F

from curvature_amd import ops

N = 32


def resnet50_bn():
    """(C, H) of the 53 BatchNorm2d layers (torchvision's v1.5 block: the stride sits on the 3 x 3 convolution)."""
    shapes = [(64, 112)]
    res = 56
    for width, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)):
        for b in range(blocks):
            out = res // stride if b == 0 else res
            shapes += [(width, res), (width, out), (4 * width, out)]
            if b == 0:
                shapes.append((4 * width, out))
            res = out
    assert len(shapes) == 53
    return shapes


def make_set(name, dev, channels_last):
    torch.manual_seed(0)
    items = []
    if name == "resnet50_bn":
        for C, H in resnet50_bn():
            layer = nn.BatchNorm2d(C).to(dev).eval()
            layer.running_mean.normal_()
            layer.running_var.uniform_(0.5, 1.5)
            x, g = torch.randn(N, C, H, H, device=dev), torch.randn(N, C, H, H, device=dev)
            if channels_last:
                x, g = (t.contiguous(memory_format=torch.channels_last) for t in (x, g))
            items.append((layer, x, g))
    else:
        for _ in range(25):
            items.append((nn.LayerNorm(768).to(dev), torch.randn(N, 197, 768, device=dev), torch.randn(N, 197, 768, device=dev)))
    return items


def torch_expression(layer, x, g):
    if isinstance(layer, nn.LayerNorm):
        xh = F.layer_norm(x, layer.normalized_shape, None, None, layer.eps)
        return torch.stack([(g * xh).sum(1).square().sum(0), g.sum(1).square().sum(0)], 1)
    xh = F.batch_norm(x, layer.running_mean, layer.running_var, None, None, False, 0.0, layer.eps)
    return torch.stack([(g * xh).sum((2, 3)).square().sum(0), g.sum((2, 3)).square().sum(0)], 1)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(values):
    return dict(median=round(statistics.median(values), 4), min=round(min(values), 4), max=round(max(values), 4))


def bench(name, rounds, reps, channels_last, peak_gbps):
    dev = torch.device("cuda:0")
    was = ops.admit_norm_layers(True)
    try:
        items = make_set(name, dev, channels_last)
        dsts = [torch.empty(l.weight.numel(), 2, device=dev) for l, _, _ in items]
        per = [ops.PerSampleNormJob.of(l, x, g, dst=d, alpha=float(N), first=True) for (l, x, g), d in zip(items, dsts)]
        fac = []
        for layer, x, g in items:
            sides = ops.factor_jobs(layer, x, g)
            C = layer.weight.numel()
            sides.a.dst, sides.a.first = torch.empty(C, 2, 2, device=dev), True
            sides.g.dst, sides.g.first = torch.empty(C, 1, 1, device=dev), True
            fac += [sides.a, sides.g]
        candidates = dict(per_sample_sq=lambda: ops.per_sample_norm_sq_accumulate(per),
                          kfac_build=lambda: ops.kfac_accumulate_norm(fac),
                          torch=lambda: [torch_expression(*item) for item in items])
        for fn in candidates.values():
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in candidates}
        for _ in range(rounds):
            for k, fn in candidates.items():
                times[k].append(timed(fn, reps))
        ops.per_sample_norm_sq_accumulate(per)
        err = max(float((d - N * torch_expression(*item)).norm() / (N * torch_expression(*item)).norm())
                  for d, item in zip(dsts, items))
        _, nbytes = ops.per_sample_norm_plan_info(per)
        elems = sum(x.numel() for _, x, _ in items)
        given = name == "resnet50_bn"
        algo = dict(per_sample_sq=sum(nbytes), kfac_build=4 * elems * (2 if given else 3), torch=sum(nbytes))
        med = {k: statistics.median(v) for k, v in times.items()}
        return dict(set=name, layers=len(items), N=N, channels_last=channels_last, activation_GB=round(4 * elems / 1e9, 3),
                    ms={k: spread(v) for k, v in times.items()},
                    algorithmic_GB={k: round(v / 1e9, 3) for k, v in algo.items()},
                    GBps={k: round(algo[k] / med[k] / 1e6, 1) for k in med},
                    hbm_fraction={k: round(algo[k] / med[k] / 1e6 / peak_gbps, 3) for k in med},
                    speedup_vs_torch=round(med["torch"] / med["per_sample_sq"], 3),
                    max_rel_err_vs_torch=float(f"{err:.2e}"))
    finally:
        ops.admit_norm_layers(was)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--channels-last", action="store_true")
    ap.add_argument("--peak-gbps", type=float, default=8000.0)
    ap.add_argument("--sets", nargs="+", default=["resnet50_bn", "vit_b_ln"])
    a = ap.parse_args()
    for name in a.sets:
        print(json.dumps(bench(name, a.rounds, a.reps, a.channels_last and name == "resnet50_bn", a.peak_gbps)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
