#!/usr/bin/env python
"""Per-sample Fisher on half-precision records and on transposed convolutions: time of `Diagonal(per_sample=True).update`.

    python tools/bench_per_sample_layers.py [--part half convt] [--batch 32] [--reps 5] [--runs 3] [--json FILE]

HIP events around `update()`, median of `--reps` calls after two warm-up calls (as tools/bench_per_sample.py).

  half   ResNet-50, N = 32, 224 x 224, bf16 autocast.  `update()` on the recorded bf16 / fp32 tensors (the pack upcasts
         them) against the route there was before half records were taken: `.float()` copies of the same records, made
         inside the timed region, then the float32 instantiation of the same pack and in-place reads.  `--runs`
         alternated runs of each.
         The split of pack against product comes from a kernel trace of this script with ``--part half``.
  convt  every ConvTranspose2d of the DCGAN generator (N = 64) and of the U-Net (N = 8, 256 x 256), one layer per call,
         against torch doing what a user would write: zero-stuff, `F.unfold`, `bmm`, square, sum.  Beside the time the
         algorithmic 2 N m n_in L and what the plan executes (curv_persample_plan_flops): the transposed X is dense with
         1 / (s_h s_w) of its entries nonzero.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from curvature_amd import models, ops  # noqa: E402
from curvature_amd.curvatures import Diagonal  # noqa: E402


def timed(fn, reps):
    """Median milliseconds of `fn()` between HIP events, after two warm-up calls."""
    for _ in range(2):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def half_records(N, reps, runs, dev):
    torch.manual_seed(0)
    model = models.resnet50().to(dev)
    x = torch.randn(N, 3, 224, 224, device=dev)
    labels = torch.randint(0, 1000, (N,), device=dev)
    diag = Diagonal(model, per_sample=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = F.cross_entropy(model(x).float(), labels)
    loss.backward()
    layers = diag._layers()
    record = {l: [t.detach() for t in diag.record[l]] for l in layers}
    half_sides = sum(t.dtype == torch.bfloat16 for r in record.values() for t in r)

    def on_half():
        diag.record = record
        diag.update(N)

    def on_copies():
        diag.record = {l: [t.float() for t in r] for l, r in record.items()}
        diag.update(N)
    rows = []
    for run in range(runs):
        rows.append(dict(part="half", run=run, route="half records, general pack", ms=timed(on_half, reps)))
        rows.append(dict(part="half", run=run, route=".float() copies, fp32 path", ms=timed(on_copies, reps)))
    for r in rows:
        r.update(model="resnet50", N=N, layers=len(layers), half_sides=int(half_sides))
    return rows


def zero_stuffed_columns(layer, x, out_size):
    """X of a transposed convolution with torch: zero-stuffed input padded by k - 1 - p, F.unfold, taps flipped."""
    N, C, H, W = x.shape
    (kh, kw), (sh, sw), (ph, pw) = layer.kernel_size, layer.stride, layer.padding
    Ho, Wo = out_size
    xs = x.new_zeros(N, C, (H - 1) * sh + 1, (W - 1) * sw + 1)
    xs[:, :, ::sh, ::sw] = x
    oph, opw = Ho - ((H - 1) * sh - 2 * ph + kh), Wo - ((W - 1) * sw - 2 * pw + kw)
    eh, ew = kh - 1 - ph, kw - 1 - pw
    xs = F.pad(xs, (ew, ew + opw, eh, eh + oph))
    return F.unfold(xs, (kh, kw)).view(N, C, kh, kw, -1).flip(2).flip(3).reshape(N, C * kh * kw, -1)


def convt_yardstick(layer, x, g):
    X = zero_stuffed_columns(layer, x, tuple(g.shape[2:]))
    if layer.bias is not None:
        X = torch.cat([X, torch.ones_like(X[:, :1])], dim=1)
    P = torch.bmm(g.flatten(2), X.transpose(1, 2))
    return P.square_().sum(0).mul_(x.shape[0])


SETUPS = {"dcgan_generator": (64, lambda n: (n, 100, 1, 1)), "unet": (8, lambda n: (n, 3, 256, 256))}


def transposed(reps, dev):
    rows = []
    for name, (N, shape) in SETUPS.items():
        torch.manual_seed(0)
        model = getattr(models, name)().to(dev)
        diag = Diagonal(model, ['ConvTranspose2d'], per_sample=True)
        model(torch.randn(*shape(N), device=dev)).square().mean().backward()
        for i, layer in enumerate(diag._layers()):
            x, g = (t.detach() for t in diag.record[layer])
            est = Diagonal(torch.nn.Sequential(layer), ['ConvTranspose2d'], per_sample=True)
            est.record = {layer: [x, g]}
            s = ops.per_sample_operands(layer, x, g)
            executed = ops.per_sample_plan_flops([ops.PerSampleJob.of(s, None, None, None)])[0]
            ms = timed(lambda: est.update(N), reps)
            ms_torch = timed(lambda: convt_yardstick(layer, x, g), reps)
            want = convt_yardstick(layer, x, g)
            err = float((est.state[layer] / (2 + reps) - want).norm() / want.norm())       # (every call accumulated)
            rows.append(dict(part="convt", model=name, layer=i, N=N, input=list(x.shape[1:]), kernel=list(layer.kernel_size),
                             stride=list(layer.stride), m=s.m, n=s.n, L=s.L, algorithmic_gflop=2 * s.N * s.m * s.n * s.L / 1e9,
                             executed_gflop=executed / 1e9, ms=ms, torch_ms=ms_torch, rel_err_vs_torch=err))
        ops.release_workspaces()
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=["half", "convt"], choices=["half", "convt"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", default=None, help="append the rows as JSON lines to this file")
    args = ap.parse_args()
    ops.widen_per_sample(True)                             # half records and ConvTranspose2d are the wider, opt-in line
    dev = torch.device("cuda:0")
    rows = []
    if "half" in args.part:
        rows += half_records(args.batch, args.reps, args.runs, dev)
    if "convt" in args.part:
        rows += transposed(args.reps, dev)
    for r in rows:
        print(json.dumps(r))
    if args.json:
        with open(args.json, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
