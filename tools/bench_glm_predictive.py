#!/usr/bin/env python
"""Linearised Laplace (GLM) predictive: time of `functional_variance` and `glm_predictive` beside torch doing the same
arithmetic on the same device.

    python tools/bench_glm_predictive.py [--batch 32] [--reps 5] [--no-resnet] [--no-lenet] [--json FILE]

  * ResNet-50 at N x 3 x 224 x 224, fp32, records of one forward pass and of the backward pass of one output resident:
    `functional_variance` of KFAC and Diagonal for that output with the input side (``inputs=True``, the first output of
    a batch) and without (``inputs=False``, every further output); the per-sample reduction alone
    (`ops.per_sample_quad_reduce` on prepared operands: the product and the reduce launch of all layers); the FLOPs its
    plan executes (curv_persample_quad_plan_flops) and those over the reduction's time as a fraction of the 157.3 TFLOP/s
    fp32 MFMA peak (a call rate over peak, not a kernel's share of it);
  * LeNet-5 at N = 100, all 10 outputs: `glm_predictive`, forward and backward passes included;
  * the torch yardstick of each: `F.unfold`, the rotations as matmuls, `torch.bmm` to (N, m, n_in), square, weigh, sum.
HIP events around each call, median of `--reps` after two warm-up calls.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from curvature_amd import models, ops  # noqa: E402
from curvature_amd.curvatures import KFAC, Diagonal  # noqa: E402
from curvature_amd.evaluate import glm_predictive  # noqa: E402

PEAK_F32_MFMA = 157.3e12


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


def estimators(model, x, labels):
    """KFAC and Diagonal of `model` after one update on (x, labels), in train() mode (see bench_glm_covariance.py), and
    an inversion."""
    kfac, diag = KFAC(model), Diagonal(model, per_sample=True)
    model.train()
    model.zero_grad()
    F.cross_entropy(model(x), labels).backward()
    kfac.update(x.shape[0])
    diag.update(x.shape[0])
    model.eval()
    kfac.invert(add=1.0, multiply=1000.0)
    diag.invert(add=1.0, multiply=1000.0)
    return {"kfac": kfac, "diagonal": diag}


def grad_matrix(layer, g):
    """G of a layer's grad_output as (N, m, L)."""
    if layer.__class__.__name__ == "Conv2d":
        return g.reshape(g.shape[0], g.shape[1], -1)
    return g.reshape(g.shape[0], -1, g.shape[-1]).transpose(1, 2)


def unfolded(layer, x, g):
    """(G, X) of a layer's records as (N, m, L) and (N, n_in [+ 1], L)."""
    if layer.__class__.__name__ == "Conv2d":
        X = F.unfold(x, layer.kernel_size, padding=layer.padding, stride=layer.stride)
    else:
        X = x.reshape(x.shape[0], -1, x.shape[-1]).transpose(1, 2)
    if layer.bias is not None:
        X = torch.cat([X, torch.ones_like(X[:, :1])], dim=1)
    return grad_matrix(layer, g), X


def torch_variance(kind, est, layers, record, inputs=True, kept=None):
    """The same arithmetic in torch; `kept`: the (rotated) X of every layer from a call with ``inputs=True``."""
    total, xs = 0, []
    for k, layer in enumerate(layers):
        x, g = record[layer]
        if inputs:
            G, X = unfolded(layer, x, g)
            if kind == "kfac":
                X = est.inv_state[layer][0].t() @ X
        else:
            G, X = grad_matrix(layer, g), kept[k]
        xs.append(X)
        if kind == "kfac":
            P = torch.bmm(est.inv_state[layer][1].t() @ G, X.transpose(1, 2))
            total = total + P.square_().sum((1, 2))
        else:
            P = torch.bmm(G, X.transpose(1, 2))
            total = total + (P.square_() * est.inv_state[layer].square()).sum((1, 2))
    return total, xs


def quad_jobs(kind, est, layers, out_rows):
    """The reduction of every layer on prepared operands (KFAC: rotated as `functional_variance` rotates them)."""
    layout = dict(rows_outer=True, in_place=False) if kind == "kfac" else {}
    operands = est._per_sample_operands("bench", layers, **layout)
    jobs = []
    for k, (layer, (s, g, x)) in enumerate(zip(layers, operands)):
        w = None
        if kind == "kfac":
            L_A, L_G = est.inv_state[layer]
            t, y = torch.empty_like(g), torch.empty_like(x)
            ops.gemm_batched([ops.Gemm(L_G.t(), g.view(s.m, -1), t.view(s.m, -1)),
                              ops.Gemm(L_A.t(), x.view(s.n, -1), y.view(s.n, -1))])
            g, x = t, y
        else:
            g, x, w = g.clone(), x.clone(), est.inv_state[layer].square()
        jobs.append(ops.PerSampleQuadJob.of(s, g, x, w, out_rows[k], first=True))
    return jobs


def run_resnet(N, reps, dev):
    torch.manual_seed(0)
    model = models.resnet50().to(dev).eval()
    x = torch.randn(N, 3, 224, 224, device=dev)
    labels = torch.randint(0, 1000, (N,), device=dev)
    ests = estimators(model, x, labels)
    logits = model(x)
    torch.autograd.grad(logits[:, 0].sum(), [p for p in model.parameters() if p.requires_grad])
    rows = []
    for kind, est in ests.items():
        layers = est._layers()
        record = {l: [t.detach() for t in est.record[l]] for l in layers}
        est.record = record
        out = torch.zeros(N, device=dev)
        row = dict(model="resnet50", N=N, estimator=kind, layers=len(layers))
        row["first_output_ms"] = timed(lambda: est.functional_variance(out, inputs=True), reps)
        row["next_output_ms"] = timed(lambda: est.functional_variance(out, inputs=False), reps)
        mine = out.clone()
        est.drop_predictive_state()
        jobs = quad_jobs(kind, est, layers, torch.empty(len(layers), N, device=dev))
        algo = sum(2 * j.S * j.M * j.Nc * j.L for j in jobs)
        executed = sum(ops.per_sample_quad_plan_flops(jobs))
        row["reduction_ms"] = ms = timed(lambda: ops.per_sample_quad_reduce(jobs), reps)
        row.update(algorithmic_gflop=algo / 1e9, executed_gflop=executed / 1e9,
                   executed_rate_over_peak=executed / (ms * 1e-3) / PEAK_F32_MFMA,
                   algorithmic_rate_over_peak=algo / (ms * 1e-3) / PEAK_F32_MFMA)
        del jobs
        torch.cuda.empty_cache()
        want, kept = torch_variance(kind, est, layers, record)
        row["rel_difference_to_torch"] = float(torch.linalg.norm(mine.double() - want.double()) / torch.linalg.norm(want.double()))
        row["torch_first_output_ms"] = timed(lambda: torch_variance(kind, est, layers, record), reps)
        row["torch_next_output_ms"] = timed(lambda: torch_variance(kind, est, layers, record, False, kept), reps)
        rows.append(row)
        del kept, want
        torch.cuda.empty_cache()
        ops.release_workspaces()
    return rows


def run_lenet(reps, dev, N=100):
    torch.manual_seed(0)
    model = models.lenet5().to(dev).eval()
    x = torch.randn(N, 1, 28, 28, device=dev)
    labels = torch.randint(0, 10, (N,), device=dev)
    ests = estimators(model, x, labels)
    params = list(model.parameters())
    rows = []
    for kind, est in ests.items():
        layers = est._layers()

        def in_torch():
            logits = model(x)
            variance, kept = torch.zeros_like(logits), None
            for c in range(10):
                torch.autograd.grad(logits[:, c].sum(), params, retain_graph=True)
                variance[:, c], xs = torch_variance(kind, est, layers, est.record, c == 0, kept)
                kept = kept or xs
            return variance, torch.softmax(logits.detach() / torch.sqrt(1 + math.pi / 8 * variance), dim=1)

        mine, want = glm_predictive(model, est, x)[1], in_torch()[0]
        rows.append(dict(model="lenet5", N=N, estimator=kind, layers=len(layers), outputs=10,
                         glm_predictive_ms=timed(lambda: glm_predictive(model, est, x), reps),
                         torch_ms=timed(in_torch, reps),
                         rel_difference_to_torch=float(torch.linalg.norm(mine.double() - want.double()) /
                                                       torch.linalg.norm(want.double()))))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-resnet", action="store_true")
    ap.add_argument("--no-lenet", action="store_true")
    ap.add_argument("--json", default=None, help="append the rows as JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_glm_predictive: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    rows = []
    if not args.no_lenet:
        rows += run_lenet(args.reps, dev)
    if not args.no_resnet:
        rows += run_resnet(args.batch, args.reps, dev)
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
