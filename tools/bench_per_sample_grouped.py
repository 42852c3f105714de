#!/usr/bin/env python
"""Per-sample Fisher and GLM variance of grouped and depthwise convolutions (`ops.admit_grouped_per_sample`).

    python tools/bench_per_sample_grouped.py [--model mobilenet_v2 resnext50_32x4d] [--batch 32] [--reps 5] [--json FILE]

Records resident (one forward / backward at N x 3 x 224 x 224, ``eval()`` mode), HIP events, median of `--reps` calls
after two warm-up calls; the library and its yardstick alternate call by call in one process.  Per model and layer class
(depthwise, group slices, ordinary, all) it prints, and appends as JSON lines to ``--json``:
  * `Diagonal(per_sample=True).update` beside the torch yardstick (`F.unfold` on the channel-sliced input, `einsum` to
    (N, C_out, n_g), square, sum);
  * one `KFAC.functional_variance` (one output, ``inputs=True``) for the grouped classes and the whole model;
  * depthwise layers only: the same `update` with the slices route forced onto them (one product per channel on the
    MFMA tile) - the comparison the direct kernel exists for - and the direct kernel alone
    (`ops.per_sample_dw_sq_accumulate`): needed bytes 4 N C (H W + Ho Wo) over its time as a share of the 8.0 TB/s HBM peak;
  * group slices: algorithmic and executed GFLOP of their products (`ops.per_sample_plan_flops`) and their ratio.
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
from curvature_amd.curvatures import KFAC, Diagonal  # noqa: E402

HBM_PEAK = 8.0e12                     # bytes / s (spec; 6.29e12 measured with a float4 copy)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternating(fns, reps):
    """Median milliseconds of every function of `fns`, called in turn: two warm-up rounds, then `reps` timed ones."""
    for _ in range(2):
        for fn in fns:
            fn()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            times[k].append(event_ms(fn))
    return [statistics.median(t) for t in times]


def torch_yardstick(layers, record, N):
    """What a user would write: unfold the channel-sliced input, per-sample gradients by einsum, square, sum."""
    out = []
    for layer in layers:
        x, g = record[layer]
        if layer.__class__.__name__ != "Conv2d":
            P = torch.einsum("nm,nk->nmk", g, torch.cat([x, torch.ones_like(x[:, :1])], 1) if layer.bias is not None else x)
            out.append(P.square_().sum(0).mul_(N))
            continue
        G = int(layer.groups)
        X = F.unfold(x, layer.kernel_size, padding=layer.padding, stride=layer.stride)          # (N, C kh kw, L)
        X = X.reshape(N, G, -1, X.shape[-1])
        gs = g.reshape(N, G, layer.out_channels // G, -1)
        P = torch.einsum("ngml,ngkl->ngmk", gs, X).reshape(N, layer.out_channels, -1)
        if layer.bias is not None:
            P = torch.cat([P, gs.sum(-1).reshape(N, -1, 1)], 2)
        out.append(P.square_().sum(0).mul_(N))
    return out


def sub_diagonal(layers, record):
    est = Diagonal(torch.nn.Sequential(*layers), per_sample=True)
    est.record = {l: record[l] for l in layers}
    return est


def sub_kfac(layers, full):
    est = KFAC(torch.nn.Sequential(*layers))
    est.record = {l: full.record[l] for l in layers}
    est.state = {l: full.state[l] for l in layers}
    est.inv_state = {l: full.inv_state[l] for l in layers}
    return est


def run(name, N, reps, dev):
    torch.manual_seed(0)
    model = getattr(models, name)().to(dev).eval()
    x = torch.randn(N, 3, 224, 224, device=dev)
    labels = torch.randint(0, 1000, (N,), device=dev)
    diag = Diagonal(model, per_sample=True)
    kfac = KFAC(model)
    logits = model(x)
    F.cross_entropy(logits, labels).backward(retain_graph=True)
    kfac.update(N)
    kfac.invert(add=1.0, multiply=1.0)
    layers = diag._layers()
    record = {l: [t.detach() for t in diag.record[l]] for l in layers}
    # the records of the predictive: the same forward pass, one output back-propagated
    torch.autograd.grad(logits[:, 0].sum(), [p for p in model.parameters() if p.requires_grad])
    classes = {"depthwise": [], "slices": [], "whole": []}
    for layer in layers:
        classes[ops.per_sample_route(layer)].append(layer)
    out = torch.empty(N, device=dev)
    rows = []
    for cls, members in [("all", layers)] + [(c, m) for c, m in classes.items() if m]:
        est = diag if cls == "all" else sub_diagonal(members, record)
        ms, ms_torch = alternating([lambda: est.update(N), lambda: torch_yardstick(members, record, N)], reps)
        row = dict(model=name, N=N, layer_class=cls, layers=len(members), update_ms=ms, torch_ms=ms_torch)
        if cls != "whole":
            pred = kfac if cls == "all" else sub_kfac(members, kfac)
            row["kfac_variance_ms"] = alternating([lambda: pred.functional_variance(out, inputs=True)], reps)[0]
            pred.drop_predictive_state()
        if cls == "slices":
            algo = executed = 0
            for item in ops.per_sample_items(members):
                s = ops.per_sample_operands(item, *record[item.layer])
                algo += 2 * s.N * s.m * s.n * s.L
                executed += ops.per_sample_plan_flops([ops.PerSampleJob.of(s, None, None, None)])[0]
            row.update(algorithmic_gflop=algo / 1e9, executed_gflop=executed / 1e9, executed_over_algorithmic=executed / algo)
        if cls == "depthwise":
            jobs = [ops.PerSampleDwJob.of(l, *record[l], dst=est.state[l], alpha=N, first=True) for l in members]
            needed = sum(ops.per_sample_dw_plan_info(jobs)[1])
            kernel_ms = alternating([lambda: ops.per_sample_dw_sq_accumulate(jobs)], reps)[0]
            row.update(needed_gbytes=needed / 1e9, direct_kernel_ms=kernel_ms,
                       hbm_peak_share=needed / (kernel_ms * 1e-3) / HBM_PEAK)
            route, ops.per_sample_route = ops.per_sample_route, lambda layer: "slices" if route(layer) != "whole" else "whole"
            try:
                forced = sub_diagonal(members, record)
                row["update_as_slices_ms"] = alternating([lambda: forced.update(N)], max(1, reps // 2))[0]
                row["slice_products"] = len(ops.per_sample_items(members))
            finally:
                ops.per_sample_route = route
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", nargs="+", default=["mobilenet_v2", "resnext50_32x4d"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None, help="append the rows as JSON lines to this file")
    args = ap.parse_args()
    ops.admit_grouped_per_sample(True)
    dev = torch.device("cuda:0")
    for name in args.model:
        rows = run(name, args.batch, args.reps, dev)
        print(f"\n{name}, N = {args.batch}")
        for r in rows:
            print("  " + "  ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in r.items()
                                   if k not in ("model", "N")), flush=True)
        if args.json:
            with open(args.json, "a") as fh:
                for r in rows:
                    fh.write(json.dumps(r) + "\n")
        torch.cuda.empty_cache()
        ops.release_workspaces()


if __name__ == "__main__":
    main()
