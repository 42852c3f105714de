#!/usr/bin/env python
"""Per-sample Fisher and GLM variance of grouped and depthwise convolutions (`ops.admit_grouped_per_sample`),
and with ``--joint`` their joint covariance and damping grid (`ops.admit_grouped_joint`).

    python tools/bench_per_sample_grouped.py [--model mobilenet_v2 resnext50_32x4d] [--batch 32] [--reps 5] [--json FILE]
                                             [--joint]

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

``--joint`` times instead, for KFAC, per layer class (all, depthwise, group slices): one `functional_variance`, one
`stage_output` (``inputs=False``), `stage_output` x 10 + `functional_covariance`, one `functional_variance_grid` with 16
pairs, and `KFAC.decompose()` once (host clock around a synchronise); for the two grouped classes beside a torch yardstick
that computes the same covariance / grid rows from `F.unfold` / `einsum` per-sample gradients.  Group slices: executed
over algorithmic GFLOP of `ops.per_sample_cov_plan_flops` and `ops.per_sample_quad_grid_plan_flops`.
"""
import argparse
import json
import os
import statistics
import sys
import time

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
        out.append(conv_gradients(layer, x, g, N).reshape(N, layer.out_channels, -1).square_().sum(0).mul_(N))
    return out


def conv_gradients(layer, x, g, N):
    """The per-sample gradients (N, G, m_g, n_g) of a (grouped) Conv2d with respect to [W | b], per group."""
    G = int(layer.groups)
    X = F.unfold(x, layer.kernel_size, padding=layer.padding, stride=layer.stride)          # (N, C kh kw, L)
    X = X.reshape(N, G, -1, X.shape[-1])
    gs = g.reshape(N, G, layer.out_channels // G, -1)
    P = torch.einsum("ngml,ngkl->ngmk", gs, X)
    if layer.bias is not None:
        P = torch.cat([P, gs.sum(-1, keepdim=True)], 3)
    return P


def torch_covariance(layers, record, kfac, N, K):
    """The joint covariance of K outputs (all from the same records, as the timed library calls) of grouped layers."""
    cov = 0
    for layer in layers:
        L_A, L_G = kfac.inv_state[layer]
        Y = torch.stack([torch.einsum("gim,ngij,gjk->ngmk", L_G, conv_gradients(layer, *record[layer], N), L_A).reshape(N, -1)
                         for _ in range(K)], 1)
        cov = cov + Y @ Y.transpose(1, 2)
    return cov


def torch_grid(layers, record, kfac, N, hypers):
    """`functional_variance_grid` of grouped layers: rotate into the eigenbases, square, weigh per damping pair."""
    out = 0
    for layer in layers:
        U_Gt, U_At, lam_G, lam_A = kfac._decomposition[layer][:4]
        Q = torch.einsum("gmi,ngij,gkj->ngmk", U_Gt, conv_gradients(layer, *record[layer], N), U_At).square_()
        rows = []
        for add, multiply in hypers:
            shift = (add / multiply) ** 0.5
            rows.append((Q / ((lam_G[None, :, :, None] + shift) * (lam_A[None, :, None, :] + shift))).sum((1, 2, 3)) / multiply)
        out = out + torch.stack(rows)
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


def run_joint(name, N, reps, dev, outputs=10, pairs=16):
    torch.manual_seed(0)
    model = getattr(models, name)().to(dev).eval()
    x = torch.randn(N, 3, 224, 224, device=dev)
    labels = torch.randint(0, 1000, (N,), device=dev)
    kfac = KFAC(model)
    logits = model(x)
    F.cross_entropy(logits, labels).backward(retain_graph=True)
    kfac.update(N)
    kfac.invert(add=1.0, multiply=1.0)
    kfac.decompose()                                                             # (warm-up: code objects, workspaces)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kfac.decompose()
    torch.cuda.synchronize()
    decompose_ms = (time.perf_counter() - t0) * 1e3
    torch.autograd.grad(logits[:, 0].sum(), [p for p in model.parameters() if p.requires_grad])
    layers = kfac._layers()
    record = {l: [t.detach() for t in kfac.record[l]] for l in layers}
    classes = {"depthwise": [], "slices": [], "whole": []}
    for layer in layers:
        classes[ops.per_sample_route(layer)].append(layer)
    matrices = sum(f.shape[0] if f.dim() == 3 else 1 for l in layers for f in kfac.state[l])
    hypers = [(10.0 ** (-3 + 0.25 * h), 1.0 + h) for h in range(pairs)]
    out, grid = torch.empty(N, device=dev), torch.empty(pairs, N, device=dev)
    cov = torch.empty(N, outputs, outputs, device=dev)
    rows = []
    for cls, members in [("all", layers)] + [(c, m) for c, m in classes.items() if m and c != "whole"]:
        pred = kfac if cls == "all" else sub_kfac(members, kfac)
        pred._decomposition = {l: kfac._decomposition[l] for l in members}

        def joint():
            for k in range(outputs):
                pred.stage_output(k, outputs, inputs=k == 0)
            pred.functional_covariance(cov)
        joint()                                                                  # (leaves a staged state for stage_output)
        fns = [lambda: pred.functional_variance(out, inputs=True), lambda: pred.stage_output(1, outputs), joint,
               lambda: pred.functional_variance_grid(grid, hypers, inputs=True)]
        if cls != "all":
            fns += [lambda: torch_covariance(members, record, kfac, N, outputs), lambda: torch_grid(members, record, kfac, N, hypers)]
        ms = alternating(fns, reps)
        row = dict(model=name, N=N, layer_class=cls, layers=len(members), variance_ms=ms[0], stage_output_ms=ms[1],
                   stage_x10_covariance_ms=ms[2], grid_16_pairs_ms=ms[3])
        if cls != "all":
            row.update(torch_covariance_ms=ms[4], torch_grid_ms=ms[5])
        else:
            row.update(decompose_ms=decompose_ms, decomposed_matrices=matrices)
        if cls == "depthwise":
            row.update(stage_over_variance=ms[1] / ms[0], grid_over_variance=ms[3] / ms[0])
        if cls == "slices":
            algo = cov_executed = grid_executed = 0
            for item in ops.per_sample_items(members):
                s = ops.per_sample_operands(item, *record[item.layer], rows_outer=True, in_place=False)
                algo += 2 * s.N * s.m * s.n * s.L
                cov_executed += ops.per_sample_cov_plan_flops([ops.PerSampleCovJob.of(s, None, None, None, None, outputs, 0)])[0]
                grid_executed += ops.per_sample_quad_grid_plan_flops(
                    [ops.PerSampleGridJob.of(s, None, None, None, None, None, None, [1.0] * pairs, [1.0] * pairs)])[0]
            row.update(algorithmic_gflop=algo / 1e9, cov_executed_gflop=cov_executed / 1e9,
                       cov_executed_over_algorithmic=cov_executed / (outputs * algo), grid_executed_gflop=grid_executed / 1e9,
                       grid_executed_over_algorithmic=grid_executed / algo)
        pred.drop_predictive_state()
        rows.append(row)
    return rows


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
    ap.add_argument("--joint", action="store_true", help="time the joint covariance and the damping grid (K15) instead")
    args = ap.parse_args()
    ops.admit_grouped_per_sample(True)
    ops.admit_grouped_joint(args.joint)
    dev = torch.device("cuda:0")
    for name in args.model:
        rows = (run_joint if args.joint else run)(name, args.batch, args.reps, dev)
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
