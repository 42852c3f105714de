#!/usr/bin/env python
"""Linearised (GLM) predictive of INF (`ops.admit_inf_predictive`): time of `functional_variance` beside
KFAC's and EFB's on the same records, of the projection kernel alone, and of torch doing the same arithmetic.

    python tools/bench_inf_predictive.py [--batch 32] [--rank 100] [--reps 5] [--models resnet18,resnet50] [--json FILE]

Per model (N x 3 x 224 x 224, fp32; the records of one forward pass and of the backward pass of one output resident; the
chain KFAC -> EFB -> Diagonal -> INF, `update(rank)`, `invert(1, 1000)`):
  * `functional_variance` of INF, KFAC and EFB for that output with the input side (``inputs=True``) and without;
  * `ops.per_sample_project` alone on prepared operands (all layers in one call): the FLOPs its plan executes
    (curv_persample_project_plan_flops: the products plus the second MFMA) over its time as a fraction of the
    157.3 TFLOP/s fp32 MFMA peak (a call rate over peak, not a kernel's share of it), and the algorithmic FLOPs
    2 N m n (L + b) likewise;
  * the torch yardstick of INF's variance on the same GPU: `F.unfold`, `torch.bmm` to P_n, the Hadamard product with r**2,
    two matmuls into the eigenbasis and one with F; and of the projection alone (unfold, bmm, Hadamard, two matmuls).
HIP events around each call, median of `--reps` after two warm-up calls.
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
from curvature_amd.curvatures import EFB, INF, KFAC, Diagonal  # noqa: E402

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


def chain(model, x, labels, rank):
    """KFAC, EFB and INF of `model` after one update on (x, labels) in train() mode, inverted; KFAC keeps its hooks."""
    kfac, diag = KFAC(model), Diagonal(model)
    model.train()
    model.zero_grad()
    F.cross_entropy(model(x), labels).backward()
    kfac.update(x.shape[0])
    diag.update(x.shape[0])
    efb = EFB(model, kfac.state)
    efb.update(x.shape[0])
    inf = INF(model, diag.state, kfac.state, efb.state, eigvecs=efb.eigvecs)
    inf.update(rank=rank)
    model.eval()
    model.zero_grad()
    for est in (kfac, efb, inf):
        est.invert(add=1.0, multiply=1000.0)
    return {"inf": inf, "kfac": kfac, "efb": efb}


def unfolded(layer, x, g):
    """(G, X) of a layer's records as (N, m, L) and (N, n_in [+ 1], L)."""
    if layer.__class__.__name__ == "Conv2d":
        X = F.unfold(x, layer.kernel_size, padding=layer.padding, stride=layer.stride)
        G = g.reshape(g.shape[0], g.shape[1], -1)
    else:
        X = x.reshape(x.shape[0], -1, x.shape[-1]).transpose(1, 2)
        G = g.reshape(g.shape[0], -1, g.shape[-1]).transpose(1, 2)
    if layer.bias is not None:
        X = torch.cat([X, torch.ones_like(X[:, :1])], dim=1)
    return G, X


def torch_inf(inf, layers, record, terms, ws, variance=True):
    """INF's arithmetic in torch: per layer P_n = G X^T, T = r**2 o P_n, Q = U_G^T T U_A; with `variance` also
    sum r**2 P**2 - ||F q||**2 (F^T in the column order of `terms`: l a + k, the order of Q.flatten)."""
    total = 0
    for layer, w in zip(layers, ws):
        x, g = record[layer]
        G, X = unfolded(layer, x, g)
        ua, ug, ft = terms[layer]
        P = torch.bmm(G, X.transpose(1, 2))                          # (N, m, n)
        T = P * w
        Q = ug.t() @ T @ ua                                          # (N, b, a)
        if variance:
            y = Q.flatten(1) @ ft
            total = total + (T * P).sum((1, 2)) - y.square().sum(1)
        else:
            total = total + Q.sum()
    return total


def run_model(name, N, rank, reps, dev):
    torch.manual_seed(0)
    model = getattr(models, name)().to(dev).eval()
    x = torch.randn(N, 3, 224, 224, device=dev)
    labels = torch.randint(0, 1000, (N,), device=dev)
    ests = chain(model, x, labels, rank)
    kfac = ests["kfac"]
    logits = model(x)
    torch.autograd.grad(logits[:, 0].sum(), [p for p in model.parameters() if p.requires_grad])
    layers = kfac._layers()
    record = {l: [t.detach() for t in kfac.record[l]] for l in layers}
    rows = []
    results = {}
    for kind, est in ests.items():
        est.record = record
        out = torch.zeros(N, device=dev)
        row = dict(model=name, N=N, rank=rank, estimator=kind, layers=len(layers))
        row["first_output_ms"] = timed(lambda: est.functional_variance(out, inputs=True), reps)
        row["next_output_ms"] = timed(lambda: est.functional_variance(out, inputs=False), reps)
        results[kind] = out.clone()
        if kind != "inf":
            est.drop_predictive_state()
            rows.append(row)
            continue
        # the projection alone, on the operands and terms functional_variance has just used
        terms = est._lowrank_terms()
        kept = est._predictive_kept["variance"]
        operands = est._per_sample_operands("bench", layers)
        jobs, keep = [], []
        for layer, (s, g, xx), w in zip(layers, operands, kept["ws"]):
            ua, ug, ft = terms[layer]
            zt = torch.empty(s.N, ug.shape[1], s.n, device=dev)
            g, xx = g.clone(), xx.clone()
            keep.append((g, xx, zt))
            jobs.append(ops.PerSampleProjectJob.of(s, g, xx, w, ug, zt.permute(0, 2, 1), first=True))
        algo = sum(2 * j.S * j.M * j.Nc * (j.L + j.R) for j in jobs)
        executed = sum(ops.per_sample_project_plan_flops(jobs))
        row["projection_ms"] = ms = timed(lambda: ops.per_sample_project(jobs), reps)
        row.update(projection_workspace_mb=ops.per_sample_project_workspace_bytes(jobs) / 2 ** 20,
                   algorithmic_gflop=algo / 1e9, executed_gflop=executed / 1e9,
                   executed_rate_over_peak=executed / (ms * 1e-3) / PEAK_F32_MFMA,
                   algorithmic_rate_over_peak=algo / (ms * 1e-3) / PEAK_F32_MFMA,
                   low_rank_sizes=sorted({(int(terms[l][0].shape[1]), int(terms[l][1].shape[1])) for l in layers}))
        ws = list(kept["ws"])
        del jobs, keep
        est.drop_predictive_state()
        torch.cuda.empty_cache()
        want = torch_inf(est, layers, record, terms, ws)
        row["rel_difference_to_torch"] = float(torch.linalg.norm(results["inf"].double() - want.double()) /
                                               torch.linalg.norm(want.double()))
        row["torch_variance_ms"] = timed(lambda: torch_inf(est, layers, record, terms, ws), reps)
        row["torch_projection_ms"] = timed(lambda: torch_inf(est, layers, record, terms, ws, variance=False), reps)
        row["first_output_over_torch"] = row["first_output_ms"] / row["torch_variance_ms"]
        row["projection_over_torch"] = row["projection_ms"] / row["torch_projection_ms"]
        rows.append(row)
        del want
        torch.cuda.empty_cache()
        ops.release_workspaces()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rank", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--models", default="resnet18,resnet50")
    ap.add_argument("--json", default=None, help="append the rows as JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_inf_predictive: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    ops.admit_inf_predictive(True)
    for name in args.models.split(","):
        for r in run_model(name, args.batch, args.rank, args.reps, dev):
            print(json.dumps(r), flush=True)
            if args.json:
                with open(args.json, "a") as fh:
                    fh.write(json.dumps(r) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
