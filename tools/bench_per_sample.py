#!/usr/bin/env python
"""Exact per-sample Fisher (``per_sample=True`` of Diagonal / EFB): time of `update()` on the records of one batch.

    python tools/bench_per_sample.py [--model resnet50 resnet18] [--batch 32] [--reps 5] [--no-efb] [--no-single]

Records resident (one forward / backward at N x 3 x 224 x 224), HIP events around `update()`, median of `--reps` calls
after two warm-up calls.  Per model it prints, and appends as JSON lines to ``--json``:
  * Diagonal: algorithmic GFLOP (2 N m n_in L), executed GFLOP (curv_persample_plan_flops), time and the fraction of the
    157.3 TFLOP/s fp32 MFMA roof, for the whole model and per layer class (each class in a call of its own);
  * the kernel yardstick: torch doing what a user would write (`F.unfold`, `torch.bmm` to (N, m, n_in), square, sum);
  * EFB: the whole `update()`, its two rotations per layer alone (the batched GEMMs) and the algorithmic GFLOP of both;
  * the use-case yardstick: N passes at batch size 1 through the default `Diagonal.update(1)` / `EFB.update(1)`, forward
    and backward included.
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
from curvature_amd.curvatures import EFB, Diagonal  # noqa: E402

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


def layer_class(layer):
    if layer.__class__.__name__ == "Linear":
        return "linear"
    k, s = layer.kernel_size[0], layer.stride[0]
    return f"conv{k}x{k}" + (f"/s{s}" if s > 1 else "")


def flops_of(layer, record):
    """(algorithmic, executed) multiply-add flops of the layer's per-sample product."""
    s = ops.per_sample_operands(layer, *record)
    job = ops.PerSampleJob.of(s, None, None, None)
    return 2 * s.N * s.m * s.n * s.L, ops.per_sample_plan_flops([job])[0]


def bmm_yardstick(layers, record, N):
    """What a user would write: unfold, per-sample products as one bmm, square, sum."""
    out = []
    for layer in layers:
        x, g = record[layer]
        if layer.__class__.__name__ == "Conv2d":
            X = F.unfold(x, layer.kernel_size, padding=layer.padding, stride=layer.stride)       # (N, n_in, L)
            G = g.reshape(g.shape[0], g.shape[1], -1)
        else:
            X, G = x.reshape(N, -1, x.shape[-1]).transpose(1, 2), g.reshape(N, -1, g.shape[-1]).transpose(1, 2)
        if layer.bias is not None:
            X = torch.cat([X, torch.ones_like(X[:, :1])], dim=1)
        P = torch.bmm(G, X.transpose(1, 2))
        out.append(P.square_().sum(0).mul_(N))
    return out


def sub_estimator(layers, record):
    est = Diagonal(torch.nn.Sequential(*layers), per_sample=True)
    est.record = {l: record[l] for l in layers}
    return est


def run(name, N, reps, do_efb, do_single, dev):
    torch.manual_seed(0)
    model = getattr(models, name)().to(dev)
    x = torch.randn(N, 3, 224, 224, device=dev)
    labels = torch.randint(0, 1000, (N,), device=dev)
    diag = Diagonal(model, per_sample=True)
    layers = diag._layers()

    def fwd_bwd(xs, ys):
        model.zero_grad()
        F.cross_entropy(model(xs), ys).backward()

    fwd_bwd(x, labels)
    record = {l: [t.detach() for t in diag.record[l]] for l in layers}
    rows = []
    classes = {}
    for layer in layers:
        classes.setdefault(layer_class(layer), []).append(layer)
    for cls, members in [("all", layers)] + sorted(classes.items()):
        algo, executed = map(sum, zip(*(flops_of(l, record[l]) for l in members)))
        est = sub_estimator(members, record) if cls != "all" else diag
        ms = timed(lambda: est.update(N), reps)
        ms_bmm = timed(lambda: bmm_yardstick(members, record, N), reps)
        rows.append(dict(model=name, N=N, estimator="diagonal", layer_class=cls, layers=len(members),
                         algorithmic_gflop=algo / 1e9, executed_gflop=executed / 1e9, ms=ms,
                         roof_fraction=algo / (ms * 1e-3) / PEAK_F32_MFMA,
                         executed_roof_fraction=executed / (ms * 1e-3) / PEAK_F32_MFMA, bmm_ms=ms_bmm))
    eig = None
    if do_efb or do_single:
        eig = {}
        for layer in layers:
            m, n = diag.state[layer].shape
            eig[layer] = tuple(torch.linalg.qr(torch.randn(k, k, device=dev))[0].contiguous() for k in (n, m))
    if do_efb:
        efb = EFB(model, {}, eigvecs=eig, per_sample=True)
        efb.record = record
        ms = timed(lambda: efb.update(N), reps)
        operands = efb._per_sample_operands("EFB", layers, rows_outer=True, in_place=False)
        gemms, rot = [], 0
        for layer, (s, g, xx) in zip(layers, operands):
            U_At, U_Gt = efb._eigvecs_t(layer)
            cols = s.N * s.g.Lp
            gemms.append(ops.Gemm(U_Gt, g.view(s.m, cols), torch.empty(s.m, cols, device=dev)))
            gemms.append(ops.Gemm(U_At, xx.view(s.n, cols), torch.empty(s.n, cols, device=dev)))
            rot += 2 * (s.m * s.m + s.n * s.n) * s.N * s.L
        ms_rot = timed(lambda: ops.gemm_batched(gemms), reps)
        algo = 2 * rows[0]["algorithmic_gflop"] * 1e9 + rot
        rows.append(dict(model=name, N=N, estimator="efb", layer_class="all", layers=len(layers),
                         algorithmic_gflop=algo / 1e9, rotation_gflop=rot / 1e9, ms=ms, rotation_ms=ms_rot,
                         roof_fraction=algo / (ms * 1e-3) / PEAK_F32_MFMA))
        del efb, gemms, operands
    if do_single:
        for kind in ("diagonal", "efb"):
            est = Diagonal(model) if kind == "diagonal" else EFB(model, {}, eigvecs=eig)

            def single_passes():
                for n in range(N):
                    fwd_bwd(x[n:n + 1], labels[n:n + 1])
                    est.update(1)

            rows.append(dict(model=name, N=N, estimator=kind, layer_class="N single-sample passes (default path)",
                             ms=timed(single_passes, max(1, reps // 2))))
        rows.append(dict(model=name, N=N, estimator="-", layer_class="one forward/backward at N",
                         ms=timed(lambda: fwd_bwd(x, labels), reps)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", nargs="+", default=["resnet50", "resnet18"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-efb", action="store_true")
    ap.add_argument("--no-single", action="store_true")
    ap.add_argument("--json", default=None, help="append the rows as JSON lines to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.model:
        rows = run(name, args.batch, args.reps, not args.no_efb, not args.no_single, dev)
        print(f"\n{name}, N = {args.batch}")
        print(f"{'estimator':10s} {'class':40s} {'layers':>6s} {'algo GF':>9s} {'exec GF':>9s} {'ms':>9s} {'roof':>6s} "
              f"{'bmm ms':>9s} {'rot GF':>8s} {'rot ms':>8s}")
        for r in rows:
            def f(key, fmt):
                return format(r[key], fmt) if key in r else "-"
            print(f"{r['estimator']:10s} {r['layer_class']:40s} {f('layers', '6d'):>6s} {f('algorithmic_gflop', '9.1f'):>9s} "
                  f"{f('executed_gflop', '9.1f'):>9s} {r['ms']:9.3f} {f('roof_fraction', '6.3f'):>6s} {f('bmm_ms', '9.3f'):>9s} "
                  f"{f('rotation_gflop', '8.1f'):>8s} {f('rotation_ms', '8.3f'):>8s}")
        if args.json:
            with open(args.json, "a") as fh:
                for r in rows:
                    fh.write(json.dumps(r) + "\n")
        torch.cuda.empty_cache()
        ops.release_workspaces()


if __name__ == "__main__":
    main()
