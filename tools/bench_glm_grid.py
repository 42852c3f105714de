#!/usr/bin/env python
"""GLM predictive over a grid of damping pairs: what one pass for 16 pairs costs beside the calls it replaces, on the
same device, in one run.

    python tools/bench_glm_grid.py [--batch 32] [--reps 5] [--no-resnet] [--no-lenet] [--json FILE]

  (a) kernel level: one `ops.per_sample_quad_grid_reduce` call with H = 16 over all layers of the model against one
      `ops.per_sample_quad_reduce` call on the same operands (one damping pair), with the plan's GFLOP - KFAC (separable
      weights on rotated operands) and Diagonal (dense weights on the operands as recorded);
  (b) end to end, one validation batch: `evaluate.glm_predictive_grid` with 16 pairs against the loop it replaces,
      ``for pair: estimator.invert(*pair); glm_predictive(...)`` - forward and backward passes included on both sides;
  (c) `KFAC.decompose()` on its own (once per estimator, not once per batch).
LeNet-5 at N = 100 with all 10 outputs, ResNet-50 at N x 3 x 224 x 224 (fp32) with the top-5 classes of the first input.
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
from curvature_amd.curvatures import KFAC, Diagonal  # noqa: E402
from curvature_amd.evaluate import glm_predictive, glm_predictive_grid  # noqa: E402

# 16 pairs; sqrt(add / multiply) >= 0.03, the damping tools/bench_glm_covariance.py inverts ResNet-50's factors with
HYPERS = [(a, s) for a in (1.0, 3.0, 10.0, 30.0) for s in (10.0, 100.0, 300.0, 1000.0)]


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
    """KFAC and Diagonal of `model` after one update on (x, labels), in train() mode (see bench_glm_covariance.py)."""
    kfac, diag = KFAC(model), Diagonal(model, per_sample=True)
    model.train()
    model.zero_grad()
    F.cross_entropy(model(x), labels).backward()
    kfac.update(x.shape[0])
    diag.update(x.shape[0])
    model.eval()
    return {"kfac": kfac, "diagonal": diag}


def kernel_jobs(kind, est, model, x, c, params):
    """The whole model's jobs of both reductions on the operands of output `c`: (grid jobs, quad jobs, what keeps their
    tensors alive)."""
    logits = model(x)
    torch.autograd.grad(logits[:, c].sum(), params)
    terms = est._predictive_terms()
    basis = terms.grid_basis
    layers, operands, _ = est._predictive_operands(kind, "bench", True, basis is not None, select="state")
    xs, _ = est._x_side("grid", layers, operands, basis, None)
    gs = est._g_side(layers, operands, basis)
    N, dev = operands[0][0].N, gs[0].device
    shifts, gains = [0.03 * 1.5 ** h for h in range(16)], [1.0 / (1 + h) for h in range(16)]
    grid_rows = torch.empty(len(layers), 16, N, device=dev)
    quad_rows = torch.empty(len(layers), N, device=dev)
    grid, quad, keep = [], [], [gs, xs, grid_rows, quad_rows]
    for k, (l, (s, _, _), g, xk) in enumerate(zip(layers, operands, gs, xs)):
        weights = terms.spectrum(l)
        W = None if terms.separable else 1.0 / (est.state[l] + shifts[0])
        keep.append(W)
        grid.append(ops.PerSampleGridJob.of(s, g, xk, *weights, grid_rows[k], shifts, gains, first=True))
        quad.append(ops.PerSampleQuadJob.of(s, g, xk, W, quad_rows[k], first=True))
    return grid, quad, keep


def run(name, model, x, labels, outputs, reps):
    ests = estimators(model, x, labels)
    params = [p for p in model.parameters() if p.requires_grad]
    rows = []
    row = dict(model=name, what="decompose", estimator="kfac", layers=len(ests["kfac"]._layers()),
               decompose_ms=timed(ests["kfac"].decompose, reps))
    rows.append(row)
    print(json.dumps(row), flush=True)
    for kind, est in ests.items():
        # (a) the two reductions alone
        grid, quad, keep = kernel_jobs(kind, est, model, x, outputs[0], params)
        row = dict(model=name, what="kernel", N=x.shape[0], estimator=kind, layers=len(grid), H=16,
                   plan_gflop=sum(ops.per_sample_quad_grid_plan_flops(grid)) / 1e9)
        row["grid16_ms"] = timed(lambda: ops.per_sample_quad_grid_reduce(grid), reps)
        row["quad1_ms"] = timed(lambda: ops.per_sample_quad_reduce(quad), reps)
        row["grid16_over_quad1"] = row["grid16_ms"] / row["quad1_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del grid, quad, keep
        est.drop_predictive_state()

        # (b) a validation batch, 16 pairs
        def loop():
            for pair in HYPERS:
                est.invert(*pair)
                glm_predictive(model, est, x, outputs=outputs)
        row = dict(model=name, what="end_to_end", N=x.shape[0], estimator=kind, outputs=len(outputs), pairs=len(HYPERS))
        row["grid_ms"] = timed(lambda: glm_predictive_grid(model, est, x, HYPERS, outputs=outputs), reps)
        row["loop_ms"] = timed(loop, reps)
        row["loop_over_grid"] = row["loop_ms"] / row["grid_ms"]
        est.invert(*HYPERS[-1])
        mine = glm_predictive_grid(model, est, x, HYPERS, outputs=outputs)[1][-1]
        want = glm_predictive(model, est, x, outputs=outputs)[1]
        row["rel_difference_last_pair"] = float(torch.linalg.norm(mine.double() - want.double()) /
                                                torch.linalg.norm(want.double()))
        rows.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
        ops.release_workspaces()
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
        raise SystemExit("bench_glm_grid: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    rows = []
    torch.manual_seed(0)
    if not args.no_lenet:
        model = models.lenet5().to(dev).eval()
        rows += run("lenet5", model, torch.randn(100, 1, 28, 28, device=dev), torch.randint(0, 10, (100,), device=dev),
                    list(range(10)), args.reps)
    if not args.no_resnet:
        model = models.resnet50().to(dev).eval()
        x = torch.randn(args.batch, 3, 224, 224, device=dev)
        with torch.no_grad():
            top5 = model(x[:1])[0].topk(5).indices.tolist()
        rows += run("resnet50", model, x, torch.randint(0, 1000, (args.batch,), device=dev), top5, args.reps)
    if args.json:
        with open(args.json, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
