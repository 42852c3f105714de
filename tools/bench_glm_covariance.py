#!/usr/bin/env python
"""Joint output covariance of the linearised Laplace (GLM) predictive: time of `glm_predictive_joint` beside two
yardsticks on the same device, in one run.

    python tools/bench_glm_covariance.py [--batch 32] [--outputs 10] [--reps 5] [--no-resnet] [--no-lenet] [--json FILE]

  * LeNet-5 at N = 100 and ResNet-50 at N x 3 x 224 x 224 (fp32), KFAC and Diagonal, the first `--outputs` classes;
    every timed call includes its forward pass and its K backward passes, the estimator's state is resident;
  * joint: `evaluate.glm_predictive_joint` - (N, K, K);
  * yardstick (a): `evaluate.glm_predictive` on the same outputs - the diagonal only, so the joint call does strictly more;
  * yardstick (b): torch - `F.unfold`, the rotations as matmuls, a batched matmul to (N, K, m, n_in), then an `einsum`
    over the entries, one layer at a time;
  * the FLOPs the plan of the joint reduction executes (curv_persample_cov_plan_flops) beside the algorithmic
    2 N K m n_in L.
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
from curvature_amd.evaluate import glm_predictive, glm_predictive_joint  # noqa: E402


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
    """KFAC and Diagonal of `model` after one update on (x, labels) and an inversion.  The update runs in train() mode:
    a randomly initialised ResNet-50 in eval() mode (BatchNorm at its initial statistics) grows its activations from
    block to block until the damping term is below the float32 resolution of the factors and `invert` refuses them."""
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


def unfolded_input(layer, x):
    """X of a layer's input as (N, n_in [+ 1], L)."""
    if layer.__class__.__name__ == "Conv2d":
        X = F.unfold(x, layer.kernel_size, padding=layer.padding, stride=layer.stride)
    else:
        X = x.reshape(x.shape[0], -1, x.shape[-1]).transpose(1, 2)
    if layer.bias is not None:
        X = torch.cat([X, torch.ones_like(X[:, :1])], dim=1)
    return X


def torch_covariance(kind, est, model, layers, x, classes, params):
    """Yardstick (b): the same arithmetic in torch, one layer at a time."""
    logits = model(x)
    gs = {l: [] for l in layers}
    for c in classes:
        torch.autograd.grad(logits[:, c].sum(), params, retain_graph=True)
        for l in layers:
            gs[l].append(grad_matrix(l, est.record[l][1]))
    total = 0
    for l in layers:
        X = unfolded_input(l, est.record[l][0])
        G = torch.stack(gs[l], dim=1)                                  # (N, K, m, L)
        if kind == "kfac":
            L_A, L_G = est.inv_state[l]
            X, G = L_A.t() @ X, L_G.t() @ G
        P = torch.matmul(G, X.transpose(1, 2).unsqueeze(1))            # (N, K, m, n_in)
        if kind == "kfac":
            total = total + torch.einsum("ncij,ndij->ncd", P, P)
        else:
            total = total + torch.einsum("ncij,ndij->ncd", P * est.inv_state[l].square(), P)
        del P, G, X
    return total


def plan_of(est, model, x, classes, params):
    """(executed, algorithmic) FLOPs of the joint reduction of all layers, from the sizes of one staged output."""
    logits = model(x)
    torch.autograd.grad(logits[:, classes[0]].sum(), params)
    est.stage_output(0, len(classes), inputs=True)
    kept = est._predictive_kept["covariance"]
    est.drop_predictive_state()
    jobs = [ops.PerSampleCovJob.of(s, None, None, None, None, len(classes), f) for s, f in zip(kept["sides"], kept["sizes"])]
    return sum(ops.per_sample_cov_plan_flops(jobs)), sum(2 * j.S * j.K * j.M * j.Nc * j.L for j in jobs)


def run(name, model, x, labels, K, reps):
    ests = estimators(model, x, labels)
    params = [p for p in model.parameters() if p.requires_grad]
    classes = list(range(K))
    rows = []
    for kind, est in ests.items():
        layers = est._layers()
        mine = glm_predictive_joint(model, est, x, outputs=classes)[1]
        want = torch_covariance(kind, est, model, layers, x, classes, params)
        row = dict(model=name, N=x.shape[0], estimator=kind, layers=len(layers), outputs=K,
                   rel_difference_to_torch=float(torch.linalg.norm(mine.double() - want.detach().double()) /
                                                 torch.linalg.norm(want.detach().double())))
        del mine, want
        row["joint_ms"] = timed(lambda: glm_predictive_joint(model, est, x, outputs=classes), reps)
        row["variance_ms"] = timed(lambda: glm_predictive(model, est, x, outputs=classes), reps)
        row["torch_ms"] = timed(lambda: torch_covariance(kind, est, model, layers, x, classes, params), reps)
        row["joint_over_variance"] = row["joint_ms"] / row["variance_ms"]
        row["joint_over_torch"] = row["joint_ms"] / row["torch_ms"]
        executed, algo = plan_of(est, model, x, classes, params)
        row.update(plan_gflop=executed / 1e9, algorithmic_gflop=algo / 1e9)
        rows.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
        ops.release_workspaces()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--outputs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-resnet", action="store_true")
    ap.add_argument("--no-lenet", action="store_true")
    ap.add_argument("--json", default=None, help="append the rows as JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_glm_covariance: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    rows = []
    torch.manual_seed(0)
    if not args.no_lenet:
        model = models.lenet5().to(dev).eval()
        rows += run("lenet5", model, torch.randn(100, 1, 28, 28, device=dev), torch.randint(0, 10, (100,), device=dev),
                    args.outputs, args.reps)
    if not args.no_resnet:
        model = models.resnet50().to(dev).eval()
        rows += run("resnet50", model, torch.randn(args.batch, 3, 224, 224, device=dev),
                    torch.randint(0, 1000, (args.batch,), device=dev), args.outputs, args.reps)
    if args.json:
        with open(args.json, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
