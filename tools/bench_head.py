#!/usr/bin/env python
"""Last-layer Laplace predictive at the ResNet-50 head: time of `Curvature.head_terms`, `ops.head_mc` (curv_head_mc) and
the whole `evaluate.last_layer_predictive`, beside the torch expression for the same draws and the per-sample line they
replace, in one run.

    python tools/bench_head.py [--reps 9] [--json FILE]

  * shape: N = 32 inputs, K = 1000 classes, in = 2048 (+ 1 for the bias), S = 256 draws; the model is the head alone,
    ``Flatten -> Linear(2048, 1000)``, under a KFAC estimator after one update and an inversion;
  * head_terms: the skinny products that give d2 and the variance;
  * head_mc lower / dense: one `ops.head_mc` call with the library's own noise (Z = NULL), M = L_G with and without
    `lower`; its `plan_flops` over the time as a fraction of the 157.3 TF fp32 MFMA peak;
  * last_layer_predictive: forward pass, head_terms and head_mc ("mc") resp. the probit softmax;
  * torch: ``randn((N, S, K))``, scale, ``matmul`` with M^T, ``softmax``, ``mean`` - the (N, S, K) tensor is written
    and read several times;
  * glm_predictive with ``outputs=range(16)``: one backward pass per class - the cost per 16 classes of the per-sample
    line;
  * the relative Frobenius difference of kernel and torch expression on the SAME explicit noise (not timed).
HIP events around each call, the candidates alternating, median of `--reps` after two warm-up calls each.

    python tools/bench_head.py --grid [--reps 9] [--json FILE]

the grid of damping pairs instead, at the same head with H = 16 pairs:
  * head_grid dense / separable: one `ops.head_grid` call (curv_head_grid) on a (K, n) table resp. (K,) and (n,) spectra;
    the dense form's `plan_flops` times H over its time as a fraction of the fp32 MFMA peak;
  * composed: the same d2 from the ops that were there before - per pair `ops.rsqrt_affine` and `ops.mul` for the
    reciprocal table and one `ops.gemm_batched` against Y o Y - and its relative difference to head_grid (not timed);
  * last_layer_predictive_grid, probit and mc, under a Diagonal estimator that holds the head;
  * sixteen rounds of `invert` + `last_layer_predictive` (probit and mc): what the grid replaces.

    python tools/bench_head.py --moments [--reps 9] [--json FILE]

the entropy split at the same head, M = L_G with `lower` and dense, four candidates alternating:
  * head_mc: `ops.head_mc`, probs alone - the kernel of K23;
  * moments_all: `ops.head_mc_moments` with probs, entropy and probs_sq;
  * moments_probs: `ops.head_mc_moments` with probs alone;
  * torch: the expression that materialises the (N, S, K) softmax and forms the same three results;
  * the relative Frobenius difference of kernel and torch expression on the SAME explicit noise, and whether the probs of
    `head_mc_moments` have the bits of `head_mc` (not timed).
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from curvature_amd import ops  # noqa: E402
from curvature_amd.curvatures import KFAC, Diagonal  # noqa: E402
from curvature_amd.evaluate import glm_predictive, last_layer_predictive, last_layer_predictive_grid  # noqa: E402

N, K, IN, S = 32, 1000, 2048, 256
PEAK_TF = 157.3


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def torch_expression(M, d2, mu, z=None):
    if z is None:
        z = torch.randn(N, S, K, device=mu.device)
    f = mu[:, None, :] + torch.matmul(z * torch.sqrt(d2)[:, None, None], M.t())
    return torch.softmax(f, dim=2).mean(dim=1)


def measure(candidates, reps, row):
    for _ in range(2):
        for fn in candidates.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in candidates}
    for _ in range(reps):
        for name, fn in candidates.items():
            times[name].append(once(fn))
    for name, ts in times.items():
        row[name + "_ms"] = statistics.median(ts)
        row[name + "_ms_min"], row[name + "_ms_max"] = min(ts), max(ts)


def torch_moments(M, d2, mu, z=None):
    if z is None:
        z = torch.randn(N, S, K, device=mu.device)
    p = torch.softmax(mu[:, None, :] + torch.matmul(z * torch.sqrt(d2)[:, None, None], M.t()), dim=2)
    return p.mean(dim=1), -torch.xlogy(p, p).sum(dim=2).mean(dim=1), (p * p).mean(dim=1)


def moments_row(dev, reps):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(IN, K)).to(dev)
    x = torch.randn(N, IN, device=dev)
    labels = torch.randint(0, K, (N,), device=dev)
    est = KFAC(model, "Linear")
    torch.nn.functional.cross_entropy(model(x), labels).backward()
    est.update(N)
    model.zero_grad()
    est.invert(add=1.0, multiply=float(N))
    terms = est.head_terms(model[1], x)
    L_G = torch.tril(terms.M).contiguous()
    with torch.no_grad():
        mu = model(x).float().contiguous()
    probs, probs_sq = torch.empty(N, K, device=dev), torch.empty(N, K, device=dev)
    entropy = torch.empty(N, device=dev)
    plain = torch.empty(N, K, device=dev)
    state = {"offset": 0}

    def position():
        state["offset"] += N * S * ((K + 3) // 4)
        return state["offset"]

    def head_mc(lower, z=None):
        ops.head_mc([ops.HeadMCJob(L_G, terms.d2, mu, S, lower=lower, noise=z, probs=plain, seed=1, offset=position())])

    def moments(lower, everything, z=None):
        more = dict(entropy=entropy, probs_sq=probs_sq) if everything else {}
        ops.head_mc_moments([ops.HeadMomentsJob(L_G, terms.d2, mu, S, lower=lower, noise=z, probs=probs, seed=1,
                                                offset=position(), **more)])

    def rel(a, b):
        return float(torch.linalg.norm(a.double() - b.double()) / torch.linalg.norm(b.double()))

    row = dict(N=N, K=K, features=IN + 1, S=S)
    z = torch.randn(N, S, K, device=dev)
    want = torch_moments(L_G, terms.d2, mu, z)
    for lower in (True, False):
        tag = "lower" if lower else "dense"
        head_mc(lower, z)
        moments(lower, True, z)
        row[f"probs_bit_equal_to_head_mc_{tag}"] = bool(torch.equal(probs, plain))
        for name, got, ref in zip(("probs", "entropy", "probs_sq"), (probs, entropy, probs_sq), want):
            row[f"rel_difference_to_torch_{name}_{tag}"] = rel(got, ref)
    del z, want
    candidates = {}
    for lower in (True, False):
        tag = "lower" if lower else "dense"
        candidates[f"head_mc_{tag}"] = lambda lower=lower: head_mc(lower)
        candidates[f"moments_all_{tag}"] = lambda lower=lower: moments(lower, True)
        candidates[f"moments_probs_{tag}"] = lambda lower=lower: moments(lower, False)
    candidates["torch_moments"] = lambda: torch_moments(L_G, terms.d2, mu)
    measure(candidates, reps, row)
    for tag in ("lower", "dense"):
        row[f"moments_all_over_head_mc_{tag}"] = row[f"moments_all_{tag}_ms"] / row[f"head_mc_{tag}_ms"]
        row[f"moments_probs_over_head_mc_{tag}"] = row[f"moments_probs_{tag}_ms"] / row[f"head_mc_{tag}_ms"]
    return row


def grid_row(dev, reps):
    H, n = ops.HEAD_GRID_MAX, IN + 1
    pairs = [(10.0 ** (-2 + 0.25 * h), float(N * (1 + h))) for h in range(H)]
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(IN, K)).to(dev)
    x = torch.randn(N, IN, device=dev)
    labels = torch.randint(0, K, (N,), device=dev)
    est = Diagonal(model, "Linear")
    torch.nn.functional.cross_entropy(model(x), labels).backward()
    est.update(N)
    model.zero_grad()
    head = model[1]
    T = est.state[head]
    Y = torch.cat([x, torch.ones(N, 1, device=dev)], dim=1).contiguous()
    u, v = torch.rand(K, device=dev), torch.rand(n, device=dev)
    rho, gain = [a / m for a, m in pairs], [1.0 / m for _, m in pairs]
    d2 = torch.empty(H, N, K, device=dev)
    composed = torch.empty(H, N, K, device=dev)

    def compose():
        y2 = ops.mul(Y, Y)
        for h, (add, multiply) in enumerate(pairs):
            inv = ops.rsqrt_affine(T, add, multiply)
            ops.gemm_batched([ops.Gemm(y2, ops.mul(inv, inv).t(), composed[h])])

    def rounds(predictive):
        for add, multiply in pairs:
            est.invert(add, multiply)
            last_layer_predictive(model, est, x, predictive=predictive, samples=S)

    row = dict(N=N, K=K, features=n, S=S, H=H)
    ops.head_grid([ops.HeadGridJob(Y, None, None, T, d2, rho, gain)])
    compose()
    row["rel_difference_composed_to_head_grid"] = float(torch.linalg.norm(composed.double() - d2.double()) /
                                                        torch.linalg.norm(d2.double()))
    candidates = {
        "head_grid_dense": lambda: ops.head_grid([ops.HeadGridJob(Y, None, None, T, d2, rho, gain)]),
        "head_grid_separable": lambda: ops.head_grid([ops.HeadGridJob(Y, u, v, None, d2, [math.sqrt(r) for r in rho], gain)]),
        "composed": compose,
        "last_layer_grid_probit": lambda: last_layer_predictive_grid(model, est, x, pairs),
        "last_layer_grid_mc": lambda: last_layer_predictive_grid(model, est, x, pairs, predictive="mc", samples=S),
        "sixteen_rounds_probit": lambda: rounds("probit"),
        "sixteen_rounds_mc": lambda: rounds("mc"),
    }
    measure(candidates, reps, row)
    flops = H * ops.head_grid_plan_flops([ops.HeadGridJob(None, None, None, None, None, rho, gain, N=N, K=K, n=n,
                                                          separable=False)])[0]
    row["plan_gflop_dense"] = flops / 1e9
    row["mfma_peak_fraction_dense"] = flops / (row["head_grid_dense_ms"] * 1e-3) / (PEAK_TF * 1e12)
    row["composed_over_head_grid_dense"] = row["composed_ms"] / row["head_grid_dense_ms"]
    row["sixteen_rounds_over_grid_probit"] = row["sixteen_rounds_probit_ms"] / row["last_layer_grid_probit_ms"]
    row["sixteen_rounds_over_grid_mc"] = row["sixteen_rounds_mc_ms"] / row["last_layer_grid_mc_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None, help="write the result as one JSON line to this file")
    ap.add_argument("--grid", action="store_true", help="measure the grid of damping pairs (K24) instead")
    ap.add_argument("--moments", action="store_true", help="measure the entropy split (K25) instead")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_head: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    if args.grid or args.moments:
        row = grid_row(dev, args.reps) if args.grid else moments_row(dev, args.reps)
        row["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(row), flush=True)
        if args.json:
            with open(args.json, "w") as fh:
                fh.write(json.dumps(row) + "\n")
        return
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(IN, K)).to(dev)
    x = torch.randn(N, IN, device=dev)
    labels = torch.randint(0, K, (N,), device=dev)
    est = KFAC(model, "Linear")
    torch.nn.functional.cross_entropy(model(x), labels).backward()
    est.update(N)
    model.zero_grad()
    est.invert(add=1.0, multiply=float(N))
    head = model[1]
    terms = est.head_terms(head, x)
    L_G = torch.tril(terms.M).contiguous()
    with torch.no_grad():
        mu = model(x).float().contiguous()
    probs = torch.empty(N, K, device=dev)
    state = {"offset": 0}

    def head_mc(lower, z=None):
        ops.head_mc([ops.HeadMCJob(L_G, terms.d2, mu, S, lower=lower, noise=z, probs=probs, seed=1,
                                   offset=state["offset"])])
        state["offset"] += N * S * ((K + 3) // 4)
        return probs

    z = torch.randn(N, S, K, device=dev)
    want = torch_expression(L_G, terms.d2, mu, z).double()
    row = dict(N=N, K=K, features=IN + 1, S=S)
    for lower in (True, False):
        mine = head_mc(lower, z).double()
        row["rel_difference_to_torch_" + ("lower" if lower else "dense")] = \
            float(torch.linalg.norm(mine - want) / torch.linalg.norm(want))
    del z, want

    candidates = {
        "head_terms": lambda: est.head_terms(head, x),
        "head_mc_lower": lambda: head_mc(True),
        "head_mc_dense": lambda: head_mc(False),
        "last_layer_mc": lambda: last_layer_predictive(model, est, x, predictive="mc", samples=S),
        "last_layer_probit": lambda: last_layer_predictive(model, est, x),
        "torch_expression": lambda: torch_expression(L_G, terms.d2, mu),
        "glm_predictive_16_classes": lambda: glm_predictive(model, est, x, outputs=range(16)),
    }
    measure(candidates, args.reps, row)
    for lower in (True, False):
        tag = "lower" if lower else "dense"
        flops = ops.head_mc_plan_flops([ops.HeadMCJob(True, None, None, S, lower=lower, N=N, K=K)])[0]
        row[f"plan_gflop_{tag}"] = flops / 1e9
        row[f"mfma_peak_fraction_{tag}"] = flops / (row[f"head_mc_{tag}_ms"] * 1e-3) / (PEAK_TF * 1e12)
    row["torch_over_head_mc_lower"] = row["torch_expression_ms"] / row["head_mc_lower_ms"]
    row["glm_1000_classes_over_last_layer_probit"] = \
        row["glm_predictive_16_classes_ms"] * (K / 16) / row["last_layer_probit_ms"]
    row["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
