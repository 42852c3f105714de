#!/usr/bin/env python
"""Monte-Carlo softmax from the joint logit covariance: time of `ops.logit_mc` (curv_logit_mc) beside the torch
composition of the same predictive on the same device, in one run.

    python tools/bench_logit_mc.py [--reps 9] [--json FILE]

  * shapes (N, S, K): 1024 x 1024 x 10 and 10 000 x 1000 x 16, definite blocks B B^T + I, every class selected;
  * kernel: one `ops.logit_mc` call with the library's own noise (Z = NULL) - reads (N, K, K) and (N, K), writes (N, K);
  * torch: `torch.linalg.cholesky`, `torch.randn((N, S, K))`, `einsum`, `softmax`, `mean` - the (N, S, K) tensor is
    written and read several times;
  * the relative Frobenius difference of the two results on the SAME explicit noise (one call each, not timed).
HIP events around each call, the two versions alternating, median of `--reps` after two warm-up calls each.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from curvature_amd import ops  # noqa: E402

SHAPES = [(1024, 1024, 10), (10000, 1000, 16)]


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def torch_composition(cov, mu, S, z=None):
    L = torch.linalg.cholesky(cov)
    if z is None:
        z = torch.randn(cov.shape[0], S, cov.shape[1], device=cov.device)
    f = mu[:, None, :] + torch.einsum("nsk,nck->nsc", z, L)
    return torch.softmax(f, dim=2).mean(dim=1)


def run(N, S, K, reps, dev):
    gen = torch.Generator(device=dev).manual_seed(N + K)
    B = torch.randn(N, K, K, device=dev, generator=gen)
    cov = B @ B.transpose(1, 2) + torch.eye(K, device=dev)
    mu = torch.randn(N, K, device=dev, generator=gen) * 2
    probs = torch.empty(N, K, device=dev)
    info = torch.empty(N, dtype=torch.int32, device=dev)
    state = {"offset": 0}

    def kernel(z=None):
        ops.logit_mc([ops.LogitMCJob(cov, mu, S, noise=z, probs=probs, info=info, seed=1, offset=state["offset"])])
        state["offset"] += N * S * ((K + 3) // 4)
        return probs

    z = torch.randn(N, S, K, device=dev, generator=gen)
    mine, want = kernel(z).double(), torch_composition(cov, mu, S, z).double()
    row = dict(N=N, S=S, K=K, rel_difference_to_torch=float(torch.linalg.norm(mine - want) / torch.linalg.norm(want)),
               dropped_columns=int(info.sum()))
    del z, mine, want
    for _ in range(2):
        kernel()
        torch_composition(cov, mu, S)
    torch.cuda.synchronize()
    ours, theirs = [], []
    for _ in range(reps):
        ours.append(once(kernel))
        theirs.append(once(lambda: torch_composition(cov, mu, S)))
    row.update(kernel_ms=statistics.median(ours), kernel_ms_min=min(ours), kernel_ms_max=max(ours),
               torch_ms=statistics.median(theirs), torch_ms_min=min(theirs), torch_ms_max=max(theirs))
    row["torch_over_kernel"] = row["torch_ms"] / row["kernel_ms"]
    row["plan_gflop"] = ops.logit_mc_plan_flops([ops.LogitMCJob(None, None, S, N=N, K=K)])[0] / 1e9
    row["draws_per_second"] = N * S / (row["kernel_ms"] * 1e-3)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None, help="append the rows as JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_logit_mc: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    rows = [run(N, S, K, args.reps, dev) for N, S, K in SHAPES]
    if args.json:
        with open(args.json, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
