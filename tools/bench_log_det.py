#!/usr/bin/env python
"""`log_det_grid` for 16 damping pairs on the ResNet-50 states beside the torch expression it replaces, on the same device,
in one run.

    python tools/bench_log_det.py [--batch 32] [--reps 5] [--json FILE]

Diagonal and EFB (one state tensor per layer, 25.5 M elements together) and KFAC after `decompose()` (two spectra per
layer) of ResNet-50 after one update at N x 3 x 224 x 224.  Beside each `log_det_grid(hypers)` call:

    torch.log(s * state.double().clamp_min(0) + n).sum()            looped over layers and pairs

(KFAC: the two weighted sums of the same form over lambda_A and lambda_G), the totals added up on the device.  The two take
turns inside every round; HIP events, median and min .. max of `--reps` rounds after two warm-up rounds; the largest
relative difference of the two results over the pairs.  `ops.logsum_grid` alone on the whole Diagonal state at 1 and at 16
pairs shows what a pair costs (the kernel is bound by the float64 logarithm, not by the read: DESIGN.md K21).
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
from curvature_amd.curvatures import EFB, KFAC, Diagonal  # noqa: E402

# 16 pairs: prior precisions 1e-2 .. 10 against data-set sizes 1e3 .. 1e6
HYPERS = [(a, s) for a in (1e-2, 0.1, 1.0, 10.0) for s in (1e3, 1e4, 1e5, 1e6)]


def alternate(fns, reps):
    """{name: (median, min, max)} in milliseconds between HIP events, the candidates taking turns inside every round."""
    times = {k: [] for k in fns}
    for r in range(reps + 2):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= 2:
                times[k].append(e0.elapsed_time(e1))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def torch_spectrum(states):
    def run():
        out = []
        for n, s in HYPERS:
            total = torch.zeros((), dtype=torch.float64, device=states[0].device)
            for state in states:
                total += torch.log(s * state.double().clamp_min(0) + n).sum()
            out.append(total)
        return torch.stack(out)
    return run


def torch_kfac(kfac):
    kept = list(kfac._decomposition.values())

    def run():
        out = []
        for n, s in HYPERS:
            total = torch.zeros((), dtype=torch.float64, device=kept[0][2].device)
            for _, _, lam_G, lam_A in kept:
                total += lam_G.numel() * torch.log(math.sqrt(s) * lam_A.double().clamp_min(0) + math.sqrt(n)).sum()
                total += lam_A.numel() * torch.log(math.sqrt(s) * lam_G.double().clamp_min(0) + math.sqrt(n)).sum()
            out.append(total)
        return torch.stack(out)
    return run


def row_of(name, est, torch_fn, elements, reps):
    mine = est.log_det_grid(HYPERS)
    want = torch_fn()
    t = alternate({"log_det_grid": lambda: est.log_det_grid(HYPERS), "torch": torch_fn}, reps)
    row = dict(model="resnet50", estimator=name, pairs=len(HYPERS), layers=len(est.state), elements=elements,
               rel_difference=float(((mine - want).abs() / want.abs()).max()))
    for k, (med, lo, hi) in t.items():
        row[k + "_ms"], row[k + "_min_ms"], row[k + "_max_ms"] = med, lo, hi
    row["torch_over_log_det_grid"] = row["torch_ms"] / row["log_det_grid_ms"]
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None, help="append the rows as JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_log_det: needs the GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = models.resnet50().to(dev)
    x = torch.randn(args.batch, 3, 224, 224, device=dev)
    labels = torch.randint(0, 1000, (args.batch,), device=dev)
    diag, kfac = Diagonal(model), KFAC(model)
    model.train()
    model.zero_grad()
    F.cross_entropy(model(x), labels).backward()
    diag.update(args.batch)
    kfac.update(args.batch)
    efb = EFB(model, kfac.state)
    efb.update(args.batch)
    kfac.decompose()
    model.eval()
    rows = []
    for name, est in (("diagonal", diag), ("efb", efb)):
        states = list(est.state.values())
        rows.append(row_of(name, est, torch_spectrum(states), sum(t.numel() for t in states), args.reps))
    rows.append(row_of("kfac", kfac, torch_kfac(kfac),
                       sum(k[2].numel() + k[3].numel() for k in kfac._decomposition.values()), args.reps))
    # what a pair costs: the whole Diagonal state at 1 and at 16 pairs through the primitive alone
    states = list(diag.state.values())
    jobs = {H: [ops.LogSumSegment.of(t, 1.0, [s for _, s in HYPERS[:H]], [n for n, _ in HYPERS[:H]]) for t in states]
            for H in (1, 16)}
    t = alternate({f"logsum_grid_{H}": (lambda H=H: ops.logsum_grid(jobs[H], H)) for H in jobs}, args.reps)
    elements = sum(t_.numel() for t_ in states)
    row = dict(model="resnet50", what="primitive", elements=elements)
    for k, (med, lo, hi) in t.items():
        row[k + "_ms"] = med
    row["read_gb_per_s_at_1"] = 4e-6 * elements / row["logsum_grid_1_ms"]
    row["giga_log_per_s_at_16"] = 16e-6 * elements / row["logsum_grid_16_ms"]
    rows.append(row)
    print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
