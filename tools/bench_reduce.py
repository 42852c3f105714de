"""KFAC-reduce factor build (curv_kfac_reduce_accumulate) at N = 32 on the two 28x28 layers of K16's table,
undilated, and the ResNet-50 stem: HIP-event times of
  - the reduce A + G build (two reduce passes, two flat builds of (N, dim) rows),
  - the expand A + G build of the same layer through `ops.kfac_accumulate` (what `KFAC(model)` runs),
  - a device-to-device copy of the A-side source (the bandwidth the reduce pass is held against),
with the executed flops of both plans and the relative error of the reduce factors against float64
(``F.unfold(...).mean(2)`` and plain sums in float64 on the device).

    python tools/bench_reduce.py [--reps 20] [--batch 32]

The reduce pass alone: a run of its own under the profiler, then the summary of its kernel trace,

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_reduce.py --profile --reps 3
    python tools/bench_reduce.py --read-trace DIR/.../*_kernel_trace.csv --reps 3

which lists, per layer and side, the time of `reduce_rows_kernel` as (source bytes + row bytes) / time beside the device
copy of the same source in the same run (2 x source bytes / time).
"""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from curvature_amd import ops

# (name, C, H, W, kernel, stride, padding, Cout)
LAYERS = [("C=256 28x28 3x3 p1", 256, 28, 28, 3, 1, 1, 256), ("C=512 28x28 3x3 p1", 512, 28, 28, 3, 1, 1, 512),
          ("stem 3x224x224 7x7 s2 p3", 3, 224, 224, 7, 2, 3, 64)]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def tensors(layer, batch, dev):
    _, C, H, W, k, s, p, Cout = layer
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    torch.manual_seed(0)
    return torch.randn(batch, C, H, W, device=dev), torch.randn(batch, Cout, Ho, Wo, device=dev) / (batch * Ho * Wo)


def reduce_jobs(layer, x, g, A, G):
    _, C, H, W, k, s, p, Cout = layer
    N = x.shape[0]
    return [ops.ReduceFactorJob(x, A, (k, k), (s, s), (p, p), True, 1.0 / N, True, mean=True),
            ops.ReduceFactorJob(g, G, scale=float(N), first=True, mean=False)]


def bench(layer, batch, reps):
    dev = torch.device("cuda:0")
    name, C, H, W, k, s, p, Cout = layer
    x, g = tensors(layer, batch, dev)
    L = g.shape[2] * g.shape[3]
    n = C * k * k + 1
    A, G = torch.empty(n, n, device=dev), torch.empty(Cout, Cout, device=dev)
    jobs = reduce_jobs(layer, x, g, A, G)
    t_reduce = timed(lambda: ops.kfac_accumulate_reduce(jobs), reps)
    t_reduce_a = timed(lambda: ops.kfac_accumulate_reduce(jobs[:1]), reps)

    Ae, Ge = torch.empty_like(A), torch.empty_like(G)
    expand = [ops.FactorJob(x, Ae, (k, k), (s, s), (p, p), True, 1.0 / (batch * L), True),
              ops.FactorJob(g, Ge, scale=float(batch) / L, first=True)]
    t_expand = timed(lambda: ops.kfac_accumulate(expand), reps)
    t_expand_a = timed(lambda: ops.kfac_accumulate(expand[:1]), reps)

    y = torch.empty_like(x)
    t_copy = timed(lambda: y.copy_(x), reps)
    del y

    # float64 on the device, sample by sample (the im2col matrix of one sample at a time)
    rows = torch.stack([F.unfold(x[i:i + 1].double(), (k, k), padding=(p, p), stride=(s, s)).mean(2)[0] for i in range(batch)])
    rows = torch.cat([rows, rows.new_ones(batch, 1)], dim=1)
    gh = g.double().sum((2, 3))
    err_a = float((A.double() - rows.t() @ rows / batch).norm() / (rows.t() @ rows / batch).norm())
    err_g = float((G.double() - gh.t() @ gh * batch).norm() / (gh.t() @ gh * batch).norm())
    shapes = [ops.ReduceFactorJob(tuple(j.src.shape), None, j.kernel, j.stride, j.padding, j.has_bias, mean=j.mean) for j in jobs]
    return dict(layer=name, N=batch, dim=n, m=Cout, L=L,
                reduce_build_ms=round(t_reduce, 4), expand_build_ms=round(t_expand, 4), speedup=round(t_expand / t_reduce, 2),
                reduce_A_ms=round(t_reduce_a, 4), expand_A_ms=round(t_expand_a, 4),
                copy_ms=round(t_copy, 4), copy_GBps=round(2 * x.numel() * 4 / t_copy / 1e6, 1),
                reduce_plan_Gflop=round(sum(ops.kfac_reduce_plan_flops(shapes)) / 1e9, 4),
                expand_plan_Gflop=round(sum(ops.kfac_plan_flops([ops.FactorJob(tuple(j.src.shape), None, j.kernel, j.stride,
                                                                              j.padding, j.has_bias) for j in expand])) / 1e9, 2),
                rel_err_A=float(f"{err_a:.2e}"), rel_err_G=float(f"{err_g:.2e}"))


def profile(batch, reps):
    """What the kernel trace is taken of: per layer `reps` x (A build, G build, copy of x, copy of g), after a warm-up."""
    dev = torch.device("cuda:0")
    for layer in LAYERS:
        _, C, H, W, k, s, p, Cout = layer
        x, g = tensors(layer, batch, dev)
        n = C * k * k + 1
        jobs = reduce_jobs(layer, x, g, torch.empty(n, n, device=dev), torch.empty(Cout, Cout, device=dev))
        yx, yg = torch.empty_like(x), torch.empty_like(g)
        for _ in range(reps + 1):                               # the first round is the warm-up: `read_trace` drops it
            ops.kfac_accumulate_reduce(jobs[:1])
            ops.kfac_accumulate_reduce(jobs[1:])
            yx.copy_(x)
            yg.copy_(g)
        torch.cuda.synchronize()


def read_trace(path, batch, reps):
    """Per layer and side: the times of `reduce_rows_kernel` and of the copy kernel in the trace `profile` produced."""
    with open(path, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    took = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3               # us
    passes = [took(r) for r in rows if "reduce_rows_kernel" in r["Kernel_Name"]]
    copies = [took(r) for r in rows if "copyBuffer" in r["Kernel_Name"]]
    per = 2 * (reps + 1)
    if len(passes) != per * len(LAYERS):
        raise SystemExit(f"expected {per * len(LAYERS)} reduce passes, found {len(passes)} (same --reps as the --profile run?)")
    if len(copies) != per * len(LAYERS):                        # the runtime split or offloaded a copy: list what there is
        print(json.dumps(dict(copy_kernels_us=[round(t, 1) for t in copies])), flush=True)
        copies = [float("nan")] * (per * len(LAYERS))
    for i, layer in enumerate(LAYERS):
        name, C, H, W, k, s, p, Cout = layer
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        for side, (src, out) in enumerate(((batch * C * H * W * 4, batch * C * k * k * 4),
                                           (batch * Cout * Ho * Wo * 4, batch * Cout * 4))):
            mine = passes[i * per + 2 + side:(i + 1) * per:2]
            copy = copies[i * per + 2 + side:(i + 1) * per:2]
            print(json.dumps(dict(layer=name, side="AG"[side], source_MB=round(src / 1e6, 2),
                                  pass_us=[round(t, 1) for t in mine],
                                  pass_GBps=[round((src + out) / t / 1e3, 1) for t in mine],
                                  copy_us=[round(t, 1) for t in copy],
                                  copy_GBps=[round(2 * src / t / 1e3, 1) for t in copy])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--profile", action="store_true", help="only run the builds and copies (for a kernel trace)")
    ap.add_argument("--read-trace", metavar="CSV", help="summarise the kernel trace of a --profile run (same --reps)")
    a = ap.parse_args()
    if a.read_trace:
        read_trace(a.read_trace, a.batch, a.reps)
    elif a.profile:
        profile(a.batch, a.reps)
    else:
        for layer in LAYERS:
            print(json.dumps(bench(layer, a.batch, a.reps)), flush=True)


if __name__ == "__main__":
    main()
