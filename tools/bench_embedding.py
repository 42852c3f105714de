"""The nn.Embedding kernels (csrc/embedding_factor.hip) against the torch expressions on the same tensors, in
the same run, on two shapes:
  - gpt2: V = 50257, D = 768, N = 8,  T = 1024, Zipf-distributed tokens (p ~ 1 / rank);
  - bert: V = 30522, D = 768, N = 32, T = 128,  uniform tokens with half of the positions padding (padding_idx = 0).
HIP-event times, the candidates run in turn inside every round (so drift and neighbours hit all alike), of
  - histogram / torch_bincount:  `ops.kfac_accumulate_embedding` against ``scale * torch.bincount(idx, minlength=V)``;
  - sq / torch_sq:     `ops.per_sample_embedding_sq_accumulate` against ``P = zeros(N, V, D); P[n].index_add_(0, idx[n],
                       g[n]); (P ** 2).sum(0)`` with the padding row zeroed;
  - quad / torch_quad: `ops.per_sample_embedding_quad_reduce` with a (V, D) weight against the same P and
                       ``(w * P ** 2).sum((1, 2))``.
The ops calls are timed whole: the position list they build with torch ops (a stable sort of the N T keys, which waits for
the device to learn its sizes) is part of what a caller pays.  With the medians and the spread over the rounds go the share
of one read of grad_output, N T D 4 bytes, at the HBM peak (`--peak-gbps`, 8000 for an MI355X) that a pass achieves, and the
error of each pass against its torch expression.

    python tools/bench_embedding.py [--rounds 5] [--reps 3] [--shapes gpt2 bert]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from curvature_amd import ops

SHAPES = {"gpt2": dict(V=50257, D=768, N=8, T=1024, pad=None), "bert": dict(V=30522, D=768, N=32, T=128, pad=0)}


def make(name, dev):
    s = SHAPES[name]
    gen = torch.Generator().manual_seed(0)
    V, D, N, T = s["V"], s["D"], s["N"], s["T"]
    if name == "gpt2":
        ranks = torch.arange(1, V + 1, dtype=torch.float64)
        idx = torch.multinomial(1.0 / ranks, N * T, replacement=True, generator=gen).view(N, T)
        idx = torch.randperm(V, generator=gen)[idx]                    # (frequent tokens anywhere in the table)
    else:
        idx = torch.randint(1, V, (N, T), generator=gen)
        idx[torch.rand(N, T, generator=gen) < 0.5] = 0
    g = torch.randn(N, T, D, generator=gen)
    w = torch.rand(V, D, generator=gen) + 0.5
    return idx.to(dev), g.to(dev), w.to(dev)


def products(idx, g, V, pad):
    P = torch.zeros(g.shape[0], V, g.shape[2], device=g.device)
    for n in range(g.shape[0]):
        P[n].index_add_(0, idx[n], g[n])
    if pad is not None:
        P[:, pad] = 0
    return P


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(values):
    return dict(median=round(statistics.median(values), 4), min=round(min(values), 4), max=round(max(values), 4))


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def bench(name, rounds, reps, peak_gbps):
    dev = torch.device("cuda:0")
    was = ops.admit_embedding(True)
    try:
        s = SHAPES[name]
        V, D, N, T, pad = s["V"], s["D"], s["N"], s["T"], s["pad"]
        idx, g, w = make(name, dev)
        a, dst, out = torch.empty(V, device=dev), torch.empty(V, D, device=dev), torch.empty(N, device=dev)
        scale = 1.0 / (N * T)

        def torch_bincount():
            count = torch.bincount(idx.reshape(-1), minlength=V).float()
            if pad is not None:
                count[pad] = 0
            return scale * count
        candidates = dict(
            histogram=lambda: ops.kfac_accumulate_embedding([ops.EmbeddingFactorJob(idx, a, V, pad, scale=scale, first=True)]),
            torch_bincount=torch_bincount,
            sq=lambda: ops.per_sample_embedding_sq_accumulate([ops.PerSampleEmbeddingJob(idx, g, V, pad, dst=dst, first=True)]),
            torch_sq=lambda: products(idx, g, V, pad).square().sum(0),
            quad=lambda: ops.per_sample_embedding_quad_reduce([ops.PerSampleEmbeddingJob(idx, g, V, pad, out=out, w=w,
                                                                                         first=True)]),
            torch_quad=lambda: (w * products(idx, g, V, pad).square()).sum((1, 2)))
        for fn in candidates.values():
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in candidates}
        for _ in range(rounds):
            for k, fn in candidates.items():
                times[k].append(timed(fn, reps))
        for k in ("histogram", "sq", "quad"):
            candidates[k]()
        errors = dict(histogram=rel(a, candidates["torch_bincount"]()), sq=rel(dst, candidates["torch_sq"]()),
                      quad=rel(out, candidates["torch_quad"]()))
        med = {k: statistics.median(v) for k, v in times.items()}
        read = 4.0 * N * T * D
        counts = torch.bincount(idx.reshape(-1), minlength=V)
        return dict(shape=name, V=V, D=D, N=N, T=T, padding_idx=pad, distinct_tokens=int((counts > 0).sum()),
                    most_frequent=int(counts.max()), ms={k: spread(v) for k, v in times.items()},
                    grad_output_MB=round(read / 1e6, 2),
                    hbm_fraction={k: round(read / med[k] / 1e6 / peak_gbps, 4) for k in ("sq", "quad")},
                    speedup_vs_torch=dict(histogram=round(med["torch_bincount"] / med["histogram"], 3),
                                          sq=round(med["torch_sq"] / med["sq"], 3),
                                          quad=round(med["torch_quad"] / med["quad"], 3)),
                    rel_err_vs_torch={k: float(f"{v:.2e}") for k, v in errors.items()})
    finally:
        ops.admit_embedding(was)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--peak-gbps", type=float, default=8000.0)
    ap.add_argument("--shapes", nargs="+", default=["gpt2", "bert"], choices=sorted(SHAPES))
    a = ap.parse_args()
    for name in a.shapes:
        print(json.dumps(bench(name, a.rounds, a.reps, a.peak_gbps)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
