#!/usr/bin/env python
"""The per-sample line of Conv3d layers (`ops.admit_conv3d_per_sample`): the 3-D pack and what rides on it.

    python tools/bench_pack3d.py [--part pack model resnet] [--rounds 5] [--json FILE]

HIP events, two warm-up calls, the candidates of a part taking turns inside every round; median and min..max over the
rounds.  Run under ``rocprofv3 --kernel-trace --stats`` (a run of its own) for the time of `ps_pack_kernel` alone.

  pack    curv_persample_pack3d on the layers of K18's table - (2, 32, 32, 64, 64) and (2, 64, 16, 32, 32) with 3x3x3 p1,
          (8, 64, 8, 56, 56) with (1, 3, 3) p(0, 1, 1) and with (3, 1, 1) p(1, 0, 0), all biased - through
          `ops.per_sample_pack`; the bytes it has to move (the record read once plus the packed operand written once) over
          its time; a `copy_` of the same byte volume; and the torch route to the same matrix (`F.pad`, three `unfold`s,
          `permute`, `contiguous`).  The two results are compared bit for bit.
  model   C3D-small (defined here: three Conv3d + ReLU + MaxPool3d stages of 32 / 64 / 128 channels, the last with a
          (1, 3, 3) kernel, global average pool, Linear(128, 10)) on a (8, 3, 8, 32, 32) batch:
          `Diagonal(per_sample=True).update` and KFAC `glm_predictive` (10 outputs) beside torch doing the same arithmetic
          (the unfold above, `bmm`, square, sum; for the predictive with the two triangular factors applied first), with
          the plan's executed GFLOP of the per-sample products.
  resnet  the 2-D pack, which must not get slower: ResNet-50, N = 32, 224 x 224, fp32, `Diagonal(per_sample=True).update`.
          A/B of two library builds: ``python tools/with_lib.py <other lib> tools/bench_pack3d.py --part resnet``.
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
from curvature_amd.evaluate import glm_predictive  # noqa: E402


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternated(candidates, rounds):
    """{name: (median, min, max)} in ms of every ``candidates[name]()``: two warm-up calls each, then `rounds` rounds in
    which the candidates take turns."""
    for fn in candidates.values():
        fn()
        fn()
    times = {name: [] for name in candidates}
    for _ in range(rounds):
        for name, fn in candidates.items():
            times[name].append(once(fn))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def spread(row, name, stats):
    row[name + "_ms"], row[name + "_min"], row[name + "_max"] = stats


def unfold3d(x, kernel, stride, padding):
    """(N, C kd kh kw, L), rows in the order of ``weight.reshape(Cout, -1)``: torch's route to the packed operand."""
    N, C = x.shape[:2]
    padded = F.pad(x, (padding[2], padding[2], padding[1], padding[1], padding[0], padding[0]))
    u = padded.unfold(2, kernel[0], stride[0]).unfold(3, kernel[1], stride[1]).unfold(4, kernel[2], stride[2])
    return u.permute(0, 1, 5, 6, 7, 2, 3, 4).contiguous().view(N, C * kernel[0] * kernel[1] * kernel[2], -1)


LAYERS = [((2, 32, 32, 64, 64), (3, 3, 3), (1, 1, 1)), ((2, 64, 16, 32, 32), (3, 3, 3), (1, 1, 1)),
          ((8, 64, 8, 56, 56), (1, 3, 3), (0, 1, 1)), ((8, 64, 8, 56, 56), (3, 1, 1), (1, 0, 0))]


def pack_part(rounds, dev):
    rows = []
    for shape, kernel, padding in LAYERS:
        torch.manual_seed(0)
        conv = torch.nn.Conv3d(shape[1], 8, kernel, padding=padding).to(dev)
        x = torch.randn(shape, device=dev)
        g = torch.zeros(shape[0], 8, *shape[2:], device=dev)
        op = ops.per_sample_operands(conv, x, g, in_place=False).x
        dst = torch.empty(op.floats, device=dev)
        moved = 4 * (x.numel() + op.floats)
        a, b = torch.empty(moved // 8, device=dev), torch.empty(moved // 8, device=dev)
        stats = alternated({"pack": lambda: ops.per_sample_pack([op], [dst]), "copy": lambda: b.copy_(a),
                            "torch": lambda: unfold3d(x, kernel, (1, 1, 1), padding)}, rounds)
        want = unfold3d(x, kernel, (1, 1, 1), padding)
        same = op.Lp == op.L and torch.equal(dst.view(shape[0], op.rows, op.Lp)[:, :op.rows - 1], want)
        row = dict(part="pack", input=list(shape), kernel=list(kernel), padding=list(padding), rows=op.rows, L=op.L,
                   moved_MB=moved / 1e6, same_bits=bool(same))
        for name in ("pack", "copy", "torch"):
            spread(row, name, stats[name])
        row["pack_TBps"], row["copy_TBps"] = moved / stats["pack"][0] / 1e9, moved / stats["copy"][0] / 1e9
        row["torch_over_pack"] = stats["torch"][0] / stats["pack"][0]
        rows.append(row)
        del x, g, dst, a, b, want
        torch.cuda.empty_cache()
    return rows


def c3d_small():
    conv = torch.nn.Conv3d
    return torch.nn.Sequential(conv(3, 32, 3, padding=1), torch.nn.ReLU(), torch.nn.MaxPool3d((1, 2, 2)),
                               conv(32, 64, 3, padding=1), torch.nn.ReLU(), torch.nn.MaxPool3d(2),
                               conv(64, 128, (1, 3, 3), padding=(0, 1, 1)), torch.nn.ReLU(), torch.nn.AdaptiveAvgPool3d(1),
                               torch.nn.Flatten(), torch.nn.Linear(128, 10))


def columns(layer, x):
    """X of `layer` with its ones row, (N, n, L), by torch."""
    if layer.__class__.__name__ == "Conv3d":
        X = unfold3d(x, layer.kernel_size, layer.stride, layer.padding)
    else:
        X = x.reshape(x.shape[0], -1, 1)
    return torch.cat([X, torch.ones_like(X[:, :1])], dim=1)


def model_part(rounds, dev):
    N, kinds = 8, ["Conv3d", "Linear"]
    torch.manual_seed(0)
    model = c3d_small().to(dev).eval()
    x = torch.randn(N, 3, 8, 32, 32, device=dev)
    labels = torch.randint(0, 10, (N,), device=dev)
    diag, kfac = Diagonal(model, kinds, per_sample=True), KFAC(model, kinds)
    model.zero_grad()
    F.cross_entropy(model(x), labels).backward()
    kfac.update(N)
    kfac.invert(0.5, 2.0)
    layers = diag._layers()
    record = {l: [t.detach() for t in diag.record[l]] for l in layers}

    def torch_update():
        out = []
        for layer in layers:
            xin, g = record[layer]
            P = torch.bmm(g.reshape(N, g.shape[1], -1), columns(layer, xin).transpose(1, 2))
            out.append(P.square_().sum(0).mul_(N))
        return out

    def torch_predictive():
        logits = model(x)
        variance = torch.zeros_like(logits)
        sides = {l: torch.matmul(columns(l, kfac.record[l][0].detach()).transpose(1, 2), kfac.inv_state[l][0]) for l in layers}
        for c in range(logits.shape[1]):
            torch.autograd.grad(logits[:, c].sum(), list(model.parameters()), retain_graph=True)
            for layer in layers:
                g = kfac.record[layer][1].detach()
                T = torch.bmm(torch.matmul(kfac.inv_state[layer][1].t(), g.reshape(N, g.shape[1], -1)), sides[layer])
                variance[:, c] += T.square_().sum((1, 2))
        return variance

    def update():
        diag.record = record
        diag.update(N)
    stats = alternated({"update": update, "torch_update": torch_update,
                        "predictive": lambda: glm_predictive(model, kfac, x), "torch_predictive": torch_predictive}, rounds)
    sides = [ops.per_sample_operands(l, *record[l]) for l in layers]
    executed = sum(ops.per_sample_plan_flops([ops.PerSampleJob.of(s, None, None, None) for s in sides]))
    algorithmic = sum(2 * s.N * s.m * s.n * s.L for s in sides)
    want = torch_update()
    fresh = Diagonal(model, kinds, per_sample=True)
    fresh.record = record
    fresh.update(N)
    err = max(float((fresh.state[l] - w).norm() / w.norm()) for l, w in zip(layers, want))
    err_p = float((glm_predictive(model, kfac, x)[1] - torch_predictive()).norm() / torch_predictive().norm())
    row = dict(part="model", model="c3d_small", N=N, input=[3, 8, 32, 32], layers=len(layers),
               algorithmic_gflop=algorithmic / 1e9, executed_gflop=executed / 1e9, update_rel_vs_torch=err,
               predictive_rel_vs_torch=err_p)
    for name, s in stats.items():
        spread(row, name, s)
    return [row]


def resnet_part(rounds, dev):
    N = 32
    torch.manual_seed(0)
    model = models.resnet50().to(dev)
    x = torch.randn(N, 3, 224, 224, device=dev)
    labels = torch.randint(0, 1000, (N,), device=dev)
    diag = Diagonal(model, per_sample=True)
    F.cross_entropy(model(x), labels).backward()
    record = {l: [t.detach() for t in diag.record[l]] for l in diag._layers()}

    def update():
        diag.record = record
        diag.update(N)
    row = dict(part="resnet", model="resnet50", N=N, lib=os.path.basename(ops._lib.LIB_PATH))
    spread(row, "update", alternated({"update": update}, rounds)["update"])
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=["pack", "model"], choices=["pack", "model", "resnet"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None, help="append the rows as JSON lines to this file")
    args = ap.parse_args()
    ops.admit_conv_nd(True)
    ops.admit_conv3d_per_sample(True)
    dev = torch.device("cuda:0")
    rows = []
    for part, run in (("pack", pack_part), ("model", model_part), ("resnet", resnet_part)):
        if part in args.part:
            rows += run(args.rounds, dev)
            ops.release_workspaces()
            torch.cuda.empty_cache()
    for r in rows:
        print(json.dumps(r))
    if args.json:
        with open(args.json, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
