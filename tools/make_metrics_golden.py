#!/usr/bin/env python
"""Writes tests/golden/metrics_reference.npz: seeded inputs and what the reference's own ``curvature/utils.py`` makes of
them - the fixture `curvature_amd.metrics` is tested against (tests/test_metrics_cpu.py).

    python tools/make_metrics_golden.py --reference DIR [--out FILE]

`DIR` is a checkout of the reference (it holds ``curvature/utils.py``; scipy, psutil and tqdm are needed to import it).
The inputs are float32; the reference gets them as float64 arrays of the same values, so both sides compute in float64.
Cases: ``a`` (N = 200, K = 5) and ``b`` (N = 64, K = 33), Dirichlet rows with uniform labels; ``ties`` (N = 48, K = 3),
confidences from {0.375, 0.5, 0.75, 1} - exact in binary, so 0.5, 0.75 and 1 sit ON edges of 4 (0.5 and 1 also of 10)
equal-width bins, all of them repeat at the equal-count edges, and a row of confidence 0.375 has two equal maxima; ``one``
(N = 1).  Per case the file holds
``<case>/probs``, ``<case>/labels`` and one entry per function and bin count.  Data only."""
import argparse
import os
import sys

import numpy as np

ECE_BINS, CURVE_BINS = (10, 4), (20, 5)


def cases():
    rng = np.random.default_rng(20240607)
    out = {}
    for name, (n, k) in (("a", (200, 5)), ("b", (64, 33)), ("one", (1, 5))):
        out[name] = (rng.dirichlet(np.full(k, 0.5), size=n).astype(np.float32), rng.integers(0, k, size=n))
    top = rng.choice(np.array([0.25, 0.5, 0.75, 1.0]), size=48)
    probs = np.stack([top, (1 - top) / 2, (1 - top) / 2], axis=1).astype(np.float32)
    out["ties"] = (probs, rng.integers(0, 3, size=48))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory that holds the reference's curvature/ package")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests",
                                                  "golden", "metrics_reference.npz"))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    from curvature import utils as ref
    data = {}
    for name, (probs, labels) in cases().items():
        p = probs.astype(np.float64)
        data[f"{name}/probs"], data[f"{name}/labels"] = probs, labels.astype(np.int64)
        data[f"{name}/accuracy"] = np.float64(ref.accuracy(p, labels))
        data[f"{name}/confidence_mean"] = np.float64(ref.confidence(p))
        data[f"{name}/confidence"] = ref.confidence(p, mean=False)
        data[f"{name}/negative_log_likelihood"] = np.float64(ref.negative_log_likelihood(p, labels))
        data[f"{name}/predictive_entropy"] = ref.predictive_entropy(p)
        data[f"{name}/predictive_entropy_mean"] = np.float64(ref.predictive_entropy(p, mean=True))
        for bins in ECE_BINS:
            for part, value in zip(("ece", "ace", "accuracy", "confidence"), ref.expected_calibration_error(p, labels, bins)):
                data[f"{name}/expected_calibration_error_{bins}/{part}"] = np.asarray(value, dtype=np.float64)
        for bins in CURVE_BINS:
            for part, value in zip(("ece", "confidence", "accuracy", "proportion"), ref.calibration_curve(p, labels, bins)):
                data[f"{name}/calibration_curve_{bins}/{part}"] = np.asarray(value, dtype=np.float64)
    np.savez_compressed(args.out, **data)
    print(f"wrote {args.out}: {len(data)} arrays, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
