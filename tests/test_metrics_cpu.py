"""`curvature_amd.metrics` against the outputs of the reference's own ``curvature/utils.py`` on seeded inputs
(tests/golden/metrics_reference.npz, written by tools/make_metrics_golden.py), and `auroc` against pair counting.

Both sides compute in float64 from the same float32 values, so floats agree to 1e-12 relative: the only difference is
the order of float64 sums.  The per-bin arrays must have the reference's length and agree element for element."""
import os

import numpy as np
import pytest
import torch

from curvature_amd import metrics

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_reference.npz"))
CASES = ("a", "b", "ties", "one")
RTOL = 1e-12


def inputs(case, as_numpy=False):
    probs, labels = GOLDEN[f"{case}/probs"], GOLDEN[f"{case}/labels"]
    assert probs.dtype == np.float32 and labels.dtype == np.int64
    return (probs, labels) if as_numpy else (torch.from_numpy(probs), torch.from_numpy(labels))


def close(got, want):
    """Same shape, every element within 1e-12 relative (an exact zero must be met exactly)."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert got.dtype == np.float64 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.all(np.abs(got - want) <= RTOL * np.abs(want)), (got, want)


def test_the_fixture_holds_the_cases_the_test_names():
    shapes = {case: GOLDEN[f"{case}/probs"].shape for case in CASES}
    assert shapes == {"a": (200, 5), "b": (64, 33), "ties": (48, 3), "one": (1, 5)}
    conf = GOLDEN["ties/probs"].max(axis=1)
    assert set(np.unique(conf)) <= {0.375, 0.5, 0.75, 1.0} and len(np.unique(conf)) >= 3      # repeated, on bin edges
    assert os.path.getsize(GOLDEN.fid.name) < 100 * 1024


@pytest.mark.parametrize("as_numpy", [False, True], ids=["tensor", "numpy"])
@pytest.mark.parametrize("case", CASES)
def test_scalars_and_per_input_arrays(case, as_numpy):
    probs, labels = inputs(case, as_numpy)
    for got in (metrics.accuracy(probs, labels), metrics.confidence(probs), metrics.negative_log_likelihood(probs, labels),
                metrics.predictive_entropy(probs, mean=True)):
        assert isinstance(got, float)
    close(metrics.accuracy(probs, labels), GOLDEN[f"{case}/accuracy"])
    close(metrics.confidence(probs), GOLDEN[f"{case}/confidence_mean"])
    close(metrics.confidence(probs, mean=False), GOLDEN[f"{case}/confidence"])
    close(metrics.negative_log_likelihood(probs, labels), GOLDEN[f"{case}/negative_log_likelihood"])
    close(metrics.predictive_entropy(probs), GOLDEN[f"{case}/predictive_entropy"])
    close(metrics.predictive_entropy(probs, mean=True), GOLDEN[f"{case}/predictive_entropy_mean"])


@pytest.mark.parametrize("as_numpy", [False, True], ids=["tensor", "numpy"])
@pytest.mark.parametrize("bins", [10, 4])
@pytest.mark.parametrize("case", CASES)
def test_expected_calibration_error(case, bins, as_numpy):
    probs, labels = inputs(case, as_numpy)
    got = metrics.expected_calibration_error(probs, labels, bins)
    assert isinstance(got[0], float) and all(tuple(part.shape) == (bins,) for part in got[1:])
    for part, value in zip(("ece", "ace", "accuracy", "confidence"), got):
        close(value, GOLDEN[f"{case}/expected_calibration_error_{bins}/{part}"])
    if bins == 10:
        close(metrics.expected_calibration_error(probs, labels)[0], GOLDEN[f"{case}/expected_calibration_error_10/ece"])


@pytest.mark.parametrize("as_numpy", [False, True], ids=["tensor", "numpy"])
@pytest.mark.parametrize("bins", [20, 5])
@pytest.mark.parametrize("case", CASES)
def test_calibration_curve(case, bins, as_numpy):
    probs, labels = inputs(case, as_numpy)
    got = metrics.calibration_curve(probs, labels, bins)
    assert isinstance(got[0], float)
    for part, value in zip(("ece", "confidence", "accuracy", "proportion"), got):
        close(value, GOLDEN[f"{case}/calibration_curve_{bins}/{part}"])
    if bins == 20:
        close(metrics.calibration_curve(probs, labels)[0], GOLDEN[f"{case}/calibration_curve_20/ece"])


def test_ties_reach_the_edges():
    """The tie case is one: with strict inequalities on both sides, predictions on an edge fall out of the equal-count
    bins, and with ``<=`` above they fall into the lower equal-width bin."""
    assert GOLDEN["ties/calibration_curve_5/proportion"].sum() < 1.0
    assert GOLDEN["a/calibration_curve_5/proportion"].sum() < 1.0           # (the edges themselves)
    probs, labels = inputs("ties")
    _, _, _, conf = metrics.expected_calibration_error(probs, labels, 4)
    # (0, 0.25] is empty; 0.5 sits in (0.25, 0.5] beside 0.375; 0.75 and 1.0 each fill the bin they close
    assert float(conf[0]) == 0.0 and 0.375 < float(conf[1]) < 0.5 and float(conf[2]) == 0.75 and float(conf[3]) == 1.0


def test_auroc_against_pair_counting():
    gen = torch.Generator().manual_seed(5)
    inside = torch.randint(0, 12, (50,), generator=gen).float() / 4          # many ties
    outside = torch.randint(3, 16, (40,), generator=gen).float() / 4
    wins = sum(1.0 if o > i else 0.5 if o == i else 0.0 for o in outside.tolist() for i in inside.tolist())
    assert any(o == i for o in outside.tolist() for i in inside.tolist())
    want = wins / (50 * 40)
    assert abs(metrics.auroc(inside, outside) - want) <= RTOL * want
    assert abs(metrics.auroc(inside.numpy(), outside.numpy()) - want) <= RTOL * want
    assert metrics.auroc(inside, inside) == 0.5
    assert metrics.auroc(inside, inside + 100.0) == 1.0 and metrics.auroc(inside + 100.0, inside) == 0.0
    with pytest.raises(ValueError, match="at least one"):
        metrics.auroc(inside, torch.empty(0))


def test_shapes_are_checked():
    with pytest.raises(ValueError, match=r"\(N, K\)"):
        metrics.accuracy(torch.zeros(3), torch.zeros(3))
    with pytest.raises(ValueError, match="labels"):
        metrics.accuracy(torch.zeros(3, 2), torch.zeros(4))
