"""Evaluation metrics of a predictive distribution on torch tensors of any device: what the reference's
``curvature/utils.py`` computes on numpy arrays, under its names, arguments, defaults and return shapes, written from the
formulas.  `probabilities` is (N, K), `labels` (N,) integers; numpy arrays are taken as well.  Everything is accumulated
in float64 on the device of `probabilities`; a scalar comes back as a Python float (one host read), an array as a float64
tensor on that device.  `auroc` scores how well an uncertainty (`evaluate.last_layer_uncertainty`'s `epistemic`, or
`predictive_entropy`) tells out-of-domain from in-domain inputs."""
from typing import Tuple, Union

import numpy
import torch


def _probabilities(probabilities) -> torch.Tensor:
    p = torch.as_tensor(probabilities)
    if p.dim() != 2:
        raise ValueError(f"probabilities must be (N, K), got {tuple(p.shape)}")
    return p.to(torch.float64)


def _labels(labels, like: torch.Tensor) -> torch.Tensor:
    t = torch.as_tensor(labels).to(device=like.device, dtype=torch.long)
    if t.dim() != 1 or t.shape[0] != like.shape[0]:
        raise ValueError(f"labels must be ({like.shape[0]},), got {tuple(t.shape)}")
    return t


def _top(p: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(confidence, prediction) per row; among equal maxima the first class, as `numpy.argmax` has it on every device."""
    conf = p.max(dim=1).values
    classes = torch.arange(p.shape[1], device=p.device)
    first = torch.where(p == conf[:, None], classes, p.shape[1]).min(dim=1).values
    return conf, first


def accuracy(probabilities, labels) -> float:
    """The top-1 accuracy in percent."""
    p = _probabilities(probabilities)
    _, prediction = _top(p)
    return float(100.0 * (prediction == _labels(labels, p)).to(torch.float64).mean())


def confidence(probabilities, mean: bool = True) -> Union[float, torch.Tensor]:
    """The largest class probability of every prediction, or its mean over the predictions."""
    conf = _probabilities(probabilities).max(dim=1).values
    return float(conf.mean()) if mean else conf


def negative_log_likelihood(probabilities, labels) -> float:
    """``-mean(log(p[n, label_n] + 1e-12))``."""
    p = _probabilities(probabilities)
    picked = p.gather(1, _labels(labels, p)[:, None])[:, 0]
    return float(-torch.log(picked + 1e-12).mean())


def expected_calibration_error(probabilities, labels, bins: int = 10):
    """The expected calibration error over `bins` bins of equal width, ``edge_i < confidence <= edge_{i+1}``:
    ``(ece, bin_ace, bin_accuracy, bin_confidence)``, the arrays of length `bins` with zeros for empty bins;
    ``ece = sum_m |B_m| / n * |confidence(B_m) - accuracy(B_m)|``."""
    p = _probabilities(probabilities)
    conf, prediction = _top(p)
    hit = (prediction == _labels(labels, p)).to(torch.float64)
    edges = torch.from_numpy(numpy.linspace(0, 1, bins + 1)).to(p.device)
    member = ((conf[None, :] > edges[:-1, None]) & (conf[None, :] <= edges[1:, None])).to(torch.float64)
    count = member.sum(dim=1)
    filled = count > 0
    safe = torch.clamp(count, min=1.0)
    bin_accuracy = torch.where(filled, (member @ hit) / safe, 0.0)
    bin_confidence = torch.where(filled, (member @ conf) / safe, 0.0)
    bin_ace = bin_confidence - bin_accuracy
    ece = (count / max(conf.shape[0], 1) * bin_ace.abs()).sum()
    return float(ece), bin_ace, bin_accuracy, bin_confidence


def calibration_curve(probabilities, labels, bins: int = 20):
    """The calibration error over bins of (about) equal count: ``(ece, confidence, accuracy, proportion)`` of the bins that
    hold a prediction.  The edges are every ``ceil(n / bins)``-th sorted confidence, the largest one appended unless
    ``n % ceil(n / bins) == 1``; a bin takes ``lower < confidence < upper``, both strict, as the reference has it - so
    predictions that sit on an edge belong to no bin."""
    p = _probabilities(probabilities)
    conf, prediction = _top(p)
    hit = (prediction == _labels(labels, p)).to(torch.float64)
    n = conf.shape[0]
    step = (n + bins - 1) // bins
    edges = torch.sort(conf).values[::step]
    if n % step != 1:
        edges = torch.cat([edges, conf.max()[None]])
    member = ((conf[None, :] > edges[:-1, None]) & (conf[None, :] < edges[1:, None])).to(torch.float64)
    count = member.sum(dim=1)
    filled = count > 0
    count = count[filled]
    xs = (member @ conf)[filled] / count
    ys = (member @ hit)[filled] / count
    zs = count / n
    return float(((xs - ys).abs() * zs).sum()), xs, ys, zs


def predictive_entropy(probabilities, mean: bool = False) -> Union[float, torch.Tensor]:
    """``H(y) = -sum_c y_c ln y_c`` of every prediction (rows are normalised to sum 1 first, ``0 ln 0 = 0``), or its mean
    over the predictions."""
    p = _probabilities(probabilities)
    p = p / p.sum(dim=1, keepdim=True)
    entropy = -torch.xlogy(p, p).sum(dim=1)
    return float(entropy.mean()) if mean else entropy


def auroc(scores_in, scores_out) -> float:
    """The area under the ROC curve of telling out-of-domain from in-domain inputs by a score that should be larger out
    of domain: the probability that a score of `scores_out` exceeds one of `scores_in`, ties counted half."""
    inside = torch.as_tensor(scores_in).to(torch.float64).flatten()
    outside = torch.as_tensor(scores_out).to(device=inside.device, dtype=torch.float64).flatten()
    if inside.numel() == 0 or outside.numel() == 0:
        raise ValueError("auroc: both sets of scores must hold at least one value")
    ordered = torch.sort(inside).values
    below = torch.searchsorted(ordered, outside, right=False)          # in-domain scores strictly smaller
    upto = torch.searchsorted(ordered, outside, right=True)            # ... smaller or equal
    wins = (below + upto).to(torch.float64).sum() / 2.0
    return float(wins / (inside.numel() * outside.numel()))
