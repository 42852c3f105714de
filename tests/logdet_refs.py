"""float64 restatements for the tests of the Laplace evidence, on the CPU: the segment sums of
`curv_logsum_grid` with their bar, the per-estimator log-determinants of `Curvature.log_det_grid` from an estimator's own
tensors, and the dense regularised precisions they stand for.  Nothing here imports the package."""
import math

import torch

BAR = 1e-11           # |got - want| <= BAR * (sum |term| + count): see `bar`


def f64(t):
    return t.detach().double().cpu()


def bar(terms: torch.Tensor) -> float:
    """The bar of one output whose float64 terms are `terms`.  At most 2e4 terms per output in these tests: a worst-case
    summation error of count * 2^-53 relative to sum |term| (2.2e-12), a couple of ulp (2^-53 each) for the multiply-add
    (fused or not) and for `log` on every term: 1e-11 leaves about a factor of 4.  `+ count` covers terms that are near
    zero because the argument of the logarithm is near 1, where its relative error is not small."""
    return BAR * (float(terms.abs().sum()) + terms.numel())


def log_terms(x, weight, gain, shift) -> torch.Tensor:
    """weight * log(gain * max(x, 0) + shift), element by element, float64."""
    return weight * torch.log(gain * f64(x).flatten().clamp_min(0.0) + shift)


def segment_sums(x, weight, gains, shifts):
    """(want, bars): lists over the pairs for one segment of logarithms."""
    terms = [log_terms(x, weight, g, s) for g, s in zip(gains, shifts)]
    return [float(t.sum()) for t in terms], [bar(t) for t in terms]


def squares_sum(x, weight=1.0):
    terms = weight * f64(x).flatten() ** 2
    return float(terms.sum()), bar(terms)


# ---------------------------------------------------------------------------------------------- per-estimator formulas
def spectrum_log_det(x, n, s):
    """Diagonal, EFB, BlockDiagonal (x = its clamped eigenvalues): sum log(s x+ + n); (want, bar)."""
    terms = log_terms(x, 1.0, s, n)
    return float(terms.sum()), bar(terms)


def kfac_log_det(lam_A, lam_G, n, s):
    """dim(G) sum log(sqrt(s) lambda_A + sqrt(n)) + dim(A) sum log(sqrt(s) lambda_G + sqrt(n)); stacked (G, .) spectra sum
    over their groups, every group with its own dimensions (the last axis)."""
    terms = torch.cat([log_terms(lam_A, float(lam_G.shape[-1]), math.sqrt(s), math.sqrt(n)),
                       log_terms(lam_G, float(lam_A.shape[-1]), math.sqrt(s), math.sqrt(n))])
    return float(terms.sum()), bar(terms)


def inf_log_det(corr, inv_b, n, s):
    """sum log(s corr+ + n) - 2 sum log diag(B^-1), B^-1 as read back from the estimator's own `ops` calls."""
    terms = torch.cat([log_terms(corr, 1.0, s, n), log_terms(torch.diagonal(f64(inv_b)), -2.0, 1.0, 0.0)])
    return float(terms.sum()), bar(terms)


# ---------------------------------------------------------------------------------------------- dense precisions
def sym(F):
    F = f64(F)
    return 0.5 * (F + F.t())


def kfac_dense(A, G, n, s):
    """(sqrt(s) A + sqrt(n) I) (x) (sqrt(s) G + sqrt(n) I) from the float32 factors, float64."""
    A, G = sym(A), sym(G)
    return torch.kron(math.sqrt(s) * A + math.sqrt(n) * torch.eye(A.shape[0], dtype=torch.float64),
                      math.sqrt(s) * G + math.sqrt(n) * torch.eye(G.shape[0], dtype=torch.float64))


def block_dense(F, n, s):
    F = sym(F)
    return s * F + n * torch.eye(F.shape[0], dtype=torch.float64)


def slogdet(P) -> float:
    sign, value = torch.linalg.slogdet(P)
    assert float(sign) == 1.0
    return float(value)


def log_prior(thetas, precisions):
    """-1/2 sum_l n_l ||theta_l||^2 + 1/2 sum_l P_l log n_l for float64 parameter vectors `thetas`."""
    return sum(-0.5 * n * float((t * t).sum()) + 0.5 * t.numel() * math.log(n) for t, n in zip(thetas, precisions))
