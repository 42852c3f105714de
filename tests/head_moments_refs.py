"""float64 reference on the CPU for `ops.head_mc_moments` (tests/test_head_moments_gpu.py), on top of
`head_refs.head_mc_reference`: the moments are formed from the float64 draws, not by the kernel's formula."""
import torch

from head_refs import head_mc_reference


def head_moments_reference(M, lower, d2, mu, z):
    """(probs (N, K), entropy (N,), probs_sq (N, K), draws (N, S, K)) in float64 from fp32 inputs on any device:
    p_s = softmax(f_s), probs = mean_s p_s, entropy = mean_s -sum_c xlogy(p_s, p_s), probs_sq = mean_s p_s ** 2."""
    _, draws = head_mc_reference(M, lower, d2, mu, z)
    p = torch.softmax(draws, dim=2)
    return p.mean(dim=1), -torch.xlogy(p, p).sum(dim=2).mean(dim=1), (p * p).mean(dim=1), draws


def entropy_of(probs):
    """H(p) per row in float64, 0 ln 0 = 0."""
    p = probs.double().cpu()
    return -torch.xlogy(p, p).sum(dim=-1)
