"""float64 references on the CPU for the last-layer Laplace predictive (tests/test_head_mc_gpu.py): the Monte-Carlo
softmax of `ops.head_mc` and the dense logit covariance behind `Curvature.head_terms`, the latter written from the
samplers' formulas entry by entry - not from the GEMM formulation the library uses."""
import torch


def head_mc_reference(M, lower, d2, mu, z):
    """(probs (N, K), draws (N, S, K)) in float64 from fp32 inputs on any device: f = mu + M (sqrt(max(d2, 0)) * z).  `M`
    (K, K) or None (identity); with `lower` its strict upper triangle may hold anything.  `d2` (N,) or (N, K)."""
    mu, z, d2 = mu.double().cpu(), z.double().cpu(), d2.double().cpu()
    N, S, K = z.shape
    scale = torch.sqrt(torch.clamp(d2, min=0.0))
    scale = scale[:, None].expand(N, K) if scale.dim() == 1 else scale
    b = scale[:, None, :] * z
    if M is not None:
        M = M.double().cpu()
        if lower:
            M = torch.tril(M.nan_to_num(0.0))
        b = torch.einsum("nsk,ck->nsc", b, M)
    draws = mu[:, None, :] + b
    return torch.softmax(draws, dim=2).mean(dim=1), draws


def head_terms_reference(kind, inv_state, eigvecs, features, has_bias):
    """The dense (N, K, K) float64 covariance of the logits of a Linear head: `kind` "KFAC" (inv_state = (L_A, L_G)),
    "EFB" (eigvecs = (U_A, U_G), inv_state = inv (K, n)) or "Diagonal" (inv_state = inv (K, n)); `features` (N, in)."""
    phi = features.double().cpu()
    if has_bias:
        phi = torch.cat([phi, torch.ones(phi.shape[0], 1, dtype=torch.float64)], dim=1)
    N, n = phi.shape
    if kind == "KFAC":
        L_A, L_G = (t.double().cpu() for t in inv_state)
        A_inv, G_inv = L_A @ L_A.t(), L_G @ L_G.t()
        scalar = torch.stack([phi[i] @ A_inv @ phi[i] for i in range(N)])
        return scalar[:, None, None] * G_inv[None]
    inv = inv_state.double().cpu()
    K = inv.shape[0]
    if kind == "EFB":
        U_A, U_G = (t.double().cpu() for t in eigvecs)
    elif kind == "Diagonal":
        U_A, U_G = torch.eye(n, dtype=torch.float64), torch.eye(K, dtype=torch.float64)
    else:
        raise ValueError(kind)
    out = torch.zeros(N, K, K, dtype=torch.float64)
    for i in range(N):
        # J_c = e_c phi^T, rotated: R_c = U_G^T J_c U_A = (U_G[c, :])^T (U_A^T phi)^T
        rot = [torch.outer(U_G[c], U_A.t() @ phi[i]) for c in range(K)]
        for c in range(K):
            for c2 in range(K):
                out[i, c, c2] = (rot[c] * rot[c2] * inv ** 2).sum()        # over the entries (a, b) of Wm
    return out
