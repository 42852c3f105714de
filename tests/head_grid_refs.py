"""float64 references on the CPU for the last-layer Laplace predictive over a grid of damping pairs
(tests/test_head_grid_gpu.py): what `ops.head_grid` computes, written from the table of DESIGN.md K24 entry by entry, and
the dense logit covariance behind `Curvature.head_terms_grid`, from `state`, the eigenvectors and the explicit
regularised inverse - not from the GEMM formulation the library uses."""
import math

import torch


def head_grid_reference(Y, shift, gain, T=None, u=None, v=None):
    """(H, N, K) float64: out[h, r, j] = gain[h] r_h[j] sum_i Y[r, i]^2 / (T[j, i] + shift[h]); dense (`T` (K, n), r_h = 1)
    or separable (`u` (K,), `v` (n,): T[j, i] = v[i], r_h[j] = 1 / (u[j] + shift[h]))."""
    Y = Y.double().cpu()
    N, n = Y.shape
    if T is not None:
        T = T.double().cpu()
        K = T.shape[0]
    else:
        u, v = u.double().cpu(), v.double().cpu()
        K = u.shape[0]
    out = torch.zeros(len(shift), N, K, dtype=torch.float64)
    for h, (s, g) in enumerate(zip(shift, gain)):
        for r in range(N):
            y2 = Y[r] ** 2
            if T is not None:
                out[h, r] = g * (y2[None, :] / (T + s)).sum(dim=1)
            else:
                out[h, r] = g * (y2 / (v + s)).sum() / (u + s)
    return out


def augmented(features, has_bias):
    phi = features.double().cpu()
    if has_bias:
        phi = torch.cat([phi, torch.ones(phi.shape[0], 1, dtype=torch.float64)], dim=1)
    return phi


def head_grid_covariance_reference(kind, state, eigvecs, features, has_bias, pairs):
    """The dense (H, N, K, K) float64 covariance of the logits of a Linear head under the posterior that
    ``invert(add, multiply)`` stands for, for every (add, multiply) = (n_h, s_h) of `pairs` (already resolved for the
    layer): `kind` "KFAC" (state = (A, G); the factored damping (sqrt(s) A + sqrt(n) I) (x) (sqrt(s) G + sqrt(n) I), both
    inverted explicitly), "EFB" (eigvecs = (U_A, U_G), state (K, n)) or "Diagonal" (state (K, n)): the precision
    s state + n, entry by entry, in the basis of the eigenvectors (EFB) or of the weights themselves (Diagonal)."""
    phi = augmented(features, has_bias)
    N, n = phi.shape
    out = []
    for add, multiply in pairs:
        if kind == "KFAC":
            A, G = (t.double().cpu() for t in state)
            A_inv = torch.linalg.inv(math.sqrt(multiply) * A + math.sqrt(add) * torch.eye(n, dtype=torch.float64))
            G_inv = torch.linalg.inv(math.sqrt(multiply) * G + math.sqrt(add) * torch.eye(G.shape[0], dtype=torch.float64))
            scalar = torch.stack([phi[i] @ A_inv @ phi[i] for i in range(N)])
            out.append(scalar[:, None, None] * G_inv[None])
            continue
        var = 1.0 / (multiply * state.double().cpu() + add)             # the variance of entry (a, b) of the rotated Wm
        K = var.shape[0]
        if kind == "EFB":
            U_A, U_G = (t.double().cpu() for t in eigvecs)
        elif kind == "Diagonal":
            U_A, U_G = torch.eye(n, dtype=torch.float64), torch.eye(K, dtype=torch.float64)
        else:
            raise ValueError(kind)
        sigma = torch.zeros(N, K, K, dtype=torch.float64)
        for i in range(N):
            # J_c = e_c phi^T, rotated: R_c = U_G^T J_c U_A = (U_G[c, :])^T (U_A^T phi)^T
            rot = [torch.outer(U_G[c], U_A.t() @ phi[i]) for c in range(K)]
            for c in range(K):
                for c2 in range(K):
                    sigma[i, c, c2] = (rot[c] * rot[c2] * var).sum()
        out.append(sigma)
    return torch.stack(out)


def condition(kind, state, pair):
    """The float64 condition number of the regularised precision of `pair` = (add, multiply): KFAC, the larger of its two
    factors, (sqrt(s) lambda_max + sqrt(n)) / sqrt(n); EFB and Diagonal, (s max state + n) / n."""
    add, multiply = pair
    if kind == "KFAC":
        top = max(float(torch.linalg.eigvalsh(F.double().cpu()).max()) for F in state)
        return (math.sqrt(multiply) * top + math.sqrt(add)) / math.sqrt(add)
    return (multiply * float(state.double().max()) + add) / add
