"""float64 restatements for the tests of INF's linearised predictive, on the CPU.

A layer's regularised precision is  Pi = V diag(s lambda) V^T + diag(s corr + add),  V = kron(U_A, U_G), parameter index
i m + j with i on the A side.  `woodbury_terms` restates the closed form the estimator evaluates; `dense_covariance`
inverts Pi as a matrix.  Nothing here imports the package."""
import torch


def project_reference(A, B, W, U):
    """Z[n, j, l] = sum_i W[i, j] (A_n B_n^T)[i, j] U[i, l] in float64: A (S, M, L), B (S, Nc, L), W (M, Nc), U (M, R)."""
    A, B, W, U = (t.detach().double().cpu() for t in (A, B, W, U))
    P = torch.einsum("nil,njl->nij", A, B)
    return torch.einsum("ij,nij,ir->njr", W, P, U)


def random_layer(n, m, a, b, gen, add=0.3, multiply=2.0):
    """(U_A, U_G, lam, corr, add, multiply) of a random layer: orthonormal columns, positive spectra."""
    ua = torch.linalg.qr(torch.randn(n, n, generator=gen, dtype=torch.float64))[0][:, :a].contiguous()
    ug = torch.linalg.qr(torch.randn(m, m, generator=gen, dtype=torch.float64))[0][:, :b].contiguous()
    lam = torch.rand(a * b, generator=gen, dtype=torch.float64) * 3 + 0.1
    corr = torch.rand(n * m, generator=gen, dtype=torch.float64) + 0.05
    return ua, ug, lam, corr, add, multiply


def kron(ua, ug):
    """V = kron(U_A, U_G): row i m + j, column k b + l."""
    ua, ug = ua.double(), ug.double()
    return (ua[:, None, :, None] * ug[None, :, None, :]).reshape(ua.shape[0] * ug.shape[0], ua.shape[1] * ug.shape[1])


def dense_precision(ua, ug, lam, corr, add, multiply):
    V = kron(ua, ug)
    return V @ torch.diag(multiply * lam.double()) @ V.t() + torch.diag(multiply * corr.double() + add)


def dense_covariance(ua, ug, lam, corr, add, multiply):
    return torch.linalg.inv(dense_precision(ua, ug, lam, corr, add, multiply))


def woodbury_terms(ua, ug, lam, corr, add, multiply):
    """(r2 as (n, m), F) with F = B^-1 diag(sigma), B = chol(V_s^T V_s + I), V_s = diag(r) V diag(sigma)."""
    ua, ug, lam, corr = ua.double(), ug.double(), lam.double(), corr.double()
    (n, a), (m, b) = ua.shape, ug.shape
    r2 = 1.0 / (multiply * corr + add)
    sigma = torch.sqrt(multiply * lam)
    V = kron(ua, ug)
    Vs = r2.sqrt()[:, None] * V * sigma[None, :]
    Bc = torch.linalg.cholesky(Vs.t() @ Vs + torch.eye(a * b, dtype=torch.float64))
    F = torch.linalg.solve_triangular(Bc, torch.diag(sigma), upper=False)
    return r2.view(n, m), F


def low_rank_vector(P, r2, ua, ug, F):
    """Y = F vec(U_A^T (R2 o P) U_G) for a Jacobian P seen as (n, m); vec in the order k b + l."""
    q = (ua.double().t() @ (r2 * P.double()) @ ug.double()).reshape(-1)
    return F @ q


def variance_terms(P, r2, ua, ug, F):
    """(T1, T2): sum r2 P**2 and ||F q||**2; the variance is T1 - T2."""
    y = low_rank_vector(P, r2, ua, ug, F)
    return float((r2 * P.double() ** 2).sum()), float(y @ y)


def sampler_covariance(ua, ug, lam, corr, add, multiply):
    """M M^T of the sampler the estimator shares with its model (INF.sampler: Y_l - Y_r with the pre-sampler P_c = S A^-T
    (I - B^-1) A^-1 S)), as a dense matrix: sample = M x for standard normal x."""
    ua, ug, lam, corr = ua.double(), ug.double(), lam.double(), corr.double()
    (n, a), (m, b) = ua.shape, ug.shape
    r2 = 1.0 / (multiply * corr + add)
    r = r2.sqrt()
    sigma = torch.sqrt(multiply * lam)
    V = kron(ua, ug)
    Vs = r[:, None] * V * sigma[None, :]
    vtv = Vs.t() @ Vs
    eye = torch.eye(a * b, dtype=torch.float64)
    invA = torch.linalg.inv(torch.linalg.cholesky(vtv))
    invB = torch.linalg.inv(torch.linalg.cholesky(vtv + eye))
    Pc = torch.diag(sigma) @ invA.t() @ (eye - invB) @ invA @ torch.diag(sigma)
    # Y_l = r x; Y_r = r**2 V P_c V^T Y_l
    M = torch.diag(r) - torch.diag(r2) @ V @ Pc @ V.t() @ torch.diag(r)
    return M @ M.t()
