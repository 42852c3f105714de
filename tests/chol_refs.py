"""Inputs and float64 references for tests/test_chol_factor_inverse_gpu.py and tests/test_chol_refs_cpu.py: torch on the
CPU (torch.linalg.cholesky, solve_triangular, cholesky_ex).  Nothing here calls the library.  Every cached tensor is
shared between tests and must not be written to."""
import functools

import torch

PIVOT_MIN = 1e-3          # threshold the prescribed-pivot matrices are run with
SMALL_DIAG = 1e-3         # L[r, r] of a planted column: its pivot is SMALL_DIAG ** 2 = 1e-6

# (n, r): a planted column at the first and last column of a 16-column panel, of a 64-block, of a 4-block (256) and a
# 6-block (384) outer panel, and at the last column of the matrix
PIVOT_CASES = [(70, 0), (70, 15), (70, 16), (70, 63), (70, 64), (300, 255), (300, 256), (300, 257), (450, 383),
               (450, 384), (450, 449)]
# (n, planted columns): the first failure must win across 64-blocks (launches) and inside one 16-column panel
DOUBLE_CASES = [(100, (70, 20)), (70, (3, 9))]


# ---------------------------------------------------------------------------------------------- matrices
@functools.lru_cache(maxsize=None)
def well_conditioned(n: int, seed: int = 0) -> torch.Tensor:
    """(n, n) float64, symmetric: X X^T / (3 n) for a fixed-seed n x 3 n normal X; condition number below 20."""
    g = torch.Generator().manual_seed(1000 * seed + n)
    X = torch.randn(n, 3 * n, dtype=torch.float64, generator=g)
    M = X @ X.t() / (3 * n)
    return (M + M.t()) / 2


def _prescribed_factor(n: int, planted, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(7000 * seed + n)
    L = torch.tril(0.1 * torch.randn(n, n, dtype=torch.float64, generator=g), -1)
    L += torch.diag(1.0 + torch.rand(n, dtype=torch.float64, generator=g))
    for r in planted:
        L[r, r] = SMALL_DIAG
    return L


@functools.lru_cache(maxsize=None)
def prescribed_pivots(n: int, planted: tuple = (), seed: int = 0) -> torch.Tensor:
    """M = L L^T (float64, symmetrised), L lower triangular with 0.1 randn below the diagonal and a diagonal in [1, 2]
    except L[r, r] = 1e-3 for r in `planted`: Cholesky pivots >= 1 everywhere, 1e-6 at the planted columns.  With the
    same seed and `planted = ()` the matrix is the positive-definite stand-in of the same size."""
    L = _prescribed_factor(n, planted, seed)
    M = L @ L.t()
    return (M + M.t()) / 2


@functools.lru_cache(maxsize=None)
def not_pd(n: int, r: int, seed: int = 0) -> torch.Tensor:
    """A well-conditioned matrix with 5 subtracted from M[r, r]: pivots before column r unchanged, pivot r <= -3."""
    M = well_conditioned(n, seed).clone()
    M[r, r] -= 5.0
    return M


@functools.lru_cache(maxsize=None)
def lower_rhs(n: int, seed: int = 0) -> torch.Tensor:
    """(n, n) float64 lower-triangular normal right-hand side."""
    g = torch.Generator().manual_seed(90000 + 10 * n + seed)
    return torch.tril(torch.randn(n, n, dtype=torch.float64, generator=g))


# ---------------------------------------------------------------------------------------------- references
def damped(M: torch.Tensor, d: float) -> torch.Tensor:
    """The matrix `curv_chol_factor_inverse` promises to factorise, in float64.  float64 input: (M + M^T) / 2 + d I in
    float64.  float32 input: M + d I in float32, symmetrised in float32, then promoted."""
    n = M.shape[0]
    if M.dtype == torch.float64:
        return (M + M.t()) / 2 + d * torch.eye(n, dtype=torch.float64)
    assert M.dtype == torch.float32
    reg = M + torch.diag(M.new_full((n,), d))
    return ((reg + reg.t()) / 2.0).double()


def damped_reversed(F: torch.Tensor, add: float, mul: float) -> torch.Tensor:
    """The matrix the sweep of `curv_chol_inv_lower` factorises: J (sqrt(mul) F + sqrt(add) I, symmetrised) J with the
    damping done in float32 as the estimators do, promoted to float64; J reverses the index order."""
    assert F.dtype == torch.float32
    reg = torch.tensor(mul ** 0.5, dtype=torch.float32) * F + torch.diag(F.new_full((F.shape[0],), add ** 0.5))
    return torch.flip(((reg + reg.t()) / 2.0).double(), (0, 1))


def chol_inverse(A: torch.Tensor):
    """(C, C^-1) for the lower Cholesky factor C of a float64 matrix A."""
    C = torch.linalg.cholesky(A)
    X = torch.linalg.solve_triangular(C, torch.eye(A.shape[0], dtype=torch.float64), upper=False)
    return C, X


@functools.lru_cache(maxsize=None)
def inverse_of(n: int, dtype: torch.dtype, d: float, seed: int = 0) -> torch.Tensor:
    """chol(damped(well_conditioned(n).to(dtype), d))^-1, float64."""
    return chol_inverse(damped(well_conditioned(n, seed).to(dtype), d))[1]


@functools.lru_cache(maxsize=None)
def factor_of(n: int, dtype: torch.dtype, d: float, seed: int = 0) -> torch.Tensor:
    """chol(damped(well_conditioned(n).to(dtype), d)), float64."""
    return torch.linalg.cholesky(damped(well_conditioned(n, seed).to(dtype), d))


def solve_lower(C: torch.Tensor, R: torch.Tensor) -> torch.Tensor:
    return torch.linalg.solve_triangular(C, R, upper=False)


def pivots(A: torch.Tensor) -> torch.Tensor:
    """The Cholesky pivots d_c = C[c, c]^2 of a positive-definite float64 matrix."""
    C, info = torch.linalg.cholesky_ex(A)
    assert int(info) == 0
    return torch.diagonal(C) ** 2


def pivots_past_failures(A: torch.Tensor) -> torch.Tensor:
    """The pivots of the root-free elimination A = L D L^T (the same d_c as `pivots` while they are positive), which does
    not stop at a non-positive one: for matrices with two planted columns, whose second planted pivot - 1e-6 behind a
    column that was divided by 1e-3 - may come out negative once the matrix is rounded to float32."""
    A = A.clone()
    d = torch.empty(A.shape[0], dtype=torch.float64)
    for c in range(A.shape[0]):
        d[c] = A[c, c]
        col = A[c + 1:, c].clone()
        A[c + 1:, c + 1:] -= torch.outer(col, col) / d[c]
    return d


def failing_word(A: torch.Tensor) -> int:
    """LAPACK's status of a Cholesky factorisation of A: 0, or 1 + the index of the first non-positive pivot."""
    return int(torch.linalg.cholesky_ex(A).info)


def condition_number(M: torch.Tensor) -> float:
    w = torch.linalg.eigvalsh(M)
    return float(w[-1] / w[0])
