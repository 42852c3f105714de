"""Inputs, float64 references and yardsticks for tests/test_eigh_direct_gpu.py and tests/test_eigh_refs_cpu.py: torch on
the CPU (torch.linalg.eigh, torch.linalg.qr).  Nothing here calls the library.  Every cached tensor is shared between
tests and must not be written to.

A generator returns the float32 matrix F the library is given.  The reference of F is torch.linalg.eigh(sym(F)) in
float64, sym(F) = (F + F^T) / 2 formed in float64 - what eigh_prepare32_kernel and eigh_input64_kernel form themselves.
The YARDSTICK of F is what that reference achieves once it is rounded to the library's output type (float32): no
float32 result can be expected to do better, and every bar of the GPU tests is a small multiple of it or follows from
the tolerance include/curv_hip.h documents (off(A) <= 1e-8 ||A||_F up to 1024 wide).  None comes from the library."""
import functools

import torch

F64 = torch.float64
# block (32), tile (64) and two-tile edges, one width with ragged last tile and several blocks, the last width of the
# 1e-8 rule; WIDE: the first width past it (np = 1088) and one more (np = 1152)
SIZES = [1, 2, 32, 33, 63, 64, 65, 127, 128, 129, 321, 1024]
WIDE = [1025, 1100]
WIDE_FAMILIES = ["lowrank", "indefinite"]
SUBSPACE_SIZES = [33, 65, 129, 321]
SUBSPACE_FAMILIES = ["planted_a", "planted_b", "planted_c"]      # planted_d is excluded: see `groups`
FAMILIES = ["lowrank", "indefinite", "planted_a", "planted_b", "planted_c", "planted_d", "asymmetric"]
SCALED = [("lowrank", 129), ("planted_a", 129)]
SCALES = [-40, 40, -100, 100]
TIE_SIZES = [65, 129]
PROMISED = 1e-8           # off(A) <= PROMISED ||A||_F: the documented default up to 1024 wide
QUANTUM = 2.0 ** -10      # `asymmetric`: every entry of both parts is a multiple of it, below 4 in size

_SEED = {"lowrank": 11, "indefinite": 12, "planted_a": 13, "planted_b": 14, "planted_c": 15, "planted_d": 16,
         "asymmetric": 17, "ties": 18}


def _gen(tag: str, n: int) -> torch.Generator:
    return torch.Generator().manual_seed(100003 * _SEED[tag] + n)


def sym(F: torch.Tensor) -> torch.Tensor:
    """(F + F^T) / 2 in float64."""
    D = F.double()
    return (D + D.t()) / 2


# ---------------------------------------------------------------------------------------------- matrices
def spectrum(n: int, which: str) -> torch.Tensor:
    """Ascending float64 eigenvalues of `planted`.  a: all simple, equally spaced in [-1, 2]; b: n // 2 times 1.0, the
    rest 3.0; c: n - 3 times 1.0 below the simple 2.0, 3.0, 4.0 (below 4 wide: the first n of the outliers);
    d: geometric, 1e-6 ... 1."""
    if which == "a":
        return torch.linspace(-1.0, 2.0, n, dtype=F64)
    if which == "b":
        return torch.cat([torch.full((n // 2,), 1.0, dtype=F64), torch.full((n - n // 2,), 3.0, dtype=F64)])
    if which == "c":
        m = max(n - 3, 0)
        return torch.cat([torch.full((m,), 1.0, dtype=F64), torch.tensor([2.0, 3.0, 4.0], dtype=F64)[:n - m]])
    assert which == "d"
    return torch.flip(torch.logspace(0.0, -6.0, n, dtype=F64), (0,))


def _planted64(n: int, which: str) -> torch.Tensor:
    Q, _ = torch.linalg.qr(torch.randn(n, n, dtype=F64, generator=_gen("planted_" + which, n)))
    M = (Q * spectrum(n, which)) @ Q.t()
    return (M + M.t()) / 2


@functools.lru_cache(maxsize=None)
def matrix(family: str, n: int) -> torch.Tensor:
    """The (n, n) float32 input of a family.
    lowrank:     X X^T / k for a normal n x k X, k = max(1, n // 3) - the shape of a Kronecker factor of few samples;
    indefinite:  (G + G^T) / (2 sqrt(n)) for a normal G: eigenvalues of both signs in about [-1.5, 1.5];
    planted_x:   Q diag(spectrum(n, x)) Q^T, Q from a float64 QR, rounded to float32;
    asymmetric:  S + K, S = planted_a rounded to multiples of 2^-10, K = T - T^T skew from multiples of 2^-10 with
                 ||K||_F about ||S||_F: F != F^T from 2 wide up, and (F + F^T) / 2 = S without any rounding."""
    if family == "lowrank":
        k = max(1, n // 3)
        X = torch.randn(n, k, dtype=F64, generator=_gen(family, n))
        M = X @ X.t() / k
        return ((M + M.t()) / 2).float()
    if family == "indefinite":
        G = torch.randn(n, n, dtype=F64, generator=_gen(family, n))
        return ((G + G.t()) / (2.0 * n ** 0.5)).float()
    if family.startswith("planted_"):
        return _planted64(n, family[-1]).float()
    assert family == "asymmetric"
    S = torch.round(_planted64(n, "a") / QUANTUM) * QUANTUM
    rms = float(S.pow(2).mean().sqrt())
    u = torch.rand(n, n, dtype=F64, generator=_gen(family, n)) * 2.0 - 1.0
    T = torch.triu(torch.round(u * (3.0 ** 0.5) * rms / QUANTUM) * QUANTUM, 1)
    K = T - T.t()
    F = (S + K).float()
    assert torch.equal(F.double(), S + K) and float(F.abs().max()) < 4.0
    return F


@functools.lru_cache(maxsize=None)
def scaled(family: str, n: int, s: int) -> torch.Tensor:
    """matrix(family, n) * 2^s in float32 (exact as long as nothing leaves the normal range: test_eigh_refs_cpu.py)."""
    return matrix(family, n) * torch.tensor(2.0 ** s, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def diagonal_with_ties(n: int) -> torch.Tensor:
    """A diagonal float32 matrix whose entries are drawn from {-2, ..., 3}: every value many times, out of order."""
    d = torch.randint(-2, 4, (n,), generator=_gen("ties", n)).float()
    return torch.diag(d)


def groups(family: str, n: int):
    """Index groups (positions in ascending order of the eigenvalues) whose invariant subspaces are compared: every
    cluster and every simple eigenvalue of planted a, b, c.  planted_d is EXCLUDED: its eigenvalues fall geometrically
    to 1e-6 and a gap is a fixed share of the eigenvalue, down to below 1e-6 ||F|| - the Davis-Kahan bar divides by
    the gap and is then far above float32 accuracy: it would check nothing (test_eigh_refs_cpu.py has the figures).
    The other families have no planted gaps, and only SUBSPACE_SIZES are compared (1024 rank-one projectors of a
    1024-wide matrix are seconds of CPU time for nothing the narrower ones do not show)."""
    if n not in SUBSPACE_SIZES:
        return []
    if family == "planted_a":
        return [[i] for i in range(n)]
    if family == "planted_b":
        return [g for g in (list(range(n // 2)), list(range(n // 2, n))) if g]
    if family == "planted_c":
        m = max(n - 3, 0)
        return [g for g in ([list(range(m))] + [[i] for i in range(m, n)]) if g]
    return []


# ---------------------------------------------------------------------------------------------- measures
def residual(S: torch.Tensor, U: torch.Tensor, w: torch.Tensor) -> float:
    """||S U - U diag(w)||_F / ||S||_F, all float64."""
    return float(torch.linalg.norm(S @ U - U * w) / torch.linalg.norm(S))


def orthogonality(U: torch.Tensor) -> float:
    """max |U^T U - I|, float64."""
    return float((U.t() @ U - torch.eye(U.shape[1], dtype=F64)).abs().max())


def projector_distance(B: torch.Tensor, C: torch.Tensor) -> float:
    """||B B^T - C C^T||_F for two n x k float64 blocks of columns (formed explicitly: the difference is ~1e-8)."""
    return float(torch.linalg.norm(B @ B.t() - C @ C.t()))


# ---------------------------------------------------------------------------------------------- references
class Yardstick:
    """The float64 reference of one input and what its float32 rounding achieves.
    w, U: eigenvalues (ascending) and eigenvectors of sym(F), float64;  fro, two: ||sym(F)||_F and ||sym(F)||_2;
    res_ref, orth_ref: residual and orthogonality of (U.float(), w.float());
    groups: [(indices, proj_ref, gap)] - proj_ref = ||P(U32[:, g]) - P(U[:, g])||_F, gap = the distance of the group's
    eigenvalues to the rest of the spectrum (absolute; gap / two is the relative gap)."""

    def __init__(self, F: torch.Tensor, index_groups=()):
        S = sym(F)
        self.S = S
        self.w, self.U = torch.linalg.eigh(S)
        self.fro = float(torch.linalg.norm(S))
        self.two = float(self.w.abs().max())
        U32, w32 = self.U.float().double(), self.w.float().double()
        self.res_ref = residual(S, U32, w32)
        self.orth_ref = orthogonality(U32)
        self.groups = []
        n = S.shape[0]
        for g in index_groups:
            inside = torch.zeros(n, dtype=torch.bool)
            inside[g] = True
            gap = float((self.w[inside][:, None] - self.w[~inside][None, :]).abs().min()) if bool((~inside).any()) else float("inf")
            self.groups.append((g, projector_distance(U32[:, g], self.U[:, g]), gap))


@functools.lru_cache(maxsize=None)
def yardstick(family: str, n: int) -> Yardstick:
    return Yardstick(matrix(family, n), groups(family, n))


def eigenvalue_bound(y: Yardstick) -> torch.Tensor:
    """|w - w_ref| may reach the rounding of the float32 output, 2^-24 |w_ref|, plus twice the promised off-norm
    (Weyl: an off-diagonal part of norm e moves no eigenvalue by more than e)."""
    return 2.0 ** -24 * y.w.abs() + 2.0 * PROMISED * y.fro


def projector_bound(y: Yardstick, proj_ref: float, gap: float, factor: float) -> float:
    """factor times the rounded reference's own distance, or Davis-Kahan on twice the promised off-norm."""
    return max(factor * proj_ref, 2.0 * PROMISED * y.fro / gap)
