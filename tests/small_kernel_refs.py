"""Plain references for tests/test_small_kernels_gpu.py and tests/test_philox_reference_cpu.py: Python integers, integer
numpy and float64 torch on the CPU.  Nothing here calls the library."""
import functools
import math

import numpy as np
import torch

# ---------------------------------------------------------------------------------------------- Philox4x32-10
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57          # multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85          # Weyl constants of the key schedule
MASK32, MASK64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 from its definition, in Python integers: (c0, c1, c2, c3), (k0, k1) -> four 32-bit words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32          # the key is bumped after each round
    return c0, c1, c2, c3


def philox_words(seed: int, offset: int, nquad: int) -> np.ndarray:
    """(nquad, 4) uint64 array of the 32-bit words of counters offset .. offset + nquad (64-bit, wrapping) of the stream
    keyed by `seed`: counter words {ctr_lo, ctr_hi, 0, 0}, key {seed_lo, seed_hi}.  The same rounds as `philox4x32_10`
    on whole arrays (a 32 x 32 bit product fits uint64)."""
    seed &= MASK64
    ctr = np.uint64(offset & MASK64) + np.arange(nquad, dtype=np.uint64)          # wraps modulo 2^64
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    c0, c1 = ctr & m32, ctr >> s32
    c2, c3 = np.zeros_like(ctr), np.zeros_like(ctr)
    k0, k1 = seed & MASK32, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return np.stack([c0, c1, c2, c3], axis=1)


def normals_from_words(words: np.ndarray) -> np.ndarray:
    """float64 Box-Muller values of (nquad, 4) Philox words, flattened: word pairs (0, 1) and (2, 3) give two values each,
        u1 = ((w >> 8) + 1) / 2^24,  u2 = (w >> 8) / 2^24,  theta = float32(float32(2 pi) * u2),
        z = sqrt(-2 ln u1) * (cos theta, sin theta).
    u1 and u2 are exact in float32; theta is the one quantity rounded to float32 on purpose, as the kernel forms it."""
    z = np.empty((words.shape[0], 4), dtype=np.float64)
    for p in range(2):
        u1 = ((words[:, 2 * p] >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
        u2 = ((words[:, 2 * p + 1] >> np.uint64(8)).astype(np.float64) / 16777216.0).astype(np.float32)
        theta = (np.float32(2.0 * math.pi) * u2).astype(np.float64)              # one float32 product
        r = np.sqrt(-2.0 * np.log(u1))
        z[:, 2 * p] = r * np.cos(theta)
        z[:, 2 * p + 1] = r * np.sin(theta)
    return z.reshape(-1)


@functools.lru_cache(maxsize=None)
def philox_normals(seed: int, offset: int, count: int) -> np.ndarray:
    """The first `count` values of `randn(seed, offset)` in float64 (read-only, computed once per argument triple)."""
    z = normals_from_words(philox_words(seed, offset, (count + 3) // 4))[:count]
    z.setflags(write=False)
    return z


# ---------------------------------------------------------------------------------------------- packed column pairs
def packed_map(a: int) -> torch.Tensor:
    """(a, a) int64 table t(i, k) = t(k, i): the pairs i <= k enumerated in order (0,0), (0,1), .., (0,a-1), (1,1), .."""
    t = torch.empty(a, a, dtype=torch.int64)
    at = 0
    for i in range(a):
        for k in range(i, a):
            t[i, k] = t[k, i] = at
            at += 1
    assert at == a * (a + 1) // 2
    return t


def vtv_unsymmetrised(V4: torch.Tensor, sigma: torch.Tensor, a: int, b: int) -> torch.Tensor:
    """w[(i, j), (k, l)] = sigma[i b + j] sigma[k b + l] V4[i a + k, j b + l] in float64, (a b, a b)."""
    V = V4.double().view(a, a, b, b)                                             # [i, k, j, l]
    s = sigma.double()
    return torch.einsum("ikjl->ijkl", V).reshape(a * b, a * b) * torch.outer(s, s)


def vtv_from_packed(V4p: torch.Tensor, sigma: torch.Tensor, a: int, b: int) -> torch.Tensor:
    """vtv[(i, j), (k, l)] = sigma[i b + j] sigma[k b + l] V4p[t_a(i, k), t_b(j, l)] in float64."""
    ta, tb = packed_map(a), packed_map(b)
    V = V4p.double()[ta[:, :, None, None], tb[None, None, :, :]]                 # [i, k, j, l]
    s = sigma.double()
    return torch.outer(s, s) * torch.einsum("ikjl->ijkl", V).reshape(a * b, a * b)


# ---------------------------------------------------------------------------------------------- selection
def select_reference(lam: torch.Tensor, n: int, m: int, rank: int):
    """(I, J) of the top-`rank` magnitudes of a tie-free CPU vector: topk of |lambda|, then the sorted distinct rows
    idx // m and columns idx % m."""
    idx = torch.topk(lam.abs(), min(rank, n * m)).indices
    return torch.unique(idx // m), torch.unique(idx % m)


def ulp32(x: torch.Tensor) -> torch.Tensor:
    """Spacing of float32 at the float32 nearest to the float64 tensor x, as float64."""
    return torch.from_numpy(np.spacing(np.abs(x.numpy()).astype(np.float32)).astype(np.float64))
