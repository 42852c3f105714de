#!/usr/bin/env python
"""The results of every kernel on the NT stage engine (csrc/nt_stage.h) as .npy files, for a byte-for-byte comparison
of two builds of the library on one box:
    python tools/dump_nt_products.py OUT_A
    CURV_ALT_LIB=/path/to/other/libcurv_hip.so python tools/dump_nt_products.py OUT_B
    cmp every file; `sha256` printed at the end is one hash over all of them in the order written.
Inputs are seeded on the CPU and copied to the GPU.  gemm_nt_kernel: the shapes and operand forms of the test_gemm_nt_*
tests of tests/test_kfac_api_gpu.py; the per-sample products: SHAPES of tests/test_glm_predictive_gpu.py (squares and
the quadratic reduction) and of tests/test_glm_covariance_gpu.py, with and without W.  The whole run is a fraction of a
second of GPU work and ends itself after LIMIT seconds."""
import hashlib
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from curvature_amd import _lib  # noqa: E402

if os.environ.get("CURV_ALT_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["CURV_ALT_LIB"])
import numpy as np  # noqa: E402
import torch  # noqa: E402
from curvature_amd import ops  # noqa: E402

LIMIT = 240
QUAD_SHAPES = [(5, 130, 150, 37), (9, 6, 151, 100), (33, 150, 16, 1), (100, 10, 85, 1), (200, 16, 26, 5)]   # S M Nc L
COV_SHAPES = [(5, 3, 37, 70, 37), (4, 16, 6, 151, 100), (33, 10, 150, 16, 1), (100, 10, 10, 85, 1), (200, 1, 16, 26, 5),
              (3, 5, 130, 150, 49)]                                                                          # S K M Nc L
ALPHA = 1.5


def strided_operand(slots, S, rows, L, gen, gpu):
    """(slots, S, rows, L) values with gaps of NaN between rows, samples and slots (the operands of the tests)."""
    rs = (L + 3) // 4 * 4 + 4
    ns = rows * rs + 8
    cs = S * ns + 12
    buf = torch.full((64 + slots * cs + 64,), float("nan"))
    view = buf[64:64 + slots * cs].view(slots, cs)[:, :S * ns].view(slots, S, ns)[:, :, :rows * rs].view(slots, S, rows, rs)
    view[..., :L] = torch.randn(slots, S, rows, L, generator=gen)
    return buf.to(gpu)[64:], cs, ns, rs


def weights(M, Nc, gen, gpu):
    wide = torch.full((M, Nc + 3), float("nan"))
    wide[:, :Nc] = torch.rand(M, Nc, generator=gen) + 0.1
    return wide.to(gpu)[:, :Nc]


def gemm_results(gpu):
    gen = torch.Generator().manual_seed(1)
    rand = lambda *shape: torch.randn(*shape, generator=gen).to(gpu)     # noqa: E731
    tril = lambda k: torch.tril(torch.randn(k, k, generator=gen)).to(gpu)  # noqa: E731
    for M, N, K in ((130, 200, 40), (128, 128, 1536)):
        A, Bt, E = rand(M, K), rand(N, K), rand(M, N)
        C = torch.full((M, N), float("nan"), device=gpu)
        ops.gemm_batched([ops.Gemm(A, Bt.t(), C, alpha=2.0, epilogue=ops.EPI_MUL_E, E=E)])
        yield f"gemm_{M}x{N}x{K}", C
    M, N, K = 128, 128, 1536
    out = torch.empty(K, N, device=gpu)
    ops.gemm_batched([ops.Gemm(tril(K), rand(N, K).t(), out, tri=ops.TRI_A_LOWER)])
    yield "gemm_tri_a_lower_1536", out
    out = torch.empty(M, K, device=gpu)
    ops.gemm_batched([ops.Gemm(rand(M, K), tril(K).t(), out, tri=ops.TRI_B_UPPER)])
    yield "gemm_tri_b_upper_1536", out
    M, N, K = 130, 200, 401                                              # odd pitches, K % 4 != 0
    A, Bt = rand(M, K + 3)[:, 1:K + 1], rand(N, K + 5)[:, 2:K + 2]
    C = torch.full((M, N), float("nan"), device=gpu)
    ops.gemm_batched([ops.Gemm(A, Bt.t(), C, alpha=0.5, epilogue=ops.EPI_ADD_E, E=rand(M, N))])
    yield "gemm_unaligned_130x200x401", C
    K = 2304                                                             # few tiles: K-sliced, with a triangular cut
    out = rand(K, 96)
    ops.gemm_batched([ops.Gemm(tril(K), rand(96, K).t(), out, beta=1.0, tri=ops.TRI_A_LOWER)])
    yield "gemm_split_tri_a_lower_2304", out
    out = rand(100, K)
    ops.gemm_batched([ops.Gemm(rand(100, K), tril(K).t(), out, alpha=2.0, beta=1.0, tri=ops.TRI_B_UPPER)])
    yield "gemm_split_tri_b_upper_2304", out


def per_sample_results(gpu):
    for index, (S, M, Nc, L) in enumerate(QUAD_SHAPES):
        gen = torch.Generator().manual_seed(100 + index)
        A, _, a_ns, a_rs = strided_operand(1, S, M, L, gen, gpu)
        B, _, b_ns, b_rs = strided_operand(1, S, Nc, L, gen, gpu)
        W = weights(M, Nc, gen, gpu)
        name = f"{S}x{M}x{Nc}x{L}"
        C = torch.full((M, Nc), float("nan"), device=gpu)
        ops.per_sample_sq_accumulate([ops.PerSampleJob(A, B, C, S, M, Nc, L, a_ns, a_rs, b_ns, b_rs, alpha=ALPHA, first=True)])
        yield f"sq_{name}", C
        for tag, w in (("ones", None), ("W", W)):
            out = torch.full((S,), float("nan"), device=gpu)
            ops.per_sample_quad_reduce([ops.PerSampleQuadJob(A, B, w, out, S, M, Nc, L, a_ns, a_rs, b_ns, b_rs, alpha=ALPHA,
                                                             first=True)])
            yield f"quad_{tag}_{name}", out
    for index, (S, K, M, Nc, L) in enumerate(COV_SHAPES):
        gen = torch.Generator().manual_seed(300 + index)
        A, a_cs, a_ns, a_rs = strided_operand(K, S, M, L, gen, gpu)
        B, _, b_ns, b_rs = strided_operand(1, S, Nc, L, gen, gpu)
        W = weights(M, Nc, gen, gpu)
        for tag, w in (("ones", None), ("W", W)):
            out = torch.full((S, K, K), float("nan"), device=gpu)
            ops.per_sample_cov_reduce([ops.PerSampleCovJob(A, B, w, out, K, a_cs, S, M, Nc, L, a_ns, a_rs, b_ns, b_rs,
                                                           alpha=ALPHA, first=True)])
            yield f"cov_{tag}_{S}x{K}x{M}x{Nc}x{L}", out


def main():
    signal.alarm(LIMIT)                                                  # the run's own time limit
    outdir = sys.argv[1]
    os.makedirs(outdir, exist_ok=True)
    gpu = torch.device("cuda:0")
    digest, count = hashlib.sha256(), 0
    for produce in (gemm_results, per_sample_results):
        for name, result in produce(gpu):
            arr = result.detach().cpu().numpy()
            assert np.isfinite(arr).all(), name
            np.save(os.path.join(outdir, name + ".npy"), arr)
            digest.update(name.encode() + arr.tobytes())
            count += 1
    print(f"{_lib.LIB_PATH}: {count} files in {outdir}, sha256 {digest.hexdigest()}")


if __name__ == "__main__":
    main()
