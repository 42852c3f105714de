"""`ops.per_sample_project` (csrc/persample.hip, mode PS_PROJECT) against a float64 einsum:

    Z[n, j, l] = sum_i W[i, j] (A_n B_n^T)[i, j] U[i, l]

Sizes on both sides of every tile edge (M: the 64 / 128 row tiles, Nc: the 128 column tiles, L: the 32-value stage and
its tail, R: the 32-column chunk), both operand layouts, a W with zero rows, a strided U, a permuted Z.  Operands are
fenced with NaN, and so is every row's tail in the padded layout: nothing outside the sizes may enter a result.  The bar
is the project's for these products (tests/test_per_sample_gpu.py): relative Frobenius error below 1e-4."""
import pytest
import torch

from conftest import rel_fro
from inf_predictive_refs import project_reference

pytestmark = pytest.mark.gpu
TOL = 1e-4


def operand(S, rows, L, layout, gpu, gen):
    """(tensor, ns, rs, float64 values (S, rows, L)): `rows_outer` is what the pack writes - (rows, S, Lp) with Lp the
    next multiple of 4, here with NaN where the pack writes zeros; `in_place` is an (S, rows, L) record, L % 4 == 0."""
    vals = torch.randn(S, rows, L, generator=gen)
    if layout == "in_place":
        assert L % 4 == 0
        Lp, shape = L, (S, rows, L)
    else:
        Lp, shape = (L + 3) // 4 * 4, (rows, S, (L + 3) // 4 * 4)
    n = shape[0] * shape[1] * shape[2]
    buf = torch.full((n + 128,), float("nan"), device=gpu)
    body = buf[64:64 + n].view(shape)
    if layout == "in_place":
        body.copy_(vals)
        return buf[64:64 + n], rows * L, L, vals.double()
    body[:, :, :L] = vals.permute(1, 0, 2).to(gpu)
    return buf[64:64 + n], Lp, S * Lp, vals.double()


def make_job(M, Nc, L, R, S, layout, gpu, gen, zero_rows=False, u_pad=0, z_permuted=False, first=True):
    from curvature_amd import ops
    A, a_ns, a_rs, Av = operand(S, M, L, layout, gpu, gen)
    B, b_ns, b_rs, Bv = operand(S, Nc, L, layout, gpu, gen)
    W = torch.rand(M, Nc, generator=gen) + 0.5
    if zero_rows:
        W[::3] = 0.0
    Ufull = torch.full((M, R + u_pad), float("nan"))
    Ufull[:, :R] = torch.randn(M, R, generator=gen)
    Wg, Ug = W.to(gpu), Ufull.to(gpu)[:, :R]
    if z_permuted:
        Z = torch.full((S, R, Nc), float("nan"), device=gpu).permute(0, 2, 1)
    else:
        Z = torch.full((S, Nc, R), float("nan"), device=gpu)
    job = ops.PerSampleProjectJob(A, B, Wg, Ug, Z, S, M, Nc, L, a_ns, a_rs, b_ns, b_rs, first=first)
    return job, project_reference(Av, Bv, W, Ufull[:, :R])


# (M, Nc, L, R, S, layout, options)
CASES = [
    (1, 1, 1, 1, 1, "rows_outer", {}),
    (33, 64, 31, 31, 3, "rows_outer", {}),
    (65, 127, 33, 32, 5, "rows_outer", {}),
    (130, 129, 49, 33, 3, "rows_outer", {}),
    (130, 64, 33, 100, 3, "rows_outer", {}),                    # Nc <= 64 < M: where the other modes swap the operands
    (65, 1, 31, 1, 5, "rows_outer", {}),
    (1, 129, 49, 100, 3, "rows_outer", {}),
    (33, 127, 49, 33, 1, "rows_outer", {}),
    (130, 127, 31, 100, 5, "rows_outer", {}),
    (65, 129, 1, 32, 3, "rows_outer", {}),
    (33, 1, 33, 31, 3, "rows_outer", {}),
    (1, 64, 31, 32, 5, "rows_outer", {}),
    (130, 1, 49, 1, 1, "rows_outer", {}),
    (65, 64, 49, 100, 1, "rows_outer", {}),
    (33, 129, 1, 1, 5, "rows_outer", {"zero_rows": True}),
    (130, 129, 33, 33, 5, "rows_outer", {"zero_rows": True, "u_pad": 7}),
    (65, 127, 31, 100, 3, "rows_outer", {"u_pad": 3, "z_permuted": True}),
    (33, 64, 32, 31, 3, "in_place", {}),
    (130, 129, 48, 33, 5, "in_place", {"u_pad": 5}),
    (65, 127, 4, 32, 3, "in_place", {"zero_rows": True}),
    (1, 1, 32, 100, 5, "in_place", {"z_permuted": True}),
    (130, 64, 48, 1, 1, "in_place", {}),
]


@pytest.mark.parametrize("case", CASES, ids=["M{}_Nc{}_L{}_R{}_S{}_{}{}".format(*c[:6], "".join("_" + k for k in c[6]))
                                            for c in CASES])
def test_project_against_float64(gpu, case):
    from curvature_amd import ops
    M, Nc, L, R, S, layout, opts = case
    gen = torch.Generator().manual_seed(1000 * M + 10 * Nc + L + R + S)
    job, want = make_job(M, Nc, L, R, S, layout, gpu, gen, **opts)
    flops = ops.per_sample_project_plan_flops([job])[0]
    assert flops >= 2 * S * M * Nc * (L + R)
    ops.per_sample_project([job])
    got = job.Z.double().cpu()
    assert torch.isfinite(got).all()
    err = rel_fro(got, want)
    print(f"per_sample_project M{M} Nc{Nc} L{L} R{R} S{S} {layout} {opts}: rel_fro {err:.3e}")
    assert err < TOL
    # accumulation: the same product added to what is there gives twice the value, bit for bit
    once = job.Z.clone()
    job.first, job.alpha = False, 1.0
    ops.per_sample_project([job])
    assert torch.equal(job.Z, once + once)
    # alpha
    job.first, job.alpha = True, -0.5
    ops.per_sample_project([job])
    assert torch.equal(job.Z, once * -0.5)


def test_project_alone_and_in_a_batch_agree_bit_for_bit(gpu):
    from curvature_amd import ops
    gen = torch.Generator().manual_seed(5)
    shapes = [(130, 129, 49, 33, 5, "rows_outer"), (33, 127, 48, 100, 3, "in_place"), (65, 64, 31, 32, 5, "rows_outer")]
    jobs = [make_job(*s, gpu, gen)[0] for s in shapes]
    alone = []
    for j in jobs:
        ops.per_sample_project([j])
        alone.append(j.Z.clone())
        j.Z.fill_(float("nan"))
    ops.per_sample_project(jobs)
    for j, z in zip(jobs, alone):
        assert torch.equal(j.Z, z)
    # plan queries of a batch: the sums over single jobs
    assert ops.per_sample_project_plan_flops(jobs) == [ops.per_sample_project_plan_flops([j])[0] for j in jobs]
    each = [ops.per_sample_project_workspace_bytes([j]) for j in jobs]
    assert all(b > 0 for b in each) and ops.per_sample_project_workspace_bytes(jobs) == sum(each)


def test_project_refuses_bad_descriptors(gpu):
    from curvature_amd import ops
    gen = torch.Generator().manual_seed(6)
    job, _ = make_job(33, 64, 32, 31, 3, "in_place", gpu, gen)
    bad = ops.PerSampleProjectJob(job.A, job.B, job.W, job.U, job.Z[:, :, :30], 3, 33, 64, 32, job.a_ns, job.a_rs, job.b_ns,
                                  job.b_rs)
    with pytest.raises(RuntimeError, match="destination must be"):
        ops.per_sample_project([bad])
    odd = ops.PerSampleProjectJob(job.A, job.B, job.W, job.U, job.Z, 3, 33, 64, 32, job.a_ns - 2, job.a_rs, job.b_ns,
                                  job.b_rs)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.per_sample_project([odd])
