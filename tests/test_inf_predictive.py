"""INF's linearised predictive without a GPU: the switch and the refusals, the C ABI of
`curv_persample_project`, and the float64 restatement of the formula the estimator evaluates against the dense inverse
of the regularised precision."""
import ctypes
import os
import re

import pytest
import torch

import inf_predictive_refs as refs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the switch
@pytest.fixture
def switch():
    from curvature_amd import ops
    was = ops.admit_inf_predictive(False)
    yield ops
    ops.admit_inf_predictive(was)


def test_switch_defaults_off_and_returns_the_previous_value(switch):
    ops = switch
    # the default is what the module is born with (the fixture has set the switch already)
    source = open(os.path.join(ROOT, "curvature_amd", "ops.py")).read()
    assert re.search(r"^_INF_PREDICTIVE = False$", source, re.M)
    assert ops.inf_predictive_admitted() is False
    assert ops.admit_inf_predictive() is False
    assert ops.inf_predictive_admitted() is True
    assert ops.admit_inf_predictive(False) is True
    assert ops.inf_predictive_admitted() is False


CALLS = [
    ("functional_variance", lambda e: e.functional_variance(torch.zeros(1))),
    ("functional_variance_grid", lambda e: e.functional_variance_grid(torch.zeros(1, 1), [(1.0, 1.0)])),
    ("stage_output", lambda e: e.stage_output(0, 1, inputs=True)),
    ("functional_covariance", lambda e: e.functional_covariance(torch.zeros(1, 1, 1))),
]


@pytest.mark.parametrize("name, call", CALLS, ids=[c[0] for c in CALLS])
def test_refusals_are_unchanged_with_the_switch_off(switch, name, call):
    """On an INF that has no attribute at all: the refusal comes before anything is touched, with `Curvature`'s message."""
    from curvature_amd.curvatures import INF, BlockDiagonal
    with pytest.raises(NotImplementedError) as off:
        call(INF.__new__(INF))
    with pytest.raises(NotImplementedError) as base:
        call(BlockDiagonal.__new__(BlockDiagonal))
    assert str(off.value) == str(base.value).replace("BlockDiagonal", "INF")
    assert str(off.value).startswith(f"INF.{name}: no linearised predictive for this")
    assert str(off.value).endswith("(KFAC, Diagonal and EFB have one)")


def test_the_grid_refuses_with_the_switch_on(switch):
    from curvature_amd.curvatures import INF
    switch.admit_inf_predictive(True)
    with pytest.raises(NotImplementedError, match="every pair needs its own factorisation"):
        INF.__new__(INF).functional_variance_grid(torch.zeros(1, 1), [(1.0, 1.0)])


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_resolve_and_the_version_is_12():
    from curvature_amd import _lib
    handle = _lib.lib()
    assert handle.curv_version() == 12 and _lib.ABI_VERSION == 12
    for name in ("curv_persample_project", "curv_persample_project_workspace_bytes", "curv_persample_project_plan_flops"):
        assert getattr(handle, name) is not None
        assert name in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "curv_hip.h")).read()
    assert re.search(r"#define CURV_ABI_VERSION 12\b", header)


def test_struct_matches_the_header():
    """Field by field against the typedef in include/curv_hip.h, and the size the C compiler gives it (pointers and
    long long: 8 bytes, the others 4, no padding in this order)."""
    from curvature_amd import _lib
    header = open(os.path.join(ROOT, "include", "curv_hip.h")).read()
    body = re.search(r"typedef struct curv_persample_project_desc \{(.*?)\} curv_persample_project_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, size = [], 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        kind, names = re.match(r"(const float\*|float\*|long long|int32_t|float)\s+(.*)", decl, re.S).groups()
        for name in names.split(","):
            fields.append(name.strip())
            size += 8 if kind.endswith("*") or kind == "long long" else 4
    assert fields == [f[0] for f in _lib.curv_persample_project_desc._fields_]
    assert ctypes.sizeof(_lib.curv_persample_project_desc) == size == 144


def plan_jobs():
    from curvature_amd import ops
    shapes = [(5, 130, 129, 49, 33), (3, 33, 127, 48, 100), (32, 64, 577, 196, 100), (1, 1, 1, 1, 1), (3, 130, 64, 33, 7)]
    return [ops.PerSampleProjectJob(None, None, None, None, None, S, M, Nc, L, M * ((L + 3) // 4 * 4), (L + 3) // 4 * 4,
                                    Nc * ((L + 3) // 4 * 4), (L + 3) // 4 * 4, R=R) for S, M, Nc, L, R in shapes], shapes


def test_plan_queries_of_a_batch_are_the_sums_over_single_jobs():
    from curvature_amd import ops
    jobs, shapes = plan_jobs()
    flops = ops.per_sample_project_plan_flops(jobs)
    assert flops == [ops.per_sample_project_plan_flops([j])[0] for j in jobs]
    for f, (S, M, Nc, L, R) in zip(flops, shapes):
        assert f >= 2 * S * M * Nc * (L + R)
    each = [ops.per_sample_project_workspace_bytes([j]) for j in jobs]
    assert ops.per_sample_project_workspace_bytes(jobs) == sum(each)
    for nbytes, (S, M, Nc, L, R) in zip(each, shapes):
        parts = 1 if M <= 64 else 2 * ((M + 127) // 128)          # no swap: M <= 64 takes the half tile, whatever Nc is
        assert nbytes == (S * parts * Nc * R * 4 + 255) // 256 * 256


def test_plan_refuses_bad_sizes():
    from curvature_amd import _lib, ops
    job = ops.PerSampleProjectJob(None, None, None, None, None, 3, 33, 64, 32, 33 * 32, 32, 64 * 32, 32, R=0)
    with pytest.raises(RuntimeError, match="R 0 below 1"):
        ops.per_sample_project_plan_flops([job])
    assert _lib.lib().curv_persample_project_workspace_bytes(None, 1) == 0


# ------------------------------------------------------------------------------------------------ the formula, float64
LAYERS = [(5, 4, 3, 2), (6, 5, 6, 5), (7, 3, 2, 3), (4, 9, 4, 1)]      # (n, m, a, b): reduced, unreduced, a < b, b = 1


@pytest.mark.parametrize("shape", LAYERS, ids=["n{}m{}a{}b{}".format(*s) for s in LAYERS])
def test_restatement_equals_the_dense_inverse(shape):
    n, m, a, b = shape
    gen = torch.Generator().manual_seed(11 * n + m)
    layer = refs.random_layer(n, m, a, b, gen)
    ua, ug = layer[0], layer[1]
    cov = refs.dense_covariance(*layer)
    r2, F = refs.woodbury_terms(*layer)
    # the Woodbury form itself
    V = refs.kron(ua, ug)
    wood = torch.diag(r2.reshape(-1)) - (r2.reshape(-1, 1) * V) @ F.t() @ F @ (V.t() * r2.reshape(1, -1))
    print(f"{shape}: max |Woodbury - dense inverse| {float((wood - cov).abs().max()):.2e}, max |inverse| "
          f"{float(cov.abs().max()):.2e}")
    assert float((wood - cov).abs().max()) <= 1e-10
    # variance and covariance of random Jacobians
    P = torch.randn(4, n, m, generator=gen, dtype=torch.float64)
    ys = torch.stack([refs.low_rank_vector(p, r2, ua, ug, F) for p in P])
    for c in range(4):
        t1, t2 = refs.variance_terms(P[c], r2, ua, ug, F)
        dense = float(P[c].reshape(-1) @ cov @ P[c].reshape(-1))
        assert abs((t1 - t2) - dense) <= 1e-10 * max(1.0, abs(dense))
        for d in range(4):
            gram = float((r2 * P[c] * P[d]).sum() - ys[c] @ ys[d])
            dense = float(P[c].reshape(-1) @ cov @ P[d].reshape(-1))
            assert abs(gram - dense) <= 1e-10 * max(1.0, abs(dense))


def test_the_samplers_covariance_is_not_the_inverse_precision():
    """The record of the discrepancy: the sampler's M M^T (pre-sampler with B^-1 B^-T where (B B^T)^-1 is needed) against
    Pi^-1 on a random layer with n, m, a, b = 5, 4, 3, 2.  The predictive follows Pi^-1; the sampler is left alone."""
    gen = torch.Generator().manual_seed(59)
    layer = refs.random_layer(5, 4, 3, 2, gen)
    cov = refs.dense_covariance(*layer)
    mmt = refs.sampler_covariance(*layer)
    gap = float((mmt - cov).abs().max())
    print(f"max |M M^T - Pi^-1| {gap:.2e}, max |Pi^-1| {float(cov.abs().max()):.2e}")
    assert torch.isfinite(mmt).all()
    assert gap > 1e-8 * float(cov.abs().max())               # they differ, far above rounding
    assert gap < 0.1 * float(cov.abs().max())                # ... and not by much
