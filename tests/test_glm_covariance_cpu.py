"""Joint output covariance of the linearised Laplace (GLM) predictive without a GPU: the new symbols, the host-only
queries of the C ABI (curv_persample_cov_*), and the error paths of `Curvature.stage_output` / `functional_covariance`,
`ops.per_sample_cov_reduce` and `evaluate.glm_predictive_joint`."""
import ctypes

import pytest
import torch

from curvature_amd import _lib, ops
from curvature_amd.curvatures import INF, KFAC, BlockDiagonal, Curvature, Diagonal, EFB
from curvature_amd.evaluate import glm_predictive_joint


def small_model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3, padding=1), torch.nn.Flatten(), torch.nn.Linear(75, 4))


def cov_desc(S=3, K=10, M=70, Nc=200, L=49, a_rs=None, b_rs=None, a_cs=None, w_rs=None, o_rs=None, o_ns=None):
    """One item; `w_rs` given: W set (to a non-null address the host queries never read)."""
    arr = (_lib.curv_persample_cov_desc * 1)()
    d = arr[0]
    d.S, d.K, d.M, d.Nc, d.L = S, K, M, Nc, L
    Lp = (L + 3) // 4 * 4                                # rows start on 16-byte boundaries
    d.a_rs, d.b_rs = Lp if a_rs is None else a_rs, Lp if b_rs is None else b_rs
    d.a_ns, d.b_ns = M * d.a_rs, Nc * d.b_rs
    d.a_cs = S * d.a_ns if a_cs is None else a_cs
    d.o_rs = K if o_rs is None else o_rs
    d.o_ns = K * d.o_rs if o_ns is None else o_ns
    d.alpha = 1.0
    if w_rs is not None:
        d.W, d.w_rs = 256, w_rs
    return arr


def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    for name in ("curv_persample_cov_workspace_bytes", "curv_persample_cov_plan_flops", "curv_persample_cov_reduce"):
        assert name in _lib.SIGNATURES
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert L.curv_version() == 12
    assert _lib.PERSAMPLE_COV_MAX_OUTPUTS == ops.PERSAMPLE_COV_MAX_OUTPUTS == 16
    for name in ("PerSampleCovJob", "per_sample_cov_reduce", "per_sample_cov_plan_flops"):
        assert hasattr(ops, name)
    assert issubclass(ops.PerSampleCovJob, ops._PerSampleProduct)
    assert callable(glm_predictive_joint)
    for est in (KFAC, Diagonal, EFB):
        assert est.stage_output is not Curvature.stage_output
        assert est.functional_covariance is not Curvature.functional_covariance


def test_empty_calls_are_noops():
    L = _lib.lib()
    assert L.curv_persample_cov_workspace_bytes(None, 0) == 0
    assert L.curv_persample_cov_plan_flops(None, 0, None) == 0
    assert L.curv_persample_cov_reduce(None, None, 0, None, 0) == 0
    ops.per_sample_cov_reduce([])
    assert ops.per_sample_cov_plan_flops([]) == []


@pytest.mark.parametrize("kw", [dict(), dict(S=1, K=1, M=1, Nc=1, L=1), dict(K=16, S=32, M=512, Nc=4608, L=49),
                                dict(K=3, S=32, M=64, Nc=147, L=12544), dict(w_rs=203, o_rs=11, o_ns=112),
                                dict(M=1, a_rs=0), dict(a_cs=0)],
                         ids=["plain", "ones", "wide", "long", "strided", "single_row", "shared_A"])
def test_host_queries(kw):
    L = _lib.lib()
    arr = cov_desc(**kw)
    d = arr[0]
    assert L.curv_persample_cov_workspace_bytes(arr, 1) >= 4 * d.S * d.K * (d.K + 1) // 2
    out = (ctypes.c_longlong * 1)()
    assert L.curv_persample_cov_plan_flops(arr, 1, out) == 0
    assert out[0] >= 2 * d.S * d.K * d.M * d.Nc * d.L


@pytest.mark.parametrize("kw", [dict(K=0), dict(K=17), dict(a_rs=50), dict(b_rs=51), dict(a_cs=10502), dict(a_cs=-4),
                                dict(o_rs=9), dict(o_ns=99), dict(S=0), dict(M=0), dict(Nc=0), dict(L=0), dict(a_rs=48),
                                dict(w_rs=199), dict(K=16, S=8, M=4096, Nc=64, L=4096)],
                         ids=["K0", "K17", "a_rs_unaligned", "b_rs_unaligned", "a_cs_unaligned", "a_cs_negative", "o_rs",
                              "o_ns", "S0", "M0", "Nc0", "L0", "a_rs", "w_rs", "2GiB_over_the_outputs"])
def test_invalid_items_are_refused(kw):
    L = _lib.lib()
    arr = cov_desc(**kw)
    assert L.curv_persample_cov_workspace_bytes(arr, 1) == 0
    assert b"item 0" in L.curv_last_error()
    assert L.curv_persample_cov_plan_flops(arr, 1, (ctypes.c_longlong * 1)()) == _lib.ERR_INVALID
    assert L.curv_persample_cov_reduce(None, arr, 1, None, 0) == _lib.ERR_INVALID
    assert b"item 0" in L.curv_last_error()


def test_plan_follows_from_the_items_own_sizes():
    """The scratch and the FLOPs of an item are the same alone and beside others."""
    L = _lib.lib()
    kws = [dict(S=5, K=3, M=37, Nc=70, L=37), dict(S=200, K=1, M=16, Nc=26, L=5), dict(S=100, K=10, M=10, Nc=85, L=1)]
    both = (_lib.curv_persample_cov_desc * len(kws))()
    alone, flops = [], []
    for k, kw in enumerate(kws):
        one = cov_desc(**kw)
        ctypes.memmove(ctypes.addressof(both[k]), one, ctypes.sizeof(_lib.curv_persample_cov_desc))
        alone.append(L.curv_persample_cov_workspace_bytes(one, 1))
        out = (ctypes.c_longlong * 1)()
        assert L.curv_persample_cov_plan_flops(one, 1, out) == 0
        flops.append(out[0])
    assert L.curv_persample_cov_workspace_bytes(both, len(kws)) == sum(alone)
    out = (ctypes.c_longlong * len(kws))()
    assert L.curv_persample_cov_plan_flops(both, len(kws), out) == 0
    assert list(out) == flops


def test_estimators_without_a_linearised_predictive():
    model = small_model()
    out = torch.zeros(3, 4, 4)
    block = BlockDiagonal(model)
    with pytest.raises(NotImplementedError, match="BlockDiagonal"):
        block.functional_covariance(out)
    with pytest.raises(NotImplementedError, match="BlockDiagonal"):
        block.stage_output(0, 4, inputs=True)
    inf = INF.__new__(INF)                               # (its constructor wants the factors of a whole chain)
    with pytest.raises(NotImplementedError, match="INF"):
        inf.functional_covariance(out)
    with pytest.raises(NotImplementedError, match="INF"):
        inf.stage_output(0, 4, inputs=True)


@pytest.mark.parametrize("make", [KFAC, lambda m: Diagonal(m, per_sample=True),
                                  lambda m: EFB(m, {}, eigvecs={}, per_sample=True)], ids=["kfac", "diag", "efb"])
def test_missing_inverse_state_and_slot_range(make):
    est = make(small_model())
    with pytest.raises(AssertionError, match="invert"):
        est.stage_output(0, 4, inputs=True)
    with pytest.raises(ValueError, match="slot"):
        est.stage_output(4, 4, inputs=True)
    with pytest.raises(ValueError, match="slot"):
        est.stage_output(0, 17, inputs=True)
    with pytest.raises(RuntimeError, match="staged"):
        est.functional_covariance(torch.zeros(3, 4, 4))


def test_cpu_model_is_refused():
    model = small_model()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        glm_predictive_joint(model, KFAC(model), torch.zeros(3, 2, 5, 5))


def test_cpu_tensors_are_refused():
    A, B, out = torch.zeros(2 * 3 * 8 * 4), torch.zeros(3 * 5 * 4), torch.zeros(3, 2, 2)
    job = ops.PerSampleCovJob(A, B, None, out, 2, 3 * 8 * 4, 3, 8, 5, 4, 8 * 4, 4, 5 * 4, 4, first=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.per_sample_cov_reduce([job])


def test_cpu_records_are_refused():
    """Past the driver's own check: CPU records reach `stage_output` and raise there."""
    model = small_model()
    diag = Diagonal(model, per_sample=True)
    model(torch.randn(3, 2, 5, 5)).sum().backward()
    diag.inv_state = {l: torch.ones(l.weight.shape[0], l.weight[0].numel() + 1) for l in (model[0], model[2])}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        diag.stage_output(0, 4, inputs=True)
