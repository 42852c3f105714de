"""Monte-Carlo softmax of the GLM predictive from the joint logit covariance, without a GPU: the new symbols, the
host-only queries of the C ABI (curv_logit_mc_*) and the error paths of `ops.logit_mc`, `evaluate.glm_predictive_mc`
and `evaluate.eval_glm`."""
import ctypes

import pytest
import torch

from curvature_amd import _lib, ops
from curvature_amd.curvatures import KFAC
from curvature_amd.evaluate import eval_glm, glm_predictive_mc, mc_softmax

NAMES = ("curv_logit_mc_workspace_bytes", "curv_logit_mc_plan_flops", "curv_logit_mc")
CHUNK_MIN, BLOCKS_TARGET = 256, 1024           # the plan of include/curv_hip.h (curv_logit_mc, "Plan")


def small_model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3, padding=1), torch.nn.Flatten(), torch.nn.Linear(75, 4))


def mc_desc(N=70, K=10, S=1000, o_rs=None, o_ns=None, mu_ns=None, z=False, z_ss=None, z_ns=None, outputs=True):
    """One item; the pointers are non-null addresses the host queries never read."""
    arr = (_lib.curv_logit_mc_desc * 1)()
    d = arr[0]
    d.N, d.K, d.S = N, K, S
    d.o_rs = K if o_rs is None else o_rs
    d.o_ns = K * d.o_rs if o_ns is None else o_ns
    d.mu_ns = K if mu_ns is None else mu_ns
    d.cov, d.mu = 256, 512
    if z:
        d.Z = 768
        d.z_ss = K if z_ss is None else z_ss
        d.z_ns = S * d.z_ss if z_ns is None else z_ns
    if outputs:
        d.probs = 1024
    return arr


def chunks_of(N, S):
    """Workgroups per input, from the item's own N and S (the rule the header states)."""
    want = -(-BLOCKS_TARGET // N)
    per = -(-S // want)
    chunk = max(CHUNK_MIN, -(-per // CHUNK_MIN) * CHUNK_MIN)
    return -(-S // chunk)


def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert L.curv_version() == 12
    for name in ("LogitMCJob", "logit_mc", "logit_mc_plan_flops"):
        assert hasattr(ops, name)
    assert callable(glm_predictive_mc) and callable(eval_glm) and callable(mc_softmax)


def test_empty_calls_are_noops():
    L = _lib.lib()
    assert L.curv_logit_mc_workspace_bytes(None, 0) == 0
    assert L.curv_logit_mc_plan_flops(None, 0, None) == 0
    assert L.curv_logit_mc(None, None, 0, None, 0) == 0
    ops.logit_mc([])
    assert ops.logit_mc_plan_flops([]) == []


@pytest.mark.parametrize("kw", [dict(), dict(N=1, K=1, S=1), dict(N=10000, K=16, S=1000), dict(N=1024, K=10, S=1024),
                                dict(N=3, K=5, S=257), dict(o_rs=13, o_ns=140, mu_ns=12), dict(z=True, z_ss=12),
                                dict(N=600, K=3, S=1000)],
                         ids=["plain", "ones", "large", "bench", "just_past_a_chunk", "strided", "explicit_z", "two_chunks"])
def test_host_queries(kw):
    """Scratch: K + 1 floats per input and chunk where the draws of an input are cut into chunks, and zero - without an
    error text - where every input has one chunk.  FLOPs: at least the multiply-adds of the triangular products."""
    L = _lib.lib()
    arr = mc_desc(**kw)
    d = arr[0]
    chunks = chunks_of(d.N, d.S)
    need = L.curv_logit_mc_workspace_bytes(arr, 1)
    if chunks > 1:
        assert need >= 4 * d.N * chunks * (d.K + 1)
    else:
        assert need == 0
    out = (ctypes.c_longlong * 1)()
    assert L.curv_logit_mc_plan_flops(arr, 1, out) == 0
    assert out[0] >= 2 * d.N * d.S * d.K * (d.K + 1) // 2
    # past the plan, the call refuses the missing workspace (chunks) - nothing is launched without a GPU
    if chunks > 1:
        assert L.curv_logit_mc(None, arr, 1, None, 0) == _lib.ERR_WORKSPACE


def test_the_chunk_rule():
    assert chunks_of(1, 256) == 1 and chunks_of(1, 257) == 2 and chunks_of(70, 1000) == 4
    assert chunks_of(600, 1000) == 2 and chunks_of(1024, 1024) == 1 and chunks_of(10000, 1000) == 1


@pytest.mark.parametrize("kw", [dict(K=0), dict(K=17), dict(o_rs=9), dict(o_ns=99), dict(mu_ns=9), dict(S=0), dict(N=0),
                                dict(outputs=False), dict(z=True, z_ss=9), dict(z=True, z_ns=9000),
                                dict(S=(1 << 30) + 1)],
                         ids=["K0", "K17", "o_rs", "o_ns", "mu_ns", "S0", "N0", "no_output", "z_ss", "z_ns", "S_too_large"])
def test_invalid_items_are_refused(kw):
    L = _lib.lib()
    arr = mc_desc(**kw)
    assert L.curv_logit_mc_workspace_bytes(arr, 1) == 0
    assert b"item 0" in L.curv_last_error()
    assert L.curv_logit_mc_plan_flops(arr, 1, (ctypes.c_longlong * 1)()) == _lib.ERR_INVALID
    assert L.curv_logit_mc(None, arr, 1, None, 0) == _lib.ERR_INVALID
    assert b"item 0" in L.curv_last_error()


def test_plan_follows_from_the_items_own_sizes():
    """The scratch and the FLOPs of an item are the same alone and beside others."""
    L = _lib.lib()
    kws = [dict(N=3, K=5, S=1000), dict(N=2000, K=16, S=300), dict(N=70, K=1, S=4096, z=True)]
    both = (_lib.curv_logit_mc_desc * len(kws))()
    alone, flops = [], []
    for k, kw in enumerate(kws):
        one = mc_desc(**kw)
        ctypes.memmove(ctypes.addressof(both[k]), one, ctypes.sizeof(_lib.curv_logit_mc_desc))
        alone.append(L.curv_logit_mc_workspace_bytes(one, 1))
        out = (ctypes.c_longlong * 1)()
        assert L.curv_logit_mc_plan_flops(one, 1, out) == 0
        flops.append(out[0])
    assert alone[0] > 0 and alone[1] == 0 and alone[2] > 0
    assert L.curv_logit_mc_workspace_bytes(both, len(kws)) == sum(alone)
    out = (ctypes.c_longlong * len(kws))()
    assert L.curv_logit_mc_plan_flops(both, len(kws), out) == 0
    assert list(out) == flops


def test_plan_flops_through_ops():
    job = ops.LogitMCJob(None, None, 1000, N=70, K=10)
    assert ops.logit_mc_plan_flops([job]) == [2 * 70 * 1000 * 8 * 3 * 4]


def test_cpu_tensors_are_refused():
    cov, mu = torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3)
    job = ops.LogitMCJob(cov, mu, 8, probs=torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.logit_mc([job])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mc_softmax(mu, cov, [0, 1, 2], 8)


def test_cpu_model_is_refused():
    model = small_model()
    x = torch.zeros(3, 2, 5, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        glm_predictive_mc(model, KFAC(model), x)
    for predictive in ("probit", "mc"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            eval_glm(model, [(x, torch.zeros(3, dtype=torch.long))], KFAC(model), predictive=predictive)


def test_unknown_predictive_and_sample_count():
    model = small_model()
    with pytest.raises(ValueError, match="predictive"):
        eval_glm(model, [], KFAC(model), predictive="other")
    with pytest.raises(ValueError, match="samples"):
        glm_predictive_mc(model, KFAC(model), torch.zeros(3, 2, 5, 5), samples=0)
