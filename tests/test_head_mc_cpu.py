"""Last-layer Laplace predictive without a GPU: the new symbols, the host-only queries of the C ABI (curv_head_mc_*), the
plan rule, and the refusals of `ops.head_mc`, `Curvature.head_terms`, `evaluate.last_layer_predictive` and
`evaluate.eval_last_layer` that need no device."""
import ctypes

import pytest
import torch

from curvature_amd import _lib, ops
from curvature_amd.curvatures import EFB, INF, KFAC, BlockDiagonal, Diagonal, HeadTerms
from curvature_amd.evaluate import _default_head, eval_last_layer, last_layer_predictive

NAMES = ("curv_head_mc_workspace_bytes", "curv_head_mc_plan_flops", "curv_head_mc")
TILE, WGS_TARGET = 32, 256                     # the plan of include/curv_hip.h (curv_head_mc, "Plan")
CAP = 1024


def small_model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3, padding=1), torch.nn.Flatten(), torch.nn.Linear(75, 4))


def mc_desc(N=32, K=100, S=256, M=True, m_rs=None, lower=0, d_cs=1, d_ns=None, mu_ns=None, z=False, z_ss=None,
            z_ns=None, outputs=True, reserved=0):
    """One item; the pointers are non-null addresses the host queries never read."""
    arr = (_lib.curv_head_mc_desc * 1)()
    d = arr[0]
    d.N, d.K, d.S, d.m_lower, d.reserved = N, K, S, lower, reserved
    if M:
        d.M = 128
    d.m_rs = K if m_rs is None else m_rs
    d.d_cs = d_cs
    d.d_ns = (K if d_cs else 1) if d_ns is None else d_ns
    d.mu_ns = K if mu_ns is None else mu_ns
    d.d2, d.mu = 256, 512
    if z:
        d.Z = 768
        d.z_ss = K if z_ss is None else z_ss
        d.z_ns = S * d.z_ss if z_ns is None else z_ns
    if outputs:
        d.probs = 1024
    return arr


def chunks_of(N, S):
    """Workgroups per input, from the item's own N and S (the rule the header states)."""
    tiles = -(-S // TILE)
    per = -(-tiles // -(-WGS_TARGET // N))
    return -(-tiles // per)


def steps_of(K, lower):
    blocks = -(-K // 32)
    return sum(min(blocks, g + 1) if lower else blocks for g in range(blocks))


def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert L.curv_version() == 12 == _lib.ABI_VERSION
    for name in ("HeadMCJob", "head_mc", "head_mc_plan_flops", "HEAD_MC_MAX_CLASSES"):
        assert hasattr(ops, name)
    assert ops.HEAD_MC_MAX_CLASSES == _lib.HEAD_MC_MAX_CLASSES == CAP >= 1024
    header = open(_lib.INCLUDE + "/curv_hip.h").read()
    assert f"#define CURV_HEAD_MC_MAX_CLASSES {CAP}" in header
    assert callable(last_layer_predictive) and callable(eval_last_layer)
    assert HeadTerms._fields == ("M", "lower", "d2", "variance")
    for est in (KFAC, EFB, Diagonal):
        assert callable(est.head_terms)


def test_descriptor_mirrors_the_header():
    """6 pointers, 6 strides, seed and offset, 4 ints, one reserved word: no hidden padding."""
    assert ctypes.sizeof(_lib.curv_head_mc_desc) == 6 * 8 + 6 * 8 + 2 * 8 + 4 * 4 + 8
    assert _lib.curv_head_mc_desc.reserved.offset == 128


def test_empty_calls_are_noops():
    L = _lib.lib()
    assert L.curv_head_mc_workspace_bytes(None, 0) == 0
    assert L.curv_head_mc_plan_flops(None, 0, None) == 0
    assert L.curv_head_mc(None, None, 0, None, 0) == 0
    ops.head_mc([])
    assert ops.head_mc_plan_flops([]) == []


@pytest.mark.parametrize("kw", [dict(), dict(N=1, K=1, S=1), dict(N=32, K=1000, S=256), dict(N=32, K=1000, S=256, lower=1),
                                dict(N=1, K=5, S=33), dict(N=300, K=CAP, S=100), dict(m_rs=103, mu_ns=102),
                                dict(z=True, z_ss=102), dict(M=False, K=10), dict(d_cs=0)],
                         ids=["plain", "ones", "bench", "bench_lower", "two_chunks", "one_chunk_cap", "strided",
                              "explicit_z", "no_M", "scalar_d2"])
def test_host_queries(kw):
    """Scratch: K floats per input and chunk where the draws of an input are cut into chunks, and zero - without an error
    text - where every input has one chunk.  FLOPs: whole 32 x 32 x 32 steps, at least the algorithmic count."""
    L = _lib.lib()
    arr = mc_desc(**kw)
    d = arr[0]
    chunks = chunks_of(d.N, d.S)
    need = L.curv_head_mc_workspace_bytes(arr, 1)
    if chunks > 1:
        assert 4 * d.N * chunks * d.K <= need < 4 * d.N * chunks * d.K + 256
    else:
        assert need == 0
    out = (ctypes.c_longlong * 1)()
    assert L.curv_head_mc_plan_flops(arr, 1, out) == 0
    if d.M:
        assert out[0] == 2 * 32 ** 3 * steps_of(d.K, d.m_lower) * -(-d.S // TILE) * d.N
        assert out[0] >= 2 * d.N * d.S * (d.K * (d.K + 1) // 2 if d.m_lower else d.K * d.K)
    else:
        assert out[0] == 0
    # past the plan, the call refuses the missing workspace (chunks) - nothing is launched without a GPU
    if chunks > 1:
        assert L.curv_head_mc(None, arr, 1, None, 0) == _lib.ERR_WORKSPACE


def test_the_chunk_rule():
    assert chunks_of(1, 32) == 1 and chunks_of(1, 33) == 2 and chunks_of(32, 256) == 8
    assert chunks_of(256, 4096) == 1 and chunks_of(3, 70) == 3 and chunks_of(1, 32 * 257) == 129
    L = _lib.lib()
    assert L.curv_head_mc_workspace_bytes(mc_desc(N=1, K=5, S=32), 1) == 0
    assert L.curv_head_mc_workspace_bytes(mc_desc(N=1, K=5, S=33), 1) == 256


def test_a_triangular_matrix_costs_about_half():
    dense, lower = ops.head_mc_plan_flops([ops.HeadMCJob(True, None, None, 256, N=32, K=1000),
                                           ops.HeadMCJob(True, None, None, 256, N=32, K=1000, lower=True)])
    assert dense == 2 * 32 ** 3 * 32 * 32 * 8 * 32
    assert 0.5 < lower / dense < 0.53
    assert ops.head_mc_plan_flops([ops.HeadMCJob(None, None, None, 256, N=32, K=1000)]) == [0]


@pytest.mark.parametrize("kw", [dict(K=0), dict(K=CAP + 1), dict(N=0), dict(S=0), dict(S=(1 << 30) + 1), dict(m_rs=99),
                                dict(d_cs=2), dict(d_ns=99), dict(d_cs=0, d_ns=0), dict(mu_ns=99), dict(z=True, z_ss=99),
                                dict(z=True, z_ns=9000), dict(outputs=False), dict(reserved=1)],
                         ids=["K0", "K_above_cap", "N0", "S0", "S_too_large", "m_rs", "d_cs", "d_ns", "d_ns_scalar", "mu_ns",
                              "z_ss", "z_ns", "no_output", "reserved"])
def test_invalid_items_are_refused(kw):
    """... with the item's index in the text, also behind valid items, and before anything is launched."""
    L = _lib.lib()
    arr = mc_desc(**kw)
    assert L.curv_head_mc_workspace_bytes(arr, 1) == 0
    assert b"item 0" in L.curv_last_error()
    assert L.curv_head_mc_plan_flops(arr, 1, (ctypes.c_longlong * 1)()) == _lib.ERR_INVALID
    assert L.curv_head_mc(None, arr, 1, None, 0) == _lib.ERR_INVALID
    assert b"item 0" in L.curv_last_error()
    three = (_lib.curv_head_mc_desc * 3)()
    for k, one in enumerate((mc_desc(), mc_desc(K=7, S=3), arr)):
        ctypes.memmove(ctypes.addressof(three[k]), one, ctypes.sizeof(_lib.curv_head_mc_desc))
    assert L.curv_head_mc(None, three, 3, None, 0) == _lib.ERR_INVALID
    assert b"item 2" in L.curv_last_error()


def test_plan_follows_from_the_items_own_sizes():
    """The scratch and the FLOPs of an item are the same alone and beside others."""
    L = _lib.lib()
    kws = [dict(N=3, K=5, S=1000), dict(N=2000, K=160, S=300), dict(N=70, K=1, S=4096, z=True),
           dict(N=2, K=CAP, S=40, lower=1)]
    both = (_lib.curv_head_mc_desc * len(kws))()
    alone, flops = [], []
    for k, kw in enumerate(kws):
        one = mc_desc(**kw)
        ctypes.memmove(ctypes.addressof(both[k]), one, ctypes.sizeof(_lib.curv_head_mc_desc))
        alone.append(L.curv_head_mc_workspace_bytes(one, 1))
        out = (ctypes.c_longlong * 1)()
        assert L.curv_head_mc_plan_flops(one, 1, out) == 0
        flops.append(out[0])
    assert alone[0] > 0 and alone[1] == 0 and alone[2] > 0 and alone[3] > 0
    assert L.curv_head_mc_workspace_bytes(both, len(kws)) == sum(alone)
    out = (ctypes.c_longlong * len(kws))()
    assert L.curv_head_mc_plan_flops(both, len(kws), out) == 0
    assert list(out) == flops


def test_cpu_tensors_are_refused():
    M, d2, mu = torch.eye(3), torch.ones(2), torch.zeros(2, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.head_mc([ops.HeadMCJob(M, d2, mu, 8, probs=torch.zeros(2, 3))])
    model = small_model()
    est = Diagonal(model)
    est.inv_state[model[2]] = torch.ones(4, 76)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        est.head_terms(model[2], torch.zeros(3, 75))


def test_cpu_model_is_refused():
    model = small_model()
    x = torch.zeros(3, 2, 5, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        last_layer_predictive(model, KFAC(model), x)
    for predictive in ("probit", "mc"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            eval_last_layer(model, [(x, torch.zeros(3, dtype=torch.long))], KFAC(model), predictive=predictive)


def test_unknown_predictive_and_sample_count():
    model = small_model()
    x = torch.zeros(3, 2, 5, 5)
    with pytest.raises(ValueError, match="predictive"):
        eval_last_layer(model, [], KFAC(model), predictive="other")
    with pytest.raises(ValueError, match="predictive"):
        last_layer_predictive(model, KFAC(model), x, predictive="other")
    with pytest.raises(ValueError, match="samples"):
        last_layer_predictive(model, KFAC(model), x, predictive="mc", samples=0)


def test_the_default_head_is_the_last_linear_of_inv_state():
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.ReLU(), torch.nn.Linear(5, 4), torch.nn.ReLU(),
                                torch.nn.Linear(4, 3))
    est = Diagonal(model)
    assert _default_head(est) is None
    est.inv_state[model[0]] = torch.ones(5, 7)
    est.inv_state[model[2]] = torch.ones(4, 6)
    assert _default_head(est) is model[2]                 # model[4] is not held
    est.inv_state[model[4]] = torch.ones(3, 5)
    assert _default_head(est) is model[4]


def test_head_terms_refusals():
    model = small_model()
    head, conv = model[2], model[0]
    est = KFAC(model)
    with pytest.raises(AssertionError, match="Inverse state dict is empty"):
        est.head_terms(head, torch.zeros(3, 75))
    est.inv_state[head] = (torch.eye(76), torch.eye(4))
    est.inv_state[conv] = (torch.eye(19), torch.eye(3))
    with pytest.raises(NotImplementedError, match=r"KFAC.head_terms: layer '0'.*nn.Linear.*Conv2d"):
        est.head_terms(conv, torch.zeros(3, 75))
    block = BlockDiagonal(model)
    block.inv_state[head] = torch.eye(4 * 76)
    with pytest.raises(NotImplementedError, match=r"BlockDiagonal.head_terms: layer '2'.*BlockDiagonal"):
        block.head_terms(head, torch.zeros(3, 75))
    assert INF._head_terms.__qualname__ == "Curvature._head_terms"          # (INF: the same refusal, on the GPU suite)

    class World:
        world, rank, force_collective = 2, 0, False

        def owns(self, index):
            return True
    est.shard = World()
    with pytest.raises(NotImplementedError, match=r"KFAC.head_terms: layer '2'.*sharded"):
        est.head_terms(head, torch.zeros(3, 75))
