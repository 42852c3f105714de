"""The entropy split of the last-layer predictive without a GPU: the new symbols and the descriptor of
curv_head_mc_moments, its host-only queries and refusals, and the refusals of `ops.head_mc_moments` and
`evaluate.last_layer_uncertainty` that need no device."""
import ctypes

import pytest
import torch

from curvature_amd import _lib, evaluate, ops
from curvature_amd.curvatures import KFAC

NAMES = ("curv_head_mc_moments_workspace_bytes", "curv_head_mc_moments_plan_flops", "curv_head_mc_moments")
CAP = 1024
SHARED = ("M", "d2", "mu", "Z", "probs", "draws", "m_rs", "d_ns", "d_cs", "mu_ns", "z_ns", "z_ss", "seed", "offset", "N",
          "K", "S", "m_lower")


def desc(N=32, K=100, S=256, M=True, m_rs=None, lower=0, d_cs=1, d_ns=None, mu_ns=None, z=False, z_ss=None, z_ns=None,
         outputs=("probs",), reserved=0, kind=None):
    """One item of `kind` (default: the moments descriptor); the pointers are non-null addresses the host queries never
    read."""
    arr = ((kind or _lib.curv_head_moments_desc) * 1)()
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
    for k, name in enumerate(outputs):
        setattr(d, name, 1024 * (k + 1))
    return arr


def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert L.curv_version() == 12 == _lib.ABI_VERSION
    for name in ("HeadMomentsJob", "head_mc_moments", "head_mc_moments_plan_flops"):
        assert hasattr(ops, name)
    assert callable(evaluate.last_layer_uncertainty) and callable(evaluate.eval_uncertainty)
    assert evaluate.Uncertainty._fields == ("logits", "variance", "probs", "probs_std", "total", "aleatoric", "epistemic")
    header = open(_lib.INCLUDE + "/curv_hip.h").read()
    assert "typedef struct curv_head_moments_desc" in header and "#define CURV_ABI_VERSION 12" in header


def test_descriptor_mirrors_the_header():
    """The first 128 bytes are field for field those of curv_head_mc_desc; then entropy, probs_sq, reserved."""
    new, old = _lib.curv_head_moments_desc, _lib.curv_head_mc_desc
    assert ctypes.sizeof(new) == 152
    assert (new.entropy.offset, new.probs_sq.offset, new.reserved.offset) == (128, 136, 144)
    for name in SHARED:
        assert getattr(new, name).offset == getattr(old, name).offset and getattr(new, name).size == getattr(old, name).size
    assert [f[0] for f in new._fields_][:len(SHARED)] == list(SHARED)
    assert old.m_lower.offset + old.m_lower.size == 128


def test_empty_calls_are_noops():
    L = _lib.lib()
    assert L.curv_head_mc_moments_workspace_bytes(None, 0) == 0
    assert L.curv_head_mc_moments_plan_flops(None, 0, None) == 0
    assert L.curv_head_mc_moments(None, None, 0, None, 0) == 0
    ops.head_mc_moments([])
    assert ops.head_mc_moments_plan_flops([]) == []


def test_workspace_bytes():
    """align_up(N chunks (2 K + 1) 4, 256) per item; 0 - without an error text - where every input has one chunk."""
    L = _lib.lib()
    L.curv_head_mc(None, desc(K=0, kind=_lib.curv_head_mc_desc), 1, None, 0)        # leaves an error text behind
    assert b"item 0" in L.curv_last_error()
    one = desc(N=1, K=5, S=32)
    assert L.curv_head_mc_moments(None, None, 0, None, 0) == 0
    before = L.curv_last_error()
    assert L.curv_head_mc_moments_workspace_bytes(one, 1) == 0
    assert L.curv_last_error() == before                                            # nothing new was said
    assert L.curv_head_mc_moments_plan_flops(one, 1, (ctypes.c_longlong * 1)()) == 0     # ... and the item is valid
    two = desc(N=1, K=5, S=33)
    assert L.curv_head_mc_moments_workspace_bytes(two, 1) == 256
    big = desc(N=1, K=CAP, S=8192)
    assert L.curv_head_mc_moments_workspace_bytes(big, 1) == 256 * 2049 * 4
    odd = desc(N=3, K=37, S=70)                                                     # 3 chunks: 3 * 3 * 75 * 4 = 2700 -> 2816
    assert L.curv_head_mc_moments_workspace_bytes(odd, 1) == 2816
    items = (one, two, big, odd)
    batch = (_lib.curv_head_moments_desc * len(items))()
    for k, item in enumerate(items):
        ctypes.memmove(ctypes.addressof(batch[k]), item, ctypes.sizeof(_lib.curv_head_moments_desc))
    assert L.curv_head_mc_moments_workspace_bytes(batch, len(items)) == 0 + 256 + 256 * 2049 * 4 + 2816
    # past the plan, the call refuses the missing workspace - nothing is launched without a GPU
    assert L.curv_head_mc_moments(None, two, 1, None, 0) == _lib.ERR_WORKSPACE


@pytest.mark.parametrize("kw", [dict(), dict(N=1, K=1, S=1), dict(N=32, K=1000, S=256), dict(N=32, K=1000, S=256, lower=1),
                                dict(N=1, K=5, S=33), dict(N=300, K=CAP, S=100), dict(M=False, K=10), dict(d_cs=0)],
                         ids=["plain", "ones", "bench", "bench_lower", "two_chunks", "one_chunk_cap", "no_M", "scalar_d2"])
def test_plan_flops_are_those_of_head_mc(kw):
    L = _lib.lib()
    new, old = (ctypes.c_longlong * 1)(), (ctypes.c_longlong * 1)()
    assert L.curv_head_mc_moments_plan_flops(desc(**kw), 1, new) == 0
    assert L.curv_head_mc_plan_flops(desc(kind=_lib.curv_head_mc_desc, **kw), 1, old) == 0
    assert new[0] == old[0] and (new[0] > 0) == kw.get("M", True)
    jobs = dict(N=kw.get("N", 32), K=kw.get("K", 100), lower=bool(kw.get("lower", 0)))
    M = True if kw.get("M", True) else None
    assert ops.head_mc_moments_plan_flops([ops.HeadMomentsJob(M, None, None, kw.get("S", 256), **jobs)]) == [new[0]]
    assert ops.head_mc_plan_flops([ops.HeadMCJob(M, None, None, kw.get("S", 256), **jobs)]) == [new[0]]


@pytest.mark.parametrize("kw", [dict(outputs=()), dict(reserved=1), dict(K=CAP + 1), dict(K=0), dict(N=0), dict(S=0),
                                dict(m_rs=99), dict(d_cs=2), dict(d_ns=99), dict(d_cs=0, d_ns=0), dict(mu_ns=99),
                                dict(z=True, z_ss=99), dict(z=True, z_ns=9000)],
                         ids=["no_output", "reserved", "K_above_cap", "K0", "N0", "S0", "m_rs", "d_cs", "d_ns",
                              "d_ns_scalar", "mu_ns", "z_ss", "z_ns"])
def test_invalid_items_are_refused(kw):
    """CURV_ERR_INVALID with the item's index in the text, also behind valid items, before anything is launched."""
    L = _lib.lib()
    arr = desc(**kw)
    assert L.curv_head_mc_moments_workspace_bytes(arr, 1) == 0
    assert b"curv_head_mc_moments: item 0" in L.curv_last_error()
    assert L.curv_head_mc_moments_plan_flops(arr, 1, (ctypes.c_longlong * 1)()) == _lib.ERR_INVALID
    assert L.curv_head_mc_moments(None, arr, 1, None, 0) == _lib.ERR_INVALID
    assert b"item 0" in L.curv_last_error()
    three = (_lib.curv_head_moments_desc * 3)()
    for k, one in enumerate((desc(), desc(K=7, S=3), arr)):
        ctypes.memmove(ctypes.addressof(three[k]), one, ctypes.sizeof(_lib.curv_head_moments_desc))
    assert L.curv_head_mc_moments(None, three, 3, None, 0) == _lib.ERR_INVALID
    assert b"item 2" in L.curv_last_error()


@pytest.mark.parametrize("output", ["probs", "draws", "entropy", "probs_sq"])
def test_any_single_output_is_enough(output):
    L = _lib.lib()
    assert L.curv_head_mc_moments_plan_flops(desc(outputs=(output,)), 1, (ctypes.c_longlong * 1)()) == 0


def test_ops_refuses_cpu_tensors_and_wrong_shapes():
    M, d2, mu = torch.eye(3), torch.ones(2), torch.zeros(2, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.head_mc_moments([ops.HeadMomentsJob(M, d2, mu, 8, entropy=torch.zeros(2))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.head_mc_moments([ops.HeadMomentsJob(M, d2, mu, 8, probs_sq=torch.zeros(2, 3))])
    # the shape checks come after the device check, so they are met with tensors that claim to be on the GPU
    meta = dict(device="meta")

    class OnGpu(torch.Tensor):
        is_cuda = True

    def fake(*shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, **meta).as_subclass(OnGpu)
    good = dict(M=fake(3, 3), d2=fake(2), mu=fake(2, 3))
    for bad, text in ((dict(entropy=fake(2, 1)), r"head_mc_moments: entropy must be a contiguous \(2,\) tensor"),
                      (dict(probs_sq=fake(3, 2)), r"head_mc_moments: probs_sq must be a contiguous \(2, 3\) tensor"),
                      (dict(probs=fake(2, 4)), r"head_mc_moments: probs must be a contiguous \(2, 3\) tensor"),
                      (dict(draws=fake(2, 8, 4)), r"head_mc_moments: draws must be a contiguous \(2, 8, 3\) tensor"),
                      (dict(mu=fake(3, 3)), r"head_mc_moments: mu must be an \(2,3\) view"),
                      (dict(M=fake(3, 4)), r"head_mc_moments: M must be a \(3,3\) view"),
                      (dict(d2=fake(3)), r"head_mc_moments: d2 must be an \(2,\) or \(2,3\) view"),
                      (dict(noise=fake(2, 7, 3)), r"head_mc_moments: noise must be an \(2,8,3\) view"),
                      (dict(entropy=fake(2, dtype=torch.float64)), "expects float32")):
        kw = dict(good, entropy=fake(2))
        kw.update(bad)
        M_, d2_, mu_ = kw.pop("M"), kw.pop("d2"), kw.pop("mu")
        with pytest.raises(RuntimeError, match=text):
            ops.head_mc_moments([ops.HeadMomentsJob(M_, d2_, mu_, 8, N=2, K=3, **kw)])


def test_last_layer_uncertainty_refuses_a_cpu_model():
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3, padding=1), torch.nn.Flatten(), torch.nn.Linear(75, 4))
    x = torch.zeros(3, 2, 5, 5)
    with pytest.raises(RuntimeError, match="last_layer_uncertainty got a CPU model or batch .no CPU fallback"):
        evaluate.last_layer_uncertainty(model, KFAC(model), x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate.eval_uncertainty(model, [(x, torch.zeros(3, dtype=torch.long))], KFAC(model))
    with pytest.raises(ValueError, match="samples"):
        evaluate.last_layer_uncertainty(model, KFAC(model), x, samples=0)
