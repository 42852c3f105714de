"""Exact per-sample Fisher (``per_sample=True`` of Diagonal / EFB) without a GPU: construction, the recording hooks,
the rejected layer kinds, the host-only queries of the C ABI (curv_persample_*) and `compute_factors`."""
import ctypes
import inspect

import pytest
import torch

from curvature_amd import _lib, ops
from curvature_amd.curvatures import EFB, KFAC, Diagonal
from curvature_amd.factors import compute_factors


def lenet_like():
    return torch.nn.Sequential(
        torch.nn.Conv2d(1, 4, 5), torch.nn.ReLU(), torch.nn.MaxPool2d(2),
        torch.nn.Conv2d(4, 6, 3, padding=1, bias=False), torch.nn.ReLU(), torch.nn.Flatten(),
        torch.nn.Linear(6 * 12 * 12, 10))


def selected(model):
    return [l for l in model.modules() if l.__class__.__name__ in ("Linear", "Conv2d")]


def n_hooks(layer):
    return len(layer._forward_hooks) + len(layer._forward_pre_hooks)


@pytest.mark.parametrize("make", [lambda m: Diagonal(m, per_sample=True), lambda m: EFB(m, {}, eigvecs={}, per_sample=True)],
                         ids=["diagonal", "efb"])
def test_constructs_and_records(make):
    torch.manual_seed(0)
    model = lenet_like()
    est = make(model)
    assert est.per_sample
    x = torch.randn(3, 1, 28, 28)
    torch.nn.functional.cross_entropy(model(x), torch.tensor([1, 2, 3])).backward()
    for layer in selected(model):
        forward, backward = est.record[layer]
        assert forward is not None and backward is not None
        assert forward.shape[0] == backward.shape[0] == 3


def test_update_on_cpu_records_raises():
    torch.manual_seed(0)
    model = lenet_like()
    diag = Diagonal(model, per_sample=True)
    torch.nn.functional.cross_entropy(model(torch.randn(2, 1, 28, 28)), torch.tensor([1, 2])).backward()
    with pytest.raises(RuntimeError):
        diag.update(2)                                  # no CPU fallback
    assert not diag.state
    efb = EFB(model, {}, eigvecs={l: (None, None) for l in selected(model)}, per_sample=True)
    torch.nn.functional.cross_entropy(model(torch.randn(2, 1, 28, 28)), torch.tensor([1, 2])).backward()
    with pytest.raises(RuntimeError):
        efb.update(2)


def test_missing_record_raises():
    model = lenet_like()
    diag = Diagonal(model, per_sample=True)
    with pytest.raises(RuntimeError, match="no recorded forward/backward"):
        diag.update(1)


def test_default_registers_no_hook():
    model = lenet_like()
    Diagonal(model)
    EFB(model, {}, eigvecs={})
    Diagonal(model, per_sample=False)
    assert all(n_hooks(l) == 0 for l in selected(model))
    Diagonal(model, per_sample=True)
    assert all(n_hooks(l) == 2 for l in selected(model))
    assert "per_sample" in inspect.signature(Diagonal.__init__).parameters
    assert inspect.signature(Diagonal.__init__).parameters["per_sample"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(EFB.__init__).parameters["per_sample"].kind is inspect.Parameter.KEYWORD_ONLY


def test_kfac_hooks_unchanged():
    model = lenet_like()
    kfac = KFAC(model)
    assert all(n_hooks(l) == 2 for l in selected(model))
    assert set(kfac.record) == set(selected(model))


REJECTED = {
    "grouped": (lambda: torch.nn.Conv2d(4, 4, 3, groups=2), ["Conv2d"]),
    "dilated": (lambda: torch.nn.Conv2d(4, 4, 3, dilation=2), ["Conv2d"]),
    "convt": (lambda: torch.nn.ConvTranspose2d(4, 4, 2, stride=2), ["ConvTranspose2d"]),
    "mha": (lambda: torch.nn.MultiheadAttention(8, 2), ["MultiheadAttention"]),
}


@pytest.mark.parametrize("kind", sorted(REJECTED))
@pytest.mark.parametrize("est", ["diagonal", "efb"])
def test_rejected_layer_kinds(kind, est):
    make, types = REJECTED[kind]
    model = torch.nn.Sequential()
    model.add_module("odd_one", make())
    with pytest.raises(NotImplementedError, match="odd_one"):
        if est == "diagonal":
            Diagonal(model, types, per_sample=True)
        else:
            EFB(model, {}, types, eigvecs={}, per_sample=True)
    if est == "diagonal":
        Diagonal(model, types)                          # the default path still takes the layer


def test_half_precision_records_raise_at_update():
    model = torch.nn.Sequential(torch.nn.Linear(4, 3))
    diag = Diagonal(model, per_sample=True)
    layer = model[0]
    diag.record[layer] = [torch.zeros(2, 4, dtype=torch.bfloat16), torch.zeros(2, 3, dtype=torch.bfloat16)]
    with pytest.raises(RuntimeError, match="bfloat16"):
        diag.update(2)


def test_operands_geometry():
    """The step from (layer, x, g) to the operands of P_n: what is read in place, what is packed, and the strides."""
    conv = torch.nn.Conv2d(8, 16, 1, bias=False)
    s = ops.per_sample_operands(conv, torch.zeros(2, 8, 4, 4), torch.zeros(2, 16, 4, 4))
    assert (s.N, s.m, s.n, s.L) == (2, 16, 8, 16)
    assert s.g.pack is None and (s.g.ns, s.g.rs) == (16 * 16, 16)
    assert s.x.pack is None and (s.x.ns, s.x.rs) == (8 * 16, 16)
    conv = torch.nn.Conv2d(8, 16, 3, padding=1)
    s = ops.per_sample_operands(conv, torch.zeros(2, 8, 7, 7), torch.zeros(2, 16, 7, 7))
    assert (s.m, s.n, s.L) == (16, 73, 49)
    assert s.g.pack is not None and s.g.Lp == 52 and (s.g.ns, s.g.rs) == (16 * 52, 52)      # L = 49: zero tail
    assert s.x.pack is not None and s.x.floats == 2 * 73 * 52
    s = ops.per_sample_operands(conv, torch.zeros(2, 8, 7, 7), torch.zeros(2, 16, 7, 7), rows_outer=True, in_place=False)
    assert (s.g.ns, s.g.rs) == (52, 2 * 52) and (s.x.ns, s.x.rs) == (52, 2 * 52)
    lin = torch.nn.Linear(5, 3)
    s = ops.per_sample_operands(lin, torch.zeros(4, 7, 5), torch.zeros(4, 7, 3))
    assert (s.N, s.m, s.n, s.L) == (4, 3, 6, 7)
    assert s.x.pack.strides == (35, 1, 5, 1) and s.g.pack.strides == (21, 1, 3, 1)          # channels-last transposes
    s = ops.per_sample_operands(lin, torch.zeros(4, 5), torch.zeros(4, 3))
    assert (s.N, s.m, s.n, s.L) == (4, 3, 6, 1)
    with pytest.raises(RuntimeError, match="float16"):
        ops.per_sample_operands(lin, torch.zeros(4, 5, dtype=torch.float16), torch.zeros(4, 3, dtype=torch.float16))


def desc(S=3, M=70, Nc=200, L=49, a_rs=None, b_rs=None, c_rs=None):
    arr = (_lib.curv_persample_desc * 1)()
    d = arr[0]
    d.S, d.M, d.Nc, d.L = S, M, Nc, L
    d.a_rs, d.b_rs = L if a_rs is None else a_rs, L if b_rs is None else b_rs
    d.a_ns, d.b_ns = M * d.a_rs, Nc * d.b_rs
    d.c_rs = Nc if c_rs is None else c_rs
    d.alpha = 1.0
    return arr


def test_host_queries():
    L = _lib.lib()
    for kw in (dict(), dict(S=1, M=1, Nc=1, L=1), dict(S=32, M=512, Nc=4608, L=49), dict(S=32, M=64, Nc=147, L=12544)):
        arr = desc(**kw)
        d = arr[0]
        assert L.curv_persample_workspace_bytes(arr, 1) > 0
        out = (ctypes.c_longlong * 1)()
        assert L.curv_persample_plan_flops(arr, 1, out) == 0
        assert out[0] >= 2 * d.S * d.M * d.Nc * d.L
    for kw in (dict(L=0), dict(M=0), dict(Nc=0), dict(S=0), dict(a_rs=48), dict(b_rs=10), dict(c_rs=199)):
        arr = (_lib.curv_persample_desc * 2)()
        ctypes.memmove(ctypes.addressof(arr[0]), desc(), ctypes.sizeof(_lib.curv_persample_desc))
        ctypes.memmove(ctypes.addressof(arr[1]), desc(**kw), ctypes.sizeof(_lib.curv_persample_desc))
        assert L.curv_persample_workspace_bytes(arr, 2) == 0, kw
        assert b"item 1" in L.curv_last_error(), kw
        assert L.curv_persample_plan_flops(arr, 2, (ctypes.c_longlong * 2)()) == _lib.ERR_INVALID
    # operands whose extent does not fit 32-bit offsets are refused with a status, not an abort
    assert L.curv_persample_workspace_bytes(desc(S=64, M=4096, Nc=64, L=4096), 1) == 0
    assert b"32-bit" in L.curv_last_error()


def test_empty_batches_are_noops():
    L = _lib.lib()
    assert L.curv_persample_workspace_bytes(None, 0) == 0
    assert L.curv_persample_plan_flops(None, 0, None) == 0
    assert L.curv_persample_sq_accumulate(None, None, 0, None, 0) == 0
    assert L.curv_persample_pack(None, None, 0) == 0
    ops.per_sample_sq_accumulate([])
    ops.per_sample_pack([], [])
    assert ops.per_sample_plan_flops([]) == []


def pack_desc(**kw):
    arr = (_lib.curv_persample_pack_desc * 1)()
    d = arr[0]
    d.N, d.C, d.H, d.W, d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.Lp = 2, 3, 8, 8, 3, 3, 1, 1, 1, 1, 64
    for k, v in kw.items():
        setattr(d, k, v)
    return arr


@pytest.mark.parametrize("bad", [dict(kh=0), dict(sh=0), dict(kh=11, kw=11, ph=0, pw=0), dict(Lp=60), dict(Lp=66), dict(N=0)],
                         ids=["kh0", "sh0", "empty_output", "Lp_below_L", "Lp_not_x4", "N0"])
def test_invalid_pack_geometry_is_refused(bad):
    L = _lib.lib()
    assert L.curv_persample_pack(None, pack_desc(**bad), 1) == _lib.ERR_INVALID
    assert b"item 0" in L.curv_last_error() and b"null" not in L.curv_last_error()     # the geometry, not the addresses


def test_a_sample_of_2_to_the_32_values_is_too_large():
    big = pack_desc(N=1, C=1 << 16, H=1 << 8, W=1 << 8, kh=1, kw=1, ph=0, pw=0, Lp=1 << 16)
    L = _lib.lib()
    assert L.curv_persample_pack(None, big, 1) == _lib.ERR_INVALID
    assert b"curv_persample_pack: item 0: too large" in L.curv_last_error()


def test_compute_factors_accepts_per_sample():
    assert inspect.signature(compute_factors).parameters["per_sample"].default is False
    model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(16, 4))
    data = [(torch.randn(2, 1, 4, 4), torch.zeros(2, dtype=torch.long))]
    with pytest.raises(RuntimeError):                   # reaches Diagonal(per_sample=True).update on CPU records
        compute_factors(None, model, data, estimator="diag", per_sample=True, device=torch.device("cpu"))
    assert all(n_hooks(l) == 2 for l in selected(model))
    with pytest.raises(ValueError, match="per_sample"):
        compute_factors(None, model, data, estimator="kfac", per_sample=True, device=torch.device("cpu"))
