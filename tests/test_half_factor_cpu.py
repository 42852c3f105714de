"""Host-only checks of the bf16 / fp16 factor build's C ABI (curv_kfac16_*, ABI 12): plan queries, error text, empty calls."""
import ctypes

import pytest
import torch

from curvature_amd import _lib, ops


def _desc(N=2, C=8, H=5, W=5, k=3, s=1, p=1, bias=1, dtype=_lib.DTYPE_BF16):
    arr = (_lib.curv_factor16_desc * 1)()
    d = arr[0]
    d.N, d.C, d.H, d.W = N, C, H, W
    d.kh = d.kw = k
    d.sh = d.sw = s
    d.ph = d.pw = p
    d.has_bias, d.first, d.scale, d.dtype = bias, 1, 1.0, dtype
    return arr


def test_abi_version_is_12():
    assert _lib.ABI_VERSION == 12
    assert _lib.lib().curv_version() == 12


@pytest.mark.parametrize("field,value", [("N", 0), ("C", -1), ("kh", 0), ("sw", 0), ("ph", -1), ("H", 1)])
def test_invalid_geometry_needs_no_workspace(field, value):
    arr = _desc()
    setattr(arr[0], field, value)
    if field == "H":                         # 3x3 kernel on a 1-row input without padding
        arr[0].ph = 0
    L = _lib.lib()
    assert L.curv_kfac16_workspace_bytes(arr, 1) == 0
    assert b"factor 0" in L.curv_last_error()


@pytest.mark.parametrize("dtype", [0, 3, -1])
def test_unknown_dtype_is_rejected(dtype):
    L = _lib.lib()
    arr = _desc(dtype=dtype)
    assert L.curv_kfac16_workspace_bytes(arr, 1) == 0
    assert b"dtype" in L.curv_last_error()
    out = (ctypes.c_longlong * 1)()
    assert L.curv_kfac16_plan_flops(arr, 1, out) == _lib.ERR_INVALID


@pytest.mark.parametrize("geom", [
    dict(N=2, C=3, H=7, W=7, k=7, s=2, p=3, bias=0),           # stem-like
    dict(N=4, C=64, H=14, W=14, k=3, s=1, p=1, bias=1),
    dict(N=3, C=129, H=7, W=7, k=1, s=1, p=0, bias=0),
    dict(N=100000, C=5, H=1, W=1, k=1, s=1, p=0, bias=1),      # Linear, K = 10^5
    dict(N=1, C=256, H=1, W=1, k=1, s=1, p=0, bias=1),         # dim 257
])
@pytest.mark.parametrize("dtype", [_lib.DTYPE_BF16, _lib.DTYPE_F16])
def test_plan_flops_cover_the_symmetric_product(geom, dtype):
    L = _lib.lib()
    arr = _desc(dtype=dtype, **geom)
    out = (ctypes.c_longlong * 1)()
    assert L.curv_kfac16_plan_flops(arr, 1, out) == 0
    g = geom
    Ho = (g["H"] + 2 * g["p"] - g["k"]) // g["s"] + 1
    Wo = (g["W"] + 2 * g["p"] - g["k"]) // g["s"] + 1
    K = g["N"] * Ho * Wo
    dim = g["C"] * g["k"] ** 2 + g["bias"]
    assert out[0] >= dim * (dim + 1) * K
    assert L.curv_kfac16_workspace_bytes(arr, 1) >= 2 * dim * K        # at least the packed image


def test_plan_is_per_factor():
    """A factor's flops and plan do not depend on the other factors of the call."""
    L = _lib.lib()
    a, b = _desc(C=64), _desc(N=8, C=3, H=32, W=32, k=7, s=2, p=3, dtype=_lib.DTYPE_F16)
    both = (_lib.curv_factor16_desc * 2)(a[0], b[0])
    out1, out2 = (ctypes.c_longlong * 1)(), (ctypes.c_longlong * 2)()
    assert L.curv_kfac16_plan_flops(a, 1, out1) == 0
    assert L.curv_kfac16_plan_flops(both, 2, out2) == 0
    assert out2[0] == out1[0]
    assert L.curv_kfac16_workspace_bytes(both, 2) == L.curv_kfac16_workspace_bytes(a, 1) + \
        L.curv_kfac16_workspace_bytes(b, 1)


def test_empty_call_is_a_no_op():
    L = _lib.lib()
    assert L.curv_kfac16_accumulate(None, None, 0, None, 0) == 0
    assert L.curv_kfac16_plan_flops(None, 0, None) == 0
    ops.kfac_accumulate_half([])
    assert ops.kfac_half_plan_flops([]) == []


def test_null_arguments_are_errors():
    L = _lib.lib()
    arr = _desc()
    assert L.curv_kfac16_accumulate(None, arr, 1, None, 0) == _lib.ERR_INVALID       # src / dst null
    assert b"null" in L.curv_last_error()


def test_python_plan_query_from_shapes():
    jobs = [ops.HalfFactorJob((2, 8, 5, 5), None, (3, 3), (1, 1), (1, 1), True, dtype=torch.bfloat16),
            ops.HalfFactorJob((6, 129), None, dtype=torch.float16)]
    flops = ops.kfac_half_plan_flops(jobs)
    assert flops[0] >= 73 * 74 * 50 and flops[1] >= 129 * 130 * 6
    with pytest.raises(RuntimeError, match="bfloat16 or float16"):
        ops.kfac_half_plan_flops([ops.HalfFactorJob((2, 3), None, dtype=torch.float64)])


def test_cpu_tensors_are_refused():
    x = torch.randn(4, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.kfac_accumulate_half([ops.HalfFactorJob(x, torch.zeros(8, 8))])
