"""Grouped / depthwise convolutions without a GPU: which estimators accept them, the host-only queries of the grouped factor
build (curv_kfac_group_workspace_bytes / curv_kfac_group_plan_flops) and the sharding cost model."""
import ctypes

import pytest
import torch

from curvature_amd import _lib, models, ops, sharding
from curvature_amd.curvatures import EFB, INF, KFAC


def _grouped_model():
    return torch.nn.Sequential(torch.nn.Conv2d(8, 8, 3, padding=1), torch.nn.ReLU(),
                               torch.nn.Conv2d(8, 16, 3, padding=1, groups=8), torch.nn.ReLU(),
                               torch.nn.Conv2d(16, 16, 3, stride=2, padding=1, groups=4, bias=False))


def test_kfac_accepts_grouped_layers():
    m = _grouped_model()
    k = KFAC(m)
    assert len(k._layers()) == 3
    assert all(layer in k.record for layer in k._layers())
    for name in ("mobilenet_v2", "resnext50_32x4d"):
        KFAC(getattr(models, name)(num_classes=10))


def test_dilation_still_rejected():
    for groups in (1, 4):
        with pytest.raises(NotImplementedError, match="dilated"):
            KFAC(torch.nn.Sequential(torch.nn.Conv2d(4, 4, 3, dilation=2, groups=groups)))


def test_efb_and_inf_reject_grouped_layers():
    m = _grouped_model()
    with pytest.raises(NotImplementedError, match="'2'"):
        EFB(m, factors={}, eigvecs={})
    with pytest.raises(NotImplementedError, match="grouped convolution"):
        INF(m, diags={}, factors={}, lambdas={}, eigvecs={})
    EFB(_grouped_model(), factors={}, layer_types="Linear", eigvecs={})      # not selected: fine


def _desc(**kw):
    d = _lib.curv_group_factor_desc()
    geo = dict(N=2, C=16, H=9, W=9, groups=16, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, has_bias=0, first=1, scale=1.0)
    geo.update(kw)
    for k, v in geo.items():
        setattr(d, k, v)
    return d


def test_host_queries():
    L = _lib.lib()
    arr = (_lib.curv_group_factor_desc * 2)(_desc(), _desc(C=64, groups=2, has_bias=1))
    assert L.curv_kfac_group_workspace_bytes(arr, 2) > 0
    out = (ctypes.c_longlong * 2)()
    assert L.curv_kfac_group_plan_flops(arr, 2, out) == 0
    K = 2 * 9 * 9
    assert out[0] == 2 * (9 * 10 // 2 + 9) * K * 16              # depthwise: whole triangle + patch sums per thread
    # wide groups: what the ordinary build executes for each group's own convolution
    one = ops.kfac_plan_flops([ops.FactorJob((2, 32, 9, 9), None, (3, 3), (1, 1), (1, 1), True)])[0]
    assert out[1] == 2 * one > 0
    assert L.curv_kfac_group_accumulate(None, arr, 0, None, 0) == 0   # empty batch is a no-op
    # the Python helper takes shapes as well as tensors
    job = ops.GroupFactorJob((2, 16, 9, 9), None, 16, (3, 3), (1, 1), (1, 1))
    assert ops.kfac_group_plan_flops([job]) == [out[0]]


@pytest.mark.parametrize("bad", [dict(C=15), dict(groups=0), dict(kh=0), dict(H=1, ph=0), dict(sh=0)])
def test_invalid_geometry_returns_zero(bad):
    L = _lib.lib()
    arr = (_lib.curv_group_factor_desc * 1)(_desc(**bad))
    assert L.curv_kfac_group_workspace_bytes(arr, 1) == 0
    assert b"factor 0" in L.curv_last_error()
    out = (ctypes.c_longlong * 1)()
    assert L.curv_kfac_group_plan_flops(arr, 1, out) == _lib.ERR_INVALID


def test_sharding_layer_dims_of_grouped_layers():
    m = _grouped_model()
    layers = [l for l in m.modules() if isinstance(l, torch.nn.Conv2d)]
    shapes = {layers[0]: ((2, 8, 10, 10), (2, 8, 10, 10)),
              layers[1]: ((2, 8, 10, 10), (2, 16, 10, 10)),
              layers[2]: ((2, 16, 10, 10), (2, 16, 5, 5))}
    dims = sharding.layer_dims(layers, shapes)
    assert len(dims[0]) == 4
    assert dims[1][:3] == (1 * 9 + 1, 2, 200) and dims[1][4] == 8
    assert dims[2][:3] == (4 * 9, 4, 50) and dims[2][4] == 4
    assert all(d[3] > 0 for d in dims)
    # the cost of a grouped layer is the sum over its groups
    one = sharding.rank_cost([dims[2][:4]])
    assert sharding.rank_cost([dims[2]]) > one
    owner = sharding.partition_layers(dims, 2)
    assert sorted(set(owner)) == [0, 1]
