"""LayerNorm, GroupNorm and BatchNorm2d without a GPU: the switch, the selection, the refusals, what
KFAC.update hands the norm build (with every build of ops.FACTOR_BUILDS replaced by a recorder, as
tests/test_kfac_jobs_cpu.py does), the planner's view of such a layer, and the C ABI's new symbols."""
import copy
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from curvature_amd import _lib, ops, sharding
from curvature_amd.curvatures import EFB, INF, KFAC, BlockDiagonal, Diagonal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = tuple(build.accumulate for build in ops.FACTOR_BUILDS)
NORM_TYPES = ['LayerNorm', 'GroupNorm', 'BatchNorm2d']


class Net(nn.Module):
    """conv -> GroupNorm -> BatchNorm2d -> LayerNorm over the last two dims -> Linear; a (2, 3, 6, 6) batch gives 4 x 4 maps."""

    def __init__(self, ln_bias=True):
        super().__init__()
        self.conv = nn.Conv2d(3, 4, 3)
        self.gn = nn.GroupNorm(2, 4)
        self.bn = nn.BatchNorm2d(4)
        self.ln = nn.LayerNorm((4, 4), bias=ln_bias)
        self.fc = nn.Linear(64, 3)

    def forward(self, x):
        return self.fc(self.ln(self.bn(self.gn(self.conv(x)))).flatten(1))


@pytest.fixture
def on():
    was = ops.admit_norm_layers(True)
    yield
    ops.admit_norm_layers(was)


def test_switch_off_nothing_changes():
    assert not ops.norm_layers_admitted()
    model = Net().eval()
    for build in (lambda t: KFAC(model, t), lambda t: Diagonal(model, t), lambda t: BlockDiagonal(model, t),
                  lambda t: EFB(model, {}, t), lambda t: INF(model, {}, {}, {}, t)):
        for kind in NORM_TYPES:
            with pytest.raises(AssertionError):
                build([kind])
    assert ops.per_sample_route(nn.Conv2d(4, 4, 3, groups=4)) == "depthwise"
    assert ops.per_sample_route(nn.Conv2d(4, 8, 3, groups=2)) == "slices"
    assert ops.per_sample_route(nn.Conv2d(4, 8, 3)) == "whole" == ops.per_sample_route(nn.LayerNorm(4))
    with pytest.raises(NotImplementedError, match="admit_norm_layers"):
        ops.norm_view(nn.LayerNorm(4), ops.ShapeOnly((2, 4)), None)
    assert ops.admit_norm_layers(True) is False and ops.norm_layers_admitted()
    assert ops.admit_norm_layers(False) is True and not ops.norm_layers_admitted()


def test_selection_follows_modules_and_stays_out_of_the_default(on):
    model = Net().eval()
    est = KFAC(model, ['Linear', 'LayerNorm', 'Conv2d', 'GroupNorm', 'BatchNorm2d'])
    assert est._layers() == [model.conv, model.gn, model.bn, model.ln, model.fc]
    assert KFAC(model)._layers() == [model.conv, model.fc]
    assert Diagonal(model, ['GroupNorm'])._layers() == [model.gn]
    assert [ops.per_sample_route(l) for l in est._layers()] == ["whole", "norm", "norm", "norm", "whole"]


def test_views(on):
    model = Net().eval()
    view = ops.norm_view(model.ln, ops.ShapeOnly((2, 5, 3, 4, 4)), None)
    assert view.dims == (2, 16, 15, 1) and view.x_strides == (240, 1, 16, 1) and view.mode == _lib.NORM_POSITION
    assert view.g_strides is None and view.x_elems == 480
    x = torch.randn(2, 4, 4, 4).contiguous(memory_format=torch.channels_last)
    view = ops.norm_view(model.gn, x, x)
    assert view.dims == (2, 4, 4, 4) and view.x_strides == (64, 1, 16, 4) and (view.mode, view.groups) == (_lib.NORM_GROUP, 2)
    view = ops.norm_view(model.bn, x, None)
    assert view.mode == _lib.NORM_GIVEN and view.mean is not None and view.mean.data_ptr() == model.bn.running_mean.data_ptr()
    sides = ops.factor_jobs(nn.LayerNorm(8, bias=False), ops.ShapeOnly((3, 5, 8)), ops.ShapeOnly((3, 5, 8)))
    assert (sides.n, sides.m, sides.N, sides.L, sides.groups) == (1, 1, 3, 5, 8)
    assert sides.a.src == (3, 5, 8) and sides.a.side == _lib.NORM_SIDE_A and sides.g.side == _lib.NORM_SIDE_G
    assert not sides.a.has_bias and not sides.g.has_bias


def test_refusals_name_the_layer(on):
    model = Net().eval()
    x = torch.randn(2, 4, 4, 4)
    with pytest.raises(RuntimeError, match=r"GroupNorm.*float32.*float64"):
        ops.factor_jobs(model.gn, x.double(), x.double())
    with pytest.raises(RuntimeError, match=r"my_gn.*float32"):
        ops.PerSampleNormJob.of(model.gn, x.half(), x.half(), name="my_gn")
    # CPU records: refused where their addresses would go to the library
    sides = ops.factor_jobs(model.gn, x, x)
    sides.a.dst = torch.zeros(4, 2, 2)
    with pytest.raises(RuntimeError, match=r"CPU tensor.*GroupNorm"):
        ops.kfac_accumulate_norm([sides.a])
    with pytest.raises(RuntimeError, match=r"CPU tensor.*GroupNorm"):
        ops.per_sample_norm_sq_accumulate([ops.PerSampleNormJob.of(model.gn, x, x, dst=torch.zeros(4, 2))])
    # a LayerNorm record whose normalised dims are not contiguous
    with pytest.raises(RuntimeError, match=r"LayerNorm.*contiguous"):
        ops.factor_jobs(model.ln, x.transpose(2, 3), x)
    with pytest.raises(RuntimeError, match=r"LayerNorm.*collapse"):
        ops.factor_jobs(nn.LayerNorm(4), torch.randn(2, 3, 5, 4).transpose(1, 2), None)
    # batch statistics couple the samples
    model.bn.train()
    with pytest.raises(NotImplementedError, match=r"BatchNorm2d.*training mode.*model\.eval\(\)"):
        ops.factor_jobs(model.bn, x, x)
    est = KFAC(model, ['BatchNorm2d'])
    with pytest.raises(NotImplementedError, match=r"'bn'.*training mode.*model\.eval\(\)"):
        model(torch.randn(2, 3, 6, 6))
    for hook in est.hooks:
        hook.remove()
    with pytest.raises(NotImplementedError, match=r"track_running_stats.*model\.eval\(\)"):
        ops.factor_jobs(nn.BatchNorm2d(4, track_running_stats=False).eval(), x, x)
    model.bn.eval()
    # nothing to estimate
    bare = nn.Sequential(nn.LayerNorm(4, elementwise_affine=False), nn.GroupNorm(2, 4, affine=False))
    for kind, name in (('LayerNorm', "'0'"), ('GroupNorm', "'1'")):
        with pytest.raises(NotImplementedError, match=name + r".*no weight"):
            KFAC(bare, [kind])
        with pytest.raises(NotImplementedError, match=name + r".*no weight"):
            Diagonal(bare, [kind])
    # the estimators and forms that do not take them say who does
    for build in (lambda: EFB(model, {}, NORM_TYPES), lambda: INF(model, {}, {}, {}, NORM_TYPES),
                  lambda: BlockDiagonal(model, NORM_TYPES)):
        with pytest.raises(NotImplementedError, match=r"'gn'.*KFAC, or Diagonal, with functional_variance"):
            build()
    with pytest.raises(NotImplementedError, match=r"'gn'.*normalisation layer"):
        KFAC(model, NORM_TYPES, approximation="reduce")
    with pytest.raises(NotImplementedError, match="reduce"):
        ops.factor_jobs(model.gn, x, x, approximation="reduce")


@pytest.fixture
def calls(monkeypatch):
    seen = {name: [] for name in BUILDS + ("order",)}

    def recorder(name):
        def record(jobs, events=None):
            seen[name].append(list(jobs))
            seen["order"].append(name)
        return record
    for name in BUILDS:
        monkeypatch.setattr(ops, name, recorder(name))
    return seen


def _price_by_shape(monkeypatch):
    """The named plan_flops functions take CPU records: each prices stand-ins that carry the shapes (host only)."""
    for build in ops.FACTOR_BUILDS:
        def priced(jobs, real=getattr(ops, build.plan_flops)):
            stand_ins = [copy.copy(j) for j in jobs]
            for j in stand_ins:
                j.src = tuple(j.src.shape) if isinstance(j.src, torch.Tensor) else tuple(j.src)
            return real(stand_ins)
        monkeypatch.setattr(ops, build.plan_flops, priced)


@pytest.mark.parametrize("ln_bias", [True, False])
def test_kfac_hands_two_norm_jobs_per_layer(on, calls, monkeypatch, ln_bias):
    _price_by_shape(monkeypatch)
    torch.manual_seed(0)
    model = Net(ln_bias).eval()
    est = KFAC(model, NORM_TYPES)
    model(torch.randn(2, 3, 6, 6)).square().mean().backward()
    est._count_flops = True
    # per layer (modules() order: gn, bn, ln): C, n_g, N, L (the LayerNorm: 16 normalised values at 4 positions).  A: input_weight / (N L), G: N / L / grad_scale^2
    expected = [(model.gn, 4, 2, 2, 16), (model.bn, 4, 2, 2, 16), (model.ln, 16, 1 + int(ln_bias), 2, 4)]
    est.update(2)
    assert calls["order"] == list(BUILDS) and BUILDS[-1] == "kfac_accumulate_norm"
    assert all(not calls[name][-1] for name in BUILDS[:-1])
    jobs = calls["kfac_accumulate_norm"][-1]
    assert len(jobs) == 6 and all(type(j) is ops.NormFactorJob for j in jobs)
    for k, (layer, C, n_g, N, L) in enumerate(expected):
        a, g = jobs[2 * k], jobs[2 * k + 1]
        assert (a.side, g.side) == (_lib.NORM_SIDE_A, _lib.NORM_SIDE_G)
        assert a.dst is est.state[layer][0] and tuple(a.dst.shape) == (C, n_g, n_g)
        assert g.dst is est.state[layer][1] and tuple(g.dst.shape) == (C, 1, 1)
        assert a.src is est.record[layer][0].detach() or a.src.data_ptr() == est.record[layer][0].data_ptr()
        assert g.src.data_ptr() == est.record[layer][1].data_ptr()
        assert a.scale == 1.0 / (N * L) and g.scale == float(N) / L
        assert a.first is True and g.first is True
        assert a.view.dims == (N, C, L, 1) if layer is model.ln else a.view.dims == (N, C, 4, 4)
    assert est._last_flops > 0
    est.update(2, inputs=False, grad_scale=4.0)
    jobs = calls["kfac_accumulate_norm"][-1]
    assert [j.side for j in jobs] == [_lib.NORM_SIDE_G] * 3
    assert [j.scale for j in jobs] == [2.0 / 16 / 16, 2.0 / 16 / 16, 2.0 / 4 / 16] and not any(j.first for j in jobs)
    est.update(2, grads=False, input_weight=3.0)
    jobs = calls["kfac_accumulate_norm"][-1]
    assert [j.side for j in jobs] == [_lib.NORM_SIDE_A] * 3
    assert [j.scale for j in jobs] == [3.0 / 32, 3.0 / 32, 3.0 / 8] and not any(j.first for j in jobs)
    est.restart_accumulation()
    est.update(2)
    assert all(j.first for j in calls["kfac_accumulate_norm"][-1])
    for hook in est.hooks:
        hook.remove()


def test_layer_dims_of_a_norm_layer(on):
    model = Net().eval()
    shapes = {model.gn: ((2, 4, 4, 4), (2, 4, 4, 4)), model.ln: ((2, 4, 4, 4), (2, 4, 4, 4)),
              model.fc: ((2, 64), (2, 3))}
    dims = sharding.layer_dims([model.gn, model.ln, model.fc], shapes)
    assert dims[0][:3] == (2, 1, 32) and dims[0][3] > 0 and dims[0][4] == 4
    assert dims[1][:3] == (2, 1, 8) and dims[1][3] > 0 and dims[1][4] == 16
    assert len(dims[2]) == 4
    # the planner's figures: statistics 6 per element, A 2 + 2 n_g, G 2 (curv_kfac_norm_plan_flops)
    assert dims[0][3] == 128 * (6 + 2 + 4) + 128 * 2


def test_host_only_abi():
    header = open(os.path.join(ROOT, "include", "curv_hip.h")).read()
    declared = set(re.findall(r"\b(curv_(?:kfac|persample)_norm_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == {"curv_kfac_norm_workspace_bytes", "curv_kfac_norm_plan_flops", "curv_kfac_norm_accumulate",
                        "curv_persample_norm_workspace_bytes", "curv_persample_norm_plan_info",
                        "curv_persample_norm_sq_accumulate", "curv_persample_norm_quad_reduce"}
    handle = _lib.lib()
    assert all(name in _lib.SIGNATURES and hasattr(handle, name) for name in declared)
    for macro, value in (("CURV_NORM_GROUP", _lib.NORM_GROUP), ("CURV_NORM_POSITION", _lib.NORM_POSITION),
                         ("CURV_NORM_GIVEN", _lib.NORM_GIVEN), ("CURV_NORM_SIDE_A", _lib.NORM_SIDE_A),
                         ("CURV_NORM_SIDE_G", _lib.NORM_SIDE_G), ("CURV_NORM_SPLIT_L", _lib.NORM_SPLIT_L),
                         ("CURV_NORM_SLICE", _lib.NORM_SLICE)):
        assert re.search(rf"#define {macro} {value}\b", header), macro
    # empty calls are no-ops; an invalid descriptor names its item, host only
    assert handle.curv_kfac_norm_accumulate(None, None, 0, None, 0) == 0
    assert handle.curv_persample_norm_sq_accumulate(None, None, 0, None, 0) == 0
    assert handle.curv_persample_norm_quad_reduce(None, None, 0, None, 0) == 0
    arr = (_lib.curv_norm_desc * 2)()
    for d in arr:
        d.N, d.C, d.H, d.W, d.mode, d.groups, d.eps = 2, 6, 3, 3, _lib.NORM_GROUP, 3, 1e-5
        d.x_sn, d.x_sc, d.x_sh, d.x_sw, d.x_elems = 54, 9, 3, 1, 108
        d.g_sn, d.g_sc, d.g_sh, d.g_sw, d.g_elems = 54, 9, 3, 1, 108
    assert handle.curv_persample_norm_workspace_bytes(arr, 2) > 0
    assert handle.curv_kfac_norm_workspace_bytes(arr, 2) > 0
    for field, value, text in (("groups", 4, b"does not divide"), ("eps", 0.0, b"eps"), ("x_elems", 107, b"extent"),
                               ("reserved", 1, b"reserved"), ("mode", 3, b"mode"), ("x_sc", -1, b"negative")):
        bad = (_lib.curv_norm_desc * 2)()
        ctypes.memmove(bad, arr, ctypes.sizeof(arr))
        setattr(bad[1], field, value)
        assert handle.curv_persample_norm_workspace_bytes(bad, 2) == 0
        message = handle.curv_last_error()
        assert b"item 1" in message and text in message, message
    arr[0].side = 2
    assert handle.curv_kfac_norm_workspace_bytes(arr, 2) == 0 and b"item 0" in handle.curv_last_error()
