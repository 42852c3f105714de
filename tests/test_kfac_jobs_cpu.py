"""What KFAC.update hands the factor builds, without a GPU: update() does no device work before ops.accumulate_factors
calls the named build of every job class (ops.kfac_accumulate, _groups, _half, _convt, _dilated, _reduce, _conv3d - the
rows of ops.FACTOR_BUILDS), so with every one of those replaced by a recorder it runs on CPU tensors.  The expected values
below are written out by hand from the layer definitions and the update() contract (A: input_weight / (N L),
G: N / L / grad_scale^2)."""
import pytest
import torch
import torch.nn as nn

from curvature_amd import _lib, ops, sharding
from curvature_amd.curvatures import KFAC

BUILDS = tuple(build.accumulate for build in ops.FACTOR_BUILDS)
BUILD_OF = {build.job.__name__: build.accumulate for build in ops.FACTOR_BUILDS}
TYPES = ['Linear', 'Conv2d', 'ConvTranspose2d', 'MultiheadAttention']
F32, BF16 = torch.float32, torch.bfloat16


class Mixed(nn.Module):
    """conv (stride 2, padding 1) -> grouped conv -> ConvTranspose2d called with output_size= -> Linear on a 3-D input
    -> self-attention.  With a (2, 3, 9, 9) batch: 5x5 maps after conv, 10x10 after the transposed convolution (9x9
    without output_size), 2 x 2 = 4 tokens into the Linear and the attention."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 4, 3, stride=2, padding=1)
        self.gconv = nn.Conv2d(4, 8, 3, padding=1, groups=2, bias=False)
        self.up = nn.ConvTranspose2d(8, 2, 3, stride=2, padding=1)
        self.fc = nn.Linear(100, 6)
        self.mha = nn.MultiheadAttention(6, 2, batch_first=True)

    def forward(self, x):
        y = torch.relu(self.gconv(torch.relu(self.conv(x))))
        y = self.up(y, output_size=(10, 10))
        y = self.fc(y.flatten(2))                                     # (2, 2, 100) -> (2, 2, 6)
        return self.mha(y, y, y, need_weights=False)[0]


@pytest.fixture
def calls(monkeypatch):
    """Recorders in place of every build of ops.FACTOR_BUILDS and around ops.kfac_path_for: {name: [argument of each call]},
    the names of the builds in the order they were called under "order", and the launch forms kfac_path_for answered
    under "form"."""
    seen = {name: [] for name in BUILDS + ("kfac_path_for", "form", "order")}

    def recorder(name):
        def record(jobs, events=None):
            seen[name].append(list(jobs))
            seen["order"].append(name)
        return record
    for name in BUILDS:
        monkeypatch.setattr(ops, name, recorder(name))
    path_for = ops.kfac_path_for

    def recorded_path_for(factors):
        factors = list(factors)
        seen["kfac_path_for"].append(factors)
        seen["form"].append(path_for(factors))
        return seen["form"][-1]
    monkeypatch.setattr(ops, "kfac_path_for", recorded_path_for)
    return seen


def _estimator(autocast=False, shard=None):
    torch.manual_seed(0)
    model = Mixed()
    est = KFAC(model, TYPES, shard=shard)
    with torch.autocast("cpu", dtype=BF16, enabled=autocast):
        out = model(torch.randn(2, 3, 9, 9))
    out.float().square().mean().backward()
    return model, est


def _shape(src):
    return tuple(src.shape) if isinstance(src, torch.Tensor) else tuple(src)


def _geometry(job):
    """Every field of a job that does not depend on the call: class, source shape, kernel, stride, padding, has_bias,
    and groups / out_size where the class has them."""
    return (type(job).__name__, _shape(job.src), job.kernel, job.stride, job.padding, job.has_bias,
            getattr(job, "groups", None), getattr(job, "out_size", None))


def _last(calls):
    """The jobs of the latest update(): {build: [jobs]}."""
    return {name: calls[name][-1] for name in BUILDS}


ONE = ((1, 1), (1, 1), (0, 0))
# per layer (modules() order: conv, gconv, up, fc, attn_in, attn_out): (A geometry, A width, G geometry, G width, N, L)
EXPECTED = [
    (("FactorJob", (2, 3, 9, 9), (3, 3), (2, 2), (1, 1), True, None, None), (28, 28),
     ("FactorJob", (2, 4, 5, 5), *ONE, False, None, None), (4, 4), 2, 25),
    (("GroupFactorJob", (2, 4, 5, 5), (3, 3), (1, 1), (1, 1), False, 2, None), (2, 18, 18),
     ("GroupFactorJob", (2, 8, 5, 5), *ONE, False, 2, None), (2, 4, 4), 2, 25),
    (("ConvTFactorJob", (2, 8, 5, 5), (3, 3), (2, 2), (1, 1), True, None, (10, 10)), (73, 73),
     ("FactorJob", (2, 2, 10, 10), *ONE, False, None, None), (2, 2), 2, 100),
    (("FactorJob", (4, 100), *ONE, True, None, None), (101, 101),
     ("FactorJob", (4, 6), *ONE, False, None, None), (6, 6), 4, 1),
    (("FactorJob", (4, 6), *ONE, True, None, None), (7, 7),
     ("FactorJob", (4, 18), *ONE, False, None, None), (18, 18), 4, 1),
    (("FactorJob", (4, 6), *ONE, True, None, None), (7, 7),
     ("FactorJob", (4, 6), *ONE, False, None, None), (6, 6), 4, 1),
]


def _check(launched, est, layers, sides, a_scale, g_scale, first, half=()):
    """`launched` holds, in layer order with A before G, exactly the `sides` (0: A, 1: G) of EXPECTED with these
    scales and this `first`; `half`: the (layer index, side) pairs that go to the half-precision build instead."""
    want = {name: [] for name in BUILDS}
    for i, (a_geo, a_dst, g_geo, g_dst, N, L) in enumerate(EXPECTED):
        for side, geo, dst, scale_of in ((0, a_geo, a_dst, a_scale), (1, g_geo, g_dst, g_scale)):
            if side in sides:
                scale = scale_of(N, L)
                if (i, side) in half:
                    assert geo[0] == "FactorJob"
                    geo = ("HalfFactorJob",) + geo[1:]
                want[BUILD_OF[geo[0]]].append((geo, dst, scale, layers[i], side))
    for name in BUILDS:
        assert len(launched[name]) == len(want[name]), name
        for job, (geo, dst, scale, layer, side) in zip(launched[name], want[name]):
            assert _geometry(job) == geo
            assert job.dst is est.state[layer][side] and tuple(job.dst.shape) == dst
            assert job.scale == scale
            assert job.first is first
            assert job.src.is_contiguous()


def test_layers_and_out_size():
    model, est = _estimator()
    layers = est._layers()
    assert layers[:4] == [model.conv, model.gconv, model.up, model.fc]
    assert [l.kind for l in layers[4:]] == ['attn_in', 'attn_out'] and all(l.module is model.mha for l in layers[4:])
    assert est._out_size == {model.up: (10, 10)}
    assert tuple(est.record[model.fc][0].shape) == (2, 2, 100)       # recorded 3-D, flattened by the job


def test_fp32_jobs_scales_and_first(calls):
    _, est = _estimator()
    layers = est._layers()
    both = (0, 1)
    est.update(2)
    _check(_last(calls), est, layers, both, lambda N, L: 1.0 / (N * L), lambda N, L: float(N) / L, True)
    assert all(j.src.dtype == F32 for name in BUILDS for j in calls[name][-1])
    assert all(j.path_hint == 0 for j in calls["kfac_accumulate"][-1])          # unsharded: the library decides
    assert not calls["kfac_path_for"]
    est.update(2)
    _check(_last(calls), est, layers, both, lambda N, L: 1.0 / (N * L), lambda N, L: float(N) / L, False)
    est.update(2, inputs=False, grad_scale=4.0)
    _check(_last(calls), est, layers, (1,), None, lambda N, L: float(N) / L / 16.0, False)
    est.update(2, grads=False, input_weight=3.0)
    _check(_last(calls), est, layers, (0,), lambda N, L: 3.0 / (N * L), None, False)
    est.restart_accumulation()
    est.update(2, grads=False)
    _check(_last(calls), est, layers, (0,), lambda N, L: 1.0 / (N * L), None, True)
    est.update(2)                                                               # A written since, G not yet
    launched = _last(calls)
    for name in BUILDS:
        for job in launched[name]:
            side = [s for l in layers for s in (0, 1) if est.state[l][s] is job.dst][0]
            assert job.first is (side == 1)


def test_one_sided_first_update_starts_from_zero(calls):
    _, est = _estimator()
    est.update(2, inputs=False)
    for layer in est._layers():
        assert all(not f.any() for f in est.state[layer])
    assert all(not j.first for name in BUILDS for j in calls[name][-1])
    with pytest.raises(ValueError):
        est.update(2, grad_scale=0.0)


def test_bf16_autocast_routing(calls):
    model, est = _estimator(autocast=True)
    layers = est._layers()
    # what autocast hands the hooks: the first layer's input is the fp32 batch, every other recorded tensor is bf16
    dtypes = [(est.record[l][0].dtype, est.record[l][1].dtype) for l in layers]
    assert dtypes == [(F32, BF16)] + [(BF16, BF16)] * 5
    est.update(2)
    # ordinary sides go by their recorded dtype; grouped sides and the transposed convolution's A side are fp32 copies
    half = {(0, 1), (2, 1), (3, 0), (3, 1), (4, 0), (4, 1), (5, 0), (5, 1)}
    _check(_last(calls), est, layers, (0, 1), lambda N, L: 1.0 / (N * L), lambda N, L: float(N) / L, True, half)
    assert [j.src.dtype for j in calls["kfac_accumulate"][-1]] == [F32]
    assert all(j.src.dtype == BF16 and j.dtype == BF16 for j in calls["kfac_accumulate_half"][-1])
    assert all(j.src.dtype == F32 for j in calls["kfac_accumulate_groups"][-1] + calls["kfac_accumulate_convt"][-1])
    est.record[model.fc][0] = est.record[model.fc][0].double()
    with pytest.raises(RuntimeError, match="float32, bfloat16 or float16"):
        est.update(2)


def test_out_size_fallbacks():
    up = nn.ConvTranspose2d(8, 2, 3, stride=2, padding=1, output_padding=1)
    x, g = ops.ShapeOnly((2, 8, 5, 5)), ops.ShapeOnly((2, 2, 7, 9))
    assert ops.factor_jobs(up, x, g, out_size=(3, 3)).a.out_size == (7, 9)      # the gradient's own size first
    assert ops.factor_jobs(up, x, None, out_size=(11, 11)).a.out_size == (11, 11)   # then what the forward produced
    sides = ops.factor_jobs(up, x, None)                                        # then the layer's own output_padding
    assert sides.a.out_size == (10, 10) and sides.g is None
    assert (sides.n, sides.m, sides.N, sides.L, sides.K, sides.groups) == (73, 2, 2, 100, 200, 1)
    assert sides.a.src == (2, 8, 5, 5)                                          # a stand-in leaves its shape
    conv = nn.Conv2d(3, 4, 3, stride=2, padding=1)
    sides = ops.factor_jobs(conv, ops.ShapeOnly((2, 3, 9, 9)), None)           # L from the input when there is no g
    assert (sides.n, sides.m, sides.N, sides.L) == (28, 4, 2, 25)
    with pytest.raises(RuntimeError):
        ops.factor_jobs(conv, None, None)


@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("kwargs", [dict(), dict(inputs=False, grad_scale=4.0), dict(grads=False, input_weight=3.0)])
def test_shard_path_hint_describes_the_unsharded_fp32_launch(calls, autocast, kwargs):
    _, whole = _estimator(autocast)
    whole.update(2, **kwargs)
    unsharded = calls["kfac_accumulate"][-1]
    owner = [0, 1, 0, 1, 0, 1]
    _, est = _estimator(autocast, shard=sharding.Shard(owner, 1, 2))
    est.update(2, **kwargs)
    assert len(calls["kfac_path_for"]) == 1
    hinted = calls["kfac_path_for"][0]
    assert all(type(j) is ops.FactorJob for j in hinted)
    assert [_geometry(j) for j in hinted] == [_geometry(j) for j in unsharded]
    # fp32: every side but the grouped layer's two and the transposed convolution's A; bf16: the first layer's input only
    sides = (0,) if "grads" in kwargs else (1,) if "inputs" in kwargs else (0, 1)
    fp32 = [(0, 0)] if autocast else [(i, s) for i in (0, 2, 3, 4, 5) for s in (0, 1) if (i, s) != (2, 0)]
    assert [_geometry(j) for j in hinted] == [EXPECTED[i][2 * s] for i, s in fp32 if s in sides]
    # this rank launches its own layers only, every fp32 job under the form of the whole model
    layers = est._layers()
    mine = {id(f) for i, l in enumerate(layers) if owner[i] == 1 for f in est.state.get(l, ())}
    assert set(est.state) == {l for i, l in enumerate(layers) if owner[i] == 1}
    launched = [j for name in BUILDS for j in calls[name][-1]]
    assert launched and all(id(j.dst) in mine for j in launched)
    assert calls["form"][0] in (_lib.PATH_SMALL, _lib.PATH_GROUPED)
    assert all(job.path_hint == calls["form"][0] for job in calls["kfac_accumulate"][-1])
    est.update(2, **kwargs)                                             # same records: same form
    assert all(job.path_hint == calls["form"][0] for job in calls["kfac_accumulate"][-1])


class Kinds(nn.Module):
    """The kinds Mixed does not hold: a dilated Conv2d (stride 1, padding = dilation), a Conv1d on one row of its output
    and a Conv3d on the batch seen as one channel of depth 3.  With a (2, 3, 9, 9) batch every map stays 9 wide."""

    def __init__(self):
        super().__init__()
        self.dil = nn.Conv2d(3, 4, 3, padding=2, dilation=2)
        self.c1 = nn.Conv1d(4, 5, 3, padding=1)
        self.c3 = nn.Conv3d(1, 3, (2, 3, 3), padding=(0, 1, 1), bias=False)

    def forward(self, x):
        z = self.c1(self.dil(x)[:, :, 0, :])                          # (2, 4, 9) -> (2, 5, 9)
        return z.mean() + self.c3(x.unsqueeze(1)).mean()              # (2, 1, 3, 9, 9) -> (2, 3, 2, 9, 9)


class Tokens(nn.Module):
    """A Conv2d and a Linear fed 3-D records, for approximation="reduce": 36 tokens of 9 features from a (2, 3, 9, 9) batch."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 4, 3, padding=1)
        self.fc = nn.Linear(9, 2)

    def forward(self, x):
        return self.fc(self.conv(x).flatten(1, 2))                    # (2, 36, 9) -> (2, 36, 2)


# per build, in table order: (job class, layer, side, source shape, factor shape, scale) of every job, in launch order.
# Kinds: L = 81 (dil), 9 (c1), 2 x 9 x 9 = 162 (c3); A: 1 / (N L), G: N / L.
KINDS_EXPECTED = [
    ("kfac_accumulate", [("FactorJob", "dil", 1, (2, 4, 9, 9), (4, 4), 2.0 / 81),
                         ("FactorJob", "c1", 0, (2, 4, 1, 9), (13, 13), 1.0 / 18),
                         ("FactorJob", "c1", 1, (2, 5, 1, 9), (5, 5), 2.0 / 9),
                         ("FactorJob", "c3", 1, (2, 3, 18, 9), (3, 3), 2.0 / 162)]),
    ("kfac_accumulate_dilated", [("DilatedFactorJob", "dil", 0, (2, 3, 9, 9), (28, 28), 1.0 / 162)]),
    ("kfac_accumulate_conv3d", [("Conv3dFactorJob", "c3", 0, (2, 1, 3, 9, 9), (18, 18), 1.0 / 324)]),
]
# Tokens under "reduce": the positions are reduced first, so L = 1 in both scales: A 1 / N, G N.
TOKENS_EXPECTED = [
    ("kfac_accumulate_reduce", [("ReduceFactorJob", "conv", 0, (2, 3, 9, 9), (28, 28), 0.5),
                                ("ReduceFactorJob", "conv", 1, (2, 4, 9, 9), (4, 4), 2.0),
                                ("ReduceFactorJob", "fc", 0, (2, 36, 9), (10, 10), 0.5),
                                ("ReduceFactorJob", "fc", 1, (2, 36, 2), (2, 2), 2.0)]),
]


def _price_by_shape(monkeypatch):
    """The named plan_flops functions take CPU records: each prices stand-ins that carry the shapes (host only)."""
    import copy
    for build in ops.FACTOR_BUILDS:
        def priced(jobs, real=getattr(ops, build.plan_flops)):
            stand_ins = [copy.copy(j) for j in jobs]
            for j in stand_ins:
                j.src = _shape(j.src)
            return real(stand_ins)
        monkeypatch.setattr(ops, build.plan_flops, priced)


@pytest.mark.parametrize("net, types, approximation, expected", [
    (Kinds, ['Conv2d', 'Conv1d', 'Conv3d'], "expand", KINDS_EXPECTED),
    (Tokens, ['Linear', 'Conv2d'], "reduce", TOKENS_EXPECTED)], ids=["expand", "reduce"])
def test_every_other_kind_goes_through_the_table(calls, monkeypatch, net, types, approximation, expected):
    _price_by_shape(monkeypatch)
    was = ops.admit_dilated(True), ops.admit_conv_nd(True)
    try:
        torch.manual_seed(0)
        model = net()
        est = KFAC(model, types, approximation=approximation)
        model(torch.randn(2, 3, 9, 9)).square().mean().backward()
        est._count_flops = True
        for first in (True, False):
            calls["order"].clear()
            est.update(2)
            assert calls["order"] == list(BUILDS)                               # table order, one call per class
            launched = _last(calls)
            assert [name for name in BUILDS if launched[name]] == [name for name, _ in expected]
            flops = 0
            for name, jobs in expected:
                assert len(launched[name]) == len(jobs)
                for job, (cls, layer, side, src, dst, scale) in zip(launched[name], jobs):
                    assert type(job).__name__ == cls and BUILD_OF[cls] == name
                    assert _shape(job.src) == src and job.src.is_contiguous()
                    assert job.dst is est.state[getattr(model, layer)][side] and tuple(job.dst.shape) == dst
                    assert job.scale == scale
                    assert job.first is first
                build = [b for b in ops.FACTOR_BUILDS if b.accumulate == name][0]
                flops += sum(getattr(ops, build.plan_flops)(launched[name]))
            assert flops > 0 and est._last_flops == flops
    finally:
        ops.admit_dilated(was[0])
        ops.admit_conv_nd(was[1])


def test_accumulate_factors_refuses_what_is_not_a_job(calls):
    job = ops.FactorJob((2, 3), None)
    with pytest.raises(TypeError, match="object"):
        ops.accumulate_factors([job, object()])
    assert calls["order"] == []                                                 # refused before any build is called
    assert ops.factor_plan_flops([]) == []
    with pytest.raises(TypeError, match="str"):
        ops.factor_plan_flops([job, "job"])
