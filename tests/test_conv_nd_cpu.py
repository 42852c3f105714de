"""Conv1d and Conv3d without a GPU: the `ops.admit_conv_nd` switch (off: every selection and refusal as before), the
construction-time refusals, the routing of `factor_jobs`, the host-only entry points of csrc/conv3d_factor.hip, the ABI,
the shard planner - and the identity the Conv3d build rests on, in float64 torch: the 2-D im2col of the
depth-unfolded stack is the 3-D im2col, column for column, in the row order of ``weight.reshape(Cout, -1)``."""
import ctypes
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from curvature_amd import _lib, ops, sharding
from curvature_amd import curvatures
from curvature_amd.curvatures import KFAC, Diagonal


@pytest.fixture
def admitted():
    was = ops.admit_conv_nd(True)
    yield
    ops.admit_conv_nd(was)


def triple(v):
    return (v, v, v) if isinstance(v, int) else tuple(v)


def model3d():
    return torch.nn.Sequential(torch.nn.Conv3d(2, 4, 3, padding=1), torch.nn.ReLU(),
                               torch.nn.Conv3d(4, 4, (1, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1)), torch.nn.Flatten(),
                               torch.nn.Linear(4 * 4 * 3 * 3, 5))


def model1d():
    return torch.nn.Sequential(torch.nn.Conv1d(3, 8, 5, padding=2), torch.nn.ReLU(), torch.nn.Conv1d(8, 8, 3, stride=2),
                               torch.nn.Flatten(), torch.nn.Linear(8 * 15, 5))


# ------------------------------------------------------------------------------------------------ the switch
def test_switch_is_off_by_default_and_returns_what_it_was():
    assert ops.conv_nd_admitted() is False
    assert ops.admit_conv_nd(True) is False
    assert ops.conv_nd_admitted() is True
    assert ops.admit_conv_nd(True) is True
    assert ops.admit_conv_nd(False) is True
    assert ops.admit_conv_nd(False) is False
    assert ops.conv_nd_admitted() is False


def test_switch_off_refuses_both_kinds_as_before():
    assert ops.conv_nd_admitted() is False
    for model, kind in ((model3d(), 'Conv3d'), (model1d(), 'Conv1d')):
        with pytest.raises(AssertionError):
            KFAC(model, [kind])
        with pytest.raises(AssertionError):
            Diagonal(model, [kind])


def test_selection_by_name_with_the_switch_on(admitted):
    assert curvatures.SUPPORTED_LAYERS == ['Linear', 'Conv2d', 'MultiheadAttention']
    assert curvatures.OPTIONAL_LAYERS == ['ConvTranspose2d']
    for model, kind in ((model3d(), 'Conv3d'), (model1d(), 'Conv1d')):
        assert KFAC(model)._layers() == [model[4]]                               # the default selection is what it was
        assert Diagonal(model)._layers() == [model[4]]
        assert KFAC(model, [kind])._layers() == [model[0], model[2]]
        # modules() order, whatever the order of the names
        assert KFAC(model, ['Linear', kind])._layers() == [model[0], model[2], model[4]]
        assert Diagonal(model, [kind, 'Linear'])._layers() == [model[0], model[2], model[4]]
    mixed = torch.nn.Sequential(torch.nn.Conv3d(1, 2, 1), torch.nn.Conv1d(1, 2, 1), torch.nn.Conv2d(1, 2, 1),
                                torch.nn.Conv3d(2, 2, 1))
    assert KFAC(mixed, ['Conv1d', 'Conv2d', 'Conv3d'])._layers() == list(mixed)
    assert list(KFAC(mixed, ['Conv1d', 'Conv2d', 'Conv3d'])._global_index()) == list(mixed)


# ------------------------------------------------------------------------------------------------ refusals
REFUSALS = [
    ("grouped Conv1d", lambda: torch.nn.Conv1d(4, 4, 3, groups=2), "groups=2"),
    ("grouped Conv3d", lambda: torch.nn.Conv3d(4, 4, 3, groups=4), "groups=4"),
    ("dilated Conv3d", lambda: torch.nn.Conv3d(2, 4, 3, dilation=(1, 2, 2)), r"dilat.*\(1, 2, 2\)"),
    ("dilated Conv1d", lambda: torch.nn.Conv1d(2, 4, 3, dilation=2), r"dilat.*admit_dilated"),
    ("string padding 1d", lambda: torch.nn.Conv1d(2, 4, 3, padding='same'), "string padding"),
    ("string padding 3d", lambda: torch.nn.Conv3d(2, 4, 3, padding='same'), "string padding"),
    ("circular 1d", lambda: torch.nn.Conv1d(2, 4, 3, padding=1, padding_mode='circular'), "padding_mode='circular'"),
    ("circular 3d", lambda: torch.nn.Conv3d(2, 4, 3, padding=1, padding_mode='circular'), "padding_mode='circular'"),
]


@pytest.mark.parametrize("make, cause", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
@pytest.mark.parametrize("estimator", [KFAC, Diagonal])
def test_refusals_name_the_layer_and_the_cause(admitted, estimator, make, cause):
    layer = make()
    model = torch.nn.Sequential()
    model.add_module("stem", torch.nn.Sequential())
    model.stem.add_module("conv", layer)
    with pytest.raises(NotImplementedError) as err:
        estimator(model, [layer.__class__.__name__])
    text = str(err.value)
    assert "'stem.conv'" in text and re.search(cause, text), text


def test_dilated_conv1d_follows_the_rule_of_the_dilated_build(admitted):
    was = ops.admit_dilated(True)
    try:
        good = torch.nn.Sequential(torch.nn.Conv1d(2, 4, 3, dilation=2, padding=2))
        assert KFAC(good, ['Conv1d'])._layers() == [good[0]]
        sides = ops.factor_jobs(good[0], ops.ShapeOnly((4, 2, 16)), ops.ShapeOnly((4, 4, 16)))
        assert type(sides.a) is ops.DilatedFactorJob and sides.a.dilation == (1, 2) and sides.a.src == (4, 2, 1, 16)
        assert sides.a.kernel == (1, 3) and sides.a.padding == (0, 2) and (sides.n, sides.m, sides.L) == (7, 4, 16)
        assert ops.kfac_dilated_plan_flops([sides.a])[0] > 0                     # the library takes the view's geometry
        for bad in (torch.nn.Conv1d(2, 4, 3, dilation=2, padding=1), torch.nn.Conv1d(2, 4, 3, dilation=2, padding=2, stride=2)):
            with pytest.raises(NotImplementedError, match="'0'.*stride 1 and a padding that is a multiple"):
                KFAC(torch.nn.Sequential(bad), ['Conv1d'])
            Diagonal(torch.nn.Sequential(bad), ['Conv1d'], per_sample=True)      # the per-sample line has no such rule
        with pytest.raises(NotImplementedError, match="'0'.*dilated Conv3d"):     # ... and a Conv3d stays refused
            KFAC(torch.nn.Sequential(torch.nn.Conv3d(2, 4, 3, dilation=2)), ['Conv3d'])
    finally:
        ops.admit_dilated(was)


def test_conv3d_is_refused_by_reduce_and_by_the_per_sample_line(admitted):
    model = model3d()
    with pytest.raises(NotImplementedError) as err:
        KFAC(model, ['Conv3d', 'Linear'], approximation="reduce")
    assert "'0'" in str(err.value) and "a 3-D convolution" in str(err.value)
    assert 'approximation="expand" takes it' in str(err.value)
    with pytest.raises(NotImplementedError, match="3-D convolution"):
        ops.factor_jobs(model[0], ops.ShapeOnly((4, 2, 4, 6, 6)), None, approximation="reduce")
    with pytest.raises(NotImplementedError) as err:
        Diagonal(model, ['Conv3d'], per_sample=True)
    text = str(err.value)
    assert "'0'" in text and "3-D convolution" in text and all(k in text for k in ("KFAC", "Diagonal", "EFB", "INF"))
    with pytest.raises(NotImplementedError, match="unsupported layer Conv3d"):
        ops.per_sample_operands(model[0], torch.zeros(1, 2, 4, 6, 6), torch.zeros(1, 4, 4, 6, 6))
    # a Conv1d passes both
    one = model1d()
    assert KFAC(one, ['Conv1d', 'Linear'], approximation="reduce")._layers() == [one[0], one[2], one[4]]
    assert len(Diagonal(one, ['Conv1d', 'Linear'], per_sample=True).record) == 3


# ------------------------------------------------------------------------------------------------ factor_jobs
def test_factor_jobs_routes_a_conv3d(admitted):
    model = model3d()
    sides = ops.factor_jobs(model[0], ops.ShapeOnly((4, 2, 4, 6, 6)), ops.ShapeOnly((4, 4, 4, 6, 6)))
    assert (type(sides.a), type(sides.g)) == (ops.Conv3dFactorJob, ops.FactorJob)
    assert (sides.n, sides.m, sides.N, sides.L, sides.groups) == (2 * 27 + 1, 4, 4, 4 * 6 * 6, 1)
    assert sides.a.src == (4, 2, 4, 6, 6) and sides.a.kernel == (3, 3, 3) and sides.a.padding == (1, 1, 1)
    assert sides.a.has_bias and sides.a.stack_shape == (16, 6, 6, 6)
    assert sides.g.src == (4, 4, 24, 6) and sides.g.kernel == (1, 1) and not sides.g.has_bias
    sides = ops.factor_jobs(model[2], ops.ShapeOnly((4, 4, 4, 6, 6)), ops.ShapeOnly((4, 4, 4, 3, 3), torch.bfloat16))
    assert (type(sides.a), type(sides.g)) == (ops.Conv3dFactorJob, ops.HalfFactorJob)
    assert (sides.n, sides.m, sides.N, sides.L) == (4 * 9 + 1, 4, 4, 4 * 3 * 3)
    assert sides.a.stride == (1, 2, 2) and sides.a.padding == (0, 1, 1) and sides.g.dtype == torch.bfloat16
    # one side alone: L from the geometry
    alone = ops.factor_jobs(model[2], ops.ShapeOnly((4, 4, 4, 6, 6), torch.bfloat16), None)
    assert alone.g is None and alone.L == 36 and type(alone.a) is ops.Conv3dFactorJob            # the A side is float32
    with pytest.raises(RuntimeError, match=r"\(N, C, D, H, W\)"):
        ops.factor_jobs(model[0], ops.ShapeOnly((4, 2, 6, 6)), None)


def test_factor_jobs_routes_a_conv1d_through_its_2d_view(admitted):
    model = model1d()
    sides = ops.factor_jobs(model[0], ops.ShapeOnly((6, 3, 32)), ops.ShapeOnly((6, 8, 32)))
    assert (type(sides.a), type(sides.g)) == (ops.FactorJob, ops.FactorJob)
    assert sides.a.src == (6, 3, 1, 32) and (sides.a.kernel, sides.a.stride, sides.a.padding) == ((1, 5), (1, 1), (0, 2))
    assert sides.g.src == (6, 8, 1, 32)
    assert (sides.n, sides.m, sides.N, sides.L, sides.groups) == (16, 8, 6, 32, 1)
    sides = ops.factor_jobs(model[2], ops.ShapeOnly((6, 8, 32), torch.bfloat16), ops.ShapeOnly((6, 8, 15), torch.float16))
    assert (type(sides.a), type(sides.g)) == (ops.HalfFactorJob, ops.HalfFactorJob)
    assert (sides.a.kernel, sides.a.stride, sides.a.padding) == ((1, 3), (1, 2), (0, 0)) and sides.L == 15
    assert ops.factor_jobs(model[2], ops.ShapeOnly((6, 8, 32)), None).L == 15
    reduce = ops.factor_jobs(model[0], ops.ShapeOnly((6, 3, 32)), ops.ShapeOnly((6, 8, 32)), approximation="reduce")
    assert type(reduce.a) is ops.ReduceFactorJob and reduce.a.src == (6, 3, 1, 32) and reduce.a.kernel == (1, 5)
    assert (reduce.n, reduce.m, reduce.N, reduce.L) == (16, 8, 6, 32)
    # tensors are viewed, not copied
    x = torch.zeros(6, 3, 32)
    assert ops.conv_view(model[0], x, None).x.data_ptr() == x.data_ptr()
    op = ops.per_sample_operands(model[0], x, torch.zeros(6, 8, 32)).x
    assert op.pack.shape == (6, 3, 1, 32) and op.pack.kernel == (1, 5) and op.rows == 16 and op.L == 32


# ------------------------------------------------------------------------------------------------ host-only entry points
# (N, C, D, H, W), kernel, stride, padding: the factor cases of tests/test_conv_nd_gpu.py
GEOMETRIES = [((2, 3, 5, 6, 7), 3, 1, 1), ((2, 2, 6, 5, 7), (2, 3, 1), (2, 1, 2), (1, 0, 1)),
              ((1, 4, 4, 4, 4), (1, 3, 3), (1, 2, 2), (0, 1, 1)), ((2, 3, 3, 5, 5), (3, 1, 1), 1, (2, 0, 0)),
              ((2, 3, 3, 5, 5), 3, 1, (3, 1, 1)), ((2, 64, 4, 8, 8), 3, 1, 1), ((2, 32, 8, 16, 16), 3, 1, 1),
              ((1, 2, 3, 3, 4101), (2, 1, 3), 1, (0, 0, 1))]


def job(shape, kernel, stride=1, padding=0, bias=True):
    return ops.Conv3dFactorJob(tuple(shape), None, triple(kernel), triple(stride), triple(padding), bias)


def bytes_of(jobs):
    return int(_lib.lib().curv_kfac_conv3d_workspace_bytes(ops._conv3d_descs(jobs, check_tensors=False), len(jobs)))


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("bias", [True, False])
def test_flops_are_those_of_the_plain_build_of_the_stack(geometry, bias):
    j = job(*geometry, bias=bias)
    (N, C, D, H, W), k, s, p = geometry[0], triple(geometry[1]), triple(geometry[2]), triple(geometry[3])
    Do = (D + 2 * p[0] - k[0]) // s[0] + 1
    assert j.stack_shape == (N * Do, C * k[0], H, W)
    plain = ops.FactorJob(j.stack_shape, None, k[1:], s[1:], p[1:], bias)
    assert ops.kfac_conv3d_plan_flops([j]) == ops.kfac_plan_flops([plain])
    arr = ops._factor_descs([plain], check_tensors=False)
    plain_bytes = int(_lib.lib().curv_kfac_workspace_bytes(arr, 1))
    stack_bytes = 4 * math.prod(j.stack_shape)
    assert stack_bytes + plain_bytes <= bytes_of([j]) <= stack_bytes + plain_bytes + 3 * 256


def test_a_batch_is_the_sum_and_the_list_of_its_items():
    jobs = [job(*g) for g in GEOMETRIES[:5]]
    assert bytes_of(jobs) == sum(bytes_of([j]) for j in jobs)
    assert ops.kfac_conv3d_plan_flops(jobs) == [ops.kfac_conv3d_plan_flops([j])[0] for j in jobs]
    assert ops.kfac_conv3d_plan_flops([]) == []


def test_the_grouped_launch_case_is_above_the_small_launch_form():
    j = job(*GEOMETRIES[6])
    plain = ops.FactorJob(j.stack_shape, None, (3, 3), (1, 1), (1, 1), True)
    assert ops.kfac_path_for([plain]) == _lib.PATH_GROUPED
    small = job(*GEOMETRIES[0])
    assert ops.kfac_path_for([ops.FactorJob(small.stack_shape, None, (3, 3), (1, 1), (1, 1), True)]) == _lib.PATH_SMALL


@pytest.mark.parametrize("change, text", [
    (dict(kernel=(7, 3, 3)), "kernel larger than the padded input"),
    (dict(kernel=(3, 9, 3)), "kernel larger than the padded input"),
    (dict(stride=(0, 1, 1)), "invalid geometry"),
    (dict(padding=(-1, 0, 0)), "invalid geometry"),
    (dict(shape=(2, 3, 0, 6, 7)), "invalid geometry"),
    (dict(shape=(2, 1 << 20, 4, 1 << 6, 1 << 6), kernel=(3, 1, 1), padding=(1, 0, 0)), "too large"),
    (dict(shape=(1 << 16, 1 << 10, 2, 16, 2), kernel=(1, 1, 1), padding=(0, 0, 0)), "plain build rejected"),
])
def test_refused_geometries_report_zero_bytes_and_name_the_factor(change, text):
    base = dict(shape=(2, 3, 4, 6, 7), kernel=(3, 3, 3), stride=(1, 1, 1), padding=(1, 1, 1))
    base.update(change)
    jobs = [job((2, 3, 5, 6, 7), 3, 1, 1), job(base["shape"], base["kernel"], base["stride"], base["padding"])]
    assert bytes_of(jobs) == 0
    with pytest.raises(RuntimeError) as err:
        ops.kfac_conv3d_plan_flops(jobs)
    assert "curv_kfac_conv3d: factor 1" in str(err.value) and text in str(err.value), str(err.value)


def test_empty_calls_and_null_descriptors():
    L = _lib.lib()
    assert L.curv_kfac_conv3d_workspace_bytes(None, 0) == 0
    assert L.curv_kfac_conv3d_plan_flops(None, 0, None) == 0
    assert L.curv_kfac_conv3d_accumulate(None, None, 0, None, 0) == 0
    assert L.curv_kfac_conv3d_workspace_bytes(None, 1) == 0
    assert L.curv_kfac_conv3d_accumulate(None, None, 1, None, 0) != 0
    ops.kfac_accumulate_conv3d([])
    with pytest.raises(RuntimeError):                                               # no CPU fallback
        ops.kfac_accumulate_conv3d([ops.Conv3dFactorJob(torch.zeros(1, 1, 2, 2, 2), torch.zeros(9, 9), (2, 2, 2),
                                                        has_bias=True)])


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_version_is_unchanged_and_the_struct_matches_the_header():
    assert _lib.lib().curv_version() == 12 == _lib.ABI_VERSION
    header = open(os.path.join(_lib.INCLUDE, "curv_hip.h")).read()
    body = re.search(r"typedef struct curv_conv3d_factor_desc \{(.*?)\} curv_conv3d_factor_desc;", header, re.S).group(1)
    fields = []                                                                     # (ctype, name) in declaration order
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind, names = re.match(r"(const float\*|float\*|int32_t|float)\s+(.*)", decl).groups()
        fields += [(kind, n.strip()) for n in names.split(",")]
    assert [n for _, n in fields] == ["src", "dst", "N", "C", "D", "H", "W", "kd", "kh", "kw", "sd", "sh", "sw", "pd", "ph",
                                      "pw", "has_bias", "first", "scale"]
    assert [n for n, _ in _lib.curv_conv3d_factor_desc._fields_] == [n for _, n in fields]
    size = {"const float*": 8, "float*": 8, "int32_t": 4, "float": 4}
    ctype = {"const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "float": ctypes.c_float}
    offset = 0
    for (kind, name), (_, ct) in zip(fields, _lib.curv_conv3d_factor_desc._fields_):
        assert ct is ctype[kind], name
        assert getattr(_lib.curv_conv3d_factor_desc, name).offset == offset, name   # no padding: pointers first, then 4-byte fields
        offset += size[kind]
    assert ctypes.sizeof(_lib.curv_conv3d_factor_desc) == (offset + 7) // 8 * 8 == 16 + 17 * 4 + 4


def test_the_new_symbols_resolve():
    L = _lib.lib()
    for name in ("curv_kfac_conv3d_workspace_bytes", "curv_kfac_conv3d_plan_flops", "curv_kfac_conv3d_accumulate"):
        assert getattr(L, name) is not None
        assert f" {name}(" in open(os.path.join(_lib.INCLUDE, "curv_hip.h")).read()
    assert "conv3d_factor.hip" in _lib.SOURCES


# ------------------------------------------------------------------------------------------------ sharding
def test_shard_planner_takes_a_conv3d_and_a_conv1d(admitted):
    model = model3d()
    layers = [model[0], model[2], model[4]]
    shapes = {model[0]: ((32, 2, 4, 6, 6), (32, 4, 4, 6, 6)), model[2]: ((32, 4, 4, 6, 6), (32, 4, 4, 3, 3)),
              model[4]: ((32, 144), (32, 5))}
    dims = sharding.layer_dims(layers, shapes)
    assert [d[:3] for d in dims] == [(55, 4, 32 * 144), (37, 4, 32 * 36), (145, 5, 32)]
    a_side = ops.kfac_conv3d_plan_flops([job((32, 2, 4, 6, 6), 3, 1, 1)])[0]
    g_side = ops.kfac_plan_flops([ops.FactorJob((32, 4, 24, 6), None)])[0]
    assert dims[0][3] == float(a_side + g_side)
    owner = sharding.partition_layers(dims, 2)
    assert len(owner) == 3 and set(owner) == {0, 1}
    assert sharding.rank_cost(dims, "kfac") > 0
    one = model1d()
    dims = sharding.layer_dims([one[0], one[2]], {one[0]: ((6, 3, 32), (6, 8, 32)), one[2]: ((6, 8, 32), (6, 8, 15))})
    assert [d[:3] for d in dims] == [(16, 8, 6 * 32), (25, 8, 6 * 15)]


# ------------------------------------------------------------------------------------------------ the identity
# isotropic; anisotropic with depth stride 2; kd = 1; pd > kd / 2
IDENTITY = [((2, 3, 5, 6, 7), 4, 3, 1, 1), ((2, 2, 6, 5, 7), 3, (2, 3, 1), (2, 1, 2), (1, 0, 1)),
            ((1, 4, 4, 4, 4), 2, (1, 3, 3), (1, 2, 2), (0, 1, 1)), ((2, 3, 3, 5, 5), 3, (3, 1, 1), 1, (2, 0, 0))]


def im2col3d(x, k, s, p):
    """(C kd kh kw, N Do Ho Wo): pad, then unfold over the three spatial axes."""
    xp = F.pad(x, (p[2], p[2], p[1], p[1], p[0], p[0]))
    u = xp.unfold(2, k[0], s[0]).unfold(3, k[1], s[1]).unfold(4, k[2], s[2])          # (N, C, Do, Ho, Wo, kd, kh, kw)
    return u.permute(1, 5, 6, 7, 0, 2, 3, 4).reshape(x.shape[1] * math.prod(k), -1)


def depth_unfolded(x, k, s, p):
    """x'[(n Do + d), (c kd + a), h, w] = x[n, c, d sd + a - pd, h, w], zero outside the input."""
    N, C, D, H, W = x.shape
    u = F.pad(x, (0, 0, 0, 0, p[0], p[0])).unfold(2, k[0], s[0])                      # (N, C, Do, H, W, kd)
    return u.permute(0, 2, 1, 5, 3, 4).reshape(N * u.shape[2], C * k[0], H, W)


@pytest.mark.parametrize("shape, M, kernel, stride, padding", IDENTITY)
def test_the_identity_in_float64(shape, M, kernel, stride, padding):
    k, s, p = triple(kernel), triple(stride), triple(padding)
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=gen, dtype=torch.float64)
    layer = torch.nn.Conv3d(shape[1], M, k, stride=s, padding=p, bias=False).double()
    X3 = im2col3d(x, k, s, p)
    stack = depth_unfolded(x, k, s, p)
    cols = F.unfold(stack, k[1:], padding=p[1:], stride=s[1:])                         # (N Do, C kd kh kw, Ho Wo)
    X2 = cols.transpose(0, 1).reshape(cols.shape[1], -1)
    assert torch.equal(X2, X3)                                                         # element for element
    # the rows are those of weight.reshape(Cout, -1): the forward product and the weight gradient
    out = layer(x)
    Wm = layer.weight.reshape(M, -1)
    assert torch.allclose((Wm @ X3).reshape(M, shape[0], *out.shape[2:]).transpose(0, 1), out, rtol=1e-12, atol=1e-12)
    g = torch.randn(out.shape, generator=gen, dtype=torch.float64)
    out.backward(g)
    G_mat = g.transpose(0, 1).reshape(M, -1)
    assert torch.allclose(layer.weight.grad.reshape(M, -1), G_mat @ X3.t(), rtol=1e-12, atol=1e-12)
    # and grad_output seen as (N, Cout, Do Ho, Wo) has these columns in this order
    g4 = g.reshape(g.shape[0], M, g.shape[2] * g.shape[3], g.shape[4])
    assert torch.equal(g4.permute(1, 0, 2, 3).reshape(M, -1), G_mat)
