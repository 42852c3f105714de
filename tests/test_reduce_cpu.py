"""KFAC-reduce without a GPU: the default stays expand, the refusals of ``KFAC(approximation="reduce")``,
the routing of `factor_jobs`, the host-only entry points of csrc/reduce_factor.hip (plan flops, workspace bytes, refusals)
and the shard planner."""
import ctypes

import pytest
import torch

from curvature_amd import _lib, ops, sharding
from curvature_amd.curvatures import KFAC


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def plane(shape, kernel=1, stride=1, padding=0, bias=True, mean=True, dtype=torch.float32):
    return ops.ReduceFactorJob(tuple(shape), None, pair(kernel), pair(stride), pair(padding), bias, mean=mean, dtype=dtype)


def token(shape, bias=True, mean=True, dtype=torch.float32):
    return ops.ReduceFactorJob(tuple(shape), None, has_bias=bias, form=_lib.REDUCE_TOKEN, mean=mean, dtype=dtype)


def bytes_of(jobs):
    arr = ops._reduce_descs(jobs, check_tensors=False)
    return int(_lib.lib().curv_kfac_reduce_workspace_bytes(arr, len(jobs)))


# ------------------------------------------------------------------------------------------------ the default is unchanged
FIELDS = ("kernel", "stride", "padding", "has_bias", "scale", "first", "src")


def same_job(a, b):
    assert type(a) is type(b)
    for f in FIELDS + tuple(type(a).__slots__):
        assert getattr(a, f, None) == getattr(b, f, None), f


def test_default_is_expand():
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.Flatten(), torch.nn.Linear(800, 5))
    assert KFAC(model).approximation == "expand"
    assert KFAC(model, approximation="expand").approximation == "expand"


@pytest.mark.parametrize("layer, x, g, types, dims", [
    (torch.nn.Linear(6, 7), (4, 6), (4, 7), ("FactorJob", "FactorJob"), (7, 7, 4, 1)),
    (torch.nn.Conv2d(3, 8, 3, padding=1), (4, 3, 10, 10), (4, 8, 10, 10), ("FactorJob", "FactorJob"), (28, 8, 4, 100)),
    (torch.nn.Linear(6, 7), (3, 5, 6), (3, 5, 7), ("FactorJob", "FactorJob"), (7, 7, 15, 1)),
], ids=["linear", "conv", "linear3d"])
def test_factor_jobs_without_the_argument_is_what_it_was(layer, x, g, types, dims):
    """The values are those of the parent commit: a 3-D Linear record is flattened to N L rows of one position."""
    sides = ops.factor_jobs(layer, ops.ShapeOnly(x), ops.ShapeOnly(g))
    assert (type(sides.a).__name__, type(sides.g).__name__) == types
    assert (sides.n, sides.m, sides.N, sides.L) == dims and sides.groups == 1
    conv = isinstance(layer, torch.nn.Conv2d)
    want_a = ops.FactorJob(x if conv else (dims[2], 6), None, layer.kernel_size if conv else (1, 1),
                           layer.stride if conv else (1, 1), layer.padding if conv else (0, 0), True)
    want_g = ops.FactorJob(g if conv else (dims[2], 7), None)
    same_job(sides.a, want_a)
    same_job(sides.g, want_g)
    half = ops.factor_jobs(layer, ops.ShapeOnly(x, torch.bfloat16), ops.ShapeOnly(g, torch.float16))
    assert type(half.a) is ops.HalfFactorJob and half.a.dtype == torch.bfloat16 and half.g.dtype == torch.float16


def test_explicit_expand_is_the_default():
    layer = torch.nn.Conv2d(3, 8, 3, padding=1)
    x, g = ops.ShapeOnly((4, 3, 10, 10)), ops.ShapeOnly((4, 8, 10, 10))
    a, b = ops.factor_jobs(layer, x, g), ops.factor_jobs(layer, x, g, approximation="expand")
    same_job(a.a, b.a)
    same_job(a.g, b.g)
    assert a[2:] == b[2:]


# ------------------------------------------------------------------------------------------------ the constructor
def test_a_bad_string_raises_value_error():
    model = torch.nn.Sequential(torch.nn.Linear(4, 3))
    with pytest.raises(ValueError, match="approximation"):
        KFAC(model, approximation="reduced")
    with pytest.raises(ValueError, match="approximation"):
        ops.factor_jobs(model[0], ops.ShapeOnly((2, 4)), None, approximation="Reduce")


@pytest.mark.parametrize("bad, text, admit", [
    (torch.nn.Conv2d(4, 8, 3, groups=2), "grouped", False),
    (torch.nn.Conv2d(4, 4, 3, groups=4), "grouped", False),
    (torch.nn.Conv2d(3, 8, 3, padding=2, dilation=2), "dilated", False),
    (torch.nn.Conv2d(3, 8, 3, padding=2, dilation=2), "dilated", True),
    (torch.nn.ConvTranspose2d(3, 8, 3), "transposed", False),
    (torch.nn.MultiheadAttention(8, 2), "attention", False),
], ids=["grouped", "depthwise", "dilated", "dilated_admitted", "convt", "mha"])
def test_reduce_refusals_name_the_layer(bad, text, admit):
    model = torch.nn.Sequential()
    model.add_module("odd_one", bad)
    types = ['Linear', 'Conv2d', 'ConvTranspose2d', 'MultiheadAttention']
    was = ops.admit_dilated(admit)
    try:
        with pytest.raises(NotImplementedError, match=text) as err:
            KFAC(model, types, approximation="reduce")
    finally:
        ops.admit_dilated(was)
    assert "odd_one" in str(err.value) and 'approximation="expand"' in str(err.value)


def test_string_padding_raises_as_before():
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding='same'))
    for kwargs in ({}, {"approximation": "reduce"}):
        with pytest.raises(NotImplementedError, match="string padding"):
            KFAC(model, **kwargs)


def test_factor_jobs_refuses_what_the_constructor_refuses():
    for bad in (torch.nn.Conv2d(4, 8, 3, groups=2), torch.nn.Conv2d(3, 8, 3, dilation=2), torch.nn.ConvTranspose2d(3, 8, 3)):
        with pytest.raises(NotImplementedError, match="expand"):
            ops.factor_jobs(bad, ops.ShapeOnly((2, bad.in_channels, 8, 8)), None, approximation="reduce")


# ------------------------------------------------------------------------------------------------ routing
def test_reduce_routing_of_a_convolution():
    layer = torch.nn.Conv2d(3, 8, 3, padding=1)
    sides = ops.factor_jobs(layer, ops.ShapeOnly((4, 3, 10, 10)), ops.ShapeOnly((4, 8, 10, 10)), approximation="reduce")
    assert type(sides.a) is ops.ReduceFactorJob and type(sides.g) is ops.ReduceFactorJob
    assert (sides.n, sides.m, sides.N, sides.L, sides.groups) == (28, 8, 4, 100, 1)
    a, g = sides.a, sides.g
    assert (a.form, a.mean, a.kernel, a.stride, a.padding, a.has_bias, a.src) == \
        (_lib.REDUCE_PLANE, True, (3, 3), (1, 1), (1, 1), True, (4, 3, 10, 10))
    assert (g.form, g.mean, g.kernel, g.stride, g.padding, g.has_bias, g.src) == \
        (_lib.REDUCE_PLANE, False, (1, 1), (1, 1), (0, 0), False, (4, 8, 10, 10))
    # no grad_output: the output size from the geometry; one position is still a plane-form job
    alone = ops.factor_jobs(torch.nn.Conv2d(3, 8, 3, stride=2, padding=1), ops.ShapeOnly((4, 3, 10, 10)), None,
                            approximation="reduce")
    assert alone.g is None and alone.L == 25
    one = ops.factor_jobs(torch.nn.Conv2d(3, 8, 3), ops.ShapeOnly((4, 3, 3, 3)), ops.ShapeOnly((4, 8, 1, 1)),
                          approximation="reduce")
    assert one.L == 1 and type(one.a) is ops.ReduceFactorJob and type(one.g) is ops.ReduceFactorJob


@pytest.mark.parametrize("shape, L", [((3, 5, 6), 5), ((3, 2, 5, 6), 10)])
def test_reduce_routing_of_a_token_linear(shape, L):
    layer = torch.nn.Linear(6, 7)
    sides = ops.factor_jobs(layer, ops.ShapeOnly(shape), ops.ShapeOnly(shape[:-1] + (7,)), approximation="reduce")
    assert type(sides.a) is ops.ReduceFactorJob and type(sides.g) is ops.ReduceFactorJob
    assert (sides.n, sides.m, sides.N, sides.L) == (7, 7, 3, L)
    assert (sides.a.form, sides.a.mean, sides.a.has_bias, sides.a.src) == (_lib.REDUCE_TOKEN, True, True, (3, L, 6))
    assert (sides.g.form, sides.g.mean, sides.g.has_bias, sides.g.src) == (_lib.REDUCE_TOKEN, False, False, (3, L, 7))


def test_reduce_routing_of_a_flat_linear_is_todays_jobs():
    layer = torch.nn.Linear(6, 7)
    x, g = ops.ShapeOnly((4, 6)), ops.ShapeOnly((4, 7))
    reduce, expand = ops.factor_jobs(layer, x, g, approximation="reduce"), ops.factor_jobs(layer, x, g)
    assert type(reduce.a) is ops.FactorJob and type(reduce.g) is ops.FactorJob
    same_job(reduce.a, expand.a)
    same_job(reduce.g, expand.g)
    assert (reduce.n, reduce.m, reduce.N, reduce.L) == (7, 7, 4, 1)
    half = ops.factor_jobs(layer, ops.ShapeOnly((4, 6), torch.bfloat16), ops.ShapeOnly((4, 7), torch.bfloat16),
                           approximation="reduce")
    assert type(half.a) is ops.HalfFactorJob and type(half.g) is ops.HalfFactorJob


def test_half_records_go_to_the_same_job_with_their_dtype():
    conv = ops.factor_jobs(torch.nn.Conv2d(3, 8, 3, padding=1), ops.ShapeOnly((4, 3, 10, 10), torch.bfloat16),
                           ops.ShapeOnly((4, 8, 10, 10), torch.float16), approximation="reduce")
    assert type(conv.a) is ops.ReduceFactorJob and conv.a.dtype == torch.bfloat16 and conv.g.dtype == torch.float16
    lin = ops.factor_jobs(torch.nn.Linear(6, 7), ops.ShapeOnly((3, 5, 6), torch.float16), None, approximation="reduce")
    assert lin.a.dtype == torch.float16 and lin.g is None
    arr = ops._reduce_descs([conv.a, conv.g, lin.a], check_tensors=False)
    assert [d.dtype for d in arr] == [_lib.DTYPE_BF16, _lib.DTYPE_F16, _lib.DTYPE_F16]
    with pytest.raises(RuntimeError, match="float32, bfloat16 or float16"):
        ops.factor_jobs(torch.nn.Linear(6, 7), ops.ShapeOnly((3, 5, 6), torch.float64), None, approximation="reduce")


def test_real_records_are_not_flattened_or_copied():
    layer = torch.nn.Linear(6, 7)
    x, g = torch.zeros(3, 2, 5, 6), torch.zeros(3, 2, 5, 7, dtype=torch.bfloat16)
    sides = ops.factor_jobs(layer, x, g, approximation="reduce")
    assert tuple(sides.a.src.shape) == (3, 10, 6) and sides.a.src.data_ptr() == x.data_ptr()
    assert tuple(sides.g.src.shape) == (3, 10, 7) and sides.g.src.data_ptr() == g.data_ptr() and sides.g.dtype == torch.bfloat16


# ------------------------------------------------------------------------------------------------ host-only entry points
def test_plan_flops_on_shapes():
    jobs = [plane((32, 256, 28, 28), 3, 1, 1), plane((32, 256, 28, 28), mean=False, bias=False), token((3, 5, 6)),
            plane((4, 3, 10, 10), 3, 2, 1, dtype=torch.bfloat16), token((2, 300, 130), bias=False, mean=False)]
    flops = ops.kfac_reduce_plan_flops(jobs)
    assert all(isinstance(f, int) and f > 0 for f in flops)
    assert flops == [ops.kfac_reduce_plan_flops([j])[0] for j in jobs]                 # additive over a batch
    assert ops.kfac_reduce_plan_flops([]) == []
    # the adds of the pass plus the flat build of the (N, dim) rows
    flat = ops.kfac_plan_flops([ops.FactorJob((32, 256 * 9), None, has_bias=True)])[0]
    assert flops[0] == 32 * 256 * (28 * 28 * 3 + 28 * 9) + flat
    assert flops[2] == 3 * 5 * 6 + ops.kfac_plan_flops([ops.FactorJob((3, 6), None, has_bias=True)])[0]
    # below the expand plan of the same 28x28 3x3 layer, on both sides
    expand = ops.kfac_plan_flops([ops.FactorJob((32, 256, 28, 28), None, (3, 3), (1, 1), (1, 1), True),
                                  ops.FactorJob((32, 256, 28, 28), None)])
    assert flops[0] < expand[0] and flops[1] < expand[1]


def test_workspace_is_the_sum_over_the_factors():
    jobs = [plane((2, 3, 5, 7), 3, 1, 1), token((2, 5, 7)), plane((4, 130, 4, 4), 3, 1, 1, bias=False)]
    alone = [bytes_of([j]) for j in jobs]
    assert all(b > 0 and b % 256 == 0 for b in alone)
    assert bytes_of(jobs) == sum(alone)
    # the rows (N, dim) float32, 256-byte aligned, then the flat build's scratch
    arr = ops._factor_descs([ops.FactorJob((2, 27), None, has_bias=True)], check_tensors=False)
    flat = int(_lib.lib().curv_kfac_workspace_bytes(arr, 1))
    assert alone[0] == 256 + (flat + 255) // 256 * 256


def test_layer_dims_prices_reduce_layers_host_only():
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.Flatten(), torch.nn.Linear(800, 5))
    layers = [model[0], model[2]]
    shapes = {model[0]: ((32, 3, 10, 10), (32, 8, 10, 10)), model[2]: ((32, 800), (32, 5))}
    dims = sharding.layer_dims(layers, shapes, approximation="reduce")
    assert [d[:3] for d in dims] == [(28, 8, 3200), (801, 5, 32)]
    want = sum(ops.kfac_reduce_plan_flops([plane((32, 3, 10, 10), 3, 1, 1), plane((32, 8, 10, 10), bias=False, mean=False)]))
    assert dims[0][3] == float(want)
    expand = sharding.layer_dims(layers, shapes)
    assert dims[1] == expand[1] and dims[0][3] < expand[0][3]
    assert sharding.layer_dims(layers, shapes, "expand") == expand
    assert len(sharding.partition_layers(dims, 2)) == 2 and sharding.rank_cost(dims, "kfac") > 0


def raw(job, **fields):
    arr = ops._reduce_descs([plane((2, 3, 8, 8), 3, 1, 1), job], check_tensors=False)
    for k, v in fields.items():
        setattr(arr[1], k, v)
    return arr


REFUSALS = [
    (lambda: raw(plane((2, 3, 8, 8), 3, 1, 1), dtype=7), "unknown dtype 7"),
    (lambda: raw(plane((2, 3, 8, 8), 3, 1, 1), form=2), "unknown form 2"),
    (lambda: raw(plane((2, 3, 8, 8), 3, (0, 1), 1)), "invalid geometry"),                  # stride below 1
    (lambda: raw(plane((2, 3, 8, 8), 3, 1, (1, -1))), "invalid geometry"),                 # negative padding
    (lambda: raw(plane((2, 3, 4, 4), 7, 1, 1)), "kernel larger than the padded input"),    # no output pixel
    (lambda: raw(plane((2, 3, 8, 2), (1, 5), 1, (0, 1))), "kernel larger than the padded input"),
    (lambda: raw(plane((2, 200000, 8, 8), 3, 1, 1)), "too large"),                         # dim above 2^20
    (lambda: raw(token((2, 5, (1 << 20) + 1))), "too large"),
    (lambda: raw(plane((1 << 16, 1 << 15, 1, 1))), "too large"),                           # 2^31 planes
    (lambda: raw(token((1 << 16, 1 << 15, 2))), "too large"),                              # 2^31 token rows
    (lambda: raw(token((2, 0, 6))), "invalid geometry"),
    (lambda: raw(token((1 << 12, 2, 1 << 19))), "flat build rejected"),                    # its limit of 2^31 row-matrix entries
]


@pytest.mark.parametrize("make, text", REFUSALS, ids=[f"{i}-{t}" for i, (_, t) in enumerate(REFUSALS)])
def test_c_side_refusals_name_the_factor(make, text):
    L = _lib.lib()
    arr = make()
    assert L.curv_kfac_reduce_workspace_bytes(arr, 2) == 0
    message = L.curv_last_error().decode()
    assert "factor 1" in message and text in message, message
    out = (ctypes.c_longlong * 2)()
    assert L.curv_kfac_reduce_plan_flops(arr, 2, out) == _lib.ERR_INVALID
    assert "factor 1" in L.curv_last_error().decode()
    # the build itself refuses before it looks at a pointer or launches anything
    assert L.curv_kfac_reduce_accumulate(None, arr, 2, None, 0) == _lib.ERR_INVALID
    assert "factor 1" in L.curv_last_error().decode()


def test_the_flat_builds_text_is_appended():
    L = _lib.lib()
    arr = raw(token((1 << 12, 2, 1 << 19)))
    assert L.curv_kfac_reduce_workspace_bytes(arr, 2) == 0
    message = L.curv_last_error().decode()
    flat = ops._factor_descs([ops.FactorJob((1 << 12, 1 << 19), None, has_bias=True)], check_tensors=False)
    assert L.curv_kfac_workspace_bytes(flat, 1) == 0
    assert message.endswith(L.curv_last_error().decode())


def test_empty_calls_and_null_descriptors():
    L = _lib.lib()
    assert L.curv_kfac_reduce_accumulate(None, None, 0, None, 0) == 0
    assert L.curv_kfac_reduce_plan_flops(None, 0, None) == 0
    assert L.curv_kfac_reduce_workspace_bytes(None, 1) == 0 and b"null descriptors" in L.curv_last_error()
    arr = ops._reduce_descs([plane((2, 3, 8, 8), 3, 1, 1)], check_tensors=False)
    assert L.curv_kfac_reduce_accumulate(None, arr, 1, None, 0) == _lib.ERR_INVALID          # valid geometry, null tensors
    assert b"null src or dst" in L.curv_last_error()
    with pytest.raises(RuntimeError, match="factor 0"):
        ops.kfac_reduce_plan_flops([plane((2, 3, 4, 4), 7, 1, 1)])


def test_abi_version_and_struct_layout():
    assert _lib.lib().curv_version() == 12 == _lib.ABI_VERSION
    # two pointers, N C H W, the window (6), has_bias first scale, dtype form mean, T E
    assert ctypes.sizeof(_lib.curv_reduce_factor_desc) == 16 + (4 + 6 + 3 + 3 + 2) * 4
    d = _lib.curv_reduce_factor_desc
    assert (d.N.offset, d.kh.offset, d.has_bias.offset, d.scale.offset, d.dtype.offset, d.form.offset, d.mean.offset,
            d.T.offset, d.E.offset) == (16, 32, 56, 64, 68, 72, 76, 80, 84)
    assert ctypes.sizeof(_lib.curv_dilated_factor_desc) == ctypes.sizeof(_lib.curv_convt_factor_desc)   # untouched
