"""Grouped and depthwise convolutions in the per-sample line, without a GPU: the switch
`ops.admit_grouped_per_sample` and what off means, the selection with it on, `ops.per_sample_route`, the operands of a
group slice, the host side of the curv_persample_dw_* entry points and the refusal of half-precision records."""
import ctypes
import os
import shutil
import subprocess
from collections import OrderedDict

import pytest
import torch

from curvature_amd import _lib, ops
from curvature_amd.curvatures import EFB, KFAC, Diagonal


@pytest.fixture
def admitted():
    was = ops.admit_grouped_per_sample(True)
    yield
    ops.admit_grouped_per_sample(was)


def model():
    torch.manual_seed(3)
    return torch.nn.Sequential(OrderedDict([("plain", torch.nn.Conv2d(2, 4, 3, padding=1)),
                                            ("grouped_one", torch.nn.Conv2d(4, 4, 3, groups=2)),
                                            ("flat", torch.nn.Flatten()), ("head", torch.nn.Linear(36, 3))]))


# ------------------------------------------------------------------------------------------------ the switch
def test_the_switch_is_off_by_default_and_returns_what_it_was():
    assert ops.per_sample_admits_groups() is False
    assert ops.admit_grouped_per_sample(True) is False
    try:
        assert ops.per_sample_admits_groups() is True
        assert ops.admit_grouped_per_sample() is True
        assert ops.per_sample_is_wide() is False                             # independent of the other switch
    finally:
        assert ops.admit_grouped_per_sample(False) is True
    assert ops.per_sample_admits_groups() is False


@pytest.mark.parametrize("wide", [False, True])
def test_off_a_grouped_layer_raises_as_it_did(wide):
    net = model()
    was = ops.widen_per_sample(wide)
    try:
        message = (r"^Diagonal\(per_sample=True\): layer 'grouped_one' is not supported \(grouped convolution "
                   r"\(groups=2\)\); select other layer types or use per_sample=False$")
        with pytest.raises(NotImplementedError, match=message):
            Diagonal(net, per_sample=True)
        est = Diagonal(net)
        with pytest.raises(NotImplementedError, match=r"^X: layer 'grouped_one' is not supported \(grouped convolution "
                                                      r"\(groups=2\)\); advice$"):
            est._per_sample_layers("X", "advice")
        with pytest.raises(NotImplementedError, match="grouped_one"):
            est._per_sample_layers("X", "advice", grouped=True)              # the caller's wish alone admits nothing
        with pytest.raises(NotImplementedError, match="^per-sample update: unsupported layer Conv2d$"):
            ops.per_sample_operands(net.grouped_one, torch.zeros(2, 4, 5, 5), torch.zeros(2, 4, 3, 3))
        with pytest.raises(NotImplementedError):
            ops.per_sample_operands(ops.GroupSlice(net.grouped_one, 0), torch.zeros(2, 4, 5, 5), torch.zeros(2, 4, 3, 3))
    finally:
        ops.widen_per_sample(was)


# ------------------------------------------------------------------------------------------------ selection
def test_on_diagonal_constructs_and_records(admitted):
    net = model()
    est = Diagonal(net, per_sample=True)
    assert set(est.record) == {net.plain, net.grouped_one, net.head}
    x = torch.randn(2, 2, 5, 5)
    net(x).sum().backward()
    forward, backward = est.record[net.grouped_one]
    assert tuple(forward.shape) == (2, 4, 5, 5) and tuple(backward.shape) == (2, 4, 3, 3)
    assert est._per_sample_layers("X", "advice", grouped=True) == [net.plain, net.grouped_one, net.head]
    for hook in est.hooks:
        hook.remove()


def test_on_the_other_callers_still_refuse_and_say_who_takes_it(admitted):
    net = model()
    with pytest.raises(NotImplementedError, match="grouped_one"):
        EFB(net, {}, per_sample=True)
    for est in (Diagonal(net, per_sample=True), KFAC(net)):
        for layer in (net.plain, net.grouped_one, net.head):                 # (any state will do: the selection comes first)
            est.state[layer] = est.inv_state[layer] = torch.zeros(1)
        with pytest.raises(NotImplementedError, match="grouped_one.*functional_variance take it"):
            est.stage_output(0, 2, inputs=True)
        est._decomposition = {}
        with pytest.raises(NotImplementedError, match="grouped_one.*functional_variance take it"):
            est.functional_variance_grid(torch.zeros(1, 2), [(1.0, 1.0)])
        for hook in est.hooks:
            hook.remove()
    convt = torch.nn.Sequential(OrderedDict([("up", torch.nn.ConvTranspose2d(4, 4, 3, groups=2))]))
    was = ops.widen_per_sample(True)
    try:
        with pytest.raises(NotImplementedError, match="ConvTranspose2d with groups > 1 is not supported"):
            Diagonal(convt, "ConvTranspose2d", per_sample=True)
    finally:
        ops.widen_per_sample(was)


# ------------------------------------------------------------------------------------------------ the route
def test_route():
    conv = torch.nn.Conv2d
    assert ops.per_sample_route(conv(8, 8, 3, groups=8)) == "depthwise"
    assert ops.per_sample_route(conv(8, 16, 3, groups=8)) == "slices"        # a channel multiplier
    assert ops.per_sample_route(conv(8, 8, 3, groups=2)) == "slices"
    assert ops.per_sample_route(conv(8, 8, 9, groups=8)) == "slices"         # 81 taps: above the kernel's 49
    assert ops.per_sample_route(conv(8, 8, 7, groups=8)) == "depthwise"
    assert ops.per_sample_route(conv(8, 8, 3)) == "whole"
    assert ops.per_sample_route(torch.nn.Linear(3, 4)) == "whole"
    layer = conv(8, 8, 3, groups=2)
    assert ops.per_sample_items([conv(8, 8, 3, groups=8)])[0].__class__.__name__ == "Conv2d"
    items = ops.per_sample_items([layer])
    assert items == [ops.GroupSlice(layer, 0), ops.GroupSlice(layer, 1)] and len({*items, ops.GroupSlice(layer, 1)}) == 2
    assert items[1].rows == slice(4, 8)


# ------------------------------------------------------------------------------------------------ operands of a slice
def test_slice_operands(admitted):
    layer = torch.nn.Conv2d(8, 8, 3, padding=1, groups=2)
    x, g = torch.zeros(2, 8, 6, 6), torch.zeros(2, 8, 6, 6)
    for k in range(2):
        s = ops.per_sample_operands(ops.GroupSlice(layer, k), x, g)
        assert (s.N, s.m, s.n, s.L) == (2, 4, 4 * 9 + 1, 36)
        assert (s.g.rows, s.x.rows) == (4, 4 * 9 + 1)
        # the x side: the pack reads the view at channel offset 4 k through the record's strides
        assert s.x.pack is not None and s.x.pack.shape == (2, 4, 6, 6) and s.x.pack.strides == (8 * 36, 36, 6, 1)
        assert s.x.pack.has_bias and s.x.pack.kernel == (3, 3) and s.x.pack.padding == (1, 1)
        assert s.x.src.storage_offset() == k * 4 * 36 and s.x.src.data_ptr() == x.data_ptr() + 4 * k * 4 * 36
        assert (s.x.Lp, s.x.ns, s.x.rs, s.x.floats) == (36, 37 * 36, 36, 2 * 37 * 36)
        d = _lib.curv_persample_pack_ex_desc()
        ops._fill_pack(d, s.x, torch.zeros(s.x.floats))
        assert (d.N, d.C, d.H, d.W, d.s_n, d.s_c, d.has_bias) == (2, 4, 6, 6, 288, 36, 1)
        assert d.src == s.x.src.data_ptr() and d.src_elems == 2 * 8 * 36 - k * 4 * 36
        # the g side: in place, 4 k 36 floats into the record, with the record's sample stride
        assert s.g.pack is None and s.g.floats == 0 and (s.g.L, s.g.Lp, s.g.ns, s.g.rs) == (36, 36, 8 * 36, 36)
        assert s.g.src.storage_offset() == k * 4 * 36 and s.g.src.data_ptr() == g.data_ptr() + 4 * k * 4 * 36
        assert s.g.src.numel() >= s.g.ns + 4 * 36                            # what the extent check of the products asks
    # L % 4 != 0, or a layout for a rotation: the g side is packed from the view
    s = ops.per_sample_operands(ops.GroupSlice(layer, 1), torch.zeros(2, 8, 5, 5), torch.zeros(2, 8, 5, 5))
    assert s.g.pack is not None and s.g.pack.shape == (2, 4, 5, 5) and s.g.pack.strides == (200, 25, 5, 1)
    assert s.g.src.storage_offset() == 100 and (s.g.Lp, s.g.ns, s.g.rs) == (28, 4 * 28, 28)
    s = ops.per_sample_operands(ops.GroupSlice(layer, 1), x, g, rows_outer=True, in_place=False)
    assert s.g.pack is not None and s.g.rows_outer and (s.g.ns, s.g.rs) == (36, 2 * 36)
    # a bias-free 1x1 / stride-1 slice: x in place as well
    point = torch.nn.Conv2d(8, 6, 1, groups=2, bias=False)
    s = ops.per_sample_operands(ops.GroupSlice(point, 1), x, torch.zeros(2, 6, 6, 6))
    assert s.x.pack is None and (s.x.rows, s.x.ns, s.x.rs) == (4, 8 * 36, 36) and s.x.src.storage_offset() == 4 * 36
    assert s.g.pack is None and (s.g.rows, s.g.ns, s.g.rs) == (3, 6 * 36, 36) and s.g.src.storage_offset() == 3 * 36
    # channels_last records are not read in place
    s = ops.per_sample_operands(ops.GroupSlice(layer, 1), x.contiguous(memory_format=torch.channels_last),
                                g.contiguous(memory_format=torch.channels_last))
    assert s.g.pack is not None and s.g.pack.strides == (288, 1, 48, 8) and s.x.pack.strides == (288, 1, 48, 8)
    with pytest.raises(RuntimeError, match="do not match"):
        ops.per_sample_operands(ops.GroupSlice(layer, 0), x, torch.zeros(2, 8, 5, 5))


def test_half_precision_records_of_a_grouped_layer_are_refused(admitted):
    layer = torch.nn.Conv2d(8, 8, 3, padding=1, groups=2)
    was = ops.widen_per_sample(True)
    try:
        for xd, gd in ((torch.bfloat16, torch.float32), (torch.float32, torch.float16)):
            bad = xd if xd != torch.float32 else gd
            with pytest.raises(RuntimeError, match="GroupSlice.*got " + str(bad).replace(".", r"\.")):
                ops.per_sample_operands(ops.GroupSlice(layer, 0), torch.zeros(2, 8, 6, 6, dtype=xd),
                                        torch.zeros(2, 8, 6, 6, dtype=gd))
        net = model()
        est = Diagonal(net, per_sample=True)
        est.record[net.grouped_one] = [torch.zeros(2, 4, 5, 5, dtype=torch.bfloat16), torch.zeros(2, 4, 3, 3)]
        with pytest.raises(RuntimeError, match=r"'grouped_one' expects float32 records, got torch\.bfloat16"):
            est._records_of("Diagonal", net.grouped_one)
        for hook in est.hooks:
            hook.remove()
    finally:
        ops.widen_per_sample(was)


# ------------------------------------------------------------------------------------------------ ABI, host only
def dw_desc(**fields):
    d = _lib.curv_persample_dw_desc()
    base = dict(N=2, C=3, H=7, W=6, kh=3, kw=3, sh=2, sw=2, ph=1, pw=1, Ho=4, Wo=3, has_bias=1,
                x_sn=126, x_sc=42, x_sh=6, x_sw=1, x_elems=252, g_sn=36, g_sc=12, g_sh=3, g_sw=1, g_elems=72)
    base.update(fields)
    for key, value in base.items():
        setattr(d, key, value)
    return d


def test_dw_entry_points_host_side():
    L = _lib.lib()
    assert L.curv_version() == 12 == _lib.ABI_VERSION
    for name in ("curv_persample_dw_workspace_bytes", "curv_persample_dw_plan_info", "curv_persample_dw_sq_accumulate",
                 "curv_persample_dw_quad_reduce"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert L.curv_persample_dw_sq_accumulate(None, None, 0, None, 0) == 0     # an empty call is a no-op
    assert L.curv_persample_dw_quad_reduce(None, None, 0, None, 0) == 0
    assert L.curv_persample_dw_plan_info(None, 0, None, None) == 0
    ops.per_sample_dw_sq_accumulate([])
    ops.per_sample_dw_quad_reduce([])
    arr = (_lib.curv_persample_dw_desc * 1)(dw_desc())
    assert L.curv_persample_dw_workspace_bytes(arr, 1) == 256                # 2 * 3 * 10 floats, 256-byte aligned
    flops, nbytes = (ctypes.c_longlong * 1)(), (ctypes.c_longlong * 1)()
    assert L.curv_persample_dw_plan_info(arr, 1, flops, nbytes) == 0
    assert flops[0] == 2 * 6 * 12 * 10 and nbytes[0] == 4 * 6 * (42 + 12)
    job = ops.PerSampleDwJob((2, 3, 7, 6), (2, 3, 4, 3), (3, 3), (2, 2), (1, 1), True)
    assert ops.per_sample_dw_plan_info([job]) == ([flops[0]], [nbytes[0]])
    for bad, text in ((dict(sh=0), "item 0"), (dict(kh=0), "item 0"), (dict(Ho=5), "item 0: output 5x3"),
                      (dict(kh=8, kw=8, H=9, W=9, Ho=2, Wo=2), "more than 49 taps"), (dict(x_sw=-1), "negative stride"),
                      (dict(x_elems=251), "extent"), (dict(g_sn=37), "extent")):
        arr = (_lib.curv_persample_dw_desc * 1)(dw_desc(**bad))
        assert L.curv_persample_dw_workspace_bytes(arr, 1) == 0, bad
        assert text in L.curv_last_error().decode(), (bad, L.curv_last_error())
    arr = (_lib.curv_persample_dw_desc * 2)(dw_desc(), dw_desc(sw=0))
    assert L.curv_persample_dw_workspace_bytes(arr, 2) == 0 and "item 1" in L.curv_last_error().decode()
    # the calls themselves refuse the same descriptors, and null records, before anything is launched
    assert L.curv_persample_dw_sq_accumulate(None, arr, 2, None, 0) == _lib.ERR_INVALID
    arr = (_lib.curv_persample_dw_desc * 1)(dw_desc())
    assert L.curv_persample_dw_quad_reduce(None, arr, 1, None, 0) == _lib.ERR_INVALID
    assert "null record" in L.curv_last_error().decode()


def test_dw_descriptor_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or shutil.which("hipcc")
    assert cc, "no host compiler"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include "curv_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                     'sizeof(curv_persample_dw_desc), (size_t)&((curv_persample_dw_desc*)0)->N, '
                     '(size_t)&((curv_persample_dw_desc*)0)->dst, (size_t)&((curv_persample_dw_desc*)0)->o_stride); '
                     'return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-x", "c", "-I", os.path.join(root, "include"), str(probe), "-o", str(exe)], check=True)
    size, n, dst, o_stride = map(int, subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split())
    desc = _lib.curv_persample_dw_desc
    assert (ctypes.sizeof(desc), desc.N.offset, desc.dst.offset, desc.o_stride.offset) == (size, n, dst, o_stride)


def test_dw_jobs_refuse_cpu_tensors_and_wrong_shapes():
    x, g = torch.zeros(2, 3, 7, 6), torch.zeros(2, 3, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.per_sample_dw_sq_accumulate([ops.PerSampleDwJob(x, g, (3, 3), (2, 2), (1, 1), True, dst=torch.zeros(3, 10))])
    with pytest.raises(RuntimeError, match=r"\(N, C, H, W\)"):
        ops.per_sample_dw_plan_info([ops.PerSampleDwJob((2, 3, 7, 6), (2, 4, 4, 3), (3, 3))])
