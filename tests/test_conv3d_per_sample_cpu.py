"""The per-sample line of a Conv3d without a GPU: the `ops.admit_conv3d_per_sample` switch (off: every
refusal as before; alone it admits nothing), what `ops.per_sample_operands` makes of 5-D records (sizes, strides, scratch,
the in-place decisions, the 2^31-byte refusal), the descriptor `ops._fill_pack` writes, the ABI of curv_persample_pack3d
and the host-only refusals of its planner."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from curvature_amd import _lib, ops
from curvature_amd.curvatures import KFAC, Diagonal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OLD_LAYERS_TEXT = "a 3-D convolution: a sample's product sums over the output depths"


def model3d():
    return torch.nn.Sequential(torch.nn.Conv3d(2, 4, 3, padding=1), torch.nn.ReLU(),
                               torch.nn.Conv3d(4, 4, (1, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1)), torch.nn.Flatten(),
                               torch.nn.Linear(4 * 4 * 3 * 3, 5))


@pytest.fixture
def nd():
    was = ops.admit_conv_nd(True)
    yield
    ops.admit_conv_nd(was)


@pytest.fixture
def both(nd):
    was = ops.admit_conv3d_per_sample(True)
    yield
    ops.admit_conv3d_per_sample(was)


def geometry(op):
    return (op.rows, op.L, op.Lp, op.ns, op.rs, op.floats)


# ------------------------------------------------------------------------------------------------ the switch
def test_the_switch_is_off_by_default_and_returns_what_it_was():
    assert ops.conv3d_per_sample_admitted() is False
    assert ops.admit_conv3d_per_sample() is False and ops.conv3d_per_sample_admitted() is True
    assert ops.admit_conv3d_per_sample(False) is True and ops.conv3d_per_sample_admitted() is False
    assert ops.admit_conv3d_per_sample(False) is False


def test_alone_it_admits_nothing():
    assert ops.conv_nd_admitted() is False
    def outcome():
        try:
            return ops.per_sample_operands(model3d()[0], torch.zeros(1, 2, 4, 6, 6), torch.zeros(1, 4, 4, 6, 6))
        except Exception as exc:                                              # whatever it is without either switch
            return type(exc), str(exc)
    before = outcome()
    assert isinstance(before, tuple) and issubclass(before[0], Exception)
    was = ops.admit_conv3d_per_sample(True)
    try:
        with pytest.raises(AssertionError):                                   # a Conv3d cannot be selected
            Diagonal(model3d(), ['Conv3d'], per_sample=True)
        assert outcome() == before
    finally:
        ops.admit_conv3d_per_sample(was)


def test_off_the_refusals_read_as_before(nd):
    model = model3d()
    for make in (lambda: Diagonal(model, ['Conv3d'], per_sample=True), lambda: Diagonal(model, ['Linear', 'Conv3d'], per_sample=True)):
        with pytest.raises(NotImplementedError) as err:
            make()
        text = str(err.value)
        assert "'0'" in text and OLD_LAYERS_TEXT in text and "which the per-sample kernels would square one by one" in text
        assert text.endswith("select other layer types or use per_sample=False")
    kfac = KFAC(model, ['Conv3d', 'Linear'])
    with pytest.raises(NotImplementedError, match="3-D convolution.*KFAC, Diagonal, EFB and INF"):
        kfac._per_sample_layers("KFAC.functional_variance", "advice")
    with pytest.raises(NotImplementedError, match="^per-sample update: unsupported layer Conv3d$"):
        ops.per_sample_operands(model[0], torch.zeros(1, 2, 4, 6, 6), torch.zeros(1, 4, 4, 6, 6))


def test_on_the_estimators_select_a_conv3d(both):
    model = model3d()
    assert len(Diagonal(model, ['Conv3d', 'Linear'], per_sample=True).record) == 3
    kfac = KFAC(model, ['Conv3d', 'Linear'])
    assert kfac._per_sample_layers("KFAC.functional_variance", "advice") == [model[0], model[2], model[4]]
    # what stays refused: the reduce approximation, dilation, groups
    with pytest.raises(NotImplementedError, match="3-D convolution"):
        KFAC(model, ['Conv3d', 'Linear'], approximation="reduce")
    for bad in (torch.nn.Conv3d(2, 4, 3, dilation=2), torch.nn.Conv3d(4, 4, 3, groups=2)):
        with pytest.raises(NotImplementedError):
            Diagonal(torch.nn.Sequential(bad), ['Conv3d'], per_sample=True)
    with pytest.raises((AssertionError, NotImplementedError)):
        Diagonal(torch.nn.Sequential(torch.nn.ConvTranspose3d(2, 2, 3)), ['ConvTranspose3d'], per_sample=True)


# ------------------------------------------------------------------------------------------------ operands
def sides_of(shape, cout, kernel, stride=1, padding=0, bias=False, **layout):
    conv = torch.nn.Conv3d(shape[1], cout, kernel, stride=stride, padding=padding, bias=bias)
    x = torch.zeros(shape)
    with torch.no_grad():
        g = torch.zeros_like(conv(x))
    return ops.per_sample_operands(conv, x, g, **layout), x, g


def test_case_1_is_packed_on_both_sides(both):
    s, x, g = sides_of((2, 3, 5, 6, 7), 4, 3, 1, 1, bias=True)                 # L = 210, Lp = 212
    assert (s.N, s.m, s.n, s.L) == (2, 4, 82, 210)
    assert geometry(s.x) == (82, 210, 212, 82 * 212, 212, 2 * 82 * 212)
    assert geometry(s.g) == (4, 210, 212, 4 * 212, 212, 2 * 4 * 212)          # L % 4 = 2: packed, with a zero tail
    assert s.x.pack == ops.PackSource((2, 3, 5, 6, 7), (3, 3, 3), (1, 1, 1), (1, 1, 1), True, (630, 210, 42, 7, 1), None, (1, 1))
    assert s.g.pack == ops.PackSource((2, 4, 5, 6, 7), (1, 1, 1), (1, 1, 1), (0, 0, 0), False, (840, 210, 42, 7, 1), None, (1, 1))
    assert s.x.src.data_ptr() == x.data_ptr() and s.g.src.data_ptr() == g.data_ptr()
    assert not s.x.rows_outer and not s.g.rows_outer
    s, _, _ = sides_of((2, 3, 5, 6, 7), 4, 3, 1, 1, bias=True, rows_outer=True, in_place=False)
    assert geometry(s.x) == (82, 210, 212, 212, 2 * 212, 2 * 82 * 212) and s.x.rows_outer
    assert geometry(s.g) == (4, 210, 212, 212, 2 * 212, 2 * 4 * 212) and s.g.rows_outer


def test_case_3_reads_g_in_place(both):
    s, x, g = sides_of((3, 4, 4, 6, 6), 5, (1, 3, 3), (1, 2, 2), (0, 1, 1))    # output 4 x 3 x 3: L = 36
    assert (s.N, s.m, s.n, s.L) == (3, 5, 36, 36)
    assert s.g.pack is None and geometry(s.g) == (5, 36, 36, 5 * 36, 36, 0) and s.g.src is not None
    assert s.g.src.data_ptr() == g.data_ptr()
    assert geometry(s.x) == (36, 36, 36, 36 * 36, 36, 3 * 36 * 36)
    assert s.x.pack.kernel == (1, 3, 3) and s.x.pack.stride == (1, 2, 2) and s.x.pack.padding == (0, 1, 1)
    assert s.x.pack.shape == (3, 4, 4, 6, 6) and s.x.pack.strides == (576, 144, 36, 6, 1) and not s.x.pack.has_bias
    s, _, _ = sides_of((3, 4, 4, 6, 6), 5, (1, 3, 3), (1, 2, 2), (0, 1, 1), rows_outer=True, in_place=False)
    assert s.g.pack is not None and geometry(s.g) == (5, 36, 36, 36, 3 * 36, 3 * 5 * 36)


def test_case_8_reads_both_sides_in_place(both):
    s, x, g = sides_of((2, 8, 3, 4, 4), 6, 1)                                  # bias-free 1x1x1: L = 48
    assert (s.N, s.m, s.n, s.L) == (2, 6, 8, 48)
    assert s.x.pack is None and geometry(s.x) == (8, 48, 48, 8 * 48, 48, 0) and s.x.src.data_ptr() == x.data_ptr()
    assert s.g.pack is None and geometry(s.g) == (6, 48, 48, 6 * 48, 48, 0)
    s, _, _ = sides_of((2, 8, 3, 4, 4), 6, 1, bias=True)                       # the ones row has to be written
    assert s.x.pack is not None and geometry(s.x) == (9, 48, 48, 9 * 48, 48, 2 * 9 * 48) and s.g.pack is None
    s, _, _ = sides_of((2, 8, 4, 6, 6), 6, 1, 2)                               # case 9: strided, L = 18
    assert s.x.pack is not None and s.g.pack is not None and geometry(s.x) == (8, 18, 20, 8 * 20, 20, 2 * 8 * 20)


def test_views_are_packed_and_not_copied(both):
    conv = torch.nn.Conv3d(8, 6, 1, bias=False)
    x = torch.zeros(2, 8, 3, 4, 4).contiguous(memory_format=torch.channels_last_3d)
    g = torch.zeros(2, 6, 3, 4, 4).contiguous(memory_format=torch.channels_last_3d)
    s = ops.per_sample_operands(conv, x, g)
    assert s.x.pack is not None and s.x.src.data_ptr() == x.data_ptr() and s.x.pack.strides == (384, 1, 128, 32, 8)
    assert s.g.pack is not None and s.g.src.data_ptr() == g.data_ptr() and s.g.pack.strides == (288, 1, 96, 24, 6)
    wide = torch.zeros(2, 12, 3, 4, 4)
    s = ops.per_sample_operands(conv, wide[:, 2:10], torch.zeros(2, 6, 3, 4, 4))    # a channel slice
    assert s.x.pack is not None and s.x.pack.strides == (12 * 48, 48, 16, 4, 1) and s.x.pack.shape == (2, 8, 3, 4, 4)
    assert s.x.src.data_ptr() == wide[:, 2:10].data_ptr() and s.g.pack is None


def test_half_records_need_the_wider_line(both):
    conv = torch.nn.Conv3d(8, 6, 1, bias=False)
    x, g = torch.zeros(2, 8, 3, 4, 4), torch.zeros(2, 6, 3, 4, 4, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="widen_per_sample"):
        ops.per_sample_operands(conv, x, g)
    was = ops.widen_per_sample(True)
    try:
        s = ops.per_sample_operands(conv, x, g)
        assert s.x.pack is None and s.g.pack is not None and s.g.src.dtype == torch.bfloat16     # a half side is packed
    finally:
        ops.widen_per_sample(was)


def test_fill_pack_writes_the_3d_descriptor(both):
    s, x, g = sides_of((2, 3, 5, 6, 7), 4, 3, (2, 1, 1), (1, 0, 1), bias=True, rows_outer=True, in_place=False)
    d = _lib.curv_persample_pack3d_desc()
    dst = torch.zeros(s.x.floats)
    ops._fill_pack(d, s.x, dst)
    assert (d.src, d.dst) == (x.data_ptr(), dst.data_ptr()) and d.reserved == 0
    assert (d.N, d.C, d.D, d.H, d.W) == (2, 3, 5, 6, 7) and (d.s_n, d.s_c, d.s_d, d.s_h, d.s_w) == (630, 210, 42, 7, 1)
    assert (d.kd, d.kh, d.kw, d.sd, d.sh, d.sw, d.pd, d.ph, d.pw) == (3, 3, 3, 2, 1, 1, 1, 0, 1)
    assert (d.has_bias, d.dtype, d.rows_outer, d.Lp, d.src_elems) == (1, _lib.DTYPE_F32, 1, s.x.Lp, 1260)
    assert s.x.L == 3 * 4 * 7 and s.x.Lp == 84


def test_an_operand_of_two_gib_is_refused_with_the_batch_that_fits(both):
    conv = torch.nn.Conv3d(32, 8, 3, padding=1)
    shape, gshape = (2, 32, 32, 64, 64), (2, 8, 32, 64, 64)                    # rows 865, L = 131072: 2 x 453 MB fits
    x, g = torch.empty(shape, device="meta"), torch.empty(gshape, device="meta")
    s = ops.per_sample_operands(conv, x, g)
    assert (s.x.rows, s.x.L, s.N) == (865, 131072, 2)
    x, g = torch.empty((5,) + shape[1:], device="meta"), torch.empty((5,) + gshape[1:], device="meta")
    with pytest.raises(RuntimeError) as err:
        ops.per_sample_operands(conv, x, g)
    text = str(err.value)
    assert "x operand of Conv3d" in text and "N 5 x rows 865 x Lp 131072" in text and "2^31" in text
    assert f"{5 * 865 * 131072 * 4} bytes" in text and "the largest batch that fits is 4" in text


def test_records_of_the_wrong_rank_are_refused(both):
    conv = torch.nn.Conv3d(2, 4, 3, padding=1)
    for x, g in ((torch.zeros(2, 2, 6, 6), torch.zeros(2, 4, 4, 6, 6)), (torch.zeros(2, 2, 4, 6, 6), torch.zeros(2, 4, 24, 6)),
                 (torch.zeros(2, 2, 4, 6, 6, 1), torch.zeros(2, 4, 4, 6, 6))):
        with pytest.raises(RuntimeError, match=r"records of Conv3d must be \(N, C, D, H, W\)"):
            ops.per_sample_operands(conv, x, g)
    with pytest.raises(RuntimeError, match="do not match the layer"):
        ops.per_sample_operands(conv, torch.zeros(2, 2, 4, 6, 6), torch.zeros(2, 4, 4, 6, 5))


# ------------------------------------------------------------------------------------------------ ABI
def test_pack3d_is_declared_bound_and_additive():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "curv_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+curv_persample_pack3d\s*\(", header)
    assert "curv_persample_pack3d" in _lib.SIGNATURES
    handle = _lib.lib()
    assert hasattr(handle, "curv_persample_pack3d")
    assert handle.curv_version() == 12 == _lib.ABI_VERSION                     # a symbol was added, nothing else
    assert handle.curv_persample_pack3d(None, None, 0) == 0                    # an empty call is a no-op
    assert handle.curv_persample_pack3d(None, None, 1) == _lib.ERR_INVALID
    assert b"curv_persample_pack3d: null descriptors" in handle.curv_last_error()


def test_descriptor_size_and_offsets_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or shutil.which("hipcc")
    assert cc, "no host compiler"
    fields = [name for name, _ in _lib.curv_persample_pack3d_desc._fields_]
    assert fields == ["src", "dst", "s_n", "s_c", "s_d", "s_h", "s_w", "src_elems", "N", "C", "D", "H", "W", "kd", "kh", "kw",
                      "sd", "sh", "sw", "pd", "ph", "pw", "has_bias", "dtype", "rows_outer", "Lp", "reserved"]
    offsets = ", ".join(f"offsetof(curv_persample_pack3d_desc, {f})" for f in fields)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "curv_hip.h"\nint main(void) { size_t v[] = {'
                     f'sizeof(curv_persample_pack3d_desc), sizeof(curv_persample_pack_ex_desc), {offsets}}};\n'
                     'for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%zu ", v[i]); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    size, ex, *offs = map(int, subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split())
    assert ctypes.sizeof(_lib.curv_persample_pack3d_desc) == size == 144
    assert ctypes.sizeof(_lib.curv_persample_pack_ex_desc) == ex               # the 2-D descriptor is what it was
    assert [getattr(_lib.curv_persample_pack3d_desc, f).offset for f in fields] == offs


# ------------------------------------------------------------------------------------------------ host-only plan refusals
def desc(**fields):
    """Case 1 with null pointers (the planner sees the sizes first), edited."""
    arr = (_lib.curv_persample_pack3d_desc * 1)()
    d = arr[0]
    d.N, d.C, d.D, d.H, d.W = 2, 3, 5, 6, 7
    d.s_n, d.s_c, d.s_d, d.s_h, d.s_w = 630, 210, 42, 7, 1
    d.src_elems = 1260
    d.kd = d.kh = d.kw = 3
    d.sd = d.sh = d.sw = 1
    d.pd = d.ph = d.pw = 1
    d.has_bias, d.Lp = 1, 212
    for key, value in fields.items():
        setattr(d, key, value)
    return arr


PLAN_REFUSALS = [
    ("null src or dst", dict()),                                              # every size is fine: the addresses are next
    ("unknown dtype 7", dict(dtype=7)),
    ("reserved is 1, must be 0", dict(reserved=1)),
    ("invalid geometry", dict(D=0)),
    ("invalid geometry", dict(kd=0)),
    ("invalid geometry", dict(sd=0)),
    ("invalid geometry", dict(pd=-1)),
    ("invalid geometry", dict(W=0)),
    ("kernel larger than the padded input", dict(kd=8)),
    ("kernel larger than the padded input", dict(kh=9)),
    ("kernel larger than the padded input", dict(kw=10)),
    ("negative stride", dict(s_d=-42)),
    ("negative stride, or source extent 0 elements below 1", dict(src_elems=0)),
    ("too large (16777233 rows", dict(C=(1 << 24) // 27 + 1, s_c=0)),
    ("too large", dict(s_d=1 << 31)),                                         # the sample span
    ("too large", dict(D=1 << 12, H=1 << 7, W=1 << 7, s_d=0, s_h=0, s_w=0, Lp=1 << 26)),   # 2^26 positions
    ("too large", dict(N=1 << 20, s_n=0)),                                    # 2^31 threads or more
    ("Lp 208 must be a multiple of 4 and at least L = 210", dict(Lp=208)),
    ("Lp 214 must be a multiple of 4", dict(Lp=214)),
    ("source extent (1259 elements) is smaller", dict(src_elems=1259)),
    ("source extent", dict(s_d=43)),
]


@pytest.mark.parametrize("text,fields", PLAN_REFUSALS, ids=[f"{k}_{t.split()[0]}" for k, (t, _) in enumerate(PLAN_REFUSALS)])
def test_plan_refusals_are_host_only(text, fields):
    handle = _lib.lib()
    assert handle.curv_persample_pack3d(None, desc(**fields), 1) == _lib.ERR_INVALID
    message = handle.curv_last_error().decode()
    assert message.startswith("curv_persample_pack3d: item 0: ") and text in message, message


def test_the_geometry_is_named_with_its_depth():
    handle = _lib.lib()
    assert handle.curv_persample_pack3d(None, desc(kd=8), 1) == _lib.ERR_INVALID
    assert handle.curv_last_error().decode() == \
        "curv_persample_pack3d: item 0: kernel larger than the padded input (N 2 C 3 D 5 H 6 W 7 kernel 8x3x3 stride " \
        "1x1x1 padding 1x1x1)"
    # addresses after sizes: a misaligned dst, then a misaligned src
    assert handle.curv_persample_pack3d(None, desc(src=64, dst=72), 1) == _lib.ERR_INVALID
    assert b"dst is not 16-byte aligned" in handle.curv_last_error()
    assert handle.curv_persample_pack3d(None, desc(src=66, dst=64), 1) == _lib.ERR_INVALID
    assert b"src is not aligned to its 4-byte elements" in handle.curv_last_error()


def test_the_2d_entry_points_keep_their_messages():
    """Adapters over the same planner: the texts of the two 2-D forms are what they were."""
    handle = _lib.lib()
    arr = (_lib.curv_persample_pack_ex_desc * 1)()
    d = arr[0]
    d.N, d.C, d.H, d.W, d.kh, d.kw, d.sh, d.sw, d.ph, d.pw = 2, 3, 5, 6, 9, 3, 1, 1, 1, 1
    d.s_n, d.s_c, d.s_h, d.s_w, d.src_elems, d.Lp = 90, 30, 6, 1, 180, 32
    assert handle.curv_persample_pack_ex(None, arr, 1) == _lib.ERR_INVALID
    assert handle.curv_last_error().decode() == \
        "curv_persample_pack_ex: item 0: kernel larger than the padded input (N 2 C 3 H 5 W 6 kernel 9x3 stride 1x1 padding 1x1)"
    d.kh, d.src_elems = 3, 179
    assert handle.curv_persample_pack_ex(None, arr, 1) == _lib.ERR_INVALID    # the addresses before the extent, as before
    assert handle.curv_last_error().decode() == "curv_persample_pack_ex: item 0: null src or dst"
    old = (_lib.curv_persample_pack_desc * 1)()
    o = old[0]
    o.N, o.C, o.H, o.W, o.kh, o.kw, o.sh, o.sw, o.Lp = 2, 3, 5, 6, 1, 1, 1, 1, 32
    assert handle.curv_persample_pack(None, old, 1) == _lib.ERR_INVALID
    assert handle.curv_last_error().decode() == "curv_persample_pack: item 0: null src or dst, or dst not 16-byte aligned"
