"""The per-sample operand step for half-precision records, ConvTranspose2d and attention projections, without a GPU:
the ABI of curv_persample_pack_ex, what `ops.per_sample_operands` makes of each kind of record (sizes, strides and
scratch), the descriptor `ops._fill_pack` writes, the shapes the attention tap records, and the refusals that stay.  The wider line is
opt-in (`ops.widen_per_sample`): every test here runs with it on, except the one that checks what off means."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from curvature_amd import _lib, ops
from curvature_amd.curvatures import EFB, KFAC, AttentionProjection, Diagonal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def wide():
    was = ops.widen_per_sample(True)
    yield
    ops.widen_per_sample(was)


def geometry(op):
    return (op.rows, op.L, op.Lp, op.ns, op.rs, op.floats)


# ------------------------------------------------------------------------------------------------ ABI
def test_pack_ex_is_declared_bound_and_additive():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "curv_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+curv_persample_pack_ex\s*\(", header)
    assert "curv_persample_pack_ex" in _lib.SIGNATURES and "curv_persample_pack" in _lib.SIGNATURES
    handle = _lib.lib()
    assert hasattr(handle, "curv_persample_pack_ex")
    assert handle.curv_version() == 12 == _lib.ABI_VERSION
    assert (_lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_F16) == (0, 1, 2)
    assert handle.curv_persample_pack_ex(None, None, 0) == 0                  # an empty call is a no-op


def test_descriptor_sizes_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or shutil.which("hipcc")
    assert cc, "no host compiler"
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include "curv_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                     'sizeof(curv_persample_pack_ex_desc), sizeof(curv_persample_pack_desc), '
                     '(size_t)&((curv_persample_pack_ex_desc*)0)->Lp); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    ex, old, lp = map(int, subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split())
    assert ctypes.sizeof(_lib.curv_persample_pack_ex_desc) == ex
    assert ctypes.sizeof(_lib.curv_persample_pack_desc) == old == 72          # the old descriptor, byte for byte
    assert _lib.curv_persample_pack_ex_desc.Lp.offset == lp


# ------------------------------------------------------------------------------------------------ operands
def test_conv2d_fp32_is_what_it_was():
    """The values of the float32 line before it was widened (hard-coded)."""
    conv = torch.nn.Conv2d(8, 16, 1, bias=False)
    s = ops.per_sample_operands(conv, torch.zeros(2, 8, 4, 4), torch.zeros(2, 16, 4, 4))
    assert (s.N, s.m, s.n, s.L) == (2, 16, 8, 16)
    assert s.g.pack is None and geometry(s.g) == (16, 16, 16, 256, 16, 0)
    assert s.x.pack is None and geometry(s.x) == (8, 16, 16, 128, 16, 0)
    conv = torch.nn.Conv2d(8, 16, 3, padding=1)
    s = ops.per_sample_operands(conv, torch.zeros(2, 8, 7, 7), torch.zeros(2, 16, 7, 7))
    assert (s.N, s.m, s.n, s.L) == (2, 16, 73, 49)
    assert geometry(s.g) == (16, 49, 52, 16 * 52, 52, 2 * 16 * 52)
    assert geometry(s.x) == (73, 49, 52, 73 * 52, 52, 2 * 73 * 52)
    assert s.g.pack.strides == (16 * 49, 49, 7, 1) and s.x.pack.strides == (8 * 49, 49, 7, 1)
    s = ops.per_sample_operands(conv, torch.zeros(2, 8, 7, 7), torch.zeros(2, 16, 7, 7), rows_outer=True, in_place=False)
    assert geometry(s.g) == (16, 49, 52, 52, 104, 2 * 16 * 52) and geometry(s.x) == (73, 49, 52, 52, 104, 2 * 73 * 52)
    lin = torch.nn.Linear(5, 3)
    s = ops.per_sample_operands(lin, torch.zeros(4, 7, 5), torch.zeros(4, 7, 3))
    assert (s.N, s.m, s.n, s.L) == (4, 3, 6, 7)
    assert geometry(s.x) == (6, 7, 8, 48, 8, 4 * 6 * 8) and geometry(s.g) == (3, 7, 8, 24, 8, 4 * 3 * 8)
    assert s.x.pack.strides == (7 * 5, 1, 5, 1) and s.g.pack.strides == (7 * 3, 1, 3, 1)     # (N, H, W, C): (HWC, 1, WC, C)
    s = ops.per_sample_operands(lin, torch.zeros(4, 5), torch.zeros(4, 3))
    assert (s.N, s.m, s.n, s.L) == (4, 3, 6, 1) and geometry(s.x) == (6, 1, 4, 24, 4, 4 * 6 * 4)
    assert s.x.pack.strides == (5, 1, 5, 1) and s.g.pack.strides == (3, 1, 3, 1)              # (N, H, W, C) with H = W = 1
    s = ops.per_sample_operands(lin, torch.zeros(4, 5), torch.zeros(4, 3))
    assert (s.N, s.m, s.n, s.L) == (4, 3, 6, 1) and geometry(s.x) == (6, 1, 4, 24, 4, 4 * 6 * 4)
    assert s.x.pack.strides == (5, 1, 5, 1) and s.g.pack.strides == (3, 1, 3, 1)              # (N, H, W, C) with H = W = 1


@pytest.mark.parametrize("half", [torch.bfloat16, torch.float16])
def test_a_half_side_is_packed_where_fp32_is_read_in_place(half):
    conv = torch.nn.Conv2d(8, 16, 1, bias=False)
    x, g = torch.zeros(2, 8, 4, 4), torch.zeros(2, 16, 4, 4)
    s = ops.per_sample_operands(conv, x, g.to(half))                          # the stem of an autocast model
    assert s.x.pack is None and geometry(s.x) == (8, 16, 16, 128, 16, 0)
    assert s.g.pack is not None and geometry(s.g) == (16, 16, 16, 256, 16, 2 * 16 * 16) and s.g.src.dtype == half
    s = ops.per_sample_operands(conv, x.to(half), g)
    assert s.g.pack is None and s.x.pack is not None and s.x.src.dtype == half
    assert geometry(s.x) == (8, 16, 16, 128, 16, 2 * 8 * 16)


def test_views_are_not_copied():
    conv = torch.nn.Conv2d(8, 16, 1, bias=False)
    x = torch.zeros(2, 4, 4, 8).permute(0, 3, 1, 2)                           # channels-last memory
    g = torch.zeros(2, 16, 4, 8)[:, :, :, ::2]
    s = ops.per_sample_operands(conv, x, g)
    assert s.x.src.data_ptr() == x.data_ptr() and s.x.pack.strides == (128, 1, 32, 8)   # (HWC, 1, WC, C)
    assert s.g.src.data_ptr() == g.data_ptr() and s.g.pack.strides == (512, 32, 8, 2)  # neither layout's
    assert geometry(s.g) == (16, 16, 16, 256, 16, 512)


def filled(op):
    """Every field of the curv_persample_pack_ex_desc `ops._fill_pack` writes for `op`, but the two addresses."""
    d = _lib.curv_persample_pack_ex_desc()
    dst = torch.zeros(op.floats)
    ops._fill_pack(d, op, dst)
    assert (d.src, d.dst) == (op.src.data_ptr(), dst.data_ptr()) and d.reserved == 0
    return dict(shape=(d.N, d.C, d.H, d.W), strides=(d.s_n, d.s_c, d.s_h, d.s_w), src_elems=d.src_elems, dtype=d.dtype,
                window=(d.kh, d.kw, d.sh, d.sw, d.ph, d.pw), has_bias=d.has_bias, transposed=d.transposed,
                out=(d.Ho, d.Wo), Lp=d.Lp, rows_outer=d.rows_outer)


def test_fill_pack_writes_every_field():
    conv = torch.nn.Conv2d(8, 16, 3, padding=1)
    s = ops.per_sample_operands(conv, torch.zeros(2, 8, 7, 7), torch.zeros(2, 16, 7, 7))
    assert filled(s.x) == dict(shape=(2, 8, 7, 7), strides=(392, 49, 7, 1), src_elems=784, dtype=_lib.DTYPE_F32,
                               window=(3, 3, 1, 1, 1, 1), has_bias=1, transposed=0, out=(0, 0), Lp=52, rows_outer=0)
    lin = torch.nn.Linear(5, 3)
    s = ops.per_sample_operands(lin, torch.zeros(4, 7, 5), torch.zeros(4, 7, 3), rows_outer=True, in_place=False)
    assert filled(s.x) == dict(shape=(4, 5, 7, 1), strides=(35, 1, 5, 1), src_elems=140, dtype=_lib.DTYPE_F32,
                               window=(1, 1, 1, 1, 0, 0), has_bias=1, transposed=0, out=(0, 0), Lp=8, rows_outer=1)
    conv = torch.nn.Conv2d(8, 16, 1, bias=False)
    whole = torch.zeros(3, 16, 4, 4, dtype=torch.bfloat16)
    s = ops.per_sample_operands(conv, torch.zeros(2, 8, 4, 4), whole[1:])     # a view: the extent counts from its start
    assert filled(s.g) == dict(shape=(2, 16, 4, 4), strides=(256, 16, 4, 1), src_elems=512, dtype=_lib.DTYPE_BF16,
                               window=(1, 1, 1, 1, 0, 0), has_bias=0, transposed=0, out=(0, 0), Lp=16, rows_outer=0)
    convt = torch.nn.ConvTranspose2d(4, 3, 4, 2, 1)
    x = torch.zeros(2, 4, 5, 6)
    s = ops.per_sample_operands(convt, x, torch.zeros_like(convt(x)))
    assert filled(s.x) == dict(shape=(2, 4, 5, 6), strides=(120, 30, 6, 1), src_elems=240, dtype=_lib.DTYPE_F32,
                               window=(4, 4, 2, 2, 1, 1), has_bias=1, transposed=1, out=(10, 12), Lp=120, rows_outer=0)


CONVT = {
    # name: (layer, input H x W, output_size or None, expected Ho x Wo)
    "k4s2p1": (lambda: torch.nn.ConvTranspose2d(4, 3, 4, 2, 1), (5, 6), None, (10, 12)),
    "k2s2p0": (lambda: torch.nn.ConvTranspose2d(4, 3, 2, 2, 0), (4, 4), None, (8, 8)),
    "k3s2p1+1": (lambda: torch.nn.ConvTranspose2d(4, 3, 3, 2, 1), (5, 5), (10, 10), (10, 10)),
}


@pytest.mark.parametrize("name", sorted(CONVT))
def test_conv_transpose_operands(name):
    make, (H, W), output_size, (Ho, Wo) = CONVT[name]
    layer = make()
    x = torch.zeros(2, 4, H, W)
    out = layer(x, output_size=output_size)
    assert tuple(out.shape[2:]) == (Ho, Wo)
    g = torch.zeros_like(out)
    s = ops.per_sample_operands(layer, x, g)
    kh, kw = layer.kernel_size
    L = Ho * Wo
    assert (s.N, s.m, s.n, s.L) == (2, 3, 4 * kh * kw + 1, L) and L % 4 == 0
    assert s.g.pack is None and geometry(s.g) == (3, L, L, 3 * L, L, 0)       # fp32, whole 16-byte groups: in place
    assert geometry(s.x) == (s.n, L, L, s.n * L, L, 2 * s.n * L)
    assert s.x.pack.out_size == (Ho, Wo)
    s = ops.per_sample_operands(layer, x, g.bfloat16(), rows_outer=True, in_place=False)
    assert geometry(s.g) == (3, L, L, L, 2 * L, 2 * 3 * L) and s.g.src.dtype == torch.bfloat16
    assert geometry(s.x) == (s.n, L, L, L, 2 * L, 2 * s.n * L)


def test_attention_projection_operands():
    T, N, E = 5, 3, 8
    proj_in, proj_out = AttentionProjection.of(torch.nn.MultiheadAttention(E, 2))
    x, g = torch.zeros(T, N, E), torch.zeros(T, N, 3 * E)
    s = ops.per_sample_operands(proj_in, x, g)
    assert (s.N, s.m, s.n, s.L) == (N, 3 * E, E + 1, T)
    assert geometry(s.x) == (E + 1, T, 8, 9 * 8, 8, N * 9 * 8) and geometry(s.g) == (3 * E, T, 8, 24 * 8, 8, N * 24 * 8)
    assert s.x.pack.shape == (N, E, T, 1) and s.x.pack.strides[:3] == (E, 1, N * E)        # the sample is the middle index
    assert s.g.pack.shape == (N, 3 * E, T, 1) and s.g.pack.strides[:3] == (3 * E, 1, N * 3 * E)
    assert s.x.src.data_ptr() == x.data_ptr()
    x2, g2 = torch.zeros(T * N, E), torch.zeros(T * N, E)
    s = ops.per_sample_operands(proj_out, x2, g2, samples=N)
    assert (s.N, s.m, s.n, s.L) == (N, E, E + 1, T)
    assert s.x.pack.shape == (N, E, T, 1) and s.x.pack.strides[:3] == (E, 1, N * E) and s.x.src.data_ptr() == x2.data_ptr()
    assert geometry(s.g) == (E, T, 8, 8 * 8, 8, N * 8 * 8)
    with pytest.raises(RuntimeError, match="attn_out"):
        ops.per_sample_operands(proj_out, x2, g2, samples=4)                  # 15 rows are no 4 samples
    with pytest.raises(RuntimeError, match="attn_in.*unbatched"):
        ops.per_sample_operands(proj_in, torch.zeros(T, E), torch.zeros(T, 3 * E))


@pytest.mark.parametrize("batch_first", [False, True])
def test_the_tap_records_token_major(batch_first):
    """What `ops.per_sample_operands` is told about the records of the two projections holds for both layouts."""
    T, N, E = 5, 3, 8
    torch.manual_seed(0)
    model = torch.nn.Sequential()
    model.add_module("attn", torch.nn.MultiheadAttention(E, 2, batch_first=batch_first))
    proj_in, proj_out = AttentionProjection.of(model.attn)
    est = EFB(model, {}, ["MultiheadAttention"], eigvecs={proj_in: (None, None), proj_out: (None, None)}, per_sample=True)
    assert list(est.record) == [proj_in, proj_out]
    x = torch.randn(N, T, E) if batch_first else torch.randn(T, N, E)
    out, _ = model.attn(x, x, x)
    out.square().sum().backward()
    assert tuple(est.record[proj_in][0].shape) == (T, N, E) and tuple(est.record[proj_in][1].shape) == (T, N, 3 * E)
    assert tuple(est.record[proj_out][0].shape) == (T * N, E) and tuple(est.record[proj_out][1].shape) == (T * N, E)
    tokens = x.transpose(0, 1) if batch_first else x
    assert torch.equal(est.record[proj_in][0], tokens)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        est.update(N)
    import torch.nn.functional as F
    assert F.linear.__module__.startswith("torch")                            # the tap has left


# ------------------------------------------------------------------------------------------------ refusals that stay
def named(layer):
    model = torch.nn.Sequential()
    model.add_module("odd_one", layer)
    return model


@pytest.mark.parametrize("make,types,why", [
    (lambda: torch.nn.Conv2d(4, 4, 3, groups=2), ["Conv2d"], "odd_one.*grouped"),
    (lambda: torch.nn.Conv2d(4, 4, 3, dilation=2), ["Conv2d"], "odd_one.*dilated"),
    (lambda: torch.nn.Conv2d(4, 4, 3, padding="same"), ["Conv2d"], "odd_one.*string padding"),
    (lambda: torch.nn.MultiheadAttention(8, 2), ["MultiheadAttention"], "odd_one.*MultiheadAttention"),
], ids=["grouped", "dilated", "string-padding", "diagonal-mha"])
def test_refusals_are_still_named(make, types, why):
    model = named(make())
    with pytest.raises(NotImplementedError, match=why):
        Diagonal(model, types, per_sample=True)
    with pytest.raises(NotImplementedError, match=why):
        Diagonal(model, types)._per_sample_layers("Diagonal.functional_variance", "select other layer types")


def test_grouped_conv_transpose_is_refused():
    model = named(torch.nn.ConvTranspose2d(4, 4, 2, stride=2, groups=2))
    for make in (lambda: Diagonal(model, ["ConvTranspose2d"], per_sample=True),
                 lambda: EFB(model, {}, ["ConvTranspose2d"], eigvecs={}, per_sample=True),
                 lambda: KFAC(model, ["ConvTranspose2d"])):
        with pytest.raises(NotImplementedError, match="groups > 1"):
            make()


def test_admitted_layers():
    convt = named(torch.nn.ConvTranspose2d(4, 4, 2, stride=2))
    assert Diagonal(convt, ["ConvTranspose2d"], per_sample=True)._per_sample_layers("x", "y") == [convt.odd_one]
    assert list(EFB(convt, {}, ["ConvTranspose2d"], eigvecs={}, per_sample=True).record) == [convt.odd_one]
    mha = named(torch.nn.MultiheadAttention(8, 2))
    projections = list(AttentionProjection.of(mha.odd_one))
    assert KFAC(mha)._per_sample_layers("x", "y") == projections
    assert EFB(mha, {}, eigvecs={}, per_sample=True)._per_sample_layers("x", "y") == projections


def test_other_dtypes_are_refused():
    lin = torch.nn.Linear(5, 3)
    with pytest.raises(RuntimeError, match="float64"):
        ops.per_sample_operands(lin, torch.zeros(4, 5, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="float64"):
        ops.per_sample_operands(lin, torch.zeros(4, 5), torch.zeros(4, 3, dtype=torch.float64))


def test_off_by_default_everything_is_what_it_was():
    ops.widen_per_sample(False)
    assert not ops.per_sample_is_wide()
    conv = torch.nn.Conv2d(8, 16, 1, bias=False)
    with pytest.raises(RuntimeError, match=r"expects float32 records, got torch.bfloat16 \(ops.widen_per_sample"):
        ops.per_sample_operands(conv, torch.zeros(2, 8, 4, 4), torch.zeros(2, 16, 4, 4).bfloat16())
    with pytest.raises(RuntimeError, match="expects float32 records, got torch.float64$"):
        ops.per_sample_operands(conv, torch.zeros(2, 8, 4, 4), torch.zeros(2, 16, 4, 4).double())
    convt = named(torch.nn.ConvTranspose2d(4, 4, 2, stride=2))
    with pytest.raises(NotImplementedError, match="odd_one.*ConvTranspose2d"):
        Diagonal(convt, ["ConvTranspose2d"], per_sample=True)
    with pytest.raises(NotImplementedError, match="odd_one.*ConvTranspose2d"):
        KFAC(convt, ["ConvTranspose2d"])._per_sample_layers("KFAC.functional_variance", "select other layer types")
    mha = named(torch.nn.MultiheadAttention(8, 2))
    with pytest.raises(NotImplementedError, match="odd_one.*MultiheadAttention"):
        EFB(mha, {}, eigvecs={}, per_sample=True)
    assert ops.widen_per_sample(True) is False and ops.per_sample_is_wide()
