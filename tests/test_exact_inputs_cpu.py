"""The exact-input technique of tests/exact_inputs.py, checked without a GPU: for one geometry of every kind of factor
build the integer Gram changes in at least one entry when a single element of the source is zeroed or doubled, one image
row is shifted by a pixel, or the last sample is dropped - the mutations a relative Frobenius bar of 1e-4 lets through.
Also the generators (no zero, the promised bit widths), the range guard, and that narrowing a 12-bit source to bf16, fp16
or 10 mantissa bits changes the rank-one Gram the GPU tests compare against."""
import math

import pytest
import torch
import torch.nn.functional as F

from exact_inputs import (assert_exact_range, conv_rows, exact_gram, flat_rows, nonzero_ints, pow2_scale, wide_ints)
from test_conv_nd_cpu import im2col3d
from test_conv_transpose_cpu import convt_patches


def plain_3x3(x):
    return exact_gram(conv_rows(x, 3, 1, 1), ones_row=True)


def strided_1x1(x):
    return exact_gram(conv_rows(x, 1, 2, 0))


def grouped(x, groups=3):
    cg = x.shape[1] // groups
    return torch.stack([exact_gram(conv_rows(x[:, k * cg:(k + 1) * cg], 3, 2, 1), ones_row=True) for k in range(groups)])


def transposed(x):
    layer = torch.nn.ConvTranspose2d(x.shape[1], 2, 3, 2, 1, 1)
    out = ((x.shape[2] - 1) * 2 - 2 + 3 + 1, (x.shape[3] - 1) * 2 - 2 + 3 + 1)
    return exact_gram(convt_patches(x, layer, out), ones_row=True)


def dilated(x):
    return exact_gram(conv_rows(x, 3, 1, 2, dilation=2), ones_row=True)


def three_d(x):
    return exact_gram(im2col3d(x.double(), (3, 3, 3), (1, 1, 1), (1, 1, 1)), ones_row=True)


def reduce_plane(x):
    """L^2 times the unscaled KFAC-reduce factor: the Gram of the per-sample SUMS over the output pixels, bias column L."""
    sums = F.unfold(x.double(), 3, padding=1).sum(2)                               # (N, dim), integers
    L = x.shape[2] * x.shape[3]
    return exact_gram(torch.cat([sums, torch.full((x.shape[0], 1), float(L), dtype=torch.float64)], dim=1).t())


# kind: (reference, source shape, index of a source element the factor reads)
KINDS = {
    "plain 3x3": (plain_3x3, (3, 4, 6, 7), (2, 3, 5, 6)),
    "strided 1x1": (strided_1x1, (3, 5, 9, 9), (2, 4, 8, 8)),                  # stride 2 samples the even rows / columns
    "grouped": (grouped, (2, 6, 7, 8), (1, 5, 6, 6)),
    "transposed": (transposed, (2, 3, 4, 5), (1, 2, 3, 4)),
    "dilated": (dilated, (2, 3, 7, 9), (1, 2, 6, 8)),
    "3-D": (three_d, (2, 2, 4, 5, 6), (1, 1, 3, 4, 5)),
    "reduce": (reduce_plane, (4, 3, 8, 8), (3, 2, 7, 7)),
}


def source(kind):
    gen = torch.Generator().manual_seed(sum(map(ord, kind)))
    return nonzero_ints(KINDS[kind][1], gen)


def zeroed(x, at):
    y = x.clone()
    y[at] = 0
    return y


def doubled(x, at):
    y = x.clone()
    y[at] *= 2
    return y


def row_shifted(x, at):
    """The image row that holds `at`, rotated by one pixel."""
    y = x.clone()
    y[at[:-1]] = x[at[:-1]].roll(1)
    assert not torch.equal(y, x)
    return y


def last_sample_dropped(x, at):
    return x[:-1]


MUTATIONS = {"one element zeroed": zeroed, "one element doubled": doubled, "one row shifted": row_shifted,
             "last sample dropped": last_sample_dropped}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_the_exact_reference_detects_a_single_mutation(kind, mutation):
    reference, shape, at = KINDS[kind]
    x = source(kind)
    want = reference(x)
    assert torch.equal(want, reference(x.clone()))
    assert torch.equal(want, want.transpose(-1, -2))
    got = reference(MUTATIONS[mutation](x, at))
    assert got.shape == want.shape
    changed = int((got != want).sum())
    print(f"{kind}, {mutation}: {changed} of {want.numel()} entries differ")
    assert changed >= 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_nonzero_ints_never_emits_zero(dtype):
    gen = torch.Generator().manual_seed(1)
    v = nonzero_ints((100000,), gen, dtype)
    assert v.dtype == dtype
    assert sorted(set(v.double().tolist())) == [-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]


@pytest.mark.parametrize("bits", [8, 12])
def test_wide_ints_fill_exactly_that_many_bits(bits):
    gen = torch.Generator().manual_seed(2)
    v = wide_ints((100000,), gen, bits).double()
    mag = v.abs()
    assert bool((mag == mag.round()).all()) and bool((mag % 2 == 1).all())
    assert float(mag.min()) > 2 ** (bits - 1) and float(mag.max()) < 2 ** bits
    assert float(mag.max()) == 2 ** bits - 1 and bool((v < 0).any()) and bool((v > 0).any())
    if bits == 8:                                     # exact in both half-precision formats
        f = v.float()
        assert torch.equal(f.bfloat16().float(), f) and torch.equal(f.half().float(), f)


def test_the_range_guard():
    assert assert_exact_range(3, 25088) == 451584          # the largest N L of the case tables, accumulated twice
    assert_exact_range(255, 128)                           # 8-bit sources, 128 terms per entry
    assert_exact_range(4095, 1, rounds=1)                  # one 24-bit product
    with pytest.raises(AssertionError, match="not exact in float32"):
        assert_exact_range(3, 2 ** 20)
    with pytest.raises(AssertionError, match="not exact in float32"):
        assert_exact_range(4095, 1)                        # a rank-one 12-bit Gram cannot be accumulated twice
    with pytest.raises(AssertionError, match="not exact in float32"):
        assert_exact_range(255, 130)


def test_pow2_scale():
    for terms in (1, 2, 3, 49, 64, 196, 25088, 100352):
        s = pow2_scale(terms)
        assert math.frexp(s)[0] == 0.5 and s <= 1.0 / terms < 2 * s


@pytest.mark.parametrize("width", [70, 513])
def test_a_narrowed_operand_changes_the_rank_one_gram(width):
    """N = 1: every entry of the Gram is a single product of two 12-bit integers - 24 bits, exact in float32 - and a source
    rounded to bf16 (8 significant bits), fp16 (11) or 10 mantissa bits (tf32-like) gives another matrix."""
    gen = torch.Generator().manual_seed(width)
    x = wide_ints((1, width), gen, 12)
    want = exact_gram(flat_rows(x))
    assert torch.equal((x.t() @ x).double(), want)                                # the float32 product is the exact one
    ten_bits = (x.view(torch.int32) + (1 << 12) & ~((1 << 13) - 1)).view(torch.float32)   # round to 10 mantissa bits
    for name, narrowed in (("bf16", x.bfloat16().float()), ("fp16", x.half().float()), ("10 mantissa bits", ten_bits)):
        assert not torch.equal(narrowed, x), name
        assert float((narrowed - x).abs().max() / x.abs().max()) < 2.0 ** -8, name         # (a rounding, not garbage)
        assert not torch.equal(exact_gram(flat_rows(narrowed)), want), name


def test_half_sources_need_float32_accumulation():
    """128 products of 8-bit integers: the sum is exact in float32 and is not what a half-precision accumulator holds."""
    gen = torch.Generator().manual_seed(5)
    x = wide_ints((128, 40), gen, 8)
    assert_exact_range(255, 128)
    want = exact_gram(flat_rows(x))
    assert torch.equal(want.float().double(), want)
    for dtype in (torch.bfloat16, torch.float16):
        assert not torch.equal(want.to(dtype).double(), want), dtype
