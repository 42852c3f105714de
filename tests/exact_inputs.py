"""Integer-valued inputs for which a Kronecker-factor build has one right answer, bit for bit.

If every value of a source is a small integer, every product x_i x_j and every partial sum of products is an integer
below 2^24: exact in float32 in ANY summation order - the fp32 MFMA, the bf16 / fp16 MFMA with fp32 accumulation, the
k-slice reduce, the shifted-correlation assembly.  With a power-of-two `scale` the factor is exact too, so a test is
``torch.equal`` against the integer Gram; one element left out or counted twice changes at least one entry.

`nonzero_ints` never emits zero (every element of a source then moves the result); `wide_ints` fills the significand
(12 bits: a 24-bit product, exact in float32 but not after the operand was narrowed to bf16 / fp16 / tf32; 8 bits: exact
in bf16 and fp16, and the sum of 128 products needs fp32 accumulation).  `assert_exact_range` is the range condition,
`exact_gram` the reference."""
import math

import torch

EXACT_LIMIT = 2 ** 24         # integers below it are float32 values


def nonzero_ints(shape, gen, dtype=torch.float32):
    """Values uniform in {-3, -2, -1, 1, 2, 3}."""
    shape = tuple(shape)
    magnitude = torch.randint(1, 4, shape, generator=gen)
    sign = 1 - 2 * torch.randint(0, 2, shape, generator=gen)
    return (magnitude * sign).to(dtype)


def wide_ints(shape, gen, bits, dtype=torch.float32):
    """Odd integers of either sign with exactly `bits` significant bits: 2^(bits-1) < |v| < 2^bits, bit 0 set."""
    assert 2 <= bits <= 12
    shape = tuple(shape)
    top = 1 << (bits - 1)
    magnitude = top + 1 + 2 * torch.randint(0, top // 2, shape, generator=gen)
    sign = 1 - 2 * torch.randint(0, 2, shape, generator=gen)
    return (magnitude * sign).to(dtype)


def pow2_scale(terms):
    """The largest power of two not above 1 / terms: what stands in for the 1 / (N L) of a factor."""
    return 2.0 ** -math.ceil(math.log2(terms))


def assert_exact_range(max_abs, terms, rounds=2):
    """Every entry of `rounds` accumulated Grams of `terms` products of values up to `max_abs` stays below 2^24."""
    bound = rounds * terms * max_abs ** 2
    assert bound < EXACT_LIMIT, f"{rounds} x {terms} products of values up to {max_abs}: {bound} >= 2^24, not exact in float32"
    return bound


def exact_gram(rows, ones_row=False):
    """rows rows^T in float64 of integer-valued `rows` (dim, K) [+ a row of ones], on the device that holds them.  Exact
    wherever it runs and in any order: every sum is an integer below 2^53."""
    rows = rows.double()
    assert bool((rows == rows.round()).all())
    if ones_row:
        rows = torch.cat([rows, torch.ones(1, rows.shape[1], dtype=rows.dtype, device=rows.device)])
    gram = rows @ rows.t()
    assert float(gram.abs().max()) < 2 ** 53
    return gram


def conv_rows(x, kernel, stride=1, padding=0, dilation=1):
    """(C kh kw, N L) columns of ``F.unfold`` in float64, on the device of `x`."""
    cols = torch.nn.functional.unfold(x.double(), kernel, dilation=dilation, padding=padding, stride=stride)
    return cols.transpose(0, 1).reshape(cols.shape[1], -1)


def flat_rows(g):
    """(C, N L) of an (N, C, ...) or (N, C) tensor in float64: the G side, or a Linear source."""
    g = g.double()
    return g.reshape(g.shape[0], g.shape[1], -1).transpose(0, 1).reshape(g.shape[1], -1)
