"""`curv_logsum_grid` (csrc/logdet.hip) on the GPU against float64 computed on the CPU: float32 segments around the chunk
size at aligned and misaligned addresses (the 16-byte and the one-element load paths), strided float64 diagonals, a segment
of squares, 1, 16 and 17 pairs, NaN fences around every input and output, and the bit-level promises.

The bar (tests/logdet_refs.py, `bar`): per output |got - want| <= 1e-11 (sum |term| + count)."""
import functools

import pytest
import torch

import logdet_refs as R

pytestmark = pytest.mark.gpu

COUNTS = [1, 3, 4095, 4096, 4097, 3 * 4096 + 5]
GRID = [(add, multiply) for add in (1e-4, 1.0, 1e4) for multiply in (1e-4, 1.0, 1e4)]        # {1e-4, 1, 1e4}^2
FENCE = 8                                   # NaNs on either side of a segment (floats)


def pairs_of(H, first=0):
    """H (gain, shift) = (multiply, add) pairs out of GRID, cycling from `first`."""
    picked = [GRID[(first + h) % len(GRID)] for h in range(H)]
    return [s for _, s in picked], [n for n, _ in picked]


@functools.lru_cache(maxsize=None)
def fenced_segment(count, offset):
    """(view on the GPU, float64 values): `count` float32 values log-uniform in [1e-12, 1e3], a tenth of them negative,
    some exact zeros, `offset` floats behind a 16-byte boundary, NaN everywhere else in the buffer."""
    gen = torch.Generator().manual_seed(1000 + 7 * count + offset)
    values = torch.exp(torch.empty(count, dtype=torch.float64).uniform_(-27.631021, 6.907755, generator=gen)).float()
    values[torch.rand(count, generator=gen) < 0.1] *= -1.0
    values[torch.rand(count, generator=gen) < 0.05] = 0.0
    values[0] = 0.0 if count > 1 else values[0]
    buf = torch.full((FENCE + offset + count + FENCE + 4,), float("nan"))
    buf[FENCE + offset:FENCE + offset + count] = values
    dev = buf.cuda()
    assert dev.data_ptr() % 16 == 0
    view = dev[FENCE + offset:FENCE + offset + count]
    assert view.data_ptr() % 16 == 4 * offset
    return dev, view, values.double()


def fences_intact(dev, offset, count):
    return bool(torch.isnan(dev[:FENCE + offset]).all()) and bool(torch.isnan(dev[FENCE + offset + count:]).all())


def check(got, want, bars, tag):
    worst = 0.0
    for g, w, b in zip(got, want, bars):
        worst = max(worst, abs(g - w) / b)
    print(f"{tag}: worst |got - want| / bar = {worst:.2e}")
    assert worst <= 1.0, tag


@pytest.mark.parametrize("H", [1, 16, 17])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("count", COUNTS)
def test_float32_segment_against_float64(gpu, count, offset, H):
    from curvature_amd import ops
    dev, view, x64 = fenced_segment(count, offset)
    gains, shifts = pairs_of(H, first=count % 9)
    want, bars = R.segment_sums(x64, 1.5, gains, shifts)
    out, total = ops.logsum_grid([ops.LogSumSegment.of(view, 1.5, gains, shifts)], H)
    assert out.dtype == total.dtype == torch.float64 and tuple(out.shape) == (1, H) and tuple(total.shape) == (H,)
    check(out[0].tolist(), want, bars, f"count {count} offset {offset} H {H}")
    assert torch.equal(total, out[0])
    assert fences_intact(dev, offset, count)


@pytest.mark.parametrize("width", [5, 65])
def test_strided_float64_diagonal(gpu, width):
    """The diagonal of a square float64 matrix, stride width + 1, gain 1, shift 0, weight -2; NaN off the diagonal."""
    from curvature_amd import ops
    gen = torch.Generator().manual_seed(width)
    diag = torch.rand(width, generator=gen, dtype=torch.float64) * 3.0 + 1e-3
    M = torch.full((width, width), float("nan"), dtype=torch.float64)
    M.diagonal().copy_(diag)
    dev = M.cuda()
    want, bars = R.segment_sums(diag, -2.0, [1.0], [0.0])
    out, _ = ops.logsum_grid([ops.LogSumSegment.of(dev.diagonal(), -2.0, [1.0], [0.0])], 1)
    check(out[0].tolist(), want, bars, f"diagonal {width}")
    assert int(torch.isnan(dev).sum()) == width * width - width and torch.equal(dev.diagonal().cpu(), diag)


def test_squares(gpu):
    from curvature_amd import ops
    dev, view, x64 = fenced_segment(4097, 1)
    want, b = R.squares_sum(x64, 0.5)
    out, total = ops.logsum_grid([ops.LogSumSegment.squares(view, 0.5)], 3)
    check([float(out[0, 0])], [want], [b], "squares 4097")
    assert out[0, 1:].tolist() == [0.0, 0.0] and total.tolist() == [float(out[0, 0]), 0.0, 0.0]
    assert fences_intact(dev, 1, 4097)


@functools.lru_cache(maxsize=None)
def mixed_table():
    """Segments of every kind with different gain and shift rows, and their float64 sums for 17 pairs."""
    from curvature_amd import ops
    H = 17
    items = []
    for k, (count, offset) in enumerate([(4097, 0), (3, 1), (3 * 4096 + 5, 1), (1, 0), (4096, 0)]):
        _, view, x64 = fenced_segment(count, offset)
        gains, shifts = pairs_of(H, first=k)
        items.append((ops.LogSumSegment.of(view, 1.0 + k, gains, shifts), R.segment_sums(x64, 1.0 + k, gains, shifts)))
    gen = torch.Generator().manual_seed(5)
    M = torch.rand(65, 65, generator=gen, dtype=torch.float64) + 0.5
    items.append((ops.LogSumSegment.of(M.cuda().diagonal(), -2.0, [1.0] * H, [0.0] * H),
                  R.segment_sums(M.diagonal(), -2.0, [1.0] * H, [0.0] * H)))
    _, view, x64 = fenced_segment(4095, 1)
    sq, sq_bar = R.squares_sum(x64)
    items.append((ops.LogSumSegment.squares(view), ([sq] + [0.0] * (H - 1), [sq_bar] * H)))
    empty = torch.empty(0, device="cuda")
    items.append((ops.LogSumSegment.of(empty, 3.0, *pairs_of(H)), ([0.0] * H, [1e-300] * H)))
    return H, items


def test_a_table_of_mixed_segments(gpu):
    from curvature_amd import ops
    H, items = mixed_table()
    out, total = ops.logsum_grid([seg for seg, _ in items], H)
    for k, (_, (want, bars)) in enumerate(items):
        check(out[k].tolist(), want, bars, f"mixed table segment {k}")
    in_order = torch.zeros(H, dtype=torch.float64)
    for row in out.cpu():
        in_order += row
    assert torch.equal(total.cpu(), in_order)                       # the segments in table order, float64


def test_alone_in_a_batch_and_again(gpu):
    from curvature_amd import ops
    H, items = mixed_table()
    segments = [seg for seg, _ in items]
    out, total = ops.logsum_grid(segments, H)
    again, total_again = ops.logsum_grid(segments, H)
    assert torch.equal(out, again) and torch.equal(total, total_again)
    for k, seg in enumerate(segments):
        alone, alone_total = ops.logsum_grid([seg], H)
        assert torch.equal(alone[0], out[k]), k
        assert torch.equal(alone_total, out[k]), k
    # a pair's column does not depend on the other pairs of the call, nor on where a chunk of 16 ends
    for h in (0, 15, 16):
        one, _ = ops.logsum_grid([seg if seg.gains is None else seg._replace(gains=seg.gains[h:h + 1], shifts=seg.shifts[h:h + 1])
                                  for seg in segments], 1)
        squares = [k for k, seg in enumerate(segments) if seg.gains is None]
        keep = [k for k in range(len(segments)) if k not in squares or h == 0]
        assert torch.equal(one[keep, 0], out[keep, h]), h


def test_output_fences_and_unused_columns(gpu):
    """The entry point itself on a NaN-filled `out` of stride 16 with 3 pairs, `total` and the workspace fenced too: columns
    3 .. 15, the rows behind the table, a squares row beyond column 0 and everything around `total` stay NaN."""
    from curvature_amd import _lib, ops
    H, items = mixed_table()
    segments = [seg for seg, _ in items]
    n, pairs, stride = len(segments), 3, 16
    arr = (_lib.curv_logsum_desc * n)()
    for d, seg in zip(arr, segments):
        t = seg.tensor
        d.x, d.count, d.stride = (t.data_ptr() if t.numel() else None), t.numel(), (t.stride(0) if t.numel() > 1 else 1)
        d.dtype, d.mode, d.weight = (_lib.DTYPE_F64 if t.dtype == torch.float64 else _lib.DTYPE_F32), seg.mode, seg.weight
        if seg.gains is not None:
            d.gain[:pairs], d.shift[:pairs] = seg.gains[:pairs], seg.shifts[:pairs]
    L = _lib.lib()
    need = L.curv_logsum_workspace_bytes(arr, n, pairs)
    assert need > 0 and need % 8 == 0
    out = torch.full((n + 2, stride), float("nan"), dtype=torch.float64, device=gpu)
    total = torch.full((stride,), float("nan"), dtype=torch.float64, device=gpu)
    ws = torch.full((need // 8 + 16,), float("nan"), dtype=torch.float64, device=gpu)
    _lib.check(L.curv_logsum_grid(_lib.stream_ptr(), arr, n, pairs, out[1].data_ptr(), stride, total[4:].data_ptr(),
                                  ws[8:].data_ptr(), need), "curv_logsum_grid")
    want, _ = ops.logsum_grid(
        [seg if seg.gains is None else seg._replace(gains=seg.gains[:pairs], shifts=seg.shifts[:pairs]) for seg in segments], pairs)
    written = torch.zeros_like(out, dtype=torch.bool)
    written[1:n + 1, :pairs] = True
    for k, seg in enumerate(segments):
        if seg.gains is None:
            written[1 + k, 1:] = False
    assert bool(torch.isnan(out[~written]).all())
    assert torch.equal(out[written], torch.cat([row[:1] if seg.gains is None else row for row, seg in zip(want, segments)]))
    assert bool(torch.isnan(total[:4]).all()) and bool(torch.isnan(total[4 + pairs:]).all()) and bool(torch.isfinite(total[4:4 + pairs]).all())
    assert bool(torch.isnan(ws[:8]).all()) and bool(torch.isnan(ws[8 + need // 8:]).all())
    for (count, offset) in [(4097, 0), (3, 1), (3 * 4096 + 5, 1), (1, 0), (4096, 0), (4095, 1)]:
        assert fences_intact(fenced_segment(count, offset)[0], offset, count)
