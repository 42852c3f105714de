"""curv_persample_pack3d on the GPU, through the C ABI, held bit for bit against torch's own 3-D unfold of the same record
(`F.pad`, `unfold` over the three spatial axes, `permute(0, 1, 5, 6, 7, 2, 3, 4)`, reshape to (N, C kd kh kw, L)): the pack
is a copy, an exact upcast and exact zeros.  Every source lies inside a larger NaN buffer, every destination has sentinels
behind its `floats`.  The references are computed once per case, on the CPU, and shared."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from curvature_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CODES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}


def triple(v):
    return (v, v, v) if isinstance(v, int) else tuple(v)


# (N, C, D, H, W), kernel, stride, padding, has_bias
CASES = {
    "1_k3p1_bias_tail": ((2, 3, 5, 6, 7), 3, 1, 1, True),                    # L = 210: zero tail and ones row
    "2_depth_stride": ((2, 2, 7, 5, 5), 3, (2, 1, 1), (1, 0, 1), False),     # output 4 x 3 x 5
    "3_kd1": ((3, 4, 4, 6, 6), (1, 3, 3), (1, 2, 2), (0, 1, 1), False),
    "4_all_padding": ((2, 2, 3, 4, 4), (2, 1, 1), 1, (2, 0, 0), False),      # output depths whose whole patch is padding
    "5_depth_only": ((2, 3, 6, 3, 3), 3, 1, (1, 0, 0), False),               # output 6 x 1 x 1
    "6_two_carries": ((1, 2, 4, 3, 5), 3, 1, (1, 0, 0), False),              # output 4 x 1 x 3
    "7_L1": ((2, 1, 2, 2, 2), 2, 1, 0, False),                               # L = 1, Lp = 4
    "8_pointwise": ((2, 8, 3, 4, 4), 1, 1, 0, False),                        # the vector path
    "9_pointwise_s2": ((2, 8, 4, 6, 6), 1, 2, 0, False),
    "10_D_is_kd": ((2, 2, 3, 5, 6), 3, 1, (0, 1, 1), False),                 # the 2-D pack of x.reshape(N, C kd, H, W)
}


def unfold3d(x, kernel, stride, padding):
    """(N, C kd kh kw, L) of a CPU record: torch's own unfold, rows in the order of ``weight.reshape(Cout, -1)``."""
    N, C = x.shape[:2]
    padded = F.pad(x, (padding[2], padding[2], padding[1], padding[1], padding[0], padding[0]))
    u = padded.unfold(2, kernel[0], stride[0]).unfold(3, kernel[1], stride[1]).unfold(4, kernel[2], stride[2])
    return u.permute(0, 1, 5, 6, 7, 2, 3, 4).reshape(N, C * kernel[0] * kernel[1] * kernel[2], -1)


@functools.lru_cache(maxsize=None)
def record(shape, dtype=torch.float32):
    """The CPU values of a case: random, rounded to `dtype` (shared; never written)."""
    gen = torch.Generator().manual_seed(sum(shape) + 7 * len(shape))
    return torch.randn(shape, generator=gen).to(dtype)


def fenced(values, gpu, lead=64):
    """`values` (a CPU tensor, any strides) inside a larger NaN buffer on the GPU, `lead` elements behind its start, with
    the strides it has (64 keeps the allocation's alignment, 65 breaks every alignment above the element's)."""
    size = max(sum((d - 1) * s for d, s in zip(values.shape, values.stride())) + 1, 1)
    buf = torch.full((size + lead + 64,), float("nan"), dtype=values.dtype, device=gpu)
    view = buf[lead:].as_strided(values.shape, values.stride())
    view.copy_(values.to(gpu))
    return view


class Item:
    """One descriptor: `view` a 5-d (N, C, D, H, W) view of the source (any strides) and the window."""

    def __init__(self, view, kernel=1, stride=1, padding=0, has_bias=False, rows_outer=False, Lp=None):
        self.view, self.kernel, self.stride, self.padding = view, triple(kernel), triple(stride), triple(padding)
        self.has_bias, self.rows_outer = has_bias, rows_outer
        N, C = view.shape[:2]
        self.out = tuple((d + 2 * p - k) // s + 1 for d, k, s, p in zip(view.shape[2:], self.kernel, self.stride, self.padding))
        self.L = self.out[0] * self.out[1] * self.out[2]
        self.Lp = (self.L + 3) // 4 * 4 if Lp is None else Lp
        self.R = C * self.kernel[0] * self.kernel[1] * self.kernel[2] + int(has_bias)
        self.floats = N * self.R * max(self.Lp, 0)

    def fill(self, d, dst):
        v = self.view
        d.src, d.dst = v.data_ptr(), dst.data_ptr()
        d.s_n, d.s_c, d.s_d, d.s_h, d.s_w = v.stride()
        d.src_elems = v.untyped_storage().nbytes() // v.element_size() - v.storage_offset()
        d.N, d.C, d.D, d.H, d.W = v.shape
        (d.kd, d.kh, d.kw), (d.sd, d.sh, d.sw), (d.pd, d.ph, d.pw) = self.kernel, self.stride, self.padding
        d.has_bias, d.rows_outer, d.Lp = int(self.has_bias), int(self.rows_outer), self.Lp
        d.dtype = CODES[v.dtype]

    def laid_out(self, cols):
        """(N, rows, L) columns as the contract lays them out: ones row, zero tail, rows_outer."""
        N = cols.shape[0]
        if self.has_bias:
            cols = torch.cat([cols, torch.ones(N, 1, self.L)], dim=1)
        cols = torch.cat([cols, torch.zeros(N, self.R, self.Lp - self.L)], dim=2)
        return (cols.permute(1, 0, 2) if self.rows_outer else cols).contiguous().reshape(-1)

    def expected(self, values):
        """From the CPU `values` the source holds (the exact upcast, then torch's unfold)."""
        return self.laid_out(unfold3d(values.float(), self.kernel, self.stride, self.padding))


def destinations(items, gpu, fill=SENTINEL):
    return [torch.full((it.floats + 64,), fill, device=gpu) for it in items]


def pack3d(items, gpu, dsts=None):
    """One call for all items; (status, [the `floats` of every destination on the CPU]) after checking the sentinels
    behind them."""
    dsts = destinations(items, gpu) if dsts is None else dsts
    arr = (_lib.curv_persample_pack3d_desc * len(items))()
    for d, it, dst in zip(arr, items, dsts):
        it.fill(d, dst)
    rc = _lib.lib().curv_persample_pack3d(_lib.stream_ptr(), arr, len(items))
    out = []
    for it, dst in zip(items, dsts):
        host = dst.cpu()
        assert bool((host[it.floats:it.floats + 64] == SENTINEL).all()), "written behind `floats`"
        out.append(host[:it.floats])
    return rc, out


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_one(item, gpu):
    rc, (got,) = pack3d([item], gpu)
    assert rc == 0, _lib.lib().curv_last_error()
    return got


def test_the_reference_unfold_is_the_convolution():
    """Wm @ X of the recipe against F.conv3d in float64, for every geometry (what makes the recipe a reference)."""
    for shape, kernel, stride, padding, _ in CASES.values():
        k, s, p = triple(kernel), triple(stride), triple(padding)
        x = record(shape).double()
        w = torch.randn(5, shape[1], *k, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        want = F.conv3d(x, w, stride=s, padding=p)
        have = (w.reshape(5, -1) @ unfold3d(x, k, s, p)).reshape(want.shape)
        assert float((have - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)


@pytest.mark.parametrize("rows_outer", [False, True], ids=["samples_outer", "rows_outer"])
@pytest.mark.parametrize("case", sorted(CASES, key=lambda c: int(c.split("_")[0])))
def test_geometries_bit_for_bit(gpu, case, rows_outer):
    shape, kernel, stride, padding, bias = CASES[case]
    values = record(shape)
    item = Item(fenced(values, gpu), kernel, stride, padding, bias, rows_outer)
    got = run_one(item, gpu)
    want = item.expected(values)
    assert not bool(torch.isnan(want).any())
    assert same_bits(got, want)
    assert same_bits(run_one(item, gpu), got)                                 # two runs equal


def test_pointwise_off_the_vector_boundary_takes_the_gather_path(gpu):
    """Case 8 one element off a 16-byte boundary: no vector load is possible, the bits are the same."""
    shape, kernel, stride, padding, bias = CASES["8_pointwise"]
    values = record(shape)
    aligned, shifted = (Item(fenced(values, gpu, lead), kernel, stride, padding, bias) for lead in (64, 65))
    assert aligned.view.data_ptr() % 16 == 0 and shifted.view.data_ptr() % 16 == 4
    want = aligned.expected(values)
    assert same_bits(run_one(aligned, gpu), want) and same_bits(run_one(shifted, gpu), want)


def special_values(shape, dtype):
    """The record of a case in a half dtype with inf, NaN, -0, a subnormal and the extremes among its first values."""
    values = record(shape, dtype).clone()
    tiny = torch.tensor([1], dtype=torch.int16).view(dtype)                   # the smallest subnormal
    odd = torch.cat([torch.tensor([float("inf"), float("-inf"), -0.0, 0.0, float("nan"), 1.0, -2.5], dtype=dtype), tiny,
                     -tiny, torch.tensor([torch.finfo(dtype).max, torch.finfo(dtype).tiny], dtype=dtype)])
    values.view(-1)[:odd.numel()] = odd
    return values


@pytest.mark.parametrize("lead", [64, 65], ids=["aligned", "shifted"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", ["1_k3p1_bias_tail", "8_pointwise"])
def test_half_sources_by_their_bits(gpu, case, dtype, lead):
    shape, kernel, stride, padding, bias = CASES[case]
    values = special_values(shape, DTYPES[dtype])
    item = Item(fenced(values, gpu, lead), kernel, stride, padding, bias)
    got = run_one(item, gpu)
    want = item.expected(values)                                              # (unfold copies: NaN, -0 and subnormals stay)
    nan = torch.isnan(want)
    assert int(nan.sum()) >= 1 and torch.equal(torch.isnan(got), nan)         # NaN compared as NaN
    assert same_bits(got[~nan], want[~nan])                                   # -0.0, subnormals and inf by their bits
    assert bool((torch.signbit(want) & (want == 0)).any())                    # a -0 is among them


def test_channels_last_3d_and_channel_slice_are_read_through_their_strides(gpu):
    shape, kernel, stride, padding, bias = CASES["1_k3p1_bias_tail"]
    values = record(shape)
    want = Item(values, kernel, stride, padding, bias).expected(values)
    last = values.contiguous(memory_format=torch.channels_last_3d)
    assert last.stride() != values.stride()
    item = Item(fenced(last, gpu), kernel, stride, padding, bias)
    assert item.view.stride() == last.stride()
    assert same_bits(run_one(item, gpu), want)
    # x[:, 1:3] of a wider record: two channels, the record's strides
    wide = record((2, 4, 5, 6, 7))
    sliced = Item(fenced(wide, gpu)[:, 1:3], kernel, stride, padding, bias)
    assert sliced.view.stride(0) == 4 * 5 * 6 * 7 and sliced.view.shape[1] == 2
    assert same_bits(run_one(sliced, gpu), sliced.expected(wide[:, 1:3]))


def test_nan_fenced_source_and_prefilled_destination(gpu):
    """Case 2 from a source with NaN on both sides into a destination of 0xFF bytes: identical to the clean run."""
    shape, kernel, stride, padding, bias = CASES["2_depth_stride"]
    values = record(shape)
    clean_src = values.to(gpu)
    clean = run_one(Item(clean_src, kernel, stride, padding, bias), gpu)
    item = Item(fenced(values, gpu), kernel, stride, padding, bias)
    dst = torch.full((item.floats + 64,), SENTINEL, device=gpu)
    dst[:item.floats].view(torch.int32).fill_(-1)                             # 0xFF bytes: a NaN pattern
    rc, (got,) = pack3d([item], gpu, [dst])
    assert rc == 0, _lib.lib().curv_last_error()
    assert same_bits(got, clean) and same_bits(got, item.expected(values))


class Flat:
    """A 2-D item of curv_persample_pack3d: D = kd = sd = 1, pd = 0 of an (N, C, H, W) record."""

    def __init__(self, values, gpu, kernel, stride, padding, has_bias, rows_outer):
        self.values = values
        self.item = Item(fenced(values, gpu).unsqueeze(2), (1,) + kernel, (1,) + stride, (0,) + padding, has_bias, rows_outer)

    def expected(self):
        it = self.item
        return it.laid_out(F.unfold(self.values.float(), it.kernel[1:], padding=it.padding[1:], stride=it.stride[1:]))


def test_seventeen_mixed_items_in_one_call(gpu):
    """2-D and 3-D kinds of three dtypes in one call (six launches): every item as in its run alone."""
    names = sorted(CASES, key=lambda c: int(c.split("_")[0]))
    items, wants = [], []
    for k in range(17):
        dtype = DTYPES[sorted(DTYPES)[k % 3]]
        if k % 4 == 3:                                                        # a 2-D kind
            flat = Flat(record((2, 3, 6, 5), dtype), gpu, (3, 3) if k % 8 == 3 else (1, 1), (1, 1),
                        (1, 1) if k % 8 == 3 else (0, 0), k % 2 == 0, k % 3 == 0)
            items.append(flat.item)
            wants.append(flat.expected())
            continue
        shape, kernel, stride, padding, _ = CASES[names[k % len(names)]]
        values = record(shape, dtype)
        items.append(Item(fenced(values, gpu), kernel, stride, padding, k % 2 == 0, k % 3 == 0))
        wants.append(items[-1].expected(values))
    rc, together = pack3d(items, gpu)
    assert rc == 0, _lib.lib().curv_last_error()
    for it, batch, want in zip(items, together, wants):
        assert same_bits(run_one(it, gpu), batch) and same_bits(batch, want)


def test_depth_equal_to_the_kernel_is_the_2d_pack(gpu):
    """Case 10: D = kd, pd = 0 is the 2-D im2col of x.reshape(N, C kd, H, W) - the same bits from curv_persample_pack_ex."""
    shape, kernel, stride, padding, bias = CASES["10_D_is_kd"]
    values = record(shape)
    N, C, D, H, W = shape
    k, s, p = triple(kernel), triple(stride), triple(padding)
    folded = values.reshape(N, C * D, H, W)
    flat = F.unfold(folded, k[1:], padding=p[1:], stride=s[1:])
    assert torch.equal(flat, unfold3d(values, k, s, p))                       # the two unfolds, on the CPU
    src = fenced(values, gpu)
    item = Item(src, kernel, stride, padding, bias)
    got = run_one(item, gpu)
    dst = torch.full((item.floats + 64,), SENTINEL, device=gpu)
    arr = (_lib.curv_persample_pack_ex_desc * 1)()
    d = arr[0]
    view = src.view(N, C * D, H, W)
    d.src, d.dst = view.data_ptr(), dst.data_ptr()
    d.s_n, d.s_c, d.s_h, d.s_w = view.stride()
    d.src_elems = view.untyped_storage().nbytes() // 4 - view.storage_offset()
    d.N, d.C, d.H, d.W = view.shape
    (d.kh, d.kw), (d.sh, d.sw), (d.ph, d.pw) = k[1:], s[1:], p[1:]
    d.Lp, d.dtype = item.Lp, _lib.DTYPE_F32
    assert _lib.lib().curv_persample_pack_ex(_lib.stream_ptr(), arr, 1) == 0, _lib.lib().curv_last_error()
    assert same_bits(dst.cpu()[:item.floats], got) and same_bits(got, item.expected(values))


REFUSALS = [
    ("kernel larger than the padded input", dict(kd=8)),                      # D + 2 pd = 7
    ("multiple of 4 and at least L", dict(Lp=208)),                           # L = 210
    ("reserved", dict(reserved=1)),
    ("source extent", dict(src_elems=2 * 3 * 5 * 6 * 7 - 1)),
    ("unknown dtype", dict(dtype=7)),
]


@pytest.mark.parametrize("text,fields", REFUSALS, ids=[t.split()[0] for t, _ in REFUSALS])
def test_plan_refusals_name_the_item_and_launch_nothing(gpu, text, fields):
    """The faulty item has null pointers: its sizes - the source extent among them - are seen first."""
    shape, kernel, stride, padding, bias = CASES["1_k3p1_bias_tail"]
    values = record(shape)
    good = Item(fenced(values, gpu), kernel, stride, padding, bias)
    bad = Item(fenced(values, gpu), kernel, stride, padding, bias)
    dsts = destinations([good, bad], gpu)
    arr = (_lib.curv_persample_pack3d_desc * 2)()
    good.fill(arr[0], dsts[0])
    bad.fill(arr[1], dsts[1])
    arr[1].src = arr[1].dst = None
    for key, value in fields.items():
        setattr(arr[1], key, value)
    rc = _lib.lib().curv_persample_pack3d(_lib.stream_ptr(), arr, 2)
    message = _lib.lib().curv_last_error().decode()
    assert rc == _lib.ERR_INVALID
    assert "curv_persample_pack3d: item 1:" in message and text in message, message
    torch.cuda.synchronize()
    for dst in dsts:                                                          # not even the valid item was packed
        assert bool((dst == SENTINEL).all())
    assert ctypes.sizeof(arr) == 2 * ctypes.sizeof(_lib.curv_persample_pack3d_desc)
