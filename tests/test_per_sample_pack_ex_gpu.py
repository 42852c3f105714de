"""curv_persample_pack_ex on the GPU, through the C ABI, held bit for bit: the pack is a copy, an exact upcast and exact
zeros.  Every source lies inside a larger NaN buffer, every destination has sentinels behind its `floats`."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from curvature_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CODES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}


def fenced(values, gpu, lead=64):
    """`values` (a CPU tensor) inside a larger NaN buffer on the GPU, `lead` elements behind its start (64 keeps the
    allocation's alignment, 65 breaks every alignment above the element's)."""
    flat = values.reshape(-1)
    buf = torch.full((flat.numel() + lead + 64,), float("nan"), dtype=values.dtype, device=gpu)
    buf[lead:lead + flat.numel()] = flat.to(gpu)
    return buf[lead:lead + flat.numel()].view(values.shape)


def random_source(shape, dtype, gpu, seed, lead=64):
    gen = torch.Generator().manual_seed(seed)
    return fenced(torch.randn(shape, generator=gen).to(dtype), gpu, lead)


class Item:
    """One descriptor: `view` a 4-d (N, C, H, W) view of the source (any strides), the window, and for the transposed
    gather the output size."""

    def __init__(self, view, kernel=(1, 1), stride=(1, 1), padding=(0, 0), has_bias=False, rows_outer=False,
                 out_size=None, Lp=None):
        self.view, self.kernel, self.stride, self.padding = view, kernel, stride, padding
        self.has_bias, self.rows_outer, self.out_size = has_bias, rows_outer, out_size
        N, C, H, W = view.shape
        if out_size is None:
            self.Ho = (H + 2 * padding[0] - kernel[0]) // stride[0] + 1
            self.Wo = (W + 2 * padding[1] - kernel[1]) // stride[1] + 1
        else:
            self.Ho, self.Wo = out_size
        self.L = self.Ho * self.Wo
        self.Lp = (self.L + 3) // 4 * 4 if Lp is None else Lp
        self.R = C * kernel[0] * kernel[1] + int(has_bias)
        self.floats = N * self.R * max(self.Lp, 0)

    def fill(self, d, dst):
        v = self.view
        d.src, d.dst = v.data_ptr(), dst.data_ptr()
        d.s_n, d.s_c, d.s_h, d.s_w = v.stride()
        d.src_elems = v.untyped_storage().nbytes() // v.element_size() - v.storage_offset()
        d.N, d.C, d.H, d.W = v.shape
        (d.kh, d.kw), (d.sh, d.sw), (d.ph, d.pw) = self.kernel, self.stride, self.padding
        d.has_bias, d.rows_outer, d.Lp = int(self.has_bias), int(self.rows_outer), self.Lp
        d.dtype = CODES[v.dtype]
        d.transposed = int(self.out_size is not None)
        if self.out_size is not None:
            d.Ho, d.Wo = self.out_size

    def laid_out(self, cols):
        """(N, rows, L) columns as the contract lays them out: ones row, zero tail, rows_outer."""
        N = cols.shape[0]
        if self.has_bias:
            cols = torch.cat([cols, torch.ones(N, 1, self.L)], dim=1)
        cols = torch.cat([cols, torch.zeros(N, self.R, self.Lp - self.L)], dim=2)
        return (cols.permute(1, 0, 2) if self.rows_outer else cols).contiguous().reshape(-1)

    def expected(self):
        x = self.view.detach().float().cpu().contiguous()
        if self.out_size is None:
            return self.laid_out(F.unfold(x, self.kernel, padding=self.padding, stride=self.stride))
        return self.laid_out(transposed_columns(x, self.kernel, self.stride, self.padding, self.out_size))


def transposed_columns(x, kernel, stride, padding, out_size):
    """X of a ConvTranspose2d by index arithmetic: row (ci, a, b) at (oh, ow) is x[n, ci, (oh + ph - a) / sh,
    (ow + pw - b) / sw] where both are whole and inside the input."""
    N, C, H, W = x.shape
    (kh, kw), (sh, sw), (ph, pw), (Ho, Wo) = kernel, stride, padding, out_size
    X = torch.zeros(N, C * kh * kw, Ho * Wo, dtype=x.dtype)
    for a in range(kh):
        for b in range(kw):
            for oh in range(Ho):
                for ow in range(Wo):
                    th, tw = oh + ph - a, ow + pw - b
                    if th < 0 or tw < 0 or th % sh or tw % sw or th // sh >= H or tw // sw >= W:
                        continue
                    X[:, a * kw + b::kh * kw, oh * Wo + ow] = x[:, :, th // sh, tw // sw]
    return X


def destinations(items, gpu):
    return [torch.full((it.floats + 64,), SENTINEL, device=gpu) for it in items]


def pack_ex(items, gpu, dsts=None):
    """One call for all items; returns (status, [the `floats` of every destination on the CPU]) after checking the
    sentinels behind them."""
    dsts = destinations(items, gpu) if dsts is None else dsts
    arr = (_lib.curv_persample_pack_ex_desc * len(items))()
    for d, it, dst in zip(arr, items, dsts):
        it.fill(d, dst)
    rc = _lib.lib().curv_persample_pack_ex(_lib.stream_ptr(), arr, len(items))
    out = []
    for it, dst in zip(items, dsts):
        host = dst.cpu()
        assert bool((host[it.floats:] == SENTINEL).all()), "written behind `floats`"
        out.append(host[:it.floats])
    return rc, out


def pack_old(view, item, gpu, channels_last):
    """The same item through curv_persample_pack (float32, contiguous sources only)."""
    dst = torch.full((item.floats + 64,), SENTINEL, device=gpu)
    arr = (_lib.curv_persample_pack_desc * 1)()
    d = arr[0]
    d.src, d.dst = view.data_ptr(), dst.data_ptr()
    d.N, d.C, d.H, d.W = item.view.shape
    (d.kh, d.kw), (d.sh, d.sw), (d.ph, d.pw) = item.kernel, item.stride, item.padding
    d.has_bias, d.channels_last, d.rows_outer, d.Lp = int(item.has_bias), int(channels_last), int(item.rows_outer), item.Lp
    assert _lib.lib().curv_persample_pack(_lib.stream_ptr(), arr, 1) == 0, _lib.lib().curv_last_error()
    return dst.cpu()[:item.floats]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# (id, builder of the 4-d view from (dtype, gpu), kernel, stride, padding, channels_last for the old entry point or None)
def nchw(shape, lead=64):
    return lambda dtype, gpu: random_source(shape, dtype, gpu, sum(shape) + lead, lead)


def ntd(shape):                                            # (N, T, D) as C = D, H = T, W = 1
    return lambda dtype, gpu: random_source(shape, dtype, gpu, 11).permute(0, 2, 1).unsqueeze(-1)


def tne(shape):                                            # (T, N, E) as sample N, C = E, H = T, W = 1
    return lambda dtype, gpu: random_source(shape, dtype, gpu, 13).permute(1, 2, 0).unsqueeze(-1)


FORWARD = [
    ("c3x3_tail", nchw((3, 5, 7, 6)), (3, 3), (1, 1), (1, 1), False),         # L = 42, Lp = 44
    ("c1x1_vector", nchw((2, 6, 4, 4)), (1, 1), (1, 1), (0, 0), False),
    ("c1x1_L49", nchw((2, 6, 7, 7)), (1, 1), (1, 1), (0, 0), False),          # rows of 49: no vector path
    ("c1x1_offset", nchw((2, 6, 4, 4), lead=65), (1, 1), (1, 1), (0, 0), False),
    ("c3x3_s2", nchw((2, 3, 9, 8)), (3, 3), (2, 2), (1, 1), False),
    ("c7x7_s2", nchw((1, 3, 12, 12)), (7, 7), (2, 2), (3, 3), False),
    ("ntd", ntd((3, 5, 8)), (1, 1), (1, 1), (0, 0), True),
    ("tne", tne((5, 3, 8)), (1, 1), (1, 1), (0, 0), None),
]


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("rows_outer", [False, True], ids=["samples_outer", "rows_outer"])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("case", FORWARD, ids=[c[0] for c in FORWARD])
def test_forward_geometries_bit_for_bit(gpu, case, dtype, rows_outer, bias):
    _, make, kernel, stride, padding, old_form = case
    view = make(DTYPES[dtype], gpu)
    item = Item(view, kernel, stride, padding, bias, rows_outer)
    rc, (got,) = pack_ex([item], gpu)
    assert rc == 0, _lib.lib().curv_last_error()
    want = item.expected()
    assert not bool(torch.isnan(want).any())
    assert same_bits(got, want)
    if dtype in ("bf16", "fp32") and old_form is not None:
        # the (upcast) contiguous copy through curv_persample_pack, the fp32-contiguous spelling: the same bits
        copy = view.float().contiguous(memory_format=torch.channels_last if old_form else torch.contiguous_format)
        assert same_bits(got, pack_old(copy, item, gpu, old_form))


TRANSPOSED = [
    # (id, kernel, stride, padding, input H x W, extra output size)
    ("k4s2p1", (4, 4), (2, 2), (1, 1), (5, 6), (0, 0)),
    ("k2s2p0", (2, 2), (2, 2), (0, 0), (4, 4), (0, 0)),
    ("k3s1p1", (3, 3), (1, 1), (1, 1), (5, 5), (0, 0)),
    ("k4s1p0_1x1", (4, 4), (1, 1), (0, 0), (1, 1), (0, 0)),
    ("k3s2p1_larger", (3, 3), (2, 2), (1, 1), (5, 5), (1, 1)),
    ("rect", (3, 2), (2, 1), (1, 0), (4, 5), (0, 0)),
]


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("rows_outer", [False, True], ids=["samples_outer", "rows_outer"])
@pytest.mark.parametrize("case", TRANSPOSED, ids=[c[0] for c in TRANSPOSED])
def test_transposed_gather(gpu, case, rows_outer, dtype):
    _, kernel, stride, padding, (H, W), extra = case
    N, Cin, Cout = 2, 3, 2
    out_size = tuple((d - 1) * s - 2 * p + k + e for d, s, p, k, e in zip((H, W), stride, padding, kernel, extra))
    view = random_source((N, Cin, H, W), DTYPES[dtype], gpu, 5 + H)
    item = Item(view, kernel, stride, padding, True, rows_outer, out_size)
    rc, (got,) = pack_ex([item], gpu)
    assert rc == 0, _lib.lib().curv_last_error()
    assert same_bits(got, item.expected())                                   # 1. index arithmetic in a Python loop
    # 2. g_n X_n^T in float64 against the per-sample weight gradient of F.conv_transpose2d, in Wm order
    X = got.view(item.R, N, item.Lp).permute(1, 0, 2) if rows_outer else got.view(N, item.R, item.Lp)
    X = X[:, :item.R - 1, :item.L].double()
    gen = torch.Generator().manual_seed(3)
    g = torch.randn(N, Cout, *out_size, generator=gen, dtype=torch.float64)
    x64 = view.detach().double().cpu()
    for n in range(N):
        w = torch.zeros(Cin, Cout, *kernel, dtype=torch.float64, requires_grad=True)
        out = F.conv_transpose2d(x64[n:n + 1], w, stride=stride, padding=padding, output_padding=extra)
        assert tuple(out.shape[2:]) == out_size
        (grad,) = torch.autograd.grad((out * g[n:n + 1]).sum(), w)
        want = grad.permute(1, 0, 2, 3).reshape(Cout, -1)
        have = g[n].reshape(Cout, -1) @ X[n].t()
        err = float(torch.linalg.norm(have - want) / torch.linalg.norm(want))
        print(f"transposed pack {case[0]} sample {n}: g X^T against autograd {err:.3e}")
        assert err <= 1e-12


@pytest.mark.parametrize("lead", [64, 65], ids=["vector", "gather"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_half_special_values_survive(gpu, dtype, lead):
    dt = DTYPES[dtype]
    tiny = torch.tensor([1], dtype=torch.int16).view(dt)                      # the smallest subnormal
    values = torch.cat([torch.tensor([float("inf"), float("-inf"), -0.0, 0.0, float("nan"), 1.0, -2.5], dtype=dt), tiny,
                        -tiny, torch.tensor([torch.finfo(dt).max, torch.finfo(dt).tiny], dtype=dt)])
    values = torch.cat([values, torch.arange(32 - values.numel()).to(dt)]).view(1, 2, 4, 4)
    view = fenced(values, gpu, lead)
    item = Item(view)
    rc, (got,) = pack_ex([item], gpu)
    assert rc == 0, _lib.lib().curv_last_error()
    want = values.float().reshape(-1)
    nan = torch.isnan(want)
    assert int(nan.sum()) == 1 and torch.equal(torch.isnan(got), nan)         # NaN compared as NaN
    assert same_bits(got[~nan], want[~nan])                                   # -0.0, subnormals and inf by their bits
    assert float(want[7]) != 0.0 and bool(torch.signbit(got[2]))


@pytest.mark.parametrize("lead", [64, 65], ids=["vector", "gather"])
def test_sample_base_is_formed_in_64_bits(gpu, lead):
    """fp16, N = 3 samples of (2, 4, 4) values 2^31 + 8 elements apart in a buffer that is never filled: sample 1 lies
    where a signed 32-bit product wraps, sample 2 (at 2^32 + 16) where an unsigned one does.  Elements 0 and 16, where a
    wrapped product lands, hold NaNs (as values of sample 0), and NaNs follow sample 0."""
    free, _ = torch.cuda.mem_get_info()
    if free < 10 << 30:
        pytest.skip(f"an 8 GiB source needs 10 GiB of free device memory, {free >> 20} MiB are free")
    s_n = (1 << 31) + 8
    buf = torch.empty(lead + 2 * s_n + 32, dtype=torch.float16, device=gpu)
    view = buf[lead:].as_strided((3, 2, 4, 4), (s_n, 16, 4, 1))
    values = ((torch.arange(96) - 40) * 0.25).half().view(3, 2, 4, 4)         # distinct, exact in fp16
    values[0, 0, 0, 0] = values[0, 1, 0, 0] = float("nan")                    # elements 0 and 16
    for n in range(3):                                                        # only the three samples are written
        view[n].copy_(values[n])
    buf[lead + 32:lead + 96] = float("nan")
    rc, (got,) = pack_ex([Item(view)], gpu)
    assert rc == 0, _lib.lib().curv_last_error()
    want = values.float().reshape(-1)
    assert int(torch.isnan(want).sum()) == 2 and same_bits(got, want)         # the upcast NaNs by their bits as well


def test_alone_and_in_a_batch_of_twenty(gpu):
    items = []
    for k in range(20):                                                       # one dtype: 16 + 4, two launches
        _, make, kernel, stride, padding, _ = FORWARD[k % len(FORWARD)]
        items.append(Item(make(torch.bfloat16, gpu), kernel, stride, padding, k % 2 == 0, k % 3 == 0))
    view = random_source((2, 3, 5, 6), torch.bfloat16, gpu, 77)
    items[5] = Item(view, (4, 4), (2, 2), (1, 1), True, False, (10, 12))
    rc, together = pack_ex(items, gpu)
    assert rc == 0, _lib.lib().curv_last_error()
    for it, batch in zip(items, together):
        rc, (alone,) = pack_ex([it], gpu)
        assert rc == 0 and same_bits(alone, batch) and same_bits(alone, it.expected())


def test_mixed_dtypes_in_one_call(gpu):
    items = [Item(make(DTYPES[name], gpu), kernel, stride, padding, True)
             for name in sorted(DTYPES) for _, make, kernel, stride, padding, _ in FORWARD[:3]]
    rc, got = pack_ex(items, gpu)
    assert rc == 0, _lib.lib().curv_last_error()
    for it, have in zip(items, got):
        assert same_bits(have, it.expected())


def refusals(gpu):
    src = random_source((2, 3, 5, 6), torch.float32, gpu, 1)

    def edited(text, **fields):
        item = Item(src, (3, 3), (1, 1), (1, 1), True)
        return text, item, fields
    convt = dict(transposed=1, kh=4, kw=4, sh=2, sw=2, ph=1, pw=1, Lp=120)
    return [
        edited("invalid geometry", kh=0),
        edited("invalid geometry", sw=0),
        edited("kernel larger than the padded input", kh=9),
        edited("transposed output", **convt, Ho=9, Wo=12),
        edited("transposed output", **convt, Ho=10, Wo=14),
        edited("multiple of 4", Lp=30),
        edited("multiple of 4", Lp=28),                                      # below L = 30
        edited("too large", C=1 << 22),
        edited("dtype", dtype=7),
        edited("dtype", dtype=-1),
        edited("source extent", src_elems=2 * 3 * 5 * 6 - 1),
        edited("source extent", s_n=1 << 20),
        edited("negative stride", s_h=-6),
        edited("null src or dst", src=None),
        edited("dst is not 16-byte aligned", dst="+4"),
        edited("src is not aligned", src="+2"),
    ]


@pytest.mark.parametrize("index", range(16))
def test_plan_refusals_name_the_item_and_launch_nothing(gpu, index):
    text, bad, fields = refusals(gpu)[index]
    good = Item(random_source((2, 3, 5, 6), torch.float32, gpu, 2), (3, 3), (1, 1), (1, 1), True)
    dsts = destinations([good, bad], gpu)
    arr = (_lib.curv_persample_pack_ex_desc * 2)()
    good.fill(arr[0], dsts[0])
    bad.fill(arr[1], dsts[1])
    for key, value in fields.items():
        if isinstance(value, str):                                            # "+n": the filled address moved by n bytes
            value = getattr(arr[1], key) + int(value)
        setattr(arr[1], key, value)
    rc = _lib.lib().curv_persample_pack_ex(_lib.stream_ptr(), arr, 2)
    message = _lib.lib().curv_last_error().decode()
    assert rc == _lib.ERR_INVALID
    assert "curv_persample_pack_ex: item 1:" in message and text in message, message
    torch.cuda.synchronize()
    for dst in dsts:                                                          # not even the valid item was packed
        assert bool((dst == SENTINEL).all())
    assert ctypes.sizeof(arr) == 2 * ctypes.sizeof(_lib.curv_persample_pack_ex_desc)
