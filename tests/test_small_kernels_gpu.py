"""The small kernels under Diagonal, EFB, INF and the samplers (csrc/elementwise.hip, csrc/inf.hip, randn_kernel with
csrc/philox.h) against plain references: Python-integer Philox, float32 / float64 torch on the CPU (small_kernel_refs.py).

Each case is sized for a path of its kernel: the grids are capped at 2048 x 256 threads, so more than 524288 elements
(2097152 for the float4 loop of rsqrt_affine and the quads of randn) make a thread take a second grid-stride trip; the
batched square and copy kernels split their descriptors at 96 items, the selection at 32 layers."""
import numpy as np
import pytest
import torch

import small_kernel_refs as R

pytestmark = pytest.mark.gpu

STRIDE = 2048 * 256                       # threads of a capped grid
NAN = float("nan")


def bits(t):
    """int32 / int64 view of a float32 / float64 CPU tensor: equality of bit patterns (NaN payloads and -0 included)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(got, want):
    return got.shape == want.shape and torch.equal(bits(got), bits(want))


def fenced(count, gpu, lead=4, shift=0):
    """(buffer, view): `count` floats inside a NaN-filled buffer, `lead + shift` NaNs before and at least one behind;
    lead = 4 keeps the view 16-byte aligned, shift = 1 moves it off by one float."""
    buf = torch.full((lead + shift + count + 5,), NAN, device=gpu)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[lead + shift:lead + shift + count]


def fence_intact(buf, view):
    at = (view.data_ptr() - buf.data_ptr()) // 4
    return bool(torch.isnan(buf[:at]).all()) and bool(torch.isnan(buf[at + view.numel():]).all())


# ================================================================================================ Philox and randn
SEEDS = [(0, 0), (0, 1), (2 ** 32 + 5, 0), (2 ** 63 + 7, 2 ** 32 - 2), (123, 250000)]
RANDN_COUNTS = [1, 3, 4, 5, 1023, 1024, 1025, STRIDE * 4 + 6]
RANDN_BAR = 1e-5      # absolute: theta is rounded as the kernel rounds it, so only logf, sqrtf and sincosf differ from
#                       float64 - a few float32 ulp of each at a radius of at most 5.8 stays below 4e-6
randn_worst = [0.0]


@pytest.mark.parametrize("seed,offset", SEEDS)
def test_randn_matches_philox_reference(gpu, seed, offset):
    """Every value of `ops.randn` is the Box-Muller image of the reference's Philox words; a bit-level mistake (shift,
    word order, counter, key) moves values by order 1.  The element behind `count` stays untouched."""
    from curvature_amd import ops
    want_all = R.philox_normals(seed, offset, max(RANDN_COUNTS))
    for count in RANDN_COUNTS:
        buf = torch.full((count + 1,), NAN, device=gpu)
        out = ops.randn((count,), gpu, seed, offset=offset, out=buf[:count])
        assert out.data_ptr() == buf.data_ptr()
        got = buf.cpu()
        assert torch.isnan(got[count]), f"count {count}: wrote past the end"
        dev = float((got[:count].double() - torch.tensor(want_all[:count])).abs().max())
        randn_worst[0] = max(randn_worst[0], dev)
        print(f"randn seed {seed} offset {offset} count {count}: max |dev| {dev:.3e} (worst so far {randn_worst[0]:.3e})")
        assert dev <= RANDN_BAR, (seed, offset, count, dev)


def test_randn_first_quad_is_the_first_known_answer(gpu):
    """Seed 0, offset 0: the words are the published zero-counter, zero-key vector."""
    from curvature_amd import ops
    words = np.array([[0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]], dtype=np.uint64)
    got = ops.randn((4,), gpu, 0).double().cpu()
    assert float((got - torch.from_numpy(R.normals_from_words(words))).abs().max()) <= RANDN_BAR


@pytest.mark.parametrize("n,k", [(1025, 300), (6, 1), (STRIDE * 4 + 6 - 4 * 5, 5)])
def test_randn_stream_continuity(gpu, n, k):
    from curvature_amd import ops
    later = ops.randn((n,), gpu, 77, offset=k)
    whole = ops.randn((n + 4 * k,), gpu, 77)
    assert same_bits(later, whole[4 * k:])


@pytest.mark.parametrize("count", [1027, 8, 1])
def test_randn_device_counter(gpu, count):
    """The form a captured graph uses: the stream position lives on the device and advances by ceil(count / 4)."""
    from curvature_amd import ops
    seed, quads = 2 ** 40 + 3, (count + 3) // 4
    c = torch.zeros(1, dtype=torch.int64, device=gpu)
    bufs = [torch.full((count + 1,), NAN, device=gpu) for _ in range(2)]
    for buf in bufs:
        ops.randn((count,), gpu, seed, out=buf[:count], counter=c)
    assert same_bits(bufs[0][:count], ops.randn((count,), gpu, seed, offset=0))
    assert same_bits(bufs[1][:count], ops.randn((count,), gpu, seed, offset=quads))
    assert int(c.item()) == 2 * quads
    assert all(bool(torch.isnan(buf[count])) for buf in bufs)


# ================================================================================================ elementwise.hip
RSQ_COUNTS = [1, 3, 4, 5, 1023, 1024, 1025, 2 ** 21 + 2 ** 10 + 7]
RSQ_PAIRS = [(3.0, 0.25), (1e-3, 1e-7), (1.0, 0.0)]          # (s, n)
_rsq_cache = {}


def rsq_values():
    """Log-uniform over 1e-12 .. 1e6 with exact zeros sprinkled in (CPU, float32, shared by every case)."""
    if "v" not in _rsq_cache:
        g = torch.Generator().manual_seed(11)
        v = torch.pow(10.0, torch.rand(max(RSQ_COUNTS), generator=g, dtype=torch.float64) * 18 - 12).float()
        v[::97] = 0.0
        v[3] = 0.0
        _rsq_cache["v"] = v
    return _rsq_cache["v"]


def rsq_reference(s, n, count):
    """The rounding sequence the kernel promises, in float32 on the CPU with the scalars cast to float32 first: mul, add, a
    correctly rounded reciprocal, a correctly rounded square root - what `torch.reciprocal(s * v + n).sqrt()` spells.
    torch's own float32 sqrt on the CPU is not correctly rounded on every host (measured on two x86 hosts: one ulp off in
    17 % of these elements on one and in 0.7 % on the other; its reciprocal was exact on both), so the same four operations
    are numpy's, which are the IEEE ones, and each of the last two is checked here against its float64 value rounded once
    (rounding a float64 quotient or root of float32 operands to float32 is the correctly rounded float32 result:
    53 >= 2 * 24 + 2).  How far this host's torch is from it is printed, not asserted."""
    if (s, n) not in _rsq_cache:
        v = rsq_values().numpy()
        with np.errstate(divide="ignore"):
            x = np.float32(s) * v + np.float32(n)
            r = np.float32(1) / x
            want = np.sqrt(r)
            assert x.dtype == r.dtype == want.dtype == np.float32
            assert np.array_equal(r, (1.0 / x.astype(np.float64)).astype(np.float32))
            assert np.array_equal(want, np.sqrt(r.astype(np.float64)).astype(np.float32))
        by_torch = torch.reciprocal(torch.tensor(s, dtype=torch.float32) * rsq_values()
                                    + torch.tensor(n, dtype=torch.float32)).sqrt()
        print(f"rsqrt_affine reference (s, n) = ({s}, {n}): this host's torch.reciprocal(...).sqrt() differs from the "
              f"correctly rounded sequence in {int((bits(by_torch) != bits(torch.from_numpy(want))).sum())} of {v.size}")
        _rsq_cache[(s, n)] = torch.from_numpy(want)
    return _rsq_cache[(s, n)][:count]


@pytest.mark.parametrize("shift_v,shift_out", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("s,n", RSQ_PAIRS)
def test_rsqrt_affine_bit_equal(gpu, s, n, shift_v, shift_out):
    """Bit equality with the reference's rounding sequence on the float4 path (both pointers 16-byte aligned: vector
    loop, second stride trip, scalar tail) and on the misaligned path (either pointer off by one float)."""
    from curvature_amd import ops
    for count in RSQ_COUNTS:
        _, v = fenced(count, gpu, shift=shift_v)
        v.copy_(rsq_values()[:count])
        obuf, out = fenced(count, gpu, shift=shift_out)
        assert v.data_ptr() % 16 == 4 * shift_v and out.data_ptr() % 16 == 4 * shift_out
        ops.rsqrt_affine(v, n, s, out=out)
        want = rsq_reference(s, n, count)
        got = out.cpu()
        bad = (bits(got) != bits(want)).nonzero().flatten()
        assert bad.numel() == 0, (count, bad.numel(), int(bad[0]), float(got[bad[0]]), float(want[bad[0]]))
        assert fence_intact(obuf, out), count
        assert same_bits(v, rsq_values()[:count])                       # the source is only read


@pytest.mark.parametrize("shift", [0, 1])
def test_rsqrt_affine_in_place(gpu, shift):
    from curvature_amd import ops
    s, n = RSQ_PAIRS[0]
    for count in [1, 5, 1025, RSQ_COUNTS[-1]]:
        buf, v = fenced(count, gpu, shift=shift)
        v.copy_(rsq_values()[:count])
        ops.rsqrt_affine(v, n, s, out=v)
        assert same_bits(v, rsq_reference(s, n, count)), count
        assert fence_intact(buf, v)


@pytest.mark.parametrize("count", [1, 257, STRIDE + 3])
@pytest.mark.parametrize("s", [0.5, 3.0, 1e-3])
def test_sqrt_scale_within_one_ulp(gpu, s, count):
    """sqrt(s * v): a rounded product under a rounded square root, at most 1 float32 ulp from the float64 value."""
    from curvature_amd import ops
    g = torch.Generator().manual_seed(count)
    v = torch.pow(10.0, torch.rand(count, generator=g, dtype=torch.float64) * 12 - 6).float()
    v[::5] = 0.0
    want = torch.sqrt(torch.tensor(s, dtype=torch.float32).double() * v.double())
    got = ops.sqrt_scale(v.to(gpu), s).cpu()
    assert got.shape == v.shape and torch.equal(got[::5], torch.zeros_like(got[::5]))
    assert bool(((got.double() - want).abs() <= R.ulp32(want)).all())


@pytest.mark.parametrize("count", [1, 255, 256, 257, STRIDE - 1, STRIDE, STRIDE + 3])
def test_clamp_min0_exact(gpu, count):
    from curvature_amd import ops
    g = torch.Generator().manual_seed(count)
    v = torch.randn(count, generator=g)
    special = torch.tensor([-1e-40, float("-inf"), NAN, float("inf"), 1e-40, -1.4e-45, 0.0, -3.5])
    k = min(count, special.numel())
    v[:k] = special[:k]
    v[count - 1] = special[(count - 1) % 2]                            # the last element is a negative one too
    assert v[0] < 0 and v[0] > -1e-38                                  # a negative denormal, not flushed on the CPU
    want = torch.where(v < 0, torch.zeros_like(v), v)                  # NaN < 0 is false: NaN stays; +0, never -0
    buf, x = fenced(count, gpu, shift=1)
    x.copy_(v)
    assert ops.clamp_min0_(x).data_ptr() == x.data_ptr()
    assert same_bits(x, want)
    assert fence_intact(buf, x)


@pytest.mark.parametrize("count", [1, 255, 256, 257, STRIDE + 3])
@pytest.mark.parametrize("form", ["fresh", "out_is_a", "out_is_b", "a_is_b", "a_is_b_is_out"])
def test_mul_bit_equal_and_in_place(gpu, form, count):
    """out = a * b, one rounding; the samplers call it with out = a (z *= inv) and with a = b (r * r)."""
    from curvature_amd import ops
    g = torch.Generator().manual_seed(count)
    a, b = torch.randn(count, generator=g), torch.randn(count, generator=g)
    if form.startswith("a_is_b"):
        b = a
    want = a * b
    da = a.to(gpu)
    db = da if b is a else b.to(gpu)
    out = {"fresh": None, "out_is_a": da, "out_is_b": db, "a_is_b": None, "a_is_b_is_out": da}[form]
    got = ops.mul(da, db, out=out)
    assert out is None or got.data_ptr() == out.data_ptr()
    assert same_bits(got, want)
    if form in ("fresh", "a_is_b"):
        assert same_bits(da, a) and same_bits(db, b)                   # operands only read


@pytest.mark.parametrize("sa,sb", [((1, 1), (1, 1)), ((3, 5), (7, 2)), ((1, 9), (4, 1)), ((64, 64), (16, 16))])
def test_kron_bit_equal(gpu, sa, sb):
    from curvature_amd import ops
    g = torch.Generator().manual_seed(sa[0] * 100 + sb[1])
    a, b = torch.randn(*sa, generator=g), torch.randn(*sb, generator=g)
    got = ops.kron(a.to(gpu), b.to(gpu))
    assert same_bits(got, torch.kron(a, b))


def test_kron_refuses_float64(gpu):
    from curvature_amd import ops
    a, b = torch.randn(3, 5, device=gpu), torch.randn(2, 2, device=gpu)
    with pytest.raises(RuntimeError):
        ops.kron(a.double(), b)
    with pytest.raises(RuntimeError):
        ops.kron(a, b.double())


def sq_reference(gw, gb, bs, state):
    """(state + val, val) in float64 with val = bs * [gw.view(rows, -1) | gb]^2."""
    g = gw.double().reshape(gw.shape[0], int(np.prod(gw.shape[1:])))     # (not -1: rows may be 0)
    if gb is not None:
        g = torch.cat([g, gb.double()[:, None]], dim=1)
    val = bs * g * g
    return (val if state is None else state.double() + val), val


def sq_close(got, state, val):
    """Elementwise 3 * 2^-24 * (|state| + |val|): up to three roundings (g * g, * bs, + state), fma contraction allowed."""
    prev = torch.zeros_like(val) if state is None else state.double()
    return bool(((got.double().cpu() - (prev + val)).abs() <= 3 * 2.0 ** -24 * (prev.abs() + val.abs())).all())


SQ_SHAPES = [((1, 7), True), ((1, 7), False), ((5, 1), True), ((5, 1), False), ((5, 3, 2, 2), True), ((5, 3, 2, 2), False),
             ((700, 750), False), ((700, 750), True)]


@pytest.mark.parametrize("shape,bias", SQ_SHAPES)
def test_sq_accumulate(gpu, shape, bias):
    from curvature_amd import ops
    g = torch.Generator().manual_seed(len(shape) * 10 + shape[0] + bias)
    gw = torch.randn(*shape, generator=g)
    gb = torch.randn(shape[0], generator=g) if bias else None
    bs = 8.0
    dw, db = gw.to(gpu), (gb.to(gpu) if bias else None)
    rows, cols = shape[0], gw[0].numel() + bias
    _, val = sq_reference(gw, gb, bs, None)
    # first=True on a NaN-filled state: overwritten, no NaN survives
    buf, st = fenced(rows * cols, gpu, shift=1)
    st = st.view(rows, cols)
    assert ops.sq_accumulate(dw, db, bs, st, first=True).data_ptr() == st.data_ptr()
    assert not bool(torch.isnan(st).any()) and sq_close(st, None, val) and fence_intact(buf, st)
    # first=False adds to what the state holds
    state = torch.randn(rows, cols, generator=g)
    buf, st = fenced(rows * cols, gpu)
    st = st.view(rows, cols).copy_(state)
    ops.sq_accumulate(dw, db, bs, st, first=False)
    assert sq_close(st, state, val) and fence_intact(buf, st)
    # first=None: a state allocated by the call is overwritten, a given one is added to
    fresh = ops.sq_accumulate(dw, db, bs, None)
    assert fresh.shape == (rows, cols) and sq_close(fresh, None, val)
    st = state.to(gpu, copy=True)
    ops.sq_accumulate(dw, db, bs, st)
    assert sq_close(st, state, val)


def sq_items(count):
    """`count` (grad_w, grad_b, initial state or None, first) CPU items: element counts around the 1024-element block of
    the batched kernel, two rows = 0 items in the middle of the first chunk and one on each side of the 96-item split."""
    shapes = [((1, 1), False), ((1, 1023), False), ((1, 1024), False), ((5, 205), False), ((3, 683), False), ((3, 4), True),
              ((2, 511), True), ((7, 3, 2, 2), True), ((1, 2048), False), ((4, 512), True), ((1, 1), True), ((33, 31), True)]
    empties = {40: ((0, 5), True), 41: ((0, 3, 2, 2), False), 95: ((0, 1), False), 96: ((0, 1024), True)}
    g = torch.Generator().manual_seed(count)
    items = []
    for i in range(count):
        shape, bias = empties.get(i, shapes[i % len(shapes)])
        gw = torch.randn(*shape, generator=g)
        gb = torch.randn(shape[0], generator=g) if bias else None
        rows, cols = shape[0], int(np.prod(shape[1:])) + bias
        mode = (i // len(shapes) + i) % 4               # first=True on NaNs | first=False | None, allocated | None, given
        state = [torch.full((rows, cols), NAN), torch.randn(rows, cols, generator=g), None,
                 torch.randn(rows, cols, generator=g)][mode]
        items.append((gw, gb, state, [True, False, None, None][mode]))
    return items


@pytest.mark.parametrize("count", [97, 200])
def test_sq_accumulate_many_equals_single_calls(gpu, count):
    """More than 96 items go out in several launches; every state must hold what a single `sq_accumulate` of its item
    gives, bit for bit (and what float64 gives, within the bar of the single call); rows = 0 items are skipped without
    moving anyone's block range, and nothing outside a state is written."""
    from curvature_amd import ops
    items = sq_items(count)
    assert sum(gw.shape[0] == 0 for gw, _, _, _ in items) >= 3
    batched, bufs, singles = [], [], []
    for gw, gb, state, first in items:
        dw, db = gw.to(gpu), (gb.to(gpu) if gb is not None else None)
        singles.append(ops.sq_accumulate(dw, db, 0.75, None if state is None else state.to(gpu, copy=True), first))
        st = None
        if state is not None and state.numel() == 0:
            st = state.to(gpu, copy=True)
        elif state is not None:
            buf, st = fenced(state.numel(), gpu, shift=len(bufs) % 2)
            st = st.view(state.shape).copy_(state)
            bufs.append((buf, st))
        batched.append((dw, db, st, first))
    got = ops.sq_accumulate_many(batched, 0.75)
    assert len(got) == count
    for i, (out, single, (gw, gb, state, first)) in enumerate(zip(got, singles, items)):
        assert same_bits(out, single), i
        added_to = None if (first is True or state is None) else state
        assert sq_close(out, added_to, sq_reference(gw, gb, 0.75, None)[1]), i
        assert not bool(torch.isnan(out).any()), i
        if batched[i][2] is not None:
            assert out.data_ptr() == batched[i][2].data_ptr()
    assert all(fence_intact(buf, st) for buf, st in bufs)


def test_concat_many_parts(gpu):
    """More than 96 buffers (several copy launches), destination offsets of every alignment, one empty part."""
    from curvature_amd import ops
    sizes = [1, 3, 4, 17, 0, 16385, 5] + [7 + i for i in range(100)]
    g = torch.Generator().manual_seed(5)
    parts = [torch.randn(s, generator=g) for s in sizes]
    got = ops.concat([p.to(gpu) for p in parts])
    assert same_bits(got, torch.cat(parts))


# ================================================================================================ inf.hip
def view_of(kind, rows, cols, g, gpu):
    """(CPU view, GPU view of the same storage layout) of shape (rows, cols): contiguous, transposed or x[::2, 1::3]."""
    if kind == "contiguous":
        x = torch.randn(rows, cols, generator=g)
        return x, x.to(gpu)
    if kind == "transposed":
        x = torch.randn(cols, rows, generator=g)
        return x.t(), x.to(gpu).t()
    x = torch.randn(2 * rows, 3 * cols + 1, generator=g)
    return x[::2, 1::3], x.to(gpu)[::2, 1::3]


KINDS = ["contiguous", "transposed", "strided"]


@pytest.mark.parametrize("kind", KINDS)
def test_gather2d(gpu, kind):
    from curvature_amd import ops
    g = torch.Generator().manual_seed(3)
    src, dsrc = view_of(kind, 37, 53, g, gpu)
    assert dsrc.shape == (37, 53) and dsrc.stride() == src.stride()
    rows = [torch.tensor([36, 0, 5, 5, 17, 0, 36, 2]), torch.tensor([9]), None]
    cols = [torch.tensor([52, 52, 1, 0, 30, 7, 7, 7, 51, 3, 0]), torch.tensor([52]), None]
    for ri in rows:
        for ci in cols:
            want = src
            if ri is not None:
                want = want.index_select(0, ri)
            if ci is not None:
                want = want.index_select(1, ci)
            want = want.contiguous()
            dri, dci = (None if ri is None else ri.to(gpu)), (None if ci is None else ci.to(gpu))
            assert same_bits(ops.gather2d(dsrc, dri, dci), want)
            buf, out = fenced(want.numel(), gpu, shift=1)
            out = out.view(want.shape)
            assert ops.gather2d(dsrc, dri, dci, out=out).data_ptr() == out.data_ptr()
            assert same_bits(out, want) and fence_intact(buf, out)


@pytest.mark.parametrize("kind", KINDS)
def test_gather2d_second_stride_trip(gpu, kind):
    from curvature_amd import ops
    g = torch.Generator().manual_seed(4)
    src, dsrc = view_of(kind, 800, 700, g, gpu)                        # 560000 elements: more than 2048 x 256 threads
    assert same_bits(ops.gather2d(dsrc), src.contiguous())
    ri, ci = torch.randperm(800, generator=g), torch.randint(0, 700, (700,), generator=g)
    assert same_bits(ops.gather2d(dsrc, ri.to(gpu), ci.to(gpu)), src.index_select(0, ri).index_select(1, ci).contiguous())


@pytest.mark.parametrize("kind_b", KINDS)
@pytest.mark.parametrize("kind_a", KINDS)
def test_mul2d(gpu, kind_a, kind_b):
    from curvature_amd import ops
    g = torch.Generator().manual_seed(6)
    for rows, cols in [(1, 1), (37, 53), (700, 800)]:
        (a, da), (b, db) = view_of(kind_a, rows, cols, g, gpu), view_of(kind_b, rows, cols, g, gpu)
        want = (a * b).contiguous()
        assert same_bits(ops.mul2d(da, db), want)
        buf, out = fenced(rows * cols, gpu, shift=1)
        out = out.view(rows, cols)
        assert ops.mul2d(da, db, out=out).data_ptr() == out.data_ptr()
        assert same_bits(out, want) and fence_intact(buf, out)


PAIR_SHAPES = [(1, 1), (5, 2), (300, 7), (17, 33), (2100, 16)]          # the last: 537600 products, a second stride trip


@pytest.mark.parametrize("n,a", PAIR_SHAPES)
def test_colpairs(gpu, n, a):
    """out[p, i a + k] = U[p, i] U[p, k]: one rounding in float32, exact in float64; the packed form keeps i <= k at
    column t(i, k), the position of (i, k) when the pairs are enumerated in order."""
    from curvature_amd import ops
    g = torch.Generator().manual_seed(n + a)
    U = torch.randn(n, a, generator=g)
    dU = U.to(gpu)
    assert same_bits(ops.colpairs(dU), (U[:, :, None] * U[:, None, :]).reshape(n, a * a))
    exact = (U.double()[:, :, None] * U.double()[:, None, :])
    assert same_bits(ops.colpairs(dU, f64=True), exact.reshape(n, a * a))
    t = R.packed_map(a)
    want = torch.full((n, a * (a + 1) // 2), NAN, dtype=torch.float64)
    for i in range(a):
        for k in range(i, a):
            want[:, t[i, k]] = exact[:, i, k]
    assert not bool(torch.isnan(want).any())
    got = ops.colpairs_sym(dU)
    assert got.dtype == torch.float64 and same_bits(got, want)


@pytest.mark.parametrize("count", [1, 257, STRIDE + 3])
def test_square_f64_exact(gpu, count):
    from curvature_amd import ops
    v = torch.randn(count, generator=torch.Generator().manual_seed(count))
    got = ops.square_f64(v.to(gpu))
    assert got.dtype == torch.float64 and same_bits(got, v.double() ** 2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("rows,cols", [(3, 7), (257, 65), (900, 600)])
def test_diag_scale(gpu, rows, cols, dtype):
    """float32(src[i, j] dl[i] dr[j]) from a float64 product: at most 1 ulp from the float64 product rounded to float32."""
    from curvature_amd import ops
    g = torch.Generator().manual_seed(rows)
    src = torch.randn(rows, cols, generator=g, dtype=dtype)
    dl, dr = torch.randn(rows, generator=g), torch.rand(cols, generator=g) + 0.5
    want = src.double() * dl.double()[:, None] * dr.double()[None, :]

    def close(got):
        return got.dtype == torch.float32 and bool(((got.double().cpu() - want).abs() <= R.ulp32(want)).all())

    dsrc, ddl, ddr = src.to(gpu), dl.to(gpu), dr.to(gpu)
    assert close(ops.diag_scale(dsrc, ddl, ddr))                               # a fresh output
    buf, out = fenced(rows * cols, gpu)
    out = out.view(rows, cols)
    assert ops.diag_scale(dsrc, ddl, ddr, out=out).data_ptr() == out.data_ptr()   # a reused one
    assert close(out) and fence_intact(buf, out) and same_bits(dsrc, src)
    if dtype == torch.float32:                                                  # in place
        assert ops.diag_scale(dsrc, ddl, ddr, out=dsrc).data_ptr() == dsrc.data_ptr()
        assert close(dsrc)


def test_diag_scale_refuses_wrong_vector_lengths(gpu):
    from curvature_amd import ops
    src = torch.randn(5, 7, device=gpu)
    ok_l, ok_r = torch.ones(5, device=gpu), torch.ones(7, device=gpu)
    for dl, dr in [(ok_l[:4], ok_r), (ok_l, ok_r[:6]), (ok_r, ok_l), (torch.ones(6, device=gpu), ok_r)]:
        with pytest.raises(RuntimeError, match="diag_scale"):
            ops.diag_scale(src, dl, dr)
    ops.diag_scale(src, ok_l, ok_r)


AB = [(1, 1), (1, 4), (3, 5), (6, 2), (30, 25)]                      # the last: 562500 outputs, a second stride trip


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("a,b", AB)
def test_inf_vtv_assemble_unsymmetric_input(gpu, a, b, dtype):
    """vtv = (w + w^T) / 2 of a V4 that is NOT symmetric under (i, k) <-> (k, i), (j, l) <-> (l, j): the two terms of the
    kernel differ, so each index expression is checked on its own (every V4 of the estimators makes them equal)."""
    from curvature_amd import ops
    g = torch.Generator().manual_seed(a * 10 + b)
    V4 = torch.randn(a * a, b * b, generator=g, dtype=dtype)
    sigma = torch.rand(a * b, generator=g) + 0.5
    w = R.vtv_unsymmetrised(V4, sigma, a, b)
    want = (w + w.t()) / 2
    got = ops.inf_vtv_assemble(V4.to(gpu), sigma.to(gpu), a, b)
    assert got.dtype == dtype and got.shape == (a * b, a * b)
    assert torch.equal(got, got.t())
    bar = 4 * torch.finfo(dtype).eps * (w.abs() + w.t().abs()) / 2
    assert bool(((got.double().cpu() - want).abs() <= bar).all())
    if a * b > 1:                                                    # the input does tell the two terms apart
        assert float((w - w.t()).abs().max()) > 0.1


@pytest.mark.parametrize("a,b", AB)
def test_inf_vtv_assemble_sym_packed_input(gpu, a, b):
    from curvature_amd import ops
    g = torch.Generator().manual_seed(a * 10 + b + 1)
    V4p = torch.randn(a * (a + 1) // 2, b * (b + 1) // 2, generator=g, dtype=torch.float64)
    sigma = torch.rand(a * b, generator=g) + 0.5
    want = R.vtv_from_packed(V4p, sigma, a, b)
    got = ops.inf_vtv_assemble_sym(V4p.to(gpu), sigma.to(gpu), a, b).cpu()
    assert got.dtype == torch.float64 and torch.equal(got, got.t())
    assert bool(((got - want).abs() <= 3 * 2.0 ** -53 * want.abs()).all())


def test_inf_vtv_forms_agree_on_column_pair_input(gpu):
    """Both forms on a genuine Khatri-Rao input, where the full form's symmetrisation averages equal terms."""
    from curvature_amd import ops
    torch.manual_seed(21)
    n, m, a, b = 70, 33, 7, 5
    ua, ug = torch.randn(n, a, device=gpu), torch.randn(m, b, device=gpu)
    sigma = torch.rand(a * b, device=gpu) + 0.5
    r2 = ops.square_f64(torch.rand(n * m, device=gpu) + 0.1).view(n, m)
    full = ops.inf_vtv_assemble(ops.gemm_f64(ops.gemm_f64(ops.colpairs(ua, f64=True).t(), r2),
                                             ops.colpairs(ug, f64=True)).contiguous(), sigma, a, b)
    packed = ops.inf_vtv_assemble_sym(ops.gemm_f64(ops.gemm_f64(ops.colpairs_sym(ua).t(), r2),
                                                   ops.colpairs_sym(ug)).contiguous(), sigma, a, b)
    assert torch.allclose(packed, full, rtol=1e-13, atol=1e-13) and torch.equal(packed, packed.t())


def test_inf_vtv_assemble_refuses_wrong_sizes(gpu):
    from curvature_amd import ops
    a, b = 3, 5
    V4, sigma = torch.randn(a * a, b * b, device=gpu), torch.ones(a * b, device=gpu)
    ops.inf_vtv_assemble(V4, sigma, a, b)
    for args in [(V4, sigma, b, a), (V4, sigma, a, b + 1), (V4[:, :-1].contiguous(), sigma, a, b),
                 (V4, sigma[:-1], a, b), (V4, torch.ones(a * b + 1, device=gpu), a, b), (V4.view(-1), sigma, a, b)]:
        with pytest.raises(RuntimeError, match="inf_vtv_assemble"):
            ops.inf_vtv_assemble(*args)


def distinct_magnitudes(total, g):
    """A random permutation of `total` distinct positive magnitudes under random signs."""
    mags = (torch.arange(1, total + 1, dtype=torch.float64) / total).float()
    assert torch.unique(mags).numel() == total
    return mags[torch.randperm(total, generator=g)] * (torch.randint(0, 2, (total,), generator=g) * 2 - 1).float()


def check_select(gpu, lam, n, m, rank):
    from curvature_amd import ops
    I, J = ops.inf_select(lam.to(gpu), n, m, rank)
    Ir, Jr = R.select_reference(lam, n, m, rank)
    assert I.dtype == torch.int64 and J.dtype == torch.int64
    assert torch.equal(I.cpu(), Ir) and torch.equal(J.cpu(), Jr)


@pytest.mark.parametrize("n,m,rank", [(8192, 2, 100), (2, 8192, 100), (1, 1, 1), (300, 200, 60000), (7, 5, 10 ** 9),
                                      (300, 200, 59999), (33, 31, 1), (64, 17, 1024)])
def test_inf_select_tie_free(gpu, n, m, rank):
    check_select(gpu, distinct_magnitudes(n * m, torch.Generator().manual_seed(n + m)), n, m, rank)


@pytest.mark.parametrize("rank", [1, 40, 255, 256])
def test_inf_select_last_radix_pass_decides(gpu, rank):
    """Keys 1 + k 2^-23, k < 256: they differ in their lowest mantissa byte only."""
    g = torch.Generator().manual_seed(rank)
    lam = (1.0 + torch.arange(256, dtype=torch.float64) * 2.0 ** -23).float()
    assert torch.unique(lam).numel() == 256
    lam = lam[torch.randperm(256, generator=g)] * (torch.randint(0, 2, (256,), generator=g) * 2 - 1).float()
    check_select(gpu, lam, 16, 16, rank)


@pytest.mark.parametrize("rank", [1, 20, 45, 64, 90])
def test_inf_select_denormals_and_negative_zero(gpu, rank):
    """30 distinct denormals, one -0.0 and 59 normal values: the key is the bit pattern of |x|, so denormals order
    above zero and below every normal value."""
    g = torch.Generator().manual_seed(rank)
    den = torch.from_numpy(np.arange(1, 31, dtype=np.int32) * 1009).view(torch.float32)
    nor = torch.pow(10.0, torch.linspace(-30, 5, 59))
    lam = torch.cat([den, torch.tensor([-0.0]), nor])
    assert bool((den > 0).all()) and bool((den < 1.2e-38).all()) and torch.unique(lam.abs()).numel() == 90
    lam = lam[torch.randperm(90, generator=g)] * (torch.randint(0, 2, (90,), generator=g) * 2 - 1).float()
    assert int((lam != 0).sum()) == 89                                 # the denormals survived the CPU
    check_select(gpu, lam, 9, 10, rank)


@pytest.mark.parametrize("r", [1, 3, 6])
@pytest.mark.parametrize("n,m,tie", [(40, 30, 1.0), (12, 11, 0.5), (90, 70, 2.0 ** -130)])
def test_inf_select_takes_exactly_the_missing_ties(gpu, n, m, tie, r):
    """Six strict winners in rows 0 .. 2 and columns 0 .. 3, seven values of one magnitude at (4 + q, 4 + q) - a row and
    a column each that no winner and no other tie uses - and everything else strictly smaller: with rank = 6 + r the
    lists hold the winners' rows / columns plus those of exactly r tied elements (which r is the kernel's choice)."""
    from curvature_amd import ops
    g = torch.Generator().manual_seed(n + r)
    lam = (torch.rand(n, m, generator=g) * 0.25 + 0.01) * tie * (torch.randint(0, 2, (n, m), generator=g) * 2 - 1).float()
    assert 0 < float(lam.abs().min()) and float(lam.abs().max()) < tie
    winners = [(0, 0), (0, 3), (1, 1), (2, 0), (2, 2), (1, 3)]
    for q, (i, j) in enumerate(winners):
        lam[i, j] = tie * (2.0 + q) * (-1) ** q
    tied = [(4 + q, 4 + q) for q in range(7)]
    for q, (i, j) in enumerate(tied):
        lam[i, j] = tie * (-1) ** q
    assert int((lam.abs() > tie).sum()) == 6 and int((lam.abs() == tie).sum()) == 7
    I, J = ops.inf_select(lam.reshape(-1).to(gpu), n, m, 6 + r)
    I, J = I.tolist(), J.tolist()
    assert I == sorted(set(I)) and J == sorted(set(J))
    assert len(I) == 3 + r and len(J) == 4 + r
    assert set(I) >= {0, 1, 2} and set(J) >= {0, 1, 2, 3}
    extra_rows, extra_cols = set(I) - {0, 1, 2}, set(J) - {0, 1, 2, 3}
    assert extra_rows <= {i for i, _ in tied} and extra_cols == extra_rows          # whole tied elements, nothing else


@pytest.mark.parametrize("layers", [33, 70])
def test_inf_select_many_equals_single_calls(gpu, layers):
    """More than 32 layers go out in several launches of one workgroup per layer, each with its own row of counts."""
    from curvature_amd import ops
    g = torch.Generator().manual_seed(layers)
    dims = [(1 + (7 * i) % 23, 1 + (5 * i) % 19) for i in range(layers)]
    dims[31], dims[32] = (120, 90), (3, 200)
    lams = [distinct_magnitudes(n * m, g) for n, m in dims]
    rank = 25
    many = ops.inf_select_many([l.to(gpu) for l in lams], dims, rank)
    assert len(many) == layers
    for (I, J), lam, (n, m) in zip(many, lams, dims):
        Is, Js = ops.inf_select(lam.to(gpu), n, m, rank)
        Ir, Jr = R.select_reference(lam, n, m, rank)
        assert torch.equal(I, Is) and torch.equal(J, Js)
        assert torch.equal(I.cpu(), Ir) and torch.equal(J.cpu(), Jr)
