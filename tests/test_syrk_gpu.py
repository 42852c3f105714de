"""Parity of the grouped implicit-im2col SYRK kernel (curv_kfac_accumulate) with the oracle's
F.unfold + mm restatement of curvature/curvatures.py:329-350.  Tolerance: 1e-4 relative Frobenius
(north_star); the kernel is exact-fp32 MFMA so the observed error is ~1e-6."""
import functools
import math

import pytest
import torch

from conftest import rel_fro
from exact_inputs import assert_exact_range, conv_rows, exact_gram, flat_rows, nonzero_ints, pow2_scale, wide_ints

pytestmark = pytest.mark.gpu

TOL = 1e-4

FENCE = 4096              # NaN floats in front of a fenced source
FENCE_AFTER = 1 << 18     # and behind it (1 MiB: more than any staging form fetches past a source's end)
OFFSETS = (0, 1)          # a source's start: on a 16-byte boundary, and 4 bytes past one (storage_offset % 4 == 1)


def fenced(shape, offset, device="cuda:0"):
    """A contiguous NaN-filled view of `shape` inside a NaN-filled buffer, `offset` floats past a 16-byte boundary (a
    narrowed batch such as x[1:] starts like that).  A kernel that lets anything outside its source reach the result
    puts NaN into it."""
    n = math.prod(shape)
    buf = torch.full((FENCE + offset + n + FENCE_AFTER,), float("nan"), device=device)
    view = buf[FENCE + offset:FENCE + offset + n].view(shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * offset
    return view


def fenced_copy(t, offset):
    return fenced(tuple(t.shape), offset).copy_(t)


@pytest.fixture(autouse=True, params=["grouped", "small"])
def build_path(request, monkeypatch):
    """Every case of this file runs twice: through the grouped build of syrk.hip (what a model that fills the GPU gets:
    every descriptor carries path_hint = PATH_GROUPED, KFAC.update's included) and with the two-launch small-model build
    of syrk_small.hip allowed (what most of these geometries - a handful of samples - are routed to by default; cases
    above its size limit take the grouped path in both runs)."""
    if request.param == "grouped":
        from curvature_amd import _lib, ops
        descs = ops._factor_descs

        def grouped(*args, **kwargs):
            arr = descs(*args, **kwargs)
            for d in arr:
                d.path_hint = _lib.PATH_GROUPED
            return arr
        monkeypatch.setattr(ops, "_factor_descs", grouped)
    return request.param


# (N, C, H, W, kernel, stride, padding, bias[, Cout: width of the G side, 37 if not given])
CONV_CASES = [
    (3, 1, 28, 28, 5, 1, 2, True),      # LeNet conv1
    (3, 6, 14, 14, 5, 1, 0, True),      # LeNet conv2
    (2, 3, 32, 32, 7, 2, 3, False),     # ResNet stem shape (small spatial)
    (2, 16, 12, 12, 3, 1, 1, False),    # 3x3 s1
    (2, 16, 13, 13, 3, 2, 1, False),    # 3x3 s2, odd size
    (2, 24, 9, 9, 1, 2, 0, False),      # 1x1 s2 downsample
    (2, 70, 7, 7, 1, 1, 0, False),      # 1x1 s1, odd L=49, n > 64
    (1, 130, 5, 6, 3, 1, 1, True),      # many tiles (n = 1171), bias, non-square
    (2, 8, 40, 150, 3, 1, 1, False),    # wide rows -> column-split chunks
    (5, 4, 6, 6, (3, 1), (1, 2), (0, 1), True),  # anisotropic kernel/stride/padding
    (2, 64, 8, 8, 1, 1, 0, False),      # flattened 1x1, 16-byte rows: float4 staging, 64x64 tiles
    (2, 256, 4, 4, 1, 1, 0, False),     # float4 staging, 128x128 tiles, several samples per chunk
    # kh x kw > 1 with full-width chunks: patch images staged by LDS-DMA from the pre-tiled copy (syrk_pre.hip)
    (3, 256, 7, 7, 3, 1, 1, False),     # odd width, 16 channels per panel, several samples per chunk (ragged group)
    (2, 5, 9, 9, 3, 1, 1, True),        # channel count below a panel's, bias row
    (2, 40, 10, 10, 3, 2, 1, False),    # stride 2, even width
    (5, 64, 7, 7, 3, 2, 1, False),      # stride 2, odd sample count in sample groups
    (3, 32, 30, 30, 3, 1, 1, False),    # several output-row groups, the last one ragged
    (2, 3, 64, 64, 7, 2, 3, True),      # stem-like 7x7 / stride 2 with a bias row, 64x64 tiles
    (3, 512, 14, 14, 3, 2, 1, False),   # ResNet-50 layer4.0.conv2 geometry: 4608-wide factor, panels ending past C
    (2, 20, 11, 23, 5, 1, 2, True),     # 5x5, non-square, odd sizes
    # 3x3 / stride 1 / pad 1 with C % 128 == 0 and N >= 8: assembled from shifted correlations (syrk_corr.hip)
    (8, 128, 14, 14, 3, 1, 1, False),   # ResNet layer3-like
    (8, 256, 7, 7, 3, 1, 1, False),     # layer4-like: odd size, border strips are half of the image
    (9, 128, 12, 21, 3, 1, 1, False),   # non-square, odd width, odd sample count
    (8, 128, 3, 3, 3, 1, 1, False),     # smallest image: every pixel is a border pixel
    # the same with exactly 64 channels: packed pair tiles (four shifted correlations per 128x128 tile)
    (8, 64, 14, 14, 3, 1, 1, False),    # ResNet layer1-like
    (9, 64, 12, 21, 3, 1, 1, False),    # non-square, odd width, odd sample count
    (8, 64, 3, 3, 3, 1, 1, False),      # smallest image
    (8, 64, 56, 56, 3, 1, 1, False),    # ResNet-50 layer1 geometry (K = 26 k positions per sample: many k-slices)
    # DenseNet-121 / 161 (README.rst:259-267): 1x1 convolutions whose input width grows by 32 / 48 per unit, 3x3 with 128 /
    # 192 input channels (192: no multiple of 128 - not eligible for the shifted-correlation path), transitions
    (8, 96, 56, 56, 1, 1, 0, False),    # block 1, unit 2: C = 64 + 32
    (8, 224, 56, 56, 1, 1, 0, False),   # block 1, last unit
    (8, 128, 56, 56, 3, 1, 1, False),   # every 3x3 of DenseNet-121, at block 1's resolution
    (8, 256, 56, 56, 1, 1, 0, False),   # transition 1
    (8, 480, 28, 28, 1, 1, 0, False),   # block 2, last unit
    (8, 992, 7, 7, 1, 1, 0, False),     # block 4, last unit
    (8, 192, 28, 28, 3, 1, 1, False),   # DenseNet-161's 3x3
    (8, 336, 28, 28, 1, 1, 0, False),   # DenseNet-161 block 2: C = 192 + 3 * 48
    (5, 144, 9, 13, 1, 1, 0, False),    # DenseNet-161 block 1: C = 96 + 48 (a ragged tile whose edge cuts a 32 x 32 MFMA block)
    (3, 1104, 7, 7, 1, 1, 0, False),    # DenseNet-161 block 4
    # 1x1 with a stride and at least 96 channels: compact copy of the sampled pixels, then the LDS-DMA kernel
    (3, 128, 9, 11, 1, 2, 0, False),    # odd sizes: Ho x Wo = 5 x 6 = 30 pixels (rows of 7.5 groups: ragged row ends)
    (2, 256, 14, 14, 1, 2, 0, False),   # ResNet down-sampling shape, 49 pixels per row
    (4, 96, 10, 13, (1, 1), (2, 3), (0, 0), False),   # anisotropic stride, ragged tile
    (5, 64, 9, 9, 1, 2, 0, False),      # 64 channels: stays on the register-staged kernel
    # exactly 64 channels, flattened (a pair-tile form of the LDS-DMA kernel was built and measured slower, LAB_NOTEBOOK R6)
    (5, 64, 9, 9, 1, 1, 0, False),      # odd sample count, 81 pixels per row
    (3, 64, 7, 7, 1, 1, 0, False),      # 49 pixels
    # G sides on the LDS-DMA kernel too (Cout >= 96, a multiple of 16): ResNet-50 layer4's 1x1 convolutions at 7 x 7 (the
    # last group of every (sample, channel) row holds one pixel), a 3x3 beside them, and a 64-pixel image (no row end
    # inside a group)
    (8, 512, 7, 7, 1, 1, 0, False, 2048),   # layer4.x.conv3: 512 -> 2048
    (8, 2048, 7, 7, 1, 1, 0, False, 512),   # layer4.x.conv1: 2048 -> 512
    (8, 512, 7, 7, 3, 1, 1, False, 256),    # layer4.x.conv2-like, G at 256
    (8, 128, 8, 8, 1, 1, 0, False, 256),    # Ho * Wo % 4 == 0 on both sides
]


def _oracle():
    import oracle.curvature_oracle as o
    return o


def _unpack(case):
    N, C, H, W, k, s, p, bias = case[:8]
    Cout = case[8] if len(case) > 8 else 37
    k2 = (k, k) if isinstance(k, int) else k
    s2 = (s, s) if isinstance(s, int) else s
    p2 = (p, p) if isinstance(p, int) else p
    Ho = (H + 2 * p2[0] - k2[0]) // s2[0] + 1
    Wo = (W + 2 * p2[1] - k2[1]) // s2[1] + 1
    return N, C, H, W, k2, s2, p2, bool(bias), Cout, Ho, Wo


@functools.lru_cache(maxsize=None)
def _conv_inputs(case):
    """(x, g, A_ref, G_ref) of a case: the fp64 oracle runs once per case, whatever the offsets and build paths."""
    o = _oracle()
    N, C, H, W, k2, s2, p2, bias, Cout, Ho, Wo = _unpack(case)
    torch.manual_seed(1234)
    x = torch.relu(torch.randn(N, C, H, W))
    g = torch.randn(N, Cout, Ho, Wo) / N
    A_ref, G_ref = o.kfac_factors(x.double(), g.double(), k2, s2, p2, bias)
    return x, g, A_ref, G_ref


def _conv_jobs(case, xg, gg, gpu):
    from curvature_amd import ops
    N, C, H, W, k2, s2, p2, bias, Cout, Ho, Wo = _unpack(case)
    n = C * k2[0] * k2[1] + int(bias)
    A = torch.full((n, n), float("nan"), device=gpu)
    G = torch.full((Cout, Cout), float("nan"), device=gpu)
    L = Ho * Wo
    return [ops.FactorJob(xg, A, k2, s2, p2, bias, 1.0 / (N * L), True),
            ops.FactorJob(gg, G, (1, 1), (1, 1), (0, 0), False, N / L, True)]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_factors(gpu, case):
    """Sources fenced by NaN (nothing outside them may reach a factor), at a 16-byte-aligned start and 4 bytes past one."""
    from curvature_amd import ops
    x, g, A_ref, G_ref = _conv_inputs(case)
    for offset in OFFSETS:
        jobs = _conv_jobs(case, fenced_copy(x, offset), fenced_copy(g, offset), gpu)
        A, G = jobs[0].dst, jobs[1].dst
        ops.kfac_accumulate(jobs)
        torch.cuda.synchronize()
        assert torch.isfinite(A).all() and torch.isfinite(G).all(), offset
        assert rel_fro(A, A_ref) < TOL, (offset, rel_fro(A, A_ref))
        assert rel_fro(G, G_ref) < TOL, (offset, rel_fro(G, G_ref))
        assert torch.equal(A, A.t()) and torch.equal(G, G.t())       # exactly symmetric
        # accumulate a second batch (the reference's `+=`, curvatures.py:347-348)
        for j in jobs:
            j.first = False
        ops.kfac_accumulate(jobs)
        torch.cuda.synchronize()
        assert rel_fro(A, 2 * A_ref) < TOL, offset
        assert rel_fro(G, 2 * G_ref) < TOL, offset


@functools.lru_cache(maxsize=None)
def _exact_conv_inputs(case):
    """(x, g, A_exact, G_exact, scale_A, scale_G) of a case with integer-valued sources (tests/exact_inputs.py): the
    unscaled integer Grams of ``F.unfold`` in float64, formed on the GPU once per case, and two power-of-two scales."""
    N, C, H, W, k2, s2, p2, bias, Cout, Ho, Wo = _unpack(case)
    assert_exact_range(3, N * Ho * Wo, rounds=2)
    gen = torch.Generator().manual_seed(4321)
    x, g = nonzero_ints((N, C, H, W), gen), nonzero_ints((N, Cout, Ho, Wo), gen)
    A_exact = exact_gram(conv_rows(x.to("cuda:0"), k2, s2, p2), ones_row=bias)
    G_exact = exact_gram(flat_rows(g.to("cuda:0")))
    scale = pow2_scale(N * Ho * Wo)
    return x, g, A_exact, G_exact, scale, 4.0 * scale


def _assert_exact(dst, want, what):
    """`dst` holds exactly `want` (float64, every entry a float32 value) and is exactly symmetric."""
    got = dst.double()
    assert torch.equal(got, want), (what, int((got != want).sum()), float((got - want).abs().max()))
    assert torch.equal(dst, dst.t()), what


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_factors_exact_on_integer_inputs(gpu, case):
    """Every case of `test_conv_factors` again, bit for bit: sources uniform in {+-1, +-2, +-3} (none zero, so every
    element moves the result) and a power-of-two scale.  Every product and partial sum is an integer below 2^24, so the
    fp32 MFMA, the k-slice reduce and the shifted-correlation assembly have one right answer in any summation order:
    ``scale * exact`` after a first call, twice that after an accumulating one.  No tolerance: an element of a ragged
    group, a last k-slice or the last pixel of the last sample that is left out or counted twice fails here, where the
    1e-4 Frobenius bar above lets it through."""
    from curvature_amd import ops
    x, g, A_exact, G_exact, scale_a, scale_g = _exact_conv_inputs(case)
    for offset in OFFSETS:
        jobs = _conv_jobs(case, fenced_copy(x, offset), fenced_copy(g, offset), gpu)     # destinations start as NaN
        A, G = jobs[0].dst, jobs[1].dst
        jobs[0].scale, jobs[1].scale = scale_a, scale_g
        ops.kfac_accumulate(jobs)
        torch.cuda.synchronize()
        _assert_exact(A, scale_a * A_exact, ("A", offset))
        _assert_exact(G, scale_g * G_exact, ("G", offset))
        for j in jobs:
            j.first = False
        ops.kfac_accumulate(jobs)
        torch.cuda.synchronize()
        _assert_exact(A, 2 * scale_a * A_exact, ("A accumulated", offset))
        _assert_exact(G, 2 * scale_g * G_exact, ("G accumulated", offset))


def test_one_dropped_pixel_fails_the_exact_comparison(gpu):
    """The comparison above has teeth where the Frobenius bar has none: at ResNet-50 layer1 geometry, a source whose last
    pixel of the last sample is zeroed (what a kernel that drops that pixel computes) moves the float64 factor by less
    than 1e-4 relative Frobenius under relu(randn) inputs, and here changes exactly the entries the
    integer reference says it changes - about half of the factor."""
    from curvature_amd import ops
    case = (8, 64, 56, 56, 3, 1, 1, False)
    x, g, A_exact, _, scale, _ = _exact_conv_inputs(case)
    dropped = x.clone()
    dropped[-1, :, -1, -1] = 0
    A_dropped = exact_gram(conv_rows(dropped.to(gpu), (3, 3), (1, 1), (1, 1)))
    jobs = _conv_jobs(case, fenced_copy(dropped, 0), fenced_copy(g, 0), gpu)[:1]
    jobs[0].scale = scale
    ops.kfac_accumulate(jobs)
    torch.cuda.synchronize()
    got = jobs[0].dst.double()
    assert torch.equal(got, scale * A_dropped)
    changed = int((got != scale * A_exact).sum())
    print(f"one pixel of 25 088 dropped: {changed} of {got.numel()} entries differ from the exact factor")
    assert changed == int((A_dropped != A_exact).sum()) and changed > 100000


LINEAR_CASES = [(100, 400, 120, True), (7, 84, 10, True), (32, 513, 1000, False), (1, 5, 3, True)]


@pytest.mark.parametrize("N,C,Cout,bias", LINEAR_CASES)
def test_linear_factors_exact_on_integer_inputs(gpu, N, C, Cout, bias):
    """The Linear cases of `test_linear_factors` bit for bit, as `test_conv_factors_exact_on_integer_inputs`."""
    from curvature_amd import ops
    assert_exact_range(3, N, rounds=2)
    gen = torch.Generator().manual_seed(77)
    x, g = nonzero_ints((N, C), gen), nonzero_ints((N, Cout), gen)
    A_exact = exact_gram(flat_rows(x.to(gpu)), ones_row=bias)
    G_exact = exact_gram(flat_rows(g.to(gpu)))
    scale_a = pow2_scale(N)
    scale_g = 1.0 / scale_a
    for offset in OFFSETS:
        A = torch.full((C + bias, C + bias), float("nan"), device=gpu)
        G = torch.full((Cout, Cout), float("nan"), device=gpu)
        jobs = [ops.FactorJob(fenced_copy(x, offset), A, has_bias=bias, scale=scale_a, first=True),
                ops.FactorJob(fenced_copy(g, offset), G, scale=scale_g, first=True)]
        ops.kfac_accumulate(jobs)
        torch.cuda.synchronize()
        _assert_exact(A, scale_a * A_exact, ("A", offset))
        _assert_exact(G, scale_g * G_exact, ("G", offset))
        for j in jobs:
            j.first = False
        ops.kfac_accumulate(jobs)
        torch.cuda.synchronize()
        _assert_exact(A, 2 * scale_a * A_exact, ("A accumulated", offset))
        _assert_exact(G, 2 * scale_g * G_exact, ("G accumulated", offset))


@pytest.mark.parametrize("shape", [(1, 70), (1, 513), (1, 70, 1, 1)], ids=["linear70", "linear513", "conv70"])
def test_fp32_operands_are_not_narrowed(gpu, shape):
    """Small integers are exact in bf16 too, so a build that narrowed its fp32 operands would pass the tests above.  Here
    N = 1 and every entry of the factor is ONE product of two odd 12-bit integers: 24 bits, exact in float32, and another
    number once an operand was rounded to bf16, fp16 or tf32 (tests/test_exact_inputs_cpu.py shows that).  A == x x^T."""
    from curvature_amd import ops
    assert_exact_range(4095, 1, rounds=1)
    gen = torch.Generator().manual_seed(12)
    x = wide_ints(shape, gen, 12)
    want = exact_gram(flat_rows(x.to(gpu)))
    n = shape[1]
    for offset in OFFSETS:
        A = torch.full((n, n), float("nan"), device=gpu)
        ops.kfac_accumulate([ops.FactorJob(fenced_copy(x, offset), A, scale=1.0, first=True)])
        torch.cuda.synchronize()
        _assert_exact(A, want, offset)


def test_kfac_update_exact_on_integer_records(gpu):
    """`KFAC.update` end to end on a Conv2d 3x3 / pad 1 over 8 x 8 images and a Linear, N = 4, records set to
    integer-valued tensors: 1 / (N L) = 2^-8, N / L = 2^-4, 1 / N and N are the scales update() itself passes (the tests
    above set their own), all powers of two, so `state` is the exact factor bit for bit after one update and twice it
    after two."""
    from curvature_amd.curvatures import KFAC
    N, L = 4, 64
    conv = torch.nn.Conv2d(3, 5, 3, padding=1)
    linear = torch.nn.Linear(5 * L, 6)
    model = torch.nn.Sequential(conv, torch.nn.Flatten(), linear).to(gpu)
    assert_exact_range(3, N * L, rounds=2)
    gen = torch.Generator().manual_seed(31)
    records = {conv: (nonzero_ints((N, 3, 8, 8), gen), nonzero_ints((N, 5, 8, 8), gen)),
               linear: (nonzero_ints((N, 5 * L), gen), nonzero_ints((N, 6), gen))}
    xc, gc = (t.to(gpu) for t in records[conv])
    xl, gl = (t.to(gpu) for t in records[linear])
    want = {conv: (exact_gram(conv_rows(xc, 3, 1, 1), ones_row=True) / (N * L), exact_gram(flat_rows(gc)) * N / L),
            linear: (exact_gram(flat_rows(xl), ones_row=True) / N, exact_gram(flat_rows(gl)) * N)}
    for offset in OFFSETS:
        kfac = KFAC(model)
        try:
            for layer, (x, g) in records.items():
                kfac.record[layer] = [fenced_copy(x, offset), fenced_copy(g, offset)]
            for rounds in (1, 2):
                kfac.update(batch_size=N)
                torch.cuda.synchronize()
                for layer in (conv, linear):
                    for side in (0, 1):
                        _assert_exact(kfac.state[layer][side], rounds * want[layer][side], (offset, rounds, side))
        finally:
            for hook in kfac.hooks:
                hook.remove()


@pytest.mark.parametrize("N,C,Cout,bias", LINEAR_CASES)
def test_linear_factors(gpu, N, C, Cout, bias):
    from curvature_amd import ops
    o = _oracle()
    torch.manual_seed(7)
    x = torch.randn(N, C)
    g = torch.randn(N, Cout) / N
    A_ref, G_ref = o.kfac_factors(x.double(), g.double(), has_bias=bias)
    for offset in OFFSETS:
        A = torch.empty(C + bias, C + bias, device=gpu)
        G = torch.empty(Cout, Cout, device=gpu)
        ops.kfac_accumulate([ops.FactorJob(fenced_copy(x, offset), A, has_bias=bias, scale=1.0 / N, first=True),
                             ops.FactorJob(fenced_copy(g, offset), G, scale=float(N), first=True)])
        torch.cuda.synchronize()
        assert torch.isfinite(A).all() and torch.isfinite(G).all(), offset
        assert rel_fro(A, A_ref) < TOL, (offset, rel_fro(A, A_ref))
        assert rel_fro(G, G_ref) < TOL, (offset, rel_fro(G, G_ref))


def _plan_rows(jobs):
    """curv_kfac_plan_info of a job list: one dict per job (fields named as in test_plan_host.py)."""
    import ctypes
    from curvature_amd import _lib, ops
    names = ("dim Ho Wo NS R Wc nchunks RS PS SS nch ntiles cpi nslices nitems base TM vec4 cshift nsub direct rshift "
             "pre dma flops").split()
    assert len(names) == ops.PLAN_INFO_FIELDS
    arr = ops._factor_descs(jobs)
    out = (ctypes.c_longlong * (ops.PLAN_INFO_FIELDS * len(jobs)))()
    _lib.check(_lib.lib().curv_kfac_plan_info(arr, len(jobs), out), "curv_kfac_plan_info")
    return [dict(zip(names, out[ops.PLAN_INFO_FIELDS * i:ops.PLAN_INFO_FIELDS * (i + 1)])) for i in range(len(jobs))]


def test_fenced_cases_reach_every_kernel(gpu, build_path):
    """The fenced cases above cover every kernel form of the fp32 factor build, as the planner routes them today (plan
    fields 17 float4 staging, 22 pre-tiled LDS-DMA, 23 flat LDS-DMA / shifted correlations; the launch form from
    kfac_path_for).  A planner change that moves a case off its kernel fails here instead of silently ending the
    coverage of that kernel."""
    from curvature_amd import _lib, ops
    seen = set()
    for case in CONV_CASES:
        N, C, H, W, k2, s2, p2, bias, Cout, Ho, Wo = _unpack(case)
        geoms = [(N, C, H, W, k2, s2, p2, bias), (N, Cout, Ho, Wo, (1, 1), (1, 1), (0, 0), False)]
        if ops.kfac_path_for(geoms) == _lib.PATH_SMALL:
            seen.add("small")
        for offset in OFFSETS:
            xg, gg = fenced((N, C, H, W), offset), fenced((N, Cout, Ho, Wo), offset)
            for (geo_n, geo_c, geo_hw, geo_k, geo_s), p in zip(
                    [(N, C, H * W, k2, s2), (N, Cout, Ho * Wo, (1, 1), (1, 1))], _plan_rows(_conv_jobs(case, xg, gg, gpu))):
                one_by_one = geo_k == (1, 1)
                if p["dma"] == 2:
                    seen.add("corr C=64" if C == 64 else "corr C%128" if C % 128 == 0 else "corr other")
                elif p["dma"] == 1 and not one_by_one:
                    seen.add("kxk unfolded")
                elif p["dma"] == 1 and geo_s != (1, 1):
                    seen.add("strided 1x1 unfolded")
                elif p["dma"] == 1:
                    seen.add("flat W%4==0" if geo_hw % 4 == 0 else "flat W%4!=0")
                    if p["dim"] % 128:
                        seen.add("flat ragged dim")
                elif p["pre"]:
                    seen.add("pre-tiled")
                elif p["dma"] == 0:
                    seen.add("im2col float4" if p["vec4"] else "im2col")
    want = {"im2col float4", "im2col", "pre-tiled", "flat W%4==0", "flat W%4!=0", "flat ragged dim", "corr C%128",
            "corr C=64", "strided 1x1 unfolded"}
    if build_path == "small":
        want.add("small")
    assert want <= seen, sorted(want - seen)


def test_resnet50_layer4_one_by_one_fenced(gpu, build_path):
    """KFAC.update() at ResNet-50 layer4.x.conv1 / conv3 (1x1, 2048 -> 512 and 512 -> 2048, 7 x 7, N = 8): every factor
    of this geometry - A of both, G of both - is flattened with 49 pixels per row, so the last 4-pixel group of each row
    straddles its end; the records end right before NaN.  Against an fp64 reference computed with plain torch."""
    from curvature_amd.curvatures import KFAC
    N, L = 8, 49
    conv1 = torch.nn.Conv2d(2048, 512, 1, bias=False)
    conv3 = torch.nn.Conv2d(512, 2048, 1, bias=False)
    model = torch.nn.Sequential(conv1, conv3).to(gpu)
    torch.manual_seed(21)
    data = {layer: (torch.relu(torch.randn(N, layer.in_channels, 7, 7)), torch.randn(N, layer.out_channels, 7, 7) / N)
            for layer in (conv1, conv3)}
    refs = {}
    for layer, (x, g) in data.items():
        X = x.to(gpu, torch.float64).reshape(N, -1, L)
        Gs = g.to(gpu, torch.float64).reshape(N, -1, L)
        refs[layer] = (torch.einsum("ncl,ndl->cd", X, X) / (N * L), torch.einsum("ncl,ndl->cd", Gs, Gs) * N / L)
    for offset in OFFSETS:
        kfac = KFAC(model)
        for layer, (x, g) in data.items():
            kfac.record[layer] = [fenced_copy(x, offset), fenced_copy(g, offset)]
        kfac.update(batch_size=N)
        torch.cuda.synchronize()
        for layer in (conv1, conv3):
            A, G = kfac.state[layer]
            RA, RG = refs[layer]
            assert torch.isfinite(A).all() and torch.isfinite(G).all(), (offset, tuple(A.shape))
            assert rel_fro(A, RA) < TOL and rel_fro(G, RG) < TOL, (offset, rel_fro(A, RA), rel_fro(G, RG))
            assert torch.equal(A, A.t()) and torch.equal(G, G.t())


def test_many_k_slices(gpu):
    """Large K (split over many k-slices and summed by the reduce kernel) and determinism."""
    from curvature_amd import ops
    o = _oracle()
    torch.manual_seed(3)
    x = torch.relu(torch.randn(8, 64, 56, 56))
    A_ref, _ = o.kfac_factors(x.double(), torch.zeros(8, 1, 56, 56).double(), (1, 1), (1, 1), (0, 0), False)
    xg = x.to(gpu)
    outs = []
    for _ in range(2):
        A = torch.empty(64, 64, device=gpu)
        ops.kfac_accumulate([ops.FactorJob(xg, A, scale=1.0 / (8 * 56 * 56), first=True)])
        torch.cuda.synchronize()
        outs.append(A)
    assert rel_fro(outs[0], A_ref) < TOL
    assert torch.equal(outs[0], outs[1])          # fixed-order slab reduction: bitwise reproducible


def test_mixed_launch_with_several_assembled_factors(gpu):
    """One grouped call holding three 3x3 / stride 1 factors of different widths (assembled from shifted correlations:
    their 3 x 29 virtual factors share the LDS-DMA work list), their G sides, a stride-2 3x3, a 1x1 and a Linear pair:
    every factor against the oracle, accumulation on the second call, bit-reproducible."""
    from curvature_amd import ops
    o = _oracle()
    torch.manual_seed(99)
    specs = [(8, 128, 14, 14, 3, 1, 1), (8, 256, 7, 7, 3, 1, 1), (8, 512, 7, 9, 3, 1, 1), (8, 128, 14, 14, 3, 2, 1),
             (8, 256, 7, 7, 1, 1, 0)]
    jobs, refs = [], []
    for N, C, H, W, k, s, p in specs:
        x = torch.relu(torch.randn(N, C, H, W))
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        g = torch.randn(N, 96, Ho, Wo) / N
        A_ref, G_ref = o.kfac_factors(x.double(), g.double(), (k, k), (s, s), (p, p), False)
        n = C * k * k
        A = torch.full((n, n), float("nan"), device=gpu)
        G = torch.full((96, 96), float("nan"), device=gpu)
        L = Ho * Wo
        jobs += [ops.FactorJob(x.to(gpu), A, (k, k), (s, s), (p, p), False, 1.0 / (N * L), True),
                 ops.FactorJob(g.to(gpu), G, (1, 1), (1, 1), (0, 0), False, N / L, True)]
        refs += [A_ref, G_ref]
    x = torch.randn(8, 300)
    g = torch.randn(8, 40) / 8
    A_ref, G_ref = o.kfac_factors(x.double(), g.double(), has_bias=True)
    jobs += [ops.FactorJob(x.to(gpu), torch.empty(301, 301, device=gpu), has_bias=True, scale=1.0 / 8, first=True),
             ops.FactorJob(g.to(gpu), torch.empty(40, 40, device=gpu), scale=8.0, first=True)]
    refs += [A_ref, G_ref]
    flops = ops.kfac_plan_flops(jobs)
    assert flops[0] < 0.4 * (1152 * 1153) * 8 * 196 and flops[6] == (1152 * 1153) * 8 * 49      # assembled vs direct (stride 2)
    ops.kfac_accumulate(jobs)
    first = [j.dst.clone() for j in jobs]
    for j, ref in zip(jobs, refs):
        assert rel_fro(j.dst, ref) < TOL, (tuple(j.dst.shape), rel_fro(j.dst, ref))
        assert torch.equal(j.dst, j.dst.t())
    for j in jobs:
        j.first = False
    ops.kfac_accumulate(jobs)
    for j, ref in zip(jobs, refs):
        assert rel_fro(j.dst, 2 * ref) < TOL
    for j, f in zip(jobs, first):                      # same inputs, fresh outputs: bit-identical to the first call
        j.first = True
    ops.kfac_accumulate(jobs)
    for j, f in zip(jobs, first):
        assert torch.equal(j.dst, f)


def test_more_pretiled_factors_than_one_argument_block(gpu):
    """The pre-tiling pass carries 32 factor descriptors per kernel-argument block: 37 convolution factors in one call
    take two launches of it."""
    from curvature_amd import ops
    o = _oracle()
    torch.manual_seed(6)
    jobs, refs = [], []
    for i in range(37):
        C, H, W, s = 3 + i % 5, 6 + i % 4, 7 + i % 3, 1 + i % 2
        x = torch.relu(torch.randn(3, C, H, W))
        Ho, Wo = (H + 2 - 3) // s + 1, (W + 2 - 3) // s + 1
        A_ref, _ = o.kfac_factors(x.double(), torch.zeros(3, 1, Ho, Wo, dtype=torch.float64), (3, 3), (s, s), (1, 1), False)
        jobs.append(ops.FactorJob(x.to(gpu), torch.empty(9 * C, 9 * C, device=gpu), (3, 3), (s, s), (1, 1), False,
                                  1.0 / (3 * Ho * Wo), True))
        refs.append(A_ref)
    ops.kfac_accumulate(jobs)
    for j, ref in zip(jobs, refs):
        assert rel_fro(j.dst, ref) < TOL and torch.equal(j.dst, j.dst.t())


def test_more_assembled_factors_than_one_argument_block(gpu):
    """The padding / assembly passes carry 14 layer descriptors per kernel-argument block: 19 assembled factors in one
    call take two launches of each (a ResNet-34 has 16 such layers, a ResNet-50 13)."""
    from curvature_amd import ops
    o = _oracle()
    torch.manual_seed(5)
    jobs, refs = [], []
    for i in range(19):
        H, W = 4 + i % 3, 5 + i % 2
        x = torch.relu(torch.randn(8, 128, H, W))
        A_ref, _ = o.kfac_factors(x.double(), torch.zeros(8, 1, H, W, dtype=torch.float64), (3, 3), (1, 1), (1, 1), False)
        jobs.append(ops.FactorJob(x.to(gpu), torch.empty(1152, 1152, device=gpu), (3, 3), (1, 1), (1, 1), False,
                                  1.0 / (8 * H * W), True))
        refs.append(A_ref)
    ops.kfac_accumulate(jobs)
    for j, ref in zip(jobs, refs):
        assert rel_fro(j.dst, ref) < TOL and torch.equal(j.dst, j.dst.t())


def _linear_jobs(ops, gpu, count, seed):
    torch.manual_seed(seed)
    jobs = []
    for i in range(count):
        C = 24 + 8 * (i % 7)
        x = torch.randn(6, C, device=gpu)
        jobs.append(ops.FactorJob(x, torch.empty(C + 1, C + 1, device=gpu), has_bias=True, scale=1.0 / 6, first=True))
    return jobs


def test_resident_table_survives_a_shorter_table_in_between(gpu):
    """Round-3 advisor: the library's host shadow of the resident descriptor table only ever grew, so a call with a
    SHORTER table (whose zero pad / slabs overwrite the tail rows of the longer one on the device) left stale shadow
    rows behind and the next long call skipped their upload.  40 factors (rows in argument blocks of 13), a 6-factor call
    on the same workspace in between, then the 40 again: bit-identical to the first result."""
    from curvature_amd import ops
    jobs = _linear_jobs(ops, gpu, 40, 11)
    ops.kfac_accumulate(jobs)
    torch.cuda.synchronize()
    want = [j.dst.clone() for j in jobs]
    ops.kfac_accumulate(jobs)                    # same buffer again: resident, every block matches
    for _ in range(3):                           # steady-state alternation, as compute_factors(share_inputs=True) does
        ops.kfac_accumulate(jobs[:6])
        for j in jobs:
            j.dst.fill_(float("nan"))
        ops.kfac_accumulate(jobs)
        torch.cuda.synchronize()
        for j, w in zip(jobs, want):
            assert torch.equal(j.dst, w)


def test_two_estimators_of_different_size_share_a_workspace(gpu):
    """The same hazard with two callers: a 35-factor and a 17-factor job list alternate on one stream (one "kfac"
    workspace); each keeps producing its own first result."""
    from curvature_amd import ops
    big, small = _linear_jobs(ops, gpu, 35, 12), _linear_jobs(ops, gpu, 17, 13)
    ops.kfac_accumulate(big)
    ops.kfac_accumulate(small)
    torch.cuda.synchronize()
    want_big, want_small = [j.dst.clone() for j in big], [j.dst.clone() for j in small]
    for _ in range(3):
        for jobs, want in ((big, want_big), (small, want_small)):
            for j in jobs:
                j.dst.fill_(float("nan"))
            ops.kfac_accumulate(jobs)
            torch.cuda.synchronize()
            for j, w in zip(jobs, want):
                assert torch.equal(j.dst, w)


def test_small_build_does_not_depend_on_the_rest_of_the_launch(gpu, build_path):
    """The two-launch small-model build slices every factor by a rule of its own: a factor built alone and the same factor
    built beside others (what a layer-sharded rank and the unsharded run do) come out bit for bit the same, also with
    more factors than one argument block carries (24)."""
    if build_path != "small":
        pytest.skip("property of the small-model build")
    from curvature_amd import ops
    torch.manual_seed(3)
    x1 = torch.randn(100, 1, 28, 28, device=gpu)               # LeNet conv1 at its real batch size: 64 slices
    x2 = torch.randn(100, 6, 14, 14, device=gpu)               # conv2: 15 blocks x 32 slices
    lin = [torch.randn(100, 7 + 13 * k, device=gpu) for k in range(26)]

    def job(x, k, p, bias, n):
        return ops.FactorJob(x, torch.empty(n, n, device=gpu), (k, k), (1, 1), (p, p), bias, 1.0 / x.shape[0], True)
    alone1, alone2 = job(x1, 5, 2, True, 26), job(x2, 5, 0, True, 151)
    ops.kfac_accumulate([alone1])
    ops.kfac_accumulate([alone2])
    together = [ops.FactorJob(t, torch.empty(t.shape[1], t.shape[1], device=gpu), scale=0.01, first=True) for t in lin[:13]]
    t1, t2 = job(x1, 5, 2, True, 26), job(x2, 5, 0, True, 151)
    together += [t1] + [ops.FactorJob(t, torch.empty(t.shape[1], t.shape[1], device=gpu), scale=0.01, first=True) for t in lin[13:]] + [t2]
    assert len(together) > 24
    ops.kfac_accumulate(together)
    assert torch.equal(alone1.dst, t1.dst) and torch.equal(alone2.dst, t2.dst)
    ref = torch.nn.functional.unfold(x1.double(), 5, padding=2)
    ref = torch.cat([ref, torch.ones(100, 1, ref.shape[2], device=gpu, dtype=torch.float64)], 1)
    want = sum(r @ r.t() for r in ref) / 100
    assert rel_fro(t1.dst.cpu().double(), want.cpu()) < TOL
    for j, t in zip(together[:3], lin[:3]):
        assert rel_fro(j.dst.cpu().double(), (0.01 * t.double().t() @ t.double()).cpu()) < TOL
