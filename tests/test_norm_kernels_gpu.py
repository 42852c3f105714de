"""The fused normalisation-layer passes of csrc/norm_factor.hip through `ops`, against float64 computed on
the CPU from the very records: the stacked A and G factors, the per-sample products p (as p**2 from
`per_sample_norm_sq_accumulate` on one sample at a time - the reductions expose squares only - and through
`per_sample_norm_quad_reduce` on the batch), `first=False`, channels_last records read in place, NaN fences, a call that
crosses the launch batch, an offset input, and invalid descriptors.  Bars: rel_fro < 1e-4 (conftest.rel_fro)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import rel_fro
from curvature_amd import _lib, ops

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(autouse=True)
def admitted():
    was = ops.admit_norm_layers(True)
    yield
    ops.admit_norm_layers(was)


def _bn(C, dev):
    bn = nn.BatchNorm2d(C).to(dev).eval()
    gen = torch.Generator().manual_seed(C)
    bn.running_mean.copy_(torch.randn(C, generator=gen))
    bn.running_var.copy_(torch.rand(C, generator=gen) + 0.3)
    return bn


# name -> (layer factory, record shape).  The smallest shapes at which each path can go wrong; `split`: one plane just past
# _lib.NORM_SPLIT_L positions (33 x 32 = 1056 >= 1024: the four waves of a workgroup share a plane, and a group of two).
CASES = {
    "gn": (lambda d: nn.GroupNorm(3, 6).to(d), (3, 6, 5, 7)),
    "gn_g1": (lambda d: nn.GroupNorm(1, 6).to(d), (3, 6, 5, 7)),
    "gn_wave": (lambda d: nn.GroupNorm(70, 70).to(d), (2, 70, 3, 4)),
    "gn_split": (lambda d: nn.GroupNorm(1, 2).to(d), (2, 2, 33, 32)),
    "bn": (lambda d: _bn(5, d), (2, 5, 3, 3)),
    "ln": (lambda d: nn.LayerNorm(70).to(d), (3, 5, 70)),
    "ln_wide": (lambda d: nn.LayerNorm(513).to(d), (4, 513)),
    "ln_2d": (lambda d: nn.LayerNorm((4, 6)).to(d), (2, 3, 4, 6)),
    "ln_nobias": (lambda d: nn.LayerNorm(70, bias=False).to(d), (3, 5, 70)),
}
assert 33 * 32 >= _lib.NORM_SPLIT_L > 31 * 33            # (and every other plane of the table lies below it)


def _records(name, dev, offset=0.0):
    torch.manual_seed(sorted(CASES).index(name))
    make, shape = CASES[name]
    return make(dev), (offset + torch.randn(shape)).to(dev), torch.randn(shape).to(dev)


def _ncl(layer, t):
    """A record as float64 (N, C, L) on the CPU."""
    t = t.detach().double().cpu()
    if isinstance(layer, nn.LayerNorm):
        D = layer.weight.numel()
        return t.reshape(t.shape[0], -1, D).transpose(1, 2)
    return t.reshape(t.shape[0], t.shape[1], -1)


def _xh64(layer, x):
    """The standardised input in float64, (N, C, L)."""
    x = x.detach().double().cpu()
    if isinstance(layer, nn.LayerNorm):
        dims = tuple(range(x.dim() - len(layer.normalized_shape), x.dim()))
        xh = (x - x.mean(dims, keepdim=True)) / torch.sqrt(x.var(dims, unbiased=False, keepdim=True) + layer.eps)
    elif isinstance(layer, nn.GroupNorm):
        v = x.reshape(x.shape[0], layer.num_groups, -1)
        xh = ((v - v.mean(2, keepdim=True)) / torch.sqrt(v.var(2, unbiased=False, keepdim=True) + layer.eps)).reshape(x.shape)
    else:
        shape = (1, -1) + (1,) * (x.dim() - 2)
        xh = (x - layer.running_mean.double().cpu().view(shape)) / \
            torch.sqrt(layer.running_var.double().cpu().view(shape) + layer.eps)
    return _ncl(layer, xh)


def _p64(layer, x, g):
    """p (N, C, n_g) in float64."""
    xh, g = _xh64(layer, x), _ncl(layer, g)
    cols = [(g * xh).sum(2)] + ([g.sum(2)] if layer.bias is not None else [])
    return torch.stack(cols, 2)


def _factors64(layer, x, g, a_scale, g_scale):
    xh, g = _xh64(layer, x), _ncl(layer, g)
    C = xh.shape[1]
    rows = [xh] + ([torch.ones_like(xh)] if layer.bias is not None else [])
    A = torch.stack([torch.stack([(r * q).sum((0, 2)) for q in rows], 1) for r in rows], 1)
    return a_scale * A, g_scale * g.square().sum((0, 2)).view(C, 1, 1)


def _build_factors(layer, x, g, a_scale, g_scale, A, G, first):
    sides = ops.factor_jobs(layer, x, g)
    sides.a.dst, sides.a.scale, sides.a.first = A, a_scale, first
    sides.g.dst, sides.g.scale, sides.g.first = G, g_scale, first
    ops.accumulate_factors([sides.a, sides.g])
    return sides


def _p_squared(layer, x, g, first_value=None):
    """p**2 (N, C, n_g) from one sq call per sample (N = 1: the sum over samples has one term); with `first_value` the
    destination holds it and the call adds."""
    n_g = 1 + int(layer.bias is not None)
    out = torch.full((x.shape[0], layer.weight.numel(), n_g), float("nan") if first_value is None else first_value,
                     device=x.device)
    ops.per_sample_norm_sq_accumulate([ops.PerSampleNormJob.of(layer, x[n:n + 1], g[n:n + 1], dst=out[n],
                                                              first=first_value is None) for n in range(x.shape[0])])
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_factors_and_products_against_float64(gpu, name):
    layer, x, g = _records(name, gpu)
    C, n_g = layer.weight.numel(), 1 + int(layer.bias is not None)
    A = torch.full((C, n_g, n_g), float("nan"), device=gpu)
    G = torch.full((C, 1, 1), float("nan"), device=gpu)
    sides = _build_factors(layer, x, g, 0.25, 3.0, A, G, True)
    N, L = x.shape[0], x.numel() // x.shape[0] // C
    assert (sides.n, sides.m, sides.N, sides.L, sides.groups) == (n_g, 1, N, L, C)
    A64, G64 = _factors64(layer, x, g, 0.25, 3.0)
    assert rel_fro(A, A64) < TOL and rel_fro(G, G64) < TOL
    assert torch.equal(A, A.transpose(1, 2))
    _build_factors(layer, x, g, 0.5, 1.0, A, G, False)                      # first=False adds
    assert rel_fro(A, 3 * A64) < TOL and rel_fro(G, G64 * (4.0 / 3.0)) < TOL

    p64 = _p64(layer, x, g)
    assert rel_fro(_p_squared(layer, x, g), p64.square()) < TOL
    assert rel_fro(_p_squared(layer, x, g, first_value=2.0), p64.square() + 2.0) < TOL
    # the batch at once: sq sums the samples, quad with T = I, weights and channel scales
    dst = torch.full((C, n_g), float("nan"), device=gpu)
    ops.per_sample_norm_sq_accumulate([ops.PerSampleNormJob.of(layer, x, g, dst=dst, alpha=0.5, first=True)])
    assert rel_fro(dst, 0.5 * p64.square().sum(0)) < TOL
    T = torch.eye(n_g, device=gpu).repeat(C, 1, 1)
    Wt, s = torch.rand(C, n_g, device=gpu) + 0.5, torch.rand(C, device=gpu) + 0.5
    out = torch.full((N,), float("nan"), device=gpu)
    want = 2.0 * (s.double().cpu().square()[None, :, None] * Wt.double().cpu()[None] * p64.square()).sum((1, 2))
    for first, scale in ((True, 1.0), (False, 2.0)):
        ops.per_sample_norm_quad_reduce([ops.PerSampleNormJob.of(layer, x, g, out=out, T=T, W=Wt, s=s, alpha=2.0,
                                                                 first=first)])
        assert rel_fro(out, scale * want) < TOL
    flops, nbytes = ops.per_sample_norm_plan_info([ops.PerSampleNormJob.of(layer, x, g)])
    assert flops[0] > 0 and nbytes[0] == 4 * x.numel() * (2 if name == "bn" else 3)


@pytest.mark.parametrize("name", ["gn", "gn_g1", "bn"])
def test_channels_last_records_are_read_in_place(gpu, name):
    layer, x, g = _records(name, gpu)
    xl, gl = x.contiguous(memory_format=torch.channels_last), g.contiguous(memory_format=torch.channels_last)
    job = ops.PerSampleNormJob.of(layer, xl, gl)
    assert job.x.data_ptr() == xl.data_ptr() and job.g.data_ptr() == gl.data_ptr()
    assert job.view.x_strides == tuple(xl.stride()) and job.view.x_strides[1] == 1
    arr = ops._per_sample_norm_descs([ops.PerSampleNormJob.of(layer, xl, gl, dst=torch.empty(x.shape[1], 2, device=gpu))],
                                     "test", "sq")
    assert arr[0].x == xl.data_ptr() and arr[0].g == gl.data_ptr() and arr[0].x_sc == 1
    assert rel_fro(_p_squared(layer, xl, gl), _p64(layer, x, g).square()) < TOL
    C, n_g = x.shape[1], 2
    A, G = torch.empty(C, n_g, n_g, device=gpu), torch.empty(C, 1, 1, device=gpu)
    sides = _build_factors(layer, xl, gl, 1.0, 1.0, A, G, True)
    assert sides.a.src.data_ptr() == xl.data_ptr() and sides.g.src.data_ptr() == gl.data_ptr()
    A64, G64 = _factors64(layer, x, g, 1.0, 1.0)
    assert rel_fro(A, A64) < TOL and rel_fro(G, G64) < TOL


@pytest.mark.parametrize("name", ["gn", "gn_split", "bn", "ln", "ln_wide"])
def test_nan_fenced_records(gpu, name):
    """The records inside NaN-filled buffers, NaN directly before and after them: finite, and the bits of the unfenced run
    (the fence shifts the records by 16 bytes + 4: an unaligned record takes the same sums through narrower loads)."""
    layer, x, g = _records(name, gpu)
    plain = _p_squared(layer, x, g)

    def fenced(t):
        buf = torch.full((t.numel() + 10,), float("nan"), device=gpu)
        view = buf[5:5 + t.numel()].view(t.shape)
        view.copy_(t)
        return view
    xf, gf = fenced(x), fenced(g)
    got = _p_squared(layer, xf, gf)
    assert torch.isfinite(got).all() and torch.equal(got, plain)
    C, n_g = layer.weight.numel(), 1 + int(layer.bias is not None)
    pair = []
    for xs, gs in ((x, g), (xf, gf)):
        A, G = torch.empty(C, n_g, n_g, device=gpu), torch.empty(C, 1, 1, device=gpu)
        _build_factors(layer, xs, gs, 1.0, 1.0, A, G, True)
        pair.append((A, G))
    assert torch.isfinite(pair[1][0]).all() and torch.isfinite(pair[1][1]).all()
    assert torch.equal(pair[0][0], pair[1][0]) and torch.equal(pair[0][1], pair[1][1])


def test_seventeen_items_cross_the_launch_batch(gpu):
    """One call of 17 items (16 per launch): each bit-equal to its solo run."""
    names = (sorted(CASES) * 2)[:17]
    items = [_records(name, gpu) for name in names]

    def jobs_of(dsts, fdsts):
        per, fac = [], []
        for (layer, x, g), dst, (A, G) in zip(items, dsts, fdsts):
            per.append(ops.PerSampleNormJob.of(layer, x, g, dst=dst, first=True))
            sides = ops.factor_jobs(layer, x, g)
            sides.a.dst, sides.a.first, sides.g.dst, sides.g.first = A, True, G, True
            fac += [sides.a, sides.g]
        return per, fac

    def buffers():
        shapes = [(l.weight.numel(), 1 + int(l.bias is not None)) for l, _, _ in items]
        return ([torch.full(s, float("nan"), device=gpu) for s in shapes],
                [(torch.full((C, n_g, n_g), float("nan"), device=gpu), torch.full((C, 1, 1), float("nan"), device=gpu))
                 for C, n_g in shapes])
    together, solo = buffers(), buffers()
    per, fac = jobs_of(*together)
    ops.per_sample_norm_sq_accumulate(per)
    ops.accumulate_factors(fac)
    per, fac = jobs_of(*solo)
    for i, job in enumerate(per):
        ops.per_sample_norm_sq_accumulate([job])
        ops.accumulate_factors(fac[2 * i:2 * i + 2])
    for i in range(17):
        assert torch.equal(together[0][i], solo[0][i]), names[i]
        assert torch.equal(together[1][i][0], solo[1][i][0]) and torch.equal(together[1][i][1], solo[1][i][1]), names[i]
        assert torch.isfinite(together[0][i]).all()


@pytest.mark.parametrize("name", ["gn", "gn_split", "ln", "ln_wide"])
def test_offset_input_is_as_accurate_as_torch(gpu, name, capsys):
    """x = 100 + randn.  |p| here (the square root of the p**2 the reduction exposes; its rounding, 6e-8 relative, is far
    below either error) against float64, next to |p| formed in fp32 torch from torch's own GPU normalisation without
    affine.  At this offset the rounding of x - mean dominates both; the margin of 4 allows for another summation order.  A
    cancelling variance formula misses the bar by orders of magnitude."""
    layer, x, g = _records(name, gpu, offset=100.0)
    p64 = _p64(layer, x, g).abs()
    got = _p_squared(layer, x, g).sqrt()
    if isinstance(layer, nn.LayerNorm):
        xh = F.layer_norm(x, layer.normalized_shape, None, None, layer.eps)
        D = layer.weight.numel()
        gx, gg = (g * xh).reshape(x.shape[0], -1, D).sum(1), g.reshape(x.shape[0], -1, D).sum(1)
    else:
        xh = F.group_norm(x, layer.num_groups, None, None, layer.eps)
        gx, gg = (g * xh).sum((2, 3)), g.sum((2, 3))
    torch_p = torch.stack([gx] + ([gg] if layer.bias is not None else []), 2).abs()
    mine, theirs = rel_fro(got, p64), rel_fro(torch_p, p64)
    with capsys.disabled():
        print(f"\noffset {name}: fused pass {mine:.3e}, torch expression {theirs:.3e}")
    assert mine <= 4 * theirs


def _call(symbol, arr, dev):
    L = _lib.lib()
    need = max(int(getattr(L, "curv_persample_norm_workspace_bytes" if "persample" in symbol
                           else "curv_kfac_norm_workspace_bytes")(arr, len(arr))), 1 << 16)
    ws = ops.workspace(need, dev, "test_norm")
    rc = getattr(L, symbol)(_lib.stream_ptr(), arr, len(arr), ws.data_ptr(), ws.numel())
    return rc, L.curv_last_error().decode()


@pytest.mark.parametrize("fault", ["groups", "eps", "var", "extent"])
def test_invalid_descriptors_name_the_item_and_write_nothing(gpu, fault):
    good = _records("gn", gpu)
    layer, x, g = _records("bn" if fault == "var" else "gn", gpu)
    C = layer.weight.numel()
    dsts = [torch.full((6, 2), 7.0, device=gpu), torch.full((C, 2), 7.0, device=gpu)]
    jobs = [ops.PerSampleNormJob.of(*good, dst=dsts[0], first=True), ops.PerSampleNormJob.of(layer, x, g, dst=dsts[1], first=True)]
    arr = ops._per_sample_norm_descs(jobs, "test", "sq")
    if fault == "groups":
        arr[1].groups = 4
    elif fault == "eps":
        arr[1].eps = 0.0
    elif fault == "var":
        arr[1].var = None
    else:
        arr[1].x_elems -= 1
    rc, text = _call("curv_persample_norm_sq_accumulate", arr, gpu)
    assert rc == _lib.ERR_INVALID and "item 1" in text, text
    assert _lib.lib().curv_persample_norm_workspace_bytes(arr, 2) == 0 or fault == "var"    # (host query: no pointers read)
    torch.cuda.synchronize()
    assert all(bool((d == 7.0).all()) for d in dsts)
    # the factor build takes the same descriptor and refuses it the same way
    A0, A = torch.full((6, 2, 2), 7.0, device=gpu), torch.full((C, 2, 2), 7.0, device=gpu)
    arr[0].side, arr[0].dst, arr[1].side, arr[1].dst = _lib.NORM_SIDE_A, A0.data_ptr(), _lib.NORM_SIDE_A, A.data_ptr()
    rc, text = _call("curv_kfac_norm_accumulate", arr, gpu)
    assert rc == _lib.ERR_INVALID and "item 1" in text, text
    torch.cuda.synchronize()
    assert bool((A0 == 7.0).all()) and bool((A == 7.0).all())
    arr[1].reserved = 1
    assert _call("curv_kfac_norm_accumulate", arr, gpu)[0] == _lib.ERR_INVALID
