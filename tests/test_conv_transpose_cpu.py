"""ConvTranspose2d support without a GPU: layer selection, construction-time checks, the host-only C ABI of the
phase-split A-factor build (curv_kfac_convt_*), and the fp64 oracle the GPU tests compare against."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from curvature_amd import _lib, ops
from curvature_amd.curvatures import EFB, INF, KFAC, SUPPORTED_LAYERS, BlockDiagonal, Diagonal


def convt_patches(x, layer, out_size):
    """fp64 oracle: (C kh kw, N Ho Wo) patch matrix of a ConvTranspose2d in Wm column order.  The input is zero-stuffed,
    padded by k - 1 - p (cropped where p > k - 1) plus the output padding at the far edge, unfolded, and the taps flipped."""
    x = x.detach().double().cpu()
    N, C, H, W = x.shape
    (kh, kw), (sh, sw), (ph, pw) = layer.kernel_size, layer.stride, layer.padding
    Ho, Wo = out_size
    xs = torch.zeros(N, C, (H - 1) * sh + 1, (W - 1) * sw + 1, dtype=torch.float64)
    xs[:, :, ::sh, ::sw] = x

    def edge(t, dim, e, extra):
        if e < 0:                                    # crop instead of padding negatively
            t = t.narrow(dim, -e, t.shape[dim] + 2 * e)
            e = 0
        before, after = list(t.shape), list(t.shape)
        before[dim], after[dim] = e, e + extra
        return torch.cat([t.new_zeros(before), t, t.new_zeros(after)], dim)

    xs = edge(xs, 2, kh - 1 - ph, Ho - ((H - 1) * sh - 2 * ph + kh))
    xs = edge(xs, 3, kw - 1 - pw, Wo - ((W - 1) * sw - 2 * pw + kw))
    U = F.unfold(xs, (kh, kw))
    assert U.shape[2] == Ho * Wo
    U = U.view(N, C, kh, kw, -1).flip(2).flip(3).reshape(N, C * kh * kw, -1)
    return U.permute(1, 0, 2).reshape(C * kh * kw, -1)


def oracle_factors(layer, x, g):
    """fp64 (A, G) of a ConvTranspose2d: A = sum a a^T / (N L) with the bias row, G = (N / L) sum g g^T."""
    g = g.detach().double().cpu()
    N, L = g.shape[0], g.shape[2] * g.shape[3]
    U = convt_patches(x, layer, g.shape[2:])
    if layer.bias is not None:
        U = torch.cat([U, torch.ones(1, U.shape[1], dtype=U.dtype)])
    gs = g.permute(1, 0, 2, 3).reshape(g.shape[1], -1)
    return U @ U.t() / (N * L), gs @ gs.t() * N / L


# (cin, cout, kernel, stride, padding, output_padding, H, W)
ORACLE_CASES = [
    (3, 2, 4, 2, 1, 0, 3, 4),
    (2, 3, 3, 2, 1, 1, 4, 3),
    (3, 2, 2, 2, 0, 0, 3, 3),
    (3, 2, (5, 3), (3, 2), (2, 1), (2, 1), 4, 5),
    (2, 2, 4, 1, 0, 0, 1, 1),
    (2, 2, 3, 2, 3, 0, 5, 5),                   # padding > k - 1
]


@pytest.mark.parametrize("case", ORACLE_CASES)
def test_oracle_matches_weight_grad(case):
    cin, cout, k, s, p, op, H, W = case
    torch.manual_seed(0)
    layer = torch.nn.ConvTranspose2d(cin, cout, k, s, p, op).double()
    x = torch.randn(2, cin, H, W, dtype=torch.float64)
    y = layer(x)
    g = torch.randn_like(y)
    y.backward(g)
    U = convt_patches(x, layer, y.shape[2:])
    gs = g.permute(1, 0, 2, 3).reshape(cout, -1)
    wm = layer.weight.grad.permute(1, 0, 2, 3).reshape(cout, -1)
    assert torch.allclose(gs @ U.t(), wm, rtol=1e-12, atol=1e-12)
    # taps of different residues (a mod s_h, b mod s_w) never meet in one patch
    A = U @ U.t()
    kh, kw = layer.kernel_size
    sh, sw = layer.stride
    t = torch.arange(cin * kh * kw) % (kh * kw)
    res = (t // kw % sh) * sw + (t % kw % sw)
    assert (A[res[:, None] != res[None, :]] == 0).all()


def _model():
    return torch.nn.Sequential(torch.nn.ConvTranspose2d(4, 3, 4, 2, 1), torch.nn.ReLU(), torch.nn.Conv2d(3, 2, 3))


def test_selection():
    assert SUPPORTED_LAYERS == ['Linear', 'Conv2d', 'MultiheadAttention']
    m = _model()
    k = KFAC(m, ['ConvTranspose2d', 'Conv2d'])
    assert k._layers() == [m[0], m[2]]
    assert KFAC(m, 'ConvTranspose2d')._layers() == [m[0]]
    assert KFAC(m)._layers() == [m[2]]                     # default selection unchanged
    with pytest.raises(AssertionError):
        KFAC(m, ['Conv3d'])


@pytest.mark.parametrize("kwargs", [dict(groups=2), dict(dilation=2)])
def test_rejected_geometries(kwargs):
    m = torch.nn.Sequential(torch.nn.ConvTranspose2d(4, 4, 3, 2, 1, **kwargs))
    for est in (KFAC, Diagonal):
        with pytest.raises(NotImplementedError):
            est(m, ['ConvTranspose2d'])
    # not selected: nothing to reject
    KFAC(m)


def test_string_padding_rejected():
    layer = torch.nn.ConvTranspose2d(4, 4, 3, 2, 1)
    layer.padding = 'same'
    with pytest.raises(NotImplementedError):
        KFAC(torch.nn.Sequential(layer), ['ConvTranspose2d'])


def test_block_diagonal_rejects():
    with pytest.raises(NotImplementedError):
        BlockDiagonal(_model(), ['ConvTranspose2d'])
    BlockDiagonal(_model(), ['Conv2d'])


def test_efb_inf_accept_the_layer_type():
    m = _model()
    EFB(m, {}, ['ConvTranspose2d'], eigvecs={})
    INF(m, {}, {}, {}, ['ConvTranspose2d'], eigvecs={})


def _desc(N=2, C=8, H=5, W=5, k=4, s=2, p=1, Ho=None, Wo=None, bias=1):
    arr = (_lib.curv_convt_factor_desc * 1)()
    d = arr[0]
    d.N, d.C, d.H, d.W = N, C, H, W
    d.kh = d.kw = k
    d.sh = d.sw = s
    d.ph = d.pw = p
    d.Ho = Ho if Ho is not None else (H - 1) * s - 2 * p + k
    d.Wo = Wo if Wo is not None else (W - 1) * s - 2 * p + k
    d.has_bias, d.first, d.scale = bias, 1, 1.0
    return arr


def test_empty_call():
    L = _lib.lib()
    assert L.curv_kfac_convt_workspace_bytes(None, 0) == 0
    assert L.curv_kfac_convt_accumulate(None, None, 0, None, 0) == 0
    assert L.curv_kfac_convt_plan_flops(None, 0, None) == 0
    ops.kfac_accumulate_convt([])
    assert ops.kfac_convt_plan_flops([]) == []


@pytest.mark.parametrize("field,value", [("N", 0), ("C", -1), ("kh", 0), ("sw", 0), ("ph", -1), ("Ho", 5), ("Wo", 12),
                                         ("sh", 9)])
def test_invalid_geometry(field, value):
    arr = _desc()
    setattr(arr[0], field, value)
    if field == "sh":                            # 9 x 2 phases: still valid geometry if the output fits ...
        arr[0].sw = 9                            # ... 81 phases is not
        arr[0].kh = arr[0].kw = 9
        arr[0].Ho = arr[0].Wo = 4 * 9 - 2 + 9
    L = _lib.lib()
    assert L.curv_kfac_convt_workspace_bytes(arr, 1) == 0
    assert b"factor 0" in L.curv_last_error()
    out = (ctypes.c_longlong * 1)()
    assert L.curv_kfac_convt_plan_flops(arr, 1, out) == _lib.ERR_INVALID


@pytest.mark.parametrize("geom", [
    dict(C=512, H=4, W=4, k=4, s=2, p=1),
    dict(C=64, H=16, W=16, k=4, s=2, p=1),
    dict(C=512, H=28, W=28, k=2, s=2, p=0),
    dict(C=100, H=1, W=1, k=4, s=1, p=0),
    dict(C=32, H=9, W=9, k=3, s=2, p=1, Ho=18, Wo=18),
])
def test_plan_flops_and_workspace(geom):
    arr = _desc(N=8, **geom)
    L = _lib.lib()
    assert L.curv_kfac_convt_workspace_bytes(arr, 1) > 0
    out = (ctypes.c_longlong * 1)()
    assert L.curv_kfac_convt_plan_flops(arr, 1, out) == 0
    d = arr[0]
    n = d.C * d.kh * d.kw + 1
    dense = n * (n + 1) * d.N * d.Ho * d.Wo
    assert 0 < out[0] <= dense / (d.sh * d.sw) * 1.1
    job = ops.ConvTFactorJob((d.N, d.C, d.H, d.W), None, (d.kh, d.kw), (d.sh, d.sw), (d.ph, d.pw), (d.Ho, d.Wo), True)
    assert ops.kfac_convt_plan_flops([job]) == [out[0]]


def test_kernel_equal_stride_builds_one_gram():
    """k == s, p == 0: every phase is the same 1x1 Gram of the input, built once: (C + 1)(C + 2) N H W flops."""
    arr = _desc(N=4, C=64, H=8, W=8, k=2, s=2, p=0)
    out = (ctypes.c_longlong * 1)()
    assert _lib.lib().curv_kfac_convt_plan_flops(arr, 1, out) == 0
    assert out[0] <= 2 * 65 * 66 * 4 * 8 * 8
