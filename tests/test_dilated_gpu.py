"""Dilated Conv2d on the GPU (`ops.admit_dilated`): the A-factor build of csrc/dilated_factor.hip through the C ABI against
the float64 Gram of ``F.unfold(..., dilation=...)``, its bit properties and memory edges, the dilated per-sample pack held
bit for bit, and KFAC / Diagonal / EFB / INF and the linearised predictives end to end on a small dilated model.

Expected values are computed here with torch in float64 (the oracle restates the reference, which drops the dilation).
The bar for factors is the project's parity bar of DESIGN.md section 5: relative Frobenius error at most 1e-4 against
float64 (`conftest.rel_fro`)."""
import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import identity_residual_bound, rel_fro
from exact_inputs import assert_exact_range, conv_rows, exact_gram, nonzero_ints, pow2_scale

pytestmark = pytest.mark.gpu
BAR = 1e-4            # the parity bar of every factor
TOL = 1e-4            # TOL of tests/test_per_sample_gpu.py, test_glm_predictive_gpu.py, test_glm_covariance_gpu.py, test_glm_grid_gpu.py


@pytest.fixture(autouse=True)
def admitted():
    from curvature_amd import ops
    was = ops.admit_dilated(True)
    yield
    ops.admit_dilated(was)


def rel2(a, b):
    """Relative 2-norm error (tests/test_glm_predictive_gpu.py)."""
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


# ------------------------------------------------------------------------------------------------ 1. the factor
# name: (N, C, H, W, kernel, dilation, padding)
CASES = {
    "a": (2, 3, 8, 8, 3, 2, 2),                      # one size group
    "b": (3, 5, 7, 9, 3, 2, 2),                      # four size groups
    "c": (2, 4, 7, 9, (5, 3), (3, 2), (6, 2)),       # anisotropic
    "d": (2, 4, 9, 10, 3, 2, 0),                     # no padding
    "e": (2, 3, 3, 4, 3, 4, 4),                      # dilation larger than the image: empty classes (without output pixels)
    "f": (2, 4, 6, 8, 3, (2, 1), (2, 1)),            # one undilated axis
    "g": (2, 64, 8, 8, 3, 2, 2),                     # class stacks of 64 channels
    "h": (2, 128, 8, 8, 3, 2, 2),                    # ... of 128
    "i": (4, 128, 32, 32, 3, 2, 2),                  # a class stack of about 5 GFLOP: above the small-launch threshold
    # beyond the table of the issue: empty classes that DO have output pixels (padding 2 d: the bias-corner rule), and a row
    # longer than the gather pass stages at once (it is walked in pieces)
    "corner": (2, 3, 3, 4, 3, 4, 8),
    "long_row": (1, 2, 3, 4101, (1, 3), (1, 3), (0, 3)),
}
NO_BIAS = ("b", "e", "corner")


@functools.lru_cache(maxsize=None)
def factor_case(name):
    """The source of a case on the GPU and its float64 A factors (with and without the ones row), scale 1 / (N L); made
    once and left unchanged."""
    N, C, H, W, k, d, p = CASES[name]
    gpu = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(N, C, H, W, generator=gen)
    cols = F.unfold(x.double(), pair(k), dilation=pair(d), padding=pair(p))            # (N, C kh kw, L)
    L = cols.shape[2]
    X = cols.transpose(0, 1).reshape(cols.shape[1], -1).to(gpu)
    X1 = torch.cat([X, torch.ones(1, X.shape[1], dtype=X.dtype, device=gpu)])
    want = {False: (X @ X.t() / (N * L)).cpu(), True: (X1 @ X1.t() / (N * L)).cpu()}
    return x.to(gpu), want, 1.0 / (N * L)


def dilated_job(name, src, dst, bias=True, scale=1.0, first=True):
    from curvature_amd import ops
    _, _, _, _, k, d, p = CASES[name]
    return ops.DilatedFactorJob(src, dst, pair(k), (1, 1), pair(p), pair(d), bias, scale, first)


def dim_of(name, bias=True):
    _, C, _, _, k, _, _ = CASES[name]
    return C * pair(k)[0] * pair(k)[1] + int(bias)


@pytest.mark.parametrize("name, bias", [(n, True) for n in CASES] + [(n, False) for n in NO_BIAS])
def test_factor_against_float64(gpu, name, bias):
    from curvature_amd import ops
    x, want, scale = factor_case(name)
    n = dim_of(name, bias)
    dst = torch.full((n, n), float("nan"), device=gpu)
    ops.kfac_accumulate_dilated([dilated_job(name, x, dst, bias, scale)])            # `first` overwrites the NaNs
    got = dst.cpu()
    err = rel_fro(got, want[bias])
    print(f"dilated factor {name} bias={bias}: rel_fro {err:.3e}")
    assert err <= BAR
    assert torch.equal(got, got.t())
    if bias:                                                                          # the ones row against itself: K / K
        assert abs(float(got[-1, -1]) - 1.0) <= 1e-6


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """An integer-valued source of a case (tests/exact_inputs.py), the unscaled integer Grams of its dilated ``F.unfold`` in
    float64 (without and with the ones row), formed on the GPU once, and a power-of-two scale."""
    N, C, H, W, k, d, p = CASES[name]
    gpu = torch.device("cuda:0")
    x = nonzero_ints((N, C, H, W), torch.Generator().manual_seed(sum(map(ord, name)) + 1))
    rows = conv_rows(x.to(gpu), pair(k), 1, pair(p), dilation=pair(d))
    assert_exact_range(3, rows.shape[1], rounds=2)
    return x, {False: exact_gram(rows), True: exact_gram(rows, ones_row=True)}, pow2_scale(rows.shape[1])


@pytest.mark.parametrize("name, bias", [(n, True) for n in CASES] + [(n, False) for n in NO_BIAS])
def test_factor_exact_on_integer_inputs(gpu, name, bias):
    """Every case again, bit for bit: a source uniform in {+-1, +-2, +-3} (none zero, so every element moves the result)
    and a power-of-two scale.  Every product and partial sum is an integer below 2^24, so the gather pass, the plain builds
    of the residue classes, their sum in `dst` and the bias corner of the empty classes have one right answer in any
    summation order: ``scale * exact`` after a first call, twice that after an accumulating one.
    The source sits in NaN-filled memory, at an aligned start and 4 bytes past one."""
    from curvature_amd import ops
    x, exact, scale = exact_case(name)
    n = dim_of(name, bias)
    for offset in (0, 1):
        fence = torch.full((x.numel() + 4096 + 64,), float("nan"), device=gpu)
        start = 2048 + offset
        xs = fence[start:start + x.numel()].view(x.shape)
        xs.copy_(x)
        dst = torch.full((n, n), float("nan"), device=gpu)
        for rounds in (1, 2):
            ops.kfac_accumulate_dilated([dilated_job(name, xs, dst, bias, scale, first=rounds == 1)])
            got, want = dst.double(), rounds * scale * exact[bias]
            assert torch.equal(got, want), (offset, rounds, int((got != want).sum()), float((got - want).abs().max()))
            assert torch.equal(dst, dst.t()), (offset, rounds)


@pytest.mark.parametrize("name", ["a", "b"])
def test_bit_properties(gpu, name):
    from curvature_amd import ops
    x, want, scale = factor_case(name)
    n = dim_of(name)
    once = torch.full((n, n), float("nan"), device=gpu)
    ops.kfac_accumulate_dilated([dilated_job(name, x, once, True, scale)])
    assert torch.equal(once, once.t())                                                # bit-for-bit symmetric
    again = torch.full((n, n), float("nan"), device=gpu)
    ops.kfac_accumulate_dilated([dilated_job(name, x, again, True, scale)])
    assert torch.equal(again, once)
    # first = 0 adds onto what dst holds
    gen = torch.Generator().manual_seed(9)
    held = torch.randn(n, n, generator=gen)
    held = (held + held.t()).to(gpu)
    dst = held.clone()
    ops.kfac_accumulate_dilated([dilated_job(name, x, dst, True, scale, first=False)])
    assert rel_fro(dst - held, want[True]) <= BAR
    assert torch.equal(dst, dst.t())
    if name == "a":                                                                   # one size group: one addition per entry
        assert torch.equal(dst, held + once)


def test_a_factor_has_the_same_bits_alone_and_in_a_call_with_others(gpu):
    from curvature_amd import ops
    names = ["c", "a", "corner", "b", "g"]
    alone, together, jobs = [], [], []
    for name in names:
        x, _, scale = factor_case(name)
        n = dim_of(name)
        a = torch.full((n, n), float("nan"), device=gpu)
        ops.kfac_accumulate_dilated([dilated_job(name, x, a, True, scale)])
        alone.append(a)
        b = torch.full((n, n), float("nan"), device=gpu)
        jobs.append(dilated_job(name, x, b, True, scale))
        together.append(b)
    ops.kfac_accumulate_dilated(jobs)
    for name, a, b in zip(names, alone, together):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("stride, padding", [(1, 1), (2, 0)])
def test_dilation_one_is_the_plain_build_bit_for_bit(gpu, stride, padding):
    from curvature_amd import ops
    x, _, _ = factor_case("b")
    n = dim_of("b")
    plain = torch.full((n, n), float("nan"), device=gpu)
    ops.kfac_accumulate([ops.FactorJob(x, plain, (3, 3), pair(stride), pair(padding), True, 0.125, True)])
    dst = torch.full((n, n), float("nan"), device=gpu)
    ops.kfac_accumulate_dilated([ops.DilatedFactorJob(x, dst, (3, 3), pair(stride), pair(padding), (1, 1), True, 0.125, True)])
    assert torch.equal(dst, plain)


def test_nan_fenced_source(gpu):
    """Case b inside a NaN-filled buffer, at an aligned start and 4 bytes past it (the scalar head of the gather pass):
    nothing outside the source is read."""
    from curvature_amd import ops
    x, want, scale = factor_case("b")
    n = dim_of("b")
    for offset in (0, 1, 3):
        fence = torch.full((x.numel() + 4096 + 64,), float("nan"), device=gpu)
        start = 2048 + offset
        xs = fence[start:start + x.numel()].view(x.shape)
        xs.copy_(x)
        dst = torch.full((n, n), float("nan"), device=gpu)
        ops.kfac_accumulate_dilated([dilated_job("b", xs, dst, True, scale)])
        got = dst.cpu()
        assert torch.isfinite(got).all(), offset
        assert rel_fro(got, want[True]) <= BAR, offset


def test_poisoned_scratch(gpu, monkeypatch):
    """Case b (four size groups) and the corner case with every scratch buffer NaN-filled when it is handed to the library
    (what CURV_DEBUG_POISON=1 does, tests/test_poisoned_workspace_gpu.py): the builds read only what the gather pass wrote."""
    from curvature_amd import ops
    monkeypatch.setattr(ops, "_POISON", True)
    for name in ("b", "corner"):
        x, want, scale = factor_case(name)
        n = dim_of(name)
        dst = torch.full((n, n), float("nan"), device=gpu)
        ops.kfac_accumulate_dilated([dilated_job(name, x, dst, True, scale)])
        got = dst.cpu()
        assert torch.isfinite(got).all(), name
        assert rel_fro(got, want[True]) <= BAR, name


# ------------------------------------------------------------------------------------------------ 2. the pack
SENTINEL = 12345.0


def packed_x(layer, x, g, rows_outer=False):
    """The x operand of `layer` packed by `ops.per_sample_pack`: (sides.x, the (N, rows, Lp) copy on the CPU)."""
    from curvature_amd import ops
    sides = ops.per_sample_operands(layer, x, g, rows_outer=rows_outer, in_place=not rows_outer)
    op = sides.x
    assert op.pack is not None and op.pack.dilation == tuple(layer.dilation)
    dst = torch.full((op.floats + 64,), SENTINEL, device=x.device)
    ops.per_sample_pack([op], [dst])
    host = dst.cpu()
    assert bool((host[op.floats:] == SENTINEL).all())
    N = x.shape[0]
    out = host[:op.floats].view(op.rows, N, op.Lp).permute(1, 0, 2) if rows_outer else host[:op.floats].view(N, op.rows, op.Lp)
    return op, out


def check_pack(layer, x, g, rows_outer=False):
    op, got = packed_x(layer, x, g, rows_outer)
    cols = F.unfold(x.detach().float().cpu().contiguous(), layer.kernel_size, dilation=layer.dilation,
                    padding=layer.padding, stride=layer.stride)
    if layer.bias is not None:
        cols = torch.cat([cols, torch.ones(cols.shape[0], 1, cols.shape[2])], dim=1)
    assert op.L == cols.shape[2] and op.rows == cols.shape[1]
    assert torch.equal(got[:, :, :op.L], cols)                       # a copy (an exact upcast for half sources)
    assert bool((got[:, :, op.L:] == 0).all())


def fenced_randn(shape, gpu, seed, dtype=torch.float32, lead=65):
    gen = torch.Generator().manual_seed(seed)
    values = torch.randn(shape, generator=gen).to(dtype)
    buf = torch.full((values.numel() + lead + 64,), float("nan"), dtype=dtype, device=gpu)
    buf[lead:lead + values.numel()] = values.reshape(-1).to(gpu)
    return buf[lead:lead + values.numel()].view(shape)


@pytest.mark.parametrize("rows_outer", [False, True], ids=["n_major", "rows_outer"])
def test_pack_of_case_b(gpu, rows_outer):
    layer = torch.nn.Conv2d(5, 6, 3, padding=2, dilation=2)
    x, g = fenced_randn((3, 5, 7, 9), gpu, 1), torch.zeros(3, 6, 7, 9, device=gpu)
    check_pack(layer, x, g, rows_outer)
    check_pack(torch.nn.Conv2d(5, 6, 3, padding=2, dilation=2, bias=False), x, g, rows_outer)


def test_pack_takes_a_stride_the_factor_build_refuses(gpu):
    from curvature_amd import ops
    layer = torch.nn.Conv2d(4, 6, 3, stride=2, padding=1, dilation=2)
    x, g = fenced_randn((2, 4, 9, 9), gpu, 2), torch.zeros(2, 6, 4, 4, device=gpu)
    check_pack(layer, x, g)
    anis = torch.nn.Conv2d(4, 6, (2, 3), stride=(1, 2), padding=(0, 3), dilation=(3, 2))
    check_pack(anis, x, torch.zeros(2, 6, 6, 6, device=gpu))
    dst = torch.empty(37, 37, device=gpu)
    with pytest.raises(RuntimeError, match="stride 2x2 with dilation 2x2"):
        ops.kfac_accumulate_dilated([ops.DilatedFactorJob(x.contiguous(), dst, (3, 3), (2, 2), (1, 1), (2, 2), True)])


def test_pack_of_a_channels_last_source(gpu):
    layer = torch.nn.Conv2d(5, 6, 3, padding=2, dilation=2)
    x = fenced_randn((3, 7, 9, 5), gpu, 3).permute(0, 3, 1, 2)            # (N, C, H, W) view of an (N, H, W, C) record
    assert x.stride()[1] == 1
    check_pack(layer, x, torch.zeros(3, 6, 7, 9, device=gpu))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_pack_of_a_half_source(gpu, dtype):
    from curvature_amd import ops
    layer = torch.nn.Conv2d(5, 6, 3, padding=2, dilation=2)
    x, g = fenced_randn((3, 5, 7, 9), gpu, 4, dtype), torch.zeros(3, 6, 7, 9, device=gpu)
    with pytest.raises(RuntimeError, match="widen_per_sample"):
        ops.per_sample_operands(layer, x, g)
    was = ops.widen_per_sample(True)
    try:
        check_pack(layer, x, g)
    finally:
        ops.widen_per_sample(was)


# ------------------------------------------------------------------------------------------------ 3. end to end
N_MODEL, CLASSES = 4, 5
ADD, MULTIPLY = 0.5, 2.0


def make_model(gpu, seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=2, dilation=2), torch.nn.ReLU(),
                               torch.nn.Conv2d(8, 8, 3, padding=4, dilation=4, bias=False), torch.nn.Flatten(),
                               torch.nn.Linear(800, CLASSES)).to(gpu)


def selected(model):
    return [model[0], model[2], model[4]]


def backward(model, x, labels):
    model.zero_grad()
    F.cross_entropy(model(x), labels).backward()


def wb(weight_grad, bias_grad):
    """[W | b] of a layer from gradients shaped like its parameters."""
    flat = weight_grad.reshape(weight_grad.shape[0], -1)
    return flat if bias_grad is None else torch.cat([flat, bias_grad.reshape(-1, 1)], dim=1)


@functools.lru_cache(maxsize=None)
def setting():
    """The model on the GPU, a batch, and from a float64 CPU copy: the per-sample gradients of the batch-mean loss
    (N single-sample backward passes) and the per-sample Jacobians of every logit, each as [W | b] per layer.  Made once."""
    gpu = torch.device("cuda:0")
    model = make_model(gpu)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(N_MODEL, 3, 10, 10, generator=gen).to(gpu)
    labels = torch.tensor([1, 4, 0, 2], device=gpu)
    ref = copy.deepcopy(model).double().cpu().eval()
    layers = selected(ref)
    params = [p for l in layers for p in l.parameters()]

    def per_layer(grads):
        out, it = [], iter(grads)
        for l in layers:
            gw = next(it)
            out.append(wb(gw, next(it) if l.bias is not None else None))
        return out
    x64, y = x.double().cpu(), labels.cpu()
    shares = []                                           # shares[n][k]: sample n's part of the batch gradient of layer k
    for n in range(N_MODEL):
        loss = F.cross_entropy(ref(x64[n:n + 1]), y[n:n + 1])
        shares.append([P / N_MODEL for P in per_layer(torch.autograd.grad(loss, params))])
    logits = ref(x64)
    jac = [[per_layer(torch.autograd.grad(logits[n, c], params, retain_graph=True)) for c in range(CLASSES)]
           for n in range(N_MODEL)]                       # jac[n][c][k]
    # (classes, N, m, n) per layer, as tests/test_glm_grid_gpu.py holds them
    jac = [torch.stack([torch.stack([jac[n][c][k] for n in range(N_MODEL)]) for c in range(CLASSES)])
           for k in range(len(layers))]
    return model, x, labels, shares, jac, logits.detach()


@functools.lru_cache(maxsize=None)
def estimator(kind):
    """`kind` after one update on the batch, inverted with (ADD, MULTIPLY); KFAC decomposed as well."""
    from curvature_amd.curvatures import KFAC, Diagonal
    model, x, labels = setting()[:3]
    est = KFAC(model) if kind == "kfac" else Diagonal(model)
    backward(model, x, labels)
    est.update(N_MODEL)
    est.invert(add=ADD, multiply=MULTIPLY)
    if kind == "kfac":
        est.decompose()
    return est


def float64_factors(layer, xin, g):
    """(A, G) of KFAC.update on the records (xin, g) in float64."""
    xin, g = xin.detach().double().cpu(), g.detach().double().cpu()
    N = xin.shape[0]
    if isinstance(layer, torch.nn.Conv2d):
        cols = F.unfold(xin, layer.kernel_size, dilation=layer.dilation, padding=layer.padding, stride=layer.stride)
        L = cols.shape[2]
        X = cols.transpose(0, 1).reshape(cols.shape[1], -1)
        gs = g.permute(1, 0, 2, 3).reshape(g.shape[1], -1)
    else:
        L, X, gs = 1, xin.t(), g.t()
    if layer.bias is not None:
        X = torch.cat([X, torch.ones(1, X.shape[1], dtype=X.dtype)])
    return X @ X.t() / (N * L), gs @ gs.t() * N / L


def test_kfac_update_invert_and_sample(gpu):
    model, x, labels = setting()[:3]
    kfac = estimator("kfac")
    layers = selected(model)
    for layer in layers:
        A_ref, G_ref = float64_factors(layer, *kfac.record[layer])
        A, G = kfac.state[layer]
        err_a, err_g = rel_fro(A, A_ref), rel_fro(G, G_ref)
        print(f"KFAC state {layer.__class__.__name__}: A {err_a:.3e}, G {err_g:.3e}")
        assert err_a <= BAR and err_g <= BAR
        assert torch.equal(A, A.t())
        for Fm, Lf in zip(kfac.state[layer], kfac.inv_state[layer]):
            n = Fm.shape[0]
            M = math.sqrt(MULTIPLY) * Fm.double() + math.sqrt(ADD) * torch.eye(n, device=gpu, dtype=torch.float64)
            M = (M + M.t()) / 2
            R = (Lf.double() @ Lf.double().t()) @ M - torch.eye(n, device=gpu, dtype=torch.float64)
            assert float(torch.linalg.norm(R)) / n ** 0.5 < identity_residual_bound(M)
    # sample_and_replace with given noise against L_G Z^T L_A^T in float64 (tests/test_conv_transpose_gpu.py: 1e-5)
    mean = {l: (l.weight.detach().clone(), None if l.bias is None else l.bias.detach().clone()) for l in layers}
    noise = {l: torch.randn(kfac.inv_state[l][0].size(0), kfac.inv_state[l][1].size(0), device=gpu) for l in layers}
    try:
        kfac.sample_and_replace(noise=noise)
        torch.cuda.synchronize()
        for layer in layers:
            la, lg = (t.double() for t in kfac.inv_state[layer])
            s = (la @ noise[layer].double() @ lg.t()).t()                       # (out, n) as [W | b]
            n0 = layer.weight[0].numel()
            assert rel_fro(layer.weight - mean[layer][0], s[:, :n0].reshape(layer.weight.shape)) <= 1e-5
            if layer.bias is not None:
                assert rel_fro(layer.bias - mean[layer][1], s[:, -1]) <= 1e-5
    finally:
        with torch.no_grad():
            for layer in layers:
                layer.weight.copy_(mean[layer][0])
                if layer.bias is not None:
                    layer.bias.copy_(mean[layer][1])


def test_per_sample_diagonal_and_efb(gpu):
    """Against per-sample gradients from N single-sample backward passes in float64 (TOL of tests/test_per_sample_gpu.py)."""
    from curvature_amd.curvatures import EFB, Diagonal
    model, x, labels, shares = setting()[:4]
    kfac = estimator("kfac")
    layers = selected(model)
    diag = Diagonal(model, per_sample=True)
    efb = EFB(model, kfac.state, per_sample=True)
    try:
        backward(model, x, labels)
        diag.update(N_MODEL)
        efb.update(N_MODEL)
        for k, layer in enumerate(layers):
            want = N_MODEL * sum(shares[n][k] ** 2 for n in range(N_MODEL))
            U_A, U_G = (u.double().cpu() for u in efb.eigvecs[layer])
            want_e = N_MODEL * sum((U_G.t() @ shares[n][k] @ U_A) ** 2 for n in range(N_MODEL))
            err, err_e, err_d = rel_fro(diag.state[layer], want), rel_fro(efb.state[layer], want_e), rel_fro(efb.diags[layer], want)
            print(f"per-sample layer {k}: Diagonal {err:.3e}, EFB lambda {err_e:.3e}, EFB diags {err_d:.3e}")
            assert err < TOL and err_e < TOL and err_d < TOL
    finally:
        for est in (diag, efb):
            for hook in est.hooks:
                hook.remove()


def float64_variance(kind, est, model, jac):
    """(N, classes, classes): Sigma_n[c, c'] = sum_layers <T(P_c), T(P_c')>, T(P) = L_G^T P L_A (KFAC) or inv * P (Diagonal)
    on the estimator's own inverse state (tests/test_glm_covariance_gpu.py)."""
    want = torch.zeros(N_MODEL, CLASSES, CLASSES, dtype=torch.float64)
    for k, layer in enumerate(selected(model)):
        P = jac[k].permute(1, 0, 2, 3)                                       # (N, classes, m, n)
        if kind == "kfac":
            L_A, L_G = (t.double().cpu() for t in est.inv_state[layer])
            T = L_G.t() @ P @ L_A
        else:
            T = est.inv_state[layer].double().cpu() * P
        want += torch.einsum("ncij,ndij->ncd", T, T)
    return want


HYPERS = [(0.1, 1.0), (1.0, 100.0), (10.0, 1.0), (ADD, MULTIPLY)]


def float64_grid(kind, est, model, jac):
    """(H, N, classes) of DESIGN K12 in float64 (tests/test_glm_grid_gpu.py)."""
    want = torch.zeros(len(HYPERS), N_MODEL, CLASSES, dtype=torch.float64)
    for k, layer in enumerate(selected(model)):
        P = jac[k]                                                            # (classes, N, m, n)
        if kind == "kfac":
            A, G = (t.double().cpu() for t in est.state[layer])
            (lam_A, U_A), (lam_G, U_G) = torch.linalg.eigh(A), torch.linalg.eigh(G)
            lam_A, lam_G = lam_A.clamp_min(0), lam_G.clamp_min(0)
            P = U_G.t() @ P @ U_A
        Q2 = (P * P).permute(1, 0, 2, 3)
        for h, (add, multiply) in enumerate(HYPERS):
            rho = add / multiply
            if kind == "kfac":
                w = 1.0 / ((lam_G + math.sqrt(rho))[:, None] * (lam_A + math.sqrt(rho))[None, :])
            else:
                w = 1.0 / (est.state[layer].double().cpu() + rho)
            want[h] += (w * Q2).sum((2, 3)) / multiply
    return want


@pytest.mark.parametrize("kind", ["kfac", "diag"])
def test_linearised_predictives_against_float64(gpu, kind):
    from curvature_amd.evaluate import glm_predictive, glm_predictive_grid, glm_predictive_joint
    model, x, labels, _, jac, logits64 = setting()
    est = estimator(kind)
    sigma = float64_variance(kind, est, model, jac)
    want_var = torch.diagonal(sigma, dim1=1, dim2=2)

    logits, variance, probs = glm_predictive(model, est, x)
    err = rel2(variance, want_var)
    print(f"{kind}: variance {err:.3e}")
    assert err < TOL and rel2(logits, logits64) < TOL
    probit = torch.softmax(logits.double().cpu() / torch.sqrt(1.0 + math.pi / 8.0 * want_var), dim=1)
    assert float((probs.double().cpu() - probit).abs().max()) < 1e-5

    _, covariance, _ = glm_predictive_joint(model, est, x)
    err = rel2(covariance, sigma)
    print(f"{kind}: covariance {err:.3e}")
    assert tuple(covariance.shape) == (N_MODEL, CLASSES, CLASSES) and err < TOL
    assert torch.equal(covariance, covariance.transpose(1, 2))
    assert rel2(torch.diagonal(covariance, dim1=1, dim2=2), variance) < 2 * TOL

    _, grid, _ = glm_predictive_grid(model, est, x, HYPERS)
    want = float64_grid(kind, est, model, jac)
    worst = max(rel2(g, w) for g, w in zip(grid, want))
    print(f"{kind}: grid, worst row {worst:.3e}")
    assert tuple(grid.shape) == (len(HYPERS), N_MODEL, CLASSES) and worst < TOL
    assert rel2(grid[-1], variance) < TOL                                    # the pair the estimator was inverted with
    assert not model.training


def test_estimator_chain(gpu):
    """Diagonal -> KFAC -> EFB -> INF construct, invert and sample; EFB's state is (U_G^T grad U_A)**2
    (tests/test_conv_transpose_gpu.py: 1e-5)."""
    from curvature_amd.curvatures import EFB, INF, KFAC, Diagonal
    model = make_model(gpu, seed=5)
    gen = torch.Generator().manual_seed(6)
    x, labels = torch.randn(N_MODEL, 3, 10, 10, generator=gen).to(gpu), torch.tensor([3, 0, 2, 2], device=gpu)
    layers = selected(model)
    diag, kfac = Diagonal(model), KFAC(model)
    backward(model, x, labels)
    diag.update(N_MODEL)
    kfac.update(N_MODEL)
    efb = EFB(model, kfac.state)
    efb.update(N_MODEL)
    torch.cuda.synchronize()
    for layer in layers:
        grad = wb(layer.weight.grad.double(), None if layer.bias is None else layer.bias.grad.double())
        ua, ug = (t.double() for t in efb.eigvecs[layer])
        assert rel_fro(efb.state[layer], (ug.t() @ grad @ ua) ** 2) <= 1e-5
        assert rel_fro(diag.state[layer], grad ** 2 * N_MODEL) <= 1e-6
    inf = INF(model, diag.state, kfac.state, efb.state, eigvecs=efb.eigvecs)
    inf.update(rank=20)
    for est in (diag, kfac, efb, inf):
        est.invert(add=ADD, multiply=MULTIPLY)
        est.sample_and_replace()
        torch.cuda.synchronize()
        for layer in layers:
            assert torch.isfinite(layer.weight).all() and (layer.bias is None or torch.isfinite(layer.bias).all())


def test_graph_replay_equals_eager(gpu):
    """One capture of the KFAC step on the dilated model (the smallest case of tests/test_graph_gpu.py): replay and eager
    agree bit for bit, factors included."""
    from curvature_amd.curvatures import KFAC
    from curvature_amd.graph import KFACStepGraph

    def setup():
        model = make_model(gpu, seed=7)
        gen = torch.Generator().manual_seed(8)
        x, labels = torch.randn(N_MODEL, 3, 10, 10, generator=gen).to(gpu), torch.tensor([0, 1, 2, 3], device=gpu)
        kfac = KFAC(model)
        kfac.noise_seed = 7
        backward(model, x, labels)
        return model, kfac

    model_e, eager = setup()
    weights = []
    for _ in range(2):
        eager.update(N_MODEL)
        eager.invert(ADD, MULTIPLY)
        eager.sample_and_replace()
        weights.append([p.detach().clone() for p in model_e.parameters()])
    model_g, kfac = setup()
    graph = KFACStepGraph(kfac, add=ADD, multiply=MULTIPLY, batch_size=N_MODEL, warmup=2)
    for step in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(model_g.parameters(), weights[step]):
            assert torch.equal(a.detach(), b), step
    graph.check()
    for le, lg in zip(selected(model_e), selected(model_g)):
        for a, b in zip(eager.state[le], kfac.state[lg]):
            assert torch.equal(a, b)
