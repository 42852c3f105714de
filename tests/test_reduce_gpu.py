"""KFAC-reduce on the GPU: the reduce pass and factor build of csrc/reduce_factor.hip through the C ABI
against float64 on the CPU (``F.unfold(...).mean(2)`` or plain sums), their bit properties and memory edges, and
``KFAC(approximation="reduce")`` end to end on a small convolutional model (C) and a token model (T).

The bar for factors and rows is the project's parity bar of DESIGN.md section 5: relative Frobenius error at most 1e-4
against float64 (`conftest.rel_fro`); predictives are held to the TOL of tests/test_dilated_gpu.py."""
import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import identity_residual_bound, rel_fro
from exact_inputs import assert_exact_range, exact_gram, nonzero_ints, pow2_scale

pytestmark = pytest.mark.gpu
BAR = 1e-4            # the parity bar of every factor
TOL = 1e-4            # TOL of tests/test_dilated_gpu.py


def rel2(a, b):
    """Relative 2-norm error (tests/test_glm_predictive_gpu.py)."""
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


# ------------------------------------------------------------------------------------------------ 1. the factor
# plane form, name: (shape, kernel, stride, padding)
PLANES = {
    "a": ((2, 3, 5, 7), 3, 1, 1),
    "b": ((2, 3, 5, 7), 3, 2, 1),
    "c": ((3, 2, 9, 6), (5, 3), (2, 1), (2, 0)),
    "d": ((1, 1, 3, 4), 3, 1, 3),
    "e": ((2, 4, 8, 8), 1, 2, 0),                    # a strided 1x1 reads a sub-grid, not the plane mean
    "f": ((2, 2, 7, 7), 7, 2, 3),
    "g": ((2, 2, 6, 5), 2, 3, (0, 1)),               # stride above kernel, trailing rows unused
    "h": ((2, 3, 1, 1), 3, 1, 1),                    # eight of nine taps see padding only
    "i": ((1, 2, 70, 70), 3, 1, 1),                  # a plane longer than one tile: walked in pieces
    "j": ((4, 130, 4, 4), 3, 1, 1),                  # dim 1170 / 1171, many small planes per workgroup
    # beyond the table of the issue: a row longer than the tile (column pieces), strided
    "long_row": ((1, 2, 3, 4201), (2, 3), (1, 2), (1, 1)),
}
G_SIDES = {"ga": (2, 3, 5, 7), "gj": (4, 130, 4, 4), "gi": (1, 2, 70, 70)}       # mean = 0, 1x1
# (the issue's four, then: several pieces of more than 256 entries each; rows longer than the tile)
TOKENS = {"t257": (2, 5, 7), "t318": (3, 1, 8), "tbig": (2, 300, 130), "tmid": (2, 20, 300), "twide": (2, 3, 4500)}


def seed_of(name):
    return sum(map(ord, name))


def gram(rows, bias, scale):
    if bias:
        rows = torch.cat([rows, torch.ones(rows.shape[0], 1, dtype=rows.dtype)], dim=1)
    return rows.t() @ rows * scale


@functools.lru_cache(maxsize=None)
def case(name, dtype=torch.float32):
    """(source on the GPU, float64 rows (N, dim) of the values as `dtype` holds them, job arguments): made once and left
    unchanged.  The factor of a case is ``gram(rows, bias, scale)`` with scale 1 / N."""
    gen = torch.Generator().manual_seed(seed_of(name))
    gpu = torch.device("cuda:0")
    if name in PLANES:
        shape, k, s, p = PLANES[name]
        x = torch.randn(shape, generator=gen).to(dtype)
        rows = F.unfold(x.double(), pair(k), padding=pair(p), stride=pair(s)).mean(2)
        args = dict(kernel=pair(k), stride=pair(s), padding=pair(p), mean=True)
    elif name in G_SIDES:
        x = torch.randn(G_SIDES[name], generator=gen).to(dtype)
        rows = x.double().sum((2, 3))
        args = dict(mean=False)
    else:
        from curvature_amd import _lib
        x = torch.randn(TOKENS[name.rstrip("+")], generator=gen).to(dtype)
        mean = not name.endswith("+")                                  # "name+": the sum over the tokens (the G side)
        rows = x.double().mean(1) if mean else x.double().sum(1)
        args = dict(form=_lib.REDUCE_TOKEN, mean=mean)
    return x.to(gpu), rows, args


def job(name, src, dst, bias=True, scale=1.0, first=True, dtype=torch.float32):
    from curvature_amd import ops
    return ops.ReduceFactorJob(src, dst, has_bias=bias, scale=scale, first=first, **case(name, dtype)[2])


def build(name, bias=True, dtype=torch.float32, src=None, first=True, dst=None):
    """The factor of a case (scale 1 / N) built alone into a NaN-filled destination."""
    from curvature_amd import ops
    x, rows, _ = case(name, dtype)
    n = rows.shape[1] + int(bias)
    if dst is None:
        dst = torch.full((n, n), float("nan"), device=x.device)
    ops.kfac_accumulate_reduce([job(name, x if src is None else src, dst, bias, 1.0 / rows.shape[0], first, dtype)])
    return dst


def last_rows(name, dtype=torch.float32):
    """The rows the reduce pass of the LAST single-factor call left at the head of its scratch."""
    from curvature_amd import ops
    x, rows, _ = case(name, dtype)
    ws = ops.workspace(1, x.device, "kfac_reduce")
    return ws[:rows.numel() * 4].view(torch.float32).view(rows.shape).cpu()


ALL = [(n, b) for n in list(PLANES) for b in (True, False)] + [(n, False) for n in G_SIDES] + \
      [(n + s, b) for n in TOKENS for s, b in (("", True), ("", False), ("+", False)) if n not in ("tmid", "twide") or (s, b) == ("", False)]


@pytest.mark.parametrize("name, bias", ALL, ids=[f"{n}-{'bias' if b else 'nobias'}" for n, b in ALL])
def test_factor_and_rows_against_float64(gpu, name, bias):
    _, rows, _ = case(name)
    got = build(name, bias).cpu()
    err_rows = rel_fro(last_rows(name), rows)
    want = gram(rows, bias, 1.0 / rows.shape[0])
    err = rel_fro(got, want)
    print(f"reduce {name} bias={bias}: rows {err_rows:.3e}, factor {err:.3e}")
    assert err_rows <= BAR and err <= BAR
    assert torch.equal(got, got.t())                                                  # symmetric bit for bit
    if bias:                                                                          # the ones column against itself: N / N
        assert abs(float(got[-1, -1]) - 1.0) <= 1e-6


# Exactness cases (tests/exact_inputs.py).  The reduce pass multiplies a mean row by 1 / L, which is exact only where L - the
# output pixels Ho Wo of a plane, the tokens T - is a power of two; a sum row (the G side) is exact at any L.
# name: (shape, kernel, stride, padding, mean) for planes, (shape, mean) for tokens
EXACT_PLANES = {
    "p8": ((2, 3, 8, 8), 3, 1, 1, True),                 # L = 64
    "p8x4": ((3, 5, 8, 4), 1, 1, 0, True),               # L = 32, 1x1
    "p_s2": ((2, 3, 8, 8), 3, 2, 1, True),               # L = 16, strided window
    "e": ((2, 4, 8, 8), 1, 2, 0, True),                  # L = 16, the sub-grid of case e
    "many": ((4, 130, 4, 4), 3, 1, 1, True),             # L = 16, dim 1170 / 1171: many small planes per workgroup
    "long": ((1, 2, 128, 64), 3, 1, 1, True),            # L = 8192: a plane longer than RD_TILE (4096), walked in pieces
    "long1x1": ((2, 2, 64, 128), 1, 1, 0, True),         # the same through the 1x1 window
    "g_sum": ((2, 3, 5, 7), 1, 1, 0, False),             # sums: any L
    "g_long": ((1, 2, 70, 70), 1, 1, 0, False),
}
EXACT_TOKENS = {
    "t16": ((2, 16, 70), True),                          # T = 16, E = 70
    "t64": ((2, 64, 130), True),                         # T E above RD_TILE: several pieces
    "t4wide": ((2, 4, 4500), True),                      # rows longer than the tile
    "t_sum": ((2, 5, 7), False),
    "tbig_sum": ((2, 300, 130), False),
}
EXACT = [(n, b) for n, c in EXACT_PLANES.items() for b in ((True, False) if c[4] else (False,))] + \
        [(n, b) for n, c in EXACT_TOKENS.items() for b in ((True, False) if c[1] else (False,))]


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """(source, integer per-sample SUMS (N, dim) in float64, L if the row is a mean else 1, job arguments): made once."""
    gen = torch.Generator().manual_seed(seed_of(name))
    if name in EXACT_PLANES:
        shape, k, s, p, mean = EXACT_PLANES[name]
        x = nonzero_ints(shape, gen)
        cols = F.unfold(x.double(), pair(k), padding=pair(p), stride=pair(s))
        sums, L = cols.sum(2), cols.shape[2]
        args = dict(kernel=pair(k), stride=pair(s), padding=pair(p), mean=mean)
    else:
        from curvature_amd import _lib
        shape, mean = EXACT_TOKENS[name]
        x = nonzero_ints(shape, gen)
        sums, L = x.double().sum(1), shape[1]
        args = dict(form=_lib.REDUCE_TOKEN, mean=mean)
    if mean:
        assert L & (L - 1) == 0, "a mean row is exact only over a power-of-two count"
    # the rows are sums / L: dyadic fractions whose products and sums over the N samples are exact while those of the
    # integer sums stay below 2^24 (the ones column has a one-bit significand and does not count)
    assert_exact_range(int(sums.abs().max()), shape[0], rounds=2)
    return x, sums, (L if mean else 1), args


@pytest.mark.parametrize("name, bias", EXACT, ids=[f"{n}-{'bias' if b else 'nobias'}" for n, b in EXACT])
def test_factor_exact_on_integer_inputs(gpu, name, bias):
    """Bit for bit: a source uniform in {+-1, +-2, +-3} (none zero, so every element moves the result) and a power-of-two
    scale.  Every per-sample sum is an integer below 2^24 whatever the order of its pieces, the division by a power-of-two
    L is exact, and the Gram of the N rows has exact products and sums: ``scale * exact`` after a first call, twice that
    after an accumulating one.  The reference is the integer Gram of the per-sample sums [and a
    column of L] divided by L^2.  The source sits in NaN-filled memory, at an aligned start and 4 bytes past one; the rows
    the pass leaves in its scratch are exact too."""
    from curvature_amd import ops
    x, sums, L, args = exact_case(name)
    N = sums.shape[0]
    rows = torch.cat([sums, torch.full((N, 1), float(L), dtype=torch.float64)], dim=1) if bias else sums
    scale = pow2_scale(N)
    want = (exact_gram(rows.t()) / L ** 2).to(gpu)
    n = rows.shape[1]
    for offset in (0, 1):
        fence = torch.full((x.numel() + 4096 + 64,), float("nan"), device=gpu)
        start = 2048 + offset
        xs = fence[start:start + x.numel()].view(x.shape)
        xs.copy_(x)
        dst = torch.full((n, n), float("nan"), device=gpu)
        for rounds in (1, 2):
            ops.kfac_accumulate_reduce([ops.ReduceFactorJob(xs, dst, has_bias=bias, scale=scale, first=rounds == 1, **args)])
            got = dst.double()
            assert torch.equal(got, rounds * scale * want), (offset, rounds, int((got != rounds * scale * want).sum()))
            assert torch.equal(dst, dst.t()), (offset, rounds)
        if not ops._POISON:                              # (a poisoned workspace is refilled with NaN when it is handed out)
            ws = ops.workspace(1, gpu, "kfac_reduce")
            left = ws[:sums.numel() * 4].view(torch.float32).view(sums.shape).cpu().double()
            assert torch.equal(left, sums / L), offset


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", ["p8", "t16", "g_sum", "tbig_sum"])
def test_half_sources_exact_on_integer_inputs(gpu, name, dtype):
    """The same values held as bf16 / fp16 (exact in both): the pass upcasts, so the factor is the fp32 one bit for bit."""
    from curvature_amd import ops
    x, sums, L, args = exact_case(name)
    N, n = sums.shape
    want = (exact_gram(sums.t()) / L ** 2).to(gpu) * pow2_scale(N)
    dst = torch.full((n, n), float("nan"), device=gpu)
    ops.kfac_accumulate_reduce([ops.ReduceFactorJob(x.to(gpu, dtype), dst, scale=pow2_scale(N), first=True, **args)])
    assert torch.equal(dst.double(), want) and torch.equal(dst, dst.t())


def test_padding_only_taps_are_exact_zeros(gpu):
    """Case h: only the centre tap of a 3x3 window over a 1x1 image sees the image."""
    build("h")
    rows = last_rows("h").view(2, 3, 9)
    assert bool((rows[:, :, [0, 1, 2, 3, 5, 6, 7, 8]] == 0).all())
    assert torch.equal(rows[:, :, 4], case("h")[0].cpu().view(2, 3))                  # L = 1: the value itself


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", ["a", "t257", "ga", "tbig+"])
def test_half_sources_against_float64_of_the_upcast_values(gpu, name, dtype):
    x, rows, _ = case(name, dtype)
    assert x.dtype == dtype
    bias = name in ("a", "t257")
    got = build(name, bias, dtype).cpu()
    err_rows, err = rel_fro(last_rows(name, dtype), rows), rel_fro(got, gram(rows, bias, 1.0 / rows.shape[0]))
    print(f"reduce {name} {dtype}: rows {err_rows:.3e}, factor {err:.3e}")
    assert err_rows <= BAR and err <= BAR
    assert torch.equal(got, got.t())


@pytest.mark.parametrize("name", ["a", "t257", "i"])
def test_first_zero_adds(gpu, name):
    once = build(name)
    twice = build(name, first=False, dst=once.clone())
    _, rows, _ = case(name)
    assert rel_fro(twice, 2.0 * gram(rows, True, 1.0 / rows.shape[0])) <= BAR
    assert torch.equal(twice, twice.t())
    assert torch.equal(twice, once + once)                                            # one addition per entry


def test_factors_in_one_call_have_the_bits_of_each_alone(gpu):
    from curvature_amd import ops
    names = ["c", "a", "t257", "j", "tbig+", "i"]
    alone = [build(n) for n in names]
    together, jobs = [], []
    for n in names:
        x, rows, _ = case(n)
        dst = torch.full((rows.shape[1] + 1,) * 2, float("nan"), device=gpu)
        jobs.append(job(n, x, dst, True, 1.0 / rows.shape[0]))
        together.append(dst)
    ops.kfac_accumulate_reduce(jobs)
    for n, a, b in zip(names, alone, together):
        assert torch.equal(a, b), n
    # and run to run
    again = [torch.full_like(t, float("nan")) for t in together]
    for j, dst in zip(jobs, again):
        j.dst = dst
    ops.kfac_accumulate_reduce(jobs)
    for n, a, b in zip(names, together, again):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("dtype, offsets", [(torch.float32, (0, 1, 3)), (torch.bfloat16, (0, 1, 3, 5))], ids=["fp32", "bf16"])
def test_nan_fenced_source(gpu, dtype, offsets):
    """Case a inside a NaN-filled buffer at element offsets past a 16-byte boundary (the single-element head and tail of
    the staging): nothing outside the source is read, and the start does not change a bit."""
    x, rows, _ = case("a", dtype)
    want = gram(rows, True, 1.0 / rows.shape[0])
    plain = build("a", True, dtype)
    for offset in offsets:
        fence = torch.full((x.numel() + 4096 + 64,), float("nan"), dtype=dtype, device=gpu)
        start = 2048 + offset
        assert (fence.data_ptr() + 2048 * fence.element_size()) % 16 == 0
        xs = fence[start:start + x.numel()].view(x.shape)
        xs.copy_(x)
        got = build("a", True, dtype, src=xs)
        assert torch.isfinite(got).all(), offset
        assert rel_fro(got, want) <= BAR, offset
        assert torch.equal(got, plain), offset


def test_poisoned_scratch(gpu, monkeypatch):
    """Every scratch buffer NaN-filled when it is handed to the library (what CURV_DEBUG_POISON=1 does): the build reads
    only what the reduce pass wrote."""
    from curvature_amd import ops
    names = ("a", "i", "j", "t257", "tbig")
    plain = [build(n) for n in names]
    monkeypatch.setattr(ops, "_POISON", True)
    for n, want in zip(names, plain):
        got = build(n)
        assert torch.isfinite(got).all(), n
        assert torch.equal(got, want), n


def test_refusals_reach_python(gpu):
    from curvature_amd import ops
    x = case("a")[0]
    with pytest.raises(RuntimeError, match="kernel larger than the padded input"):
        ops.kfac_accumulate_reduce([ops.ReduceFactorJob(x, torch.empty(148, 148, device=gpu), (7, 7), (1, 1), (0, 0), True)])
    with pytest.raises(RuntimeError, match="destination"):
        ops.kfac_accumulate_reduce([ops.ReduceFactorJob(x, torch.empty(27, 27, device=gpu), (3, 3), (1, 1), (1, 1), True)])


# ------------------------------------------------------------------------------------------------ 2. model C
N_MODEL, CLASSES = 4, 5
ADD, MULTIPLY = 0.5, 2.0


def make_model(gpu, seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.ReLU(),
                               torch.nn.Conv2d(8, 8, 3, stride=2, padding=1, bias=False), torch.nn.Flatten(),
                               torch.nn.Linear(200, CLASSES)).to(gpu)


def selected(model):
    return [model[0], model[2], model[4]]


def backward(model, x, labels):
    model.zero_grad()
    F.cross_entropy(model(x), labels).backward()


def wb(weight_grad, bias_grad):
    """[W | b] of a layer from gradients shaped like its parameters."""
    flat = weight_grad.reshape(weight_grad.shape[0], -1)
    return flat if bias_grad is None else torch.cat([flat, bias_grad.reshape(-1, 1)], dim=1)


def float64_factors(layer, xin, g, approximation="reduce"):
    """(A, G) of KFAC.update on the records (xin, g) in float64, input_weight 1 and grad_scale 1."""
    xin, g = xin.detach().double().cpu(), g.detach().double().cpu()
    N = xin.shape[0]
    if isinstance(layer, torch.nn.Conv2d):
        cols = F.unfold(xin, layer.kernel_size, padding=layer.padding, stride=layer.stride)     # (N, dim, L)
        gs = g.reshape(N, g.shape[1], -1)                                                        # (N, m, L)
    else:
        cols, gs = xin.reshape(N, -1, xin.shape[-1]).transpose(1, 2), g.reshape(N, -1, g.shape[-1]).transpose(1, 2)
    L = cols.shape[2]
    if approximation == "reduce":
        X, gh, cols_n = cols.mean(2), gs.sum(2), N
    else:
        X, gh, cols_n = cols.transpose(1, 2).reshape(N * L, -1), gs.transpose(1, 2).reshape(N * L, -1), N * L
    if layer.bias is not None:
        X = torch.cat([X, torch.ones(X.shape[0], 1, dtype=X.dtype)], dim=1)
    return X.t() @ X / cols_n, gh.t() @ gh * N / (cols_n / N)


@functools.lru_cache(maxsize=None)
def setting():
    """The model on the GPU, a batch, and from a float64 CPU copy the per-sample Jacobians of every logit, each as [W | b]
    per layer.  Made once."""
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
    logits = ref(x.double().cpu())
    assert tuple(logits.shape) == (N_MODEL, CLASSES)
    jac = [[per_layer(torch.autograd.grad(logits[n, c], params, retain_graph=True)) for c in range(CLASSES)]
           for n in range(N_MODEL)]                       # jac[n][c][k]
    jac = [torch.stack([torch.stack([jac[n][c][k] for c in range(CLASSES)]) for n in range(N_MODEL)])
           for k in range(len(layers))]                   # per layer (N, classes, m, n)
    return model, x, labels, jac, logits.detach()


@functools.lru_cache(maxsize=None)
def estimator(approximation):
    """KFAC of that approximation after one update on the batch, inverted with (ADD, MULTIPLY)."""
    from curvature_amd.curvatures import KFAC
    model, x, labels = setting()[:3]
    est = KFAC(model, approximation=approximation) if approximation == "reduce" else KFAC(model)
    backward(model, x, labels)
    est.update(N_MODEL)
    est.invert(add=ADD, multiply=MULTIPLY)
    return est


def test_model_state_against_float64_and_expand(gpu):
    model = setting()[0]
    kfac, expand = estimator("reduce"), estimator("expand")
    assert kfac.approximation == "reduce"
    layers = selected(model)
    for k, layer in enumerate(layers):
        A_ref, G_ref = float64_factors(layer, *kfac.record[layer])
        A, G = kfac.state[layer]
        err_a, err_g = rel_fro(A, A_ref), rel_fro(G, G_ref)
        print(f"KFAC reduce state layer {k}: A {err_a:.3e}, G {err_g:.3e}")
        assert err_a <= BAR and err_g <= BAR
        assert torch.equal(A, A.t()) and torch.equal(G, G.t())
        assert A.shape == expand.state[layer][0].shape and G.shape == expand.state[layer][1].shape
    for layer in layers[:2]:                              # a build that silently took the expand route fails here
        gap = rel_fro(kfac.state[layer][0], expand.state[layer][0])
        print(f"reduce A against expand A: {gap:.3f}")
        assert gap > 0.1
    for a, b in zip(kfac.state[layers[2]], expand.state[layers[2]]):                  # L = 1: the very same build
        assert torch.equal(a, b)


def test_model_update_keywords(gpu):
    from curvature_amd.curvatures import KFAC
    model, x, labels = setting()[:3]
    kfac = KFAC(model, approximation="reduce")
    try:
        backward(model, x, labels)
        kfac.update(N_MODEL)
        once = {l: [t.clone() for t in kfac.state[l]] for l in selected(model)}
        kfac.update(N_MODEL)                                                          # two calls accumulate
        for l in selected(model):
            for a, b in zip(kfac.state[l], once[l]):
                assert rel_fro(a, 2.0 * b) <= BAR
        twice = {l: [t.clone() for t in kfac.state[l]] for l in selected(model)}
        kfac.update(N_MODEL, inputs=False)                                            # A untouched
        for l in selected(model):
            assert torch.equal(kfac.state[l][0], twice[l][0])
            assert rel_fro(kfac.state[l][1], 3.0 * once[l][1]) <= BAR
        kfac.restart_accumulation()
        kfac.update(N_MODEL, grad_scale=8.0, input_weight=3.0)                        # G / 64, A x 3
        for l in selected(model):
            assert rel_fro(kfac.state[l][0], 3.0 * once[l][0]) <= BAR
            assert rel_fro(kfac.state[l][1], once[l][1] / 64.0) <= BAR
        kfac._count_flops = True
        kfac.restart_accumulation()
        kfac.update(N_MODEL)
        assert kfac._last_flops > 0
        for l in selected(model):
            for a, b in zip(kfac.state[l], once[l]):
                assert torch.equal(a, b)
    finally:
        for hook in kfac.hooks:
            hook.remove()


def test_model_invert_and_sample(gpu):
    import oracle.curvature_oracle as o
    model = setting()[0]
    kfac = estimator("reduce")
    layers = selected(model)
    for layer in layers:
        for Fm, Lf in zip(kfac.state[layer], kfac.inv_state[layer]):
            n = Fm.shape[0]
            M = math.sqrt(MULTIPLY) * Fm.double() + math.sqrt(ADD) * torch.eye(n, device=gpu, dtype=torch.float64)
            M = (M + M.t()) / 2
            R = (Lf.double() @ Lf.double().t()) @ M - torch.eye(n, device=gpu, dtype=torch.float64)
            assert float(torch.linalg.norm(R)) / n ** 0.5 < identity_residual_bound(M)
    mean = {l: (l.weight.detach().clone(), None if l.bias is None else l.bias.detach().clone()) for l in layers}
    noise = {l: torch.randn(kfac.inv_state[l][0].size(0), kfac.inv_state[l][1].size(0), device=gpu) for l in layers}
    try:
        kfac.sample_and_replace(noise=noise)
        torch.cuda.synchronize()
        for layer in layers:
            la, lg = (t.double().cpu() for t in kfac.inv_state[layer])
            s = o.kfac_sample(la, lg, noise[layer].double().cpu())                    # (out, n) as [W | b]
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


def test_estimator_chain(gpu):
    """Diagonal -> KFAC(reduce) -> EFB -> INF construct, invert and sample finite values."""
    from curvature_amd.curvatures import EFB, INF, KFAC, Diagonal
    model = make_model(gpu, seed=5)
    gen = torch.Generator().manual_seed(6)
    x, labels = torch.randn(N_MODEL, 3, 10, 10, generator=gen).to(gpu), torch.tensor([3, 0, 2, 2], device=gpu)
    layers = selected(model)
    diag, kfac = Diagonal(model), KFAC(model, approximation="reduce")
    backward(model, x, labels)
    diag.update(N_MODEL)
    kfac.update(N_MODEL)
    efb = EFB(model, kfac.state)
    efb.update(N_MODEL)
    inf = INF(model, diag.state, kfac.state, efb.state, eigvecs=efb.eigvecs)
    inf.update(rank=20)
    for est in (diag, kfac, efb, inf):
        est.invert(add=ADD, multiply=MULTIPLY)
        est.sample_and_replace()
        torch.cuda.synchronize()
        for layer in layers:
            assert torch.isfinite(layer.weight).all() and (layer.bias is None or torch.isfinite(layer.bias).all())


def test_linearised_predictives_against_float64(gpu):
    """Sigma_n[c, c'] = sum_layers tr(P_c^T G^-1 P_c' A^-1) with the damped inverses of the FLOAT64 reduce factors."""
    from curvature_amd.evaluate import glm_predictive, glm_predictive_joint
    model, x, labels, jac, logits64 = setting()
    est = estimator("reduce")
    sigma = torch.zeros(N_MODEL, CLASSES, CLASSES, dtype=torch.float64)
    for k, layer in enumerate(selected(model)):
        inv = []
        for Fm in float64_factors(layer, *est.record[layer]):
            inv.append(torch.linalg.inv(math.sqrt(MULTIPLY) * Fm + math.sqrt(ADD) * torch.eye(Fm.shape[0], dtype=torch.float64)))
        P = jac[k]                                                                    # (N, classes, m, n)
        sigma += torch.einsum("ncij,ndij->ncd", inv[1] @ P @ inv[0], P)
    want_var = torch.diagonal(sigma, dim1=1, dim2=2)
    logits, variance, probs = glm_predictive(model, est, x)
    err = rel2(variance, want_var)
    print(f"reduce: variance {err:.3e}")
    assert err < TOL and rel2(logits, logits64) < TOL
    _, covariance, _ = glm_predictive_joint(model, est, x)
    err = rel2(covariance, sigma)
    print(f"reduce: covariance {err:.3e}")
    assert tuple(covariance.shape) == (N_MODEL, CLASSES, CLASSES) and err < TOL
    assert torch.equal(covariance, covariance.transpose(1, 2))


def test_graph_replay_equals_eager(gpu):
    """One capture of the KFAC(reduce) step (tests/test_dilated_gpu.py::test_graph_replay_equals_eager): replay and eager
    agree bit for bit, factors included."""
    from curvature_amd.curvatures import KFAC
    from curvature_amd.graph import KFACStepGraph

    def setup():
        model = make_model(gpu, seed=7)
        gen = torch.Generator().manual_seed(8)
        x, labels = torch.randn(N_MODEL, 3, 10, 10, generator=gen).to(gpu), torch.tensor([0, 1, 2, 3], device=gpu)
        kfac = KFAC(model, approximation="reduce")
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


# ------------------------------------------------------------------------------------------------ 3. model T
class TokenMean(torch.nn.Module):
    def forward(self, x):
        return x.mean(1)


def make_token_model(gpu):
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(6, 7), torch.nn.ReLU(), TokenMean(), torch.nn.Linear(7, 4)).to(gpu)


def token_batch(gpu):
    gen = torch.Generator().manual_seed(4)
    return torch.randn(3, 5, 6, generator=gen).to(gpu), torch.tensor([2, 0, 3], device=gpu)


def test_token_model_against_float64_and_expand(gpu):
    from curvature_amd.curvatures import KFAC
    model = make_token_model(gpu)
    x, labels = token_batch(gpu)
    kfac, expand = KFAC(model, approximation="reduce"), KFAC(model)
    backward(model, x, labels)
    kfac.update(3)
    expand.update(3)
    first, second = model[0], model[3]
    assert tuple(kfac.record[first][0].shape) == (3, 5, 6)
    for layer in (first, second):
        A_ref, G_ref = float64_factors(layer, *kfac.record[layer])
        err_a, err_g = rel_fro(kfac.state[layer][0], A_ref), rel_fro(kfac.state[layer][1], G_ref)
        print(f"token model {layer}: A {err_a:.3e}, G {err_g:.3e}")
        assert err_a <= BAR and err_g <= BAR
    # expand flattens the record to N L rows of one position: another matrix
    A_exp = float64_factors(first, *expand.record[first], approximation="expand")[0]
    assert rel_fro(expand.state[first][0], A_exp) <= BAR
    assert rel_fro(kfac.state[first][0], expand.state[first][0]) > 0.1
    for a, b in zip(kfac.state[second], expand.state[second]):
        assert torch.equal(a, b)


def test_token_model_under_autocast(gpu):
    from curvature_amd.curvatures import KFAC
    model = make_token_model(gpu)
    x, labels = token_batch(gpu)
    kfac = KFAC(model, approximation="reduce")
    model.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = F.cross_entropy(model(x), labels)
    loss.backward()
    kfac.update(3)
    assert kfac.record[model[0]][1].dtype == torch.bfloat16                           # the token-form G side reads bf16
    for layer in (model[0], model[3]):
        A_ref, G_ref = float64_factors(layer, *kfac.record[layer])
        err_a, err_g = rel_fro(kfac.state[layer][0], A_ref), rel_fro(kfac.state[layer][1], G_ref)
        print(f"token model under autocast {layer}: A {err_a:.3e}, G {err_g:.3e}")
        assert err_a <= BAR and err_g <= BAR


def test_two_middle_dimensions_through_factor_jobs(gpu):
    """(2, 3, 4, 9) records of a Linear(9, 5): N = 2 samples of 12 positions."""
    from curvature_amd import ops
    layer = torch.nn.Linear(9, 5).to(gpu)
    gen = torch.Generator().manual_seed(21)
    x, g = torch.randn(2, 3, 4, 9, generator=gen).to(gpu), torch.randn(2, 3, 4, 5, generator=gen).to(gpu)
    sides = ops.factor_jobs(layer, x, g, approximation="reduce")
    assert (sides.n, sides.m, sides.N, sides.L) == (10, 5, 2, 12)
    A, G = torch.full((10, 10), float("nan"), device=gpu), torch.full((5, 5), float("nan"), device=gpu)
    sides.a.dst, sides.a.scale, sides.a.first = A, 1.0 / 2, True
    sides.g.dst, sides.g.scale, sides.g.first = G, 2.0, True
    ops.kfac_accumulate_reduce([sides.a, sides.g])
    A_ref, G_ref = float64_factors(layer, x, g)
    assert rel_fro(A, A_ref) <= BAR and rel_fro(G, G_ref) <= BAR
