"""KFAC factors from bf16 / fp16 activations and gradients (torch.autocast) on the bf16 / fp16 MFMA (curv_kfac16_accumulate,
ABI 12): every geometry against fp64 of the upcast input and against today's fp32 build of the same tensors (`.float()`
copies), bit properties, the accumulation flags, autocast end to end, GradScaler, graph replay, a 2-rank shard and
sources that end right before NaN-filled memory."""
import functools
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_fro
from exact_inputs import assert_exact_range, conv_rows, exact_gram, flat_rows, nonzero_ints, pow2_scale, wide_ints

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float16]
TOL_FP64, TOL_FP32 = 1e-5, 1e-6


def ref_factors(layer, x, g):
    """fp64 (A, G) of the reference's formulas on the upcast tensors."""
    x, g = x.detach().double().cpu(), g.detach().double().cpu()
    if isinstance(layer, torch.nn.Conv2d):
        N, L = g.shape[0], g.shape[2] * g.shape[3]
        U = F.unfold(x, layer.kernel_size, padding=layer.padding, stride=layer.stride)
        U = U.permute(1, 0, 2).reshape(U.shape[1], -1)
        gs = g.permute(1, 0, 2, 3).reshape(g.shape[1], -1)
    else:
        U, gs = x.reshape(-1, x.shape[-1]).t(), g.reshape(-1, g.shape[-1]).t()
        N, L = U.shape[1], 1
    if layer.bias is not None:
        U = torch.cat([U, torch.ones(1, U.shape[1], dtype=U.dtype)])
    return U @ U.t() / (N * L), gs @ gs.t() * N / L


def fp32_path(model, kfac, **kw):
    """Today's update() on .float() copies of the recorded tensors."""
    from curvature_amd.curvatures import KFAC
    ref = KFAC(model)
    ref.record = {l: [None if t is None else t.detach().float() for t in v] for l, v in kfac.record.items()}
    ref.update(**kw)
    return ref


def _single(gpu, kind, dtype, seed=0):
    """One-layer model with half-precision records: kind = ("linear", N, C, out, bias[, T]) or
    ("conv", cin, cout, k, stride, padding, bias, N, H[, W])."""
    from curvature_amd.curvatures import KFAC
    torch.manual_seed(seed)
    if kind[0] == "linear":
        _, N, C, out, bias, *T = kind
        layer = torch.nn.Linear(C, out, bias=bias)
        shape, gshape = (N, *T, C), (N, *T, out)
    else:
        _, cin, cout, k, s, p, bias, N, H, *W = kind
        W = W[0] if W else H
        layer = torch.nn.Conv2d(cin, cout, k, stride=s, padding=p, bias=bias)
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        shape, gshape = (N, cin, H, W), (N, cout, Ho, Wo)
    model = torch.nn.Sequential(layer).to(gpu)
    x = torch.randn(shape, device=gpu).to(dtype)
    g = torch.randn(gshape, device=gpu).to(dtype)
    kfac = KFAC(model)
    kfac.record[layer] = [x, g]
    return model, layer, kfac, x, g


CASES = [
    ("linear", 64, 5, 7, True),
    ("linear", 4, 129, 33, True, 7),                    # (N, T, C)
    ("linear", 100000, 5, 3, True),                     # K = 10^5
    ("conv", 64, 32, 1, 1, 0, False, 4, 14),            # 1x1 s1
    ("conv", 64, 32, 1, 2, 0, True, 4, 14),             # 1x1 s2
    ("conv", 5, 16, 3, 1, 1, True, 3, 7),               # 3x3 s1 p1, 7x7 rows
    ("conv", 129, 8, 3, 2, 1, False, 2, 14),            # 3x3 s2 p1, dim 1161
    ("conv", 3, 64, 7, 2, 3, False, 2, 32),             # stem 7x7 s2 p3, C = 3
    ("conv", 5, 8, 5, 1, 0, True, 3, 14),               # 5x5 p0
    ("conv", 64, 129, 3, 1, 1, False, 2, 7),            # G dim 129
    ("conv", 256, 257, 1, 1, 0, True, 2, 7),            # A and G dim 257
    ("conv", 3, 5, 3, 1, 1, True, 2, 14, 13),           # odd width
    ("conv", 8, 16, 3, 1, 1, True, 32, 56),             # K = 100 352
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=[str(i) for i in range(len(CASES))])
def test_geometry_against_fp64_and_fp32_path(gpu, case, dtype):
    model, layer, kfac, x, g = _single(gpu, case, dtype)
    kfac.update(batch_size=x.shape[0])
    ref = fp32_path(model, kfac, batch_size=x.shape[0])
    torch.cuda.synchronize()
    R = ref_factors(layer, x, g)
    for side in (0, 1):
        got, want32 = kfac.state[layer][side], ref.state[layer][side]
        e64, e32 = rel_fro(got, R[side]), rel_fro(got, want32)
        print(f"{case} {dtype} side {side}: rel_fro vs fp64 {e64:.2e}, vs fp32 path {e32:.2e}")
        assert e64 < TOL_FP64 and e32 < TOL_FP32
        assert torch.equal(got, got.t())


def _fenced_copy(t, gpu, pad=4096):
    """A copy of `t` on the GPU that starts right after and ends right before NaN-filled memory."""
    buf = torch.full((pad + t.numel() + pad,), float("nan"), device=gpu, dtype=t.dtype)
    buf[pad:pad + t.numel()] = t.reshape(-1).to(gpu)
    return buf[pad:pad + t.numel()].view(t.shape)


@functools.lru_cache(maxsize=None)
def _exact_case(case, dtype):
    """(layer, x, g, A_exact, G_exact, scale_A, scale_G) of a case with integer-valued half-precision records
    (tests/exact_inputs.py): the unscaled integer Grams in float64, formed on the GPU once per case."""
    gpu = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(99)
    if case[0] == "linear":
        _, N, C, out, bias, *T = case
        layer = torch.nn.Linear(C, out, bias=bias)
        x, g = nonzero_ints((N, *T, C), gen, dtype), nonzero_ints((N, *T, out), gen, dtype)
        rows_a, rows_g = x.to(gpu).double().reshape(-1, C).t(), g.to(gpu).double().reshape(-1, out).t()
    else:
        _, cin, cout, k, s, p, bias, N, H, *W = case
        W = W[0] if W else H
        layer = torch.nn.Conv2d(cin, cout, k, stride=s, padding=p, bias=bias)
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        x, g = nonzero_ints((N, cin, H, W), gen, dtype), nonzero_ints((N, cout, Ho, Wo), gen, dtype)
        rows_a, rows_g = conv_rows(x.to(gpu), k, s, p), flat_rows(g.to(gpu))
    terms = rows_a.shape[1]
    assert rows_g.shape[1] == terms
    assert_exact_range(3, terms, rounds=2)
    scale = pow2_scale(terms)
    return layer, x, g, exact_gram(rows_a, ones_row=bias), exact_gram(rows_g), scale, 4.0 * scale


def _assert_exact(dst, want, what):
    got = dst.double()
    assert torch.equal(got, want), (what, int((got != want).sum()), float((got - want).abs().max()))
    assert torch.equal(dst, dst.t()), what


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=[str(i) for i in range(len(CASES))])
def test_geometry_exact_on_integer_inputs(gpu, case, dtype):
    """Every geometry again, bit for bit: records uniform in {+-1, +-2, +-3} (exact in bf16 and fp16, none zero) and
    power-of-two scales, through the jobs `ops.factor_jobs` makes for the layer.  Every product and partial sum is an
    integer below 2^24, so the bf16 / fp16 MFMA with fp32 accumulation and the slice reduce have one right answer in any
    summation order: ``scale * exact`` after a first call and twice that after an accumulating one (DESIGN.md section
    5).  fp16 also with the gradients scaled by 2^12 and the G scale divided by 2^24, what ``grad_scale = 2**12`` does."""
    from curvature_amd import ops
    layer, x, g, A_exact, G_exact, scale_a, scale_g = _exact_case(case, dtype)
    sides = ops.factor_jobs(layer, _fenced_copy(x, gpu), _fenced_copy(g, gpu))
    assert type(sides.a) is ops.HalfFactorJob and type(sides.g) is ops.HalfFactorJob
    A = torch.full((sides.n, sides.n), float("nan"), device=gpu)
    G = torch.full((sides.m, sides.m), float("nan"), device=gpu)
    sides.a.dst, sides.a.scale, sides.a.first = A, scale_a, True
    sides.g.dst, sides.g.scale, sides.g.first = G, scale_g, True
    ops.kfac_accumulate_half([sides.a, sides.g])
    torch.cuda.synchronize()
    _assert_exact(A, scale_a * A_exact, "A")
    _assert_exact(G, scale_g * G_exact, "G")
    sides.a.first = sides.g.first = False
    ops.kfac_accumulate_half([sides.a, sides.g])
    torch.cuda.synchronize()
    _assert_exact(A, 2 * scale_a * A_exact, "A accumulated")
    _assert_exact(G, 2 * scale_g * G_exact, "G accumulated")
    if dtype == torch.float16:
        scaled = ops.factor_jobs(layer, None, _fenced_copy(g * 2 ** 12, gpu)).g
        G2 = torch.full_like(G, float("nan"))
        scaled.dst, scaled.scale, scaled.first = G2, scale_g / 2.0 ** 24, True
        ops.kfac_accumulate_half([scaled])
        torch.cuda.synchronize()
        _assert_exact(G2, scale_g * G_exact, "G from gradients scaled by 2^12")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape, kernel", [((128, 40), 1), ((2, 40, 8, 8), 1), ((2, 5, 8, 8), 3)],
                         ids=["linear", "conv1x1", "conv3x3"])
def test_accumulation_is_fp32(gpu, shape, kernel, dtype):
    """Odd 8-bit integers are exact in bf16 and fp16; their products have 16 bits and the 128 terms of an entry sum to less
    than 2^24.  The factor is the exact Gram only if the MFMA accumulates in fp32 and the slices are summed in fp32: a
    half-precision accumulator or a narrowed partial sum holds another number (tests/test_exact_inputs_cpu.py)."""
    from curvature_amd import ops
    gen = torch.Generator().manual_seed(8)
    x = wide_ints(shape, gen, 8, dtype)
    pad = (kernel - 1) // 2
    rows = flat_rows(x.to(gpu)) if kernel == 1 else conv_rows(x.to(gpu), kernel, 1, pad)
    assert rows.shape[1] == 128
    assert_exact_range(255, 128, rounds=2)
    want = exact_gram(rows)
    n = rows.shape[0]
    A = torch.full((n, n), float("nan"), device=gpu)
    job = ops.HalfFactorJob(_fenced_copy(x, gpu), A, (kernel, kernel), (1, 1), (pad, pad), False, 0.5, True)
    ops.kfac_accumulate_half([job])
    torch.cuda.synchronize()
    _assert_exact(A, 0.5 * want, "first")
    job.first = False
    ops.kfac_accumulate_half([job])
    torch.cuda.synchronize()
    _assert_exact(A, want, "accumulated")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_symmetric_and_reproducible(gpu, dtype):
    model, layer, kfac, x, g = _single(gpu, ("conv", 64, 129, 3, 2, 1, True, 3, 15), dtype)
    kfac.update(batch_size=3)
    once = [t.clone() for t in kfac.state[layer]]
    kfac.restart_accumulation()
    kfac.update(batch_size=3)
    for a, b in zip(kfac.state[layer], once):
        assert torch.equal(a, a.t())
        assert torch.equal(a, b)


def _autocast_run(gpu, name, N=8, size=64, dtype=torch.bfloat16, seed=3):
    from curvature_amd import models
    from curvature_amd.curvatures import KFAC
    torch.manual_seed(seed)
    model = getattr(models, name)(num_classes=10).to(gpu)
    x = torch.randn(N, 3, size, size, device=gpu)
    kfac = KFAC(model)
    with torch.autocast("cuda", dtype=dtype):
        loss = F.cross_entropy(model(x), torch.randint(0, 10, (N,), device=gpu))
    model.zero_grad()
    loss.backward()
    return model, kfac


def test_bits_alone_equal_bits_in_a_model(gpu):
    """A half-precision factor's bits do not depend on the other factors of the call."""
    from curvature_amd.curvatures import KFAC
    model, kfac = _autocast_run(gpu, "resnet18", N=2)
    kfac.update(batch_size=2)
    checked = 0
    for layer, (x, g) in kfac.record.items():
        if x.dtype == torch.float32 and g.dtype == torch.float32:
            continue
        if isinstance(layer, torch.nn.Conv2d):
            twin = torch.nn.Conv2d(layer.in_channels, layer.out_channels, layer.kernel_size, layer.stride, layer.padding,
                                   bias=layer.bias is not None)
        else:
            twin = torch.nn.Linear(layer.in_features, layer.out_features, bias=layer.bias is not None)
        alone = KFAC(torch.nn.Sequential(twin).to(gpu))
        part = next(iter(alone.record))
        alone.record[part] = [x, g]
        alone.update(batch_size=2)
        for side, t in enumerate((x, g)):
            if t.dtype != torch.float32:
                assert torch.equal(alone.state[part][side], kfac.state[layer][side])
                checked += 1
    assert checked >= 30


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_accumulation_flags(gpu, dtype):
    model, layer, kfac, x, g = _single(gpu, ("conv", 16, 24, 3, 1, 1, True, 2, 9), dtype)
    kfac.update(batch_size=2)
    once = [t.clone() for t in kfac.state[layer]]
    kfac.update(batch_size=2)
    for a, b in zip(kfac.state[layer], once):
        assert rel_fro(a, 2 * b) < 1e-6 and torch.equal(a, a.t())
    kfac.restart_accumulation()
    kfac.update(batch_size=2)
    for a, b in zip(kfac.state[layer], once):
        assert torch.equal(a, b)
    # A side once with input_weight = 3, G side three times: 3 x (A, G)
    est = _single(gpu, ("conv", 16, 24, 3, 1, 1, True, 2, 9), dtype)[2]
    est.record[next(iter(est.record))] = [x, g]
    est.update(batch_size=2, grads=False, input_weight=3.0)
    for _ in range(3):
        est.update(batch_size=2, inputs=False)
    A, G = next(iter(est.state.values()))
    assert rel_fro(A, 3 * once[0]) < 1e-6 and rel_fro(G, 3 * once[1]) < 1e-6


@pytest.mark.parametrize("name", ["resnet18", "mobilenet_v2"])
def test_autocast_end_to_end(gpu, name):
    """bf16 autocast forward + backward: update() takes the half-precision records (today: RuntimeError), every factor
    equals the fp32 build of the upcast records, and invert + sample_and_replace give finite weights."""
    model, kfac = _autocast_run(gpu, name)
    dtypes = [t.dtype for pair in kfac.record.values() for t in pair]
    assert torch.bfloat16 in dtypes and torch.float32 in dtypes        # the stem's A side stays fp32
    kfac.update(batch_size=8)
    ref = fp32_path(model, kfac, batch_size=8)
    torch.cuda.synchronize()
    worst = 0.0
    for layer in kfac.state:
        for side in (0, 1):
            worst = max(worst, rel_fro(kfac.state[layer][side], ref.state[layer][side]))
    print(f"{name}: worst rel_fro against the fp32 path {worst:.2e}")
    assert worst < TOL_FP32
    kfac.invert(0.5, 1)
    kfac.sample_and_replace()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_compute_factors_autocast_equals_manual_loop(gpu):
    from curvature_amd.curvatures import KFAC
    from curvature_amd.factors import compute_factors

    def setup():
        torch.manual_seed(5)
        model = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten(),
                                    torch.nn.Linear(8 * 8 * 8, 10)).to(gpu)
        data = [(torch.randn(4, 3, 8, 8, device=gpu), None) for _ in range(2)]
        return model, data

    labels = [torch.randint(0, 10, (4,), device=gpu) for _ in range(2)]
    sampler = lambda logits, b, s: labels[b]                            # noqa: E731
    model, data = setup()
    est = compute_factors(None, model, data, estimator="kfac", samples=1, label_sampler=sampler,
                          autocast=torch.bfloat16)
    assert any(t.dtype == torch.bfloat16 for pair in est.record.values() for t in pair)
    model2, data2 = setup()
    manual = KFAC(model2)
    for b, (images, _) in enumerate(data2):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = model2(images)
            loss = torch.nn.CrossEntropyLoss()(logits, labels[b])
        model2.zero_grad()
        loss.backward()
        manual.update(images.size(0))
    torch.cuda.synchronize()
    for l1, l2 in zip(est.state, manual.state):
        for a, b in zip(est.state[l1], manual.state[l2]):
            assert rel_fro(a, b) < 1e-6


def test_fp16_grad_scale(gpu):
    """G of gradients scaled by 2^12 with grad_scale = 2^12 equals the unscaled build."""
    model, layer, kfac, x, g = _single(gpu, ("conv", 16, 24, 3, 1, 1, True, 2, 9), torch.float16)
    kfac.update(batch_size=2)
    scaled = _single(gpu, ("conv", 16, 24, 3, 1, 1, True, 2, 9), torch.float16)[2]
    scaled.record[next(iter(scaled.record))] = [x, g * 2 ** 12]
    scaled.update(batch_size=2, grad_scale=2.0 ** 12)
    A, G = next(iter(scaled.state.values()))
    assert rel_fro(G, kfac.state[layer][1]) < 1e-6
    assert torch.equal(A, kfac.state[layer][0])


def test_graph_replay_equals_eager(gpu):
    from curvature_amd.curvatures import KFAC
    from curvature_amd.graph import KFACStepGraph

    def setup():
        torch.manual_seed(4)
        model = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3, padding=1), torch.nn.ReLU(),
                                    torch.nn.Conv2d(16, 16, 3, padding=1, groups=4), torch.nn.ReLU(),
                                    torch.nn.Conv2d(16, 24, 3, stride=2, padding=1), torch.nn.ReLU(),
                                    torch.nn.Flatten(), torch.nn.Linear(24 * 25, 10)).to(gpu)
        x = torch.randn(2, 8, 10, 10, device=gpu)
        kfac = KFAC(model)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model(x).float().square().sum()
        loss.backward()
        kfac.noise_seed = 7
        return model, kfac

    model_e, eager = setup()
    assert any(t.dtype == torch.bfloat16 for pair in eager.record.values() for t in pair)
    weights = []
    for _ in range(3):
        eager.update(2)
        eager.invert(0.5, 1.0)
        eager.sample_and_replace()
        weights.append([p.detach().clone() for p in model_e.parameters()])
    model_g, kfac = setup()
    graph = KFACStepGraph(kfac, add=0.5, multiply=1.0, batch_size=2, warmup=2)
    for step in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(model_g.parameters(), weights[step]):
            assert torch.equal(a.detach(), b)
    graph.check()


def test_two_rank_shard_same_bits(gpu):
    """Each rank of a 2-rank layer shard of a bf16-autocast model builds and inverts its own layers: the same bits as the
    unsharded run."""
    from curvature_amd import sharding
    from curvature_amd.curvatures import KFAC
    model, full = _autocast_run(gpu, "resnet18", N=2, size=32)
    layers = full._layers()
    shapes = {l: (tuple(full.record[l][0].shape), tuple(full.record[l][1].shape)) for l in layers}
    dims = sharding.layer_dims(layers, shapes)
    full.update(batch_size=2)
    full.invert(add=0.5, multiply=1.0)
    owner = sharding.partition_layers(dims, 2)
    assert set(owner) == {0, 1}
    seen = set()
    for rank in range(2):
        est = KFAC(model, shard=sharding.Shard(owner, rank, 2))
        est.record = full.record
        est.update(batch_size=2)
        est.invert(add=0.5, multiply=1.0)
        for layer in est.state:
            seen.add(layer)
            assert all(torch.equal(a, b) for a, b in zip(est.state[layer], full.state[layer]))
            assert all(torch.equal(a, b) for a, b in zip(est.inv_state[layer], full.inv_state[layer]))
    assert seen == set(full.state)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_source_at_the_edge_of_memory(gpu, dtype):
    """Sources are views that end right before (and start right after) NaN-filled memory: nothing outside is read."""
    from curvature_amd.curvatures import KFAC
    pad = 4096

    def fenced(shape):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((pad + n + pad,), float("nan"), device=gpu, dtype=dtype)
        buf[pad:pad + n] = torch.randn(n, device=gpu).to(dtype)
        return buf[pad:pad + n].view(shape)

    for layer, xs, gs in ((torch.nn.Conv2d(5, 7, 3, padding=1), (2, 5, 9, 7), (2, 7, 9, 7)),
                          (torch.nn.Conv2d(3, 4, 7, stride=2, padding=3), (1, 3, 13, 13), (1, 4, 7, 7)),
                          (torch.nn.Linear(13, 5), (3, 13), (3, 5))):
        torch.manual_seed(2)
        layer = layer.to(gpu)
        x, g = fenced(xs), fenced(gs)
        kfac = KFAC(torch.nn.Sequential(layer))
        kfac.record[layer] = [x, g]
        kfac.update(batch_size=xs[0])
        torch.cuda.synchronize()
        A, G = kfac.state[layer]
        assert torch.isfinite(A).all() and torch.isfinite(G).all()
        RA, RG = ref_factors(layer, x, g)
        assert rel_fro(A, RA) < TOL_FP64 and rel_fro(G, RG) < TOL_FP64


def test_other_dtypes_still_raise(gpu):
    model, layer, kfac, x, g = _single(gpu, ("conv", 4, 4, 3, 1, 1, True, 2, 5), torch.bfloat16)
    kfac.record[layer] = [x.double(), g.float()]
    with pytest.raises(RuntimeError, match="float64"):
        kfac.update(batch_size=2)


def test_poisoned_scratch(gpu):
    """This file again with CURV_DEBUG_POISON=1: no kernel reads scratch it has not written."""
    env = dict(os.environ, CURV_DEBUG_POISON="1")
    proc = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                           "tests/test_half_factor_gpu.py", "-k", "not poisoned and not two_rank"],
                          cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert proc.returncode == 0, proc.stdout[-3000:]
    passed = re.search(r"(\d+) passed", proc.stdout)
    assert passed and int(passed.group(1)) >= 30, proc.stdout[-3000:]
    assert "skipped" not in proc.stdout and "deselected" in proc.stdout, proc.stdout[-3000:]
