"""KFAC for grouped and depthwise convolutions: one Kronecker pair per group (curv_kfac_group_accumulate), checked against an
fp64 F.unfold of each channel slice, against G ordinary layers run through today's KFAC, and through every sampler, the
graph capture, save / load and a 2-rank layer shard."""
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_fro
from exact_inputs import assert_exact_range, conv_rows, exact_gram, flat_rows, nonzero_ints, pow2_scale

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5


def ref_factors(layer, x, g):
    """fp64 stacked (A, G) of a grouped Conv2d: the reference's formulas on each channel slice."""
    G = layer.groups
    cg, mg = layer.in_channels // G, layer.out_channels // G
    x, g = x.detach().double().cpu(), g.detach().double().cpu()
    N, L = g.shape[0], g.shape[2] * g.shape[3]
    As, Gs = [], []
    for k in range(G):
        U = F.unfold(x[:, k * cg:(k + 1) * cg], layer.kernel_size, padding=layer.padding, stride=layer.stride)
        U = U.permute(1, 0, 2).reshape(U.shape[1], -1)
        if layer.bias is not None:
            U = torch.cat([U, torch.ones(1, U.shape[1], dtype=U.dtype)])
        As.append(U @ U.t() / (N * L))
        gs = g[:, k * mg:(k + 1) * mg].permute(1, 0, 2, 3).reshape(mg, -1)
        Gs.append(gs @ gs.t() * N / L)
    return torch.stack(As), torch.stack(Gs)


def _layer_and_record(gpu, cin, cout, k, stride, padding, groups, bias, N, H, W=None, seed=0):
    from curvature_amd.curvatures import KFAC
    torch.manual_seed(seed)
    layer = torch.nn.Conv2d(cin, cout, k, stride=stride, padding=padding, groups=groups, bias=bias)
    model = torch.nn.Sequential(layer).to(gpu)
    x = torch.randn(N, cin, H, W or H, device=gpu)
    out = layer(x)
    g = torch.randn_like(out)
    kfac = KFAC(model)
    kfac.record[layer] = [x, g]
    return model, layer, kfac, x, g


# (cin, cout, kernel, stride, padding, groups, bias, N, H[, W])
CASES = [
    (16, 16, 3, 1, 1, 16, False, 4, 12),            # depthwise 3x3
    (16, 16, 3, 1, 1, 16, True, 4, 12),
    (24, 24, 3, 2, 1, 24, False, 3, 14),            # depthwise stride 2
    (24, 24, 3, 2, 1, 24, True, 2, 13),
    (8, 8, 5, 1, 2, 8, False, 2, 11),               # EfficientNet 5x5
    (8, 16, 3, 1, 1, 8, True, 2, 9),                # channel multiplier 2
    (6, 6, (1, 3), 1, (0, 1), 3, True, 2, 10),      # non-square kernel
    (32, 32, 3, 1, 1, 8, False, 2, 9),              # ResNeXt cg = 4
    (64, 64, 3, 2, 1, 8, True, 2, 14),              # cg = 8, stride 2
    (128, 128, 3, 1, 1, 4, False, 2, 7),            # cg = 32 (n_g = 288)
    (66, 66, 1, 1, 0, 2, False, 2, 7),              # n_g = 33 / 34
    (130, 130, 1, 1, 0, 2, True, 1, 7),             # n_g = 65 + bias, m_g = 65
    (258, 258, 1, 2, 0, 2, False, 2, 13),           # n_g = 129, stride 2
    (12, 12, 3, 2, 1, 12, True, 1, 7),              # N = 1, W % 4 != 0
    (4, 8, (3, 2), (2, 1), (1, 0), 2, True, 2, 9, 6),
    # more than one slice of 16 384 output pixels, the slice edges mid-image (K not a multiple of the slice)
    (8, 8, 3, 1, 1, 8, False, 2, 96, 97),           # depthwise, K = 18 624
    (8, 8, 3, 1, 1, 8, True, 5, 80, 81),            # depthwise + bias, K = 32 400: 2 slices
    (24, 24, 3, 1, 1, 3, True, 3, 80),              # cg = 8 with bias (wide), K = 19 200
    (8, 16, 1, 1, 0, 8, True, 3, 90, 70),           # 1x1, multiplier 2, K = 18 900
]


@pytest.mark.parametrize("case", CASES)
def test_factors_match_fp64_unfold(gpu, case):
    model, layer, kfac, x, g = _layer_and_record(gpu, *case)
    kfac.update(batch_size=x.shape[0])
    torch.cuda.synchronize()
    A, G = kfac.state[layer]
    RA, RG = ref_factors(layer, x, g)
    assert A.shape == RA.shape and G.shape == RG.shape and A.is_contiguous() and G.is_contiguous()
    assert rel_fro(A, RA) < TOL and rel_fro(G, RG) < TOL
    for k in range(A.shape[0]):                      # every group, not only the norm over all
        assert rel_fro(A[k], RA[k]) < TOL and rel_fro(G[k], RG[k]) < TOL
        assert torch.equal(A[k], A[k].t()) and torch.equal(G[k], G[k].t())


@functools.lru_cache(maxsize=None)
def _exact_case(case):
    """(layer, x, g, stacked A_exact, stacked G_exact, scale_A, scale_G) of a case with integer-valued records
    (tests/exact_inputs.py): the unscaled integer Gram of ``F.unfold`` of each channel slice in float64, on the GPU."""
    cin, cout, k, stride, padding, groups, bias, N, H, *W = case
    gpu = torch.device("cuda:0")
    layer = torch.nn.Conv2d(cin, cout, k, stride=stride, padding=padding, groups=groups, bias=bias)
    gen = torch.Generator().manual_seed(17)
    x = nonzero_ints((N, cin, H, W[0] if W else H), gen)
    with torch.no_grad():
        out_shape = layer(x).shape
    g = nonzero_ints(out_shape, gen)
    terms = N * out_shape[2] * out_shape[3]
    assert_exact_range(3, terms, rounds=2)
    cg, mg = cin // groups, cout // groups
    xs, gs = x.to(gpu), g.to(gpu)
    As = [exact_gram(conv_rows(xs[:, q * cg:(q + 1) * cg], layer.kernel_size, layer.stride, layer.padding), ones_row=bias)
          for q in range(groups)]
    Gs = [exact_gram(flat_rows(gs[:, q * mg:(q + 1) * mg])) for q in range(groups)]
    scale = pow2_scale(terms)
    return layer, x, g, torch.stack(As), torch.stack(Gs), scale, 4.0 * scale


def _fenced_copy(t, gpu, pad=4096):
    """A copy of `t` on the GPU that starts right after and ends right before NaN-filled memory."""
    buf = torch.full((pad + t.numel() + pad,), float("nan"), device=gpu)
    buf[pad:pad + t.numel()] = t.reshape(-1).to(gpu)
    return buf[pad:pad + t.numel()].view(t.shape)


def _assert_exact(dst, want, what):
    got = dst.double()
    assert torch.equal(got, want), (what, int((got != want).sum()), float((got - want).abs().max()))
    assert torch.equal(dst, dst.transpose(1, 2)), what


@pytest.mark.parametrize("case", CASES)
def test_factors_exact_on_integer_inputs(gpu, case):
    """Every case again, bit for bit: records uniform in {+-1, +-2, +-3} (none zero, so every element moves the result)
    and power-of-two scales, through the `GroupFactorJob`s `ops.factor_jobs` makes for the layer.  Every product and
    partial sum is an integer below 2^24, so the Gram kernels, the slice reduce, the patch sums of the bias row and the
    pixel count of its corner have one right answer in any summation order: ``scale * exact`` in every group after a
    first call, twice that after an accumulating one."""
    from curvature_amd import ops
    layer, x, g, A_exact, G_exact, scale_a, scale_g = _exact_case(case)
    sides = ops.factor_jobs(layer, _fenced_copy(x, gpu), _fenced_copy(g, gpu))
    assert type(sides.a) is ops.GroupFactorJob and type(sides.g) is ops.GroupFactorJob
    A = torch.full((sides.groups, sides.n, sides.n), float("nan"), device=gpu)
    G = torch.full((sides.groups, sides.m, sides.m), float("nan"), device=gpu)
    sides.a.dst, sides.a.scale, sides.a.first = A, scale_a, True
    sides.g.dst, sides.g.scale, sides.g.first = G, scale_g, True
    ops.kfac_accumulate_groups([sides.a, sides.g])
    torch.cuda.synchronize()
    _assert_exact(A, scale_a * A_exact, "A")
    _assert_exact(G, scale_g * G_exact, "G")
    sides.a.first = sides.g.first = False
    ops.kfac_accumulate_groups([sides.a, sides.g])
    torch.cuda.synchronize()
    _assert_exact(A, 2 * scale_a * A_exact, "A accumulated")
    _assert_exact(G, 2 * scale_g * G_exact, "G accumulated")


def test_split_equivalence(gpu):
    """A grouped layer gives the factors of G ordinary layers built from its weight slices and fed its channel slices."""
    from curvature_amd.curvatures import KFAC
    model, layer, kfac, x, g = _layer_and_record(gpu, 12, 24, 3, 1, 1, 4, True, 3, 10)
    kfac.update(batch_size=3)
    cg, mg = 3, 6
    for k in range(4):
        part = torch.nn.Conv2d(cg, mg, 3, padding=1).to(gpu)
        est = KFAC(torch.nn.Sequential(part))
        est.record[part] = [x[:, k * cg:(k + 1) * cg].contiguous(), g[:, k * mg:(k + 1) * mg].contiguous()]
        est.update(batch_size=3)
        torch.cuda.synchronize()
        assert rel_fro(kfac.state[layer][0][k], est.state[part][0]) < TOL
        assert rel_fro(kfac.state[layer][1][k], est.state[part][1]) < TOL


def test_accumulation_flags(gpu):
    model, layer, kfac, x, g = _layer_and_record(gpu, 16, 16, 3, 1, 1, 16, True, 2, 8)
    kfac.update(batch_size=2)
    once = [t.clone() for t in kfac.state[layer]]
    kfac.update(batch_size=2)
    for a, b in zip(kfac.state[layer], once):
        assert rel_fro(a, 2 * b) < 1e-6
    kfac.restart_accumulation()
    kfac.update(batch_size=2)
    for a, b in zip(kfac.state[layer], once):
        assert torch.equal(a, b)
    # A side once with input_weight = 3, G side three times: 3 x (A, G)
    est = _layer_and_record(gpu, 16, 16, 3, 1, 1, 16, True, 2, 8)[2]
    est.record[next(iter(est.record))] = [x, g]
    est.update(batch_size=2, grads=False, input_weight=3.0)
    for _ in range(3):
        est.update(batch_size=2, inputs=False)
    A, G = next(iter(est.state.values()))
    assert rel_fro(A, 3 * once[0]) < 1e-6 and rel_fro(G, 3 * once[1]) < 1e-6


@pytest.mark.parametrize("name", ["mobilenet_v2", "resnext50_32x4d"])
def test_determinism_alone_and_in_a_model(gpu, name):
    from curvature_amd import models
    from curvature_amd.curvatures import KFAC
    torch.manual_seed(1)
    model = getattr(models, name)(num_classes=10).to(gpu)
    x = torch.randn(2, 3, 64, 64, device=gpu)
    kfac = KFAC(model)
    loss = model(x).square().sum()
    loss.backward()
    kfac.update(batch_size=2)
    first = {l: [t.clone() for t in v] for l, v in kfac.state.items()}
    kfac.restart_accumulation()
    kfac.update(batch_size=2)
    for l, v in kfac.state.items():
        assert all(torch.equal(a, b) for a, b in zip(v, first[l]))
    grouped = [l for l in kfac.state if isinstance(l, torch.nn.Conv2d) and l.groups > 1]
    for layer in grouped[:4] + grouped[-2:]:
        alone = KFAC(torch.nn.Sequential(torch.nn.Conv2d(layer.in_channels, layer.out_channels, layer.kernel_size,
                                                         layer.stride, layer.padding, groups=layer.groups,
                                                         bias=False)).to(gpu))
        part = next(iter(alone.record))
        alone.record[part] = list(kfac.record[layer])
        alone.update(batch_size=2)
        assert all(torch.equal(a, b) for a, b in zip(alone.state[part], first[layer]))


def test_source_at_the_edge_of_memory(gpu):
    """The input is a view that ends right before NaN-filled memory: nothing past it is read."""
    from curvature_amd.curvatures import KFAC
    pad = 4096
    for cin, groups in ((16, 16), (64, 2)):
        torch.manual_seed(2)
        layer = torch.nn.Conv2d(cin, cin, 3, padding=1, groups=groups).to(gpu)
        shape = (2, cin, 9, 7)
        n = 2 * cin * 9 * 7
        # NaN on both sides of each source: a read before the start (a negative padding offset) or past the end shows
        buf = torch.full((pad + n + pad,), float("nan"), device=gpu)
        buf[pad:pad + n] = torch.randn(n, device=gpu)
        x = buf[pad:pad + n].view(shape)
        gbuf = torch.full((pad + n + pad,), float("nan"), device=gpu)
        gbuf[pad:pad + n] = torch.randn(n, device=gpu)
        g = gbuf[pad:pad + n].view(shape)
        kfac = KFAC(torch.nn.Sequential(layer))
        kfac.record[layer] = [x, g]
        kfac.update(batch_size=2)
        torch.cuda.synchronize()
        A, G = kfac.state[layer]
        assert torch.isfinite(A).all() and torch.isfinite(G).all()
        RA, RG = ref_factors(layer, x, g)
        assert rel_fro(A, RA) < TOL and rel_fro(G, RG) < TOL


def _inverted(gpu, bias=True):
    model, layer, kfac, x, g = _layer_and_record(gpu, 12, 24, 3, 1, 1, 4, bias, 3, 8)
    kfac.update(batch_size=3)
    kfac.invert(add=0.3, multiply=2.0)
    return model, layer, kfac


def _ref_chol(Fm, add, mul):
    Fm = Fm.double().cpu()
    n = Fm.shape[-1]
    return torch.linalg.cholesky(torch.linalg.inv(mul ** 0.5 * Fm + add ** 0.5 * torch.eye(n, dtype=torch.float64)))


def test_invert_and_sample(gpu):
    model, layer, kfac = _inverted(gpu)
    LA, LG = kfac.inv_state[layer]
    A, G = kfac.state[layer]
    assert LA.shape == A.shape and LG.shape == G.shape
    for k in range(4):
        assert rel_fro(LA[k], _ref_chol(A[k], 0.3, 2.0)) < 1e-4
        assert rel_fro(LG[k], _ref_chol(G[k], 0.3, 2.0)) < 1e-4
    z = torch.randn(4, LA.shape[1], LG.shape[1], device=gpu)
    s = kfac.sample(layer, z)
    assert tuple(s.shape) == (24, LA.shape[1])
    want = torch.cat([(LA[k].double() @ z[k].double() @ LG[k].double().t()).t() for k in range(4)])
    assert rel_fro(s, want) < TOL


def test_sample_and_replace_and_sample_many(gpu):
    model, layer, kfac = _inverted(gpu)
    LA, LG = kfac.inv_state[layer]
    n, m = LA.shape[1], LG.shape[1]
    mean_w, mean_b = layer.weight.detach().clone(), layer.bias.detach().clone()
    z = torch.randn(4, n, m, device=gpu)
    kfac.sample_and_replace(noise={layer: z})
    torch.cuda.synchronize()
    s = torch.cat([(LA[k].double() @ z[k].double() @ LG[k].double().t()).t() for k in range(4)])
    assert rel_fro(layer.weight.view(24, -1), mean_w.view(24, -1).double().cpu() + s[:, :-1].cpu()) < TOL
    assert rel_fro(layer.bias, mean_b.double().cpu() + s[:, -1].cpu()) < TOL
    # device noise: G n m numbers per layer, and the result is the mean plus a finite draw
    kfac.sample_and_replace()
    torch.cuda.synchronize()
    assert torch.isfinite(layer.weight).all() and not torch.equal(layer.weight, mean_w)
    S = 3
    noise = torch.randn(S, 4, n, m, device=gpu)
    bank = kfac.sample_many(S, noise={layer: noise})
    torch.cuda.synchronize()
    for k in range(S):
        single = torch.cat([(LA[q].double() @ noise[k, q].double() @ LG[q].double().t()).t() for q in range(4)]).cpu()
        assert rel_fro(bank.weights[layer][k], mean_w.view(24, -1).double().cpu() + single[:, :-1]) < TOL
        assert rel_fro(bank.biases[layer][k], mean_b.double().cpu() + single[:, -1]) < TOL


def test_not_positive_definite_names_the_group(gpu):
    model, layer, kfac = _inverted(gpu)
    kfac.state[layer][0][2].copy_(-torch.eye(kfac.state[layer][0].shape[1], device=gpu))
    with pytest.raises(RuntimeError, match="group 2"):
        kfac.invert(add=0.0, multiply=1.0)


def _model_run(gpu, name, N=4, size=64, seed=3):
    from curvature_amd import models
    from curvature_amd.curvatures import KFAC
    torch.manual_seed(seed)
    model = getattr(models, name)(num_classes=10).to(gpu)
    x = torch.randn(N, 3, size, size, device=gpu)
    kfac = KFAC(model)
    loss = F.cross_entropy(model(x), torch.randint(0, 10, (N,), device=gpu))
    model.zero_grad()
    loss.backward()
    return model, kfac


@pytest.mark.parametrize("name", ["mobilenet_v2", "resnext50_32x4d"])
def test_whole_model_chain(gpu, name):
    model, kfac = _model_run(gpu, name)
    kfac.update(batch_size=4)
    kfac.invert(add=0.5, multiply=1.0)
    kfac.sample_and_replace()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in model.parameters())
    grouped = [l for l in kfac.state if isinstance(l, torch.nn.Conv2d) and l.groups > 1]
    assert len(grouped) == {"mobilenet_v2": 17, "resnext50_32x4d": 16}[name]
    for layer in (grouped[0], grouped[1], grouped[len(grouped) // 2], grouped[-1]):
        RA, RG = ref_factors(layer, *kfac.record[layer])
        assert rel_fro(kfac.state[layer][0], RA) < TOL and rel_fro(kfac.state[layer][1], RG) < TOL
        for t in kfac.inv_state[layer]:
            assert torch.isfinite(t).all()


def test_diagonal_on_mobilenet(gpu):
    from curvature_amd.curvatures import Diagonal
    model, _ = _model_run(gpu, "mobilenet_v2")
    diag = Diagonal(model)
    diag.update(batch_size=4)
    torch.cuda.synchronize()
    layer = [l for l in model.modules() if isinstance(l, torch.nn.Conv2d) and l.groups > 1][0]
    want = 4 * layer.weight.grad.double().cpu().view(layer.out_channels, -1) ** 2
    assert rel_fro(diag.state[layer], want) < 1e-6


def test_save_load_round_trip(gpu, tmp_path):
    from curvature_amd import io
    from curvature_amd.curvatures import KFAC
    model, kfac = _model_run(gpu, "mobilenet_v2", N=2, size=32)
    kfac.update(batch_size=2)
    kfac.invert(add=0.5, multiply=1.0)
    path = str(tmp_path / "state.pt")
    io.save_state(kfac, path, attrs=("state", "inv_state"))
    other = KFAC(model)
    io.load_state(other, path, "state")
    io.load_state(other, path, "inv_state")
    for layer in kfac.state:
        for a, b in zip(kfac.state[layer], other.state[layer]):
            assert torch.equal(a, b)
        for a, b in zip(kfac.inv_state[layer], other.inv_state[layer]):
            assert torch.equal(a, b)


def test_graph_replay_equals_eager(gpu):
    from curvature_amd.curvatures import KFAC
    from curvature_amd.graph import KFACStepGraph

    def setup():
        torch.manual_seed(4)
        model = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3, padding=1), torch.nn.ReLU(),
                                    torch.nn.Conv2d(16, 16, 3, padding=1, groups=16), torch.nn.ReLU(),
                                    torch.nn.Conv2d(16, 16, 3, stride=2, padding=1, groups=4)).to(gpu)
        x = torch.randn(2, 8, 10, 10, device=gpu)
        kfac = KFAC(model)
        model(x).square().sum().backward()
        kfac.noise_seed = 7
        return model, kfac

    model_e, eager = setup()
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
    """Each rank of a 2-rank layer shard builds and inverts its own layers: the same bits as the unsharded run."""
    from curvature_amd import sharding
    from curvature_amd.curvatures import KFAC
    model, full = _model_run(gpu, "mobilenet_v2", N=2, size=32)
    layers = full._layers()
    shapes = {l: (tuple(full.record[l][0].shape), tuple(full.record[l][1].shape)) for l in layers}
    dims = sharding.layer_dims(layers, shapes)
    assert any(len(d) == 5 for d in dims)
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


def test_poisoned_scratch(gpu):
    """This file again with CURV_DEBUG_POISON=1: no kernel reads scratch it has not written."""
    import re
    env = dict(os.environ, CURV_DEBUG_POISON="1")
    proc = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                           "tests/test_grouped_conv_gpu.py", "-k", "not poisoned and not two_rank"],
                          cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert proc.returncode == 0, proc.stdout[-3000:]
    passed = re.search(r"(\d+) passed", proc.stdout)
    assert passed and int(passed.group(1)) >= 20, proc.stdout[-3000:]
    assert "skipped" not in proc.stdout and "deselected" in proc.stdout, proc.stdout[-3000:]
