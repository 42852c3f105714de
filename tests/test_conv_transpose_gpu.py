"""KFAC, Diagonal, EFB and INF for ConvTranspose2d on the GPU: the phase-split A-factor build (curv_kfac_convt_accumulate)
against an fp64 oracle of the zero-stuffed input, its bit properties and memory edges, and the estimators end to end on
the DCGAN generator and the U-Net (samplers through the weight permutation, autocast, graph replay, a 2-rank shard,
save / load, poisoned scratch)."""
import functools
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import rel_fro
from exact_inputs import assert_exact_range, exact_gram, nonzero_ints, pow2_scale
from test_conv_transpose_cpu import convt_patches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-6


def _wm(t):
    """Wm = weight.permute(1, 0, 2, 3).reshape(Cout, -1) of a tensor shaped like a ConvTranspose2d weight."""
    return t.permute(1, 0, 2, 3).reshape(t.shape[1], -1)


def _residue_mask(layer):
    """True where two rows of A belong to taps of different residues (a mod s_h, b mod s_w); the bias row is False."""
    kh, kw = layer.kernel_size
    sh, sw = layer.stride
    t = torch.arange(layer.in_channels * kh * kw) % (kh * kw)
    res = (t // kw % sh) * sw + (t % kw % sw)
    mask = res[:, None] != res[None, :]
    if layer.bias is not None:
        n = mask.shape[0] + 1
        full = torch.zeros(n, n, dtype=torch.bool)
        full[:-1, :-1] = mask
        mask = full
    return mask


def _oracle_a_gpu(layer, x, out_size, gpu):
    """fp64 A of one layer, the product on the GPU (large cases)."""
    U = convt_patches(x, layer, out_size).to(gpu)
    if layer.bias is not None:
        U = torch.cat([U, torch.ones(1, U.shape[1], dtype=U.dtype, device=gpu)])
    N, L = x.shape[0], out_size[0] * out_size[1]
    return (U @ U.t() / (N * L)).cpu()


# (cin, cout, kernel, stride, padding, output_padding, N, H, W, bias, output_size)
CASES = [
    (100, 32, 4, 1, 0, 0, 4, 1, 1, False, None),               # DCGAN first layer: 1x1 latent
    (512, 16, 4, 2, 1, 0, 2, 4, 4, False, None),
    (64, 32, 4, 2, 1, 0, 2, 16, 16, True, None),
    (512, 16, 2, 2, 0, 0, 2, 28, 28, True, None),              # U-Net up-convolution: one Gram for all phases
    (64, 32, 2, 2, 0, 0, 2, 128, 128, False, None),            # long K: k-sliced
    (24, 16, 3, 2, 1, 1, 3, 9, 11, True, None),
    (32, 16, 3, 1, 1, 0, 2, 12, 12, True, None),               # stride 1: the 3x3 correlation form
    (7, 5, (5, 3), (3, 2), (2, 1), (2, 1), 3, 6, 7, True, None),
    (16, 8, 3, 2, 3, 0, 2, 9, 9, True, None),                  # padding > k - 1
    (16, 8, 3, 2, 1, 0, 2, 7, 7, True, (14, 14)),              # output_size=
]


def _run_layer(gpu, case, seed=0, dtype=torch.float32):
    from curvature_amd.curvatures import KFAC
    cin, cout, k, s, p, op, N, H, W, bias, osize = case
    torch.manual_seed(seed)
    layer = torch.nn.ConvTranspose2d(cin, cout, k, s, p, op, bias=bias).to(gpu)
    model = torch.nn.Sequential(layer)
    kfac = KFAC(model, ['ConvTranspose2d'])
    x = torch.randn(N, cin, H, W, device=gpu)
    out = layer(x, output_size=osize) if osize is not None else layer(x)
    if osize is not None:
        assert tuple(out.shape[2:]) == osize
    g = torch.randn_like(out)
    out.backward(g)
    return layer, kfac, x, g, out


@pytest.mark.parametrize("case", CASES)
def test_factors_match_fp64_oracle(gpu, case):
    layer, kfac, x, g, out = _run_layer(gpu, case)
    kfac.update(batch_size=x.shape[0])
    A, G = kfac.state[layer]
    torch.cuda.synchronize()
    A_ref = _oracle_a_gpu(layer, x, tuple(out.shape[2:]), gpu)
    gs = g.detach().double().permute(1, 0, 2, 3).reshape(g.shape[1], -1)
    G_ref = (gs @ gs.t() * g.shape[0] / (g.shape[2] * g.shape[3])).cpu()
    Ac = A.cpu()
    assert rel_fro(Ac, A_ref) <= TOL, rel_fro(Ac, A_ref)
    assert rel_fro(G, G_ref) <= 1e-5, rel_fro(G, G_ref)
    assert torch.equal(Ac, Ac.t())
    assert (Ac[_residue_mask(layer)] == 0).all()


def _job(layer, x, out_size, dst, first=True, scale=1.0):
    from curvature_amd import ops
    return ops.ConvTFactorJob(x, dst, layer.kernel_size, layer.stride, layer.padding, out_size, layer.bias is not None,
                              scale, first)


@functools.lru_cache(maxsize=None)
def _exact_case(case):
    """(layer, x, output size, A_exact, scale) of a case with an integer-valued input (tests/exact_inputs.py): the
    unscaled integer Gram of `convt_patches` in float64, the product on the GPU, once per case."""
    cin, cout, k, s, p, op, N, H, W, bias, osize = case
    layer = torch.nn.ConvTranspose2d(cin, cout, k, s, p, op, bias=bias)
    out = osize or tuple((n - 1) * layer.stride[d] - 2 * layer.padding[d] + layer.kernel_size[d] + layer.output_padding[d]
                         for d, n in enumerate((H, W)))
    terms = N * out[0] * out[1]
    assert_exact_range(3, terms, rounds=2)
    x = nonzero_ints((N, cin, H, W), torch.Generator().manual_seed(23))
    A_exact = exact_gram(convt_patches(x, layer, out).to("cuda:0"), ones_row=bias)
    return layer, x, out, A_exact, pow2_scale(terms)


@pytest.mark.parametrize("case", CASES)
def test_factors_match_exact_integers(gpu, case):
    """Every case again, bit for bit: an input uniform in {+-1, +-2, +-3} (none zero, so every element moves the result)
    and a power-of-two scale.  Every product and partial sum is an integer below 2^24, so the window copies, the phase
    Grams on the fp32 MFMA and the assembly have one right answer in any summation order: ``scale * exact`` after a first
    call, twice that after an accumulating one, exact zeros between taps of different residues included (DESIGN.md
    section 5).  The source sits in NaN-filled memory, at an aligned start and 4 bytes past one."""
    from curvature_amd import ops
    layer, x, out, A_exact, scale = _exact_case(case)
    n = A_exact.shape[0]
    for offset in (0, 1):
        fence = torch.full((x.numel() + 4096 + 64,), float("nan"), device=gpu)
        start = 2048 + offset
        xs = fence[start:start + x.numel()].view(x.shape)
        xs.copy_(x)
        a = torch.full((n, n), float("nan"), device=gpu)
        for rounds in (1, 2):
            ops.kfac_accumulate_convt([_job(layer, xs, out, a, first=rounds == 1, scale=scale)])
            got = a.double()
            want = rounds * scale * A_exact
            assert torch.equal(got, want), (offset, rounds, int((got != want).sum()), float((got - want).abs().max()))
            assert torch.equal(a, a.t()), (offset, rounds)


def test_first_accumulate_and_determinism(gpu):
    from curvature_amd import ops
    layer, _, x, _, out = _run_layer(gpu, CASES[2])
    n = layer.in_channels * 16 + 1
    a1 = torch.empty(n, n, device=gpu)
    a2 = torch.empty(n, n, device=gpu)
    ops.kfac_accumulate_convt([_job(layer, x, out.shape[2:], a1)])
    ops.kfac_accumulate_convt([_job(layer, x, out.shape[2:], a2)])
    assert torch.equal(a1, a2)
    ops.kfac_accumulate_convt([_job(layer, x, out.shape[2:], a2, first=False)])
    assert torch.equal(a2, 2 * a1)


def test_factor_alone_equals_whole_model_call(gpu):
    from curvature_amd import ops
    runs = [_run_layer(gpu, CASES[i], seed=i) for i in (1, 3, 5, 7)]
    alone, together, jobs = [], [], []
    for layer, _, x, _, out in runs:
        n = layer.in_channels * layer.kernel_size[0] * layer.kernel_size[1] + int(layer.bias is not None)
        a = torch.empty(n, n, device=gpu)
        ops.kfac_accumulate_convt([_job(layer, x, out.shape[2:], a, scale=0.25)])
        alone.append(a)
        b = torch.empty(n, n, device=gpu)
        jobs.append(_job(layer, x, out.shape[2:], b, scale=0.25))
        together.append(b)
    ops.kfac_accumulate_convt(jobs)
    for a, b in zip(alone, together):
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[3], CASES[5], CASES[7]])
def test_nan_fenced_sources(gpu, case):
    """The source sits inside a NaN-filled buffer, at an aligned start and 4 bytes past it: nothing outside is read."""
    from curvature_amd import ops
    layer, _, x, _, out = _run_layer(gpu, case)
    n = layer.in_channels * layer.kernel_size[0] * layer.kernel_size[1] + int(layer.bias is not None)
    N, L = x.shape[0], out.shape[2] * out.shape[3]
    A_ref = _oracle_a_gpu(layer, x, tuple(out.shape[2:]), gpu)
    for offset in (0, 1):
        fence = torch.full((x.numel() + 4096 + 64,), float("nan"), device=gpu)
        start = 2048 + offset
        xs = fence[start:start + x.numel()].view(x.shape)
        xs.copy_(x)
        a = torch.empty(n, n, device=gpu)
        ops.kfac_accumulate_convt([_job(layer, xs, out.shape[2:], a, scale=1.0 / (N * L))])
        ac = a.cpu()
        assert torch.isfinite(ac).all(), offset
        assert rel_fro(ac, A_ref) <= TOL, (offset, rel_fro(ac, A_ref))


# ---------------------------------------------------------------------------------------------------------------- models
def _model_run(gpu, which, seed=0, autocast=False, types=('Conv2d', 'ConvTranspose2d')):
    from curvature_amd import models
    from curvature_amd.curvatures import KFAC
    torch.manual_seed(seed)
    if which == "dcgan":
        model = models.dcgan_generator(nz=16, ngf=8).to(gpu)
        x = torch.randn(4, 16, 1, 1, device=gpu)
    else:
        model = models.unet(in_channels=3, num_classes=2, width=8).to(gpu)
        x = torch.randn(2, 3, 32, 32, device=gpu)
    types = list(types)
    kfac = KFAC(model, types)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out = model(x)
    model.zero_grad()
    out.float().square().mean().backward()
    return model, kfac, x, types


def _convts(model):
    return [m for m in model.modules() if isinstance(m, torch.nn.ConvTranspose2d)]


@pytest.mark.parametrize("which", ["dcgan", "unet"])
def test_kfac_update_and_samplers(gpu, which):
    model, kfac, x, _ = _model_run(gpu, which)
    kfac.update(batch_size=x.shape[0])
    for layer in _convts(model):
        xin, g = kfac.record[layer]
        A_ref = _oracle_a_gpu(layer, xin.detach(), tuple(g.shape[2:]), gpu)
        assert rel_fro(kfac.state[layer][0], A_ref) <= TOL
    kfac.invert(add=0.5, multiply=1.0)
    layers = kfac._layers()
    noise = {l: torch.randn(kfac.inv_state[l][0].size(0), kfac.inv_state[l][1].size(0), device=gpu) for l in layers}
    mean = {l: (l.weight.detach().clone(), None if l.bias is None else l.bias.detach().clone()) for l in layers}
    kfac.sample_and_replace(noise=noise)
    torch.cuda.synchronize()
    for layer in _convts(model):
        la, lg = (t.double() for t in kfac.inv_state[layer])
        s = (la @ noise[layer].double() @ lg.t()).t()                       # (Cout, n) in Wm order
        n0 = layer.weight.numel() // layer.out_channels
        w_ref = mean[layer][0].double() + s[:, :n0].reshape(layer.out_channels, layer.in_channels,
                                                             *layer.kernel_size).transpose(0, 1)
        assert rel_fro(layer.weight - mean[layer][0], w_ref - mean[layer][0].double()) <= 1e-5
        if layer.bias is not None:
            assert rel_fro(layer.bias - mean[layer][1], s[:, -1]) <= 1e-5
        # the plain sample() is in Wm order
        assert rel_fro(kfac.sample(layer, z=noise[layer]), s) <= 1e-5
    # sample_many with the same noise: the same weights as sample_and_replace
    after = {l: l.weight.detach().clone() for l in layers}
    bank = kfac.sample_many(1, noise={l: z[None] for l, z in noise.items()})
    kfac.replace_from(bank, 0)
    torch.cuda.synchronize()
    for layer in layers:
        assert rel_fro(layer.weight, after[layer]) <= 1e-6


def test_autocast_update(gpu):
    """Under bf16 autocast a ConvTranspose2d fed by another one records a bf16 input: cast to fp32 on the device for the
    A side; the bf16 gradients take the half-precision G build."""
    from curvature_amd.curvatures import KFAC
    torch.manual_seed(2)
    model = torch.nn.Sequential(torch.nn.ConvTranspose2d(16, 32, 4, 1, 0), torch.nn.ReLU(),
                                torch.nn.ConvTranspose2d(32, 8, 4, 2, 1)).to(gpu)
    kfac = KFAC(model, ['ConvTranspose2d'])
    x = torch.randn(4, 16, 1, 1, device=gpu)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = model(x)
    out.float().square().mean().backward()
    assert kfac.record[model[2]][0].dtype == torch.bfloat16
    assert all(kfac.record[l][1].dtype == torch.bfloat16 for l in _convts(model))
    kfac.update(batch_size=x.shape[0])
    for layer in _convts(model):
        xin, g = kfac.record[layer]
        A_ref = _oracle_a_gpu(layer, xin.detach().float(), tuple(g.shape[2:]), gpu)
        assert rel_fro(kfac.state[layer][0], A_ref) <= TOL
        gs = g.detach().double().permute(1, 0, 2, 3).reshape(g.shape[1], -1)
        G_ref = gs @ gs.t() * g.shape[0] / (g.shape[2] * g.shape[3])
        assert rel_fro(kfac.state[layer][1], G_ref) <= 1e-5


def test_diagonal_efb_inf_states(gpu):
    from curvature_amd.curvatures import EFB, INF, Diagonal
    model, kfac, x, types = _model_run(gpu, "unet", types=('ConvTranspose2d',))
    N = x.shape[0]
    kfac.update(batch_size=N)
    diag = Diagonal(model, types)
    diag.update(N)
    efb = EFB(model, kfac.state, types)
    efb.update(N)
    torch.cuda.synchronize()
    for layer in _convts(model):
        grad = torch.cat([_wm(layer.weight.grad.double()), layer.bias.grad.double()[:, None]], 1)
        assert rel_fro(diag.state[layer], grad ** 2 * N) <= 1e-6
        ua, ug = (t.double() for t in efb.eigvecs[layer])
        assert rel_fro(efb.state[layer], (ug.t() @ grad @ ua) ** 2) <= 1e-5
        assert rel_fro(efb.diags[layer], grad ** 2 * N) <= 1e-6
    inf = INF(model, efb.diags, kfac.state, efb.state, types, eigvecs=efb.eigvecs)
    inf.update(rank=100)
    torch.cuda.synchronize()
    for layer in _convts(model):
        ua, ug, lam, corr = (t.double() for t in inf.state[layer])
        D = efb.diags[layer].double().t() - (ua ** 2) @ lam.view(ua.shape[1], ug.shape[1]) @ (ug ** 2).t()
        assert rel_fro(corr, D.reshape(-1)) <= 1e-5
    # the fused samplers write through the permutation what sample() returns in Wm order
    for est in (diag, efb, inf):
        est.invert(add=0.5, multiply=1.0)
    for est, kind in ((efb, "efb"), (inf, "inf")):
        layers = [l for l in est._layers()]
        if kind == "efb":
            noise = {l: torch.randn(est.eigvecs[l][0].shape[0], est.eigvecs[l][1].shape[0], device=gpu) for l in layers}
            ref = {l: est.sample(l, z=noise[l]) for l in layers}
        else:
            noise = {l: torch.randn(est.eigvecs[l][0].shape[0] * est.eigvecs[l][1].shape[0], device=gpu) for l in layers}
            ref = {l: est.sample(l, X=noise[l]) for l in layers}
        est.sample_and_replace(noise=noise)
        torch.cuda.synchronize()
        for layer in _convts(model):
            mean = est.model_state_of(layer, 'weight').double()
            s = ref[layer].double()
            n0 = layer.weight.numel() // layer.out_channels
            w_ref = mean + s[:, :n0].reshape(layer.out_channels, layer.in_channels, *layer.kernel_size).transpose(0, 1)
            assert rel_fro(layer.weight.double() - mean, w_ref - mean) <= 1e-5, kind
    # Diagonal: mean + z * inv through the permutation (noise from its own generator: compare statistics of the layout)
    diag.noise_seed = 3
    diag.sample_and_replace()
    torch.cuda.synchronize()
    for layer in _convts(model):
        mean = diag.model_state_of(layer, 'weight')
        z = _wm(layer.weight.detach() - mean) / diag.inv_state[layer][:, :-1]
        assert torch.isfinite(z).all() and 0.5 < float(z.std()) < 2.0


def test_graph_replay_equals_eager(gpu):
    from curvature_amd.graph import KFACStepGraph

    def setup():
        model, kfac, _, _ = _model_run(gpu, "dcgan", seed=4)
        kfac.noise_seed = 7
        return model, kfac

    model_e, eager = setup()
    weights = []
    for _ in range(3):
        eager.update(4)
        eager.invert(0.5, 1.0)
        eager.sample_and_replace()
        weights.append([p.detach().clone() for p in model_e.parameters()])
    model_g, kfac = setup()
    graph = KFACStepGraph(kfac, add=0.5, multiply=1.0, batch_size=4, warmup=2)
    for step in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(model_g.parameters(), weights[step]):
            assert torch.equal(a.detach(), b)
    graph.check()


def test_two_rank_shard_same_bits(gpu):
    from curvature_amd import sharding
    from curvature_amd.curvatures import KFAC
    model, full, x, types = _model_run(gpu, "unet")
    layers = full._layers()
    shapes = {l: (tuple(full.record[l][0].shape), tuple(full.record[l][1].shape)) for l in layers}
    dims = sharding.layer_dims(layers, shapes)
    full.update(batch_size=x.shape[0])
    full.invert(add=0.5, multiply=1.0)
    owner = sharding.partition_layers(dims, 2)
    assert set(owner) == {0, 1}
    seen = set()
    for rank in range(2):
        est = KFAC(model, types, shard=sharding.Shard(owner, rank, 2))
        est.record = full.record
        est.update(batch_size=x.shape[0])
        est.invert(add=0.5, multiply=1.0)
        for layer in est.state:
            seen.add(layer)
            assert all(torch.equal(a, b) for a, b in zip(est.state[layer], full.state[layer]))
            assert all(torch.equal(a, b) for a, b in zip(est.inv_state[layer], full.inv_state[layer]))
    assert seen == set(full.state)


def test_save_load_round_trip(gpu, tmp_path):
    from curvature_amd import io
    from curvature_amd.curvatures import KFAC
    model, kfac, x, types = _model_run(gpu, "dcgan")
    kfac.update(batch_size=x.shape[0])
    kfac.invert(add=0.5, multiply=1.0)
    path = str(tmp_path / "state.pt")
    io.save_state(kfac, path, attrs=("state", "inv_state"))
    other = KFAC(model, types)
    io.load_state(other, path, "state")
    io.load_state(other, path, "inv_state")
    assert set(other.state) >= set(_convts(model))
    for layer in kfac.state:
        for a, b in zip(kfac.state[layer], other.state[layer]):
            assert torch.equal(a, b)
        for a, b in zip(kfac.inv_state[layer], other.inv_state[layer]):
            assert torch.equal(a, b)


def test_poisoned_scratch(gpu):
    """The factor-build cases again with CURV_DEBUG_POISON=1: no kernel reads scratch it has not written."""
    env = dict(os.environ, CURV_DEBUG_POISON="1")
    proc = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                           "tests/test_conv_transpose_gpu.py", "-k",
                           "factors_match or first_accumulate or alone or nan_fenced or samplers"],
                          cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert proc.returncode == 0, proc.stdout[-3000:]
    passed = re.search(r"(\d+) passed", proc.stdout)
    assert passed and int(passed.group(1)) >= 15, proc.stdout[-3000:]
    assert "skipped" not in proc.stdout and "deselected" in proc.stdout, proc.stdout[-3000:]
