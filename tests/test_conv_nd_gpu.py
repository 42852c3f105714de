"""Conv1d and Conv3d on the GPU (`ops.admit_conv_nd`): the Conv3d A-factor build of csrc/conv3d_factor.hip
against the float64 Gram of the explicit 3-D unfold and, bit for bit, against the plain build of the torch-made stack; its
bit properties and memory edges; KFAC end to end on a small 3-D model; and twins - the same estimators on a Conv2d model
that shares weights and inputs.

Expected values are computed here with torch in float64.  The bar for factors is the project's parity bar of DESIGN.md
section 5: relative Frobenius error at most 1e-4 against float64 (`conftest.rel_fro`)."""
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
TOL = 1e-4            # TOL of tests/test_per_sample_gpu.py, test_glm_predictive_gpu.py
ADD, MULTIPLY = 0.5, 2.0


@pytest.fixture(autouse=True)
def admitted():
    from curvature_amd import ops
    was = ops.admit_conv_nd(True)
    yield
    ops.admit_conv_nd(was)


def rel2(a, b):
    """Relative 2-norm error (tests/test_glm_predictive_gpu.py)."""
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


def triple(v):
    return (v, v, v) if isinstance(v, int) else tuple(v)


def im2col3d(x, k, s, p):
    """(C kd kh kw, N Do Ho Wo) and Do Ho Wo: pad, then unfold over the three spatial axes."""
    xp = F.pad(x, (p[2], p[2], p[1], p[1], p[0], p[0]))
    u = xp.unfold(2, k[0], s[0]).unfold(3, k[1], s[1]).unfold(4, k[2], s[2])          # (N, C, Do, Ho, Wo, kd, kh, kw)
    return u.permute(1, 5, 6, 7, 0, 2, 3, 4).reshape(x.shape[1] * math.prod(k), -1), math.prod(u.shape[2:5])


def depth_unfolded(x, k, s, p):
    """The stack by torch: x'[(n Do + d), (c kd + a), h, w] = x[n, c, d sd + a - pd, h, w], zero outside the input."""
    N, C, D, H, W = x.shape
    u = F.pad(x, (0, 0, 0, 0, p[0], p[0])).unfold(2, k[0], s[0])                      # (N, C, Do, H, W, kd)
    return u.permute(0, 2, 1, 5, 3, 4).reshape(N * u.shape[2], C * k[0], H, W).contiguous()


# ------------------------------------------------------------------------------------------------ 1. the factor
# name: (N, C, D, H, W, kernel, stride, padding)
CASES = {
    "basic": (2, 3, 5, 6, 7, 3, 1, 1),                                   # isotropic 3x3x3
    "anisotropic": (2, 2, 6, 5, 7, (2, 3, 1), (2, 1, 2), (1, 0, 1)),     # depth stride 2 with depth padding
    "kd1": (1, 4, 4, 4, 4, (1, 3, 3), (1, 2, 2), (0, 1, 1)),             # depth kernel 1
    "temporal": (2, 3, 3, 5, 5, (3, 1, 1), 1, (2, 0, 0)),                # temporal kernel, padding above kd / 2
    "all_padding": (2, 3, 3, 5, 5, 3, 1, (3, 1, 1)),                     # output depths whose whole patch is padding
    "correlation": (2, 64, 4, 8, 8, 3, 1, 1),                            # 192-channel stacks on the correlation path
    "grouped_launch": (2, 32, 8, 16, 16, 3, 1, 1),                       # about 6 GFLOP: above the small-launch form
    "long_plane": (1, 2, 3, 3, 4101, (2, 1, 3), 1, (0, 0, 1)),           # a plane longer than one staging pass, odd length
}
NO_BIAS = ("basic", "anisotropic", "all_padding")


def geometry(name):
    N, C, D, H, W, k, s, p = CASES[name]
    return (N, C, D, H, W), triple(k), triple(s), triple(p)


@functools.lru_cache(maxsize=None)
def factor_case(name):
    """The source of a case on the GPU and its float64 A factors (with and without the ones row), scale 1 / (N L); made
    once and left unchanged."""
    shape, k, s, p = geometry(name)
    gpu = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(*shape, generator=gen)
    X, L = im2col3d(x.double().to(gpu), k, s, p)
    X1 = torch.cat([X, torch.ones(1, X.shape[1], dtype=X.dtype, device=gpu)])
    K = shape[0] * L
    assert X.shape[1] == K
    want = {False: (X @ X.t() / K).cpu(), True: (X1 @ X1.t() / K).cpu()}
    return x.to(gpu), want, 1.0 / K


def conv3d_job(name, src, dst, bias=True, scale=1.0, first=True):
    from curvature_amd import ops
    _, k, s, p = geometry(name)
    return ops.Conv3dFactorJob(src, dst, k, s, p, bias, scale, first)


def dim_of(name, bias=True):
    shape, k, _, _ = geometry(name)
    return shape[1] * math.prod(k) + int(bias)


def built(name, bias=True, src=None, first=True, into=None):
    from curvature_amd import ops
    x, _, scale = factor_case(name)
    n = dim_of(name, bias)
    dst = torch.full((n, n), float("nan"), device=x.device) if into is None else into
    ops.kfac_accumulate_conv3d([conv3d_job(name, x if src is None else src, dst, bias, scale, first)])
    return dst


@pytest.mark.parametrize("name, bias", [(n, True) for n in CASES] + [(n, False) for n in NO_BIAS])
def test_factor_against_float64_and_the_plain_build_of_the_torch_stack(gpu, name, bias):
    from curvature_amd import ops
    x, want, scale = factor_case(name)
    _, k, s, p = geometry(name)
    dst = built(name, bias)                                                          # `first` overwrites the NaNs
    got = dst.cpu()
    err = rel_fro(got, want[bias])
    print(f"conv3d factor {name} bias={bias}: rel_fro {err:.3e}")
    assert err <= BAR
    assert torch.equal(got, got.t())
    if bias:                                                                          # the ones row against itself: K / K
        assert abs(float(got[-1, -1]) - 1.0) <= 1e-6
    # bit for bit the plain build of the stack torch makes from the same x, in a call of its own: this pins the gather
    stack = depth_unfolded(x, k, s, p)
    plain = torch.full_like(dst, float("nan"))
    ops.kfac_accumulate([ops.FactorJob(stack, plain, k[1:], s[1:], p[1:], bias, scale, True)])
    assert torch.equal(dst, plain)


def _fenced_copy(t, gpu, offset):
    """A copy of `t` inside NaN-filled memory, `offset` floats past a 16-byte boundary."""
    fence = torch.full((t.numel() + 4096 + 64,), float("nan"), device=gpu)
    start = 2048 + offset
    view = fence[start:start + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _assert_exact(dst, want, what):
    got = dst.double()
    assert torch.equal(got, want), (what, int((got != want).sum()), float((got - want).abs().max()))
    assert torch.equal(dst, dst.t()), what


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """An integer-valued source of a case (tests/exact_inputs.py), the unscaled integer Grams of its 3-D unfold in float64
    (without and with the ones row), formed on the GPU once, and a power-of-two scale."""
    shape, k, s, p = geometry(name)
    gpu = torch.device("cuda:0")
    x = nonzero_ints(shape, torch.Generator().manual_seed(sum(map(ord, name)) + 1))
    X, L = im2col3d(x.double().to(gpu), k, s, p)
    assert_exact_range(3, shape[0] * L, rounds=2)
    return x, {False: exact_gram(X), True: exact_gram(X, ones_row=True)}, pow2_scale(shape[0] * L)


@pytest.mark.parametrize("name, bias", [(n, True) for n in CASES] + [(n, False) for n in NO_BIAS])
def test_conv3d_factor_exact_on_integer_inputs(gpu, name, bias):
    """Every Conv3d case again, bit for bit: a source uniform in {+-1, +-2, +-3} (none zero, so every element moves the
    result) and a power-of-two scale.  Every product and partial sum is an integer below 2^24, so the depth gather and the
    plain build of the stack have one right answer in any summation order: ``scale * exact`` after a first call, twice
    that after an accumulating one.  The source sits in NaN-filled memory, at an aligned start and 4
    bytes past one."""
    from curvature_amd import ops
    x, exact, scale = exact_case(name)
    n = dim_of(name, bias)
    for offset in (0, 1):
        xs = _fenced_copy(x, gpu, offset)
        dst = torch.full((n, n), float("nan"), device=gpu)
        for rounds in (1, 2):
            ops.kfac_accumulate_conv3d([conv3d_job(name, xs, dst, bias, scale, first=rounds == 1)])
            _assert_exact(dst, rounds * scale * exact[bias], (offset, rounds))


@pytest.mark.parametrize("which", [0, 2], ids=["k5_p2", "k3_s2"])
def test_conv1d_factors_exact_on_integer_inputs(gpu, which):
    """The two Conv1d layers of `make_model1d` on integer-valued (N, C, L) records, through the jobs `ops.factor_jobs` makes
    for them (the Conv2d build of the (N, C, 1, L) views): both factors bit for bit, as above."""
    from curvature_amd import ops
    layer = make_model1d(torch.device("cpu"))[which]
    gen = torch.Generator().manual_seed(40 + which)
    N, length = 6, 32
    x = nonzero_ints((N, layer.in_channels, length), gen)
    L = (length + 2 * layer.padding[0] - layer.kernel_size[0]) // layer.stride[0] + 1
    g = nonzero_ints((N, layer.out_channels, L), gen)
    assert_exact_range(3, N * L, rounds=2)
    rows = F.unfold(x.double().to(gpu).unsqueeze(2), (1,) + layer.kernel_size, padding=(0,) + layer.padding,
                    stride=(1,) + layer.stride)
    assert rows.shape[2] == L
    A_exact = exact_gram(rows.transpose(0, 1).reshape(rows.shape[1], -1), ones_row=True)
    G_exact = exact_gram(g.double().to(gpu).transpose(0, 1).reshape(g.shape[1], -1))
    scale_a = pow2_scale(N * L)
    scale_g = 4.0 * scale_a
    for offset in (0, 1):
        sides = ops.factor_jobs(layer, _fenced_copy(x, gpu, offset), _fenced_copy(g, gpu, offset))
        assert type(sides.a) is ops.FactorJob and type(sides.g) is ops.FactorJob and (sides.N, sides.L) == (N, L)
        A = torch.full((sides.n, sides.n), float("nan"), device=gpu)
        G = torch.full((sides.m, sides.m), float("nan"), device=gpu)
        sides.a.dst, sides.a.scale = A, scale_a
        sides.g.dst, sides.g.scale = G, scale_g
        for rounds in (1, 2):
            sides.a.first = sides.g.first = rounds == 1
            ops.kfac_accumulate([sides.a, sides.g])
            _assert_exact(A, rounds * scale_a * A_exact, ("A", offset, rounds))
            _assert_exact(G, rounds * scale_g * G_exact, ("G", offset, rounds))


def test_the_grouped_launch_case_is_above_the_small_launch_form(gpu):
    from curvature_amd import _lib, ops
    x, _, _ = factor_case("grouped_launch")
    job = conv3d_job("grouped_launch", x, None)
    _, k, s, p = geometry("grouped_launch")
    assert ops.kfac_path_for([ops.FactorJob(job.stack_shape, None, k[1:], s[1:], p[1:], True)]) == _lib.PATH_GROUPED
    assert ops.kfac_path_for([ops.FactorJob(conv3d_job("basic", factor_case("basic")[0], None).stack_shape, None, (3, 3),
                                            (1, 1), (1, 1), True)]) == _lib.PATH_SMALL


@pytest.mark.parametrize("name", ["basic", "anisotropic"])
def test_bit_properties(gpu, name):
    _, want, _ = factor_case(name)
    n = dim_of(name)
    once = built(name)
    assert torch.equal(once, once.t())                                                # bit-for-bit symmetric
    assert torch.equal(built(name), once)                                             # two runs are equal
    # first = 0 adds onto what dst holds
    gen = torch.Generator().manual_seed(9)
    held = torch.randn(n, n, generator=gen)
    held = (held + held.t()).to(gpu)
    dst = built(name, first=False, into=held.clone())
    assert rel_fro(dst - held, want[True]) <= BAR
    assert torch.equal(dst, dst.t())


def test_a_factor_has_the_same_bits_alone_and_in_a_call_with_others(gpu):
    from curvature_amd import ops
    names = ["anisotropic", "basic", "correlation", "all_padding", "long_plane"]
    alone, together, jobs = [], [], []
    for name in names:
        x, _, scale = factor_case(name)
        alone.append(built(name))
        n = dim_of(name)
        b = torch.full((n, n), float("nan"), device=gpu)
        jobs.append(conv3d_job(name, x, b, True, scale))
        together.append(b)
    ops.kfac_accumulate_conv3d(jobs)
    for name, a, b in zip(names, alone, together):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("name", ["basic", "all_padding", "long_plane"])
def test_memory_edges(gpu, name):
    """The source a contiguous slice that starts 4 bytes past a 16-byte boundary and ends right before NaN-filled memory,
    the workspace filled with 0xFF on the same stream before the call: finite, and the bits of the clean run."""
    from curvature_amd import _lib, ops
    x, _, scale = factor_case(name)
    clean = built(name)
    buf = torch.full((x.numel() + 1 + 1024,), float("nan"), device=gpu)
    assert buf.data_ptr() % 16 == 0
    xs = buf[1:1 + x.numel()].view(x.shape)
    xs.copy_(x)
    assert xs.is_contiguous() and xs.data_ptr() % 16 == 4
    n = dim_of(name)
    dst = torch.full((n, n), float("nan"), device=gpu)
    job = conv3d_job(name, xs, dst, True, scale)
    need = int(_lib.lib().curv_kfac_conv3d_workspace_bytes(ops._conv3d_descs([job]), 1))
    ws = ops.workspace(need, gpu, "kfac_conv3d")
    ws.fill_(0xFF)
    ops.kfac_accumulate_conv3d([job])
    assert ops.workspace(need, gpu, "kfac_conv3d").data_ptr() == ws.data_ptr()        # the buffer the call used
    assert torch.isfinite(dst).all()
    assert torch.equal(dst, clean)
    assert torch.isnan(buf[0]) and torch.isnan(buf[1 + x.numel():]).all()            # and nothing around it was written


def test_destination_shape_and_device_are_checked(gpu):
    from curvature_amd import ops
    x, _, scale = factor_case("basic")
    n = dim_of("basic")
    for bad in (torch.empty(n + 1, n + 1, device=gpu), torch.empty(n, n - 1, device=gpu), torch.empty(n * n, device=gpu)):
        with pytest.raises(RuntimeError, match="destination must be"):
            ops.kfac_accumulate_conv3d([conv3d_job("basic", x, bad, True, scale)])
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.kfac_accumulate_conv3d([conv3d_job("basic", x, torch.empty(n, n), True, scale)])
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.kfac_accumulate_conv3d([conv3d_job("basic", x.cpu(), torch.empty(n, n, device=gpu), True, scale)])
    with pytest.raises(RuntimeError, match=r"\(N,C,D,H,W\)"):
        ops.kfac_accumulate_conv3d([conv3d_job("basic", x[0], torch.empty(n, n, device=gpu), True, scale)])


# ------------------------------------------------------------------------------------------------ 2. end to end
N_MODEL, CLASSES = 4, 5


def make_model3d(gpu, seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv3d(2, 4, 3, padding=1), torch.nn.ReLU(),
                               torch.nn.Conv3d(4, 4, (1, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1)), torch.nn.Flatten(),
                               torch.nn.Linear(4 * 4 * 3 * 3, CLASSES)).to(gpu)


KINDS_3D = ['Conv3d', 'Linear']


def selected(model):
    return [model[0], model[2], model[4]]


def backward(model, x, labels):
    model.zero_grad()
    F.cross_entropy(model(x), labels).backward()


def batches3d(gpu):
    gen = torch.Generator().manual_seed(11)
    xs = [torch.randn(N_MODEL, 2, 4, 6, 6, generator=gen).to(gpu) for _ in range(2)]
    return xs, [torch.tensor([1, 4, 0, 2], device=gpu), torch.tensor([3, 3, 0, 1], device=gpu)]


def float64_factors(layer, xin, g):
    """(A, G) of one KFAC.update on the records (xin, g) in float64: A = X X^T / (N L), G = N / L g g^T."""
    xin, g = xin.detach().double().cpu(), g.detach().double().cpu()
    N = xin.shape[0]
    if isinstance(layer, torch.nn.Conv3d):
        X, L = im2col3d(xin, triple(layer.kernel_size), triple(layer.stride), triple(layer.padding))
        gs = g.transpose(0, 1).reshape(g.shape[1], -1)
    elif isinstance(layer, (torch.nn.Conv2d, torch.nn.Conv1d)):
        if xin.dim() == 3:
            xin, g = xin.unsqueeze(2), g.unsqueeze(2)
        pad = lambda v: ((1,) if len(v) == 1 else ()) + tuple(v)
        cols = F.unfold(xin, pad(layer.kernel_size), dilation=pad(layer.dilation),
                        padding=((0,) if len(layer.padding) == 1 else ()) + tuple(layer.padding), stride=pad(layer.stride))
        L = cols.shape[2]
        X = cols.transpose(0, 1).reshape(cols.shape[1], -1)
        gs = g.transpose(0, 1).reshape(g.shape[1], -1)
    else:
        L, X, gs = 1, xin.t(), g.t()
    if layer.bias is not None:
        X = torch.cat([X, torch.ones(1, X.shape[1], dtype=X.dtype)])
    return X @ X.t() / (N * L), gs @ gs.t() * N / L


def test_kfac_on_a_3d_model_end_to_end(gpu, tmp_path):
    from curvature_amd import io
    from curvature_amd.curvatures import KFAC
    model = make_model3d(gpu)
    layers = selected(model)
    kfac = KFAC(model, KINDS_3D)
    assert kfac._layers() == layers
    want = {l: [0, 0] for l in layers}
    for x, labels in zip(*batches3d(gpu)):
        backward(model, x, labels)
        kfac.update(N_MODEL)
        for l in layers:
            A, G = float64_factors(l, *kfac.record[l])
            want[l][0], want[l][1] = want[l][0] + A, want[l][1] + G
    for layer in layers:
        A, G = kfac.state[layer]
        err_a, err_g = rel_fro(A, want[layer][0]), rel_fro(G, want[layer][1])
        print(f"KFAC state {layer.__class__.__name__}: A {err_a:.3e}, G {err_g:.3e}")
        assert err_a <= BAR and err_g <= BAR
        assert torch.equal(A, A.t()) and torch.equal(G, G.t())
    assert kfac.state[layers[0]][0].shape == (2 * 27 + 1, 2 * 27 + 1) and kfac.state[layers[1]][0].shape == (37, 37)
    kfac.invert(add=ADD, multiply=MULTIPLY)
    for layer in layers:
        for Fm, Lf in zip(kfac.state[layer], kfac.inv_state[layer]):
            assert torch.isfinite(Lf).all()
            n = Fm.shape[0]
            M = math.sqrt(MULTIPLY) * Fm.double() + math.sqrt(ADD) * torch.eye(n, device=gpu, dtype=torch.float64)
            M = (M + M.t()) / 2
            R = (Lf.double() @ Lf.double().t()) @ M - torch.eye(n, device=gpu, dtype=torch.float64)
            assert float(torch.linalg.norm(R)) / n ** 0.5 < identity_residual_bound(M)
    # sample_and_replace writes the 5-D weights in place, keeps their shapes and leaves the other parameters alone
    only = KFAC(model, ['Conv3d'])
    only.state = {l: kfac.state[l] for l in layers[:2]}
    only.invert(add=ADD, multiply=MULTIPLY)
    before = {name: (p.data_ptr(), p.detach().clone()) for name, p in model.named_parameters()}
    only.sample_and_replace()
    torch.cuda.synchronize()
    for name, p in model.named_parameters():
        ptr, old = before[name]
        assert p.data_ptr() == ptr and p.shape == old.shape and torch.isfinite(p).all()
        assert torch.equal(p, old) == name.startswith("4.")                          # the Linear layer is not selected
    assert model[0].weight.shape == (4, 2, 3, 3, 3) and model[2].weight.shape == (4, 4, 1, 3, 3)
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(before[name][1])
    # io round trip, by name, into an estimator of a fresh copy of the model
    path = str(tmp_path / "kfac3d.pt")
    io.save_state(kfac, path, attrs=("state", "inv_state"))
    fresh = make_model3d(gpu, seed=1)
    fresh.load_state_dict(model.state_dict())
    other = KFAC(fresh, KINDS_3D)
    io.load_state(other, path)
    io.load_state(other, path, attr="inv_state")
    for la, lb in zip(layers, selected(other.model)):
        for a, b in zip(kfac.state[la] + list(kfac.inv_state[la]), other.state[lb] + list(other.inv_state[lb])):
            assert torch.equal(a, b)
    other.sample_and_replace()
    assert all(torch.isfinite(p).all() for p in other.model.parameters())


def test_banks_decompose_and_the_gradient_estimators_on_the_3d_model(gpu):
    """`sample_many` / `replace_from`, `decompose`, and Diagonal / BlockDiagonal (which read ``weight.grad`` through the
    (out, -1) layer matrix) take the 5-D weights."""
    from curvature_amd.curvatures import KFAC, BlockDiagonal, Diagonal
    model = make_model3d(gpu, seed=2)
    layers = selected(model)
    (x, _), (labels, _) = batches3d(gpu)
    kfac, diag, block = KFAC(model, KINDS_3D), Diagonal(model, KINDS_3D), BlockDiagonal(model, ['Conv3d'])
    backward(model, x, labels)
    for est in (kfac, diag, block):
        est.update(N_MODEL)
    for layer in layers:
        grad = torch.cat([layer.weight.grad.reshape(layer.weight.shape[0], -1), layer.bias.grad.reshape(-1, 1)], dim=1)
        assert rel_fro(diag.state[layer], grad.double() ** 2 * N_MODEL) <= 1e-6
    g = torch.cat([model[0].weight.grad.reshape(-1), model[0].bias.grad]).double()
    assert rel_fro(block.state[model[0]], torch.outer(g, g) * N_MODEL) <= BAR
    kfac.decompose()
    for est in (kfac, diag, block):
        est.invert(add=ADD, multiply=MULTIPLY)
    mean = [p.detach().clone() for p in model.parameters()]
    bank = kfac.sample_many(3)
    assert bank.weights[model[0]].shape[0] == 3 and bank.weights[model[0]][0].numel() == model[0].weight.numel()
    kfac.replace_from(bank, 1)
    torch.cuda.synchronize()
    for layer in layers:
        assert torch.equal(layer.weight.detach().reshape(-1), bank.weights[layer][1].reshape(-1))
        assert torch.equal(layer.bias.detach(), bank.biases[layer][1])
    assert model[0].weight.shape == (4, 2, 3, 3, 3)
    for est in (diag, block):
        est.sample_and_replace()
        torch.cuda.synchronize()
        assert all(torch.isfinite(p).all() for p in model.parameters())
        assert not torch.equal(model[0].weight.detach(), mean[0])
    for hook in kfac.hooks:
        hook.remove()


def test_graph_replay_equals_eager(gpu):
    """One capture of the KFAC step on the 3-D model (as tests/test_dilated_gpu.py): replay and eager agree bit for bit,
    factors included - the Conv3d build neither waits on the host nor allocates."""
    from curvature_amd.curvatures import KFAC
    from curvature_amd.graph import KFACStepGraph

    def setup():
        model = make_model3d(gpu, seed=7)
        gen = torch.Generator().manual_seed(8)
        x, labels = torch.randn(N_MODEL, 2, 4, 6, 6, generator=gen).to(gpu), torch.tensor([0, 1, 2, 3], device=gpu)
        kfac = KFAC(model, KINDS_3D)
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


# ------------------------------------------------------------------------------------------------ 3. twins
def twin_of(model, gpu):
    """The Conv2d model with the same weights: a Conv3d (D = kd, pd = 0, so Do = 1) as Conv2d(C kd, M, (kh, kw)) with
    weight.reshape(M, C kd, kh, kw); a Conv1d as the Conv2d with H = 1."""
    mods = []
    for mod in model:
        if isinstance(mod, torch.nn.Conv3d):
            kd = mod.kernel_size[0]
            assert mod.padding[0] == 0
            two = torch.nn.Conv2d(mod.in_channels * kd, mod.out_channels, mod.kernel_size[1:], stride=mod.stride[1:],
                                  padding=mod.padding[1:], bias=mod.bias is not None)
        elif isinstance(mod, torch.nn.Conv1d):
            two = torch.nn.Conv2d(mod.in_channels, mod.out_channels, (1,) + mod.kernel_size, stride=(1,) + mod.stride,
                                  padding=(0,) + mod.padding, dilation=(1,) + mod.dilation, bias=mod.bias is not None)
        else:
            mods.append(copy.deepcopy(mod))
            continue
        with torch.no_grad():
            two.weight.copy_(mod.weight.reshape(two.weight.shape))
            if mod.bias is not None:
                two.bias.copy_(mod.bias)
        mods.append(two)
    return torch.nn.Sequential(*mods).to(gpu)


def chain(model, kinds, x, labels, eigvecs=None):
    """Diagonal, KFAC, EFB and INF of `model` after one pass on (x, labels), INF over every (I, J) pair; KFAC inverted and
    sampled with a pinned seed: (diag, kfac, efb, inf, the drawn [W | b] per layer)."""
    from curvature_amd.curvatures import EFB, INF, KFAC, Diagonal
    layers = [m for m in model if m.__class__.__name__ in kinds]
    diag, kfac = Diagonal(model, kinds), KFAC(model, kinds)
    backward(model, x, labels)
    diag.update(x.shape[0])
    kfac.update(x.shape[0])
    if eigvecs is not None:
        eigvecs = dict(zip(layers, eigvecs))
    efb = EFB(model, kfac.state, kinds, eigvecs=eigvecs)
    efb.update(x.shape[0])
    inf = INF(model, diag.state, kfac.state, efb.state, kinds, eigvecs=efb.eigvecs)
    inf.update(rank=1 << 20)
    kfac.invert(add=ADD, multiply=MULTIPLY)
    mean = [p.detach().clone() for p in model.parameters()]
    kfac.noise_seed = 1234
    kfac.sample_and_replace()
    torch.cuda.synchronize()
    drawn = [l.weight.detach().reshape(l.weight.shape[0], -1).clone() for l in layers]
    with torch.no_grad():
        for p, m in zip(model.parameters(), mean):
            p.copy_(m)
    for hook in kfac.hooks:
        hook.remove()
    return layers, diag, kfac, efb, inf, drawn


def compare_twins(what, a, b):
    """The chains of a model and of its twin: everything at the 1e-4 bar, the first layer's A factor bit for bit.  The twin's
    EFB and INF are given the eigenvectors of the model's own EFB: eigenvalues are compared in one basis (two
    decompositions of factors that agree to rounding may differ by signs and by rotations inside close eigenvalues)."""
    (la, diag_a, kfac_a, efb_a, inf_a, drawn_a), (lb, diag_b, kfac_b, efb_b, inf_b, drawn_b) = a, b
    worst = {}

    def bar(key, got, want):
        err = rel_fro(got, want)
        worst[key] = max(worst.get(key, 0.0), err)
        assert err <= BAR, (what, key, err)
    assert torch.equal(kfac_a.state[la[0]][0], kfac_b.state[lb[0]][0])
    for k, (x, y) in enumerate(zip(la, lb)):
        for side in (0, 1):
            bar("KFAC.state", kfac_a.state[x][side], kfac_b.state[y][side])
        bar("Diagonal.state", diag_a.state[x], diag_b.state[y])
        bar("EFB.state", efb_a.state[x], efb_b.state[y])
        bar("EFB.diags", efb_a.diags[x], efb_b.diags[y])
        bar("INF lambda", inf_a.state[x][2], inf_b.state[y][2])
        bar("INF D", inf_a.state[x][3], inf_b.state[y][3])
        bar("drawn weights", drawn_a[k], drawn_b[k])
        assert float(torch.linalg.norm(drawn_a[k] - x.weight.detach().reshape(drawn_a[k].shape))) > 0
    print(f"twins {what}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


def test_conv3d_with_one_output_depth_against_its_conv2d_twin(gpu):
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Conv3d(3, 6, 3, padding=(0, 1, 1)), torch.nn.ReLU(), torch.nn.Flatten(),
                                torch.nn.Linear(6 * 8 * 8, CLASSES)).to(gpu)
    twin = twin_of(model, gpu)
    gen = torch.Generator().manual_seed(4)
    x, labels = torch.randn(N_MODEL, 3, 3, 8, 8, generator=gen).to(gpu), torch.tensor([0, 4, 2, 2], device=gpu)
    assert rel_fro(twin(x.reshape(N_MODEL, 9, 8, 8)), model(x)) <= 1e-6
    a = chain(model, ['Conv3d', 'Linear'], x, labels)
    b = chain(twin, ['Conv2d', 'Linear'], x.reshape(N_MODEL, 9, 8, 8), labels, eigvecs=[a[3].eigvecs[l] for l in a[0]])
    compare_twins("Conv3d (Do = 1)", a, b)


def make_model1d(gpu, seed=5, **first):
    torch.manual_seed(seed)
    first = dict(dict(kernel_size=5, padding=2), **first)
    return torch.nn.Sequential(torch.nn.Conv1d(3, 8, **first), torch.nn.ReLU(), torch.nn.Conv1d(8, 8, 3, stride=2),
                               torch.nn.Flatten(), torch.nn.Linear(8 * 15, CLASSES)).to(gpu)


@functools.lru_cache(maxsize=None)
def setting1d():
    gpu = torch.device("cuda:0")
    model = make_model1d(gpu)
    gen = torch.Generator().manual_seed(6)
    x, labels = torch.randn(6, 3, 32, generator=gen).to(gpu), torch.tensor([0, 4, 2, 2, 1, 3], device=gpu)
    return model, twin_of(model, gpu), x, labels


KINDS_1D, KINDS_2D = ['Conv1d', 'Linear'], ['Conv2d', 'Linear']


def test_conv1d_model_against_its_conv2d_twin(gpu):
    model, twin, x, labels = setting1d()
    assert rel_fro(twin(x.unsqueeze(2)), model(x)) <= 1e-6
    a = chain(model, KINDS_1D, x, labels)
    b = chain(twin, KINDS_2D, x.unsqueeze(2), labels, eigvecs=[a[3].eigvecs[l] for l in a[0]])
    compare_twins("Conv1d", a, b)
    # and against float64 from the records
    kfac = a[2]
    for layer in a[0]:
        A, G = float64_factors(layer, *kfac.record[layer])
        assert rel_fro(kfac.state[layer][0], A) <= BAR and rel_fro(kfac.state[layer][1], G) <= BAR


def test_conv1d_per_sample_line_against_its_twin(gpu):
    """Diagonal(per_sample=True) and the variance of `evaluate.glm_predictive`: the records are read through their
    (N, C, 1, L) views."""
    from curvature_amd.curvatures import KFAC, Diagonal
    from curvature_amd.evaluate import glm_predictive
    model, twin, x, labels = setting1d()
    out = []
    for m, kinds, xin in ((model, KINDS_1D, x), (twin, KINDS_2D, x.unsqueeze(2))):
        diag, kfac = Diagonal(m, kinds, per_sample=True), KFAC(m, kinds)
        try:
            backward(m, xin, labels)
            diag.update(x.shape[0])
            kfac.update(x.shape[0])
            diag.invert(add=ADD, multiply=MULTIPLY)
            kfac.invert(add=ADD, multiply=MULTIPLY)
            layers = [l for l in m if l.__class__.__name__ in kinds]
            state = [diag.state[l].clone() for l in layers]
            var_d = glm_predictive(m, diag, xin)[1].clone()
            var_k = glm_predictive(m, kfac, xin)[1].clone()
            out.append((state, var_d, var_k))
        finally:
            for est in (diag, kfac):
                for hook in est.hooks:
                    hook.remove()
    (state_a, vd_a, vk_a), (state_b, vd_b, vk_b) = out
    errs = [rel_fro(sa, sb) for sa, sb in zip(state_a, state_b)]
    print(f"Conv1d per-sample Diagonal vs twin: {max(errs):.3e}; glm variance Diagonal {rel2(vd_a, vd_b):.3e}, "
          f"KFAC {rel2(vk_a, vk_b):.3e}")
    assert max(errs) <= BAR
    assert rel2(vd_a, vd_b) <= TOL and rel2(vk_a, vk_b) <= TOL
    assert float(vd_a.min()) > 0 and float(vk_a.min()) > 0
    # the exact Fisher diagonal against N single-sample passes in float64
    ref = make_model1d(torch.device("cpu"), seed=0)
    ref.load_state_dict(model.state_dict())
    ref = ref.double()
    layers = [ref[0], ref[2], ref[4]]
    params = [p for l in layers for p in l.parameters()]
    want = [0, 0, 0]
    for n in range(x.shape[0]):
        loss = F.cross_entropy(ref(x[n:n + 1].double().cpu()), labels[n:n + 1].cpu())
        grads = torch.autograd.grad(loss, params)
        for k in range(3):
            P = torch.cat([grads[2 * k].reshape(grads[2 * k].shape[0], -1), grads[2 * k + 1].reshape(-1, 1)], dim=1) / x.shape[0]
            want[k] = want[k] + x.shape[0] * P ** 2
    for k in range(3):
        assert rel_fro(state_a[k], want[k]) < TOL


def test_conv1d_reduce_and_autocast_against_its_twin(gpu):
    from curvature_amd.curvatures import KFAC
    model, twin, x, labels = setting1d()
    for what, kwargs, autocast in (("reduce", dict(approximation="reduce"), False), ("bf16 autocast", {}, True)):
        states = []
        for m, kinds, xin in ((model, KINDS_1D, x), (twin, KINDS_2D, x.unsqueeze(2))):
            kfac = KFAC(m, kinds, **kwargs)
            try:
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    backward(m, xin, labels)
                if autocast:
                    assert kfac.record[m[2]][0].dtype == torch.bfloat16
                kfac.update(x.shape[0])
                states.append([t for l in m if l.__class__.__name__ in kinds for t in kfac.state[l]])
            finally:
                for hook in kfac.hooks:
                    hook.remove()
        errs = [rel_fro(a, b) for a, b in zip(*states)]
        print(f"Conv1d {what} vs twin: worst {max(errs):.3e}")
        assert max(errs) <= BAR, what
        assert torch.equal(states[0][0], states[1][0]), what                          # the first layer's A factor


def test_dilated_conv1d_a_factor_against_float64(gpu):
    from curvature_amd import ops
    from curvature_amd.curvatures import KFAC
    was = ops.admit_dilated(True)
    try:
        model = make_model1d(gpu, seed=9, kernel_size=3, dilation=2, padding=2)
        gen = torch.Generator().manual_seed(10)
        x, labels = torch.randn(6, 3, 32, generator=gen).to(gpu), torch.tensor([0, 4, 2, 2, 1, 3], device=gpu)
        kfac = KFAC(model, KINDS_1D)
        backward(model, x, labels)
        kfac.update(6)
        A, G = float64_factors(model[0], *kfac.record[model[0]])                      # the Gram of the dilated unfold
        err = rel_fro(kfac.state[model[0]][0], A)
        print(f"dilated Conv1d A factor: rel_fro {err:.3e}")
        assert kfac.state[model[0]][0].shape == (10, 10) and err <= BAR and rel_fro(kfac.state[model[0]][1], G) <= BAR
        for hook in kfac.hooks:
            hook.remove()
    finally:
        ops.admit_dilated(was)
