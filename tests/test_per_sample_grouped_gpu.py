"""Grouped and depthwise convolutions in the per-sample line on the GPU: the direct kernel of
csrc/persample_dw.hip through `ops` against float64, the exact Fisher diagonal and the linearised predictive of a small
model with one layer of every route, and MobileNetV2 / ResNeXt-50.

Expected values are computed here in float64 on the CPU, from the very records.  Bars: matrices - the project's 1e-4
relative Frobenius error against float64; per-sample variances - `TOL` of tests/test_glm_predictive_gpu.py, relative
2-norm error below 1e-4 against float64."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_fro

pytestmark = pytest.mark.gpu
TOL = 1e-4
N = 3


@pytest.fixture(autouse=True)
def admitted():
    from curvature_amd import ops
    was = ops.admit_grouped_per_sample(True)
    yield
    ops.admit_grouped_per_sample(was)


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


# ------------------------------------------------------------------------------------------------ 1. the direct kernel
# (C, kernel, stride, padding, (H, W), bias)
CASES = [
    (3, 3, 1, 1, (5, 5), True),                  # L = 25: under one wave, not a multiple of 4
    (4, 3, 2, 1, (7, 6), True),
    (2, 5, 1, 2, (9, 9), False),
    (2, 7, 1, 3, (9, 9), True),                  # n_g = 50, the register ceiling
    (5, 1, 1, 0, (4, 4), True),
    (3, (3, 1), (1, 2), (1, 0), (6, 7), True),
    (2, 3, 1, 0, (57, 57), True),                # 3 025 outputs: several waves per plane, odd rows
    (2, 3, 2, 1, (112, 112), False),             # MobileNetV2's first depthwise plane
]
IDS = ["5x5", "7x6s2", "9x9k5", "9x9k7", "4x4k1", "6x7k3x1", "57x57", "112x112s2"]


def products64(x, g, kernel, stride, padding, bias):
    """p (N, C, n_g) in float64: unfold on the channel planes."""
    n, c, h, w = x.shape
    cols = F.unfold(x.double().reshape(n * c, 1, h, w), kernel, padding=padding, stride=stride)     # (N C, kh kw, L)
    gf = g.double().reshape(n * c, -1)
    p = torch.einsum("pkl,pl->pk", cols, gf)
    if bias:
        p = torch.cat([p, gf.sum(1, keepdim=True)], 1)
    return p.reshape(n, c, -1)


@functools.lru_cache(maxsize=None)
def case(index, seed=0):
    """The records of CASES[index] (CPU, float32) and their float64 products; made once."""
    C, kernel, stride, padding, (H, W), bias = CASES[index]
    kernel, stride, padding = pair(kernel), pair(stride), pair(padding)
    gen = torch.Generator().manual_seed(1000 * seed + index)
    Ho, Wo = ((H + 2 * padding[0] - kernel[0]) // stride[0] + 1, (W + 2 * padding[1] - kernel[1]) // stride[1] + 1)
    x, g = torch.randn(N, C, H, W, generator=gen), torch.randn(N, C, Ho, Wo, generator=gen)
    return dict(x=x, g=g, geometry=(kernel, stride, padding, bias), p=products64(x, g, kernel, stride, padding, bias))


def fenced(t, gpu):
    """`t` on the GPU, cut from the middle of a larger NaN-filled buffer."""
    buf = torch.full((t.numel() + 2 * 333,), float("nan"), device=gpu)
    view = buf[333:333 + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def sq_job(c, x, g, dst, alpha, first):
    from curvature_amd import ops
    return ops.PerSampleDwJob(x, g, *c["geometry"], dst=dst, alpha=alpha, first=first)


def nan_matrix(rows, cols, gpu):
    """A (rows, cols) view with row stride cols + 3 into a NaN-filled buffer."""
    return torch.full((rows, cols + 3), float("nan"), device=gpu)[:, :cols]


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_dw_sq_against_float64(gpu, index):
    from curvature_amd import ops
    c = case(index)
    x, g = c["x"].to(gpu), c["g"].to(gpu)
    want = (c["p"] ** 2).sum(0)
    dst = nan_matrix(*want.shape, gpu)
    ops.per_sample_dw_sq_accumulate([sq_job(c, x, g, dst, 1.5, True)])           # `first` overwrites the NaNs
    err = rel_fro(dst, 1.5 * want)
    print(f"dw sq {IDS[index]}: rel Frobenius error {err:.3e}")
    assert err < TOL
    once = dst.clone()
    ops.per_sample_dw_sq_accumulate([sq_job(c, x, g, dst, 2.5, False)])          # accumulates onto it
    assert rel_fro(dst, 4.0 * want) < TOL
    again = nan_matrix(*want.shape, gpu)
    ops.per_sample_dw_sq_accumulate([sq_job(c, x, g, again, 1.5, True)])         # the same call twice: the same bits
    assert torch.equal(again, once)
    flops, nbytes = ops.per_sample_dw_plan_info([sq_job(c, x, g, None, 1.0, True)])
    assert flops[0] == 2 * g.numel() * want.shape[1] and nbytes[0] == 4 * (x.numel() + g.numel())


def test_dw_channels_last_records(gpu):
    """Both records as channels_last views (the per-element path) against float64 and against the contiguous run."""
    from curvature_amd import ops
    c = case(6)
    want = (c["p"] ** 2).sum(0)
    x, g = c["x"].to(gpu), c["g"].to(gpu)
    plain, last = nan_matrix(*want.shape, gpu), nan_matrix(*want.shape, gpu)
    ops.per_sample_dw_sq_accumulate([sq_job(c, x, g, plain, 1.0, True)])
    xl, gl = x.contiguous(memory_format=torch.channels_last), g.contiguous(memory_format=torch.channels_last)
    assert xl.stride(3) == 2 and gl.stride(1) == 1
    ops.per_sample_dw_sq_accumulate([sq_job(c, xl, gl, last, 1.0, True)])
    assert rel_fro(last, want) < TOL and rel_fro(last, plain) < TOL


@pytest.mark.parametrize("index", [2, 3], ids=["9x9k5", "9x9k7"])
def test_dw_records_inside_a_nan_filled_buffer(gpu, index):
    from curvature_amd import ops
    c = case(index)
    want = (c["p"] ** 2).sum(0)
    dst = nan_matrix(*want.shape, gpu)
    ops.per_sample_dw_sq_accumulate([sq_job(c, fenced(c["x"], gpu), fenced(c["g"], gpu), dst, 1.0, True)])
    assert bool(torch.isfinite(dst).all())
    assert rel_fro(dst, want) < TOL
    out = torch.full((N, 4), float("nan"), device=gpu)
    ops.per_sample_dw_quad_reduce([ops.PerSampleDwJob(fenced(c["x"], gpu), fenced(c["g"], gpu), *c["geometry"],
                                                      out=out[:, 1], first=True)])
    assert bool(torch.isfinite(out[:, 1]).all()) and rel_fro(out[:, 1], (c["p"] ** 2).sum((1, 2))) < TOL


def test_dw_seventeen_layers_cross_the_launch_boundary(gpu):
    """17 items in one call (16 per launch): each has the bits of a call of its own."""
    cases = [case(0, seed) for seed in range(17)]
    from curvature_amd import ops
    records = [(c["x"].to(gpu), c["g"].to(gpu)) for c in cases]
    alone = []
    for c, (x, g) in zip(cases, records):
        dst = nan_matrix(3, 10, gpu)
        ops.per_sample_dw_sq_accumulate([sq_job(c, x, g, dst, 1.0, True)])
        alone.append(dst)
    together = [nan_matrix(3, 10, gpu) for _ in cases]
    ops.per_sample_dw_sq_accumulate([sq_job(c, x, g, dst, 1.0, True) for c, (x, g), dst in zip(cases, records, together)])
    for k, (a, b, c) in enumerate(zip(alone, together, cases)):
        assert torch.equal(a, b), k
        assert rel_fro(b, (c["p"] ** 2).sum(0)) < TOL
    assert not torch.equal(together[0], together[16])


@pytest.mark.parametrize("form", ["W", "T_s", "none"])
@pytest.mark.parametrize("index", [1, 3, 6], ids=["7x6s2", "9x9k7", "57x57"])
def test_dw_quad_against_float64(gpu, index, form):
    from curvature_amd import ops
    c = case(index)
    p = c["p"]
    C, n_g = p.shape[1:]
    gen = torch.Generator().manual_seed(77 + index)
    T = W = s = None
    y = p
    if form == "W":
        wide = torch.full((C, n_g + 2), float("nan"))
        wide[:, :n_g] = torch.rand(C, n_g, generator=gen) + 0.1
        W = wide.to(gpu)[:, :n_g]                                               # row stride n_g + 2, NaN in the gap
        want = (wide[:, :n_g].double() * p * p).sum((1, 2))
    elif form == "T_s":
        T = torch.tril(torch.randn(C, n_g, n_g, generator=gen))
        s = torch.randn(C, 1, 1, generator=gen)
        y = torch.einsum("cij,nci->ncj", T.double(), p)
        want = (s.double().reshape(1, C, 1) ** 2 * y * y).sum((1, 2))
        T, s = T.to(gpu), s.to(gpu)
    else:
        want = (p * p).sum((1, 2))
    x, g = c["x"].to(gpu), c["g"].to(gpu)
    mat = torch.full((N, 4), float("nan"), device=gpu)
    mat[:, 3] = 7.0
    job = lambda alpha, first: ops.PerSampleDwJob(x, g, *c["geometry"], out=mat[:, 2], T=T, W=W, s=s, alpha=alpha, first=first)
    ops.per_sample_dw_quad_reduce([job(1.5, True)])
    err = rel_fro(mat[:, 2], 1.5 * want)
    print(f"dw quad {IDS[index]} {form}: rel 2-norm error {err:.3e}")
    assert err < TOL
    ops.per_sample_dw_quad_reduce([job(2.5, False)])
    assert rel_fro(mat[:, 2], 4.0 * want) < TOL
    assert bool(torch.isnan(mat[:, :2]).all()) and bool((mat[:, 3] == 7.0).all())       # the other columns are untouched


# ------------------------------------------------------------------------------------------------ 2. a small model
def small_model():
    torch.manual_seed(11)
    nn = torch.nn
    return nn.Sequential(nn.Conv2d(2, 4, 3, padding=1), nn.ReLU(), nn.Conv2d(4, 4, 3, padding=1, groups=2), nn.ReLU(),
                         nn.Conv2d(4, 4, 3, padding=1, groups=4), nn.ReLU(),
                         nn.Conv2d(4, 8, 3, stride=2, padding=1, groups=4), nn.Flatten(), nn.Linear(72, 4)).eval()


def selected(model):
    return [m for m in model if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear))]


def matrix_of(layer, grads=False):
    w = layer.weight.grad if grads else layer.weight
    b = layer.bias.grad if grads else layer.bias
    return torch.cat([w.reshape(w.shape[0], -1), b.reshape(-1, 1)], 1).detach().clone()


@functools.lru_cache(maxsize=None)
def small_case():
    """The model, a batch, and in float64: the per-sample gradients of the mean cross-entropy and the Jacobians of the
    outputs, per selected layer as [W | b] matrices; made once and left unchanged."""
    model = small_model()
    gen = torch.Generator().manual_seed(12)
    x, labels = torch.randn(N, 2, 5, 5, generator=gen), torch.tensor([0, 3, 1])
    m64 = copy.deepcopy(model).double()
    layers = selected(m64)
    per_sample, jac = [], []
    for n in range(N):
        m64.zero_grad()
        (F.cross_entropy(m64(x[n:n + 1].double()), labels[n:n + 1], reduction="sum") / N).backward()
        per_sample.append([matrix_of(l, grads=True) for l in layers])
        rows = []
        for c in range(4):
            m64.zero_grad()
            m64(x[n:n + 1].double())[0, c].backward()
            rows.append([matrix_of(l, grads=True) for l in layers])
        jac.append(rows)
    return dict(model=model, x=x, labels=labels, per_sample=per_sample, jac=jac)


def test_the_small_model_has_one_layer_of_every_route():
    from curvature_amd import ops
    assert [ops.per_sample_route(l) for l in selected(small_model())] == ["whole", "slices", "depthwise", "slices", "whole"]


def test_diagonal_update_against_float64(gpu):
    from curvature_amd.curvatures import Diagonal
    sc = small_case()
    model = copy.deepcopy(sc["model"]).to(gpu)
    est = Diagonal(model, per_sample=True)
    F.cross_entropy(model(sc["x"].to(gpu)), sc["labels"].to(gpu)).backward()
    est.update(N)
    for k, layer in enumerate(selected(model)):
        want = N * sum(sc["per_sample"][n][k] ** 2 for n in range(N))
        assert tuple(est.state[layer].shape) == tuple(want.shape)
        err = rel_fro(est.state[layer], want)
        print(f"Diagonal per-sample state, layer {k}: rel Frobenius error {err:.3e}")
        assert err < TOL
    once = {l: est.state[l].clone() for l in selected(model)}
    est.update(N)                                                                # the same records again: accumulated
    for layer in selected(model):
        assert rel_fro(est.state[layer], 2 * once[layer]) < 1e-6
    for hook in est.hooks:
        hook.remove()


def test_diagonal_at_batch_size_one_agrees_with_the_default_update(gpu):
    from curvature_amd.curvatures import Diagonal
    sc = small_case()
    model = copy.deepcopy(sc["model"]).to(gpu)
    exact, default = Diagonal(model, per_sample=True), Diagonal(model)
    F.cross_entropy(model(sc["x"][:1].to(gpu)), sc["labels"][:1].to(gpu)).backward()
    exact.update(1)
    default.update(1)
    for layer in selected(model):
        assert rel_fro(exact.state[layer], default.state[layer]) < TOL
    for hook in exact.hooks:
        hook.remove()


def fitted(kind, model, x, labels):
    """An estimator of the small model after one update and an inversion with hyper-parameters under which the float64
    inverse of every damped factor is well conditioned (the factors of this model have eigenvalues up to a few units; add
    0.5 keeps the condition number of sqrt(multiply) F + sqrt(add) I below 100)."""
    from curvature_amd.curvatures import KFAC, Diagonal
    est = KFAC(model) if kind == "kfac" else Diagonal(model)
    model.zero_grad()
    F.cross_entropy(model(x), labels).backward()
    est.update(x.shape[0])
    est.invert(add=0.5, multiply=2.0)
    return est


def variance64(kind, est, model, jac):
    """J Sigma J^T per (sample, output) in float64, Sigma the covariance the estimator samples from: per layer and group
    (L_G L_G^T) kron (L_A L_A^T), or diag(inv**2)."""
    want = torch.zeros(N, 4, dtype=torch.float64)
    for k, layer in enumerate(selected(model)):
        groups = int(getattr(layer, "groups", 1))
        if kind == "kfac":
            L_A, L_G = (t.double().cpu() for t in est.inv_state[layer])
            if groups == 1:
                L_A, L_G = L_A.unsqueeze(0), L_G.unsqueeze(0)
            m = L_G.shape[-1]
        for n in range(N):
            for c in range(4):
                J = jac[n][c][k]
                if kind == "kfac":
                    want[n, c] += sum(float((L_G[g].t() @ J[g * m:(g + 1) * m] @ L_A[g]).pow(2).sum()) for g in range(groups))
                else:
                    want[n, c] += float((est.inv_state[layer].double().cpu() ** 2 * J * J).sum())
    return want


@pytest.mark.parametrize("kind", ["kfac", "diag"])
def test_glm_predictive_against_float64_jacobians(gpu, kind):
    from curvature_amd.evaluate import glm_predictive
    sc = small_case()
    model = copy.deepcopy(sc["model"]).to(gpu)
    x, labels = sc["x"].to(gpu), sc["labels"].to(gpu)
    est = fitted(kind, model, x, labels)
    logits, variance, probs = glm_predictive(model, est, x)
    want = variance64(kind, est, model, sc["jac"])
    err = rel_fro(variance, want)
    print(f"glm_predictive {kind}: rel 2-norm error of the variances {err:.3e}")
    assert err < TOL
    for n in range(N):                                                           # ... and of every sample on its own
        assert rel_fro(variance[n], want[n]) < TOL
    assert torch.allclose(probs.sum(1), torch.ones(N, device=gpu), atol=1e-5)
    # nothing is left behind: no kept state; a Diagonal built without per_sample gave its borrowed hooks back
    assert not est.__dict__.get("_predictive_kept")
    if kind == "diag":
        assert not hasattr(est, "hooks") and not hasattr(est, "record")
        assert all(not l._forward_pre_hooks and not l._forward_hooks for l in selected(model))
    else:
        for hook in est.hooks:
            hook.remove()


@pytest.mark.parametrize("kind", ["kfac", "diag"])
def test_inputs_false_gives_the_same_bits(gpu, kind):
    sc = small_case()
    model = copy.deepcopy(sc["model"]).to(gpu)
    x, labels = sc["x"].to(gpu), sc["labels"].to(gpu)
    est = fitted(kind, model, x, labels)
    if kind == "diag":
        est._record_per_sample("Diagonal")
    params = list(model.parameters())
    logits = model(x)
    out = torch.empty(3, N, device=gpu)
    torch.autograd.grad(logits[:, 1].sum(), params, retain_graph=True)
    est.functional_variance(out[0], inputs=True)
    torch.autograd.grad(logits[:, 2].sum(), params, retain_graph=True)
    est.functional_variance(out[1], inputs=False)
    est.functional_variance(out[2], inputs=True)
    assert torch.equal(out[1], out[2]) and not torch.equal(out[0], out[1])
    want = variance64(kind, est, model, sc["jac"])
    assert rel_fro(out[0], want[:, 1]) < TOL and rel_fro(out[1], want[:, 2]) < TOL
    model(x)                                                                     # a new forward pass: other input tensors
    with pytest.raises(RuntimeError, match="inputs=True"):
        est.functional_variance(out[1], inputs=False)
    est.drop_predictive_state()
    for hook in est.hooks:
        hook.remove()


def test_switch_off_the_small_model_is_refused_as_before(gpu):
    from curvature_amd import ops
    from curvature_amd.evaluate import glm_predictive
    sc = small_case()
    model = copy.deepcopy(sc["model"]).to(gpu)
    x, labels = sc["x"].to(gpu), sc["labels"].to(gpu)
    est = fitted("kfac", model, x, labels)
    was = ops.admit_grouped_per_sample(False)
    try:
        with pytest.raises(NotImplementedError, match=r"layer '2' is not supported \(grouped convolution \(groups=2\)\); "
                                                      "select other layer types$"):
            glm_predictive(model, est, x)
    finally:
        ops.admit_grouped_per_sample(was)
    for hook in est.hooks:
        hook.remove()


# ------------------------------------------------------------------------------------------------ 3. whole models
def state64(layer, x, g, n_samples):
    """N sum_n P_n**2 of a (grouped) Conv2d in float64 from its records: unfold on the channel slices."""
    G = int(layer.groups)
    x, g = x.double().cpu(), g.double().cpu()
    n = x.shape[0]
    cols = F.unfold(x, layer.kernel_size, padding=layer.padding, stride=layer.stride)           # (N, C kh kw, L)
    cols = cols.reshape(n, G, -1, cols.shape[-1])
    gs = g.reshape(n, G, layer.out_channels // G, -1)
    P = torch.einsum("ngml,ngkl->ngmk", gs, cols)
    if layer.bias is not None:
        P = torch.cat([P, gs.sum(-1, keepdim=True)], -1)
    return n_samples * (P ** 2).sum(0).reshape(layer.out_channels, -1)


@pytest.mark.parametrize("name", ["mobilenet_v2", "resnext50_32x4d"])
def test_whole_model_diagonal(gpu, name):
    from curvature_amd import models, ops
    from curvature_amd.curvatures import Diagonal
    torch.manual_seed(21)
    model = getattr(models, name)(num_classes=10).to(gpu).eval()
    est = Diagonal(model, "Conv2d", per_sample=True)
    x, labels = torch.randn(2, 3, 64, 64, device=gpu), torch.tensor([1, 7], device=gpu)
    F.cross_entropy(model(x), labels).backward()
    est.update(2)
    convs = [m for m in model.modules() if isinstance(m, torch.nn.Conv2d)]
    grouped = [l for l in convs if l.groups > 1]
    routes = {ops.per_sample_route(l) for l in grouped}
    if name == "mobilenet_v2":
        assert len(grouped) == 17 and routes == {"depthwise"}                    # two launch batches
    else:
        assert len(grouped) == 16 and routes == {"slices"} and all(l.groups == 32 for l in grouped)
    plain = [l for l in convs if l.groups == 1]
    worst = 0.0
    for layer in grouped + [plain[0], plain[len(plain) // 2], plain[-1]]:
        want = state64(layer, *est.record[layer], 2)
        got = est.state[layer]
        assert tuple(got.shape) == tuple(want.shape) and bool(torch.isfinite(got).all())
        err = rel_fro(got, want)
        worst = max(worst, err)
        assert err < TOL, (layer, err)
    print(f"{name}: worst rel Frobenius error of a layer's state {worst:.3e}")
    for hook in est.hooks:
        hook.remove()
