"""The joint covariance, the Monte-Carlo softmax and the damping grid of grouped and depthwise convolutions on the GPU
(DESIGN.md K15): curv_persample_dw_project, curv_persample_gram_reduce and curv_persample_dw_quad_grid_reduce through
`ops` against float64, then `glm_predictive_joint`, `glm_predictive_mc` and `glm_predictive_grid` on a small model with
one layer of every route, and the joint covariance of MobileNetV2.

Expected values are computed here in float64 on the CPU, from the very records.  The bar is the project's own: relative
Frobenius (matrices) or 2-norm (vectors) error below 1e-4 against float64, `TOL` below; where two float32 results of the
library are compared with each other the same bar holds, and "the same bits" means `torch.equal`."""
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
    was = ops.admit_grouped_per_sample(True), ops.admit_grouped_joint(True)
    yield
    ops.admit_grouped_per_sample(was[0])
    ops.admit_grouped_joint(was[1])


# ------------------------------------------------------------------------------------------------ 1. the entry points
# (C, kernel, stride, padding, (H, W)); all with bias
CASES = {
    "a": (3, 3, 1, 1, (5, 5)),                   # n_g = 10, under one wave
    "b": (2, 7, 1, 3, (9, 9)),                   # n_g = 50, the register ceiling
    "c": (2, 3, 1, 0, (57, 57)),                 # 3 025 outputs: several waves per plane
    "d": (4, 3, 2, 1, (7, 6)),
}


def products64(x, g, kernel, stride, padding):
    """p (N, C, n_g) in float64, bias included: unfold on the channel planes."""
    n, c, h, w = x.shape
    cols = F.unfold(x.double().reshape(n * c, 1, h, w), kernel, padding=padding, stride=stride)     # (N C, kh kw, L)
    gf = g.double().reshape(n * c, -1)
    p = torch.cat([torch.einsum("pkl,pl->pk", cols, gf), gf.sum(1, keepdim=True)], 1)
    return p.reshape(n, c, -1)


@functools.lru_cache(maxsize=None)
def case(name, seed=0):
    """The records of CASES[name] (CPU, float32), their float64 products, and the terms of every form; made once."""
    C, k, s, pad, (H, W) = CASES[name]
    gen = torch.Generator().manual_seed(100 * seed + ord(name))
    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    x, g = torch.randn(N, C, H, W, generator=gen), torch.randn(N, C, Ho, Wo, generator=gen)
    n_g = k * k + 1
    return dict(x=x, g=g, geometry=((k, k), (s, s), (pad, pad), True), p=products64(x, g, (k, k), (s, s), (pad, pad)),
                C=C, n_g=n_g, T=torch.randn(C, n_g, n_g, generator=gen) / n_g ** 0.5, s=torch.randn(C, 1, 1, generator=gen),
                w=torch.rand(C, n_g, generator=gen) + 0.1, u=torch.rand(C, generator=gen),
                v=torch.rand(C, n_g, generator=gen))


def strided_rows(t, gpu, gap=3):
    """`t` (rows, cols) on the GPU as a view with row stride cols + gap into a NaN-filled buffer, and that buffer."""
    buf = torch.full((t.shape[0], t.shape[1] + gap), float("nan"), device=gpu)
    buf[:, :t.shape[1]] = t.to(gpu)
    return buf[:, :t.shape[1]], buf


def project64(c, form):
    p = c["p"]
    if form == "T_s":
        return c["s"].double().reshape(1, -1, 1) * torch.einsum("cij,nci->ncj", c["T"].double(), p)
    return c["w"].double() * p if form == "w" else p


def project_job(c, form, x, g, y, gpu):
    from curvature_amd import ops
    own = {}
    if form == "T_s":
        own = dict(T=c["T"].to(gpu), s=c["s"].to(gpu))
    elif form == "w":
        own = dict(W=strided_rows(c["w"], gpu)[0])                              # row stride n_g + 3, NaN in the gap
    return ops.PerSampleDwProjectJob(x, g, *c["geometry"], y=y, **own)


@pytest.mark.parametrize("form", ["T_s", "w", "none"])
@pytest.mark.parametrize("name", list(CASES))
def test_project_against_float64(gpu, name, form):
    from curvature_amd import ops
    c = case(name)
    E = c["C"] * c["n_g"]
    x, g = c["x"].to(gpu), c["g"].to(gpu)
    buf = torch.full((N, E + 5), float("nan"), device=gpu)                      # y_ns = E + 5 > C n_g
    ops.per_sample_dw_project([project_job(c, form, x, g, buf[:, :E], gpu)])
    want = project64(c, form).reshape(N, E)
    err = rel_fro(buf[:, :E], want)
    print(f"dw project {name} {form}: rel Frobenius error {err:.3e}")
    assert err < TOL
    assert bool(torch.isnan(buf[:, E:]).all())                                  # nothing between the rows is touched
    again = torch.full((N, E), float("nan"), device=gpu)
    ops.per_sample_dw_project([project_job(c, form, x, g, again, gpu)])
    assert torch.equal(again, buf[:, :E])                                       # whatever y_ns: the same bits
    if form == "none":                                                           # phase 1 is that of the quad reduction
        out = torch.empty(N, device=gpu)
        ops.per_sample_dw_quad_reduce([ops.PerSampleDwJob(x, g, *c["geometry"], out=out, first=True)])
        assert rel_fro(out, (again.double() ** 2).sum(1)) < TOL


@pytest.mark.parametrize("E", [1, 50, 257, 9600])
@pytest.mark.parametrize("K", [1, 3, 16])
def test_gram_against_float64(gpu, K, E):
    from curvature_amd import ops
    gen = torch.Generator().manual_seed(7 * K + E)
    Y = torch.randn(K, N, E, generator=gen)
    fence = torch.full((K, N, E + 3), float("nan"), device=gpu)                 # NaN between the rows of Y
    fence[:, :, :E] = Y.to(gpu)
    out = torch.full((N, K, K + 2), float("nan"), device=gpu)                   # o_rs = K + 2 > K
    want = torch.einsum("kne,lne->nkl", Y.double(), Y.double())
    ops.per_sample_gram_reduce([ops.PerSampleGramJob(fence[:, :, :E], out[:, :, :K], alpha=1.5, first=True)])
    err = rel_fro(out[:, :, :K], 1.5 * want)
    print(f"gram K {K} E {E}: rel Frobenius error {err:.3e}")
    assert err < TOL
    assert torch.equal(out[:, :, :K], out[:, :, :K].transpose(1, 2))            # symmetric bit for bit
    ops.per_sample_gram_reduce([ops.PerSampleGramJob(fence[:, :, :E], out[:, :, :K], alpha=2.5, first=False)])
    assert rel_fro(out[:, :, :K], 4.0 * want) < TOL
    assert torch.equal(out[:, :, :K], out[:, :, :K].transpose(1, 2))
    assert bool(torch.isnan(out[:, :, K:]).all())                               # nothing between the entries is touched


def grid64(c, separable, shifts, gains):
    """(H, N) in float64."""
    p = c["p"]
    y = torch.einsum("cij,nci->ncj", c["T"].double(), p) if separable else p
    rows = []
    for shift, gain in zip(shifts, gains):
        # (the float32 values the kernel gets)
        shift, gain = float(torch.tensor(shift, dtype=torch.float32)), float(torch.tensor(gain, dtype=torch.float32))
        if separable:
            w = 1.0 / ((c["u"].double().reshape(-1, 1) + shift) * (c["v"].double() + shift))
        else:
            w = 1.0 / (c["v"].double() + shift)
        rows.append(gain * (w * y * y).sum((1, 2)))
    return torch.stack(rows)


def grid_job(c, separable, x, g, out, shifts, gains, gpu):
    from curvature_amd import ops
    if separable:
        own = dict(T=c["T"].to(gpu), u=c["u"].to(gpu), v=strided_rows(c["v"], gpu)[0])
    else:
        own = dict(V=strided_rows(c["v"], gpu)[0])
    return ops.PerSampleDwGridJob(x, g, *c["geometry"], out=out, shift=shifts, gain=gains, first=True, **own)


SHIFTS = [0.05 * 1.6 ** h for h in range(16)]
GAINS = [1.0 / (1 + h) for h in range(16)]


@pytest.mark.parametrize("separable", [True, False], ids=["separable", "dense"])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_dw_grid_against_float64(gpu, name, separable):
    from curvature_amd import ops
    c = case(name)
    x, g = c["x"].to(gpu), c["g"].to(gpu)
    buf = torch.full((16, N + 2), float("nan"), device=gpu)                     # o_hs = N + 2
    ops.per_sample_dw_quad_grid_reduce([grid_job(c, separable, x, g, buf[:, :N], SHIFTS, GAINS, gpu)])
    want = grid64(c, separable, SHIFTS, GAINS)
    for h in range(16):
        err = rel_fro(buf[h, :N], want[h])
        assert err < TOL, (h, err)
    print(f"dw grid {name} {'separable' if separable else 'dense'}: rel 2-norm error {rel_fro(buf[:, :N], want):.3e}")
    assert bool(torch.isnan(buf[:, N:]).all())
    for h in range(16):                                                          # H = 1 with that pair: the same bits
        one = torch.full((1, N), float("nan"), device=gpu)
        ops.per_sample_dw_quad_grid_reduce([grid_job(c, separable, x, g, one, SHIFTS[h:h + 1], GAINS[h:h + 1], gpu)])
        assert torch.equal(one[0], buf[h, :N]), h
    twice = buf[:, :N].clone()
    job = grid_job(c, separable, x, g, twice, SHIFTS, GAINS, gpu)
    job.first = False
    ops.per_sample_dw_quad_grid_reduce([job])                                    # accumulates
    assert rel_fro(twice, 2 * want) < TOL


def test_seventeen_items_cross_the_launch_boundary(gpu):
    """17 items in one call (16 per launch; 8 per launch of the grid reduction): each has the bits of a call of its own."""
    from curvature_amd import ops
    cases = [case("a", seed) for seed in range(17)]
    records = [(c["x"].to(gpu), c["g"].to(gpu)) for c in cases]
    E = 30
    fresh = lambda *shape: torch.full(shape, float("nan"), device=gpu)
    # project
    alone, together = [fresh(N, E) for _ in cases], [fresh(N, E) for _ in cases]
    for c, (x, g), y in zip(cases, records, alone):
        ops.per_sample_dw_project([project_job(c, "T_s", x, g, y, gpu)])
    ops.per_sample_dw_project([project_job(c, "T_s", x, g, y, gpu) for c, (x, g), y in zip(cases, records, together)])
    for k, (a, b, c) in enumerate(zip(alone, together, cases)):
        assert torch.equal(a, b), k
        assert rel_fro(b, project64(c, "T_s").reshape(N, E)) < TOL
    assert not torch.equal(together[0], together[16])
    # grid, H = 3
    alone, together = [fresh(3, N) for _ in cases], [fresh(3, N) for _ in cases]
    for c, (x, g), out in zip(cases, records, alone):
        ops.per_sample_dw_quad_grid_reduce([grid_job(c, True, x, g, out, SHIFTS[:3], GAINS[:3], gpu)])
    ops.per_sample_dw_quad_grid_reduce([grid_job(c, True, x, g, out, SHIFTS[:3], GAINS[:3], gpu)
                                        for c, (x, g), out in zip(cases, records, together)])
    for k, (a, b, c) in enumerate(zip(alone, together, cases)):
        assert torch.equal(a, b), k
        assert rel_fro(b, grid64(c, True, SHIFTS[:3], GAINS[:3])) < TOL
    # Gram: every number of outputs from 1 to 16, so all compiled-in widths in one call
    stacks = [torch.randn(1 + k % 16, N, E, device=gpu) for k in range(17)]
    alone = [fresh(N, s.shape[0], s.shape[0]) for s in stacks]
    together = [fresh(N, s.shape[0], s.shape[0]) for s in stacks]
    for s, out in zip(stacks, alone):
        ops.per_sample_gram_reduce([ops.PerSampleGramJob(s, out, first=True)])
    ops.per_sample_gram_reduce([ops.PerSampleGramJob(s, out, first=True) for s, out in zip(stacks, together)])
    for k, (a, b, s) in enumerate(zip(alone, together, stacks)):
        assert torch.equal(a, b), k
        assert rel_fro(b, torch.einsum("kne,lne->nkl", s.double().cpu(), s.double().cpu())) < TOL


# ------------------------------------------------------------------------------------------------ 2. a small model
K = 4
HYPERS = [(0.5, 2.0), (0.05, 1.0), ([0.5, 0.3, 0.2, 0.4, 0.6], [2.0, 1.0, 1.5, 0.5, 3.0])]      # one pair of per-layer lists


def small_model():
    """The four-route model of tests/test_per_sample_grouped_gpu.py: plain, groups=2 slices, depthwise, depthwise with a
    channel multiplier (slices), linear head."""
    torch.manual_seed(11)
    nn = torch.nn
    return nn.Sequential(nn.Conv2d(2, 4, 3, padding=1), nn.ReLU(), nn.Conv2d(4, 4, 3, padding=1, groups=2), nn.ReLU(),
                         nn.Conv2d(4, 4, 3, padding=1, groups=4), nn.ReLU(),
                         nn.Conv2d(4, 8, 3, stride=2, padding=1, groups=4), nn.Flatten(), nn.Linear(72, 4)).eval()


def selected(model):
    return [m for m in model if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear))]


def matrix_of_grads(layer):
    w, b = layer.weight.grad, layer.bias.grad
    return torch.cat([w.reshape(w.shape[0], -1), b.reshape(-1, 1)], 1).detach().clone()


@functools.lru_cache(maxsize=None)
def small_case(size=5):
    """The model, a batch of `size` x `size` inputs, and in float64 the Jacobians of the K outputs per sample and selected
    layer as [W | b] matrices; made once and left unchanged.  5 x 5: planes of 25 and 9 values, so every g side is
    packed; 6 x 6: planes of 36 values up to the last convolution, so Diagonal reads those g sides in place - the slices
    of the ``groups=2`` layer then share one copy of its record per staged output."""
    model = small_model()
    gen = torch.Generator().manual_seed(12)
    x, labels = torch.randn(N, 2, size, size, generator=gen), torch.tensor([0, 3, 1])
    m64 = copy.deepcopy(model).double()
    layers = selected(m64)
    jac = []
    for n in range(N):
        rows = []
        for c in range(K):
            m64.zero_grad()
            m64(x[n:n + 1].double())[0, c].backward()
            rows.append([matrix_of_grads(l) for l in layers])
        jac.append(rows)
    return dict(model=model, x=x, labels=labels, jac=jac)


def test_the_small_model_has_one_layer_of_every_route():
    from curvature_amd import ops
    assert [ops.per_sample_route(l) for l in selected(small_model())] == ["whole", "slices", "depthwise", "slices", "whole"]
    assert ops.per_sample_admits_grouped_joint()


def fitted(kind, model, x, labels, invert=True):
    """An estimator of the small model after one update and (unless told otherwise) an inversion under which the float64
    inverse of every damped factor is well conditioned (add 0.5 keeps the condition number of sqrt(multiply) F +
    sqrt(add) I below 100 for this model's factors)."""
    from curvature_amd.curvatures import KFAC, Diagonal
    est = KFAC(model) if kind == "kfac" else Diagonal(model)
    model.zero_grad()
    F.cross_entropy(model(x), labels).backward()
    est.update(x.shape[0])
    if invert:
        est.invert(add=0.5, multiply=2.0)
    return est


def setup(gpu, kind, invert=True, size=5):
    sc = small_case(size)
    model = copy.deepcopy(sc["model"]).to(gpu)
    x, labels = sc["x"].to(gpu), sc["labels"].to(gpu)
    return sc, model, x, fitted(kind, model, x, labels, invert)


def done(est):
    for hook in getattr(est, "hooks", []):
        hook.remove()


def blocks_of(layer, J):
    """The row blocks of a [W | b] matrix that one Kronecker pair covers: one per group."""
    groups = int(getattr(layer, "groups", 1))
    m = J.shape[0] // groups
    return [J[g * m:(g + 1) * m] for g in range(groups)]


def covariance64(kind, model, jac, sigma):
    """J Sigma J^T per sample in float64, (N, K, K).  ``sigma(k, layer)``: KFAC - per group the pair (S_G, S_A) of the
    covariance S_G kron S_A; Diagonal - the (m, n) matrix of variances."""
    want = torch.zeros(N, K, K, dtype=torch.float64)
    for k, layer in enumerate(selected(model)):
        S = sigma(k, layer)
        for n in range(N):
            if kind == "kfac":
                # <J_c, S_G J_c' S_A> summed over the groups
                left = [blocks_of(layer, jac[n][c][k]) for c in range(K)]
                right = [[S_G @ B @ S_A for B, (S_G, S_A) in zip(blocks, S)] for blocks in left]
                for c in range(K):
                    for d in range(K):
                        want[n, c, d] += sum(float((a * b).sum()) for a, b in zip(left[c], right[d]))
            else:
                for c in range(K):
                    for d in range(K):
                        want[n, c, d] += float((S * jac[n][c][k] * jac[n][d][k]).sum())
    return want


def posterior64(kind, est):
    """`sigma` of `covariance64` from the estimator's inverse state."""
    def sigma(k, layer):
        if kind == "diag":
            return est.inv_state[layer].double().cpu() ** 2
        L_A, L_G = (t.double().cpu() for t in est.inv_state[layer])
        if L_A.dim() == 2:
            L_A, L_G = L_A.unsqueeze(0), L_G.unsqueeze(0)
        return [(g @ g.t(), a @ a.t()) for a, g in zip(L_A, L_G)]
    return sigma


def damped64(kind, est, model, add, multiply):
    """`sigma` of `covariance64` from the estimator's state, damped by the pair (add, multiply) in float64:
    KFAC (sqrt(s) F + sqrt(n) I)^-1 on both sides, Diagonal 1 / (s state + n); lists are per selected layer."""
    def sigma(k, layer):
        n, s = (add[k], multiply[k]) if isinstance(add, list) else (add, multiply)
        if kind == "diag":
            return 1.0 / (s * est.state[layer].double().cpu() + n)
        A, G = (t.double().cpu() for t in est.state[layer])
        if A.dim() == 2:
            A, G = A.unsqueeze(0), G.unsqueeze(0)
        inv = lambda M: torch.linalg.inv(s ** 0.5 * M + n ** 0.5 * torch.eye(M.shape[0], dtype=torch.float64))
        return [(inv(g), inv(a)) for a, g in zip(A, G)]
    return sigma


@pytest.mark.parametrize("size", [5, 6])
@pytest.mark.parametrize("kind", ["kfac", "diag"])
def test_joint_covariance_against_float64_jacobians(gpu, kind, size):
    from curvature_amd import ops
    from curvature_amd.evaluate import glm_predictive, glm_predictive_joint
    sc, model, x, est = setup(gpu, kind, size=size)
    in_place = [ops.per_sample_operands(item, torch.empty(N, 4, size, size), torch.empty(N, 4, size, size)).g.pack is None
                for item in ops.GroupSlice.of(model[2])]
    assert in_place == [size == 6] * 2                                           # (what the two sizes are there for)
    logits, covariance, probs = glm_predictive_joint(model, est, x)
    want = covariance64(kind, model, sc["jac"], posterior64(kind, est))
    err = rel_fro(covariance, want)
    print(f"glm_predictive_joint {kind} {size}x{size}: rel Frobenius error of the covariances {err:.3e}")
    assert err < TOL
    for n in range(N):                                                           # ... and of every sample on its own
        assert rel_fro(covariance[n], want[n]) < TOL
    assert torch.equal(covariance, covariance.transpose(1, 2))
    variance = glm_predictive(model, est, x)[1]                                  # the other reduction, the same estimator
    assert rel_fro(torch.diagonal(covariance, dim1=1, dim2=2), variance) < TOL
    assert not est.__dict__.get("_predictive_kept")                              # nothing is left behind
    done(est)


@pytest.mark.parametrize("kind", ["kfac", "diag"])
def test_mc_softmax_over_the_joint_covariance(gpu, kind):
    from curvature_amd.evaluate import glm_predictive_joint, glm_predictive_mc, mc_softmax
    sc, model, x, est = setup(gpu, kind)
    joint = glm_predictive_joint(model, est, x)[1]
    noise = torch.randn(N, 64, K, generator=torch.Generator().manual_seed(5)).to(gpu)
    logits, covariance, probs = glm_predictive_mc(model, est, x, samples=64, noise=noise)
    assert torch.equal(covariance, joint)                                        # the same passes, the same bits
    assert rel_fro(covariance, covariance64(kind, model, sc["jac"], posterior64(kind, est))) < TOL
    assert torch.allclose(probs.sum(1), torch.ones(N, device=gpu), atol=1e-5)
    again, _ = mc_softmax(logits, covariance, list(range(K)), 64, noise=noise)
    assert torch.equal(probs, again)
    drawn = glm_predictive_mc(model, est, x, samples=64)[2]                      # the estimator's own noise stream
    assert torch.allclose(drawn.sum(1), torch.ones(N, device=gpu), atol=1e-5)
    done(est)


@pytest.mark.parametrize("size", [5, 6])
@pytest.mark.parametrize("kind", ["kfac", "diag"])
def test_grid_against_float64_and_against_an_inversion_per_pair(gpu, kind, size):
    from curvature_amd.evaluate import glm_predictive_grid
    sc, model, x, est = setup(gpu, kind, invert=False, size=size)
    if kind == "kfac":
        est.decompose()
    logits, variance, probs = glm_predictive_grid(model, est, x, HYPERS)
    assert tuple(variance.shape) == (len(HYPERS), N, K)
    if kind == "diag":
        est._record_per_sample("Diagonal")
    params = list(model.parameters())
    for h, (add, multiply) in enumerate(HYPERS):
        want = torch.diagonal(covariance64(kind, model, sc["jac"], damped64(kind, est, model, add, multiply)), dim1=1, dim2=2)
        err = rel_fro(variance[h], want)
        print(f"glm_predictive_grid {kind} {size}x{size} pair {h}: rel 2-norm error {err:.3e}")
        assert err < TOL
        est.invert(add=add, multiply=multiply)                                   # ... and an inversion with that pair
        out = model(x)
        direct = torch.empty(N, K, device=gpu)
        for c in range(K):
            torch.autograd.grad(out[:, c].sum(), params, retain_graph=True)
            est.functional_variance(direct[:, c], inputs=c == 0)
        assert rel_fro(variance[h], direct) < TOL
    est.drop_predictive_state()
    done(est)


@pytest.mark.parametrize("kind", ["kfac", "diag"])
def test_restaging_gives_the_same_bits_and_a_new_forward_pass_needs_inputs(gpu, kind):
    sc, model, x, est = setup(gpu, kind)
    if kind == "diag":
        est._record_per_sample("Diagonal")
    params = list(model.parameters())
    logits = model(x)

    def stage(inputs_first):
        for c in range(K):
            torch.autograd.grad(logits[:, c].sum(), params, retain_graph=True)
            est.stage_output(c, K, inputs=inputs_first and c == 0)
    first, second = torch.empty(N, K, K, device=gpu), torch.empty(N, K, K, device=gpu)
    stage(True)
    est.functional_covariance(first)
    stage(False)                                                                 # the same outputs staged again
    est.functional_covariance(second)
    assert torch.equal(first, second)
    assert rel_fro(first, covariance64(kind, model, sc["jac"], posterior64(kind, est))) < TOL
    logits = model(x)                                                            # a new forward pass: other input tensors
    torch.autograd.grad(logits[:, 0].sum(), params, retain_graph=True)
    with pytest.raises(RuntimeError, match="inputs=True"):
        est.stage_output(0, K)
    with pytest.raises(RuntimeError, match="recorded inputs are no longer those"):
        est.functional_covariance(second)
    est.drop_predictive_state()
    done(est)


def test_tune_glm_and_eval_glm_mc_take_the_small_model(gpu):
    """The two drivers on top: `tune_glm` is `glm_predictive_grid` per batch, ``eval_glm(predictive="mc")`` is
    `glm_predictive_mc` per batch."""
    from curvature_amd.evaluate import eval_glm, glm_predictive_grid, tune_glm
    sc, model, x, est = setup(gpu, "kfac")
    est.decompose()
    labels = sc["labels"].to(gpu)
    tuned = tune_glm(model, [(x, labels)], est, HYPERS)
    probs = glm_predictive_grid(model, est, x, HYPERS)[2]
    want = -torch.log(probs[:, torch.arange(N, device=gpu), labels].double()).mean(1).cpu()
    assert torch.allclose(tuned["nll"], want, rtol=1e-6) and tuned["best"] == int(torch.argmin(want))
    predictions, seen = eval_glm(model, [(x, labels)], est, predictive="mc", samples=32)
    assert predictions.shape == (N, K) and abs(predictions.sum(1) - 1).max() < 1e-5 and list(seen) == labels.tolist()
    done(est)


def test_joint_switch_off_the_old_refusal_returns(gpu):
    from curvature_amd import ops
    from curvature_amd.evaluate import glm_predictive_grid, glm_predictive_joint, glm_predictive_mc
    sc, model, x, est = setup(gpu, "kfac")
    est.decompose()
    was = ops.admit_grouped_joint(False)
    try:
        text = (r"layer '2' is not supported \(grouped convolution \(groups=2\); Diagonal\(per_sample=True\) and "
                r"functional_variance take it\); select other layer types$")
        for call in (lambda: glm_predictive_joint(model, est, x), lambda: glm_predictive_mc(model, est, x),
                     lambda: glm_predictive_grid(model, est, x, HYPERS[:1])):
            with pytest.raises(NotImplementedError, match=text):
                call()
        est.decompose()                                                          # ... and leaves the stacked factors out
        assert set(est._decomposition) == {model[0], model[8]}
    finally:
        ops.admit_grouped_joint(was)
    done(est)


def test_decompose_keeps_stacked_factors_stacked(gpu):
    sc, model, x, est = setup(gpu, "kfac", invert=False)
    est.decompose()
    assert set(est._decomposition) == set(selected(model))
    for layer in selected(model):
        A, G = est.state[layer]
        kept = est._decomposition[layer]
        U_Gt, U_At, lam_G, lam_A = kept[:4]
        assert U_Gt.shape == G.shape and U_At.shape == A.shape and lam_G.shape == G.shape[:-1] and lam_A.shape == A.shape[:-1]
        assert bool((lam_G >= 0).all()) and bool((lam_A >= 0).all())
        for U_t, lam, factor in ((U_Gt, lam_G, G), (U_At, lam_A, A)):            # F = U diag(lambda) U^T, per group
            U = U_t.double().transpose(-1, -2)
            assert rel_fro(U @ torch.diag_embed(lam.double()) @ U.transpose(-1, -2), factor.double()) < TOL
        assert len(kept) == (5 if layer is model[4] else 4)                      # the depthwise layer: U_A as well
    assert torch.equal(est._decomposition[model[4]][4], est._decomposition[model[4]][1].transpose(1, 2))
    done(est)


# ------------------------------------------------------------------------------------------------ 3. a whole model
def test_mobilenet_v2_joint_covariance(gpu):
    """17 depthwise layers (two launch batches) among 35 plain ones: the diagonal of the joint covariance against the
    variance of `glm_predictive`, Diagonal with a positive random state."""
    from curvature_amd import models, ops
    from curvature_amd.curvatures import Diagonal
    from curvature_amd.evaluate import glm_predictive, glm_predictive_joint
    torch.manual_seed(21)
    model = models.mobilenet_v2(num_classes=10).to(gpu).eval()
    est = Diagonal(model, "Conv2d")
    convs = [m for m in model.modules() if isinstance(m, torch.nn.Conv2d)]
    assert sum(ops.per_sample_route(l) == "depthwise" for l in convs) == 17
    for layer in convs:
        shape = (layer.out_channels, layer.weight[0].numel() + int(layer.bias is not None))
        est.state[layer] = torch.rand(shape, device=gpu) + 0.5
    est.invert(add=1.0, multiply=1.0)
    x = torch.randn(2, 3, 32, 32, device=gpu)                                    # 32 x 32: the last stage is 1 x 1
    outputs = [0, 3, 7]
    logits, covariance, probs = glm_predictive_joint(model, est, x, outputs=outputs)
    variance = glm_predictive(model, est, x, outputs=outputs)[1][:, outputs]
    assert bool(torch.isfinite(covariance).all()) and bool((variance > 0).all())
    err = rel_fro(torch.diagonal(covariance, dim1=1, dim2=2), variance)
    print(f"mobilenet_v2: rel 2-norm error of the covariance diagonal against the variance {err:.3e}")
    assert err < TOL
    assert torch.equal(covariance, covariance.transpose(1, 2))
    eig = torch.linalg.eigvalsh(covariance.double().cpu())
    assert bool((eig > -1e-6 * eig.max()).all())                                 # positive semi-definite
