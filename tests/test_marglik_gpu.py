"""The Laplace evidence on the GPU: `Curvature.log_det_grid` of every estimator against the float64 formula evaluated on the
estimator's own tensors (the reduction) and against `torch.linalg.slogdet` of the dense regularised precision built from the
float32 `state` (the meaning), its preconditions, `log_prior_grid`, and `evaluate.log_marginal_likelihood`.

The model is LeNet-class with two layers, Conv2d(1, 4, 3) on 8 x 8 inputs, a 2 x 2 pooling and Linear(36, 10), batch 8: the
factors are 4, 10, 10 and 37 wide, the blocks of BlockDiagonal 40 and 370 - all within the widths (up to 1024) for which
`ops.eigh` promises off(A) <= 1e-8 ||A||, so the eigenvalue yardstick of tests/eigh_refs.py applies."""
import functools
import math

import pytest
import torch

import eigh_refs
import inf_predictive_refs as inf_refs
import logdet_refs as R

pytestmark = pytest.mark.gpu

N = 8
KINDS = ["diag", "efb", "kfac", "block", "inf"]
RANK = 4
# three pairs, one of them with per-layer lists (two layers)
HYPERS = [(1e-2, 1.0), (1.0, 60.0), ([10.0, 0.5], [6e4, 30.0])]
MEANING = [(1e-2, 1.0), (1.0, 60.0), (10.0, 6e4)]
EIG_FACTOR = 4.0                 # FACTOR of tests/test_eigh_direct_gpu.py


def make_model(gpu, conv_bias=True):
    torch.manual_seed(11)
    return torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3, bias=conv_bias), torch.nn.ReLU(), torch.nn.MaxPool2d(2),
                               torch.nn.Flatten(), torch.nn.Linear(36, 10)).to(gpu).eval()


def matrix_layers(model):
    return [l for l in model if isinstance(l, (torch.nn.Conv2d, torch.nn.Linear))]


def batch(gpu, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(N, 1, 8, 8, generator=gen).to(gpu), torch.randint(0, 10, (N,), generator=gen).to(gpu)


def build_chain(gpu, conv_bias=True):
    """Every estimator after one update on one batch (KFAC decomposed, INF at rank 4), nothing inverted, no hooks left."""
    from curvature_amd.curvatures import EFB, INF, KFAC, BlockDiagonal, Diagonal
    model = make_model(gpu, conv_bias)
    x, labels = batch(gpu)
    diag, kfac, block = Diagonal(model), KFAC(model), BlockDiagonal(model)
    model.zero_grad()
    torch.nn.functional.cross_entropy(model(x), labels).backward()
    diag.update(N)
    kfac.update(N)
    block.update(N)
    efb = EFB(model, kfac.state)
    efb.update(N)
    inf = INF(model, diag.state, kfac.state, efb.state, eigvecs=efb.eigvecs)
    inf.update(rank=RANK)
    kfac.decompose()
    for hook in kfac.hooks:
        hook.remove()
    model.zero_grad()
    return dict(model=model, diag=diag, kfac=kfac, block=block, efb=efb, inf=inf)


@functools.lru_cache(maxsize=None)
def chain():
    return build_chain(torch.device("cuda:0"))


def resolve(value, k):
    return float(value[k]) if isinstance(value, (list, tuple)) else float(value)


def inf_inverse_factors(inf, n_of, s_of):
    """B^-1 of every layer for one pair, from the `ops` calls `INF.log_det_grid` makes, and the clamped corrections."""
    from curvature_amd import ops
    from curvature_amd.curvatures import INF
    regs, plus = [], []
    for k, layer in enumerate(inf.state):
        ua, ug, lam, corr = inf.state[layer]
        plus.append(corr.clamp_min(0.0).contiguous())
        regs.append((ua, ug, ops.sqrt_scale(lam, s_of(k)), ops.rsqrt_affine(plus[-1], n_of(k), s_of(k))))
    vtvs = INF._vtv_many(regs)
    return ops.chol_factor_inverse(vtvs, [1.0] * len(vtvs)), plus


def check(got, want, bar, tag):
    print(f"{tag}: got {got:.15e} want {want:.15e} |diff| {abs(got - want):.3e} bar {bar:.3e}")
    assert abs(got - want) <= bar, tag


# ------------------------------------------------------------------------------------------------ 1. the reduction
@pytest.mark.parametrize("kind", KINDS)
def test_log_det_grid_is_the_float64_formula_on_the_estimators_tensors(gpu, kind):
    est = chain()[kind]
    rows = est.log_det_grid(HYPERS, per_layer=True)
    total = est.log_det_grid(HYPERS)
    assert rows.dtype == total.dtype == torch.float64 and rows.is_cuda and total.is_cuda
    assert tuple(rows.shape) == (2, len(HYPERS)) and tuple(total.shape) == (len(HYPERS),)
    rows, total = rows.cpu(), total.cpu()
    for h, (add, multiply) in enumerate(HYPERS):
        if kind == "inf":
            inv_b, plus = inf_inverse_factors(est, lambda k: resolve(add, k), lambda k: resolve(multiply, k))
        bars = 0.0
        for k, layer in enumerate(est.state):
            n, s = resolve(add, k), resolve(multiply, k)
            if kind in ("diag", "efb"):
                want, bar = R.spectrum_log_det(est.state[layer], n, s)
            elif kind == "block":
                want, bar = R.spectrum_log_det(est._spectrum[layer], n, s)
            elif kind == "kfac":
                want, bar = R.kfac_log_det(est._decomposition[layer][3], est._decomposition[layer][2], n, s)
            else:
                want, bar = R.inf_log_det(plus[k], inv_b[k], n, s)
            check(float(rows[k, h]), want, bar, f"{kind} layer {k} pair {h}")
            bars += bar
        assert abs(float(total[h]) - float(rows[:, h].sum())) <= bars


# ------------------------------------------------------------------------------------------------ 2. the meaning
def eig_eps(F):
    """FACTOR x the eigenvalue yardstick of tests/eigh_refs.py (`eigenvalue_bound`: the float32 rounding of the output plus
    twice the promised off-norm) relative to ||F||_2; (eps, ||F||_2)."""
    S = R.sym(F)
    two = float(torch.linalg.eigvalsh(S).abs().max())
    return EIG_FACTOR * (2.0 ** -24 + 2.0 * eigh_refs.PROMISED * float(torch.linalg.norm(S)) / two), two


def factor_bar(F, mult, gain, shift):
    """eps * mult * dim * gain * ||F||_2 / shift: every one of the dim eigenvalues is off by at most eps ||F||_2, and
    d log(gain x + shift) <= gain dx / shift."""
    eps, two = eig_eps(F)
    return eps * mult * F.shape[0] * gain * two / shift


@pytest.mark.parametrize("kind", ["kfac", "block"])
def test_log_det_grid_is_slogdet_of_the_dense_precision(gpu, kind):
    est = chain()[kind]
    rows = est.log_det_grid(MEANING, per_layer=True).cpu()
    for h, (n, s) in enumerate(MEANING):
        for k, layer in enumerate(est.state):
            if kind == "kfac":
                A, G = est.state[layer]
                want = R.slogdet(R.kfac_dense(A, G, n, s))
                bar = factor_bar(A, G.shape[0], math.sqrt(s), math.sqrt(n)) + factor_bar(G, A.shape[0], math.sqrt(s), math.sqrt(n))
            else:
                F = est.state[layer]
                want = R.slogdet(R.block_dense(F, n, s))
                bar = factor_bar(F, 1, s, n)
            check(float(rows[k, h]), want, bar, f"{kind} layer {k} pair ({n}, {s}) against slogdet")


def test_inf_log_det_grid_is_slogdet_of_the_dense_precision(gpu):
    """Pi as tests/inf_predictive_refs.py builds it (the correction clamped at 0).  Bar: 1e-6 k per layer, k the width of
    vtv - r and sigma are float32-rounded (2^-24 relative each), which to first order moves log det(I + M) by at most
    2.4e-7 tr((I + M)^-1 M) <= 2.4e-7 k, times 4 - plus the reduction's bar."""
    est = chain()["inf"]
    rows = est.log_det_grid(MEANING, per_layer=True).cpu()
    for h, (n, s) in enumerate(MEANING):
        inv_b, plus = inf_inverse_factors(est, lambda k: n, lambda k: s)
        for k, layer in enumerate(est.state):
            ua, ug, lam, _ = est.state[layer]
            Pi = inf_refs.dense_precision(R.f64(ua), R.f64(ug), R.f64(lam), R.f64(plus[k]), n, s)
            width = lam.numel()
            assert width == inv_b[k].shape[0] >= 1
            bar = 1e-6 * width + R.inf_log_det(plus[k], inv_b[k], n, s)[1]
            check(float(rows[k, h]), R.slogdet(Pi), bar, f"inf layer {k} (k = {width}) pair ({n}, {s}) against slogdet")


# ------------------------------------------------------------------------------------------------ 3. preconditions
def test_kfac_needs_a_current_decomposition(gpu):
    from curvature_amd.curvatures import KFAC
    model = make_model(gpu)
    x, labels = batch(gpu)
    kfac = KFAC(model)
    sentence = "no eigendecomposition of the current factors: call decompose() after the last update()"

    def update():
        model.zero_grad()
        torch.nn.functional.cross_entropy(model(x), labels).backward()
        kfac.update(N)
    try:
        update()
        with pytest.raises(RuntimeError) as info:
            kfac.log_det_grid(HYPERS)
        assert "KFAC.log_det_grid" in str(info.value) and sentence in str(info.value)
        kfac.decompose()
        assert bool(torch.isfinite(kfac.log_det_grid(HYPERS)).all())
        update()
        with pytest.raises(RuntimeError) as info:
            kfac.log_det_grid(HYPERS)
        assert sentence in str(info.value)
    finally:
        for hook in kfac.hooks:
            hook.remove()


def test_inf_needs_neither_invert_nor_the_predictive_switch(gpu):
    from curvature_amd import ops
    inf = build_chain(gpu)["inf"]
    assert not ops.inf_predictive_admitted() and not inf.inv_state
    assert bool(torch.isfinite(inf.log_det_grid(HYPERS)).all())
    assert not inf.inv_state and not hasattr(inf, "_sigma") and not hasattr(inf, "_r_version")


def tensors_of(value):
    if isinstance(value, torch.Tensor):
        return [value]
    return [t for v in value for t in tensors_of(v)]


def snapshot(est):
    return [[(t, t.clone()) for v in d.values() for t in tensors_of(v)] for d in (est.state, est.inv_state)]


@pytest.mark.parametrize("kind", KINDS)
def test_nothing_is_written_and_the_sampler_is_undisturbed(gpu, kind):
    """`state` and `inv_state` (the same tensors, the same bits) after `log_det_grid` and `log_prior_grid`, and
    `sample_and_replace` with a fixed seed with and without the calls in between."""
    made = build_chain(gpu)
    model, est = made["model"], made[kind]
    est.invert(1.0, 60.0)
    before = snapshot(est)
    extra = (est._r_version, dict(est._sigma)) if kind == "inf" else None

    def draw():
        est.noise_seed, est.noise_offset = 1234, 0
        est.sample_and_replace()
        return [p.detach().clone() for p in model.parameters()]
    first = draw()
    est.log_det_grid(HYPERS)
    est.log_det_grid(MEANING, per_layer=True)
    est.log_prior_grid(HYPERS)
    after = snapshot(est)
    for old, new in zip(before, after):
        assert len(old) == len(new)
        for (t0, v0), (t1, _) in zip(old, new):
            assert t0 is t1 and torch.equal(t1, v0)
    if kind == "inf":
        assert est._r_version == extra[0] and all(est._sigma[l] is t for l, t in extra[1].items())
    second = draw()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert any(not torch.equal(a, m) for a, m in zip(first, (est.model_state[k] for k, _ in model.named_parameters())))


# ------------------------------------------------------------------------------------------------ 4. the prior
def test_log_prior_grid_reads_the_means(gpu):
    """Against float64 from `model_state`, on a model whose convolution has no bias; unchanged while the model holds a
    sample.  Bar: 1/2 n_l times the bar of the layer's sum of squares, and a few ulp of the P log n terms."""
    made = build_chain(gpu, conv_bias=False)
    model, est = made["model"], made["diag"]
    layers = matrix_layers(model)
    assert layers[0].bias is None and layers[1].bias is not None
    got = est.log_prior_grid(HYPERS)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (len(HYPERS),)
    thetas = [torch.cat([R.f64(est.model_state_of(l, name)).flatten() for name in ("weight", "bias")
                         if getattr(l, name) is not None]) for l in layers]
    assert [t.numel() for t in thetas] == [36, 370]
    for h, (add, multiply) in enumerate(HYPERS):
        ns = [resolve(add, k) for k in range(2)]
        want = R.log_prior(thetas, ns)
        bar = sum(0.5 * n * R.squares_sum(t)[1] + 2.0 ** -50 * abs(0.5 * t.numel() * math.log(n)) for t, n in zip(thetas, ns))
        check(float(got[h]), want, bar, f"log prior pair {h}")
    est.invert(1.0, 60.0)
    est.sample_and_replace()
    assert any(not torch.equal(p.detach(), est.model_state[k]) for k, p in model.named_parameters())
    assert torch.equal(est.log_prior_grid(HYPERS), got)


# ------------------------------------------------------------------------------------------------ 5. the evidence
GRID20 = [(add, multiply) for add in (1e-3, 1e-2, 0.1, 1.0, 10.0) for multiply in (1.0, 16.0, 60.0, 6e4)]


@pytest.mark.parametrize("kind", ["diag", "kfac"])
def test_log_marginal_likelihood(gpu, kind):
    from curvature_amd.evaluate import log_likelihood, log_marginal_likelihood
    made = chain()
    model, est = made["model"], made[kind]
    dataset = [batch(gpu, seed=21), batch(gpu, seed=22)]
    ll, count = log_likelihood(model, dataset)
    assert count == 2 * N and isinstance(ll, float)
    ref = make_model(gpu).double()
    ref.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
    with torch.no_grad():
        want = sum(float(torch.log_softmax(ref(x.double()), dim=1).gather(1, y.view(-1, 1)).sum()) for x, y in dataset)
    print(f"log likelihood {ll:.9e} float64 {want:.9e}")
    assert abs(ll - want) <= 1e-5 * abs(want)
    res = log_marginal_likelihood(model, dataset, est, GRID20)
    log_det, log_prior = est.log_det_grid(GRID20).cpu(), est.log_prior_grid(GRID20).cpu()
    assert res["log_likelihood"] == ll
    assert all(res[k].dtype == torch.float64 and not res[k].is_cuda and tuple(res[k].shape) == (20,)
               for k in ("evidence", "log_det", "log_prior"))
    assert torch.equal(res["log_det"], log_det) and torch.equal(res["log_prior"], log_prior)
    assert torch.equal(res["evidence"], (log_prior - 0.5 * log_det) + ll)
    assert res["best"] == int(torch.argmax(res["evidence"])) and isinstance(res["best"], int)
    given = log_marginal_likelihood(model, None, est, GRID20, log_likelihood=ll)
    assert all(torch.equal(given[k], res[k]) for k in ("evidence", "log_det", "log_prior")) and given["best"] == res["best"]
    with pytest.raises(ValueError):
        log_marginal_likelihood(model, [], est, GRID20)
    halves = [log_marginal_likelihood(model, None, est, GRID20[a:a + 10], log_likelihood=ll) for a in (0, 10)]
    for k in ("evidence", "log_det", "log_prior"):
        assert torch.equal(torch.cat([half[k] for half in halves]), res[k]), k
