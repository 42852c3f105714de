"""Last-layer Laplace predictive on the GPU: csrc/head_mc.hip through `ops.head_mc` against float64 (tests/head_refs.py),
its noise stream, its chunks and batches; `Curvature.head_terms` of KFAC, EFB and Diagonal against the dense covariance
written entry by entry, and against the per-sample line (`glm_predictive`, `glm_predictive_joint`, `glm_predictive_mc`)
on an estimator that holds the head alone; the drivers `evaluate.last_layer_predictive` / `eval_last_layer`.

The bar is the project's (`TOL` of tests/test_glm_mc_gpu.py): relative Frobenius error below 1e-4
against float64.  Every measured error is printed."""
import types

import pytest
import torch

from head_refs import head_mc_reference, head_terms_reference

pytestmark = pytest.mark.gpu
TOL = 1e-4


def rel2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    denom = float(torch.linalg.norm(b))
    return float(torch.linalg.norm(a - b)) / denom if denom > 0 else float(torch.linalg.norm(a - b))


# ------------------------------------------------------------------------------------------------ inputs
def matrix(K, form, gen, gpu, scale=1.0, pad=3):
    """(view or None, lower): `form` "dense", "lower" (NaN above the diagonal) or "none"; rows K + pad apart in a
    NaN-filled buffer."""
    if form == "none":
        return None, False
    M = torch.randn(K, K, generator=gen) * scale
    if form == "lower":
        M = torch.tril(M) + torch.triu(torch.full((K, K), float("nan")), diagonal=1)
    buf = torch.full((K, K + pad), float("nan"))
    buf[:, :K] = M
    return buf.to(gpu)[:, :K], form == "lower"


def padded_rows(values, gpu, pad=2):
    """(N, K) values as a view with row stride K + pad into a NaN-filled buffer."""
    N, K = values.shape
    buf = torch.full((N, K + pad), float("nan"))
    buf[:, :K] = values
    return buf.to(gpu)[:, :K]


def spread(N, K, scalar, gen, gpu):
    d2 = torch.rand(N, generator=gen) + 0.1 if scalar else torch.rand(N, K, generator=gen) + 0.1
    return d2.to(gpu)


def run(gpu, M, lower, d2, mu, S, noise=None, seed=0, offset=0, draws=True, probs=True):
    from curvature_amd import ops
    N, K = mu.shape
    out = {}
    if probs:
        out["probs"] = torch.full((N, K), float("nan"), device=gpu)
    if draws:
        out["draws"] = torch.full((N, S, K), float("nan"), device=gpu)
    ops.head_mc([ops.HeadMCJob(M, d2, mu, S, lower=lower, noise=noise, seed=seed, offset=offset, **out)])
    torch.cuda.synchronize()
    return out


def errors_against_float64(got, M, lower, d2, mu, z):
    probs, draws = head_mc_reference(M, lower, d2, mu, z)
    assert torch.isfinite(got["probs"]).all() and torch.isfinite(got["draws"]).all()
    own = torch.softmax(got["draws"].double().cpu(), dim=2).mean(dim=1)      # probs is the mean softmax of its own draws
    return rel2(got["probs"], probs), rel2(got["draws"], draws), rel2(got["probs"], own)


# ------------------------------------------------------------------------------------------------ 1. the primitive
@pytest.mark.parametrize("K", [1, 3, 4, 5, 31, 32, 33, 65, 130])
def test_head_mc_against_float64(gpu, K):
    """Both sides of a Philox quad, of an MFMA block, of a wave's row share and of a draw tile; every form of M and d2;
    strided M and mu in NaN-filled buffers."""
    gen = torch.Generator().manual_seed(100 + K)
    worst = 0.0
    for N in (1, 3):
        for S in (1, 31, 32, 33, 70):
            for form in ("dense", "lower", "none"):
                for scalar in (True, False):
                    M, lower = matrix(K, form, gen, gpu, scale=K ** -0.5)
                    d2 = spread(N, K, scalar, gen, gpu)
                    mu = padded_rows(torch.randn(N, K, generator=gen) * 2, gpu)
                    z = torch.randn(N, S, K, generator=gen).to(gpu)
                    got = run(gpu, M, lower, d2, mu, S, noise=z)
                    errs = errors_against_float64(got, M, lower, d2, mu, z)
                    worst = max(worst, *errs)
                    assert max(errs) < TOL, (N, S, form, scalar, errs)
    print(f"head_mc K={K}: worst relative error against float64 {worst:.3e}")


@pytest.mark.parametrize("form", ["dense", "lower", "none"])
def test_zero_and_negative_spread(gpu, form):
    """A d2 row of zeros: probs are the plain softmax; -1e-12 is clamped to 0 - nothing non-finite."""
    N, K, S = 3, 37, 40
    gen = torch.Generator().manual_seed(7)
    M, lower = matrix(K, form, gen, gpu)
    mu = torch.randn(N, K, generator=gen).to(gpu)
    z = torch.randn(N, S, K, generator=gen).to(gpu)
    d2 = torch.rand(N, K, generator=gen)
    d2[1] = 0.0
    d2[2, ::3] = -1e-12
    d2 = d2.to(gpu)
    got = run(gpu, M, lower, d2, mu, S, noise=z)
    errs = errors_against_float64(got, M, lower, d2, mu, z)
    plain = rel2(got["probs"][1], torch.softmax(mu[1].double(), dim=0))
    assert torch.equal(got["draws"][1], mu[1].expand(S, K))
    print(f"head_mc {form}: zero / negative spread {max(errs):.3e}, zero row against softmax {plain:.3e}")
    assert max(errs) < TOL and plain < TOL
    scalar = torch.tensor([0.5, 0.0, -1e-12]).to(gpu)
    got = run(gpu, M, lower, scalar, mu, S, noise=z)
    assert max(errors_against_float64(got, M, lower, scalar, mu, z)) < TOL
    assert torch.equal(got["draws"][1:], mu[1:, None, :].expand(2, S, K))


# ------------------------------------------------------------------------------------------------ 2. at the cap
@pytest.mark.parametrize("form", ["lower", "dense"])
def test_at_the_cap(gpu, form):
    from curvature_amd import ops
    K, N, S = ops.HEAD_MC_MAX_CLASSES, 2, 40
    gen = torch.Generator().manual_seed(3)
    M, lower = matrix(K, form, gen, gpu, scale=K ** -0.5)
    d2 = spread(N, K, form == "lower", gen, gpu)
    mu = padded_rows(torch.randn(N, K, generator=gen), gpu)
    z = torch.randn(N, S, K, generator=gen).to(gpu)
    got = run(gpu, M, lower, d2, mu, S, noise=z)
    errs = errors_against_float64(got, M, lower, d2, mu, z)
    print(f"head_mc at the cap K={K} {form}: probs {errs[0]:.3e} draws {errs[1]:.3e} own draws {errs[2]:.3e}")
    assert max(errs) < TOL


# ------------------------------------------------------------------------------------------------ 3. chunks
def test_chunked_draws(gpu):
    """N = 1: the smallest S the plan cuts into two chunks per input (its workspace is no longer 0)."""
    from curvature_amd import _lib, ops
    L = _lib.lib()
    K = 37

    def scratch(S):
        return L.curv_head_mc_workspace_bytes(ops._head_mc_descs([ops.HeadMCJob(True, None, None, S, N=1, K=K)], False), 1)
    S = next(s for s in range(1, 200) if scratch(s) > 0)
    assert S == 33 and scratch(S - 1) == 0
    gen = torch.Generator().manual_seed(5)
    worst = 0.0
    for s in (S, 3 * 32 + 5):
        for form in ("dense", "lower", "none"):
            M, lower = matrix(K, form, gen, gpu)
            d2 = spread(1, K, False, gen, gpu)
            mu = torch.randn(1, K, generator=gen).to(gpu)
            z = torch.randn(1, s, K, generator=gen).to(gpu)
            got = run(gpu, M, lower, d2, mu, s, noise=z)
            worst = max(worst, *errors_against_float64(got, M, lower, d2, mu, z))
    print(f"head_mc chunked (S = {S}, 101): {worst:.3e}")
    assert worst < TOL


# ------------------------------------------------------------------------------------------------ 4. the noise stream
@pytest.mark.parametrize("K", [3, 4, 33])
def test_implicit_noise_is_the_explicit_stream(gpu, K):
    from curvature_amd import ops
    N, S, seed, offset = 3, 45, 20260101, 12345
    Kq = (K + 3) // 4
    gen = torch.Generator().manual_seed(K)
    z = ops.randn((N, S, 4 * Kq), gpu, seed, offset)[:, :, :K]
    for form in ("dense", "lower", "none"):
        M, lower = matrix(K, form, gen, gpu)
        d2 = spread(N, K, False, gen, gpu)
        mu = torch.randn(N, K, generator=gen).to(gpu)
        implicit = run(gpu, M, lower, d2, mu, S, seed=seed, offset=offset)
        explicit = run(gpu, M, lower, d2, mu, S, noise=z)
        assert torch.isfinite(implicit["probs"]).all()
        assert torch.equal(implicit["draws"], explicit["draws"]) and torch.equal(implicit["probs"], explicit["probs"])
        other = run(gpu, M, lower, d2, mu, S, seed=seed, offset=offset + 1)
        assert not torch.equal(other["draws"], implicit["draws"])


# ------------------------------------------------------------------------------------------------ 5. batches
def test_an_item_has_the_same_bits_alone_and_in_a_batch(gpu):
    """17 items of different shapes: two launches."""
    from curvature_amd import ops
    gen = torch.Generator().manual_seed(11)
    forms = ("dense", "lower", "none")
    shapes = [(1 + i % 3, (1, 3, 5, 31, 33, 65, 130, 200, 40)[i % 9], (1, 33, 70, 32, 100)[i % 5]) for i in range(17)]
    jobs, outs = [], []
    for i, (N, K, S) in enumerate(shapes):
        M, lower = matrix(K, forms[i % 3], gen, gpu, scale=K ** -0.5)
        d2 = spread(N, K, i % 2 == 0, gen, gpu)
        mu = torch.randn(N, K, generator=gen).to(gpu)
        outs.append([dict(probs=torch.empty(N, K, device=gpu), draws=torch.empty(N, S, K, device=gpu)) for _ in range(2)])
        jobs.append([ops.HeadMCJob(M, d2, mu, S, lower=lower, seed=5, offset=1000 * i, **o) for o in outs[-1]])
    ops.head_mc([j[0] for j in jobs])
    for j in jobs:
        ops.head_mc([j[1]])
    torch.cuda.synchronize()
    for together, alone in outs:
        assert torch.isfinite(together["probs"]).all()
        assert torch.equal(together["probs"], alone["probs"]) and torch.equal(together["draws"], alone["draws"])


# ------------------------------------------------------------------------------------------------ 6. head_terms
def head_model(gpu, bias=True):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.ReLU(), torch.nn.Flatten(),
                                torch.nn.Linear(4 * 6 * 6, 7, bias=bias))
    return model.to(gpu)


def batches(gpu, count=2, N=5):
    gen = torch.Generator().manual_seed(21)
    return [(torch.randn(N, 1, 8, 8, generator=gen).to(gpu), torch.randint(0, 7, (N,), generator=gen).to(gpu))
            for _ in range(count)]


def make_estimator(kind, model, data, layer_types=None, add=1.0, multiply=50.0):
    """`kind` after one update per batch of `data` and an inversion."""
    from curvature_amd.curvatures import EFB, KFAC, Diagonal

    def sweep(est):
        for x, labels in data:
            model.zero_grad()
            torch.nn.functional.cross_entropy(model(x), labels).backward()
            est.update(x.shape[0])
    if kind == "Diagonal":
        est = Diagonal(model, layer_types)
    else:
        kfac = KFAC(model, layer_types)
        sweep(kfac)
        if kind == "KFAC":
            est = kfac
        else:
            for hook in kfac.hooks:
                hook.remove()
            est = EFB(model, kfac.state, layer_types)
    if kind != "KFAC":
        sweep(est)
    model.zero_grad()
    est.invert(add=add, multiply=multiply)
    return est


def dense_of(terms):
    """M diag(d2) M^T in float64 from what `head_terms` returned."""
    d2 = terms.d2.double().cpu()
    N, K = terms.variance.shape
    d2 = d2[:, None].expand(N, K) if d2.dim() == 1 else d2
    M = torch.eye(K, dtype=torch.float64) if terms.M is None else terms.M.double().cpu()
    if terms.lower:
        M = torch.tril(M)
    return torch.einsum("ca,na,da->ncd", M, d2, M)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("kind", ["KFAC", "EFB", "Diagonal"])
def test_head_terms(gpu, kind, bias):
    model = head_model(gpu, bias)
    est = make_estimator(kind, model, batches(gpu))
    head = model[3]
    x = torch.randn(5, 1, 8, 8, generator=torch.Generator().manual_seed(8)).to(gpu)
    with torch.no_grad():
        features = model[:3](x)
    terms = est.head_terms(head, features)
    N, K = 5, 7
    assert tuple(terms.variance.shape) == (N, K) and tuple(terms.d2.shape) == ((N,) if kind == "KFAC" else (N, K))
    assert (terms.M is None) == (kind == "Diagonal") and terms.lower == (kind == "KFAC")
    sigma = head_terms_reference(kind, est.inv_state[head], getattr(est, "eigvecs", {}).get(head), features, bias)
    e_var = rel2(terms.variance, torch.diagonal(sigma, dim1=1, dim2=2))
    e_cov = rel2(dense_of(terms), sigma)
    half = est.head_terms(head, features.bfloat16())
    e_half = rel2(half.variance, est.head_terms(head, features.bfloat16().float()).variance)
    print(f"head_terms {kind} bias={bias}: variance {e_var:.3e}, M diag(d2) M^T {e_cov:.3e}")
    assert e_var < TOL and e_cov < TOL and e_half == 0.0


# ------------------------------------------------------------------------------------------------ 7. the per-sample line
@pytest.mark.parametrize("kind", ["KFAC", "EFB", "Diagonal"])
def test_against_the_per_sample_line(gpu, kind):
    """The estimator holds the head alone, so the whole-network GLM predictive is the head's."""
    from curvature_amd.evaluate import glm_predictive, glm_predictive_joint, glm_predictive_mc, last_layer_predictive
    model = head_model(gpu)
    est = make_estimator(kind, model, batches(gpu), layer_types="Linear")
    head = model[3]
    assert list(est.inv_state) == [head]
    x = torch.randn(5, 1, 8, 8, generator=torch.Generator().manual_seed(9)).to(gpu)
    logits, variance, probs = last_layer_predictive(model, est, x)
    logits_g, variance_g, probs_g = glm_predictive(model, est, x)
    e_var, e_probs = rel2(variance, variance_g), rel2(probs, probs_g)
    assert torch.equal(logits, logits_g)
    with torch.no_grad():
        terms = est.head_terms(head, model[:3](x))
    covariance = glm_predictive_joint(model, est, x)[1]
    e_cov = rel2(dense_of(terms), covariance)
    print(f"{kind}: against glm_predictive: variance {e_var:.3e} probs {e_probs:.3e}; against the joint covariance {e_cov:.3e}")
    assert e_var < TOL and e_probs < TOL and e_cov < TOL
    if kind != "KFAC":
        return
    # chol(s_n L_G L_G^T) = sqrt(s_n) L_G by uniqueness - while curv_logit_mc drops no column: every pivot far above its
    # threshold 16 * 2^-23 * max diag, recomputed in float64
    sigma = dense_of(terms)
    for n in range(sigma.shape[0]):
        pivots = torch.diagonal(torch.linalg.cholesky(sigma[n])) ** 2
        assert float(pivots.min()) > 100 * 16 * 2.0 ** -23 * float(torch.diagonal(sigma[n]).max())
    S = 300
    z = torch.randn(5, S, 7, generator=torch.Generator().manual_seed(10)).to(gpu)
    _, _, probs_mc, draws_mc = last_layer_predictive(model, est, x, predictive="mc", samples=S, noise=z, return_draws=True)
    _, _, probs_g, draws_g = glm_predictive_mc(model, est, x, samples=S, noise=z, return_draws=True)
    e_probs, e_draws = rel2(probs_mc, probs_g), rel2(draws_mc, draws_g)
    print(f"KFAC: against glm_predictive_mc: probs {e_probs:.3e} draws {e_draws:.3e}")
    assert e_probs < TOL and e_draws < TOL


# ------------------------------------------------------------------------------------------------ 8. drivers
@pytest.mark.parametrize("kind", ["KFAC", "EFB", "Diagonal"])
def test_drivers(gpu, kind):
    from curvature_amd.evaluate import eval_last_layer, last_layer_predictive
    model = head_model(gpu)
    data = batches(gpu)
    est = make_estimator(kind, model, data)
    again = make_estimator(kind, model, data)                      # the same estimator, rebuilt
    model.eval()
    gen = torch.Generator().manual_seed(30)
    dataset = [(torch.randn(n, 1, 8, 8, generator=gen), torch.randint(0, 7, (n,), generator=gen)) for n in (4, 5, 2)]
    params = [p.detach().clone() for p in model.parameters()]
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.25)
    hooks = [(len(m._forward_hooks), len(m._forward_pre_hooks), len(m._backward_hooks)) for m in model.modules()]
    N, K, S = 11, 7, 64

    predictions, labels = eval_last_layer(model, dataset, est)
    single = torch.cat([last_layer_predictive(model, est, x.to(gpu))[2] for x, _ in dataset])
    assert predictions.shape == (N, K) and labels.shape == (N,)
    assert torch.equal(torch.from_numpy(predictions), single.cpu())
    assert torch.equal(torch.from_numpy(labels), torch.cat([l for _, l in dataset]))
    assert float((single.sum(dim=1) - 1).abs().max()) < 1e-5

    est.noise_seed, est.noise_offset = 77, 10
    predictions, _ = eval_last_layer(model, dataset, est, predictive="mc", samples=S)
    assert est.noise_offset == 10 + N * S * 2                      # ceil(7 / 4) = 2 counters per draw
    again.noise_seed, again.noise_offset = 77, 10
    single = []
    for x, _ in dataset:
        before = again.noise_offset
        single.append(last_layer_predictive(model, again, x.to(gpu), predictive="mc", samples=S)[2])
        assert again.noise_offset == before + x.shape[0] * S * 2
    single = torch.cat(single)
    assert torch.equal(torch.from_numpy(predictions), single.cpu())
    assert float((single.sum(dim=1) - 1).abs().max()) < 1e-5
    explicit = last_layer_predictive(model, again, dataset[0][0].to(gpu), predictive="mc", samples=S,
                                     noise=torch.randn(4, S, K, device=gpu), return_draws=True)
    assert again.noise_offset == 10 + N * S * 2 and tuple(explicit[3].shape) == (4, S, K)

    # left as found
    for p, before in zip(model.parameters(), params):
        assert torch.equal(p.detach(), before) and torch.equal(p.grad, torch.full_like(p, 0.25))
    assert hooks == [(len(m._forward_hooks), len(m._forward_pre_hooks), len(m._backward_hooks)) for m in model.modules()]
    assert not any(m.training for m in model.modules())            # the training flags too
    again.use_device_noise_counter(True)
    with pytest.raises(RuntimeError, match="device noise counter"):
        last_layer_predictive(model, again, dataset[0][0].to(gpu), predictive="mc", samples=S)


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals(gpu):
    from curvature_amd import ops
    from curvature_amd.curvatures import INF, BlockDiagonal
    from curvature_amd.evaluate import last_layer_predictive
    model = head_model(gpu)
    data = batches(gpu, count=1)
    x = data[0][0]
    est = make_estimator("Diagonal", model, data)

    block = BlockDiagonal(model, "Linear")
    torch.nn.functional.cross_entropy(model(x), data[0][1]).backward()
    block.update(x.shape[0])
    block.invert(add=1.0, multiply=1.0)
    model.zero_grad()
    with pytest.raises(NotImplementedError, match=r"BlockDiagonal.head_terms: layer '3'.*BlockDiagonal"):
        last_layer_predictive(model, block, x)
    inf = object.__new__(INF)                                      # (the refusal needs none of its factors)
    inf.model, inf.shard, inf.inv_state = model, None, {model[3]: torch.ones(1, device=gpu)}
    with pytest.raises(NotImplementedError, match=r"INF.head_terms: layer '3'.*INF"):
        last_layer_predictive(model, inf, x)

    # a head that is not the output; a head that did not run
    post = torch.nn.Sequential(*model, torch.nn.LogSoftmax(dim=1))
    with pytest.raises(RuntimeError, match="'3'.*post-processes"):
        last_layer_predictive(post, est, x)
    with pytest.raises(RuntimeError, match="'3'.*did not run"):
        last_layer_predictive(model[:3], est, x)

    # a head applied per token
    torch.manual_seed(1)
    tokens = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.ReLU(), torch.nn.Linear(5, 4)).to(gpu)
    token_est = types.SimpleNamespace(model=tokens, inv_state={tokens[2]: torch.ones(4, 6, device=gpu)})
    with pytest.raises(RuntimeError, match=r"'2'.*\(2, 3, 5\).*per token"):
        last_layer_predictive(tokens, token_est, torch.randn(2, 3, 6, device=gpu))

    # K above the cap: "mc" refuses and advises "probit", which works
    from curvature_amd.curvatures import Diagonal
    cap = ops.HEAD_MC_MAX_CLASSES
    torch.manual_seed(2)
    wide = torch.nn.Sequential(torch.nn.Linear(8, cap + 1)).to(gpu)
    xw, yw = torch.randn(4, 8, device=gpu), torch.randint(0, cap + 1, (4,), device=gpu)
    wide_est = Diagonal(wide)
    torch.nn.functional.cross_entropy(wide(xw), yw).backward()
    wide_est.update(4)
    wide_est.invert(add=1.0, multiply=10.0)
    with pytest.raises(ValueError, match=rf"HEAD_MC_MAX_CLASSES = {cap}.*probit"):
        last_layer_predictive(wide, wide_est, xw, predictive="mc", samples=8)
    logits, variance, probs = last_layer_predictive(wide, wide_est, xw)
    assert tuple(probs.shape) == (4, cap + 1) and torch.isfinite(probs).all() and bool((variance > 0).all())
    assert float((probs.sum(dim=1) - 1).abs().max()) < 1e-5
