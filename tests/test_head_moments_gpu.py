"""The entropy split of the last-layer Laplace predictive on the GPU: curv_head_mc_moments through `ops.head_mc_moments`
against float64 (tests/head_moments_refs.py), bit for bit against `ops.head_mc`, its noise stream, chunks and batches; the
drivers `evaluate.last_layer_uncertainty` / `eval_uncertainty`.

The bar is the project's (tests/test_head_mc_gpu.py): relative Frobenius error below `TOL` = 1e-4
against float64 for `probs`, `entropy`, `probs_sq` and `draws`.  The mutual information `epistemic` is a difference of two
nearly equal numbers where it is small, so it is judged as ``|got - ref| / |total_ref|`` - never relative to itself.  Every
measured error is printed."""
import itertools
import types

import pytest
import torch

from head_moments_refs import entropy_of, head_moments_reference

pytestmark = pytest.mark.gpu
TOL = 1e-4
OUTPUTS = ("probs", "entropy", "probs_sq", "draws")
FENCE = 5


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
    N, K = values.shape
    buf = torch.full((N, K + pad), float("nan"))
    buf[:, :K] = values
    return buf.to(gpu)[:, :K]


def spread(N, K, scalar, gen, gpu):
    d2 = torch.rand(N, generator=gen) + 0.1 if scalar else torch.rand(N, K, generator=gen) + 0.1
    return d2.to(gpu)


def fenced(shape, gpu):
    """(buffer, view): a contiguous view of `shape` with FENCE NaNs on either side."""
    count = 1
    for s in shape:
        count *= s
    buf = torch.full((count + 2 * FENCE,), float("nan"), device=gpu)
    return buf, buf[FENCE:FENCE + count].view(shape)


def run(gpu, M, lower, d2, mu, S, noise=None, seed=0, offset=0, outputs=OUTPUTS):
    """One `ops.head_mc_moments` call; every output a view inside a NaN-fenced buffer that starts as NaN.  The fences
    must come back untouched."""
    from curvature_amd import ops
    N, K = mu.shape
    shapes = dict(probs=(N, K), entropy=(N,), probs_sq=(N, K), draws=(N, S, K))
    held = {name: fenced(shapes[name], gpu) for name in outputs}
    ops.head_mc_moments([ops.HeadMomentsJob(M, d2, mu, S, lower=lower, noise=noise, seed=seed, offset=offset,
                                            **{name: view for name, (_, view) in held.items()})])
    torch.cuda.synchronize()
    for name, (buf, view) in held.items():
        assert torch.isnan(buf[:FENCE]).all() and torch.isnan(buf[-FENCE:]).all(), name
        assert torch.isfinite(view).all(), name
    return {name: view for name, (_, view) in held.items()}


def errors_against_float64(got, M, lower, d2, mu, z):
    """Relative errors of whatever `got` holds, in the order of OUTPUTS."""
    ref = dict(zip(OUTPUTS, head_moments_reference(M, lower, d2, mu, z)))
    return {name: rel2(got[name], ref[name]) for name in OUTPUTS if name in got}


# ------------------------------------------------------------------------------------------------ 1. the primitive
@pytest.mark.parametrize("K", [1, 5, 33, 130])
def test_moments_against_float64(gpu, K):
    """Both sides of a Philox quad, of an MFMA block, of a wave's row share and of a draw tile; every form of M and d2;
    strided M and mu in NaN-filled buffers; outputs inside NaN fences."""
    gen = torch.Generator().manual_seed(200 + K)
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for N in (1, 3):
        for S in (1, 31, 33, 70):
            for form in ("dense", "lower", "none"):
                for scalar in (True, False):
                    M, lower = matrix(K, form, gen, gpu, scale=K ** -0.5)
                    d2 = spread(N, K, scalar, gen, gpu)
                    mu = padded_rows(torch.randn(N, K, generator=gen) * 2, gpu)
                    z = torch.randn(N, S, K, generator=gen).to(gpu)
                    got = run(gpu, M, lower, d2, mu, S, noise=z)
                    errs = errors_against_float64(got, M, lower, d2, mu, z)
                    for name, e in errs.items():
                        worst[name] = max(worst[name], e)
                    assert max(errs.values()) < TOL, (N, S, form, scalar, errs)
                    if K == 1:
                        assert torch.equal(got["entropy"], torch.zeros(N, device=gpu))
                        assert not torch.signbit(got["entropy"]).any()                       # +0.0
                        assert torch.equal(got["probs_sq"], torch.ones(N, 1, device=gpu))
                        assert torch.equal(got["probs"], torch.ones(N, 1, device=gpu))
    print(f"head_mc_moments K={K}: worst relative error against float64 " +
          " ".join(f"{name} {e:.3e}" for name, e in worst.items()))


@pytest.mark.parametrize("K", [1, 5, 33, 130])
def test_every_combination_of_outputs(gpu, K):
    """Any output may be missing: the others have the bits of the call that asked for all four."""
    gen = torch.Generator().manual_seed(300 + K)
    for N, S, form in ((3, 33, "dense"), (1, 70, "lower"), (3, 31, "none")):
        M, lower = matrix(K, form, gen, gpu, scale=K ** -0.5)
        d2 = spread(N, K, form == "lower", gen, gpu)
        mu = padded_rows(torch.randn(N, K, generator=gen) * 2, gpu)
        z = torch.randn(N, S, K, generator=gen).to(gpu)
        full = run(gpu, M, lower, d2, mu, S, noise=z)
        assert max(errors_against_float64(full, M, lower, d2, mu, z).values()) < TOL
        for count in (1, 2, 3):
            for outputs in itertools.combinations(OUTPUTS, count):
                got = run(gpu, M, lower, d2, mu, S, noise=z, outputs=outputs)
                for name in outputs:
                    assert torch.equal(got[name], full[name]), (N, S, form, outputs, name)


# ------------------------------------------------------------------------------------------------ 2. at the cap
@pytest.mark.parametrize("form", ["lower", "dense"])
def test_at_the_cap(gpu, form):
    from curvature_amd import ops
    K, N, S = ops.HEAD_MC_MAX_CLASSES, 1, 33
    gen = torch.Generator().manual_seed(3)
    M, lower = matrix(K, form, gen, gpu, scale=K ** -0.5)
    d2 = spread(N, K, form == "lower", gen, gpu)
    mu = padded_rows(torch.randn(N, K, generator=gen), gpu)
    z = torch.randn(N, S, K, generator=gen).to(gpu)
    got = run(gpu, M, lower, d2, mu, S, noise=z)
    errs = errors_against_float64(got, M, lower, d2, mu, z)
    print(f"head_mc_moments at the cap K={K} {form}: " + " ".join(f"{name} {e:.3e}" for name, e in errs.items()))
    assert max(errs.values()) < TOL


# ------------------------------------------------------------------------------------------------ 3. chunks
def chunked_case(gpu):
    N, K, S = 2, 37, 4100
    gen = torch.Generator().manual_seed(5)
    M, lower = matrix(K, "lower", gen, gpu, scale=K ** -0.5)
    d2 = spread(N, K, False, gen, gpu)
    mu = torch.randn(N, K, generator=gen).to(gpu)
    z = torch.randn(N, S, K, generator=gen).to(gpu)
    return M, lower, d2, mu, S, z


def test_chunked_draws(gpu):
    """N = 2, S = 4100: 129 tiles in 65 chunks of two; 2 K + 1 partial sums per input and chunk."""
    from curvature_amd import _lib, ops
    M, lower, d2, mu, S, z = chunked_case(gpu)
    N, K = mu.shape
    chunks = 65
    need = _lib.lib().curv_head_mc_moments_workspace_bytes(
        ops._head_moments_descs([ops.HeadMomentsJob(True, None, None, S, N=N, K=K)], False), 1)
    assert need == -(-(N * chunks * (2 * K + 1) * 4) // 256) * 256 == 39168
    got = run(gpu, M, lower, d2, mu, S, noise=z, outputs=("probs", "entropy", "probs_sq"))
    errs = errors_against_float64(got, M, lower, d2, mu, z)
    print("head_mc_moments chunked (65 chunks): " + " ".join(f"{name} {e:.3e}" for name, e in errs.items()))
    assert len(errs) == 3 and max(errs.values()) < TOL
    only = run(gpu, M, lower, d2, mu, S, noise=z, outputs=("entropy",))
    assert torch.equal(only["entropy"], got["entropy"])


# ------------------------------------------------------------------------------------------------ 4. the bits of head_mc
def test_probs_have_the_bits_of_head_mc(gpu):
    from curvature_amd import ops
    gen = torch.Generator().manual_seed(9)
    cases = [(3, 5, 70, "dense"), (1, 33, 33, "lower"), (3, 130, 31, "none"), (2, 130, 70, "lower"),
             (1, ops.HEAD_MC_MAX_CLASSES, 33, "dense"), (1, 1, 40, "dense")]
    for N, K, S, form in cases:
        M, lower = matrix(K, form, gen, gpu, scale=K ** -0.5)
        d2 = spread(N, K, form == "lower", gen, gpu)
        mu = padded_rows(torch.randn(N, K, generator=gen) * 2, gpu)
        for noise in (torch.randn(N, S, K, generator=gen).to(gpu), None):
            plain = torch.full((N, K), float("nan"), device=gpu)
            ops.head_mc([ops.HeadMCJob(M, d2, mu, S, lower=lower, noise=noise, probs=plain, seed=31, offset=77)])
            got = run(gpu, M, lower, d2, mu, S, noise=noise, seed=31, offset=77)
            assert torch.equal(got["probs"], plain), (N, K, S, form, noise is None)
            alone = run(gpu, M, lower, d2, mu, S, noise=noise, seed=31, offset=77, outputs=("probs",))
            assert torch.equal(alone["probs"], plain)
    M, lower, d2, mu, S, z = chunked_case(gpu)
    for noise in (z, None):
        plain = torch.full(tuple(mu.shape), float("nan"), device=gpu)
        ops.head_mc([ops.HeadMCJob(M, d2, mu, S, lower=lower, noise=noise, probs=plain, seed=31, offset=77)])
        got = run(gpu, M, lower, d2, mu, S, noise=noise, seed=31, offset=77, outputs=("probs", "entropy", "probs_sq"))
        assert torch.equal(got["probs"], plain)


# ------------------------------------------------------------------------------------------------ 5. noise and batches
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
        for name in OUTPUTS:
            assert torch.equal(implicit[name], explicit[name]), (form, name)
        other = run(gpu, M, lower, d2, mu, S, seed=seed, offset=offset + 1)
        assert not torch.equal(other["draws"], implicit["draws"])


def test_an_item_has_the_same_bits_alone_and_in_a_batch(gpu):
    """17 items of different shapes, chunked ones among them: two launches."""
    from curvature_amd import ops
    gen = torch.Generator().manual_seed(11)
    forms = ("dense", "lower", "none")
    shapes = [(1 + i % 3, (1, 3, 5, 31, 33, 65, 130, 200, 40)[i % 9], (1, 33, 70, 32, 100)[i % 5]) for i in range(17)]
    jobs, outs = [], []
    for i, (N, K, S) in enumerate(shapes):
        M, lower = matrix(K, forms[i % 3], gen, gpu, scale=K ** -0.5)
        d2 = spread(N, K, i % 2 == 0, gen, gpu)
        mu = torch.randn(N, K, generator=gen).to(gpu)
        outs.append([dict(probs=torch.empty(N, K, device=gpu), entropy=torch.empty(N, device=gpu),
                          probs_sq=torch.empty(N, K, device=gpu), draws=torch.empty(N, S, K, device=gpu))
                     for _ in range(2)])
        jobs.append([ops.HeadMomentsJob(M, d2, mu, S, lower=lower, seed=5, offset=1000 * i, **o) for o in outs[-1]])
    ops.head_mc_moments([j[0] for j in jobs])
    for j in jobs:
        ops.head_mc_moments([j[1]])
    torch.cuda.synchronize()
    for together, alone in outs:
        for name in OUTPUTS:
            assert torch.isfinite(together[name]).all()
            assert torch.equal(together[name], alone[name]), name


# ------------------------------------------------------------------------------------------------ 6. no spread
class FixedTerms:
    """An estimator that holds `head` and hands out the given head terms."""

    def __init__(self, model, head, terms):
        self.model, self.inv_state, self.terms = model, {head: None}, terms

    def head_terms(self, layer, features):
        return self.terms


@pytest.mark.parametrize("form", ["dense", "lower", "none"])
def test_zero_and_negative_spread(gpu, form):
    """d2 = 0 or slightly negative: every draw is mu, so the mean entropy is H(softmax(mu)), the mean square is
    softmax(mu) ** 2 and nothing is epistemic."""
    from curvature_amd.curvatures import HeadTerms
    from curvature_amd.evaluate import last_layer_uncertainty
    N, K, S = 3, 37, 40
    gen = torch.Generator().manual_seed(7)
    M, lower = matrix(K, form, gen, gpu)
    mu = torch.randn(N, K, generator=gen).to(gpu)
    z = torch.randn(N, S, K, generator=gen).to(gpu)
    d2 = torch.zeros(N, K)
    d2[2, ::3] = -1e-12
    d2[1, 1::2] = -3.0
    soft = torch.softmax(mu.double().cpu(), dim=1)
    for spread_ in (d2.to(gpu), torch.tensor([0.0, -1e-12, -2.0]).to(gpu)):
        got = run(gpu, M, lower, spread_, mu, S, noise=z)
        e_h, e_sq, e_p = rel2(got["entropy"], entropy_of(soft)), rel2(got["probs_sq"], soft ** 2), rel2(got["probs"], soft)
        print(f"head_mc_moments {form}: no spread: entropy {e_h:.3e} probs_sq {e_sq:.3e} probs {e_p:.3e}")
        assert max(e_h, e_sq, e_p) < TOL
        assert torch.equal(got["draws"], mu[:, None, :].expand(N, S, K))

    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(6, K)).to(gpu)
    terms = HeadTerms(None if M is None else M.contiguous().nan_to_num(0.0), lower, d2.to(gpu),
                      torch.zeros(N, K, device=gpu))
    est = FixedTerms(model, model[0], terms)
    result = last_layer_uncertainty(model, est, torch.randn(N, 6, device=gpu), samples=S, noise=z)
    total = float(torch.linalg.norm(entropy_of(torch.softmax(result.logits.double().cpu(), dim=1))))
    print(f"head_mc_moments {form}: no spread: |epistemic| / |total| "
          f"{float(torch.linalg.norm(result.epistemic.double().cpu())) / total:.3e}")
    assert float(torch.linalg.norm(result.epistemic.double().cpu())) < TOL * total
    assert float(result.probs_std.max()) < 1e-3                   # sqrt of a cancelled difference: sqrt(eps) at most


# ------------------------------------------------------------------------------------------------ 7. underflow
@pytest.mark.parametrize("form", ["dense", "lower", "none"])
def test_logits_far_apart(gpu, form):
    """Gaps of 200 between logits: exp(t) is 0 in float32 for most classes and e * t must not turn into 0 * inf.  Row 0
    has nothing but gaps (its entropy is 0 in float32 and 1e-85 in float64), the others keep two or more classes close to
    the top, so the entropies the relative error is taken over are of order 1."""
    N, K, S = 3, 37, 40
    gen = torch.Generator().manual_seed(13)
    M, lower = matrix(K, form, gen, gpu, scale=K ** -0.5)
    mu = -200.0 * torch.arange(K, dtype=torch.float32).repeat(N, 1)
    mu[1, 1] = -0.3
    mu[2, :6] = torch.randn(6, generator=gen)
    mu = mu[:, torch.randperm(K, generator=gen)].contiguous().to(gpu)
    d2 = torch.full((N, K), 1e-4).to(gpu)
    z = torch.randn(N, S, K, generator=gen).to(gpu)
    got = run(gpu, M, lower, d2, mu, S, noise=z)                 # (finite: checked there)
    errs = errors_against_float64(got, M, lower, d2, mu, z)
    print(f"head_mc_moments {form}: logits 200 apart: " + " ".join(f"{name} {e:.3e}" for name, e in errs.items()))
    assert max(errs.values()) < TOL
    assert float(got["entropy"][0]) == 0.0 and float(got["entropy"][1]) > 0.1


# ------------------------------------------------------------------------------------------------ 8. drivers
def head_model(gpu):
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(12, 7), torch.nn.Tanh(), torch.nn.Linear(7, 5)).to(gpu)


def batches(gpu, count=2, N=6):
    gen = torch.Generator().manual_seed(21)
    return [(torch.randn(N, 3, 4, generator=gen).to(gpu), torch.randint(0, 5, (N,), generator=gen).to(gpu))
            for _ in range(count)]


def make_estimator(kind, model, data, add=1.0, multiply=20.0):
    from curvature_amd.curvatures import EFB, KFAC, Diagonal

    def sweep(est):
        for x, labels in data:
            model.zero_grad()
            torch.nn.functional.cross_entropy(model(x), labels).backward()
            est.update(x.shape[0])
    if kind == "Diagonal":
        est = Diagonal(model)
    else:
        kfac = KFAC(model)
        sweep(kfac)
        if kind == "KFAC":
            est = kfac
        else:
            for hook in kfac.hooks:
                hook.remove()
            est = EFB(model, kfac.state)
    if kind != "KFAC":
        sweep(est)
    model.zero_grad()
    est.invert(add=add, multiply=multiply)
    return est


@pytest.mark.parametrize("kind", ["KFAC", "EFB", "Diagonal"])
def test_last_layer_uncertainty(gpu, kind):
    from curvature_amd import ops
    from curvature_amd.evaluate import Uncertainty, last_layer_predictive, last_layer_uncertainty
    model = head_model(gpu)
    data = batches(gpu)
    est = make_estimator(kind, model, data)
    model.eval()
    N, K, S = 4, 5, 70
    gen = torch.Generator().manual_seed(40)
    x = torch.randn(N, 3, 4, generator=gen).to(gpu)
    z = torch.randn(N, S, K, generator=gen).to(gpu)

    result = last_layer_uncertainty(model, est, x, samples=S, noise=z)
    assert isinstance(result, Uncertainty)
    assert [tuple(t.shape) for t in result] == [(N, K)] * 4 + [(N,)] * 3

    # the composition of head_terms, head_mc_moments and the formulas
    with torch.no_grad():
        features = model[:3](x)
        logits = model(x)
    terms = est.head_terms(model[3], features)
    probs, probs_sq = torch.empty(N, K, device=gpu), torch.empty(N, K, device=gpu)
    entropy = torch.empty(N, device=gpu)
    ops.head_mc_moments([ops.HeadMomentsJob(terms.M, terms.d2, logits.float().contiguous(), S, lower=terms.lower, noise=z,
                                            probs=probs, entropy=entropy, probs_sq=probs_sq)])
    total = -torch.xlogy(probs, probs).sum(dim=1)
    assert torch.equal(result.logits, logits) and torch.equal(result.variance, terms.variance)
    assert torch.equal(result.probs, probs) and torch.equal(result.aleatoric, entropy) and torch.equal(result.total, total)
    assert torch.equal(result.epistemic, torch.clamp(total - entropy, min=0.0))
    assert torch.equal(result.probs_std, torch.sqrt(torch.clamp(probs_sq - probs * probs, min=0.0)))

    # the predictive of last_layer_predictive("mc"), bit for bit
    plain = last_layer_predictive(model, est, x, predictive="mc", samples=S, noise=z)
    for mine, theirs in zip(result[:3], plain):
        assert torch.equal(mine, theirs)

    # against float64: the mutual information relative to the total entropy
    p64, h64, sq64, _ = head_moments_reference(terms.M, terms.lower, terms.d2, logits.float(), z)
    total64 = entropy_of(p64)
    scale = float(torch.linalg.norm(total64))
    e_total, e_alea = rel2(result.total, total64), rel2(result.aleatoric, h64)
    e_epi = float(torch.linalg.norm(result.epistemic.double().cpu() - (total64 - h64))) / scale
    e_std = rel2(result.probs_std, torch.sqrt(torch.clamp(sq64 - p64 ** 2, min=0.0)))
    print(f"last_layer_uncertainty {kind}: total {e_total:.3e} aleatoric {e_alea:.3e} epistemic / |total| {e_epi:.3e} "
          f"probs_std {e_std:.3e}; mean epistemic {float(result.epistemic.mean()):.3e}")
    assert max(e_total, e_alea, e_epi) < TOL
    difference = result.total - result.aleatoric
    positive = difference > 0
    assert torch.equal(result.epistemic[positive], difference[positive])
    assert bool((result.epistemic >= 0).all()) and bool((result.probs_std >= 0).all())
    assert bool((result.total >= result.aleatoric - TOL * scale).all())             # Jensen

    # explicit noise is reproducible and leaves the stream alone; the stream advances by N S ceil(K / 4)
    est.noise_seed, est.noise_offset = 77, 10
    again = last_layer_uncertainty(model, est, x, samples=S, noise=z)
    assert est.noise_offset == 10 and all(torch.equal(a, b) for a, b in zip(again, result))
    first = last_layer_uncertainty(model, est, x, samples=S)
    assert est.noise_offset == 10 + N * S * 2
    second = last_layer_uncertainty(model, est, x, samples=S)
    assert est.noise_offset == 10 + 2 * N * S * 2 and not torch.equal(first.probs, second.probs)
    est.noise_offset = 10
    assert torch.equal(last_layer_uncertainty(model, est, x, samples=S).aleatoric, first.aleatoric)
    est.noise_offset = 10
    assert torch.equal(last_layer_predictive(model, est, x, predictive="mc", samples=S)[2], first.probs)


@pytest.mark.parametrize("kind", ["KFAC", "EFB", "Diagonal"])
def test_a_tighter_posterior_is_less_epistemic(gpu, kind):
    from curvature_amd.evaluate import last_layer_uncertainty
    model = head_model(gpu)
    est = make_estimator(kind, model, batches(gpu))
    model.eval()
    gen = torch.Generator().manual_seed(41)
    x = torch.randn(4, 3, 4, generator=gen).to(gpu)
    z = torch.randn(4, 256, 5, generator=gen).to(gpu)
    est.invert(add=1e-2, multiply=20.0)
    loose = last_layer_uncertainty(model, est, x, noise=z)
    est.invert(add=1e6, multiply=20.0)
    tight = last_layer_uncertainty(model, est, x, noise=z)
    print(f"{kind}: mean epistemic {float(loose.epistemic.mean()):.3e} (add 1e-2) {float(tight.epistemic.mean()):.3e} "
          f"(add 1e6)")
    assert float(tight.epistemic.mean()) < float(loose.epistemic.mean())
    assert float(tight.probs_std.mean()) < float(loose.probs_std.mean())


@pytest.mark.parametrize("kind", ["KFAC", "EFB", "Diagonal"])
def test_eval_uncertainty(gpu, kind):
    from curvature_amd.evaluate import eval_uncertainty, last_layer_uncertainty
    model = head_model(gpu)
    data = batches(gpu)
    est = make_estimator(kind, model, data)
    again = make_estimator(kind, model, data)
    model.eval()
    gen = torch.Generator().manual_seed(30)
    dataset = [(torch.randn(n, 3, 4, generator=gen), torch.randint(0, 5, (n,), generator=gen)) for n in (4, 3)]
    params = [p.detach().clone() for p in model.parameters()]
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.25)
    hooks = [(len(m._forward_hooks), len(m._forward_pre_hooks), len(m._backward_hooks)) for m in model.modules()]
    N, K, S = 7, 5, 64
    est.noise_seed, est.noise_offset = 77, 10
    again.noise_seed, again.noise_offset = 77, 10
    out = eval_uncertainty(model, dataset, est, samples=S)
    assert sorted(out) == ["aleatoric", "epistemic", "labels", "probs", "total"]
    assert est.noise_offset == 10 + N * S * 2
    single = [last_layer_uncertainty(model, again, x.to(gpu), samples=S) for x, _ in dataset]
    assert out["probs"].shape == (N, K) and out["labels"].shape == (N,)
    for key in ("probs", "total", "aleatoric", "epistemic"):
        assert out[key].shape[0] == N
        assert torch.equal(torch.from_numpy(out[key]), torch.cat([getattr(s, key) for s in single]).cpu()), key
    assert torch.equal(torch.from_numpy(out["labels"]), torch.cat([l for _, l in dataset]))
    for p, before in zip(model.parameters(), params):
        assert torch.equal(p.detach(), before) and torch.equal(p.grad, torch.full_like(p, 0.25))
    assert hooks == [(len(m._forward_hooks), len(m._forward_pre_hooks), len(m._backward_hooks)) for m in model.modules()]
    assert not any(m.training for m in model.modules())
    again.use_device_noise_counter(True)
    with pytest.raises(RuntimeError, match="device noise counter"):
        last_layer_uncertainty(model, again, dataset[0][0].to(gpu), samples=S)


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals(gpu):
    from curvature_amd import ops
    from curvature_amd.curvatures import INF, BlockDiagonal, Diagonal
    from curvature_amd.evaluate import last_layer_uncertainty
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
        last_layer_uncertainty(model, block, x)
    inf = object.__new__(INF)                                      # (the refusal needs none of its factors)
    inf.model, inf.shard, inf.inv_state = model, None, {model[3]: torch.ones(1, device=gpu)}
    with pytest.raises(NotImplementedError, match=r"INF.head_terms: layer '3'.*INF"):
        last_layer_uncertainty(model, inf, x)

    post = torch.nn.Sequential(*model, torch.nn.LogSoftmax(dim=1))
    with pytest.raises(RuntimeError, match="'3'.*post-processes"):
        last_layer_uncertainty(post, est, x)
    with pytest.raises(RuntimeError, match="'3'.*did not run"):
        last_layer_uncertainty(model[:3], est, x)

    torch.manual_seed(1)
    tokens = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.ReLU(), torch.nn.Linear(5, 4)).to(gpu)
    token_est = types.SimpleNamespace(model=tokens, inv_state={tokens[2]: torch.ones(4, 6, device=gpu)})
    with pytest.raises(RuntimeError, match=r"'2'.*\(2, 3, 5\).*per token"):
        last_layer_uncertainty(tokens, token_est, torch.randn(2, 3, 6, device=gpu))

    cap = ops.HEAD_MC_MAX_CLASSES
    torch.manual_seed(2)
    wide = torch.nn.Sequential(torch.nn.Linear(8, cap + 1)).to(gpu)
    xw, yw = torch.randn(4, 8, device=gpu), torch.randint(0, cap + 1, (4,), device=gpu)
    wide_est = Diagonal(wide)
    torch.nn.functional.cross_entropy(wide(xw), yw).backward()
    wide_est.update(4)
    wide_est.invert(add=1.0, multiply=10.0)
    before = wide_est.noise_offset
    with pytest.raises(ValueError, match=rf"{cap + 1} classes.*HEAD_MC_MAX_CLASSES = {cap}"):
        last_layer_uncertainty(wide, wide_est, xw, samples=8)
    assert wide_est.noise_offset == before
