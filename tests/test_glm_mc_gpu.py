"""Monte-Carlo softmax of the GLM predictive from the joint logit covariance on the GPU: csrc/logit_mc.hip through
`ops.logit_mc` against float64, its semidefinite rule, its noise stream, and `evaluate.glm_predictive_mc` / `eval_glm`
end to end.

Expected values are computed here, in float64 on the CPU, from the same fp32 inputs: an explicit-loop Cholesky with the
kernel's drop rule (thr = 16 * 2^-23 * max diagonal; a pivot <= thr gives a zero column), f = mu + z L^T, a softmax over
[f, rest] and the mean over the draws.  The bar is the project's (`TOL` of tests/test_glm_covariance_gpu.py): relative
Frobenius error below 1e-4 against float64.  Measured on an MI355X: see DESIGN.md K11."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4
CHUNK = 256                  # the shortest chunk of the plan (include/curv_hip.h): few inputs -> S = 257 is two chunks


def rel2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    denom = float(torch.linalg.norm(b))
    return float(torch.linalg.norm(a - b)) / denom if denom > 0 else float(torch.linalg.norm(a - b))


# ------------------------------------------------------------------------------------------------ float64 reference
def chol_drop(sigma):
    """Lower Cholesky factors of the (N, K, K) float64 blocks with the drop rule, reading lower triangles only;
    (L, info) with info = dropped columns, or -(j + 1) for the first pivot below -thr."""
    N, K, _ = sigma.shape
    L = torch.zeros(N, K, K, dtype=torch.float64)
    info = torch.zeros(N, dtype=torch.int32)
    for n in range(N):
        thr = 16.0 * 2.0 ** -23 * max(float(torch.diagonal(sigma[n]).max()), 0.0)
        dropped = bad = 0
        for j in range(K):
            d = float(sigma[n, j, j] - (L[n, j, :j] ** 2).sum())
            if d <= thr:
                dropped += 1
                if bad == 0 and d < -thr:
                    bad = -(j + 1)
                continue
            L[n, j, j] = math.sqrt(d)
            L[n, j + 1:, j] = (sigma[n, j + 1:, j] - L[n, j + 1:, :j] @ L[n, j, :j]) / L[n, j, j]
        info[n] = bad if bad else dropped
    return L, info


def reference(sigma, mu, rest, z):
    """(probs, probs_rest, draws, info) in float64 from fp32 inputs on any device; `sigma` may hold anything above the
    diagonals."""
    sigma, mu, z = sigma.double().cpu(), mu.double().cpu(), z.double().cpu()
    L, info = chol_drop(torch.tril(sigma.nan_to_num(0.0)))
    draws = mu[:, None, :] + torch.einsum("nsk,nck->nsc", z, L)
    everything = draws
    if rest is not None:
        everything = torch.cat([draws, rest.double().cpu()[:, None, None].expand(-1, draws.shape[1], 1)], dim=2)
    p = torch.softmax(everything, dim=2).mean(dim=1)
    K = mu.shape[1]
    left = p[:, K] if rest is not None else torch.zeros(mu.shape[0], dtype=torch.float64)
    return p[:, :K], left, draws, info


# ------------------------------------------------------------------------------------------------ inputs
def definite_blocks(N, K, gen, gpu):
    """B B^T + I per input, in a buffer with o_rs = K + 3, five more floats between the blocks, NaN everywhere the kernel
    must not read: between the entries and in the strict upper triangles.  Returns (view, dense float64 blocks)."""
    B = torch.randn(N, K, K, generator=gen)
    dense = (B @ B.transpose(1, 2) + torch.eye(K)).float()
    o_rs, o_ns = K + 3, K * (K + 3) + 5
    buf = torch.full((N * o_ns,), float("nan"))
    view = buf.as_strided((N, K, K), (o_ns, o_rs, 1))
    view.copy_(torch.tril(dense) + torch.triu(torch.full((K, K), float("nan")), diagonal=1))
    dev = buf.to(gpu)
    return dev.as_strided((N, K, K), (o_ns, o_rs, 1)), dense.double()


def padded_rows(values, gpu):
    """(N, K) values as a view with row stride K + 2 into a NaN-filled buffer."""
    N, K = values.shape
    buf = torch.full((N, K + 2), float("nan"))
    buf[:, :K] = values
    return buf.to(gpu)[:, :K]


def run(gpu, cov, mu, S, rest=None, noise=None, seed=0, offset=0, draws=True):
    from curvature_amd import ops
    N, K = mu.shape
    out = dict(probs=torch.empty(N, K, device=gpu), probs_rest=torch.empty(N, device=gpu),
               info=torch.empty(N, dtype=torch.int32, device=gpu))
    if draws:
        out["draws"] = torch.empty(N, S, K, device=gpu)
    ops.logit_mc([ops.LogitMCJob(cov, mu, S, rest=rest, noise=noise, seed=seed, offset=offset, **out)])
    torch.cuda.synchronize()
    return out


def check_against_float64(gpu, N, K, S, with_rest, gen):
    cov, dense = definite_blocks(N, K, gen, gpu)
    mu_cpu = torch.randn(N, K, generator=gen) * 2
    mu = padded_rows(mu_cpu, gpu)
    rest = (torch.randn(N, generator=gen) + 1).to(gpu) if with_rest else None
    z = torch.randn(N, S, K, generator=gen).to(gpu)
    got = run(gpu, cov, mu, S, rest=rest, noise=z)
    probs, left, draws, info = reference(cov, mu, rest, z)
    assert torch.isfinite(got["probs"]).all() and torch.isfinite(got["draws"]).all()
    assert torch.equal(got["info"].cpu(), torch.zeros(N, dtype=torch.int32)) and not info.any()
    errs = [rel2(got["probs"], probs), rel2(got["draws"], draws)]
    if with_rest:
        errs.append(rel2(got["probs_rest"], left))
    else:
        assert torch.equal(got["probs_rest"].cpu(), torch.zeros(N))
    # L's effect against LAPACK's factor of the dense float64 block
    lapack = torch.linalg.cholesky(dense)
    errs.append(rel2(got["draws"], mu_cpu.double()[:, None, :] + torch.einsum("nsk,nck->nsc", z.double().cpu(), lapack)))
    # probs is the mean of the softmax of the kernel's own draws
    own = got["draws"].double().cpu()
    if with_rest:
        own = torch.cat([own, rest.double().cpu()[:, None, None].expand(-1, S, 1)], dim=2)
    errs.append(rel2(got["probs"], torch.softmax(own, dim=2).mean(dim=1)[:, :K]))
    return max(errs)


# ------------------------------------------------------------------------------------------------ 1. the primitive
@pytest.mark.parametrize("N", [1, 3, 70])
@pytest.mark.parametrize("K", [1, 3, 4, 5, 10, 16])
def test_logit_mc_against_float64(gpu, K, N):
    """Both sides of a Philox quad and the limit in K; S on both sides of a wave and of a chunk (few inputs: chunks of 256
    draws, so 257 is two chunks and 1000 four - the workspace path - and the others one); rest present and NULL; padded
    cov and mu with NaN wherever the kernel must not read."""
    gen = torch.Generator().manual_seed(100 * K + N)
    worst = 0.0
    for S in (1, 63, 64, 65, CHUNK + 1, 1000):
        for with_rest in (True, False):
            err = check_against_float64(gpu, N, K, S, with_rest, gen)
            print(f"K {K} N {N} S {S} rest {with_rest}: worst rel Frobenius error {err:.3e}")
            worst = max(worst, err)
    print(f"K {K} N {N}: worst {worst:.3e}")
    assert worst < TOL


@pytest.mark.parametrize("N,K,S", [(600, 3, 1000), (1100, 5, 600)], ids=["two_chunks_of_512", "one_chunk_of_768"])
def test_many_inputs_take_longer_chunks(gpu, N, K, S):
    """From about a thousand inputs on a lane owns several draws: chunks of 512 (two per input, through the workspace) and
    one chunk of 768 with a ragged last round (written by the kernel itself)."""
    err = check_against_float64(gpu, N, K, S, True, torch.Generator().manual_seed(N))
    print(f"N {N} K {K} S {S}: worst rel Frobenius error {err:.3e}")
    assert err < TOL


# ------------------------------------------------------------------------------------------------ 2. semidefinite blocks
def test_zero_covariance_is_the_softmax(gpu):
    gen = torch.Generator().manual_seed(7)
    for K in (1, 5, 16):
        mu = (torch.randn(3, K, generator=gen) * 3).to(gpu)
        z = torch.randn(3, 300, K, generator=gen).to(gpu)
        got = run(gpu, torch.zeros(3, K, K, device=gpu), mu, 300, noise=z)
        assert torch.equal(got["info"].cpu(), torch.full((3,), K, dtype=torch.int32))
        want = torch.softmax(mu.double().cpu(), dim=1)
        assert float((got["probs"].double().cpu() - want).abs().max()) < 1e-6
        assert torch.equal(got["draws"], mu[:, None, :].expand(-1, 300, -1))


def test_rank_one_covariance(gpu):
    gen = torch.Generator().manual_seed(8)
    v = torch.tensor([[1.5, -0.7, 0.3, 2.1], [0.4, 0.9, -1.3, 0.2]], dtype=torch.float64)
    sigma = (v[:, :, None] * v[:, None, :]).float()                     # formed in float64, rounded to fp32
    _, info = chol_drop(sigma.double())
    assert info.tolist() == [3, 3], "the case must drop exactly three pivots under the stated threshold"
    mu = torch.randn(2, 4, generator=gen).to(gpu)
    z = torch.randn(2, 500, 4, generator=gen).to(gpu)
    got = run(gpu, sigma.to(gpu), mu, 500, noise=z)
    assert got["info"].tolist() == [3, 3]
    assert all(bool(torch.isfinite(t).all()) for t in (got["probs"], got["probs_rest"], got["draws"]))
    want = mu.double().cpu()[:, None, :] + v[:, None, :] * z.double().cpu()[:, :, :1]
    err = rel2(got["draws"], want)
    probs, _, _, _ = reference(sigma, mu, None, z)
    print(f"rank one: draws {err:.3e} probs {rel2(got['probs'], probs):.3e}")
    assert err < TOL and rel2(got["probs"], probs) < TOL


def negative_block(gpu):
    sigma = torch.eye(4).repeat(3, 1, 1)
    sigma[1, 2, 2] = -1.0
    return sigma.to(gpu)


def test_a_negative_pivot_is_named_and_dropped(gpu):
    gen = torch.Generator().manual_seed(9)
    sigma = negative_block(gpu)
    mu = torch.randn(3, 4, generator=gen).to(gpu)
    z = torch.randn(3, 100, 4, generator=gen).to(gpu)
    got = run(gpu, sigma, mu, 100, noise=z)
    assert got["info"].tolist() == [0, -3, 0]
    assert all(bool(torch.isfinite(t).all()) for t in (got["probs"], got["probs_rest"], got["draws"]))
    probs, _, draws, info = reference(sigma, mu, None, z)
    assert info.tolist() == [0, -3, 0]
    assert rel2(got["probs"], probs) < TOL and rel2(got["draws"], draws) < TOL

    from curvature_amd.evaluate import mc_softmax
    with pytest.raises(RuntimeError, match="input 1"):
        mc_softmax(mu, sigma, [0, 1, 2, 3], 100, noise=z, what="glm_predictive_mc")


# ------------------------------------------------------------------------------------------------ 3. noise
@pytest.mark.parametrize("K", [5, 16])
def test_implicit_noise_is_the_explicit_stream(gpu, K):
    from curvature_amd import ops
    N, S, Kq, seed, offset = 3, 300, (K + 3) // 4, 1234567, 77
    gen = torch.Generator().manual_seed(K)
    cov, _ = definite_blocks(N, K, gen, gpu)
    mu = torch.randn(N, K, generator=gen).to(gpu)
    rest = torch.randn(N, generator=gen).to(gpu)
    z = ops.randn((N, S, 4 * Kq), gpu, seed, offset)[:, :, :K]
    explicit = run(gpu, cov, mu, S, rest=rest, noise=z)
    implicit = run(gpu, cov, mu, S, rest=rest, seed=seed, offset=offset)
    again = run(gpu, cov, mu, S, rest=rest, seed=seed, offset=offset)
    for key in ("probs", "probs_rest", "draws", "info"):
        assert torch.equal(explicit[key], implicit[key]), key
        assert torch.equal(implicit[key], again[key]), key
    other = run(gpu, cov, mu, S, rest=rest, seed=seed, offset=offset + N * S * Kq)
    assert not torch.equal(other["draws"], implicit["draws"])


def test_an_item_has_the_same_bits_alone_and_in_a_batch(gpu):
    from curvature_amd import ops
    gen = torch.Generator().manual_seed(11)
    shapes = [(3, 5, 1000), (70, 16, 64), (2, 1, 300)]             # (N, K, S): chunks, one chunk, chunks
    jobs, outs = [], []
    for i, (N, K, S) in enumerate(shapes):
        cov, _ = definite_blocks(N, K, gen, gpu)
        mu = torch.randn(N, K, generator=gen).to(gpu)
        outs.append([dict(probs=torch.empty(N, K, device=gpu), probs_rest=torch.empty(N, device=gpu)) for _ in range(2)])
        jobs.append([ops.LogitMCJob(cov, mu, S, rest=torch.zeros(N, device=gpu), seed=5, offset=1000 * i, **o)
                     for o in outs[-1]])
    ops.logit_mc([j[0] for j in jobs])
    for j in jobs:
        ops.logit_mc([j[1]])
    torch.cuda.synchronize()
    for together, alone in outs:
        assert torch.isfinite(together["probs"]).all()
        assert torch.equal(together["probs"], alone["probs"]) and torch.equal(together["probs_rest"], alone["probs_rest"])


def test_moments_of_the_implicit_draws(gpu):
    """Sample mean and covariance of the draws within 6 standard errors under the normal model:
    se(mean_c) = sqrt(Sigma_cc / S), se(cov_cc') = sqrt((Sigma_cc Sigma_c'c' + Sigma_cc'^2) / S).  The seed is fixed, so
    is the outcome."""
    N, K, S = 2, 3, 4096
    gen = torch.Generator().manual_seed(12)
    cov, dense = definite_blocks(N, K, gen, gpu)
    mu = torch.randn(N, K, generator=gen).to(gpu)
    draws = run(gpu, cov, mu, S, seed=20260101, offset=3)["draws"].double().cpu()
    mu64 = mu.double().cpu()
    var = torch.diagonal(dense, dim1=1, dim2=2)
    mean_dev = (draws.mean(dim=1) - mu64).abs() / torch.sqrt(var / S)
    centred = draws - mu64[:, None, :]
    sample_cov = torch.einsum("nsc,nsd->ncd", centred, centred) / S
    se = torch.sqrt((var[:, :, None] * var[:, None, :] + dense ** 2) / S)
    cov_dev = (sample_cov - dense).abs() / se
    print(f"moments: mean off by {float(mean_dev.max()):.2f} se, covariance by {float(cov_dev.max()):.2f} se")
    assert float(mean_dev.max()) < 6 and float(cov_dev.max()) < 6


# ------------------------------------------------------------------------------------------------ 4. end to end
def small_model(gpu):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3, padding=1), torch.nn.Flatten(), torch.nn.Linear(75, 4))
    return model.to(gpu)


def make_estimator(kind, model, x, labels):
    """`kind` after one update on the batch (x, labels) and an inversion."""
    from curvature_amd.curvatures import EFB, KFAC, Diagonal

    def backward():
        model.zero_grad()
        torch.nn.functional.cross_entropy(model(x), labels).backward()
    if kind == "diag":
        est = Diagonal(model)
    else:
        kfac = KFAC(model)
        backward()
        kfac.update(x.shape[0])
        if kind == "kfac":
            est = kfac
        else:
            for hook in kfac.hooks:
                hook.remove()
            est = EFB(model, kfac.state)
    if kind != "kfac":
        backward()
        est.update(x.shape[0])
    est.invert(add=0.5, multiply=2.0)
    return est


def full_reference(logits, covariance, classes, z):
    """(N, classes) expected softmax in float64, the logits that are not selected held constant."""
    logits, z = logits.double().cpu(), z.double().cpu()
    L, _ = chol_drop(torch.tril(covariance.double().cpu()))
    f = logits[:, None, :].repeat(1, z.shape[1], 1)
    f[:, :, classes] = f[:, :, classes] + torch.einsum("nsk,nck->nsc", z, L)
    return torch.softmax(f, dim=2).mean(dim=1)


@pytest.mark.parametrize("kind", ["kfac", "diag", "efb"])
def test_glm_predictive_mc(gpu, kind):
    from curvature_amd.evaluate import glm_predictive_joint, glm_predictive_mc
    model = small_model(gpu)
    torch.manual_seed(4)
    x, labels = torch.randn(3, 2, 5, 5, device=gpu), torch.tensor([0, 3, 1], device=gpu)
    est = make_estimator(kind, model, x, labels)
    N, S = 3, 500
    logits_j, cov_j, _ = glm_predictive_joint(model, est, x)
    had_hooks = hasattr(est, "hooks")
    params = [p.detach().clone() for p in model.parameters()]
    grads = [None if p.grad is None else p.grad.clone() for p in model.parameters()]

    z = torch.randn(N, S, 4, device=gpu)
    logits, cov, probs, draws = glm_predictive_mc(model, est, x, samples=S, noise=z, return_draws=True)
    assert torch.equal(logits, logits_j) and torch.equal(cov, cov_j)
    assert tuple(probs.shape) == (N, 4) and tuple(draws.shape) == (N, S, 4)
    err = rel2(probs, full_reference(logits, cov, [0, 1, 2, 3], z))
    assert float((probs.sum(dim=1) - 1).abs().max()) < 1e-5

    # a subset: the two unselected logits are constants and share what is left by their softmax weights
    z2 = torch.randn(N, S, 2, device=gpu)
    logits2, cov2, probs2 = glm_predictive_mc(model, est, x, outputs=[3, 1], samples=S, noise=z2)
    lj, cj, _ = glm_predictive_joint(model, est, x, outputs=[3, 1])
    assert torch.equal(logits2, lj) and torch.equal(cov2, cj) and tuple(cov2.shape) == (N, 2, 2)
    err2 = rel2(probs2, full_reference(logits2, cov2, [3, 1], z2))
    assert float((probs2.sum(dim=1) - 1).abs().max()) < 1e-5
    share = probs2[:, [0, 2]] / probs2[:, [0, 2]].sum(dim=1, keepdim=True)
    assert float((share - torch.softmax(logits2[:, [0, 2]], dim=1)).abs().max()) < 1e-5
    print(f"{kind}: probs against float64: all outputs {err:.3e}, outputs [3, 1] {err2:.3e}")
    assert err < TOL and err2 < TOL

    # the estimator's own stream: pinned by noise_seed / noise_offset, advanced by N S Kq
    est.noise_seed, est.noise_offset = 99, 40
    first = glm_predictive_mc(model, est, x, samples=S)[2]
    assert est.noise_offset == 40 + N * S * 1
    later = glm_predictive_mc(model, est, x, outputs=[3, 1], samples=7)[2]
    assert est.noise_offset == 40 + N * S + N * 7
    est.noise_offset = 40
    assert torch.equal(glm_predictive_mc(model, est, x, samples=S)[2], first)
    assert float((first.sum(dim=1) - 1).abs().max()) < 1e-5 and float((later.sum(dim=1) - 1).abs().max()) < 1e-5

    # left as glm_predictive_joint leaves it
    assert hasattr(est, "hooks") == had_hooks
    assert not est.__dict__.get("_predictive_kept")
    for p, before, grad in zip(model.parameters(), params, grads):
        assert torch.equal(p.detach(), before)
        assert (p.grad is None) == (grad is None) and (grad is None or torch.equal(p.grad, grad))


def test_eval_glm(gpu):
    from curvature_amd.evaluate import eval_glm, glm_predictive
    model = small_model(gpu)
    torch.manual_seed(4)
    x, labels = torch.randn(5, 2, 5, 5, device=gpu), torch.tensor([0, 3, 1, 2, 2], device=gpu)
    est = make_estimator("kfac", model, x, labels)
    dataset = [(x[:3].cpu(), labels[:3].cpu()), (x[3:].cpu(), labels[3:].cpu())]
    predictions, got_labels = eval_glm(model, dataset, est)
    want = torch.cat([glm_predictive(model, est, b.to(gpu))[2] for b, _ in dataset]).cpu().numpy()
    assert (predictions == want).all() and got_labels.tolist() == labels.tolist()
    est.noise_seed, est.noise_offset = 5, 0
    predictions, got_labels = eval_glm(model, dataset, est, predictive="mc", samples=64)
    assert predictions.shape == (5, 4) and got_labels.tolist() == labels.tolist()
    assert float(abs(predictions.sum(axis=1) - 1).max()) < 1e-5
    assert est.noise_offset == 5 * 64
