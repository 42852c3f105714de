"""Joint output covariance of the linearised Laplace (GLM) predictive on the GPU: the Gram reduction of csrc/persample.hip
through `ops.per_sample_cov_reduce` against float64, `Curvature.stage_output` / `functional_covariance` through
`evaluate.glm_predictive_joint` against the estimator's own sampler and against a float64 restatement on LeNet-5, and
the error paths.

Expected values are computed here, in float64 on the CPU, from the same fp32 inputs.  The bar is the project's (`TOL` of
tests/test_per_sample_gpu.py): relative Frobenius error below 1e-4 against float64."""
import functools
import math
from collections import OrderedDict

import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4


def rel2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


# ------------------------------------------------------------------------------------------------ 1. the primitive
# (S, K, M, Nc, L)
SHAPES = [
    (5, 3, 37, 70, 37),      # K not a multiple of 4, ragged in both sides, l tail
    (4, 16, 6, 151, 100),    # largest K, tiny M, several stages per sample
    (33, 10, 150, 16, 1),    # L = 1, narrow Nc, M beyond one tile
    (100, 10, 10, 85, 1),    # LeNet-5's last layer
    (200, 1, 16, 26, 5),     # K = 1, many samples: sample ranges if the plan splits
    (3, 5, 130, 150, 49),    # several tiles on both sides, the 49-pixel row
]
K1 = 4                       # index of the K = 1 shape
ALPHA = 1.5
SENTINEL = 7.0


def strided_operand(slots, S, rows, L, gen, gpu):
    """(slots, S, rows, L) random values whose rows are `rs` > L floats apart, whose samples are more than rows * rs apart and
    whose slots are more than S samples apart, in a buffer that holds NaN everywhere else: the gaps, and what lies behind
    the last row.  (Strides are multiples of 4 floats: every row starts on a 16-byte boundary, as the rows of the library's
    own packed operands do.)  Returns the GPU view from the first value on, the float64 values and (cs, ns, rs)."""
    rs = (L + 3) // 4 * 4 + 4
    ns = rows * rs + 8
    cs = S * ns + 12
    buf = torch.full((64 + slots * cs + 64,), float("nan"))
    vals = torch.randn(slots, S, rows, L, generator=gen)
    view = buf[64:64 + slots * cs].view(slots, cs)[:, :S * ns].view(slots, S, ns)[:, :, :rows * rs].view(slots, S, rows, rs)
    view[..., :L] = vals
    return buf.to(gpu)[64:], vals.double(), (cs, ns, rs)


@functools.lru_cache(maxsize=None)
def primitive_case(index, weighted):
    """The operands of SHAPES[index] on the GPU and the float64 value of the Gram (alpha included); made once."""
    S, K, M, Nc, L = SHAPES[index]
    gpu = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(300 + index)
    A, A64, (a_cs, a_ns, a_rs) = strided_operand(K, S, M, L, gen, gpu)
    B, B64, (_, b_ns, b_rs) = strided_operand(1, S, Nc, L, gen, gpu)
    W = W64 = None
    if weighted:
        wide = torch.full((M, Nc + 3), float("nan"))
        wide[:, :Nc] = torch.rand(M, Nc, generator=gen) + 0.1
        W64 = wide[:, :Nc].double()
        W = wide.to(gpu)[:, :Nc]                                   # row stride Nc + 3, NaN in the gap
    P = torch.einsum("ksml,snl->ksmn", A64, B64[0])
    want = ALPHA * torch.einsum("ksmn,tsmn->skt", P if W64 is None else P * W64, P)
    return dict(A=A, B=B, W=W, sizes=(S, M, Nc, L), K=K, a_cs=a_cs, strides=(a_ns, a_rs, b_ns, b_rs), want=want)


def cov_job(case, out, first):
    from curvature_amd import ops
    return ops.PerSampleCovJob(case["A"], case["B"], case["W"], out, case["K"], case["a_cs"], *case["sizes"],
                               *case["strides"], alpha=ALPHA, first=first)


def strided_out(S, K, gpu):
    """An (S, K, K) view with row stride K + 1 and sample stride K (K + 1) + 2 that holds NaN, in a buffer of sentinels;
    and the mask of the buffer's entries outside the view."""
    o_rs = K + 1
    o_ns = K * o_rs + 2
    buf = torch.full((S * o_ns,), SENTINEL, device=gpu)
    out = torch.as_strided(buf, (S, K, K), (o_ns, o_rs, 1))
    out.fill_(float("nan"))
    gaps = torch.ones_like(buf, dtype=torch.bool)
    torch.as_strided(gaps, (S, K, K), (o_ns, o_rs, 1)).fill_(False)
    return buf, out, gaps


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "W"])
@pytest.mark.parametrize("index", range(len(SHAPES)), ids=["x".join(map(str, s)) for s in SHAPES])
def test_cov_reduce_against_float64(gpu, index, weighted):
    from curvature_amd import ops
    case = primitive_case(index, weighted)
    S, M, Nc, L = case["sizes"]
    K = case["K"]
    assert ops.per_sample_cov_plan_flops([cov_job(case, None, True)])[0] >= 2 * S * K * M * Nc * L
    buf, out, gaps = strided_out(S, K, gpu)
    ops.per_sample_cov_reduce([cov_job(case, out, True)])              # `first` overwrites the NaNs
    err = rel2(out, case["want"])
    got = out.double().cpu()
    worst = max(rel2(got[s], case["want"][s]) for s in range(S))
    print(f"cov reduce {SHAPES[index]} weighted={weighted}: rel Frobenius error {err:.3e}, worst sample {worst:.3e}")
    assert err < TOL
    assert worst < TOL
    assert torch.equal(out, out.transpose(1, 2))                       # bit for bit
    once = out.clone()
    ops.per_sample_cov_reduce([cov_job(case, out, False)])             # accumulates: twice the value
    assert torch.equal(out, once + once)
    assert bool((buf[gaps] == SENTINEL).all())


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "W"])
def test_one_output_is_the_quadratic_reduction(gpu, weighted):
    """K = 1: the same sum as `ops.per_sample_quad_reduce` on the same operands (another tiling, so not the same bits)."""
    from curvature_amd import ops
    case = primitive_case(K1, weighted)
    S = case["sizes"][0]
    assert case["K"] == 1
    cov = torch.empty(S, 1, 1, device=gpu)
    ops.per_sample_cov_reduce([cov_job(case, cov, True)])
    quad = torch.empty(S, device=gpu)
    ops.per_sample_quad_reduce([ops.PerSampleQuadJob(case["A"], case["B"], case["W"], quad, *case["sizes"],
                                                     *case["strides"], alpha=ALPHA, first=True)])
    want = case["want"].flatten()
    print(f"K = 1 weighted={weighted}: cov {rel2(cov, want):.3e}, quad {rel2(quad, want):.3e}, "
          f"cov against quad {rel2(cov, quad):.3e}")
    assert rel2(cov, want) < TOL and rel2(quad, want) < TOL
    assert rel2(cov, quad) < 2 * TOL


def test_an_item_has_the_same_bits_alone_and_in_a_batch(gpu):
    """All twelve items (six shapes, with W and without) in one call against twelve calls of one item."""
    from curvature_amd import ops
    cases = [primitive_case(i, w) for i in range(len(SHAPES)) for w in (False, True)]
    alone = []
    for case in cases:
        out = strided_out(case["sizes"][0], case["K"], gpu)[1]
        ops.per_sample_cov_reduce([cov_job(case, out, True)])
        alone.append(out.clone())
    outs = [strided_out(case["sizes"][0], case["K"], gpu)[1] for case in cases]
    ops.per_sample_cov_reduce([cov_job(case, out, True) for case, out in zip(cases, outs)])
    for k, (a, b) in enumerate(zip(alone, outs)):
        assert torch.equal(a, b), k


# ------------------------------------------------------------------------------------------------ estimators
def make_estimator(kind, model, x, labels, layer_types=None, per_sample=False):
    """`kind` after one update on the batch (x, labels) and an inversion."""
    from curvature_amd.curvatures import EFB, KFAC, Diagonal
    extra = {"per_sample": True} if per_sample else {}

    def backward():
        model.zero_grad()
        torch.nn.functional.cross_entropy(model(x), labels).backward()
    if kind == "diag":
        est = Diagonal(model, layer_types, **extra)
    else:
        kfac = KFAC(model, layer_types)
        backward()
        kfac.update(x.shape[0])
        if kind == "kfac":
            est = kfac
        else:
            for hook in kfac.hooks:
                hook.remove()
            est = EFB(model, kfac.state, layer_types, **extra)
    if kind != "kfac":
        backward()
        est.update(x.shape[0])
    est.invert(add=0.5, multiply=2.0)
    return est


# ------------------------------------------------------------------------------------------------ 2. the sampler
def linear_model(gpu):
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3, padding=1, bias=True), torch.nn.Flatten(), torch.nn.Linear(75, 4))
    return model.to(gpu)


@pytest.mark.parametrize("kind", ["kfac", "diag", "efb"])
def test_covariance_is_that_of_the_estimators_own_sampler(gpu, kind):
    """The outputs of Conv2d -> Flatten -> Linear are linear in the convolution's [W | b], so the covariance of outputs c
    and c' under the sampler is sum_k df_c(e_k) df_c'(e_k) over the samples drawn from the 57 unit-noise vectors e_k."""
    from curvature_amd.evaluate import glm_predictive_joint
    model = linear_model(gpu)
    torch.manual_seed(4)
    x, labels = torch.randn(3, 2, 5, 5, device=gpu), torch.tensor([0, 3, 1], device=gpu)
    est = make_estimator(kind, model, x, labels, layer_types="Conv2d")
    conv, lin = model[0], model[2]
    _, covariance, _ = glm_predictive_joint(model, est, x)
    assert tuple(covariance.shape) == (3, 4, 4)

    m, n = 3, 19
    x64, head = x.double().cpu(), lin.weight.detach().double().cpu()
    want = torch.zeros(3, 4, 4, dtype=torch.float64)
    for k in range(m * n):
        z = torch.zeros(m * n, device=gpu)
        z[k] = 1.0
        z = z.view(m, n) if kind == "diag" else z.view(n, m)              # the noise shape of each sampler
        d = est.sample(conv, z).double().cpu()                             # (m, n) as [W | b]
        df = torch.nn.functional.conv2d(x64, d[:, :-1].reshape(3, 2, 3, 3), d[:, -1], padding=1).flatten(1) @ head.t()
        want += df.unsqueeze(2) * df.unsqueeze(1)
    err = rel2(covariance, want)
    print(f"{kind}: covariance against the sampler: rel Frobenius error {err:.3e}")
    assert err < TOL


# ------------------------------------------------------------------------------------------------ 3. LeNet-5
N_LENET = 8


@functools.lru_cache(maxsize=None)
def lenet():
    """LeNet-5 on the GPU, a batch, and the float64 per-sample Jacobians of every logit with respect to every layer's
    [W | b]: ``jac[layer index]`` (N, 10, m, n_in + 1), from N * classes backward passes on a CPU copy.  Made once."""
    import copy
    from curvature_amd import models
    gpu = torch.device("cuda:0")
    torch.manual_seed(0)
    model = models.lenet5().to(gpu)
    x = torch.randn(N_LENET, 1, 28, 28, device=gpu)
    labels = torch.randint(0, 10, (N_LENET,), device=gpu)
    ref = copy.deepcopy(model).double().cpu().eval()
    layers = [l for l in ref if isinstance(l, (torch.nn.Conv2d, torch.nn.Linear))]
    logits = ref(x.double().cpu())
    jac = [[[None] * 10 for _ in range(N_LENET)] for _ in layers]
    for n in range(N_LENET):
        for c in range(10):
            grads = torch.autograd.grad(logits[n, c], [p for l in layers for p in (l.weight, l.bias)], retain_graph=True)
            for k in range(len(layers)):
                gw, gb = grads[2 * k], grads[2 * k + 1]
                jac[k][n][c] = torch.cat([gw.reshape(gw.shape[0], -1), gb.reshape(-1, 1)], dim=1)
    jac = [torch.stack([torch.stack(per_n) for per_n in per_layer]) for per_layer in jac]
    return model, x, labels, jac, logits.detach()


@functools.lru_cache(maxsize=None)
def lenet_estimator(kind):
    model, x, labels, _, _ = lenet()
    return make_estimator(kind, model, x, labels, per_sample=kind == "efb")


@functools.lru_cache(maxsize=None)
def float64_covariance(kind):
    """Sigma_n[c, c'] = sum_layers <T(P_c), T(P_c')> with T(P) = L_G^T P L_A (KFAC), inv * P (Diagonal), inv * (U_G^T P U_A)
    (EFB), on the estimator's own inverse state / eigenvectors copied to the host."""
    model, _, _, jac, _ = lenet()
    est = lenet_estimator(kind)
    layers = [l for l in model if isinstance(l, (torch.nn.Conv2d, torch.nn.Linear))]
    want = torch.zeros(N_LENET, 10, 10, dtype=torch.float64)
    for k, layer in enumerate(layers):
        P = jac[k]                                                         # (N, 10, m, n)
        if kind == "kfac":
            L_A, L_G = (t.double().cpu() for t in est.inv_state[layer])
            T = L_G.t() @ P @ L_A
        elif kind == "diag":
            T = est.inv_state[layer].double().cpu() * P
        else:
            U_A, U_G = (t.double().cpu() for t in est.eigvecs[layer])
            T = est.inv_state[layer].double().cpu() * (U_G.t() @ P @ U_A)
        want += torch.einsum("ncij,ndij->ncd", T, T)
    return want


@pytest.mark.parametrize("kind", ["kfac", "diag", "efb"])
def test_lenet_against_float64(gpu, kind):
    from curvature_amd.evaluate import glm_predictive, glm_predictive_joint
    model, x, labels, _, logits64 = lenet()
    est = lenet_estimator(kind)
    model.zero_grad()
    torch.nn.functional.cross_entropy(model(x), labels).backward()            # some .grad to find again afterwards
    before = [(p.detach().clone(), p.grad, p.grad.clone()) for p in model.parameters()]
    hooked = hasattr(est, "hooks")
    _, variance, probs_before = glm_predictive(model, est, x)

    logits, covariance, probs = glm_predictive_joint(model, est, x)

    want = float64_covariance(kind)
    err = rel2(covariance, want)
    diag_err = rel2(torch.diagonal(covariance, dim1=1, dim2=2), variance)
    print(f"{kind}: LeNet-5 covariance: rel Frobenius error {err:.3e}; diagonal against glm_predictive {diag_err:.3e}")
    assert tuple(covariance.shape) == (N_LENET, 10, 10)
    assert err < TOL
    assert diag_err < 2 * TOL
    assert torch.equal(covariance, covariance.transpose(1, 2))
    sigma = covariance.double().cpu()
    for n in range(N_LENET):
        low = float(torch.linalg.eigvalsh(sigma[n])[0])
        bound = -TOL * float(torch.linalg.norm(sigma[n]))
        print(f"  sample {n}: smallest eigenvalue {low:.3e} (bound {bound:.3e})")
        assert low >= bound
    assert rel2(logits, logits64) < TOL
    want_var = torch.diagonal(want, dim1=1, dim2=2)
    probit = torch.softmax(logits.double().cpu() / torch.sqrt(1.0 + math.pi / 8.0 * want_var), dim=1)
    assert float((probs.double().cpu() - probit).abs().max()) < 1e-5
    assert float((probs.sum(1) - 1.0).abs().max()) < 1e-5
    for p, (value, grad, grad_value) in zip(model.parameters(), before):
        assert torch.equal(p.detach(), value) and p.grad is grad and torch.equal(p.grad, grad_value)
    assert hasattr(est, "hooks") == hooked                                     # borrowed hooks are gone again
    assert not getattr(est, "_predictive_kept", None)
    assert not model.training
    _, variance_after, probs_after = glm_predictive(model, est, x)             # the variance path is what it was
    assert torch.equal(variance_after, variance) and torch.equal(probs_after, probs_before)


def test_a_subset_of_the_outputs(gpu):
    from curvature_amd.evaluate import glm_predictive_joint
    model, x, _, _, _ = lenet()
    est = lenet_estimator("kfac")
    logits, part, probs = glm_predictive_joint(model, est, x, outputs=[7, 2])
    assert tuple(part.shape) == (N_LENET, 2, 2)
    want = float64_covariance("kfac")[:, [7, 2]][:, :, [7, 2]]
    err = rel2(part, want)
    print(f"outputs [7, 2]: rel Frobenius error {err:.3e}")
    assert err < TOL
    variance = torch.zeros(N_LENET, 10, dtype=torch.float64)
    variance[:, [7, 2]] = torch.diagonal(want, dim1=1, dim2=2)
    probit = torch.softmax(logits.double().cpu() / torch.sqrt(1.0 + math.pi / 8.0 * variance), dim=1)
    assert float((probs.double().cpu() - probit).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------ 4. error paths
def test_too_many_or_repeated_outputs(gpu):
    from curvature_amd.evaluate import glm_predictive_joint
    torch.manual_seed(6)
    model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(50, 17)).to(gpu)
    x, labels = torch.randn(3, 2, 5, 5, device=gpu), torch.tensor([0, 16, 1], device=gpu)
    est = make_estimator("kfac", model, x, labels)
    with pytest.raises(ValueError, match="outputs="):
        glm_predictive_joint(model, est, x)                                    # 17 classes
    with pytest.raises(ValueError, match="outputs="):
        glm_predictive_joint(model, est, x, outputs=[1, 2, 1])
    _, covariance, _ = glm_predictive_joint(model, est, x, outputs=range(16))  # the largest call is fine
    assert tuple(covariance.shape) == (3, 16, 16) and bool(torch.isfinite(covariance).all())


def test_half_precision_records_are_refused(gpu):
    from curvature_amd.evaluate import glm_predictive_joint
    model = linear_model(gpu)
    x, labels = torch.randn(3, 2, 5, 5, device=gpu), torch.tensor([0, 3, 1], device=gpu)
    est = make_estimator("kfac", model, x, labels, layer_types="Conv2d")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(RuntimeError, match="bfloat16"):
            glm_predictive_joint(model, est, x)


def test_a_grouped_convolution_is_named(gpu):
    from curvature_amd.evaluate import glm_predictive_joint
    torch.manual_seed(5)
    model = torch.nn.Sequential(OrderedDict([("plain", torch.nn.Conv2d(2, 4, 3, padding=1)),
                                             ("grouped_one", torch.nn.Conv2d(4, 4, 3, padding=1, groups=2)),
                                             ("flat", torch.nn.Flatten()), ("head", torch.nn.Linear(100, 4))])).to(gpu)
    x, labels = torch.randn(3, 2, 5, 5, device=gpu), torch.tensor([0, 3, 1], device=gpu)
    kfac = make_estimator("kfac", model, x, labels)
    with pytest.raises(NotImplementedError, match="grouped_one"):
        glm_predictive_joint(model, kfac, x)
    for hook in kfac.hooks:
        hook.remove()
    diag = make_estimator("diag", model, x, labels)
    with pytest.raises(NotImplementedError, match="grouped_one"):
        glm_predictive_joint(model, diag, x)
    assert not hasattr(diag, "hooks") and not model.plain._forward_pre_hooks      # nothing is left behind


def test_unstaged_slots_and_stale_inputs_are_refused(gpu):
    model, x, _, _, _ = lenet()
    est = lenet_estimator("kfac")
    params = list(model.parameters())
    out = torch.empty(N_LENET, 3, 3, device=gpu)
    try:
        logits = model(x)
        with pytest.raises(RuntimeError, match="staged"):
            est.functional_covariance(out)                                     # nothing staged at all
        torch.autograd.grad(logits[:, 0].sum(), params, retain_graph=True)
        with pytest.raises(RuntimeError, match="inputs=True"):
            est.stage_output(1, 3, inputs=False)                               # no X side yet
        est.stage_output(0, 3, inputs=True)
        with pytest.raises(RuntimeError, match=r"slots \[1, 2\]"):
            est.functional_covariance(out)
        for slot in (1, 2):
            torch.autograd.grad(logits[:, slot].sum(), params, retain_graph=True)
            est.stage_output(slot, 3)
        est.functional_covariance(out)
        want = float64_covariance("kfac")[:, :3, :3]
        assert rel2(out, want) < TOL
        once = out.clone()
        est.functional_covariance(out, first=False)
        assert torch.equal(out, once + once)
        model(x)                                                               # a new forward pass: other input tensors
        with pytest.raises(RuntimeError, match="recorded inputs"):
            est.functional_covariance(out)
    finally:
        est.drop_predictive_state()
