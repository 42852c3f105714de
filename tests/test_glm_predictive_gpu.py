"""Linearised Laplace (GLM) predictive on the GPU: the per-sample quadratic reduction of csrc/persample.hip through
`ops.per_sample_quad_reduce` against float64, `Curvature.functional_variance` against the estimator's own sampler and
against a float64 restatement on LeNet-5, the reuse of the input side, and the error paths.

Expected values are computed here, in float64 on the CPU.  The bar is the project's (`TOL` of
tests/test_per_sample_gpu.py): relative 2-norm error below 1e-4 against float64."""
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
# (S, M, Nc, L): the smallest sizes at which each path of the kernel can still go wrong
SHAPES = [
    (5, 130, 150, 37),       # 2 x 2 ragged full tiles, l tail
    (9, 6, 151, 100),        # half tile
    (33, 150, 16, 1),        # half tile, swapped; L = 1
    (100, 10, 85, 1),        # LeNet fc3
    (200, 16, 26, 5),        # several sample ranges per tile, if the plan splits
]
ALPHA = 1.5
SENTINEL = 7.0


def strided_operand(S, rows, L, gen, gpu):
    """(S, rows, L) random values whose rows are `rs` > L floats apart and whose samples are more than rows * rs apart, in a
    buffer that holds NaN everywhere else: the gaps, and what lies behind the last row.  (Strides are multiples of 4
    floats: every row starts on a 16-byte boundary, as the rows of the library's own packed operands do.)"""
    rs = (L + 3) // 4 * 4 + 4
    ns = rows * rs + 8
    buf = torch.full((64 + S * ns + 64,), float("nan"))
    vals = torch.randn(S, rows, L, generator=gen)
    view = buf[64:64 + S * ns].view(S, ns)[:, :rows * rs].view(S, rows, rs)
    view[:, :, :L] = vals
    return buf.to(gpu)[64:], vals.double(), ns, rs


@functools.lru_cache(maxsize=None)
def primitive_case(index, weighted):
    """The operands of SHAPES[index] on the GPU and the float64 value of the sum (alpha included); made once."""
    S, M, Nc, L = SHAPES[index]
    gpu = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(100 + index)
    A, A64, a_ns, a_rs = strided_operand(S, M, L, gen, gpu)
    B, B64, b_ns, b_rs = strided_operand(S, Nc, L, gen, gpu)
    W = W64 = None
    if weighted:
        wide = torch.full((M, Nc + 3), float("nan"))
        wide[:, :Nc] = torch.rand(M, Nc, generator=gen) + 0.1
        W64 = wide[:, :Nc].double()
        W = wide.to(gpu)[:, :Nc]                                   # row stride Nc + 3, NaN in the gap
    P = torch.einsum("sml,snl->smn", A64, B64)
    want = ALPHA * ((P * P) if W64 is None else (W64 * P * P)).sum((1, 2))
    return dict(A=A, B=B, W=W, sizes=(S, M, Nc, L), strides=(a_ns, a_rs, b_ns, b_rs), want=want)


def quad_job(case, out, first):
    from curvature_amd import ops
    return ops.PerSampleQuadJob(case["A"], case["B"], case["W"], out, *case["sizes"], *case["strides"], alpha=ALPHA,
                                first=first)


def strided_out(S, gpu):
    """A length-S view of stride 3 that holds NaN, with sentinels between its entries."""
    buf = torch.full((3 * S,), SENTINEL, device=gpu)
    buf[::3] = float("nan")
    return buf, buf[::3]


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "W"])
@pytest.mark.parametrize("index", range(len(SHAPES)), ids=["x".join(map(str, s)) for s in SHAPES])
def test_quad_reduce_against_float64(gpu, index, weighted):
    from curvature_amd import ops
    case = primitive_case(index, weighted)
    S, M, Nc, L = case["sizes"]
    assert ops.per_sample_quad_plan_flops([quad_job(case, None, True)])[0] >= 2 * S * M * Nc * L
    buf, out = strided_out(S, gpu)
    ops.per_sample_quad_reduce([quad_job(case, out, True)])           # `first` overwrites the NaNs
    err = rel2(out, case["want"])
    print(f"quad reduce {SHAPES[index]} weighted={weighted}: rel 2-norm error {err:.3e}")
    assert err < TOL
    once = out.clone()
    ops.per_sample_quad_reduce([quad_job(case, out, False)])          # accumulates: twice the value
    assert rel2(out, 2 * case["want"]) < TOL
    assert torch.equal(out, once + once)
    assert bool((buf[1::3] == SENTINEL).all()) and bool((buf[2::3] == SENTINEL).all())


def test_an_item_has_the_same_bits_alone_and_in_a_batch(gpu):
    """All five shapes (weighted and not, alternating) in one call against five calls of one item."""
    from curvature_amd import ops
    cases = [primitive_case(i, i % 2 == 0) for i in range(len(SHAPES))] + \
            [primitive_case(i, i % 2 == 1) for i in range(len(SHAPES))]
    alone = []
    for case in cases:
        out = strided_out(case["sizes"][0], gpu)[1]
        ops.per_sample_quad_reduce([quad_job(case, out, True)])
        alone.append(out.clone())
    outs = [strided_out(case["sizes"][0], gpu)[1] for case in cases]
    ops.per_sample_quad_reduce([quad_job(case, out, True) for case, out in zip(cases, outs)])
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
def test_variance_is_that_of_the_estimators_own_sampler(gpu, kind):
    """The outputs of Conv2d -> Flatten -> Linear are linear in the convolution's [W | b], so the variance of output c
    under the sampler is sum_k (df_c of the sample drawn from unit noise e_k)**2, over all 57 entries of the noise."""
    from curvature_amd.evaluate import glm_predictive
    model = linear_model(gpu)
    torch.manual_seed(4)
    x, labels = torch.randn(3, 2, 5, 5, device=gpu), torch.tensor([0, 3, 1], device=gpu)
    est = make_estimator(kind, model, x, labels, layer_types="Conv2d")
    conv, lin = model[0], model[2]
    _, variance, _ = glm_predictive(model, est, x)

    m, n = 3, 19
    x64, head = x.double().cpu(), lin.weight.detach().double().cpu()
    want = torch.zeros(3, 4, dtype=torch.float64)
    for k in range(m * n):
        z = torch.zeros(m * n, device=gpu)
        z[k] = 1.0
        z = z.view(m, n) if kind == "diag" else z.view(n, m)              # the noise shape of each sampler
        d = est.sample(conv, z).double().cpu()                             # (m, n) as [W | b]
        df = torch.nn.functional.conv2d(x64, d[:, :-1].reshape(3, 2, 3, 3), d[:, -1], padding=1).flatten(1) @ head.t()
        want += df * df
    err = rel2(variance, want)
    print(f"{kind}: variance against the sampler: rel 2-norm error {err:.3e}")
    assert err < TOL


# ------------------------------------------------------------------------------------------------ 3. LeNet-5
N_LENET = 8


@functools.lru_cache(maxsize=None)
def lenet():
    """LeNet-5 on the GPU, a batch, and the float64 per-sample Jacobians of every logit with respect to every layer's
    [W | b]: ``jac[layer index][n][c]`` (m, n_in + 1), from N * classes backward passes on a CPU copy.  Made once."""
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
    return model, x, labels, jac, logits.detach()


@functools.lru_cache(maxsize=None)
def lenet_estimator(kind):
    model, x, labels, _, _ = lenet()
    return make_estimator(kind, model, x, labels, per_sample=kind == "efb")


def float64_variance(kind, est, model, jac):
    """The table of the issue, applied to the estimator's own inverse state / eigenvectors copied to the host."""
    layers = [l for l in model if isinstance(l, (torch.nn.Conv2d, torch.nn.Linear))]
    want = torch.zeros(N_LENET, 10, dtype=torch.float64)
    for k, layer in enumerate(layers):
        if kind == "kfac":
            L_A, L_G = (t.double().cpu() for t in est.inv_state[layer])
        elif kind == "efb":
            U_A, U_G = (t.double().cpu() for t in est.eigvecs[layer])
        if kind != "kfac":
            inv = est.inv_state[layer].double().cpu()
        for n in range(N_LENET):
            for c in range(10):
                P = jac[k][n][c]
                if kind == "kfac":
                    want[n, c] += (L_G.t() @ P @ L_A).pow(2).sum()
                elif kind == "diag":
                    want[n, c] += (inv.pow(2) * P.pow(2)).sum()
                else:
                    want[n, c] += (inv.pow(2) * (U_G.t() @ P @ U_A).pow(2)).sum()
    return want


@pytest.mark.parametrize("kind", ["kfac", "diag", "efb"])
def test_lenet_against_float64(gpu, kind):
    from curvature_amd.evaluate import glm_predictive
    model, x, labels, jac, logits64 = lenet()
    est = lenet_estimator(kind)
    model.zero_grad()
    torch.nn.functional.cross_entropy(model(x), labels).backward()            # some .grad to find again afterwards
    before = [(p.detach().clone(), p.grad, p.grad.clone()) for p in model.parameters()]
    hooked = hasattr(est, "hooks")

    logits, variance, probs = glm_predictive(model, est, x)

    want = float64_variance(kind, est, model, jac)
    err = rel2(variance, want)
    print(f"{kind}: LeNet-5 variance: rel 2-norm error {err:.3e}")
    assert err < TOL
    assert rel2(logits, logits64) < TOL
    probit = torch.softmax(logits.double().cpu() / torch.sqrt(1.0 + math.pi / 8.0 * want), dim=1)
    assert float((probs.double().cpu() - probit).abs().max()) < 1e-5
    assert float((probs.sum(1) - 1.0).abs().max()) < 1e-5
    for p, (value, grad, grad_value) in zip(model.parameters(), before):
        assert torch.equal(p.detach(), value) and p.grad is grad and torch.equal(p.grad, grad_value)
    assert hasattr(est, "hooks") == hooked                                     # borrowed hooks are gone again
    assert not model.training


def test_a_subset_of_the_outputs(gpu):
    from curvature_amd.evaluate import glm_predictive
    model, x, _, _, _ = lenet()
    est = lenet_estimator("kfac")
    _, full, _ = glm_predictive(model, est, x)
    _, part, _ = glm_predictive(model, est, x, outputs=[7, 2])
    assert torch.equal(part[:, [7, 2]], full[:, [7, 2]])
    assert float(part[:, [0, 1, 3, 4, 5, 6, 8, 9]].abs().max()) == 0


# ------------------------------------------------------------------------------------------------ 4. inputs=False
@pytest.mark.parametrize("kind", ["kfac", "diag", "efb"])
def test_input_side_reuse_is_bit_identical(gpu, kind):
    """The X side worked out once per forward pass (what `glm_predictive` does) against once per output; and `first`."""
    from curvature_amd.evaluate import glm_predictive
    model, x, _, _, _ = lenet()
    est = lenet_estimator(kind)
    _, once, _ = glm_predictive(model, est, x)
    borrowed = not hasattr(est, "record")
    if borrowed:
        est._record_per_sample("Diagonal")
    try:
        logits = model(x)
        every = torch.zeros_like(once)
        twice = once.clone()
        for c in range(10):
            torch.autograd.grad(logits[:, c].sum(), list(model.parameters()), retain_graph=True)
            est.functional_variance(every[:, c], inputs=True)
            est.functional_variance(twice[:, c], first=False, inputs=False)
    finally:
        if borrowed:
            for hook in est.hooks:
                hook.remove()
            del est.hooks, est.record
    assert torch.equal(every, once)
    assert torch.equal(twice, once + once)


# ------------------------------------------------------------------------------------------------ 5. error paths
def test_half_precision_records_are_refused(gpu):
    from curvature_amd.evaluate import glm_predictive
    model = linear_model(gpu)
    x, labels = torch.randn(3, 2, 5, 5, device=gpu), torch.tensor([0, 3, 1], device=gpu)
    est = make_estimator("kfac", model, x, labels, layer_types="Conv2d")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(RuntimeError, match="bfloat16"):
            glm_predictive(model, est, x)


def test_a_grouped_convolution_is_named(gpu):
    from curvature_amd.curvatures import Diagonal
    from curvature_amd.evaluate import glm_predictive
    torch.manual_seed(5)
    model = torch.nn.Sequential(OrderedDict([("plain", torch.nn.Conv2d(2, 4, 3, padding=1)),
                                             ("grouped_one", torch.nn.Conv2d(4, 4, 3, padding=1, groups=2)),
                                             ("flat", torch.nn.Flatten()), ("head", torch.nn.Linear(100, 4))])).to(gpu)
    x, labels = torch.randn(3, 2, 5, 5, device=gpu), torch.tensor([0, 3, 1], device=gpu)
    kfac = make_estimator("kfac", model, x, labels)
    with pytest.raises(NotImplementedError, match="grouped_one"):
        glm_predictive(model, kfac, x)
    for hook in kfac.hooks:
        hook.remove()
    diag = make_estimator("diag", model, x, labels)
    with pytest.raises(NotImplementedError, match="grouped_one"):
        glm_predictive(model, diag, x)
    assert not hasattr(diag, "hooks") and not model.plain._forward_pre_hooks      # nothing is left behind
