"""GLM predictive over a grid of damping pairs on the GPU: the grid mode of csrc/persample.hip through
`ops.per_sample_quad_grid_reduce` against float64 and against the plain quadratic reduction, its bit-level promises,
`Curvature.functional_variance_grid` / `evaluate.glm_predictive_grid` on LeNet-5 against a float64 restatement and against
the existing path (`invert` then `glm_predictive`), and `evaluate.tune_glm`.

Expected values are computed here, in float64 on the CPU.  The bar is the project's (`TOL` of
tests/test_per_sample_gpu.py): relative 2-norm error below 1e-4 against float64, per grid row.  Every case prints its
figure; on an MI355X the worst of them was 2.3e-7 (KFAC on LeNet-5 against float64; the primitive: 1.9e-7)."""
import copy
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4


def rel2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


def worst_row(got, want):
    """The largest relative 2-norm error over the grid rows (dimension 0)."""
    return max(rel2(g, w) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ 1. the primitive
# (S, M, Nc, L): the shapes of tests/test_glm_predictive_gpu.py - the smallest at which each tile path can still go wrong
SHAPES = [
    (5, 130, 150, 37),       # 2 x 2 ragged full tiles, l tail
    (9, 6, 151, 100),        # half tile
    (33, 150, 16, 1),        # half tile, swapped; L = 1
    (100, 10, 85, 1),        # LeNet fc3
    (200, 16, 26, 5),        # several sample ranges per tile, if the plan splits
]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
SENTINEL = 7.0


def strided_operand(S, rows, L, gen, gpu):
    """(S, rows, L) random values whose rows are `rs` > L floats apart and whose samples are more than rows * rs apart, in a
    buffer that holds NaN everywhere else (strides are multiples of 4 floats)."""
    rs = (L + 3) // 4 * 4 + 4
    ns = rows * rs + 8
    buf = torch.full((64 + S * ns + 64,), float("nan"))
    vals = torch.randn(S, rows, L, generator=gen)
    view = buf[64:64 + S * ns].view(S, ns)[:, :rows * rs].view(S, rows, rs)
    view[:, :, :L] = vals
    return buf.to(gpu)[64:], vals.double(), ns, rs


def fenced_vector(n, gen, gpu):
    """n non-negative values (the first an exact zero) with NaN on both sides."""
    buf = torch.full((n + 8,), float("nan"))
    buf[4:4 + n] = 2.0 * torch.rand(n, generator=gen)
    buf[4] = 0.0
    return buf.to(gpu)[4:4 + n], buf[4:4 + n].double()


def grid_points(H):
    """`shift` spanning 1e-3 .. 10 and unequal gains, as the float32 values the kernel receives."""
    shift = torch.logspace(-3, 1, H) if H > 1 else torch.tensor([1e-3])
    gain = 1.0 / (1.0 + torch.arange(H, dtype=torch.float32)) ** 2
    return shift.float(), gain.float()


@functools.lru_cache(maxsize=None)
def primitive_case(index):
    """The operands of SHAPES[index] on the GPU - A, B, and u, v, V >= 0 in NaN-padded buffers (V with row stride Nc + 3) -
    and the float64 squares of the products; made once."""
    S, M, Nc, L = SHAPES[index]
    gpu = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(300 + index)
    A, A64, a_ns, a_rs = strided_operand(S, M, L, gen, gpu)
    B, B64, b_ns, b_rs = strided_operand(S, Nc, L, gen, gpu)
    u, u64 = fenced_vector(M, gen, gpu)
    v, v64 = fenced_vector(Nc, gen, gpu)
    wide = torch.full((M, Nc + 3), float("nan"))
    wide[:, :Nc] = 2.0 * torch.rand(M, Nc, generator=gen)
    wide[0, 0] = 0.0
    P = torch.einsum("sml,snl->smn", A64, B64)
    return dict(A=A, B=B, u=u, v=v, V=wide.to(gpu)[:, :Nc], u64=u64, v64=v64, V64=wide[:, :Nc].double(), P2=P * P,
                sizes=(S, M, Nc, L), strides=(a_ns, a_rs, b_ns, b_rs))


def want_of(case, dense, shift, gain):
    """(H, S) in float64, from the float32 grid points."""
    rows = []
    for sh, ga in zip(shift.double().tolist(), gain.double().tolist()):
        if dense:
            w = 1.0 / (case["V64"] + sh)
        else:
            w = 1.0 / ((case["u64"] + sh)[:, None] * (case["v64"] + sh)[None, :])
        rows.append(ga * (w * case["P2"]).sum((1, 2)))
    return torch.stack(rows)


def grid_job(case, dense, out, shift, gain, first=True):
    from curvature_amd import ops
    weights = (None, None, case["V"]) if dense else (case["u"], case["v"], None)
    return ops.PerSampleGridJob(case["A"], case["B"], *weights, out, shift.tolist(), gain.tolist(), *case["sizes"],
                                *case["strides"], first=first)


def strided_out(H, S, gpu):
    """An (H, S) view of strides (3 S + 5, 3) that holds NaN, with sentinels everywhere else."""
    buf = torch.full((H, 3 * S + 5), SENTINEL, device=gpu)
    view = buf[:, :3 * S:3]
    view.fill_(float("nan"))
    return buf, view


def sentinels_survive(buf, S):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:, :3 * S:3] = False
    return bool((buf[mask] == SENTINEL).all())


@pytest.mark.parametrize("H", [1, 3, 16])
@pytest.mark.parametrize("dense", [False, True], ids=["separable", "dense"])
@pytest.mark.parametrize("index", range(len(SHAPES)), ids=SHAPE_IDS)
def test_grid_reduce_against_float64(gpu, index, dense, H):
    from curvature_amd import ops
    case = primitive_case(index)
    S, M, Nc, L = case["sizes"]
    shift, gain = grid_points(H)
    want = want_of(case, dense, shift, gain)
    assert ops.per_sample_quad_grid_plan_flops([grid_job(case, dense, None, shift, gain)])[0] >= 2 * S * M * Nc * L
    buf, out = strided_out(H, S, gpu)
    ops.per_sample_quad_grid_reduce([grid_job(case, dense, out, shift, gain)])      # `first` overwrites the NaNs
    err = worst_row(out, want)
    print(f"grid reduce {SHAPES[index]} {'dense' if dense else 'separable'} H={H}: worst row rel 2-norm error {err:.3e}")
    assert err < TOL
    once = out.clone()
    ops.per_sample_quad_grid_reduce([grid_job(case, dense, out, shift, gain, first=False)])     # accumulates
    assert torch.equal(out, once + once)
    assert sentinels_survive(buf, S)


# ------------------------------------------------------------------------------------------------ 2. bits
@pytest.mark.parametrize("dense", [False, True], ids=["separable", "dense"])
@pytest.mark.parametrize("index", range(len(SHAPES)), ids=SHAPE_IDS)
def test_a_grid_row_does_not_depend_on_the_other_grid_points(gpu, index, dense):
    """Row h of an H = 16 call against the H = 1 call with that shift and gain (chunking above 16 pairs relies on it)."""
    from curvature_amd import ops
    case = primitive_case(index)
    S = case["sizes"][0]
    shift, gain = grid_points(16)
    whole = strided_out(16, S, gpu)[1]
    ops.per_sample_quad_grid_reduce([grid_job(case, dense, whole, shift, gain)])
    for h in range(16):
        one = strided_out(1, S, gpu)[1]
        ops.per_sample_quad_grid_reduce([grid_job(case, dense, one, shift[h:h + 1], gain[h:h + 1])])
        assert torch.equal(one[0], whole[h]), h


def test_an_item_has_the_same_bits_alone_and_in_a_batch_and_again(gpu):
    """Ten items (every shape in both forms, H alternating: more than one launch's worth) in one call against ten calls
    of one item; and the same call once more."""
    from curvature_amd import ops
    items = [(primitive_case(i), dense, grid_points((16, 3, 1)[(i + dense) % 3]))
             for dense in (False, True) for i in range(len(SHAPES))]
    alone = []
    for case, dense, (shift, gain) in items:
        out = strided_out(len(shift), case["sizes"][0], gpu)[1]
        ops.per_sample_quad_grid_reduce([grid_job(case, dense, out, shift, gain)])
        alone.append(out.clone())
    for _ in range(2):
        outs = [strided_out(len(shift), case["sizes"][0], gpu)[1] for case, _, (shift, _) in items]
        ops.per_sample_quad_grid_reduce([grid_job(case, dense, out, shift, gain)
                                         for (case, dense, (shift, gain)), out in zip(items, outs)])
        for k, (a, b) in enumerate(zip(alone, outs)):
            assert torch.equal(a, b), k


# ------------------------------------------------------------------------------------------------ 3. against K9
@pytest.mark.parametrize("index", range(len(SHAPES)), ids=SHAPE_IDS)
def test_dense_single_point_against_the_plain_quadratic_reduction(gpu, index):
    from curvature_amd import ops
    case = primitive_case(index)
    S = case["sizes"][0]
    worst = 0.0
    for shift, gain in ((1e-3, 1.0), (0.37, 2.5), (10.0, 0.01)):
        W = 1.0 / (case["V"] + shift)                                   # (M, Nc), contiguous
        plain = torch.empty(S, device=gpu)
        ops.per_sample_quad_reduce([ops.PerSampleQuadJob(case["A"], case["B"], W, plain, *case["sizes"], *case["strides"],
                                                         alpha=gain, first=True)])
        out = torch.empty(1, S, device=gpu)
        ops.per_sample_quad_grid_reduce([grid_job(case, True, out, torch.tensor([shift]), torch.tensor([gain]))])
        worst = max(worst, rel2(out[0], plain))
    print(f"dense H=1 against per_sample_quad_reduce {SHAPES[index]}: rel 2-norm difference {worst:.3e}")
    assert worst < TOL


# ------------------------------------------------------------------------------------------------ 4. LeNet-5
N_LENET = 8
HYPERS = [(a, s) for a in (0.1, 1.0, 10.0) for s in (1.0, 100.0)]          # five distinct rho, 1e-3 .. 10
KINDS = ["kfac", "diag", "efb"]


def matrix_layers(model):
    return [l for l in model if isinstance(l, (torch.nn.Conv2d, torch.nn.Linear))]


@functools.lru_cache(maxsize=None)
def lenet():
    """LeNet-5 on the GPU, a batch, and in float64 the per-sample Jacobians of every logit with respect to every layer's
    [W | b] as P = g X^T (grad_output of ``logits[:, c].sum()`` against the unfolded input with its ones row):
    ``jac[layer index]`` of shape (classes, N, m, n_in + 1), from ten backward passes on a CPU copy.  Made once."""
    from curvature_amd import models
    gpu = torch.device("cuda:0")
    torch.manual_seed(0)
    model = models.lenet5().to(gpu)
    x = torch.randn(N_LENET, 1, 28, 28, device=gpu)
    labels = torch.randint(0, 10, (N_LENET,), device=gpu)
    ref = copy.deepcopy(model).double().cpu().eval()
    layers = matrix_layers(ref)
    record = {l: [None, None] for l in layers}
    hooks = []

    def save_input(mod, inp):
        record[mod][0] = inp[0].detach()

    def save_grad_output(mod, inp, out):
        def save(grad):
            record[mod][1] = grad.detach()
        out.register_hook(save)
    for l in layers:
        hooks.append(l.register_forward_pre_hook(save_input))
        hooks.append(l.register_forward_hook(save_grad_output))
    logits = ref(x.double().cpu())
    jac = [[] for _ in layers]
    for c in range(10):
        torch.autograd.grad(logits[:, c].sum(), list(ref.parameters()), retain_graph=True)
        for k, l in enumerate(layers):
            xin, g = record[l]
            if isinstance(l, torch.nn.Conv2d):
                X = torch.nn.functional.unfold(xin, l.kernel_size, padding=l.padding, stride=l.stride)
                G = g.reshape(g.shape[0], g.shape[1], -1)
            else:
                X, G = xin.unsqueeze(2), g.unsqueeze(2)
            X = torch.cat([X, torch.ones_like(X[:, :1])], dim=1)
            jac[k].append(torch.einsum("nml,nkl->nmk", G, X))
    for hook in hooks:
        hook.remove()
    return model, x, labels, [torch.stack(j) for j in jac], logits.detach()


@functools.lru_cache(maxsize=None)
def lenet_estimator(kind):
    """`kind` after one update on the batch; KFAC decomposed.  No inversion: the grid does not need one."""
    from curvature_amd.curvatures import EFB, KFAC, Diagonal
    model, x, labels, _, _ = lenet()

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
            kfac.decompose()
            return kfac
        for hook in kfac.hooks:
            hook.remove()
        est = EFB(model, kfac.state, per_sample=True)
    backward()
    est.update(x.shape[0])
    return est


def resolve(value, k):
    return float(value[k]) if isinstance(value, (list, tuple)) else float(value)


def float64_grid(kind, est, model, jac, hypers):
    """The table of DESIGN K12 in float64, on the estimator's own state copied to the host: (H, N, classes)."""
    layers = matrix_layers(model)
    want = torch.zeros(len(hypers), N_LENET, 10, dtype=torch.float64)
    for k, layer in enumerate(layers):
        P = jac[k]                                                         # (classes, N, m, n)
        if kind == "kfac":
            A, G = (t.double().cpu() for t in est.state[layer])
            (lam_A, U_A), (lam_G, U_G) = torch.linalg.eigh(A), torch.linalg.eigh(G)
            lam_A, lam_G = lam_A.clamp_min(0), lam_G.clamp_min(0)
        elif kind == "efb":
            U_A, U_G = (t.double().cpu() for t in est.eigvecs[layer])
        if kind != "diag":
            P = U_G.t() @ P @ U_A
        Q2 = (P * P).permute(1, 0, 2, 3)                                   # (N, classes, m, n)
        for h, (add, multiply) in enumerate(hypers):
            n, s = resolve(add, k), resolve(multiply, k)
            rho = n / s
            if kind == "kfac":
                w = 1.0 / ((lam_G + math.sqrt(rho))[:, None] * (lam_A + math.sqrt(rho))[None, :])
            else:
                w = 1.0 / (est.state[layer].double().cpu() + rho)
            want[h] += (w * Q2).sum((2, 3)) / s
    return want


@pytest.mark.parametrize("kind", KINDS)
def test_lenet_grid_against_float64_and_against_invert(gpu, kind):
    """Every row of the grid against the float64 restatement, and against the existing path: `invert(a, s)` then
    `glm_predictive`.  Parameters, .grad and hooks are left as they were."""
    from curvature_amd.evaluate import glm_predictive, glm_predictive_grid
    model, x, labels, jac, logits64 = lenet()
    est = lenet_estimator(kind)
    model.zero_grad()
    torch.nn.functional.cross_entropy(model(x), labels).backward()            # some .grad to find again afterwards
    before = [(p.detach().clone(), p.grad, p.grad.clone()) for p in model.parameters()]
    hooked = hasattr(est, "hooks")

    logits, variance, probs = glm_predictive_grid(model, est, x, HYPERS)

    assert tuple(variance.shape) == tuple(probs.shape) == (len(HYPERS), N_LENET, 10)
    want = float64_grid(kind, est, model, jac, HYPERS)
    err = worst_row(variance, want)
    print(f"{kind}: LeNet-5 grid against float64: worst row rel 2-norm error {err:.3e}")
    assert err < TOL
    assert rel2(logits, logits64) < TOL
    probit = torch.softmax(logits.double().cpu() / torch.sqrt(1.0 + math.pi / 8.0 * want), dim=2)
    assert float((probs.double().cpu() - probit).abs().max()) < 1e-5
    for p, (value, grad, grad_value) in zip(model.parameters(), before):
        assert torch.equal(p.detach(), value) and p.grad is grad and torch.equal(p.grad, grad_value)
    assert hasattr(est, "hooks") == hooked                                     # borrowed hooks are gone again
    assert not getattr(est, "_predictive_kept", None)                          # ... and so is the kept X side
    assert not model.training

    worst = 0.0
    for h, (add, multiply) in enumerate(HYPERS):
        est.invert(add, multiply)
        _, plain, plain_probs = glm_predictive(model, est, x)
        worst = max(worst, rel2(variance[h], plain))
        assert float((probs[h] - plain_probs).abs().max()) < 1e-5
    print(f"{kind}: LeNet-5 grid against invert + glm_predictive: worst row rel 2-norm difference {worst:.3e}")
    assert worst < TOL


def test_kfac_per_layer_lists(gpu):
    from curvature_amd.evaluate import glm_predictive, glm_predictive_grid
    model, x, _, jac, _ = lenet()
    est = lenet_estimator("kfac")
    count = len(matrix_layers(model))
    adds = [0.1 * (k + 1) for k in range(count)]
    multiplies = [10.0 * (count - k) for k in range(count)]
    hypers = [(adds, multiplies), (1.0, 100.0), (multiplies, adds)]
    _, variance, _ = glm_predictive_grid(model, est, x, hypers)
    err = worst_row(variance, float64_grid("kfac", est, model, jac, hypers))
    worst = 0.0
    for h, (add, multiply) in enumerate(hypers):
        est.invert(add, multiply)
        worst = max(worst, rel2(variance[h], glm_predictive(model, est, x)[1]))
    print(f"kfac: per-layer lists: against float64 {err:.3e}, against invert + glm_predictive {worst:.3e}")
    assert err < TOL and worst < TOL


@pytest.mark.parametrize("kind", KINDS)
def test_twenty_pairs_run_as_two_chunks(gpu, kind):
    """20 pairs in one call (chunks of 16 and 4) against the same pairs in two calls, bit for bit."""
    from curvature_amd.evaluate import glm_predictive_grid
    model, x, _, _, _ = lenet()
    est = lenet_estimator(kind)
    hypers = [(10.0 ** (a / 3.0 - 2.0), 10.0 ** s) for a in range(10) for s in (0, 2)]
    assert len(hypers) == 20
    _, whole, _ = glm_predictive_grid(model, est, x, hypers, outputs=[3, 0])
    _, head, _ = glm_predictive_grid(model, est, x, hypers[:16], outputs=[3, 0])
    _, tail, _ = glm_predictive_grid(model, est, x, hypers[16:], outputs=[3, 0])
    assert torch.equal(whole, torch.cat([head, tail]))
    assert float(whole[:, :, [3, 0]].min()) > 0


def test_a_subset_of_the_outputs(gpu):
    from curvature_amd.evaluate import glm_predictive_grid
    model, x, _, _, _ = lenet()
    est = lenet_estimator("kfac")
    _, full, _ = glm_predictive_grid(model, est, x, HYPERS)
    _, part, _ = glm_predictive_grid(model, est, x, HYPERS, outputs=[7, 2])
    assert torch.equal(part[:, :, [7, 2]], full[:, :, [7, 2]])
    assert float(part[:, :, [0, 1, 3, 4, 5, 6, 8, 9]].abs().max()) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_input_side_reuse(gpu, kind):
    """``inputs=False`` reuses the X side of the call before, bit for bit, accumulates with ``first=False``, and raises once
    the recorded inputs are those of another forward pass."""
    model, x, _, _, _ = lenet()
    est = lenet_estimator(kind)
    borrowed = not hasattr(est, "record")
    if borrowed:
        est._record_per_sample("Diagonal")
    params = list(model.parameters())
    try:
        logits = model.eval()(x)
        fresh, reused = (torch.empty(len(HYPERS), N_LENET, device=gpu) for _ in range(2))
        torch.autograd.grad(logits[:, 4].sum(), params, retain_graph=True)
        est.functional_variance_grid(fresh, HYPERS, inputs=True)
        torch.autograd.grad(logits[:, 1].sum(), params, retain_graph=True)
        est.functional_variance_grid(reused, HYPERS, inputs=False)
        est.functional_variance_grid(fresh, HYPERS, inputs=True)
        assert torch.equal(fresh, reused)
        est.functional_variance_grid(reused, HYPERS, first=False, inputs=False)
        assert torch.equal(reused, fresh + fresh)
        logits = model(x)                                                      # a new forward pass: new records
        torch.autograd.grad(logits[:, 1].sum(), params)
        with pytest.raises(RuntimeError, match="inputs=True"):
            est.functional_variance_grid(reused, HYPERS, inputs=False)
        with pytest.raises(RuntimeError, match="shape"):
            est.functional_variance_grid(torch.empty(len(HYPERS) + 1, N_LENET, device=gpu), HYPERS)
    finally:
        est.drop_predictive_state()
        if borrowed:
            for hook in est.hooks:
                hook.remove()
            del est.hooks, est.record


def test_kfac_needs_a_decomposition_of_the_current_factors(gpu):
    from curvature_amd.curvatures import KFAC
    from curvature_amd.evaluate import glm_predictive_grid
    model, x, labels, _, _ = lenet()
    kfac = KFAC(model)
    try:
        def update():
            model.zero_grad()
            torch.nn.functional.cross_entropy(model(x), labels).backward()
            kfac.update(x.shape[0])
        update()
        with pytest.raises(RuntimeError, match="decompose"):
            glm_predictive_grid(model, kfac, x, HYPERS)
        kfac.decompose()
        U_G_t, U_A_t, lam_G, lam_A = kfac._decomposition[matrix_layers(model)[0]]
        assert float(lam_G.min()) >= 0 and float(lam_A.min()) >= 0
        A, G = kfac.state[matrix_layers(model)[0]]
        assert rel2(U_A_t.t() @ torch.diag(lam_A) @ U_A_t, A) < TOL and rel2(U_G_t.t() @ torch.diag(lam_G) @ U_G_t, G) < TOL
        glm_predictive_grid(model, kfac, x, HYPERS[:1], outputs=[0])
        update()
        with pytest.raises(RuntimeError, match="decompose"):
            glm_predictive_grid(model, kfac, x, HYPERS)
        kfac.decompose()
        kfac.restart_accumulation()
        with pytest.raises(RuntimeError, match="decompose"):
            glm_predictive_grid(model, kfac, x, HYPERS)
    finally:
        for hook in kfac.hooks:
            hook.remove()


# ------------------------------------------------------------------------------------------------ 5. tune_glm
@pytest.mark.parametrize("kind", ["kfac", "diag"])
def test_tune_glm(gpu, kind):
    from curvature_amd.evaluate import glm_predictive_grid, tune_glm
    model, x, labels, _, _ = lenet()
    est = lenet_estimator(kind)
    torch.manual_seed(11)
    x2, labels2 = torch.randn(N_LENET, 1, 28, 28, device=gpu), torch.randint(0, 10, (N_LENET,))
    dataset = [(x, labels), (x2.cpu(), labels2)]                               # device and host batches
    model.zero_grad()
    torch.nn.functional.cross_entropy(model(x), labels).backward()
    before = [(p.detach().clone(), p.grad, p.grad.clone()) for p in model.parameters()]
    hooked = hasattr(est, "hooks")
    inv_before = dict(est.inv_state)

    result = tune_glm(model, dataset, est, HYPERS)

    probs = torch.cat([glm_predictive_grid(model, est, b, HYPERS)[2] for b in (x, x2)], dim=1).double().cpu()
    y = torch.cat([labels.cpu(), labels2])
    nll = -torch.log(probs[:, torch.arange(2 * N_LENET), y]).mean(1)
    accuracy = (probs.argmax(2) == y).double().mean(1)
    assert tuple(result["nll"].shape) == tuple(result["accuracy"].shape) == (len(HYPERS),)
    assert float((result["nll"] - nll).abs().max()) < 1e-6 * float(nll.abs().max())
    assert torch.equal(result["accuracy"], accuracy)
    assert isinstance(result["best"], int) and result["best"] == int(torch.argmin(result["nll"]))
    assert float(result["nll"].max()) > float(result["nll"].min())              # the grid does move the predictive
    for p, (value, grad, grad_value) in zip(model.parameters(), before):
        assert torch.equal(p.detach(), value) and p.grad is grad and torch.equal(p.grad, grad_value)
    assert hasattr(est, "hooks") == hooked and hasattr(est, "record") == hooked  # borrowed hooks are gone afterwards
    assert est.inv_state.keys() == inv_before.keys() and all(est.inv_state[k] is inv_before[k] for k in inv_before)
