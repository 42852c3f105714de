"""Per-sample Fisher and GLM predictive for autocast (bf16 / fp16) records, ConvTranspose2d and the two projections of a
MultiheadAttention module, end to end on the GPU.  The bar is the project's: relative Frobenius / 2-norm error below 1e-4
against float64; every figure is printed before it is asserted.

Half records: the float64 value is formed from the recorded tensors themselves, upcast - the records are what the
estimators are defined on.  ConvTranspose2d and attention: from autograd per-sample Jacobians of a float64 CPU copy."""
import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(autouse=True)
def wide():
    """The wider per-sample line is opt-in; everything here is about it."""
    from curvature_amd import ops
    was = ops.widen_per_sample(True)
    yield
    ops.widen_per_sample(was)


def rel2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


def report(what, err):
    print(f"{what}: rel error {err:.3e}")
    assert err < TOL, what


# ------------------------------------------------------------------------------------------------ float64 from records
def operand_matrices(layer, x, g, samples=None):
    """float64 (g_n, X_n) of every sample from a layer's records: (N, m, L) and (N, n_in [+ 1], L)."""
    from test_per_sample_pack_ex_gpu import transposed_columns
    x, g = x.detach().double().cpu(), g.detach().double().cpu()
    kind = layer.__class__.__name__
    if kind == "Conv2d":
        X = F.unfold(x, layer.kernel_size, padding=layer.padding, stride=layer.stride)
        G = g.flatten(2)
    elif kind == "ConvTranspose2d":
        X = transposed_columns(x, layer.kernel_size, layer.stride, layer.padding, tuple(g.shape[2:]))
        G = g.flatten(2)
    elif kind == "AttentionProjection":                    # (T, N, E) or (T N, E) rows t N + n
        x, g = (t if t.dim() == 3 else t.view(-1, samples, t.shape[-1]) for t in (x, g))
        X, G = x.permute(1, 2, 0), g.permute(1, 2, 0)
    else:
        N = x.shape[0]
        X, G = x.reshape(N, -1, x.shape[-1]).transpose(1, 2), g.reshape(N, -1, g.shape[-1]).transpose(1, 2)
    if layer.bias is not None:
        X = torch.cat([X, torch.ones(X.shape[0], 1, X.shape[2], dtype=torch.float64)], dim=1)
    return G, X


def record_jacobians(est, layers, samples=None):
    """[P_n] (N, m, n) per layer in float64 from the estimator's current records."""
    out = []
    for layer in layers:
        G, X = operand_matrices(layer, *est.record[layer], samples=samples)
        out.append(torch.einsum("nml,nkl->nmk", G, X))
    return out


def transformed(kind, est, layer, P):
    """T(P) whose squared norm is the layer's share of the variance, from the estimator's own inverse state."""
    if kind == "kfac":
        L_A, L_G = (t.double().cpu() for t in est.inv_state[layer])
        return L_G.t() @ P @ L_A
    inv = est.inv_state[layer].double().cpu()
    if kind == "diag":
        return inv * P
    U_A, U_G = (t.double().cpu() for t in est.eigvecs[layer])
    return inv * (U_G.t() @ P @ U_A)


def make_estimator(kind, model, loss_pass, N, layer_types=None):
    """`kind` after one update on the pass `loss_pass()` (forward and backward) and an inversion."""
    from curvature_amd.curvatures import EFB, KFAC, Diagonal
    if kind == "diag":
        est = Diagonal(model, layer_types)
    else:
        kfac = KFAC(model, layer_types)
        loss_pass()
        kfac.update(N)
        if kind == "kfac":
            est = kfac
        else:
            for hook in kfac.hooks:
                hook.remove()
            est = EFB(model, kfac.state, layer_types)
    if kind != "kfac":
        loss_pass()
        est.update(N)
    est.invert(add=0.5, multiply=2.0)
    return est


def spy_on_records(est, method):
    """`est.<method>` wrapped so that every call first files the records it is about to read: [{layer: (x, g)}]."""
    seen, original = [], getattr(est, method)

    def wrapper(*args, **kwargs):
        seen.append({l: (r[0].detach().clone(), r[1].detach().clone()) for l, r in est.record.items()})
        return original(*args, **kwargs)
    setattr(est, method, wrapper)
    return seen


# ------------------------------------------------------------------------------------------------ 1. half records
HALF = {"bf16": torch.bfloat16, "fp16": torch.float16}
N_HALF = 5


def half_model(gpu):
    torch.manual_seed(11)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(8, 8, 1),
                               torch.nn.AdaptiveAvgPool2d(2), torch.nn.Flatten(), torch.nn.Linear(32, 4)).to(gpu)


def half_batch(gpu):
    torch.manual_seed(12)
    return torch.randn(N_HALF, 3, 8, 8, device=gpu), torch.tensor([0, 3, 1, 2, 3], device=gpu)


def matrix_layers(model):
    return [l for l in model.modules() if l.__class__.__name__ in ("Linear", "Conv2d", "ConvTranspose2d")]


@pytest.mark.parametrize("half", sorted(HALF))
def test_half_records_exact_fisher(gpu, half):
    """Diagonal / EFB (per_sample=True) under autocast against N sum_n (g_n X_n^T)**2 of the recorded tensors, upcast."""
    from curvature_amd.curvatures import EFB, Diagonal
    model = half_model(gpu)
    x, labels = half_batch(gpu)
    layers = matrix_layers(model)
    gen = torch.Generator().manual_seed(5)
    eig = {}
    for l in layers:
        m, n = l.weight.shape[0], l.weight[0].numel() + 1
        eig[l] = (torch.linalg.qr(torch.randn(n, n, generator=gen))[0].to(gpu),
                  torch.linalg.qr(torch.randn(m, m, generator=gen))[0].to(gpu))
    diag, efb = Diagonal(model, per_sample=True), EFB(model, {}, eigvecs=eig, per_sample=True)
    with torch.autocast("cuda", dtype=HALF[half]):
        loss = F.cross_entropy(model(x).float(), labels)
    loss.backward()
    dtypes = {tuple(t.dtype for t in diag.record[l]) for l in layers}
    assert (torch.float32, HALF[half]) in dtypes and (HALF[half], HALF[half]) in dtypes      # the stem's input is fp32
    diag.update(N_HALF)
    efb.update(N_HALF)
    for k, (layer, P) in enumerate(zip(layers, record_jacobians(diag, layers))):
        report(f"{half} Diagonal layer {k}", rel2(diag.state[layer], N_HALF * P.pow(2).sum(0)))
        report(f"{half} EFB diags layer {k}", rel2(efb.diags[layer], N_HALF * P.pow(2).sum(0)))
        U_A, U_G = (t.double().cpu() for t in eig[layer])
        report(f"{half} EFB layer {k}", rel2(efb.state[layer], N_HALF * (U_G.t() @ P @ U_A).pow(2).sum(0)))
    for est in (diag, efb):
        for hook in est.hooks:
            hook.remove()


@pytest.mark.parametrize("kind", ["kfac", "diag", "efb"])
@pytest.mark.parametrize("half", sorted(HALF))
def test_half_records_glm_predictive(gpu, half, kind):
    from curvature_amd.evaluate import glm_predictive
    model = half_model(gpu)
    x, labels = half_batch(gpu)
    layers = matrix_layers(model)

    def loss_pass():
        model.zero_grad()
        with torch.autocast("cuda", dtype=HALF[half]):
            loss = F.cross_entropy(model(x).float(), labels)
        loss.backward()
    est = make_estimator(kind, model, loss_pass, N_HALF)       # KFAC.update takes the half records (K1b)
    seen = spy_on_records(est, "functional_variance")
    with torch.autocast("cuda", dtype=HALF[half]):
        logits, variance, probs = glm_predictive(model, est, x)
    assert variance.dtype == probs.dtype == torch.float32 and logits.dtype == HALF[half]
    assert len(seen) == 4 and seen[0][layers[1]][0].dtype == HALF[half]
    want = torch.zeros(N_HALF, 4, dtype=torch.float64)
    for c, records in enumerate(seen):
        for layer in layers:
            G, X = operand_matrices(layer, *records[layer])
            P = torch.einsum("nml,nkl->nmk", G, X)
            want[:, c] += torch.stack([transformed(kind, est, layer, P[n]).pow(2).sum() for n in range(N_HALF)])
    report(f"{half} {kind} glm_predictive variance", rel2(variance, want))
    probit = torch.softmax(logits.double().cpu() / torch.sqrt(1.0 + math.pi / 8.0 * want), dim=1)
    assert float((probs.double().cpu() - probit).abs().max()) < 1e-5
    if hasattr(est, "hooks"):
        for hook in est.hooks:
            hook.remove()


def test_half_logits_every_driver_returns_float32(gpu):
    """All four drivers under bf16 autocast: half logits in, float32 variance / covariance / probs out, and the joint,
    Monte-Carlo and grid drivers agree with `glm_predictive` on the same records."""
    from curvature_amd.evaluate import glm_predictive, glm_predictive_grid, glm_predictive_joint, glm_predictive_mc
    model = half_model(gpu)
    x, labels = half_batch(gpu)

    def loss_pass():
        model.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = F.cross_entropy(model(x).float(), labels)
        loss.backward()
    est = make_estimator("kfac", model, loss_pass, N_HALF)
    noise = torch.randn(N_HALF, 64, 4, device=gpu, generator=torch.Generator(gpu).manual_seed(1))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits, variance, probs = glm_predictive(model, est, x)
        _, covariance, probs_j = glm_predictive_joint(model, est, x)
        _, cov_mc, probs_mc = glm_predictive_mc(model, est, x, samples=64, noise=noise)
        est.decompose()
        _, grid, probs_g = glm_predictive_grid(model, est, x, [(0.5, 2.0)])
    assert logits.dtype == torch.bfloat16
    for t in (variance, probs, covariance, probs_j, cov_mc, probs_mc, grid, probs_g):
        assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
    report("bf16 joint diagonal against glm_predictive", rel2(torch.diagonal(covariance, dim1=1, dim2=2), variance))
    report("bf16 grid at the inverted pair against glm_predictive", rel2(grid[0], variance))
    assert torch.equal(cov_mc, covariance) and torch.equal(probs_j, probs)
    assert float((probs_mc.sum(1) - 1).abs().max()) < 1e-5
    for hook in est.hooks:
        hook.remove()


# ------------------------------------------------------------------------------------------------ 2. ConvTranspose2d
N_CONVT, K_CONVT = 4, 5
CONVT_TYPES = ["Linear", "ConvTranspose2d"]


class Decoder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(6, 4 * 3 * 3)
        self.up1 = torch.nn.ConvTranspose2d(4, 3, 4, 2, 1)
        self.up2 = torch.nn.ConvTranspose2d(3, 2, 3, 1, 1)
        self.head = torch.nn.Linear(2 * 6 * 6, K_CONVT)

    def forward(self, z):
        h = torch.relu(self.up1(self.fc(z).view(-1, 4, 3, 3)))
        return self.head(self.up2(h).flatten(1))


def wm_jacobian(layer, grad_w, grad_b):
    """[W | b] gradient in Wm order, float64."""
    if layer.__class__.__name__ == "ConvTranspose2d":
        grad_w = grad_w.permute(1, 0, 2, 3)
    return torch.cat([grad_w.reshape(grad_w.shape[0], -1), grad_b.reshape(-1, 1)], dim=1)


@functools.lru_cache(maxsize=None)
def decoder():
    """The decoder on the GPU, a batch, and jac[layer index][n][c]: the float64 Jacobian of logit c of sample n with
    respect to the layer's [W | b], by autograd on a CPU copy.  Made once."""
    gpu = torch.device("cuda:0")
    torch.manual_seed(21)
    model = Decoder().to(gpu)
    z = torch.randn(N_CONVT, 6, device=gpu)
    labels = torch.tensor([0, 4, 2, 1], device=gpu)
    ref = copy.deepcopy(model).double().cpu().eval()
    layers = matrix_layers(ref)
    logits = ref(z.double().cpu())
    jac = [[[None] * K_CONVT for _ in range(N_CONVT)] for _ in layers]
    for n in range(N_CONVT):
        for c in range(K_CONVT):
            grads = torch.autograd.grad(logits[n, c], [p for l in layers for p in (l.weight, l.bias)], retain_graph=True)
            for k, layer in enumerate(layers):
                jac[k][n][c] = wm_jacobian(layer, grads[2 * k], grads[2 * k + 1])
    return model, z, labels, jac


def decoder_pass(model, z, labels):
    def loss_pass():
        model.zero_grad()
        F.cross_entropy(model(z), labels).backward()
    return loss_pass


@functools.lru_cache(maxsize=None)
def decoder_estimator(kind):
    model, z, labels, _ = decoder()
    return make_estimator(kind, model, decoder_pass(model, z, labels), N_CONVT, CONVT_TYPES)


def test_conv_transpose_exact_fisher(gpu):
    """K8's identity: at N = 1 the per-sample state is the default path's; at N = 4 it is the sum of the four
    single-sample default updates - each of those holds 1 * P_n**2, the per-sample update N * sum_n P_n**2 - so
    state = N * sum of the four."""
    from curvature_amd.curvatures import Diagonal
    model, z, labels, _ = decoder()
    layers = matrix_layers(model)
    singles = []
    for n in range(N_CONVT):
        # P_n of the batch pass: the loss of sample n alone, scaled as its share of the batch mean
        default, exact = Diagonal(model, CONVT_TYPES), Diagonal(model, CONVT_TYPES, per_sample=True)
        model.zero_grad()
        F.cross_entropy(model(z[n:n + 1]), labels[n:n + 1]).backward()
        default.update(1)
        exact.update(1)
        for k, layer in enumerate(layers):
            report(f"ConvTranspose2d model, N = 1, sample {n}, layer {k}", rel2(exact.state[layer], default.state[layer]))
        singles.append({l: default.state[l].double().cpu() for l in layers})
        for hook in exact.hooks:
            hook.remove()
    exact = Diagonal(model, CONVT_TYPES, per_sample=True)
    decoder_pass(model, z, labels)()
    exact.update(N_CONVT)
    for hook in exact.hooks:
        hook.remove()
    for k, layer in enumerate(layers):
        # the batch loss is the mean: g_n of the batch pass is 1 / N of the single pass, P_n**2 is 1 / N**2 of it
        want = N_CONVT * sum(s[layer] for s in singles) / N_CONVT ** 2
        report(f"ConvTranspose2d model, N = {N_CONVT}, layer {k}", rel2(exact.state[layer], want))


def float64_covariance(kind, est, layers_gpu, jac, classes):
    N = len(jac[0])
    cov = torch.zeros(N, len(classes), len(classes), dtype=torch.float64)
    for k, layer in enumerate(layers_gpu):
        for n in range(N):
            T = torch.stack([transformed(kind, est, layer, jac[k][n][c]).flatten() for c in classes])
            cov[n] += T @ T.t()
    return cov


@pytest.mark.parametrize("kind", ["kfac", "diag", "efb"])
def test_conv_transpose_predictives(gpu, kind):
    from test_glm_mc_gpu import full_reference
    from curvature_amd.evaluate import glm_predictive, glm_predictive_joint, glm_predictive_mc
    model, z, _, jac = decoder()
    est = decoder_estimator(kind)
    layers = matrix_layers(model)
    classes = list(range(K_CONVT))
    want = float64_covariance(kind, est, layers, jac, classes)
    logits, variance, probs = glm_predictive(model, est, z)
    report(f"ConvTranspose2d {kind} glm_predictive", rel2(variance, torch.diagonal(want, dim1=1, dim2=2)))
    assert variance.dtype == probs.dtype == torch.float32
    _, covariance, _ = glm_predictive_joint(model, est, z)
    report(f"ConvTranspose2d {kind} glm_predictive_joint", rel2(covariance, want))
    assert torch.equal(covariance, covariance.transpose(1, 2))
    noise = torch.randn(N_CONVT, 200, K_CONVT, device=gpu, generator=torch.Generator(gpu).manual_seed(3))
    logits_mc, cov_mc, probs_mc = glm_predictive_mc(model, est, z, samples=200, noise=noise)
    assert torch.equal(cov_mc, covariance) and torch.equal(logits_mc, logits)
    report(f"ConvTranspose2d {kind} glm_predictive_mc", rel2(probs_mc, full_reference(logits_mc, cov_mc, classes, noise)))


def test_conv_transpose_variance_is_that_of_the_sampler(gpu):
    """As the existing GLM tests do: Linear -> ConvTranspose2d -> flatten -> Linear is linear in the transposed
    convolution's [W | b], so the variance of output c is sum_k (df_c of the sample drawn from unit noise e_k)**2 - the
    sampler's own linear map, which writes the weight through `_slots`."""
    from curvature_amd.curvatures import KFAC
    from curvature_amd.evaluate import glm_predictive
    torch.manual_seed(31)
    up = torch.nn.ConvTranspose2d(2, 3, 4, 2, 1)
    model = torch.nn.Sequential(up, torch.nn.Flatten(), torch.nn.Linear(3 * 6 * 6, 4)).to(gpu)
    x, labels = torch.randn(3, 2, 3, 3, device=gpu), torch.tensor([0, 3, 1], device=gpu)
    est = KFAC(model, "ConvTranspose2d")
    F.cross_entropy(model(x), labels).backward()
    est.update(3)
    est.invert(add=0.5, multiply=2.0)
    _, variance, _ = glm_predictive(model, est, x)
    m, n = 3, 2 * 16 + 1
    x64, head = x.double().cpu(), model[2].weight.detach().double().cpu()
    want = torch.zeros(3, 4, dtype=torch.float64)
    for k in range(m * n):
        noise = torch.zeros(m * n, device=gpu)
        noise[k] = 1.0
        d = est.sample(up, noise.view(n, m)).double().cpu()                   # (m, n) as [Wm | b]
        w = d[:, :-1].reshape(3, 2, 4, 4).permute(1, 0, 2, 3)                 # Wm -> (in, out, kh, kw)
        df = F.conv_transpose2d(x64, w, d[:, -1], stride=2, padding=1).flatten(1) @ head.t()
        want += df * df
    report("ConvTranspose2d kfac variance against its sampler", rel2(variance, want))
    for hook in est.hooks:
        hook.remove()


def test_conv_transpose_grid(gpu):
    from curvature_amd.evaluate import glm_predictive_grid
    model, z, _, jac = decoder()
    est = decoder_estimator("kfac")
    est.decompose()
    hypers = [(0.5, 2.0), (1e-2, 1.0), (3.0, 0.25)]
    _, variance, probs = glm_predictive_grid(model, est, z, hypers)
    assert tuple(variance.shape) == (3, N_CONVT, K_CONVT) and probs.dtype == torch.float32
    layers = matrix_layers(model)
    want = torch.zeros(3, N_CONVT, K_CONVT, dtype=torch.float64)
    for k, layer in enumerate(layers):
        A, G = (t.double().cpu() for t in est.state[layer])
        lam_A, U_A = torch.linalg.eigh(A)
        lam_G, U_G = torch.linalg.eigh(G)
        for n in range(N_CONVT):
            for c in range(K_CONVT):
                Q2 = (U_G.t() @ jac[k][n][c] @ U_A).pow(2)
                for h, (add, multiply) in enumerate(hypers):
                    r = math.sqrt(add / multiply)
                    want[h, n, c] += (Q2 / ((lam_G[:, None] + r) * (lam_A[None, :] + r))).sum() / multiply
    for h in range(3):
        report(f"ConvTranspose2d kfac grid pair {h}", rel2(variance[h], want[h]))


# ------------------------------------------------------------------------------------------------ 3. attention
T_ATTN, N_ATTN, E_ATTN = 5, 3, 8


class Attn(torch.nn.Module):
    def __init__(self, batch_first):
        super().__init__()
        self.batch_first = batch_first
        self.attn = torch.nn.MultiheadAttention(E_ATTN, 2, batch_first=batch_first)
        self.head = torch.nn.Linear(E_ATTN, 4)

    def forward(self, x):                                  # x: (N, T, E), the sample first
        tokens = x if self.batch_first else x.transpose(0, 1)
        out, _ = self.attn(tokens, tokens, tokens)
        return self.head(out.mean(dim=1 if self.batch_first else 0))


@functools.lru_cache(maxsize=None)
def attention(batch_first):
    from curvature_amd.curvatures import AttentionProjection
    gpu = torch.device("cuda:0")
    torch.manual_seed(41)
    model = Attn(batch_first).to(gpu)
    x = torch.randn(N_ATTN, T_ATTN, E_ATTN, device=gpu)
    labels = torch.tensor([1, 3, 0], device=gpu)
    ref = copy.deepcopy(model).double().cpu().eval()
    params = [(ref.attn.in_proj_weight, ref.attn.in_proj_bias), (ref.attn.out_proj.weight, ref.attn.out_proj.bias),
              (ref.head.weight, ref.head.bias)]
    logits = ref(x.double().cpu())
    jac = [[[None] * 4 for _ in range(N_ATTN)] for _ in params]
    for n in range(N_ATTN):
        for c in range(4):
            grads = torch.autograd.grad(logits[n, c], [p for pair in params for p in pair], retain_graph=True)
            for k in range(len(params)):
                jac[k][n][c] = torch.cat([grads[2 * k], grads[2 * k + 1].reshape(-1, 1)], dim=1)
    layers = list(AttentionProjection.of(model.attn)) + [model.head]
    return model, x, labels, jac, layers


@pytest.mark.parametrize("kind", ["kfac", "efb"])
@pytest.mark.parametrize("batch_first", [False, True], ids=["tokens_first", "batch_first"])
def test_attention_glm_predictive(gpu, batch_first, kind):
    from curvature_amd.evaluate import glm_predictive
    model, x, labels, jac, layers = attention(batch_first)

    def loss_pass():
        model.zero_grad()
        F.cross_entropy(model(x), labels).backward()
    est = make_estimator(kind, model, loss_pass, N_ATTN)
    assert set(est.inv_state) == set(layers)
    _, variance, _ = glm_predictive(model, est, x)
    want = float64_covariance(kind, est, layers, jac, range(4))
    report(f"attention {kind} batch_first={batch_first} glm_predictive", rel2(variance, torch.diagonal(want, dim1=1, dim2=2)))
    # a permutation of the batch permutes the variances and changes nothing else (T != N: a sample index taken from the
    # token dimension would show here)
    perm = [2, 0, 1]
    _, permuted, _ = glm_predictive(model, est, x[perm].contiguous())
    report(f"attention {kind} batch_first={batch_first} permuted batch", rel2(permuted, variance[perm]))
    assert rel2(permuted, variance) > 1e-2                                   # (the samples do differ)
    if hasattr(est, "hooks"):
        for hook in est.hooks:
            hook.remove()


@pytest.mark.parametrize("batch_first", [False, True], ids=["tokens_first", "batch_first"])
def test_attention_exact_efb(gpu, batch_first):
    from curvature_amd.curvatures import EFB
    model, x, labels, jac, layers = attention(batch_first)
    gen = torch.Generator().manual_seed(6)
    eig = {}
    for l in layers:
        m, n = l.weight.shape[0], l.weight.shape[1] + 1
        eig[l] = (torch.linalg.qr(torch.randn(n, n, generator=gen))[0].to(gpu),
                  torch.linalg.qr(torch.randn(m, m, generator=gen))[0].to(gpu))
    efb = EFB(model, {}, eigvecs=eig, per_sample=True)
    model.eval()                                           # (the Jacobians are those of the eval-mode copy)
    model.zero_grad()
    logits = model(x)
    logits[:, 2].sum().backward()                          # g_n of output 2: P_n is jac[.][n][2]
    efb.update(N_ATTN)
    for hook in efb.hooks:
        hook.remove()
    for k, layer in enumerate(layers):
        U_A, U_G = (t.double().cpu() for t in eig[layer])
        P = torch.stack([jac[k][n][2] for n in range(N_ATTN)])
        report(f"attention EFB(per_sample) batch_first={batch_first} layer {k}",
               rel2(efb.state[layer], N_ATTN * (U_G.t() @ P @ U_A).pow(2).sum(0)))
        report(f"attention EFB(per_sample) diags batch_first={batch_first} layer {k}",
               rel2(efb.diags[layer], N_ATTN * P.pow(2).sum(0)))


def test_attention_output_projection_names_a_missing_input_record(gpu):
    from curvature_amd.curvatures import KFAC, AttentionProjection
    model = torch.nn.Sequential()
    model.add_module("attn", torch.nn.MultiheadAttention(8, 2))
    est = KFAC(model.to(gpu))
    proj_in, proj_out = AttentionProjection.of(model.attn)
    est.record[proj_out] = [torch.zeros(15, 8, device=gpu), torch.zeros(15, 8, device=gpu)]
    with pytest.raises(RuntimeError, match="input projection, which has no record"):
        est._per_sample_operands("KFAC", [proj_out])
    est.record[proj_in] = [torch.zeros(5, 8, device=gpu), torch.zeros(5, 24, device=gpu)]
    with pytest.raises(RuntimeError, match="unbatched"):
        est._per_sample_operands("KFAC", [proj_out])
    for hook in est.hooks:
        hook.remove()


def test_off_by_default(gpu):
    """Without the switch a bf16 autocast pass and a ConvTranspose2d are refused as they always were, by name."""
    from curvature_amd import ops
    from curvature_amd.curvatures import Diagonal
    from curvature_amd.evaluate import glm_predictive
    ops.widen_per_sample(False)
    model = half_model(gpu)
    x, labels = half_batch(gpu)
    diag = Diagonal(model, per_sample=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = F.cross_entropy(model(x).float(), labels)
    loss.backward()
    with pytest.raises(RuntimeError, match="bfloat16.*widen_per_sample"):
        diag.update(N_HALF)
    for hook in diag.hooks:
        hook.remove()
    decoder_model, z, _, _ = decoder()
    with pytest.raises(NotImplementedError, match="up1"):
        glm_predictive(decoder_model, decoder_estimator("kfac"), z)


# ------------------------------------------------------------------------------------------------ 4. unchanged ground
def test_fp32_lenet_is_bit_identical_through_the_general_pack(gpu, monkeypatch):
    """One route: LeNet-5 `Diagonal(per_sample=True).update`, `invert` and `glm_predictive` call curv_persample_pack_ex
    once per `ops.per_sample_pack` and never curv_persample_pack - whose adapter writes the same bits for every packed
    operand of the model."""
    from curvature_amd import _lib, models, ops
    from curvature_amd.curvatures import Diagonal
    from curvature_amd.evaluate import glm_predictive
    torch.manual_seed(0)
    model = models.lenet5().to(gpu)
    x, labels = torch.randn(8, 1, 28, 28, device=gpu), torch.randint(0, 10, (8,), device=gpu)
    calls = {"curv_persample_pack": 0, "curv_persample_pack_ex": 0, "per_sample_pack": 0}
    handle = _lib.lib()
    direct = handle.curv_persample_pack
    for name in ("curv_persample_pack", "curv_persample_pack_ex"):
        def counted(*args, _name=name, _original=getattr(handle, name)):
            calls[_name] += 1
            return _original(*args)
        monkeypatch.setattr(handle, name, counted, raising=False)
    layouts, original = [], ops.per_sample_pack

    def through_the_adapter(op):
        """`op` packed by curv_persample_pack itself, and whether its source is (N, H, W, C)."""
        geo = op.pack
        N, C, H, W = geo.shape
        nhwc = geo.strides[1] == 1 and (C > 1 or H * W == 1)
        assert op.src.dtype == torch.float32 and geo.out_size is None
        assert all(d == 1 or s == w for d, s, w in
                   zip(geo.shape, geo.strides, (H * W * C, 1, W * C, C) if nhwc else (C * H * W, H * W, W, 1)))
        arr = (_lib.curv_persample_pack_desc * 1)()
        d = arr[0]
        dst = torch.full((op.floats,), float("nan"), device=gpu)
        d.src, d.dst = op.src.data_ptr(), dst.data_ptr()
        d.N, d.C, d.H, d.W = geo.shape
        (d.kh, d.kw), (d.sh, d.sw), (d.ph, d.pw) = geo.kernel, geo.stride, geo.padding
        d.has_bias, d.channels_last, d.rows_outer, d.Lp = int(geo.has_bias), int(nhwc), int(op.rows_outer), op.Lp
        assert direct(_lib.stream_ptr(), arr, 1) == 0, handle.curv_last_error()
        return dst, nhwc

    def recorded(operands, dsts):
        calls["per_sample_pack"] += bool(operands)             # (an empty call makes no library call)
        original(operands, dsts)
        for op, wrote in zip(operands, dsts):
            again, nhwc = through_the_adapter(op)
            assert torch.equal(again.view(torch.int32), wrote[:op.floats].view(torch.int32))
            layouts.append(nhwc)
    monkeypatch.setattr(ops, "per_sample_pack", recorded)
    est = Diagonal(model, per_sample=True)
    F.cross_entropy(model(x), labels).backward()
    est.update(8)
    est.invert(add=0.5, multiply=2.0)
    glm_predictive(model, est, x, outputs=[0, 7])
    for hook in est.hooks:
        hook.remove()
    assert calls["per_sample_pack"] >= 2 and calls["curv_persample_pack_ex"] == calls["per_sample_pack"]
    assert calls["curv_persample_pack"] == 0
    assert layouts.count(True) >= 6 and layouts.count(False) >= 2            # three Linear layers, two Conv2d inputs
