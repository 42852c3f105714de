"""The per-sample line of a Conv3d on the GPU, with `ops.admit_conv_nd` and
`ops.admit_conv3d_per_sample` on: the exact Fisher of Diagonal / EFB against per-sample gradients from batch-size-1 backward
passes on a float64 copy of the model (autograd only), and every linearised predictive against its dense float64 form,
with per-sample Jacobians from autograd and the estimator's own state upcast.

The model is that of tests/test_conv_nd_cpu.py: Conv3d(2, 4, 3, p1) - ReLU - Conv3d(4, 4, (1, 3, 3), s(1, 2, 2), p(0, 1, 1)) -
Flatten - Linear(144, 5) on a (4, 2, 4, 6, 6) input; all three layers are selected.  The bar is the project's (`TOL` of
tests/test_per_sample_gpu.py and tests/test_glm_predictive_gpu.py): relative 2-norm error below 1e-4 against float64.
The float64 references are made once and shared."""
import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import inf_predictive_refs as refs

pytestmark = pytest.mark.gpu
TOL = 1e-4
N, CLASSES = 4, 5
KINDS = ["Conv3d", "Linear"]
ADD, MULTIPLY = 0.5, 2.0
HYPERS = [(0.5, 2.0), (0.05, 1.0), (3.0, 8.0)]
OLD_TEXT = "a 3-D convolution: a sample's product sums over the output depths"


@pytest.fixture(autouse=True)
def admitted():
    from curvature_amd import ops
    was = ops.admit_conv_nd(True), ops.admit_conv3d_per_sample(True)
    yield ops
    ops.admit_conv_nd(was[0])
    ops.admit_conv3d_per_sample(was[1])


def rel2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


def model3d():
    return torch.nn.Sequential(torch.nn.Conv3d(2, 4, 3, padding=1), torch.nn.ReLU(),
                               torch.nn.Conv3d(4, 4, (1, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1)), torch.nn.Flatten(),
                               torch.nn.Linear(4 * 4 * 3 * 3, CLASSES))


def matrix_layers(model):
    return [l for l in model if l.__class__.__name__ in KINDS + ["Conv2d"]]


def as_matrix(gw, gb):
    """[W.grad | b.grad] as the layer matrix (m, n + 1), columns in the order of ``weight.reshape(Cout, -1)``."""
    return torch.cat([gw.reshape(gw.shape[0], -1), gb.reshape(-1, 1)], dim=1)


def backward(model, x, labels):
    model.zero_grad()
    F.cross_entropy(model(x), labels).backward()


@functools.lru_cache(maxsize=None)
def case():
    """The model on the GPU, two batches, and from a float64 CPU copy (autograd only): `grads[b][k][n]`, the gradient of
    sample n's own loss of batch b with respect to layer k's [W | b], and `jac[k]` (N, classes, m, n + 1), the Jacobians of
    the logits of batch 0."""
    gpu = torch.device("cuda:0")
    torch.manual_seed(11)
    model = model3d().to(gpu).eval()
    batches = [(torch.randn(N, 2, 4, 6, 6, device=gpu), torch.randint(0, CLASSES, (N,), device=gpu)) for _ in range(2)]
    twin = copy.deepcopy(model).double().cpu().eval()
    layers = matrix_layers(twin)
    params = [p for l in layers for p in (l.weight, l.bias)]
    grads = []
    for x, labels in batches:
        x64, y = x.double().cpu(), labels.cpu()
        per_layer = [[] for _ in layers]
        for n in range(N):
            g = torch.autograd.grad(F.cross_entropy(twin(x64[n:n + 1]), y[n:n + 1]), params)
            for k in range(len(layers)):
                per_layer[k].append(as_matrix(g[2 * k], g[2 * k + 1]))
        grads.append([torch.stack(p) for p in per_layer])
    logits = twin(batches[0][0].double().cpu())
    jac = [torch.zeros(N, CLASSES, l.weight.shape[0], l.weight[0].numel() + 1, dtype=torch.float64) for l in layers]
    for n in range(N):
        for c in range(CLASSES):
            g = torch.autograd.grad(logits[n, c], params, retain_graph=True)
            for k in range(len(layers)):
                jac[k][n, c] = as_matrix(g[2 * k], g[2 * k + 1])
    return dict(model=model, batches=batches, grads=grads, jac=jac, logits=logits.detach())


def fisher_reference(k, rotate=None):
    """batch_size * sum_n P_n**2 over both batches, P_n = (gradient of sample n's loss) / N its share in the batch gradient;
    `rotate` = (U_A, U_G): of U_G^T P_n U_A."""
    total = 0
    for per_layer in case()["grads"]:
        P = per_layer[k] / N
        if rotate is not None:
            P = rotate[1].t() @ P @ rotate[0]
        total = total + N * (P * P).sum(0)
    return total


# ------------------------------------------------------------------------------------------------ exact Fisher
def test_diagonal_is_the_per_sample_fisher(gpu):
    from curvature_amd.curvatures import Diagonal
    c = case()
    model = c["model"]
    diag = Diagonal(model, KINDS, per_sample=True)
    for x, labels in c["batches"]:
        backward(model, x, labels)
        diag.update(N)
    for hook in diag.hooks:
        hook.remove()
    for k, layer in enumerate(matrix_layers(model)):
        err = rel2(diag.state[layer], fisher_reference(k))
        print(f"conv3d model, Diagonal(per_sample) layer {k}: rel 2-norm error {err:.3e}")
        assert err < TOL


def test_efb_eigenvalue_state_is_the_rotated_per_sample_fisher(gpu):
    from curvature_amd.curvatures import EFB, KFAC
    c = case()
    model = c["model"]
    kfac = KFAC(model, KINDS)
    backward(model, *c["batches"][0])
    kfac.update(N)
    for hook in kfac.hooks:
        hook.remove()
    efb = EFB(model, kfac.state, KINDS, per_sample=True)
    for x, labels in c["batches"]:
        backward(model, x, labels)
        efb.update(N)
    for hook in efb.hooks:
        hook.remove()
    for k, layer in enumerate(matrix_layers(model)):
        U_A, U_G = (u.double().cpu() for u in efb.eigvecs[layer])
        err = rel2(efb.state[layer], fisher_reference(k, (U_A, U_G)))
        err_d = rel2(efb.diags[layer], fisher_reference(k))
        print(f"conv3d model, EFB(per_sample) layer {k}: lambda {err:.3e}, diags {err_d:.3e}")
        assert err < TOL and err_d < TOL


# ------------------------------------------------------------------------------------------------ estimators
@functools.lru_cache(maxsize=None)
def estimator(kind):
    """`kind` after one update on batch 0 and ``invert(ADD, MULTIPLY)`` (KFAC decomposed as well); no hooks of the chain's
    helpers are left on the model."""
    from curvature_amd import ops
    from curvature_amd.curvatures import EFB, INF, KFAC, Diagonal
    c = case()
    model, (x, labels) = c["model"], c["batches"][0]
    was = ops.admit_conv_nd(True), ops.admit_conv3d_per_sample(True)          # (cached: may be made outside a test)
    try:
        if kind == "diag":
            est = Diagonal(model, KINDS, per_sample=True)
            backward(model, x, labels)
            est.update(N)
        else:
            kfac = KFAC(model, KINDS)
            backward(model, x, labels)
            kfac.update(N)
            est = kfac
            if kind == "kfac":
                kfac.decompose()
            else:
                for hook in kfac.hooks:
                    hook.remove()
                est = efb = EFB(model, kfac.state, KINDS, per_sample=kind == "efb")
                backward(model, x, labels)
                efb.update(N)
                if kind == "inf":
                    diag = Diagonal(model, KINDS)
                    backward(model, x, labels)
                    diag.update(N)
                    est = INF(model, diag.state, kfac.state, efb.state, KINDS, eigvecs=efb.eigvecs)
                    est.update(rank=100)
                    for hook in getattr(efb, "hooks", []):
                        hook.remove()
        est.invert(ADD, MULTIPLY)
    finally:
        ops.admit_conv_nd(was[0])
        ops.admit_conv3d_per_sample(was[1])
    model.zero_grad()
    return est


def float64_covariance(kind, est):
    """(N, classes, classes): sum over the layers of <T(P_c), T(P_c')> with T(P) = L_G^T P L_A (KFAC), inv * P (Diagonal),
    inv * (U_G^T P U_A) (EFB); INF: P_c^T Pi^-1 P_c' with the dense inverse of the regularised precision."""
    c = case()
    want = torch.zeros(N, CLASSES, CLASSES, dtype=torch.float64)
    for k, layer in enumerate(matrix_layers(c["model"])):
        P = c["jac"][k]
        if kind == "inf":
            ua, ug, lam, corr = (t.detach().double().cpu() for t in est.state[layer])
            dense = refs.dense_covariance(ua, ug, lam.reshape(-1), corr.reshape(-1).clamp_min(0.0), ADD, MULTIPLY)
            p = P.transpose(2, 3).reshape(N, CLASSES, -1)                      # index i m + j, i on the input side
            want += torch.einsum("nce,ef,ndf->ncd", p, dense, p)
            continue
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


# ------------------------------------------------------------------------------------------------ predictive
@pytest.mark.parametrize("kind", ["diag", "kfac", "efb", "inf"])
def test_glm_predictive_against_float64(gpu, kind, admitted):
    from curvature_amd.evaluate import glm_predictive
    c = case()
    est = estimator(kind)
    was = admitted.admit_inf_predictive(kind == "inf")
    try:
        logits, variance, probs = glm_predictive(c["model"], est, c["batches"][0][0])
    finally:
        admitted.admit_inf_predictive(was)
    want = torch.diagonal(float64_covariance(kind, est), dim1=1, dim2=2)
    err = rel2(variance, want)
    print(f"conv3d model, {kind}: glm_predictive variance: rel 2-norm error {err:.3e}")
    assert tuple(variance.shape) == (N, CLASSES)
    assert err < TOL
    assert rel2(logits, c["logits"]) < TOL
    probit = torch.softmax(logits.double().cpu() / torch.sqrt(1.0 + math.pi / 8.0 * want), dim=1)
    assert float((probs.double().cpu() - probit).abs().max()) < 1e-5


def test_glm_predictive_joint_kfac(gpu):
    from curvature_amd.evaluate import glm_predictive_joint
    c = case()
    est = estimator("kfac")
    _, covariance, probs = glm_predictive_joint(c["model"], est, c["batches"][0][0])
    err = rel2(covariance, float64_covariance("kfac", est))
    print(f"conv3d model, kfac: joint covariance (K = 5): rel Frobenius error {err:.3e}")
    assert tuple(covariance.shape) == (N, CLASSES, CLASSES)
    assert err < TOL
    assert torch.equal(covariance, covariance.transpose(1, 2))
    assert float((probs.sum(1) - 1.0).abs().max()) < 1e-5


def test_glm_predictive_mc_kfac(gpu):
    """Pinned noise; the expected softmax in float64 from the float64 logits' covariance."""
    from curvature_amd.evaluate import glm_predictive_mc
    c = case()
    est = estimator("kfac")
    S = 500
    z = torch.randn(N, S, CLASSES, generator=torch.Generator().manual_seed(21)).to(gpu)
    logits, covariance, probs = glm_predictive_mc(c["model"], est, c["batches"][0][0], samples=S, noise=z)
    sigma = float64_covariance("kfac", est)
    L = torch.linalg.cholesky(sigma)
    draws = logits.double().cpu()[:, None, :] + torch.einsum("nsk,nck->nsc", z.double().cpu(), L)
    want = torch.softmax(draws, dim=2).mean(dim=1)
    err = rel2(probs, want)
    print(f"conv3d model, kfac: MC softmax against float64: rel 2-norm error {err:.3e}; covariance "
          f"{rel2(covariance, sigma):.3e}")
    assert err < TOL and rel2(covariance, sigma) < TOL
    assert float((probs.sum(dim=1) - 1).abs().max()) < 1e-5


def test_glm_predictive_grid_kfac(gpu):
    from curvature_amd.evaluate import glm_predictive_grid
    c = case()
    est = estimator("kfac")
    _, variance, probs = glm_predictive_grid(c["model"], est, c["batches"][0][0], HYPERS)
    want = torch.zeros(len(HYPERS), N, CLASSES, dtype=torch.float64)
    for k, layer in enumerate(matrix_layers(c["model"])):
        A, G = (t.double().cpu() for t in est.state[layer])
        (lam_A, U_A), (lam_G, U_G) = torch.linalg.eigh(A), torch.linalg.eigh(G)
        lam_A, lam_G = lam_A.clamp_min(0), lam_G.clamp_min(0)
        Q = U_G.t() @ c["jac"][k] @ U_A
        for h, (add, multiply) in enumerate(HYPERS):
            root = math.sqrt(add / multiply)
            w = 1.0 / ((lam_G + root)[:, None] * (lam_A + root)[None, :])
            want[h] += (w * Q * Q).sum((2, 3)) / multiply
    assert tuple(variance.shape) == tuple(probs.shape) == (len(HYPERS), N, CLASSES)
    for h in range(len(HYPERS)):
        err = rel2(variance[h], want[h])
        print(f"conv3d model, kfac: grid row {HYPERS[h]}: rel 2-norm error {err:.3e}")
        assert err < TOL


# ------------------------------------------------------------------------------------------------ twin, autocast, off
def test_depth_equal_to_the_kernel_is_the_conv2d_model(gpu):
    """Conv3d with D = kd, pd = 0 against the Conv2d on x.reshape(N, C kd, H, W) with the same weights."""
    from curvature_amd.curvatures import KFAC, Diagonal
    from curvature_amd.evaluate import glm_predictive
    torch.manual_seed(5)
    deep = torch.nn.Sequential(torch.nn.Conv3d(2, 4, (3, 3, 3), padding=(0, 1, 1)), torch.nn.ReLU(), torch.nn.Flatten(),
                               torch.nn.Linear(4 * 5 * 6, CLASSES)).to(gpu).eval()
    flat = torch.nn.Sequential(torch.nn.Conv2d(6, 4, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten(),
                               torch.nn.Linear(4 * 5 * 6, CLASSES)).to(gpu).eval()
    with torch.no_grad():
        flat[0].weight.copy_(deep[0].weight.reshape(4, 6, 3, 3))
        flat[0].bias.copy_(deep[0].bias)
        flat[3].weight.copy_(deep[3].weight)
        flat[3].bias.copy_(deep[3].bias)
    x = torch.randn(N, 2, 3, 5, 6, device=gpu)
    labels = torch.randint(0, CLASSES, (N,), device=gpu)
    out = {}
    for name, model, inp, kinds in (("deep", deep, x, ["Conv3d", "Linear"]), ("flat", flat, x.reshape(N, 6, 5, 6), ["Conv2d", "Linear"])):
        diag = Diagonal(model, kinds, per_sample=True)
        kfac = KFAC(model, kinds)
        backward(model, inp, labels)
        diag.update(N)
        kfac.update(N)
        for hook in diag.hooks:
            hook.remove()
        kfac.invert(ADD, MULTIPLY)
        _, variance, _ = glm_predictive(model, kfac, inp)
        for hook in kfac.hooks:
            hook.remove()
        out[name] = [diag.state[l] for l in matrix_layers(model)], variance
    for k, (a, b) in enumerate(zip(out["deep"][0], out["flat"][0])):
        err = rel2(a, b)
        print(f"twin: Diagonal(per_sample) layer {k}: Conv3d against Conv2d {err:.3e}")
        assert a.shape == b.shape and err < TOL
    err = rel2(out["deep"][1], out["flat"][1])
    print(f"twin: KFAC variance: Conv3d against Conv2d {err:.3e}")
    assert err < TOL


def unfold3d(x, kernel, stride, padding):
    n, ch = x.shape[:2]
    padded = F.pad(x, (padding[2], padding[2], padding[1], padding[1], padding[0], padding[0]))
    u = padded.unfold(2, kernel[0], stride[0]).unfold(3, kernel[1], stride[1]).unfold(4, kernel[2], stride[2])
    return u.permute(0, 1, 5, 6, 7, 2, 3, 4).reshape(n, ch * kernel[0] * kernel[1] * kernel[2], -1)


def test_bf16_autocast_records_with_the_wider_line(gpu, admitted):
    """The exact Fisher from the records of a bf16-autocast pass against the float64 form of the same records, upcast."""
    from curvature_amd.curvatures import Diagonal
    c = case()
    model, (x, labels) = c["model"], c["batches"][0]
    was = admitted.widen_per_sample(True)
    diag = Diagonal(model, KINDS, per_sample=True)
    try:
        model.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = F.cross_entropy(model(x), labels)
        loss.backward()
        diag.update(N)
    finally:
        admitted.widen_per_sample(was)
        for hook in diag.hooks:
            hook.remove()
    halves = 0
    for k, layer in enumerate(matrix_layers(model)):
        fwd, bwd = (t.detach().double().cpu() for t in diag.record[layer])
        halves += sum(t.dtype == torch.bfloat16 for t in diag.record[layer])
        if layer.__class__.__name__ == "Conv3d":
            X = unfold3d(fwd, layer.kernel_size, layer.stride, layer.padding)
            g = bwd.reshape(N, bwd.shape[1], -1)
        else:
            X, g = fwd.reshape(N, -1, 1), bwd.reshape(N, -1, 1)
        X = torch.cat([X, torch.ones(N, 1, X.shape[2], dtype=torch.float64)], dim=1)
        P = torch.einsum("nml,nkl->nmk", g, X)
        err = rel2(diag.state[layer], N * (P * P).sum(0))
        print(f"bf16 autocast, Diagonal(per_sample) layer {k}: rel 2-norm error {err:.3e}")
        assert err < TOL
    assert halves >= 3                                                        # the pass did record half tensors


def test_with_the_new_switch_off_every_call_raises_as_before(gpu, admitted):
    from curvature_amd.curvatures import EFB, Diagonal
    from curvature_amd.evaluate import (glm_predictive, glm_predictive_grid, glm_predictive_joint, glm_predictive_mc)
    c = case()
    model, x = c["model"], c["batches"][0][0]
    kfac, inf = estimator("kfac"), estimator("inf")
    admitted.admit_conv3d_per_sample(False)
    for make in (lambda: Diagonal(model, KINDS, per_sample=True), lambda: EFB(model, kfac.state, KINDS, per_sample=True)):
        with pytest.raises(NotImplementedError) as err:
            make()
        assert "'0'" in str(err.value) and OLD_TEXT in str(err.value)
    calls = [lambda: glm_predictive(model, kfac, x), lambda: glm_predictive_joint(model, kfac, x),
             lambda: glm_predictive_mc(model, kfac, x, samples=8), lambda: glm_predictive_grid(model, kfac, x, HYPERS),
             lambda: glm_predictive(model, estimator("diag"), x), lambda: glm_predictive(model, estimator("efb"), x)]
    for call in calls:
        with pytest.raises(NotImplementedError) as err:
            call()
        assert "'0'" in str(err.value) and OLD_TEXT in str(err.value)
    was = admitted.admit_inf_predictive(True)
    try:
        with pytest.raises(NotImplementedError, match="3-D convolution"):
            glm_predictive(model, inf, x)
    finally:
        admitted.admit_inf_predictive(was)
    with pytest.raises(NotImplementedError, match="^per-sample update: unsupported layer Conv3d$"):
        admitted.per_sample_operands(model[0], x, torch.zeros(N, 4, 4, 6, 6, device=gpu))
