"""LayerNorm, GroupNorm and eval-mode BatchNorm2d in KFAC and Diagonal, end to end on the GPU, against a
float64 twin of the model on the CPU: the records, the exact Fisher diagonal, the stacked KFAC factors, their inversion
and the sampler, the linearised predictive, the refusals, and the default selection with the switch on and off.
Bars: rel_fro < 1e-4 for matrices, relative 2-norm error < 1e-4 for the per-sample variances (TOL of
tests/test_glm_predictive_gpu.py)."""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import rel_fro
from curvature_amd import ops

pytestmark = pytest.mark.gpu
TOL = 1e-4
N, CLASSES = 4, 4
TYPES = ['Conv2d', 'Linear', 'GroupNorm', 'BatchNorm2d', 'LayerNorm']
NORMS = (nn.GroupNorm, nn.BatchNorm2d, nn.LayerNorm)


@pytest.fixture(autouse=True)
def admitted():
    was = ops.admit_norm_layers(True)
    yield
    ops.admit_norm_layers(was)


def make_model(inplace=True):
    torch.manual_seed(21)
    model = nn.Sequential(nn.Conv2d(3, 6, 3), nn.GroupNorm(3, 6), nn.ReLU(), nn.Conv2d(6, 8, 3), nn.BatchNorm2d(8),
                          nn.ReLU(inplace=inplace), nn.AdaptiveAvgPool2d(2), nn.Flatten(), nn.LayerNorm(32), nn.Linear(32, 4))
    gen = torch.Generator().manual_seed(22)
    model[4].running_mean.copy_(0.3 * torch.randn(8, generator=gen))
    model[4].running_var.copy_(torch.rand(8, generator=gen) + 0.5)
    for m in model:                                                              # gains and shifts away from 1 and 0
        if isinstance(m, NORMS):
            m.weight.data.add_(0.2 * torch.randn(m.weight.shape, generator=gen))
            m.bias.data.add_(0.2 * torch.randn(m.bias.shape, generator=gen))
    return model.eval()


def selected(model):
    return [m for m in model if isinstance(m, (nn.Conv2d, nn.Linear) + NORMS)]


def matrix_of(layer, grads=False):
    w = layer.weight.grad if grads else layer.weight
    b = layer.bias.grad if grads else layer.bias
    rows = w.numel() if isinstance(layer, NORMS) else w.shape[0]
    return torch.cat([w.reshape(rows, -1), b.reshape(-1, 1)], 1).detach().clone()


def standardised(layer, x):
    if isinstance(layer, nn.LayerNorm):
        return F.layer_norm(x, layer.normalized_shape, None, None, layer.eps)
    if isinstance(layer, nn.GroupNorm):
        return F.group_norm(x, layer.num_groups, None, None, layer.eps)
    return F.batch_norm(x, layer.running_mean, layer.running_var, None, None, False, 0.0, layer.eps)


@functools.lru_cache(maxsize=None)
def case():
    """The model, a batch and, from a float64 twin with an out-of-place ReLU: the records of the mean cross-entropy's
    backward pass at the norm layers, the per-sample gradients and the Jacobians of the outputs per selected layer as
    [W | b] matrices.  Made once and left unchanged."""
    model = make_model()
    gen = torch.Generator().manual_seed(23)
    x, labels = torch.randn(N, 3, 8, 8, generator=gen), torch.tensor([0, 3, 1, 2])
    m64 = make_model(inplace=False).double()
    m64.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
    layers = selected(m64)
    records = {}
    hooks = []
    for k, layer in enumerate(layers):
        def forward(module, inputs, output, k=k):
            records[k] = [inputs[0].detach().clone(), None]
            output.register_hook(lambda grad, k=k: records[k].__setitem__(1, grad.detach().clone()))
        hooks.append(layer.register_forward_hook(forward))
    m64.zero_grad()
    F.cross_entropy(m64(x.double()), labels).backward()
    batch_records = {k: tuple(v) for k, v in records.items()}
    for hook in hooks:
        hook.remove()
    per_sample, jac = [], []
    for n in range(N):
        m64.zero_grad()
        (F.cross_entropy(m64(x[n:n + 1].double()), labels[n:n + 1], reduction="sum") / N).backward()
        per_sample.append([matrix_of(l, grads=True) for l in layers])
        rows = []
        for c in range(CLASSES):
            m64.zero_grad()
            m64(x[n:n + 1].double())[0, c].backward()
            rows.append([matrix_of(l, grads=True) for l in layers])
        jac.append(rows)
    return dict(model=model, m64=m64, x=x, labels=labels, records=batch_records, per_sample=per_sample, jac=jac)


def on_gpu(gpu):
    sc = case()
    return sc, copy.deepcopy(sc["model"]).to(gpu), sc["x"].to(gpu), sc["labels"].to(gpu)


def factors64(sc, k, layer64, a_scale, g_scale):
    """[A (C, 2, 2), G (C, 1, 1)] of norm layer k in float64 from the twin's records."""
    x, g = sc["records"][k]
    xh = standardised(layer64, x)
    if isinstance(layer64, nn.LayerNorm):
        xh, g = xh.reshape(N, -1, 32).transpose(1, 2), g.reshape(N, -1, 32).transpose(1, 2)
    else:
        xh, g = xh.flatten(2), g.flatten(2)
    rows = [xh, torch.ones_like(xh)]
    A = torch.stack([torch.stack([(r * q).sum((0, 2)) for q in rows], 1) for r in rows], 1)
    return a_scale * A, g_scale * g.square().sum((0, 2)).view(-1, 1, 1)


def test_records_of_the_batchnorm_before_the_inplace_relu(gpu):
    from curvature_amd.curvatures import KFAC
    sc, model, x, labels = on_gpu(gpu)
    est = KFAC(model, TYPES)
    assert est._layers() == selected(model)                                      # modules() order
    F.cross_entropy(model(x), labels).backward()
    for k, layer in enumerate(selected(model)):
        if isinstance(layer, NORMS):
            forward, backward = est.record[layer]
            assert rel_fro(forward, sc["records"][k][0]) < TOL and rel_fro(backward, sc["records"][k][1]) < TOL
    for hook in est.hooks:
        hook.remove()


def test_diagonal_exact_fisher(gpu):
    from curvature_amd.curvatures import Diagonal
    sc, model, x, labels = on_gpu(gpu)
    est = Diagonal(model, TYPES, per_sample=True)
    F.cross_entropy(model(x), labels).backward()
    est.update(N)
    for k, layer in enumerate(selected(model)):
        want = N * sum(sc["per_sample"][n][k] ** 2 for n in range(N))
        assert tuple(est.state[layer].shape) == tuple(want.shape)
        err = rel_fro(est.state[layer], want)
        print(f"Diagonal per-sample state, layer {k} ({type(layer).__name__}): rel Frobenius error {err:.3e}")
        assert err < TOL
    for hook in est.hooks:
        hook.remove()
    # at batch size 1 the exact diagonal is the default update's
    model.zero_grad()
    exact, default = Diagonal(model, TYPES, per_sample=True), Diagonal(model, TYPES)
    F.cross_entropy(model(x[:1]), labels[:1]).backward()
    exact.update(1)
    default.update(1)
    for layer in selected(model):
        assert rel_fro(exact.state[layer], default.state[layer]) < TOL
    for hook in exact.hooks:
        hook.remove()


def test_kfac_factors(gpu):
    from curvature_amd.curvatures import KFAC
    sc, model, x, labels = on_gpu(gpu)
    est = KFAC(model, TYPES)
    F.cross_entropy(model(x), labels).backward()
    est.update(N)
    norms = [(k, l, l64) for k, (l, l64) in enumerate(zip(selected(model), selected(sc["m64"]))) if isinstance(l, NORMS)]
    assert [type(l) for _, l, _ in norms] == list(NORMS)
    want = {}
    for k, layer, layer64 in norms:
        L = sc["records"][k][0].numel() // N // layer.weight.numel()
        want[layer] = factors64(sc, k, layer64, 1.0 / (N * L), float(N) / L)
        A, G = est.state[layer]
        assert tuple(A.shape) == (layer.weight.numel(), 2, 2) and tuple(G.shape) == (layer.weight.numel(), 1, 1)
        errs = rel_fro(A, want[layer][0]), rel_fro(G, want[layer][1])
        print(f"KFAC factors of {type(layer).__name__}: rel Frobenius errors {errs[0]:.3e} {errs[1]:.3e}")
        assert max(errs) < TOL
    est.update(N, inputs=False)                                                  # G again
    est.update(N, grads=False, input_weight=3.0)                                 # A three times more
    for _, layer, _ in norms:
        assert rel_fro(est.state[layer][0], 4 * want[layer][0]) < TOL
        assert rel_fro(est.state[layer][1], 2 * want[layer][1]) < TOL
    for hook in est.hooks:
        hook.remove()


def fitted(kind, model, x, labels, types=TYPES):
    """An estimator after one update and an inversion under which every damped factor is well conditioned (add 0.5)."""
    from curvature_amd.curvatures import KFAC, Diagonal
    est = KFAC(model, types) if kind == "kfac" else Diagonal(model, types)
    model.zero_grad()
    F.cross_entropy(model(x), labels).backward()
    est.update(x.shape[0])
    est.invert(add=0.5, multiply=2.0)
    return est


def test_inversion_and_sampling(gpu):
    sc, model, x, labels = on_gpu(gpu)
    est = fitted("kfac", model, x, labels)
    means = {l: (l.weight.detach().clone(), l.bias.detach().clone()) for l in selected(model)}
    gen = torch.Generator().manual_seed(24)
    noise = {}
    for layer in est._layers():
        first, second = est.inv_state[layer]
        shape = (first.shape[0], first.shape[-1], second.shape[-1]) if first.dim() == 3 else (first.shape[-1], second.shape[-1])
        noise[layer] = torch.randn(shape, generator=gen).to(gpu)
    est.sample_and_replace(noise=noise)
    for layer in selected(model):
        if not isinstance(layer, NORMS):
            continue
        C = layer.weight.numel()
        L_A, L_G = (t.double().cpu() for t in est.inv_state[layer])
        for side, (L, factor) in enumerate(zip((L_A, L_G), est.state[layer])):
            # the reference's definition per channel: L L^T = (sqrt(multiply) F + sqrt(add) I)^-1
            damped = 2.0 ** 0.5 * factor.double().cpu() + 0.5 ** 0.5 * torch.eye(factor.shape[-1], dtype=torch.float64)
            assert rel_fro(L @ L.transpose(1, 2) @ damped, torch.eye(factor.shape[-1], dtype=torch.float64).expand_as(damped)) < TOL
            assert torch.equal(L, torch.tril(L))
        z = noise[layer].double().cpu()
        rows = torch.stack([(L_A[c] @ z[c] @ L_G[c].t()).t() for c in range(C)]).view(C, 2)
        assert layer.weight.shape == means[layer][0].shape and layer.weight.dim() == 1 and layer.bias.dim() == 1
        assert rel_fro(layer.weight, means[layer][0].double().cpu() + rows[:, 0]) < TOL
        assert rel_fro(layer.bias, means[layer][1].double().cpu() + rows[:, 1]) < TOL
        assert torch.equal(est.model_state_of(layer, 'weight'), means[layer][0])
    est._reload_mean()
    for layer in selected(model):
        assert torch.equal(layer.weight, means[layer][0]) and torch.equal(layer.bias, means[layer][1])
    bank = est.sample_many(2)
    est.replace_from(bank, 1)
    norm = selected(model)[1]
    assert norm.weight.dim() == 1 and not torch.equal(norm.weight, means[norm][0])
    assert torch.equal(norm.weight, bank.weights[norm][1].view(-1))
    for hook in est.hooks:
        hook.remove()


def variance64(kind, est, model, jac):
    """J Sigma J^T per (sample, output) in float64, Sigma the covariance the estimator samples from: per layer and channel
    (L_G L_G^T) kron (L_A L_A^T), or diag(inv**2)."""
    want = torch.zeros(N, CLASSES, dtype=torch.float64)
    for k, layer in enumerate(selected(model)):
        if kind == "kfac":
            L_A, L_G = (t.double().cpu() for t in est.inv_state[layer])
            if L_A.dim() == 2:
                L_A, L_G = L_A.unsqueeze(0), L_G.unsqueeze(0)
            groups, m = L_A.shape[0], L_G.shape[-1]
        for n in range(N):
            for c in range(CLASSES):
                J = jac[n][c][k]
                if kind == "kfac":
                    want[n, c] += sum(float((L_G[g].t() @ J[g * m:(g + 1) * m] @ L_A[g]).pow(2).sum()) for g in range(groups))
                else:
                    want[n, c] += float((est.inv_state[layer].double().cpu() ** 2 * J * J).sum())
    return want


@pytest.mark.parametrize("kind", ["kfac", "diag"])
def test_glm_predictive_against_float64_jacobians(gpu, kind):
    from curvature_amd.evaluate import glm_predictive
    sc, model, x, labels = on_gpu(gpu)
    est = fitted(kind, model, x, labels)
    logits, variance, probs = glm_predictive(model, est, x)
    want = variance64(kind, est, model, sc["jac"])
    err = rel_fro(variance, want)
    print(f"glm_predictive {kind}: rel 2-norm error of the variances {err:.3e}")
    assert err < TOL
    for n in range(N):
        assert rel_fro(variance[n], want[n]) < TOL
    assert torch.allclose(probs.sum(1), torch.ones(N, device=gpu), atol=1e-5)
    assert not est.__dict__.get("_predictive_kept")
    if kind == "kfac":
        for hook in est.hooks:
            hook.remove()


def test_refusals_name_a_norm_layer(gpu):
    from curvature_amd.curvatures import EFB, INF, KFAC, BlockDiagonal
    from curvature_amd.evaluate import glm_predictive_grid, glm_predictive_joint
    sc, model, x, labels = on_gpu(gpu)
    est = fitted("kfac", model, x, labels)
    named = r"'(1|4|8)'"                                                         # the three norm layers of the Sequential
    with pytest.raises(NotImplementedError, match=named):
        glm_predictive_joint(model, est, x)
    with pytest.raises(NotImplementedError, match=named):
        est.decompose()
    with pytest.raises(NotImplementedError, match=named):
        glm_predictive_grid(model, est, x, [(0.5, 2.0)])
    for build in (lambda: EFB(model, {}, TYPES), lambda: INF(model, {}, {}, {}, TYPES), lambda: BlockDiagonal(model, TYPES)):
        with pytest.raises(NotImplementedError, match=named):
            build()
    model.train()
    with pytest.raises(NotImplementedError, match=r"'4'.*model\.eval\(\)"):
        model(x)
    model.eval()
    for hook in est.hooks:
        hook.remove()


def test_default_selection_is_the_same_with_the_switch_on_and_off(gpu):
    from curvature_amd.curvatures import KFAC
    sc, model, x, labels = on_gpu(gpu)
    states = []
    for on in (True, False):
        ops.admit_norm_layers(on)
        est = KFAC(model)
        model.zero_grad()
        F.cross_entropy(model(x), labels).backward()
        est.update(N)
        assert all(not isinstance(l, NORMS) for l in est.state)
        states.append([t.clone() for l in est.state for t in est.state[l]])
        for hook in est.hooks:
            hook.remove()
    assert len(states[0]) == len(states[1]) == 6
    assert all(torch.equal(a, b) for a, b in zip(*states))
