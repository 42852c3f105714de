"""KFAC and Diagonal on an nn.Embedding (`ops.admit_embedding`) against the twin that makes the layer a
bias-free Linear on one-hot rows and goes through the existing Linear paths: same labels, same backward pass.  The
embedding's matrix is `weight` (V, D), the twin's `weight.T`: every per-layer quantity is compared transposed.  The diagonal
form is exact because the twin's A is diagonal, which is asserted too.  Bar: rel_fro < 1e-4 (conftest.rel_fro)."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import rel_fro
from curvature_amd import io, ops
from curvature_amd.curvatures import KFAC, Diagonal
from curvature_amd.evaluate import glm_predictive

pytestmark = pytest.mark.gpu
TOL = 1e-4
V, D, N, T = 11, 6, 4, 5


@pytest.fixture(autouse=True)
def admitted():
    was = ops.admit_embedding(True)
    yield
    ops.admit_embedding(was)


class TokenModel(nn.Module):
    """Embedding(11, 6) -> Linear(6, 8) -> tanh -> mean over T -> Linear(8, 4); `twin`: the embedding as
    Linear(11, 6, bias=False) on one-hot rows."""

    def __init__(self, twin=False, pad=None):
        super().__init__()
        self.pad, self.twin = pad, twin
        self.emb = nn.Linear(V, D, bias=False) if twin else nn.Embedding(V, D, padding_idx=pad)
        self.fc1, self.fc2 = nn.Linear(D, 8), nn.Linear(8, 4)
        if twin and pad is not None:
            self.register_buffer("pad_row", torch.zeros(D))

    def forward(self, idx):
        if self.twin:
            x = F.one_hot(idx, V).float()
            if self.pad is None:
                h = self.emb(x)
            else:
                # the one-hot rows are zeroed at padding, where the embedding has no gradient; the row it looks up there
                # enters as a constant
                h = self.emb(x * (idx != self.pad).unsqueeze(-1)) + (idx == self.pad).unsqueeze(-1) * self.pad_row
        else:
            h = self.emb(idx)
        return self.fc2(torch.tanh(self.fc1(h)).mean(1))


def _pair(dev, pad=None):
    torch.manual_seed(3)
    model = TokenModel(pad=pad).to(dev)
    with torch.no_grad():
        model.emb.weight.normal_()                      # (also the padding row: a mean that a sampler must leave alone)
    twin = TokenModel(twin=True, pad=pad).to(dev)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    if pad is not None:
        state["pad_row"] = state["emb.weight"][pad].clone()
    state["emb.weight"] = state["emb.weight"].t().contiguous()
    twin.load_state_dict(state)
    return model, twin


def _batches(dev, pad=None):
    gen = torch.Generator().manual_seed(4)
    out = []
    for _ in range(2):
        idx = torch.randint(0, V, (N, T), generator=gen)
        if pad is not None:
            idx[0, :2], idx[2, 4] = pad, pad
        out.append((idx.to(dev), torch.randint(0, 4, (N,), generator=gen).to(dev)))
    return out


def _updated(cls, dev, pad=None, **kwargs):
    """(estimator, twin estimator, model, twin model) after two update() calls on the same two batches."""
    model, twin = _pair(dev, pad)
    est = cls(model, ['Embedding', 'Linear'], **kwargs)
    ref = cls(twin, ['Linear'], **kwargs)
    for idx, labels in _batches(dev, pad):
        for m, e in ((model, est), (twin, ref)):
            m.zero_grad()
            F.cross_entropy(m(idx), labels).backward()
            e.update(N)
    return est, ref, model, twin


def _rows(t, pad):
    """The rows of a (V, ...) quantity that are compared with the twin: all but the padding row."""
    keep = [v for v in range(V) if v != pad]
    return t[keep]


HYPERS = [(0.5, 1.0), ([0.3, 0.5, 0.7], [1.0, 2.0, 3.0])]


@pytest.mark.parametrize("pad", [None, 0])
def test_kfac_against_the_one_hot_twin(gpu, pad):
    est, ref, model, twin = _updated(KFAC, gpu, pad)
    a, G = est.state[model.emb]
    A_twin, G_twin = ref.state[twin.emb]
    assert tuple(a.shape) == (V,) and tuple(G.shape) == (D, D)
    assert torch.equal(A_twin - torch.diag(torch.diag(A_twin)), torch.zeros_like(A_twin))      # exactly diagonal
    assert rel_fro(a, torch.diag(A_twin)) < TOL and rel_fro(G, G_twin) < TOL
    if pad is not None:
        assert a[pad] == 0
    for layer, other in ((model.fc1, twin.fc1), (model.fc2, twin.fc2)):
        assert all(rel_fro(x, y) < TOL for x, y in zip(est.state[layer], ref.state[other]))
    for add, multiply in HYPERS:
        est.invert(add, multiply)
        ref.invert(add, multiply)
        l_a, L_G = est.inv_state[model.emb]
        L_A_twin, L_G_twin = ref.inv_state[twin.emb]
        assert rel_fro(_rows(l_a, pad), _rows(torch.diag(L_A_twin), pad)) < TOL and rel_fro(L_G, L_G_twin) < TOL
        if pad is not None:
            assert l_a[pad] == 0
        # the twin's noise is (n, m) = (V, D) as well: its sample (D, V) is ours transposed
        z = torch.randn(V, D, generator=torch.Generator().manual_seed(9)).to(gpu)
        ours, theirs = est.sample(model.emb, z), ref.sample(twin.emb, z).t()
        assert tuple(ours.shape) == (V, D) and rel_fro(_rows(ours, pad), _rows(theirs, pad)) < TOL
        if pad is not None:
            assert bool((ours[pad] == 0).all())


@pytest.mark.parametrize("pad", [None, 0])
def test_kfac_samplers_write_mean_plus_sample(gpu, pad):
    est, _, model, _ = _updated(KFAC, gpu, pad)
    est.invert(0.5, 1.0)
    mean = est.model_state_of(model.emb, 'weight').clone()
    noise = {l: torch.randn(est.inv_state[l][0].shape[-1], est.inv_state[l][1].shape[-1],
                            generator=torch.Generator().manual_seed(k)).to(gpu) for k, l in enumerate(est._layers())}
    est.sample_and_replace(noise)
    want = mean + est.sample(model.emb, noise[model.emb])
    assert rel_fro(model.emb.weight, want) < TOL
    assert rel_fro(model.fc1.weight, est.model_state_of(model.fc1, 'weight') + est.sample(model.fc1, noise[model.fc1])[:, :-1]) < TOL
    if pad is not None:
        assert torch.equal(model.emb.weight[pad], mean[pad])
    # noise pinned by noise_seed: the same draw twice, another after it; the padding row stays at its mean bit for bit
    est.noise_seed, est.noise_offset = 17, 0
    est.sample_and_replace()
    first = model.emb.weight.detach().clone()
    est.sample_and_replace()
    assert not torch.equal(first, model.emb.weight)
    est.noise_offset = 0
    est.sample_and_replace()
    assert torch.equal(first, model.emb.weight)
    assert rel_fro(first, mean) > 1e-3
    if pad is not None:
        assert torch.equal(first[pad], mean[pad])
    # sample_many / replace_from: set k is mean + sample(z_k)
    many = {l: torch.stack([z, -2 * z]) for l, z in noise.items()}
    bank = est.sample_many(2, many)
    assert tuple(bank.weights[model.emb].shape) == (2, V, D) and bank.biases[model.emb] is None
    assert rel_fro(bank.weights[model.emb][0], want) < TOL
    assert rel_fro(bank.weights[model.emb][1], mean - 2 * est.sample(model.emb, noise[model.emb])) < TOL
    est.replace_from(bank, 1)
    assert torch.equal(model.emb.weight, bank.weights[model.emb][1])
    drawn = est.sample_many(3)
    assert tuple(drawn.weights[model.emb].shape) == (3, V, D) and bool(torch.isfinite(drawn.weights[model.emb]).all())
    if pad is not None:
        assert all(torch.equal(drawn.weights[model.emb][k][pad], mean[pad]) for k in range(3))


@pytest.mark.parametrize("pad", [None, 0])
@pytest.mark.parametrize("cls,kwargs", [(KFAC, {}), (Diagonal, {}), (Diagonal, {"per_sample": True})])
def test_glm_predictive_equals_the_twins(gpu, cls, kwargs, pad):
    est, ref, model, twin = _updated(cls, gpu, pad, **kwargs)
    est.invert(0.5, 2.0)
    ref.invert(0.5, 2.0)
    # (the twin has a posterior spread on the padding row, whose one-hot rows are zeroed: it never reaches an output)
    idx = _batches(gpu, pad)[1][0]
    logits, variance, probs = glm_predictive(model, est, idx)
    logits_t, variance_t, probs_t = glm_predictive(twin, ref, idx)
    assert rel_fro(logits, logits_t) < TOL
    assert bool((variance > 0).all()) and rel_fro(variance, variance_t) < TOL and rel_fro(probs, probs_t) < TOL


@pytest.mark.parametrize("pad", [None, 0])
@pytest.mark.parametrize("per_sample", [False, True])
def test_diagonal_against_the_one_hot_twin(gpu, per_sample, pad):
    est, ref, model, twin = _updated(Diagonal, gpu, pad, per_sample=per_sample)
    state, state_t = est.state[model.emb], ref.state[twin.emb].t()
    assert tuple(state.shape) == (V, D) and rel_fro(state, state_t) < TOL
    if pad is not None:
        assert bool((state[pad] == 0).all())
    for add, multiply in HYPERS:
        est.invert(add, multiply)
        ref.invert(add, multiply)
        inv, inv_t = est.inv_state[model.emb], ref.inv_state[twin.emb].t()
        assert rel_fro(_rows(inv, pad), _rows(inv_t, pad)) < TOL
        z = torch.randn(V, D, generator=torch.Generator().manual_seed(9)).to(gpu)
        ours, theirs = est.sample(model.emb, z), ref.sample(twin.emb, z.t().contiguous()).t()
        assert rel_fro(_rows(ours, pad), _rows(theirs, pad)) < TOL
        if pad is not None:
            assert bool((inv[pad] == 0).all()) and bool((ours[pad] == 0).all())
    mean = est.model_state_of(model.emb, 'weight').clone()
    est.noise_seed, est.noise_offset = 5, 0
    est.sample_and_replace()
    assert rel_fro(model.emb.weight, mean) > 1e-3
    if pad is not None:
        assert torch.equal(model.emb.weight[pad], mean[pad])


def test_diagonal_evidence_terms_leave_the_padding_row_out(gpu):
    pad = 0
    est, ref, model, twin = _updated(Diagonal, gpu, pad)
    hypers = [(0.5, 2.0), (2.0, 30.0), ([0.3, 0.5, 0.7], [1.0, 2.0, 3.0])]
    ours, theirs = est.log_det_grid(hypers, per_layer=True).cpu(), ref.log_det_grid(hypers, per_layer=True).cpu()
    gone = torch.tensor([D * math.log(s * 0 + n) for n, s in ((0.5, 2.0), (2.0, 30.0), (0.3, 1.0))], dtype=torch.float64)
    assert ours.dtype == torch.float64 and rel_fro(ours[0], theirs[0] - gone) < 1e-9 and rel_fro(ours[1:], theirs[1:]) < 1e-6
    assert rel_fro(est.log_det_grid(hypers).cpu(), ref.log_det_grid(hypers).cpu() - gone) < 1e-9
    # the prior: the row's squares and its D counts are left out
    w = est.model_state_of(model.emb, 'weight').double().cpu()
    n = torch.tensor([0.5, 2.0, 0.3], dtype=torch.float64)
    row = -0.5 * n * w[pad].square().sum() + 0.5 * D * torch.log(n)
    assert rel_fro(est.log_prior_grid(hypers).cpu(), ref.log_prior_grid(hypers).cpu() - row) < 1e-9


@pytest.mark.parametrize("cls", [KFAC, Diagonal])
def test_state_round_trip(gpu, cls, tmp_path):
    est, _, model, _ = _updated(cls, gpu, 0)
    est.invert(0.5, 1.0)
    path = str(tmp_path / "state.pt")
    io.save_state(est, path, attrs=("state", "inv_state"))
    other = cls(_pair(gpu, 0)[0], ['Embedding', 'Linear'])
    io.load_state(other, path, "state")
    io.load_state(other, path, "inv_state")
    emb = other.model.emb
    for attr in ("state", "inv_state"):
        mine, theirs = getattr(est, attr)[model.emb], getattr(other, attr)[emb]
        for x, y in zip(mine, theirs) if cls is KFAC else ((mine, theirs),):
            assert x.shape == y.shape and y.is_cuda and torch.equal(x, y)
    if cls is KFAC:
        assert tuple(other.state[emb][0].shape) == (V,)
    z = torch.randn(V, D, generator=torch.Generator().manual_seed(1)).to(gpu)
    assert torch.equal(est.sample(model.emb, z), other.sample(emb, z))


def test_switch_off_refuses_as_before(gpu):
    ops.admit_embedding(False)
    model, _ = _pair(gpu)
    for cls in (KFAC, Diagonal):
        with pytest.raises(AssertionError):
            cls(model, ['Embedding', 'Linear'])
        assert model.emb not in cls(model)._layers()            # never part of the default selection
