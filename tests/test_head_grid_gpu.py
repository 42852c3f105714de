"""Last-layer Laplace predictive over a grid of damping pairs on the GPU: csrc/head_grid.hip through `ops.head_grid`
against float64 (tests/head_grid_refs.py) in both forms, inside NaN fences, with its chunks, batches and bit-level promises;
`Curvature.head_terms_grid` of KFAC, EFB and Diagonal against the dense covariance from the explicit regularised inverse and
against `invert` + `head_terms` pair by pair; the drivers `evaluate.last_layer_predictive_grid` / `tune_last_layer` against
`glm_predictive_grid` on an estimator that holds the head alone, against `ops.head_mc`'s reference and against a loop of
`invert` + `eval_last_layer`.

The bar is the project's (`TOL` of tests/test_head_mc_gpu.py): relative Frobenius error below 1e-4
against float64.  Every measured error is printed; on an MI355X the worst of them was 4.4e-7 (KFAC `head_terms_grid` against
`invert` + `head_terms`; the kernel alone: 1.8e-7)."""
import functools

import numpy
import pytest
import torch

from head_grid_refs import condition, head_grid_covariance_reference, head_grid_reference
from head_refs import head_mc_reference

pytestmark = pytest.mark.gpu
TOL = 1e-4


def rel2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    denom = float(torch.linalg.norm(b))
    return float(torch.linalg.norm(a - b)) / denom if denom > 0 else float(torch.linalg.norm(a - b))


# ------------------------------------------------------------------------------------------------ inputs
def fenced_rows(values, gpu, pad=3):
    """(R, C) values as a view with row stride C + pad, one row and one column into a NaN-filled buffer (the view starts
    4 bytes past a row start: no alignment beyond a float).  Returns (view, buffer)."""
    R, C = values.shape
    buf = torch.full((R + 2, C + pad), float("nan"))
    buf[1:R + 1, 1:C + 1] = values
    buf = buf.to(gpu)
    return buf[1:R + 1, 1:C + 1], buf


def fenced_vector(values, gpu):
    n = values.shape[0]
    buf = torch.full((n + 8,), float("nan"))
    buf[3:3 + n] = values
    buf = buf.to(gpu)
    return buf[3:3 + n], buf


def fenced_out(H, N, K, gpu):
    buf = torch.full((H * N * K + 16,), float("nan"), device=gpu)
    return buf[5:5 + H * N * K].view(H, N, K), buf


def out_fences_intact(buf, count):
    return bool(torch.isnan(buf[:5]).all()) and bool(torch.isnan(buf[5 + count:]).all())


def spectrum(rows, cols, gen):
    """Non-negative values of a rank-deficient factor: a third of the entries, the first among them, are exact zeros."""
    values = 2.0 * torch.rand(rows, cols, generator=gen)
    values[torch.rand(rows, cols, generator=gen) < 1.0 / 3.0] = 0.0
    values.view(-1)[0] = 0.0
    return values


def grid_points(H):
    """`shift` spanning 1e-4 .. 1e2 and unequal gains, as the float32 values the kernel receives."""
    shift = torch.logspace(-4, 2, H) if H > 1 else torch.tensor([1e-4])
    gain = 1.0 / (1.0 + torch.arange(H, dtype=torch.float32)) ** 2
    return [float(x) for x in shift.float()], [float(x) for x in gain.float()]


# (N, K, n, H): every K of {1, 3, 31, 32, 33, 65, 130}, n of {1, 2, 31, 33, 65, 145}, N of {1, 3, 33}, H of {1, 3, 16}; both
# forms run every case.  n <= 128 is one chunk, 145 two; (4, 40, 2049) is the issue's cheap many-chunk shape (17 chunks).
SHAPES = [(1, 1, 1, 1), (3, 3, 2, 3), (33, 31, 31, 16), (1, 32, 33, 3), (3, 33, 65, 1), (33, 65, 145, 16), (3, 130, 145, 3),
          (1, 130, 2, 16), (4, 40, 2049, 16)]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]


@functools.lru_cache(maxsize=None)
def primitive_case(index, separable):
    """The operands of SHAPES[index] on the GPU inside NaN fences, and the float64 reference; made once."""
    N, K, n, H = SHAPES[index]
    gpu = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(500 + 2 * index + separable)
    y = torch.randn(N, n, generator=gen)
    Y, y_buf = fenced_rows(y, gpu)
    shift, gain = grid_points(H)
    if separable:
        u, u_buf = fenced_vector(spectrum(1, K, gen)[0], gpu)
        v, v_buf = fenced_vector(spectrum(1, n, gen)[0], gpu)
        want = head_grid_reference(Y, shift, gain, u=u, v=v)
        return dict(Y=Y, u=u, v=v, T=None, shift=shift, gain=gain, want=want, inputs=(y_buf, u_buf, v_buf))
    T, t_buf = fenced_rows(spectrum(K, n, gen), gpu, pad=5)
    want = head_grid_reference(Y, shift, gain, T=T)
    return dict(Y=Y, u=None, v=None, T=T, shift=shift, gain=gain, want=want, inputs=(y_buf, t_buf))


def run(case, pairs=None, out=None):
    from curvature_amd import ops
    pairs = range(len(case["shift"])) if pairs is None else pairs
    shift, gain = [case["shift"][h] for h in pairs], [case["gain"][h] for h in pairs]
    N, n = case["Y"].shape
    K = case["want"].shape[2]
    view, buf = fenced_out(len(shift), N, K, case["Y"].device) if out is None else out
    ops.head_grid([ops.HeadGridJob(case["Y"], case["u"], case["v"], case["T"], view, shift, gain)])
    torch.cuda.synchronize()
    return view, buf


# ------------------------------------------------------------------------------------------------ 1. the primitive
@pytest.mark.parametrize("separable", [False, True], ids=["dense", "separable"])
@pytest.mark.parametrize("index", range(len(SHAPES)), ids=SHAPE_IDS)
def test_head_grid_against_float64(gpu, index, separable):
    case = primitive_case(index, separable)
    before = [b.clone() for b in case["inputs"]]
    got, buf = run(case)
    assert torch.isfinite(got).all() and out_fences_intact(buf, got.numel())
    for b, was in zip(case["inputs"], before):                   # the operands and their fences are as they were
        assert torch.equal(torch.isnan(b), torch.isnan(was)) and torch.equal(b.nan_to_num(0.0), was.nan_to_num(0.0))
    worst = max(rel2(g, w) for g, w in zip(got, case["want"]))
    print(f"head_grid {'separable' if separable else 'dense'} {SHAPE_IDS[index]}: worst pair {worst:.3e}")
    assert worst < TOL


def test_the_smallest_chunked_shape(gpu):
    """Found with the host query: the first n at which a 1 x 1 output needs scratch - two chunks of the sum over i."""
    from curvature_amd import _lib, ops
    L = _lib.lib()

    def need(n):
        job = ops.HeadGridJob(None, None, None, None, None, [1.0], [1.0], N=1, K=1, n=n, separable=False)
        return L.curv_head_grid_workspace_bytes(ops._head_grid_descs([job], check_tensors=False), 1)
    n = next(n for n in range(1, 4096) if need(n) > 0)
    assert n == 129 and need(n - 1) == 0
    gen = torch.Generator().manual_seed(77)
    for N, K in ((1, 1), (3, 33)):
        Y, _ = fenced_rows(torch.randn(N, n, generator=gen), gpu)
        T, _ = fenced_rows(spectrum(K, n, gen), gpu)
        shift, gain = grid_points(3)
        case = dict(Y=Y, u=None, v=None, T=T, shift=shift, gain=gain, want=head_grid_reference(Y, shift, gain, T=T))
        got, buf = run(case)
        worst = max(rel2(g, w) for g, w in zip(got, case["want"]))
        print(f"head_grid dense {N}x{K}x{n} (two chunks): worst pair {worst:.3e}")
        assert out_fences_intact(buf, got.numel()) and worst < TOL


# ------------------------------------------------------------------------------------------------ 2. bits
@pytest.mark.parametrize("separable", [False, True], ids=["dense", "separable"])
@pytest.mark.parametrize("index", [2, 5], ids=["one_chunk", "two_chunks"])
def test_a_pair_has_the_same_bits_alone_and_in_a_list_of_16(gpu, index, separable):
    case = primitive_case(index, separable)
    assert len(case["shift"]) == 16
    together, _ = run(case)
    for h in range(16):
        alone, _ = run(case, pairs=[h])
        assert torch.equal(alone[0], together[h])
    some, _ = run(case, pairs=[11, 2, 7])
    assert torch.equal(some, together[[11, 2, 7]])


def test_an_item_has_the_same_bits_alone_and_in_a_batch(gpu):
    """17 items of both forms and different shapes: three launches."""
    from curvature_amd import ops
    cases = [primitive_case(i % len(SHAPES), (i // 2) % 2 == 0) for i in range(17)]
    jobs, outs = [], []
    for case in cases:
        H, N, K = case["want"].shape
        outs.append([torch.full((H, N, K), float("nan"), device=gpu) for _ in range(2)])
        jobs.append([ops.HeadGridJob(case["Y"], case["u"], case["v"], case["T"], o, case["shift"], case["gain"])
                     for o in outs[-1]])
    ops.head_grid([j[0] for j in jobs])
    for j in jobs:
        ops.head_grid([j[1]])
    torch.cuda.synchronize()
    for together, alone in outs:
        assert torch.isfinite(together).all() and torch.equal(together, alone)


def test_ops_refuses_wrong_shapes_strides_and_dtypes(gpu):
    """... naming the item, before anything is launched: the outputs keep their NaN."""
    from curvature_amd import ops
    N, K, n, H = 3, 5, 6, 2
    Y, T = torch.ones(N, n, device=gpu), torch.ones(K, n, device=gpu)
    u, v = torch.ones(K, device=gpu), torch.ones(n, device=gpu)
    out = torch.full((H, N, K), float("nan"), device=gpu)
    good = ops.HeadGridJob(Y, None, None, T, out, [1.0] * H, [1.0] * H)

    def job(Y=Y, u=None, v=None, T=T, out=out):
        return ops.HeadGridJob(Y, u, v, T, out, [1.0] * H, [1.0] * H, N=N, K=K, n=n)
    wide = torch.ones(N, 2 * n, device=gpu)
    for bad, match in ((job(Y=wide[:, ::2]), "item 1: Y must be an .3,6. view with unit last stride"),
                       (job(Y=torch.ones(N + 1, n, device=gpu)), "item 1: Y must be"),
                       (job(T=torch.ones(K, 2 * n, device=gpu)[:, ::2]), "item 1: T must be a .5,6. view with unit column"),
                       (job(T=torch.ones(n, K, device=gpu)), "item 1: T must be"),
                       (job(T=None, u=torch.ones(K + 1, device=gpu), v=v), "item 1: u must be a contiguous vector of 5"),
                       (job(T=None, u=u, v=torch.ones(2 * n, device=gpu)[::2]), "item 1: v must be a contiguous vector of 6"),
                       (job(out=torch.ones(H, N, K + 1, device=gpu)[:, :, :K]), "item 1: out must be a contiguous .2,3,5."),
                       (job(out=torch.ones(H + 1, N, K, device=gpu)), "item 1: out must be"),
                       (job(Y=Y.double()), "expects float32 tensors, got torch.float64"),
                       (job(T=T.half()), "expects float32 tensors, got torch.float16")):
        with pytest.raises(RuntimeError, match=match):
            ops.head_grid([good, bad])
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    ops.head_grid([good])
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full((H, N, K), float(n) / 2.0, device=gpu))       # sum of 6 ones / (1 + 1), gain 1


# ------------------------------------------------------------------------------------------------ 3. head_terms_grid
PAIRS = [(1.0, 50.0), (10.0, 100.0), (0.1, 1.0), (5.0, 20.0)]


def head_model(gpu, bias=True):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.ReLU(), torch.nn.Flatten(),
                                torch.nn.Linear(4 * 6 * 6, 7, bias=bias))
    return model.to(gpu)


def batches(gpu, count=2, N=5):
    gen = torch.Generator().manual_seed(21)
    return [(torch.randn(N, 1, 8, 8, generator=gen).to(gpu), torch.randint(0, 7, (N,), generator=gen).to(gpu))
            for _ in range(count)]


def make_estimator(kind, model, data, layer_types=None):
    """`kind` after one update per batch of `data`: no inversion; KFAC decomposed."""
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
    else:
        est.decompose()
    model.zero_grad()
    return est


def dense_grid(M, d2):
    """M diag(d2[h, n]) M^T in float64: (H, N, K, K)."""
    d2 = d2.double().cpu()
    M = torch.eye(d2.shape[-1], dtype=torch.float64) if M is None else M.double().cpu()
    return torch.einsum("ca,hna,da->hncd", M, d2, M)


def dense_of(terms):
    """M diag(d2) M^T in float64 from what `head_terms` returned (tests/test_head_mc_gpu.py)."""
    d2 = terms.d2.double().cpu()
    N, K = terms.variance.shape
    d2 = d2[:, None].expand(N, K) if d2.dim() == 1 else d2
    M = torch.eye(K, dtype=torch.float64) if terms.M is None else terms.M.double().cpu()
    if terms.lower:
        M = torch.tril(M)
    return torch.einsum("ca,na,da->ncd", M, d2, M)


def features_of(model, gpu, seed=8):
    x = torch.randn(5, 1, 8, 8, generator=torch.Generator().manual_seed(seed)).to(gpu)
    with torch.no_grad():
        return x, model[:3](x)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("kind", ["KFAC", "EFB", "Diagonal"])
def test_head_terms_grid(gpu, kind, bias):
    model = head_model(gpu, bias)
    est = make_estimator(kind, model, batches(gpu))
    head = model[3]
    _, features = features_of(model, gpu)
    assert not est.inv_state
    terms = est.head_terms_grid(head, features, PAIRS)
    H, N, K = len(PAIRS), 5, 7
    assert tuple(terms.d2.shape) == (H, N, K) and tuple(terms.variance.shape) == (H, N, K)
    assert (terms.M is None) == (kind == "Diagonal")
    assert terms.M is None or (tuple(terms.M.shape) == (K, K) and terms.M.stride(1) == 1)
    assert not est.inv_state                                       # neither needed nor touched

    # the conditioning the comparison with the inversion rests on, in float64
    state = est.state[head]
    for pair in PAIRS:
        assert condition(kind, state, pair) < 1e3
    sigma = head_grid_covariance_reference(kind, state, getattr(est, "eigvecs", {}).get(head), features, bias, PAIRS)
    got = dense_grid(terms.M, terms.d2)
    e_var = max(rel2(terms.variance[h], torch.diagonal(sigma[h], dim1=1, dim2=2)) for h in range(H))
    e_cov = max(rel2(got[h], sigma[h]) for h in range(H))

    # bf16 features give the bits of their upcast
    half = est.head_terms_grid(head, features.bfloat16(), PAIRS)
    up = est.head_terms_grid(head, features.bfloat16().float(), PAIRS)
    assert torch.equal(half.d2, up.d2) and torch.equal(half.variance, up.variance)

    # pair by pair against the inversion
    e_inv, e_inv_ref = 0.0, 0.0
    for h, pair in enumerate(PAIRS):
        est.invert(*pair)
        single = est.head_terms(head, features)
        e_inv = max(e_inv, rel2(got[h], dense_of(single)), rel2(terms.variance[h], single.variance))
        e_inv_ref = max(e_inv_ref, rel2(dense_of(single), sigma[h]))
    print(f"head_terms_grid {kind} bias={bias}: variance {e_var:.3e}, M diag(d2) M^T {e_cov:.3e}, against invert + "
          f"head_terms {e_inv:.3e} (that path against float64: {e_inv_ref:.3e})")
    assert e_var < TOL and e_cov < TOL and e_inv < TOL and e_inv_ref < TOL


@pytest.mark.parametrize("kind", ["KFAC", "EFB", "Diagonal"])
def test_seventeen_pairs_are_two_chunks_concatenated(gpu, kind):
    model = head_model(gpu)
    est = make_estimator(kind, model, batches(gpu))
    head = model[3]
    _, features = features_of(model, gpu)
    pairs = [(10.0 ** (-2 + 0.2 * h), 10.0 + 7.0 * h) for h in range(17)]
    whole = est.head_terms_grid(head, features, pairs)
    first, last = est.head_terms_grid(head, features, pairs[:16]), est.head_terms_grid(head, features, pairs[16:])
    assert tuple(whole.d2.shape) == (17, 5, 7)
    assert torch.equal(whole.d2, torch.cat([first.d2, last.d2]))
    assert torch.equal(whole.variance, torch.cat([first.variance, last.variance]))
    assert torch.isfinite(whole.variance).all() and bool((whole.variance > 0).all())


@pytest.mark.parametrize("kind", ["KFAC", "Diagonal"])
def test_per_layer_lists_resolve_to_the_heads_entries(gpu, kind):
    model = head_model(gpu)
    est = make_estimator(kind, model, batches(gpu))
    head = model[3]
    assert list(est.state) == [model[0], head]
    _, features = features_of(model, gpu)
    lists = [([3.0, 1.0], [7.0, 50.0]), ([0.25, 10.0], [2.0, 100.0])]      # (conv, head) entries of add and multiply
    got = est.head_terms_grid(head, features, lists)
    want = est.head_terms_grid(head, features, [(1.0, 50.0), (10.0, 100.0)])
    assert torch.equal(got.d2, want.d2) and torch.equal(got.variance, want.variance)
    other = est.head_terms_grid(head, features, [(3.0, 7.0), (0.25, 2.0)])
    assert not torch.equal(got.d2, other.d2)


def test_kfac_needs_a_current_decomposition(gpu):
    model = head_model(gpu)
    data = batches(gpu)
    est = make_estimator("KFAC", model, data)
    _, features = features_of(model, gpu)
    est.head_terms_grid(model[3], features, PAIRS)
    torch.nn.functional.cross_entropy(model(data[0][0]), data[0][1]).backward()
    est.update(5)
    model.zero_grad()
    with pytest.raises(RuntimeError, match=r"KFAC.head_terms_grid: layer '3'.*call decompose\(\) after the last update\(\)"):
        est.head_terms_grid(model[3], features, PAIRS)
    with pytest.raises(RuntimeError, match=r"features must be \(N, 144\)"):
        make_estimator("Diagonal", model, data).head_terms_grid(model[3], features[:, :100], PAIRS)


# ------------------------------------------------------------------------------------------------ 4. drivers
@pytest.mark.parametrize("kind", ["KFAC", "EFB", "Diagonal"])
def test_against_the_per_sample_grid(gpu, kind):
    """The estimator holds the head alone, so the whole-network GLM grid is the head's."""
    from curvature_amd.evaluate import glm_predictive_grid, last_layer_predictive_grid
    model = head_model(gpu)
    est = make_estimator(kind, model, batches(gpu), layer_types="Linear")
    assert list(est.state) == [model[3]]
    x, _ = features_of(model, gpu, seed=9)
    logits, variance, probs = last_layer_predictive_grid(model, est, x, PAIRS)
    logits_g, variance_g, probs_g = glm_predictive_grid(model, est, x, PAIRS)
    assert tuple(variance.shape) == tuple(probs.shape) == (len(PAIRS), 5, 7)
    assert torch.equal(logits, logits_g)
    e_var = max(rel2(a, b) for a, b in zip(variance, variance_g))
    e_probs = max(rel2(a, b) for a, b in zip(probs, probs_g))
    print(f"{kind}: against glm_predictive_grid: variance {e_var:.3e} probs {e_probs:.3e}")
    assert e_var < TOL and e_probs < TOL
    assert float((probs.sum(dim=2) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("kind", ["KFAC", "EFB", "Diagonal"])
def test_mc_grid(gpu, kind):
    from curvature_amd.evaluate import last_layer_predictive_grid
    model = head_model(gpu)
    est = make_estimator(kind, model, batches(gpu))
    head = model[3]
    x, features = features_of(model, gpu, seed=10)
    N, K, S = 5, 7, 64
    z = torch.randn(N, S, K, generator=torch.Generator().manual_seed(12)).to(gpu)
    est.noise_seed, est.noise_offset = 91, 40
    logits, variance, probs = last_layer_predictive_grid(model, est, x, PAIRS, predictive="mc", samples=S, noise=z)
    assert est.noise_offset == 40                                  # explicit noise: the stream is not touched
    terms = est.head_terms_grid(head, features, PAIRS)
    assert torch.equal(variance, terms.variance)
    worst = 0.0
    for h in range(len(PAIRS)):
        want, _ = head_mc_reference(terms.M, False, terms.d2[h], logits.float(), z)
        worst = max(worst, rel2(probs[h], want))
    print(f"{kind}: mc grid against float64 per pair: {worst:.3e}")
    assert worst < TOL

    # the estimator's stream: one stretch for every pair - common random numbers - and one advance per call
    all_pairs = last_layer_predictive_grid(model, est, x, PAIRS, predictive="mc", samples=S)[2]
    assert est.noise_offset == 40 + N * S * 2                      # ceil(7 / 4) = 2 counters per draw
    for h, pair in enumerate(PAIRS):
        est.noise_offset = 40
        one = last_layer_predictive_grid(model, est, x, [pair], predictive="mc", samples=S)[2]
        assert est.noise_offset == 40 + N * S * 2
        assert torch.equal(one[0], all_pairs[h])
    assert float((all_pairs.sum(dim=2) - 1).abs().max()) < 1e-5
    est.use_device_noise_counter(True)
    with pytest.raises(RuntimeError, match="last_layer_predictive_grid: .*device noise counter"):
        last_layer_predictive_grid(model, est, x, PAIRS, predictive="mc", samples=S)


@pytest.mark.parametrize("kind", ["KFAC", "EFB", "Diagonal"])
def test_tune_last_layer(gpu, kind):
    from curvature_amd.evaluate import eval_last_layer, tune_last_layer
    model = head_model(gpu)
    est = make_estimator(kind, model, batches(gpu))
    gen = torch.Generator().manual_seed(31)
    dataset = [(torch.randn(n, 1, 8, 8, generator=gen), torch.randint(0, 7, (n,), generator=gen)) for n in (4, 5)]
    hooks = [(len(m._forward_hooks), len(m._forward_pre_hooks)) for m in model.modules()]
    tuned = tune_last_layer(model, dataset, est, PAIRS)
    assert hooks == [(len(m._forward_hooks), len(m._forward_pre_hooks)) for m in model.modules()]
    assert not est.inv_state
    assert tuple(tuned["nll"].shape) == tuple(tuned["accuracy"].shape) == (len(PAIRS),)
    assert tuned["nll"].dtype == torch.float64 and not tuned["nll"].is_cuda
    nll, accuracy = [], []
    for pair in PAIRS:
        est.invert(*pair)
        predictions, labels = eval_last_layer(model, dataset, est)
        picked = predictions.astype(numpy.float64)[numpy.arange(len(labels)), labels]
        nll.append(float(-numpy.log(picked).mean()))
        accuracy.append(float((predictions.argmax(axis=1) == labels).mean()))
    worst = max(abs(a - b) / abs(b) for a, b in zip(tuned["nll"].tolist(), nll))
    print(f"{kind}: tune_last_layer nll {tuned['nll'].tolist()} against the loop {nll}: {worst:.3e}")
    assert worst < TOL
    assert tuned["best"] == min(range(len(PAIRS)), key=lambda h: nll[h]) == int(torch.argmin(tuned["nll"]))
    assert tuned["accuracy"].tolist() == accuracy
    mc = tune_last_layer(model, dataset, est, PAIRS, predictive="mc", samples=32)
    assert torch.isfinite(mc["nll"]).all() and 0 <= mc["best"] < len(PAIRS)


def test_refusals(gpu):
    from curvature_amd import ops
    from curvature_amd.curvatures import Diagonal
    from curvature_amd.evaluate import last_layer_predictive_grid
    model = head_model(gpu)
    data = batches(gpu, count=1)
    x = data[0][0]
    est = make_estimator("Diagonal", model, data)
    post = torch.nn.Sequential(*model, torch.nn.LogSoftmax(dim=1))
    with pytest.raises(RuntimeError, match="last_layer_predictive_grid: .*'3'.*post-processes"):
        last_layer_predictive_grid(post, est, x, PAIRS)
    with pytest.raises(RuntimeError, match="last_layer_predictive_grid: .*'3'.*did not run"):
        last_layer_predictive_grid(model[:3], est, x, PAIRS)
    conv_only = make_estimator("Diagonal", model, data, layer_types="Conv2d")
    with pytest.raises(RuntimeError, match="last_layer_predictive_grid: the estimator holds no nn.Linear layer in state"):
        last_layer_predictive_grid(model, conv_only, x, PAIRS)

    # K above the cap of head_mc: "mc" refuses and advises "probit", which works
    cap = ops.HEAD_MC_MAX_CLASSES
    torch.manual_seed(2)
    wide = torch.nn.Sequential(torch.nn.Linear(8, cap + 1)).to(gpu)
    xw, yw = torch.randn(4, 8, device=gpu), torch.randint(0, cap + 1, (4,), device=gpu)
    wide_est = Diagonal(wide)
    torch.nn.functional.cross_entropy(wide(xw), yw).backward()
    wide_est.update(4)
    with pytest.raises(ValueError, match=rf"last_layer_predictive_grid: .*HEAD_MC_MAX_CLASSES = {cap}.*probit"):
        last_layer_predictive_grid(wide, wide_est, xw, PAIRS, predictive="mc", samples=8)
    logits, variance, probs = last_layer_predictive_grid(wide, wide_est, xw, PAIRS)
    assert tuple(probs.shape) == (len(PAIRS), 4, cap + 1) and torch.isfinite(probs).all() and bool((variance > 0).all())
    assert float((probs.sum(dim=2) - 1).abs().max()) < 1e-5
