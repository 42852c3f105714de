"""Exact per-sample Fisher on the GPU: the pack and the product of csrc/persample.hip through the C ABI against float64
for every layer geometry, then ``Diagonal(per_sample=True)`` / ``EFB(per_sample=True)`` on LeNet-5 and on layers of a
ResNet-50, bit properties (alone / whole model / sharded) and the chain into INF.

Expected values are computed here, in float64, from `oracle.unfold_input`, `oracle.grad_matrix`, `oracle.diag_update` and
`oracle.efb_update`.  The bar is the project's: relative Frobenius error below 1e-4 against float64."""
import pytest
import torch

from conftest import rel_fro

pytestmark = pytest.mark.gpu
TOL = 1e-4


def fenced(shape, gpu, gen):
    """A contiguous random tensor whose storage is surrounded by NaN: whatever a kernel fetches outside it must not
    enter a result."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 128,), float("nan"), device=gpu)
    buf[64:64 + n] = torch.randn(n, generator=gen).to(gpu)
    return buf[64:64 + n].view(shape)


def sample_matrices(layer, x, g, n):
    """float64 (g_n, X_n) of sample n: (m, L) and (n_in [+ 1], L)."""
    import oracle.curvature_oracle as o
    has_bias = layer.bias is not None
    xn, gn = x[n:n + 1].detach().double().cpu(), g[n:n + 1].detach().double().cpu()
    if isinstance(layer, torch.nn.Conv2d):
        X = o.unfold_input(xn, layer.kernel_size, layer.stride, layer.padding, has_bias)
        return gn.reshape(gn.shape[1], -1), X
    X = o.unfold_input(xn.reshape(-1, xn.shape[-1]), None, None, None, has_bias)
    return gn.reshape(-1, gn.shape[-1]).t(), X


def per_sample_grads(layer, x, g):
    """[P_n] in float64: the share of every sample in [W.grad | b.grad]."""
    out = []
    for n in range(x.shape[0]):
        gn, X = sample_matrices(layer, x, g, n)
        out.append(gn @ X.t())
    return out


def split(P, layer):
    """(grad_w, grad_b) views of a [W | b] matrix for the oracle's update functions."""
    if layer.bias is not None:
        return P[:, :-1], P[:, -1]
    return P, None


def diag_reference(layer, x, g, batch_size):
    import oracle.curvature_oracle as o
    return sum(o.diag_update(*split(P, layer), batch_size) for P in per_sample_grads(layer, x, g))


def run_product(layer, x, g, alpha, dst, first, **layout):
    from curvature_amd import ops
    sides = ops.per_sample_operands(layer, x, g, **layout)
    flat = [sides.g, sides.x]
    bufs = ops.per_sample_scratch([op.floats for op in flat], x.device)
    packed = [(op, b) for op, b in zip(flat, bufs) if op.pack is not None]
    ops.per_sample_pack([op for op, _ in packed], [b for _, b in packed])
    gt, xt = (b if op.pack is not None else op.src for op, b in zip(flat, bufs))
    job = ops.PerSampleJob(gt, xt, dst, sides.N, sides.m, sides.n, sides.L, sides.g.ns, sides.g.rs, sides.x.ns,
                           sides.x.rs, alpha=alpha, first=first)
    flops = ops.per_sample_plan_flops([job])[0]
    assert flops >= 2 * sides.N * sides.m * sides.n * sides.L
    ops.per_sample_sq_accumulate([job])
    return sides


# (id, kind, cin, cout, kernel, stride, padding, H, S): output sides below 64, equal to 64 and no multiples of 128
CASES = [
    ("c3x3_L3136", "conv", 8, 64, 3, 1, 1, 56, 3),
    ("c3x3_L49", "conv", 32, 160, 3, 1, 1, 7, 32),
    ("c3x3_s2", "conv", 16, 48, 3, 2, 1, 28, 3),
    ("c1x1_L3136", "conv", 64, 40, 1, 1, 0, 56, 1),
    ("c1x1_L196", "conv", 200, 130, 1, 1, 0, 14, 3),
    ("c1x1_L49", "conv", 130, 64, 1, 1, 0, 7, 32),
    ("c1x1_s2", "conv", 24, 64, 1, 2, 0, 28, 3),
    ("c1x1_64_to_256", "conv", 64, 256, 1, 1, 0, 12, 3),       # n_in = 64 is the short side (65 with the bias)
    ("c7x7_s2_stem", "conv", 3, 64, 7, 2, 3, 64, 3),
    ("c5x5_lenet", "conv", 6, 16, 5, 1, 0, 14, 32),
    ("linear_2d", "linear", 300, 130, None, None, None, None, 32),
    ("linear_2d_one", "linear", 64, 10, None, None, None, None, 1),
    ("linear_3d", "linear", 65, 33, None, None, None, 7, 3),
]


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_pack_and_product_against_float64(gpu, case, bias):
    _, kind, cin, cout, k, s, p, H, S = case
    gen = torch.Generator().manual_seed(len(case[0]) + 7 * S)
    torch.manual_seed(1)
    if kind == "conv":
        layer = torch.nn.Conv2d(cin, cout, k, stride=s, padding=p, bias=bias)
        Ho = (H + 2 * p - k) // s + 1
        x, g = fenced((S, cin, H, H), gpu, gen), fenced((S, cout, Ho, Ho), gpu, gen)
    else:
        layer = torch.nn.Linear(cin, cout, bias=bias)
        mid = () if H is None else (H,)
        x, g = fenced((S, *mid, cin), gpu, gen), fenced((S, *mid, cout), gpu, gen)
    alpha = 3.0
    want = diag_reference(layer, x, g, alpha)
    dst = torch.full(tuple(want.shape), float("nan"), device=gpu)
    run_product(layer, x, g, alpha, dst, True)                      # `first` overwrites the NaNs
    err = rel_fro(dst, want)
    print(f"per-sample product {case[0]} bias={bias}: rel_fro {err:.3e}")
    assert err < TOL
    once = dst.clone()
    run_product(layer, x, g, alpha, dst, False)                     # accumulates: twice the value
    assert rel_fro(dst, 2 * want) < TOL
    assert torch.equal(dst, once + once)
    again = torch.full_like(dst, float("nan"))
    run_product(layer, x, g, alpha, again, True)
    assert torch.equal(again, once)                                 # bit-identical runs
    # the (rows, N, Lp) layout EFB rotates: same value within the bar (another order of the same sums is not required)
    rows = torch.full_like(dst, float("nan"))
    run_product(layer, x, g, alpha, rows, True, rows_outer=True, in_place=False)
    assert rel_fro(rows, want) < TOL


def test_destination_with_a_row_stride(gpu):
    """C may be a column block of a wider matrix (row stride above Nc)."""
    gen = torch.Generator().manual_seed(5)
    layer = torch.nn.Conv2d(16, 24, 1, bias=False)
    x, g = fenced((3, 16, 8, 8), gpu, gen), fenced((3, 24, 8, 8), gpu, gen)
    wide = torch.zeros(24, 40, device=gpu)
    run_product(layer, x, g, 1.0, wide[:, 8:24], True)
    assert rel_fro(wide[:, 8:24], diag_reference(layer, x, g, 1.0)) < TOL
    assert float(wide[:, :8].abs().max()) == 0 and float(wide[:, 24:].abs().max()) == 0


def lenet_batch(gpu, N=8):
    """LeNet-5 with `torch.manual_seed(0)` weights and inputs and labels drawn by `oracle.capture(seed=1)`."""
    import oracle.curvature_oracle as o
    from curvature_amd import models
    torch.manual_seed(0)
    model = models.lenet5().to(gpu)
    x = torch.randn(N, 1, 28, 28, device=gpu)
    _, _, labels = o.capture(model, x, seed=1)
    layers = o.selected_layers(model)
    return model, layers, x, labels


def backward(model, x, labels):
    model.zero_grad()
    torch.nn.functional.cross_entropy(model(x), labels).backward()


def test_lenet_diagonal_is_the_per_sample_fisher(gpu):
    import oracle.curvature_oracle as o
    from curvature_amd.curvatures import Diagonal
    N = 8
    model, layers, x, labels = lenet_batch(gpu, N)
    diag = Diagonal(model, per_sample=True)
    backward(model, x, labels)
    diag.update(N)
    # the existing path, one sample at a time (LeNet-5 has no BatchNorm: the two definitions agree)
    single = Diagonal(model)
    for n in range(N):
        backward(model, x[n:n + 1], labels[n:n + 1])
        single.update(1)
    backward(model, x, labels)
    for li, layer in enumerate(layers):
        fwd, bwd = diag.record[layer]
        want = diag_reference(layer, fwd, bwd, N)
        err = rel_fro(diag.state[layer], want)
        err_single = rel_fro(diag.state[layer], single.state[layer] / N)
        batch_form = o.diag_update(layer.weight.grad.double().cpu(), layer.bias.grad.double().cpu(), N)
        away = rel_fro(diag.state[layer], batch_form)
        print(f"lenet diagonal l{li}: vs float64 {err:.3e}, vs N single-sample updates {err_single:.3e}, "
              f"from the batch form {away:.3f}")
        assert err < TOL
        assert err_single < TOL
        assert away > 0.1                          # not the old formula
    # a second update accumulates
    diag.update(N)
    for layer in layers:
        assert rel_fro(diag.state[layer], 2 * diag_reference(layer, *diag.record[layer], N)) < TOL


def test_batch_size_one_agrees_with_the_existing_path(gpu):
    from curvature_amd.curvatures import EFB, KFAC, Diagonal
    from curvature_amd.utils import get_eigenvectors
    model, layers, x, labels = lenet_batch(gpu, 1)
    kfac = KFAC(model)
    backward(model, x, labels)
    kfac.update(1)
    eig = get_eigenvectors(kfac.state)
    old_d, new_d = Diagonal(model), Diagonal(model, per_sample=True)
    old_e, new_e = EFB(model, {}, eigvecs=eig), EFB(model, {}, eigvecs=eig, per_sample=True)
    backward(model, x, labels)
    for est in (old_d, new_d, old_e, new_e):
        est.update(1)
    for layer in layers:
        assert rel_fro(new_d.state[layer], old_d.state[layer]) < TOL
        assert rel_fro(new_e.state[layer], old_e.state[layer]) < TOL
        assert rel_fro(new_e.diags[layer], old_e.diags[layer]) < TOL


def efb_reference(layer, x, g, U_A, U_G, batch_size):
    import oracle.curvature_oracle as o
    return batch_size * sum(o.efb_update(U_A, U_G, *split(P, layer)) for P in per_sample_grads(layer, x, g))


def test_lenet_efb_per_sample(gpu):
    from curvature_amd.curvatures import EFB, KFAC
    from curvature_amd.utils import get_eigenvectors
    N = 8
    model, layers, x, labels = lenet_batch(gpu, N)
    kfac = KFAC(model)
    backward(model, x, labels)
    kfac.update(N)
    eig = get_eigenvectors(kfac.state)
    efb = EFB(model, {}, eigvecs=eig, per_sample=True)
    backward(model, x, labels)
    efb.update(N)
    for li, layer in enumerate(layers):
        fwd, bwd = efb.record[layer]
        U_A, U_G = (u.double().cpu() for u in eig[layer])
        err = rel_fro(efb.state[layer], efb_reference(layer, fwd, bwd, U_A, U_G, N))
        err_d = rel_fro(efb.diags[layer], diag_reference(layer, fwd, bwd, N))
        print(f"lenet efb l{li}: lambda {err:.3e}, diags {err_d:.3e}")
        assert err < TOL and err_d < TOL
    efb.update(N)                                                   # accumulates onto both
    for layer in layers:
        fwd, bwd = efb.record[layer]
        U_A, U_G = (u.double().cpu() for u in eig[layer])
        assert rel_fro(efb.state[layer], 2 * efb_reference(layer, fwd, bwd, U_A, U_G, N)) < TOL
        assert rel_fro(efb.diags[layer], 2 * diag_reference(layer, fwd, bwd, N)) < TOL


def test_chain_into_inf(gpu):
    """Diagonal(per_sample) -> KFAC -> EFB(per_sample) -> INF: shapes and the scale convention still fit INF."""
    from curvature_amd.curvatures import EFB, INF, KFAC, Diagonal
    N = 8
    model, layers, x, labels = lenet_batch(gpu, N)
    diag, kfac = Diagonal(model, per_sample=True), KFAC(model)
    backward(model, x, labels)
    diag.update(N)
    kfac.update(N)
    efb = EFB(model, kfac.state, per_sample=True)
    backward(model, x, labels)
    efb.update(N)
    inf = INF(model, diag.state, kfac.state, efb.state, eigvecs=efb.eigvecs)
    inf.update(rank=20)
    inf.invert(add=0.5, multiply=2.0)
    inf.sample_and_replace()
    for layer in layers:
        assert torch.isfinite(layer.weight).all() and torch.isfinite(layer.bias).all()
    for est in (diag, efb):
        est.invert(add=0.5, multiply=2.0)
        est.sample_and_replace()
        assert all(torch.isfinite(l.weight).all() for l in layers)


def test_alone_whole_model_and_sharded_bits(gpu):
    from curvature_amd import sharding
    from curvature_amd.curvatures import EFB, KFAC, Diagonal
    from curvature_amd.utils import get_eigenvectors
    N = 8
    model, layers, x, labels = lenet_batch(gpu, N)
    kfac = KFAC(model)
    full = Diagonal(model, per_sample=True)
    backward(model, x, labels)
    full.update(N)
    kfac.update(N)
    eig = get_eigenvectors(kfac.state)
    full_e = EFB(model, {}, eigvecs=eig, per_sample=True)
    full_e.record = full.record
    full_e.update(N)
    for layer in layers:                            # one layer built alone
        alone = Diagonal(torch.nn.Sequential(layer), per_sample=True)
        alone.record = {layer: full.record[layer]}
        alone.update(N)
        assert torch.equal(alone.state[layer], full.state[layer])
        alone_e = EFB(torch.nn.Sequential(layer), {}, eigvecs={layer: eig[layer]}, per_sample=True)
        alone_e.record = {layer: full.record[layer]}
        alone_e.update(N)
        assert torch.equal(alone_e.state[layer], full_e.state[layer])
        assert torch.equal(alone_e.diags[layer], full_e.diags[layer])
    owner = [0, 1, 0, 1, 1]
    for rank in range(2):
        part = Diagonal(model, per_sample=True, shard=sharding.Shard(owner, rank, 2))
        part.record = full.record
        part.update(N)
        part_e = EFB(model, {}, eigvecs=eig, per_sample=True, shard=sharding.Shard(owner, rank, 2))
        part_e.record = full.record
        part_e.update(N)
        mine = [l for l, r in zip(layers, owner) if r == rank]
        assert set(part.state) == set(mine) and set(part_e.state) == set(mine)
        for layer in mine:
            assert torch.equal(part.state[layer], full.state[layer])
            assert torch.equal(part_e.state[layer], full_e.state[layer])


def test_half_precision_records_raise(gpu):
    from curvature_amd.curvatures import Diagonal
    model = torch.nn.Sequential(torch.nn.Linear(8, 4)).to(gpu)
    diag = Diagonal(model, per_sample=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = model(torch.randn(4, 8, device=gpu)).float().square().mean()
    loss.backward()
    with pytest.raises(RuntimeError, match="bfloat16"):
        diag.update(4)


def resnet50_pass(gpu, N):
    from curvature_amd import models
    torch.manual_seed(0)
    model = models.resnet50().to(gpu)                       # training mode: BatchNorm uses the batch's statistics
    x = torch.randn(N, 3, 224, 224, device=gpu)
    labels = torch.randint(0, 1000, (N,), device=gpu)
    picked = {"stem": model.conv1, "layer1_3x3": model.layer1[1].conv2, "first_s2_3x3": model.layer2[0].conv2,
              "layer4_3x3": model.layer4[1].conv2, "1x1_2048_512": model.layer4[1].conv1, "fc": model.fc}
    return model, x, labels, picked


def test_resnet50_diagonal_layers(gpu):
    """ResNet-50 at N = 32, 224 x 224: the whole-model update, six layers against float64 on the CPU.  The per-sample
    quantities are those of the batch pass's records (training-mode BatchNorm couples the samples)."""
    from curvature_amd.curvatures import Diagonal
    N = 32
    model, x, labels, picked = resnet50_pass(gpu, N)
    diag = Diagonal(model, per_sample=True)
    backward(model, x, labels)
    diag.update(N)
    assert len(diag.state) == 54
    for name, layer in picked.items():
        want = diag_reference(layer, *diag.record[layer], N)
        err = rel_fro(diag.state[layer], want)
        print(f"resnet50 diagonal {name}: rel_fro {err:.3e}")
        assert err < TOL
    layer = picked["layer4_3x3"]                            # alone = in the whole-model call, bit for bit
    alone = Diagonal(torch.nn.Sequential(layer), per_sample=True)
    alone.record = {layer: diag.record[layer]}
    alone.update(N)
    assert torch.equal(alone.state[layer], diag.state[layer])


def test_resnet50_efb_layers(gpu):
    """EFB on the layer4 3x3 (4608 x 512, L = 49) and a 1x1 2048 -> 512 at N = 8; the identity holds for any orthogonal
    U_A, U_G, so they come from a QR of a seeded Gaussian.  The float64 side rotates the operands, not P_n."""
    from curvature_amd.curvatures import EFB
    N = 8
    model, x, labels, picked = resnet50_pass(gpu, N)
    gen = torch.Generator().manual_seed(3)
    eig64, eig = {}, {}
    for name in ("layer4_3x3", "1x1_2048_512"):
        layer = picked[name]
        n, m = layer.in_channels * layer.kernel_size[0] * layer.kernel_size[1], layer.out_channels
        U_A = torch.linalg.qr(torch.randn(n, n, generator=gen, dtype=torch.float64))[0].float()
        U_G = torch.linalg.qr(torch.randn(m, m, generator=gen, dtype=torch.float64))[0].float()
        eig64[layer] = (U_A.double(), U_G.double())
        eig[layer] = (U_A.to(gpu), U_G.to(gpu))
    efb = EFB(model, {}, eigvecs=eig, per_sample=True)
    backward(model, x, labels)
    efb.update(N)
    for name in ("layer4_3x3", "1x1_2048_512"):
        layer = picked[name]
        fwd, bwd = efb.record[layer]
        U_A, U_G = eig64[layer]
        want = 0
        for n in range(N):
            gn, X = sample_matrices(layer, fwd, bwd, n)
            want = want + ((U_G.t() @ gn) @ (U_A.t() @ X).t()) ** 2
        err = rel_fro(efb.state[layer], N * want)
        err_d = rel_fro(efb.diags[layer], diag_reference(layer, fwd, bwd, N))
        print(f"resnet50 efb {name}: lambda {err:.3e}, diags {err_d:.3e}")
        assert err < TOL and err_d < TOL
