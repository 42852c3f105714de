"""Kronecker factors whose fp32 matrix exceeds 2 GiB, through update(), invert() and sample().

The model is VGG-16's fc6, Linear(25088, 4096, bias=True), at N = 32: its A factor is 25089 wide (2.52 GB in fp32,
5.04 GB as the fp64 work matrix of the Cholesky sweep, 2^32 bytes and more).  Linear(20000, 64) puts A (np = 20032) in
the band where 32-bit signed byte offsets into the work matrix overflow (16384 <= np < 23171) but unsigned ones do not.
Every reference is computed in fp64 with plain torch on the GPU (conftest.rel_fro copies to the host: too slow here).

Device memory (estimate for the 25089-wide case, not measured): the factor 2.5 GB and its fp64 reference 5 GB; the
sweep's workspace 28 np^2 bytes = 17.7 GB (np = 25152), cached at up to 1.25x; the inverse factor 2.5 GB; the residual
check about 20 GB (M, L, M L and L^T M L in fp64).  About 56 GB at the peak: less free memory skips with that reason."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4
PEAK_BYTES = 56e9
HYPER = [(0.5, 1.0), (1.0, 1000.0)]          # (add, multiply): smoke()'s, and bench.py's large multiply


def rel_fro_gpu(a, ref):
    """||a - ref||_F / ||ref||_F in fp64, on the device."""
    return float(torch.linalg.norm(a.double() - ref) / torch.linalg.norm(ref))


def damped(F, add, mul):
    """M = sqrt(s) F + sqrt(n) I as the sweep damps it (fp32, symmetrised: tests/test_invert_gpu.py damp32_then_64),
    promoted to fp64, on the device."""
    reg = torch.tensor(mul ** 0.5, dtype=torch.float32, device=F.device) * F
    reg.diagonal().add_(torch.tensor(add ** 0.5, dtype=torch.float32))
    out = reg.double()
    del reg
    out.add_(out.t().clone()).mul_(0.5)
    return out


def lambda_max(M, steps=50):
    """Rayleigh quotient after `steps` power iterations (eigvalsh at this size takes minutes)."""
    gen = torch.Generator(device=M.device).manual_seed(0)
    v = torch.randn(M.shape[0], dtype=torch.float64, device=M.device, generator=gen)
    v /= torch.linalg.norm(v)
    for _ in range(steps):
        w = M @ v
        v = w / torch.linalg.norm(w)
    return float(v @ (M @ v))


def check_inverse(L, F, add, mul):
    """L lower triangular, finite, positive diagonal, and L^T M L = I up to what fp32 delivery allows
    (conftest.identity_residual_bound; lambda_min >= sqrt(add) from the damping of a positive semi-definite F)."""
    n = F.shape[0]
    assert torch.isfinite(L).all()
    assert not torch.triu(L, 1).any()
    assert bool((L.diagonal() > 0).all())
    M = damped(F, add, mul)
    cond = 1.1 * lambda_max(M) / add ** 0.5                      # (10 % above what the power iteration found)
    L64 = L.double()
    R = L64.t() @ (M @ L64)
    del M, L64
    R.diagonal().sub_(1.0)
    res = float(torch.linalg.norm(R)) / n ** 0.5
    del R
    bound = max(1e-4, 6e-8 * cond)
    assert res < bound, (n, add, mul, res, bound)


@pytest.mark.parametrize("cin,cout", [(25088, 4096), (20000, 64)], ids=["vgg16_fc6", "np20032"])
def test_wide_linear_update_invert_sample(gpu, cin, cout):
    from curvature_amd.curvatures import KFAC
    free, _ = torch.cuda.mem_get_info(gpu)
    if free < PEAK_BYTES:
        pytest.skip(f"needs about {PEAK_BYTES / 1e9:.0f} GB of free device memory, {free / 1e9:.1f} GB free")
    N = 32
    torch.manual_seed(0)
    layer = torch.nn.Linear(cin, cout, bias=True).to(gpu)
    kfac = KFAC(torch.nn.Sequential(layer))
    x = torch.randn(N, cin, device=gpu)
    g = torch.randn(N, cout, device=gpu) / N
    kfac.record[layer] = [x, g]

    # ---- update: first=True, then accumulated
    X1 = torch.cat([x.double(), torch.ones(N, 1, dtype=torch.float64, device=gpu)], 1)
    A_ref = X1.t() @ X1 / N
    del X1
    G_ref = (g.double().t() @ g.double()) * N
    for rounds in (1, 2):
        kfac.update(batch_size=N)
        torch.cuda.synchronize()
        A, G = kfac.state[layer]
        assert A.shape == (cin + 1, cin + 1) and G.shape == (cout, cout)
        for F, ref in ((A, A_ref), (G, G_ref)):
            assert torch.isfinite(F).all()
            assert torch.equal(F, F.t())
            err = rel_fro_gpu(F, rounds * ref)
            assert err < TOL, (rounds, F.shape[0], err)
    del A_ref, G_ref
    # the factors are now 2 X^T X / N: one sample's worth of curvature, twice
    A, G = kfac.state[layer]

    # ---- invert (A and G in one sweep, as invert() batches them)
    for add, mul in HYPER:
        kfac.invert(add=add, multiply=mul)
        torch.cuda.synchronize()
        LA, LG = kfac.inv_state[layer]
        check_inverse(LA, A, add, mul)
        check_inverse(LG, G, add, mul)

    # ---- sample with a fixed z, against (L_A z L_G^T)^T from the L's the library returned
    LA, LG = kfac.inv_state[layer]
    z = torch.randn(cin + 1, cout, device=gpu, generator=torch.Generator(device=gpu).manual_seed(5))
    out = kfac.sample(layer, z)
    torch.cuda.synchronize()
    assert out.shape == (cout, cin + 1) and torch.isfinite(out).all()
    ref = (LA.double() @ z.double() @ LG.double().t()).t()
    err = rel_fro_gpu(out, ref)
    assert err < TOL, err
