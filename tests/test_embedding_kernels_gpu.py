"""The kernels of csrc/embedding_factor.hip through `ops`: the token histogram (`torch.equal` to
``scale * count``: integer counts, power-of-two scales) and the two modes of the segment walker against float64 computed on
the CPU from the very records (rel_fro < 1e-4, conftest.rel_fro), bit for bit on integer-valued records
(tests/exact_inputs.py), bit-reproducible on real-valued ones, with padding, `first=False`, `alpha`, both forms of `w`,
records read through strides, NaN fences behind every record and a NaN-filled workspace; and the descriptors the host
refuses.  No test feeds an index outside [0, V): the forward pass rejects those, and the kernels' checks are read."""
import pytest
import torch

from conftest import rel_fro
from curvature_amd import _lib, ops
from exact_inputs import EXACT_LIMIT, assert_exact_range, nonzero_ints

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(autouse=True)
def admitted():
    was = ops.admit_embedding(True)
    yield
    ops.admit_embedding(was)


# ------------------------------------------------------------------------------------------------ histogram
def _tokens(name):
    gen = torch.Generator().manual_seed(11)
    if name == "small":
        return torch.randint(0, 7, (3, 5), generator=gen), 7
    if name == "wide":                   # wider than a wave, a multi-dimensional index
        return torch.randint(0, 70, (2, 3, 4), generator=gen), 70
    if name == "sparse":                 # crosses a workgroup; most of the 1025 bins stay empty
        return torch.randint(0, 40, (4, 1025), generator=gen) * 25, 1025
    if name == "same":                   # every lane of every wave on one bin
        return torch.full((3, 50), 4), 7
    raise KeyError(name)


def _histogram(idx, V, dev, pad=None, scale=1.0, first=True, start=None):
    dst = torch.full((V,), float("nan"), device=dev) if start is None else start.clone().to(dev)
    ops.workspace(1 << 20, dev, "kfac_embedding").fill_(0xFF)             # the counts start from garbage
    ops.kfac_accumulate_embedding([ops.EmbeddingFactorJob(idx.to(dev), dst, V, pad, scale=scale, first=first)])
    return dst.cpu()


def _counts(idx, V, pad=None):
    count = torch.bincount(idx.reshape(-1).long(), minlength=V).float()
    if pad is not None:
        count[pad] = 0
    return count


@pytest.mark.parametrize("name", ["small", "wide", "sparse", "same"])
def test_histogram_is_the_scaled_count(gpu, name):
    idx, V = _tokens(name)
    if name == "sparse":
        assert idx.numel() == 4100 and V == 1025
    for scale in (1.0, 2.0 ** -5):
        assert torch.equal(_histogram(idx, V, gpu, scale=scale), scale * _counts(idx, V))


def test_histogram_int32_indices(gpu):
    idx, V = _tokens("wide")
    assert torch.equal(_histogram(idx.int(), V, gpu, scale=0.25), 0.25 * _counts(idx, V))


def test_histogram_accumulates(gpu):
    idx, V = _tokens("small")
    start = torch.arange(V, dtype=torch.float32)
    assert torch.equal(_histogram(idx, V, gpu, scale=0.5, first=False, start=start), start + 0.5 * _counts(idx, V))


@pytest.mark.parametrize("pad", [0, 6])
def test_histogram_padding_row_counts_nothing(gpu, pad):
    idx, V = _tokens("small")
    idx[0, :2] = pad
    assert pad == 0 or pad == V - 1
    got = _histogram(idx, V, gpu, pad=pad)
    assert torch.equal(got, _counts(idx, V, pad)) and got[pad] == 0
    start = torch.ones(V)
    assert torch.equal(_histogram(idx, V, gpu, pad=pad, first=False, start=start), 1 + _counts(idx, V, pad))


# ------------------------------------------------------------------------------------------------ the segment walker
# name -> (N, T, V, D) and how the tokens are drawn.  The smallest shapes at which each path can go wrong.
SHAPES = {
    "base": (3, 5, 7, 6),                # a token repeated inside a sample and shared across samples (fixed below)
    "d70": (3, 5, 7, 70),                # D not a multiple of a wave
    "d129": (2, 4, 5, 129),              # ... nor of a vector
    "d300": (2, 4, 5, 300),              # two waves per group
    "t1": (4, 1, 5, 6),
    "n1": (1, 6, 5, 6),
    "one_segment": (1, 130, 3, 8),       # one sample, every position on one token: the segment is the sample
    "everywhere": (4, 5, 7, 6),          # one token present in every sample
    "split_token": (3, 100, 4, 10),      # 300 positions on one token: its list is split, segments straddle the cuts
    "split_sample": (2, 300, 3, 10),     # samples of 300 positions: both modes split, several segments per chunk
}


def _case(name, dev=None, ints=False):
    N, T, V, D = SHAPES[name]
    gen = torch.Generator().manual_seed(sorted(SHAPES).index(name))
    idx = torch.randint(0, V, (N, T), generator=gen)
    if name == "base":
        idx = torch.tensor([[1, 3, 1, 6, 1], [3, 3, 0, 2, 5], [6, 1, 4, 4, 2]])
    elif name in ("one_segment", "split_token"):
        idx = torch.full((N, T), 1)
    elif name == "everywhere":
        idx[:, 2] = 3
    g = nonzero_ints((N, T, D), gen) if ints else torch.randn(N, T, D, generator=gen)
    return idx, g, V


def test_split_cases_cross_the_list_split_length():
    """The cases named for it are past `_lib.EMB_SPLIT_L` - and the others below it - in the mode that groups them."""
    L = _lib.EMB_SPLIT_L
    assert 130 > L and 3 * 100 > L and 300 > L
    for name in SHAPES:
        idx, _, V = _case(name)
        plans = {mode: ops.embedding_walk_plan(idx, V, None, mode) for mode in (_lib.EMB_SQ, _lib.EMB_QUAD)}
        split = {mode: plan.mgroups.shape[0] > 0 for mode, plan in plans.items()}
        want = {"one_segment": (True, True), "split_token": (True, False), "split_sample": (True, True)}.get(name, (False, False))
        assert (split[_lib.EMB_SQ], split[_lib.EMB_QUAD]) == want, name


def _products64(idx, g, V, pad=None):
    """P (N, V, D) in float64: row v of sample n is the sum of the rows of g[n] at the positions that hold v."""
    N, D = g.shape[0], g.shape[-1]
    idx, g = idx.reshape(N, -1).long().cpu(), g.detach().double().cpu().reshape(N, -1, D)
    P = torch.zeros(N, V, D, dtype=torch.float64)
    for n in range(N):
        P[n].index_add_(0, idx[n], g[n])
    if pad is not None:
        P[:, pad] = 0
    return P


def _sq(idx, g, V, dev, pad=None, alpha=1.0, start=None):
    D = g.shape[-1]
    dst = torch.full((V, D), float("nan"), device=dev) if start is None else start.clone().to(dev)
    ops.per_sample_embedding_sq_accumulate([ops.PerSampleEmbeddingJob(idx, g, V, pad, dst=dst, alpha=alpha, first=start is None)])
    return dst


def _quad(idx, g, V, dev, w=None, pad=None, alpha=1.0, start=None):
    out = torch.full((g.shape[0],), float("nan"), device=dev) if start is None else start.clone().to(dev)
    ops.per_sample_embedding_quad_reduce([ops.PerSampleEmbeddingJob(idx, g, V, pad, out=out, w=w, alpha=alpha,
                                                                    first=start is None)])
    return out


def _quad64(P, w=None):
    if w is None:
        return P.square().sum((1, 2))
    w = w.detach().double().cpu()
    return (P.square() * (w if w.dim() == 2 else w.view(-1, 1))).sum((1, 2))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_sq_and_quad_against_float64(gpu, name):
    idx, g, V = _case(name)
    P = _products64(idx, g, V)
    gen = torch.Generator().manual_seed(5)
    w = torch.rand(V, g.shape[-1], generator=gen) + 0.5
    assert rel_fro(_sq(idx.to(gpu), g.to(gpu), V, gpu), P.square().sum(0)) < TOL
    assert rel_fro(_quad(idx.to(gpu), g.to(gpu), V, gpu, w=w.to(gpu)), _quad64(P, w)) < TOL


@pytest.mark.parametrize("name", ["base", "d129", "split_sample"])
def test_w_forms_alpha_and_accumulation(gpu, name):
    idx, g, V = _case(name)
    N, D = g.shape[0], g.shape[-1]
    P = _products64(idx, g, V)
    gen = torch.Generator().manual_seed(6)
    w_matrix, w_vector = torch.rand(V, D, generator=gen) + 0.5, torch.rand(V, generator=gen) + 0.5
    i, gg = idx.to(gpu), g.to(gpu)
    assert rel_fro(_quad(i, gg, V, gpu), _quad64(P)) < TOL                                            # no w: ones
    assert rel_fro(_quad(i, gg, V, gpu, w=w_vector.to(gpu)), _quad64(P, w_vector)) < TOL
    assert rel_fro(_quad(i, gg, V, gpu, w=w_matrix.to(gpu), alpha=0.3), 0.3 * _quad64(P, w_matrix)) < TOL
    assert rel_fro(_sq(i, gg, V, gpu, alpha=1.7), 1.7 * P.square().sum(0)) < TOL
    start_q, start_s = torch.rand(N, generator=gen), torch.rand(V, D, generator=gen)
    assert rel_fro(_quad(i, gg, V, gpu, w=w_matrix.to(gpu), start=start_q), start_q.double() + _quad64(P, w_matrix)) < TOL
    assert rel_fro(_sq(i, gg, V, gpu, alpha=0.5, start=start_s), start_s.double() + 0.5 * P.square().sum(0)) < TOL


@pytest.mark.parametrize("name,pad", [("base", 1), ("split_sample", 0), ("d70", 6)])
def test_padding_positions_are_skipped(gpu, name, pad):
    idx, g, V = _case(name)
    assert bool((idx == pad).any())
    P = _products64(idx, g, V, pad)
    w = torch.rand(V, generator=torch.Generator().manual_seed(7)) + 0.5
    got = _sq(idx.to(gpu), g.to(gpu), V, gpu, pad=pad)
    assert rel_fro(got, P.square().sum(0)) < TOL and bool((got[pad] == 0).all())
    assert rel_fro(_quad(idx.to(gpu), g.to(gpu), V, gpu, w=w.to(gpu), pad=pad), _quad64(P, w)) < TOL


def test_all_padding_gives_zeros(gpu):
    idx, g, V = torch.zeros(2, 3, dtype=torch.int64), torch.randn(2, 3, 5), 4
    assert bool((_sq(idx.to(gpu), g.to(gpu), V, gpu, pad=0) == 0).all())
    assert bool((_quad(idx.to(gpu), g.to(gpu), V, gpu, pad=0) == 0).all())


@pytest.mark.parametrize("name", ["base", "d70"])
def test_transposed_record_and_int32_indices(gpu, name):
    """grad_output as the transposed view of a (T, N, D) tensor, read through its strides; int32 and non-contiguous indices."""
    idx, g, V = _case(name)
    P = _products64(idx, g, V)
    view = g.transpose(0, 1).contiguous().to(gpu).transpose(0, 1)
    assert not view.is_contiguous() and tuple(view.shape) == tuple(g.shape)
    assert rel_fro(_sq(idx.to(gpu), view, V, gpu), P.square().sum(0)) < TOL
    assert rel_fro(_quad(idx.int().to(gpu), view, V, gpu), _quad64(P)) < TOL
    strided = idx.t().contiguous().to(gpu).t()
    assert not strided.is_contiguous()
    assert rel_fro(_sq(strided, g.to(gpu), V, gpu), P.square().sum(0)) < TOL


def _fenced(t, dev, fill=float("nan")):
    """`t` as a view that ends right before `fill`-filled memory (and starts right behind some)."""
    buf = torch.full((t.numel() + 128,), fill, dtype=t.dtype, device=dev)
    view = buf[64:64 + t.numel()].view(t.shape)
    view.copy_(t)
    return view


@pytest.mark.parametrize("name", ["base", "d129", "one_segment", "split_sample"])
def test_nan_fences_and_poisoned_workspace(gpu, name):
    """A read past the end of a record, or of workspace the kernels have not written, shows as a NaN in the result."""
    idx, g, V = _case(name)
    N, D = g.shape[0], g.shape[-1]
    P = _products64(idx, g, V)
    w = torch.rand(V, D, generator=torch.Generator().manual_seed(8)) + 0.5
    i, gg, ww = _fenced(idx, gpu, fill=-7), _fenced(g, gpu), _fenced(w, gpu)
    dst, out = _fenced(torch.zeros(V, D), gpu), _fenced(torch.zeros(N), gpu)
    for mode in ("sq", "quad"):
        ops.workspace(1 << 20, gpu, "persample_embedding").fill_(0xFF)
        if mode == "sq":
            ops.per_sample_embedding_sq_accumulate([ops.PerSampleEmbeddingJob(i, gg, V, dst=dst, first=True)])
            assert bool(torch.isfinite(dst).all()) and rel_fro(dst, P.square().sum(0)) < TOL
        else:
            ops.per_sample_embedding_quad_reduce([ops.PerSampleEmbeddingJob(i, gg, V, out=out, w=ww, first=True)])
            assert bool(torch.isfinite(out).all()) and rel_fro(out, _quad64(P, w)) < TOL
    for t in (gg, ww, dst, out):                            # the fences stand
        buf = torch.empty(0, device=gpu).set_(t.untyped_storage(), 0, (t.numel() + 128,))
        assert bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[64 + t.numel():]).all())


@pytest.mark.parametrize("name", ["base", "d129", "one_segment", "everywhere", "split_token", "split_sample"])
def test_exact_on_integer_records(gpu, name):
    """Integer-valued g: every segment sum is an integer of magnitude at most 3 T, the squares summed over the samples (sq)
    or over tokens and columns (quad) stay below 2^24, so float32 has one right answer in any order."""
    idx, g, V = _case(name, ints=True)
    N, T, _, D = SHAPES[name]
    assert_exact_range(3 * T, N, rounds=1)                     # N (3 T)^2 < 2^24
    P = _products64(idx, g, V)
    assert float(P.square().sum((1, 2)).max()) * 4 < EXACT_LIMIT    # the quad sums of this case, times alpha = 4
    for alpha in (1.0, 0.25):
        assert torch.equal(_sq(idx.to(gpu), g.to(gpu), V, gpu, alpha=alpha).double().cpu(), alpha * P.square().sum(0))
    w = torch.full((V,), 2.0)
    assert torch.equal(_quad(idx.to(gpu), g.to(gpu), V, gpu, alpha=2.0).double().cpu(), 2.0 * _quad64(P))
    assert torch.equal(_quad(idx.to(gpu), g.to(gpu), V, gpu, w=w.to(gpu), alpha=2.0).double().cpu(), 2.0 * _quad64(P, w))


@pytest.mark.parametrize("name", ["d70", "split_sample"])
def test_two_calls_give_the_same_bits(gpu, name):
    idx, g, V = _case(name)
    w = torch.rand(V, g.shape[-1], generator=torch.Generator().manual_seed(9)).to(gpu)
    i, gg = idx.to(gpu), g.to(gpu)
    assert torch.equal(_sq(i, gg, V, gpu), _sq(i, gg, V, gpu))
    assert torch.equal(_quad(i, gg, V, gpu, w=w), _quad(i, gg, V, gpu, w=w))
    assert torch.equal(_histogram(idx, V, gpu, scale=0.5), _histogram(idx, V, gpu, scale=0.5))


# ------------------------------------------------------------------------------------------------ what the host refuses
def test_invalid_descriptors_raise_on_the_host(gpu):
    idx, g, V = _case("base")
    i, gg = idx.to(gpu), g.to(gpu)
    N, D = g.shape[0], g.shape[-1]
    dst, out = torch.zeros(V, D, device=gpu), torch.zeros(N, device=gpu)
    sq, quad = ops.per_sample_embedding_sq_accumulate, ops.per_sample_embedding_quad_reduce
    Job = ops.PerSampleEmbeddingJob
    bad = [
        lambda: sq([Job(i, gg.double(), V, dst=dst)]),                                # records must be float32
        lambda: sq([Job(i, gg.bfloat16(), V, dst=dst)]),
        lambda: sq([Job(i.float(), gg, V, dst=dst)]),                                 # indices int64 / int32
        lambda: sq([Job(i, gg, V, dst=torch.zeros(V, D + 1, device=gpu))]),           # destination of the wrong shape
        lambda: sq([Job(i, gg, V, dst=dst.double())]),
        lambda: sq([Job(i, gg, V, dst=None)]),
        lambda: sq([Job(i, gg[:, :, :0], V, dst=dst[:, :0])]),                        # D = 0
        lambda: sq([Job(i, gg, 0, dst=dst[:0])]),                                     # V = 0
        lambda: sq([Job(i[:, :4], gg, V, dst=dst)]),                                  # records that do not match
        lambda: sq([Job(i.cpu(), gg, V, dst=dst)]),                                   # no CPU fallback
        lambda: quad([Job(i, gg, V, out=torch.zeros(N + 1, device=gpu))]),
        lambda: quad([Job(i, gg, V, out=out, w=torch.zeros(V + 1, device=gpu))]),
        lambda: quad([Job(i, gg, V, out=out, w=torch.zeros(V, D, device=gpu).double())]),
        lambda: ops.kfac_accumulate_embedding([ops.EmbeddingFactorJob(i.float(), torch.zeros(V, device=gpu), V)]),
        lambda: ops.kfac_accumulate_embedding([ops.EmbeddingFactorJob(i, torch.zeros(V + 1, device=gpu), V)]),
        lambda: ops.kfac_accumulate_embedding([ops.EmbeddingFactorJob(i, torch.zeros(V, device=gpu).double(), V)]),
        lambda: ops.kfac_accumulate_embedding([ops.EmbeddingFactorJob(i, torch.zeros(0, device=gpu), 0)]),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"descriptor {k} was accepted")
    with pytest.raises(RuntimeError, match="float32"):
        sq([Job(i, gg.half(), V, dst=dst)])
