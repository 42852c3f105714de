"""`ops.chol_factor_inverse` (curv_chol_factor_inverse, csrc/invert.hip: the fp64 chol(M + d I)^-1 sweep under INF and the
low-rank eigensolver) and the status words of both sweeps, against float64 torch on the CPU (chol_refs.py).

Which kernels a call reaches is decided in `chol_sweep`:
  * at most 64 matrices and no right-hand side -> the CHAIN-BOUND form: outer panels of 4 blocks (256 columns), the block
    square of a panel in one launch (chol_square_kernel), the quarter panel product, one group on one stream;
  * more than 64 matrices, or any right-hand side -> the PER-STEP form: outer panels of 6 blocks (384 columns),
    chol_diag_kernel / chol_panel_kernel / inner_update_kernel per block step, and two groups on two streams when a
    matrix has more than max(16, Pmax / 2) blocks of 64;
  * a panel has far tiles (side stream: outer_update_dma_kernel for the trailing matrix, outer_update_kernel for the S
    tiles of the fp64 inverse) once a matrix has more than 2 panels' worth of blocks: more than 8 (chain-bound), more
    than 12 (per-step).
The widths below are the block (64), 16-column-panel and outer-panel (256 / 384) edges and the first widths past those
thresholds, not a model's.  Sources sit inside NaN-filled buffers: a read past a ragged edge turns the result into NaN."""
import pytest
import torch

import chol_refs as R
from conftest import identity_residual_bound

pytestmark = pytest.mark.gpu

NAN = float("nan")
BAR = 1e-9                                # max |X - want| <= BAR max |want|: the bar tests/test_efb_inf_gpu.py holds
F64, F32 = torch.float64, torch.float32
DTYPES = [F64, F32]
DTYPE_IDS = ["f64", "f32"]
ADDS = (0.0, 1.0, 0.3, 1e-3)              # 0.0 and 1.0 are what INF passes; 0.3 and 1e-3 are not exact in float32
CHAIN_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 320, 513, 577, 1100]
STEP_SIZES = CHAIN_SIZES + [383, 384, 385, 449, 769, 833]
RHS_SIZES = [1, 2, 63, 64, 65, 257, 385, 833, 1100]
N_FILLERS = 70                            # 8 x 8 matrices that take a call past the 64 of the chain-bound form
worst = {}                                # case family -> largest ratio max |X - want| / max |want| seen


def fenced(t, gpu):
    """A contiguous GPU copy of the CPU matrix `t` in the middle of a NaN-filled flat buffer (8 NaNs on either side)."""
    buf = torch.full((t.numel() + 16,), NAN, dtype=t.dtype, device=gpu)
    view = buf[8:8 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 8 * t.element_size()
    return view


def source(n, dtype, gpu, seed=0):
    return fenced(R.well_conditioned(n, seed).to(dtype), gpu)


def fillers(dtype, gpu):
    return [source(8, dtype, gpu) for _ in range(N_FILLERS)]


def check_values(family, tag, got, want):
    """The assertions of every value case: finite, exact zeros above the diagonal, within BAR of the reference."""
    g = got.cpu()
    assert g.dtype == torch.float64 and g.shape == want.shape, tag
    assert bool(torch.isfinite(g).all()), tag
    if g.shape[0] > 1:
        assert float(torch.triu(g, 1).abs().max()) == 0.0, tag
    ratio = float((g - want).abs().max()) / float(want.abs().max())
    worst[family] = max(worst.get(family, 0.0), ratio)
    print(f"{family} {tag}: ratio {ratio:.3e} (worst of the family so far {worst[family]:.3e})")
    assert ratio <= BAR, (family, tag, ratio)


def dname(dtype):
    return "f64" if dtype == F64 else "f32"


# ================================================================================================ 1. chain-bound form
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_chain_bound_inverse_batched(gpu, dtype):
    """12 matrices, no right-hand side: at most 64, so `latency_bound` holds - 4-block outer panels, chol_square_kernel
    (runner and helpers with one to four rows: 1 .. 64 wide has one block, 65 two, 255 / 256 four, 257 starts a second
    panel), panel_product_quarter_kernel, the near strips on outer_update_wide_kernel.  513 (9 blocks) and 577 (10) are
    past 8 blocks: their first panel has far tiles on the side stream, trailing and S; 1100 (18 blocks) takes five
    panels.  This is the form `INF.pre_sampler_many` takes for a small model and every low-rank `eigh` call.
    `diag_add` cycles through 0, 1, 0.3 and 1e-3: the last two are added in float64 for float64 input, in float32
    for float32 input (chol_refs.damped)."""
    from curvature_amd import ops
    shift = 0 if dtype == F64 else 1
    adds = [ADDS[(k + shift) % 4] for k in range(len(CHAIN_SIZES))]
    got = ops.chol_factor_inverse([source(n, dtype, gpu) for n in CHAIN_SIZES], adds)
    for n, d, X in zip(CHAIN_SIZES, adds, got):
        check_values("chain-bound", f"{dname(dtype)} n {n} d {d}", X, R.inverse_of(n, dtype, d))


@pytest.mark.parametrize("n", [65, 577, 1100])
def test_chain_bound_inverse_alone(gpu, n):
    """One matrix per call (a single factor of a layer-sharded rank): the same chain-bound kernels with nothing beside
    them in the launch - every `locate` scan sees one row.  Two blocks, ten (far tiles), eighteen (five panels)."""
    from curvature_amd import ops
    for dtype, d in ((F64, 0.3), (F32, 0.3), (F64, 0.0), (F32, 1e-3)):
        X, = ops.chol_factor_inverse([source(n, dtype, gpu)], [d])
        check_values("chain-bound alone", f"{dname(dtype)} n {n} d {d}", X, R.inverse_of(n, dtype, d))


# ================================================================================================ 2. per-step form
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_per_step_inverse_in_two_groups(gpu, dtype):
    """18 matrices and 70 fillers: more than 64, so the per-step kernels run (chol_diag_kernel, chol_panel_kernel,
    inner_update_kernel, panel_product(_wide)_kernel, outer_update(_wide)_kernel) on 6-block outer panels - 383 / 384 /
    385 are the panel edge, 449 ends inside the second panel.  769 (13 blocks) and 833 (14) are past 12 blocks: far tiles
    on the side stream.  1100 has 18 blocks, more than max(SPLIT_P, Pmax / 2) = 16: it is swept alone as the large
    group on one stream, the other 87 matrices as the small group on another - the two-group form of a whole model."""
    from curvature_amd import ops
    shift = 2 if dtype == F64 else 3
    adds = [ADDS[(k + shift) % 4] for k in range(len(STEP_SIZES))] + [1.0] * N_FILLERS
    got = ops.chol_factor_inverse([source(n, dtype, gpu) for n in STEP_SIZES] + fillers(dtype, gpu), adds)
    for n, d, X in zip(STEP_SIZES + [8] * N_FILLERS, adds, got):
        check_values("per-step", f"{dname(dtype)} n {n} d {d}", X, R.inverse_of(n, dtype, d))


# ================================================================================================ 3. right-hand sides
@pytest.mark.parametrize("minus", [False, True], ids=["solve", "rhs_minus"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_right_hand_side_forms(gpu, dtype, minus):
    """X = C^-1 R and, with `rhs_minus`, X = R - C^-1 R (inv_finalize_kernel's subtraction).  A right-hand side anywhere
    in the call switches `latency_bound` off: per-step kernels and 6-block panels although there are only 21 entries;
    the work matrix Zm starts as R (inv_prepare_kernel) and takes the place of the inverse in the panel product and
    the S tiles.  1100 goes to the large group again.  Three entries without a right-hand side (plain inverses) sit in
    the same call.  Every width with d = 0 and d = 0.3."""
    from curvature_amd import ops
    mats, adds, rhs, want, tags = [], [], [], [], []
    for n in RHS_SIZES:
        Rn = R.lower_rhs(n)
        for d in (0.0, 0.3):
            mats.append(source(n, dtype, gpu))
            adds.append(d)
            rhs.append(fenced(Rn, gpu))
            Z = R.solve_lower(R.factor_of(n, dtype, d), Rn)
            want.append(Rn - Z if minus else Z)
            tags.append(f"{dname(dtype)} n {n} d {d} rhs")
        if n in (2, 65, 385):
            mats.append(source(n, dtype, gpu))
            adds.append(0.3)
            rhs.append(None)
            want.append(R.inverse_of(n, dtype, 0.3))
            tags.append(f"{dname(dtype)} n {n} d 0.3 plain")
    got = ops.chol_factor_inverse(mats, adds, rhs=rhs, rhs_minus=minus)
    for tag, X, w in zip(tags, got, want):
        check_values("rhs_minus" if minus else "rhs", tag, X, w)


def test_right_hand_side_from_an_earlier_call(gpu):
    """R is the result of an earlier call, as in `INF.pre_sampler_many`: X2 = chol(M + 0.3 I)^-1 chol(M)^-1.  The second
    call reads the first one's output as it lies on the device (lower triangle, exact zeros above)."""
    from curvature_amd import ops
    sizes = [65, 385, 1100]
    mats = [source(n, F64, gpu) for n in sizes]
    first = ops.chol_factor_inverse(mats, [0.0] * len(sizes))
    second = ops.chol_factor_inverse(mats, [0.3] * len(sizes), rhs=first)
    for n, X in zip(sizes, second):
        want = R.solve_lower(R.factor_of(n, F64, 0.3), R.inverse_of(n, F64, 0.0))
        check_values("rhs", f"f64 n {n} chained", X, want)


# ================================================================================================ 4. INF's two shapes
def test_both_call_shapes_of_inf_give_the_same_t(gpu):
    """T = A^-1 - B^-1 A^-1 with A = chol(v), B = chol(v + I), the two ways `INF.pre_sampler_many` forms it.  Few layers:
    ONE chain-bound call with mats = [v, v, ...], adds = [0, 1, ...] (both inverses explicit, the product formed here
    in float64 torch).  More than RHS_SWEEP_ABOVE layers: invA = f(v, 0), then T = f(v, 1, rhs=invA, rhs_minus=True) -
    two per-step calls, no explicit B^-1.  v is float64 as INF's V^T V is; widths of 2, 5 and 10 blocks."""
    from curvature_amd import ops
    sizes = [65, 257, 577]
    vs = [source(n, F64, gpu) for n in sizes]
    want = []
    for n in sizes:
        invA = R.inverse_of(n, F64, 0.0)
        want.append(invA - R.solve_lower(R.factor_of(n, F64, 1.0), invA))
    mats, adds = [], []
    for v in vs:
        mats += [v, v]
        adds += [0.0, 1.0]
    both = ops.chol_factor_inverse(mats, adds)
    for i, n in enumerate(sizes):
        invA, invB = both[2 * i].cpu(), both[2 * i + 1].cpu()
        check_values("INF shapes", f"n {n} chain-bound invA", both[2 * i], R.inverse_of(n, F64, 0.0))
        check_values("INF shapes", f"n {n} chain-bound invB", both[2 * i + 1], R.inverse_of(n, F64, 1.0))
        check_values("INF shapes", f"n {n} chain-bound T", (invA - invB @ invA).to(gpu), want[i])
    invA = ops.chol_factor_inverse(vs, [0.0] * len(vs))
    Ts = ops.chol_factor_inverse(vs, [1.0] * len(vs), rhs=invA, rhs_minus=True)
    for n, T, w in zip(sizes, Ts, want):
        check_values("INF shapes", f"n {n} rhs sweep T", T, w)


# ================================================================================================ 5. status words
def status_case(kind, dtype):
    """(failing matrices, positive-definite stand-ins of the same sizes, expected words, diag_add, pivot_min) on the CPU."""
    bad, good, words = [], [], []
    if kind == "pivot_min":
        for n, r in R.PIVOT_CASES:
            bad.append(R.prescribed_pivots(n, (r,)).to(dtype))
            good.append(R.prescribed_pivots(n).to(dtype))
            words.append(r + 1)
        for n, planted in R.DOUBLE_CASES:
            bad.append(R.prescribed_pivots(n, planted).to(dtype))
            good.append(R.prescribed_pivots(n).to(dtype))
            words.append(min(planted) + 1)
        return bad, good, words, 0.0, R.PIVOT_MIN
    for n, r in R.PIVOT_CASES:
        bad.append(R.not_pd(n, r).to(dtype))
        good.append(R.well_conditioned(n).to(dtype))
        words.append(R.failing_word(R.damped(bad[-1], 0.3)))
        assert words[-1] == r + 1
    return bad, good, words, 0.3, 0.0


@pytest.mark.parametrize("with_fillers", [False, True], ids=["chain-bound", "per-step"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kind", ["pivot_min", "not_pd"])
def test_status_words_of_chol_factor_inverse(gpu, kind, dtype, with_fillers):
    """The word is 1 + the index of the first failing pivot.  factor_invert_64 finds it once per 16-column panel
    (ballot, first set bit, pivot_base + c0) and keeps the first one across panels, 64-blocks and launches: the
    planted columns are the first and last of a 16-column panel (0, 15, 16), of a 64-block (63, 64), of a 256 / 384
    outer panel (255, 256, 257, 383, 384) and the last column (449).  `pivot_min`: a pivot of 1e-6 against a threshold
    of 1e-3, every other pivot >= 1 (expected word r + 1; test_chol_refs_cpu.py has the margins); two matrices carry
    two planted columns - 70 and 20: expected 21, the first failure wins across 64-blocks; 3 and 9: expected 4, inside
    one panel.  `not_pd`: 5 subtracted from M[r, r], expected word from torch.linalg.cholesky_ex.  Without fillers the
    words come from chol_square_kernel's runner, with 70 fillers from chol_diag_kernel and inner_update_kernel.
    Three good matrices in the call return 0, and their outputs are bit-identical to a call of the same geometry in
    which every failing matrix is replaced by a positive-definite one: a failed neighbour changes nothing."""
    from curvature_amd import ops
    bad, good, words, add, pivot_min = status_case(kind, dtype)
    bystanders = [R.well_conditioned(n).to(dtype) for n in (70, 300, 450)]
    extra = [R.well_conditioned(8).to(dtype)] * (N_FILLERS if with_fillers else 0)
    count = len(bad) + len(bystanders) + len(extra)
    adds, pivot_mins = [add] * count, [pivot_min] * count

    def run(first):
        mats = [fenced(m, gpu) for m in first + bystanders + extra]
        outs = ops.chol_factor_inverse(mats, adds, check=False, pivot_mins=pivot_mins)
        return outs, ops.chol_factor_inverse.last_info.cpu().tolist()

    outs_bad, info_bad = run(bad)
    outs_good, info_good = run(good)
    print(f"{kind} {dname(dtype)} {'per-step' if with_fillers else 'chain-bound'}: words {info_bad[:len(bad)]}")
    assert info_bad[:len(bad)] == words
    assert info_bad[len(bad):] == [0] * (count - len(bad))
    assert info_good == [0] * count
    for k in range(len(bad), count):
        assert torch.equal(outs_bad[k].cpu().view(torch.int64), outs_good[k].cpu().view(torch.int64)), k
    for m, X in zip(bystanders, outs_bad[len(bad):]):
        check_values("status bystanders", f"{kind} {dname(dtype)} n {m.shape[0]}", X, R.chol_inverse(R.damped(m, add))[1])


# ================================================================================================ 6. chol_inv_lower
REVERSED_AT = [0, 15, 16, 63, 64, 255, 256, 383, 384, 449]      # index of the failing pivot in the sweep's order, n = 450


@pytest.mark.parametrize("with_fillers", [False, True], ids=["chain-bound", "per-step"])
def test_status_words_of_chol_inv_lower(gpu, with_fillers):
    """`chol_inv_lower(check=False).info`: the sweep factorises the index-reversed damped factor J (.) J, so the word
    counts pivots in THAT order - a failure planted at row n - 1 - q of F is reported as q + 1.  Expected word:
    torch.linalg.cholesky_ex of the reversed matrix, damped in float32 and promoted (chol_refs.damped_reversed).
    Failures at sweep index 0, 15, 16, 63, 64, 255, 256, 383, 384 and n - 1 of 450-wide factors, and at 0, 63, 64, 69 of
    70-wide ones; two good factors return 0.  At most 64 factors: chol_square_kernel; with 70 fillers the per-step
    kernels.  Both with the fp32 inverse off the chain (supd32_kernel, xrows32_kernel), as in KFAC.invert."""
    from curvature_amd import ops
    add, mul = 0.25, 1.0
    cases = [(450, q) for q in REVERSED_AT] + [(70, q) for q in (0, 63, 64, 69)]
    factors = [R.not_pd(n, n - 1 - q).float() for n, q in cases] + [R.well_conditioned(n).float() for n in (70, 450)]
    factors += [R.well_conditioned(8).float()] * (N_FILLERS if with_fillers else 0)
    words = [R.failing_word(R.damped_reversed(F, add, mul)) for F in factors]
    assert words[:len(cases)] == [q + 1 for _, q in cases] and not any(words[len(cases):])
    outs = ops.chol_inv_lower([fenced(F, gpu) for F in factors], [add] * len(factors), [mul] * len(factors), check=False)
    got = outs.info.cpu().tolist()
    print(f"chol_inv_lower {'per-step' if with_fillers else 'chain-bound'}: words {got[:len(cases)]}")
    assert got == words
    for F, L in zip(factors[len(cases):len(cases) + 2], outs[len(cases):]):
        # the good factors beside them: L L^T is the inverse of the damped factor, to the bar of the invert tests
        A = torch.flip(R.damped_reversed(F, add, mul), (0, 1))
        Ld = L.cpu().double()
        assert float(torch.triu(Ld, 1).abs().max()) == 0.0
        resid = Ld @ Ld.t() @ A - torch.eye(A.shape[0], dtype=torch.float64)
        assert float(torch.linalg.norm(resid)) / A.shape[0] ** 0.5 < identity_residual_bound(A)
