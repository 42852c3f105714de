"""The input generators of tests/chol_refs.py against the float64 reference alone (no GPU, no library): the condition
number of the well-conditioned matrices, and the distance of every Cholesky pivot of the planted matrices from the
threshold they are run with - for the float64 matrices and for their float32 roundings."""
import pytest
import torch

import chol_refs as R

# every width tests/test_chol_factor_inverse_gpu.py asks `well_conditioned` for
WIDTHS = [1, 2, 8, 63, 64, 65, 70, 100, 255, 256, 257, 300, 320, 383, 384, 385, 449, 450, 513, 577, 769, 833, 1100]
DTYPES = [torch.float64, torch.float32]
MARGIN = 100.0


def test_well_conditioned_matrices_have_condition_number_below_20():
    worst = 0.0
    for n in WIDTHS:
        M = R.well_conditioned(n)
        assert M.dtype == torch.float64 and torch.equal(M, M.t())
        worst = max(worst, R.condition_number(M))
        assert R.condition_number(M) < 20.0, (n, R.condition_number(M))
        # the float32 rounding, damped the way the library documents float32 input, stays as well conditioned
        assert R.condition_number(R.damped(M.float(), 0.0)) < 20.0, n
    print(f"largest condition number {worst:.2f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,r", R.PIVOT_CASES)
def test_prescribed_pivot_is_the_only_one_near_the_threshold(n, r, dtype):
    """Pivot r sits a factor MARGIN below PIVOT_MIN, every other pivot a factor MARGIN above it: the status word
    r + 1 does not depend on rounding, neither in the matrix (float32) nor in the factorisation."""
    d = R.pivots(R.damped(R.prescribed_pivots(n, (r,)).to(dtype), 0.0))
    others = torch.cat([d[:r], d[r + 1:]])
    print(f"n {n} r {r} {dtype}: pivot {float(d[r]):.3e}, smallest other {float(others.min()):.3f}")
    assert 0.0 < float(d[r]) <= R.PIVOT_MIN / MARGIN
    assert float(others.min()) >= R.PIVOT_MIN * MARGIN
    # the stand-in with nothing planted is positive definite with the same margin
    assert float(R.pivots(R.damped(R.prescribed_pivots(n).to(dtype), 0.0)).min()) >= R.PIVOT_MIN * MARGIN


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,planted", R.DOUBLE_CASES)
def test_two_planted_pivots_both_fall_below_the_threshold(n, planted, dtype):
    """The earlier planted pivot is positive and a factor MARGIN below the threshold, the later one below it as well
    (in float32 possibly negative: it follows a column divided by 1e-3), every other pivot a factor MARGIN above: the
    word is min(planted) + 1 only if the first failure is the one that is kept."""
    A = R.damped(R.prescribed_pivots(n, planted).to(dtype), 0.0)
    d = R.pivots_past_failures(A)
    # the two eliminations are the same quantity: compared on the stand-in, whose pivots are all >= 1 (no amplification)
    standin = R.damped(R.prescribed_pivots(n).to(dtype), 0.0)
    assert float((R.pivots_past_failures(standin) - R.pivots(standin)).abs().max()) <= 1e-12
    first = min(planted)
    keep = torch.ones(n, dtype=torch.bool)
    for r in planted:
        print(f"n {n} planted {r} {dtype}: pivot {float(d[r]):.3e}")
        assert float(d[r]) <= R.PIVOT_MIN / MARGIN
        keep[r] = False
    assert float(d[first]) > 0.0
    assert float(d[keep].min()) >= R.PIVOT_MIN * MARGIN


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,r", R.PIVOT_CASES)
def test_not_positive_definite_matrices_fail_at_their_column(n, r, dtype):
    """Subtracting 5 from M[r, r] leaves the leading r x r block alone (pivots before r as before, positive) and makes
    pivot r at most -3; LAPACK's status word is then r + 1, which is what the GPU test expects."""
    for add in (0.0, 0.3):
        A = R.damped(R.not_pd(n, r).to(dtype), add)
        good = R.damped(R.well_conditioned(n).to(dtype), add)
        assert R.failing_word(A) == r + 1
        C = torch.linalg.cholesky(good)
        # pivot r of A = pivot r of the good matrix - 5 (the columns before r are the same)
        assert float(C[r, r] ** 2) - 5.0 <= -3.0
        if r > 0:
            assert float(R.pivots(good)[:r].min()) > 0.05


def test_reversed_damped_factor_is_the_flip_of_the_damped_factor():
    F = R.not_pd(70, 6).float()
    A = R.damped_reversed(F, 0.25, 1.0)
    want = (F.double() + F.double().t()) / 2 + 0.5 * torch.eye(70, dtype=torch.float64)
    assert float((torch.flip(A, (0, 1)) - want).abs().max()) <= 1e-6            # float32 damping vs float64 damping
    assert R.failing_word(A) == 70 - 6                                           # reversed index 63, plus one
