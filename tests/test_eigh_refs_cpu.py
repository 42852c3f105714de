"""The inputs of tests/eigh_refs.py against the float64 reference alone (no GPU, no library): the bars of
tests/test_eigh_direct_gpu.py are multiples of what the float32-rounded reference achieves, so that yardstick has to be
what they assume - non-zero, at the float32 rounding level, with the planted multiplicities and gaps really there.

Two places where a 1 x 1 or an equally spaced spectrum cannot be what a general rule asks for are stated where they
are asserted: a 1 x 1 input has nothing to round (its yardstick is exactly 0, and so is the bar), and the simple
eigenvalues of planted_a are 3 / (n - 1) apart - from 33 wide up that is below 0.05 ||F||_2, so their gap is asserted
as what it is; the projector bar of the GPU test divides by the gap itself."""
import pytest
import torch

import eigh_refs as R

ROUNDING_LEVEL = 2e-7          # res_ref and orth_ref lie below it (float32: 2^-24 = 6e-8 per entry)
MIN_GAP = 0.05                 # relative to ||F||_2: every cluster, every outlier
CLUSTER_SPREAD = 1e-6          # relative to ||F||_2: what the float32 rounding of F leaves of a planted cluster

CASES = [(f, n) for f in R.FAMILIES for n in R.SIZES] + [(f, n) for f in R.WIDE_FAMILIES for n in R.WIDE]


@pytest.mark.parametrize("family", R.FAMILIES)
def test_yardstick_is_the_float32_rounding_level(family):
    """res_ref and orth_ref of every (family, n) the GPU file uses: non-zero and below 2e-7.  1 x 1: U = [1] and
    w = F[0, 0] are float32 numbers already, both are exactly 0 - the GPU test then asks for the exact result."""
    worst_res = worst_orth = 0.0
    for f, n in CASES:
        if f != family:
            continue
        F = R.matrix(f, n)
        assert F.dtype == torch.float32 and F.shape == (n, n) and bool(torch.isfinite(F).all())
        y = R.yardstick(f, n)
        if n == 1:
            assert y.res_ref == 0.0 and y.orth_ref == 0.0 and float(F[0, 0]) != 0.0
            continue
        assert 0.0 < y.res_ref < ROUNDING_LEVEL, (f, n, y.res_ref)
        assert 0.0 < y.orth_ref < ROUNDING_LEVEL, (f, n, y.orth_ref)
        worst_res, worst_orth = max(worst_res, y.res_ref), max(worst_orth, y.orth_ref)
        assert bool((y.w[1:] >= y.w[:-1]).all())
    print(f"{family}: largest res_ref {worst_res:.2e}, largest orth_ref {worst_orth:.2e}")


@pytest.mark.parametrize("family", [f for f in R.FAMILIES if f != "asymmetric"])
def test_symmetric_families_are_symmetric(family):
    for n in R.SIZES:
        F = R.matrix(family, n)
        assert torch.equal(F, F.t()), (family, n)


def test_asymmetric_input_symmetrises_without_rounding():
    """F != F^T, the skew part is as large as the symmetric one, and (F + F^T) / 2 formed in float64 is a float32
    matrix: the call on F and the call on that matrix are given the same problem to the last bit."""
    for n in R.SIZES:
        F = R.matrix("asymmetric", n)
        S = R.sym(F)
        assert torch.equal(S.float().double(), S), n
        if n == 1:
            continue
        K = F.double() - S
        assert not torch.equal(F, F.t()), n
        ratio = float(torch.linalg.norm(K) / torch.linalg.norm(S))
        assert ratio > 0.1, (n, ratio)                     # (2 wide: one skew entry, whatever it drew)
        if n >= 32:
            assert 0.5 < ratio < 2.0, (n, ratio)


@pytest.mark.parametrize("family", R.SUBSPACE_FAMILIES)
def test_planted_multiplicities_and_gaps(family):
    """In the float32-rounded F: every cluster has its multiplicity within 1e-6 ||F||_2, and every cluster and every
    outlier is at least 0.05 ||F||_2 away from the rest.  planted_a: the n simple eigenvalues are 3 / (n - 1) apart,
    1.5 / (n - 1) of ||F||_2 = 2 - the stated gap is asserted (to 1 %), it is below 0.05 from 33 wide up."""
    for n in R.SUBSPACE_SIZES:
        y = R.yardstick(family, n)
        lam = R.spectrum(n, family[-1])
        assert float((y.w - lam).abs().max()) <= CLUSTER_SPREAD * y.two, (family, n)
        assert len(y.groups) == len(R.groups(family, n)) > 0
        covered = sorted(i for g, _, _ in y.groups for i in g)
        assert covered == list(range(n))
        for g, proj_ref, gap in y.groups:
            assert 0.0 < proj_ref < 10 * ROUNDING_LEVEL, (family, n, g[0], proj_ref)
            spread = float(y.w[g].max() - y.w[g].min())
            assert spread <= CLUSTER_SPREAD * y.two, (family, n, g[0], spread)
            assert float((lam[g] - lam[g[0]]).abs().max()) == 0.0          # one planted value per group
            if family == "planted_a":
                assert len(g) == 1
                assert abs(gap / y.two - 1.5 / (n - 1)) <= 0.01 * 1.5 / (n - 1), (n, g[0], gap)
            else:
                assert gap >= MIN_GAP * y.two, (family, n, g[0], gap / y.two)
        if family == "planted_b":
            assert [len(g) for g, _, _ in y.groups] == [n // 2, n - n // 2]
        if family == "planted_c":
            assert [len(g) for g, _, _ in y.groups] == [n - 3, 1, 1, 1]


def test_geometric_spectrum_has_no_usable_gaps():
    """Why planted_d is left out of the projector checks: a gap is a fixed share of the eigenvalue itself, so more than
    a third of the eigenvalues are closer than 1e-3 ||F||_2 to a neighbour and the closest pair is below 1e-6 ||F||_2 -
    the Davis-Kahan bar 2e-8 ||F||_F / gap is then orders of magnitude above float32 accuracy and checks nothing."""
    for n in R.SUBSPACE_SIZES:
        y = R.yardstick("planted_d", n)
        gaps = (y.w[1:] - y.w[:-1]) / y.two
        assert float((gaps < 1e-3).float().mean()) > 1.0 / 3.0, n
        assert float(gaps.min()) < 1e-6, n
        assert R.groups("planted_d", n) == []


def test_scaling_by_a_power_of_two_is_exact():
    """2^s F stays inside the normal float32 range for s = -100 ... 100: the scaled problem is the unscaled one."""
    for family, n in R.SCALED:
        F = R.matrix(family, n)
        for s in R.SCALES:
            Fs = R.scaled(family, n, s)
            assert bool(torch.isfinite(Fs).all())
            assert torch.equal(Fs.double() * 2.0 ** -s, F.double()), (family, n, s)


def test_diagonal_inputs_repeat_their_values():
    for n in R.TIE_SIZES:
        d = torch.diagonal(R.diagonal_with_ties(n))
        assert len(set(d.tolist())) == 6 and not torch.equal(d, torch.sort(d).values)
