"""`curv_syevd_ex` / `curv_syevd` (csrc/eigh.hip behind csrc/eigh_lowrank.hip: the block-Jacobi eigensolver under EFB, INF,
KFAC.decompose and the damping grid) called through the C entry point itself, against float64 torch on the CPU and the
yardsticks of eigh_refs.py (what the reference achieves once it is rounded to float32).

What a call runs through: eigh_diag_order_kernel and eigh_prepare32_kernel (sym(F), diagonal in descending order), phase A
in float32 down to off(A) <= 2e-6 ||A|| or a stall, the switch (eigh_widen_kernel, one Newton-Schulz step, the exact
A = V'^T sym(F) V' by four float64 products and eigh_mirror_kernel), phase B in float64 to the tolerance, eigh_sort_kernel and
eigh_gather_kernel.  Phase A alone leaves a residual of 2e-6 - 50 times the yardstick - so the bars here (4 times the
yardstick) are only met when the float64 half really ran on the right matrix.

Every matrix is narrower than 2048: the projection path of eigh_lowrank.hip is never taken (ranks[i] == 0 is asserted).
Widths are the block (32), tile (64) and two-tile edges, 321 (six tiles wide, ragged), 1024 and the two widths past the 1e-8
rule.  F lies inside a NaN-filled arena and must come back bit-unchanged; U and w are views inside arenas of a marked NaN
pattern that must come back bit-identical everywhere outside the n x n and n views (a pad row of the np-wide work matrix or
the perm_stride of a wider neighbour written through would show there)."""
import ctypes

import pytest
import torch

import eigh_refs as R

pytestmark = pytest.mark.gpu

FACTOR = 4.0                      # bars = FACTOR x yardstick: headroom for the 1e-8 off-norm and the Newton-Schulz remainder
MARK = 0x7FC5A5A5                 # a quiet NaN with a payload: what U and w arenas are filled with
F_FILL = 0x7FC00000               # the plain quiet NaN around F
WIDE_RESIDUAL = 2 * 5e-6          # above 1024 wide the documented default is off(A) <= 5e-6 ||A||
worst = {}                        # (family, measure) -> largest got / yardstick seen


class Arena:
    """One flat float32 GPU buffer filled with a bit pattern; item i (sizes[i] floats) has 64 n_i + 64 pattern words in
    front of it and behind it - more than the 63 pad rows of an np-wide matrix."""

    def __init__(self, sizes, widths, gpu, fill):
        self.fill, self.offsets, self.sizes = fill, [], list(sizes)
        pos = 8
        for s, n in zip(sizes, widths):
            gap = 64 * n + 64
            self.offsets.append(pos + gap)
            pos += gap + s + gap
        self.bits = torch.full((pos,), fill, dtype=torch.int32, device=gpu)
        self.buf = self.bits.view(torch.float32)

    def view(self, i, shape):
        v = self.buf[self.offsets[i]:self.offsets[i] + self.sizes[i]].view(shape)
        assert v.data_ptr() == self.buf.data_ptr() + 4 * self.offsets[i]
        return v

    def outside_is_untouched(self, include_views=False):
        bits = self.bits.cpu()
        keep = torch.ones(bits.numel(), dtype=torch.bool)
        if not include_views:
            for o, s in zip(self.offsets, self.sizes):
                keep[o:o + s] = False
        return bool((bits[keep] == self.fill).all())


class Result:
    pass


def run(gpu, mats, max_sweeps=0, tol=0.0, with_w=True, entry="ex", with_ranks=True, ws=None, null=None, short=0,
        expect_untouched=False):
    """One call of the C entry point on CPU float32 matrices `mats`.  `null` = (position, "F" | "U"): that pointer is
    passed as NULL; `short`: bytes taken off the workspace size the call is told.  Asserts the fences and that F is
    bit-unchanged; `expect_untouched`: the U and w views still hold the mark as well."""
    from curvature_amd import _lib, ops
    L = _lib.lib()
    m = len(mats)
    widths = [F.shape[0] for F in mats]
    fa = Arena([n * n for n in widths], widths, gpu, F_FILL)
    ua = Arena([n * n for n in widths], widths, gpu, MARK)
    wa = Arena(widths, widths, gpu, MARK)
    arr = (_lib.curv_eigh_desc * m)()
    for i, F in enumerate(mats):
        fa.view(i, F.shape).copy_(F)
        arr[i].F = fa.view(i, F.shape).data_ptr()
        arr[i].U = ua.view(i, F.shape).data_ptr()
        arr[i].w = wa.view(i, (widths[i],)).data_ptr() if with_w else None
        arr[i].n = widths[i]
    if null is not None:
        setattr(arr[null[0]], null[1], None)
    before = fa.bits.clone()
    need = L.curv_syevd_workspace_bytes(arr, m)
    assert need > 0
    if ws is None:
        ws = ops.workspace(need, gpu, "eigh_direct")
    assert ws.numel() >= need
    sweeps = ctypes.c_int(-1)
    ranks = (ctypes.c_int * m)(*([-1] * m))
    torch.cuda.synchronize()
    if entry == "ex":
        rc = L.curv_syevd_ex(_lib.stream_ptr(), arr, m, ws.data_ptr(), need - short, int(max_sweeps), float(tol),
                             ctypes.byref(sweeps), ranks if with_ranks else None)
    else:
        rc = L.curv_syevd(_lib.stream_ptr(), arr, m, ws.data_ptr(), need - short, int(max_sweeps), float(tol),
                          ctypes.byref(sweeps))
    torch.cuda.synchronize()
    r = Result()
    r.rc, r.sweeps, r.ws = rc, sweeps.value, ws
    r.error = L.curv_last_error().decode("utf-8", "replace") if rc != 0 else ""
    r.ranks = list(ranks) if (entry == "ex" and with_ranks) else None
    assert torch.equal(fa.bits, before), "F was written to"
    assert ua.outside_is_untouched(expect_untouched), "a write outside the n x n views of U"
    assert wa.outside_is_untouched(expect_untouched or not with_w), "a write outside the n views of w"
    r.U = [ua.view(i, F.shape).cpu() for i, F in enumerate(mats)]
    r.w = [wa.view(i, (widths[i],)).cpu() for i in range(m)]
    return r


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def note(family, measure, got, ref):
    """got / ref into the table of worst ratios (a yardstick of exactly 0 - a 1 x 1 input - admits exactly 0)."""
    ratio = got / ref if ref > 0.0 else (0.0 if got == 0.0 else float("inf"))
    worst[(family, measure)] = max(worst.get((family, measure), 0.0), ratio)
    return ratio


def check_bars(family, tag, y, U, w, residual_bar=None):
    """The bars of an accuracy case, in float64: finite, w ascending, residual and orthogonality within FACTOR of the
    yardstick (or the residual within `residual_bar`), eigenvalues within output rounding plus twice the promised
    off-norm.  `w` may be float64 already (the scaled cases divide it by 2^s first)."""
    assert U.dtype == torch.float32 and U.shape == y.U.shape, tag
    Ud, wd = U.double(), w.double()
    assert bool(torch.isfinite(Ud).all()) and bool(torch.isfinite(wd).all()), tag
    assert bool((wd[1:] >= wd[:-1]).all()), tag
    res, orth = R.residual(y.S, Ud, wd), R.orthogonality(Ud)
    eig = float(((wd - y.w).abs() / R.eigenvalue_bound(y)).max())
    r_res = note(family, "residual", res, y.res_ref)
    r_orth = note(family, "orthogonality", orth, y.orth_ref)
    worst[(family, "eigenvalues / bound")] = max(worst.get((family, "eigenvalues / bound"), 0.0), eig)
    print(f"{family} {tag}: residual {res:.3e} ({r_res:.2f} x yardstick), orthogonality {orth:.3e} ({r_orth:.2f} x), "
          f"eigenvalue error {eig:.3f} of its bound")
    if residual_bar is None:
        assert res <= FACTOR * y.res_ref, (family, tag, res, y.res_ref)
    else:
        assert res <= residual_bar, (family, tag, res)
    assert orth <= FACTOR * y.orth_ref, (family, tag, orth, y.orth_ref)
    assert eig <= 1.0, (family, tag, eig)


def check_subspaces(family, tag, y, U):
    assert y.groups, tag
    Ud = U.double()
    for g, proj_ref, gap in y.groups:
        d = R.projector_distance(Ud[:, g], y.U[:, g])
        bar = R.projector_bound(y, proj_ref, gap, FACTOR)
        note(family, "projector", d, proj_ref)
        worst[(family, "projector / bar")] = max(worst.get((family, "projector / bar"), 0.0), d / bar)
        assert d <= bar, (family, tag, g[0], len(g), d, proj_ref, gap)
    print(f"{family} {tag}: {len(y.groups)} subspaces, worst so far {worst[(family, 'projector')]:.2f} x yardstick, "
          f"{worst[(family, 'projector / bar')]:.3f} of the bar")


def converged_plainly(r):
    assert r.rc == 0, (r.rc, r.error)
    assert r.ranks is None or r.ranks == [0] * len(r.ranks)


# ================================================================================================ 1. accuracy
@pytest.mark.parametrize("family", R.FAMILIES)
def test_accuracy_at_float32_output_precision(gpu, family):
    """Every width up to 1024 of one family in one default call (np = 64 ... 1024; 1 and 2 wide are one tile of padding
    around one or two numbers).  Residual and orthogonality within 4 x what the float64 reference rounded to float32
    achieves, eigenvalues ascending and within 2^-24 |w| + 2e-8 ||F||_F.  `asymmetric`: the reference is that of
    sym(F).  Phase A alone ends at a residual of 2e-6, 50 x the yardstick."""
    r = run(gpu, [R.matrix(family, n) for n in R.SIZES])
    converged_plainly(r)
    assert 2 <= r.sweeps < 60
    for n, U, w in zip(R.SIZES, r.U, r.w):
        check_bars(family, f"n {n}", R.yardstick(family, n), U, w)
    print(f"{family}: sweeps_done {r.sweeps}; worst ratios " +
          ", ".join(f"{k[1]} {v:.2f}" for k, v in sorted(worst.items()) if k[0] == family))


# ================================================================================================ 2. subspaces
@pytest.mark.parametrize("family", R.SUBSPACE_FAMILIES)
def test_invariant_subspaces(gpu, family):
    """The orthogonal projector onto every cluster and every simple eigenvector against the reference's:
    ||P(U[:, g]) - P(U_ref[:, g])||_F <= max(4 x what the rounded reference achieves, 2e-8 ||F||_F / gap) - the second
    term is Davis-Kahan on twice the promised off-norm.  A residual cannot see a rotation inside the wrong subspace when
    eigenvalues are close; this does.  (planted_d has no determined subspaces: eigh_refs.groups.)"""
    r = run(gpu, [R.matrix(family, n) for n in R.SUBSPACE_SIZES])
    converged_plainly(r)
    for n, U in zip(R.SUBSPACE_SIZES, r.U):
        check_subspaces(family, f"n {n}", R.yardstick(family, n), U)


# ================================================================================================ 3. the tolerance rule
def test_default_tolerance_reaches_1e_8_at_1024(gpu):
    """np = 1024 is the last width of the 1e-8 rule (`d.np <= 1024`), alone in its call."""
    r = run(gpu, [R.matrix("lowrank", 1024)])
    converged_plainly(r)
    check_bars("tolerance", "lowrank n 1024 default", R.yardstick("lowrank", 1024), r.U[0], r.w[0])


def test_default_tolerance_above_1024_and_an_explicit_one(gpu):
    """1025 (np = 1088) and 1100 (np = 1152) with default arguments stop at off(A) <= 5e-6 ||A||: residual within twice
    that, orthogonality still at the yardstick (the Newton-Schulz step does not depend on the tolerance).  With
    tol = 1e-8 - "an explicit tol applies to every matrix" - the same matrices meet the bars of the narrow ones."""
    cases = [(f, n) for n in R.WIDE for f in R.WIDE_FAMILIES]
    mats = [R.matrix(f, n) for f, n in cases]
    loose = run(gpu, mats)
    converged_plainly(loose)
    for (f, n), U, w in zip(cases, loose.U, loose.w):
        y = R.yardstick(f, n)
        assert bool(torch.isfinite(U).all()) and bool((w[1:] >= w[:-1]).all())
        res, orth = R.residual(y.S, U.double(), w.double()), R.orthogonality(U.double())
        print(f"tolerance {f} n {n} default: residual {res:.3e}, orthogonality {orth:.3e} ({orth / y.orth_ref:.2f} x)")
        assert res <= WIDE_RESIDUAL, (f, n, res)
        assert orth <= FACTOR * y.orth_ref, (f, n, orth, y.orth_ref)
    tight = run(gpu, mats, tol=1e-8)
    converged_plainly(tight)
    print(f"tolerance: sweeps_done default {loose.sweeps}, tol 1e-8 {tight.sweeps}")
    assert tight.sweeps >= loose.sweeps
    for (f, n), U, w in zip(cases, tight.U, tight.w):
        check_bars("tolerance", f"{f} n {n} tol 1e-8", R.yardstick(f, n), U, w)


def test_a_loose_explicit_tolerance_ends_early(gpu):
    """tol = 1e-3 at 321 wide: converged, in no more sweeps than the default call, residual within 2e-3, and the
    basis still orthogonal to the yardstick."""
    mats = [R.matrix("lowrank", 321), R.matrix("indefinite", 321)]
    default = run(gpu, mats)
    loose = run(gpu, mats, tol=1e-3)
    converged_plainly(default)
    converged_plainly(loose)
    print(f"tolerance: n 321 sweeps_done default {default.sweeps}, tol 1e-3 {loose.sweeps}")
    assert 1 <= loose.sweeps <= default.sweeps
    for f, U, w in zip(("lowrank", "indefinite"), loose.U, loose.w):
        y = R.yardstick(f, 321)
        assert bool(torch.isfinite(U).all()) and bool((w[1:] >= w[:-1]).all())
        res, orth = R.residual(y.S, U.double(), w.double()), R.orthogonality(U.double())
        print(f"tolerance {f} n 321 tol 1e-3: residual {res:.3e}, orthogonality {orth:.3e} ({orth / y.orth_ref:.2f} x)")
        assert res <= 2e-3 and orth <= FACTOR * y.orth_ref, (f, res, orth, y.orth_ref)


# ================================================================================================ 4. max_sweeps
def test_max_sweeps_returns_the_last_iterate(gpu):
    """max_sweeps = 2 on lowrank(321): one float32 sweep (phase A always leaves one to phase B), the switch, one float64
    sweep - not converged, CURV_ERR_NOT_CONVERGED with text, and the outputs are the last iterate: finite, ascending,
    orthogonal to 1e-5.  A default call on the same workspace afterwards is as good as any."""
    from curvature_amd import _lib
    F, y = R.matrix("lowrank", 321), R.yardstick("lowrank", 321)
    cut = run(gpu, [F], max_sweeps=2)
    assert cut.rc == _lib.ERR_NOT_CONVERGED and "not converged" in cut.error
    assert cut.sweeps == 2
    U, w = cut.U[0].double(), cut.w[0].double()
    assert bool(torch.isfinite(U).all()) and bool(torch.isfinite(w).all())
    assert bool((w[1:] >= w[:-1]).all())
    assert R.orthogonality(U) <= 1e-5
    print(f"max_sweeps 2: residual {R.residual(y.S, U, w):.3e}, orthogonality {R.orthogonality(U):.3e}")
    again = run(gpu, [F], ws=cut.ws)
    converged_plainly(again)
    assert 2 <= again.sweeps < 60
    check_bars("max_sweeps", "lowrank n 321 default after a cut call", y, again.U[0], again.w[0])


# ================================================================================================ 5. w == NULL, curv_syevd
def test_null_w_and_the_plain_entry_point_give_the_same_bits(gpu):
    mats = [R.matrix("indefinite", 65), R.matrix("lowrank", 129), R.matrix("planted_c", 33)]
    full = run(gpu, mats)
    converged_plainly(full)
    no_w = run(gpu, mats, with_w=False)
    no_ranks = run(gpu, mats, with_ranks=False)
    plain = run(gpu, mats, entry="plain")
    for other in (no_w, no_ranks, plain):
        assert other.rc == 0 and other.sweeps == full.sweeps
        for a, b in zip(full.U, other.U):
            assert same_bits(a, b)
    for a, b, c in zip(full.w, no_ranks.w, plain.w):
        assert same_bits(a, b) and same_bits(a, c)
    for (f, n), U, w in zip((("indefinite", 65), ("lowrank", 129), ("planted_c", 33)), plain.U, plain.w):
        check_bars("entry points", f"{f} n {n} curv_syevd", R.yardstick(f, n), U, w)


# ================================================================================================ 6. refusals
def test_sizes_out_of_range_are_refused(gpu):
    from curvature_amd import _lib
    L = _lib.lib()
    for n in (0, 8193):
        arr = (_lib.curv_eigh_desc * 2)()
        arr[0].n, arr[1].n = 64, n
        assert L.curv_syevd_workspace_bytes(arr, 2) == 0
        arr[0].n = n
        assert L.curv_syevd_workspace_bytes(arr, 1) == 0
    arr = (_lib.curv_eigh_desc * 1)()
    arr[0].n = 8192
    assert L.curv_syevd_workspace_bytes(arr, 1) > 0
    # the call itself: a good matrix first, the refused size second; nothing may be written
    ua, wa = Arena([64 * 64], [64], gpu, MARK), Arena([64], [64], gpu, MARK)
    F = R.matrix("lowrank", 64).to(gpu)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=gpu)
    for n in (0, 8193):
        arr = (_lib.curv_eigh_desc * 2)()
        for d in arr:
            d.F, d.U, d.w, d.n = F.data_ptr(), ua.view(0, (64, 64)).data_ptr(), wa.view(0, (64,)).data_ptr(), 64
        arr[1].n = n
        rc = L.curv_syevd_ex(_lib.stream_ptr(), arr, 2, ws.data_ptr(), ws.numel(), 0, 0.0, None, None)
        torch.cuda.synchronize()
        assert rc == _lib.ERR_INVALID
        assert "out of range" in L.curv_last_error().decode()
        assert ua.outside_is_untouched(True) and wa.outside_is_untouched(True)


@pytest.mark.parametrize("which", ["F", "U"])
def test_null_pointers_are_refused_before_anything_is_launched(gpu, which):
    """A null F or U in the SECOND of two matrices: the first one's outputs still hold the mark."""
    from curvature_amd import _lib
    r = run(gpu, [R.matrix("lowrank", 65), R.matrix("indefinite", 33)], null=(1, which), expect_untouched=True)
    assert r.rc == _lib.ERR_INVALID and "null pointer" in r.error


def test_a_workspace_one_byte_short_is_refused(gpu):
    from curvature_amd import _lib
    mats = [R.matrix("lowrank", 65), R.matrix("indefinite", 33)]
    r = run(gpu, mats, short=1, expect_untouched=True)
    assert r.rc == _lib.ERR_WORKSPACE and "workspace too small" in r.error
    converged_plainly(run(gpu, mats, ws=r.ws))              # the size the library asked for is enough


# ================================================================================================ 7. asymmetric input
def test_asymmetric_input_is_symmetrised_by_the_library(gpu):
    """F = S + K with a skew K as large as S: the call on F and the call on (F + F^T) / 2 - a float32 matrix without
    rounding (test_eigh_refs_cpu.py) - return the same bits, from both symmetrising kernels (eigh_prepare32_kernel feeds
    phase A, eigh_input64_kernel the exact A of the switch)."""
    sizes = [33, 129]
    raw = [R.matrix("asymmetric", n) for n in sizes]
    halves = [R.sym(F).float() for F in raw]
    a, b = run(gpu, raw), run(gpu, halves)
    converged_plainly(a)
    converged_plainly(b)
    assert a.sweeps == b.sweeps
    for n, Ua, Ub, wa, wb in zip(sizes, a.U, b.U, a.w, b.w):
        assert same_bits(Ua, Ub) and same_bits(wa, wb), n
        check_bars("asymmetric", f"n {n} beside its symmetric half", R.yardstick("asymmetric", n), Ua, wa)


# ================================================================================================ 8. scale
@pytest.mark.parametrize("s", R.SCALES)
def test_scaled_matrices(gpu, s):
    """2^s F for s = -40, 40 (gradient-side factors of a trained network; activations of an unnormalised one) and
    s = -100, 100, where the float32 sub-problem solve stops rotating: |apq| falls below its absolute 1e-30, or
    app * aqq overflows in float.  Phase A then stalls after two sweeps and the float64 phase does the work.  After
    dividing w by 2^s (exact) the bars of the unscaled problem hold.  One matrix per call: sweeps_done is its own."""
    for f, n in R.SCALED:
        unscaled = run(gpu, [R.matrix(f, n)])
        r = run(gpu, [R.scaled(f, n, s)])
        converged_plainly(unscaled)
        converged_plainly(r)
        assert 2 <= r.sweeps < 60
        U, w, U0, w0 = r.U[0], r.w[0], unscaled.U[0], unscaled.w[0]
        y = R.yardstick(f, n)
        back = w.double() * 2.0 ** -s
        identical = same_bits(U, U0) and torch.equal(back, w0.double())
        print(f"scale 2^{s} {f} n {n}: sweeps_done {r.sweeps} (unscaled {unscaled.sweeps}), "
              f"bit-identical to the unscaled result: {identical}")
        check_bars(f"scale 2^{s}", f"{f} n {n}", y, U, back)
        if y.groups:
            check_subspaces(f"scale 2^{s}", f"{f} n {n}", y, U)


# ================================================================================================ 9. non-finite input
def test_non_finite_matrices_do_not_disturb_their_neighbours(gpu):
    """A NaN off the diagonal of one matrix and +inf on the diagonal of another, between three good ones.  Every loop
    of the iteration is bounded by max_sweeps and a NaN norm freezes the matrix (state 2), so the call returns - with
    CURV_ERR_NOT_CONVERGED - and the good matrices come out bit-identical to calls of their own."""
    from curvature_amd import _lib
    bad_nan = R.matrix("lowrank", 65).clone()
    bad_nan[3, 40] = float("nan")
    bad_inf = R.matrix("indefinite", 33).clone()
    bad_inf[5, 5] = float("inf")
    good = {0: ("lowrank", 65), 2: ("planted_b", 129), 4: ("indefinite", 64)}
    mats = [R.matrix(*good[0]), bad_nan, R.matrix(*good[2]), bad_inf, R.matrix(*good[4])]
    r = run(gpu, mats)
    assert r.rc == _lib.ERR_NOT_CONVERGED and "not converged: 2 of 5 matrices (first: 1)" in r.error
    assert r.ranks == [0] * 5
    for pos, (f, n) in good.items():
        alone = run(gpu, [R.matrix(f, n)])
        converged_plainly(alone)
        assert same_bits(r.U[pos], alone.U[0]) and same_bits(r.w[pos], alone.w[0]), (f, n)
        check_bars("non-finite neighbours", f"{f} n {n}", R.yardstick(f, n), r.U[pos], r.w[pos])


# ================================================================================================ 10. batch bookkeeping
BATCH = 130
BATCH_SIZES = [1, 33, 64, 65, 129]
SAMPLED = [0, 23, 24, 47, 48, 63, 64, 65, 127, 128, 129, 100]


def batch_case(pos):
    if pos == 0:
        return "lowrank", 321
    if pos == BATCH - 1:
        return "indefinite", 321
    return R.FAMILIES[pos % len(R.FAMILIES)], BATCH_SIZES[pos % len(BATCH_SIZES)]


def test_a_batch_of_130_matrices(gpu):
    """130 descriptors: six uploads of up to 24 table rows (EIG_UPLOAD_CHUNK), three 64-descriptor rounds of eig_locate's
    scan (its running `base`), widths cycling through 1, 33, 64, 65, 129 and families through all seven, a 321-wide
    matrix first and last (perm_stride = 321 for everybody).  Every matrix meets the accuracy bars; twelve positions -
    both sides of every chunk edge - are bit-identical to the same matrix in a call of its own."""
    cases = [batch_case(p) for p in range(BATCH)]
    r = run(gpu, [R.matrix(f, n) for f, n in cases])
    converged_plainly(r)
    for pos, (f, n) in enumerate(cases):
        check_bars("batch of 130", f"position {pos} {f} n {n}", R.yardstick(f, n), r.U[pos], r.w[pos])
    for pos in SAMPLED:
        f, n = cases[pos]
        alone = run(gpu, [R.matrix(f, n)])
        converged_plainly(alone)
        assert same_bits(r.U[pos], alone.U[0]) and same_bits(r.w[pos], alone.w[0]), (pos, f, n)


# ================================================================================================ 11. exact ties
@pytest.mark.parametrize("n", R.TIE_SIZES)
def test_a_diagonal_matrix_comes_back_exactly_with_ties_in_index_order(gpu, n):
    """A diagonal F needs no rotation: w is its diagonal sorted, U a permutation matrix, both exact.  Equal values keep
    their index order - eigh_diag_order_kernel and eigh_sort_kernel break ties by index, so that the order is a function
    of F alone and the same as the stable sort of the low-rank path."""
    F = R.diagonal_with_ties(n)
    d = torch.diagonal(F)
    r = run(gpu, [F])
    converged_plainly(r)
    order = torch.sort(d, stable=True).indices
    assert torch.equal(r.w[0], d[order])
    want = torch.zeros(n, n)
    want[order, torch.arange(n)] = 1.0
    assert torch.equal(r.U[0], want)
