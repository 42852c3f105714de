"""curv_gemm_batched against fp64 on every launch path, with the strided general kernel (gemm_f32_kernel) first.

Operands are views inside NaN-filled buffers (pitch wider than the view, first element off the buffer start): a read
outside a view that reaches an accumulator shows as NaN in the result while staying inside the allocation.  The output
view lies in a buffer of marked NaNs that must be bit-identical after the call.

Tolerance, derived and not measured: with u = 2^-24 and P = |A| @ |B| in fp64, every order of round-to-nearest fp32
products and sums of K terms errs by at most (K - 1 + 1) u P to first order; alpha, the epilogue's one or two
operations and the beta term add a few u of their own operands.  `S` is the epilogue on absolute values (|alpha| P,
2 |alpha| P P, |alpha| P |E|, |alpha| P + |E|, |alpha| P |E| + |F|) plus |beta| |C0|, and the bound is
(K + 8) u S per element.  Where S is 0 (K == 0, no E / F / C0 term) the result must be exactly 0.  The project's bar
of 2e-5 max|want| must hold too.  Every call is guarded by ops.gemm_plan_info: the kernels it is meant to reach are
the ones it reaches.

Triangular hints (CURV_TRI_*): the contract says op(A)(i, k) = 0 for k > i and cuts each tile's K range at the tile's
far edge, so a kernel still reads the zeros between the diagonal and that edge.  The tests keep zeros there and put
NaN behind the cut of the kernel that takes the product (tile edge 64 / 128 of the general kernel, 128 of the NT
kernel, the row itself for the gemv kernel): a cut one tile late reads NaN, a cut too early misses terms."""
import pytest
import torch

from curvature_amd import ops

U = 2.0 ** -24
NAN = float("nan")
MARK = 0x7FC0BEEF          # the NaN that fills the gaps of an output buffer
EPS = (ops.EPI_NONE, ops.EPI_SQUARE, ops.EPI_MUL_E, ops.EPI_ADD_E, ops.EPI_MUL_E_ADD_F)


def fenced(gpu, rows, cols, layout="rm", fill="randn", wide=0):
    """A (rows, cols) view inside a NaN-filled buffer -> (view, buffer).
    "rm": rows of the buffer, pitch cols + 3 + wide, starting at row 1, column 2 (with wide > 0: a column slice of a
    wider buffer); "t": the transposed view of such a block; "bcast_r" / "bcast_c": one row / column, expanded with
    stride 0."""
    if layout == "rm":
        buf = torch.full((rows + 2, cols + 3 + wide), NAN, device=gpu)
        view = buf[1:1 + rows, 2:2 + cols]
    elif layout == "t":
        buf = torch.full((cols + 2, rows + 3 + wide), NAN, device=gpu)
        view = buf[1:1 + cols, 2:2 + rows].t()
    elif layout == "bcast_r":
        buf = torch.full((3, cols + 3), NAN, device=gpu)
        view = buf[1:2, 2:2 + cols]
    elif layout == "bcast_c":
        buf = torch.full((rows + 2, 3), NAN, device=gpu)
        view = buf[1:1 + rows, 1:2]
    else:
        raise ValueError(layout)
    if fill == "randn":
        view.copy_(torch.randn(view.shape, device=gpu))
    if layout in ("bcast_r", "bcast_c"):
        view = view.expand(rows, cols)
    assert tuple(view.shape) == (rows, cols)
    return view, buf


class Case:
    """One product: the job, its fp64 reference and bound, and the output buffer's state before the call."""

    def __init__(self, gpu, M, N, K, la="rm", lb="rm", lc="rm", alpha=1.0, beta=0.0, ep=ops.EPI_NONE, le="rm", lf="rm",
                 tri=ops.TRI_NONE, cut=0, A=None, B=None):
        self.shape = (M, N, K)
        self.A = fenced(gpu, M, K, la)[0] if A is None else A
        self.B = fenced(gpu, K, N, lb)[0] if B is None else B
        if tri == ops.TRI_A_LOWER:            # zeros above the diagonal up to the tile's cut, NaN behind it
            i, k = torch.arange(M, device=gpu).view(-1, 1), torch.arange(K, device=gpu).view(1, -1)
            self.A.masked_fill_(k > i, 0.0)
            self.A.masked_fill_(k >= (i // cut + 1) * cut, NAN)
        elif tri == ops.TRI_B_UPPER:
            k, j = torch.arange(K, device=gpu).view(-1, 1), torch.arange(N, device=gpu).view(1, -1)
            self.B.masked_fill_(k > j, 0.0)
            self.B.masked_fill_(k >= (j // cut + 1) * cut, NAN)
        self.E = fenced(gpu, M, N, le, wide=5)[0] if ep >= ops.EPI_MUL_E else None
        self.F = fenced(gpu, M, N, lf, wide=2)[0] if ep == ops.EPI_MUL_E_ADD_F else None
        self.C, self.cbuf = fenced(gpu, M, N, lc, fill="none")
        self.cbuf.view(torch.int32).fill_(MARK)
        if beta != 0.0:
            self.C.copy_(torch.randn(M, N, device=gpu))
        self.cbuf0 = self.cbuf.clone()
        self.C0 = self.C.double().clone() if beta != 0.0 else None
        self.inside = torch.zeros_like(self.cbuf, dtype=torch.bool)
        (self.inside[1:1 + M, 2:2 + N] if lc == "rm" else self.inside[1:1 + N, 2:2 + M]).fill_(True)
        self.alpha, self.beta, self.ep, self.tri = alpha, beta, ep, tri
        self.job = ops.Gemm(self.A, self.B, self.C, alpha=alpha, beta=beta, epilogue=ep, E=self.E, F=self.F, tri=tri)
        self.refresh()

    def refresh(self):
        """want and bound from the operands' present contents"""
        A, B = self.A.double(), self.B.double()
        if self.tri == ops.TRI_A_LOWER:
            A = torch.tril(torch.nan_to_num(A, nan=0.0))
        elif self.tri == ops.TRI_B_UPPER:
            B = torch.triu(torch.nan_to_num(B, nan=0.0))
        acc, P, a = A @ B, A.abs() @ B.abs(), abs(self.alpha)
        E = self.E.double() if self.E is not None else None
        F = self.F.double() if self.F is not None else None
        if self.ep == ops.EPI_NONE:
            want, S = self.alpha * acc, a * P
        elif self.ep == ops.EPI_SQUARE:
            want, S = self.alpha * acc * acc, 2 * a * P * P
        elif self.ep == ops.EPI_MUL_E:
            want, S = self.alpha * acc * E, a * P * E.abs()
        elif self.ep == ops.EPI_ADD_E:
            want, S = self.alpha * acc + E, a * P + E.abs()
        else:
            want, S = self.alpha * acc * E + F, a * P * E.abs() + F.abs()
        if self.C0 is not None:
            want, S = want + self.beta * self.C0, S + abs(self.beta) * self.C0.abs()
        self.want, self.bound = want, (self.shape[2] + 8) * U * S
        assert bool(torch.isfinite(want).all())

    def reset(self):
        self.cbuf.copy_(self.cbuf0)

    def bits(self):
        return self.C.contiguous().view(torch.int32).clone()

    def check(self):
        """-> worst err / bound of this product; asserts the bound, the project's bar and the untouched gaps"""
        tag = (self.shape, self.ep, self.tri, self.alpha, self.beta)
        assert torch.equal(self.cbuf.view(torch.int32)[~self.inside], self.cbuf0.view(torch.int32)[~self.inside]), \
            f"{tag}: wrote outside the output view"
        got = self.C.double()
        if got.numel() == 0:
            return 0.0
        assert bool(torch.isfinite(got).all()), f"{tag}: {int((~torch.isfinite(got)).sum())} non-finite results"
        err = (got - self.want).abs()
        zero = self.bound == 0
        assert float(err[zero].max() if bool(zero.any()) else 0.0) == 0.0, f"{tag}: a result with bound 0 is not exact"
        ratio = float((err[~zero] / self.bound[~zero]).max()) if bool((~zero).any()) else 0.0
        assert ratio <= 1.0, f"{tag}: err / bound = {ratio:.3f}"
        assert float(err.max()) <= 2e-5 * float(self.want.abs().max()), tag
        return ratio


def run(cases):
    ops.gemm_batched([c.job for c in cases])


def check_all(cases, what):
    worst = max(c.check() for c in cases)
    print(f"{what}: worst err / bound = {worst:.4f} over {len(cases)} products")
    return worst


def plan(cases):
    return ops.gemm_plan_info([c.job for c in cases])


def tiles(shape, t):
    return -(-shape[0] // t) * -(-shape[1] // t)


SHAPES_A = [(70, 50, 40), (65, 129, 17), (130, 97, 33), (200, 161, 16), (97, 300, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("lc", ["rm", "t"])
@pytest.mark.parametrize("lb", ["rm", "t"])
@pytest.mark.parametrize("la", ["rm", "t"])
def test_layouts_and_tile_templates(gpu, la, lb, lc):
    """(a) The four staging maps x both tile templates x C row-major / transposed, ragged M / N, K % 16 in {0, 1, odd}.
    With A row-major and B transposed every product is in NT layout: one product outside it rides along so that the
    call is not small; the NT kernel then takes the three products it is eligible for, and the general kernel runs its
    a_kfast x b_kfast map on (70, 50, 40) and (97, 300, 1)."""
    torch.manual_seed(1)
    cases = [Case(gpu, M, N, K, la, lb, lc) for M, N, K in SHAPES_A]
    if (la, lb) == ("rm", "t"):
        cases.append(Case(gpu, 70, 50, 40, "t", "rm", lc))
        want = dict(tiles64=2 + 2, tiles128=3, nt_items=2 + 2 + 4)
    else:
        want = dict(tiles64=2 + 6, tiles128=2 + 4 + 3)
    assert plan(cases) == {**dict.fromkeys(ops.GEMM_PLAN_KEYS, 0), **want}
    run(cases)
    check_all(cases, f"general A {la} B {lb} C {lc}")


@pytest.mark.gpu
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_k_edges(gpu, beta):
    """(b) K around the stage depth of 16 (and 0, 1): the K-tail fetch form, the last partial stage, no stage at all.
    K == 0 with beta == 0 must store exact zeros over the NaN prefill.  (An empty view hands over a null data pointer:
    at K == 0 the descriptors carry A = B = NULL, which the entry point allows and the kernel must not touch.)"""
    torch.manual_seed(2)
    cases = []
    for K in (0, 1, 15, 16, 17, 31, 32, 33):
        cases.append(Case(gpu, 70, 50, K, "t", "t", "rm", beta=beta))          # 64 tiles, A strided / B k-fast
        cases.append(Case(gpu, 130, 100, K, "rm", "rm", "rm", beta=beta))      # 128 tiles, A k-fast / B strided
    assert plan(cases) == {**dict.fromkeys(ops.GEMM_PLAN_KEYS, 0), "tiles64": 8 * 2, "tiles128": 8 * 2}
    run(cases)
    check_all(cases, f"general K edges beta {beta}")
    if beta == 0.0:
        for c in cases[:2]:
            assert c.shape[2] == 0 and int(torch.count_nonzero(c.C)) == 0


E_LAYOUTS = ["t", "rm", "bcast_r", "bcast_c"]          # ("rm" with wide > 0: a column slice of a wider buffer)


@pytest.mark.gpu
@pytest.mark.parametrize("ep", EPS)
def test_epilogues_with_strided_operands(gpu, ep):
    """(c) Every epilogue with alpha != 1 and beta in {0, 1, -0.5} on a 64-tile and a 128-tile product; E and F as
    transposed views, column slices of wider buffers and stride-0 broadcasts along either axis; C row-major / transposed."""
    torch.manual_seed(3 + ep)
    cases = []
    for s, (M, N, K) in enumerate([(70, 50, 40), (130, 97, 33)]):
        for b, beta in enumerate((0.0, 1.0, -0.5)):
            n = 3 * s + b
            cases.append(Case(gpu, M, N, K, "t", "rm", "t" if n % 2 else "rm", alpha=-1.25 if s else 0.75, beta=beta, ep=ep,
                              le=E_LAYOUTS[n % 4], lf=E_LAYOUTS[(n + 1 + n // 4) % 4]))
    assert plan(cases) == {**dict.fromkeys(ops.GEMM_PLAN_KEYS, 0), "tiles64": 3 * 2, "tiles128": 3 * 2}
    run(cases)
    check_all(cases, f"general epilogue {ep}")


@pytest.mark.gpu
def test_triangular_cuts_on_the_general_kernel(gpu):
    """(d) TRI_A_LOWER with A = tril read through the transposed view of an upper-triangular buffer, TRI_B_UPPER with
    B = triu likewise; n below, at and above one and two tiles of either template, a ragged other edge."""
    torch.manual_seed(4)
    cases, t64, t128 = [], 0, 0
    for n in (37, 64, 65, 130, 200):
        for other in (50, 97):
            t = 128 if n >= 96 and other >= 96 else 64
            cases.append(Case(gpu, n, other, n, "t", "rm", "rm", tri=ops.TRI_A_LOWER, cut=t))
            cases.append(Case(gpu, other, n, n, "t", "t", "rm", beta=1.0, tri=ops.TRI_B_UPPER, cut=t))
            t64 += 2 * tiles((n, other), 64) if t == 64 else 0
            t128 += 2 * tiles((n, other), 128) if t == 128 else 0
    assert plan(cases) == {**dict.fromkeys(ops.GEMM_PLAN_KEYS, 0), "tiles64": t64, "tiles128": t128} and t128 > 0
    run(cases)
    check_all(cases, "general triangular")


SHAPES_E = [(31, 65, 1025), (63, 200, 40), (200, 63, 40), (129, 64, 7)]


@pytest.mark.gpu
def test_nt_layout_products_on_the_general_and_the_small_kernel(gpu):
    """(e) NT-layout products too thin or too short for the NT kernel: beside one product outside NT layout the general
    kernel takes them (its a_kfast x b_kfast map, K up to 1025); alone, with K <= 1024, the small kernel does."""
    torch.manual_seed(5)
    cases = [Case(gpu, M, N, K, "rm", "t", "rm") for M, N, K in SHAPES_E] + [Case(gpu, 70, 50, 40, "t", "rm", "rm")]
    assert plan(cases) == {**dict.fromkeys(ops.GEMM_PLAN_KEYS, 0), "tiles64": 2 + 4 + 4 + 3 + 2}
    run(cases)
    check_all(cases, "general, NT layout")
    alone = [Case(gpu, M, N, min(K, 1024), "rm", "t", "rm") for M, N, K in SHAPES_E]
    assert plan(alone) == {**dict.fromkeys(ops.GEMM_PLAN_KEYS, 0), "small_blocks": 3 + 14 + 14 + 10}
    run(alone)
    check_all(alone, "small kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("m, n", [(121, 401), (10, 85)])
def test_estimator_shapes(gpu, m, n):
    """(f) The products of the estimators as they issue them, for a layer of m outputs and n inputs (bias column in)."""
    torch.manual_seed(6)
    none = dict.fromkeys(ops.GEMM_PLAN_KEYS, 0)
    # Diagonal.sample_and_replace: ones (m, 1) x ones (1, n') with E = z[:, cols] (a column slice), F = the mean
    ones_r = torch.ones(m + 7, 1, device=gpu)[:m]
    ones_c = torch.ones(1, n + 9, device=gpu)[:, :n - 1]
    diag = Case(gpu, m, n - 1, 1, ep=ops.EPI_MUL_E_ADD_F, le="rm", lf="rm", A=ones_r, B=ones_c)
    assert diag.E.stride(0) > n - 1 and diag.job.B.stride(0) != 1
    # EFB.update: tmp = U_G^T G, then state += (tmp U_A)**2
    ug = fenced(gpu, m, m)[0]
    efb1 = Case(gpu, m, n, m, A=ug.t(), lb="rm")
    # INF.sampler: Xq^T = (t1 U_A)^T written through a transposed view
    inf = Case(gpu, m, n, n, "rm", "rm", "t")
    first = [diag, efb1, inf]
    t = 128 if m >= 96 else 64
    assert plan(first) == {**none, ("tiles128" if t == 128 else "tiles64"): 3 * tiles((m, n), t)}
    run(first)
    check_all(first, f"estimator products {m} x {n}")
    efb2 = Case(gpu, m, n, n, beta=1.0, ep=ops.EPI_SQUARE, A=efb1.C, lb="rm")
    assert plan([efb2]) == {**none, ("tiles128" if t == 128 else "tiles64"): tiles((m, n), t)}
    run([efb2])
    check_all([efb2], f"EFB state update {m} x {n}")


def mixed_call(gpu):
    """3 general + 3 NT (K = 1536 and 2000 sliced, 1100 not) + 3 gemv + 2 empty products, interleaved.  Every product
    keeps its kernel when sent alone (K > 1024 wherever the layout is NT, so that no single-product call is small)."""
    g = [Case(gpu, 70, 50, 40, "t", "rm", "rm", alpha=0.5),
         Case(gpu, 130, 97, 33, "rm", "rm", "t", beta=1.0),
         Case(gpu, 31, 200, 17, "t", "t", "rm", ep=ops.EPI_ADD_E, le="t")]
    nt = [Case(gpu, 130, 200, 1536, "rm", "t", "rm", beta=1.0),
          Case(gpu, 128, 65, 1100, "rm", "t", "t", ep=ops.EPI_MUL_E, le="bcast_c"),
          Case(gpu, 200, 64, 2000, "rm", "t", "rm", alpha=-2.0, ep=ops.EPI_SQUARE)]
    v = [Case(gpu, 7, 1, 1100, "rm", "t", "rm"),
         Case(gpu, 130, 1, 1537, "rm", "t", "rm", alpha=1.5, beta=-0.5, ep=ops.EPI_MUL_E_ADD_F),
         Case(gpu, 1101, 1, 1101, "rm", "t", "rm", tri=ops.TRI_A_LOWER, cut=1)]       # the row's own length: no zeros read
    empty = [Case(gpu, 0, 40, 16, "t", "rm", "rm"), Case(gpu, 33, 0, 1100, "rm", "t", "rm")]
    cases = [g[0], nt[0], v[0], empty[0], g[1], nt[1], v[1], g[2], empty[1], nt[2], v[2]]
    for kind, group in (("general", g), ("nt", nt), ("gemv", v), ("empty", empty)):
        for c in group:
            c.kind = kind
    want = {**dict.fromkeys(ops.GEMM_PLAN_KEYS, 0), "tiles64": 2 + 4, "tiles128": 2, "nt_items": 4 * 2 + 1 + 2 * 3,
            "split_products": 2, "reduce_wgs": 4 + 2, "gemv_wgs": 2 + 33 + 276}
    return cases, want


@pytest.mark.gpu
def test_one_call_with_all_four_lists(gpu):
    """(g) The table holds the general list, then the NT list, then the gemv list: every product meets the bound, and
    its bits are those it gets alone (the sliced products alone in calls that slice them too)."""
    torch.manual_seed(7)
    cases, want = mixed_call(gpu)
    assert plan(cases) == want
    run(cases)
    check_all(cases, "mixed call")
    together = [c.bits() for c in cases]
    for c, bits in zip(cases, together):
        c.reset()
        p = plan([c])
        used = {k for k, v in p.items() if v}
        assert used == {"general": {"tiles128" if c.shape[0] >= 96 and c.shape[1] >= 96 else "tiles64"},
                        "nt": {"nt_items", "split_products", "reduce_wgs"} if c.shape[2] >= 1536 else {"nt_items"},
                        "gemv": {"gemv_wgs"}, "empty": set()}[c.kind], (c.shape, p)
        run([c])
        c.check()
        assert torch.equal(c.bits(), bits), c.shape


@pytest.mark.gpu
def test_tables_beyond_64_descriptors(gpu):
    """(h) 70 general + 70 NT + 70 gemv products in one call: 210 table rows uploaded 17 at a time, gemm_find's second
    ballot round in both tiled kernels, and the reduce kernel's look-up with split products below and above row 64."""
    torch.manual_seed(8)
    cases, split_at = [], (3, 30, 62, 64, 65, 69)
    want = dict.fromkeys(ops.GEMM_PLAN_KEYS, 0)
    for i in range(70):
        M, N, K = 5 + (i * 37) % 126, 3 + (i * 53) % 128, (i * 7) % 41
        cases.append(Case(gpu, M, N, K, "t" if i % 2 else "rm", "rm", "rm" if i % 3 else "t", beta=float(i % 2)))
        t = 128 if M >= 96 and N >= 96 else 64
        want["tiles128" if t == 128 else "tiles64"] += tiles((M, N), t)
        M, N, K = 64 + (i * 29) % 67, 64 + (i * 41) % 67, 8 + (i * 11) % 33
        if i in split_at:
            cases.append(Case(gpu, M, N, 1536, "rm", "t", "rm", beta=1.0))
            want["split_products"] += 1
            want["reduce_wgs"] += tiles((M, N), 128)
            want["nt_items"] += 2 * tiles((M, N), 128)
        else:
            cases.append(Case(gpu, M, N, K, "rm", "t", "rm", ep=EPS[i % 5], le="t"))
            want["nt_items"] += tiles((M, N), 128)
        M, K = 1 + (i * 13) % 41, 1 + (i * 59) % 300
        cases.append(Case(gpu, M, 1, K, "rm", "t", "rm", beta=float(i % 3 == 0)))
        want["gemv_wgs"] += -(-M // 4)
    assert plan(cases) == want
    run(cases)
    for name, sub in (("general", cases[0::3]), ("NT", cases[1::3]), ("gemv", cases[2::3])):
        check_all(sub, f"210-row table, {name}")


@pytest.mark.gpu
def test_k_sorted_order_list(gpu):
    """(i) 17 NT products of 1024 x 1024 = 1088 tiles: no slices, tiles walked through the K-sorted order list; two of
    them triangular at K = 1024, whose tiles carry K cuts of their own into the sort."""
    torch.manual_seed(9)
    ks = [8 + 17 * i + (i % 3) for i in range(15)]
    assert len(set(ks)) == 15 and min(ks) == 8 and max(ks) <= 264
    cases = [Case(gpu, 1024, 1024, K, "rm", "t", "rm") for K in ks]
    cases.insert(4, Case(gpu, 1024, 1024, 1024, "rm", "t", "rm", tri=ops.TRI_A_LOWER, cut=128))
    cases.insert(11, Case(gpu, 1024, 1024, 1024, "rm", "t", "rm", tri=ops.TRI_B_UPPER, cut=128))
    assert plan(cases) == {**dict.fromkeys(ops.GEMM_PLAN_KEYS, 0), "nt_items": 1088, "order_entries": 1088}
    run(cases)
    check_all(cases, "NT kernel, order list")
    first = [c.bits() for c in cases]
    for c in cases:
        c.reset()
    run(cases)
    for c, bits in zip(cases, first):
        assert torch.equal(c.bits(), bits), c.shape


@pytest.mark.gpu
def test_replay_with_the_table_resident(gpu):
    """(j) A plan's second run skips the table upload (CURV_GEMM_TABLE_RESIDENT); with new operand contents it must give
    the bits a fresh plan gives."""
    from curvature_amd import _lib
    torch.manual_seed(10)
    cases, want = mixed_call(gpu)
    assert plan(cases) == want
    p = ops.GemmPlan([c.job for c in cases])
    p.run()
    assert p._resident_on == _lib.stream_ptr()           # what run() turns into the flag next time
    check_all(cases, "plan, first run")
    for c in cases:
        if c.tri == ops.TRI_NONE:                         # (a triangular operand keeps its zeros and NaNs)
            c.A.mul_(-0.5).add_(0.25)
            c.B.mul_(1.5).sub_(0.125)
        c.reset()
        c.refresh()
    p.run()
    assert p._resident_on == _lib.stream_ptr()
    check_all(cases, "plan, replay")
    replay = [c.bits() for c in cases]
    for c in cases:
        c.reset()
    ops.GemmPlan([c.job for c in cases]).run()
    for c, bits in zip(cases, replay):
        assert torch.equal(c.bits(), bits), c.shape
