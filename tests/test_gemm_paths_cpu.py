"""The dispatch of curv_gemm_batched, pinned at its boundaries through curv_gemm_plan_info (host only, no GPU).

One call's descriptors are sorted into four work lists (csrc/gemm.hip: gemm_classify):

  general  gemm_f32_kernel          any layout; 128 tiles when M >= 96 and N >= 96, else 64
  NT       gemm_nt_kernel           a_cs == 1, b_rs == 1, M, N >= 64, K >= 8; K-sliced (+ gemm_nt_reduce_kernel) when the
                                    call has < 1024 NT tiles, K >= 1536 and the workspace has room; walked through a
                                    K-sorted order list when the call has >= 1024 tiles and more than one NT product
  small    gemm_nt_small_kernel     every product of the call in NT layout, K <= 1024, <= 64 tiles of 128
  gemv     gemv_rows_kernel         N == 1, NT layout, not TRI_B_UPPER

The descriptors carry fabricated non-null pointers: the query dereferences none, and the launch is only ever called
here with descriptors it refuses before any device work."""
import ctypes

import pytest

from curvature_amd import _lib, ops

PTR = 0x1000
ZERO = dict.fromkeys(ops.GEMM_PLAN_KEYS, 0)


def desc(M, N, K, layout="nt", **kw):
    """One descriptor with fabricated pointers.  layout "nt": K-contiguous rows of A and columns of B; "at": A read
    transposed (a_cs != 1), B row-major."""
    d = _lib.curv_gemm_desc()
    d.A = d.B = d.C = PTR
    d.M, d.N, d.K = M, N, K
    if layout == "nt":
        d.a_rs, d.a_cs, d.b_rs, d.b_cs = max(K, 1), 1, 1, max(K, 1)
    else:
        d.a_rs, d.a_cs, d.b_rs, d.b_cs = 1, max(M, 2), max(N, 1), 1
    d.c_rs, d.c_cs = max(N, 1), 1
    d.alpha = 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


GENERAL = (70, 50, 40, "at")          # a product that keeps a call from being small: 2 tiles of 64


def plan(descs, workspace="for"):
    """plan_info of the call; workspace "for": what GemmPlan allocates, "base": the table alone."""
    arr = (_lib.curv_gemm_desc * len(descs))(*descs)
    nbytes = None if workspace == "for" else int(_lib.lib().curv_gemm_workspace_bytes(len(descs)))
    return ops.gemm_plan_info(arr, nbytes)


def expect(**kw):
    return {**ZERO, **kw}


# ---------------------------------------------------------------- NT eligibility
@pytest.mark.parametrize("shape, nt", [((64, 64, 8), True), ((63, 64, 8), False), ((64, 63, 8), False), ((64, 64, 7), False)])
def test_nt_eligibility_edges(shape, nt):
    got = plan([desc(*GENERAL), desc(*shape)])
    assert got == (expect(tiles64=2, nt_items=1) if nt else expect(tiles64=3))


# ---------------------------------------------------------------- tile template
@pytest.mark.parametrize("M, N, want", [(96, 96, dict(tiles128=1)), (95, 96, dict(tiles64=4)), (96, 95, dict(tiles64=4)),
                                        (300, 200, dict(tiles128=6)), (300, 95, dict(tiles64=10))])
def test_tile_template_threshold(M, N, want):
    assert plan([desc(M, N, 16, "at")]) == expect(**want)


# ---------------------------------------------------------------- gemv
def test_one_column_products():
    assert plan([desc(*GENERAL), desc(10, 1, 20)]) == expect(tiles64=2, gemv_wgs=3)
    assert plan([desc(*GENERAL), desc(10, 1, 20, tri=ops.TRI_B_UPPER)]) == expect(tiles64=3)
    assert plan([desc(*GENERAL), desc(10, 1, 20, "at")]) == expect(tiles64=3)
    assert plan([desc(*GENERAL), desc(10, 1, 20, tri=ops.TRI_A_LOWER)]) == expect(tiles64=2, gemv_wgs=3)
    # rows are padded to whole workgroups of 4 per product
    assert plan([desc(*GENERAL), desc(5, 1, 20), desc(4, 1, 3), desc(1, 1, 0)]) == expect(tiles64=2, gemv_wgs=2 + 1 + 1)


# ---------------------------------------------------------------- small launch
def test_small_launch_k_limit():
    assert plan([desc(64, 64, 1024)]) == expect(small_blocks=4)
    assert plan([desc(64, 64, 1025)]) == expect(nt_items=1)
    # one long product moves its short companions too
    assert plan([desc(64, 64, 1024), desc(33, 5, 9)]) == expect(small_blocks=4 + 2)
    assert plan([desc(64, 64, 1025), desc(33, 5, 9)]) == expect(nt_items=1, tiles64=1)


def test_small_launch_tile_limit():
    assert plan([desc(1024, 1024, 16)]) == expect(small_blocks=1024)                   # 64 tiles of 128
    assert plan([desc(1024, 1024, 16), desc(1, 1, 16)]) == expect(nt_items=64, gemv_wgs=1)     # 65


def test_small_launch_block_limit_lies_behind_the_tile_limit():
    """The rule also caps a small call at 2048 blocks of 32 x 32.  A tile of 128 holds at most 16 such blocks, so a
    call within the 64-tile limit has at most 1024 of them: no call reaches 2048 / 2049 blocks while it is small, and
    the tile limit is the one that flips.  Calls of exactly 2048 and 2049 blocks are both past it."""
    assert plan([desc(2048, 1024, 16)]) == expect(nt_items=128)                        # 2048 blocks, 128 tiles
    assert plan([desc(2048, 1024, 16), desc(1, 1, 16)]) == expect(nt_items=128, gemv_wgs=1)    # 2049 blocks
    assert plan([desc(2048, 32, 16)] * 4) == expect(small_blocks=256)                  # thin products: 64 tiles hold 256 blocks
    assert plan([desc(2048, 32, 16)] * 5) == expect(tiles64=160)                       # 80 tiles (N < 64: the general kernel)


def test_one_product_outside_nt_layout_ends_the_small_launch():
    assert plan([desc(64, 64, 16), desc(20, 30, 5)]) == expect(small_blocks=4 + 1)
    assert plan([desc(64, 64, 16), desc(20, 30, 5, "at")]) == expect(nt_items=1, tiles64=1)
    assert plan([desc(64, 64, 16), desc(20, 30, 5), desc(0, 30, 5, "at")]) == expect(small_blocks=5)    # empty: not counted


# ---------------------------------------------------------------- K slicing
def test_slicing_k_threshold():
    assert plan([desc(128, 128, 1535)]) == expect(nt_items=1)
    assert plan([desc(128, 128, 1536)]) == expect(nt_items=2, split_products=1, reduce_wgs=1)


@pytest.mark.parametrize("K, slices", [(1536, 2), (1537, 3), (2304, 3), (2305, 4), (4609, 7)])
def test_slice_count(K, slices):
    assert plan([desc(128, 256, K)]) == expect(nt_items=2 * slices, split_products=1, reduce_wgs=2)


def test_slicing_tile_count_threshold():
    big = desc(128 * 33, 128 * 31, 1536)                                               # 1023 tiles
    assert plan([big]) == expect(nt_items=2 * 1023, split_products=1, reduce_wgs=1023)
    assert plan([big, desc(64, 64, 8)]) == expect(nt_items=1024, order_entries=1024)   # 1024: no slices


def test_no_slices_without_slab_room():
    assert plan([desc(128, 128, 1536)], workspace="base") == expect(nt_items=1)
    assert plan([desc(256, 128, 4609), desc(*GENERAL)], workspace="base") == expect(nt_items=2, tiles64=2)


def test_reduce_launch_covers_split_products_only():
    got = plan([desc(256, 128, 1536), desc(128, 128, 40), desc(*GENERAL), desc(130, 300, 2000)])
    assert got == expect(nt_items=2 * 2 + 1 + 6 * 3, split_products=2, reduce_wgs=2 + 6, tiles64=2)


# ---------------------------------------------------------------- order list
def test_order_list():
    big, one = desc(128 * 33, 128 * 31, 16), desc(128, 128, 16)                         # 1023 tiles, 1 tile
    assert plan([big, one]) == expect(nt_items=1024, order_entries=1024)
    assert plan([big, one], workspace="base") == expect(nt_items=1024)                 # nowhere to put it
    assert plan([desc(128 * 32, 128 * 32, 16)]) == expect(nt_items=1024)               # a single NT product
    assert plan([desc(128 * 33, 128 * 31 - 128, 16), one]) == expect(nt_items=991)     # fewer than 1024 tiles
    # products of the other lists do not count as NT products
    assert plan([desc(128 * 32, 128 * 32, 16), desc(*GENERAL), desc(9, 1, 5)]) == expect(nt_items=1024, tiles64=2, gemv_wgs=3)
    assert plan([big, one, desc(*GENERAL), desc(200, 200, 24)]) == expect(nt_items=1028, order_entries=1028, tiles64=2)


# ---------------------------------------------------------------- empty products
def test_empty_products_vanish():
    assert plan([desc(0, 5, 3), desc(5, 0, 3, "at")]) == ZERO
    assert plan([desc(0, 5, 3), desc(*GENERAL), desc(5, 0, 3)]) == expect(tiles64=2)
    assert plan([desc(0, 64, 16), desc(64, 64, 16)]) == expect(small_blocks=4)
    assert plan([desc(70, 50, 0, "at")]) == expect(tiles64=2)                          # K == 0 is a product: C = beta C


def test_no_descriptors_is_a_no_op():
    L = _lib.lib()
    out = (ctypes.c_longlong * _lib.GEMM_PLAN_FIELDS)(*([7] * _lib.GEMM_PLAN_FIELDS))
    assert L.curv_gemm_plan_info(None, 0, 0, out) == 0 and list(out) == [0] * _lib.GEMM_PLAN_FIELDS
    assert L.curv_gemm_batched(None, None, 0, None, 0) == 0
    assert ops.gemm_plan_info([]) == ZERO


# ---------------------------------------------------------------- refusals
BIG = 1 << 22
REFUSALS = [
    (dict(M=-1), "desc 1: negative shape"),
    (dict(K=-3), "desc 1: negative shape"),
    (dict(C=None), "desc 1: null pointer"),
    (dict(A=None), "desc 1: null pointer"),
    (dict(epilogue=5), "desc 1: bad epilogue"),
    (dict(epilogue=-1), "desc 1: bad epilogue"),
    (dict(epilogue=ops.EPI_MUL_E), "desc 1: epilogue needs E"),
    (dict(epilogue=ops.EPI_MUL_E_ADD_F, E=PTR), "desc 1: epilogue needs F"),
    (dict(tri=3), "desc 1: bad tri flag"),
    (dict(tri=-1), "desc 1: bad tri flag"),
    (dict(a_rs=-1), "desc 1: negative stride"),
    (dict(b_cs=-8), "desc 1: negative stride"),
    (dict(a_rs=1 << 25), "desc 1: operand stride too large"),
    (dict(b_rs=1 << 27), "desc 1: operand stride too large"),
    (dict(M=BIG, N=BIG), "too many tiles"),
]


@pytest.mark.parametrize("fields, message", REFUSALS)
def test_refusals_are_the_launch_s_own(fields, message):
    L = _lib.lib()
    bad = desc(*GENERAL)
    for k, v in fields.items():
        setattr(bad, k, v)
    arr = (_lib.curv_gemm_desc * 2)(desc(*GENERAL), bad)
    nbytes = 1 << 20
    out = (ctypes.c_longlong * _lib.GEMM_PLAN_FIELDS)()
    assert L.curv_gemm_plan_info(arr, 2, nbytes, out) == _lib.ERR_INVALID
    said = L.curv_last_error()
    assert message.encode() in said
    # the launch refuses in the same words, before any device work (the workspace pointer is never touched)
    assert L.curv_gemm_batched(None, arr, 2, PTR, nbytes) == _lib.ERR_INVALID
    assert L.curv_last_error() == said


def test_aligned_with_the_launch_on_workspace_and_arguments():
    L = _lib.lib()
    arr = (_lib.curv_gemm_desc * 1)(desc(*GENERAL))
    out = (ctypes.c_longlong * _lib.GEMM_PLAN_FIELDS)()
    need = int(L.curv_gemm_workspace_bytes(1))
    assert L.curv_gemm_plan_info(arr, 1, need - 1, out) == _lib.ERR_WORKSPACE
    said = L.curv_last_error()
    assert b"workspace too small" in said
    assert L.curv_gemm_batched(None, arr, 1, PTR, need - 1) == _lib.ERR_WORKSPACE and L.curv_last_error() == said
    assert L.curv_gemm_plan_info(arr, 1, need, out) == 0
    assert L.curv_gemm_plan_info(None, 1, need, out) == _lib.ERR_INVALID
    assert L.curv_gemm_plan_info(arr, 1, need, None) == _lib.ERR_INVALID
    with pytest.raises(RuntimeError, match="bad tri flag"):
        ops.gemm_plan_info((_lib.curv_gemm_desc * 1)(desc(70, 50, 40, "at", tri=9)))
