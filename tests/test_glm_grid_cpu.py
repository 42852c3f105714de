"""GLM predictive over a grid of damping pairs, without a GPU: the new symbols, the host-only queries of the C ABI
(curv_persample_quad_grid_*) and the error paths of `ops.per_sample_quad_grid_reduce`,
`Curvature.functional_variance_grid`, `evaluate.glm_predictive_grid` and `evaluate.tune_glm`."""
import ctypes

import pytest
import torch

from curvature_amd import _lib, ops
from curvature_amd.curvatures import INF, KFAC, BlockDiagonal, Diagonal
from curvature_amd.evaluate import glm_predictive_grid, tune_glm

NAMES = ("curv_persample_quad_grid_workspace_bytes", "curv_persample_quad_grid_plan_flops",
         "curv_persample_quad_grid_reduce")


def small_model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3, padding=1), torch.nn.Flatten(), torch.nn.Linear(75, 4))


def grid_desc(S=5, M=130, Nc=150, L=37, H=3, shift=None, gain=None, dense=False, a_rs=None, b_rs=None, a_ns=None,
              b_ns=None, v_rs=None, o_stride=1, o_hs=None):
    """One item; the device pointers are non-null addresses the host queries never read, `shift` and `gain` real host
    arrays (kept alive on the returned array)."""
    arr = (_lib.curv_persample_grid_desc * 1)()
    d = arr[0]
    d.S, d.M, d.Nc, d.L, d.H = S, M, Nc, L, H
    Lp = (L + 3) // 4 * 4
    d.a_rs = Lp if a_rs is None else a_rs
    d.b_rs = Lp if b_rs is None else b_rs
    d.a_ns = M * Lp if a_ns is None else a_ns
    d.b_ns = Nc * Lp if b_ns is None else b_ns
    d.A, d.B, d.out = 256, 512, 768
    if dense:
        d.V = 1024
    else:
        d.u, d.v = 1024, 2048
    d.v_rs = Nc if v_rs is None else v_rs
    d.o_stride, d.o_hs = o_stride, S * o_stride if o_hs is None else o_hs
    n = max(H, 1)
    shift = [0.5 + h for h in range(n)] if shift is None else shift
    gain = [1.0] * n if gain is None else gain
    arr.tables = ((ctypes.c_float * len(shift))(*shift), (ctypes.c_float * len(gain))(*gain))
    d.shift = ctypes.cast(arr.tables[0], ctypes.POINTER(ctypes.c_float))
    d.gain = ctypes.cast(arr.tables[1], ctypes.POINTER(ctypes.c_float))
    return arr


def tiles_of(M, Nc):
    """Output tiles, from the item's own sizes (the rule of curv_persample_plan_flops in the header): 128 x 128, or
    64 x 128 with the smaller side as the 64 where min(M, Nc) <= 64."""
    if min(M, Nc) <= 64:
        return -(-max(M, Nc) // 128) if M > 64 else -(-Nc // 128)
    return -(-M // 128) * -(-Nc // 128)


def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert L.curv_version() == 12                                    # additive: the ABI version stays
    assert ops.PERSAMPLE_GRID_MAX == _lib.PERSAMPLE_GRID_MAX == 16
    for name in ("PerSampleGridJob", "per_sample_quad_grid_reduce", "per_sample_quad_grid_plan_flops"):
        assert hasattr(ops, name)
    assert callable(glm_predictive_grid) and callable(tune_glm)
    assert callable(KFAC.decompose) and callable(KFAC.functional_variance_grid)


def test_empty_calls_are_noops():
    L = _lib.lib()
    assert L.curv_persample_quad_grid_workspace_bytes(None, 0) == 0
    assert L.curv_persample_quad_grid_plan_flops(None, 0, None) == 0
    assert L.curv_persample_quad_grid_reduce(None, None, 0, None, 0) == 0
    ops.per_sample_quad_grid_reduce([])
    assert ops.per_sample_quad_grid_plan_flops([]) == []


@pytest.mark.parametrize("kw", [dict(), dict(H=1), dict(H=16, dense=True), dict(S=9, M=6, Nc=151, L=100),
                                dict(S=33, M=150, Nc=16, L=1, H=16), dict(S=200, M=16, Nc=26, L=5, dense=True, v_rs=29),
                                dict(o_stride=3, o_hs=700)],
                         ids=["plain", "H1", "H16_dense", "half", "half_swapped", "dense_strided", "strided_out"])
def test_host_queries(kw):
    """Scratch: H floats per output tile and sample.  FLOPs: those of the plain quadratic reduction of the same
    operands, whatever H - at least the algorithmic 2 S M Nc L."""
    L = _lib.lib()
    arr = grid_desc(**kw)
    d = arr[0]
    need = L.curv_persample_quad_grid_workspace_bytes(arr, 1)
    floats = tiles_of(d.M, d.Nc) * d.S * d.H
    assert need == (4 * floats + 255) // 256 * 256
    out = (ctypes.c_longlong * 1)()
    assert L.curv_persample_quad_grid_plan_flops(arr, 1, out) == 0
    assert out[0] >= 2 * d.S * d.M * d.Nc * d.L
    quad = ops.PerSampleQuadJob(None, None, None, None, d.S, d.M, d.Nc, d.L, d.a_ns, d.a_rs, d.b_ns, d.b_rs)
    assert out[0] == ops.per_sample_quad_plan_flops([quad])[0]
    # past the plan, the call refuses the missing workspace - nothing is launched without a GPU
    assert L.curv_persample_quad_grid_reduce(None, arr, 1, None, 0) == _lib.ERR_WORKSPACE


@pytest.mark.parametrize("kw", [dict(H=0), dict(H=17, shift=[1.0] * 17, gain=[1.0] * 17), dict(shift=[1.0, 0.0, 1.0]),
                                dict(shift=[1.0, 1.0, -0.5]), dict(shift=[float("nan"), 1.0, 1.0]),
                                dict(shift=[1.0, float("inf"), 1.0]), dict(gain=[1.0, float("nan"), 1.0]),
                                dict(a_rs=42), dict(b_ns=150 * 40 + 2), dict(dense=True, v_rs=149), dict(o_stride=0),
                                dict(o_hs=0), dict(S=0), dict(a_rs=36)],
                         ids=["H0", "H17", "shift_zero", "shift_negative", "shift_nan", "shift_inf", "gain_nan",
                              "a_rs_misaligned", "b_ns_misaligned", "v_rs_below_Nc", "o_stride", "o_hs", "S0",
                              "a_rs_below_L"])
def test_invalid_items_are_refused(kw):
    L = _lib.lib()
    arr = grid_desc(**kw)
    assert L.curv_persample_quad_grid_workspace_bytes(arr, 1) == 0
    assert b"item 0" in L.curv_last_error()
    assert L.curv_persample_quad_grid_plan_flops(arr, 1, (ctypes.c_longlong * 1)()) == _lib.ERR_INVALID
    assert L.curv_persample_quad_grid_reduce(None, arr, 1, None, 0) == _lib.ERR_INVALID
    assert b"item 0" in L.curv_last_error()


def test_the_second_item_is_named():
    L = _lib.lib()
    both = (_lib.curv_persample_grid_desc * 2)()
    good, bad = grid_desc(), grid_desc(shift=[1.0, -1.0, 1.0])
    for k, one in enumerate((good, bad)):
        ctypes.memmove(ctypes.addressof(both[k]), one, ctypes.sizeof(_lib.curv_persample_grid_desc))
    assert L.curv_persample_quad_grid_workspace_bytes(both, 2) == 0
    assert b"item 1" in L.curv_last_error() and b"grid point 1" in L.curv_last_error()


def test_plan_follows_from_the_items_own_sizes():
    """The scratch and the FLOPs of an item are the same alone and beside others."""
    L = _lib.lib()
    kws = [dict(), dict(S=9, M=6, Nc=151, L=100, H=16), dict(S=200, M=16, Nc=26, L=5, H=1, dense=True)]
    ones = [grid_desc(**kw) for kw in kws]
    both = (_lib.curv_persample_grid_desc * len(kws))()
    alone, flops = [], []
    for k, one in enumerate(ones):
        ctypes.memmove(ctypes.addressof(both[k]), one, ctypes.sizeof(_lib.curv_persample_grid_desc))
        alone.append(L.curv_persample_quad_grid_workspace_bytes(one, 1))
        out = (ctypes.c_longlong * 1)()
        assert L.curv_persample_quad_grid_plan_flops(one, 1, out) == 0
        flops.append(out[0])
    assert all(a > 0 for a in alone)
    assert L.curv_persample_quad_grid_workspace_bytes(both, len(kws)) == sum(alone)
    out = (ctypes.c_longlong * len(kws))()
    assert L.curv_persample_quad_grid_plan_flops(both, len(kws), out) == 0
    assert list(out) == flops


def test_plan_flops_through_ops():
    job = ops.PerSampleGridJob(None, None, None, None, None, None, [0.1, 1.0], [1.0, 0.5], 5, 130, 150, 37, 5200, 40,
                               6000, 40)
    # 2 x 2 full tiles, L = 37 padded to two stages of 32
    assert ops.per_sample_quad_grid_plan_flops([job]) == [2 * 4 * 128 * 128 * 5 * 64]


def test_bad_grids_are_refused_by_ops():
    sizes = (5, 130, 150, 37, 5200, 40, 6000, 40)
    for shift, gain in (([], []), ([1.0] * 17, [1.0] * 17), ([1.0, 2.0], [1.0]), ([0.0], [1.0]), ([-1.0], [1.0]),
                        ([float("nan")], [1.0]), ([1.0], [float("inf")])):
        with pytest.raises(ValueError, match="grid point"):
            ops.per_sample_quad_grid_plan_flops([ops.PerSampleGridJob(None, None, None, None, None, None, shift, gain, *sizes)])
    with pytest.raises(ValueError, match="alpha"):
        ops.PerSampleGridJob(None, None, None, None, None, None, [1.0], [1.0], *sizes, alpha=2.0)


def test_cpu_tensors_are_refused():
    A, B = torch.zeros(2, 3, 4), torch.zeros(2, 5, 4)
    job = ops.PerSampleGridJob(A, B, torch.ones(3), torch.ones(5), None, torch.zeros(2, 2), [1.0, 2.0], [1.0, 1.0],
                               2, 3, 5, 4, 12, 4, 20, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.per_sample_quad_grid_reduce([job])
    model = small_model()
    x = torch.zeros(3, 2, 5, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        glm_predictive_grid(model, KFAC(model), x, [(1.0, 1.0)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tune_glm(model, [(x, torch.zeros(3, dtype=torch.long))], KFAC(model), [(1.0, 1.0)])


def test_both_weight_forms_at_once_are_refused():
    A, B = torch.zeros(2, 3, 4), torch.zeros(2, 5, 4)
    for u, v, V in ((torch.ones(3), torch.ones(5), torch.ones(3, 5)), (None, None, None), (torch.ones(3), None, None)):
        job = ops.PerSampleGridJob(A, B, u, v, V, torch.zeros(1, 2), [1.0], [1.0], 2, 3, 5, 4, 12, 4, 20, 4)
        with pytest.raises(RuntimeError, match="separable"):
            ops.per_sample_quad_grid_reduce([job])


@pytest.mark.parametrize("pair", [(0.0, 1.0), (-1.0, 1.0), (1.0, 0.0), (1.0, -2.0), (float("nan"), 1.0),
                                  (1.0, float("inf")), ([1.0, 0.0], [1.0, 1.0])])
@pytest.mark.parametrize("cls", [KFAC, Diagonal])
def test_damping_must_be_positive(cls, pair):
    """add <= 0 or multiply <= 0 (or a non-finite value) is a ValueError that names the pair, before anything else."""
    model = small_model()
    with pytest.raises(ValueError, match="pair 1"):
        cls(model).functional_variance_grid(torch.zeros(2, 3), [(1.0, 1.0), pair])
    with pytest.raises(ValueError, match="no damping pairs"):
        cls(model).functional_variance_grid(torch.zeros(0, 3), [])


def test_estimators_without_a_glm_predictive():
    model = small_model()
    with pytest.raises(NotImplementedError, match="BlockDiagonal"):
        BlockDiagonal(model).functional_variance_grid(torch.zeros(1, 3), [(1.0, 1.0)])
    inf = INF.__new__(INF)                         # (its constructor wants the factors of a whole pipeline)
    with pytest.raises(NotImplementedError, match="INF"):
        inf.functional_variance_grid(torch.zeros(1, 3), [(1.0, 1.0)])


def test_kfac_needs_a_decomposition():
    model = small_model()
    with pytest.raises(RuntimeError, match="decompose"):
        KFAC(model).functional_variance_grid(torch.zeros(1, 3), [(1.0, 1.0)])
