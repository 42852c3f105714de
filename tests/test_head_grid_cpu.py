"""Last-layer Laplace predictive over a grid of damping pairs without a GPU: the new symbols, the host-only queries of the
C ABI (curv_head_grid_*), the plan rule, and the refusals of `ops.head_grid`, `Curvature.head_terms_grid`,
`evaluate.last_layer_predictive_grid` and `evaluate.tune_last_layer` that need no device."""
import ctypes

import pytest
import torch

from curvature_amd import _lib, ops
from curvature_amd.curvatures import EFB, INF, KFAC, BlockDiagonal, Diagonal, HeadGridTerms
from curvature_amd.evaluate import last_layer_predictive_grid, tune_glm, tune_last_layer

NAMES = ("curv_head_grid_workspace_bytes", "curv_head_grid_plan_flops", "curv_head_grid")
WGS_TARGET, MIN_STEPS, MAX = 256, 4, 16        # the plan of include/curv_hip.h (curv_head_grid, "Plan")


def small_model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3, padding=1), torch.nn.Flatten(), torch.nn.Linear(75, 4))


def grid_desc(N=32, K=100, n=300, H=3, dense=True, both=False, neither=False, y_rs=None, t_rs=None, shift=None, gain=None,
              tables=True):
    """One item; the device pointers are non-null addresses the host queries never read.  Returns (array, keep-alive)."""
    arr = (_lib.curv_head_grid_desc * 1)()
    d = arr[0]
    d.N, d.K, d.n, d.H = N, K, n, H
    d.Y, d.out = 128, 256
    if (dense or both) and not neither:
        d.T = 512
    if (not dense or both) and not neither:
        d.u, d.v = 768, 1024
    d.y_rs = n if y_rs is None else y_rs
    d.t_rs = n if t_rs is None else t_rs
    count = max(H, 1)
    shift = [0.5 + h for h in range(count)] if shift is None else shift
    gain = [1.0 / (1 + h) for h in range(count)] if gain is None else gain
    keep = ((ctypes.c_float * len(shift))(*shift), (ctypes.c_float * len(gain))(*gain))
    if tables:
        d.shift = ctypes.cast(keep[0], ctypes.POINTER(ctypes.c_float))
        d.gain = ctypes.cast(keep[1], ctypes.POINTER(ctypes.c_float))
    return arr, keep


def chunks_of(N, K, n):
    """Waves per block and group of pairs, from the item's own N, K and n (the rule the header states)."""
    steps, blocks = -(-n // 32), -(-N // 32) * -(-K // 32)
    per = max(MIN_STEPS, -(-steps // -(-WGS_TARGET // blocks)))
    return -(-steps // per)


def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
    assert L.curv_version() == 12 == _lib.ABI_VERSION
    for name in ("HeadGridJob", "head_grid", "head_grid_plan_flops", "HEAD_GRID_MAX"):
        assert hasattr(ops, name)
    assert ops.HEAD_GRID_MAX == _lib.HEAD_GRID_MAX == MAX
    header = open(_lib.INCLUDE + "/curv_hip.h").read()
    assert f"#define CURV_HEAD_GRID_MAX {MAX}" in header
    assert "head_grid.hip" in _lib.SOURCES
    assert callable(last_layer_predictive_grid) and callable(tune_last_layer)
    assert HeadGridTerms._fields == ("M", "d2", "variance")
    for est in (KFAC, EFB, Diagonal):
        assert callable(est.head_terms_grid)


def test_descriptor_mirrors_the_header():
    """5 device pointers, 2 host pointers, 2 strides, 4 ints: no hidden padding."""
    assert ctypes.sizeof(_lib.curv_head_grid_desc) == 5 * 8 + 2 * 8 + 2 * 8 + 4 * 4
    assert [f[0] for f in _lib.curv_head_grid_desc._fields_] == ["Y", "u", "v", "T", "out", "shift", "gain", "y_rs", "t_rs",
                                                                 "N", "K", "n", "H"]
    assert _lib.curv_head_grid_desc.H.offset == 84


def test_empty_calls_are_noops():
    L = _lib.lib()
    assert L.curv_head_grid_workspace_bytes(None, 0) == 0
    assert L.curv_head_grid_plan_flops(None, 0, None) == 0
    assert L.curv_head_grid(None, None, 0, None, 0) == 0
    ops.head_grid([])
    assert ops.head_grid_plan_flops([]) == []


@pytest.mark.parametrize("kw", [dict(), dict(N=1, K=1, n=1, H=1), dict(N=32, K=1000, n=2049, H=16), dict(N=4, K=40, n=2049),
                                dict(N=1, K=1, n=128), dict(N=1, K=1, n=129), dict(N=300, K=300, n=4000),
                                dict(y_rs=303, t_rs=301), dict(dense=False), dict(dense=False, N=32, K=1000, n=2049, H=16)],
                         ids=["plain", "ones", "bench", "issue_shape", "one_chunk", "two_chunks", "many_blocks", "strided",
                              "separable", "separable_bench"])
def test_host_queries(kw):
    """Scratch: 16 N K floats per chunk - whatever H - where the sum over i is cut into chunks, and zero, without an error
    text, where it is not and for a separable item.  FLOPs of one pair: whole 32 x 32 x 32 steps."""
    L = _lib.lib()
    arr, keep = grid_desc(**kw)
    d = arr[0]
    chunks = chunks_of(d.N, d.K, d.n) if d.T else 1
    need = L.curv_head_grid_workspace_bytes(arr, 1)
    if chunks > 1:
        assert 4 * chunks * MAX * d.N * d.K <= need < 4 * chunks * MAX * d.N * d.K + 256
    else:
        assert need == 0
    out = (ctypes.c_longlong * 1)()
    assert L.curv_head_grid_plan_flops(arr, 1, out) == 0
    if d.T:
        assert out[0] == 2 * 32 ** 3 * -(-d.n // 32) * -(-d.N // 32) * -(-d.K // 32)
        assert out[0] >= 2 * d.N * d.K * d.n
    else:
        assert out[0] == 0
    # past the plan, the call refuses the missing workspace (chunks) - nothing is launched without a GPU
    if chunks > 1:
        assert L.curv_head_grid(None, arr, 1, None, 0) == _lib.ERR_WORKSPACE


def test_the_chunk_rule():
    assert chunks_of(1, 1, 128) == 1 and chunks_of(1, 1, 129) == 2 and chunks_of(32, 1000, 2049) == 8
    assert chunks_of(4, 40, 2049) == 17 and chunks_of(33, 33, 145) == 2 and chunks_of(3000, 3000, 4000) == 1
    L = _lib.lib()
    assert L.curv_head_grid_workspace_bytes(grid_desc(N=1, K=1, n=128)[0], 1) == 0
    assert L.curv_head_grid_workspace_bytes(grid_desc(N=1, K=1, n=129)[0], 1) == 256


def test_plan_does_not_depend_on_the_number_of_pairs_nor_on_the_other_items():
    L = _lib.lib()
    kws = [dict(N=3, K=5, n=1000), dict(N=2000, K=160, n=100), dict(N=70, K=1, n=4096, dense=False),
           dict(N=32, K=1000, n=2049), dict(N=5, K=7, n=145, y_rs=150)]
    for H in (1, 3, 16):
        items = [grid_desc(H=H, **kw) for kw in kws]
        both = (_lib.curv_head_grid_desc * len(kws))()
        alone, flops = [], []
        for k, (one, _) in enumerate(items):
            ctypes.memmove(ctypes.addressof(both[k]), one, ctypes.sizeof(_lib.curv_head_grid_desc))
            alone.append(L.curv_head_grid_workspace_bytes(one, 1))
            out = (ctypes.c_longlong * 1)()
            assert L.curv_head_grid_plan_flops(one, 1, out) == 0
            flops.append(out[0])
        assert alone[0] > 0 and alone[1] == 0 and alone[2] == 0 and alone[3] > 0 and alone[4] > 0
        assert L.curv_head_grid_workspace_bytes(both, len(kws)) == sum(alone)
        out = (ctypes.c_longlong * len(kws))()
        assert L.curv_head_grid_plan_flops(both, len(kws), out) == 0
        assert list(out) == flops
        if H == 1:
            first = (alone, flops)
        assert (alone, flops) == first
    jobs = [ops.HeadGridJob(None, None, None, None, None, [1.0] * H, [1.0] * H, N=32, K=1000, n=2049, separable=False)
            for H in (1, 16)]
    assert ops.head_grid_plan_flops(jobs) == [2 * 32 ** 3 * 65 * 32] * 2
    assert ops.head_grid_plan_flops([ops.HeadGridJob(None, None, None, None, None, [1.0], [1.0], N=32, K=1000, n=2049,
                                                     separable=True)]) == [0]


@pytest.mark.parametrize("kw", [dict(H=0), dict(H=17), dict(shift=[1.0, 0.0, 1.0]), dict(shift=[1.0, -2.0, 1.0]),
                                dict(shift=[1.0, float("inf"), 1.0]), dict(shift=[float("nan"), 1.0, 1.0]),
                                dict(gain=[1.0, 1.0, float("inf")]), dict(gain=[float("nan"), 1.0, 1.0]),
                                dict(both=True), dict(neither=True), dict(N=0), dict(K=0), dict(n=0), dict(y_rs=299),
                                dict(t_rs=299), dict(N=1 << 16, K=1 << 12, n=8), dict(N=1 << 20, n=1 << 11),
                                dict(K=1 << 20, n=1 << 11), dict(tables=False)],
                         ids=["H0", "H17", "shift_zero", "shift_negative", "shift_inf", "shift_nan", "gain_inf", "gain_nan",
                              "both_forms", "no_form", "N0", "K0", "n0", "y_rs", "t_rs", "out_too_large", "Y_too_large",
                              "T_too_large", "no_tables"])
def test_invalid_items_are_refused(kw):
    """... with the item's index in the text, also behind valid items, and before anything is launched."""
    L = _lib.lib()
    arr, keep = grid_desc(**kw)
    assert L.curv_head_grid_workspace_bytes(arr, 1) == 0
    assert b"item 0" in L.curv_last_error()
    assert L.curv_head_grid_plan_flops(arr, 1, (ctypes.c_longlong * 1)()) == _lib.ERR_INVALID
    assert L.curv_head_grid(None, arr, 1, None, 0) == _lib.ERR_INVALID
    assert b"item 0" in L.curv_last_error()
    three = (_lib.curv_head_grid_desc * 3)()
    others = (grid_desc(), grid_desc(K=7, n=3, dense=False))
    for k, one in enumerate((others[0][0], others[1][0], arr)):
        ctypes.memmove(ctypes.addressof(three[k]), one, ctypes.sizeof(_lib.curv_head_grid_desc))
    assert L.curv_head_grid(None, three, 3, None, 0) == _lib.ERR_INVALID
    assert b"item 2" in L.curv_last_error()


def test_ops_refuses_invalid_jobs_with_the_item_named():
    Y, T, u, v = torch.zeros(2, 5), torch.zeros(3, 5), torch.zeros(3), torch.zeros(5)

    def job(Y=Y, u=None, v=None, T=T, H=2, shift=None, gain=None, out=None):
        out = torch.zeros(H, 2, 3) if out is None else out
        return ops.HeadGridJob(Y, u, v, T, out, [1.0] * H if shift is None else shift, [1.0] * H if gain is None else gain)
    good = job()
    for bad, match in ((job(H=0), "item 1: 0 shifts"), (job(H=17), "item 1: 17 shifts"),
                       (job(gain=[1.0]), "item 1: 2 shifts and 1 gains"),
                       (job(shift=[1.0, 0.0]), "item 1: pair 1: shift 0.0"),
                       (job(shift=[float("inf"), 1.0]), "item 1: pair 0: shift inf"),
                       (job(gain=[1.0, float("nan")]), "item 1: pair 1: .*gain nan")):
        with pytest.raises(ValueError, match=match):
            ops.head_grid([good, bad])
    for bad in (job(u=u, v=v), job(T=None), job(u=u, T=None), job(v=v)):
        with pytest.raises(RuntimeError, match="item 1: give the spectrum as u and v .* or as T"):
            ops.head_grid([good, bad])
    # CPU tensors and other dtypes are refused before shapes are looked at, and before the device is touched
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.head_grid([good])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.head_grid([job(u=u, v=v, T=None)])


def test_estimator_refusals():
    model = small_model()
    head, conv = model[2], model[0]
    x, pairs = torch.zeros(3, 75), [(1.0, 50.0), (2.0, 10.0)]
    est = KFAC(model)
    with pytest.raises(AssertionError, match="State dict is empty"):
        est.head_terms_grid(head, x, pairs)
    est.state[head] = (torch.eye(76), torch.eye(4))
    est.state[conv] = (torch.eye(19), torch.eye(3))
    with pytest.raises(NotImplementedError, match=r"KFAC.head_terms_grid: layer '0'.*nn.Linear.*Conv2d"):
        est.head_terms_grid(conv, x, pairs)
    with pytest.raises(RuntimeError, match=r"KFAC.head_terms_grid: layer '2'.*call decompose\(\) after the last update\(\)"):
        est.head_terms_grid(head, x, pairs)
    est._decomposition = {head: (torch.eye(4), torch.eye(76), torch.ones(4), torch.ones(76))}
    with pytest.raises(RuntimeError, match=r"KFAC.head_terms_grid: layer '2' got CPU features \(no CPU fallback\)"):
        est.head_terms_grid(head, x, pairs)
    est.state[head] = (torch.ones(2, 38, 38), torch.ones(2, 2, 2))
    with pytest.raises(NotImplementedError, match=r"KFAC.head_terms_grid: layer '2': stacked \(grouped\) factors"):
        est.head_terms_grid(head, x, pairs)
    est.state[head] = (torch.eye(76), torch.eye(4))
    del est.state[head]
    with pytest.raises(NotImplementedError, match=r"KFAC.head_terms_grid: layer '2': KFAC holds no state for this layer"):
        est.head_terms_grid(head, x, pairs)
    est.state[head] = (torch.eye(76), torch.eye(4))

    # the pairs, named by index, before anything else
    for bad, match in (([], "no damping pairs"), ([(1.0, 50.0), (1.0,)], "pair 1 is not an"),
                       ([(1.0, 50.0), (0.0, 1.0)], "pair 1 .*finite and > 0"),
                       ([(float("inf"), 1.0)], "pair 0 .*finite and > 0"), ([(1.0, [1.0, -1.0])], "pair 0 .*finite and > 0")):
        with pytest.raises(ValueError, match=f"KFAC.head_terms_grid: {match}"):
            est.head_terms_grid(head, x, bad)

    diag = Diagonal(model)
    diag.state[head] = torch.ones(4, 76)
    with pytest.raises(RuntimeError, match=r"Diagonal.head_terms_grid: layer '2' got CPU features"):
        est_x = diag.head_terms_grid(head, x, pairs)
        del est_x
    diag.state[head] = torch.ones(4 * 76)
    with pytest.raises(NotImplementedError, match=r"Diagonal.head_terms_grid: layer '2': the state \(304,\) is not one"):
        diag.head_terms_grid(head, x, pairs)

    block = BlockDiagonal(model)
    block.state[head] = torch.eye(4 * 76)
    with pytest.raises(NotImplementedError, match=r"BlockDiagonal.head_terms_grid: layer '2'.*BlockDiagonal"):
        block.head_terms_grid(head, x, pairs)
    assert INF._head_terms.__qualname__ == "Curvature._head_terms"          # (INF: the same refusal)
    inf = object.__new__(INF)
    inf.model, inf.shard, inf.state = model, None, {head: torch.ones(1)}
    with pytest.raises(NotImplementedError, match=r"INF.head_terms_grid: layer '2'.*INF"):
        inf.head_terms_grid(head, x, pairs)

    from curvature_amd.curvatures import AttentionProjection
    torch.manual_seed(0)
    attention = torch.nn.MultiheadAttention(8, 2)
    projection = AttentionProjection.of(attention)[0]
    with pytest.raises(NotImplementedError, match=r"KFAC.head_terms_grid: .*attention projection"):
        est.head_terms_grid(projection, x, pairs)

    class World:
        world, rank, force_collective = 2, 0, False

        def owns(self, index):
            return True
    est.shard = World()
    with pytest.raises(NotImplementedError, match=r"KFAC.head_terms_grid: layer '2'.*sharded"):
        est.head_terms_grid(head, x, pairs)


def test_head_terms_keeps_its_refusals():
    """The checks `head_terms` now shares with `head_terms_grid` read as before."""
    model = small_model()
    head = model[2]
    est = KFAC(model)
    with pytest.raises(AssertionError, match="Inverse state dict is empty. Did you call 'invert' prior to this?"):
        est.head_terms(head, torch.zeros(3, 75))
    est.inv_state[model[0]] = (torch.eye(19), torch.eye(3))
    with pytest.raises(NotImplementedError, match=r"^KFAC.head_terms: layer '2': KFAC holds no inverse state for this layer$"):
        est.head_terms(head, torch.zeros(3, 75))
    est.inv_state[head] = (torch.eye(76), torch.eye(4))
    with pytest.raises(RuntimeError, match=r"^curvature_amd runs on MI355X only: KFAC.head_terms: layer '2' got CPU features"):
        est.head_terms(head, torch.zeros(3, 75))


def test_driver_refusals():
    model = small_model()
    x, pairs = torch.zeros(3, 2, 5, 5), [(1.0, 50.0)]
    data = [(x, torch.zeros(3, dtype=torch.long))]
    with pytest.raises(RuntimeError, match="last_layer_predictive_grid got a CPU model or batch \\(no CPU fallback\\)"):
        last_layer_predictive_grid(model, KFAC(model), x, pairs)
    for predictive in ("probit", "mc"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            tune_last_layer(model, data, KFAC(model), pairs, predictive=predictive)
    with pytest.raises(ValueError, match="last_layer_predictive_grid: predictive must be 'probit' or 'mc', got 'other'"):
        last_layer_predictive_grid(model, KFAC(model), x, pairs, predictive="other")
    with pytest.raises(ValueError, match="tune_last_layer: predictive must be 'probit' or 'mc', got 'other'"):
        tune_last_layer(model, [], KFAC(model), pairs, predictive="other")
    with pytest.raises(ValueError, match="last_layer_predictive_grid: samples must be at least 1, got 0"):
        last_layer_predictive_grid(model, KFAC(model), x, pairs, predictive="mc", samples=0)
    for driver in (lambda bad: last_layer_predictive_grid(model, KFAC(model), x, bad),
                   lambda bad: tune_last_layer(model, data, KFAC(model), bad)):
        with pytest.raises(ValueError, match="KFAC.head_terms_grid: pair 1 .*finite and > 0"):
            driver([(1.0, 50.0), (1.0, -3.0)])
        with pytest.raises(ValueError, match="KFAC.head_terms_grid: no damping pairs"):
            driver([])


def test_an_empty_dataset_is_refused_by_name():
    model = small_model()
    with pytest.raises(ValueError, match="^tune_last_layer: the dataset is empty$"):
        tune_last_layer(model, [], KFAC(model), [(1.0, 50.0)])
    with pytest.raises(ValueError, match="^tune_glm: the dataset is empty$"):
        tune_glm(model, [], KFAC(model), [(1.0, 50.0)])
