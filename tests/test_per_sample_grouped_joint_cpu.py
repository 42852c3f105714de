"""The joint covariance and the damping grid of grouped and depthwise convolutions, without a GPU: the
switch `ops.admit_grouped_joint` and what off means, the new symbols and descriptors of `_lib`, and the host side of
curv_persample_dw_project, curv_persample_dw_quad_grid_reduce and curv_persample_gram_reduce."""
import ctypes
import os
import shutil
import subprocess
from collections import OrderedDict

import pytest
import torch

from curvature_amd import _lib, ops
from curvature_amd.curvatures import KFAC, Diagonal


def model():
    torch.manual_seed(3)
    return torch.nn.Sequential(OrderedDict([("plain", torch.nn.Conv2d(2, 4, 3, padding=1)),
                                            ("grouped_one", torch.nn.Conv2d(4, 4, 3, groups=2)),
                                            ("flat", torch.nn.Flatten()), ("head", torch.nn.Linear(36, 3))]))


# ------------------------------------------------------------------------------------------------ the switch
def test_the_switch_is_off_by_default_and_returns_what_it_was():
    assert ops.per_sample_admits_grouped_joint() is False
    assert ops.admit_grouped_joint(True) is False
    try:
        assert ops.per_sample_admits_grouped_joint() is True
        assert ops.admit_grouped_joint() is True
        assert ops.per_sample_admits_groups() is False                       # independent of the other switches
        assert ops.per_sample_is_wide() is False
    finally:
        assert ops.admit_grouped_joint(False) is True
    assert ops.per_sample_admits_grouped_joint() is False


def refusals(net, text):
    """`stage_output`, `functional_variance_grid` of KFAC and Diagonal refuse the grouped layer of `net` with `text`."""
    for est in (Diagonal(net, per_sample=True) if ops.per_sample_admits_groups() else Diagonal(net), KFAC(net)):
        for layer in (net.plain, net.grouped_one, net.head):                 # (any state will do: the selection comes first)
            est.state[layer] = est.inv_state[layer] = torch.zeros(1)
        if getattr(est, "record", None) is None:
            est.record = {}
        with pytest.raises(NotImplementedError, match=text):
            est.stage_output(0, 2, inputs=True)
        est._decomposition = {}
        with pytest.raises(NotImplementedError, match=text):
            est.functional_variance_grid(torch.zeros(1, 2), [(1.0, 1.0)])
        for hook in getattr(est, "hooks", []):
            hook.remove()


def test_alone_the_switch_admits_nothing():
    was = ops.admit_grouped_joint(True)
    try:
        refusals(model(), r"layer 'grouped_one' is not supported \(grouped convolution \(groups=2\)\); select other layer types$")
    finally:
        ops.admit_grouped_joint(was)


def test_with_only_the_per_sample_switch_on_the_refusals_are_worded_as_before():
    was = ops.admit_grouped_per_sample(True)
    try:
        assert ops.per_sample_admits_grouped_joint() is False
        refusals(model(), r"layer 'grouped_one' is not supported \(grouped convolution \(groups=2\); Diagonal"
                          r"\(per_sample=True\) and functional_variance take it\); select other layer types$")
    finally:
        ops.admit_grouped_per_sample(was)


def test_with_both_switches_on_the_selection_passes_and_the_records_are_asked_for():
    was = ops.admit_grouped_per_sample(True), ops.admit_grouped_joint(True)
    try:
        net = model()
        for est in (Diagonal(net, per_sample=True), KFAC(net)):
            for layer in (net.plain, net.grouped_one, net.head):
                est.state[layer] = est.inv_state[layer] = torch.zeros(1)
            with pytest.raises(RuntimeError, match="no recorded forward/backward pass"):      # past the selection
                est.stage_output(0, 2, inputs=True)
            est._decomposition = {}
            with pytest.raises(RuntimeError, match="no recorded forward/backward pass"):
                est.functional_variance_grid(torch.zeros(1, 2), [(1.0, 1.0)])
            for hook in est.hooks:
                hook.remove()
        # what still refuses says who takes the layer now
        with pytest.raises(NotImplementedError, match="grouped_one.*linearised predictive of KFAC and Diagonal take it"):
            Diagonal(net)._per_sample_layers("X", "advice")
    finally:
        ops.admit_grouped_per_sample(was[0])
        ops.admit_grouped_joint(was[1])


def test_decompose_leaves_stacked_factors_out_unless_both_switches_are_on():
    net = model()
    for per_sample, joint in ((False, False), (True, False), (False, True)):
        was = ops.admit_grouped_per_sample(per_sample), ops.admit_grouped_joint(joint)
        try:
            est = KFAC(net)
            est.state[net.grouped_one] = [torch.zeros(2, 19, 19), torch.zeros(2, 2, 2)]      # stacked only: no solver call
            est.decompose()
            assert est._decomposition == {}
            for hook in est.hooks:
                hook.remove()
        finally:
            ops.admit_grouped_per_sample(was[0])
            ops.admit_grouped_joint(was[1])
    was = ops.admit_grouped_per_sample(True), ops.admit_grouped_joint(True)
    try:
        est = KFAC(net)
        est.state[net.grouped_one] = [torch.zeros(2, 19, 19), torch.zeros(2, 2, 2)]
        with pytest.raises(RuntimeError, match="no CPU fallback"):            # now the stacked factors go to the solver
            est.decompose()
        for hook in est.hooks:
            hook.remove()
    finally:
        ops.admit_grouped_per_sample(was[0])
        ops.admit_grouped_joint(was[1])


# ------------------------------------------------------------------------------------------------ ABI, host only
RECORD = dict(N=2, C=3, H=7, W=6, kh=3, kw=3, sh=2, sw=2, ph=1, pw=1, Ho=4, Wo=3, has_bias=1,
              x_sn=126, x_sc=42, x_sh=6, x_sw=1, x_elems=252, g_sn=36, g_sc=12, g_sh=3, g_sw=1, g_elems=72)


def desc(kind, **fields):
    d = kind()
    for key, value in {**RECORD, **fields}.items():
        setattr(d, key, value)
    return d


def grid_desc(shift=(0.5, 2.0), gain=(1.0, 0.25), **fields):
    d = desc(_lib.curv_persample_dw_grid_desc, v_rs=10, o_stride=1, o_hs=2, **fields)
    tables = (ctypes.c_float * max(len(shift), 1))(*shift), (ctypes.c_float * max(len(gain), 1))(*gain)
    d._tables = tables
    d.shift, d.gain = (ctypes.cast(t, ctypes.POINTER(ctypes.c_float)) for t in tables)
    d.Hn = fields.get("Hn", len(shift))
    return d


def test_new_symbols_and_descriptors_are_visible():
    L = _lib.lib()
    assert L.curv_version() == 12 == _lib.ABI_VERSION
    for name in ("curv_persample_dw_project", "curv_persample_dw_project_workspace_bytes",
                 "curv_persample_dw_project_plan_info", "curv_persample_dw_quad_grid_reduce",
                 "curv_persample_dw_quad_grid_workspace_bytes", "curv_persample_dw_quad_grid_plan_info",
                 "curv_persample_gram_reduce"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert ctypes.sizeof(_lib.curv_persample_dw_desc) == 240                  # the existing descriptor keeps its layout
    assert L.curv_persample_dw_project(None, None, 0, None, 0) == 0           # an empty call is a no-op
    assert L.curv_persample_dw_quad_grid_reduce(None, None, 0, None, 0) == 0
    assert L.curv_persample_gram_reduce(None, None, 0) == 0
    ops.per_sample_dw_project([])
    ops.per_sample_dw_quad_grid_reduce([])
    ops.per_sample_gram_reduce([])


def test_descriptors_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or shutil.which("hipcc")
    assert cc, "no host compiler"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    probes = [("curv_persample_dw_desc", ("N", "dst", "o_stride")),
              ("curv_persample_dw_project_desc", ("N", "has_bias", "T", "y", "y_ns")),
              ("curv_persample_dw_grid_desc", ("N", "first", "T", "V", "shift", "o_hs", "Hn")),
              ("curv_persample_gram_desc", ("Y", "o_rs", "N", "E", "alpha"))]
    prints = "".join(f'printf("%zu", sizeof({name})); ' +
                     "".join(f'printf(" %zu", (size_t)&(({name}*)0)->{field}); ' for field in fields) + 'printf("\\n"); '
                     for name, fields in probes)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include "curv_hip.h"\nint main(void) { ' + prints + 'return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-x", "c", "-I", os.path.join(root, "include"), str(probe), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    for (name, fields), line in zip(probes, lines):
        kind = getattr(_lib, name)
        assert [ctypes.sizeof(kind)] + [getattr(kind, f).offset for f in fields] == list(map(int, line.split())), name


def test_project_host_side():
    L = _lib.lib()
    kind = _lib.curv_persample_dw_project_desc
    arr = (kind * 1)(desc(kind, y_ns=30))
    assert L.curv_persample_dw_project_workspace_bytes(arr, 1) == 256         # 2 * 3 * 10 floats, 256-byte aligned
    flops, nbytes = (ctypes.c_longlong * 1)(), (ctypes.c_longlong * 1)()
    assert L.curv_persample_dw_project_plan_info(arr, 1, flops, nbytes) == 0
    assert flops[0] == 2 * 6 * 12 * 10 and nbytes[0] == 4 * 6 * (42 + 12) + 4 * 60
    job = ops.PerSampleDwProjectJob((2, 3, 7, 6), (2, 3, 4, 3), (3, 3), (2, 2), (1, 1), True)
    assert ops.per_sample_dw_project_plan_info([job]) == ([flops[0]], [nbytes[0]])
    assert ops.per_sample_dw_project_plan_info([]) == ([], [])
    for bad, text in ((dict(sh=0), "item 0"), (dict(Ho=5), "item 0: output 5x3"),
                      (dict(kh=8, kw=8, H=9, W=9, Ho=2, Wo=2), "more than 49 taps"), (dict(x_elems=251), "extent"),
                      (dict(y_ns=29), "y_ns 29 below C n_g = 30")):
        arr = (kind * 1)(desc(kind, **{"y_ns": 30, **bad}))
        assert L.curv_persample_dw_project_workspace_bytes(arr, 1) == 0, bad
        assert text in L.curv_last_error().decode(), (bad, L.curv_last_error())
        assert L.curv_persample_dw_project_plan_info(arr, 1, flops, nbytes) == _lib.ERR_INVALID
    arr = (kind * 2)(desc(kind, y_ns=30), desc(kind, y_ns=30, Wo=4))
    assert L.curv_persample_dw_project_workspace_bytes(arr, 2) == 0 and "item 1" in L.curv_last_error().decode()
    # the call itself refuses the same descriptors, and null records, before anything is launched
    assert L.curv_persample_dw_project(None, arr, 2, None, 0) == _lib.ERR_INVALID
    arr = (kind * 1)(desc(kind, y_ns=30))
    assert L.curv_persample_dw_project(None, arr, 1, None, 0) == _lib.ERR_INVALID
    assert "null record" in L.curv_last_error().decode()


def test_grid_host_side():
    L = _lib.lib()
    kind = _lib.curv_persample_dw_grid_desc
    arr = (kind * 1)(grid_desc())
    assert L.curv_persample_dw_quad_grid_workspace_bytes(arr, 1) == 256
    flops, nbytes = (ctypes.c_longlong * 1)(), (ctypes.c_longlong * 1)()
    assert L.curv_persample_dw_quad_grid_plan_info(arr, 1, flops, nbytes) == 0
    assert flops[0] == 2 * 6 * 12 * 10 + 2 * 60 * 2 and nbytes[0] == 4 * 6 * (42 + 12)
    job = ops.PerSampleDwGridJob((2, 3, 7, 6), (2, 3, 4, 3), (3, 3), (2, 2), (1, 1), True, shift=[0.5, 2.0], gain=[1.0, 0.25])
    assert ops.per_sample_dw_quad_grid_plan_info([job]) == ([flops[0]], [nbytes[0]])
    sixteen, seventeen = [1.0] * 16, [1.0] * 17
    assert L.curv_persample_dw_quad_grid_workspace_bytes((kind * 1)(grid_desc(sixteen, sixteen)), 1) == 256
    for d, text in ((grid_desc(Hn=0), "item 0: H 0"), (grid_desc(seventeen, seventeen), "item 0: H 17"),
                    (grid_desc((0.5, 0.0)), "grid point 1: shift 0"), (grid_desc((-1.0, 1.0)), "grid point 0: shift -1"),
                    (grid_desc((0.5, float("inf"))), "grid point 1"), (grid_desc(gain=(1.0, float("nan"))), "grid point 1"),
                    (grid_desc(kh=8, kw=8, H=9, W=9, Ho=2, Wo=2), "more than 49 taps"),
                    (grid_desc(Wo=4), "item 0: output 4x4")):
        arr = (kind * 1)(d)
        assert L.curv_persample_dw_quad_grid_workspace_bytes(arr, 1) == 0, text
        assert text in L.curv_last_error().decode(), (text, L.curv_last_error())
        assert L.curv_persample_dw_quad_grid_plan_info(arr, 1, flops, nbytes) == _lib.ERR_INVALID
    arr = (kind * 2)(grid_desc(), grid_desc((0.5, -2.0)))
    assert L.curv_persample_dw_quad_grid_workspace_bytes(arr, 2) == 0 and "item 1" in L.curv_last_error().decode()
    assert L.curv_persample_dw_quad_grid_reduce(None, arr, 2, None, 0) == _lib.ERR_INVALID
    for shift in ([], [1.0] * 17, [0.0], [float("nan")]):
        with pytest.raises(ValueError):
            ops.per_sample_dw_quad_grid_plan_info([ops.PerSampleDwGridJob((2, 3, 7, 6), (2, 3, 4, 3), (3, 3), (2, 2), (1, 1),
                                                                          True, shift=shift, gain=[1.0] * len(shift))])


def test_gram_refuses_invalid_items_before_anything_is_launched():
    L = _lib.lib()
    kind = _lib.curv_persample_gram_desc

    def gram(**fields):
        d = kind()
        for key, value in {**dict(Y=256, out=512, y_ks=60, y_ns=30, o_ns=9, o_rs=3, N=2, K=3, E=30, first=1, alpha=1.0),
                           **fields}.items():
            setattr(d, key, value)
        return d
    for bad, text in ((dict(K=0), "item 0: K 0"), (dict(K=17, o_rs=17, o_ns=289), "item 0: K 17"), (dict(E=0), "invalid sizes"),
                      (dict(N=0), "invalid sizes"), (dict(o_rs=2), "o_rs 2 below K = 3"), (dict(o_ns=8), "below K o_rs"),
                      (dict(y_ns=-1), "negative stride"), (dict(Y=None), "null"), (dict(out=514), "aligned")):
        assert L.curv_persample_gram_reduce(None, (kind * 1)(gram(**bad)), 1) == _lib.ERR_INVALID, bad
        assert text in L.curv_last_error().decode(), (bad, L.curv_last_error())
    # every item is checked before the first launch: a valid item in front of an invalid one changes nothing
    assert L.curv_persample_gram_reduce(None, (kind * 2)(gram(), gram(K=17)), 2) == _lib.ERR_INVALID
    assert "item 1" in L.curv_last_error().decode()


def test_jobs_refuse_cpu_tensors_and_wrong_shapes():
    x, g = torch.zeros(2, 3, 7, 6), torch.zeros(2, 3, 4, 3)
    geometry = ((3, 3), (2, 2), (1, 1), True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.per_sample_dw_project([ops.PerSampleDwProjectJob(x, g, *geometry, y=torch.zeros(2, 30))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.per_sample_dw_quad_grid_reduce([ops.PerSampleDwGridJob(x, g, *geometry, out=torch.zeros(1, 2), V=torch.ones(3, 10),
                                                                   shift=[1.0], gain=[1.0])])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.per_sample_gram_reduce([ops.PerSampleGramJob(torch.zeros(2, 3, 5), torch.zeros(3, 2, 2))])
    with pytest.raises(RuntimeError, match=r"\(N, C, H, W\)"):
        ops.per_sample_dw_project_plan_info([ops.PerSampleDwProjectJob((2, 3, 7, 6), (2, 4, 4, 3), (3, 3))])
