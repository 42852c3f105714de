"""`curv_logsum_grid` and the evidence methods without a GPU: the descriptor against the header, the host-side checks of
the entry point, the workspace size, and the refusal of bad `hypers` before anything touches a device."""
import ctypes
import os
import re

import pytest
import torch

from curvature_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "curv_hip.h")).read()
SIZES = {"const void*": 8, "int32_t": 4, "int64_t": 8, "double": 8}


def macro(name: str) -> int:
    return int(re.search(rf"#define {name} (\d+)", HEADER).group(1))


def header_layout():
    """[(field, offset)] and the size of curv_logsum_desc as the header declares it, with natural alignment."""
    body = re.search(r"typedef struct curv_logsum_desc \{(.*?)\} curv_logsum_desc;", HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, at = [], 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        kind = next(k for k in SIZES if decl.startswith(k))
        for name in (n.strip() for n in decl[len(kind):].split(",")):
            count = 1
            m = re.match(r"(\w+)\[(\w+)\]", name)
            if m:
                name, count = m.group(1), macro(m.group(2))
            at = (at + SIZES[kind] - 1) // SIZES[kind] * SIZES[kind]
            fields.append((name, at))
            at += SIZES[kind] * count
    return fields, (at + 7) // 8 * 8


def test_descriptor_matches_the_header():
    fields, size = header_layout()
    assert [n for n, _ in fields] == [n for n, *_ in _lib.curv_logsum_desc._fields_]
    for name, offset in fields:
        assert getattr(_lib.curv_logsum_desc, name).offset == offset, name
    assert ctypes.sizeof(_lib.curv_logsum_desc) == size == 296
    assert (_lib.LOGSUM_GRID_MAX, _lib.LOGSUM_CHUNK, _lib.LOGSUM_ROW_BYTES) == \
        (macro("CURV_LOGSUM_GRID_MAX"), macro("CURV_LOGSUM_CHUNK"), macro("CURV_LOGSUM_ROW_BYTES"))
    assert (_lib.LOGSUM_LOG, _lib.LOGSUM_SQUARES, _lib.DTYPE_F64) == \
        (macro("CURV_LOGSUM_LOG"), macro("CURV_LOGSUM_SQUARES"), macro("CURV_DTYPE_F64"))


def test_abi_version_stays_12():
    assert _lib.lib().curv_version() == 12 == macro("CURV_ABI_VERSION")


def segment(count=8, x=64, dtype=_lib.DTYPE_F32, mode=_lib.LOGSUM_LOG, stride=1, gain=1.0, shift=1.0):
    arr = (_lib.curv_logsum_desc * 3)()
    for d in arr:                                       # three valid segments (never dereferenced on the host)
        d.x, d.count, d.stride, d.dtype, d.mode, d.weight = 64, 8, 1, _lib.DTYPE_F32, _lib.LOGSUM_LOG, 1.0
        d.gain[:2], d.shift[:2] = [1.0, 2.0], [0.5, 0.0]
    arr[1].x, arr[1].count, arr[1].stride, arr[1].dtype, arr[1].mode = x, count, stride, dtype, mode
    arr[1].gain[1], arr[1].shift[1] = gain, shift
    return arr


def test_an_empty_call_is_a_no_op():
    assert _lib.lib().curv_logsum_grid(None, None, 0, 1, None, 0, None, None, 0) == 0


@pytest.mark.parametrize("kwargs, text", [
    (dict(count=-1), "negative count"), (dict(x=None), "null pointer"), (dict(dtype=7), "unknown dtype"),
    (dict(dtype=_lib.DTYPE_BF16), "unknown dtype"), (dict(mode=2), "unknown mode"), (dict(stride=0), "stride"),
    (dict(gain=-1.0), "pair 1"), (dict(shift=float("nan")), "pair 1"),
])
def test_an_invalid_segment_is_named(kwargs, text):
    L = _lib.lib()
    arr = segment(**kwargs)
    out = (ctypes.c_double * 48)()
    for call in (lambda: L.curv_logsum_grid(None, arr, 3, 2, ctypes.addressof(out), 16, None, ctypes.addressof(out), 0),
                 lambda: int(L.curv_logsum_workspace_bytes(arr, 3, 2) == 0) * _lib.ERR_INVALID):
        assert call() == _lib.ERR_INVALID
        message = L.curv_last_error().decode()
        assert "segment 1" in message and text in message, message


@pytest.mark.parametrize("pairs", [0, -1, 17])
def test_pairs_outside_1_to_16(pairs):
    L = _lib.lib()
    arr = segment()
    out = (ctypes.c_double * 64)()
    assert L.curv_logsum_grid(None, arr, 3, pairs, ctypes.addressof(out), 17, None, ctypes.addressof(out), 0) == _lib.ERR_INVALID
    assert "pairs" in L.curv_last_error().decode()
    assert L.curv_logsum_workspace_bytes(arr, 3, pairs) == 0


@pytest.mark.parametrize("pairs", [1, 5, 16])
def test_workspace_bytes(pairs):
    """n table rows of CURV_LOGSUM_ROW_BYTES (the stated extra) and exactly one float64 per chunk and pair."""
    L = _lib.lib()
    chunks = 0
    for count, has in [(0, 0), (1, 1), (4096, 1), (4097, 2)]:
        arr = (_lib.curv_logsum_desc * 1)()
        arr[0].x, arr[0].count, arr[0].stride = (64 if count else None), count, 1
        assert L.curv_logsum_workspace_bytes(arr, 1, pairs) == _lib.LOGSUM_ROW_BYTES + has * pairs * 8, count
        chunks += has
    arr = (_lib.curv_logsum_desc * 4)()
    for d, count in zip(arr, (0, 1, 4096, 4097)):
        d.x, d.count, d.stride = (64 if count else None), count, 1
    assert L.curv_logsum_workspace_bytes(arr, 4, pairs) == 4 * _lib.LOGSUM_ROW_BYTES + chunks * pairs * 8


def test_a_small_workspace_is_refused_before_any_launch():
    L = _lib.lib()
    arr = segment()
    out = (ctypes.c_double * 48)()
    assert L.curv_logsum_grid(None, arr, 3, 2, ctypes.addressof(out), 16, None, ctypes.addressof(out), 8) == _lib.ERR_WORKSPACE


BAD = [([], "no damping pairs"), ([1.0], "not an (add, multiply) pair"), ([(1.0, 2.0, 3.0)], "not an (add, multiply) pair"),
       ([(1.0, 1.0), (0.0, 1.0)], "pair 1"), ([(1.0, -1.0)], "finite and > 0"), ([(float("inf"), 1.0)], "finite and > 0"),
       ([(1.0, float("nan"))], "finite and > 0"), ([([1.0, 0.0], [1.0, 1.0])], "finite and > 0")]


@pytest.mark.parametrize("method", ["log_det_grid", "log_prior_grid"])
@pytest.mark.parametrize("kind", ["Diagonal", "KFAC", "BlockDiagonal"])
def test_bad_hypers_are_refused_by_name_before_the_device(kind, method):
    """On a CPU model with an empty `state`: nothing but the check of `hypers` can have run when ValueError comes."""
    from curvature_amd import curvatures
    model = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.Linear(2, 2))
    est = getattr(curvatures, kind)(model)
    for hypers, text in BAD:
        with pytest.raises(ValueError) as info:
            getattr(est, method)(hypers)
        assert f"{kind}.{method}" in str(info.value) and text in str(info.value), str(info.value)
