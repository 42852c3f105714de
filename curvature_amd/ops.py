"""Tensor-level wrappers over the C ABI: torch tensors in, ``data_ptr()``s and shapes out.

PyTorch is plumbing here (device memory, streams); all arithmetic happens in ``libcurv_hip.so``.
Every wrapper requires CUDA(=HIP) fp32 contiguous tensors and raises ``RuntimeError`` otherwise:
there is no CPU fallback.
"""
import ctypes
import math
import os
import sys
import threading
from typing import List, NamedTuple, Optional, Sequence

import torch

from . import _lib
from ._lib import curv_factor_desc, curv_gemm_desc, curv_inv_desc, curv_sq_desc

_workspaces = {}
_workspace_lock = threading.Lock()


def _require_gpu(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("curvature_amd runs on MI355X only: got a CPU tensor (no CPU fallback)")
        if t.dtype != torch.float32:
            raise RuntimeError(f"curvature_amd expects float32 tensors, got {t.dtype}")
        if not t.is_contiguous():
            raise RuntimeError("curvature_amd expects contiguous tensors")


def workspace(nbytes: int, device: torch.device, tag: str = "default") -> torch.Tensor:
    """A cached scratch buffer owned by torch (the library never allocates device memory).

    One buffer per (device, tag, current stream): launches on one stream are ordered, so they may share
    scratch; two estimators driven from different streams (or threads, each with its own current stream) get
    different buffers and cannot overwrite each other's slabs or descriptor tables mid-kernel.  The buffer is
    allocated on the stream it is keyed by, so the caching allocator's stream ownership matches its use, and
    a regrown buffer's predecessor is only recycled for later work of that same stream."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (index, tag, int(torch.cuda.current_stream(index).cuda_stream))
    with _workspace_lock:
        buf = _workspaces.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes * 1.25), 1 << 20), dtype=torch.uint8, device=device)
            _workspaces[key] = buf
    if _POISON:
        buf.fill_(0xFF)
    return buf


# CURV_DEBUG_POISON=1 (diagnostics, tests/test_poisoned_workspace_gpu.py): every scratch buffer is filled with NaN bit patterns
# each time it is handed to the library, and no descriptor table is assumed to have survived in it - a kernel that reads
# scratch it has not written shows up as a non-finite result instead of depending on what the buffer held before
_POISON = os.environ.get("CURV_DEBUG_POISON", "0") not in ("", "0")
if _POISON:
    # ... and every GPU tensor that torch.empty / torch.empty_like hands out in this process starts as NaNs (integers: all
    # bits set): an output a kernel only partly writes cannot pass a test on what the allocator happened to return
    _torch_empty, _torch_empty_like = torch.empty, torch.empty_like

    def _poisoned(t):
        if isinstance(t, torch.Tensor) and t.is_cuda and t.numel() > 0:
            if t.is_floating_point():
                t.fill_(float("nan"))
            elif t.dtype == torch.uint8:
                t.fill_(0xFF)
            elif t.dtype in (torch.int8, torch.int16, torch.int32, torch.int64):
                t.fill_(-1)
        return t

    torch.empty = lambda *a, **k: _poisoned(_torch_empty(*a, **k))
    torch.empty_like = lambda *a, **k: _poisoned(_torch_empty_like(*a, **k))


def release_workspaces() -> None:
    """Drop every cached scratch buffer (they are re-created on demand)."""
    with _workspace_lock:
        _workspaces.clear()
    _kfac_last.clear()


_kfac_last = {}                        # thread ident -> the "kfac" workspace its last curv_kfac_accumulate call used


class _ConvJob:
    """What the factor jobs share: source and destination, the convolution geometry, and how the product enters the
    destination.  Every subclass adds one field of its own."""
    __slots__ = ("src", "dst", "kernel", "stride", "padding", "has_bias", "scale", "first")

    def _set(self, src, dst, kernel, stride, padding, has_bias, scale, first):
        self.src, self.dst = src, dst
        self.kernel, self.stride, self.padding = tuple(kernel), tuple(stride), tuple(padding)
        self.has_bias, self.scale, self.first = bool(has_bias), float(scale), bool(first)


class FactorJob(_ConvJob):
    """One Kronecker-factor accumulation: dst (+)= scale * unfold(src) unfold(src)^T.  `src` may also be just its shape
    (plan queries)."""
    __slots__ = ("path_hint",)

    def __init__(self, src, dst, kernel=(1, 1), stride=(1, 1), padding=(0, 0), has_bias=False,
                 scale=1.0, first=False, path_hint=0):
        self._set(src, dst, kernel, stride, padding, has_bias, scale, first)
        self.path_hint = int(path_hint)            # _lib.PATH_*: which launch form the UNSHARDED model takes


def small_path_flop(dim: int, K: int) -> float:
    """Executed flops of one factor in the small launch form (32 x 32 blocks on and above the diagonal): the quantity
    CURV_SMALL_MAX_FLOP bounds (csrc/syrk_small.hip)."""
    nb = (int(dim) + 31) // 32
    return 2.0 * 1024.0 * (nb * (nb + 1) // 2) * float(K)


def _set_geometry(d, shape, kernel, stride, padding, has_bias) -> None:
    """The geometry fields every convolution descriptor names alike."""
    d.N, d.C, d.H, d.W = map(int, shape)
    d.kh, d.kw = kernel
    d.sh, d.sw = stride
    d.ph, d.pw = padding
    d.has_bias = int(has_bias)


def _fill_desc(d, j, check_tensors: bool, flat_ok: bool = False, groups: Optional[int] = None,
               source: str = "factor source must be (N,C,H,W) or (N,C)") -> None:
    """Descriptor `d` of any factor build from job `j`: the source as (N, C, H, W) (`flat_ok`: an (N, C) one as
    (N, C, 1, 1)), geometry, `has_bias`, `first`, `scale`; with `check_tensors` also the destination shape, (dim, dim) or
    (groups, dim, dim), and the two addresses.  The caller checks the tensors themselves and adds its own field."""
    shape = tuple(j.src.shape) if isinstance(j.src, torch.Tensor) else tuple(j.src)
    if flat_ok and len(shape) == 2:
        shape += (1, 1)
    if len(shape) != 4:
        raise RuntimeError(source)
    if check_tensors:
        dim = shape[1] // (groups or 1) * j.kernel[0] * j.kernel[1] + int(j.has_bias)
        want = (dim, dim) if groups is None else (groups, dim, dim)
        if shape[1] % (groups or 1) or tuple(j.dst.shape) != want:
            raise RuntimeError(f"{'factor' if groups is None else 'grouped factor'} destination must be "
                               f"({','.join(map(str, want))}), got {tuple(j.dst.shape)}")
        d.src, d.dst = j.src.data_ptr(), j.dst.data_ptr()
    _set_geometry(d, shape, j.kernel, j.stride, j.padding, j.has_bias)
    d.first, d.scale = int(j.first), j.scale


def _all_tensors(jobs) -> bool:
    return all(isinstance(j.src, torch.Tensor) for j in jobs)


def _plan_flops(name: str, arr, n: int) -> List[int]:
    """``<name>(arr, n, out)``: one FLOP count per descriptor."""
    out = (ctypes.c_longlong * n)()
    _lib.check(getattr(_lib.lib(), name)(arr, n, out), name)
    return [int(v) for v in out]


def _run_build(bytes_name: str, name: str, arr, n: int, device, tag: str, events=None) -> None:
    """A side build on the current stream: ``<bytes_name>(arr, n)`` bytes of scratch (0: the library refused the
    descriptors) from `workspace(tag)`, then ``<name>``; `events` = (start, stop) ``torch.cuda.Event``s around it."""
    L = _lib.lib()
    need = getattr(L, bytes_name)(arr, n)
    if need == 0:
        _lib.check(_lib.ERR_INVALID, bytes_name)
    ws = workspace(need, device, tag)
    if events is not None:
        events[0].record()
    _lib.check(getattr(L, name)(_lib.stream_ptr(), arr, n, ws.data_ptr(), ws.numel()), name)
    if events is not None:
        events[1].record()


def _side_plan_flops(cls, jobs) -> List[int]:
    """``<symbol>_plan_flops`` of the `FACTOR_BUILDS` record of job class `cls`."""
    if not jobs:
        return []
    build = _BUILD_OF[cls]
    return _plan_flops(build.symbol + "_plan_flops", build.descs(jobs, check_tensors=_all_tensors(jobs)), len(jobs))


def _side_accumulate(cls, jobs, events) -> None:
    """``<symbol>_accumulate`` of the `FACTOR_BUILDS` record of job class `cls`, with scratch from ``workspace(tag)``."""
    if not jobs:
        return
    build = _BUILD_OF[cls]
    _run_build(build.symbol + "_workspace_bytes", build.symbol + "_accumulate", build.descs(jobs), len(jobs),
               jobs[0].src.device, build.tag, events)


def _factor_descs(jobs: Sequence[FactorJob], check_tensors: bool = True):
    arr = (curv_factor_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        if check_tensors:
            _require_gpu(j.src, j.dst)
        _fill_desc(d, j, check_tensors, flat_ok=True)
        d.path_hint = getattr(j, "path_hint", 0)
    return arr


def kfac_path_for(factors) -> int:
    """The launch form (``_lib.PATH_SMALL`` / ``_lib.PATH_GROUPED``) a factor build of exactly these factors takes on its
    own, decided by the library (curv_kfac_path_for: flops, factor count, slice length, workgroup count).
    `factors`: the fp32 factors of the UNSHARDED model, each a `FactorJob` (its `src` may be just a shape) or a tuple
    ``(N, C, H, W, kernel, stride, padding, has_bias)``; host only."""
    jobs = [f if isinstance(f, FactorJob) else FactorJob(f[:4], None, *f[4:]) for f in factors]
    if not jobs:
        return _lib.PATH_GROUPED
    arr = _factor_descs(jobs, check_tensors=_all_tensors(jobs))
    return int(_lib.lib().curv_kfac_path_for(arr, len(jobs)))


PLAN_INFO_FIELDS = 25                 # CURV_PLAN_INFO_FIELDS


def kfac_plan_flops(jobs: Sequence[FactorJob]) -> List[int]:
    """Multiply-add FLOPs the launch plan executes for each job (curv_kfac_plan_info, last field): dim (dim + 1) K for
    a symmetric product; the sum over its 29 shifted correlations for a 3x3 / stride 1 / pad 1 factor.  `job.src` may
    be a tensor or just its shape (host only)."""
    if not jobs:
        return []
    arr = _factor_descs(jobs, check_tensors=_all_tensors(jobs))
    out = (ctypes.c_longlong * (PLAN_INFO_FIELDS * len(jobs)))()
    _lib.check(_lib.lib().curv_kfac_plan_info(arr, len(jobs), out), "curv_kfac_plan_info")
    return [int(out[PLAN_INFO_FIELDS * i + PLAN_INFO_FIELDS - 1]) for i in range(len(jobs))]


def kfac_accumulate(jobs: Sequence[FactorJob], events=None) -> None:
    """Grouped factor build over any number of factors: one SYRK launch + one reduce launch.

    `events` = (start, stop) handles from ``_lib.lib().curv_event_create()`` are recorded around the SYRK
    kernel (bench.py's roofline measurement)."""
    if not jobs:
        return
    n = len(jobs)
    arr = _factor_descs(jobs)
    L = _lib.lib()
    need = L.curv_kfac_workspace_bytes(arr, n)
    if need == 0:
        _lib.check(_lib.ERR_INVALID, "curv_kfac_workspace_bytes")
    ws = workspace(need, jobs[0].src.device, "kfac")
    # the "kfac" workspaces are written by this function only: if this thread's previous call used this very buffer,
    # its head still holds the descriptor table of that call and unchanged argument blocks need no second upload
    # (a ResNet-50 update() is 26 of them)
    me = threading.get_ident()
    flags = _lib.KFAC_TABLE_RESIDENT if (_kfac_last.get(me) is ws and not _POISON) else 0
    _kfac_last[me] = ws
    ev0, ev1 = events if events is not None else (None, None)
    rc = L.curv_kfac_accumulate_ex(_lib.stream_ptr(), arr, n, ws.data_ptr(), ws.numel(), flags, ev0, ev1)
    if rc != 0:
        _kfac_last.pop(me, None)
    _lib.check(rc, "curv_kfac_accumulate")


_HALF_DTYPES = {torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}


class HalfFactorJob(_ConvJob):
    """A Kronecker-factor accumulation from a bf16 / fp16 source (what autocast hands the hooks) into an fp32 factor:
    dst (+)= scale * unfold(src) unfold(src)^T, built on the bf16 / fp16 MFMA with fp32 accumulation
    (curv_kfac16_accumulate).  Same fields as `FactorJob`; there is no path hint: a factor's plan is its own.
    `src` may also be just its shape plus ``dtype`` (plan queries)."""
    __slots__ = ("dtype",)

    def __init__(self, src, dst, kernel=(1, 1), stride=(1, 1), padding=(0, 0), has_bias=False, scale=1.0,
                 first=False, dtype=None):
        self._set(src, dst, kernel, stride, padding, has_bias, scale, first)
        self.dtype = src.dtype if isinstance(src, torch.Tensor) else dtype


def _half_descs(jobs: Sequence[HalfFactorJob], check_tensors: bool = True):
    arr = (_lib.curv_factor16_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        if j.dtype not in _HALF_DTYPES:
            raise RuntimeError(f"half-precision factor source must be bfloat16 or float16, got {j.dtype}")
        if check_tensors:
            if len(j.src.shape) not in (2, 4):
                raise RuntimeError("factor source must be (N,C,H,W) or (N,C)")
            if not (j.src.is_cuda and j.dst.is_cuda):
                raise RuntimeError("curvature_amd runs on MI355X only: got a CPU tensor (no CPU fallback)")
            if not j.src.is_contiguous():
                raise RuntimeError("curvature_amd expects contiguous tensors")
            _require_gpu(j.dst)
        _fill_desc(d, j, check_tensors, flat_ok=True)
        d.dtype = _HALF_DTYPES[j.dtype]
    return arr


def kfac_half_plan_flops(jobs: Sequence[HalfFactorJob]) -> List[int]:
    """FLOPs (2 per multiply-add) the half-precision build executes for each job (curv_kfac16_plan_flops, host only):
    every 128 x 128 tile on and above the diagonal over K padded to 16."""
    return _side_plan_flops(HalfFactorJob, jobs)


def kfac_accumulate_half(jobs: Sequence[HalfFactorJob], events=None) -> None:
    """Factor build from bf16 / fp16 sources (curv_kfac16_accumulate): a pack, an MFMA and a reduce launch per batch of
    factors, on the current stream.  Scratch from `workspace` (so CURV_DEBUG_POISON covers it).  `events` = (start,
    stop) ``torch.cuda.Event``s (enable_timing) are recorded around the whole build."""
    _side_accumulate(HalfFactorJob, jobs, events)


class GroupFactorJob(_ConvJob):
    """The stacked Kronecker factors of a grouped convolution: dst[g] (+)= scale * unfold(src_g) unfold(src_g)^T, src_g
    the g-th of `groups` equal channel slices of src (curv_kfac_group_accumulate)."""
    __slots__ = ("groups",)

    def __init__(self, src, dst, groups, kernel=(1, 1), stride=(1, 1), padding=(0, 0), has_bias=False, scale=1.0,
                 first=False):
        self._set(src, dst, kernel, stride, padding, has_bias, scale, first)
        self.groups = int(groups)


def _group_descs(jobs: Sequence[GroupFactorJob], check_tensors: bool = True):
    arr = (_lib.curv_group_factor_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        if check_tensors:
            _require_gpu(j.src, j.dst)
        _fill_desc(d, j, check_tensors, groups=j.groups, source="grouped factor source must be (N,C,H,W)")
        d.groups = j.groups
    return arr


def kfac_group_plan_flops(jobs: Sequence[GroupFactorJob]) -> List[int]:
    """Multiply-add FLOPs (2 per multiply-add) the grouped build executes for each job (curv_kfac_group_plan_flops, host
    only).  `job.src` may be a tensor or just its (N, C, H, W) shape."""
    return _side_plan_flops(GroupFactorJob, jobs)


def kfac_accumulate_groups(jobs: Sequence[GroupFactorJob], events=None) -> None:
    """Factor build of grouped convolutions (curv_kfac_group_accumulate): a Gram launch per kernel class and one reduce
    launch per batch of factors, on the current stream.  Scratch from `workspace` (so CURV_DEBUG_POISON covers it).
    `events` = (start, stop) ``torch.cuda.Event``s (enable_timing) are recorded around the whole build."""
    _side_accumulate(GroupFactorJob, jobs, events)


class ConvTFactorJob(_ConvJob):
    """The A factor of a ConvTranspose2d (curv_kfac_convt_accumulate): dst (+)= scale * sum_o a(o) a(o)^T over the output
    pixels, a(o) the layer's patch in Wm = weight.permute(1, 0, 2, 3).reshape(Cout, -1) order [+ 1].  `out_size` = (Ho, Wo)
    of the layer's output (it carries the effective output_padding).  `src` may also be just its (N, C, H, W) shape (plan
    queries)."""
    __slots__ = ("out_size",)

    def __init__(self, src, dst, kernel, stride, padding, out_size, has_bias=False, scale=1.0, first=False):
        self._set(src, dst, kernel, stride, padding, has_bias, scale, first)
        self.out_size = tuple(int(v) for v in out_size)


def _convt_descs(jobs: Sequence[ConvTFactorJob], check_tensors: bool = True):
    arr = (_lib.curv_convt_factor_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        if check_tensors:
            _require_gpu(j.src, j.dst)
        _fill_desc(d, j, check_tensors,
                   source="transposed-convolution factor source must be a contiguous float32 (N,C,H,W) tensor")
        d.Ho, d.Wo = j.out_size
    return arr


def kfac_convt_plan_flops(jobs: Sequence[ConvTFactorJob]) -> List[int]:
    """Multiply-add FLOPs (2 per multiply-add) the transposed-convolution build executes for each job: the sum over the
    phase Grams it runs (curv_kfac_convt_plan_flops, host only).  `job.src` may be a tensor or its (N, C, H, W) shape."""
    return _side_plan_flops(ConvTFactorJob, jobs)


def kfac_accumulate_convt(jobs: Sequence[ConvTFactorJob], events=None) -> None:
    """A-factor build of transposed convolutions (curv_kfac_convt_accumulate) on the current stream: per factor the window
    copies of its phases, one fp32 MFMA build of the phase Grams and one assembly launch.  Scratch from `workspace` (so
    CURV_DEBUG_POISON covers it).  `events` = (start, stop) ``torch.cuda.Event``s are recorded around the whole build."""
    _side_accumulate(ConvTFactorJob, jobs, events)


class DilatedFactorJob(_ConvJob):
    """The A factor of a dilated Conv2d (curv_kfac_dilated_accumulate): dst (+)= scale * X X^T with X =
    F.unfold(src, kernel, dilation, padding, stride 1) [+ ones row], built as the sum of the plain factors of the residue
    classes ``src[:, :, rh::dh, rw::dw]``.  Stride 1 and a padding that is a multiple of the dilation (the library refuses
    anything else).  `src` may also be just its (N, C, H, W) shape (plan queries)."""
    __slots__ = ("dilation",)

    def __init__(self, src, dst, kernel, stride, padding, dilation, has_bias=False, scale=1.0, first=False):
        self._set(src, dst, kernel, stride, padding, has_bias, scale, first)
        self.dilation = tuple(int(v) for v in dilation)


def _dilated_descs(jobs: Sequence[DilatedFactorJob], check_tensors: bool = True):
    arr = (_lib.curv_dilated_factor_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        if check_tensors:
            _require_gpu(j.src, j.dst)
        _fill_desc(d, j, check_tensors, source="dilated-convolution factor source must be a contiguous float32 (N,C,H,W) tensor")
        d.dh, d.dw = j.dilation
    return arr


def kfac_dilated_plan_flops(jobs: Sequence[DilatedFactorJob]) -> List[int]:
    """Multiply-add FLOPs (2 per multiply-add) the dilated build executes for each job: the sum over the plain builds of
    its class stacks (curv_kfac_dilated_plan_flops, host only).  `job.src` may be a tensor or its (N, C, H, W) shape."""
    return _side_plan_flops(DilatedFactorJob, jobs)


def kfac_accumulate_dilated(jobs: Sequence[DilatedFactorJob], events=None) -> None:
    """A-factor build of dilated convolutions (curv_kfac_dilated_accumulate) on the current stream: per factor one gather
    pass that writes the residue-class sub-images, then one fp32 MFMA build per size group (at most four).  Scratch from
    `workspace` (so CURV_DEBUG_POISON covers it).  `events` = (start, stop) ``torch.cuda.Event``s are recorded around the
    whole build."""
    _side_accumulate(DilatedFactorJob, jobs, events)


class Conv3dFactorJob(_ConvJob):
    """The A factor of a Conv3d (curv_kfac_conv3d_accumulate): dst (+)= scale * X X^T with X the 3-D im2col of
    `src` (N, C, D, H, W) [+ ones row], rows in the order of ``weight.reshape(Cout, -1)``; built as the plain factor of the
    depth-unfolded (N Do, C kd, H, W) stack.  `kernel`, `stride` and `padding` are (depth, height, width) triples; groups 1,
    dilation 1.  `src` may also be just its (N, C, D, H, W) shape (plan queries)."""
    __slots__ = ()

    def __init__(self, src, dst, kernel, stride=(1, 1, 1), padding=(0, 0, 0), has_bias=False, scale=1.0, first=False):
        self._set(src, dst, kernel, stride, padding, has_bias, scale, first)

    @property
    def stack_shape(self) -> tuple:
        """(N Do, C kd, H, W): the stack the plain build runs on, with the 2-D window ``kernel[1:]`` etc."""
        N, C, D, H, W = (int(v) for v in (self.src.shape if isinstance(self.src, torch.Tensor) else self.src))
        Do = (D + 2 * self.padding[0] - self.kernel[0]) // self.stride[0] + 1
        return (N * Do, C * self.kernel[0], H, W)


def _conv3d_descs(jobs: Sequence[Conv3dFactorJob], check_tensors: bool = True):
    arr = (_lib.curv_conv3d_factor_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        if check_tensors:
            _require_gpu(j.src, j.dst)
        shape = tuple(j.src.shape) if isinstance(j.src, torch.Tensor) else tuple(j.src)
        if len(shape) != 5 or not len(j.kernel) == len(j.stride) == len(j.padding) == 3:
            raise RuntimeError("3-D convolution factor source must be a contiguous float32 (N,C,D,H,W) tensor, with "
                               "(depth, height, width) kernel, stride and padding")
        if check_tensors:
            dim = shape[1] * math.prod(j.kernel) + int(j.has_bias)
            if tuple(j.dst.shape) != (dim, dim):
                raise RuntimeError(f"factor destination must be ({dim},{dim}), got {tuple(j.dst.shape)}")
            d.src, d.dst = j.src.data_ptr(), j.dst.data_ptr()
        d.N, d.C, d.D, d.H, d.W = map(int, shape)
        d.kd, d.kh, d.kw = j.kernel
        d.sd, d.sh, d.sw = j.stride
        d.pd, d.ph, d.pw = j.padding
        d.has_bias, d.first, d.scale = int(j.has_bias), int(j.first), j.scale
    return arr


def kfac_conv3d_plan_flops(jobs: Sequence[Conv3dFactorJob]) -> List[int]:
    """Multiply-add FLOPs (2 per multiply-add) the Conv3d build executes for each job: those of the plain build of its
    depth-unfolded stack (curv_kfac_conv3d_plan_flops, host only).  `job.src` may be a tensor or its (N, C, D, H, W) shape."""
    return _side_plan_flops(Conv3dFactorJob, jobs)


def kfac_accumulate_conv3d(jobs: Sequence[Conv3dFactorJob], events=None) -> None:
    """A-factor build of 3-D convolutions (curv_kfac_conv3d_accumulate) on the current stream: per factor one gather pass
    that writes the depth-unfolded stack, then one fp32 MFMA build of it.  Scratch from `workspace` (so CURV_DEBUG_POISON
    covers it).  `events` = (start, stop) ``torch.cuda.Event``s are recorded around the whole build."""
    _side_accumulate(Conv3dFactorJob, jobs, events)


class ReduceFactorJob(_ConvJob):
    """One KFAC-reduce factor (curv_kfac_reduce_accumulate): dst (+)= scale * R R^T with R the (N, dim)
    per-sample rows [+ ones column].  `form` = ``_lib.REDUCE_PLANE``: `src` is (N, C, H, W) and a row the mean (`mean`) or
    sum over the output pixels of the im2col columns of the window; ``_lib.REDUCE_TOKEN``: `src` is (N, T, E) and a row the
    mean or sum over T.  `src` is float32, bfloat16 or float16 (the rows and the build are float32); it may also be just
    its shape, with `dtype` (plan queries)."""
    __slots__ = ("form", "mean", "dtype")

    def __init__(self, src, dst, kernel=(1, 1), stride=(1, 1), padding=(0, 0), has_bias=False, scale=1.0, first=False,
                 form=_lib.REDUCE_PLANE, mean=True, dtype=None):
        self._set(src, dst, kernel, stride, padding, has_bias, scale, first)
        self.form, self.mean = int(form), bool(mean)
        self.dtype = src.dtype if isinstance(src, torch.Tensor) else (dtype or torch.float32)


def _reduce_descs(jobs: Sequence[ReduceFactorJob], check_tensors: bool = True):
    arr = (_lib.curv_reduce_factor_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        if j.dtype not in _PACK_DTYPES:
            raise RuntimeError(f"reduce factor source must be float32, bfloat16 or float16, got {j.dtype}")
        shape = tuple(int(v) for v in j.src.shape) if isinstance(j.src, torch.Tensor) else tuple(int(v) for v in j.src)
        token = j.form == _lib.REDUCE_TOKEN
        if len(shape) != (3 if token else 4):
            raise RuntimeError("reduce factor source must be (N,T,E)" if token else "reduce factor source must be (N,C,H,W)")
        if token:
            d.N, d.T, d.E = shape
            d.has_bias = int(j.has_bias)
            dim = shape[2] + int(j.has_bias)
        else:
            _set_geometry(d, shape, j.kernel, j.stride, j.padding, j.has_bias)
            dim = shape[1] * j.kernel[0] * j.kernel[1] + int(j.has_bias)
        if check_tensors:
            if not (j.src.is_cuda and j.dst.is_cuda):
                raise RuntimeError("curvature_amd runs on MI355X only: got a CPU tensor (no CPU fallback)")
            if not j.src.is_contiguous():
                raise RuntimeError("curvature_amd expects contiguous tensors")
            _require_gpu(j.dst)
            if tuple(j.dst.shape) != (dim, dim):
                raise RuntimeError(f"factor destination must be ({dim},{dim}), got {tuple(j.dst.shape)}")
            d.src, d.dst = j.src.data_ptr(), j.dst.data_ptr()
        d.first, d.scale = int(j.first), j.scale
        d.dtype, d.form, d.mean = _PACK_DTYPES[j.dtype], j.form, int(j.mean)
    return arr


def kfac_reduce_plan_flops(jobs: Sequence[ReduceFactorJob]) -> List[int]:
    """What the reduce build executes for each job (curv_kfac_reduce_plan_flops, host only): the additions of the reduce
    pass plus the multiply-add FLOPs of the flat build of its (N, dim) rows.  `job.src` may be a tensor or its shape."""
    return _side_plan_flops(ReduceFactorJob, jobs)


def kfac_accumulate_reduce(jobs: Sequence[ReduceFactorJob], events=None) -> None:
    """KFAC-reduce factor build (curv_kfac_reduce_accumulate) on the current stream: per factor one streaming pass that
    writes the per-sample rows, then one fp32 build of their Gram.  Scratch from `workspace` (so CURV_DEBUG_POISON covers
    it).  `events` = (start, stop) ``torch.cuda.Event``s are recorded around the whole build."""
    _side_accumulate(ReduceFactorJob, jobs, events)


class NormFactorJob(_ConvJob):
    """One stacked factor of a normalisation layer (curv_kfac_norm_accumulate): `side` ``_lib.NORM_SIDE_A``:
    dst (C, n_g, n_g) (+)= scale * sum [xh, 1][xh, 1]^T over samples and positions, `src` the layer's input;
    ``_lib.NORM_SIDE_G``: dst (C, 1, 1) (+)= scale * sum g**2, `src` the grad_output.  `view`: the `NormView` of the layer
    on its records (`norm_view`): sizes, strides, statistics mode.  `src` may also be just its shape (plan queries)."""
    __slots__ = ("side", "view")

    def __init__(self, src, dst, side, view, scale=1.0, first=False):
        self._set(src, dst, (1, 1), (1, 1), (0, 0), view.has_bias and side == _lib.NORM_SIDE_A, scale, first)
        self.side, self.view = int(side), view


def _fill_norm_view(d, view, x, g, name: str) -> None:
    """The record, geometry and statistics fields of a curv_norm_desc from a `NormView`; `x` / `g`: the records whose
    addresses go in (tensors: float32 on the GPU), or None."""
    d.N, d.C, d.H, d.W = view.dims
    d.mode, d.groups, d.eps, d.has_bias = view.mode, view.groups, view.eps, int(view.has_bias)
    for side, strides, elems in (("x", view.x_strides, view.x_elems), ("g", view.g_strides, view.g_elems)):
        if strides is None:
            continue
        for k, v in zip(("sn", "sc", "sh", "sw"), strides):
            setattr(d, f"{side}_{k}", int(v))
        setattr(d, f"{side}_elems", int(elems))
    for t in (x, g) + ((view.mean, view.var) if x is not None else ()):   # (a plan query reads no statistics)
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{name}: curvature_amd runs on MI355X only: got a CPU tensor for {view.name} (no CPU "
                               f"fallback)")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name}: {view.name} expects float32 records, got {t.dtype}")
    if x is not None:
        d.x = x.data_ptr()
        if view.mean is not None:
            d.mean, d.var = view.mean.data_ptr(), view.var.data_ptr()
    if g is not None:
        d.g = g.data_ptr()


def _norm_descs(jobs: Sequence[NormFactorJob], check_tensors: bool = True):
    arr = (_lib.curv_norm_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        a_side = j.side == _lib.NORM_SIDE_A
        src = j.src if check_tensors else None
        _fill_norm_view(d, j.view, src if a_side else None, None if a_side else src, "norm factor build")
        d.side, d.first, d.scale = j.side, int(j.first), j.scale
        if check_tensors:
            C, n_g = j.view.dims[1], (1 + int(j.view.has_bias)) if a_side else 1
            _require_gpu(j.dst)
            if tuple(j.dst.shape) != (C, n_g, n_g):
                raise RuntimeError(f"norm factor destination must be ({C},{n_g},{n_g}), got {tuple(j.dst.shape)}")
            d.dst = j.dst.data_ptr()
    return arr


def kfac_norm_plan_flops(jobs: Sequence[NormFactorJob]) -> List[int]:
    """FLOPs the normalisation-layer build executes for each job (curv_kfac_norm_plan_flops, host only): the statistics
    pass plus the products.  `job.src` may be a tensor or just its shape."""
    return _side_plan_flops(NormFactorJob, jobs)


def kfac_accumulate_norm(jobs: Sequence[NormFactorJob], events=None) -> None:
    """Factor build of normalisation layers (curv_kfac_norm_accumulate) on the current stream: a statistics pass and a
    product pass over the records (the standardised input is never written), then the sum over samples.  Scratch from
    `workspace` (so CURV_DEBUG_POISON covers it).  `events` = (start, stop) ``torch.cuda.Event``s around the build."""
    _side_accumulate(NormFactorJob, jobs, events)


class EmbeddingFactorJob(_ConvJob):
    """The diagonal A factor of an nn.Embedding (curv_kfac_embedding_accumulate): dst (V,) (+)= scale * the
    count of every token in `src`, the (N, *) int64 / int32 index record (contiguous; or just its shape, for plan queries,
    with `i64` saying which); the count of row `padding_idx` (None: no such row) is 0."""
    __slots__ = ("V", "padding_idx", "i64")

    def __init__(self, src, dst, V, padding_idx=None, scale=1.0, first=False, i64=True):
        self._set(src, dst, (1, 1), (1, 1), (0, 0), False, scale, first)
        self.V, self.padding_idx = int(V), None if padding_idx is None else int(padding_idx)
        self.i64 = bool(src.dtype == torch.int64) if isinstance(src, torch.Tensor) else bool(i64)


_INDEX_DTYPES = (torch.int64, torch.int32)


def _embedding_descs(jobs: Sequence[EmbeddingFactorJob], check_tensors: bool = True):
    arr = (_lib.curv_embedding_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        shape = tuple(j.src.shape) if isinstance(j.src, torch.Tensor) else tuple(j.src)
        d.positions, d.idx_i64, d.V = math.prod(shape), int(j.i64), j.V
        d.padding_idx = -1 if j.padding_idx is None else j.padding_idx
        d.first, d.scale = int(j.first), j.scale
        if check_tensors:
            if not j.src.is_cuda or not j.dst.is_cuda:
                raise RuntimeError("curvature_amd runs on MI355X only: got a CPU tensor (no CPU fallback)")
            if j.src.dtype not in _INDEX_DTYPES or not j.src.is_contiguous():
                raise RuntimeError(f"embedding factor source must be a contiguous int64 or int32 index tensor, got {j.src.dtype}")
            if j.dst.dtype != torch.float32 or tuple(j.dst.shape) != (j.V,) or not j.dst.is_contiguous():
                raise RuntimeError(f"embedding factor destination must be a contiguous float32 ({j.V},) vector, got "
                                   f"{tuple(j.dst.shape)} {j.dst.dtype}")
            d.idx, d.a = j.src.data_ptr(), j.dst.data_ptr()
    return arr


def kfac_embedding_plan_flops(jobs: Sequence[EmbeddingFactorJob]) -> List[int]:
    """What the histogram executes for each job (curv_kfac_embedding_plan_flops, host only): one add per position and one
    multiply-add per row.  `job.src` may be a tensor or just its shape."""
    return _side_plan_flops(EmbeddingFactorJob, jobs)


def kfac_accumulate_embedding(jobs: Sequence[EmbeddingFactorJob], events=None) -> None:
    """The token histograms of nn.Embedding layers (curv_kfac_embedding_accumulate) on the current stream: int32 counts in
    `workspace` scratch, one atomic per distinct token of a wave, then ``dst (+)= scale * count``: the same bits in any
    order.  `events` = (start, stop) ``torch.cuda.Event``s around the build."""
    _side_accumulate(EmbeddingFactorJob, jobs, events)


class FactorBuild(NamedTuple):
    """One kind of factor build: the job class, its descriptor filler, the names of the `ops` functions that price and
    build jobs of that class and, for the side builds, the library's symbol stem and the tag of their scratch."""
    job: type
    descs: object
    plan_flops: str
    accumulate: str
    symbol: Optional[str] = None
    tag: Optional[str] = None


# Every kind of factor build, in launch order.  A new kind is a job class, its filler, its two named functions and a row
# here: KFAC.update, sharding.layer_dims and the job tests read the kinds from this table.
FACTOR_BUILDS = (
    FactorBuild(FactorJob, _factor_descs, "kfac_plan_flops", "kfac_accumulate"),
    FactorBuild(GroupFactorJob, _group_descs, "kfac_group_plan_flops", "kfac_accumulate_groups", "curv_kfac_group",
                "kfac_groups"),
    FactorBuild(HalfFactorJob, _half_descs, "kfac_half_plan_flops", "kfac_accumulate_half", "curv_kfac16", "kfac_half"),
    FactorBuild(ConvTFactorJob, _convt_descs, "kfac_convt_plan_flops", "kfac_accumulate_convt", "curv_kfac_convt",
                "kfac_convt"),
    FactorBuild(DilatedFactorJob, _dilated_descs, "kfac_dilated_plan_flops", "kfac_accumulate_dilated",
                "curv_kfac_dilated", "kfac_dilated"),
    FactorBuild(ReduceFactorJob, _reduce_descs, "kfac_reduce_plan_flops", "kfac_accumulate_reduce", "curv_kfac_reduce",
                "kfac_reduce"),
    FactorBuild(Conv3dFactorJob, _conv3d_descs, "kfac_conv3d_plan_flops", "kfac_accumulate_conv3d", "curv_kfac_conv3d",
                "kfac_conv3d"),
    FactorBuild(EmbeddingFactorJob, _embedding_descs, "kfac_embedding_plan_flops", "kfac_accumulate_embedding",
                "curv_kfac_embedding", "kfac_embedding"),
    FactorBuild(NormFactorJob, _norm_descs, "kfac_norm_plan_flops", "kfac_accumulate_norm", "curv_kfac_norm", "kfac_norm"),
)
_BUILD_OF = {build.job: build for build in FACTOR_BUILDS}


def _by_build(jobs) -> list:
    """[(record, its jobs)] for every kind, in table order, a kind's jobs ([] where it has none) in input order."""
    batches = {build.job: [] for build in FACTOR_BUILDS}
    for job in jobs:
        if type(job) not in batches:
            raise TypeError(f"not a factor job: {type(job).__name__} (ops.FACTOR_BUILDS lists the job classes)")
        batches[type(job)].append(job)
    return [(_BUILD_OF[cls], batch) for cls, batch in batches.items()]


def factor_plan_flops(jobs) -> List[int]:
    """What the library executes for each of `jobs`, a list of factor jobs of any classes, in input order: the jobs of one
    class are priced together by the class's named function (``ops.kfac_*_plan_flops``, looked up when called)."""
    flops = {}
    for build, batch in _by_build(jobs):
        flops.update(zip(map(id, batch), getattr(sys.modules[__name__], build.plan_flops)(batch)))
    return [flops[id(job)] for job in jobs]


def accumulate_factors(jobs, events=None) -> None:
    """Build `jobs`, a list of factor jobs of any classes: one call of the named build (``ops.kfac_accumulate*``, looked up
    when called) per class, in table order, a class's jobs in input order.  A class without jobs is called with an empty
    list, which launches nothing - as `KFAC.update` always called every build, so what stands in for a build sees every
    update.  `events` go to the fp32 `FactorJob` build only.  TypeError, before any build is called, for a job of a class
    the table does not list."""
    for build, batch in _by_build(jobs):
        getattr(sys.modules[__name__], build.accumulate)(batch, events=events if build.job is FactorJob else None)


# Dilated convolutions are opt-in: with the switch off - the default - every selection, refusal and message
# is exactly what it was.
_DILATED = False


def admit_dilated(enable: bool = True) -> bool:
    """Switch dilated convolutions on or off for the process; returns what it was.  On: `factor_jobs` routes the A side
    of a groups-1 Conv2d with a dilation other than (1, 1) to `DilatedFactorJob`, KFAC (and with it EFB and INF) records
    such a layer - stride 1, padding a multiple of the dilation - and the per-sample line (``per_sample=True``, the
    linearised predictives) takes it with any stride and integer padding.  Off: such a layer raises where it did.
    Dilation with ``groups > 1``, string padding and dilated ConvTranspose2d are refused either way."""
    global _DILATED
    was, _DILATED = _DILATED, bool(enable)
    return was


def dilated_admitted() -> bool:
    return _DILATED


# Conv1d and Conv3d are opt-in too: with the switch off - the default - every selection, refusal and message
# is exactly what it was.
_CONV_ND = False
_ND_KINDS = ('Conv1d', 'Conv3d')


def admit_conv_nd(enable: bool = True) -> bool:
    """Switch Conv1d and Conv3d layers on or off for the process; returns what it was.  On: the estimators accept
    ``'Conv1d'`` and ``'Conv3d'`` in `layer_types` by name (they never enter the default selection) and `factor_jobs` routes
    them: a Conv1d as the Conv2d it is with a height of 1, the A side of a Conv3d to `Conv3dFactorJob`.  Groups 1, integer
    zero padding; a Conv1d may be dilated with `admit_dilated` on, a Conv3d not.  The per-sample line takes a Conv1d, and a
    Conv3d only with `admit_conv3d_per_sample` on as well.  Off: both kinds are refused where they were."""
    global _CONV_ND
    was, _CONV_ND = _CONV_ND, bool(enable)
    return was


def conv_nd_admitted() -> bool:
    return _CONV_ND


# The per-sample line of a Conv3d has a switch of its own: with it off - the default - `admit_conv_nd`
# admits what it admitted, and every refusal of a Conv3d in the per-sample line reads as it did.
_CONV3D_PER_SAMPLE = False


def admit_conv3d_per_sample(enable: bool = True) -> bool:
    """Switch the per-sample line of Conv3d layers on or off for the process; returns what it was.  On, and with
    `admit_conv_nd` on as well (alone it admits nothing: a Conv3d cannot be selected without that switch):
    `per_sample_operands` takes a Conv3d - its X side the 3-D im2col of the (N, C, D, H, W) record, written per sample by
    curv_persample_pack3d, its g side grad_output as (m, Do Ho Wo) - and with it ``Diagonal(per_sample=True)``,
    ``EFB(per_sample=True)`` and the linearised predictives (`functional_variance`, `stage_output` /
    `functional_covariance`, `functional_variance_grid`) do.  Groups 1, integer zero padding, dilation 1.  Off: a Conv3d
    is refused there as before."""
    global _CONV3D_PER_SAMPLE
    was, _CONV3D_PER_SAMPLE = _CONV3D_PER_SAMPLE, bool(enable)
    return was


def conv3d_per_sample_admitted() -> bool:
    return _CONV3D_PER_SAMPLE


# LayerNorm, GroupNorm and BatchNorm2d are opt-in as well: with the switch off - the default - every
# selection, refusal and message is exactly what it was.
_NORM = False
_NORM_KINDS = ('LayerNorm', 'GroupNorm', 'BatchNorm2d')


def admit_norm_layers(enable: bool = True) -> bool:
    """Switch the affine parameters of normalisation layers on or off for the process; returns what it was.  On: the
    estimators accept ``'LayerNorm'``, ``'GroupNorm'`` and ``'BatchNorm2d'`` in `layer_types` by name (they never enter the
    default selection), `factor_jobs` routes them to two `NormFactorJob`s and `per_sample_route` answers ``"norm"``: the
    gain and shift of channel c are the 1 x (1 + has_bias) row of a depthwise 1x1 convolution of the standardised input,
    which csrc/norm_factor.hip forms on the fly.  KFAC and Diagonal take them (`functional_variance` included); a
    BatchNorm2d in eval mode only.  Off: the three kinds are refused where they were."""
    global _NORM
    was, _NORM = _NORM, bool(enable)
    return was


def norm_layers_admitted() -> bool:
    return _NORM


def is_norm_layer(layer) -> bool:
    """A LayerNorm, GroupNorm or BatchNorm2d while `admit_norm_layers` is on."""
    return _NORM and layer.__class__.__name__ in _NORM_KINDS


class NormView(NamedTuple):
    """`norm_view` of a normalisation layer on its records: the logical (N, C, H, W) `dims`, the element strides and the
    extent of each record (None without that record), the statistics `mode` (``_lib.NORM_*``) with `groups`, `eps` and, for
    given statistics, the `mean` / `var` tensors; `name` for messages."""
    dims: tuple
    x_strides: Optional[tuple]
    x_elems: int
    g_strides: Optional[tuple]
    g_elems: int
    mode: int
    groups: int
    eps: float
    has_bias: bool
    mean: object
    var: object
    name: str


def _dense_strides(shape) -> tuple:
    out, run = [], 1
    for v in reversed(shape):
        out.append(run)
        run *= int(v)
    return tuple(reversed(out))


def _norm_record_view(kind: str, name: str, t, k: int):
    """(dims, strides, extent) of one record of a normalisation layer: `t` a tensor or `ShapeOnly` (taken as dense), `k`
    the number of normalised dims of a LayerNorm.  Nothing is copied: a record whose dims do not collapse is refused."""
    shape = tuple(int(v) for v in t.shape)
    tensor = isinstance(t, torch.Tensor)
    strides = tuple(int(v) for v in t.stride()) if tensor else _dense_strides(shape)
    elems = _source_extent(t) if tensor else math.prod(shape)

    def collapse(lo: int, hi: int):
        """(size, stride) of dims [lo, hi) as one axis, or None where the strides do not allow it."""
        size, stride = 1, 1
        for i in reversed(range(lo, hi)):
            if shape[i] == 1:
                continue
            if size > 1 and strides[i] != stride * size:
                return None
            if size == 1:
                stride = strides[i]
            size *= shape[i]
        return size, stride

    if kind == 'LayerNorm':
        if len(shape) < k + 1:
            raise RuntimeError(f"{name}: LayerNorm records must be (N, *, normalized_shape), got {shape}")
        inner, mid = collapse(len(shape) - k, len(shape)), collapse(1, len(shape) - k)
        if inner is None or (inner[0] > 1 and inner[1] != 1):
            raise RuntimeError(f"{name}: the normalised dims of a LayerNorm record must be contiguous (shape {shape}, "
                               f"strides {strides}); record a contiguous tensor")
        if mid is None:
            raise RuntimeError(f"{name}: the dims between the batch and the normalised dims of a LayerNorm record must "
                               f"collapse to one stride (shape {shape}, strides {strides}); record a contiguous tensor")
        return (shape[0], inner[0], mid[0], 1), (strides[0], 1, mid[1], 1), elems
    if not 2 <= len(shape) <= 4:
        raise RuntimeError(f"{name}: {kind} records must be (N, C), (N, C, L) or (N, C, H, W), got {shape}")
    if kind == 'BatchNorm2d' and len(shape) != 4:
        raise RuntimeError(f"{name}: BatchNorm2d records must be (N, C, H, W), got {shape}")
    shape4 = shape[:2] + (1,) * (4 - len(shape)) + shape[2:]
    strides4 = strides[:2] + (1,) * (4 - len(shape)) + strides[2:]
    return shape4, strides4, elems


def norm_view(layer, x=None, g=None, name: Optional[str] = None) -> NormView:
    """The one place that turns a normalisation layer and its records (tensors, `ShapeOnly`s or None) into what
    csrc/norm_factor.hip reads.  LayerNorm on (N, *, normalized_shape): C = the product of the normalised dims, H = the
    product of the middle ones, W = 1, statistics per position.  GroupNorm on (N, C), (N, C, L) or (N, C, H, W): the natural
    view, any strides (channels_last included), statistics per (sample, group).  BatchNorm2d: the natural view, the running
    statistics - in eval mode only: batch statistics couple the samples, so there is no per-sample Jacobian."""
    kind = layer.__class__.__name__
    name = name or repr(layer)
    if not is_norm_layer(layer):
        raise NotImplementedError(f"{kind} layers are not supported (ops.admit_norm_layers() admits LayerNorm, GroupNorm "
                                  f"and BatchNorm2d)")
    if layer.weight is None:
        raise NotImplementedError(f"{kind} layer {name} has no affine parameters (elementwise_affine / affine is False): "
                                  f"there is nothing to estimate")
    C = layer.weight.numel()
    mean = var = None
    groups, k = 1, 0
    if kind == 'LayerNorm':
        mode, k = _lib.NORM_POSITION, len(layer.normalized_shape)
    elif kind == 'GroupNorm':
        mode, groups = _lib.NORM_GROUP, int(layer.num_groups)
    else:
        mode = _lib.NORM_GIVEN
        if layer.training or not layer.track_running_stats or layer.running_mean is None:
            raise NotImplementedError(
                f"BatchNorm2d layer {name} {'is in training mode' if layer.training else 'has track_running_stats=False'}: "
                f"batch statistics couple the samples, so the layer has no per-sample Jacobian; call model.eval() (with "
                f"track_running_stats=True) before the passes that are recorded")
        mean, var = layer.running_mean.detach(), layer.running_var.detach()
    views = [None if t is None else _norm_record_view(kind, name, t, k) for t in (x, g)]
    if views[0] is None and views[1] is None:
        raise RuntimeError(f"{name}: no recorded forward/backward pass")
    dims = (views[0] or views[1])[0]
    if views[0] is not None and views[1] is not None and views[0][0] != views[1][0]:
        raise RuntimeError(f"{name}: input and grad_output differ in shape ({tuple(x.shape)} and {tuple(g.shape)})")
    if dims[1] != C:
        raise RuntimeError(f"{name}: the records have {dims[1]} channels, the layer {C}")
    for t in (x, g):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f"{name}: {kind} expects float32 records, got {t.dtype}")
    (xs, xe), (gs, ge) = ((None, 0) if v is None else v[1:] for v in views)
    return NormView(dims, xs, xe, gs, ge, mode, groups, float(layer.eps), layer.bias is not None, mean, var, name)


def _norm_jobs(layer, x, g, name: Optional[str] = None) -> "LayerJobs":
    """`factor_jobs` of a normalisation layer (`admit_norm_layers`): two `NormFactorJob`s on the records as they are (no
    copy); n = 1 + has_bias, m = 1, C stacked factors, L positions per sample."""
    if x is None and g is None:
        raise RuntimeError("KFAC.update: no recorded forward/backward pass for a selected layer")
    x, g = (t.detach() if isinstance(t, torch.Tensor) else t for t in (x, g))
    view = norm_view(layer, x, g, name)
    a_job = None if x is None else NormFactorJob(_job_source(x), None, _lib.NORM_SIDE_A, view)
    g_job = None if g is None else NormFactorJob(_job_source(g), None, _lib.NORM_SIDE_G, view)
    N, C, H, W = view.dims
    return LayerJobs(a_job, g_job, 1 + int(view.has_bias), 1, N, H * W, C)


# nn.Embedding is opt-in in the same way: with the switch off - the default - every selection, refusal and
# message is exactly what it was.
_EMBEDDING = False


def admit_embedding(enable: bool = True) -> bool:
    """Switch the weight of nn.Embedding layers on or off for the process; returns what it was.  On: KFAC and Diagonal accept
    ``'Embedding'`` in `layer_types` by name (it never enters the default selection), `factor_jobs` routes the layer to an
    `EmbeddingFactorJob` (the token histogram: the exactly diagonal A factor of a bias-free Linear on one-hot rows) and the
    flat build of grad_output, and `per_sample_route` answers ``"embedding"``.  Off: the layer is refused where it was."""
    global _EMBEDDING
    was, _EMBEDDING = _EMBEDDING, bool(enable)
    return was


def embedding_admitted() -> bool:
    return _EMBEDDING


def is_embedding_layer(layer) -> bool:
    """An nn.Embedding while `admit_embedding` is on."""
    return _EMBEDDING and layer.__class__.__name__ == 'Embedding'


def _embedding_indices(t, name: str):
    """The index record of an Embedding as the kernels read it: int64 or int32, contiguous (read in place if it is, copied
    by torch otherwise); a `ShapeOnly` stays one."""
    if t.dtype not in _INDEX_DTYPES:
        raise RuntimeError(f"{name}: an Embedding expects int64 or int32 indices, got {t.dtype}")
    if len(t.shape) < 1 or math.prod(t.shape) < 1:
        raise RuntimeError(f"{name}: empty index record {tuple(t.shape)}")
    return t if isinstance(t, ShapeOnly) else t.detach().contiguous()


def _embedding_jobs(layer, x, g, name: Optional[str] = None) -> "LayerJobs":
    """`factor_jobs` of an nn.Embedding (`admit_embedding`): the A side an `EmbeddingFactorJob` on the (N, *) indices, the G
    side the flat build of grad_output seen as (N T, D), routed by its dtype like a Linear's.  n = V, m = D; the positions
    count as the expand build of a Linear on tokens counts them: N T rows of one position each."""
    name = name or repr(layer)
    if x is None and g is None:
        raise RuntimeError("KFAC.update: no recorded forward/backward pass for a selected layer")
    V, D = int(layer.num_embeddings), int(layer.embedding_dim)
    a_job = g_job = None
    if x is not None:
        x = _embedding_indices(x, name)
        a_job = EmbeddingFactorJob(_job_source(x), None, V, layer.padding_idx, i64=x.dtype == torch.int64)
    if g is not None:
        if g.shape[-1] != D or (x is not None and tuple(g.shape[:-1]) != tuple(x.shape)):
            raise RuntimeError(f"{name}: grad_output {tuple(g.shape)} does not match the indices "
                               f"{None if x is None else tuple(x.shape)} and embedding_dim {D}")
        g = _factor_source(g, fp32=False, flatten=True)
        src = _job_source(g)
        g_job = FactorJob(src, None) if g.dtype == torch.float32 else HalfFactorJob(src, None, dtype=g.dtype)
    rows = math.prod(x.shape) if x is not None else g.shape[0]
    return LayerJobs(a_job, g_job, V, D, rows, 1, 1)


class ConvView(NamedTuple):
    """`conv_view` of a convolution layer: its 2-D window and its records as 4-D tensors."""
    kernel: tuple
    stride: tuple
    padding: tuple
    dilation: tuple
    x: object
    g: object
    depth: Optional[tuple]


def _reshaped(t, dims: int, shape_of):
    """The record `t` (tensor, `ShapeOnly` or None) of `dims` dimensions with the shape `shape_of(its shape)`: a view where
    the strides allow one.  A record of another rank is handed on as it is (the caller's own check names it)."""
    if t is None or len(t.shape) != dims:
        return t
    shape = shape_of(tuple(int(v) for v in t.shape))
    return ShapeOnly(shape, t.dtype) if isinstance(t, ShapeOnly) else t.reshape(shape)


def conv_view(layer, x=None, g=None) -> ConvView:
    """The 2-D geometry of a convolution layer and the 4-D views of its records (tensors, `ShapeOnly`s or None) - the one
    place that knows how the convolution kinds map onto the (N, C, H, W) builds:
    Conv2d / ConvTranspose2d: themselves.  Conv1d (`admit_conv_nd`): the Conv2d with H = 1 - kernel (1, k), stride (1, s),
    padding (0, p), dilation (1, d), records (N, C, L) seen as (N, C, 1, L) (views: the strides of the record stay).
    Conv3d (`admit_conv_nd`): the window (kh, kw) / (sh, sw) / (ph, pw) of the depth-unfolded stack, `depth` =
    (kd, sd, pd); grad_output (N, Cout, Do, Ho, Wo) seen as (N, Cout, Do Ho, Wo), the input left as (N, C, D, H, W) - the
    gather of curv_kfac_conv3d_accumulate reads it.  `dilation` is what the layer says (whether it is honoured is the
    caller's business)."""
    kind = layer.__class__.__name__
    kernel, stride, padding, dilation = (tuple(v) if not isinstance(v, str) else v
                                         for v in (layer.kernel_size, layer.stride, layer.padding, layer.dilation))
    if kind not in _ND_KINDS:
        return ConvView(kernel, stride, padding, dilation, x, g, None)
    if not _CONV_ND:
        raise NotImplementedError(f"{kind} layers are not supported (ops.admit_conv_nd() admits Conv1d and Conv3d)")
    if int(layer.groups) != 1:
        raise NotImplementedError(f"grouped {kind} (groups={layer.groups}) is not supported")
    if isinstance(padding, str):
        raise NotImplementedError(f"{kind} with string padding is not supported")
    if layer.padding_mode != 'zeros':
        raise NotImplementedError(f"{kind} with padding_mode={layer.padding_mode!r} is not supported")
    if kind == 'Conv1d':
        wide = lambda s: s[:2] + (1, s[2])
        return ConvView((1,) + kernel, (1,) + stride, (0,) + padding, (1,) + dilation, _reshaped(x, 3, wide),
                        _reshaped(g, 3, wide), None)
    if dilation != (1, 1, 1):
        raise NotImplementedError(f"dilated Conv3d (dilation {dilation}) is not supported")
    return ConvView(kernel[1:], stride[1:], padding[1:], (1, 1), x,
                    _reshaped(g, 5, lambda s: s[:2] + (s[2] * s[3], s[4])), (kernel[0], stride[0], padding[0]))


class LayerJobs(NamedTuple):
    """The two factor builds of one layer (`factor_jobs`): `a` / `g` the job of the A / G side (None without a source),
    `n` / `m` the widths of A / G (of one group's, for a grouped layer), `N` samples of `L` positions each."""
    a: object
    g: object
    n: int
    m: int
    N: int
    L: int
    groups: int

    @property
    def K(self) -> int:
        """Columns summed over by either side."""
        return self.N * self.L


class ShapeOnly(NamedTuple):
    """Stand-in for a recorded tensor where `factor_jobs` is asked for a plan only: its shape and dtype."""
    shape: tuple
    dtype: torch.dtype = torch.float32


def _factor_source(t, fp32: bool, flatten: bool):
    """A recorded activation / gradient as the factor build takes it: contiguous; float32 or (ordinary layers)
    bfloat16 / float16.  A grouped layer's half-precision side becomes a float32 copy on the device: the grouped build
    (curv_kfac_group_accumulate) has no half-precision form; neither has the transposed-convolution A-side build
    (`fp32`).  `flatten`: the (N, *, in) input of a Linear layer as (rows, in).  A `ShapeOnly` stays one."""
    if t is None:
        return None
    if t.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise RuntimeError(f"KFAC.update expects float32, bfloat16 or float16 activations and gradients, got {t.dtype}")
    if isinstance(t, ShapeOnly):
        shape = tuple(t.shape)
        if flatten and len(shape) != 2:
            shape = (math.prod(shape[:-1]), shape[-1])
        return ShapeOnly(shape, torch.float32 if fp32 else t.dtype)
    t = t.detach()
    if fp32 and t.dtype != torch.float32:
        t = t.float()
    t = t.contiguous()
    if flatten and t.dim() != 2:
        t = t.reshape(-1, t.shape[-1])
    return t


def _job_source(t):
    """The `src` of a job for the record `t`: the tensor itself, or the shape of a `ShapeOnly`."""
    return tuple(t.shape) if isinstance(t, ShapeOnly) else t


def _conv_out_size(shape, kernel, stride, padding, dilation=None) -> tuple:
    """The output size of a convolution over an (N, C, *spatial) input of `shape`: what a layer without a recorded
    gradient takes its positions from."""
    dilation = dilation or (1,) * len(kernel)
    return tuple((shape[2 + d] + 2 * padding[d] - dilation[d] * (kernel[d] - 1) - 1) // stride[d] + 1
                 for d in range(len(kernel)))


def _reduce_jobs(layer, x, g) -> LayerJobs:
    """`factor_jobs` for ``approximation="reduce"``: a Linear layer on 2-D records has one position per
    sample, where both forms coincide - today's jobs; a Linear layer on (N, *, in) records gets token-form jobs with N the
    first dimension and L the product of the middle ones; a Conv2d (groups 1, dilation 1, integer padding) gets plane-form
    jobs, also when L = 1.  Either dtype goes to the same job: the reduce pass upcasts."""
    kind = layer.__class__.__name__
    if x is None and g is None:
        raise RuntimeError("KFAC.update: no recorded forward/backward pass for a selected layer")
    has_bias = getattr(layer, "bias", None) is not None
    if kind == 'Linear':
        if len((x if x is not None else g).shape) == 2:
            return factor_jobs(layer, x, g)
        jobs = []
        for t, bias, mean in ((x, has_bias, True), (g, False, False)):
            t = _factor_source(t, fp32=False, flatten=False)
            if t is None:
                jobs.append(None)
                continue
            if len(t.shape) < 3:
                raise RuntimeError("KFAC.update: the records of a Linear layer must both be (N, in) or both (N, *, in)")
            N, L, E = t.shape[0], math.prod(t.shape[1:-1]), t.shape[-1]
            src = (N, L, E) if isinstance(t, ShapeOnly) else t.reshape(N, L, E)
            jobs.append(ReduceFactorJob(src, None, has_bias=bias, form=_lib.REDUCE_TOKEN, mean=mean, dtype=t.dtype))
        return LayerJobs(jobs[0], jobs[1], layer.in_features + int(has_bias), layer.out_features, N, L, 1)
    if kind == 'Conv3d' and _CONV_ND:
        raise NotImplementedError('approximation="reduce" does not take a 3-D convolution (Conv3d): the reduce pass has no '
                                  'depth window; approximation="expand" takes it')
    if kind != 'Conv2d' and not (kind == 'Conv1d' and _CONV_ND):
        raise NotImplementedError(f'approximation="reduce" does not take a {kind} layer; approximation="expand" does')
    if int(layer.groups) != 1 or any(d != 1 for d in layer.dilation) or not all(isinstance(p, int) for p in layer.padding):
        raise NotImplementedError(f'approximation="reduce" takes a {kind} with groups 1, dilation 1 and integer padding, '
                                  f'got groups={layer.groups}, dilation={tuple(layer.dilation)}, padding={layer.padding}; '
                                  f'approximation="expand" takes grouped and dilated layers')
    view = conv_view(layer, _factor_source(x, fp32=False, flatten=False), _factor_source(g, fp32=False, flatten=False))
    x, g = view.x, view.g
    for t in (x, g):
        if t is not None and len(t.shape) != 4:
            raise RuntimeError("KFAC.update: Conv2d records must be (N, C, H, W)" if kind == 'Conv2d' else
                               "KFAC.update: Conv1d records must be (N, C, L)")
    kernel, stride, padding = view.kernel, view.stride, view.padding
    out_size = tuple(g.shape[2:]) if g is not None else _conv_out_size(x.shape, kernel, stride, padding)
    a_job = g_job = None
    if x is not None:
        a_job = ReduceFactorJob(_job_source(x), None, kernel, stride, padding, has_bias, mean=True, dtype=x.dtype)
    if g is not None:
        g_job = ReduceFactorJob(_job_source(g), None, mean=False, dtype=g.dtype)
    return LayerJobs(a_job, g_job, layer.in_channels * kernel[0] * kernel[1] + int(has_bias), layer.out_channels,
                     (x if x is not None else g).shape[0], out_size[0] * out_size[1], 1)


def _conv3d_jobs(layer, x, g, has_bias: bool) -> LayerJobs:
    """`factor_jobs` of a Conv3d (`admit_conv_nd`; `x` float32, both contiguous): the A side to `Conv3dFactorJob` on the
    (N, C, D, H, W) input; the G side a 1x1 factor of grad_output seen as (N, Cout, Do Ho, Wo), routed by its dtype.
    L = Do Ho Wo, n = Cin kd kh kw [+ 1], m = Cout."""
    kernel, stride, padding = (tuple(v) for v in (layer.kernel_size, layer.stride, layer.padding))
    if x is not None and len(x.shape) != 5:
        raise RuntimeError("KFAC.update: Conv3d inputs must be (N, C, D, H, W)")
    if g is not None and len(g.shape) != 5:
        raise RuntimeError("KFAC.update: Conv3d gradients must be (N, C, D, H, W)")
    a_job = g_job = None
    if x is not None:
        a_job = Conv3dFactorJob(_job_source(x), None, kernel, stride, padding, has_bias)
    if g is not None:
        L = math.prod(g.shape[2:])
        g = conv_view(layer, None, g).g
        src = _job_source(g)
        g_job = FactorJob(src, None) if g.dtype == torch.float32 else HalfFactorJob(src, None, dtype=g.dtype)
    else:
        L = math.prod(_conv_out_size(x.shape, kernel, stride, padding))
    return LayerJobs(a_job, g_job, layer.in_channels * math.prod(kernel) + int(has_bias), layer.out_channels,
                     (x if x is not None else g).shape[0], L, 1)


def factor_jobs(layer, x, g, out_size=None, approximation="expand") -> LayerJobs:
    """Which build each side of a selected layer goes to, and with which geometry: the one place that knows the layer
    kinds (Linear and attention projections, Conv2d, grouped Conv2d, ConvTranspose2d) and the dtype routing.
    `approximation`: "expand" (every position of a weight-sharing layer is a column of the Gram: what follows) or "reduce"
    (the positions are reduced first: `ReduceFactorJob`s, see `_reduce_jobs`).

    `x` / `g`: the recorded input / grad_output (either may be None: that side gets no job) or `ShapeOnly`
    stand-ins (the jobs' `src` is then a shape: plan queries).  Each side is routed by its dtype: float32 to `FactorJob`,
    bfloat16 / float16 to `HalfFactorJob`; both sides of a grouped convolution to `GroupFactorJob` and the A side of a
    transposed convolution to `ConvTFactorJob`, as float32; with `admit_dilated` the A side of a dilated groups-1 Conv2d
    to `DilatedFactorJob`, as float32 too (without it the dilation is not looked at, as before).  With `admit_conv_nd` a
    Conv1d (groups 1) is routed as the Conv2d of `conv_view` - its records seen as (N, C, 1, L) - and the A side of a Conv3d
    goes to `Conv3dFactorJob`, as float32, its G side to the 1x1 job of grad_output seen as (N, Cout, Do Ho, Wo)
    (`_conv3d_jobs`).  `out_size`: the output size a ConvTranspose2d forward was
    seen to produce (it carries the effective output_padding), used when there is no `g` to read it from.  The jobs come
    without `dst`, `scale` and `first`."""
    if is_norm_layer(layer) or is_embedding_layer(layer):
        if approximation == "reduce":
            raise NotImplementedError(f'approximation="reduce" does not take a {layer.__class__.__name__} layer; '
                                      f'approximation="expand" does')
        return _norm_jobs(layer, x, g) if is_norm_layer(layer) else _embedding_jobs(layer, x, g)
    if approximation == "reduce":
        return _reduce_jobs(layer, x, g)
    if approximation != "expand":
        raise ValueError(f'approximation must be "expand" or "reduce", got {approximation!r}')
    kind = layer.__class__.__name__
    nd = _CONV_ND and kind in _ND_KINDS                  # a Conv1d rides the Conv2d route through its (N, C, 1, L) view
    conv, convt = kind in ('Conv2d', 'ConvTranspose2d') or nd, kind == 'ConvTranspose2d'
    groups = int(layer.groups) if kind == 'Conv2d' else 1
    has_bias = layer.bias is not None
    dilation = tuple(layer.dilation) if _DILATED and kind == 'Conv2d' else (1, 1)
    depth = None
    if nd:
        view = conv_view(layer)                          # (refuses what neither kind can be: groups, string padding ...)
        depth = view.depth                               # (kd, sd, pd) of a Conv3d
        if view.dilation != (1, 1):
            if not _DILATED:
                raise NotImplementedError(f"dilated {kind} (dilation {tuple(layer.dilation)}) is not supported "
                                          f"(ops.admit_dilated() admits a dilated Conv1d)")
            dilation = view.dilation
    if dilation != (1, 1) and groups > 1:
        raise NotImplementedError(f"dilated convolution with groups > 1 (groups={groups}) is not supported")
    x = _factor_source(x, fp32=groups > 1 or convt or dilation != (1, 1) or depth is not None, flatten=not conv)
    g = _factor_source(g, fp32=groups > 1, flatten=not conv)
    if x is None and g is None:
        raise RuntimeError("KFAC.update: no recorded forward/backward pass for a selected layer")
    if depth is not None:
        return _conv3d_jobs(layer, x, g, has_bias)
    if conv:
        kernel, stride, padding = layer.kernel_size, layer.stride, layer.padding
        if nd:                                           # the 2-D geometry and the (N, C, 1, L) views of a Conv1d
            view = conv_view(layer, x, g)
            kernel, stride, padding, x, g = view.kernel, view.stride, view.padding, view.x, view.g
            if any(t is not None and len(t.shape) != 4 for t in (x, g)):
                raise RuntimeError(f"KFAC.update: {kind} records must be (N, C, L)")
        C, m = layer.in_channels // groups, layer.out_channels // groups
        if convt and x is not None and len(x.shape) != 4:
            raise RuntimeError("KFAC.update: ConvTranspose2d inputs must be (N, C, H, W)")
        if g is not None:
            out_size = tuple(g.shape[2:])
        elif not convt:
            out_size = _conv_out_size(x.shape, kernel, stride, padding, dilation)
        elif out_size is None:                           # records that did not pass the estimator's hooks
            out_size = tuple((x.shape[2 + d] - 1) * stride[d] - 2 * padding[d] + kernel[d] +
                             layer.output_padding[d] for d in range(2))
    else:
        C, m = layer.in_features, layer.out_features
        kernel, stride, padding, out_size = (1, 1), (1, 1), (0, 0), (1, 1)
    a_job = g_job = None
    if x is not None:
        src = _job_source(x)
        if groups > 1:
            a_job = GroupFactorJob(src, None, groups, kernel, stride, padding, has_bias)
        elif convt:
            a_job = ConvTFactorJob(src, None, kernel, stride, padding, out_size, has_bias)
        elif dilation != (1, 1):
            a_job = DilatedFactorJob(src, None, kernel, stride, padding, dilation, has_bias)
        elif x.dtype == torch.float32:
            a_job = FactorJob(src, None, kernel, stride, padding, has_bias)
        else:
            a_job = HalfFactorJob(src, None, kernel, stride, padding, has_bias, dtype=x.dtype)
    if g is not None:
        src = _job_source(g)
        if groups > 1:
            g_job = GroupFactorJob(src, None, groups)
        elif g.dtype == torch.float32:
            g_job = FactorJob(src, None)
        else:
            g_job = HalfFactorJob(src, None, dtype=g.dtype)
    return LayerJobs(a_job, g_job, C * kernel[0] * kernel[1] + int(has_bias), m,
                     (x if x is not None else g).shape[0], out_size[0] * out_size[1], groups)


class PackSource(NamedTuple):
    """Where `per_sample_pack` reads an operand: the source seen as ``(N, C, H, W)`` with element `strides`
    ``(s_n, s_c, s_h, s_w)`` (the tensor itself gives the address, the dtype and the extent), the window, and `out_size`
    ``(Ho, Wo)`` for the transposed gather of a ConvTranspose2d input (None: the forward im2col, with `dilation`).  The
    record of a Conv3d (`admit_conv3d_per_sample`): `shape` ``(N, C, D, H, W)``, five `strides`, and `kernel`, `stride`
    and `padding` as 3-tuples (depth first); `out_size` None and `dilation` (1, 1)."""
    shape: tuple
    kernel: tuple
    stride: tuple
    padding: tuple
    has_bias: bool
    strides: tuple
    out_size: Optional[tuple]
    dilation: tuple = (1, 1)


def _pack_source(shape, strides, kernel=(1, 1), stride=(1, 1), padding=(0, 0), has_bias=False, out_size=None,
                 dilation=(1, 1)) -> PackSource:
    return PackSource(tuple(map(int, shape)), tuple(kernel), tuple(stride), tuple(padding), bool(has_bias),
                      tuple(map(int, strides)), None if out_size is None else tuple(map(int, out_size)),
                      tuple(map(int, dilation)))


def _is_contiguous_nchw(geometry: PackSource) -> bool:
    """The strides are those of a contiguous (N, C, H, W) - or (N, C, D, H, W) - tensor (the stride of a dimension of size 1
    addresses nothing)."""
    dense = [math.prod(geometry.shape[k + 1:]) for k in range(len(geometry.shape))]
    return all(d == 1 or s == w for d, s, w in zip(geometry.shape, geometry.strides, dense))


class PerSampleOperand(NamedTuple):
    """One side of P_n = g_n X_n^T as `per_sample_sq_accumulate` reads it: `rows` rows of `L` values per sample, sample
    `n` row `r` at ``ns * n + rs * r`` floats.  `pack` is None where the record `src` is read in place, otherwise the
    `PackSource` of the copy `per_sample_pack` writes (`floats` of scratch, rows of `Lp` values with a zero tail,
    `rows_outer`: (rows, N, Lp) instead of (N, rows, Lp)); `src` is then float32, bfloat16 or float16 and may be any view
    with non-negative strides."""
    src: object
    rows: int
    L: int
    Lp: int
    ns: int
    rs: int
    pack: Optional[PackSource]
    rows_outer: bool
    floats: int


class PerSampleSides(NamedTuple):
    """`per_sample_operands` of one layer: the `g` (m rows) and `x` (n rows, ones row included) operands of `N` samples."""
    g: PerSampleOperand
    x: PerSampleOperand
    n: int
    m: int
    N: int
    L: int


# The wider per-sample line is opt-in: with it off - the default - the per-sample selection, its refusals
# and their messages are exactly what they were.
_WIDE = False


def widen_per_sample(enable: bool = True) -> bool:
    """Switch the wider per-sample line on or off for the process; returns what it was.  On: `per_sample_operands`, the
    exact Fisher of Diagonal / EFB (``per_sample=True``) and the linearised predictive take bfloat16 / float16 records
    (a model run under ``torch.autocast``; each side by its own dtype), ConvTranspose2d layers and, for KFAC and EFB, the
    two projections of a MultiheadAttention module.  Off: float32 records of Linear and Conv2d only; the others raise."""
    global _WIDE
    was, _WIDE = _WIDE, bool(enable)
    return was


def per_sample_is_wide() -> bool:
    return _WIDE


def per_sample_dtype_fault(what: str, t) -> Optional[str]:
    """Why the record `t` cannot enter the per-sample line (None: it can): float32 always; bfloat16 / float16 with
    `widen_per_sample`; nothing else."""
    if t.dtype == torch.float32 or (_WIDE and t.dtype in _PACK_DTYPES):
        return None
    if t.dtype in _PACK_DTYPES:
        return f"{what} expects float32 records, got {t.dtype} (ops.widen_per_sample() admits bfloat16 / float16)"
    return f"{what} expects float32" + (", bfloat16 or float16" if _WIDE else "") + f" records, got {t.dtype}"


# Grouped and depthwise convolutions in the per-sample line are opt-in as well, by a switch of their own:
# with it off - the default - selection, refusals and messages are exactly what they were, whatever `widen_per_sample` says.
_GROUPS = False


def admit_grouped_per_sample(enable: bool = True) -> bool:
    """Switch grouped convolutions in the per-sample line on or off for the process; returns what it was.  On:
    ``Diagonal(per_sample=True)`` and the `functional_variance` of Diagonal and KFAC take a Conv2d with ``groups > 1``
    (dilation 1, integer padding, float32 records) by the route `per_sample_route` names.  Off: such a layer raises.
    Independent of `widen_per_sample`.  The other linearised predictives (`stage_output` / `functional_covariance`,
    `functional_variance_grid`) take such a layer with `admit_grouped_joint` on as well; EFB, INF and
    ``ConvTranspose2d(groups > 1)`` refuse it either way."""
    global _GROUPS
    was, _GROUPS = _GROUPS, bool(enable)
    return was


def per_sample_admits_groups() -> bool:
    return _GROUPS


# The joint covariance and the damping grid of grouped convolutions have a switch of their own again: off -
# the default - `stage_output`, `functional_variance_grid` and `KFAC.decompose` are exactly what they were.
_GROUPS_JOINT = False


def admit_grouped_joint(enable: bool = True) -> bool:
    """Switch grouped convolutions in `stage_output` / `functional_covariance`, `functional_variance_grid` and
    `KFAC.decompose` on or off for the process; returns what it was.  It has an effect only while
    `admit_grouped_per_sample` is on as well: alone it admits nothing."""
    global _GROUPS_JOINT
    was, _GROUPS_JOINT = _GROUPS_JOINT, bool(enable)
    return was


def per_sample_admits_grouped_joint() -> bool:
    return _GROUPS_JOINT


DW_MAX_TAPS = 49                       # kernel taps up to which a depthwise layer takes the direct kernel


def per_sample_route(layer) -> str:
    """How the per-sample products of `layer` are formed (host only; the one place that decides it): ``"whole"`` - one
    product P_n = g_n X_n^T (every layer but a grouped Conv2d); ``"depthwise"`` - the direct kernel of
    csrc/persample_dw.hip (in_channels == out_channels == groups, at most `DW_MAX_TAPS` kernel taps); ``"slices"`` - one
    product per group on channel slices of the records (`GroupSlice`: every other grouped Conv2d); ``"norm"`` - the fused
    pass of csrc/norm_factor.hip (LayerNorm, GroupNorm, BatchNorm2d while `admit_norm_layers` is on); ``"embedding"`` - the
    segment walker of csrc/embedding_factor.hip (nn.Embedding while `admit_embedding` is on)."""
    if is_norm_layer(layer):
        return "norm"
    if is_embedding_layer(layer):
        return "embedding"
    if layer.__class__.__name__ != 'Conv2d' or int(layer.groups) == 1:
        return "whole"
    if layer.in_channels == layer.out_channels == int(layer.groups) and \
            layer.kernel_size[0] * layer.kernel_size[1] <= DW_MAX_TAPS:
        return "depthwise"
    return "slices"


class GroupSlice(NamedTuple):
    """Group `g` of a grouped Conv2d `layer` as a layer of its own in the per-sample line (a pseudo-layer like
    `AttentionProjection`; hashable, equal by (layer, g)): the convolution of the input channels
    [g c_g, (g + 1) c_g) to the output channels [g m_g, (g + 1) m_g), rows [g m_g, (g + 1) m_g) of the layer matrix."""
    layer: object
    g: int

    @property
    def rows(self) -> slice:
        m = self.layer.out_channels // int(self.layer.groups)
        return slice(self.g * m, (self.g + 1) * m)

    @staticmethod
    def of(layer) -> list:
        return [GroupSlice(layer, g) for g in range(int(layer.groups))]


def per_sample_items(layers) -> list:
    """`layers` with every grouped layer of the ``"slices"`` route replaced by its `GroupSlice`s, in group order."""
    out = []
    for layer in layers:
        out.extend(GroupSlice.of(layer) if per_sample_route(layer) == "slices" else [layer])
    return out


def grouped_dtype_fault(name: str, t) -> Optional[str]:
    """Why the record `t` of the grouped layer `name` cannot enter the per-sample line (None: it can): float32 only,
    whatever `widen_per_sample` says."""
    if t.dtype == torch.float32:
        return None
    return f"per-sample update: grouped convolution {name} expects float32 records, got {t.dtype}"


_PACK_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}


def _per_sample_operand(src, geometry: PackSource, in_place: bool, rows_outer: bool) -> PerSampleOperand:
    """`in_place` is the caller's wish; it holds only for a float32 source that is that very matrix in memory."""
    kernel, stride, padding = geometry.kernel, geometry.stride, geometry.padding
    N, C = geometry.shape[:2]
    if geometry.out_size is not None:
        L = geometry.out_size[0] * geometry.out_size[1]
    else:                                                  # every windowed axis: two of a 4-D record, three of a 5-D one
        dilation = (1,) * (len(kernel) - 2) + tuple(geometry.dilation)
        L = math.prod((size + 2 * p - d * (k - 1) - 1) // s + 1
                      for size, k, s, p, d in zip(geometry.shape[2:], kernel, stride, padding, dilation))
    rows = C * math.prod(kernel) + int(geometry.has_bias)
    if in_place and src.dtype == torch.float32 and _is_contiguous_nchw(geometry):
        return PerSampleOperand(src, rows, L, L, rows * L, L, None, False, 0)
    Lp = (L + 3) // 4 * 4
    ns, rs = (Lp, N * Lp) if rows_outer else (rows * Lp, Lp)
    return PerSampleOperand(src, rows, L, Lp, ns, rs, geometry, rows_outer, N * rows * Lp)


def _token_major(what: str, t, N: Optional[int]):
    """The record of an attention projection as (T, N, E): the attention forward hands F.linear a (T, N, E) tensor
    (input projection) or (T N, E) rows t N + n (output projection, `N` from the module's input projection)."""
    if t.dim() == 3:
        return t
    if t.dim() == 2 and N is not None and N >= 1 and t.shape[0] % N == 0:
        return t.view(t.shape[0] // N, N, t.shape[1]) if t.is_contiguous() else t.reshape(t.shape[0] // N, N, t.shape[1])
    if t.dim() == 2 and N is None:
        raise RuntimeError(f"per-sample update: {what}: unbatched (T, E) attention input is not supported (the record "
                           f"{tuple(t.shape)} has no sample dimension); pass a batch of one")
    raise RuntimeError(f"per-sample update: {what}: record {tuple(t.shape)} does not fit {N} samples")


def per_sample_operands(layer, x, g, rows_outer: bool = False, in_place: bool = True,
                        samples: Optional[int] = None) -> PerSampleSides:
    """The step from a layer's records `(x, g)` to the operands of its per-sample gradients P_n = g_n X_n^T, on the
    geometry of `factor_jobs`.

    Conv2d (groups 1; dilation 1, or any with `admit_dilated`): g_n = grad_output[n] as (m, Ho Wo), X_n = unfold(x[n])
    [+ ones row].  ConvTranspose2d
    (groups 1, dilation 1): g_n likewise, X_n the transposed gather (row (ci, a, b) at (oh, ow) is
    x[n, ci, (oh + ph - a) / sh, (ow + pw - b) / sw] where that is a whole position inside the input, else 0) - the column
    order of Wm; the output size is grad_output's.  Linear: g_n = grad_output[n]^T (m, T), X_n = x[n]^T [+ ones row] (D [+ 1], T)
    with T the product of the middle dimensions (1 for an (N, D) input).  Conv3d (`admit_conv_nd` and
    `admit_conv3d_per_sample`; groups 1, dilation 1): g_n = grad_output[n] as (m, Do Ho Wo), X_n the 3-D im2col of x[n]
    [+ ones row], rows in the order of ``weight.reshape(Cout, -1)``; the records are read through their five strides, in
    place under the rule below (the input of a bias-free 1x1x1 / stride-1 one), and a side of 2^31 bytes or more raises
    RuntimeError naming the largest batch that fits.  The sample is the leading index, as in
    `KFAC.update` - except for an `AttentionProjection` (curvatures.py), whose records are token-major: (T, N, E), or
    (T N, E) for the output projection with `samples` = N; they are read through strides, not transposed.  An operand is
    read in place where the record already is that matrix in float32, rows contiguous and a whole number of 16-byte groups
    long (grad_output of a convolution; the input of a bias-free 1x1 / stride-1 one); everything else names the pack that
    writes it.  `rows_outer` / ``in_place=False``: every operand packed as one (rows, N Lp) matrix (EFB rotates it with
    one product).  float32 records; with `widen_per_sample` each side float32, bfloat16 or float16 by its own dtype (an
    autocast ResNet-50 has a float32 stem input and a bfloat16 grad_output): a half side is always packed - the pack
    upcasts it - and never read in place.  Any other dtype raises RuntimeError.  Views are not copied: the pack reads
    them through their strides.  A grouped Conv2d itself raises NotImplementedError; with `admit_grouped_per_sample` one
    group of it, a `GroupSlice`, is a layer here (`_slice_operands`)."""
    if isinstance(layer, GroupSlice):
        if not _GROUPS:
            raise NotImplementedError("per-sample update: unsupported layer GroupSlice")
        return _slice_operands(layer, x.detach(), g.detach(), rows_outer, in_place)
    for t in (x, g):
        fault = per_sample_dtype_fault("per-sample update", t)
        if fault:
            raise RuntimeError(fault)
    kind = layer.__class__.__name__
    x, g = x.detach(), g.detach()
    if kind == 'AttentionProjection':
        what = f"attention projection '{layer.kind}'"
        x, g = _token_major(what, x, samples), _token_major(what, g, samples)
        if x.shape[:2] != g.shape[:2]:
            raise RuntimeError(f"per-sample update: {what}: records do not match (input {tuple(x.shape)}, grad_output "
                               f"{tuple(g.shape)})")
    conv3d = kind == 'Conv3d' and _CONV_ND and _CONV3D_PER_SAMPLE
    if conv3d and (x.dim() != 5 or g.dim() != 5):
        raise RuntimeError(f"per-sample update: records of Conv3d must be (N, C, D, H, W), got {tuple(x.shape)} and "
                           f"{tuple(g.shape)}")
    sides = factor_jobs(layer, ShapeOnly(tuple(x.shape)), ShapeOnly(tuple(g.shape)))
    if sides.groups != 1 or not isinstance(sides.a, (FactorJob, ConvTFactorJob, DilatedFactorJob) +
                                           ((Conv3dFactorJob,) if conv3d else ())):
        raise NotImplementedError(f"per-sample update: unsupported layer {kind}")
    has_bias = sides.a.has_bias
    if conv3d:
        # the records themselves, through their five strides (a channels_last_3d record or a channel slice is not copied):
        # the X side is the 3-D im2col the pack writes per sample, the g side grad_output as (m, Do Ho Wo)
        N, Ng = int(x.shape[0]), int(g.shape[0])
        one, none = (1, 1, 1), (0, 0, 0)
        geo_x = _pack_source(x.shape, x.stride(), sides.a.kernel, sides.a.stride, sides.a.padding, has_bias)
        geo_g = _pack_source(g.shape, g.stride(), one, one, none)
        whole = in_place and math.prod(g.shape[2:]) % 4 == 0
        plain = (sides.a.kernel, sides.a.stride, sides.a.padding) == (one, one, none) and not has_bias
        x_op = _per_sample_operand(x, geo_x, whole and plain, rows_outer)
        g_op = _per_sample_operand(g, geo_g, whole, rows_outer)
        for side, op in (("x", x_op), ("g", g_op)):
            size = N * op.rows * op.Lp * 4                 # the product kernels address an operand in 31 bits
            if size >= 1 << 31:
                fits = ((1 << 31) - 1) // (op.rows * op.Lp * 4)
                raise RuntimeError(f"per-sample update: the {side} operand of Conv3d is too large for the per-sample "
                                   f"products: N {N} x rows {op.rows} x Lp {op.Lp} float32 values are {size} bytes, 2^31 or "
                                   f"more; the largest batch that fits is {fits}")
    elif kind in ('Conv2d', 'ConvTranspose2d') or (_CONV_ND and kind == 'Conv1d'):
        if kind == 'Conv1d':                               # read through its (N, C, 1, L) views: nothing is copied
            if x.dim() != 3 or g.dim() != 3:
                raise RuntimeError(f"per-sample update: records of Conv1d must be (N, C, L), got {tuple(x.shape)} and "
                                   f"{tuple(g.shape)}")
            view = conv_view(layer, x, g)
            x, g = view.x, view.g
        if x.dim() != 4 or g.dim() != 4:
            raise RuntimeError(f"per-sample update: records of {kind} must be (N, C, H, W), got {tuple(x.shape)} and "
                               f"{tuple(g.shape)}")
        N, Ng = int(x.shape[0]), int(g.shape[0])
        Ho, Wo = map(int, g.shape[2:])
        geo_x = _pack_source(x.shape, x.stride(), sides.a.kernel, sides.a.stride, sides.a.padding, has_bias,
                             (Ho, Wo) if kind == 'ConvTranspose2d' else None, getattr(sides.a, "dilation", (1, 1)))
        geo_g = _pack_source(g.shape, g.stride())
        whole = in_place and (Ho * Wo) % 4 == 0
        plain = kind == 'Conv2d' and sides.a.kernel == (1, 1) and sides.a.stride == (1, 1) and \
            sides.a.padding == (0, 0) and not has_bias
        x_op = _per_sample_operand(x, geo_x, whole and plain, rows_outer)
        g_op = _per_sample_operand(g, geo_g, whole, rows_outer)
    else:
        if kind == 'AttentionProjection':                  # (T, N, E): the sample is the middle index
            N = Ng = int(x.shape[1])
            views = [(t, (N, int(t.shape[2]), int(t.shape[0]), 1), (t.stride(1), t.stride(2), t.stride(0), 1)) for t in (x, g)]
        else:                                              # (N, *, D) as (N, T, D): X_n = x[n]^T
            N, Ng = int(x.shape[0]), int(g.shape[0])
            T = math.prod(x.shape[1:-1])
            x, g = x.reshape(N, T, x.shape[-1]), g.reshape(int(g.shape[0]), -1, g.shape[-1])
            views = [(t, (int(t.shape[0]), int(t.shape[2]), int(t.shape[1]), 1), (t.stride(0), t.stride(2), t.stride(1), 1))
                     for t in (x, g)]
        (x, shape_x, strides_x), (g, shape_g, strides_g) = views
        x_op = _per_sample_operand(x, _pack_source(shape_x, strides_x, has_bias=has_bias), False, rows_outer)
        g_op = _per_sample_operand(g, _pack_source(shape_g, strides_g), False, rows_outer)
    if g_op.L != x_op.L or g_op.rows != sides.m or x_op.rows != sides.n or Ng != N:
        raise RuntimeError(f"per-sample update: records of {kind} do not match the layer "
                           f"(input {tuple(x.shape)}, grad_output {tuple(g.shape)})")
    return PerSampleSides(g_op, x_op, sides.n, sides.m, N, x_op.L)


def _slice_operands(item: GroupSlice, x, g, rows_outer: bool, in_place: bool) -> PerSampleSides:
    """`per_sample_operands` of one group of a grouped Conv2d (`admit_grouped_per_sample`): the geometry of `factor_jobs`
    with C = c_g and m = m_g on the channel slices of the two records, which are neither copied nor made contiguous.
    The g side ``grad_output[:, g m_g:(g + 1) m_g]`` is read in place under the rule of every layer (float32 - the only dtype
    a grouped layer takes -, the record contiguous, L % 4 == 0: the slice then starts on a 16-byte boundary), with the
    record's own sample stride; otherwise the pack reads the view through its strides.  The x side is the view
    ``x[:, g c_g:(g + 1) c_g]``: packed (its ones row written per slice), or read in place for a bias-free 1x1 / stride-1
    layer.  An operand read in place has as `src` the flat run from the slice's first element to the record's end."""
    layer, k = item.layer, int(item.g)
    for t in (x, g):
        fault = grouped_dtype_fault(repr(item), t)
        if fault:
            raise RuntimeError(fault)
    if x.dim() != 4 or g.dim() != 4:
        raise RuntimeError(f"per-sample update: records of Conv2d must be (N, C, H, W), got {tuple(x.shape)} and "
                           f"{tuple(g.shape)}")
    sides = factor_jobs(layer, ShapeOnly(tuple(x.shape)), ShapeOnly(tuple(g.shape)))
    if not 0 <= k < sides.groups or x.shape[1] != layer.in_channels or g.shape[1] != layer.out_channels:
        raise RuntimeError(f"per-sample update: records of {item!r} do not match the layer (input {tuple(x.shape)}, "
                           f"grad_output {tuple(g.shape)})")
    a, has_bias = sides.a, sides.a.has_bias
    c_g, m_g = layer.in_channels // sides.groups, sides.m
    N, Ng = int(x.shape[0]), int(g.shape[0])
    Ho, Wo = map(int, g.shape[2:])
    xv, gv = x[:, k * c_g:(k + 1) * c_g], g[:, k * m_g:(k + 1) * m_g]
    geo_x = _pack_source(xv.shape, x.stride(), a.kernel, a.stride, a.padding, has_bias)
    geo_g = _pack_source(gv.shape, g.stride())
    whole = in_place and (Ho * Wo) % 4 == 0
    plain = a.kernel == (1, 1) and a.stride == (1, 1) and a.padding == (0, 0) and not has_bias

    def operand(record, view, geometry, wish):
        op = _per_sample_operand(view, geometry, False, rows_outer)
        full = _pack_source(record.shape, record.stride())
        if not (wish and _is_contiguous_nchw(full)):
            return op
        plane = int(record.shape[2]) * int(record.shape[3])
        flat = record.reshape(-1)[view.storage_offset() - record.storage_offset():]           # (a view: it is contiguous)
        return PerSampleOperand(flat, op.rows, op.L, op.L, int(record.shape[1]) * plane, plane, None, False, 0)
    x_op = operand(x, xv, geo_x, whole and plain)
    g_op = operand(g, gv, geo_g, whole)
    if g_op.L != x_op.L or g_op.rows != sides.m or x_op.rows != sides.n or Ng != N:
        raise RuntimeError(f"per-sample update: records of {item!r} do not match the layer "
                           f"(input {tuple(x.shape)}, grad_output {tuple(g.shape)})")
    return PerSampleSides(g_op, x_op, sides.n, sides.m, N, x_op.L)


def _source_extent(t: torch.Tensor) -> int:
    """Elements from `t`'s first one to the end of its storage."""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


def _fill_pack(d, op: PerSampleOperand, dst: torch.Tensor) -> None:
    """The descriptor `d` of `op` into `dst`: a curv_persample_pack_ex_desc, or a curv_persample_pack3d_desc for an
    operand with a 5-D source."""
    geo = op.pack
    d.src, d.dst = op.src.data_ptr(), dst.data_ptr()
    d.rows_outer, d.Lp = int(op.rows_outer), op.Lp
    d.src_elems = _source_extent(op.src)
    d.dtype = _PACK_DTYPES[op.src.dtype]
    if len(geo.shape) == 5:
        d.N, d.C, d.D, d.H, d.W = geo.shape
        d.kd, d.kh, d.kw = geo.kernel
        d.sd, d.sh, d.sw = geo.stride
        d.pd, d.ph, d.pw = geo.padding
        d.has_bias = int(geo.has_bias)
        d.s_n, d.s_c, d.s_d, d.s_h, d.s_w = geo.strides
        return
    _set_geometry(d, geo.shape, geo.kernel, geo.stride, geo.padding, geo.has_bias)
    d.s_n, d.s_c, d.s_h, d.s_w = geo.strides
    d.transposed = int(geo.out_size is not None)
    if geo.dilation != (1, 1):                         # dh | dw << 16 in `reserved`; 0 is dilation 1
        if not all(1 <= v < 1 << 16 for v in geo.dilation):
            raise RuntimeError(f"per_sample_pack: dilation {geo.dilation} outside [1, 65535]")
        d.reserved = geo.dilation[0] | geo.dilation[1] << 16
    if geo.out_size is not None:
        d.Ho, d.Wo = geo.out_size


def per_sample_pack(operands: Sequence[PerSampleOperand], dsts: Sequence[torch.Tensor]) -> None:
    """The packed float32 copy of every operand into its `dst` (a float32 GPU buffer of `floats` values, 16-byte aligned),
    all layers in one call of curv_persample_pack_ex - and one of curv_persample_pack3d for the operands with a 5-D source
    (the records of a Conv3d), if there are any."""
    if len(dsts) != len(operands):
        raise RuntimeError(f"per_sample_pack: {len(operands)} operands, {len(dsts)} destinations")
    deep = [len(op.pack.shape) == 5 for op in operands]
    arr = (_lib.curv_persample_pack_ex_desc * deep.count(False))()
    arr3 = (_lib.curv_persample_pack3d_desc * deep.count(True))()
    flat, volume = iter(arr), iter(arr3)
    for op, dst, is_deep in zip(operands, dsts, deep):
        d = next(volume if is_deep else flat)
        _require_gpu(dst)
        if not op.src.is_cuda:
            raise RuntimeError("curvature_amd runs on MI355X only: got a CPU tensor (no CPU fallback)")
        if op.src.dtype not in _PACK_DTYPES:
            raise RuntimeError(f"per_sample_pack expects float32, bfloat16 or float16 sources, got {op.src.dtype}")
        if dst.numel() < op.floats:
            raise RuntimeError("per_sample_pack: destination too small")
        _fill_pack(d, op, dst)
    if len(arr):
        _lib.check(_lib.lib().curv_persample_pack_ex(_lib.stream_ptr(), arr, len(arr)), "curv_persample_pack_ex")
    if len(arr3):
        _lib.check(_lib.lib().curv_persample_pack3d(_lib.stream_ptr(), arr3, len(arr3)), "curv_persample_pack3d")


class _PerSampleProduct:
    """What `PerSampleJob`, `PerSampleQuadJob`, `PerSampleGridJob` and `PerSampleCovJob` share: the operands A_n (M, L) at ``A + n a_ns`` with row stride `a_rs` and
    B_n (Nc, L) likewise, for `S` samples, and `alpha` / `first`."""
    __slots__ = ("A", "B", "S", "M", "Nc", "L", "a_ns", "a_rs", "b_ns", "b_rs", "alpha", "first")

    def _set_operands(self, A, B, S, M, Nc, L, a_ns, a_rs, b_ns, b_rs, alpha, first):
        self.A, self.B = A, B
        self.S, self.M, self.Nc, self.L = int(S), int(M), int(Nc), int(L)
        self.a_ns, self.a_rs, self.b_ns, self.b_rs = int(a_ns), int(a_rs), int(b_ns), int(b_rs)
        self.alpha, self.first = float(alpha), bool(first)

    @classmethod
    def of(cls, sides: PerSampleSides, A, B, *own, alpha=1.0, first=False):
        """The job on a layer's `per_sample_operands`: A the g side, B the x side, `own` the remaining tensors of the
        constructor (C; W, out; u, v, V, out, shift, gain; W, out, K, a_cs)."""
        return cls(A, B, *own, sides.N, sides.m, sides.n, sides.L, sides.g.ns, sides.g.rs, sides.x.ns, sides.x.rs,
                   alpha=alpha, first=first)


class PerSampleJob(_PerSampleProduct):
    """C (+)= alpha * sum_n (A_n B_n^T)**2 over `S` samples: A_n is (M, L) at ``A + n a_ns`` with row stride `a_rs`, B_n
    (Nc, L) likewise, C an (M, Nc) view with unit column stride.  `first`: overwrite C.  A / B may also be `None` with
    explicit sizes (plan queries)."""
    __slots__ = ("C",)

    def __init__(self, A, B, C, S, M, Nc, L, a_ns, a_rs, b_ns, b_rs, alpha=1.0, first=False):
        self.C = C
        self._set_operands(A, B, S, M, Nc, L, a_ns, a_rs, b_ns, b_rs, alpha, first)


def _fill_per_sample_sizes(d, j: _PerSampleProduct) -> None:
    d.S, d.M, d.Nc, d.L = j.S, j.M, j.Nc, j.L
    d.a_ns, d.a_rs, d.b_ns, d.b_rs = j.a_ns, j.a_rs, j.b_ns, j.b_rs
    d.first = int(j.first)


def _fill_per_sample(d, j: _PerSampleProduct, name: str, tensors) -> None:
    """The shared fields of job `j` into descriptor `d`; with `tensors` (the job's own, behind A and B, None among them
    skipped; None: a plan query) also the device / dtype checks, the extent check of A and B under `name`, and their
    addresses."""
    _fill_per_sample_sizes(d, j)
    d.alpha = j.alpha
    if tensors is not None:
        _check_per_sample_tensors(d, j, name, tensors)


def _check_per_sample_tensors(d, j: _PerSampleProduct, name: str, tensors) -> None:
    for t in (j.A, j.B) + tuple(t for t in tensors if t is not None):
        if not t.is_cuda:
            raise RuntimeError("curvature_amd runs on MI355X only: got a CPU tensor (no CPU fallback)")
        if t.dtype != torch.float32:
            raise RuntimeError(f"curvature_amd expects float32 tensors, got {t.dtype}")
    a_need = (j.S - 1) * j.a_ns + (j.M - 1) * j.a_rs + j.L
    b_need = (j.S - 1) * j.b_ns + (j.Nc - 1) * j.b_rs + j.L
    if j.A.numel() < a_need or j.B.numel() < b_need:
        raise RuntimeError(f"{name}: an operand is smaller than its sizes and strides say")
    d.A, d.B = j.A.data_ptr(), j.B.data_ptr()


def _per_sample_descs(jobs: Sequence[PerSampleJob], check_tensors: bool = True):
    arr = (_lib.curv_persample_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        _fill_per_sample(d, j, "per_sample_sq_accumulate", (j.C,) if check_tensors else None)
        d.c_rs = j.Nc
        if check_tensors:
            if j.C.dim() != 2 or tuple(j.C.shape) != (j.M, j.Nc) or j.C.stride(1) != 1:
                raise RuntimeError(f"per_sample_sq_accumulate: destination must be an ({j.M},{j.Nc}) view with unit "
                                   f"column stride, got {tuple(j.C.shape)}")
            d.C, d.c_rs = j.C.data_ptr(), j.C.stride(0)
    return arr


def per_sample_plan_flops(jobs: Sequence[PerSampleJob]) -> List[int]:
    """Multiply-add FLOPs (2 per multiply-add) the plan executes per job (curv_persample_plan_flops, host only)."""
    if not jobs:
        return []
    return _plan_flops("curv_persample_plan_flops", _per_sample_descs(jobs, check_tensors=False), len(jobs))


def per_sample_sq_accumulate(jobs: Sequence[PerSampleJob]) -> None:
    """curv_persample_sq_accumulate over any number of products, on the current stream; slabs from `workspace`."""
    if not jobs:
        return
    _run_build("curv_persample_workspace_bytes", "curv_persample_sq_accumulate", _per_sample_descs(jobs), len(jobs),
               jobs[0].C.device, "persample")


class PerSampleQuadJob(_PerSampleProduct):
    """out[n] (+)= alpha * sum_ij W[i, j] * (A_n B_n^T)[i, j]**2 for `S` samples: A, B and their sizes and strides as in
    `PerSampleJob`; `W` an (M, Nc) view with unit column stride or None (all ones); `out` a length-S float32 view of any
    stride (a column of an (N, classes) matrix).  `first`: overwrite out.  A / B / out may also be `None` with explicit
    sizes (plan queries)."""
    __slots__ = ("W", "out")

    def __init__(self, A, B, W, out, S, M, Nc, L, a_ns, a_rs, b_ns, b_rs, alpha=1.0, first=False):
        self.W, self.out = W, out
        self._set_operands(A, B, S, M, Nc, L, a_ns, a_rs, b_ns, b_rs, alpha, first)


def _per_sample_quad_descs(jobs: Sequence[PerSampleQuadJob], check_tensors: bool = True):
    arr = (_lib.curv_persample_quad_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        _fill_per_sample(d, j, "per_sample_quad_reduce", (j.out, j.W) if check_tensors else None)
        d.w_rs, d.o_stride = j.Nc, 1
        if check_tensors:
            if j.W is not None:
                if j.W.dim() != 2 or tuple(j.W.shape) != (j.M, j.Nc) or j.W.stride(1) != 1:
                    raise RuntimeError(f"per_sample_quad_reduce: weights must be an ({j.M},{j.Nc}) view with unit column "
                                       f"stride, got {tuple(j.W.shape)}")
                d.W, d.w_rs = j.W.data_ptr(), j.W.stride(0)
            if j.out.dim() != 1 or j.out.shape[0] != j.S or (j.S > 1 and j.out.stride(0) < 1):
                raise RuntimeError(f"per_sample_quad_reduce: destination must be a length-{j.S} view with a positive "
                                   f"stride, got {tuple(j.out.shape)}")
            d.out, d.o_stride = j.out.data_ptr(), max(j.out.stride(0), 1)
    return arr


def per_sample_quad_plan_flops(jobs: Sequence[PerSampleQuadJob]) -> List[int]:
    """Multiply-add FLOPs (2 per multiply-add) the plan executes per job (curv_persample_quad_plan_flops, host only)."""
    if not jobs:
        return []
    return _plan_flops("curv_persample_quad_plan_flops", _per_sample_quad_descs(jobs, check_tensors=False), len(jobs))


def per_sample_quad_reduce(jobs: Sequence[PerSampleQuadJob]) -> None:
    """curv_persample_quad_reduce over any number of products, on the current stream; partials from `workspace`."""
    if not jobs:
        return
    _run_build("curv_persample_quad_workspace_bytes", "curv_persample_quad_reduce", _per_sample_quad_descs(jobs),
               len(jobs), jobs[0].out.device, "persample")


class PerSampleProjectJob(_PerSampleProduct):
    """Z[n, j, l] (+)= alpha * sum_i W[i, j] * (A_n B_n^T)[i, j] * U[i, l] for `S` samples (`per_sample_project`): A, B and
    their sizes and strides as in `PerSampleQuadJob`; `W` an (M, Nc) view with unit column stride (required); `U` an
    (M, R) view with unit column stride, any R; `Z` an (S, Nc, R) float32 view of any positive, non-overlapping strides
    (a permuted buffer is fine).  `first`: overwrite Z.  A / B / W / U / Z may also be `None` with explicit sizes (plan
    queries: `R` then says how many columns U has)."""
    __slots__ = ("W", "U", "Z", "R")

    def __init__(self, A, B, W, U, Z, S, M, Nc, L, a_ns, a_rs, b_ns, b_rs, alpha=1.0, first=False, R=None):
        self.W, self.U, self.Z = W, U, Z
        self.R = int(U.shape[1]) if U is not None and U.dim() == 2 else int(R or 0)
        self._set_operands(A, B, S, M, Nc, L, a_ns, a_rs, b_ns, b_rs, alpha, first)


def _per_sample_project_descs(jobs: Sequence[PerSampleProjectJob], check_tensors: bool = True):
    name = "per_sample_project"
    arr = (_lib.curv_persample_project_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        _fill_per_sample(d, j, name, (j.W, j.U, j.Z) if check_tensors else None)
        d.R = j.R
        d.w_rs, d.u_rs, d.z_ns, d.z_rs, d.z_cs = j.Nc, max(j.R, 1), j.Nc * max(j.R, 1), max(j.R, 1), 1
        if check_tensors:
            if j.W.dim() != 2 or tuple(j.W.shape) != (j.M, j.Nc) or (j.Nc > 1 and j.W.stride(1) != 1):
                raise RuntimeError(f"{name}: weights must be an ({j.M},{j.Nc}) view with unit column stride, got "
                                   f"{tuple(j.W.shape)}")
            if j.U.dim() != 2 or j.U.shape[0] != j.M or j.U.shape[1] < 1 or (j.R > 1 and j.U.stride(1) != 1) or \
                    (j.M > 1 and j.U.stride(0) < j.R):
                raise RuntimeError(f"{name}: U must be an ({j.M}, R) view with unit column stride and rows that do not "
                                   f"overlap, got {tuple(j.U.shape)} with strides {tuple(j.U.stride())}")
            if j.Z.dim() != 3 or tuple(j.Z.shape) != (j.S, j.Nc, j.R):
                raise RuntimeError(f"{name}: destination must be an ({j.S},{j.Nc},{j.R}) view, got {tuple(j.Z.shape)}")
            # (the stride of a dimension of size 1 says nothing: take 1)
            zs = [max(int(st), 1) if size == 1 else int(st) for st, size in zip(j.Z.stride(), j.Z.shape)]
            order = sorted(range(3), key=lambda k: zs[k])
            live = [k for k in order if j.Z.shape[k] > 1]
            if any(zs[k] < 1 for k in range(3)) or \
                    any(zs[hi] < zs[lo] * j.Z.shape[lo] for lo, hi in zip(live, live[1:])):
                raise RuntimeError(f"{name}: destination strides {tuple(j.Z.stride())} are not positive or overlap")
            d.W, d.w_rs = j.W.data_ptr(), max(j.W.stride(0), j.Nc)
            d.U, d.u_rs = j.U.data_ptr(), max(j.U.stride(0), j.R)
            d.Z, (d.z_ns, d.z_rs, d.z_cs) = j.Z.data_ptr(), zs
    return arr


def per_sample_project_plan_flops(jobs: Sequence[PerSampleProjectJob]) -> List[int]:
    """Multiply-add FLOPs (2 per multiply-add) the plan executes per job (curv_persample_project_plan_flops, host only):
    those of the products plus those of the second MFMA at every sample's end."""
    if not jobs:
        return []
    return _plan_flops("curv_persample_project_plan_flops", _per_sample_project_descs(jobs, check_tensors=False), len(jobs))


def per_sample_project_workspace_bytes(jobs: Sequence[PerSampleProjectJob]) -> int:
    """Bytes of scratch `per_sample_project` takes for these jobs (curv_persample_project_workspace_bytes, host only)."""
    if not jobs:
        return 0
    return int(_lib.lib().curv_persample_project_workspace_bytes(_per_sample_project_descs(jobs, check_tensors=False),
                                                                 len(jobs)))


def per_sample_project(jobs: Sequence[PerSampleProjectJob]) -> None:
    """curv_persample_project over any number of products, on the current stream; partials from `workspace`."""
    if not jobs:
        return
    _run_build("curv_persample_project_workspace_bytes", "curv_persample_project", _per_sample_project_descs(jobs),
               len(jobs), jobs[0].Z.device, "persample")


# The linearised predictive of INF is opt-in: with the switch off - the default - INF refuses the four
# methods exactly as it did, with the same messages.
_INF_PREDICTIVE = False


def admit_inf_predictive(enable: bool = True) -> bool:
    """Switch INF's linearised (GLM) predictive on or off for the process; returns what it was.  On: `INF` answers
    `functional_variance`, `stage_output` and `functional_covariance` (and with them the `evaluate.glm_predictive*`
    drivers) by `per_sample_project`; `functional_variance_grid` stays refused.  Off: the four raise NotImplementedError
    where they did."""
    global _INF_PREDICTIVE
    was, _INF_PREDICTIVE = _INF_PREDICTIVE, bool(enable)
    return was


def inf_predictive_admitted() -> bool:
    return _INF_PREDICTIVE


PERSAMPLE_GRID_MAX = _lib.PERSAMPLE_GRID_MAX


class PerSampleGridJob(_PerSampleProduct):
    """out[h, n] (+)= gain[h] * sum_ij w_h[i, j] * (A_n B_n^T)[i, j]**2 for `S` samples and the H grid points
    ``(shift[h], gain[h])`` (at most `PERSAMPLE_GRID_MAX`): A, B and their sizes and strides as in `PerSampleQuadJob`.
    The weights are separable, ``w_h[i, j] = 1 / ((u[i] + shift[h]) (v[j] + shift[h]))`` with `u` (M,) and `v` (Nc,)
    contiguous, or dense, ``w_h[i, j] = 1 / (V[i, j] + shift[h])`` with `V` an (M, Nc) view with unit column stride: give
    `u` and `v`, or `V`, and None for the other.  `shift` (finite, > 0) and `gain` (finite) are sequences of H Python
    floats; they travel with the kernel arguments.  `out` an (H, S) float32 view with positive strides.  `first`:
    overwrite out.  There is no `alpha`.  A / B / out and the weights may also be `None` with explicit sizes (plan
    queries)."""
    __slots__ = ("u", "v", "V", "out", "shift", "gain")

    def __init__(self, A, B, u, v, V, out, shift, gain, S, M, Nc, L, a_ns, a_rs, b_ns, b_rs, alpha=1.0, first=False):
        self.u, self.v, self.V, self.out = u, v, V, out
        self.shift, self.gain = [float(x) for x in shift], [float(x) for x in gain]
        if float(alpha) != 1.0:
            raise ValueError("PerSampleGridJob has no alpha: the scale of grid point h is gain[h]")
        self._set_operands(A, B, S, M, Nc, L, a_ns, a_rs, b_ns, b_rs, 1.0, first)


def _per_sample_grid_descs(jobs: Sequence[PerSampleGridJob], check_tensors: bool = True):
    name = "per_sample_quad_grid_reduce"
    arr = (_lib.curv_persample_grid_desc * len(jobs))()
    keep = []                                        # the host tables the descriptors point to
    for d, j in zip(arr, jobs):
        H = len(j.shift)
        if not 1 <= H <= PERSAMPLE_GRID_MAX or len(j.gain) != H:
            raise ValueError(f"{name}: {H} shifts and {len(j.gain)} gains; a job takes 1 to {PERSAMPLE_GRID_MAX} grid "
                             "points, as many gains as shifts")
        for h, (s, g) in enumerate(zip(j.shift, j.gain)):
            if not (s > 0 and math.isfinite(s) and math.isfinite(g)):
                raise ValueError(f"{name}: grid point {h}: shift {s} must be finite and > 0, gain {g} finite")
        _fill_per_sample_sizes(d, j)
        d.H = H
        tables = ((ctypes.c_float * H)(*j.shift), (ctypes.c_float * H)(*j.gain))
        keep.append(tables)
        d.shift, d.gain = ctypes.cast(tables[0], ctypes.POINTER(ctypes.c_float)), ctypes.cast(tables[1], ctypes.POINTER(ctypes.c_float))
        d.v_rs, d.o_stride, d.o_hs = j.Nc, 1, j.S
        if not check_tensors:
            continue
        separable = j.V is None
        if (j.u is None) != (j.v is None) or separable == (j.u is None):
            raise RuntimeError(f"{name}: give the weights as u and v (separable) or as V (dense), not both")
        _check_per_sample_tensors(d, j, name, (j.out, j.u, j.v, j.V))
        if separable:
            for what, t, rows in (("u", j.u, j.M), ("v", j.v, j.Nc)):
                if t.dim() != 1 or t.shape[0] != rows or not t.is_contiguous():
                    raise RuntimeError(f"{name}: {what} must be a contiguous vector of {rows} values, got {tuple(t.shape)}")
            d.u, d.v = j.u.data_ptr(), j.v.data_ptr()
        else:
            if j.V.dim() != 2 or tuple(j.V.shape) != (j.M, j.Nc) or j.V.stride(1) != 1:
                raise RuntimeError(f"{name}: V must be an ({j.M},{j.Nc}) view with unit column stride, got "
                                   f"{tuple(j.V.shape)}")
            d.V, d.v_rs = j.V.data_ptr(), j.V.stride(0)
        if j.out.dim() != 2 or tuple(j.out.shape) != (H, j.S) or (j.S > 1 and j.out.stride(1) < 1) or \
                (H > 1 and j.out.stride(0) < 1):
            raise RuntimeError(f"{name}: destination must be an ({H},{j.S}) view with positive strides, got "
                               f"{tuple(j.out.shape)}")
        d.out, d.o_stride, d.o_hs = j.out.data_ptr(), max(j.out.stride(1), 1), max(j.out.stride(0), 1)
    arr._tables = keep
    return arr


def per_sample_quad_grid_plan_flops(jobs: Sequence[PerSampleGridJob]) -> List[int]:
    """Multiply-add FLOPs (2 per multiply-add) of the MFMA products the plan executes per job
    (curv_persample_quad_grid_plan_flops, host only): those of `per_sample_quad_plan_flops`, whatever H."""
    if not jobs:
        return []
    return _plan_flops("curv_persample_quad_grid_plan_flops", _per_sample_grid_descs(jobs, check_tensors=False), len(jobs))


def per_sample_quad_grid_reduce(jobs: Sequence[PerSampleGridJob]) -> None:
    """curv_persample_quad_grid_reduce over any number of products, on the current stream; partials from `workspace`."""
    if not jobs:
        return
    _run_build("curv_persample_quad_grid_workspace_bytes", "curv_persample_quad_grid_reduce", _per_sample_grid_descs(jobs),
               len(jobs), jobs[0].out.device, "persample")


PERSAMPLE_COV_MAX_OUTPUTS = _lib.PERSAMPLE_COV_MAX_OUTPUTS


class PerSampleCovJob(_PerSampleProduct):
    """out[n, c, c'] (+)= alpha * sum_ij W[i, j] * (A_{c,n} B_n^T)[i, j] * (A_{c',n} B_n^T)[i, j] for `S` samples and `K`
    outputs (at most `PERSAMPLE_COV_MAX_OUTPUTS`): output c of A at ``A + c a_cs``, otherwise A, B, W and their sizes
    and strides as in `PerSampleQuadJob`; `out` an (S, K, K) float32 view with unit last stride (any other strides the
    library allows).  `first`: overwrite out.  A / B / out may also be `None` with explicit sizes (plan queries)."""
    __slots__ = ("W", "out", "K", "a_cs")

    def __init__(self, A, B, W, out, K, a_cs, S, M, Nc, L, a_ns, a_rs, b_ns, b_rs, alpha=1.0, first=False):
        self.W, self.out, self.K, self.a_cs = W, out, int(K), int(a_cs)
        self._set_operands(A, B, S, M, Nc, L, a_ns, a_rs, b_ns, b_rs, alpha, first)


def _per_sample_cov_descs(jobs: Sequence[PerSampleCovJob], check_tensors: bool = True):
    arr = (_lib.curv_persample_cov_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        _fill_per_sample(d, j, "per_sample_cov_reduce", (j.out, j.W) if check_tensors else None)
        d.K, d.a_cs = j.K, j.a_cs
        d.w_rs, d.o_rs, d.o_ns = j.Nc, j.K, j.K * j.K
        if check_tensors:
            if j.A.numel() < (j.K - 1) * j.a_cs + (j.S - 1) * j.a_ns + (j.M - 1) * j.a_rs + j.L:
                raise RuntimeError("per_sample_cov_reduce: an operand is smaller than its sizes and strides say")
            if j.W is not None:
                if j.W.dim() != 2 or tuple(j.W.shape) != (j.M, j.Nc) or j.W.stride(1) != 1:
                    raise RuntimeError(f"per_sample_cov_reduce: weights must be an ({j.M},{j.Nc}) view with unit column "
                                       f"stride, got {tuple(j.W.shape)}")
                d.W, d.w_rs = j.W.data_ptr(), j.W.stride(0)
            if j.out.dim() != 3 or tuple(j.out.shape) != (j.S, j.K, j.K) or (j.K > 1 and j.out.stride(2) != 1):
                raise RuntimeError(f"per_sample_cov_reduce: destination must be an ({j.S},{j.K},{j.K}) view with unit "
                                   f"last stride, got {tuple(j.out.shape)}")
            # (the stride of a dimension of size 1 says nothing: take the smallest the library allows)
            d.o_rs = j.out.stride(1) if j.K > 1 else j.K
            d.o_ns = j.out.stride(0) if j.S > 1 else j.K * d.o_rs
            d.out = j.out.data_ptr()
    return arr


def per_sample_cov_plan_flops(jobs: Sequence[PerSampleCovJob]) -> List[int]:
    """Multiply-add FLOPs (2 per multiply-add) the plan executes per job (curv_persample_cov_plan_flops, host only)."""
    if not jobs:
        return []
    return _plan_flops("curv_persample_cov_plan_flops", _per_sample_cov_descs(jobs, check_tensors=False), len(jobs))


def per_sample_cov_reduce(jobs: Sequence[PerSampleCovJob]) -> None:
    """curv_persample_cov_reduce over any number of products, on the current stream; partials from `workspace`."""
    if not jobs:
        return
    _run_build("curv_persample_cov_workspace_bytes", "curv_persample_cov_reduce", _per_sample_cov_descs(jobs),
               len(jobs), jobs[0].out.device, "persample")


class LogitMCJob:
    """probs[n, c] = mean over `S` draws of softmax([f, rest[n]])[c] with f = mu[n] + L_n z, L_n L_n^T = cov[n]
    (curv_logit_mc): `cov` an (N, K, K) float32 view with unit last stride (what `per_sample_cov_reduce` writes; only the
    lower triangles are read), `mu` an (N, K) view with unit last stride, `rest` (N,) - the log-sum-exp of the logits that
    are not selected - or None, `noise` an (N, S, K) view of explicit z with unit last stride or None (then the library's
    Philox stream at `seed`, `offset`; the call consumes ``N * S * ceil(K / 4)`` counters).  Outputs, contiguous, any of
    them None but not all: `probs` (N, K), `probs_rest` (N,), `draws` (N, S, K), `info` (N,) int32 - the number of dropped
    Cholesky columns, or -(j + 1) for a negative pivot j.  Every tensor may also be None with explicit `N`, `K` (plan
    queries)."""
    __slots__ = ("cov", "mu", "rest", "noise", "probs", "probs_rest", "draws", "info", "N", "K", "S", "seed", "offset")

    def __init__(self, cov, mu, S, rest=None, noise=None, probs=None, probs_rest=None, draws=None, info=None,
                 seed: int = 0, offset: int = 0, N: Optional[int] = None, K: Optional[int] = None):
        self.cov, self.mu, self.rest, self.noise = cov, mu, rest, noise
        self.probs, self.probs_rest, self.draws, self.info = probs, probs_rest, draws, info
        self.N = int(cov.shape[0] if N is None else N)
        self.K = int(cov.shape[-1] if K is None else K)
        self.S, self.seed, self.offset = int(S), int(seed), int(offset)


def _logit_mc_descs(jobs: Sequence[LogitMCJob], check_tensors: bool = True):
    name = "logit_mc"
    arr = (_lib.curv_logit_mc_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        N, K, S = j.N, j.K, j.S
        d.N, d.K, d.S = N, K, S
        d.o_rs, d.o_ns, d.mu_ns = K, K * K, K
        d.seed, d.offset = j.seed & (2 ** 64 - 1), j.offset & (2 ** 64 - 1)
        if not check_tensors:
            d.probs = 256                # (an item without outputs is refused; the host queries never read the address)
            continue
        floats = (j.cov, j.mu, j.rest, j.noise, j.probs, j.probs_rest, j.draws)
        for t in floats + (j.info,):
            if t is not None and not t.is_cuda:
                raise RuntimeError("curvature_amd runs on MI355X only: got a CPU tensor (no CPU fallback)")
        for t in floats:
            if t is not None and t.dtype != torch.float32:
                raise RuntimeError(f"curvature_amd expects float32 tensors, got {t.dtype}")
        if j.cov.dim() != 3 or tuple(j.cov.shape) != (N, K, K) or (K > 1 and j.cov.stride(2) != 1):
            raise RuntimeError(f"{name}: cov must be an ({N},{K},{K}) view with unit last stride, got {tuple(j.cov.shape)}")
        if j.mu.dim() != 2 or tuple(j.mu.shape) != (N, K) or (K > 1 and j.mu.stride(1) != 1):
            raise RuntimeError(f"{name}: mu must be an ({N},{K}) view with unit last stride, got {tuple(j.mu.shape)}")
        # (the stride of a dimension of size 1 says nothing: take the smallest the library allows)
        d.o_rs = j.cov.stride(1) if K > 1 else K
        d.o_ns = j.cov.stride(0) if N > 1 else K * d.o_rs
        d.mu_ns = j.mu.stride(0) if N > 1 else K
        d.cov, d.mu = j.cov.data_ptr(), j.mu.data_ptr()
        if j.noise is not None:
            if j.noise.dim() != 3 or tuple(j.noise.shape) != (N, S, K) or (K > 1 and j.noise.stride(2) != 1):
                raise RuntimeError(f"{name}: noise must be an ({N},{S},{K}) view with unit last stride, got "
                                   f"{tuple(j.noise.shape)}")
            d.z_ss = j.noise.stride(1) if S > 1 else K
            d.z_ns = j.noise.stride(0) if N > 1 else (S - 1) * d.z_ss + K
            d.Z = j.noise.data_ptr()
        for what, t, shape in (("rest", j.rest, (N,)), ("probs", j.probs, (N, K)), ("probs_rest", j.probs_rest, (N,)),
                               ("draws", j.draws, (N, S, K)), ("info", j.info, (N,))):
            if t is None:
                continue
            if tuple(t.shape) != shape or not t.is_contiguous() or (what == "info" and t.dtype != torch.int32):
                raise RuntimeError(f"{name}: {what} must be a contiguous {shape} tensor"
                                   f"{' of int32' if what == 'info' else ''}, got {tuple(t.shape)} {t.dtype}")
            setattr(d, what, t.data_ptr())
    return arr


def logit_mc_plan_flops(jobs: Sequence[LogitMCJob]) -> List[int]:
    """Multiply-add FLOPs (2 per multiply-add) of the draws the plan executes per job (curv_logit_mc_plan_flops, host
    only)."""
    if not jobs:
        return []
    return _plan_flops("curv_logit_mc_plan_flops", _logit_mc_descs(jobs, check_tensors=False), len(jobs))


def logit_mc(jobs: Sequence[LogitMCJob]) -> None:
    """curv_logit_mc over any number of items, on the current stream; the partial sums of items whose draws are cut into
    chunks from `workspace` (an item of one chunk per input needs none)."""
    if not jobs:
        return
    L, arr, n = _lib.lib(), _logit_mc_descs(jobs), len(jobs)
    need = L.curv_logit_mc_workspace_bytes(arr, n)       # 0: nothing needed - or refused, which the call itself reports
    ws = workspace(need, jobs[0].cov.device, "persample") if need else None
    _lib.check(L.curv_logit_mc(_lib.stream_ptr(), arr, n, ws.data_ptr() if need else None, ws.numel() if need else 0),
               "curv_logit_mc")


HEAD_MC_MAX_CLASSES = _lib.HEAD_MC_MAX_CLASSES


class HeadMCJob:
    """probs[n, c] = mean over `samples` draws of softmax(f)[c] with f = mu[n] + M (sqrt(max(d2[n], 0)) * z)
    (curv_head_mc): `M` a (K, K) float32 view with unit column stride (with `lower` only its lower triangle is read) or
    None (identity: no product), `d2` an (N,) or (N, K) view with unit last stride, `mu` an (N, K) view with unit last
    stride, K at most `HEAD_MC_MAX_CLASSES`; `noise` an (N, S, K) view of explicit z with unit last stride or None (then the
    library's Philox stream at `seed`, `offset`; the call consumes ``N * S * ceil(K / 4)`` counters).  Outputs, contiguous,
    one of them may be None: `probs` (N, K), `draws` (N, S, K).  `d2` and `mu` may also be None with explicit `N`, `K`
    (plan queries, which only ask whether `M` is None)."""
    __slots__ = ("M", "d2", "mu", "noise", "probs", "draws", "lower", "N", "K", "S", "seed", "offset")

    def __init__(self, M, d2, mu, samples, *, lower=False, noise=None, probs=None, draws=None, seed: int = 0,
                 offset: int = 0, N: Optional[int] = None, K: Optional[int] = None):
        self.M, self.d2, self.mu, self.noise, self.probs, self.draws = M, d2, mu, noise, probs, draws
        self.lower = bool(lower)
        self.N = int(mu.shape[0] if N is None else N)
        self.K = int(mu.shape[-1] if K is None else K)
        self.S, self.seed, self.offset = int(samples), int(seed), int(offset)


def _head_mc_descs(jobs: Sequence[HeadMCJob], check_tensors: bool = True, name: str = "head_mc",
                   desc=_lib.curv_head_mc_desc, outputs=(("probs", "N,K"), ("draws", "N,S,K"))):
    """The descriptors of `head_mc` and, with the other `name`, `desc` and `outputs` (attribute, shape), of
    `head_mc_moments`."""
    arr = (desc * len(jobs))()
    for d, j in zip(arr, jobs):
        N, K, S = j.N, j.K, j.S
        d.N, d.K, d.S, d.m_lower = N, K, S, int(j.lower)
        d.m_rs, d.mu_ns, d.d_cs, d.d_ns = K, K, 1, K
        d.seed, d.offset = j.seed & (2 ** 64 - 1), j.offset & (2 ** 64 - 1)
        if not check_tensors:
            d.probs = 256                # (an item without outputs is refused; the host queries never read the address)
            d.M = 256 if j.M is not None else None
            continue
        shapes = {"N,K": (N, K), "N,S,K": (N, S, K), "N": (N,)}
        floats = (j.M, j.d2, j.mu, j.noise) + tuple(getattr(j, what) for what, _ in outputs)
        for t in floats:
            if t is not None and not t.is_cuda:
                raise RuntimeError("curvature_amd runs on MI355X only: got a CPU tensor (no CPU fallback)")
        for t in floats:
            if t is not None and t.dtype != torch.float32:
                raise RuntimeError(f"curvature_amd expects float32 tensors, got {t.dtype}")
        if j.mu.dim() != 2 or tuple(j.mu.shape) != (N, K) or (K > 1 and j.mu.stride(1) != 1):
            raise RuntimeError(f"{name}: mu must be an ({N},{K}) view with unit last stride, got {tuple(j.mu.shape)}")
        # (the stride of a dimension of size 1 says nothing: take the smallest the library allows)
        d.mu_ns = j.mu.stride(0) if N > 1 else K
        d.mu = j.mu.data_ptr()
        if j.M is not None:
            if j.M.dim() != 2 or tuple(j.M.shape) != (K, K) or (K > 1 and j.M.stride(1) != 1):
                raise RuntimeError(f"{name}: M must be a ({K},{K}) view with unit column stride, got {tuple(j.M.shape)}")
            d.m_rs = j.M.stride(0) if K > 1 else K
            d.M = j.M.data_ptr()
        if j.d2.dim() == 1 and tuple(j.d2.shape) == (N,):
            d.d_cs, d.d_ns = 0, (j.d2.stride(0) if N > 1 else 1)
        elif j.d2.dim() == 2 and tuple(j.d2.shape) == (N, K) and (K == 1 or j.d2.stride(1) == 1):
            d.d_cs, d.d_ns = 1, (j.d2.stride(0) if N > 1 else K)
        else:
            raise RuntimeError(f"{name}: d2 must be an ({N},) or ({N},{K}) view with unit last stride, got "
                               f"{tuple(j.d2.shape)}")
        d.d2 = j.d2.data_ptr()
        if j.noise is not None:
            if j.noise.dim() != 3 or tuple(j.noise.shape) != (N, S, K) or (K > 1 and j.noise.stride(2) != 1):
                raise RuntimeError(f"{name}: noise must be an ({N},{S},{K}) view with unit last stride, got "
                                   f"{tuple(j.noise.shape)}")
            d.z_ss = j.noise.stride(1) if S > 1 else K
            d.z_ns = j.noise.stride(0) if N > 1 else (S - 1) * d.z_ss + K
            d.Z = j.noise.data_ptr()
        for what, key in outputs:
            t, shape = getattr(j, what), shapes[key]
            if t is None:
                continue
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise RuntimeError(f"{name}: {what} must be a contiguous {shape} tensor, got {tuple(t.shape)} {t.dtype}")
            setattr(d, what, t.data_ptr())
    return arr


def head_mc_plan_flops(jobs: Sequence[HeadMCJob]) -> List[int]:
    """Multiply-add FLOPs (2 per multiply-add) of the MFMA products the plan executes per job (curv_head_mc_plan_flops,
    host only): 0 for a job without `M`."""
    if not jobs:
        return []
    return _plan_flops("curv_head_mc_plan_flops", _head_mc_descs(jobs, check_tensors=False), len(jobs))


def head_mc(jobs: Sequence[HeadMCJob]) -> None:
    """curv_head_mc over any number of items, on the current stream; the partial sums of items whose draws are cut into
    chunks from `workspace` (an item of one chunk per input needs none)."""
    if not jobs:
        return
    L, arr, n = _lib.lib(), _head_mc_descs(jobs), len(jobs)
    need = L.curv_head_mc_workspace_bytes(arr, n)        # 0: nothing needed - or refused, which the call itself reports
    ws = workspace(need, jobs[0].mu.device, "persample") if need else None
    _lib.check(L.curv_head_mc(_lib.stream_ptr(), arr, n, ws.data_ptr() if need else None, ws.numel() if need else 0),
               "curv_head_mc")


class HeadMomentsJob(HeadMCJob):
    """`HeadMCJob` with two more moments of the same draws (curv_head_mc_moments): `entropy` (N,), the mean over the draws
    of the entropy of softmax(f) - the aleatoric part of the uncertainty -, and `probs_sq` (N, K), the mean of
    softmax(f)[c] ** 2, beside `probs` (N, K; the bits `head_mc` gives for the same inputs) and `draws` (N, S, K).  All
    four contiguous float32, any may be None but not all."""
    __slots__ = ("entropy", "probs_sq")

    def __init__(self, M, d2, mu, samples, *, lower=False, noise=None, probs=None, entropy=None, probs_sq=None, draws=None,
                 seed: int = 0, offset: int = 0, N: Optional[int] = None, K: Optional[int] = None):
        super().__init__(M, d2, mu, samples, lower=lower, noise=noise, probs=probs, draws=draws, seed=seed, offset=offset,
                         N=N, K=K)
        self.entropy, self.probs_sq = entropy, probs_sq


def _head_moments_descs(jobs: Sequence[HeadMomentsJob], check_tensors: bool = True):
    return _head_mc_descs(jobs, check_tensors, "head_mc_moments", _lib.curv_head_moments_desc,
                          (("probs", "N,K"), ("draws", "N,S,K"), ("entropy", "N"), ("probs_sq", "N,K")))


def head_mc_moments_plan_flops(jobs: Sequence[HeadMomentsJob]) -> List[int]:
    """`head_mc_plan_flops` of the same jobs (curv_head_mc_moments_plan_flops, host only): the moments add no product."""
    if not jobs:
        return []
    return _plan_flops("curv_head_mc_moments_plan_flops", _head_moments_descs(jobs, check_tensors=False), len(jobs))


def head_mc_moments(jobs: Sequence[HeadMomentsJob]) -> None:
    """curv_head_mc_moments over any number of items, on the current stream; the partial sums of items whose draws are
    cut into chunks from `workspace` (an item of one chunk per input needs none)."""
    if not jobs:
        return
    L, arr, n = _lib.lib(), _head_moments_descs(jobs), len(jobs)
    need = L.curv_head_mc_moments_workspace_bytes(arr, n)    # 0: nothing needed - or refused, which the call itself reports
    ws = workspace(need, jobs[0].mu.device, "persample") if need else None
    _lib.check(L.curv_head_mc_moments(_lib.stream_ptr(), arr, n, ws.data_ptr() if need else None,
                                      ws.numel() if need else 0), "curv_head_mc_moments")


HEAD_GRID_MAX = _lib.HEAD_GRID_MAX


class HeadGridJob:
    """out[h, r, j] = gain[h] * r_h[j] * sum_i Y[r, i]**2 / (T[j, i] + shift[h]) for the H pairs ``(shift[h], gain[h])``
    (at most `HEAD_GRID_MAX`; curv_head_grid): the `d2` of `HeadMCJob` for a whole grid of damping pairs.  `Y` an (N, n)
    float32 view with unit last stride.  The spectrum is dense - `T` a (K, n) view with unit column stride, r_h = 1 - or
    separable - `u` (K,) and `v` (n,) contiguous, ``T[j, i] = v[i]`` and ``r_h[j] = 1 / (u[j] + shift[h])``: give `u` and
    `v`, or `T`, and None for the other.  `shift` (finite, > 0) and `gain` (finite) are sequences of H Python floats; they
    travel with the kernel arguments.  `out` a contiguous (H, N, K) float32 tensor, overwritten.  `Y` and `out` may also be
    None with explicit `N`, `K`, `n`, and then the spectrum too with `separable` saying which form is meant (plan queries,
    which read no tensor)."""
    __slots__ = ("Y", "u", "v", "T", "out", "shift", "gain", "N", "K", "n", "separable")

    def __init__(self, Y, u, v, T, out, shift, gain, *, N: Optional[int] = None, K: Optional[int] = None,
                 n: Optional[int] = None, separable: Optional[bool] = None):
        self.Y, self.u, self.v, self.T, self.out = Y, u, v, T, out
        self.separable = None if separable is None else bool(separable)
        self.shift, self.gain = [float(x) for x in shift], [float(x) for x in gain]
        self.N = int(Y.shape[0] if N is None else N)
        self.n = int(Y.shape[-1] if n is None else n)
        spectrum = T if T is not None else u                 # (neither: refused with the item named when the job is used)
        self.K = int((spectrum.shape[0] if spectrum is not None else out.shape[-1]) if K is None else K)


def _head_grid_descs(jobs: Sequence[HeadGridJob], check_tensors: bool = True):
    name = "head_grid"
    arr = (_lib.curv_head_grid_desc * len(jobs))()
    keep = []                                        # the host tables the descriptors point to
    forms = []
    for k, j in enumerate(jobs):                     # the pairs and the form of every job, before any tensor is looked at
        H = len(j.shift)
        if not 1 <= H <= HEAD_GRID_MAX or len(j.gain) != H:
            raise ValueError(f"{name}: item {k}: {H} shifts and {len(j.gain)} gains; a job takes 1 to {HEAD_GRID_MAX} "
                             "pairs, as many gains as shifts")
        for h, (s, g) in enumerate(zip(j.shift, j.gain)):
            if not (s > 0 and math.isfinite(s) and math.isfinite(g)):
                raise ValueError(f"{name}: item {k}: pair {h}: shift {s} must be finite and > 0, gain {g} finite")
        separable = j.separable if not check_tensors else None
        if separable is None:
            if (j.u is None) != (j.v is None) or (j.T is None) == (j.u is None):
                raise RuntimeError(f"{name}: item {k}: give the spectrum as u and v (separable) or as T (dense), not both")
            separable = j.T is None
        forms.append(separable)
    for k, (d, j, separable) in enumerate(zip(arr, jobs, forms)):
        H, N, K, n = len(j.shift), j.N, j.K, j.n
        d.N, d.K, d.n, d.H = N, K, n, H
        d.y_rs, d.t_rs = n, n
        tables = ((ctypes.c_float * H)(*j.shift), (ctypes.c_float * H)(*j.gain))
        keep.append(tables)
        d.shift, d.gain = ctypes.cast(tables[0], ctypes.POINTER(ctypes.c_float)), ctypes.cast(tables[1], ctypes.POINTER(ctypes.c_float))
        if not check_tensors:
            if separable:                         # (the host queries ask which pointers are null and read none)
                d.u = d.v = 256
            else:
                d.T = 256
            continue
        floats = (j.Y, j.u, j.v, j.T, j.out)
        for t in floats:
            if t is not None and not t.is_cuda:
                raise RuntimeError("curvature_amd runs on MI355X only: got a CPU tensor (no CPU fallback)")
        for t in floats:
            if t is not None and t.dtype != torch.float32:
                raise RuntimeError(f"curvature_amd expects float32 tensors, got {t.dtype}")
        if j.Y.dim() != 2 or tuple(j.Y.shape) != (N, n) or (n > 1 and j.Y.stride(1) != 1):
            raise RuntimeError(f"{name}: item {k}: Y must be an ({N},{n}) view with unit last stride, got "
                               f"{tuple(j.Y.shape)}")
        # (the stride of a dimension of size 1 says nothing: take the smallest the library allows)
        d.y_rs = j.Y.stride(0) if N > 1 else n
        d.Y = j.Y.data_ptr()
        if separable:
            for what, t, rows in (("u", j.u, K), ("v", j.v, n)):
                if t.dim() != 1 or t.shape[0] != rows or not t.is_contiguous():
                    raise RuntimeError(f"{name}: item {k}: {what} must be a contiguous vector of {rows} values, got "
                                       f"{tuple(t.shape)}")
            d.u, d.v = j.u.data_ptr(), j.v.data_ptr()
        else:
            if j.T.dim() != 2 or tuple(j.T.shape) != (K, n) or (n > 1 and j.T.stride(1) != 1):
                raise RuntimeError(f"{name}: item {k}: T must be a ({K},{n}) view with unit column stride, got "
                                   f"{tuple(j.T.shape)}")
            d.t_rs = j.T.stride(0) if K > 1 else n
            d.T = j.T.data_ptr()
        if tuple(j.out.shape) != (H, N, K) or not j.out.is_contiguous():
            raise RuntimeError(f"{name}: item {k}: out must be a contiguous ({H},{N},{K}) tensor, got {tuple(j.out.shape)}")
        d.out = j.out.data_ptr()
    arr._tables = keep
    return arr


def head_grid_plan_flops(jobs: Sequence[HeadGridJob]) -> List[int]:
    """Multiply-add FLOPs (2 per multiply-add) of the MFMA products the plan executes per job FOR ONE PAIR
    (curv_head_grid_plan_flops, host only): whatever H; a call runs them once per pair.  0 for a separable job."""
    if not jobs:
        return []
    return _plan_flops("curv_head_grid_plan_flops", _head_grid_descs(jobs, check_tensors=False), len(jobs))


def head_grid(jobs: Sequence[HeadGridJob]) -> None:
    """curv_head_grid over any number of items, on the current stream; the partial sums of dense items whose sum over i
    is cut into chunks from `workspace` (an item of one chunk, and a separable one, needs none)."""
    if not jobs:
        return
    L, arr, n = _lib.lib(), _head_grid_descs(jobs), len(jobs)
    need = L.curv_head_grid_workspace_bytes(arr, n)      # 0: nothing needed - or refused, which the call itself reports
    ws = workspace(need, jobs[0].out.device, "persample") if need else None
    _lib.check(L.curv_head_grid(_lib.stream_ptr(), arr, n, ws.data_ptr() if need else None, ws.numel() if need else 0),
               "curv_head_grid")


class PerSampleDwJob:
    """The per-sample products of a true depthwise convolution (csrc/persample_dw.hip): `x` the (N, C, H, W) input and `g`
    the (N, C, Ho, Wo) grad_output, float32 GPU tensors of any strides (not negative), with the layer's `kernel`, `stride`,
    `padding` and `has_bias`; n_g = kh kw + has_bias.  For `per_sample_dw_sq_accumulate`: `dst` a (C, n_g) view with unit
    column stride.  For `per_sample_dw_quad_reduce`: `out` a length-N view of positive stride, `T` (C, n_g, n_g) with unit
    last stride, `W` (C, n_g) with unit column stride and `s` C values (any shape, contiguous), each or all None (identity,
    ones, ones).  `alpha`, `first` as in `PerSampleJob`.  `x` / `g` may also be shapes (plan queries)."""
    __slots__ = ("x", "g", "kernel", "stride", "padding", "has_bias", "dst", "out", "T", "W", "s", "alpha", "first")

    def __init__(self, x, g, kernel, stride=(1, 1), padding=(0, 0), has_bias=False, dst=None, out=None, T=None, W=None,
                 s=None, alpha=1.0, first=False):
        self.x, self.g = x, g
        self.kernel, self.stride, self.padding = tuple(map(int, kernel)), tuple(map(int, stride)), tuple(map(int, padding))
        self.has_bias, self.dst, self.out, self.T, self.W, self.s = bool(has_bias), dst, out, T, W, s
        self.alpha, self.first = float(alpha), bool(first)

    @classmethod
    def of(cls, layer, x, g, **own):
        """The job of a depthwise Conv2d `layer` on its records."""
        return cls(x.detach(), g.detach(), layer.kernel_size, layer.stride, layer.padding, layer.bias is not None, **own)


def _fill_dw_record(d, j, name: str):
    """The record, geometry and extent fields every curv_persample_dw_*_desc has, from job `j` (`x` / `g` tensors or, for a
    plan query, shapes); returns the two shapes."""
    xs, gs = (tuple(t.shape) if isinstance(t, torch.Tensor) else tuple(t) for t in (j.x, j.g))
    if len(xs) != 4 or len(gs) != 4 or xs[:2] != gs[:2]:
        raise RuntimeError(f"{name}: records must be (N, C, H, W) and (N, C, Ho, Wo), got {xs} and {gs}")
    _set_geometry(d, xs, j.kernel, j.stride, j.padding, j.has_bias)
    d.Ho, d.Wo = gs[2:]
    for side, t, shape in (("x", j.x, xs), ("g", j.g, gs)):
        if isinstance(t, torch.Tensor):
            strides, elems = t.stride(), _source_extent(t)
        else:
            strides, elems = (math.prod(shape[1:]), shape[2] * shape[3], shape[3], 1), math.prod(shape)
        for k, v in zip(("sn", "sc", "sh", "sw"), strides):
            setattr(d, f"{side}_{k}", int(v))
        setattr(d, f"{side}_elems", int(elems))
    return xs, gs


def _fill_dw_pointers(d, j, own) -> None:
    """The device / dtype checks of the records and of the job's `own` tensors (None among them skipped), and the records'
    addresses."""
    for t in (j.x, j.g) + tuple(t for t in own if t is not None):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("curvature_amd runs on MI355X only: got a CPU tensor (no CPU fallback)")
        if t.dtype != torch.float32:
            raise RuntimeError(f"curvature_amd expects float32 tensors, got {t.dtype}")
    d.x, d.g = j.x.data_ptr(), j.g.data_ptr()


def _dw_transform(d, j, name: str, C: int, n_g: int) -> None:
    """`T` (C, n_g, n_g) of job `j` into descriptor `d`, if it has one."""
    if j.T is not None:
        if tuple(j.T.shape) != (C, n_g, n_g) or (n_g > 1 and j.T.stride(2) != 1):
            raise RuntimeError(f"{name}: T must be a ({C},{n_g},{n_g}) view with unit last stride, got {tuple(j.T.shape)}")
        d.T, d.t_cs, d.t_rs = j.T.data_ptr(), j.T.stride(0) if C > 1 else n_g * n_g, j.T.stride(1) if n_g > 1 else n_g


def _per_sample_dw_descs(jobs: Sequence[PerSampleDwJob], name: str, reduction: Optional[str]):
    """`reduction`: "sq", "quad" or None (a plan query: geometry only, `x` / `g` may be shapes)."""
    arr = (_lib.curv_persample_dw_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        xs, gs = _fill_dw_record(d, j, name)
        d.first, d.alpha = int(j.first), j.alpha
        if reduction is None:
            continue
        C, n_g = xs[1], j.kernel[0] * j.kernel[1] + int(j.has_bias)
        _fill_dw_pointers(d, j, (j.dst,) if reduction == "sq" else (j.out, j.T, j.W, j.s))
        if reduction == "sq":
            if j.dst is None or j.dst.dim() != 2 or tuple(j.dst.shape) != (C, n_g) or j.dst.stride(1) != 1:
                raise RuntimeError(f"{name}: destination must be a ({C},{n_g}) view with unit column stride, got "
                                   f"{None if j.dst is None else tuple(j.dst.shape)}")
            d.dst, d.c_rs = j.dst.data_ptr(), j.dst.stride(0) if C > 1 else n_g
            continue
        if j.out is None or j.out.dim() != 1 or j.out.shape[0] != xs[0] or (xs[0] > 1 and j.out.stride(0) < 1):
            raise RuntimeError(f"{name}: destination must be a length-{xs[0]} view with a positive stride, got "
                               f"{None if j.out is None else tuple(j.out.shape)}")
        d.out, d.o_stride = j.out.data_ptr(), max(j.out.stride(0), 1)
        _dw_transform(d, j, name, C, n_g)
        if j.W is not None:
            if tuple(j.W.shape) != (C, n_g) or (n_g > 1 and j.W.stride(1) != 1):
                raise RuntimeError(f"{name}: W must be a ({C},{n_g}) view with unit column stride, got {tuple(j.W.shape)}")
            d.Wt, d.w_rs = j.W.data_ptr(), j.W.stride(0) if C > 1 else n_g
        if j.s is not None:
            if j.s.numel() != C or not j.s.is_contiguous():
                raise RuntimeError(f"{name}: s must hold {C} contiguous values, got {tuple(j.s.shape)}")
            d.s = j.s.data_ptr()
    return arr


def per_sample_dw_plan_info(jobs: Sequence[PerSampleDwJob]):
    """(flops, bytes) per job (curv_persample_dw_plan_info, host only): the FLOPs of the plane products, 2 N C Ho Wo n_g,
    and the bytes the algorithm needs, 4 N C (H W + Ho Wo).  `x` / `g` of a job may be shapes."""
    if not jobs:
        return [], []
    n = len(jobs)
    arr = _per_sample_dw_descs(jobs, "per_sample_dw_plan_info", None)
    flops, nbytes = (ctypes.c_longlong * n)(), (ctypes.c_longlong * n)()
    _lib.check(_lib.lib().curv_persample_dw_plan_info(arr, n, flops, nbytes), "curv_persample_dw_plan_info")
    return [int(v) for v in flops], [int(v) for v in nbytes]


def per_sample_dw_sq_accumulate(jobs: Sequence[PerSampleDwJob]) -> None:
    """``dst[c, j] (+)= alpha sum_n p[n, c, j]**2`` for every job (curv_persample_dw_sq_accumulate), on the current stream;
    the products p from `workspace`."""
    if not jobs:
        return
    _run_build("curv_persample_dw_workspace_bytes", "curv_persample_dw_sq_accumulate",
               _per_sample_dw_descs(jobs, "per_sample_dw_sq_accumulate", "sq"), len(jobs), jobs[0].dst.device, "persample_dw")


def per_sample_dw_quad_reduce(jobs: Sequence[PerSampleDwJob]) -> None:
    """``out[n] (+)= alpha sum_c s[c]**2 sum_j W[c, j] (sum_i T[c, i, j] p[n, c, i])**2`` for every job
    (curv_persample_dw_quad_reduce), on the current stream; the products p from `workspace`."""
    if not jobs:
        return
    _run_build("curv_persample_dw_workspace_bytes", "curv_persample_dw_quad_reduce",
               _per_sample_dw_descs(jobs, "per_sample_dw_quad_reduce", "quad"), len(jobs), jobs[0].out.device,
               "persample_dw")


class PerSampleNormJob:
    """The per-sample products of a normalisation layer (csrc/norm_factor.hip): p[n, c] = (sum g xh, sum g)
    over the positions, from the layer's records `x` and `g` as they are (float32 GPU tensors; shapes for a plan query) seen
    through `view` (`norm_view`).  `dst`, `out`, `T`, `W`, `s`, `alpha`, `first`: as in `PerSampleDwJob`, with
    n_g = 1 + has_bias."""
    __slots__ = ("x", "g", "view", "dst", "out", "T", "W", "s", "alpha", "first")

    def __init__(self, x, g, view, dst=None, out=None, T=None, W=None, s=None, alpha=1.0, first=False):
        self.x, self.g, self.view = x, g, view
        self.dst, self.out, self.T, self.W, self.s = dst, out, T, W, s
        self.alpha, self.first = float(alpha), bool(first)

    @classmethod
    def of(cls, layer, x, g, name: Optional[str] = None, **own):
        """The job of a normalisation `layer` on its records."""
        x, g = (t.detach() if isinstance(t, torch.Tensor) else t for t in (x, g))
        if x is None or g is None:
            raise RuntimeError(f"{name or repr(layer)}: the per-sample products need both records")
        return cls(_job_source(x), _job_source(g), norm_view(layer, x, g, name), **own)


def _per_sample_norm_descs(jobs: Sequence[PerSampleNormJob], name: str, reduction: Optional[str]):
    """`reduction`: "sq", "quad" or None (a plan query: geometry only, `x` / `g` may be shapes)."""
    arr = (_lib.curv_norm_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        tensors = reduction is not None
        _fill_norm_view(d, j.view, j.x if tensors else None, j.g if tensors else None, name)
        d.first, d.alpha = int(j.first), j.alpha
        if reduction is None:
            continue
        N, C, n_g = j.view.dims[0], j.view.dims[1], 1 + int(j.view.has_bias)
        for t in (j.dst,) if reduction == "sq" else (j.out, j.T, j.W, j.s):
            if t is not None and (not t.is_cuda or t.dtype != torch.float32):
                raise RuntimeError(f"{name}: {j.view.name}: float32 GPU tensors expected (no CPU fallback)")
        if reduction == "sq":
            if j.dst is None or j.dst.dim() != 2 or tuple(j.dst.shape) != (C, n_g) or j.dst.stride(1) != 1:
                raise RuntimeError(f"{name}: destination must be a ({C},{n_g}) view with unit column stride, got "
                                   f"{None if j.dst is None else tuple(j.dst.shape)}")
            d.dst, d.c_rs = j.dst.data_ptr(), j.dst.stride(0) if C > 1 else n_g
            continue
        if j.out is None or j.out.dim() != 1 or j.out.shape[0] != N or (N > 1 and j.out.stride(0) < 1):
            raise RuntimeError(f"{name}: destination must be a length-{N} view with a positive stride, got "
                               f"{None if j.out is None else tuple(j.out.shape)}")
        d.out, d.o_stride = j.out.data_ptr(), max(j.out.stride(0), 1)
        _dw_transform(d, j, name, C, n_g)
        if j.W is not None:
            if tuple(j.W.shape) != (C, n_g) or (n_g > 1 and j.W.stride(1) != 1):
                raise RuntimeError(f"{name}: W must be a ({C},{n_g}) view with unit column stride, got {tuple(j.W.shape)}")
            d.Wt, d.w_rs = j.W.data_ptr(), j.W.stride(0) if C > 1 else n_g
        if j.s is not None:
            if j.s.numel() != C or not j.s.is_contiguous():
                raise RuntimeError(f"{name}: s must hold {C} contiguous values, got {tuple(j.s.shape)}")
            d.s = j.s.data_ptr()
    return arr


def per_sample_norm_plan_info(jobs: Sequence[PerSampleNormJob]):
    """(flops, bytes) per job (curv_persample_norm_plan_info, host only): the FLOPs of the statistics and product passes
    and the bytes the algorithm needs (x twice - once with given statistics - and g once)."""
    if not jobs:
        return [], []
    n = len(jobs)
    arr = _per_sample_norm_descs(jobs, "per_sample_norm_plan_info", None)
    flops, nbytes = (ctypes.c_longlong * n)(), (ctypes.c_longlong * n)()
    _lib.check(_lib.lib().curv_persample_norm_plan_info(arr, n, flops, nbytes), "curv_persample_norm_plan_info")
    return [int(v) for v in flops], [int(v) for v in nbytes]


def per_sample_norm_sq_accumulate(jobs: Sequence[PerSampleNormJob]) -> None:
    """``dst[c, j] (+)= alpha sum_n p[n, c, j]**2`` for every job (curv_persample_norm_sq_accumulate), on the current
    stream; the statistics and the products p from `workspace`."""
    if not jobs:
        return
    _run_build("curv_persample_norm_workspace_bytes", "curv_persample_norm_sq_accumulate",
               _per_sample_norm_descs(jobs, "per_sample_norm_sq_accumulate", "sq"), len(jobs), jobs[0].dst.device,
               "persample_norm")


def per_sample_norm_quad_reduce(jobs: Sequence[PerSampleNormJob]) -> None:
    """``out[n] (+)= alpha sum_c s[c]**2 sum_j W[c, j] (sum_i T[c, i, j] p[n, c, i])**2`` for every job
    (curv_persample_norm_quad_reduce), on the current stream; the statistics and the products p from `workspace`."""
    if not jobs:
        return
    _run_build("curv_persample_norm_workspace_bytes", "curv_persample_norm_quad_reduce",
               _per_sample_norm_descs(jobs, "per_sample_norm_quad_reduce", "quad"), len(jobs), jobs[0].out.device,
               "persample_norm")


class EmbeddingWalk(NamedTuple):
    """`embedding_walk_plan`: the grouped position list the segment walker of csrc/embedding_factor.hip reads (int32
    tensors on the device of the indices).  `pos`: the kept positions n T + t, sorted by outer key, inner key, position;
    `chunks` (C, 4): {begin, end, group, slot} - pos[begin:end] belongs to outer key `group`, at most `split` positions,
    `slot` -1 where the chunk is its whole group, else its number among the chunks of split groups; `mgroups` (M, 3):
    {slot_begin, slot_end, group} of every split group; `n_slots`: how many chunks have a slot."""
    pos: torch.Tensor
    chunks: torch.Tensor
    mgroups: torch.Tensor
    n_slots: int


def embedding_walk_plan(idx: torch.Tensor, V: int, padding_idx: Optional[int], mode: int,
                        split: int = _lib.EMB_SPLIT_L) -> EmbeddingWalk:
    """The positions of the (N, *) index tensor `idx` grouped for the per-sample kernels: by token and, inside it, sample
    (`mode` ``_lib.EMB_SQ``) or by sample and, inside it, token (``_lib.EMB_QUAD``), positions ascending inside both (a stable
    sort of the N T keys); positions that hold `padding_idx` or an index outside [0, V) are left out.  Every group's list is
    cut into chunks of at most `split` positions.  Plumbing in torch ops, on the device of `idx` (a CPU tensor gives the plan
    on the CPU: the planner's test)."""
    N, dev = idx.shape[0], idx.device
    flat = idx.reshape(-1).to(torch.int64)
    T = flat.numel() // N
    p = torch.arange(flat.numel(), dtype=torch.int64, device=dev)
    keep = (flat >= 0) & (flat < V)
    if padding_idx is not None:
        keep &= flat != padding_idx
    p, v = p[keep], flat[keep]
    n = torch.div(p, T, rounding_mode="floor")
    outer, key = (v, v * N + n) if mode == _lib.EMB_SQ else (n, n * V + v)
    order = torch.sort(key, stable=True).indices
    pos, outer = p[order], outer[order]
    groups, counts = torch.unique_consecutive(outer, return_counts=True)
    starts = torch.cumsum(counts, 0) - counts
    pieces = torch.div(counts + (split - 1), split, rounding_mode="floor")
    which = torch.repeat_interleave(torch.arange(groups.numel(), device=dev), pieces)        # chunk -> its group's number
    first = torch.cumsum(pieces, 0) - pieces
    within = torch.arange(which.numel(), device=dev) - first[which]
    begin = starts[which] + within * split
    end = torch.minimum(begin + split, (starts + counts)[which])
    multi = pieces[which] > 1
    slot = torch.where(multi, torch.cumsum(multi.to(torch.int64), 0) - 1, torch.full_like(begin, -1))
    chunks = torch.stack([begin, end, groups[which], slot], 1).to(torch.int32).contiguous()
    split_groups = pieces > 1
    slot_begin = (torch.cumsum(torch.where(split_groups, pieces, torch.zeros_like(pieces)), 0) - pieces)[split_groups]
    mgroups = torch.stack([slot_begin, slot_begin + pieces[split_groups], groups[split_groups]], 1).to(torch.int32).contiguous()
    return EmbeddingWalk(pos.to(torch.int32).contiguous(), chunks.view(-1, 4), mgroups.view(-1, 3), int(multi.sum()))


def check_embedding_record(what: str, g) -> None:
    """The per-sample kernels of an Embedding read float32 records only, whatever `widen_per_sample` says: RuntimeError in
    the wording of `per_sample_dtype_fault` otherwise."""
    if g.dtype != torch.float32:
        raise RuntimeError(per_sample_dtype_fault(what, g) or f"{what} expects float32 records, got {g.dtype}")


class PerSampleEmbeddingJob:
    """The per-sample gradient of an nn.Embedding weight (csrc/embedding_factor.hip): row v of sample n is
    P_n[v, :] = sum_{t : idx[n, t] = v} g[n, t, :], from the layer's records as they are: `idx` (N, *) int64 / int32, `g`
    (N, *, D) float32, read through its strides where its middle dims collapse to one.  `dst` (V, D): the destination of
    `per_sample_embedding_sq_accumulate`; `out` (N,) and `w` ((V, D) or (V,), or None for ones): those of
    `per_sample_embedding_quad_reduce`.  `alpha`, `first`: as in `PerSampleDwJob`."""
    __slots__ = ("idx", "g", "V", "padding_idx", "name", "dst", "out", "w", "alpha", "first")

    def __init__(self, idx, g, V, padding_idx=None, name="Embedding", dst=None, out=None, w=None, alpha=1.0, first=False):
        self.idx, self.g, self.V = idx, g, int(V)
        self.padding_idx = None if padding_idx is None else int(padding_idx)
        self.name, self.dst, self.out, self.w = name, dst, out, w
        self.alpha, self.first = float(alpha), bool(first)

    @classmethod
    def of(cls, layer, x, g, name: Optional[str] = None, T=None, W=None, s=None, **own):
        """The job of an Embedding `layer` on its records; `W`: the `w` of a quad job (the `direct` terms of an estimator
        name it so; a layer of this kind has no `T` and no `s`)."""
        if x is None or g is None:
            raise RuntimeError(f"{name or repr(layer)}: the per-sample products need both records")
        return cls(x.detach(), g.detach(), layer.num_embeddings, layer.padding_idx, name or repr(layer), w=W, **own)


def _per_sample_embedding_descs(jobs: Sequence[PerSampleEmbeddingJob], what: str, mode: int):
    """The descriptors of `jobs` and what they point to (index copies, record views, position lists), to be kept alive
    until the launches are enqueued."""
    arr = (_lib.curv_embedding_walk_desc * len(jobs))()
    keep = []
    for d, j in zip(arr, jobs):
        for t in (j.idx, j.g):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"{what}: curvature_amd runs on MI355X only: got a CPU tensor for {j.name} (no CPU fallback)")
        check_embedding_record(f"{what}: {j.name}", j.g)
        idx = _embedding_indices(j.idx, f"{what}: {j.name}")
        N, D = int(idx.shape[0]), int(j.g.shape[-1])
        T = idx.numel() // N
        if tuple(j.g.shape[:-1]) != tuple(idx.shape) or D < 1 or j.V < 1:
            raise RuntimeError(f"{what}: {j.name}: grad_output {tuple(j.g.shape)} does not match the indices {tuple(idx.shape)} "
                               f"(V {j.V}, D {D})")
        g = j.g.reshape(N, T, D)                             # (a view where the middle dims collapse to one stride)
        if (D > 1 and g.stride(2) != 1) or any(v < 0 for v in g.stride()):
            g = g.contiguous()
        walk = embedding_walk_plan(idx, j.V, j.padding_idx, mode)
        keep += [idx, g, walk]
        d.idx, d.g, d.positions, d.idx_i64 = idx.data_ptr(), g.data_ptr(), idx.numel(), int(idx.dtype == torch.int64)
        d.g_sn, d.g_st, d.g_elems = (g.stride(0) if N > 1 else 0), (g.stride(1) if T > 1 else 0), _source_extent(g)
        d.N, d.T, d.V, d.D, d.mode, d.first, d.alpha = N, T, j.V, D, mode, int(j.first), j.alpha
        d.padding_idx = -1 if j.padding_idx is None else j.padding_idx
        d.pos, d.chunks, d.mgroups = walk.pos.data_ptr(), walk.chunks.data_ptr(), walk.mgroups.data_ptr()
        d.n_pos, d.n_chunks, d.n_mgroups, d.n_slots = walk.pos.numel(), walk.chunks.shape[0], walk.mgroups.shape[0], walk.n_slots
        if mode == _lib.EMB_SQ:
            t = j.dst
            if t is None or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (j.V, D) or \
                    (D > 1 and t.stride(1) != 1) or (j.V > 1 and t.stride(0) < D):
                raise RuntimeError(f"{what}: {j.name}: destination must be a float32 GPU ({j.V},{D}) view with unit column "
                                   f"stride, got {None if t is None else (tuple(t.shape), t.dtype)}")
            d.dst, d.dst_rs = t.data_ptr(), t.stride(0) if j.V > 1 else D
            continue
        t = j.out
        if t is None or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != N or \
                (N > 1 and t.stride(0) < 1):
            raise RuntimeError(f"{what}: {j.name}: destination must be a float32 GPU length-{N} view with a positive stride, "
                               f"got {None if t is None else (tuple(t.shape), t.dtype)}")
        d.out, d.o_stride = t.data_ptr(), max(t.stride(0), 1)
        if j.w is not None:
            w = j.w
            if not w.is_cuda or w.dtype != torch.float32:
                raise RuntimeError(f"{what}: {j.name}: w must be a float32 GPU tensor, got {w.dtype} on {w.device}")
            if tuple(w.shape) == (j.V, D) and (D == 1 or w.stride(1) == 1) and (j.V == 1 or w.stride(0) >= D):
                d.w, d.w_rs, d.w_kind = w.data_ptr(), w.stride(0) if j.V > 1 else D, _lib.EMB_W_MATRIX
            elif tuple(w.shape) == (j.V,) and w.is_contiguous():
                d.w, d.w_kind = w.data_ptr(), _lib.EMB_W_VECTOR
            else:
                raise RuntimeError(f"{what}: {j.name}: w must be a ({j.V},{D}) view with unit column stride or a contiguous "
                                   f"({j.V},) vector, got {tuple(w.shape)}")
    return arr, keep


def per_sample_embedding_sq_accumulate(jobs: Sequence[PerSampleEmbeddingJob]) -> None:
    """``dst[v, :] (+)= alpha sum_n P_n[v, :]**2`` for every job (curv_persample_embedding_sq_accumulate), on the current
    stream: the exact per-sample Fisher diagonal of an Embedding weight.  No floating-point atomics: two calls on the same
    inputs give the same bits."""
    if not jobs:
        return
    arr, keep = _per_sample_embedding_descs(jobs, "per_sample_embedding_sq_accumulate", _lib.EMB_SQ)
    _run_build("curv_persample_embedding_workspace_bytes", "curv_persample_embedding_sq_accumulate", arr, len(jobs),
               jobs[0].dst.device, "persample_embedding")
    del keep


def per_sample_embedding_quad_reduce(jobs: Sequence[PerSampleEmbeddingJob]) -> None:
    """``out[n] (+)= alpha sum_v sum_d w[v, d] P_n[v, d]**2`` for every job (curv_persample_embedding_quad_reduce), on the
    current stream; `w` (V, D), or (V,) broadcast over d: the Embedding's row of `functional_variance`."""
    if not jobs:
        return
    arr, keep = _per_sample_embedding_descs(jobs, "per_sample_embedding_quad_reduce", _lib.EMB_QUAD)
    _run_build("curv_persample_embedding_workspace_bytes", "curv_persample_embedding_quad_reduce", arr, len(jobs),
               jobs[0].out.device, "persample_embedding")
    del keep


class PerSampleDwProjectJob(PerSampleDwJob):
    """``y[n, c n_g + j] = s[c] W[c, j] sum_i T[c, i, j] p[n, c, i]`` of a depthwise layer (`per_sample_dw_project`): records
    and geometry as in `PerSampleDwJob`, `T`, `W` (not squared) and `s` likewise, each or all None; `y` an (N, C n_g) float32
    view with unit last stride (a slot of a staged stack).  `x` / `g` may also be shapes (plan queries)."""
    __slots__ = ("y",)

    def __init__(self, x, g, kernel, stride=(1, 1), padding=(0, 0), has_bias=False, y=None, T=None, W=None, s=None):
        super().__init__(x, g, kernel, stride, padding, has_bias, T=T, W=W, s=s)
        self.y = y


class PerSampleDwGridJob(PerSampleDwJob):
    """``out[h, n] (+)= gain[h] sum_cj w_h[c, j] (sum_i T[c, i, j] p[n, c, i])**2`` of a depthwise layer for the H grid points
    ``(shift[h], gain[h])`` (`per_sample_dw_quad_grid_reduce`; at most `PERSAMPLE_GRID_MAX`): records, geometry and `T` as
    in `PerSampleDwJob`.  The weights are separable, ``w_h[c, j] = 1 / ((u[c] + shift[h]) (v[c, j] + shift[h]))`` with `u` C
    contiguous values and `v` a (C, n_g) view with unit column stride, or dense, ``w_h[c, j] = 1 / (V[c, j] + shift[h])``
    with `V` such a view: give `u` and `v`, or `V`.  `shift` (finite, > 0) and `gain` (finite) are sequences of H Python
    floats; `out` an (H, N) float32 view with positive strides.  There is no `alpha`.  `x` / `g` may also be shapes
    (plan queries)."""
    __slots__ = ("u", "v", "V", "shift", "gain")

    def __init__(self, x, g, kernel, stride=(1, 1), padding=(0, 0), has_bias=False, out=None, T=None, u=None, v=None, V=None,
                 shift=(), gain=(), first=False):
        super().__init__(x, g, kernel, stride, padding, has_bias, out=out, T=T, first=first)
        self.u, self.v, self.V = u, v, V
        self.shift, self.gain = [float(x) for x in shift], [float(x) for x in gain]


def _per_sample_dw_project_descs(jobs: Sequence[PerSampleDwProjectJob], name: str, check_tensors: bool = True):
    arr = (_lib.curv_persample_dw_project_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        xs, _ = _fill_dw_record(d, j, name)
        N, C, n_g = xs[0], xs[1], j.kernel[0] * j.kernel[1] + int(j.has_bias)
        d.y_ns = C * n_g
        if not check_tensors:
            continue
        _fill_dw_pointers(d, j, (j.y, j.T, j.W, j.s))
        if j.y is None or j.y.dim() != 2 or tuple(j.y.shape) != (N, C * n_g) or (C * n_g > 1 and j.y.stride(1) != 1) or \
                (N > 1 and j.y.stride(0) < C * n_g):
            raise RuntimeError(f"{name}: destination must be an ({N},{C * n_g}) view with unit last stride and rows that do "
                               f"not overlap, got {None if j.y is None else tuple(j.y.shape)}")
        d.y, d.y_ns = j.y.data_ptr(), j.y.stride(0) if N > 1 else C * n_g
        _dw_transform(d, j, name, C, n_g)
        if j.W is not None:
            if tuple(j.W.shape) != (C, n_g) or (n_g > 1 and j.W.stride(1) != 1):
                raise RuntimeError(f"{name}: W must be a ({C},{n_g}) view with unit column stride, got {tuple(j.W.shape)}")
            d.Wt, d.w_rs = j.W.data_ptr(), j.W.stride(0) if C > 1 else n_g
        if j.s is not None:
            if j.s.numel() != C or not j.s.is_contiguous():
                raise RuntimeError(f"{name}: s must hold {C} contiguous values, got {tuple(j.s.shape)}")
            d.s = j.s.data_ptr()
    return arr


def _per_sample_dw_grid_descs(jobs: Sequence[PerSampleDwGridJob], name: str, check_tensors: bool = True):
    arr = (_lib.curv_persample_dw_grid_desc * len(jobs))()
    keep = []                                        # the host tables the descriptors point to
    for d, j in zip(arr, jobs):
        H = len(j.shift)
        if not 1 <= H <= PERSAMPLE_GRID_MAX or len(j.gain) != H:
            raise ValueError(f"{name}: {H} shifts and {len(j.gain)} gains; a job takes 1 to {PERSAMPLE_GRID_MAX} grid "
                             "points, as many gains as shifts")
        for h, (s, g) in enumerate(zip(j.shift, j.gain)):
            if not (s > 0 and math.isfinite(s) and math.isfinite(g)):
                raise ValueError(f"{name}: grid point {h}: shift {s} must be finite and > 0, gain {g} finite")
        xs, _ = _fill_dw_record(d, j, name)
        N, C, n_g = xs[0], xs[1], j.kernel[0] * j.kernel[1] + int(j.has_bias)
        d.Hn, d.first = H, int(j.first)
        tables = ((ctypes.c_float * H)(*j.shift), (ctypes.c_float * H)(*j.gain))
        keep.append(tables)
        d.shift, d.gain = ctypes.cast(tables[0], ctypes.POINTER(ctypes.c_float)), ctypes.cast(tables[1], ctypes.POINTER(ctypes.c_float))
        d.v_rs, d.o_stride, d.o_hs = n_g, 1, N
        if not check_tensors:
            continue
        separable = j.V is None
        if (j.u is None) != (j.v is None) or separable == (j.u is None):
            raise RuntimeError(f"{name}: give the weights as u and v (separable) or as V (dense), not both")
        _fill_dw_pointers(d, j, (j.out, j.T, j.u, j.v, j.V))
        _dw_transform(d, j, name, C, n_g)
        table = j.v if separable else j.V
        if tuple(table.shape) != (C, n_g) or (n_g > 1 and table.stride(1) != 1):
            raise RuntimeError(f"{name}: {'v' if separable else 'V'} must be a ({C},{n_g}) view with unit column stride, got "
                               f"{tuple(table.shape)}")
        d.v_rs = table.stride(0) if C > 1 else n_g
        if separable:
            if j.u.numel() != C or not j.u.is_contiguous():
                raise RuntimeError(f"{name}: u must hold {C} contiguous values, got {tuple(j.u.shape)}")
            d.u, d.v = j.u.data_ptr(), j.v.data_ptr()
        else:
            d.V = j.V.data_ptr()
        if j.out is None or j.out.dim() != 2 or tuple(j.out.shape) != (H, N) or (N > 1 and j.out.stride(1) < 1) or \
                (H > 1 and j.out.stride(0) < 1):
            raise RuntimeError(f"{name}: destination must be an ({H},{N}) view with positive strides, got "
                               f"{None if j.out is None else tuple(j.out.shape)}")
        d.out, d.o_stride, d.o_hs = j.out.data_ptr(), max(j.out.stride(1), 1), max(j.out.stride(0), 1)
    arr._tables = keep
    return arr


def _dw_plan_info(symbol: str, arr, n: int):
    flops, nbytes = (ctypes.c_longlong * n)(), (ctypes.c_longlong * n)()
    _lib.check(getattr(_lib.lib(), symbol)(arr, n, flops, nbytes), symbol)
    return [int(v) for v in flops], [int(v) for v in nbytes]


def per_sample_dw_project_plan_info(jobs: Sequence[PerSampleDwProjectJob]):
    """(flops, bytes) per job (curv_persample_dw_project_plan_info, host only): those of `per_sample_dw_plan_info` plus the
    transform by T and the N C n_g values written."""
    if not jobs:
        return [], []
    return _dw_plan_info("curv_persample_dw_project_plan_info",
                         _per_sample_dw_project_descs(jobs, "per_sample_dw_project_plan_info", False), len(jobs))


def per_sample_dw_quad_grid_plan_info(jobs: Sequence[PerSampleDwGridJob]):
    """(flops, bytes) per job (curv_persample_dw_quad_grid_plan_info, host only): those of `per_sample_dw_plan_info` plus the
    transform by T and the H weighted sums."""
    if not jobs:
        return [], []
    return _dw_plan_info("curv_persample_dw_quad_grid_plan_info",
                         _per_sample_dw_grid_descs(jobs, "per_sample_dw_quad_grid_plan_info", False), len(jobs))


def per_sample_dw_project(jobs: Sequence[PerSampleDwProjectJob]) -> None:
    """``y[n, c n_g + j] = s[c] W[c, j] sum_i T[c, i, j] p[n, c, i]`` for every job (curv_persample_dw_project), on the
    current stream; the products p from `workspace`."""
    if not jobs:
        return
    _run_build("curv_persample_dw_project_workspace_bytes", "curv_persample_dw_project",
               _per_sample_dw_project_descs(jobs, "per_sample_dw_project"), len(jobs), jobs[0].y.device, "persample_dw")


def per_sample_dw_quad_grid_reduce(jobs: Sequence[PerSampleDwGridJob]) -> None:
    """``out[h, n] (+)= gain[h] sum_cj w_h[c, j] (sum_i T[c, i, j] p[n, c, i])**2`` for every job
    (curv_persample_dw_quad_grid_reduce), on the current stream; the products p from `workspace`."""
    if not jobs:
        return
    _run_build("curv_persample_dw_quad_grid_workspace_bytes", "curv_persample_dw_quad_grid_reduce",
               _per_sample_dw_grid_descs(jobs, "per_sample_dw_quad_grid_reduce"), len(jobs), jobs[0].out.device,
               "persample_dw")


class PerSampleGramJob:
    """``out[n, k, k'] (+)= alpha sum_e Y[k, n, e] Y[k', n, e]`` (`per_sample_gram_reduce`): `Y` a (K, N, E) float32 view with
    unit last stride (K at most `PERSAMPLE_COV_MAX_OUTPUTS`; a staged stack of `per_sample_dw_project` rows), `out` an
    (N, K, K) view with unit last stride, as `PerSampleCovJob` takes it.  `first`: overwrite out."""
    __slots__ = ("Y", "out", "alpha", "first")

    def __init__(self, Y, out, alpha=1.0, first=False):
        self.Y, self.out, self.alpha, self.first = Y, out, float(alpha), bool(first)


def per_sample_gram_reduce(jobs: Sequence[PerSampleGramJob]) -> None:
    """curv_persample_gram_reduce over any number of jobs, on the current stream (no workspace).  The jobs of a call must
    not share destinations."""
    if not jobs:
        return
    name = "per_sample_gram_reduce"
    arr = (_lib.curv_persample_gram_desc * len(jobs))()
    for d, j in zip(arr, jobs):
        for t in (j.Y, j.out):
            if not t.is_cuda:
                raise RuntimeError("curvature_amd runs on MI355X only: got a CPU tensor (no CPU fallback)")
            if t.dtype != torch.float32:
                raise RuntimeError(f"curvature_amd expects float32 tensors, got {t.dtype}")
        if j.Y.dim() != 3 or not 1 <= j.Y.shape[0] <= PERSAMPLE_COV_MAX_OUTPUTS or j.Y.shape[2] < 1 or \
                (j.Y.shape[2] > 1 and j.Y.stride(2) != 1) or min(j.Y.stride()) < 0:
            raise RuntimeError(f"{name}: Y must be a (K, N, E) view with unit last stride, 1 <= K <= "
                               f"{PERSAMPLE_COV_MAX_OUTPUTS}, got {tuple(j.Y.shape)}")
        K, N, E = map(int, j.Y.shape)
        if j.out.dim() != 3 or tuple(j.out.shape) != (N, K, K) or (K > 1 and j.out.stride(2) != 1):
            raise RuntimeError(f"{name}: destination must be an ({N},{K},{K}) view with unit last stride, got "
                               f"{tuple(j.out.shape)}")
        d.Y, d.out, d.N, d.K, d.E = j.Y.data_ptr(), j.out.data_ptr(), N, K, E
        d.y_ks, d.y_ns = j.Y.stride(0) if K > 1 else 0, j.Y.stride(1) if N > 1 else 0
        # (the stride of a dimension of size 1 says nothing: take the smallest the library allows)
        d.o_rs = j.out.stride(1) if K > 1 else K
        d.o_ns = j.out.stride(0) if N > 1 else K * d.o_rs
        d.first, d.alpha = int(j.first), j.alpha
    _lib.check(_lib.lib().curv_persample_gram_reduce(_lib.stream_ptr(), arr, len(arr)), "curv_persample_gram_reduce")


def per_sample_scratch(floats: Sequence[int], device, tag: str = "persample_x") -> List[torch.Tensor]:
    """One float32 buffer of each given size (0: None), carved 256-byte aligned out of the `tag` workspace: the
    packed operands of one `update()`; valid until the next call with that tag."""
    offs, at = [], 0
    for f in floats:
        offs.append(at)
        at += (int(f) * 4 + 255) // 256 * 256
    if at == 0:
        return [None] * len(offs)
    ws = workspace(at, device, tag)
    return [ws[o:o + int(f) * 4].view(torch.float32) if f else None for o, f in zip(offs, floats)]


def rsqrt_affine(value: torch.Tensor, add: float, multiply: float, out: Optional[torch.Tensor] = None):
    _require_gpu(value, out)
    if out is None:
        out = torch.empty_like(value)
    _lib.check(_lib.lib().curv_rsqrt_affine(_lib.stream_ptr(), value.data_ptr(), float(multiply), float(add),
                                            out.data_ptr(), value.numel()), "curv_rsqrt_affine")
    return out


def sq_accumulate(grad_w: torch.Tensor, grad_b: Optional[torch.Tensor], batch_size: float,
                  state: Optional[torch.Tensor], first: Optional[bool] = None) -> torch.Tensor:
    """state (+)= batch_size * [grad_w.view(m,-1) | grad_b]**2 ; allocates when state is None.  `first`: overwrite a
    given (preallocated, uninitialised) state instead of adding to it; default: only when it is allocated here."""
    _require_gpu(grad_w, grad_b, state)
    rows = grad_w.shape[0]
    cols_w = math.prod(grad_w.shape[1:])
    if first is None:
        first = state is None
    if state is None:
        state = torch.empty(rows, cols_w + (grad_b is not None), dtype=torch.float32, device=grad_w.device)
    elif tuple(state.shape) != (rows, cols_w + (grad_b is not None)) or not state.is_contiguous():
        raise RuntimeError("sq_accumulate: state does not match the gradient's [W | b] shape")
    _lib.check(_lib.lib().curv_sq_accumulate(_lib.stream_ptr(), grad_w.data_ptr(),
                                             grad_b.data_ptr() if grad_b is not None else None,
                                             rows, cols_w, float(batch_size), state.data_ptr(), int(first)),
               "curv_sq_accumulate")
    return state


def sq_accumulate_many(items, batch_size: float) -> List[torch.Tensor]:
    """`sq_accumulate` for a list of (grad_w, grad_b or None, state or None, first or None) in ONE launch
    (curv_sq_accumulate_batched); returns the state tensors (allocated where None was given)."""
    items = list(items)
    if not items:
        return []
    arr = (curv_sq_desc * len(items))()
    states = []
    for d, (grad_w, grad_b, state, first) in zip(arr, items):
        _require_gpu(grad_w, grad_b, state)
        if not grad_w.is_contiguous() or (grad_b is not None and not grad_b.is_contiguous()):
            raise RuntimeError("sq_accumulate_many: gradients must be contiguous")
        rows = grad_w.shape[0]
        cols_w = math.prod(grad_w.shape[1:])           # not numel() // rows: a rows = 0 item is legal and skipped
        if first is None:
            first = state is None
        if state is None:
            state = torch.empty(rows, cols_w + (grad_b is not None), dtype=torch.float32, device=grad_w.device)
        elif tuple(state.shape) != (rows, cols_w + (grad_b is not None)) or not state.is_contiguous():
            raise RuntimeError("sq_accumulate_many: state does not match the gradient's [W | b] shape")
        states.append(state)
        d.grad_w, d.grad_b, d.state = grad_w.data_ptr(), (grad_b.data_ptr() if grad_b is not None else None), state.data_ptr()
        d.rows, d.cols_w, d.first = rows, cols_w, int(first)
    _lib.check(_lib.lib().curv_sq_accumulate_batched(_lib.stream_ptr(), arr, len(items), float(batch_size)),
               "curv_sq_accumulate_batched")
    return states


def chol_inv_lower(factors: Sequence[torch.Tensor], adds: Sequence[float], multiplies: Sequence[float],
                   check: bool = True, outs: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """[chol_lower((sqrt(s_i) F_i + sqrt(n_i) I)^-1)] for all factors in one batched sweep.

    Raises ``RuntimeError`` (like torch's cholesky in the reference, curvatures.py:378-380) when a damped
    factor is not positive definite; set ``check=False`` to skip the host read-back of the status words."""
    n = len(factors)
    if n == 0:
        return []
    arr = (curv_inv_desc * n)()
    given = list(outs) if outs is not None else [None] * n
    outs = []
    for d, F, a, s, out in zip(arr, factors, adds, multiplies, given):
        _require_gpu(F)
        if F.dim() != 2 or F.shape[0] != F.shape[1]:
            raise RuntimeError("factor must be a square matrix")
        if out is None or out.shape != F.shape or out.device != F.device or not out.is_contiguous() \
                or out.dtype != torch.float32:
            out = torch.empty_like(F)          # `outs` entries are reused when they fit (stable pointers)
        outs.append(out)
        d.F, d.L, d.n, d.add, d.multiply = F.data_ptr(), out.data_ptr(), F.shape[0], float(a), float(s)
    dev = factors[0].device
    info = torch.empty(n, dtype=torch.int32, device=dev)
    L = _lib.lib()
    need = L.curv_chol_inv_workspace_bytes(arr, n)
    ws = workspace(need, dev, "invert")
    early = check and not torch.cuda.is_current_stream_capturing()
    if early:
        # the verdict travels to pinned host memory BEFORE the finalize passes (curv_chol_inv_lower_status): the host
        # waits for that copy only, and what it does next - raising, or preparing the sampler's launches - runs in the
        # shadow of the finalize passes instead of behind them (0.12 ms of idle GPU per ResNet-50 step otherwise)
        host, event = _status_box(n, dev)
        _lib.check(L.curv_chol_inv_lower_status(_lib.stream_ptr(), arr, n, info.data_ptr(), ws.data_ptr(), ws.numel(),
                                                host.data_ptr(), event), "curv_chol_inv_lower_status")
    else:
        _lib.check(L.curv_chol_inv_lower(_lib.stream_ptr(), arr, n, info.data_ptr(), ws.data_ptr(), ws.numel()),
                   "curv_chol_inv_lower")
    chol_inv_lower.last_info = info              # (kept for older callers; process-global: use the attribute below)
    outs = _ListWithInfo(outs)
    outs.info = info                             # check=False: the caller reads it later (check_chol_info)
    if early:
        _lib.check(L.curv_event_synchronize(event), "curv_event_synchronize")    # the one host wait of invert()
        check_chol_info(host)
    elif check:
        check_chol_info(info)
    return outs


_status_boxes = threading.local()


def _status_box(n: int, device):
    """Pinned host words and a HIP event for the early verdict of one `chol_inv_lower` call: one box per thread AND
    device (a HIP event belongs to the device that was current when it was created; recording it on a stream of another
    device is an invalid-handle error), grown on demand; a call waits for its own copy before it returns."""
    boxes = _status_boxes.__dict__.setdefault("boxes", {})
    key = torch.device(device).index
    if key is None:
        key = torch.cuda.current_device()
    box = boxes.get(key)
    if box is None or box[0].numel() < n:
        with torch.cuda.device(key):
            if box is not None:
                _lib.lib().curv_event_destroy(box[1])
            event = _lib.lib().curv_event_create()
        if not event:
            raise RuntimeError("curv_event_create failed")
        box = boxes[key] = (torch.empty(max(n, 256), dtype=torch.int32).pin_memory(), event)
    return box[0][:n], box[1]


class _ListWithInfo(list):
    """The list of inverse factors of one `chol_inv_lower` call, carrying that call's status words (`.info`)."""
    info = None


def check_chol_info(info: torch.Tensor) -> None:
    """Raise ``RuntimeError`` if a status word of a finished `chol_inv_lower` sweep reports a non-positive pivot."""
    host = info.cpu()
    bad = torch.nonzero(host).flatten().tolist()
    if bad:
        lost = [i for i in bad if int(host[i]) < 0]
        if lost:
            # status -1: a workgroup of chol_square_kernel gave up waiting for a tile from another workgroup of its
            # launch (bounded spin: all workgroups of a factor must be resident at once) - not a property of the matrix
            raise RuntimeError(f"cholesky: inter-workgroup hand-off timed out for factor(s) {lost} (the GPU could not keep "
                               "the sweep's workgroups resident: CU-masked / partitioned device or heavy contention); "
                               "set CURV_LATENCY_MAX=0 to use the per-step launches")
        raise RuntimeError(f"cholesky: damped factor(s) {bad} are not positive-definite "
                           f"(first failing pivot {int(host[bad[0]]) - 1})")


EPI_NONE, EPI_SQUARE, EPI_MUL_E, EPI_ADD_E, EPI_MUL_E_ADD_F = 0, 1, 2, 3, 4
TRI_NONE, TRI_A_LOWER, TRI_B_UPPER = 0, 1, 2


class Gemm:
    """C = epilogue(alpha * A @ B) [+ beta * C] on 2-D views (any strides: .t() and slices are free)."""
    __slots__ = ("A", "B", "C", "E", "F", "alpha", "beta", "epilogue", "tri")

    def __init__(self, A, B, C, alpha=1.0, beta=0.0, epilogue=EPI_NONE, E=None, tri=0, F=None):
        self.A, self.B, self.C, self.E, self.F = A, B, C, E, F
        self.alpha, self.beta, self.epilogue, self.tri = float(alpha), float(beta), int(epilogue), int(tri)


def _check_view(t: torch.Tensor):
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
        raise RuntimeError("GEMM operands must be 2-D float32 GPU tensors (no CPU fallback)")


def _gemm_descs(jobs: Sequence[Gemm]):
    n = len(jobs)
    arr = (curv_gemm_desc * n)()
    for d, j in zip(arr, jobs):
        for t in (j.A, j.B, j.C):
            _check_view(t)
        M, K = j.A.shape
        K2, N = j.B.shape
        if K != K2 or tuple(j.C.shape) != (M, N):
            raise RuntimeError(f"GEMM shape mismatch: {tuple(j.A.shape)} @ {tuple(j.B.shape)} -> {tuple(j.C.shape)}")
        d.A, d.B, d.C = j.A.data_ptr(), j.B.data_ptr(), j.C.data_ptr()
        d.a_rs, d.a_cs = j.A.stride()
        d.b_rs, d.b_cs = j.B.stride()
        d.c_rs, d.c_cs = j.C.stride()
        if j.E is not None:
            _check_view(j.E)
            if tuple(j.E.shape) != (M, N):
                raise RuntimeError("GEMM epilogue operand must match the output shape")
            d.E = j.E.data_ptr()
            d.e_rs, d.e_cs = j.E.stride()
        if j.F is not None:
            _check_view(j.F)
            if tuple(j.F.shape) != (M, N):
                raise RuntimeError("GEMM epilogue operand must match the output shape")
            d.F = j.F.data_ptr()
            d.f_rs, d.f_cs = j.F.stride()
        d.M, d.N, d.K = M, N, K
        d.alpha, d.beta, d.epilogue, d.tri = j.alpha, j.beta, j.epilogue, j.tri
    return arr


def gemm_batched(jobs: Sequence[Gemm]) -> None:
    """All products in one launch (one work item per 64x64 output tile)."""
    if not jobs:
        return
    GemmPlan(jobs).run()


GEMM_PLAN_KEYS = ("tiles64", "tiles128", "nt_items", "split_products", "reduce_wgs", "small_blocks", "gemv_wgs",
                  "order_entries")


def gemm_plan_info(jobs, workspace_bytes: Optional[int] = None) -> dict:
    """What `gemm_batched(jobs)` would launch (curv_gemm_plan_info; host only): work items per kernel under the keys of
    GEMM_PLAN_KEYS.  `jobs`: a list of Gemm, or a ctypes array of curv_gemm_desc.  `workspace_bytes`: the size GemmPlan
    allocates unless given."""
    descs = jobs if isinstance(jobs, ctypes.Array) else (_gemm_descs(jobs) if len(jobs) else None)
    n = len(jobs)
    L = _lib.lib()
    if workspace_bytes is None:
        workspace_bytes = max(int(L.curv_gemm_workspace_bytes_for(descs, n)), 256) if n else 0
    out = (ctypes.c_longlong * _lib.GEMM_PLAN_FIELDS)()
    _lib.check(L.curv_gemm_plan_info(descs, n, int(workspace_bytes), out), "curv_gemm_plan_info")
    return dict(zip(GEMM_PLAN_KEYS, (int(v) for v in out)))


class GemmPlan:
    """A fixed list of products: descriptors are built once, `run()` only enqueues (one launch).  The
    operand tensors are kept alive by the plan; their contents may change between runs."""

    def __init__(self, jobs: Sequence[Gemm]):
        self.jobs = list(jobs)
        self.n = len(self.jobs)
        self.descs = _gemm_descs(self.jobs) if self.n else None

    def run(self) -> None:
        if not self.n:
            return
        L = _lib.lib()
        if getattr(self, "_ws", None) is None:
            # table + slabs of K-sliced products (underfilled launches), owned by the plan: nobody else writes there, so
            # the device copy of the descriptor table is uploaded by the first run only (a ResNet-50 sample was 6 upload
            # launches per call otherwise).  Slab space is shared scratch in effect - only this plan's launches use it.
            nbytes = int(L.curv_gemm_workspace_bytes_for(self.descs, self.n))
            self._ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.jobs[0].C.device)
            if _POISON:
                self._ws.fill_(0xFF)
            self._resident_on = None
        stream = _lib.stream_ptr()
        # (the table is written by launches on a stream: only replays on that same stream may rely on it)
        flags = _lib.GEMM_TABLE_RESIDENT if self._resident_on == stream else 0
        rc = L.curv_gemm_batched_ex(stream, self.descs, self.n, self._ws.data_ptr(), self._ws.numel(), flags)
        self._resident_on = stream if rc == 0 else None
        _lib.check(rc, "curv_gemm_batched")


def randn(shape, device, seed: int, offset: int = 0, out: Optional[torch.Tensor] = None,
          counter: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Standard normal noise from the library's Philox generator (counter `offset` in units of 4 values).
    `counter`: a one-element int64 GPU tensor that holds the stream position instead (read by the kernel, advanced by
    a second launch): the form a captured HIP graph needs, see `curvature_amd.graph`."""
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=device)
    else:
        _require_gpu(out)
    if counter is not None:
        if not counter.is_cuda or counter.dtype != torch.int64 or counter.numel() != 1:
            raise RuntimeError("randn: the device counter must be a one-element int64 GPU tensor")
        _lib.check(_lib.lib().curv_randn_counter(_lib.stream_ptr(), out.data_ptr(), out.numel(), int(seed) & (2 ** 64 - 1),
                                                 counter.data_ptr()), "curv_randn_counter")
        return out
    _lib.check(_lib.lib().curv_randn(_lib.stream_ptr(), out.data_ptr(), out.numel(), int(seed) & (2 ** 64 - 1),
                                     int(offset)), "curv_randn")
    return out


def mul(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _require_gpu(a, b, out)
    if a.shape != b.shape:
        raise RuntimeError("mul: shape mismatch")
    if out is None:
        out = torch.empty_like(a)
    _lib.check(_lib.lib().curv_mul(_lib.stream_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel()),
               "curv_mul")
    return out


class CopyPlan:
    """A fixed list of (dst, src) tensor pairs copied with one or a few launches (curv_copy_batched).

    The descriptor array is built once; `run()` only enqueues.  Every pair must be contiguous, of equal
    byte size and on the GPU; the tensors are kept alive by the plan."""

    def __init__(self, dsts: Sequence[torch.Tensor], srcs: Sequence[torch.Tensor]):
        if len(dsts) != len(srcs):
            raise RuntimeError("CopyPlan: list lengths differ")
        for t in (*dsts, *srcs):                 # any dtype: this is a byte copy
            if not t.is_cuda:
                raise RuntimeError("curvature_amd runs on MI355X only: got a CPU tensor (no CPU fallback)")
        self._keep = (list(dsts), list(srcs))
        self.n = len(dsts)
        self.descs = (_lib.curv_copy_desc * max(self.n, 1))()
        for i, (d, s) in enumerate(zip(dsts, srcs)):
            if not (d.is_contiguous() and s.is_contiguous()):
                raise RuntimeError("CopyPlan: tensors must be contiguous")
            nb = d.numel() * d.element_size()
            if nb != s.numel() * s.element_size() or d.dtype != s.dtype:
                raise RuntimeError("CopyPlan: size / dtype mismatch")
            self.descs[i].dst, self.descs[i].src, self.descs[i].bytes = d.data_ptr(), s.data_ptr(), nb

    def run(self) -> None:
        if self.n:
            _lib.check(_lib.lib().curv_copy_batched(_lib.stream_ptr(), self.descs, self.n), "curv_copy_batched")


# ---------------------------------------------------------------------------------------------- EFB / INF helpers
from ._lib import curv_cholinv_desc, curv_gemm64_desc, curv_select_desc  # noqa: E402


def mul2d(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Contiguous a * b for two strided 2-D float32 views of equal shape."""
    _check_view(a)
    _check_view(b)
    if a.shape != b.shape:
        raise RuntimeError("mul2d: shape mismatch")
    if out is None:
        out = torch.empty(a.shape, dtype=torch.float32, device=a.device)
    else:
        _require_gpu(out)
        if out.shape != a.shape:
            raise RuntimeError("mul2d: output shape mismatch")
    _lib.check(_lib.lib().curv_mul2d(_lib.stream_ptr(), a.data_ptr(), a.stride(0), a.stride(1), b.data_ptr(),
                                     b.stride(0), b.stride(1), out.data_ptr(), a.shape[0], a.shape[1]), "curv_mul2d")
    return out


def gather2d(src: torch.Tensor, rows: Optional[torch.Tensor] = None, cols: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Contiguous copy of the strided 2-D view `src`, optionally restricted to the int64 index lists `rows` /
    `cols` (``src.index_select(0, rows).index_select(1, cols).contiguous()`` in one launch; a transposed view
    as `src` gives ``src.t().contiguous()``)."""
    _check_view(src)
    for idx in (rows, cols):
        if idx is not None and (not idx.is_cuda or idx.dtype != torch.int64 or not idx.is_contiguous()):
            raise RuntimeError("gather2d: index lists must be contiguous int64 GPU tensors")
    R = src.shape[0] if rows is None else rows.numel()
    C = src.shape[1] if cols is None else cols.numel()
    if out is None:
        out = torch.empty(R, C, dtype=torch.float32, device=src.device)
    else:
        _require_gpu(out)
        if out.numel() != R * C:
            raise RuntimeError("gather2d: output size mismatch")
    _lib.check(_lib.lib().curv_gather2d(_lib.stream_ptr(), src.data_ptr(), src.stride(0), src.stride(1),
                                        rows.data_ptr() if rows is not None else None,
                                        cols.data_ptr() if cols is not None else None, out.data_ptr(), R, C),
               "curv_gather2d")
    return out


def clamp_min0_(v: torch.Tensor) -> torch.Tensor:
    _require_gpu(v)
    _lib.check(_lib.lib().curv_clamp_min0(_lib.stream_ptr(), v.data_ptr(), v.numel()), "curv_clamp_min0")
    return v


def sqrt_scale(v: torch.Tensor, s: float) -> torch.Tensor:
    _require_gpu(v)
    out = torch.empty_like(v)
    _lib.check(_lib.lib().curv_sqrt_scale(_lib.stream_ptr(), v.data_ptr(), float(s), out.data_ptr(), v.numel()),
               "curv_sqrt_scale")
    return out


def inf_select_many(lambda_vecs, dims, rank: int):
    """[(I, J), ...] int64 index tensors of INF._dim_reduction (exact integers, ascending) for several layers:
    one launch (a workgroup per layer) and ONE host read-back of all low-rank sizes."""
    if not lambda_vecs:
        return []
    dev = lambda_vecs[0].device
    k = len(lambda_vecs)
    counts = torch.zeros(k, 2, dtype=torch.int32, device=dev)
    d = (curv_select_desc * k)()
    Is, Js = [], []
    for i, (vec, (n, m)) in enumerate(zip(lambda_vecs, dims)):
        _require_gpu(vec)
        I = torch.empty(n, dtype=torch.int64, device=dev)
        J = torch.empty(m, dtype=torch.int64, device=dev)
        Is.append(I)
        Js.append(J)
        d[i].lambda_vec, d[i].I, d[i].J, d[i].counts = vec.data_ptr(), I.data_ptr(), J.data_ptr(), counts[i].data_ptr()
        d[i].n, d[i].m, d[i].rank = n, m, int(rank)
    _lib.check(_lib.lib().curv_inf_select(_lib.stream_ptr(), d, k), "curv_inf_select")
    sizes = counts.tolist()                    # host read-back: sizes of the low-rank factors
    return [(I[:a], J[:b]) for I, J, (a, b) in zip(Is, Js, sizes)]


def inf_select(lambda_vec: torch.Tensor, n: int, m: int, rank: int):
    """(I, J) of one layer (see inf_select_many)."""
    return inf_select_many([lambda_vec], [(n, m)], rank)[0]


def colpairs(U: torch.Tensor, f64: bool = False) -> torch.Tensor:
    """(n, a) -> (n, a*a) with out[p, i*a+k] = U[p,i] U[p,k]; `f64`: exact products in float64."""
    _require_gpu(U)
    n, a = U.shape
    out = torch.empty(n, a * a, dtype=torch.float64 if f64 else torch.float32, device=U.device)
    fn = _lib.lib().curv_colpairs_f64 if f64 else _lib.lib().curv_colpairs
    _lib.check(fn(_lib.stream_ptr(), U.data_ptr(), n, a, U.stride(0), out.data_ptr()), "curv_colpairs")
    return out


def colpairs_sym(U: torch.Tensor) -> torch.Tensor:
    """(n, a) -> (n, a (a + 1) / 2) float64 with out[p, t(i, k)] = U[p,i] U[p,k] for i <= k, t(i, k) = i a - i (i - 1) / 2 + k - i:
    the distinct columns of `colpairs`."""
    _require_gpu(U)
    n, a = U.shape
    out = torch.empty(n, a * (a + 1) // 2, dtype=torch.float64, device=U.device)
    _lib.check(_lib.lib().curv_colpairs_sym_f64(_lib.stream_ptr(), U.data_ptr(), n, a, U.stride(0), out.data_ptr()),
               "curv_colpairs_sym_f64")
    return out


def inf_vtv_assemble_sym(V4p: torch.Tensor, sigma: torch.Tensor, a: int, b: int) -> torch.Tensor:
    """vtv (ab x ab, float64) from the packed V4p (a (a + 1) / 2 x b (b + 1) / 2) of `colpairs_sym` operands."""
    _require_gpu(sigma)
    if not V4p.is_cuda or not V4p.is_contiguous() or V4p.dtype != torch.float64 \
            or V4p.shape != (a * (a + 1) // 2, b * (b + 1) // 2):
        raise RuntimeError("inf_vtv_assemble_sym: bad V4p")
    out = torch.empty(a * b, a * b, dtype=torch.float64, device=V4p.device)
    _lib.check(_lib.lib().curv_inf_vtv_assemble_sym_f64(_lib.stream_ptr(), V4p.data_ptr(), sigma.data_ptr(), a, b,
                                                        out.data_ptr()), "curv_inf_vtv_assemble_sym_f64")
    return out


def square_f64(v: torch.Tensor) -> torch.Tensor:
    """float64 v**2 of a float32 tensor (same shape)."""
    _require_gpu(v)
    out = torch.empty(v.shape, dtype=torch.float64, device=v.device)
    _lib.check(_lib.lib().curv_square_f64(_lib.stream_ptr(), v.data_ptr(), out.data_ptr(), v.numel()), "curv_square_f64")
    return out


def inf_vtv_assemble(V4: torch.Tensor, sigma: torch.Tensor, a: int, b: int) -> torch.Tensor:
    """vtv (ab x ab) from V4 (a*a x b*b), in V4's precision (float32 or float64)."""
    _require_gpu(sigma)
    if not V4.is_cuda or not V4.is_contiguous() or V4.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("inf_vtv_assemble: bad V4")
    if a <= 0 or b <= 0 or tuple(V4.shape) != (a * a, b * b):
        raise RuntimeError(f"inf_vtv_assemble: V4 is {tuple(V4.shape)}, a = {a}, b = {b} need ({a * a}, {b * b})")
    if sigma.numel() != a * b:
        raise RuntimeError(f"inf_vtv_assemble: sigma has {sigma.numel()} elements, a * b = {a * b}")
    out = torch.empty(a * b, a * b, dtype=V4.dtype, device=V4.device)
    fn = _lib.lib().curv_inf_vtv_assemble_f64 if V4.dtype == torch.float64 else _lib.lib().curv_inf_vtv_assemble
    _lib.check(fn(_lib.stream_ptr(), V4.data_ptr(), sigma.data_ptr(), a, b, out.data_ptr()), "curv_inf_vtv_assemble")
    return out


def diag_scale(src: torch.Tensor, dl: torch.Tensor, dr: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 out[i,j] = src[i,j] dl[i] dr[j]; src float32 or float64, contiguous.  `out` is reused when it is a
    contiguous float32 tensor of the right shape on the right device."""
    if not src.is_cuda or not src.is_contiguous() or src.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("diag_scale: bad source")
    _require_gpu(dl, dr)
    if src.dim() != 2 or dl.numel() != src.shape[0] or dr.numel() != src.shape[1]:
        raise RuntimeError(f"diag_scale: source {tuple(src.shape)} needs dl, dr of {src.shape[0]}, {src.shape[1]} "
                           f"elements, got {dl.numel()}, {dr.numel()}")
    if out is None or out.shape != src.shape or out.dtype != torch.float32 or out.device != src.device \
            or not out.is_contiguous():
        out = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    _lib.check(_lib.lib().curv_diag_scale(_lib.stream_ptr(), src.data_ptr(), int(src.dtype == torch.float64),
                                          out.data_ptr(), dl.data_ptr(), dr.data_ptr(), src.shape[0], src.shape[1]),
               "curv_diag_scale")
    return out


def chol_factor_inverse(mats: Sequence[torch.Tensor], diag_adds: Sequence[float], check: bool = True,
                        rhs: Optional[Sequence[Optional[torch.Tensor]]] = None, rhs_minus: bool = False,
                        pivot_mins: Optional[Sequence[float]] = None) -> List[torch.Tensor]:
    """[chol_lower(M + d I)^-1] in float64 for symmetric float32 or float64 matrices (batched).  `check=False` leaves
    the status words on the device (``chol_factor_inverse.last_info``) for `check_factor_inverse_info`: a caller with
    more launches to enqueue does that first and synchronises once, at its end.  `rhs[i]` (lower triangular, float64):
    entry i of the result is chol_lower(M_i + d_i I)^-1 rhs[i] instead - the forward substitution runs inside the sweep, at
    the cost of the inverse it replaces (with `rhs_minus`: rhs[i] minus that); the right-hand side may be ANOTHER entry's
    result only across calls.  `pivot_mins[i]` > 0: a pivot at or below it counts as failed (the status word then holds the
    number of columns factorised before it, plus one: the numerical rank of a Gram matrix in general position)."""
    n = len(mats)
    arr = (curv_cholinv_desc * n)()
    outs = []
    if pivot_mins is not None:
        for d, pm in zip(arr, pivot_mins):
            d.pivot_min = float(pm)
    for d, M, da in zip(arr, mats, diag_adds):
        if not M.is_cuda or not M.is_contiguous() or M.dtype not in (torch.float32, torch.float64) or M.dim() != 2:
            raise RuntimeError("chol_factor_inverse: contiguous float32 / float64 GPU matrices expected")
        X = torch.empty(M.shape, dtype=torch.float64, device=M.device)
        d.M, d.X, d.n, d.diag_add = M.data_ptr(), X.data_ptr(), M.shape[0], float(da)
        d.m_is_f64 = int(M.dtype == torch.float64)
        R = rhs[len(outs)] if rhs is not None else None
        if R is not None:
            if not R.is_cuda or R.dtype != torch.float64 or R.shape != M.shape or not R.is_contiguous():
                raise RuntimeError("chol_factor_inverse: a right-hand side is a contiguous float64 GPU matrix of M's shape")
            d.R = R.data_ptr()
            d.r_minus = int(bool(rhs_minus))
        outs.append(X)
    dev = mats[0].device
    info = torch.empty(n, dtype=torch.int32, device=dev)
    L = _lib.lib()
    ws = workspace(L.curv_chol_factor_inverse_workspace_bytes(arr, n), dev, "invert")
    _lib.check(L.curv_chol_factor_inverse(_lib.stream_ptr(), arr, n, info.data_ptr(), ws.data_ptr(), ws.numel()),
               "curv_chol_factor_inverse")
    chol_factor_inverse.last_info = info
    if check:
        check_factor_inverse_info(info)
    return outs


def check_factor_inverse_info(info: torch.Tensor) -> None:
    """Raise like `chol_factor_inverse` does when a status word of the batch is non-zero (one host synchronisation)."""
    bad = torch.nonzero(info).flatten().tolist()
    if bad:
        raise RuntimeError(f"cholesky: matrix/matrices {bad} are not positive-definite")


def eigh(mats: Sequence[torch.Tensor], with_values: bool = False, max_sweeps: int = 0, tol: float = 0.0,
         allow_unconverged: bool = False, _project: bool = True):
    """Eigenvectors (columns, ascending eigenvalues) of symmetric float32 matrices, batched block-Jacobi.

    Raises ``RuntimeError`` when the iteration has not converged to `tol` within `max_sweeps` sweeps (default 60 sweeps;
    default tolerance off(A) <= 1e-8 ||A|| for matrices up to 1024 wide and 5e-6 ||A|| above - where the reference's
    fp32 LAPACK delivers 1e-5; an explicit `tol` applies to every matrix; the loop ends at convergence) unless
    `allow_unconverged` is set, in which case the last iterate is returned and ``eigh.converged`` is False."""
    from ._lib import curv_eigh_desc
    if len(mats) == 0:
        return []
    for F in mats:
        _require_gpu(F)
        if F.dim() != 2 or F.shape[0] != F.shape[1]:
            raise RuntimeError("eigh: square matrices expected")
    # Wide, numerically rank-deficient matrices (a KFAC factor with fewer samples than rows) are projected onto their range
    # inside the library (csrc/eigh_lowrank.hip: only the k x k projected problem is iterated on); the others - and every
    # matrix that turns out not to be rank-deficient - take the block-Jacobi iteration on the whole matrix.  `_project=False`
    # asks for the plain iteration.
    n = len(mats)
    arr = (curv_eigh_desc * n)()
    vecs, vals = [], []
    mats = [F if (F.dtype == torch.float32 and F.is_contiguous()) else F.float().contiguous() for F in mats]
    for d, F in zip(arr, mats):
        U = torch.empty_like(F)
        w = torch.empty(F.shape[0], dtype=torch.float32, device=F.device)
        vecs.append(U)
        vals.append(w)
        d.F, d.U, d.w, d.n = F.data_ptr(), U.data_ptr(), w.data_ptr(), F.shape[0]
    L = _lib.lib()
    need = L.curv_syevd_workspace_bytes(arr, n)
    if need == 0:
        raise RuntimeError("eigh: matrix size out of range")
    ws = workspace(need, mats[0].device, "eigh")
    sweeps = ctypes.c_int(0)
    ranks = (ctypes.c_int * n)()
    # (an explicit sweep limit keeps the projection off: max_sweeps = 60 is the plain iteration's own default)
    plain = (not _project) and max_sweeps == 0 and tol <= 0.0
    rc = L.curv_syevd_ex(_lib.stream_ptr(), arr, n, ws.data_ptr(), ws.numel(), 60 if plain else int(max_sweeps), float(tol),
                         ctypes.byref(sweeps), ranks)
    eigh.last_ranks = {i: int(k) for i, k in enumerate(ranks) if k > 0}      # position in `mats` -> rank of the projected problem
    eigh.last_lowrank = len(eigh.last_ranks)
    eigh.last_sweeps = sweeps.value
    eigh.converged = rc == 0
    if not (rc == _lib.ERR_NOT_CONVERGED and allow_unconverged):
        _lib.check(rc, "curv_syevd")
    return (vecs, vals) if with_values else vecs



def kron(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Kronecker product, reference index convention (utils.py:288-310): (ar*br) x (ac*bc)."""
    a, b = a.contiguous(), b.contiguous()
    _require_gpu(a, b)
    if a.dim() != 2 or b.dim() != 2:
        raise RuntimeError("kron: 2-D operands expected")
    out = torch.empty(a.shape[0] * b.shape[0], a.shape[1] * b.shape[1], dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().curv_kron(_lib.stream_ptr(), a.data_ptr(), a.shape[0], a.shape[1], b.data_ptr(),
                                    b.shape[0], b.shape[1], out.data_ptr()), "curv_kron")
    return out


def concat(parts: Sequence[torch.Tensor]) -> torch.Tensor:
    """1-D concatenation of contiguous float32 GPU tensors: one batched copy launch."""
    for t in parts:
        _require_gpu(t)
    total = sum(t.numel() for t in parts)
    out = torch.empty(total, dtype=torch.float32, device=parts[0].device)
    pos, dsts = 0, []
    for t in parts:
        dsts.append(out[pos:pos + t.numel()])
        pos += t.numel()
    CopyPlan(dsts, [t.reshape(-1) for t in parts]).run()
    return out


TRI64_A_LOWER, TRI64_A_UPPER, TRI64_B_LOWER, TRI64_B_UPPER, TRI64_C_LOWER = 1, 2, 4, 8, 16      # CURV_TRI64_*


class Gemm64:
    """float64 C = alpha * A @ B [+ beta * C] on strided 2-D GPU views; C = None allocates the output.
    `tri`: TRI64_* flags for triangular operands (their other triangle must hold zeros; only the K range that can
    contribute to a tile is visited); TRI64_C_LOWER for a square product known to be symmetric (tiles strictly above the
    diagonal of C are not computed and keep what they held)."""
    __slots__ = ("A", "B", "C", "alpha", "beta", "tri", "E", "row_scale", "col_scale", "out32")

    def __init__(self, A, B, C=None, alpha=1.0, beta=0.0, tri=0, E=None, row_scale=None, col_scale=None, out32=None):
        """`E` (float64, shape of C, not C itself): C = alpha A B + beta E.  `out32` (float32, shape of the product): the
        result goes there instead, as float32(alpha * row_scale[i] * col_scale[j] * (A B)[i, j]) - either scale vector
        (float32, length M / N) may be None; no C, beta or E in that form."""
        self.A, self.B, self.C, self.alpha, self.beta, self.tri = A, B, C, float(alpha), float(beta), int(tri)
        self.E, self.row_scale, self.col_scale, self.out32 = E, row_scale, col_scale, out32


def gemm_f64_batched(jobs: Sequence[Gemm64]) -> List[torch.Tensor]:
    """All products through one call of curv_gemm_f64_batched (up to 24 descriptors per launch; the products must be
    independent of each other: large ones run in a launch of their own behind the small ones)."""
    n = len(jobs)
    if n == 0:
        return []
    d = (curv_gemm64_desc * n)()
    outs = []
    for k, j in enumerate(jobs):
        for t in (j.A, j.B):
            if not t.is_cuda or t.dtype != torch.float64 or t.dim() != 2:
                raise RuntimeError("gemm_f64 operands must be 2-D float64 GPU tensors")
        M, K = j.A.shape
        K2, N = j.B.shape
        if K != K2:
            raise RuntimeError("gemm_f64: shape mismatch")
        C = j.C
        if j.out32 is not None:
            o = j.out32
            if not o.is_cuda or o.dtype != torch.float32 or tuple(o.shape) != (M, N) or j.beta != 0.0 or j.E is not None \
                    or C is not None:
                raise RuntimeError("gemm_f64: the float32 output is an (M, N) float32 GPU tensor and takes no C / beta / E")
            for v, length in ((j.row_scale, M), (j.col_scale, N)):
                if v is not None and (not v.is_cuda or v.dtype != torch.float32 or not v.is_contiguous() or v.numel() != length):
                    raise RuntimeError("gemm_f64: scale vectors are contiguous float32 GPU tensors of length M / N")
            outs.append(o)
            d[k].A, d[k].B, d[k].C, d[k].C32 = j.A.data_ptr(), j.B.data_ptr(), None, o.data_ptr()
            d[k].row_scale = j.row_scale.data_ptr() if j.row_scale is not None else None
            d[k].col_scale = j.col_scale.data_ptr() if j.col_scale is not None else None
            d[k].c_rs, d[k].c_cs = o.stride()
        else:
            if C is None:
                if j.beta != 0.0 and j.E is None:
                    raise RuntimeError("gemm_f64: beta needs an existing C (or E)")
                C = torch.empty(M, N, dtype=torch.float64, device=j.A.device)
            elif not C.is_cuda or C.dtype != torch.float64 or tuple(C.shape) != (M, N):
                raise RuntimeError("gemm_f64: bad output tensor")
            if j.E is not None:
                E = j.E
                if not E.is_cuda or E.dtype != torch.float64 or tuple(E.shape) != (M, N) or E.stride() != C.stride() \
                        or E.data_ptr() == C.data_ptr():
                    raise RuntimeError("gemm_f64: E is a float64 GPU tensor with C's shape and strides, not C itself")
                d[k].E = E.data_ptr()
            outs.append(C)
            d[k].A, d[k].B, d[k].C = j.A.data_ptr(), j.B.data_ptr(), C.data_ptr()
            d[k].c_rs, d[k].c_cs = C.stride()
        d[k].a_rs, d[k].a_cs = j.A.stride()
        d[k].b_rs, d[k].b_cs = j.B.stride()
        d[k].M, d[k].N, d[k].K, d[k].alpha, d[k].beta, d[k].tri = M, N, K, j.alpha, j.beta, j.tri
    _lib.check(_lib.lib().curv_gemm_f64_batched(_lib.stream_ptr(), d, n), "curv_gemm_f64_batched")
    return outs


def gemm_f64(A: torch.Tensor, B: torch.Tensor, alpha: float = 1.0, beta: float = 0.0,
             C: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float64 C = alpha * A @ B [+ beta * C] on strided 2-D GPU views."""
    return gemm_f64_batched([Gemm64(A, B, C, alpha, beta)])[0]


LOGSUM_GRID_MAX = _lib.LOGSUM_GRID_MAX
_LOGSUM_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.float64: _lib.DTYPE_F64}


class LogSumSegment(NamedTuple):
    """One segment of `logsum_grid`: a float32 or float64 GPU tensor - a 1-D view with any positive stride (the diagonal of
    a square matrix is ``M.diagonal()``: a stride of width + 1), or a contiguous tensor of any shape - read in place."""
    tensor: torch.Tensor
    weight: float
    gains: Optional[Sequence[float]]       # per pair; None for a segment of squares
    shifts: Optional[Sequence[float]]
    mode: int = _lib.LOGSUM_LOG

    @classmethod
    def of(cls, tensor: torch.Tensor, weight: float, gains: Sequence[float], shifts: Sequence[float]):
        """``weight * sum_e log(gains[h] * max(tensor[e], 0) + shifts[h])`` for every pair h."""
        return cls(tensor, float(weight), [float(g) for g in gains], [float(s) for s in shifts], _lib.LOGSUM_LOG)

    @classmethod
    def squares(cls, tensor: torch.Tensor, weight: float = 1.0):
        """``weight * sum_e tensor[e]**2``, in column 0 of its row (the other columns are 0)."""
        return cls(tensor, float(weight), None, None, _lib.LOGSUM_SQUARES)


def _logsum_extent(name: str, k: int, t: torch.Tensor):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in _LOGSUM_DTYPES:
        raise RuntimeError(f"{name}: segment {k}: a float32 or float64 GPU tensor expected")
    if t.dim() == 1 and (t.numel() <= 1 or t.stride(0) >= 1):
        return t.numel(), (t.stride(0) if t.numel() > 1 else 1)
    if t.is_contiguous():
        return t.numel(), 1
    raise RuntimeError(f"{name}: segment {k}: a 1-D view with a positive stride or a contiguous tensor expected, got shape "
                       f"{tuple(t.shape)} with strides {tuple(t.stride())}")


def logsum_grid(segments: Sequence[LogSumSegment], pairs: int):
    """``(per_segment, total)``: float64 GPU tensors of shape (len(segments), pairs) and (pairs,) with
    ``per_segment[i, h] = weight_i * sum_e log(gains_i[h] * max(x_i[e], 0) + shifts_i[h])`` (a segment of squares:
    ``weight_i * sum_e x_i[e]**2`` in column 0, zeros beside it) and ``total[h]`` the sum of column h over the segments in
    their order.  float64 from the load on, one read of the data for every pair, nothing copied; a fixed reduction order:
    a result has the same bits alone, in a larger batch and on a repeat call (`curv_logsum_grid`).  More
    than `LOGSUM_GRID_MAX` pairs run as chunks of that many."""
    name = "logsum_grid"
    segments, pairs = list(segments), int(pairs)
    if pairs < 1:
        raise ValueError(f"{name}: pairs {pairs} below 1")
    if not segments:
        raise ValueError(f"{name}: no segments")
    extents = [_logsum_extent(name, k, s.tensor) for k, s in enumerate(segments)]
    for k, s in enumerate(segments):
        if s.mode == _lib.LOGSUM_LOG and (len(s.gains) != pairs or len(s.shifts) != pairs):
            raise ValueError(f"{name}: segment {k}: {len(s.gains)} gains and {len(s.shifts)} shifts for {pairs} pairs")
    n, dev = len(segments), segments[0].tensor.device
    out = torch.zeros(n, pairs, dtype=torch.float64, device=dev)
    total = torch.empty(pairs, dtype=torch.float64, device=dev)
    L = _lib.lib()
    arr = (_lib.curv_logsum_desc * n)()
    for d, s, (count, stride) in zip(arr, segments, extents):
        d.x, d.dtype, d.mode = s.tensor.data_ptr() if count else None, _LOGSUM_DTYPES[s.tensor.dtype], s.mode
        d.count, d.stride, d.weight = count, stride, s.weight
    for h0 in range(0, pairs, LOGSUM_GRID_MAX):
        k = min(LOGSUM_GRID_MAX, pairs - h0)
        for d, s, (count, _) in zip(arr, segments, extents):
            if s.mode == _lib.LOGSUM_LOG:
                d.gain[:k], d.shift[:k] = s.gains[h0:h0 + k], s.shifts[h0:h0 + k]
            elif h0 > 0:
                d.count, d.x = 0, None           # the squares went into column 0 with the first chunk
        need = L.curv_logsum_workspace_bytes(arr, n, k)
        if need == 0:
            _lib.check(_lib.ERR_INVALID, "curv_logsum_workspace_bytes")
        ws = workspace(need, dev, "logsum")
        _lib.check(L.curv_logsum_grid(_lib.stream_ptr(), arr, n, k, out.data_ptr() + 8 * h0, pairs,
                                      total.data_ptr() + 8 * h0, ws.data_ptr(), ws.numel()), "curv_logsum_grid")
    return out, total
