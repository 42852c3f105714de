"""MI355X-native estimators behind the reference's plugin API.

Same classes, constructor signatures, method names, public attributes (``state``, ``inv_state``,
``model_state`` ...) and error behaviour as ``curvature/curvatures.py`` of DLR-RM/curvature, so that the
reference's call sequences run unchanged::

    kfac = KFAC(model)
    for images, labels in data:                # scripts/test.py:32-47
        loss = criterion(model(images), sampled_labels); model.zero_grad(); loss.backward()
        kfac.update(batch_size=images.size(0))
    kfac.invert(add=0.5, multiply=1)
    kfac.sample_and_replace()

All arithmetic runs in ``libcurv_hip.so`` (hand-written HIP for gfx950) through the C ABI of
``include/curv_hip.h``; PyTorch only runs the model's forward/backward and owns the tensors.  There is
no CPU fallback: CPU models raise ``RuntimeError``.
"""
import copy
import math
import numbers
from abc import ABC, abstractmethod
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Union

import torch
from torch import Tensor
from torch.nn import Module, Sequential

from . import _lib, ops
from .predictive import LinearisedPredictive, PredictiveTerms

SUPPORTED_LAYERS = ['Linear', 'Conv2d', 'MultiheadAttention']
# selectable by name but not part of the default selection (which stays what the reference selects)
OPTIONAL_LAYERS = ['ConvTranspose2d']
# layer classes whose parameters are a weight matrix (Wm) and an optional bias
_MATRIX_LAYERS = ('Linear', 'Conv2d', 'ConvTranspose2d', 'Conv1d', 'Conv3d', 'LayerNorm', 'GroupNorm', 'BatchNorm2d',
                  'Embedding')
# selectable by name only while `ops.admit_conv_nd` is on
_ND_LAYERS = ('Conv1d', 'Conv3d')
# selectable by name only while `ops.admit_norm_layers` is on: Wm = [weight.reshape(C, 1) | bias], one
# 1 x (1 + has_bias) row per channel, C stacked Kronecker pairs like a depthwise 1x1 convolution
_NORM_LAYERS = ('LayerNorm', 'GroupNorm', 'BatchNorm2d')
_NORM_ADVICE = "KFAC, or Diagonal, with functional_variance take the layer"


def _is_norm(layer) -> bool:
    return layer.__class__.__name__ in _NORM_LAYERS


def _check_norm(model, layer, what: str, takes: bool) -> None:
    """What the estimators represent of a selected normalisation layer (`ops.admit_norm_layers`): a layer with affine
    parameters over more than one channel, for KFAC and Diagonal."""
    kind, name = layer.__class__.__name__, _layer_name(model, layer)
    if not takes:
        raise NotImplementedError(f"{what}: the normalisation layer {name} ({kind}) is not supported; {_NORM_ADVICE}")
    if layer.weight is None:
        raise NotImplementedError(f"{what}: {kind} layer {name} has no weight (elementwise_affine / affine is False): "
                                  f"there is nothing to estimate")
    if layer.weight.numel() < 2:
        raise NotImplementedError(f"{what}: {kind} layer {name} has a single channel, which the stacked factors do not hold")


# selectable by name only while `ops.admit_embedding` is on: Wm = weight itself, (V, D), no bias; its rows are
# the INPUT side (the transpose of the Linear(V, D, bias=False) twin on one-hot rows, whose Wm is weight.T)
_EMBEDDING_ADVICE = "KFAC (approximation=\"expand\"), or Diagonal, with the weight samplers and functional_variance take the layer"


def _is_embedding(layer) -> bool:
    return layer.__class__.__name__ == 'Embedding'


def _bias_of(layer):
    """The layer's bias parameter, None where it has none (an Embedding has no such attribute)."""
    return getattr(layer, 'bias', None)


def _refuse_embedding(model, layer, what: str) -> None:
    raise NotImplementedError(f"{what}: the embedding layer {_layer_name(model, layer)} (Embedding) is not supported; "
                              f"{_EMBEDDING_ADVICE}")


def _check_embedding(model, layer, what: str, takes: bool, selected: Sequence[str], shard) -> None:
    """What the estimators represent of a selected nn.Embedding (`ops.admit_embedding`): a dense lookup of a weight of its
    own with at least two rows, for KFAC and Diagonal on one rank."""
    name = _layer_name(model, layer)
    if not takes:
        _refuse_embedding(model, layer, what)
    why = None
    if layer.max_norm is not None:
        why = f"has max_norm={layer.max_norm}: the forward pass rewrites the weight, so there is no fixed mean to expand around"
    elif layer.sparse:
        why = "has sparse=True: its gradient is a sparse tensor, which the estimators do not read"
    elif layer.scale_grad_by_freq:
        why = "has scale_grad_by_freq=True: the gradient PyTorch forms is not the loss's"
    elif layer.num_embeddings < 2:
        why = "has a single row, which the factors do not hold"
    if why is not None:
        raise NotImplementedError(f"{what}: Embedding layer {name} {why}")
    for other in model.modules():
        if other is layer or other.__class__.__name__ not in selected:
            continue
        if any(p is layer.weight for p in other.parameters(recurse=False)):
            raise NotImplementedError(f"{what}: the weight of Embedding layer {name} is also a parameter of the selected layer "
                                      f"{_layer_name(model, other)} ({other.__class__.__name__}), a tied weight: the curvature "
                                      f"of a shared parameter is the sum of both layers', which neither layer's factors hold")
    _check_embedding_shard(model, layer, what, shard)


def _check_embedding_shard(model, layer, what: str, shard) -> None:
    if shard is not None and shard.world > 1:
        raise NotImplementedError(f"{what}: Embedding layer {_layer_name(model, layer)} under a shard of {shard.world} ranks is "
                                  f"not supported: the shard planner would price a V^3 inversion for its diagonal factor")


def _is_convt(layer) -> bool:
    return layer.__class__.__name__ == 'ConvTranspose2d'


def _check_convt(layer) -> None:
    """What the transposed-convolution estimators represent: groups 1, dilation 1, integer padding."""
    if layer.groups != 1:
        raise NotImplementedError("ConvTranspose2d with groups > 1 is not supported")
    if tuple(layer.dilation) != (1, 1):
        raise NotImplementedError("dilated ConvTranspose2d is not supported")
    if not all(isinstance(p, int) for p in layer.padding):
        raise NotImplementedError("ConvTranspose2d with string padding is not supported")


def _layer_name(model, layer) -> str:
    """The layer's `named_modules()` name in quotes (its repr if the model does not hold it)."""
    return next((f"'{n}'" for n, mod in model.named_modules() if mod is layer), repr(layer))


def _check_conv_nd(model, layer) -> None:
    """What the estimators represent of a selected Conv1d / Conv3d (`ops.admit_conv_nd`): groups 1, integer zero padding,
    no dilation - except a Conv1d with `ops.admit_dilated` on, which is the dilated Conv2d of its (N, C, 1, L) view."""
    kind, name = layer.__class__.__name__, _layer_name(model, layer)
    why = None
    if int(layer.groups) != 1:
        why = f"has groups={layer.groups}; grouped {kind} layers are not supported"
    elif isinstance(layer.padding, str):
        why = f"has string padding ({layer.padding!r}); string padding modes are not supported"
    elif layer.padding_mode != 'zeros':
        why = f"has padding_mode={layer.padding_mode!r}; only zero padding is supported"
    elif any(d != 1 for d in layer.dilation):
        if kind == 'Conv3d':
            why = f"is dilated (dilation {tuple(layer.dilation)}); dilated Conv3d layers are not supported"
        elif not ops.dilated_admitted():
            why = f"is dilated (dilation {tuple(layer.dilation)}); ops.admit_dilated() admits a dilated Conv1d"
    if why is not None:
        raise NotImplementedError(f"{kind} layer {name} {why}")


def _check_dilated(model, layer) -> None:
    """What the A-factor build of a dilated Conv2d represents (`ops.admit_dilated`; curv_kfac_dilated_accumulate): groups 1,
    integer padding, stride 1 and a padding that is a multiple of the dilation - the residue classes of the input grid are
    then undilated convolutions of their own."""
    name = next((f"'{n}'" for n, mod in model.named_modules() if mod is layer), repr(layer))
    if int(layer.groups) != 1:
        raise NotImplementedError(f"KFAC: dilated convolution {name} has groups={layer.groups}; dilation with groups > 1 is "
                                  "not supported")
    if not all(isinstance(p, int) for p in layer.padding):
        raise NotImplementedError(f"KFAC: dilated convolution {name}: string padding modes are not supported")
    if any(s != 1 for s in layer.stride) or any(p % d for p, d in zip(layer.padding, layer.dilation)):
        raise NotImplementedError(
            f"KFAC: dilated convolution {name} (stride {tuple(layer.stride)}, padding {tuple(layer.padding)}, dilation "
            f"{tuple(layer.dilation)}): the A-factor build needs stride 1 and a padding that is a multiple of the dilation; "
            "the per-sample line (Diagonal(per_sample=True), the linearised predictive of Diagonal) does not have this "
            "restriction")


def _wm(layer, t: Tensor) -> Tensor:
    """A tensor shaped like `layer.weight` as the layer matrix Wm (out, in*kh*kw): a view for Linear / Conv2d, a
    contiguous copy of ``t.permute(1, 0, 2, 3)`` for ConvTranspose2d (whose weight is (in, out, kh, kw))."""
    if _is_convt(layer):
        return t.transpose(0, 1).reshape(t.shape[1], -1)
    if _is_norm(layer):
        return t.reshape(-1, 1)
    return t.reshape(t.shape[0], -1)


def _wm_rows(layer) -> int:
    """Rows of the layer matrix Wm: output features / channels."""
    if _is_norm(layer):
        return layer.weight.numel()                      # (a LayerNorm with several normalised dims flattens)
    return layer.weight.shape[1] if _is_convt(layer) else layer.weight.shape[0]


def _check_reduce(model, layer) -> None:
    """The layers ``KFAC(approximation="reduce")`` takes: Linear and Conv2d with groups 1 and dilation 1 (the reduce pass
    of curv_kfac_reduce_accumulate has no grouped or dilated form, whatever `ops.admit_dilated` says; string padding is
    refused as for expand)."""
    kind = layer.__class__.__name__
    why = None
    if kind == 'Conv2d':
        if layer.groups != 1:
            why = f"a grouped convolution (groups={layer.groups})"
        elif tuple(layer.dilation) != (1, 1):
            why = f"a dilated convolution (dilation {tuple(layer.dilation)})"
    elif kind == 'Conv1d':                               # (groups 1 and zero padding: `_check_conv_nd`)
        if any(d != 1 for d in layer.dilation):
            why = f"a dilated convolution (dilation {tuple(layer.dilation)})"
    elif kind == 'Conv3d':
        why = "a 3-D convolution (the reduce pass has no depth window)"
    elif kind == 'ConvTranspose2d':
        why = "a transposed convolution"
    elif kind == 'MultiheadAttention':
        why = "an attention layer (its records are (T, N, E), with the batch second)"
    elif kind in _NORM_LAYERS:
        why = "a normalisation layer"
    elif kind == 'Embedding':
        why = "an embedding layer (its A factor is the diagonal of token counts)"
    if why is not None:
        name = next((f"'{n}'" for n, mod in model.named_modules() if mod is layer), repr(layer))
        raise NotImplementedError(f'KFAC(approximation="reduce"): layer {name} is {why}, which the '
                                  f'reduce build does not take; approximation="expand" takes it')


class HeadTerms(NamedTuple):
    """`Curvature.head_terms`: the logit covariance of input n is ``M diag(d2[n]) M^T``."""
    M: Optional[Tensor]       # (K, K), or None for the identity
    lower: bool               # M is lower triangular
    d2: Tensor                # (N,) - one scalar per input - or (N, K)
    variance: Tensor          # (N, K): the diagonal of the covariance


class HeadGridTerms(NamedTuple):
    """`Curvature.head_terms_grid`: the logit covariance of input n under pair h is ``M diag(d2[h, n]) M^T``."""
    M: Optional[Tensor]       # (K, K), dense, or None for the identity
    d2: Tensor                # (H, N, K)
    variance: Tensor          # (H, N, K): the diagonals of the covariances


class _Slot(NamedTuple):
    """One piece of a layer's parameters as a block of columns of its [W | b] matrix (`_slots`)."""
    cols: slice       # the columns of Wm this piece holds
    view: Tensor      # (rows, len(cols)) view into the parameter storage
    lead: bool        # Wm's leading columns stored as they are: only there a slice of a triangular factor stays triangular


def _slots(layer, weight: Tensor, bias: Optional[Tensor]) -> List[_Slot]:
    """Where the columns of the layer matrix [W | b] (Wm order: (out, in*kh*kw [+1]), the bias last) live in `weight` (shaped
    like `layer.weight`) and `bias` (or None): slots that cover the columns exactly once, in the order the samplers launch
    them.  One slot for the weight of a Linear / Conv2d; one per kernel tap (a, b) for a ConvTranspose2d:
    Wm[:, ci kh kw + a kw + b] = weight[ci, :, a, b], an (out, in) view with strides (kh kw, out kh kw); the bias, if any,
    is the last slot, an (out, 1) view.  A product that writes these views writes Wm through the permutation, with no copy
    pass.  The same map serves the live parameters, their means in `model_state` and one set of a `SampleBank`.  A grouped
    layer takes row blocks of the views: group g owns rows [g m, (g + 1) m)."""
    if _is_convt(layer):
        cin, cout = weight.shape[0], weight.shape[1]
        khw = weight.numel() // (cin * cout)
        n0 = cin * khw
        v = weight.view(cin, cout, khw)
        out = [_Slot(slice(k, n0, khw), v[:, :, k].t(), False) for k in range(khw)]
    else:
        w = weight.view(-1, 1) if _is_norm(layer) else weight.view(weight.shape[0], -1)
        n0 = w.shape[1]
        out = [_Slot(slice(0, n0), w, True)]
    if bias is not None:
        out.append(_Slot(slice(n0, n0 + 1), bias.view(-1, 1), False))
    return out


def _live_slots(layer) -> List[_Slot]:
    """`_slots` of the layer's own parameters (what the fused samplers write)."""
    weight, bias = layer._parameters['weight'], layer._parameters.get('bias')
    return _slots(layer, weight.data, bias.data if bias is not None else None)


def _bank_buffers(layer, count: int, device):
    """(weights, biases or None): buffers for `count` fp32 parameter sets of the layer, set k to be addressed through
    `_slots(layer, weights[k], biases[k])`.  A ConvTranspose2d's sets are held in the weight's own (in, out, kh, kw)
    layout, every other layer's as (out, in*kh*kw)."""
    w = layer.weight
    shape = w.shape if _is_convt(layer) else (_wm_rows(layer), w.numel() // _wm_rows(layer))
    weights = torch.empty(count, *shape, dtype=torch.float32, device=device)
    if _bias_of(layer) is None:
        return weights, None
    return weights, torch.empty(count, _wm_rows(layer), dtype=torch.float32, device=device)


def _largest_first(stage: list) -> None:
    """Sort the products of one launch by M K N, largest first (stable): the tail of the launch is then made of the short
    tiles."""
    stage.sort(key=lambda j: -(j.A.shape[0] * j.A.shape[1] * j.B.shape[1]))


def _run_of(tensors: Sequence[Tensor]) -> Optional[Tensor]:
    """The flat view over `tensors` if they are contiguous fp32 tensors that lie back to back, in this order, inside ONE
    allocation (an elementwise step over all of them is then one launch); None otherwise."""
    if not tensors:
        return None
    pos = tensors[0].data_ptr()
    for t in tensors:
        if not t.is_contiguous() or t.dtype != torch.float32 or t.data_ptr() != pos:
            return None
        pos += 4 * t.numel()
    head, total = tensors[0], (pos - tensors[0].data_ptr()) // 4
    if head.untyped_storage().nbytes() < 4 * (head.storage_offset() + total):
        return None
    return torch.as_strided(head.reshape(-1), (total,), (1,))


class _Arena:
    """One flat fp32 buffer and one view per shape, laid out back to back: whole-model elementwise steps (noise scaling,
    scalar-hyper-parameter inverts) then take ONE launch over `flat` instead of one per layer.  `flat` has at least one
    element, also when there are no views (a layer-sharded rank can own nothing)."""

    def __init__(self, shapes: Sequence[Sequence[int]], device, zero: bool = False):
        sizes = [math.prod(map(int, shape)) for shape in shapes]
        self.total = sum(sizes)
        self.flat = (torch.zeros if zero else torch.empty)(max(self.total, 1), dtype=torch.float32, device=device)
        self.views, pos = [], 0
        for shape, count in zip(shapes, sizes):
            self.views.append(self.flat[pos:pos + count].view(*shape))
            pos += count

    def is_whole(self, tensors: Sequence[Tensor]) -> bool:
        """True if `tensors` are this arena's views, all of them, in order, back to back: one launch over `flat` then
        does what a loop over `tensors` does.  (Checked by address: contiguous fp32 tensors that tile `flat` from its first
        to its last element.)  False for an empty list, also on an arena without views: there is nothing to launch, the
        per-layer loop of the caller is the empty one."""
        run = _run_of(tensors)
        return run is not None and run.data_ptr() == self.flat.data_ptr() and run.numel() == self.total


def _is_scalar(x) -> bool:
    """Python / numpy real scalars (a superset of what the reference accepts)."""
    return isinstance(x, numbers.Real) or (hasattr(x, "ndim") and getattr(x, "ndim") == 0)


class AttentionProjection:
    """One of the two linear maps of an ``nn.MultiheadAttention`` module seen as a Linear layer: ``'attn_in'`` = the packed
    input projection (in_proj_weight (3E, E), in_proj_bias), ``'attn_out'`` = out_proj (E, E).  KFAC / EFB / INF treat
    each as a layer of its own (the reference raises NotImplementedError for these modules, curvatures.py:303-304,
    351-352, 435-436; SURVEY 8f-4 asks for them): state dicts are keyed by these objects, which are created once per
    module (`of`), so that every estimator of a model uses the same keys.  Self-attention only (query, key and value are
    one tensor: the packed projection is then exactly a Linear(E, 3E) applied to every token)."""

    def __init__(self, module: Module, kind: str):
        self.module, self.kind = module, kind

    @staticmethod
    def of(module: Module):
        cached = module.__dict__.get("_curv_projections")
        if cached is None:
            if not getattr(module, "_qkv_same_embed_dim", True) or module.in_proj_weight is None:
                raise NotImplementedError("MultiheadAttention with kdim / vdim different from embed_dim is not supported")
            cached = (AttentionProjection(module, 'attn_in'), AttentionProjection(module, 'attn_out'))
            module.__dict__["_curv_projections"] = cached
        return cached

    @property
    def weight(self):
        return self.module.in_proj_weight if self.kind == 'attn_in' else self.module.out_proj.weight

    @property
    def bias(self):
        return self.module.in_proj_bias if self.kind == 'attn_in' else self.module.out_proj.bias

    @property
    def _parameters(self):
        return {'weight': self.weight, 'bias': self.bias}

    @property
    def in_features(self) -> int:
        return self.weight.shape[1]

    @property
    def out_features(self) -> int:
        return self.weight.shape[0]

    def state_key(self, prefix: str, name: str) -> str:
        """Key of `name` ('weight' / 'bias') in the model's state_dict, `prefix` = qualified name of the module."""
        dot = prefix + "." if prefix else ""
        return dot + ("in_proj_" + name if self.kind == 'attn_in' else "out_proj." + name)

    def __repr__(self):
        return f"AttentionProjection({self.kind}, {self.in_features} -> {self.out_features})"


class _LinearTap:
    """While an ``nn.MultiheadAttention`` forward runs, the module-level name ``torch.nn.functional.linear`` is replaced
    by a wrapper that records, for the module's two projections, the input of the product and (through a tensor hook)
    the gradient of its output - what the forward / backward hooks of an ordinary Linear layer record
    (curvatures.py:306-310).  The attention forward calls F.linear directly (also for out_proj, whose own module hooks
    therefore never fire).  Installed by a forward pre-hook, removed by an always-called forward hook.  Several taps may
    be active at once (two estimators on one model, nested modules): ONE wrapper serves all of them and F.linear is
    restored when the last one leaves."""

    _active: List["_LinearTap"] = []
    _original = None

    def __init__(self, estimator, module: Module):
        self.estimator, self.module = estimator, module

    @staticmethod
    def _dispatch(input, weight, bias=None):
        out = _LinearTap._original(input, weight, bias)
        for tap in list(_LinearTap._active):
            proj_in, proj_out = AttentionProjection.of(tap.module)
            target = proj_in if weight is proj_in.weight else proj_out if weight is proj_out.weight else None
            if target is None and weight.data_ptr() == proj_in.weight.data_ptr() and weight.shape != proj_in.weight.shape:
                raise NotImplementedError("KFAC / EFB / INF support MultiheadAttention for self-attention only (query, key "
                                          "and value must be the same tensor)")
            if target is not None:
                record = tap.estimator.record
                record[target][0] = input
                if out.requires_grad:
                    out.register_hook(lambda grad, r=record, t=target: r[t].__setitem__(1, grad))
        return out

    def install(self, *_):
        import torch.nn.functional as F
        if self in _LinearTap._active:
            return
        if not _LinearTap._active:
            _LinearTap._original = F.linear
            F.linear = _LinearTap._dispatch
        _LinearTap._active.append(self)

    def remove(self, *_):
        import torch.nn.functional as F
        if self in _LinearTap._active:
            _LinearTap._active.remove(self)
            if not _LinearTap._active:
                F.linear = _LinearTap._original
                _LinearTap._original = None


class Curvature(ABC):
    """Base class: layer selection, mean weights, `_replace`, `sample_and_replace`.

    Mirrors curvature/curvatures.py:17-129.  Layers are selected by class NAME in ``model.modules()``
    order; that order is the layer index used by per-layer ``add`` / ``multiply`` lists."""

    # estimators whose reference implementation handles nn.MultiheadAttention (Diagonal only here; the
    # reference's KFAC / EFB raise NotImplementedError for it, curvatures.py:303-304, 435-436)
    _supports_mha = False
    # KFAC / EFB / INF: every selected MultiheadAttention module contributes its two projections as layers of their own
    # (`AttentionProjection`), an extension of the reference (which raises for them)
    _mha_as_projections = False
    # KFAC, Diagonal: the affine parameters of normalisation layers (`ops.admit_norm_layers`)
    _takes_norm = False
    # KFAC, Diagonal: the weight of nn.Embedding layers (`ops.admit_embedding`)
    _takes_embedding = False
    # the `_Arena`s this estimator allocated for its `state` / `inv_state` tensors (None until then): Diagonal and EFB
    # keep the first two, INF the other three (its corrections D, Lambda_lr and r)
    _state_arena = _inv_arena = _corr_arena = _lam_arena = _r_arena = None

    def __init__(self, model: Union[Module, Sequential], layer_types: Union[List[str], str] = None, *,
                 shard=None):
        self.model = model
        self.model_state = copy.deepcopy(model.state_dict())
        self.layer_types = list()
        if isinstance(layer_types, str):
            self.layer_types.append(layer_types)
        elif isinstance(layer_types, list):
            self.layer_types.extend(layer_types if layer_types else SUPPORTED_LAYERS)
        elif layer_types is None:
            self.layer_types.extend(SUPPORTED_LAYERS)
        else:
            raise TypeError
        for _type in self.layer_types:
            assert _type in SUPPORTED_LAYERS or _type in OPTIONAL_LAYERS or \
                (ops.conv_nd_admitted() and _type in _ND_LAYERS) or (ops.norm_layers_admitted() and _type in _NORM_LAYERS) or \
                (ops.embedding_admitted() and _type == 'Embedding')
        if 'ConvTranspose2d' in self.layer_types:
            for layer in model.modules():
                if _is_convt(layer):
                    _check_convt(layer)
        if any(_type in _ND_LAYERS for _type in self.layer_types):
            for layer in model.modules():
                if layer.__class__.__name__ in _ND_LAYERS and layer.__class__.__name__ in self.layer_types:
                    _check_conv_nd(model, layer)
        if any(_type in _NORM_LAYERS for _type in self.layer_types):
            for layer in model.modules():
                if _is_norm(layer) and layer.__class__.__name__ in self.layer_types:
                    _check_norm(model, layer, type(self).__name__, self._takes_norm)
        if 'Embedding' in self.layer_types:
            for layer in model.modules():
                if _is_embedding(layer):
                    _check_embedding(model, layer, type(self).__name__, self._takes_embedding, self.layer_types, shard)
        self.state = dict()
        self.inv_state = dict()
        # optional layer sharding across ranks (curvature_amd.sharding.Shard); None = own every layer.
        # Keyword-only extension of the reference signature; may also be assigned after construction for
        # estimators whose constructor does no per-layer work (Diagonal, KFAC).
        self.shard = shard
        # device-side noise generator of the samplers (Philox4x32): `noise_offset` advances per draw.  The
        # seed is drawn from torch's default generator at the FIRST draw of this instance (the reference
        # draws its noise from that generator, so successive estimators and samples are independent and
        # torch.manual_seed() before sampling is honoured); assign `noise_seed` to pin it.
        self.noise_seed = None
        self.noise_offset = 0
        # the library's internal streams should exist before unrelated ones (RCCL's, a data loader's, eval_bnn's): the
        # estimator constructor is the earliest point at which the device is known (include/curv_hip.h: curv_init_streams)
        first = next(iter(model.parameters()), None)
        if first is not None and first.is_cuda:
            _lib.init_streams(first.device)

    # ------------------------------------------------------------------ helpers
    def _layers(self) -> List[Module]:
        """Selected Linear / Conv2d layers in ``model.modules()`` order (curvatures.py:120-122).  The walk over the
        module tree is done once per estimator (0.1 ms for a ResNet-50, paid by every phase of a step otherwise): the
        forward / backward hooks are registered on the layers found at construction, so layers added to the model
        later are outside the estimator here as they are in the reference."""
        cached = self.__dict__.get("_layers_cache")
        if cached is not None and cached[0] is self.model and cached[1] == tuple(self.layer_types):
            return list(cached[2])
        out = []
        for layer in self.model.modules():
            name = layer.__class__.__name__
            if name in self.layer_types:
                if name in _MATRIX_LAYERS:
                    out.append(layer)
                elif name == 'MultiheadAttention' and self._mha_as_projections:
                    out.extend(AttentionProjection.of(layer))
                elif name == 'MultiheadAttention' and not self._supports_mha:
                    raise NotImplementedError
        self.__dict__["_layers_cache"] = (self.model, tuple(self.layer_types), tuple(out))
        return out

    def _attention(self) -> List[Module]:
        """Selected MultiheadAttention modules in ``model.modules()`` order (Diagonal only)."""
        if 'MultiheadAttention' not in self.layer_types:
            return []
        return [l for l in self.model.modules() if l.__class__.__name__ == 'MultiheadAttention']

    def _owned(self):
        """[(global layer index, layer)] of the layers this rank owns (all of them without a shard)."""
        layers = self._layers()
        if self.shard is None:
            return list(enumerate(layers))
        return [(i, l) for i, l in enumerate(layers) if self.shard.owns(i)]

    def _global_index(self) -> Dict[Any, int]:
        """state key -> position in the reference's ``enumerate(self.state)`` order of an UNSHARDED run:
        first-seen order over ``model.modules()`` of the selected Linear / Conv2d layers (and, for Diagonal,
        the 'attn_in' / 'attn_out' keys).  This is the index of per-layer ``add`` / ``multiply`` lists
        (curvatures.py:184, 360, 444, 515); a rank that holds only its own layers in `state` still looks its
        hyper-parameters up by this global position."""
        order = []
        for layer in self.model.modules():
            name = layer.__class__.__name__
            if name not in self.layer_types:
                continue
            if name in _MATRIX_LAYERS:
                order.append(layer)
            elif name == 'MultiheadAttention' and self._mha_as_projections:
                order.extend(AttentionProjection.of(layer))
            elif name == 'MultiheadAttention' and self._supports_mha:
                order.extend(k for k in ('attn_in', 'attn_out') if k not in order)
        return {k: i for i, k in enumerate(order)}

    def _allgather_sampled(self):
        """Multi-GPU: the single collective of the path, reassembling every layer's sampled parameters.
        Attention modules (Diagonal only) are not part of the layer partition: rank 0 samples them and their
        projection parameters travel in the same all-gather, so that every rank ends with the same weights."""
        if self.shard is not None and (self.shard.world > 1 or self.shard.force_collective):
            entries = [[p.data for p in (l.weight, _bias_of(l)) if p is not None] for l in self._layers()]
            owners = list(self.shard.owner)
            for layer in (self._attention() if self._supports_mha else []):
                entries.append([p.data for p in (layer.in_proj_weight, layer.in_proj_bias, layer.out_proj.weight,
                                                 layer.out_proj.bias) if p is not None])
                owners.append(0)
            self.shard.allgather_params(entries, owners)

    _is_scalar = staticmethod(_is_scalar)

    @staticmethod
    def _hyper(add, multiply, index: int, count: int):
        """(n, s) of layer `index`: lists only when BOTH are non-scalars (curvatures.py:361-365)."""
        if not _is_scalar(add) and not _is_scalar(multiply):
            assert len(add) == len(multiply) == count
            return float(add[index]), float(multiply[index])
        return float(add), float(multiply)

    def _seed(self) -> int:
        if self.noise_seed is None:
            drawn = int(torch.empty((), dtype=torch.int64).random_().item())      # torch's default CPU generator
            rank = self.shard.rank if self.shard is not None else 0
            # ranks of a sharded run replay the same torch seeds (replicated forward/backward): decorrelate them
            self.noise_seed = (drawn + 0x9E3779B97F4A7C15 * rank) & (2 ** 63 - 1)
        return self.noise_seed

    def _randn(self, *shape, device, out: Optional[Tensor] = None) -> Tensor:
        numel = 1
        for s in shape:
            numel *= int(s)
        counter = getattr(self, "_noise_counter", None)
        if counter is not None:
            # stream position on the device (curvature_amd.graph): the same draws as with the host-side offset, but a
            # captured replay advances it too
            return ops.randn(shape, device, self._seed(), out=out, counter=counter)
        out = ops.randn(shape, device, self._seed(), self.noise_offset, out=out)
        self.noise_offset += (numel + 3) // 4
        return out

    def use_device_noise_counter(self, enable: bool = True) -> None:
        """Keep the position of the noise stream in a device word instead of `noise_offset` (needed inside a captured
        HIP graph, where a host-side offset would be frozen).  Switching back reads the word once (a host sync)."""
        counter = getattr(self, "_noise_counter", None)
        if enable and counter is None:
            dev = next(self.model.parameters()).device
            self._seed()
            self._noise_counter = torch.tensor([self.noise_offset], dtype=torch.int64, device=dev)
        elif not enable and counter is not None:
            self.noise_offset = int(counter.item())
            self._noise_counter = None

    def _sample_plans(self) -> dict:
        """Launch plans of sample_and_replace, keyed by the addresses they were described for.  TWO are kept: the
        overlapped inference loop (evaluate.eval_bnn) alternates between two parameter buffer sets."""
        return self.__dict__.setdefault("_sample_plan_cache", {})

    def _keep_plan(self, key, plan) -> None:
        plans = self._sample_plans()
        while len(plans) >= 2:
            plans.pop(next(iter(plans)))
        plans[key] = plan

    def _reload_mean(self, skip: Sequence[Tensor] = ()):
        """``model.load_state_dict(model_state)`` (curvatures.py:119) as one batched copy: a ResNet-50 has
        ~320 state tensors, i.e. ~320 copy launches (3 ms) through torch.  `skip`: live tensors the
        caller overwrites completely right afterwards."""
        live = getattr(self, "_reload_live", None)
        if live is None:
            state = self.model.state_dict(keep_vars=True)
            if list(state.keys()) != list(self.model_state.keys()):
                raise RuntimeError("model structure changed since the estimator was created")
            self._reload_live = live = [(k, v) for k, v in state.items()]
            self._reload_keys = [k for k, _ in live]
            self._reload_tensors = [v for _, v in live]
            self._reload_plans = {}
        if not live or not live[0][1].is_cuda:
            self.model.load_state_dict(self.model_state)     # CPU models: torch plumbing, nothing to batch
            return
        # parameters may have been re-homed (.to(), ...) and model_state may have been reassigned: the plan is keyed on
        # every address (C-level loops: this runs in front of every sample of a BNN loop, with the GPU waiting)
        ptr = Tensor.data_ptr
        ms = self.model_state
        ptrs = tuple(map(ptr, self._reload_tensors))
        means = tuple(map(ptr, [ms[k] for k in self._reload_keys]))
        key = (ptrs, means, tuple(sorted(map(ptr, skip))))
        plan = self._reload_plans.get(key)
        if plan is None:
            while len(self._reload_plans) >= 2:                  # two parameter buffer sets (evaluate.eval_bnn)
                self._reload_plans.pop(next(iter(self._reload_plans)))
            skipped = set(key[2])
            pairs = [(v.data, self.model_state[k]) for k, v in live if v.data_ptr() not in skipped]
            plan = ops.CopyPlan([d for d, _ in pairs], [s_ for _, s_ in pairs])
            self._reload_plans[key] = plan
        plan.run()

    def model_state_of(self, layer: Module, name: str) -> Tensor:
        """The mean (MAP) tensor of `layer.<name>` inside ``model_state``."""
        if not hasattr(self, "_state_keys"):
            self._state_keys = {}
            for prefix, mod in self.model.named_modules():
                for pname, _ in mod.named_parameters(recurse=False):
                    self._state_keys[(mod, pname)] = (prefix + "." if prefix else "") + pname
                if mod.__class__.__name__ == 'MultiheadAttention' and "_curv_projections" in mod.__dict__:
                    for proj in mod.__dict__["_curv_projections"]:
                        for pname in ('weight', 'bias'):
                            self._state_keys[(proj, pname)] = proj.state_key(prefix, pname)
        return self.model_state[self._state_keys[(layer, name)]]

    def _mean_slots(self, layer) -> List[_Slot]:
        """`_slots` of the layer's mean (MAP) parameters inside ``model_state``."""
        return _slots(layer, self.model_state_of(layer, 'weight'),
                      self.model_state_of(layer, 'bias') if _bias_of(layer) is not None else None)

    def _param_ptrs(self, layers, means: bool = True):
        """(params, their addresses, the addresses of their means) of `layers`: the weight and, where there is one, the
        bias of each.  The address tuples are parts of the samplers' plan keys (plain ints: `evaluate._drop_plans_for`
        searches them); built by C-level loops, this runs in front of every sample of a BNN loop.  `means=False`: a
        sampler that does not read the means leaves their addresses out."""
        ptr = Tensor.data_ptr
        params = [p for l in layers for p in (l._parameters['weight'], l._parameters.get('bias')) if p is not None]
        mean = [self.model_state_of(l, nm) for l in layers for nm in ('weight', 'bias')
                if l._parameters.get(nm) is not None] if means else ()
        return params, tuple(map(ptr, params)), tuple(map(ptr, mean))

    # ------------------------------------------------------------------ recording hooks (KFAC; per-sample Diagonal / EFB)
    _per_sample_groups = False       # Diagonal, KFAC: grouped convolutions have a per-sample form (ops.admit_grouped_per_sample)

    def _record_layer(self, layer) -> None:
        """Record `layer`'s input (by reference) and raw grad_output into ``self.record[layer]`` at every pass."""
        self.record[layer] = [None, None]
        if layer.__class__.__name__ == 'BatchNorm2d':
            self.hooks.append(layer.register_forward_pre_hook(self._check_eval))
        self.hooks.append(layer.register_forward_pre_hook(self._save_input))
        self.hooks.append(layer.register_forward_hook(self._hook_output))

    def _check_eval(self, module, input):
        """A recorded BatchNorm2d must normalise with its running statistics: batch statistics couple the samples."""
        if module.training or not module.track_running_stats:
            raise NotImplementedError(
                f"{type(self).__name__}: BatchNorm2d layer {_layer_name(self.model, module)} "
                f"{'is in training mode' if module.training else 'has track_running_stats=False'}: batch statistics couple "
                f"the samples, so the layer has no per-sample Jacobian; call model.eval() before the passes that are recorded")

    def _save_input(self, module, input):
        self.record[module][0] = input[0]            # by reference, like curvatures.py:307

    def _hook_output(self, module, input, output):
        if _is_convt(module):
            # the output size carries the effective output_padding (layer(x, output_size=...) changes it)
            self._out_size[module] = tuple(output.shape[-2:])
        if output.requires_grad:
            output.register_hook(lambda grad, module=module: self._save_output(module, grad))

    def _save_output(self, module, grad_output):
        self.record[module][1] = grad_output         # raw; the reference stores grad * N (curvatures.py:310)

    def _per_sample_layers(self, what: str, advice: str, grouped: bool = False, norm: bool = False,
                           embedding: bool = False) -> List[Module]:
        """The selected layers, in ``modules()`` order, after checking that every one has a per-sample form P_n = g_n X_n^T:
        Linear, and Conv2d with groups 1, dilation 1 (any dilation with `ops.admit_dilated`) and integer padding; a Conv3d
        (selectable with `ops.admit_conv_nd`) with `ops.admit_conv3d_per_sample`; with
        `ops.widen_per_sample` also ConvTranspose2d with groups 1, dilation 1 and integer padding and, for the estimators that treat a MultiheadAttention module as its two projections
        (KFAC, EFB), those two `AttentionProjection`s.  Any other raises NotImplementedError naming it.  `grouped`: the
        caller takes grouped Conv2d layers (`ops.per_sample_route`: as group slices or by the depthwise kernel); they
        pass only with `ops.admit_grouped_per_sample` on, and a caller that does not take them then says who does
        (`stage_output` and `functional_variance_grid` take them with `ops.admit_grouped_joint` on as well)."""
        names = {mod: name for name, mod in self.model.named_modules()}
        wide = ops.per_sample_is_wide()
        groups_on = ops.per_sample_admits_groups()
        layers = []
        for layer in self.model.modules():
            kind = layer.__class__.__name__
            if kind not in self.layer_types:
                continue
            why = None
            if kind == 'Conv3d':                             # groups 1, zero padding, dilation 1 (`_check_conv_nd`)
                if not ops.conv3d_per_sample_admitted():
                    why = "a 3-D convolution: a sample's product sums over the output depths, which the per-sample " \
                          "kernels would square one by one; KFAC, Diagonal, EFB and INF with the weight samplers take it"
            elif kind == 'Conv1d':                           # groups 1, zero padding (`_check_conv_nd`): as a Conv2d
                if any(d != 1 for d in layer.dilation) and not ops.dilated_admitted():
                    why = "dilated convolution"
            elif kind == 'Conv2d' or (kind == 'ConvTranspose2d' and wide):
                if int(layer.groups) != 1 and tuple(layer.dilation) != (1, 1) and kind == 'Conv2d' and \
                        ops.dilated_admitted():
                    why = f"dilated convolution with groups={layer.groups}: ops.admit_dilated covers groups 1 only"
                elif int(layer.groups) != 1 and not (grouped and groups_on and kind == 'Conv2d'):
                    why = f"grouped convolution (groups={layer.groups})"
                    if groups_on and kind == 'Conv2d':
                        why += "; Diagonal(per_sample=True) and the linearised predictive of KFAC and Diagonal take it" \
                            if ops.per_sample_admits_grouped_joint() else \
                            "; Diagonal(per_sample=True) and functional_variance take it"
                elif tuple(layer.dilation) != (1, 1) and not (kind == 'Conv2d' and ops.dilated_admitted()):
                    why = "dilated convolution"
                elif not all(isinstance(p, int) for p in layer.padding):
                    why = "string padding mode"
            elif kind == 'MultiheadAttention' and self._mha_as_projections and wide:
                layers.extend(AttentionProjection.of(layer))
                continue
            elif kind in _NORM_LAYERS and ops.norm_layers_admitted():
                if not norm:                                 # (`norm`: the caller takes `ops.per_sample_route` "norm")
                    why = f"a normalisation layer; {_NORM_ADVICE}"
            elif kind == 'Embedding' and ops.embedding_admitted():
                if not embedding:                            # (the caller takes `ops.per_sample_route` "embedding")
                    why = f"an embedding layer; {_EMBEDDING_ADVICE}"
            elif kind != 'Linear':
                why = kind
            if why is not None:
                raise NotImplementedError(f"{what}: layer '{names.get(layer, '?')}' is not supported ({why}); {advice}")
            layers.append(layer)
        return layers

    def _record_per_sample(self, what: str) -> None:
        """``per_sample=True`` of Diagonal / EFB: check that every selected layer has a per-sample form and register
        KFAC's recording hooks on it (for the projections of an attention module: its tap on F.linear)."""
        self.hooks = list()
        self.record = dict()
        self._out_size = dict()
        for layer in self._per_sample_layers(f"{what}(per_sample=True)", "select other layer types or use per_sample=False",
                                             grouped=self._per_sample_groups, norm=self._takes_norm,
                                             embedding=self._takes_embedding):
            if not isinstance(layer, AttentionProjection):
                self._record_layer(layer)
                continue
            self.record[layer] = [None, None]
            if layer.kind == 'attn_in':                      # once per module
                tap = _LinearTap(self, layer.module)
                self.hooks.append(layer.module.register_forward_pre_hook(tap.install))
                self.hooks.append(layer.module.register_forward_hook(tap.remove, always_call=True))

    def _records_of(self, what: str, layer):
        """(input, grad_output) recorded for `layer` - for an `ops.GroupSlice`, or a grouped layer itself, those of the
        grouped layer, which must be float32 (RuntimeError naming the layer and the dtype otherwise)."""
        module = layer.layer if isinstance(layer, ops.GroupSlice) else layer
        forward, backward = self.record[module]
        if forward is None or backward is None:
            raise RuntimeError(f"{what}.update: no recorded forward/backward pass for a selected layer")
        if _groups_of(module) > 1:
            name = next((f"'{name}'" for name, mod in self.model.named_modules() if mod is module), repr(module))
            for t in (forward, backward):
                fault = ops.grouped_dtype_fault(name, t)
                if fault:
                    raise RuntimeError(fault)
                if not t.is_cuda:
                    raise RuntimeError("curvature_amd runs on MI355X only: got a CPU tensor (no CPU fallback)")
        return forward, backward

    def _per_sample_operands(self, what: str, layers, x_side: bool = True, **layout):
        """The per-sample operands of `layers` from their records, packed where they cannot be read in place:
        [(sides, g tensor, x tensor)] with `sides` the `ops.PerSampleSides` whose strides address the two tensors.  A missing
        record raises like KFAC's; CPU records raise RuntimeError (no fallback), as do records whose dtype the line does
        not take (`ops.per_sample_dtype_fault`).  The packed copies live in shared
        scratch: they are valid until the next per-sample update on this stream.  ``x_side=False``: only the g side is
        packed (the x tensor comes back as None), into scratch of its own, so that the x side of the call before stays
        valid."""
        sides = []
        for layer in layers:
            forward, backward = self._records_of(what, layer)
            for t in (forward, backward):
                fault = ops.per_sample_dtype_fault(f"{what}.update(per_sample=True)", t)
                if fault:
                    raise RuntimeError(fault)
                if not t.is_cuda:
                    raise RuntimeError("curvature_amd runs on MI355X only: got a CPU tensor (no CPU fallback)")
            extra = {}
            if isinstance(layer, AttentionProjection) and layer.kind == 'attn_out':
                # its record is (T N, E): the batch size is that of the module's input projection, recorded as (T, N, E)
                first = self.record.get(AttentionProjection.of(layer.module)[0], (None, None))[0]
                if first is None:
                    raise RuntimeError(f"{what}: the output projection of an attention module takes its batch size from "
                                       "the module's input projection, which has no record (select MultiheadAttention as "
                                       "a whole)")
                if first.dim() != 3:
                    raise RuntimeError(f"{what}: unbatched (T, E) attention input is not supported (the input projection "
                                       f"recorded {tuple(first.shape)}); pass a batch of one")
                extra["samples"] = int(first.shape[1])
            sides.append(ops.per_sample_operands(layer, forward, backward, **layout, **extra))
        flat = [op for s in sides for op in ((s.g, s.x) if x_side else (s.g,))]
        bufs = ops.per_sample_scratch([op.floats for op in flat], flat[0].src.device,
                                      "persample_x" if x_side else "persample_g")
        packed = [(op, buf) for op, buf in zip(flat, bufs) if op.pack is not None]
        ops.per_sample_pack([op for op, _ in packed], [buf for _, buf in packed])
        tensors = [buf if op.pack is not None else op.src for op, buf in zip(flat, bufs)]
        if not x_side:
            return [(s, tensors[k], None) for k, s in enumerate(sides)]
        return [(s, tensors[2 * k], tensors[2 * k + 1]) for k, s in enumerate(sides)]

    @staticmethod
    def _rotated(sides, out: List[Tensor] = None) -> List[Tensor]:
        """R t for every (R, t, rows) of `sides`, t an operand packed as one (rows, N Lp) matrix: into `out`, or fresh
        buffers of t's size; all products in one call."""
        if out is None:
            out = [torch.empty(t.numel(), dtype=torch.float32, device=t.device) for _, t, _ in sides]
        ops.gemm_batched([ops.Gemm(R, t.view(rows, -1), y.view(rows, -1)) for (R, t, rows), y in zip(sides, out)])
        return out

    # ------------------------------------------------------------------ linearised (GLM) predictive: the API (predictive.py)
    def functional_variance(self, out: Tensor, *, first: bool = True, inputs: bool = True) -> Tensor:
        """The variance of a network output under the posterior this estimator samples from, linearised in the weights:
        with P_n the Jacobian of the output for sample n with respect to a layer's [W | b], adds ``sum_layers v_layer[n]``
        into ``out[n]`` (overwrites it when `first`), v_layer[n] the variance of ``<P_n, sample(layer)>``:

            KFAC      ||L_G^T P_n L_A||_F**2
            Diagonal  sum_ij inv_ij**2 P_n[i, j]**2
            EFB       sum_ij inv_ij**2 (U_G^T P_n U_A)[i, j]**2

        P_n = g_n X_n^T comes from the current records: the layer inputs of the last forward pass and the raw grad_outputs
        of the last backward pass, which the caller ran on ``output[:, c].sum()`` for the output c in question (in ``eval()``
        mode, so that the samples of the batch are independent; `evaluate.glm_predictive` drives this).  No weights are
        sampled and no P_n is written (`ops.per_sample_quad_reduce`).  `out`: a length-N float32 GPU view of any stride (a
        column of an (N, classes) matrix).  ``inputs=False`` reuses the X side of the previous call - rotated into the
        posterior's basis once per forward pass, not once per output - like ``KFAC.update(inputs=False)``; it raises
        RuntimeError unless the recorded inputs are the very tensors of that call, and nothing else may have used the
        per-sample scratch in between.  The kept X side (the unfolded inputs of every layer) stays on the estimator (entry
        ``"variance"`` of ``_predictive_kept``) until the next ``inputs=True`` call replaces it or `drop_predictive_state`
        drops it, as `evaluate.glm_predictive` does.  Linear and Conv2d (groups 1, dilation 1, integer padding) with
        float32 GPU records; with `ops.widen_per_sample` also ConvTranspose2d, for KFAC and EFB the two projections of a
        MultiheadAttention module, and bfloat16 / float16 records (a model run under ``torch.autocast``: the pack upcasts
        them, all sums are float32).  With `ops.admit_grouped_per_sample`, for KFAC and Diagonal, also Conv2d with
        ``groups > 1`` (float32 records): one product per group on channel slices of the records, or the direct kernel of
        csrc/persample_dw.hip for a depthwise layer, which keeps no X side - its recorded input is read again
        (`ops.per_sample_route`).  Other selected layers raise NotImplementedError, as does a layer-sharded estimator.
        Implemented by KFAC, Diagonal and EFB, and by INF with `ops.admit_inf_predictive` (see `INF`).  No counterpart in the
        reference, which has the Monte-Carlo predictive only."""
        opted = self._opt_in_predictive()
        if opted is not None:
            return opted.functional_variance(out, first=first, inputs=inputs)
        raise NotImplementedError(f"{type(self).__name__}.functional_variance: no linearised predictive for this estimator "
                                  "(KFAC, Diagonal and EFB have one)")

    def functional_variance_grid(self, out: Tensor, hypers, *, first: bool = True, inputs: bool = True) -> Tensor:
        """`functional_variance` for a whole list of damping pairs at once, without an inversion: row h of `out` receives
        (`first`: is overwritten with) what ``invert(*hypers[h])`` followed by `functional_variance` would give.  In the
        posterior's eigenbasis the damping enters a layer's share only through the weights of the squared entries of
        Q_n = U_G^T P_n U_A (Diagonal: P_n itself), with rho = add / multiply:

            KFAC      (1 / multiply) sum_ij Q_ij**2 / ((lambda_G,i + sqrt(rho)) (lambda_A,j + sqrt(rho)))
            Diagonal  (1 / multiply) sum_ij P_ij**2 / (state_ij + rho)
            EFB       (1 / multiply) sum_ij Q_ij**2 / (state_ij + rho)

        so one backward pass, one rotation and one pass over the per-sample products per output serve every pair
        (`ops.per_sample_quad_grid_reduce`).  `hypers`: a sequence of ``(add, multiply)``, each a pair of scalars or a pair of
        per-layer lists, resolved per layer exactly as `invert` resolves them; every value finite and > 0 (ValueError naming
        the pair).  `out`: a contiguous ``(len(hypers), N)`` float32 GPU tensor.  More than `ops.PERSAMPLE_GRID_MAX` pairs
        run as chunks of that many over the same operands.  Needs `state` only, not `inv_state`; KFAC needs
        `KFAC.decompose()` after its last `update()`.  Records, layers, ``inputs=False`` (the kept X side is entry
        ``"grid"`` of ``_predictive_kept``; `evaluate.glm_predictive_grid` drops it) and the refusal of a layer-sharded
        estimator as for `functional_variance` - except that a grouped Conv2d needs `ops.admit_grouped_joint` beside
        `ops.admit_grouped_per_sample` (KFAC, Diagonal): its group slices then are layers with their group's spectra, and a
        depthwise layer takes `ops.per_sample_dw_quad_grid_reduce` on its records.  Implemented by KFAC, Diagonal and EFB."""
        opted = self._opt_in_predictive()
        if opted is not None:
            return opted.functional_variance_grid(out, hypers, first=first, inputs=inputs)
        raise NotImplementedError(f"{type(self).__name__}.functional_variance_grid: no linearised predictive for this "
                                  "estimator (KFAC, Diagonal and EFB have one)")

    def stage_output(self, slot: int, count: int, *, inputs: bool = False) -> None:
        """One output of `functional_covariance`: the caller has just back-propagated ``output[:, c].sum()`` (in ``eval()``
        mode, as for `functional_variance`); the g side of every layer from the current records - packed, and rotated by
        L_G^T (KFAC) or U_G^T (EFB) - goes into slot `slot` of a stack of `count` slots (scratch of its own: `count` x the
        packed g side of the model).  ``inputs=True``, once per forward pass and before the other slots: also the X side
        and the squared weights, exactly as ``functional_variance(inputs=True)`` works them out, and a fresh stack (no slot
        staged).  The stack and the X side stay on the estimator (entry ``"covariance"`` of ``_predictive_kept``) until the
        next ``inputs=True`` call replaces them (`evaluate.glm_predictive_joint` drops them); nothing else may use the
        per-sample scratch in between.  RuntimeError without ``inputs=True`` on these very recorded inputs (tensor and version) and `count`
        before.  Layers, records and estimators as for `functional_variance` - except that a grouped Conv2d needs
        `ops.admit_grouped_joint` beside `ops.admit_grouped_per_sample` (KFAC, Diagonal).  Its group slices then are layers
        (those that read the record in place share one copy of it per slot); a depthwise layer has no g side to stage:
        its transformed products ``s w (T^T p)`` (`ops.per_sample_dw_project`) go into slot `slot` of a (count, N, C n_g)
        stack kept beside the others, and nothing of its X is kept."""
        opted = self._opt_in_predictive()
        if opted is not None:
            return opted.stage_output(slot, count, inputs=inputs)
        raise NotImplementedError(f"{type(self).__name__}.stage_output: no linearised predictive for this estimator "
                                  "(KFAC, Diagonal and EFB have one)")

    def functional_covariance(self, out: Tensor, *, first: bool = True) -> Tensor:
        """The joint covariance of the `count` staged outputs (`stage_output`) under the posterior this estimator samples
        from, linearised in the weights: adds ``sum_layers <T(P_{n,c}), T(P_{n,c'})>`` into ``out[n, c, c']`` (overwrites
        it when `first`), with P_{n,c} the Jacobian of output c for sample n with respect to a layer's [W | b] and T the
        map whose squared norm `functional_variance` sums (L_G^T P L_A, inv * P, inv * (U_G^T P U_A)).  `out`: a contiguous
        (N, count, count) float32 GPU tensor; both triangles are written and are bit-for-bit symmetric; its diagonal is
        what `functional_variance` gives for each output.  One pass over the products (`ops.per_sample_cov_reduce`): the X
        side of a layer is staged once for all outputs, no P is written (a depthwise layer: the Gram of its staged rows,
        `ops.per_sample_gram_reduce`).  RuntimeError if a slot has not been staged since
        the last ``stage_output(inputs=True)`` or the recorded inputs are no longer those tensors.  At most
        `ops.PERSAMPLE_COV_MAX_OUTPUTS` outputs.  Implemented by KFAC, Diagonal and EFB."""
        opted = self._opt_in_predictive()
        if opted is not None:
            return opted.functional_covariance(out, first=first)
        raise NotImplementedError(f"{type(self).__name__}.functional_covariance: no linearised predictive for this "
                                  "estimator (KFAC, Diagonal and EFB have one)")

    # ------------------------------------------------------------------ last-layer predictive
    def head_terms(self, layer: Module, features: Tensor) -> "HeadTerms":
        """The covariance of ALL logits of a `Linear` head under this estimator's posterior over that layer alone, in
        closed form: the Jacobian of logit c with respect to the head's [W | b] is ``e_c phi~^T`` (phi~ the head's input,
        with a one appended where it has a bias), so ``Sigma_n = M diag(d2_n) M^T`` with one (K, K) matrix `M` for the
        whole batch - KFAC: L_G (`lower`), d2 (N,) = ``||L_A^T phi~_n||^2``; EFB: U_G, d2 (N, K); Diagonal: None (the
        identity), d2 (N, K).  Returns ``HeadTerms(M, lower, d2, variance)`` with `variance` (N, K) the diagonal of
        Sigma_n: what `evaluate.last_layer_predictive` hands to the probit softmax or, with `M` and `d2`, to
        `ops.head_mc`.  `features`: the (N, in) input of the head, float32 / bfloat16 / float16 on the GPU (upcast).  No
        backward pass and no limit on the number of outputs; a few skinny products (`ops.gemm_batched`, `ops.mul`,
        `ops.mul2d`).  Implemented by KFAC, EFB and Diagonal for a `Linear` layer held in `inv_state`; everything else -
        INF, BlockDiagonal, a layer-sharded estimator, an attention projection, another layer type, stacked factors -
        raises NotImplementedError naming the layer and the estimator."""
        what, phi = self._head_input("head_terms", layer, features, "inv_state")
        return self._head_terms(layer, phi, what)

    def _head_input(self, method: str, layer, features, held: str, check=None):
        """(what, phi~): the refusals `head_terms` and `head_terms_grid` share, decided before the device is touched, then
        the head's input as float32 with a one appended where it has a bias.  `held`: the dict that must hold the layer;
        ``check(layer, what)``: the estimator's own refusals, made before the features are looked at."""
        kind = type(self).__name__
        name = _layer_name(self.model, layer) if isinstance(layer, Module) else repr(layer)
        what = f"{kind}.{method}: layer {name}"
        if type(self)._head_terms is Curvature._head_terms:
            raise NotImplementedError(f"{what}: no closed-form last-layer predictive for {kind} (KFAC, EFB and Diagonal "
                                      "have one)")
        if self.shard is not None and self.shard.world > 1:
            raise NotImplementedError(f"{what}: not available on a layer-sharded {kind} (world {self.shard.world})")
        if isinstance(layer, AttentionProjection):
            raise NotImplementedError(f"{what}: an attention projection of {kind} is no classification head")
        if not isinstance(layer, torch.nn.Linear):
            raise NotImplementedError(f"{what}: {kind} takes an nn.Linear head, got {layer.__class__.__name__}")
        if held == "inv_state":
            assert self.inv_state, "Inverse state dict is empty. Did you call 'invert' prior to this?"
            if layer not in self.inv_state:
                raise NotImplementedError(f"{what}: {kind} holds no inverse state for this layer")
        else:
            assert self.state, "State dict is empty. Did you call 'update' prior to this?"
            if layer not in self.state:
                raise NotImplementedError(f"{what}: {kind} holds no state for this layer")
        if check is not None:
            check(layer, what)
        n = layer.in_features + (layer.bias is not None)
        if not isinstance(features, Tensor) or not features.is_cuda:
            raise RuntimeError(f"curvature_amd runs on MI355X only: {what} got CPU features (no CPU fallback)")
        if features.dim() != 2 or features.shape[1] != layer.in_features:
            raise RuntimeError(f"{what}: features must be (N, {layer.in_features}), got {tuple(features.shape)}")
        phi = torch.empty(features.shape[0], n, dtype=torch.float32, device=features.device)
        phi[:, :layer.in_features] = features.float()
        if layer.bias is not None:
            phi[:, layer.in_features:] = 1.0                 # (Wm order: the bias is the last column)
        return what, phi

    def _head_terms(self, layer, phi: Tensor, what: str) -> "HeadTerms":
        raise NotImplementedError

    def head_terms_grid(self, layer: Module, features: Tensor, hypers) -> "HeadGridTerms":
        """`head_terms` for a whole list of damping pairs ``hypers = [(add, multiply), ...]`` at once and without an
        inversion: ``HeadGridTerms(M, d2, variance)`` with ONE (K, K) matrix `M` for every pair and input
        (KFAC, EFB: U_G, dense; Diagonal: None, the identity), `d2` (H, N, K) and `variance` (H, N, K) - the logit
        covariance of input n under pair h is ``M diag(d2[h, n]) M^T``, what ``invert(*hypers[h])`` followed by
        `head_terms` stands for.  In the posterior's eigenbasis the damping enters only the weights of the squared rotated
        features, so the rotation ``Y = Phi~ U_A`` and one read of the spectrum serve every pair (`ops.head_grid`):

            KFAC      d2[h, n, j] = (1 / s_h) / (lambda_G,j + sqrt(rho_h)) * sum_i Y[n, i]^2 / (lambda_A,i + sqrt(rho_h))
            EFB       d2[h, n, j] = (1 / s_h) sum_i Y[n, i]^2 / (state[j, i] + rho_h)
            Diagonal  the same with Y = Phi~

        with ``rho_h = n_h / s_h`` and (n_h, s_h) the pair resolved for this layer as `invert` resolves it (per-layer lists
        work) - the conventions of `functional_variance_grid`, KFAC with the reference's factored damping.  KFAC needs
        `decompose()` after the last `update()` (RuntimeError otherwise).  The layer must be in `state`; `inv_state` is
        neither needed nor touched.  More than `ops.HEAD_GRID_MAX` pairs run as chunks over the same `Y`, bit-equal to the
        concatenation.  `variance` is one `ops.gemm_batched` of the (H N, K) view of `d2` against ``(M o M)^T``.  `features`
        and the refusals as for `head_terms`; every pair finite and > 0 (ValueError naming the pair)."""
        hypers = self._evidence_pairs("head_terms_grid", hypers)
        what, phi = self._head_input("head_terms_grid", layer, features, "state", self._head_grid_check)
        M, Y, (u, v, T), separable = self._head_grid_terms(layer, phi)
        points = dict(self._resolved(hypers))[layer]
        rhos = [n / s for n, s in points]
        shifts, gains = [math.sqrt(r) for r in rhos] if separable else rhos, [1.0 / s for _, s in points]
        H, N, K = len(hypers), phi.shape[0], layer.out_features
        d2 = torch.empty(H, N, K, dtype=torch.float32, device=phi.device)
        for h0 in range(0, H, ops.HEAD_GRID_MAX):
            h1 = min(h0 + ops.HEAD_GRID_MAX, H)
            ops.head_grid([ops.HeadGridJob(Y, u, v, T, d2[h0:h1], shifts[h0:h1], gains[h0:h1])])
        if M is None:
            return HeadGridTerms(None, d2, d2)
        variance = torch.empty(H, N, K, dtype=torch.float32, device=phi.device)
        ops.gemm_batched([ops.Gemm(d2.view(H * N, K), ops.mul2d(M, M).t(), variance.view(H * N, K))])
        return HeadGridTerms(M, d2, variance)

    def _head_grid_check(self, layer, what: str) -> None:
        """What `head_terms_grid` needs of this layer's `state` beyond its presence, or the refusal."""
        raise NotImplementedError

    def _head_grid_terms(self, layer, phi: Tensor):
        """(M, Y, (u, v, T), separable) of `head_terms_grid`, after `_head_grid_check`."""
        raise NotImplementedError

    @staticmethod
    def _row_sums(rows: Tensor, tri: int = ops.TRI_NONE) -> Tensor:
        """(R,) sums over the columns of the (R, C) view `rows`: a product with a column of ones (`_sum_layers`)."""
        ones = torch.ones(rows.shape[1], 1, dtype=torch.float32, device=rows.device)
        out = torch.empty(rows.shape[0], 1, dtype=torch.float32, device=rows.device)
        ops.gemm_batched([ops.Gemm(rows, ones, out, tri=tri)])
        return out.view(-1)

    def _opt_in_predictive(self):
        """The object that answers the four methods above for an estimator whose linearised predictive is behind a switch
        of `ops` (INF), or None: they then refuse.  Called on the class's method only - an estimator without any attribute
        still gets the refusal."""
        return None

    def drop_predictive_state(self) -> None:
        """Forget what the four methods above kept of the last forward pass for their next call (the X sides, the stack of
        staged outputs: ``_predictive_kept``).  Nothing to do for an estimator that keeps nothing."""
        self.__dict__.pop("_predictive_kept", None)

    # ------------------------------------------------------------------ Laplace evidence
    def _evidence_pairs(self, method: str, hypers) -> list:
        """`hypers` checked as `LinearisedPredictive._grid_points` checks them, before anything touches the device."""
        what = f"{type(self).__name__}.{method}"
        hypers = list(hypers)
        if not hypers:
            raise ValueError(f"{what}: no damping pairs")
        for h, pair in enumerate(hypers):
            if not isinstance(pair, (tuple, list)) or len(pair) != 2:
                raise ValueError(f"{what}: pair {h} is not an (add, multiply) pair: {pair!r}")
            for value in pair:
                values = [value] if _is_scalar(value) else list(value)
                if not values or not all(math.isfinite(float(x)) and float(x) > 0 for x in values):
                    raise ValueError(f"{what}: pair {h} {tuple(pair)!r}: add and multiply must be finite and > 0")
        return hypers

    def _resolved(self, hypers) -> list:
        """[(state key, [(n, s) of every pair])] for the entries of `state`, resolved as `invert` resolves them."""
        gindex = self._global_index()
        count = max(len(gindex), len(self.state))
        return [(key, [self._hyper(add, multiply, gindex.get(key, position), count) for add, multiply in hypers])
                for position, key in enumerate(self.state)]

    def _spectrum_log_det(self, hypers, spectra):
        """(rows, total) of `_log_det_parts` for Pi = s diag(x+) + n I in the basis `spectra[key]` holds the x of."""
        segments = [ops.LogSumSegment.of(spectra[key], 1.0, [s for _, s in points], [n for n, _ in points])
                    for key, points in self._resolved(hypers)]
        return ops.logsum_grid(segments, len(hypers))

    def _log_det_parts(self, hypers):
        """(rows (L, H), total (H,)): float64 GPU tensors, log det Pi_l(n_lh, s_lh) per entry of `state` and their sum."""
        raise NotImplementedError(f"{type(self).__name__}.log_det_grid: not implemented for this estimator")

    def log_det_grid(self, hypers, *, per_layer: bool = False) -> Tensor:
        """``sum_l log det Pi_l(n_l, s_l)`` of the regularised precision that ``invert(add, multiply)`` stands for, for every
        pair of ``hypers = [(add, multiply), ...]`` at once and without an inversion: a float64 GPU tensor of shape (H,), or
        (L, H) - one row per entry of `state`, in its order - with `per_layer`.  Each pair holds scalars or per-layer lists,
        resolved per layer as `invert` resolves them; every value finite and > 0 (ValueError naming the pair).  With
        x+ = max(x, 0), as `invert` and `decompose` clamp:

            Diagonal, EFB   Pi = s diag(state+) + n I (EFB: in the U_A (x) U_G basis): sum_e log(s state[e]+ + n)
            KFAC            the reference's factored damping, Pi = (sqrt(s) A + sqrt(n) I) (x) (sqrt(s) G + sqrt(n) I):
                            dim(G) sum_i log(sqrt(s) lambda_A,i + sqrt(n)) + dim(A) sum_j log(sqrt(s) lambda_G,j + sqrt(n))
                            from `decompose()` (needed after the last `update()`); stacked decompositions of grouped
                            layers sum over their groups.  Because of the factored damping this is an approximation of the
                            log-determinant under the prior N(0, I / n), exact where A or G is a multiple of I
            BlockDiagonal   Pi = s F + n I: the eigenvalues of `state` by one batched `ops.eigh`, clamped at 0 and kept
                            until the next `update()`, then as Diagonal
            INF             Pi = V diag(s lambda) V^T + diag(s corr+ + n):
                            sum_e log(s corr[e]+ + n) - 2 sum_k log diag(B^-1)_k, B = chol(vtv + I): one factorisation
                            sweep per pair for all layers, on scratch - `state`, `inv_state` and what `invert` keeps for
                            the sampler are untouched; needs neither `invert` nor `ops.admit_inf_predictive`

        `multiply` is the data-set size in the reference's convention (the curvature is accumulated as a mean).  The whole
        model goes through one `ops.logsum_grid` call per `ops.LOGSUM_GRID_MAX` pairs: one read of the float32 state,
        float64 from the load on, a fixed summation order (the same bits for the same pair in any list).  Nothing in
        `state` or `inv_state` is written.  On a layer-sharded estimator the result covers the owned layers: the caller
        all-reduces."""
        hypers = self._evidence_pairs("log_det_grid", hypers)
        assert self.state, "State dict is empty. Did you call 'update' prior to this?"
        rows, total = self._log_det_parts(hypers)
        return rows if per_layer else total

    def log_prior_grid(self, hypers) -> Tensor:
        """The prior's share of the Laplace evidence for every pair of `hypers` (as for `log_det_grid`): a float64 GPU
        tensor (H,) of ``-1/2 sum_l n_l ||theta_l||^2 + 1/2 sum_l P_l log n_l`` over the layers of `state`, theta_l the
        MAP [W | b] of layer l - read from ``model_state`` (`_mean_slots`), so a model that currently holds a sample gives
        the same value - and P_l its parameter count (the 2 pi terms cancel against the log-determinant's).  The squared
        norms are one `ops.logsum_grid` call.  On a layer-sharded estimator the owned layers only: the caller all-reduces."""
        hypers = self._evidence_pairs("log_prior_grid", hypers)
        assert self.state, "State dict is empty. Did you call 'update' prior to this?"
        resolved = self._resolved(hypers)
        segments, first, biased, second, counts, dropped = [], [], [], [], [], []
        for k, (key, _) in enumerate(resolved):
            if isinstance(key, str):
                raise NotImplementedError(f"{type(self).__name__}.log_prior_grid: the attention entry {key!r} of `state` has "
                                          "no [W | b] matrix")
            views = [slot.view for slot in self._mean_slots(key)]
            if not all(v.is_contiguous() for v in views):
                # (the tap views of a ConvTranspose2d: together they are its weight tensor, which is read whole)
                views = [self.model_state_of(key, 'weight')] + \
                    ([self.model_state_of(key, 'bias')] if _bias_of(key) is not None else [])
            weight, rest = views[0], views[1:]
            first.append(len(segments))
            segments.append(ops.LogSumSegment.squares(weight))
            if rest:
                biased.append(k)
                second.append(len(segments))
                segments.append(ops.LogSumSegment.squares(rest[0]))
            counts.append(sum(v.numel() for v in views))
            if ops.is_embedding_layer(key) and key.padding_idx is not None:
                # the padding row is no parameter: its squares and its D entries are taken out again
                dropped.append((k, len(segments)))
                segments.append(ops.LogSumSegment.squares(weight[key.padding_idx:key.padding_idx + 1]))
                counts[-1] -= key.embedding_dim
        out, _ = ops.logsum_grid(segments, 1)
        dev = out.device
        squares = out[torch.tensor(first, device=dev), 0]
        for k, at in dropped:
            squares[k] -= out[at, 0]
        if biased:
            squares[torch.tensor(biased, device=dev)] += out[torch.tensor(second, device=dev), 0]
        precisions = torch.tensor([[n for n, _ in points] for _, points in resolved], dtype=torch.float64, device=dev)
        prior = torch.tensor([0.5 * math.fsum(P * math.log(points[h][0]) for P, (_, points) in zip(counts, resolved))
                              for h in range(len(hypers))], dtype=torch.float64, device=dev)
        for k in range(len(resolved)):             # layer by layer, elementwise in h: the same bits for a pair in any list
            prior.addcmul_(precisions[k], squares[k], value=-0.5)
        return prior

    @staticmethod
    def _replace(sample: Tensor, weight: Tensor, bias: Tensor = None):
        """weight += sample[:, :-1], bias += sample[:, -1] (curvatures.py:67-82)."""
        if bias is not None:
            bias_sample = sample[:, -1].contiguous().view(*bias.shape)
            bias.data.add_(bias_sample)
            sample = sample[:, :-1]
        weight.data.add_(sample.contiguous().view(*weight.shape))

    # ------------------------------------------------------------------ plugin API
    @abstractmethod
    def update(self, *args: Any, **kwargs: Any):
        raise NotImplementedError

    @abstractmethod
    def invert(self, add: Union[float, list, tuple] = 0., multiply: Union[float, list, tuple] = 1.):
        raise NotImplementedError

    @abstractmethod
    def sample(self, layer: Module) -> Tensor:
        raise NotImplementedError

    def sample_many(self, count: int) -> "SampleBank":
        """`count` sampled parameter sets of the estimator's own layers as a `SampleBank` (see `KFAC.sample_many`, which
        produces them in two launches; this generic form runs `sample_and_replace` `count` times and files the
        parameters away, so that `evaluate.eval_bnn(samples_per_launch=...)` works with every estimator)."""
        S = int(count)
        assert S >= 1
        owned = [l for _, l in self._owned() if getattr(l, "weight", None) is not None]
        # every parameter sample_and_replace modifies goes into the bank: Diagonal also samples the projections of the
        # selected nn.MultiheadAttention modules (string keys, outside `_layers()`); left out, `replace_from` would reset
        # them to their means
        for mha in (self._attention() if self._supports_mha else []):
            owned += AttentionProjection.of(mha)
        weights = {l: torch.empty(S, *l.weight.shape, dtype=l.weight.dtype, device=l.weight.device) for l in owned}
        biases = {l: (torch.empty(S, *l.bias.shape, dtype=l.bias.dtype, device=l.bias.device) if _bias_of(l) is not None else None)
                  for l in owned}
        gather, self._allgather_sampled = self._allgather_sampled, (lambda: None)     # the sets travel when they are loaded
        try:
            for k in range(S):
                self.sample_and_replace()
                for l in owned:
                    weights[l][k].copy_(l.weight.data)
                    if biases[l] is not None:
                        biases[l][k].copy_(l.bias.data)
        finally:
            self._allgather_sampled = gather
        return SampleBank(S, weights, biases)

    def replace_from(self, bank: "SampleBank", index: int) -> None:
        """Load parameter set `index` of a `sample_many` bank into the model (the other state tensors go back to their
        means; under a layer shard the sets of all ranks are all-gathered as in `sample_and_replace`)."""
        if not 0 <= index < bank.count:
            raise IndexError("replace_from: sample index out of range")
        plans = bank.__dict__.setdefault("_copy_plans", {})
        layers = list(bank.weights.keys())
        params = [p for l in layers for p in (l._parameters['weight'], l._parameters.get('bias')) if p is not None]
        key = (index, tuple(map(Tensor.data_ptr, params)))
        plan = plans.get(key)
        if plan is None:
            sets = [t[index] for l in layers for t in (bank.weights[l], bank.biases[l]) if t is not None]   # like `params`
            plan = plans[key] = ops.CopyPlan([p.data for p in params], [t.view(p.shape) for p, t in zip(params, sets)])
        plan.run()
        self._reload_mean(skip=params)
        self._allgather_sampled()

    @staticmethod
    def _replace_layer(sample: Tensor, layer) -> None:
        """`_replace` of an (out, in*kh*kw [+1]) sample in Wm order, for every kind of layer (a ConvTranspose2d weight
        takes it permuted)."""
        for slot in _live_slots(layer):
            slot.view.add_(sample[:, slot.cols])

    def sample_and_replace(self):
        """Reset to the mean weights, then add one posterior sample per selected layer (curvatures.py:117-129)."""
        self._reload_mean()
        for _, layer in self._owned():
            _sample = self.sample(layer)
            self._replace_layer(_sample, layer)
        self._allgather_sampled()


class Diagonal(LinearisedPredictive, Curvature):
    """Diagonal Fisher: state += grad**2 * batch_size (curvatures.py:132-193).

    ``nn.MultiheadAttention`` modules are handled as in the reference (:159-174, 125-129): their input and
    output projections accumulate under the string keys ``'attn_in'`` / ``'attn_out'`` (ONE pair of keys for
    the whole model, as in the reference).  With a layer shard every rank owns a disjoint set of the
    Linear / Conv2d layers; the attention entries are small: every rank accumulates and inverts them, rank 0
    draws their sample and the all-gather of `sample_and_replace` distributes it (each rank has its own noise
    stream, so sampling them everywhere would leave the ranks with different attention weights)."""

    _supports_mha = True
    _per_sample_groups = True
    _takes_norm = True
    _takes_embedding = True

    def __init__(self, model: Union[Module, Sequential], layer_types: Union[List[str], str] = None, *, shard=None,
                 per_sample: bool = False):
        """`per_sample` (keyword-only extension, default off: nothing changes): the exact Fisher diagonal at any batch
        size.  ``update(batch_size)`` then accumulates ``batch_size * sum_n P_n**2`` with P_n = g_n X_n^T the share of
        sample n (index of the leading dimension) in [W.grad | b.grad], from the layer inputs and raw grad_outputs that
        KFAC's hooks record, instead of ``batch_size * (sum_n P_n)**2`` from ``.grad`` - the two agree at batch size 1.
        The P_n are those of the BATCH pass: a BatchNorm layer in training mode couples the samples of a batch, and the
        per-sample quantities are defined from that pass's records, not from N separate passes.  Linear and Conv2d
        (groups 1, dilation 1, integer padding) with float32 records; any other selected layer raises
        NotImplementedError here.  `ops.widen_per_sample` adds ConvTranspose2d and bfloat16 / float16 records
        (MultiheadAttention stays refused: the state for it here is not one matrix per projection);
        `ops.admit_grouped_per_sample` adds Conv2d with ``groups > 1`` (float32 records; `ops.per_sample_route`)."""
        super().__init__(model, layer_types, shard=shard)
        self.per_sample = bool(per_sample)
        if self.per_sample:
            self._record_per_sample("Diagonal")

    def _update_per_sample(self, batch_size):
        layers = [l for _, l in self._owned()]
        if not layers:
            return
        # a grouped layer (ops.admit_grouped_per_sample) enters as its group slices - products of their own into row
        # blocks of the layer's state - or, a true depthwise one, through the direct kernel
        direct = [l for l in layers if ops.per_sample_route(l) == "depthwise"]
        normed = [l for l in layers if ops.per_sample_route(l) == "norm"]
        embedded = [l for l in layers if ops.per_sample_route(l) == "embedding"]
        for l in embedded:
            _check_embedding_shard(self.model, l, "Diagonal.update", self.shard)
        fused = direct + normed + embedded
        items = ops.per_sample_items([l for l in layers if l not in fused])
        operands = self._per_sample_operands("Diagonal", items) if items else []
        records = {l: self._records_of("Diagonal", l) for l in fused}
        device = operands[0][1].device if operands else records[fused[0]][0].device
        new = [l for l in layers if l not in self.state]
        fresh = {}
        if new:
            self._state_arena = _Arena([(_wm_rows(l), l.weight.numel() // _wm_rows(l) + int(_bias_of(l) is not None))
                                        for l in new], device)
            fresh = dict(zip(new, self._state_arena.views))
        state = {l: fresh.get(l, self.state.get(l)) for l in layers}
        jobs = []
        for item, (sides, g, x) in zip(items, operands):
            layer, dst = (item.layer, state[item.layer][item.rows]) if isinstance(item, ops.GroupSlice) else (item, state[item])
            jobs.append(ops.PerSampleJob.of(sides, g, x, dst, alpha=batch_size, first=layer in fresh))
        ops.per_sample_sq_accumulate(jobs)                 # one product per layer or slice, all in one call
        ops.per_sample_dw_sq_accumulate([ops.PerSampleDwJob.of(l, *records[l], dst=state[l], alpha=batch_size,
                                                               first=l in fresh) for l in direct])
        ops.per_sample_norm_sq_accumulate([ops.PerSampleNormJob.of(l, *records[l], name=_layer_name(self.model, l),
                                                                   dst=state[l], alpha=batch_size, first=l in fresh)
                                           for l in normed])
        ops.per_sample_embedding_sq_accumulate([ops.PerSampleEmbeddingJob.of(l, *records[l], name=_layer_name(self.model, l),
                                                                             dst=state[l], alpha=batch_size,
                                                                             first=l in fresh) for l in embedded])
        for layer in layers:
            self.state[layer] = state[layer]

    def update(self, batch_size: int):
        if self.per_sample:
            return self._update_per_sample(batch_size)
        # one pass over modules() so that `state` gets the reference's insertion order (curvatures.py:149-174),
        # which is the order per-layer hyper-parameter lists are indexed by
        owned = {l for _, l in self._owned()}
        # the state of all (new) Linear / Conv2d layers in one arena: invert() with one pair of hyper-parameters is
        # then a single launch over it
        new = [l for _, l in self._owned() if l not in self.state and l.weight.grad is not None]
        fresh = {}
        if new:
            self._state_arena = _Arena(
                [(_wm_rows(l), l.weight.numel() // _wm_rows(l) + int(_bias_of(l) is not None)) for l in new],
                new[0].weight.device)
            fresh = dict(zip(new, self._state_arena.views))
        keys, items = [], []
        for layer in self.model.modules():
            name = layer.__class__.__name__
            if name not in self.layer_types:
                continue
            if name in _MATRIX_LAYERS:
                if name == 'Embedding':
                    _check_embedding_shard(self.model, layer, "Diagonal.update", self.shard)
                if layer in owned:
                    bias_grad = layer.bias.grad.contiguous().view(-1) if _bias_of(layer) is not None else None
                    keys.append(layer)
                    # state in Wm layout (out, in*kh*kw [+1]); a ConvTranspose2d gradient is permuted into it
                    items.append((_wm(layer, layer.weight.grad).contiguous(), bias_grad, fresh.get(layer, self.state.get(layer)),
                                  True if layer in fresh else None))
            elif name == 'MultiheadAttention':
                for key, weight, bias in (('attn_in', layer.in_proj_weight, layer.in_proj_bias),
                                          ('attn_out', layer.out_proj.weight, layer.out_proj.bias)):
                    keys.append(key)
                    items.append((weight.grad.contiguous(), bias.grad.contiguous(), self.state.get(key), None))
        # several modules may share the 'attn_*' keys (one pair for the whole model, as in the reference): the first
        # occurrence of every key goes into ONE launch, later ones accumulate onto it afterwards
        firsts, later = {}, []
        for key, item in zip(keys, items):
            if key in firsts:
                later.append((key, item))
            else:
                firsts[key] = item
        for key, st in zip(firsts, ops.sq_accumulate_many(firsts.values(), batch_size)):
            self.state[key] = st                   # new keys enter in modules() order, like the reference's
        for key, item in later:
            self.state[key] = ops.sq_accumulate(item[0], item[1], batch_size, self.state[key])

    def invert(self, add: Union[float, list, tuple] = 0., multiply: Union[float, list, tuple] = 1.):
        assert self.state, "State dict is empty. Did you call 'update' prior to this?"
        gindex = self._global_index()
        # first inversion: all inverse-state tensors of the Linear / Conv2d layers in ONE arena, so that sampling can
        # scale the whole model's noise with one launch (later calls overwrite them in place)
        arena = {}
        fresh = [l for l in self.state if l not in self.inv_state and not isinstance(l, str)]
        if fresh:
            self._inv_arena = _Arena([tuple(self.state[l].shape) for l in fresh], self.state[fresh[0]].device)
            arena = dict(zip(fresh, self._inv_arena.views))
        plain = [l for l in self.state if not isinstance(l, str)]
        states, invs = self._state_arena, self._inv_arena
        # (the last condition is not implied by the others: the inverse arena was shaped after whatever `state` held at
        # the first inversion, and `state` may have been rebuilt since)
        whole = _is_scalar(add) and _is_scalar(multiply) and len(plain) == len(self.state) and \
            states is not None and states.is_whole([self.state[l] for l in plain]) and \
            invs is not None and invs.is_whole([self.inv_state.get(l, arena.get(l)) for l in plain]) and \
            states.total == invs.total
        if whole:      # one pair of hyper-parameters, both dicts whole arenas (no attention entries): one launch
            for l in plain:
                self.inv_state.setdefault(l, arena.get(l))
            ops.rsqrt_affine(states.flat, float(add), float(multiply), out=invs.flat)
            self._zero_padding_rows()
            return
        for position, (layer, value) in enumerate(self.state.items()):
            # Diagonal uses lists when both are list/tuple (curvatures.py:183); same outcome as _hyper.
            # Keys that are not layers of this model (a foreign state dict) fall back to their position.
            n, s = self._hyper(add, multiply, gindex.get(layer, position), max(len(gindex), len(self.state)))
            out = self._reuse(self.inv_state.get(layer), value)
            if out is None and layer in arena:
                out = arena[layer]
            self.inv_state[layer] = ops.rsqrt_affine(value, n, s, out=out)
        self._zero_padding_rows()

    def _padded(self):
        """[(position in `state`, layer)] of the Embedding layers with a `padding_idx`: that row is not a parameter."""
        return [(k, l) for k, l in enumerate(self.state)
                if not isinstance(l, str) and ops.is_embedding_layer(l) and l.padding_idx is not None]

    def _zero_padding_rows(self) -> None:
        """The `padding_idx` row of an Embedding has no posterior spread: its inverse-state entries are 0, so the samplers
        leave it at its mean and it adds nothing to a variance."""
        for _, layer in self._padded():
            self.inv_state[layer][layer.padding_idx].zero_()

    def _log_det_parts(self, hypers):
        rows, total = self._spectrum_log_det(hypers, self.state)
        padded = self._padded()
        if padded:
            # the D entries of a padding row (state 0: log n each) are no parameters: taken out again, in float64
            resolved = self._resolved(hypers)
            for k, layer in padded:
                gone = torch.tensor([layer.embedding_dim * math.log(n) for n, _ in resolved[k][1]], dtype=torch.float64,
                                    device=rows.device)
                rows[k] -= gone
                total -= gone
        return rows, total

    @staticmethod
    def _reuse(prev: Optional[Tensor], like: Tensor) -> Optional[Tensor]:
        """The previous inverse-state tensor if it can be overwritten in place (stable addresses keep cached
        launch plans valid)."""
        if prev is not None and prev.shape == like.shape and prev.device == like.device and prev.is_contiguous():
            return prev
        return None

    def _predictive_terms(self) -> PredictiveTerms:
        # grid: inv**2 = 1 / (s state + n) = (1 / s) / (state + n / s)
        def weights(layer):                                # (a group slice: its row block of the layer's matrix)
            return self.inv_state[layer.layer][layer.rows] if isinstance(layer, ops.GroupSlice) else self.inv_state[layer]
        def spectrum(layer):
            return None, None, self.state[layer.layer][layer.rows] if isinstance(layer, ops.GroupSlice) else self.state[layer]
        return PredictiveTerms("Diagonal", basis=None, weights=weights, grid_basis=None, spectrum=spectrum, separable=False,
                               direct=lambda layer: (None, self.inv_state[layer], None),
                               direct_grid=lambda layer: (None, None, None, self.state[layer]))

    def _head_terms(self, layer, phi: Tensor, what: str) -> HeadTerms:
        # sample = Z * inv: Var f_c = sum_j inv[c, j]^2 phi~_j^2, and the logits are independent
        inv = self.inv_state[layer]
        if inv.dim() != 2 or inv.shape[1] != phi.shape[1]:
            raise NotImplementedError(f"{what}: the inverse state {tuple(inv.shape)} is not one (out, in) matrix")
        d2 = torch.empty(phi.shape[0], inv.shape[0], dtype=torch.float32, device=phi.device)
        ops.gemm_batched([ops.Gemm(ops.mul(phi, phi), ops.mul(inv, inv).t(), d2)])
        return HeadTerms(None, False, d2, d2)

    def _head_grid_check(self, layer, what: str) -> None:
        state = self.state[layer]
        if state.dim() != 2 or state.shape[1] != layer.in_features + (layer.bias is not None):
            raise NotImplementedError(f"{what}: the state {tuple(state.shape)} is not one (out, in) matrix")

    def _head_grid_terms(self, layer, phi: Tensor):
        return None, phi, (None, None, self.state[layer]), False

    def sample(self, layer: Union[Module, str], z: Optional[Tensor] = None) -> Tensor:
        assert self.inv_state, "Inverse state dict is empty. Did you call 'invert' prior to this?"
        inv = self.inv_state[layer]
        if z is None:
            z = self._randn(*inv.shape, device=inv.device)
        return ops.mul(z, inv)

    def sample_and_replace(self):
        """curvatures.py:117-129 including the MultiheadAttention branch.  For the Linear / Conv2d layers the
        per-layer loop (draw, multiply, two adds: ~5 launches per layer, launch-bound for a ResNet) is one noise
        launch, one multiply over an arena and one batched launch that writes ``mean + z * inv_state`` through the
        [W | b] split straight onto the parameters (a K = 1 product with the `MUL_E_ADD_F` epilogue)."""
        assert self.inv_state, "Inverse state dict is empty. Did you call 'invert' prior to this?"
        layers = [l for _, l in self._owned() if l in self.inv_state]
        params, param_ptrs, mean_ptrs = self._param_ptrs(layers)
        self._reload_mean(skip=params)
        if layers:
            key = (tuple(map(Tensor.data_ptr, [self.inv_state[l] for l in layers])), param_ptrs, mean_ptrs)
            plan = self._sample_plans().get(key)
            if plan is None:
                invs = [self.inv_state[l] for l in layers]
                dev = invs[0].device
                noise = _Arena([tuple(inv.shape) for inv in invs], dev)
                ones_r = torch.ones(max(inv.shape[0] for inv in invs), 1, dtype=torch.float32, device=dev)
                ones_c = torch.ones(1, max(inv.shape[1] for inv in invs), dtype=torch.float32, device=dev)
                jobs = []
                for layer, z in zip(layers, noise.views):
                    if not layer.weight.data.is_contiguous():
                        raise RuntimeError("Diagonal.sample_and_replace: parameters must be contiguous")
                    for live, mean in zip(_live_slots(layer), self._mean_slots(layer)):
                        jobs.append(ops.Gemm(ones_r[:z.shape[0]], ones_c[:, :live.view.shape[1]], live.view,
                                             epilogue=ops.EPI_MUL_E_ADD_F, E=z[:, live.cols], F=mean.view))
                # z and inv_state are shaped alike: one launch scales the noise when inv_state is invert()'s whole arena
                whole = self._inv_arena is not None and self._inv_arena.is_whole(invs)
                plan = (key, noise.flat, list(zip(noise.views, invs)), ops.GemmPlan(jobs),
                        self._inv_arena.flat if whole else None)
                self._keep_plan(key, plan)
            _, zflat, scale, gemms, inv_flat = plan
            self._randn(zflat.numel(), device=zflat.device, out=zflat)
            if inv_flat is not None:                               # z *= inv_state: one launch over the arena
                ops.mul(zflat, inv_flat, out=zflat)
            else:
                for z, inv in scale:
                    ops.mul(z, inv, out=z)
            gemms.run()
        if self.shard is None or self.shard.rank == 0:         # one owner for the attention entries
            for layer in self._attention():
                for weight, bias, key in ((layer.in_proj_weight, layer.in_proj_bias, 'attn_in'),
                                          (layer.out_proj.weight, layer.out_proj.bias, 'attn_out')):
                    self._replace(self.sample(key), weight, bias)
        self._allgather_sampled()


class BlockDiagonal(Curvature):
    """Block-diagonal (per-layer, full P x P) Fisher: state += ger(g, g) * batch_size with
    g = [W.grad.view(-1) ; b.grad] (curvatures.py:196-261).

    * ``update``: the rank-1 accumulation is the factor-build kernel on a one-sample linear "layer" (src (1, P)).
    * ``invert``: ``(s F + n I).inverse().cholesky()`` (:252-253) is the KFAC factor inversion with (n^2, s^2)
      passed for (add, multiply) - that routine damps with sqrt(s) F + sqrt(n) I, computed in double on the host.
    * ``sample``: ``z @ L`` (:258) as one GEMM.  The reference then views the weight part with ``weight.shape`` and
      concatenates the bias column along dim 1, which raises for Conv2d (4-D with 2-D).  Here the weight part is
      (out, -1) for every layer type - identical for Linear, and what ``_replace`` consumes for Conv2d.
    O(P^2) memory per layer: meant for small layers, like the reference's.  MultiheadAttention is not supported
    (the reference's branch, :220-239, concatenates a 2-D gradient with a 1-D bias and raises)."""

    def __init__(self, model: Union[Module, Sequential], layer_types: Union[List[str], str] = None, *, shard=None):
        super().__init__(model, layer_types, shard=shard)
        if any(_is_convt(l) for l in self._layers()):
            raise NotImplementedError("BlockDiagonal: ConvTranspose2d layers are not supported")

    def update(self, batch_size: int):
        jobs = []
        for _, layer in self._owned():
            parts = [layer.weight.grad.contiguous().view(-1)]
            if layer.bias is not None:
                parts.append(layer.bias.grad.contiguous())
            g = ops.concat(parts) if len(parts) > 1 else parts[0]
            first = layer not in self.state
            if first:
                self.state[layer] = torch.empty(g.numel(), g.numel(), dtype=torch.float32, device=g.device)
            jobs.append(ops.FactorJob(g.view(1, -1), self.state[layer], scale=float(batch_size), first=first))
        ops.kfac_accumulate(jobs)
        self._spectrum = None                        # (of the blocks as they were: `log_det_grid`)

    def _log_det_parts(self, hypers):
        kept = self.__dict__.get("_spectrum")
        if kept is None or list(kept) != list(self.state):
            _, values = ops.eigh(list(self.state.values()), with_values=True)
            kept = self._spectrum = {layer: ops.clamp_min0_(w) for layer, w in zip(self.state, values)}
        return self._spectrum_log_det(hypers, kept)

    def invert(self, add: Union[float, list, tuple] = 0., multiply: Union[float, list, tuple] = 1.):
        assert self.state, "State dict is empty. Did you call 'update' prior to this?"
        gindex = self._global_index()
        adds, muls = [], []
        for position, layer in enumerate(self.state.keys()):
            n, s = self._hyper(add, multiply, gindex.get(layer, position), max(len(gindex), len(self.state)))
            adds.append(n * n)
            muls.append(s * s)
        prev = [self.inv_state.get(layer) for layer in self.state.keys()]
        chols = ops.chol_inv_lower(list(self.state.values()), adds, muls, outs=prev)
        for layer, chol in zip(self.state.keys(), chols):
            self.inv_state[layer] = chol

    def _draw(self, layer: Module, z: Optional[Tensor]) -> Tensor:
        inv = self.inv_state[layer]
        if z is None:
            z = self._randn(inv.shape[0], device=inv.device)
        x = torch.empty(1, inv.shape[0], dtype=torch.float32, device=inv.device)
        ops.gemm_batched([ops.Gemm(z.view(1, -1), inv, x)])
        return x.view(-1)

    def sample(self, layer: Module, z: Optional[Tensor] = None) -> Tensor:
        assert self.inv_state, "Inverse state dict is empty. Did you call 'invert' prior to this?"
        x = self._draw(layer, z)
        n_w = layer.weight.numel()
        rows = layer.weight.shape[0]
        out = torch.empty(rows, n_w // rows + int(layer.bias is not None), dtype=torch.float32, device=x.device)
        out[:, :n_w // rows] = x[:n_w].view(rows, -1)         # the reference's torch.cat (:260-261): API plumbing
        if layer.bias is not None:
            out[:, -1] = x[n_w:]
        return out

    def sample_and_replace(self):
        """The base-class loop fused: one noise launch and one batched GEMM launch for all owned layers.  The draw
        z @ L is written straight onto the parameters in g's order (weights, then biases) with the mean added in the
        epilogue: no [W | b] detour, and the reload of the mean skips the parameters that are overwritten here."""
        assert self.inv_state, "Inverse state dict is empty. Did you call 'invert' prior to this?"
        owned = [(i, l) for i, l in self._owned() if l in self.inv_state]
        jobs, skip = [], []
        if owned:
            dev = self.inv_state[owned[0][1]].device
            flat = self._randn(sum(self.inv_state[l].shape[0] for _, l in owned), device=dev)
            pos = 0
            for _, layer in owned:
                inv = self.inv_state[layer]
                P = inv.shape[0]
                z = flat[pos:pos + P].view(1, P)
                pos += P
                col = 0
                for name in ('weight', 'bias'):                       # g's order: the weight, flat, then the bias
                    if layer._parameters[name] is None:
                        continue
                    p = layer._parameters[name].data
                    if not p.is_contiguous():
                        raise RuntimeError("BlockDiagonal.sample_and_replace: parameters must be contiguous")
                    k = p.numel()
                    jobs.append(ops.Gemm(z, inv[:, col:col + k], p.view(1, k), epilogue=ops.EPI_ADD_E,
                                         E=self.model_state_of(layer, name).view(1, k)))
                    skip.append(p)
                    col += k
        self._reload_mean(skip=skip)
        ops.gemm_batched(jobs)
        self._allgather_sampled()


def _groups_of(layer) -> int:
    """`groups` of a Conv2d; the channels of a normalisation layer (`ops.admit_norm_layers`: one 1 x n_g row each, the
    stacked paths of a depthwise convolution); 1 for every other layer."""
    if ops.is_norm_layer(layer):
        return layer.weight.numel()
    return int(getattr(layer, "groups", 1)) if layer.__class__.__name__ == 'Conv2d' else 1


def _reject_grouped(est, what: str) -> None:
    """EFB / INF have no eigen-correction for the block-diagonal factors of grouped convolutions (yet)."""
    names = {mod: name for name, mod in est.model.named_modules()}
    for layer in est._layers():
        if _groups_of(layer) > 1:
            raise NotImplementedError(f"{what}: grouped convolution '{names.get(layer, '?')}' (groups={layer.groups}) is not "
                                      "supported; select other layer types or use KFAC")


def _noise_count(first: Tensor, second: Tensor) -> int:
    """Normal draws one sample of a layer takes, from its pair of inverse factors: n m per Kronecker pair (an Embedding's
    first entry is the (V,) diagonal: V D)."""
    if first.dim() == 1:
        return first.numel() * second.size(-1)
    return first.numel() // first.size(-1) * second.size(-1)


def _pairs(first: Tensor, second: Tensor):
    """(L_A, L_G) of a layer as per-group lists of 2-D views: one pair for an ordinary layer, G for a grouped one."""
    if first.dim() == 3:
        return [(first[g], second[g]) for g in range(first.shape[0])]
    return [(first, second)]


class KFAC(LinearisedPredictive, Curvature):
    """Kronecker-factored Fisher (curvatures.py:264-392).

    ``state[layer] = [A, G]`` (fp32, exactly symmetric), ``inv_state[layer] = (L_A, L_G)`` with
    L = chol_lower((sqrt(s) F + sqrt(n) I)^-1).  ``record[layer] = [input, grad_output]``: unlike the
    reference the recorded grad_output is NOT pre-multiplied by the batch size (curvatures.py:310); the
    factor N is folded into the scale of the G-side SYRK, which saves one pass over every gradient.

    ``approximation`` (keyword-only extension) says how a layer that applies its weight at L positions per sample (the
    output pixels of a Conv2d, the tokens of a Linear on (N, *, in) inputs) enters the factors.  ``"expand"``, the default
    and the reference's form: all N L positions are columns of both Grams.  ``"reduce"`` (KFAC-reduce, Eschenhagen et al.,
    NeurIPS 2023): the positions are reduced first, x_n = mean_l x_{n,l} (the ones entry of a biased layer
    stays 1) and g_n = sum_l g_{n,l}, and A (+)= input_weight / N sum_n x_n x_n^T, G (+)= N / grad_scale^2 sum_n g_n g_n^T;
    for L = 1 both forms coincide.  The shapes of ``state`` / ``inv_state`` are the same, so everything downstream
    (``invert``, ``decompose``, the samplers, EFB, INF, the linearised predictives) takes either.  A reduce factor has
    rank at most the number of SAMPLES accumulated into it (an expand factor: positions): accumulate it over many batches
    and invert with ``add > 0``.  ``"reduce"`` takes Linear and Conv2d with groups 1, dilation 1 and integer padding."""

    _mha_as_projections = True
    _per_sample_groups = True
    _takes_norm = True
    _takes_embedding = True

    def __init__(self, model: Union[Module, Sequential], layer_types: Union[List[str], str] = None, *, shard=None,
                 approximation: str = "expand"):
        if approximation not in ("expand", "reduce"):
            raise ValueError(f'KFAC: approximation must be "expand" or "reduce", got {approximation!r}')
        super().__init__(model, layer_types, shard=shard)
        self.approximation = approximation
        self.hooks = list()
        self.record = dict()
        self._fresh = set()                          # (layer, side) of factors that nothing has written yet
        self._out_size = dict()                      # ConvTranspose2d layer -> (Ho, Wo) its last forward produced
        self._path_hints = dict()                    # sharded update(): recorded shapes -> launch form of the whole model
        for layer in model.modules():
            name = layer.__class__.__name__
            if name in self.layer_types:
                if approximation == "reduce":
                    _check_reduce(model, layer)
                if name in ('Linear', 'Conv2d'):
                    if name == 'Conv2d' and tuple(layer.dilation) != (1, 1):
                        # the reference silently ignores it (curvatures.py:329)
                        if not ops.dilated_admitted():
                            raise NotImplementedError("KFAC: dilated convolutions are not supported")
                        _check_dilated(model, layer)
                    # grouped convolutions (groups > 1): block-diagonal KFAC, one Kronecker pair per group (the
                    # reference ignores `groups` and then fails in _replace): state[layer] = [A, G] stacked (G, n, n)
                    if name == 'Conv2d' and not all(isinstance(p, int) for p in layer.padding):
                        raise NotImplementedError("KFAC: string padding modes are not supported")
                    self._record_layer(layer)
                elif name in _ND_LAYERS:
                    # `_check_conv_nd` has passed; a Conv1d is the Conv2d of its (N, C, 1, L) view, a dilated one (with
                    # `ops.admit_dilated`) under the rule of the class split; a Conv3d builds A from its depth-unfolded
                    # stack (curv_kfac_conv3d_accumulate), G as a 1x1 factor of grad_output
                    if any(d != 1 for d in layer.dilation):
                        _check_dilated(model, layer)
                    self._record_layer(layer)
                elif name in _NORM_LAYERS:
                    # `_check_norm` has passed; C stacked pairs [A (C, n_g, n_g), G (C, 1, 1)] from the fused pass of
                    # csrc/norm_factor.hip on the records as they are (a BatchNorm2d: in eval mode, `_check_eval`)
                    self._record_layer(layer)
                elif name == 'Embedding':
                    # `_check_embedding` has passed; state = [a (V,), G (D, D)]: the A factor of the bias-free Linear on
                    # one-hot rows is exactly diagonal - the token histogram of csrc/embedding_factor.hip - and G the
                    # flat build of grad_output; the record's input is the index tensor
                    self._record_layer(layer)
                elif name == 'ConvTranspose2d':
                    # Wm = weight.permute(1, 0, 2, 3).reshape(out, -1) [| bias]; A from the phase-split build
                    # (curv_kfac_convt_accumulate), G a 1x1 factor of grad_output as for Conv2d
                    _check_convt(layer)
                    self._record_layer(layer)
                elif name == 'MultiheadAttention':
                    # the two projections as Linear-like layers (extension: curvatures.py:303-304 raises here); their
                    # inputs / output gradients are tapped off the F.linear calls of the attention forward
                    tap = _LinearTap(self, layer)
                    for proj in AttentionProjection.of(layer):
                        self.record[proj] = [None, None]
                    self.hooks.append(layer.register_forward_pre_hook(tap.install))
                    self.hooks.append(layer.register_forward_hook(tap.remove, always_call=True))

    def update(self, batch_size: int = None, *, inputs: bool = True, grads: bool = True, input_weight: float = 1.0,
               grad_scale: float = 1.0):
        """A += X X^T / (N L), G += (N g)(N g)^T / (N L) for every selected layer: one grouped launch.  (With
        ``approximation="reduce"``: the position-reduced rows, N columns and L = 1 in these scales - the class docstring.)

        The keyword-only arguments extend the reference's ``update(batch_size)`` (curvatures.py:312) for
        Monte-Carlo Fisher loops that run several backward passes per forward pass
        (``curvature_amd.factors.compute_factors``): the A side depends only on the layer inputs, so it is
        built once per forward with ``input_weight`` = number of backward passes (``inputs=False`` for the
        others), instead of adding the same matrix again and again.

        Mixed precision: each side is routed by the dtype of its recorded tensor.  float32 goes to the fp32 build;
        bfloat16 / float16 (a model run under ``torch.autocast``) to the half-precision MFMA build
        (``ops.kfac_accumulate_half``), which computes the same factor as the fp32 build of the upcast tensor up to
        the order of the sums.  A grouped convolution's half-precision side is copied to float32 on the device and
        built by the grouped fp32 kernels (not on the half-precision kernel).  Any other dtype raises RuntimeError.
        ``grad_scale``: the loss scale of a ``torch.cuda.amp.GradScaler`` whose scaled loss produced the recorded
        gradients; the G side is divided by ``grad_scale ** 2``.  The caller skips ``update()`` on the steps the scaler
        skips (non-finite gradients)."""
        self._decomposition = None                   # (of the factors as they were: `decompose`)
        jobs = []                                    # of every class: ops.accumulate_factors sorts them to their builds
        if not grad_scale > 0:
            raise ValueError(f"KFAC.update: grad_scale must be positive, got {grad_scale}")
        g_div = float(grad_scale) ** 2
        for _, layer in self._owned():
            forward, backward = self.record[layer]
            if (inputs and forward is None) or (grads and backward is None):
                raise RuntimeError("KFAC.update: no recorded forward/backward pass for a selected layer")
            embedding = ops.is_embedding_layer(layer)
            if embedding:
                _check_embedding_shard(self.model, layer, "KFAC.update", self.shard)
            sides = ops.factor_jobs(layer, forward, backward, self._out_size.get(layer), self.approximation)
            N, L = sides.N, sides.L
            if self.approximation == "reduce":
                L = 1                                    # the positions are reduced before the Gram: N columns, not N L
            if layer not in self.state:
                # a side that is not written by this call must start from zero, not from garbage
                alloc = torch.empty if (inputs and grads) else torch.zeros
                dev = (sides.a or sides.g).src.device
                lead = (sides.groups,) if sides.groups > 1 else ()   # a grouped layer: one Kronecker pair per group
                a_shape = (sides.n,) if embedding else (*lead, sides.n, sides.n)   # an Embedding: the diagonal of A
                self.state[layer] = [alloc(*a_shape, dtype=torch.float32, device=dev),
                                     alloc(*lead, sides.m, sides.m, dtype=torch.float32, device=dev)]
                if inputs and grads:
                    self._fresh.update(((layer, 0), (layer, 1)))
            A, G = self.state[layer]
            if inputs:
                job = sides.a
                job.dst, job.scale, job.first = A, float(input_weight) / (N * L), self._take_fresh(layer, 0)
                jobs.append(job)
            if grads:
                job = sides.g                            # same scales for every kind of layer
                job.dst, job.scale, job.first = G, float(N) / L / g_div, self._take_fresh(layer, 1)
                jobs.append(job)
        if self.shard is not None and self.shard.world > 1:
            # the launch form is a property of the MODEL, not of this rank's share: a share under the small-launch threshold
            # would otherwise sum its factors in another order than the unsharded run (which is over it).  It follows
            # from the recorded shapes and dtypes of ALL selected layers (the hooks record every layer on every rank),
            # so it is worked out once per set of them
            records = [(layer, *(t if t is None else ops.ShapeOnly(t.shape, t.dtype) for t in self.record[layer]))
                       for layer in self._layers()]
            key = (inputs, grads, tuple(r[1:] for r in records))
            hint = self._path_hints.get(key)
            if hint is None:
                hint = self._path_hints[key] = self._unsharded_path(records, inputs, grads)
            for job in jobs:
                if type(job) is ops.FactorJob:
                    job.path_hint = hint
        if getattr(self, "_count_flops", False):                 # bench.py: what the launch plan executes
            self._last_flops = sum(ops.factor_plan_flops(jobs))
        ops.accumulate_factors(jobs, events=getattr(self, "_timing_events", None))

    def _unsharded_path(self, records, inputs: bool, grads: bool) -> int:
        """The launch form of the fp32 factor build of an unsharded update() on `records` = [(layer, input, grad_output)]
        (`ops.ShapeOnly`s): decided by the library itself (curv_kfac_path_for evaluates every gate of the small form, not
        only the flops) for the sides that come back as `FactorJob`.  Grouped, half-precision, transposed-convolution,
        dilated A sides and reduce factors are built by launches of their own, whose plans are per factor."""
        model_jobs = []
        for layer, forward, backward in records:
            if (inputs and forward is None) or (grads and backward is None):
                return _lib.PATH_GROUPED
            sides = ops.factor_jobs(layer, forward, backward, self._out_size.get(layer), self.approximation)
            model_jobs += [job for job, wanted in ((sides.a, inputs), (sides.g, grads))
                           if wanted and isinstance(job, ops.FactorJob)]
        return ops.kfac_path_for(model_jobs)

    def _take_fresh(self, layer, side: int) -> bool:
        """True once for a factor that nothing has written yet: its next build overwrites instead of adding."""
        if (layer, side) in self._fresh:
            self._fresh.discard((layer, side))
            return True
        return False

    def restart_accumulation(self) -> None:
        """The next `update()` overwrites the factors of every layer instead of adding to them (the tensors, their
        addresses and the launch plans built on them stay).  Extension of the reference API: its only way to start
        over is a new estimator."""
        self._fresh.update((layer, side) for layer in self.state for side in (0, 1))
        self._decomposition = None

    def invert(self, add: Union[float, list, tuple] = 0., multiply: Union[float, list, tuple] = 1., *, check: bool = True):
        """`check=False` (keyword-only extension): skip the read-back of the status words - the call's only host
        synchronisation - and leave them for `check_invert()`; a HIP-graph capture of the step needs that."""
        assert self.state, "State dict is empty. Did you call 'update' prior to this?"
        factors, adds, muls, prev = [], [], [], []
        gindex = self._global_index()
        stacked, where = {}, []
        for position, (layer, value) in enumerate(self.state.items()):
            # layer index = position among the selected layers in modules() order (== enumerate(state)
            # of the reference, curvatures.py:360, when every layer is owned)
            index = gindex.get(layer, position)
            n, s = self._hyper(add, multiply, index, max(len(gindex), len(self.state)))
            old = self.inv_state.get(layer, (None, None))
            for side, factor in enumerate(value):
                if factor.dim() == 1:
                    # the diagonal A of an Embedding: l_a = 1 / sqrt(sqrt(s) a + sqrt(n)) elementwise, the diagonal of what
                    # the sweep gives for diag(a); 0 for the padding row, which is no parameter
                    out = old[side]
                    if out is None or out.shape != factor.shape or out.device != factor.device:
                        out = torch.empty_like(factor)
                    ops.rsqrt_affine(factor, math.sqrt(n), math.sqrt(s), out=out)
                    if layer.padding_idx is not None:
                        out[layer.padding_idx].zero_()
                    stacked[(layer, side)] = out
                elif factor.dim() == 3:
                    # grouped layer: one descriptor per group slice, written in place into the stacked inverse
                    out = old[side]
                    if out is None or out.shape != factor.shape or out.device != factor.device:
                        out = torch.empty_like(factor)
                    stacked[(layer, side)] = out
                    for g in range(factor.shape[0]):
                        factors.append(factor[g])
                        prev.append(out[g])
                        adds.append(n)
                        muls.append(s)
                        where.append((layer, index, side, g))
                else:
                    factors.append(factor)
                    prev.append(old[side])
                    adds.append(n)
                    muls.append(s)
                    where.append((layer, index, side, None))
        # outputs of the previous call are overwritten in place (stable addresses keep the cached launch
        # plan of sample_and_replace valid); RuntimeError if a damped factor is not positive definite
        self._invert_where = where if any(f.dim() == 3 for f in stacked.values()) else None
        try:
            chols = ops.chol_inv_lower(factors, adds, muls, check=check, outs=prev)
        except RuntimeError as exc:
            if self._invert_where:
                self._raise_not_pd(ops.chol_inv_lower.last_info, exc)
            raise
        self._invert_info = chols.info
        pos = 0
        for layer, value in self.state.items():
            pair = []
            for side, factor in enumerate(value):
                if factor.dim() == 1:
                    pair.append(stacked[(layer, side)])
                elif factor.dim() == 3:
                    pair.append(stacked[(layer, side)])
                    pos += factor.shape[0]
                else:
                    pair.append(chols[pos])
                    pos += 1
            self.inv_state[layer] = tuple(pair)

    def _raise_not_pd(self, info: Tensor, cause: Exception):
        """Re-raise a failed inversion of a model with grouped layers, naming the layer and group of each bad factor."""
        host = info.cpu()
        names = {mod: name for name, mod in self.model.named_modules()}
        bad = []
        for i in torch.nonzero(host).flatten().tolist():
            if int(host[i]) < 0:
                raise cause
            layer, index, side, g = self._invert_where[i]
            what = f"layer {index} ({names.get(layer, layer.__class__.__name__)}) factor {'AG'[side]}"
            bad.append(what if g is None else f"{what} group {g}")
        raise RuntimeError("cholesky: damped factor(s) not positive-definite: " + "; ".join(bad)) from cause

    def check_invert(self) -> None:
        """Raise ``RuntimeError`` if the last ``invert(check=False)`` (or the last replay of a graph that contains it)
        met a damped factor that is not positive definite (curvatures.py:377-383 raises at that point)."""
        info = getattr(self, "_invert_info", None)
        if info is not None:
            try:
                ops.check_chol_info(info)
            except RuntimeError as exc:
                if getattr(self, "_invert_where", None):
                    self._raise_not_pd(info, exc)
                raise

    def _predictive_terms(self) -> PredictiveTerms:
        # sample = L_G Z L_A^T: T = L_G^T g, Y = L_A^T X.  Grid:
        # L L^T = (sqrt(s) F + sqrt(n) I)^-1 = U diag(1 / (sqrt(s) (lambda + sqrt(n / s)))) U^T on both sides: the two
        # 1 / sqrt(s) make the gain 1 / s, and the shift of both spectra is sqrt(n / s)
        kept = getattr(self, "_decomposition", None)
        def basis(layer):                                  # (a group slice: its pair of the stacked inverse factors)
            if isinstance(layer, ops.GroupSlice):
                return tuple(f[layer.g].t() for f in reversed(self.inv_state[layer.layer]))
            return tuple(f.t() for f in reversed(self.inv_state[layer]))
        def eigen(layer):                                  # (a group slice: its group of the stacked decomposition)
            if isinstance(layer, ops.GroupSlice):
                return tuple(t[layer.g] for t in kept[layer.layer][:4])
            return kept[layer]
        return PredictiveTerms(
            "KFAC", basis=basis, weights=None,
            grid_basis=lambda layer: eigen(layer)[:2], spectrum=lambda layer: (eigen(layer)[2], eigen(layer)[3], None),
            separable=True, grid_missing=None if kept is not None else
            "no eigendecomposition of the current factors: call decompose() after the last update()",
            # depthwise (one output channel per group): T = L_A stacked (C, n_g, n_g), s = L_G stacked (C, 1, 1), in place
            # (an Embedding, `ops.per_sample_route` "embedding": T = l_a (V,), s = L_G (D, D))
            direct=lambda layer: (self.inv_state[layer][0], None, self.inv_state[layer][1]),
            # its grid: T = U_A stacked, u = the 1 x 1 G factors (their own eigenvalues), v = eig(A) (C, n_g)
            direct_grid=lambda layer: (kept[layer][4], kept[layer][2].view(-1), kept[layer][3], None))

    def decompose(self) -> None:
        """The eigendecompositions F = U diag(lambda) U^T of the accumulated factors of every owned layer, in one batched
        `ops.eigh`: what `functional_variance_grid` needs instead of an inversion.  Kept per layer as
        ``(U_G^T, U_A^T, lambda_G, lambda_A)``, the eigenvalues clamped at 0 (a factor is positive semi-definite; the
        iteration may leave -1e-9); `update()` and `restart_accumulation()` drop it.  Grouped layers (stacked factors)
        are left out - unless `ops.admit_grouped_per_sample` and `ops.admit_grouped_joint` are both on: then the per-group
        matrices go into the same `ops.eigh` call (a 1 x 1 factor is its own eigenvalue and does not) and the result stays
        stacked, ``(U_G^T (G, m, m), U_A^T (G, n, n), lambda_G (G, m), lambda_A (G, n))``, for a depthwise layer
        (`ops.per_sample_route`) with U_A (G, n, n) itself as a fifth entry, which its grid job reads."""
        assert self.state, "State dict is empty. Did you call 'update' prior to this?"
        for layer in self.state:
            if ops.is_norm_layer(layer):
                raise NotImplementedError(f"KFAC.decompose: the normalisation layer {_layer_name(self.model, layer)} "
                                          f"({layer.__class__.__name__}) is not supported; {_NORM_ADVICE}")
            if ops.is_embedding_layer(layer):
                _refuse_embedding(self.model, layer, "KFAC.decompose")
        stacked = ops.per_sample_admits_groups() and ops.per_sample_admits_grouped_joint()
        layers = [l for l, (A, G) in self.state.items() if (A.dim() == 2 and G.dim() == 2) or
                  (stacked and A.dim() == 3 and G.dim() == 3)]

        def solved(F):                                     # the 2-D matrices of a factor that go to the solver
            return [F] if F.dim() == 2 else [f for f in F if f.shape[-1] > 1]
        mats = [f for l in layers for F in self.state[l] for f in solved(F)]
        vecs, vals = ops.eigh(mats, with_values=True) if mats else ([], [])
        self._decomposition = {}
        at = 0
        for layer in layers:
            sides = []                                     # (U, lambda) of the A and of the G side
            for F in self.state[layer]:
                count = len(solved(F))
                U, lam = vecs[at:at + count], vals[at:at + count]
                at += count
                if F.dim() == 2:
                    sides.append((U[0], ops.clamp_min0_(lam[0])))
                elif count:
                    sides.append((torch.stack(U), ops.clamp_min0_(torch.stack(lam))))
                else:
                    sides.append((torch.ones_like(F), ops.clamp_min0_(F.reshape(F.shape[0], 1).clone())))
            (U_A, lam_A), (U_G, lam_G) = sides
            kept = (U_G.transpose(-1, -2).contiguous(), U_A.transpose(-1, -2).contiguous(), lam_G, lam_A)
            if U_A.dim() == 3 and ops.per_sample_route(layer) == "depthwise":
                kept += (U_A,)
            self._decomposition[layer] = kept

    def _log_det_parts(self, hypers):
        for layer in self.state:
            if ops.is_embedding_layer(layer):
                _refuse_embedding(self.model, layer, "KFAC.log_det_grid")
        kept = getattr(self, "_decomposition", None)
        if kept is None:
            raise RuntimeError("KFAC.log_det_grid: no eigendecomposition of the current factors: call decompose() after the "
                               "last update()")
        left_out = [_layer_name(self.model, l) for l in self.state if l not in kept]
        if left_out:
            raise RuntimeError(f"KFAC.log_det_grid: decompose() left out the grouped layer(s) {', '.join(left_out)}: switch "
                               "ops.admit_grouped_per_sample and ops.admit_grouped_joint on and call decompose() again")
        segments = []
        for layer, points in self._resolved(hypers):
            lam_G, lam_A = kept[layer][2], kept[layer][3]           # (m,), (n,) - stacked: (G, m), (G, n), every group alike
            gains, shifts = [math.sqrt(s) for _, s in points], [math.sqrt(n) for n, _ in points]
            segments.append(ops.LogSumSegment.of(lam_A, lam_G.shape[-1], gains, shifts))
            segments.append(ops.LogSumSegment.of(lam_G, lam_A.shape[-1], gains, shifts))
        out, total = ops.logsum_grid(segments, len(hypers))
        return out[0::2] + out[1::2], total

    def _head_terms(self, layer, phi: Tensor, what: str) -> HeadTerms:
        # sample = L_G Z L_A^T: Cov(f_c, f_c') = ||L_A^T phi~||^2 (L_G L_G^T)[c, c']
        L_A, L_G = self.inv_state[layer]
        if L_A.dim() != 2 or L_G.dim() != 2:
            raise NotImplementedError(f"{what}: stacked (grouped) factors {tuple(L_A.shape)}, {tuple(L_G.shape)}")
        N, dev = phi.shape[0], phi.device
        Y = torch.empty(N, L_A.shape[1], dtype=torch.float32, device=dev)
        ops.gemm_batched([ops.Gemm(phi, L_A, Y)])
        d2 = self._row_sums(ops.mul(Y, Y))
        g = self._row_sums(ops.mul2d(L_G, L_G), tri=ops.TRI_A_LOWER)       # diag(L_G L_G^T) from the lower triangle
        variance = torch.empty(N, L_G.shape[0], dtype=torch.float32, device=dev)
        ops.gemm_batched([ops.Gemm(d2.view(N, 1), g.view(1, -1), variance)])
        return HeadTerms(L_G, True, d2, variance)

    def _head_grid_check(self, layer, what: str) -> None:
        A, G = self.state[layer]
        if A.dim() != 2 or G.dim() != 2:
            raise NotImplementedError(f"{what}: stacked (grouped) factors {tuple(A.shape)}, {tuple(G.shape)}")
        kept = getattr(self, "_decomposition", None)
        if kept is None or layer not in kept:
            raise RuntimeError(f"{what}: no eigendecomposition of the current factors: call decompose() after the last "
                               "update()")

    def _head_grid_terms(self, layer, phi: Tensor):
        # (sqrt(s) F + sqrt(n) I)^-1 = U diag(1 / (sqrt(s) (lambda + sqrt(n / s)))) U^T on both sides: Sigma = U_G diag(d2) U_G^T
        U_Gt, U_At, lam_G, lam_A = self._decomposition[layer][:4]
        Y = torch.empty(phi.shape[0], U_At.shape[0], dtype=torch.float32, device=phi.device)
        ops.gemm_batched([ops.Gemm(phi, U_At.t(), Y)])
        return U_Gt.t().contiguous(), Y, (lam_G, lam_A, None), True     # (head_mc wants M with unit column stride)

    def sample(self, layer: Module, z: Optional[Tensor] = None) -> Tensor:
        """(L_A z L_G^T)^T -> (m, n) (curvatures.py:387-392); `z` (n, m) may be supplied for parity tests."""
        assert self.inv_state, "Inverse state dict is empty. Did you call 'invert' prior to this?"
        first, second = self.inv_state[layer]
        n, m = first.size(-1), second.size(-1)
        if first.dim() == 1:
            # an Embedding: (V, D) = diag(l_a) z L_G^T, the row scale in the product's epilogue
            if z is None:
                z = self._randn(n, m, device=first.device)
            if tuple(z.shape) != (n, m):
                raise RuntimeError(f"KFAC.sample: noise of an Embedding layer must be ({n}, {m})")
            out = torch.empty(n, m, dtype=torch.float32, device=first.device)
            ops.gemm_batched([ops.Gemm(z, second.t(), out, epilogue=ops.EPI_MUL_E, E=first.view(n, 1).expand(n, m),
                                       tri=ops.TRI_B_UPPER)])
            return out
        if first.dim() == 3:
            # grouped layer: z (G, n, m); row block g of the (C_out, n) result is (L_A[g] z[g] L_G[g]^T)^T
            G = first.shape[0]
            if z is None:
                z = self._randn(G, n, m, device=first.device)
            if tuple(z.shape) != (G, n, m):
                raise RuntimeError(f"KFAC.sample: noise of a grouped layer must be ({G}, {n}, {m})")
            tmp = torch.empty(G, m, n, dtype=torch.float32, device=first.device)
            out = torch.empty(G * m, n, dtype=torch.float32, device=first.device)
            blocks = out.view(G, m, n)
            pairs = _pairs(first, second)
            ops.gemm_batched([ops.Gemm(lg, z[g].t(), tmp[g], tri=ops.TRI_A_LOWER) for g, (_, lg) in enumerate(pairs)])
            ops.gemm_batched([ops.Gemm(tmp[g], la.t(), blocks[g], tri=ops.TRI_B_UPPER) for g, (la, _) in enumerate(pairs)])
            return out
        if z is None:
            z = self._randn(n, m, device=first.device)
        tmp = torch.empty(m, n, dtype=torch.float32, device=first.device)
        out = torch.empty(m, n, dtype=torch.float32, device=first.device)
        ops.gemm_batched([ops.Gemm(second, z.t(), tmp, tri=ops.TRI_A_LOWER)])       # L_G lower triangular
        ops.gemm_batched([ops.Gemm(tmp, first.t(), out, tri=ops.TRI_B_UPPER)])      # L_A^T upper triangular
        return out

    def sample_and_replace(self, noise: Optional[Dict[Module, Tensor]] = None):
        """Fused form of the base-class loop: two batched GEMM launches for the whole model, the second
        writing ``mean + sample`` straight into the parameters (same result as curvatures.py:117-129)."""
        assert self.inv_state, "Inverse state dict is empty. Did you call 'invert' prior to this?"
        owned = self._owned()
        ptr = Tensor.data_ptr
        params, param_ptrs, mean_ptrs = self._param_ptrs([l for _, l in owned])
        # The two GEMM launches are described once and replayed while the tensors involved stay where they
        # are (invert() rewrites inv_state in place): per call only the noise is drawn.
        inv_state = self.inv_state
        key = (noise is None, tuple(map(ptr, [t for _, l in owned for t in inv_state[l]])), param_ptrs, mean_ptrs,
               tuple(map(ptr, noise.values())) if noise is not None else ())
        plan = self._sample_plans().get(key)
        if plan is None:
            stage1, stage2 = [], []
            flat, pos = None, 0
            if noise is None and owned:        # one generator launch for the whole model
                dev = self.inv_state[owned[0][1]][0].device
                total = sum(_noise_count(*self.inv_state[l]) for _, l in owned)
                flat = torch.empty(total, dtype=torch.float32, device=dev)
            for _, layer in owned:
                first, second = self.inv_state[layer]
                n, m = first.size(-1), second.size(-1)
                G = first.shape[0] if first.dim() == 3 else 1
                if noise is not None:
                    z = noise[layer]
                else:
                    z = flat[pos:pos + G * n * m].view(*((G,) if first.dim() == 3 else ()), n, m)
                    pos += G * n * m
                zs = z if G > 1 else [z]
                slots = list(zip(_live_slots(layer), self._mean_slots(layer)))
                if first.dim() == 1:
                    # an Embedding: weight = mean + diag(l_a) z L_G^T in one product (no first stage: A is diagonal)
                    (live, mean), = slots
                    stage2.append(ops.Gemm(z, second.t(), live.view, epilogue=ops.EPI_MUL_E_ADD_F,
                                           E=first.view(n, 1).expand(n, m), F=mean.view, tri=ops.TRI_B_UPPER))
                    continue
                # grouped layer: group g owns the rows [g m, (g + 1) m) of every slot - one pair of products per group
                for g, (la, lg) in enumerate(_pairs(first, second)):
                    rows = slice(g * m, (g + 1) * m)
                    tmp = torch.empty(m, n, dtype=torch.float32, device=first.device)
                    stage1.append(ops.Gemm(lg, zs[g].t(), tmp, tri=ops.TRI_A_LOWER))
                    la_t = la.t()
                    for live, mean in slots:
                        # one product per slot, its epilogue writing through the slot's strides.  Only the leading columns
                        # of L_A^T are still upper triangular: a kernel tap's column slice and the bias column run dense
                        stage2.append(ops.Gemm(tmp, la_t[:, live.cols], live.view[rows], epilogue=ops.EPI_ADD_E,
                                               E=mean.view[rows], tri=ops.TRI_B_UPPER if live.lead else ops.TRI_NONE))
            _largest_first(stage1)
            _largest_first(stage2)
            plan = (key, flat, ops.GemmPlan(stage1), ops.GemmPlan(stage2))
            self._keep_plan(key, plan)
        if plan[1] is not None:
            self._randn(plan[1].numel(), device=plan[1].device, out=plan[1])
        plan[2].run()
        plan[3].run()
        # the other state tensors (BatchNorm, layers outside the estimator) go back to their means BEHIND the GEMMs: the
        # second stage has written weight and bias of every owned layer (mean + sample), the copies touch the rest, and
        # a step that has just synchronised in invert() gets its long kernels queued ~0.1 ms earlier this way
        self._reload_mean(skip=params)
        self._allgather_sampled()

    # ------------------------------------------------------------------ batched multi-sample generation
    def sample_many(self, count: int, noise: Optional[Dict[Module, Tensor]] = None) -> "SampleBank":
        """`count` posterior samples of every owned layer in two launches (scripts/evaluate.py:134-139 draws one sample
        per forward sweep; a BNN evaluation needs 10-100 of them).

        With z_s (n x m) the noise of sample s, W_s = (L_A z_s L_G^T)^T = L_G (L_A z_s)^T (curvatures.py:387-392).
        Stage A forms V = L_A [z_1 | ... | z_S] as ONE product per layer with S m columns - the n x n triangular factor
        (80 % of a ResNet-50 sample's flops) is streamed once for all S samples instead of once per sample - and stage
        B the S products W_s = L_G V_s^T with ``mean +`` fused, written into a bank of parameter sets
        (`SampleBank.weights[layer]`: (S, m, n0), `.biases[layer]`: (S, m)).  `replace_from(bank, s)` loads set s into
        the model.  `noise[layer]`: (S, n, m) caller-supplied z_s (parity tests); otherwise one generator launch."""
        assert self.inv_state, "Inverse state dict is empty. Did you call 'invert' prior to this?"
        S = int(count)
        assert S >= 1
        owned = self._owned()
        ptr = Tensor.data_ptr
        key = ("many", S, noise is None, tuple(map(ptr, [t for _, l in owned for t in self.inv_state[l]])),
               tuple(map(ptr, noise.values())) if noise is not None else ())
        cache = self.__dict__.setdefault("_many_plans", {})
        plan = cache.get(key)
        if plan is None:
            cache.clear()                                    # one bank's worth of buffers at a time
            dev = self.inv_state[owned[0][1]][0].device
            total = sum(_noise_count(*self.inv_state[l]) for _, l in owned)
            flat = torch.empty(S * total, dtype=torch.float32, device=dev) if noise is None else None
            stage_a, stage_b, weights, biases, keep = [], [], {}, {}, []
            pos = 0
            for _, layer in owned:
                first, second = self.inv_state[layer]
                n, m = first.size(-1), second.size(-1)
                grouped = first.dim() == 3
                G = first.shape[0] if grouped else 1
                shape = (S, G, n, m) if grouped else (S, n, m)
                if first.dim() == 1:
                    # an Embedding: set k = mean + diag(l_a) z_k L_G^T, one product per set in the second launch
                    if noise is not None:
                        z = noise[layer]
                        if tuple(z.shape) != shape:
                            raise RuntimeError(f"sample_many: noise of a layer must be {shape}")
                    else:
                        z = flat[pos:pos + S * n * m].view(S, n, m)
                        pos += S * n * m
                    wb, bb = _bank_buffers(layer, S, dev)
                    mean, = self._mean_slots(layer)
                    for k in range(S):
                        stage_b.append(ops.Gemm(z[k], second.t(), wb[k], epilogue=ops.EPI_MUL_E_ADD_F,
                                                E=first.view(n, 1).expand(n, m), F=mean.view, tri=ops.TRI_B_UPPER))
                    keep.append(z)
                    weights[layer], biases[layer] = wb, bb
                    continue
                if noise is not None:
                    z = noise[layer]
                    if tuple(z.shape) != shape:
                        raise RuntimeError(f"sample_many: noise of a layer must be {shape}")
                    z = z.view(S, G, n, m)
                    zts = [z[:, g].transpose(1, 2).contiguous().view(S * m, n) for g in range(G)]   # rows (s, j): z_s^T
                else:
                    zts = list(flat[pos:pos + S * G * n * m].view(G, S * m, n))       # iid: drawn directly as z_s^T
                    pos += S * G * n * m
                wb, bb = _bank_buffers(layer, S, dev)
                sets = [_slots(layer, wb[k], bb[k] if bb is not None else None) for k in range(S)]
                means = self._mean_slots(layer)
                for g, ((la, lg), zt) in enumerate(zip(_pairs(first, second), zts)):
                    rows = slice(g * m, (g + 1) * m)                              # of group g, as in sample_and_replace
                    V = torch.empty(n, S * m, dtype=torch.float32, device=dev)
                    stage_a.append(ops.Gemm(la, zt.t(), V, tri=ops.TRI_A_LOWER))     # V = L_A [z_1 | ... | z_S]
                    for k in range(S):
                        Vs_t = V[:, k * m:(k + 1) * m].t()                        # (m, n) view of V_s^T: K-contiguous columns
                        for slot, mean in zip(sets[k], means):
                            stage_b.append(ops.Gemm(lg, Vs_t[:, slot.cols], slot.view[rows], epilogue=ops.EPI_ADD_E,
                                                    E=mean.view[rows], tri=ops.TRI_A_LOWER))
                    keep += [zt, V]
                weights[layer], biases[layer] = wb, bb
            _largest_first(stage_a)
            _largest_first(stage_b)
            plan = (flat, ops.GemmPlan(stage_a), ops.GemmPlan(stage_b), SampleBank(S, weights, biases), keep)
            cache[key] = plan
        if plan[0] is not None:
            self._randn(plan[0].numel(), device=plan[0].device, out=plan[0])
        plan[1].run()
        plan[2].run()
        return plan[3]


class SampleBank:
    """`count` sampled parameter sets of an estimator's own layers (`KFAC.sample_many`): ``weights[layer]`` is
    (count, out, in[*kh*kw]) and ``biases[layer]`` (count, out) or None, each entry ``mean + sample``.  The buffers belong
    to the estimator's launch plan: the next `sample_many` call of the same size overwrites them."""

    def __init__(self, count: int, weights: Dict[Module, Tensor], biases: Dict[Module, Optional[Tensor]]):
        self.count, self.weights, self.biases = count, weights, biases


class EFB(LinearisedPredictive, Curvature):
    """Eigenvalue-corrected Kronecker factorisation (curvatures.py:395-460).

    ``state[layer]`` = Lambda (m, n) accumulating (U_G^T grad U_A)**2, ``diags[layer]`` the diagonal Fisher
    grad**2 * batch_size, ``eigvecs[layer] = (U_A, U_G)``, ``inv_state[layer] = (s Lambda + n)^-1/2``.

    Keyword-only extensions of the reference constructor: `shard` (this rank decomposes, updates, inverts and
    samples only the layers it owns; with a layer-sharded KFAC `factors` already holds just those) and
    `eigvecs` (a precomputed ``{layer: (U_A, U_G)}``, e.g. another estimator's, instead of decomposing)."""

    _mha_as_projections = True

    def __init__(self, model: Union[Module, Sequential], factors: Dict[Module, Tensor],
                 layer_types: Union[List[str], str] = None, *, shard=None, eigvecs=None, per_sample: bool = False):
        """`per_sample` (keyword-only, default off: nothing changes): ``update(batch_size)`` accumulates the exact
        ``batch_size * sum_n (U_G^T P_n U_A)**2`` into `state` and ``batch_size * sum_n P_n**2`` into `diags`, with
        P_n = g_n X_n^T the share of sample n in [W.grad | b.grad], from recorded layer inputs and grad_outputs (see
        `Diagonal`; the P_n are those of the batch pass, also under a training-mode BatchNorm) instead of squaring the
        batch gradient.  The two agree at batch size 1.  Layers and record dtypes as for `Diagonal`; with
        `ops.widen_per_sample` also the two projections of a selected MultiheadAttention module."""
        super().__init__(model, layer_types, shard=shard)
        self.per_sample = bool(per_sample)
        if self.per_sample:
            self._record_per_sample("EFB")
        _reject_grouped(self, "EFB")
        if eigvecs is None:
            from .utils import get_eigenvectors
            if shard is not None:
                mine = {l for _, l in self._owned()}
                factors = {l: f for l, f in factors.items() if l in mine}
            eigvecs = get_eigenvectors(factors)
        self.eigvecs = eigvecs
        self.diags = dict()

    def _mine(self) -> List[Module]:
        """Owned layers that have eigenvectors, in ``modules()`` order."""
        return [l for _, l in self._owned() if l in self.eigvecs]

    def _update_per_sample(self, batch_size):
        layers = self._mine()
        if not layers:
            return
        # both operands of every layer packed as ONE (rows, N Lp) matrix: a rotation is one product per layer,
        #   T = U_G^T g (m x N Lp),  Y = U_A^T X (n x N Lp),  then  Lambda += batch_size * sum_n (T_n Y_n^T)**2
        operands = self._per_sample_operands("EFB", layers, rows_outer=True, in_place=False)
        dev = operands[0][1].device
        missing = [(l, s) for l, (s, _, _) in zip(layers, operands) if l not in self.state]
        if missing:
            self._state_arena = _Arena([(s.m, s.n) for _, s in missing], dev, zero=True)
            for (l, _), v in zip(missing, self._state_arena.views):
                self.state[l] = v
        rotations = []
        for layer, (sides, g, x) in zip(layers, operands):
            U_At, U_Gt = self._eigvecs_t(layer)
            rotations += [(U_Gt, g, sides.m), (U_At, x, sides.n)]
        rotated = self._rotated(rotations)
        jobs = []
        for k, (layer, (sides, g, x)) in enumerate(zip(layers, operands)):
            jobs.append(ops.PerSampleJob.of(sides, rotated[2 * k], rotated[2 * k + 1], self.state[layer], alpha=batch_size))
            first = layer not in self.diags
            if first:
                self.diags[layer] = torch.empty(sides.m, sides.n, dtype=torch.float32, device=dev)
            jobs.append(ops.PerSampleJob.of(sides, g, x, self.diags[layer], alpha=batch_size, first=first))
        ops.per_sample_sq_accumulate(jobs)

    def update(self, batch_size: int):
        if self.per_sample:
            return self._update_per_sample(batch_size)
        layers = self._mine()
        if not layers:
            return
        grads = []
        for layer in layers:
            gw = layer.weight.grad
            if gw is None:
                raise RuntimeError("EFB.update: a selected layer has no gradient (call backward() first)")
            # Wm layout (out, in*kh*kw): a ConvTranspose2d gradient is permuted into it
            grads.append((_wm(layer, gw).contiguous(), layer.bias.grad if layer.bias is not None else None))
        dev = grads[0][0].device
        missing = [k for k, layer in enumerate(layers) if layer not in self.state]
        if missing:
            # Lambda of all (new) layers in one zeroed arena: every update is then the same accumulate launch pair
            self._state_arena = _Arena([(grads[k][0].shape[0], grads[k][0].numel() // grads[k][0].shape[0] +
                                         int(grads[k][1] is not None)) for k in missing], dev, zero=True)
            for k, v in zip(missing, self._state_arena.views):
                self.state[layers[k]] = v
        # The launch plan is keyed by what it writes and by the eigenvectors only.  The gradients are staged into an arena the
        # plan owns with one batched copy per call: after zero_grad(set_to_none=True) every backward pass allocates new
        # .grad tensors, so a plan keyed by their addresses would be rebuilt on every update() and would pin the old
        # gradients (a second copy of all of them) through its descriptors.
        key = tuple(self.state[l].data_ptr() for l in layers) + tuple(t.data_ptr() for l in layers for t in self.eigvecs[l])
        plan = getattr(self, "_update_plan", None)
        if plan is None or plan[0] != key:
            stage1, stage2, staged = [], [], []
            tmps = _Arena([tuple(self.state[l].shape) for l in layers], dev).views
            shapes = []
            for layer, (gw, gb) in zip(layers, grads):
                m = gw.shape[0]
                shapes.append((m, gw.numel() // m))
                if gb is not None:
                    shapes.append((m, 1))
            views = _Arena(shapes, dev).views
            vi = 0
            for layer, (gw, gb), tmp in zip(layers, grads, tmps):
                n0 = gw.numel() // gw.shape[0]
                U_A, U_G = self.eigvecs[layer]
                if gb is None and min(gw.shape[0], n0) >= 64:
                    # bias-free layer: both products in the "rows times rows" form the LDS-DMA GEMM kernel takes (every operand
                    # contiguous along the summation index) - the eigenvectors are constants, their transposes are kept:
                    #   T^T = U_A^T W.grad^T  (n0 x m),   Lambda += (U_G^T T)**2 = (U_G^T (T^T)^T)**2
                    U_At, U_Gt = self._eigvecs_t(layer)
                    tmp_t = tmp.view(-1)[:n0 * gw.shape[0]].view(n0, gw.shape[0])
                    stage1.append(ops.Gemm(U_At, views[vi].t(), tmp_t))
                    staged.append(views[vi])
                    vi += 1
                    stage2.append(ops.Gemm(U_Gt, tmp_t.t(), self.state[layer], beta=1.0, epilogue=ops.EPI_SQUARE))
                    continue
                stage1.append(ops.Gemm(U_G.t(), views[vi], tmp[:, :n0]))              # U_G^T [W.grad | b.grad]
                staged.append(views[vi])
                vi += 1
                if gb is not None:
                    stage1.append(ops.Gemm(U_G.t(), views[vi], tmp[:, n0:]))
                    staged.append(views[vi])
                    vi += 1
                stage2.append(ops.Gemm(tmp, U_A, self.state[layer], beta=1.0, epilogue=ops.EPI_SQUARE))   # Lambda += (. U_A)**2
            plan = (key, ops.GemmPlan(stage1), ops.GemmPlan(stage2), staged)
            self._update_plan = plan
        srcs = []
        for gw, gb in grads:
            srcs.append(gw.view(gw.shape[0], -1))
            if gb is not None:
                srcs.append(gb.contiguous().view(-1, 1))
        ops.CopyPlan(plan[3], srcs).run()
        plan[1].run()
        plan[2].run()
        done = ops.sq_accumulate_many([(gw, gb.contiguous() if gb is not None else None, self.diags.get(layer), None)
                                       for layer, (gw, gb) in zip(layers, grads)], batch_size)      # one launch
        for layer, st in zip(layers, done):
            self.diags[layer] = st

    def _eigvecs_t(self, layer):
        """(U_A^T, U_G^T) as contiguous tensors, formed once per layer (the eigenvectors are constants of the estimator)."""
        cache = self.__dict__.setdefault("_eigvecs_t_cache", {})
        U_A, U_G = self.eigvecs[layer]
        hit = cache.get(layer)
        if hit is None or hit[0] != (U_A.data_ptr(), U_G.data_ptr()):
            hit = ((U_A.data_ptr(), U_G.data_ptr()), U_A.t().contiguous(), U_G.t().contiguous())
            cache[layer] = hit
        return hit[1], hit[2]

    def invert(self, add: Union[float, list, tuple] = 0., multiply: Union[float, list, tuple] = 1.):
        assert self.state, "State dict is empty. Did you call 'update' prior to this?"
        gindex = self._global_index()
        layers = list(self.state.keys())
        values = [self.state[l] for l in layers]
        prev = [self.inv_state.get(l) for l in layers]
        if not (all(p is not None and p.shape == v.shape for p, v in zip(prev, values))
                and self._inv_arena is not None and self._inv_arena.is_whole(prev)):
            # inverse state of all layers in one arena, overwritten in place by later calls (stable addresses
            # keep the sampler's launch plan valid; the noise scaling is one launch over the flat buffer)
            self._inv_arena = _Arena([tuple(v.shape) for v in values], values[0].device)
            for layer, v in zip(layers, self._inv_arena.views):
                self.inv_state[layer] = v
        states = self._state_arena
        if _is_scalar(add) and _is_scalar(multiply) and states is not None and states.is_whole(values):
            # one pair of hyper-parameters for every layer and both dicts are whole arenas (inv_state is one, shaped like
            # `values`, after the block above): one launch
            ops.rsqrt_affine(states.flat, float(add), float(multiply), out=self._inv_arena.flat)
            return
        for position, (layer, value) in enumerate(zip(layers, values)):
            n, s = self._hyper(add, multiply, gindex.get(layer, position), max(len(gindex), len(layers)))
            ops.rsqrt_affine(value, n, s, out=self.inv_state[layer])

    def _log_det_parts(self, hypers):
        return self._spectrum_log_det(hypers, self.state)

    def _predictive_terms(self) -> PredictiveTerms:
        # sample = U_G (Z * inv) U_A^T: T = U_G^T g, Y = U_A^T X, as `_update_per_sample`
        basis = lambda layer: self._eigvecs_t(layer)[::-1]     # noqa: E731
        return PredictiveTerms("EFB", basis=basis, weights=lambda layer: self.inv_state[layer], grid_basis=basis,
                               spectrum=lambda layer: (None, None, self.state[layer]), separable=False)

    def _head_terms(self, layer, phi: Tensor, what: str) -> HeadTerms:
        # sample = U_G (Z * inv) U_A^T: Cov(f) = U_G diag(w) U_G^T, w[a] = sum_b inv[a, b]^2 (U_A^T phi~)_b^2
        U_A, U_G = self.eigvecs[layer]
        inv = self.inv_state[layer]
        if U_A.dim() != 2 or U_G.dim() != 2 or inv.dim() != 2:
            raise NotImplementedError(f"{what}: stacked (grouped) factors {tuple(U_A.shape)}, {tuple(U_G.shape)}")
        N, K, dev = phi.shape[0], U_G.shape[0], phi.device
        Y = torch.empty(N, U_A.shape[1], dtype=torch.float32, device=dev)
        ops.gemm_batched([ops.Gemm(phi, U_A, Y)])
        d2 = torch.empty(N, K, dtype=torch.float32, device=dev)
        ops.gemm_batched([ops.Gemm(ops.mul(Y, Y), ops.mul(inv, inv).t(), d2)])
        variance = torch.empty(N, K, dtype=torch.float32, device=dev)
        ops.gemm_batched([ops.Gemm(d2, ops.mul2d(U_G, U_G).t(), variance)])
        return HeadTerms(U_G, False, d2, variance)

    def _head_grid_check(self, layer, what: str) -> None:
        U_A, U_G = self.eigvecs[layer]
        if U_A.dim() != 2 or U_G.dim() != 2 or self.state[layer].dim() != 2:
            raise NotImplementedError(f"{what}: stacked (grouped) factors {tuple(U_A.shape)}, {tuple(U_G.shape)}")

    def _head_grid_terms(self, layer, phi: Tensor):
        U_A, U_G = self.eigvecs[layer]
        state = self.state[layer]
        Y = torch.empty(phi.shape[0], U_A.shape[1], dtype=torch.float32, device=phi.device)
        ops.gemm_batched([ops.Gemm(phi, U_A, Y)])
        return U_G, Y, (None, None, state), False

    def sample(self, layer: Module, z: Optional[Tensor] = None) -> Tensor:
        """(U_A (z * inv^T) U_G^T)^T = U_G (z^T * inv) U_A^T -> (m, n) (curvatures.py:453-460)."""
        assert self.inv_state, "Inverse state dict is empty. Did you call 'invert' prior to this?"
        first, second = self.eigvecs[layer]
        lambdas = self.inv_state[layer]
        n, m = first.size(0), second.size(0)
        if z is None:
            z = self._randn(n, m, device=first.device)
        zt = ops.mul2d(z.t(), lambdas)                                    # (m, n)
        pt = torch.empty(n, m, dtype=torch.float32, device=first.device)
        out = torch.empty(m, n, dtype=torch.float32, device=first.device)
        ops.gemm_batched([ops.Gemm(first, zt.t(), pt)])                   # P^T = U_A zt^T (see sample_and_replace)
        ops.gemm_batched([ops.Gemm(second, pt.t(), out)])                 # U_G P
        return out

    def sample_and_replace(self, noise: Optional[Dict[Module, Tensor]] = None):
        """Fused form of the base-class loop (same result as curvatures.py:117-129 with EFB.sample): the
        scaled noise, then two batched GEMM launches for the whole model, the second writing
        ``mean + sample`` straight into the parameters.  `noise[layer]` (n, m) may be supplied.  The launches
        are described once and replayed while the tensors involved stay where they are."""
        assert self.inv_state, "Inverse state dict is empty. Did you call 'invert' prior to this?"
        layers = self._mine()
        params, param_ptrs, mean_ptrs = self._param_ptrs(layers)
        self._reload_mean(skip=params)
        if not layers:
            self._allgather_sampled()
            return
        key = (noise is None, tuple(map(Tensor.data_ptr, [t for l in layers for t in (*self.eigvecs[l], self.inv_state[l])])),
               param_ptrs, mean_ptrs)
        plan = self._sample_plans().get(key)
        if plan is None:
            invs = [self.inv_state[l] for l in layers]
            shapes = [tuple(inv.shape) for inv in invs]                             # (m, n)
            zs = _Arena(shapes, invs[0].device)
            zflat, zts = zs.flat, zs.views
            tmps = _Arena(shapes, invs[0].device).views
            stage1, stage2 = [], []
            for layer, zt, tmp in zip(layers, zts, tmps):
                first, second = self.eigvecs[layer]
                n, m = first.size(0), second.size(0)
                # U_G zt U_A^T as  P^T = U_A zt^T (n x m),  out = U_G P: both products "rows times rows" (every operand
                # contiguous along the summation index - the form the LDS-DMA GEMM kernel takes), no transposed copies
                pt = tmp.view(-1).view(n, m)
                stage1.append(ops.Gemm(first, zt.t(), pt))
                p = pt.t()                                                          # (m, n) view of P
                for live, mean in zip(_live_slots(layer), self._mean_slots(layer)):
                    stage2.append(ops.Gemm(second, p[:, live.cols], live.view, epilogue=ops.EPI_ADD_E, E=mean.view))
            _largest_first(stage1)
            _largest_first(stage2)
            # zt and inv_state are shaped alike: one launch scales the noise when inv_state is invert()'s whole arena
            whole = self._inv_arena is not None and self._inv_arena.is_whole(invs)
            plan = (key, zflat, zts, ops.GemmPlan(stage1), ops.GemmPlan(stage2), self._inv_arena.flat if whole else None)
            self._keep_plan(key, plan)
        _, zflat, zts, plan1, plan2, inv_flat = plan
        if noise is None:
            # z^T of the reference drawn directly in (m, n) layout: the transpose of iid noise is iid noise
            self._randn(zflat.numel(), device=zflat.device, out=zflat)
            if inv_flat is not None:
                ops.mul(zflat, inv_flat, out=zflat)                                 # one launch for the model
            else:
                for layer, zt in zip(layers, zts):
                    ops.mul(zt, self.inv_state[layer], out=zt)
        else:
            for layer, zt in zip(layers, zts):
                ops.mul2d(noise[layer].t(), self.inv_state[layer], out=zt)          # (m, n)
        plan1.run()
        plan2.run()
        self._allgather_sampled()


class INF(Curvature):
    """Sparse information form: low-rank eigen subset + diagonal correction (curvatures.py:463-672).

    ``state[layer] = (U_A[:, I], U_G[:, J], lambda[I x J], D)``; ``inv_state[layer] = (U_A_lr, U_G_lr, r, P_c)``.
    The (n m) x (a b) Kronecker matrix V_s of the reference's pre_sampler is never formed: V_s^T V_s is
    computed in closed form from Khatri-Rao squares, and the dense chain after it,
    L_c = (C^-1 + vtv)^-1 with C = A^-T (B - I) A^-1, A = chol(vtv), B = chol(vtv + I), is evaluated as the
    algebraically identical A^-T (I - B^-1) A^-1 in fp64 (no symmetry is assumed; P_c stays non-symmetric).

    Keyword-only extensions of the reference constructor: `shard` (only this rank's layers are decomposed,
    reduced, inverted and sampled; dicts coming from sharded estimators already hold just those) and `eigvecs`
    (reuse e.g. ``efb.eigvecs`` instead of decomposing the same factors again, curvatures.py:403 vs :473).

    The linearised predictive (`functional_variance`, `stage_output`, `functional_covariance`; opt-in:
    `ops.admit_inf_predictive`) is that of the regularised precision `invert` stands for,

        Pi = V diag(s lambda) V^T + diag(s corr + add),   V = kron(U_A, U_G),   r = (s corr + add)^(-1/2),

    whose inverse is, by Woodbury with sigma = sqrt(s lambda), S = diag(sigma), vtv = V_s^T V_s as `vtv` forms it and
    B = chol(vtv + I),  Pi^-1 = diag(r^2) - diag(r^2) V S (I + vtv)^-1 S V^T diag(r^2).  A layer's share of the variance of
    an output with per-sample Jacobian P (n x m, index i m + j) is

        sum_ij r2_ij P_ij^2 - ||F q||^2,   q = vec(U_A^T (R2 o P) U_G) in the order k b + l,   F = B^-1 S.

    This is NOT the covariance of `sampler`: the pre-sampler P_c it shares with the reference uses B^-1 B^-T where
    (B B^T)^-1 = B^-T B^-1 is needed, so the samples' covariance M M^T differs from Pi^-1 (4e-3 against entries of 1.4 on a
    random layer with n, m, a, b = 5, 4, 3, 2; tests/test_inf_predictive.py records it).  The sampler is left as it is."""

    _mha_as_projections = True

    def __init__(self, model: Union[Module, Sequential], diags: Dict[Module, Tensor],
                 factors: Dict[Module, Tensor], lambdas: Dict[Module, Tensor],
                 layer_types: Union[List[str], str] = None, *, shard=None, eigvecs=None):
        super().__init__(model, layer_types, shard=shard)
        _reject_grouped(self, "INF")
        assert diags.keys() == factors.keys() == lambdas.keys()
        if shard is not None:
            mine = {l for _, l in self._owned()}
            diags = {l: v for l, v in diags.items() if l in mine}
            factors = {l: v for l, v in factors.items() if l in mine}
            lambdas = {l: v for l, v in lambdas.items() if l in mine}
        if eigvecs is None:
            from .utils import get_eigenvectors
            eigvecs = get_eigenvectors(factors)
        self.eigvecs = eigvecs
        self.lambdas = lambdas
        self.diags = diags

    def update(self, rank: int = 100):
        layers = list(self.diags.keys())
        # lambda^T.flatten() (index i*m + j) of every layer, then the index sets of all layers in one launch and
        # one read-back (a launch + host sync per layer was a quarter of update() on ResNet-18)
        vecs = {layer: ops.gather2d(self.lambdas[layer].t()).view(-1) for layer in layers}
        need = [layer for layer in layers if rank < vecs[layer].shape[0]]
        picked = dict(zip(need, ops.inf_select_many(
            [vecs[layer] for layer in need],
            [(self.eigvecs[layer][0].shape[0], self.eigvecs[layer][1].shape[0]) for layer in need], rank)))
        stage1, stage2 = [], []
        # Lambda_lr and D of all layers live in one arena each: invert() with one pair of hyper-parameters then clamps,
        # scales and inverts them in three launches instead of three per layer
        dev = vecs[layers[0]].device if layers else None
        shapes = []
        for layer in layers:
            n, m = self.eigvecs[layer][0].shape[0], self.eigvecs[layer][1].shape[0]
            a, b = (picked[layer][0].numel(), picked[layer][1].numel()) if layer in picked else (n, m)
            shapes.append((n, m, a, b))
        self._corr_arena = self._lam_arena = None
        corrs = lams = ()
        if layers:
            self._corr_arena = _Arena([(n, m) for n, m, _, _ in shapes], dev)
            self._lam_arena = _Arena([(a * b,) for _, _, a, b in shapes], dev)
            corrs, lams = self._corr_arena.views, self._lam_arena.views
        for layer, corr, lam in zip(layers, corrs, lams):
            xxt_eigvecs, ggt_eigvecs = self.eigvecs[layer]
            n, m = xxt_eigvecs.shape[0], ggt_eigvecs.shape[0]
            lambda_vec = vecs[layer]
            diag_vec = ops.gather2d(self.diags[layer].t())                          # (n, m): index i*m + j
            if layer not in picked:
                ua, ug = xxt_eigvecs, ggt_eigvecs
                lam.copy_(lambda_vec)
            else:
                I, J = picked[layer]
                ua = ops.gather2d(xxt_eigvecs, cols=I)
                ug = ops.gather2d(ggt_eigvecs, cols=J)
                ops.gather2d(lambda_vec.view(n, m), rows=I, cols=J, out=lam)
            a, b = ua.shape[1], ug.shape[1]
            # D = diag_vec - ((U_A**2) Lambda_lr (U_G**2)^T).flatten()
            ua2, ug2 = ops.mul(ua, ua), ops.mul(ug, ug)
            tmp = torch.empty(n, b, dtype=torch.float32, device=ua.device)
            stage1.append(ops.Gemm(ua2, lam.view(a, b), tmp))
            stage2.append(ops.Gemm(tmp, ug2.t(), corr, alpha=-1.0, epilogue=ops.EPI_ADD_E, E=diag_vec))
            self.state[layer] = (ua, ug, lam, corr.view(-1))
        ops.gemm_batched(stage1)
        ops.gemm_batched(stage2)
        self.__dict__.pop("_sample_plan_cache", None)

    def invert(self, add: Union[float, list, tuple] = 0., multiply: Union[float, list, tuple] = 1.):
        assert self.state, "State dict is empty. Did you call 'update' prior to this?"
        # All layers advance together through the stages of pre_sampler (:538-572): one batched launch per GEMM
        # stage, ONE batched fp64 factorisation sweep for the 2 x layers matrices vtv and vtv + I (and one
        # status read-back) instead of a sweep and a host synchronisation per layer.
        layers, regs = list(self.state.keys()), []
        gindex = self._global_index()
        # r of all layers in one arena, overwritten in place by later calls (stable addresses for the sampler's plan)
        rs = [self.inv_state[l][2] for l in layers] if len(self.inv_state) == len(layers) else []
        if self._r_arena is None or not self._r_arena.is_whole(rs) or \
                any(r.numel() != self.state[l][3].numel() for r, l in zip(rs, layers)):
            self._r_arena = _Arena([(self.state[l][3].numel(),) for l in layers], self.state[layers[0]][3].device)
            rs = self._r_arena.views
        hypers = [self._hyper(add, multiply, gindex.get(layer, position), max(len(gindex), len(layers)))
                  for position, layer in enumerate(layers)]
        corrs, lams = self._corr_arena, self._lam_arena
        # (the r of the layers are a whole arena, each as long as its layer's D, after the block above: as long as `corrs`)
        one_pair = len(set(hypers)) == 1 and \
            corrs is not None and corrs.is_whole([self.state[l][3] for l in layers]) and \
            lams is not None and lams.is_whole([self.state[l][2] for l in layers])
        if one_pair:
            # the three elementwise steps of :521-530 over the arenas of update(): three launches for the whole model
            n, s = hypers[0]
            ops.clamp_min0_(corrs.flat)                                  # in place on `state`, like :523
            reg_flat = ops.sqrt_scale(lams.flat, s)
            ops.rsqrt_affine(corrs.flat, n, s, out=self._r_arena.flat)
            pos = 0
            for layer, r in zip(layers, rs):
                lr_frst_eigvecs, lr_scnd_eigvecs, lr_lambda, _ = self.state[layer]
                regs.append((lr_frst_eigvecs, lr_scnd_eigvecs, reg_flat[pos:pos + lr_lambda.numel()], r))
                pos += lr_lambda.numel()
        else:
            for (n, s), layer, r in zip(hypers, layers, rs):
                lr_frst_eigvecs, lr_scnd_eigvecs, lr_lambda, correction = self.state[layer]
                ops.clamp_min0_(correction)                              # in place on `state`, like :523
                reg_lr_lambda = ops.sqrt_scale(lr_lambda, s)
                ops.rsqrt_affine(correction, n, s, out=r)
                regs.append((lr_frst_eigvecs, lr_scnd_eigvecs, reg_lr_lambda, r))
        self._r_version = getattr(self, "_r_version", 0) + 1            # (the sampler's cached r**2 is stale)
        prev = [self.inv_state[l][3] if l in self.inv_state else None for l in layers]
        pre_samples = self.pre_sampler_many(regs, outs=prev)
        self._sigma = dict()                                             # sqrt(s lambda) per layer: the predictive's F = B^-1 S
        for layer, (ua, ug, sigma, r), pre_sample in zip(layers, regs, pre_samples):
            self.inv_state[layer] = (ua, ug, r, pre_sample)
            self._sigma[layer] = sigma

    def _log_det_parts(self, hypers):
        # det Pi = det diag(s corr+ + n) det(I + vtv) with vtv as `invert` forms it from sigma = sqrt(s lambda) and
        # r = (s corr+ + n)^(-1/2), and log det(I + vtv) = 2 sum log diag(B) = -2 sum log diag(B^-1), B = chol(vtv + I).
        # Everything on scratch: `invert` clamps `state`'s correction in place, this works on a clamped copy
        layers, resolved = list(self.state), self._resolved(hypers)
        corrs = self._corr_arena
        if corrs is not None and corrs.is_whole([self.state[l][3] for l in layers]):
            flat, plus, pos = ops.clamp_min0_(corrs.flat.clone()), [], 0
            for l in layers:
                plus.append(flat[pos:pos + self.state[l][3].numel()])
                pos += plus[-1].numel()
        else:
            plus = [ops.clamp_min0_(self.state[l][3].clone()) for l in layers]
        rows, total = ops.logsum_grid([ops.LogSumSegment.of(c, 1.0, [s for _, s in points], [n for n, _ in points])
                                       for c, (_, points) in zip(plus, resolved)], len(hypers))
        infos = []
        for h in range(len(hypers)):
            regs = []
            for l, c, (_, points) in zip(layers, plus, resolved):
                n, s = points[h]
                regs.append((self.state[l][0], self.state[l][1], ops.sqrt_scale(self.state[l][2], s), ops.rsqrt_affine(c, n, s)))
            for group in self._scratch_groups(regs):
                vtvs = self._vtv_many([regs[k] for k in group])
                invB = ops.chol_factor_inverse(vtvs, [1.0] * len(vtvs), check=False)
                infos.append(ops.chol_factor_inverse.last_info)
                part, part_total = ops.logsum_grid([ops.LogSumSegment.of(B.diagonal(), -2.0, [1.0], [0.0]) for B in invB], 1)
                rows[torch.tensor(group, device=rows.device), h] += part[:, 0]
                total[h] += part_total[0]
        ops.check_factor_inverse_info(torch.cat(infos))                  # one read-back for the call
        return rows, total

    # ------------------------------------------------------------------ linearised (GLM) predictive (opt-in)
    def _opt_in_predictive(self):
        """`Curvature._opt_in_predictive`: with `ops.admit_inf_predictive` on, the four methods of the linearised predictive
        run `LinearisedPredictive` on this estimator (`_INFPredictive`); off - the default - they are `Curvature`'s refusals,
        reached before any attribute of the estimator is touched.  Per layer ``sum r2 P**2`` by
        `ops.per_sample_quad_reduce` minus ``||F q||**2`` with q from `ops.per_sample_project` (the class docstring);
        `stage_output` also writes the output's vectors ``F q_n`` into slot `slot` of a (count, N, a b) stack per layer, and
        `functional_covariance` is `ops.per_sample_cov_reduce` with W = r**2 minus the Gram of those stacks.  Layers,
        records and ``inputs=False`` as for EFB.  `functional_variance_grid` stays refused: a damping pair changes r and with
        it V_s^T V_s, so every pair needs a factorisation of its own."""
        return _INFPredictive(self) if ops.inf_predictive_admitted() else None

    def _lowrank_terms(self) -> dict:
        """``{layer: (U_A, U_G, F^T)}`` for the current inversion, F = B^-1 S with B = chol(vtv + I) and its columns in the
        order l a + k (the order in which the projected products come out of their GEMM; `LinearisedPredictive._lowrank`).
        Built at the first predictive call after an inversion (all layers together through the stages: `_vtv_many`, one
        float64 factorisation sweep, one float64 product that scales and rounds to float32), kept with the predictive's
        other state: `drop_predictive_state` drops it."""
        state = self.__dict__.setdefault("_predictive_kept", {})
        kept = state.get("lowrank")
        if kept is not None and kept["version"] == self._r_version:
            return kept["terms"]
        layers = list(self.inv_state)
        regs = [(self.inv_state[l][0], self.inv_state[l][1], self._sigma[l], self.inv_state[l][2]) for l in layers]
        terms, infos = dict(), []
        for group in self._scratch_groups(regs):
            vtvs = self._vtv_many([regs[k] for k in group])
            invB = ops.chol_factor_inverse(vtvs, [1.0] * len(vtvs), check=False)
            infos.append(ops.chol_factor_inverse.last_info)
            jobs = []
            for k, inv in zip(group, invB):
                ua, ug, sigma, _ = regs[k]
                a, b = ua.shape[1], ug.shape[1]
                # column l a + k of the result is column k b + l of B^-1 S: a permutation as the B operand, sigma in
                # the permuted order as the column scale
                order = torch.arange(a * b, device=ua.device).view(a, b).t().reshape(-1)
                perm = torch.zeros(a * b, a * b, dtype=torch.float64, device=ua.device)
                perm[order, torch.arange(a * b, device=ua.device)] = 1.0
                F = torch.empty(a * b, a * b, dtype=torch.float32, device=ua.device)
                jobs.append(ops.Gemm64(inv, perm, tri=ops.TRI64_A_LOWER, out32=F,
                                       col_scale=ops.gather2d(sigma.view(a, b).t()).view(-1)))
                terms[layers[k]] = (ua, ug, F.t())
            ops.gemm_f64_batched(jobs)
        ops.check_factor_inverse_info(torch.cat(infos))
        state["lowrank"] = dict(version=self._r_version, terms=terms)
        return terms

    def _predictive_terms(self) -> PredictiveTerms:
        def weights(layer):                                  # r (index i m + j) as the (m, n) matrix of the products' entries
            ua, ug, r, _ = self.inv_state[layer]
            return ops.gather2d(r.view(ua.shape[0], ug.shape[0]).t())
        return PredictiveTerms("INF", basis=None, weights=weights, grid_basis=None, spectrum=None, separable=False,
                               grid_missing="not supported", lowrank=lambda layer: self._lowrank_terms()[layer])

    RHS_SWEEP_ABOVE = 16        # layers per call from which T is built by the sweep's right-hand side mode (pre_sampler_many)

    @staticmethod
    def _scratch_groups(regs) -> List[List[int]]:
        """The positions of `regs` in groups whose float64 scratch (PA, M, V4, vtv, the two inverses, T, L_c per layer)
        stays below ~24 GB, far below the 288 GB of the device."""
        def scratch(reg):
            (n, a), (m, b) = reg[0].shape, reg[1].shape
            return 8.0 * (n * a * a / 2 + m * b * b / 2 + n * m + a * a * m / 2 + 6.0 * (a * b) ** 2)
        groups, cur, size = [], [], 0.0
        for k, reg in enumerate(regs):
            if cur and size + scratch(reg) > 24e9:
                groups.append(cur)
                cur, size = [], 0.0
            cur.append(k)
            size += scratch(reg)
        groups.append(cur)
        return groups

    @staticmethod
    def _vtv_many(regs) -> List[Tensor]:
        """`vtv` for a list of (U_A_lr, U_G_lr, sigma, r) tuples, stage by stage, float64."""
        first, parts = [], []
        # r**2 in fp64: one launch for the model when the r of its layers lie back to back (invert()'s arena)
        # (bare tensors here, no arena to ask: the tensor-level check `_Arena.is_whole` is built on)
        r_run = _run_of([reg[3] for reg in regs]) if len(regs) > 1 else None
        r2_flat = ops.square_f64(r_run) if r_run is not None else None
        pos = 0
        for ua, ug, sigma, r in regs:
            (n, a), (m, b) = ua.shape, ug.shape
            # distinct column pairs only (i <= k): (n, a (a + 1) / 2), (m, b (b + 1) / 2) - half the flops of the first
            # product, a quarter of the second, the same values
            PA, PG = ops.colpairs_sym(ua), ops.colpairs_sym(ug)
            r2 = (r2_flat[pos:pos + n * m] if r2_flat is not None else ops.square_f64(r)).view(n, m)
            pos += n * m
            first.append(ops.Gemm64(PA.t(), r2))
            parts.append((PG, sigma, a, b))
        Ms = ops.gemm_f64_batched(first)
        V4s = ops.gemm_f64_batched([ops.Gemm64(M, PG) for M, (PG, _, _, _) in zip(Ms, parts)])
        return [ops.inf_vtv_assemble_sym(V4.contiguous(), sigma, a, b) for V4, (_, sigma, a, b) in zip(V4s, parts)]

    @staticmethod
    def pre_sampler_many(regs, outs: Optional[Sequence[Optional[Tensor]]] = None) -> List[Tensor]:
        """`pre_sampler` for a list of (U_A_lr, U_G_lr, sigma, r) tuples, stage by stage.  `outs`: previous
        P_c tensors, overwritten in place where the shape still fits."""
        if not regs:
            return []
        # bound the float64 scratch of a batch: layers are processed in groups (`_scratch_groups`)
        if len(regs) > 1:
            groups = INF._scratch_groups(regs)
            if len(groups) > 1:
                res: List[Optional[Tensor]] = [None] * len(regs)
                for g in groups:
                    part = INF.pre_sampler_many([regs[k] for k in g], [outs[k] for k in g] if outs is not None else None)
                    for k, t in zip(g, part):
                        res[k] = t
                return res
        # V_s^T V_s in closed form, fp64 end to end: with strongly varying r (e.g. invert(1, 1000) on a ResNet) it is a
        # badly conditioned weighted Gram matrix, and an fp32 evaluation caps P_c - and the samples - at ~1e-3
        # (measured on ResNet-50's stem: 1.7e-3; with fp64: at the level of the fp32 inputs)
        vtvs = INF._vtv_many(regs)
        # float64, lower triangular: A^-1 = chol(vtv)^-1, then T = (I - B^-1) A^-1 = A^-1 - chol(vtv + I)^-1 A^-1 by forward
        # substitution INSIDE the second sweep (`rhs`): no explicit B^-1, no product with it (a sixth of the call's flops).
        # The status words are read at the END of this function: a read-back here would leave the GPU idle while the
        # launches below are described and enqueued (14 of 115 ms on ResNet-50)
        if len(vtvs) > INF.RHS_SWEEP_ABOVE:
            invA = ops.chol_factor_inverse(vtvs, [0.0] * len(vtvs), check=False)
            info = ops.chol_factor_inverse.last_info
            Ts = ops.chol_factor_inverse(vtvs, [1.0] * len(vtvs), check=False, rhs=invA, rhs_minus=True)
            info = torch.cat([info, ops.chol_factor_inverse.last_info])
        else:
            # few layers (a small model, a layer-sharded rank): such a sweep is bound by its chain, and the chain-bound
            # kernels have no right-hand side form - both inverses explicitly in ONE sweep, then the product (its epilogue
            # reads A^-1 as the E operand)
            mats, adds = [], []
            for v in vtvs:
                mats += [v, v]
                adds += [0.0, 1.0]
            both = ops.chol_factor_inverse(mats, adds, check=False)
            info = ops.chol_factor_inverse.last_info
            invA = [both[2 * i] for i in range(len(vtvs))]
            Ts = [torch.empty_like(a) for a in invA]
            ops.gemm_f64_batched([ops.Gemm64(both[2 * i + 1], invA[i], T, alpha=-1.0, beta=1.0, E=invA[i],
                                             tri=ops.TRI64_A_LOWER | ops.TRI64_B_LOWER) for i, T in enumerate(Ts)])
        inv = [None] * (2 * len(regs))
        for i, a in enumerate(invA):
            inv[2 * i] = a
        out = []
        for i, (_, _, sigma, _) in enumerate(regs):
            prev = outs[i] if outs is not None else None
            shape = tuple(Ts[i].shape)
            if prev is None or tuple(prev.shape) != shape or prev.dtype != torch.float32 or prev.device != Ts[i].device \
                    or not prev.is_contiguous():
                prev = torch.empty(shape, dtype=torch.float32, device=Ts[i].device)
            out.append(prev)
        ops.gemm_f64_batched([ops.Gemm64(inv[2 * i].t(), T, tri=ops.TRI64_A_UPPER | ops.TRI64_B_LOWER, out32=out[i],
                                         row_scale=regs[i][2].contiguous(), col_scale=regs[i][2].contiguous())
                              for i, T in enumerate(Ts)])
        ops.check_factor_inverse_info(info)                              # RuntimeError where curvatures.py:566-567 raises: inside invert()
        return out

    @staticmethod
    def vtv(frst_eigvecs: Tensor, scnd_eigvecs: Tensor, reg_lambda: Tensor, reg_inv_correction: Tensor) -> Tensor:
        """V_s^T V_s, symmetrised, in closed form (no Kronecker matrix), evaluated in float64."""
        (n, a), (m, b) = frst_eigvecs.shape, scnd_eigvecs.shape
        PA, PG = ops.colpairs_sym(frst_eigvecs), ops.colpairs_sym(scnd_eigvecs)
        r2 = ops.square_f64(reg_inv_correction).view(n, m)
        M = ops.gemm_f64(PA.t(), r2)
        V4 = ops.gemm_f64(M, PG)
        return ops.inf_vtv_assemble_sym(V4.contiguous(), reg_lambda, a, b)

    @staticmethod
    def pre_sampler(frst_eigvecs: Tensor, scnd_eigvecs: Tensor, reg_lambda: Tensor,
                    reg_inv_correction: Tensor) -> Tensor:
        """P_c of one layer (curvatures.py:538-572)."""
        return INF.pre_sampler_many([(frst_eigvecs, scnd_eigvecs, reg_lambda, reg_inv_correction)])[0]

    def sample(self, layer: Module, X: Optional[Tensor] = None) -> Tensor:
        assert self.inv_state, "Inverse state dict is empty. Did you call 'invert' prior to this?"
        a, b, c, d = self.inv_state[layer]
        return self.sampler(a, b, c, d, X=X, randn=self._randn).t()

    def sample_and_replace(self, noise: Optional[Dict[Module, Tensor]] = None):
        """The base-class loop (curvatures.py:117-129) with INF.sample, all layers advancing together through the
        five products of `sampler` (one batched launch each); the last one writes
        ``mean + (Y_l - Y_r)^T`` straight into the parameters through its output strides.  `noise[layer]`: the
        (n*m,) vector X of :578.  Launches are described once and replayed while the tensors stay in place."""
        assert self.inv_state, "Inverse state dict is empty. Did you call 'invert' prior to this?"
        layers = [l for _, l in self._owned() if l in self.inv_state]
        self._reload_mean()                                   # the last product accumulates onto the mean
        if not layers:
            self._allgather_sampled()
            return
        # (no mean addresses: the last product accumulates onto the parameters, which _reload_mean has just reset)
        key = (tuple(map(Tensor.data_ptr, [t for l in layers for t in self.inv_state[l]])), self._param_ptrs(layers, means=False)[1])
        plan = self._sample_plans().get(key)
        if plan is None:
            dev = self.inv_state[layers[0]][0].device
            dims = [(self.inv_state[l][0].shape, self.inv_state[l][1].shape) for l in layers]
            vecs = [(n * m,) for (n, _), (m, _) in dims]
            xs, ys, r2 = _Arena(vecs, dev), _Arena(vecs, dev), _Arena([(n, m) for (n, _), (m, _) in dims], dev)
            xflat, Xs, yflat, Ys, r2flat, r2s = xs.flat, xs.views, ys.flat, ys.views, r2.flat, r2.views
            small = []
            for (n, a), (m, b) in dims:
                small += [(b, n), (a, b), (a * b, 1), (m, a)]
            sm = _Arena(small, dev).views
            stages = [[], [], [], [], []]
            for k, (layer, ((n, a), (m, b)), Y_l, r2) in enumerate(zip(layers, dims, Ys, r2s)):
                ua, ug, r, P = self.inv_state[layer]
                t1, xq_t, qx, t2 = sm[4 * k:4 * k + 4]
                stages[0].append(ops.Gemm(ug.t(), Y_l.view(m, n), t1))               # U_G^T unvec(Y_l): (b, n)
                stages[1].append(ops.Gemm(t1, ua, xq_t.t()))                         # flat order of Xq^T: k*b + l
                stages[2].append(ops.Gemm(P, xq_t.view(a * b, 1), qx))
                stages[3].append(ops.Gemm(ug, qx.view(b, a), t2))                    # U_G unvec(Qx): (m, a)
                # (Y_l - r^2 * (U_A t2^T)) as an (n, m) matrix is the transposed sample: rows < n0 go to the
                # weight seen through transposed strides, the last row to the bias (curvatures.py:67-82, 536)
                Yv = Y_l.view(n, m)
                for slot in _live_slots(layer):
                    # the slot's columns of Wm are rows here; a single column (the bias) is written as the plain row it is,
                    # strides (m, 1) rather than the (1, 1) of the transposed (m, 1) view
                    dst = slot.view.t()
                    if dst.shape[0] == 1:
                        dst = dst.reshape(1, m)
                    stages[4].append(ops.Gemm(ua[slot.cols], t2.t(), dst, alpha=-1.0, beta=1.0,
                                              epilogue=ops.EPI_MUL_E_ADD_F, E=r2[slot.cols], F=Yv[slot.cols]))
            # X, Y_l and r are as long as each other: one launch each over the model when r is invert()'s whole arena
            r_whole = self._r_arena is not None and self._r_arena.is_whole([self.inv_state[l][2] for l in layers])
            plan = (key, xflat, Xs, yflat, Ys, r2flat, r2s, [ops.GemmPlan(st) for st in stages],
                    self._r_arena.flat if r_whole else None, [None])   # (last: the inversion whose r**2 `r2flat` holds)
            self._keep_plan(key, plan)
        _, xflat, Xs, yflat, Ys, r2flat, r2s, gemms, r_flat, r2_of = plan
        if noise is None:
            self._randn(xflat.numel(), device=xflat.device, out=xflat)
        else:
            ops.CopyPlan(Xs, [noise[l].reshape(-1).contiguous() for l in layers]).run()
        if r_flat is not None:                                  # Y_l = r * X and r^2 for the whole model
            ops.mul(r_flat, xflat, out=yflat)
            if r2_of[0] != getattr(self, "_r_version", 0):       # r changes with invert() only: r^2 once per inversion
                ops.mul(r_flat, r_flat, out=r2flat)
                r2_of[0] = getattr(self, "_r_version", 0)
        else:
            for layer, X, Y_l, r2 in zip(layers, Xs, Ys, r2s):
                r = self.inv_state[layer][2]
                ops.mul(r, X, out=Y_l)
                ops.mul(r, r, out=r2.view(-1))
        for g in gemms:
            g.run()
        self._allgather_sampled()

    @staticmethod
    def sampler(frst_eigvecs: Tensor, scnd_eigvecs: Tensor, reg_inv_correction: Tensor, pre_sample: Tensor,
                X: Optional[Tensor] = None, randn=None) -> Tensor:
        """(Y_l - Y_r) as an (n, m) matrix (the reference returns it flat and reshapes in `sample`,
        curvatures.py:532-536, 574-600; reshape conventions reproduced literally)."""
        (n, a), (m, b) = frst_eigvecs.shape, scnd_eigvecs.shape
        dev = frst_eigvecs.device
        if X is None:
            X = randn(n * m, device=dev) if randn is not None else ops.randn((n * m,), dev, 0)
        Y_l = ops.mul(reg_inv_correction, X)                                   # (n*m,)
        t1 = torch.empty(b, n, dtype=torch.float32, device=dev)
        ops.gemm_batched([ops.Gemm(scnd_eigvecs.t(), Y_l.view(m, n), t1)])      # U_G^T unvec(Y_l): (b, n)
        xq_t = torch.empty(a, b, dtype=torch.float32, device=dev)               # Xq^T, so that its flat order is k*b + l
        ops.gemm_batched([ops.Gemm(t1, frst_eigvecs, xq_t.t())])
        qx = torch.empty(a * b, 1, dtype=torch.float32, device=dev)
        ops.gemm_batched([ops.Gemm(pre_sample, xq_t.view(a * b, 1), qx)])
        t2 = torch.empty(m, a, dtype=torch.float32, device=dev)
        ops.gemm_batched([ops.Gemm(scnd_eigvecs, qx.view(b, a), t2)])           # U_G unvec(Qx): (m, a)
        out = torch.empty(n, m, dtype=torch.float32, device=dev)
        r2 = ops.mul(reg_inv_correction, reg_inv_correction).view(n, m)
        # X_p_s = t2 U_A^T (m, n); Y_r[i*m + q] = r^2[i*m + q] X_p_s[q, i]: write X_p_s^T through the strides
        ops.gemm_batched([ops.Gemm(frst_eigvecs, t2.t(), out, alpha=-1.0, epilogue=ops.EPI_MUL_E_ADD_F, E=r2,
                                   F=Y_l.view(n, m))])
        return out


class _INFPredictive(LinearisedPredictive):
    """`LinearisedPredictive` on an `INF` it does not derive from: INF's four methods stay `Curvature`'s own (refusals with
    `ops.admit_inf_predictive` off), which hand over to an object of this class with the switch on
    (`INF._opt_in_predictive`).  Everything the mixin asks of its estimator - state, records, hooks, `_predictive_terms`,
    the kept state - is the INF's: nothing lives here but the reference."""

    def __init__(self, inf: INF):
        object.__setattr__(self, "_inf", inf)

    def __getattr__(self, name):                   # (only what the mixin itself does not define)
        return getattr(object.__getattribute__(self, "_inf"), name)

    def _kept(self) -> dict:
        return self._inf.__dict__.setdefault("_predictive_kept", {})

    def functional_variance_grid(self, out: Tensor, hypers, *, first: bool = True, inputs: bool = True) -> Tensor:
        raise NotImplementedError("INF.functional_variance_grid: a damping pair changes r and V_s^T V_s, so every pair needs "
                                  "its own factorisation; call invert(add, multiply) and functional_variance per pair")
