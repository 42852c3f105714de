"""The two pieces every fused sampler is built on, on CPU tensors: `_slots`, the one map from the columns of a layer's
[W | b] matrix (Wm order) to its parameter storage, and `_Arena`, the flat buffer that knows what it handed out."""
import pytest
import torch
import torch.nn as nn

from curvature_amd.curvatures import AttentionProjection, Curvature, _Arena, _bank_buffers, _live_slots, _run_of, _slots, _wm, \
    _wm_rows

LAYERS = {
    "linear": lambda: nn.Linear(5, 3),
    "linear_nobias": lambda: nn.Linear(5, 3, bias=False),
    "conv": lambda: nn.Conv2d(3, 4, (3, 2)),
    "conv_nobias": lambda: nn.Conv2d(3, 4, (3, 2), bias=False),
    "grouped": lambda: nn.Conv2d(4, 6, 3, groups=2),
    "depthwise_nobias": lambda: nn.Conv2d(4, 4, 3, groups=4, bias=False),
    "convt": lambda: nn.ConvTranspose2d(4, 3, (3, 2)),
    "convt_nobias": lambda: nn.ConvTranspose2d(4, 3, (2, 3), bias=False),
    "attn_in": lambda: AttentionProjection.of(nn.MultiheadAttention(6, 2))[0],
    "attn_out": lambda: AttentionProjection.of(nn.MultiheadAttention(6, 2))[1],
}


def _columns(layer):
    return layer.weight.numel() // _wm_rows(layer) + int(layer.bias is not None)


@pytest.mark.parametrize("kind", LAYERS)
def test_slots_cover_every_column_once_and_write_wm(kind):
    torch.manual_seed(0)
    layer = LAYERS[kind]()
    m, n = _wm_rows(layer), _columns(layer)
    weight = torch.zeros_like(layer.weight)
    bias = torch.zeros_like(layer.bias) if layer.bias is not None else None
    slots = _slots(layer, weight, bias)
    seen = torch.zeros(n, dtype=torch.int64)
    for slot in slots:
        seen[slot.cols] += 1
        assert tuple(slot.view.shape) == (m, len(range(*slot.cols.indices(n))))
    assert torch.equal(seen, torch.ones(n, dtype=torch.int64))
    if bias is not None:                                           # the bias is the last slot, Wm's last column
        assert slots[-1].cols == slice(n - 1, n) and slots[-1].view.data_ptr() == bias.data_ptr()
    # writing a random matrix through the slots is writing Wm: `_wm` reads the weight columns back, the bias is the rest
    sample = torch.randn(m, n)
    for slot in slots:
        slot.view.copy_(sample[:, slot.cols])
    n0 = n - int(bias is not None)
    assert torch.equal(_wm(layer, weight), sample[:, :n0])
    if bias is not None:
        assert torch.equal(bias, sample[:, n0])
    # only an ordinary layer's weight is Wm's leading column block stored as it is
    lead = [slot.lead for slot in slots]
    assert lead == ([False] * len(slots) if kind.startswith("convt") else [True] + [False] * (len(slots) - 1))


@pytest.mark.parametrize("kind", ["grouped", "depthwise_nobias"])
def test_grouped_row_blocks(kind):
    layer = LAYERS[kind]()
    G, rows = layer.groups, _wm_rows(layer)
    m = rows // G
    weight, bias = layer.weight.data, layer.bias.data if layer.bias is not None else None
    slots = _slots(layer, weight, bias)
    n0 = weight.numel() // rows
    for g in range(G):
        block = slots[0].view[g * m:(g + 1) * m]
        want = weight.view(G, m, n0)[g]
        assert (block.shape, block.stride(), block.storage_offset()) == (want.shape, want.stride(), want.storage_offset())
        if bias is not None:
            block, want = slots[1].view[g * m:(g + 1) * m], bias.view(G, m, 1)[g]
            assert (block.shape, block.stride(), block.storage_offset()) == (want.shape, want.stride(), want.storage_offset())


def test_convt_tap_strides_and_live_slots():
    layer = LAYERS["convt"]()                                      # weight (4, 3, 3, 2): kh kw = 6, out = 3
    slots = _live_slots(layer)
    assert len(slots) == 7
    for k, slot in enumerate(slots[:6]):
        assert slot.cols == slice(k, 24, 6)
        assert (tuple(slot.view.shape), slot.view.stride(), slot.view.storage_offset()) == ((3, 4), (6, 18), k)
        assert slot.view.data_ptr() == layer.weight.data_ptr() + 4 * k
    assert slots[6].view.data_ptr() == layer.bias.data_ptr()


@pytest.mark.parametrize("kind", LAYERS)
def test_replace_layer_adds_the_sample_in_wm_order(kind):
    torch.manual_seed(1)
    layer = LAYERS[kind]()
    m, n = _wm_rows(layer), _columns(layer)
    n0 = n - int(layer.bias is not None)
    w0 = layer.weight.detach().clone()
    b0 = layer.bias.detach().clone() if layer.bias is not None else None
    sample = torch.randn(m, n)
    Curvature._replace_layer(sample, layer)
    assert torch.equal(_wm(layer, layer.weight.detach()), _wm(layer, w0) + sample[:, :n0])
    if b0 is not None:
        assert torch.equal(layer.bias.detach(), b0 + sample[:, n0])


@pytest.mark.parametrize("kind,shape", [("conv", (5, 4, 18)), ("grouped", (5, 6, 18)), ("convt", (5, 4, 3, 3, 2)),
                                        ("linear_nobias", (5, 3, 5))])
def test_bank_buffers(kind, shape):
    layer = LAYERS[kind]()
    weights, biases = _bank_buffers(layer, 5, torch.device("cpu"))
    assert tuple(weights.shape) == shape and weights.dtype == torch.float32
    assert (biases is None) == (layer.bias is None)
    if biases is not None:
        assert tuple(biases.shape) == (5, _wm_rows(layer))
    slots = _slots(layer, weights[2], biases[2] if biases is not None else None)
    mine = _live_slots(layer)
    assert [(s.cols, s.view.shape, s.view.stride()) for s in slots] == [(s.cols, s.view.shape, s.view.stride()) for s in mine]


def test_arena_is_whole():
    shapes = [(3, 4), (5,), (2, 1, 2)]
    arena = _Arena(shapes, torch.device("cpu"))
    assert [tuple(v.shape) for v in arena.views] == shapes and arena.flat.numel() == arena.total == 21
    assert arena.views[1].data_ptr() == arena.flat.data_ptr() + 4 * 12
    views = arena.views
    assert arena.is_whole(views)
    assert arena.is_whole([v.view(-1) for v in views])                 # the same memory under another shape
    assert not arena.is_whole([views[1], views[0], views[2]])         # permuted
    assert not arena.is_whole(views[:2])                              # a strict prefix
    assert not arena.is_whole(views[1:])                              # a strict suffix
    assert not arena.is_whole([views[0], views[1].clone(), views[2]])  # a clone of one view
    assert not arena.is_whole([views[0].t(), views[1], views[2]])     # a non-contiguous view
    assert not arena.is_whole([views[0], views[1], views[2].double()])
    other = _Arena(shapes, torch.device("cpu"))
    assert not arena.is_whole(other.views) and other.is_whole(other.views)   # views of a second arena
    assert not arena.is_whole([])
    assert _Arena(shapes, torch.device("cpu"), zero=True).flat.eq(0).all()


def test_arena_without_views():
    """A layer-sharded rank can own nothing: one element, no views, and never whole (the caller's per-layer loop, which
    is then empty, is the branch that runs)."""
    arena = _Arena([], torch.device("cpu"))
    assert arena.flat.numel() == 1 and arena.views == [] and arena.total == 0
    assert not arena.is_whole([])
    assert not arena.is_whole([arena.flat])


def test_run_of():
    flat = torch.arange(12, dtype=torch.float32)
    a, b, c = flat[:4].view(2, 2), flat[4:6], flat[6:12].view(3, 2)
    run = _run_of([a, b, c])
    assert run.data_ptr() == flat.data_ptr() and torch.equal(run, flat)
    assert torch.equal(_run_of([b, c]), flat[4:])
    assert _run_of([]) is None
    assert _run_of([a, c]) is None                                    # a gap
    assert _run_of([b, a]) is None                                    # out of order
    assert _run_of([a, b.double()]) is None
    assert torch.equal(_run_of([b]), b)
