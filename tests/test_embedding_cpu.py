"""nn.Embedding without a GPU: the switch, the selection, every refusal by the layer's name, the jobs
`ops.factor_jobs` hands out for `ShapeOnly` records and their price, the per-sample route, the position-list planner against
a brute-force grouping in Python on the index sets of the kernel tests, and the host-only side of the C ABI."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from curvature_amd import _lib, ops
from curvature_amd.curvatures import EFB, INF, KFAC, BlockDiagonal, Diagonal
from curvature_amd.graph import KFACStepGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Net(nn.Module):
    def __init__(self, **kwargs):
        super().__init__()
        self.emb = nn.Embedding(11, 6, **kwargs)
        self.fc = nn.Linear(6, 4)

    def forward(self, idx):
        return self.fc(self.emb(idx).mean(1))


class Tied(nn.Module):
    """A language-model head that shares the embedding's weight."""

    def __init__(self):
        super().__init__()
        self.emb = nn.Embedding(11, 6)
        self.lm_head = nn.Linear(6, 11, bias=False)
        self.lm_head.weight = self.emb.weight

    def forward(self, idx):
        return self.lm_head(self.emb(idx).mean(1))


@pytest.fixture
def on():
    was = ops.admit_embedding(True)
    yield
    ops.admit_embedding(was)


def test_switch_is_off_by_default_and_returns_what_it_was():
    assert not ops.embedding_admitted()
    model = Net()
    for build in (lambda t: KFAC(model, t), lambda t: Diagonal(model, t), lambda t: BlockDiagonal(model, t),
                  lambda t: EFB(model, {}, t), lambda t: INF(model, {}, {}, {}, t)):
        with pytest.raises(AssertionError):
            build(['Embedding'])
    assert ops.per_sample_route(model.emb) == "whole" and not ops.is_embedding_layer(model.emb)
    assert ops.admit_embedding(True) is False and ops.embedding_admitted()
    assert ops.admit_embedding(True) is True
    assert ops.admit_embedding(False) is True and not ops.embedding_admitted()
    assert ops.admit_embedding(False) is False


def test_selected_by_name_only(on):
    from curvature_amd import curvatures
    model = Net()
    assert 'Embedding' not in curvatures.SUPPORTED_LAYERS and 'Embedding' not in curvatures.OPTIONAL_LAYERS
    assert KFAC(model)._layers() == [model.fc] and Diagonal(model)._layers() == [model.fc]
    assert KFAC(model, ['Embedding', 'Linear'])._layers() == [model.emb, model.fc]
    assert Diagonal(model, 'Embedding', per_sample=True)._layers() == [model.emb]
    assert ops.per_sample_route(model.emb) == "embedding" and ops.per_sample_route(model.fc) == "whole"


def test_refusals_name_the_layer(on):
    def refused(build, *words):
        with pytest.raises(NotImplementedError) as info:
            build()
        for word in ("'emb'",) + words:
            assert word in str(info.value), (word, str(info.value))

    for cls in (KFAC, Diagonal):
        refused(lambda: cls(Net(max_norm=1.0), ['Embedding']), "max_norm")
        refused(lambda: cls(Net(sparse=True), ['Embedding']), "sparse")
        refused(lambda: cls(Net(scale_grad_by_freq=True), ['Embedding']), "scale_grad_by_freq")
        refused(lambda: cls(Tied(), ['Embedding', 'Linear']), "'lm_head'", "tied")
        refused(lambda: cls(Net(), ['Embedding'], shard=_shard(2)), "shard")
        assert cls(Tied(), ['Embedding'])._layers()                      # the head not selected: nothing is shared
    single = Net()
    single.emb = nn.Embedding(1, 6)
    refused(lambda: KFAC(single, ['Embedding']), "single row")
    refused(lambda: BlockDiagonal(Net(), ['Embedding']), "Embedding")
    refused(lambda: EFB(Net(), {}, ['Embedding']), "Embedding")
    refused(lambda: INF(Net(), {}, {}, {}, ['Embedding']), "Embedding")
    refused(lambda: KFAC(Net(), ['Embedding'], approximation="reduce"), "reduce")
    # a shard assigned after construction is met at the call
    est = KFAC(Net(), ['Embedding'])
    est.shard = _shard(2)
    est.record[est.model.emb] = [torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3, 6)]
    refused(lambda: est.update(2), "shard")
    # decompose and, with it, KFAC's log-determinant; the reductions that need the joint products; graph capture
    est = KFAC(Net(), ['Embedding', 'Linear'])
    est.state[est.model.emb] = [torch.zeros(11), torch.zeros(6, 6)]
    est.inv_state[est.model.emb] = (torch.zeros(11), torch.zeros(6, 6))
    refused(est.decompose, "decompose")
    refused(lambda: est.log_det_grid([(1.0, 1.0)]), "log_det_grid")
    refused(lambda: est.stage_output(0, 2, inputs=True), "stage_output")
    refused(lambda: est.functional_variance_grid(torch.zeros(1, 2), [(1.0, 1.0)]), "functional_variance_grid")
    refused(lambda: KFACStepGraph(est), "KFACStepGraph")
    with pytest.raises(NotImplementedError, match="reduce"):
        ops.factor_jobs(est.model.emb, ops.ShapeOnly((2, 3), torch.int64), ops.ShapeOnly((2, 3, 6)), approximation="reduce")


def _shard(world):
    class Two:                                       # what the constructor reads of a curvature_amd.sharding.Shard
        rank = 0

        def owns(self, index):
            return True
    shard = Two()
    shard.world = world
    return shard


def test_factor_jobs_on_shapes_and_their_price(on):
    layer = nn.Embedding(11, 6, padding_idx=2)
    for dtype in (torch.int64, torch.int32):
        sides = ops.factor_jobs(layer, ops.ShapeOnly((4, 5), dtype), ops.ShapeOnly((4, 5, 6)))
        assert type(sides.a) is ops.EmbeddingFactorJob and type(sides.g) is ops.FactorJob
        assert (sides.n, sides.m, sides.K, sides.groups) == (11, 6, 20, 1)
        assert sides.a.src == (4, 5) and sides.a.V == 11 and sides.a.padding_idx == 2 and sides.a.i64 == (dtype == torch.int64)
        assert sides.g.src == (20, 6)
    half = ops.factor_jobs(layer, ops.ShapeOnly((4, 5), torch.int64), ops.ShapeOnly((4, 5, 6), torch.bfloat16))
    assert type(half.g) is ops.HalfFactorJob                      # a half-precision record takes the existing route
    only_g = ops.factor_jobs(layer, None, ops.ShapeOnly((2, 3, 4, 6)))
    assert only_g.a is None and only_g.K == 24
    rows = [build for build in ops.FACTOR_BUILDS if build.job is ops.EmbeddingFactorJob]
    assert len(rows) == 1 and rows[0].accumulate == "kfac_accumulate_embedding" and rows[0].symbol == "curv_kfac_embedding"
    assert ops.FACTOR_BUILDS[-2] is rows[0] and len(ops.FACTOR_BUILDS) == 9    # (a new row: the others stand as they were)
    flops = ops.factor_plan_flops([sides.g, sides.a])
    assert flops[1] == 20 + 11 and flops[0] == ops.kfac_plan_flops([sides.g])[0] > 0
    with pytest.raises(RuntimeError, match="int64 or int32"):
        ops.factor_jobs(layer, ops.ShapeOnly((4, 5), torch.float32), ops.ShapeOnly((4, 5, 6)))
    with pytest.raises(RuntimeError, match="does not match"):
        ops.factor_jobs(layer, ops.ShapeOnly((4, 5), torch.int64), ops.ShapeOnly((4, 6, 6)))


def test_kfac_update_hands_out_both_jobs(on, monkeypatch):
    """What KFAC.update asks of the builds for an Embedding: the histogram with input_weight / (N T), the flat G build with
    the scale of the one-hot twin (the expand build sees N T rows of one position), `first` once."""
    seen = []
    for build in ops.FACTOR_BUILDS:
        monkeypatch.setattr(ops, build.accumulate, lambda jobs, events=None: seen.extend(jobs))
    model = Net(padding_idx=0)
    est = KFAC(model, ['Embedding'])
    est.record[model.emb] = [torch.zeros(4, 5, dtype=torch.int64), torch.zeros(4, 5, 6)]
    est.update(4, input_weight=3.0, grad_scale=2.0)
    est.update(4, inputs=False)
    a, G = est.state[model.emb]
    assert tuple(a.shape) == (11,) and tuple(G.shape) == (6, 6)
    second, first, third = seen                                    # (each update: the builds in table order)
    assert type(first) is ops.EmbeddingFactorJob and first.dst is a and first.first and first.scale == 3.0 / 20
    assert first.padding_idx == 0
    assert type(second) is ops.FactorJob and second.dst is G and second.first and second.scale == 20 / 4.0
    assert type(third) is ops.FactorJob and not third.first and third.scale == 20.0
    est.restart_accumulation()
    est.update(4)
    assert len(seen) == 5 and seen[3].first and seen[4].first


SHAPES = {"base": (3, 5, 7), "t1": (4, 1, 5), "n1": (1, 6, 5), "one_segment": (1, 130, 3), "split_token": (3, 100, 4),
          "split_sample": (2, 300, 3), "hist_wide": (2, 12, 70)}


def _indices(name):
    N, T, V = SHAPES[name]
    idx = torch.randint(0, V, (N, T), generator=torch.Generator().manual_seed(sorted(SHAPES).index(name)))
    if name in ("one_segment", "split_token"):
        idx = torch.full((N, T), 1)
    return idx, V


def _brute(idx, V, pad, mode, split):
    N = idx.shape[0]
    flat = idx.reshape(-1).tolist()
    T = len(flat) // N
    items = [(p, v, p // T) for p, v in enumerate(flat) if 0 <= v < V and v != pad]
    items.sort(key=(lambda e: (e[1], e[2], e[0])) if mode == _lib.EMB_SQ else (lambda e: (e[2], e[1], e[0])))
    outer = [e[1] if mode == _lib.EMB_SQ else e[2] for e in items]
    chunks, mgroups, slot, i = [], [], 0, 0
    while i < len(items):
        j = i
        while j < len(items) and outer[j] == outer[i]:
            j += 1
        pieces = -(-(j - i) // split)
        if pieces > 1:
            mgroups.append([slot, slot + pieces, outer[i]])
        for k in range(pieces):
            chunks.append([i + k * split, min(i + (k + 1) * split, j), outer[i], slot if pieces > 1 else -1])
            slot += pieces > 1
        i = j
    return [e[0] for e in items], chunks, mgroups, slot


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("mode", [_lib.EMB_SQ, _lib.EMB_QUAD])
def test_walk_plan_is_the_brute_force_grouping(name, mode):
    idx, V = _indices(name)
    for pad in (None, 1):
        for split in (_lib.EMB_SPLIT_L, 4):
            for t in (idx, idx.int(), idx.reshape(idx.shape[0], -1, 1)):
                plan = ops.embedding_walk_plan(t, V, pad, mode, split)
                pos, chunks, mgroups, slots = _brute(idx, V, pad, mode, split)
                assert plan.pos.dtype == plan.chunks.dtype == plan.mgroups.dtype == torch.int32
                assert plan.pos.tolist() == pos and plan.chunks.tolist() == chunks
                assert plan.mgroups.tolist() == mgroups and plan.n_slots == slots
                assert all(0 < end - begin <= split for begin, end, _, _ in chunks)


def test_walk_plan_of_nothing():
    plan = ops.embedding_walk_plan(torch.zeros(2, 3, dtype=torch.int64), 4, 0, _lib.EMB_SQ)
    assert plan.pos.numel() == 0 and tuple(plan.chunks.shape) == (0, 4) and tuple(plan.mgroups.shape) == (0, 3)
    assert plan.n_slots == 0
    # an index outside [0, V) is left out like a padding position (the kernels check every index again)
    wild = ops.embedding_walk_plan(torch.tensor([[0, 9, -1, 2]]), 4, None, _lib.EMB_QUAD)
    assert wild.pos.tolist() == [0, 3]


def test_host_only_abi():
    header = open(os.path.join(ROOT, "include", "curv_hip.h")).read()
    declared = set(re.findall(r"\b(curv_(?:kfac|persample)_embedding_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == {"curv_kfac_embedding_workspace_bytes", "curv_kfac_embedding_plan_flops",
                        "curv_kfac_embedding_accumulate", "curv_persample_embedding_workspace_bytes",
                        "curv_persample_embedding_sq_accumulate", "curv_persample_embedding_quad_reduce"}
    handle = _lib.lib()
    assert all(name in _lib.SIGNATURES and hasattr(handle, name) for name in declared)
    assert "embedding_factor.hip" in _lib.SOURCES
    for macro, value in (("CURV_EMB_SPLIT_L", _lib.EMB_SPLIT_L), ("CURV_EMB_SQ", _lib.EMB_SQ), ("CURV_EMB_QUAD", _lib.EMB_QUAD),
                         ("CURV_EMB_W_MATRIX", _lib.EMB_W_MATRIX), ("CURV_EMB_W_VECTOR", _lib.EMB_W_VECTOR)):
        assert re.search(rf"#define {macro} {value}\b", header), macro
    assert handle.curv_version() == 12                            # symbols and descriptors are added, no record changes
    assert handle.curv_kfac_embedding_accumulate(None, None, 0, None, 0) == 0
    assert handle.curv_persample_embedding_sq_accumulate(None, None, 0, None, 0) == 0
    assert handle.curv_persample_embedding_quad_reduce(None, None, 0, None, 0) == 0
    hist = (_lib.curv_embedding_desc * 2)()
    for d in hist:
        d.positions, d.V, d.padding_idx, d.idx_i64 = 20, 11, -1, 1
    assert handle.curv_kfac_embedding_workspace_bytes(hist, 2) >= 2 * 44
    for field, value in (("V", 0), ("positions", 0), ("positions", 1 << 31), ("padding_idx", 11), ("reserved", 1)):
        bad = (_lib.curv_embedding_desc * 2)()
        ctypes.memmove(bad, hist, ctypes.sizeof(hist))
        setattr(bad[1], field, value)
        assert handle.curv_kfac_embedding_workspace_bytes(bad, 2) == 0
        assert b"item 1" in handle.curv_last_error()
    walk = (_lib.curv_embedding_walk_desc * 2)()
    for d in walk:
        d.positions, d.N, d.T, d.V, d.D, d.padding_idx, d.mode = 20, 4, 5, 11, 6, -1, _lib.EMB_SQ
        d.g_sn, d.g_st, d.g_elems, d.dst_rs, d.alpha = 30, 6, 120, 6, 1.0
        d.n_pos, d.n_chunks, d.n_mgroups, d.n_slots = 20, 12, 1, 3
    assert handle.curv_persample_embedding_workspace_bytes(walk, 2) >= 2 * 3 * 3 * 8 * 4
    for field, value, text in (("D", 0, b"sizes"), ("V", 0, b"sizes"), ("positions", 19, b"sizes"), ("g_elems", 119, b"extent"),
                               ("g_st", -1, b"extent"), ("mode", 2, b"mode"), ("reserved", 1, b"reserved"),
                               ("padding_idx", 11, b"padding_idx"), ("dst_rs", 5, b"dst_rs"), ("n_slots", 13, b"list sizes"),
                               ("n_pos", 21, b"list sizes"), ("alpha", float("inf"), b"alpha")):
        bad = (_lib.curv_embedding_walk_desc * 2)()
        ctypes.memmove(bad, walk, ctypes.sizeof(walk))
        setattr(bad[1], field, value)
        assert handle.curv_persample_embedding_workspace_bytes(bad, 2) == 0, field
        message = handle.curv_last_error()
        assert b"item 1" in message and text in message, message
    walk[0].mode = walk[1].mode = _lib.EMB_QUAD
    walk[0].o_stride = walk[1].o_stride = 1
    assert handle.curv_persample_embedding_workspace_bytes(walk, 2) > 0
    walk[1].w_kind = 3
    assert handle.curv_persample_embedding_workspace_bytes(walk, 2) == 0 and b"w_kind" in handle.curv_last_error()
