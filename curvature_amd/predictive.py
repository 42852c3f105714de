"""The linearised (GLM) predictive of KFAC, Diagonal, EFB and INF: `functional_variance`, `functional_variance_grid`,
`stage_output` and `functional_covariance` once, for every estimator that describes itself by a `PredictiveTerms`.

`Curvature` documents the four methods (and refuses them for the estimators that have no linearised predictive);
`LinearisedPredictive` goes in front of it in the bases of KFAC, Diagonal and EFB; INF, whose predictive is behind a switch,
hands over to a `LinearisedPredictive` that holds it by reference (`curvatures._INFPredictive`).  What a call keeps for the next
``inputs=False`` call lives in one dict on the estimator, ``_predictive_kept``, with at most the entries ``"variance"``,
``"grid"``, ``"covariance"`` and (INF) ``"lowrank"``: each reduction replaces its own entry only,
`Curvature.drop_predictive_state` drops them all.
"""
import math
from typing import Callable, List, NamedTuple, Optional

import torch
from torch import Tensor

from . import ops


class PredictiveTerms(NamedTuple):
    """What an estimator says about itself.  `name` goes into the messages.  ``basis(layer)`` = (R_G, R_A), the rotations
    T = R_G g and Y = R_A X of the packed (rows, N Lp) operands, or `basis` None (no rotation: the operands are read where
    they are); ``weights(layer)`` = the (m, n) tensor whose square weighs the entries, or `weights` None (all ones).  The
    grid has a basis of its own and ``spectrum(layer)`` = (u, v, None) - the eigenvalues of the G and the A side:
    `separable` weights - or (None, None, V): dense ones; `grid_missing`: why the grid cannot run yet, if it cannot."""
    name: str
    basis: Optional[Callable]
    weights: Optional[Callable]
    grid_basis: Optional[Callable]
    spectrum: Callable
    separable: bool
    grid_missing: Optional[str] = None
    direct: Optional[Callable] = None          # ``direct(layer)`` = (T, w, s) of a depthwise layer for `ops.PerSampleDwJob`
                                               # (w not yet squared; each may be None)
    direct_grid: Optional[Callable] = None     # ``direct_grid(layer)`` = (T, u, v, V) of a depthwise layer for
                                               # `ops.PerSampleDwGridJob`: separable (u, v) or dense (V) grid weights
    lowrank: Optional[Callable] = None         # ``lowrank(layer)`` = (U_A, U_G, F^T): the posterior is diag(w**2) minus a
                                               # low-rank part in the Kronecker eigenbasis (INF; `_lowrank`)


def _module_of(layer):
    """The module whose records and hyperparameters an item of the per-sample line has: a group slice's grouped layer."""
    return layer.layer if isinstance(layer, ops.GroupSlice) else layer


class LinearisedPredictive:
    """The four reductions of `Curvature`'s linearised predictive (documented there) for an estimator whose
    ``_predictive_terms()`` gives its `PredictiveTerms`, with `Curvature`'s recording hooks and `state` / `inv_state`."""

    def _kept(self) -> dict:
        return self.__dict__.setdefault("_predictive_kept", {})

    # ------------------------------------------------------------------ the shared steps
    def _predictive_operands(self, what: str, call: str, inputs: bool, rotated: bool, check=None,
                             select: str = "inv_state", grouped: bool = False, norm: bool = False,
                             embedding: bool = False):
        """What every reduction starts from: the checks, the selected layers that have an inverse state (`select`: the
        dict that says so - the grid needs `state` only), their per-sample operands from the current records (the g side
        only unless `inputs`; packed for a rotation if `rotated`), and the key that ties a kept X side to the recorded
        inputs themselves (tensor and version), not just to their shapes.  ``check(N)`` runs last (the caller's
        test of its own arguments against the batch of N samples).  `grouped`: the caller takes grouped convolutions
        (`ops.admit_grouped_per_sample`): their group slices stand among the layers as `ops.GroupSlice` items, and the
        true depthwise ones come back apart, with their records; `norm`: the caller takes normalisation layers
        (`ops.admit_norm_layers`), which come back among them (`ops.per_sample_route` tells them apart), `embedding`: and
        nn.Embedding layers (`ops.admit_embedding`), likewise.  Returns (layers, operands, key, direct), `direct` a list
        of (layer, input, grad_output)."""
        have = getattr(self, select)
        assert have, ("Inverse state dict is empty. Did you call 'invert' prior to this?" if select == "inv_state" else
                      "State dict is empty. Did you call 'update' prior to this?")
        if self.shard is not None and self.shard.world > 1:
            raise NotImplementedError(f"{what}.{call}: layer-sharded estimators are not supported")
        if getattr(self, "record", None) is None:
            raise RuntimeError(f"{what}.{call}: no recording hooks (construct with per_sample=True, or go "
                               "through evaluate.glm_predictive)")
        layers = self._per_sample_layers(f"{what}.{call}", "select other layer types", grouped=grouped, norm=norm,
                                         embedding=embedding)
        layers = [l for l in layers if l in have]
        assert layers, f"{select} holds none of the selected layers"
        fused = ("depthwise", "norm", "embedding")
        direct = [l for l in layers if ops.per_sample_route(l) in fused]
        direct = [(l, *self._records_of(what, l)) for l in direct]
        layers = ops.per_sample_items([l for l in layers if ops.per_sample_route(l) not in fused])
        layout = dict(rows_outer=True, in_place=False) if rotated else {}
        operands = self._per_sample_operands(what, layers, x_side=inputs, **layout) if layers else []
        if check is not None:
            check(operands[0][0].N if operands else int(direct[0][1].shape[0]))
        inputs_of = [self.record[_module_of(l)][0] for l in layers]
        key = tuple((l, id(x), x._version, s.n, s.N, s.L, s.x.ns, s.x.rs)
                    for l, x, (s, _, _) in zip(layers, inputs_of, operands)) + \
            tuple((l, id(x), x._version, tuple(x.shape), tuple(x.stride())) for l, x, _ in direct)
        return layers, operands, key, direct

    def _x_side(self, entry: str, layers, operands, basis, weights):
        """What depends on the forward pass and the posterior only: X (rotated) and the squared weights.  Entry `entry` of
        the kept state is dropped first: the X side of other records goes before the new one is made."""
        self._kept().pop(entry, None)
        xs = [x for _, _, x in operands] if basis is None else \
            self._rotated([(basis(l)[1], x, s.n) for l, (s, _, x) in zip(layers, operands)])
        return xs, [None if weights is None else ops.mul(weights(l), weights(l)) for l in layers]

    def _kept_entry(self, what: str, call: str, entry: str, key, count: Optional[int] = None) -> dict:
        """Entry `entry` of the kept state, if a call with ``inputs=True`` made it on these very recorded inputs (and for
        `count` outputs); RuntimeError otherwise."""
        kept = self._kept().get(entry)
        if kept is None or kept["key"] != key or (count is not None and kept["count"] != count):
            outputs = "" if count is None else f" and {count} outputs"
            raise RuntimeError(f"{what}.{call}(inputs=False): no call with inputs=True on these recorded inputs{outputs} "
                               "before (a new forward pass needs inputs=True once)")
        return kept

    def _g_side(self, layers, operands, basis, out: List[Tensor] = None) -> List[Tensor]:
        """The g side of every layer, rotated by the G half of `basis` (into `out`, or fresh buffers) if there is one."""
        if basis is None:
            return [g for _, g, _ in operands]
        return self._rotated([(basis(l)[0], g, s.m) for l, (s, g, _) in zip(layers, operands)], out)

    @staticmethod
    def _sum_layers(rows: Tensor, out: Tensor, first: bool) -> None:
        """``out (+)= sum_k rows[k]``, `out` a (1, row size) view: the per-layer rows summed in layer order by one product
        with a row of ones, so that the result does not depend on how the layers are grouped into launches."""
        ones = torch.ones(1, rows.shape[0], dtype=torch.float32, device=rows.device)
        ops.gemm_batched([ops.Gemm(ones, rows.view(rows.shape[0], -1), out, beta=0.0 if first else 1.0)])

    @staticmethod
    def _lowrank(operands, gs, xs, ws, low, outs: List[Tensor]) -> None:
        """The low-rank vectors of every layer into `outs` (each (N, a b)): ``outs[k][n] = F vec(U_A^T (W o P_n)^T U_G)``
        with P_n = g_n X_n^T the (m, n) product, W = `ws` (m, n) and (U_A, U_G, F^T) = `low`.  The weights enter entry by
        entry BEFORE the rotation, which no rotation of the operands can express: `ops.per_sample_project` gives
        Z_n = (W o P_n)^T U_G without writing P_n, stored as (N, b, n) so that ONE product per layer, (N b, n) x U_A, rotates
        all samples; its rows are the vectors q_n in the order l a + k, which the columns of F^T follow."""
        project, rotate, scale = [], [], []
        for (s, _, _), g, x, w, (ua, ug, ft), y in zip(operands, gs, xs, ws, low, outs):
            a, b = ua.shape[1], ug.shape[1]
            zt = torch.empty(s.N, b, s.n, dtype=torch.float32, device=y.device)
            qt = torch.empty(s.N * b, a, dtype=torch.float32, device=y.device)
            project.append(ops.PerSampleProjectJob.of(s, g, x, w, ug, zt.permute(0, 2, 1), first=True))
            rotate.append(ops.Gemm(zt.view(s.N * b, s.n), ua, qt))
            scale.append(ops.Gemm(qt.view(s.N, b * a), ft, y))
        ops.per_sample_project(project)
        ops.gemm_batched(rotate)
        ops.gemm_batched(scale)

    # ------------------------------------------------------------------ the variance of one output
    def functional_variance(self, out: Tensor, *, first: bool = True, inputs: bool = True) -> Tensor:
        """`Curvature.functional_variance`."""
        what, basis, weights, *_ = self._predictive_terms()
        lowrank = self._predictive_terms().lowrank

        def check(N):
            if out.dim() != 1 or out.shape[0] != N or out.dtype != torch.float32 or not out.is_cuda:
                raise RuntimeError(f"{what}.functional_variance: out must be a float32 GPU view of length {N}, got "
                                   f"{tuple(out.shape)} {out.dtype} on {out.device}")
        layers, operands, key, direct = self._predictive_operands(what, "functional_variance", inputs, basis is not None,
                                                                  check, grouped=True, norm=True, embedding=True)
        if inputs:
            xs, ws = self._x_side("variance", layers, operands, basis, weights)
            # a depthwise layer has no packed X to keep: its recorded input is read again; (T, w**2, s) is what it keeps
            terms = [self._predictive_terms().direct(l) for l, _, _ in direct]
            terms = [(T, None if w is None else ops.mul(w, w), s) for T, w, s in terms]
            # an Embedding keeps its row weights, l_a**2 (V,) of KFAC or inv**2 (V, D) of Diagonal, as W
            terms = [(None, W if T is None else ops.mul(T, T), s) if ops.per_sample_route(l) == "embedding" else (T, W, s)
                     for (l, _, _), (T, W, s) in zip(direct, terms)]
            self._kept()["variance"] = dict(key=key, xs=xs, ws=ws, direct=terms,
                                            low=None if lowrank is None else [lowrank(l) for l in layers])
        kept = self._kept_entry(what, "functional_variance", "variance", key)
        gs = self._g_side(layers, operands, basis)
        rows = torch.empty(len(layers) + len(direct), out.shape[0], dtype=torch.float32, device=out.device)
        ops.per_sample_quad_reduce([ops.PerSampleQuadJob.of(s, g, x, w, rows[k], first=True)
                                    for k, ((s, _, _), g, x, w) in enumerate(zip(operands, gs, kept["xs"], kept["ws"]))])
        fused = {"depthwise": (ops.PerSampleDwJob, []), "norm": (ops.PerSampleNormJob, []),
                 "embedding": (ops.PerSampleEmbeddingJob, [])}
        rotate = []
        for k, ((l, x, g), (T, w, s)) in enumerate(zip(direct, kept["direct"])):
            job, jobs = fused[ops.per_sample_route(l)]
            if job is ops.PerSampleEmbeddingJob and s is not None:
                # KFAC: the rows of grad_output times L_G, one product over the (N T, D) rows; the walker sums those
                ops.check_embedding_record(f"{what}.functional_variance: layer {l.__class__.__name__}", g)
                flat = g.detach().reshape(-1, g.shape[-1])
                g = torch.empty(flat.shape, dtype=torch.float32, device=flat.device)
                rotate.append(ops.Gemm(flat, s, g))
                g, s = g.view(*x.shape, -1), None
            jobs.append(job.of(l, x, g, out=rows[len(layers) + k], T=T, W=w, s=s, first=True))
        ops.gemm_batched(rotate)
        ops.per_sample_dw_quad_reduce(fused["depthwise"][1])
        ops.per_sample_norm_quad_reduce(fused["norm"][1])
        ops.per_sample_embedding_quad_reduce(fused["embedding"][1])
        if kept["low"] is not None:
            # minus the squared norm of every layer's low-rank vector, into the layer's row
            ys = [torch.empty(out.shape[0], ft.shape[1], dtype=torch.float32, device=out.device) for _, _, ft in kept["low"]]
            self._lowrank(operands, gs, kept["xs"], kept["ws"], kept["low"], ys)
            ops.per_sample_gram_reduce([ops.PerSampleGramJob(y.unsqueeze(0), rows[k].view(-1, 1, 1), alpha=-1.0)
                                        for k, y in enumerate(ys)])
        self._sum_layers(rows, out.unsqueeze(0), first)
        return out

    # ------------------------------------------------------------------ the variance over a grid of damping pairs
    def _grid_points(self, what: str, hypers, separable: bool):
        """`hypers` checked and resolved: for every selected layer index the lists ``shift[h]`` (rho, or sqrt(rho) for the
        separable weights) and ``gain[h]`` = 1 / multiply, as a function ``(layer) -> (shifts, gains)``."""
        hypers = list(hypers)
        if not hypers:
            raise ValueError(f"{what}.functional_variance_grid: no damping pairs")
        for h, pair in enumerate(hypers):
            if not isinstance(pair, (tuple, list)) or len(pair) != 2:
                raise ValueError(f"{what}.functional_variance_grid: pair {h} is not an (add, multiply) pair: {pair!r}")
            for value in pair:
                values = [value] if self._is_scalar(value) else list(value)
                if not values or not all(math.isfinite(float(x)) and float(x) > 0 for x in values):
                    raise ValueError(f"{what}.functional_variance_grid: pair {h} {tuple(pair)!r}: add and multiply must "
                                     "be finite and > 0")
        gindex = self._global_index()

        def points(layer):
            resolved = [self._hyper(add, multiply, gindex[layer], len(gindex)) for add, multiply in hypers]
            rhos = [n / s for n, s in resolved]
            return [math.sqrt(r) for r in rhos] if separable else rhos, [1.0 / s for _, s in resolved]
        return hypers, points

    def functional_variance_grid(self, out: Tensor, hypers, *, first: bool = True, inputs: bool = True) -> Tensor:
        """`Curvature.functional_variance_grid`."""
        terms = self._predictive_terms()
        what, basis, spectrum = terms.name, terms.grid_basis, terms.spectrum
        hypers, points = self._grid_points(what, hypers, terms.separable)
        if (ops.norm_layers_admitted() or ops.embedding_admitted()) and getattr(self, "record", None) is not None:
            # a selected normalisation layer is refused by name before the missing decomposition, which refuses it too
            self._per_sample_layers(f"{what}.functional_variance_grid", "select other layer types",
                                    grouped=ops.per_sample_admits_grouped_joint())
        if terms.grid_missing is not None:
            raise RuntimeError(f"{what}.functional_variance_grid: {terms.grid_missing}")

        def check(N):
            if tuple(out.shape) != (len(hypers), N) or out.dtype != torch.float32 or not out.is_cuda or \
                    not out.is_contiguous():
                raise RuntimeError(f"{what}.functional_variance_grid: out must be a contiguous float32 GPU tensor of shape "
                                   f"({len(hypers)}, {N}), got {tuple(out.shape)} {out.dtype} on {out.device}")
        layers, operands, key, direct = self._predictive_operands(what, "functional_variance_grid", inputs,
                                                                  basis is not None, check, select="state",
                                                                  grouped=ops.per_sample_admits_grouped_joint())
        if inputs:
            xs, _ = self._x_side("grid", layers, operands, basis, None)
            self._kept()["grid"] = dict(key=key, xs=xs)
        xs = self._kept_entry(what, "functional_variance_grid", "grid", key)["xs"]
        gs = self._g_side(layers, operands, basis)
        tables = [points(_module_of(l)) for l in layers]
        # a depthwise layer: one grid job on its records, with the grid terms of its stacked factors
        direct = [(l, x, g, terms.direct_grid(l), points(l)) for l, x, g in direct]
        N, dev = out.shape[1], out.device
        # chunks of PERSAMPLE_GRID_MAX pairs over the same operands; every layer into its own (pairs, N) block
        for h0 in range(0, len(hypers), ops.PERSAMPLE_GRID_MAX):
            h1 = min(h0 + ops.PERSAMPLE_GRID_MAX, len(hypers))
            rows = torch.empty(len(layers) + len(direct), h1 - h0, N, dtype=torch.float32, device=dev)
            ops.per_sample_quad_grid_reduce([
                ops.PerSampleGridJob.of(s, g, x, *spectrum(l), rows[k], shifts[h0:h1], gains[h0:h1], first=True)
                for k, (l, (s, _, _), g, x, (shifts, gains)) in enumerate(zip(layers, operands, gs, xs, tables))])
            ops.per_sample_dw_quad_grid_reduce([
                ops.PerSampleDwGridJob.of(l, x, g, out=rows[len(layers) + k], T=T, u=u, v=v, V=V, shift=shifts[h0:h1],
                                          gain=gains[h0:h1], first=True)
                for k, (l, x, g, (T, u, v, V), (shifts, gains)) in enumerate(direct)])
            self._sum_layers(rows, out[h0:h1].view(1, -1), first)
        return out

    # ------------------------------------------------------------------ joint covariance of the outputs
    def stage_output(self, slot: int, count: int, *, inputs: bool = False) -> None:
        """`Curvature.stage_output`."""
        what, basis, weights, *_ = self._predictive_terms()
        lowrank = self._predictive_terms().lowrank
        slot, count = int(slot), int(count)
        if not 1 <= count <= ops.PERSAMPLE_COV_MAX_OUTPUTS or not 0 <= slot < count:
            raise ValueError(f"{what}.stage_output: slot {slot} of {count} (at most {ops.PERSAMPLE_COV_MAX_OUTPUTS} outputs)")
        layers, operands, key, direct = self._predictive_operands(what, "stage_output", inputs, basis is not None,
                                                                  grouped=ops.per_sample_admits_grouped_joint())
        if inputs:
            xs, ws = self._x_side("covariance", layers, operands, basis, weights)
            # a slot is what one output's g side takes: its packed copy, or the record itself where that is read in place.
            # The slices of a grouped layer that read its record in place share one copy of it per slot and are views into
            # it: `place` = (buffer, offset) of every item, `whole` = the grouped layer a shared buffer copies
            sizes, place, whole, shared = [], [], {}, {}
            for l, (s, _, _) in zip(layers, operands):
                if isinstance(l, ops.GroupSlice) and not s.g.floats:
                    if l.layer not in shared:
                        shared[l.layer] = len(sizes)
                        whole[len(sizes)] = l.layer
                        sizes.append(self.record[l.layer][1].numel())
                    place.append((shared[l.layer], l.rows.start * s.g.rs))
                else:
                    place.append((len(sizes), 0))
                    sizes.append(s.g.floats or s.N * s.g.ns)
            N = operands[0][0].N if operands else int(direct[0][1].shape[0])
            dev = operands[0][1].device if operands else direct[0][1].device
            stack = ops.per_sample_scratch([count * f for f in sizes], dev, "persample_cov_g") if sizes else []
            # a depthwise layer keeps nothing of X: (T, w, s) and, per slot, the N rows its transformed products take
            terms = [self._predictive_terms().direct(l) for l, _, _ in direct]
            projected = [torch.empty(count, N, l.out_channels * (l.kernel_size[0] * l.kernel_size[1] + int(l.bias is not None)),
                                     dtype=torch.float32, device=dev) for l, _, _ in direct]
            self._kept()["covariance"] = dict(key=key, count=count, xs=xs, ws=ws, sizes=sizes, stack=stack, place=place,
                                              whole=whole, sides=[s for s, _, _ in operands], staged=set(),
                                              direct=terms, projected=projected, N=N, device=dev,
                                              low=None if lowrank is None else [lowrank(l) for l in layers],
                                              inputs=[self.record[_module_of(l)][0] for l in layers] +
                                                     [x for _, x, _ in direct])
        kept = self._kept_entry(what, "stage_output", "covariance", key, count)
        slots = [t[slot * f:(slot + 1) * f] for t, f in zip(kept["stack"], kept["sizes"])]
        if basis is not None:
            self._g_side(layers, operands, basis, [slots[b][at:] for b, at in kept["place"]])
        else:
            sources = [None] * len(slots)
            for (b, _), (_, g, _) in zip(kept["place"], operands):
                sources[b] = self.record[kept["whole"][b]][1].detach().reshape(-1) if b in kept["whole"] else \
                    g.reshape(-1)[:kept["sizes"][b]]
            ops.CopyPlan(slots, sources).run()
        ops.per_sample_dw_project([ops.PerSampleDwProjectJob.of(l, x, g, y=y[slot], T=T, W=w, s=s)
                                   for (l, x, g), (T, w, s), y in zip(direct, kept["direct"], kept["projected"])])
        if kept["low"] is not None:
            # the output's low-rank vectors into slot `slot` of a (count, N, a b) stack per layer
            if "lowstack" not in kept:
                kept["lowstack"] = [torch.empty(count, kept["N"], ft.shape[1], dtype=torch.float32, device=kept["device"])
                                    for _, _, ft in kept["low"]]
            self._lowrank(operands, [g for _, g, _ in operands], kept["xs"], kept["ws"], kept["low"],
                          [stack[slot] for stack in kept["lowstack"]])
        kept["staged"].add(slot)

    def functional_covariance(self, out: Tensor, *, first: bool = True) -> Tensor:
        """`Curvature.functional_covariance` (basis and weights went into the staged operands)."""
        what = self._predictive_terms().name
        kept = self._kept().get("covariance")
        if kept is None:
            raise RuntimeError(f"{what}.functional_covariance: no output staged (stage_output(inputs=True) first)")
        record = getattr(self, "record", None) or {}
        for (layer, _, version, *_), x in zip(kept["key"], kept["inputs"]):
            now = record.get(_module_of(layer), (None, None))[0]
            if now is not x or now._version != version:
                raise RuntimeError(f"{what}.functional_covariance: the recorded inputs are no longer those of "
                                   "stage_output(inputs=True) (a new forward pass needs its outputs staged again)")
        count, missing = kept["count"], sorted(set(range(kept["count"])) - kept["staged"])
        if missing:
            raise RuntimeError(f"{what}.functional_covariance: output slots {missing} of {count} have not been staged since "
                               "the last stage_output(inputs=True)")
        sides, N, dev = kept["sides"], kept["N"], kept["device"]
        if tuple(out.shape) != (N, count, count) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
            raise RuntimeError(f"{what}.functional_covariance: out must be a contiguous float32 GPU tensor of shape "
                               f"({N}, {count}, {count}), got {tuple(out.shape)} {out.dtype} on {out.device}")
        # every layer (a group slice, a depthwise layer) into its own (N, count, count) row
        rows = torch.empty(len(sides) + len(kept["projected"]), N, count, count, dtype=torch.float32, device=dev)
        ops.per_sample_cov_reduce([ops.PerSampleCovJob.of(s, kept["stack"][b][at:], x, w, rows[k], count, kept["sizes"][b],
                                                          first=True)
                                   for k, (s, (b, at), x, w) in enumerate(zip(sides, kept["place"], kept["xs"], kept["ws"]))])
        ops.per_sample_gram_reduce([ops.PerSampleGramJob(y, rows[len(sides) + k], first=True)
                                    for k, y in enumerate(kept["projected"])])
        if kept["low"] is not None:
            ops.per_sample_gram_reduce([ops.PerSampleGramJob(y, rows[k], alpha=-1.0) for k, y in enumerate(kept["lowstack"])])
        self._sum_layers(rows, out.view(1, -1), first)
        return out
