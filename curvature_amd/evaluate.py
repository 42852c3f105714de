"""Bayesian-network inference loop: ``eval_nn`` / ``eval_bnn`` of the reference's ``scripts/evaluate.py``
(:88-152) on the MI355X estimators.

``eval_bnn`` is the deployed hot loop of the path: per Monte-Carlo sample one ``sample_and_replace()`` (two
batched GEMM launches + one batched copy here) and a forward pass over the data; the predictive
distribution is the mean of the per-sample softmax outputs.  Unlike the reference, probabilities are
accumulated on the device and cross to the host once at the end (the reference concatenates logits batch
by batch and converts every sample to numpy).  SURVEY.md section 8(f), rank 3.

``overlap=True`` software-pipelines the loop: the model's state tensors get a second buffer set, and weight sample
k + 1 (and, with a layer shard, its all-gather) is produced on a second HIP stream into the set the forward sweep of
sample k is NOT reading.  Two events per set order the streams (sample written -> forward may read; forward done ->
next sample may overwrite).  The noise stream and every launch are the serial loop's, so the predictions are the
same bit for bit (tests/test_estimator_chain_gpu.py).  Measured on one MI355X (tools/bench_bnn_loop.py, KFAC, ms per
Monte-Carlo sample, serial -> overlapped): ResNet-50 batch 32: 6.36 -> 6.28; batch 32 x 4 sweeps: 21.6 -> 21.8; batch
256: 37.9 -> 37.9; LeNet-5 batch 100: 0.30 -> 0.64.  On one GPU there is nothing to win: a throughput-bound forward
sweep leaves no idle CUs for the 1.5 ms of sampling work, a launch-bound one (batch 32) is bound by the same Python
thread that enqueues the sample, and a tiny model pays for re-pointing its state tensors.  The default is therefore
the serial loop, and the pipelined one is switched on only for a layer-sharded estimator, where it takes the
all-gather of the sampled parameters (a wait on the other ranks, not local work) off the forward stream.
"""
import contextlib
import math
from typing import Iterable, List, NamedTuple, Tuple

import torch

from . import ops


def eval_nn(model: torch.nn.Module, dataset: Iterable, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Softmax predictions (N, classes) and labels (N,) over `dataset` (scripts/evaluate.py:88-119), as
    tensors on `device` / CPU respectively."""
    if device is None:
        device = next(model.parameters()).device
    model.eval()
    probs, labels_all = [], []
    with torch.no_grad():
        for images, labels in dataset:
            logits = model(images.to(device, non_blocking=True))
            probs.append(torch.softmax(logits, dim=1))
            if labels is not None:
                labels_all.append(labels.cpu() if isinstance(labels, torch.Tensor) else torch.as_tensor(labels))
    predictions = torch.cat(probs) if probs else torch.empty(0, device=device)
    labels = torch.cat(labels_all) if labels_all else torch.empty(0, dtype=torch.long)
    return predictions, labels


class _StateBufferSets:
    """Two storage sets for every state tensor of a model (parameters and buffers); `activate(i)` points the
    model at set i.  Set 0 is the storage the model came with."""

    def __init__(self, model: torch.nn.Module):
        self.live: List[torch.Tensor] = list(model.state_dict(keep_vars=True).values())
        first = [t.data for t in self.live]
        self.sets = [first, [t.clone() for t in first]]

    def activate(self, index: int) -> None:
        for t, buf in zip(self.live, self.sets[index]):
            t.data = buf

    def copy(self, dst: int, src: int) -> None:
        pairs = [(d, s_) for d, s_ in zip(self.sets[dst], self.sets[src]) if d.numel()]
        batched = [(d, s_) for d, s_ in pairs if d.is_contiguous() and s_.is_contiguous()]
        ops.CopyPlan([d for d, _ in batched], [s_ for _, s_ in batched]).run()      # one launch group, any dtype
        for d, s_ in pairs:
            if not (d.is_contiguous() and s_.is_contiguous()):
                d.copy_(s_)


_SIDE_STREAMS = {}


def _side_stream(device: torch.device) -> "torch.cuda.Stream":
    index = device.index if device.index is not None else torch.cuda.current_device()
    stream = _SIDE_STREAMS.get(index)
    if stream is None:
        stream = _SIDE_STREAMS[index] = torch.cuda.Stream(device)
    return stream


def _drop_plans_for(estimator, tensors) -> None:
    """Forget the estimator's (and its shard's) cached launch plans that mention any of `tensors` by address."""
    ptrs = {t.data_ptr() for t in tensors if t.numel()}

    def mentions(key) -> bool:
        if isinstance(key, (tuple, list)):
            return any(mentions(k) for k in key)
        return isinstance(key, int) and key in ptrs
    for owner, name in ((estimator, "_sample_plan_cache"), (estimator, "_reload_plans"),
                        (getattr(estimator, "shard", None), "_plans")):
        cache = getattr(owner, name, None) if owner is not None else None
        if isinstance(cache, dict):
            for key in [k for k in cache if mentions(k)]:
                del cache[key]


def eval_bnn(model: torch.nn.Module, dataset: Iterable, estimator, samples: int = 30, device=None,
             overlap: bool = None, samples_per_launch: int = 1):
    """Mean predictive distribution over `samples` posterior weight samples (scripts/evaluate.py:121-152,
    ``stats=False`` path).  Returns ``(mean_predictions, labels)`` as numpy arrays like the reference.
    The model is left at the last sampled weights, as in the reference, in its original storage.

    `overlap`: produce sample k + 1 on a second stream while the forward sweep of sample k runs (see the module
    docstring for what that does and does not buy); default: only for a layer-sharded estimator on the GPU.
    ``overlap=False`` is the reference's serial loop.

    `samples_per_launch` = S > 1: the weight samples are produced S at a time (`sample_many`: for KFAC two GEMM launches
    for S parameter sets, the triangular factors streamed once per S samples; the other estimators file S ordinary samples
    away) and loaded into the model one by one (`replace_from`); serial loop only."""
    if device is None:
        device = next(model.parameters()).device
    device = torch.device(device)
    if overlap is None:
        shard = getattr(estimator, "shard", None)
        overlap = device.type == "cuda" and shard is not None and shard.world > 1
    model.eval()
    mean_predictions = None
    labels = None
    with torch.no_grad():
        if samples_per_launch > 1:
            done = 0
            while done < samples:
                group = min(int(samples_per_launch), samples - done)
                bank = estimator.sample_many(group)
                for k in range(group):
                    estimator.replace_from(bank, k)
                    predictions, labels = eval_nn(model, dataset, device)
                    mean_predictions = predictions if mean_predictions is None else mean_predictions + predictions
                done += group
        elif not overlap or samples < 2:
            for _ in range(samples):
                estimator.sample_and_replace()
                predictions, labels = eval_nn(model, dataset, device)
                mean_predictions = predictions if mean_predictions is None else mean_predictions + predictions
        else:
            main = torch.cuda.current_stream(device)
            side = _side_stream(device)         # one per device for the life of the process: scratch workspaces are
            sets = _StateBufferSets(model)      # cached per stream, a fresh stream per call would pin a new set each time
            written = [torch.cuda.Event(), torch.cuda.Event()]     # sample is complete in set i
            consumed = [torch.cuda.Event(), torch.cuda.Event()]    # the forward sweep has finished reading set i
            side.wait_stream(main)                                 # invert() etc. enqueued by the caller
            with torch.cuda.stream(side):
                estimator.sample_and_replace()                     # sample 0 -> set 0
                written[0].record(side)
            cur = 0
            for k in range(samples):
                cur, nxt = k % 2, 1 - k % 2
                if k + 1 < samples:
                    sets.activate(nxt)
                    with torch.cuda.stream(side):
                        if k >= 1:
                            side.wait_event(consumed[nxt])         # sweep k - 1 read set nxt
                        estimator.sample_and_replace()             # sample k + 1 -> set nxt, concurrent with sweep k
                        written[nxt].record(side)
                sets.activate(cur)
                main.wait_event(written[cur])
                predictions, labels = eval_nn(model, dataset, device)
                consumed[cur].record(main)
                mean_predictions = predictions if mean_predictions is None else mean_predictions + predictions
            if cur != 0:                                           # leave the last sample in the original storage
                sets.copy(0, 1)
                sets.activate(0)
            main.wait_stream(side)
            # the launch plans described for the temporary second buffer set keep a whole model copy alive: drop them
            _drop_plans_for(estimator, sets.sets[1])
        mean_predictions = mean_predictions / samples
    return mean_predictions.cpu().numpy(), labels.numpy()


@contextlib.contextmanager
def _linearised(what: str, model: torch.nn.Module, estimator, images: torch.Tensor, outputs=None):
    """What `glm_predictive` and `glm_predictive_joint` do around their reductions: the model goes into ``eval()`` mode, an
    estimator without recording hooks borrows them for the length of the block, one forward pass.  Yields
    ``(logits, classes, backward)``: `classes` the selected `outputs` (default: all), and ``backward(c)`` back-propagates
    ``logits[:, c].sum()`` into the records with `torch.autograd.grad` on the parameters that require grad (no ``.grad`` is
    touched).  On the way out the borrowed hooks are removed and what the estimator kept of this batch is dropped
    (`drop_predictive_state`).  Mixed precision is the caller's (with `ops.widen_per_sample`): a call wrapped in
    ``torch.autocast`` records bfloat16 / float16 tensors and may yield half-precision `logits`; the drivers do not enter
    autocast themselves, and everything they allocate or return beside `logits` (`variance`, `covariance`, `probs`) is
    float32 - `_probit` and `mc_softmax` work on ``logits.float()``."""
    first_param = next(model.parameters())
    if not first_param.is_cuda or not images.is_cuda:
        raise RuntimeError(f"curvature_amd runs on MI355X only: {what} got a CPU model or batch (no CPU fallback)")
    model.eval()
    borrowed = getattr(estimator, "record", None) is None
    params = [p for p in model.parameters() if p.requires_grad]
    try:
        if borrowed:
            estimator._record_per_sample(type(estimator).__name__)
        logits = model(images)
        if logits.dim() != 2:
            raise RuntimeError(f"{what}: the model must return (N, classes) logits, got {tuple(logits.shape)}")

        def backward(c: int) -> None:
            # (torch.autograd.grad fills the recording hooks like backward(), and touches no .grad.  A selected layer the
            # pass does not reach - frozen parameters behind inputs that need no grad - records nothing: its stale
            # grad_output is cleared first, so that the reduction raises instead of using it)
            for pair in estimator.record.values():
                pair[1] = None
            torch.autograd.grad(logits[:, c].sum(), params, retain_graph=True, allow_unused=True)
        classes = list(range(logits.shape[1])) if outputs is None else [int(c) for c in outputs]
        yield logits, classes, backward
    finally:
        if borrowed:
            for hook in estimator.hooks:
                hook.remove()
            del estimator.hooks, estimator.record
        estimator.drop_predictive_state()                      # the X sides of this batch, the stack of its g sides


def _probit(logits: torch.Tensor, variance: torch.Tensor) -> torch.Tensor:
    return torch.softmax(logits.float() / torch.sqrt(1.0 + (math.pi / 8.0) * variance), dim=-1)


def glm_predictive(model: torch.nn.Module, estimator, images: torch.Tensor, outputs=None):
    """The linearised-Laplace (GLM) predictive of one batch: ``(logits, variance, probs)``, each (N, classes).

    ``variance[n, c]`` is the closed-form variance of output c for input n under the posterior `estimator` samples from,
    with the network linearised in its weights at their mean (`Curvature.functional_variance`: KFAC, Diagonal, EFB; INF
    with `ops.admit_inf_predictive`, for the posterior its regularised precision stands for - see `INF`);
    ``probs = softmax(logits / sqrt(1 + pi / 8 * variance))`` is the probit approximation of the expected softmax.  No
    weights are sampled: one forward pass, then for every output c in `outputs` (default: all; the variance of the
    others stays 0) one backward pass of ``logits[:, c].sum()`` and one `functional_variance` call - the side of it that
    depends on the layer inputs only is worked out for the first output and reused for the others.

    The model is put into ``eval()`` mode, which makes the samples of the batch independent under BatchNorm: the
    gradient of ``sum_n f_c(x_n)`` then splits into the per-sample Jacobians the variance is made of.  A Diagonal / EFB
    built without ``per_sample=True``, or an INF, gets the recording hooks for the length of the call.  The parameters and their
    ``.grad`` are left as they were found (the backward passes are `torch.autograd.grad` calls on the parameters that
    require grad; a selected layer they do not reach raises RuntimeError).  GPU only (RuntimeError for a CPU model: no fallback).
    `glm_predictive_joint` gives the covariance between the outputs as well."""
    with _linearised("glm_predictive", model, estimator, images, outputs) as (logits, classes, backward):
        variance = torch.zeros(logits.shape, dtype=torch.float32, device=logits.device)
        for k, c in enumerate(classes):
            backward(c)
            estimator.functional_variance(variance[:, c], inputs=k == 0)
    logits = logits.detach()
    return logits, variance, _probit(logits, variance)


def glm_predictive_grid(model: torch.nn.Module, estimator, images: torch.Tensor, hypers, outputs=None):
    """`glm_predictive` for a whole list of damping pairs ``hypers = [(add, multiply), ...]`` at once, without an
    inversion: ``(logits, variance, probs)`` with `logits` (N, classes) and `variance`, `probs` of shape
    ``(len(hypers), N, classes)`` - slice h is what ``estimator.invert(*hypers[h])`` followed by `glm_predictive` gives.
    One forward pass and per output one backward pass and one `Curvature.functional_variance_grid` call serve every
    pair (KFAC: after `KFAC.decompose()`); the estimator's `inv_state` is neither needed nor touched.  `outputs`, model
    mode, hooks, parameters and ``.grad`` as in `glm_predictive`.  A grouped Conv2d needs `ops.admit_grouped_joint`
    beside `ops.admit_grouped_per_sample` (KFAC, Diagonal; `tune_glm` goes through here).  GPU only."""
    hypers = list(hypers)
    with _linearised("glm_predictive_grid", model, estimator, images, outputs) as (logits, classes, backward):
        N, C = logits.shape
        variance = torch.zeros(len(hypers), N, C, dtype=torch.float32, device=logits.device)
        column = torch.empty(len(hypers), N, dtype=torch.float32, device=logits.device)
        for k, c in enumerate(classes):
            backward(c)
            estimator.functional_variance_grid(column, hypers, inputs=k == 0)
            variance[:, :, c] = column
    logits = logits.detach()
    return logits, variance, _probit(logits, variance)         # (N, classes) against (H, N, classes)


def tune_glm(model: torch.nn.Module, dataset: Iterable, estimator, hypers, outputs=None):
    """The damping pair of ``hypers = [(add, multiply), ...]`` under which the probit GLM predictive explains the labelled
    `dataset` best - the search the reference's ``scripts/hyper.py`` does with one inversion and one evaluation per
    candidate, here one `glm_predictive_grid` per batch for all of them.  Returns ``dict(nll=(H,), accuracy=(H,),
    best=int)``: `nll` the mean negative log-likelihood of the probit probabilities at the labels, `accuracy` the share
    of inputs whose most probable class is the label (both float64 CPU tensors, accumulated on the device and read
    once), `best` the argmin of `nll` (the first on a tie).  Nothing is called on the estimator afterwards: the caller
    goes on with ``estimator.invert(*hypers[best])``."""
    hypers = list(hypers)
    return _tune("tune_glm", model, dataset, len(hypers),
                 lambda images: glm_predictive_grid(model, estimator, images, hypers, outputs=outputs)[2])


def _tune(what: str, model: torch.nn.Module, dataset: Iterable, pairs: int, probs_of) -> dict:
    """``dict(nll, accuracy, best)`` of `tune_glm` / `tune_last_layer` from ``probs_of(images)`` -> (pairs, N, classes)."""
    device = next(model.parameters()).device
    nll = torch.zeros(pairs, dtype=torch.float64, device=device)
    hits = torch.zeros(pairs, dtype=torch.float64, device=device)
    count = 0
    for images, labels in dataset:
        images = images.to(device, non_blocking=True)
        labels = torch.as_tensor(labels).to(device, non_blocking=True).long()
        probs = probs_of(images)
        index = labels.view(1, -1, 1).expand(pairs, -1, 1)
        nll -= torch.log(probs.gather(2, index).squeeze(2).double()).sum(1)
        hits += (probs.argmax(2) == labels.view(1, -1)).double().sum(1)
        count += int(labels.numel())
    if count == 0:
        raise ValueError(f"{what}: the dataset is empty")
    nll, accuracy = (nll / count).cpu(), (hits / count).cpu()
    return dict(nll=nll, accuracy=accuracy, best=int(torch.argmin(nll)))


def log_likelihood(model: torch.nn.Module, dataset: Iterable, device=None) -> Tuple[float, int]:
    """``(sum, count)``: the SUM over `dataset` of the log-softmax at the label under the weights the model holds (float64,
    accumulated on the device and read once), and the number of labelled inputs."""
    if device is None:
        device = next(model.parameters()).device
    model.eval()
    total = torch.zeros((), dtype=torch.float64, device=device)
    count = 0
    with torch.no_grad():
        for images, labels in dataset:
            logits = model(images.to(device, non_blocking=True))
            labels = torch.as_tensor(labels).to(device, non_blocking=True).long()
            total += torch.log_softmax(logits.double(), dim=1).gather(1, labels.view(-1, 1)).sum()
            count += int(labels.numel())
    return float(total.item()), count


_data_log_likelihood = log_likelihood          # (`log_marginal_likelihood` has a keyword of the function's name)


def log_marginal_likelihood(model: torch.nn.Module, dataset: Iterable, estimator, hypers, *, log_likelihood=None):
    """The Laplace approximation of the log marginal likelihood (the "evidence") for every damping pair of
    ``hypers = [(add, multiply), ...]`` - what the prior precision of a Laplace posterior is usually chosen by, with no
    held-out labels and no backward pass:

        evidence(h) = loglik - 1/2 sum_l n_l ||theta_l||^2 + 1/2 sum_l P_l log n_l - 1/2 sum_l log det Pi_l(n_l, s_l)

    over the estimator's (owned) layers, with (n_l, s_l) the pair `invert` would resolve for layer l
    (`Curvature.log_det_grid`, `Curvature.log_prior_grid`; the 2 pi terms cancel).  `multiply` is the data-set size in the
    reference's convention: the accumulated curvature is a mean over the data, and s scales it to the sum the evidence
    needs.  `loglik` is `log_likelihood(model, dataset)` under the weights the model holds now - the MAP weights, unless
    the caller left a sample in it.  Passing ``log_likelihood=`` (the sum, or the ``(sum, count)`` pair) skips the data
    pass; `dataset` may then be None.  Returns ``dict(evidence=(H,), log_likelihood=float, log_det=(H,), log_prior=(H,),
    best=int)``: float64 CPU tensors read back once, `best` the argmax of `evidence` (the first on a tie).  ValueError on
    an empty dataset.  On a layer-sharded estimator the three sums cover the owned layers; the caller all-reduces."""
    hypers = list(hypers)
    if log_likelihood is None:
        device = next(model.parameters()).device
        value, count = _data_log_likelihood(model, dataset, device)
        if count == 0:
            raise ValueError("log_marginal_likelihood: the dataset is empty")
    else:
        value = float(log_likelihood[0] if isinstance(log_likelihood, (tuple, list)) else log_likelihood)
    log_det = estimator.log_det_grid(hypers)
    log_prior = estimator.log_prior_grid(hypers)
    evidence = (log_prior - 0.5 * log_det) + value
    evidence, log_det, log_prior = torch.stack([evidence, log_det, log_prior]).cpu()
    # (argmax of the first maximum: torch.argmax does not promise which of several equal entries it returns)
    best = min(range(len(hypers)), key=lambda h: (-float(evidence[h]), h))
    return dict(evidence=evidence, log_likelihood=value, log_det=log_det, log_prior=log_prior, best=best)


def _joint_covariance(what: str, model: torch.nn.Module, estimator, images: torch.Tensor, outputs):
    """What `glm_predictive_joint` and `glm_predictive_mc` share: ``(logits, covariance, classes)`` from one forward pass,
    one backward pass and one `Curvature.stage_output` per selected output, and one `Curvature.functional_covariance`."""
    with _linearised(what, model, estimator, images, outputs) as (logits, classes, backward):
        K = len(classes)
        if not 1 <= K <= ops.PERSAMPLE_COV_MAX_OUTPUTS or len(set(classes)) != K:
            raise ValueError(f"{what}: {K} outputs ({len(set(classes))} distinct); the joint covariance takes "
                             f"1 to {ops.PERSAMPLE_COV_MAX_OUTPUTS} distinct outputs per call: pass outputs= (for instance "
                             "the top-k classes)")
        covariance = torch.empty(logits.shape[0], K, K, dtype=torch.float32, device=logits.device)
        for k, c in enumerate(classes):
            backward(c)
            estimator.stage_output(k, K, inputs=k == 0)
        estimator.functional_covariance(covariance)
    return logits.detach(), covariance, classes


def glm_predictive_joint(model: torch.nn.Module, estimator, images: torch.Tensor, outputs=None):
    """`glm_predictive` with the joint covariance of the outputs: ``(logits, covariance, probs)``.

    ``covariance[n]`` is the K x K covariance matrix of the outputs `outputs` (in that order; default: all classes) for
    input n under the linearised posterior - the logits share every weight below the head, so they are not independent;
    the covariance is what sampling logits, a multi-output regression head or ``Var(f_c - f_c')`` need.  Its diagonal is
    `glm_predictive`'s variance.  ``probs`` is the same probit softmax on that diagonal (the variance of an output that
    is not selected is 0); `glm_predictive_mc` gives the expected softmax under the whole covariance.  One forward pass,
    per output one backward pass and one `Curvature.stage_output`, then one
    `Curvature.functional_covariance`: a single pass over the per-sample products in which the input side of every layer
    is staged once for all outputs.  At most `ops.PERSAMPLE_COV_MAX_OUTPUTS` (16) distinct outputs per call: ValueError
    otherwise (raised after the forward pass, when the class count is known) - pass ``outputs=``, for instance the top-k
    classes.  Model mode, hooks, parameters and ``.grad`` as in `glm_predictive`.  A grouped Conv2d needs
    `ops.admit_grouped_joint` beside `ops.admit_grouped_per_sample` (KFAC, Diagonal; `glm_predictive_mc` and
    ``eval_glm(predictive="mc")`` go through the same passes).  INF takes part with `ops.admit_inf_predictive`.  GPU only."""
    logits, covariance, classes = _joint_covariance("glm_predictive_joint", model, estimator, images, outputs)
    variance = torch.zeros(logits.shape, dtype=torch.float32, device=logits.device)
    variance[:, classes] = torch.diagonal(covariance, dim1=1, dim2=2)
    return logits, covariance, _probit(logits, variance)


def mc_softmax(logits: torch.Tensor, covariance: torch.Tensor, classes, samples: int, noise=None, seed: int = 0,
               offset: int = 0, return_draws: bool = False, what: str = "mc_softmax"):
    """``E softmax(f)`` for ``f[:, classes] ~ N(logits[:, classes], covariance)`` and the other logits held fixed, by
    `samples` draws in one `ops.logit_mc` call: ``(probs, draws)`` with `probs` (N, all classes) and `draws` the
    (N, samples, K) logit draws or None.  The selected columns are the kernel's means; an unselected class c gets the mass
    left over, ``probs_rest[n] * exp(logits[n, c] - rest[n])`` with ``rest = logsumexp`` of the unselected logits, so rows
    sum to 1.  `noise`: explicit (N, samples, K) standard-normal z; otherwise the library's Philox stream at `seed`,
    `offset` (``N * samples * ceil(K / 4)`` counters).  A covariance with a negative Cholesky pivot raises RuntimeError
    naming the input (one host read of the status words, after the kernel); columns dropped because the covariance is
    singular are no error."""
    N, C = logits.shape
    K = len(classes)
    dev = logits.device
    chosen = set(classes)
    others = [c for c in range(C) if c not in chosen]
    logits = logits.float()
    mu = logits[:, classes].contiguous()
    rest = torch.logsumexp(logits[:, others], dim=1) if others else None
    selected = torch.empty(N, K, dtype=torch.float32, device=dev)
    left = torch.empty(N, dtype=torch.float32, device=dev)
    info = torch.empty(N, dtype=torch.int32, device=dev)
    draws = torch.empty(N, samples, K, dtype=torch.float32, device=dev) if return_draws else None
    ops.logit_mc([ops.LogitMCJob(covariance, mu, samples, rest=rest, noise=noise, probs=selected, probs_rest=left,
                                 draws=draws, info=info, seed=seed, offset=offset)])
    status = info.cpu()
    if bool((status < 0).any()):
        n = int(torch.nonzero(status < 0)[0])
        raise RuntimeError(f"{what}: the covariance of input {n} is not positive semi-definite (Cholesky pivot "
                           f"{-int(status[n]) - 1} is negative)")
    probs = torch.empty(N, C, dtype=torch.float32, device=dev)
    probs[:, classes] = selected
    if others:
        probs[:, others] = left[:, None] * torch.exp(logits[:, others] - rest[:, None])
    return probs, draws


def glm_predictive_mc(model: torch.nn.Module, estimator, images: torch.Tensor, outputs=None, samples: int = 256,
                      noise=None, return_draws: bool = False):
    """The GLM predictive by Monte Carlo over the joint logit covariance: ``(logits, covariance, probs)``, plus `draws`
    (N, samples, K) with ``return_draws=True``.

    `logits` and `covariance` are `glm_predictive_joint`'s (same passes, same bits).  ``probs`` (N, classes) is the mean
    over `samples` draws ``f ~ N(logits[:, outputs], covariance)`` of the softmax over all classes, the logits that are not
    selected held at their values (their variance is 0 by the convention of the covariance): the expectation the probit
    softmax of `glm_predictive` approximates from the diagonal alone, here with the correlations between the logits.  One
    fused kernel (`ops.logit_mc`): a Cholesky factor per input, the draws, their softmax and the mean, without an
    (N, samples, K) tensor unless `draws` is asked for.  `noise`: explicit (N, samples, K) float32 GPU z, mirroring
    ``KFAC.sample(layer, z)``; otherwise the draws come from the estimator's own noise stream (`noise_seed` pins them,
    `noise_offset` advances by ``N * samples * ceil(K / 4)``, so successive calls are independent).  A covariance that is
    singular is fine (`Curvature.functional_covariance` gives one whenever there are more outputs than the Jacobians'
    rank); one that is not positive semi-definite raises RuntimeError naming the input.  Estimators as for
    `glm_predictive_joint` (INF with `ops.admit_inf_predictive`).  GPU only."""
    samples = int(samples)
    if samples < 1:
        raise ValueError(f"glm_predictive_mc: samples must be at least 1, got {samples}")
    logits, covariance, classes = _joint_covariance("glm_predictive_mc", model, estimator, images, outputs)
    seed = offset = 0
    if noise is None:
        if getattr(estimator, "_noise_counter", None) is not None:
            raise RuntimeError("glm_predictive_mc: the noise position is kept on the host only; switch the estimator's "
                               "device noise counter off (use_device_noise_counter(False)) or pass noise=")
        seed, offset = estimator._seed(), estimator.noise_offset
        estimator.noise_offset += logits.shape[0] * samples * ((len(classes) + 3) // 4)
    probs, draws = mc_softmax(logits, covariance, classes, samples, noise=noise, seed=seed, offset=offset,
                              return_draws=return_draws, what="glm_predictive_mc")
    return (logits, covariance, probs, draws) if return_draws else (logits, covariance, probs)


def _default_head(estimator):
    """The last `nn.Linear` of the estimator's `inv_state` in ``model.modules()`` order, or None."""
    held = [layer for layer in estimator.model.modules()
            if isinstance(layer, torch.nn.Linear) and layer in estimator.inv_state]
    return held[-1] if held else None


def _head_pass(what: str, model: torch.nn.Module, estimator, images: torch.Tensor, head, predictive: str, samples: int,
               held: str, refuse):
    """(head, features, logits) of one forward pass for `last_layer_predictive` (`held` "inv_state") and
    `last_layer_predictive_grid` ("state"): the checks that need no device, the default head - the last `nn.Linear` of
    the estimator's `held` dict in ``modules()`` order -, the two hooks on it, and what the captured tensors must be.
    ``refuse(layer)`` raises the estimator's refusal of a head that is no module."""
    if predictive not in ("probit", "mc"):
        raise ValueError(f"{what}: predictive must be 'probit' or 'mc', got {predictive!r}")
    if samples < 1:
        raise ValueError(f"{what}: samples must be at least 1, got {samples}")
    first_param = next(model.parameters())
    if not first_param.is_cuda or not images.is_cuda:
        raise RuntimeError(f"curvature_amd runs on MI355X only: {what} got a CPU model or batch (no CPU fallback)")
    if head is None:
        if held == "inv_state":
            assert estimator.inv_state, "Inverse state dict is empty. Did you call 'invert' prior to this?"
            head = _default_head(estimator)
        else:
            assert estimator.state, "State dict is empty. Did you call 'update' prior to this?"
            linear = [layer for layer in estimator.model.modules()
                      if isinstance(layer, torch.nn.Linear) and layer in estimator.state]
            head = linear[-1] if linear else None
        if head is None:
            raise RuntimeError(f"{what}: the estimator holds no nn.Linear layer in {held}; pass head=")
    names = {m: n for n, m in estimator.model.named_modules()}
    names.update({m: n for n, m in model.named_modules()})
    name = names.get(head, repr(head))
    if not isinstance(head, torch.nn.Module):
        refuse(head)                                           # (an attention projection: the estimator's refusal)
    model.eval()
    seen = {}
    hooks = [head.register_forward_pre_hook(lambda module, args: seen.__setitem__("input", args[0])),
             head.register_forward_hook(lambda module, args, output: seen.__setitem__("output", output))]
    try:
        with torch.no_grad():
            output = model(images)
    finally:
        for hook in hooks:
            hook.remove()
    if "output" not in seen:
        raise RuntimeError(f"{what}: the head '{name}' did not run in the model's forward pass")
    features, logits = seen["input"], seen["output"]
    if not isinstance(features, torch.Tensor) or features.dim() != 2:
        shape = tuple(features.shape) if isinstance(features, torch.Tensor) else type(features).__name__
        raise RuntimeError(f"{what}: the input of the head '{name}' must be (N, features), got {shape} (a head applied "
                           "per token is not supported)")
    if not isinstance(output, torch.Tensor) or output.shape != logits.shape or not torch.equal(output, logits):
        raise RuntimeError(f"{what}: the model's output is not the output of the head '{name}' (a model that "
                           "post-processes its logits is not supported)")
    return head, features, logits


def _head_noise(what: str, estimator, noise, counters: int):
    """(seed, offset) of one `ops.head_mc` call: zeros with explicit `noise`, otherwise the estimator's stream, advanced
    by `counters`."""
    if noise is not None:
        return 0, 0
    if getattr(estimator, "_noise_counter", None) is not None:
        raise RuntimeError(f"{what}: the noise position is kept on the host only; switch the estimator's "
                           "device noise counter off (use_device_noise_counter(False)) or pass noise=")
    seed, offset = estimator._seed(), estimator.noise_offset
    estimator.noise_offset += counters
    return seed, offset


def last_layer_predictive(model: torch.nn.Module, estimator, images: torch.Tensor, *, head=None,
                          predictive: str = "probit", samples: int = 256, noise=None, return_draws: bool = False):
    """The Laplace predictive of one batch under the posterior over the LAST `Linear` layer alone, for every class from one
    forward pass: ``(logits, variance, probs)``, each (N, K), plus `draws` (N, samples, K) with ``return_draws=True``
    (``predictive="mc"`` only; None otherwise).

    The Jacobian of logit c with respect to the head's [W | b] is ``e_c phi~^T``, so the covariance of all K logits is
    closed form in what the estimator holds (`Curvature.head_terms`: KFAC, EFB, Diagonal): no backward pass per output as
    in `glm_predictive`, and no limit of `ops.PERSAMPLE_COV_MAX_OUTPUTS` outputs as in `glm_predictive_mc`.
    ``predictive="probit"``: ``softmax(logits / sqrt(1 + pi / 8 * variance))``.  ``"mc"``: the mean softmax over `samples`
    draws ``f ~ N(logits, M diag(d2) M^T)`` in one `ops.head_mc` call over all classes (K at most
    `ops.HEAD_MC_MAX_CLASSES`: ValueError above).  `noise`: explicit (N, samples, K) float32 GPU z; otherwise the
    estimator's own noise stream (`noise_seed` pins it, `noise_offset` advances by ``N * samples * ceil(K / 4)``).

    The model is put into ``eval()`` mode and run once under ``torch.no_grad()``; a forward pre-hook and a forward hook on
    `head` (default: the last `nn.Linear` of ``estimator.inv_state`` in ``modules()`` order) capture its input and output
    and are removed on the way out.  Recording hooks, parameters and ``.grad`` are not touched.  RuntimeError, naming the
    layer, if the head did not run, if its input is not 2-D (a head applied per token), or if the model's output is not
    the head's output (a model that post-processes its logits).  GPU only."""
    what = "last_layer_predictive"
    samples = int(samples)
    head, features, logits = _head_pass(what, model, estimator, images, head, predictive, samples, "inv_state",
                                        lambda layer: estimator.head_terms(layer, None))
    terms = estimator.head_terms(head, features)
    N, K = logits.shape
    if predictive == "probit":
        return (logits, terms.variance, _probit(logits, terms.variance)) + ((None,) if return_draws else ())
    if K > ops.HEAD_MC_MAX_CLASSES:
        raise ValueError(f"{what}: {K} classes; predictive='mc' takes at most ops.HEAD_MC_MAX_CLASSES = "
                         f"{ops.HEAD_MC_MAX_CLASSES}: use predictive='probit'")
    seed, offset = _head_noise(what, estimator, noise, N * samples * ((K + 3) // 4))
    probs = torch.empty(N, K, dtype=torch.float32, device=logits.device)
    draws = torch.empty(N, samples, K, dtype=torch.float32, device=logits.device) if return_draws else None
    ops.head_mc([ops.HeadMCJob(terms.M, terms.d2, logits.float().contiguous(), samples, lower=terms.lower, noise=noise,
                               probs=probs, draws=draws, seed=seed, offset=offset)])
    return (logits, terms.variance, probs, draws) if return_draws else (logits, terms.variance, probs)


def last_layer_predictive_grid(model: torch.nn.Module, estimator, images: torch.Tensor, hypers, *, head=None,
                               predictive: str = "probit", samples: int = 256, noise=None):
    """`last_layer_predictive` for a whole list of damping pairs ``hypers = [(add, multiply), ...]`` at once, without an
    inversion: ``(logits, variance, probs)`` with `logits` (N, K) and `variance`, `probs` of shape ``(len(hypers), N, K)`` -
    slice h is what ``estimator.invert(*hypers[h])`` followed by `last_layer_predictive` stands for.  One forward pass,
    one rotation of the features and one read of the spectrum serve every pair (`Curvature.head_terms_grid`: KFAC after
    `KFAC.decompose()`, EFB, Diagonal); the estimator's `inv_state` is neither needed nor touched, so the default head is
    the last `nn.Linear` of ``estimator.state`` in ``modules()`` order.  ``predictive="probit"``: the probit softmax,
    broadcast over the pairs.  ``"mc"``: ONE `ops.head_mc` call with one item per pair; the items share the matrix, the
    logits and the noise - explicit `noise` (N, samples, K) or one stretch of the estimator's stream, `noise_offset`
    advancing once by ``N * samples * ceil(K / 4)`` - so the pairs are compared on the same draws (common random
    numbers).  Model mode, hooks, refusals and the cap of `ops.HEAD_MC_MAX_CLASSES` classes as in
    `last_layer_predictive`.  GPU only."""
    what = "last_layer_predictive_grid"
    samples = int(samples)
    hypers = estimator._evidence_pairs("head_terms_grid", hypers)
    head, features, logits = _head_pass(what, model, estimator, images, head, predictive, samples, "state",
                                        lambda layer: estimator.head_terms_grid(layer, None, hypers))
    terms = estimator.head_terms_grid(head, features, hypers)
    N, K = logits.shape
    if predictive == "probit":
        return logits, terms.variance, _probit(logits, terms.variance)         # (N, K) against (H, N, K)
    if K > ops.HEAD_MC_MAX_CLASSES:
        raise ValueError(f"{what}: {K} classes; predictive='mc' takes at most ops.HEAD_MC_MAX_CLASSES = "
                         f"{ops.HEAD_MC_MAX_CLASSES}: use predictive='probit'")
    seed, offset = _head_noise(what, estimator, noise, N * samples * ((K + 3) // 4))
    probs = torch.empty(len(hypers), N, K, dtype=torch.float32, device=logits.device)
    mu = logits.float().contiguous()
    ops.head_mc([ops.HeadMCJob(terms.M, terms.d2[h], mu, samples, noise=noise, probs=probs[h], seed=seed, offset=offset)
                 for h in range(len(hypers))])
    return logits, terms.variance, probs


def tune_last_layer(model: torch.nn.Module, dataset: Iterable, estimator, hypers, *, predictive: str = "probit",
                    samples: int = 256, head=None):
    """`tune_glm` for the last-layer predictive: the damping pair of ``hypers = [(add, multiply), ...]`` under which
    `last_layer_predictive` explains the labelled `dataset` best, from one `last_layer_predictive_grid` per batch for all
    of them - no inversion and one forward pass per batch, where the reference's ``scripts/hyper.py`` loop pays one
    `invert` and one pass over the data per candidate.  Returns ``dict(nll=(H,), accuracy=(H,), best=int)`` computed as
    `tune_glm` computes them.  ``predictive="mc"`` draws from the estimator's noise stream, every pair of a batch on the
    same draws.  The caller goes on with ``estimator.invert(*hypers[best])``."""
    if predictive not in ("probit", "mc"):
        raise ValueError(f"tune_last_layer: predictive must be 'probit' or 'mc', got {predictive!r}")
    hypers = estimator._evidence_pairs("head_terms_grid", hypers)
    return _tune("tune_last_layer", model, dataset, len(hypers),
                 lambda images: last_layer_predictive_grid(model, estimator, images, hypers, head=head,
                                                           predictive=predictive, samples=samples)[2])


def eval_last_layer(model: torch.nn.Module, dataset: Iterable, estimator, predictive: str = "probit", samples: int = 256,
                    head=None, device=None):
    """`last_layer_predictive` over `dataset`: ``(predictions, labels)`` as numpy arrays - the loop of `eval_glm` at one
    forward pass per batch for any number of classes.  ``predictive="mc"`` draws from the estimator's noise stream.  The
    probabilities stay on the device and cross to the host once at the end."""
    if predictive not in ("probit", "mc"):
        raise ValueError(f"eval_last_layer: predictive must be 'probit' or 'mc', got {predictive!r}")
    if device is None:
        device = next(model.parameters()).device
    probs, labels_all = [], []
    for images, labels in dataset:
        images = images.to(device, non_blocking=True)
        probs.append(last_layer_predictive(model, estimator, images, head=head, predictive=predictive,
                                           samples=samples)[2])
        if labels is not None:
            labels_all.append(labels.cpu() if isinstance(labels, torch.Tensor) else torch.as_tensor(labels))
    predictions = torch.cat(probs) if probs else torch.empty(0, device=device)
    labels = torch.cat(labels_all) if labels_all else torch.empty(0, dtype=torch.long)
    return predictions.cpu().numpy(), labels.numpy()


class Uncertainty(NamedTuple):
    """What `last_layer_uncertainty` returns: `logits`, `variance`, `probs` (N, K) as `last_layer_predictive` gives them,
    `probs_std` (N, K) the standard deviation of each class probability over the draws, and the entropies (N,) in nats:
    `total` = H(probs), `aleatoric` = the mean entropy of the draws, `epistemic` = their difference, the mutual
    information between the prediction and the head's weights."""
    logits: torch.Tensor
    variance: torch.Tensor
    probs: torch.Tensor
    probs_std: torch.Tensor
    total: torch.Tensor
    aleatoric: torch.Tensor
    epistemic: torch.Tensor


def last_layer_uncertainty(model: torch.nn.Module, estimator, images: torch.Tensor, *, head=None, samples: int = 256,
                           noise=None) -> Uncertainty:
    """The uncertainty of the last-layer Laplace predictive of one batch, split into what the data leave open and what the
    posterior over the head's weights leaves open: `Uncertainty` (logits, variance, probs, probs_std, total, aleatoric,
    epistemic).

    One forward pass, `Curvature.head_terms` and ONE `ops.head_mc_moments` call: the draws
    ``f ~ N(logits, M diag(d2) M^T)`` of ``last_layer_predictive(predictive="mc")`` - `logits`, `variance` and `probs` have
    its bits on the same noise - give, without an (N, samples, K) tensor, the mean entropy of their softmax (`aleatoric`)
    and the mean square of every class probability.  ``total = H(probs)`` with ``0 ln 0 = 0``;
    ``epistemic = clamp(total - aleatoric, min=0)`` (non-negative by Jensen's inequality in exact arithmetic; where it is
    small it is a difference of two nearly equal numbers, accurate relative to `total` and not to itself);
    ``probs_std = sqrt(clamp(probs_sq - probs ** 2, min=0))``, so ``probs_std / sqrt(samples)`` is the Monte-Carlo standard
    error of `probs`.  Noise, the cap of `ops.HEAD_MC_MAX_CLASSES` classes, model mode, hooks and refusals as in
    `last_layer_predictive`; `noise_offset` advances by ``N * samples * ceil(K / 4)``.  GPU only."""
    what = "last_layer_uncertainty"
    samples = int(samples)
    head, features, logits = _head_pass(what, model, estimator, images, head, "mc", samples, "inv_state",
                                        lambda layer: estimator.head_terms(layer, None))
    terms = estimator.head_terms(head, features)
    N, K = logits.shape
    if K > ops.HEAD_MC_MAX_CLASSES:
        raise ValueError(f"{what}: {K} classes; the draws take at most ops.HEAD_MC_MAX_CLASSES = "
                         f"{ops.HEAD_MC_MAX_CLASSES}")
    seed, offset = _head_noise(what, estimator, noise, N * samples * ((K + 3) // 4))
    probs = torch.empty(N, K, dtype=torch.float32, device=logits.device)
    probs_sq = torch.empty(N, K, dtype=torch.float32, device=logits.device)
    aleatoric = torch.empty(N, dtype=torch.float32, device=logits.device)
    ops.head_mc_moments([ops.HeadMomentsJob(terms.M, terms.d2, logits.float().contiguous(), samples, lower=terms.lower,
                                            noise=noise, probs=probs, entropy=aleatoric, probs_sq=probs_sq, seed=seed,
                                            offset=offset)])
    total = -torch.xlogy(probs, probs).sum(dim=1)
    epistemic = torch.clamp(total - aleatoric, min=0.0)
    probs_std = torch.sqrt(torch.clamp(probs_sq - probs * probs, min=0.0))
    return Uncertainty(logits, terms.variance, probs, probs_std, total, aleatoric, epistemic)


def eval_uncertainty(model: torch.nn.Module, dataset: Iterable, estimator, samples: int = 256, head=None, device=None):
    """`last_layer_uncertainty` over `dataset` - the loop of `eval_last_layer`: a dict of numpy arrays `probs` (N, K),
    `labels` (N,), `total`, `aleatoric`, `epistemic` (N,).  The draws come from the estimator's noise stream.  Everything
    stays on the device and crosses to the host once at the end."""
    if device is None:
        device = next(model.parameters()).device
    keys = ("probs", "total", "aleatoric", "epistemic")
    parts, labels_all = {key: [] for key in keys}, []
    for images, labels in dataset:
        images = images.to(device, non_blocking=True)
        result = last_layer_uncertainty(model, estimator, images, head=head, samples=samples)
        for key in keys:
            parts[key].append(getattr(result, key))
        if labels is not None:
            labels_all.append(labels.cpu() if isinstance(labels, torch.Tensor) else torch.as_tensor(labels))
    out = {key: (torch.cat(parts[key]) if parts[key] else torch.empty(0, device=device)).cpu().numpy() for key in keys}
    out["labels"] = (torch.cat(labels_all) if labels_all else torch.empty(0, dtype=torch.long)).numpy()
    return out


def eval_glm(model: torch.nn.Module, dataset: Iterable, estimator, predictive: str = "probit", outputs=None,
             samples: int = 256, device=None):
    """The GLM predictive over `dataset`: ``(predictions, labels)`` as numpy arrays, the counterpart of `eval_bnn` without
    weight samples.  ``predictive="probit"`` goes through `glm_predictive`, ``"mc"`` through `glm_predictive_mc` with
    `samples` draws per input from the estimator's noise stream; `outputs` as there.  Every estimator with a linearised
    predictive (KFAC, Diagonal, EFB; INF with `ops.admit_inf_predictive`).  The probabilities stay on the device and cross
    to the host once at the end."""
    if predictive not in ("probit", "mc"):
        raise ValueError(f"eval_glm: predictive must be 'probit' or 'mc', got {predictive!r}")
    if device is None:
        device = next(model.parameters()).device
    probs, labels_all = [], []
    for images, labels in dataset:
        images = images.to(device, non_blocking=True)
        if predictive == "probit":
            probs.append(glm_predictive(model, estimator, images, outputs=outputs)[2])
        else:
            probs.append(glm_predictive_mc(model, estimator, images, outputs=outputs, samples=samples)[2])
        if labels is not None:
            labels_all.append(labels.cpu() if isinstance(labels, torch.Tensor) else torch.as_tensor(labels))
    predictions = torch.cat(probs) if probs else torch.empty(0, device=device)
    labels = torch.cat(labels_all) if labels_all else torch.empty(0, dtype=torch.long)
    return predictions.cpu().numpy(), labels.numpy()
