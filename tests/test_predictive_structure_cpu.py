"""Where the linearised (GLM) predictive lives: one mixin (`predictive.LinearisedPredictive`) in front of `Curvature` for
KFAC, Diagonal and EFB, the documented API on `Curvature`, and one kept-state record with one method that drops it."""
import glob
import os

import torch

from curvature_amd.curvatures import EFB, INF, KFAC, BlockDiagonal, Curvature, Diagonal
from curvature_amd.predictive import LinearisedPredictive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("functional_variance", "functional_variance_grid", "stage_output", "functional_covariance")


def test_the_mixin_is_where_it_belongs():
    for cls in (KFAC, Diagonal, EFB):
        mro = cls.__mro__
        assert LinearisedPredictive in mro and mro.index(LinearisedPredictive) < mro.index(Curvature)
    for cls in (BlockDiagonal, INF, Curvature):
        assert LinearisedPredictive not in cls.__mro__


def test_the_four_methods_are_defined_once():
    for name in METHODS:
        method = getattr(LinearisedPredictive, name)
        assert getattr(KFAC, name) is getattr(Diagonal, name) is getattr(EFB, name) is method
        assert method is not getattr(Curvature, name)
        for cls in (KFAC, Diagonal, EFB):
            assert name not in cls.__dict__
        assert getattr(BlockDiagonal, name) is getattr(INF, name) is getattr(Curvature, name)


def test_the_api_documentation_stays_on_curvature():
    for name in METHODS:
        doc = Curvature.__dict__[name].__doc__
        assert doc and len(doc) > 400 and name.split("_")[-1] in doc       # (the API documentation, not a one-line pointer)


def test_every_estimator_names_itself_literally():
    model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(8, 3))

    class Mine(KFAC):
        pass
    assert Mine(model)._predictive_terms().name == "KFAC"
    assert Diagonal(model)._predictive_terms().name == "Diagonal"
    assert EFB(model, {}, eigvecs={})._predictive_terms().name == "EFB"
    assert KFAC(model)._predictive_terms().grid_missing and not Diagonal(model)._predictive_terms().grid_missing


def test_dropping_the_kept_state():
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 3, padding=1), torch.nn.Flatten(), torch.nn.Linear(75, 4))
    diag = Diagonal(model, per_sample=True)
    model(torch.randn(3, 2, 5, 5)).sum().backward()
    diag.inv_state = {l: torch.ones(l.weight.shape[0], l.weight[0].numel() + 1) for l in (model[0], model[2])}
    record, hooks = diag.record, diag.hooks
    assert not getattr(diag, "_predictive_kept", None)
    diag.drop_predictive_state()                                       # nothing kept yet: fine
    diag._kept()["variance"] = dict(key=(), xs=[torch.zeros(1)], ws=[None])
    diag._kept()["covariance"] = dict(key=(), count=2, staged=set())
    assert set(diag._predictive_kept) == {"variance", "covariance"}
    for _ in range(2):
        diag.drop_predictive_state()
        assert not getattr(diag, "_predictive_kept", None)
        assert diag.record is record and diag.hooks is hooks and len(hooks) == 4 and set(record) == {model[0], model[2]}
    BlockDiagonal(model).drop_predictive_state()                       # the drivers call it on whatever they are given


def test_the_three_old_attributes_are_gone():
    files = glob.glob(os.path.join(ROOT, "curvature_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py"))
    assert len(files) > 20
    for path in files:
        with open(path) as fh:
            text = fh.read()
        for name in ("_variance" + "_inputs", "_variance_grid" + "_inputs", "_covariance" + "_outputs"):
            assert name not in text, (path, name)
