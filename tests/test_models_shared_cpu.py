"""What SVR and OneClassSVM share (dpsvm_amd/models/_base.py): one refusal list, four resolved settings, the
refused fit arguments, one decision path behind every loaded model, and the engine note taken from the native
problem kind.  CPU, n = 200 rows."""
import numpy as np
import pytest

from dpsvm_amd import OneClassSVM, SVR, load_model, load_one_class, load_svr
from dpsvm_amd.models import _base

ESTIMATORS = [SVR, OneClassSVM]
# one setting per entry of the shared list, in its order
REFUSED = [dict(clip="independent"), dict(solver="smo"), dict(ws_blocks=8), dict(shrink="on"),
           dict(ws_recompute="on"), dict(class_weight={1: 2.0}), dict(cache_lines=100), dict(engines="all"),
           dict(x_mode="partitioned"), dict(exchange="peer"), dict(checkpoint_every=5)]
MORE_REFUSED = [dict(force_cache=True), dict(host_cache_lines=10), dict(dp="shard"), dict(force_collectives=True),
                dict(checkpoint_path="x.ckpt")]


@pytest.fixture(scope="module")
def X():
    return np.random.default_rng(3).standard_normal((200, 5)).astype(np.float32)


def test_the_refusal_list_is_covered():
    assert len(REFUSED) == len(_base._REFUSED)


@pytest.mark.parametrize("kw", REFUSED + MORE_REFUSED, ids=lambda kw: next(iter(kw)))
@pytest.mark.parametrize("est", ESTIMATORS)
def test_shared_refusals_name_the_estimator(est, kw):
    with pytest.raises(NotImplementedError, match="^" + est.__name__ + ": "):
        est(device="cpu", **kw)


@pytest.mark.parametrize("est", ESTIMATORS)
def test_shared_settings_resolve(est):
    gp = est(device="cpu").get_params()
    assert (gp["solver"], gp["ws_blocks"], gp["shrink"], gp["ws_recompute"]) == ("ws", 1, "off", "off")
    assert gp["clip"] == "box"


@pytest.mark.parametrize("arg", ["comm", "resume", "rank_rows", "sample_weight"])
@pytest.mark.parametrize("est", ESTIMATORS)
def test_shared_fit_arguments_are_refused(est, arg, X):
    m = est(device="cpu")
    with pytest.raises(NotImplementedError, match="^" + est.__name__ + ": " + arg):
        m.fit(X, X[:, 0], **{arg: 1})
    assert not hasattr(m, "alpha_")


def test_loaded_models_share_one_decision_path(X, tmp_path):
    m = OneClassSVM(nu=0.2, gamma=0.3, device="cpu").fit(X)
    path = str(tmp_path / "oc.model")
    m.save(path)
    Xt = np.random.default_rng(4).standard_normal((50, 5)).astype(np.float32)
    dec = load_model(path, device="cpu").decision_function(Xt)
    assert dec.dtype == np.float32 and dec.shape == (50,)
    np.testing.assert_array_equal(load_svr(path, device="cpu").predict(Xt), dec)
    np.testing.assert_array_equal(load_one_class(path, device="cpu").decision_function(Xt), dec)
    np.testing.assert_array_equal(m.decision_function(Xt), dec)


@pytest.mark.parametrize("est", ESTIMATORS)
def test_cpu_engine_note_is_the_native_problem_note(est, X, C):
    m = est(gamma=0.3, device="cpu").fit(X, X[:, 0])
    note = C.problem_note(m._params(X.shape[1]))
    assert note and m.setup_info_ == {"iteration": "cpu", "engine_note": note}
    assert C.problem_note(C.SolverParams()) == ""
