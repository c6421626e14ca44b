"""One-class SVM on the CPU solver (device="cpu", the GPU tests' oracle) against scikit-learn
(tests/data/sklearn_oneclass.json, bench/make_oneclass_fixture.py).

Bounds: decisions and rho within 1e-2 (PRED_TOL / B_TOL of tests/test_svr_gpu.py: two solvers at stop tolerance
1e-3; scikit-learn at tol=1e-3 differs from scikit-learn at tol=1e-7 by at most 7e-4 on these settings).
"""
import json
import os

import numpy as np
import pytest

EPS = 1e-3
PRED_TOL = 1e-2
B_TOL = 1e-2
BAND = 1e-2   # decisions within BAND of 0 are undecided at these tolerances


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "sklearn_oneclass.json")) as f:
        d = json.load(f)
    for k in ("X", "X_test"):
        d[k] = np.array(d[k], dtype=np.float32)
    return d


@pytest.fixture(scope="module")
def fits(fx):
    from dpsvm_amd import OneClassSVM

    return [OneClassSVM(nu=s["nu"], gamma=s["gamma"], eps=EPS, device="cpu").fit(fx["X"]) for s in fx["settings"]]


def check_invariants(m, nu, n):
    a = m.alpha_
    assert a.shape == (n,) and a.dtype == np.float32
    assert np.all(a >= 0) and np.all(a <= 1)
    assert abs(float(np.sum(a.astype(np.float64))) - nu * n) < 1e-2
    td = m.train_decision_
    assert np.mean(td < -BAND) <= nu <= np.mean(td <= BAND)   # the nu-property, with the band
    assert m.offset_ == m.b_ and m.intercept_ == -m.b_
    assert m.n_support_ == len(m.support_) == len(m.dual_coef_) == len(m.support_vectors_)
    np.testing.assert_array_equal(m.dual_coef_, a[m.support_])


def test_fixture_is_what_the_generator_describes(fx):
    assert fx["X"].shape == (500, 8) and fx["X_test"].shape == (200, 8)
    assert [(s["nu"], s["gamma"]) for s in fx["settings"]] == [(0.1, 0.5), (0.5, 0.125), (0.05, 1.0), (0.3003, 0.5)]
    for s in fx["settings"]:
        assert abs(s["sum_alpha"] - s["nu"] * 500) < 1e-6
        dt = np.array(s["dec_train"])
        assert np.mean(dt < -BAND) <= s["nu"] <= np.mean(dt <= BAND)
        assert np.mean(np.abs(np.array(s["dec_test"])) < BAND) <= 0.05


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_oneclass_cpu_matches_sklearn(fx, fits, k):
    s, m = fx["settings"][k], fits[k]
    n = len(fx["X"])
    assert m.converged_ and m.status_ == 1
    assert m.setup_info_["iteration"] == "cpu"
    ref_train, ref_test = np.array(s["dec_train"]), np.array(s["dec_test"])
    d_train, d_test = m.decision_function(fx["X"]), m.decision_function(fx["X_test"])
    assert d_train.dtype == np.float32
    e_train = float(np.max(np.abs(d_train - ref_train)))
    e_test = float(np.max(np.abs(d_test - ref_test)))
    e_own = float(np.max(np.abs(m.train_decision_ - d_train)))
    print(f"setting {k}: max |d decision| {e_train:.3g} / {e_test:.3g} |d rho| {abs(m.offset_ - s['rho']):.3g}; "
          f"train_decision_ vs decision_function {e_own:.3g}; steps {m.n_iter_} n_sv {m.n_support_} "
          f"(sklearn {s['n_sv']})")
    assert e_train < PRED_TOL and e_test < PRED_TOL and abs(m.offset_ - s["rho"]) < B_TOL
    assert e_own < PRED_TOL
    check_invariants(m, s["nu"], n)
    # predict against the sign of the reference, where the reference is decided
    sure = np.abs(ref_test) >= BAND
    assert np.mean(~sure) <= 0.05
    np.testing.assert_array_equal(m.predict(fx["X_test"])[sure], np.where(ref_test[sure] >= 0, 1, -1))
    np.testing.assert_array_equal(m.score_samples(fx["X_test"]), d_test + np.float32(m.offset_))


def test_oneclass_cpu_start_is_libsvms(fx, C):
    """max_iter = 1: one pair step away from the start — alpha = 1 on floor(nu n) rows, the remainder on the
    next — with f = K alpha (the start accumulated in double, then the step's two rows)"""
    X = fx["X"]
    n = len(X)
    p = C.SolverParams()
    p.clip, p.gamma, p.one_class_nu, p.max_iter = C.ClipMode.box, 0.5, 0.3003, 1
    alpha, info = C.solve_cpu(X, np.zeros(n, np.float32), p)
    assert info["iters"] == 1 and info["status"] == 2
    start = np.zeros(n, np.float32)
    start[:150] = 1.0
    start[150] = np.float32(np.float64(np.float32(0.3003)) * n - 150)
    moved = np.nonzero(alpha != start)[0]
    assert len(moved) == 2 and alpha[moved[0]] < 1.0 and alpha[moved[1]] > 0.0   # one left the prefix, one joined
    assert abs(float(alpha.astype(np.float64).sum()) - float(start.astype(np.float64).sum())) < 1e-5
    x = X.astype(np.float64)
    K = np.exp(-0.5 * ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    # the kernel values are fp32 (relative 2^-23 and a few ulps of the exponent's argument): 1e-5 of the sum
    np.testing.assert_allclose(info["f"], K @ alpha.astype(np.float64), rtol=1e-5, atol=0)


def test_oneclass_native_cpu_refusals(fx, C):
    X = fx["X"][:50]
    y = np.zeros(50, np.float32)

    def params(**kw):
        p = C.SolverParams()
        p.clip, p.one_class_nu = C.ClipMode.box, 0.2
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    for kw, msg in ((dict(clip=C.ClipMode.independent), "box"), (dict(one_class_nu=1.0), r"\(0, 1\)"),
                    (dict(one_class_nu=-0.1), r"\(0, 1\)"), (dict(C=2.0), "C must be 1"),
                    (dict(problem=1), "problem"), (dict(checkpoint_every=5), "resume")):
        with pytest.raises(RuntimeError, match="one-class.*" + msg):
            C.solve_cpu(X, y, params(**kw))
    with pytest.raises(RuntimeError, match="one-class.*per-row C"):
        C.solve_cpu(X, y, params(), row_C=np.ones(50, np.float32))
    with pytest.raises(RuntimeError, match="one-class.*resume"):
        C.solve_cpu(X, y, params(), resume=C.Checkpoint())
    with pytest.raises(RuntimeError, match="one-class.*comm"):
        C.solve_cpu(X, y, params(), comm=FakeWorld2(C))
    # nu = 0 is off: a plain classifier, which needs both labels like any other
    alpha, info = C.solve_cpu(X, np.where(np.arange(50) % 2, 1.0, -1.0).astype(np.float32), params(one_class_nu=0.0))
    assert "f" not in info and alpha.shape == (50,)


def FakeWorld2(C):
    """a two-rank host communicator (rank 0): the refusal comes before any collective"""
    ident = lambda *a: a[0]  # noqa: E731
    return C.callback_comm(0, 2, ident, ident, ident, ident, ident, lambda: None)


def test_oneclass_get_params_and_save_load(fx, fits, tmp_path):
    from dpsvm_amd import OneClassSVM, load_one_class

    m = fits[0]
    gp = m.get_params()
    assert gp["nu"] == 0.1 and gp["gamma"] == 0.5 and gp["C"] == 1.0
    assert (gp["solver"], gp["ws_blocks"], gp["clip"], gp["shrink"], gp["ws_recompute"]) == ("ws", 1, "box", "off", "off")
    assert OneClassSVM(device="cpu").get_params()["nu"] == 0.5
    path = str(tmp_path / "oneclass.model")
    m.save(path, precision=9)
    back = load_one_class(path, device="cpu")
    assert back.n_support == m.n_support_ and back.offset == pytest.approx(m.offset_, rel=1e-6)
    np.testing.assert_array_equal(back.decision_function(fx["X_test"]), m.decision_function(fx["X_test"]))
    np.testing.assert_array_equal(back.predict(fx["X_test"]), m.predict(fx["X_test"]))


@pytest.mark.parametrize("nu", [0.0, 1.0, -0.1, 1.5, float("nan")])
def test_oneclass_nu_outside_the_open_interval_is_a_value_error(nu):
    from dpsvm_amd import OneClassSVM

    with pytest.raises(ValueError, match="nu"):
        OneClassSVM(nu=nu, device="cpu")
    with pytest.raises(ValueError, match="nu"):
        OneClassSVM(device="cpu").nu_path(np.zeros((4, 2), np.float32), [0.2, nu])


@pytest.mark.parametrize("kw", [dict(clip="independent"), dict(ws_blocks=8), dict(solver="smo"), dict(shrink="on"),
                                dict(ws_recompute="on"), dict(class_weight="balanced"), dict(force_cache=True),
                                dict(engines="all"), dict(checkpoint_every=10), dict(C=2.0)])
def test_oneclass_refuses_settings(kw):
    from dpsvm_amd import OneClassSVM

    with pytest.raises(NotImplementedError):
        OneClassSVM(device="cpu", **kw)


@pytest.mark.parametrize("arg", ["sample_weight", "comm", "resume", "rank_rows"])
def test_oneclass_refuses_fit_arguments(fx, C, arg):
    from dpsvm_amd import OneClassSVM

    n = len(fx["X"])
    val = {"sample_weight": np.ones(n), "comm": C.local_comm(), "resume": "nowhere.ckpt", "rank_rows": n}[arg]
    m = OneClassSVM(device="cpu")
    with pytest.raises(NotImplementedError):
        m.fit(fx["X"], **{arg: val})
    assert not hasattr(m, "alpha_")


def test_oneclass_cpu_nu_path(fx, fits):
    from dpsvm_amd import OneClassSVM

    nus = [0.1, 0.3003]
    m = OneClassSVM(gamma=0.5, eps=EPS, device="cpu")
    path = m.nu_path(fx["X"], nus)
    assert path["nu"] == nus and len(m.path_stats_) == 2
    for i, k in enumerate((0, 3)):   # the fixture's settings with gamma = 0.5
        np.testing.assert_array_equal(m.path_alpha_[i], fits[k].alpha_)
        assert path["rho"][i] == fits[k].offset_ and path["n_support"][i] == fits[k].n_support_
        assert path["outlier_fraction"][i] == float(np.mean(fits[k].train_decision_ < 0))
    assert not hasattr(m, "alpha_")
