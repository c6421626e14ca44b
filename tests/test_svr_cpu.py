"""epsilon-SVR on the CPU solver (device="cpu"): the folded 2n-row dual against scikit-learn.

Reference: tests/data/sklearn_svr.json (bench/make_svr_fixture.py: sklearn.svm.SVR, tol 1e-7, float64) —
500 x 8 training rows, 200 held-out rows, three settings.  Bounds: predictions and intercept within 1e-2,
what tests/test_weights_gpu.py allows between a solver at stop tolerance 1e-3 and a reference at 1e-7.
"""
import json
import os

import numpy as np
import pytest

from ref_svr import fold_labels, fold_start, svr_predict, svr_reference

EPS = 1e-3
PRED_TOL = 1e-2
B_TOL = 1e-2


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "sklearn_svr.json")) as f:
        d = json.load(f)
    d["X"] = np.array(d["X"], dtype=np.float32)
    d["z"] = np.array(d["z"], dtype=np.float32)
    d["X_test"] = np.array(d["X_test"], dtype=np.float32)
    return d


@pytest.fixture(scope="module")
def fits(fx):
    """the three settings' CPU fits, shared by the tests below"""
    from dpsvm_amd import SVR

    return [SVR(C=s["C"], gamma=s["gamma"], epsilon=s["epsilon"], eps=EPS, device="cpu").fit(fx["X"], fx["z"])
            for s in fx["settings"]]


@pytest.mark.parametrize("k", [0, 1, 2])
def test_svr_cpu_matches_sklearn(fx, fits, k):
    """Measured maxima (CPU solver against the fixture; train / held-out predictions, intercept):
    C=1 gamma=0.5 epsilon=0.1: 1.6e-3 / 1.7e-3, 2.0e-4; C=10 gamma=0.125 epsilon=0.05: 3.5e-3 / 3.9e-3, 2.6e-3;
    C=1 gamma=0.5 epsilon=0: 2.0e-3 / 1.5e-3, 1.1e-4 — inside the 1e-2 bounds."""
    s, m = fx["settings"][k], fits[k]
    assert m.converged_ and m.status_ == 1
    d_train = float(np.max(np.abs(m.predict(fx["X"]) - np.array(s["pred_train"]))))
    d_test = float(np.max(np.abs(m.predict(fx["X_test"]) - np.array(s["pred_test"]))))
    d_b = abs(m.intercept_ - s["intercept"])
    print(f"setting {k}: max |d pred| train {d_train:.3g} held-out {d_test:.3g} |d intercept| {d_b:.3g} "
          f"steps {m.n_iter_} n_sv {m.n_support_} (sklearn {s['n_sv']})")
    assert m.predict(fx["X"]).dtype == np.float32
    assert d_train < PRED_TOL and d_test < PRED_TOL
    assert d_b < B_TOL
    assert m.intercept_ == -m.b_


@pytest.mark.parametrize("k", [0, 1, 2])
def test_svr_cpu_invariants(fx, fits, k):
    s, m = fx["settings"][k], fits[k]
    C = s["C"]
    n = len(fx["z"])
    assert m.alpha_.shape == (2, n) and m.alpha_.dtype == np.float32
    beta = m.alpha_[0].astype(np.float64) - m.alpha_[1]
    assert abs(beta.sum()) < 1e-2 * C  # the equality constraint, kept by the joint box
    assert np.all(m.alpha_ >= 0) and np.all(m.alpha_ <= np.float32(C))
    assert not np.any((m.alpha_[0] > 0) & (m.alpha_[1] > 0))
    # ... and on the solver's own output, before SVR removes min(alpha_j, alpha*_j): a pair (j, j + n) with both
    # positive violates by 2 epsilon, so the stop test (2 eps) leaves none whenever epsilon > eps.  At epsilon
    # = 0 the objective is flat along the common part and the solver keeps it (the documented exception)
    if s["epsilon"] > EPS:
        assert m.n_common_ == 0
    assert abs(m.n_support_ - s["n_sv"]) <= 0.02 * s["n_sv"]
    np.testing.assert_array_equal(m.support_, np.nonzero(beta != 0)[0])
    np.testing.assert_array_equal(m.dual_coef_, beta[m.support_].astype(np.float32))
    np.testing.assert_array_equal(m.support_vectors_, fx["X"][m.support_])
    assert m.n_iter_ == m.stats_["iters"] and m.fit_time_ > 0
    r2 = m.score(fx["X_test"], np.array(fx["z_test"]))
    assert abs(r2 - s["r2_test"]) < 0.01


def test_svr_native_cpu_solve_is_the_folded_dual(fx, C):
    """solve_cpu with problem = 1: alpha has 2n entries; with epsilon > eps no row keeps alpha and alpha* > 0
    by the solver's own steps; the numpy model of the folded dual agrees."""
    s = fx["settings"][0]
    X, z = fx["X"][:200], fx["z"][:200]
    p = C.SolverParams()
    p.C, p.gamma, p.eps, p.clip = s["C"], s["gamma"], EPS, C.ClipMode.box
    p.problem, p.svr_epsilon = 1, s["epsilon"]
    alpha, info = C.solve_cpu(X, z, p)
    n = len(z)
    assert alpha.shape == (2 * n,) and info["converged"]
    assert not np.any((alpha[:n] > 0) & (alpha[n:] > 0))
    for s2 in fx["settings"][:2]:  # the raw alphas of the whole fixture, every setting with epsilon > eps
        p2 = C.SolverParams()
        p2.C, p2.gamma, p2.eps, p2.clip = s2["C"], s2["gamma"], EPS, C.ClipMode.box
        p2.problem, p2.svr_epsilon = 1, s2["epsilon"]
        raw, info2 = C.solve_cpu(fx["X"], fx["z"], p2)
        assert info2["converged"] and not np.any((raw[:500] > 0) & (raw[500:] > 0))
        assert np.all(raw >= 0) and np.all(raw <= np.float32(s2["C"]))
    a_ref, b_ref, steps = svr_reference(X, z, s["C"], s["gamma"], s["epsilon"], eps=EPS)
    assert abs(info["b"] - b_ref) < B_TOL
    got = svr_predict(X, alpha.astype(np.float64), info["b"], s["gamma"], fx["X_test"])
    want = svr_predict(X, a_ref, b_ref, s["gamma"], fx["X_test"])
    assert np.max(np.abs(got - want)) < PRED_TOL
    # the start of the folded dual, as the model states it
    f0 = fold_start(z, s["epsilon"])
    np.testing.assert_allclose(f0[:n] - f0[n:], 2 * s["epsilon"], rtol=0, atol=4 * 2.0 ** -24 * (1 + np.abs(z).max()))
    assert np.all(fold_labels(n)[:n] == 1) and np.all(fold_labels(n)[n:] == -1)


def test_svr_save_load_round_trip(fx, fits, tmp_path):
    from dpsvm_amd import load_svr

    m = fits[0]
    path = str(tmp_path / "svr.model")
    m.save(path, precision=9)
    back = load_svr(path, device="cpu")
    assert back.n_support == m.n_support_
    np.testing.assert_array_equal(back.predict(fx["X_test"]), m.predict(fx["X_test"]))


@pytest.mark.parametrize("kw", [dict(epsilon=-1.0), dict(clip="independent"), dict(ws_blocks=8), dict(solver="smo"),
                                dict(shrink="on"), dict(ws_recompute="on"), dict(class_weight="balanced"),
                                dict(force_cache=True), dict(engines="all"), dict(checkpoint_every=10)])
def test_svr_refuses_settings(kw):
    from dpsvm_amd import SVR

    with pytest.raises(ValueError if "epsilon" in kw else NotImplementedError):
        SVR(device="cpu", **kw)


@pytest.mark.parametrize("arg", ["sample_weight", "comm", "resume", "rank_rows"])
def test_svr_refuses_fit_arguments(fx, C, arg):
    from dpsvm_amd import SVR

    n = len(fx["z"])
    val = {"sample_weight": np.ones(n), "comm": C.local_comm(), "resume": "nowhere.ckpt", "rank_rows": n}[arg]
    m = SVR(device="cpu")
    with pytest.raises(NotImplementedError):
        m.fit(fx["X"], fx["z"], **{arg: val})
    assert not hasattr(m, "alpha_")


def test_svr_native_refusals(fx, C):
    """the native CPU solver refuses what the folded dual does not run"""
    X, z = fx["X"][:50], fx["z"][:50]

    def params(**kw):
        p = C.SolverParams()
        p.clip, p.problem = C.ClipMode.box, 1
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    with pytest.raises(RuntimeError, match="box"):
        C.solve_cpu(X, z, params(clip=C.ClipMode.independent))
    with pytest.raises(RuntimeError, match="svr_epsilon"):
        C.solve_cpu(X, z, params(svr_epsilon=-0.5))
    with pytest.raises(RuntimeError, match="per-row C"):
        C.solve_cpu(X, z, params(), row_C=np.ones(50, np.float32))
    with pytest.raises(RuntimeError, match="problem"):
        C.solve_cpu(X, z, params(problem=2))
