"""One-class SVM end to end on the GPU: the classifier's one-block working-set rounds on the resident Gram from
the nu start, whose gradient f = K alpha_0 gram_rows_wsum reads off that Gram (gram_wsum.hip), against
scikit-learn (tests/data/sklearn_oneclass.json, bench/make_oneclass_fixture.py) and the CPU solver.

Bounds: decisions and rho within 1e-2 (PRED_TOL / B_TOL of tests/test_svr_gpu.py: two solvers at stop tolerance
1e-3; scikit-learn at tol=1e-3 differs from scikit-learn at tol=1e-7 by at most 7e-4 on these settings).
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-3
PRED_TOL = 1e-2
B_TOL = 1e-2
BAND = 1e-2   # decisions within BAND of 0 are undecided at these tolerances


def note():
    """what engine_note says about one-class: the native problem_note"""
    from dpsvm_amd._native import load

    p = load().SolverParams()
    p.one_class_nu = 0.5
    return load().problem_note(p)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "sklearn_oneclass.json")) as f:
        d = json.load(f)
    for k in ("X", "X_test"):
        d[k] = np.array(d[k], dtype=np.float32)
    return d


@pytest.fixture(scope="module")
def cpu_fits(fx):
    from dpsvm_amd import OneClassSVM

    return [OneClassSVM(nu=s["nu"], gamma=s["gamma"], eps=EPS, device="cpu").fit(fx["X"]) for s in fx["settings"]]


def check_setup(m):
    si = m.setup_info_
    assert si["iteration"] == "ws-dense" and si["ws_rows"] == "gram"
    assert si["ws_blocks"] == 1
    assert note() in si["engine_note"]


def check_invariants(m, nu, n):
    a = m.alpha_
    assert a.shape == (n,) and a.dtype == np.float32
    assert np.all(a >= 0) and np.all(a <= 1)
    assert abs(float(np.sum(a.astype(np.float64))) - nu * n) < 1e-2
    td = m.train_decision_
    assert np.mean(td < -BAND) <= nu <= np.mean(td <= BAND)   # the nu-property, with the band


@pytest.mark.parametrize("wss", [1, 2])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_oneclass_gpu_matches_sklearn_and_cpu(fx, cpu_fits, k, wss):
    from dpsvm_amd import OneClassSVM

    s, ref = fx["settings"][k], cpu_fits[k]
    n = len(fx["X"])
    m = OneClassSVM(nu=s["nu"], gamma=s["gamma"], eps=EPS, device="cuda", ws_wss=wss).fit(fx["X"])
    assert m.converged_ and m.status_ == 1
    check_setup(m)
    assert m.setup_info_["ws_wss"] == wss
    assert m.stats_["t_start"] > 0 and not m.stats_["gram_reused"]
    sk_train, sk_test = np.array(s["dec_train"]), np.array(s["dec_test"])
    d_train, d_test = m.decision_function(fx["X"]), m.decision_function(fx["X_test"])
    e_train = float(np.max(np.abs(d_train - sk_train)))
    e_test = float(np.max(np.abs(d_test - sk_test)))
    e_rho = abs(m.offset_ - s["rho"])
    c_train = float(np.max(np.abs(d_train - ref.decision_function(fx["X"]))))
    c_test = float(np.max(np.abs(d_test - ref.decision_function(fx["X_test"]))))
    e_own = float(np.max(np.abs(m.train_decision_ - d_train)))
    print(f"setting {k} wss {wss}: vs sklearn max |d decision| {e_train:.3g} / {e_test:.3g} |d rho| {e_rho:.3g}; "
          f"vs cpu {c_train:.3g} / {c_test:.3g} |d rho| {abs(m.offset_ - ref.offset_):.3g}; train_decision_ vs "
          f"decision_function {e_own:.3g}; rounds {m.n_rounds_} steps {m.n_iter_} n_sv {m.n_support_} "
          f"(sklearn {s['n_sv']}, cpu {ref.n_support_}) t_start {m.stats_['t_start'] * 1e6:.1f} us")
    assert d_train.dtype == np.float32
    assert e_train < PRED_TOL and e_test < PRED_TOL and e_rho < B_TOL
    assert c_train < PRED_TOL and c_test < PRED_TOL and abs(m.offset_ - ref.offset_) < B_TOL
    assert e_own < PRED_TOL
    check_invariants(m, s["nu"], n)
    assert m.offset_ == m.b_ and m.intercept_ == -m.b_
    # predict against the sign of the reference, where the reference is decided
    sure = np.abs(sk_test) >= BAND
    assert np.mean(~sure) <= 0.05
    np.testing.assert_array_equal(m.predict(fx["X_test"])[sure], np.where(sk_test[sure] >= 0, 1, -1))
    assert not hasattr(m, "_solver")  # the estimator does not keep the solver, and with it the Gram, alive


def big_problem(n=3000, d=20, seed=5, n_out=150):
    rng = np.random.default_rng(seed)
    X = np.concatenate([0.5 * rng.standard_normal(size=(n - n_out, d)), rng.uniform(-2, 2, size=(n_out, d))])
    return X[rng.permutation(n)].astype(np.float32)


BIG = dict(nu=0.5, gamma=0.05)


def test_oneclass_gpu_larger_shape():
    """n = 3,000, d = 20: 12 selection workgroups, ~1,500 support vectors (the 192-row set turns over), a start
    of m = 1,500 Gram rows over several slices"""
    from dpsvm_amd import OneClassSVM
    from dpsvm_amd._native import load

    X = big_problem()
    n = len(X)
    g = OneClassSVM(eps=EPS, device="cuda", **BIG).fit(X)
    c = OneClassSVM(eps=EPS, device="cpu", **BIG).fit(X)
    assert g.converged_ and c.converged_
    check_setup(g)
    assert g.setup_info_["groups"] == 12 and g.setup_info_["rows_per_group"] == 256
    assert g.n_support_ > 192 and g.n_rounds_ > 10
    assert load().k_gram_wsum_slices(n, 1500) > 1
    Xt = big_problem(n=500, seed=6, n_out=25)
    e_train = float(np.max(np.abs(g.train_decision_ - c.train_decision_)))
    e_test = float(np.max(np.abs(g.decision_function(Xt) - c.decision_function(Xt))))
    print(f"gpu vs cpu: max |d decision| {e_train:.3g} / {e_test:.3g} |d rho| {abs(g.offset_ - c.offset_):.3g}; "
          f"rounds {g.n_rounds_} steps {g.n_iter_} (cpu {c.n_iter_}) n_sv {g.n_support_} (cpu {c.n_support_})")
    assert e_train < PRED_TOL and e_test < PRED_TOL and abs(g.offset_ - c.offset_) < B_TOL
    check_invariants(g, BIG["nu"], n)


def native_params(mod, nu=0.1, gamma=0.5, **kw):
    p = mod.SolverParams()
    p.C, p.gamma, p.eps, p.clip = 1.0, gamma, EPS, mod.ClipMode.box
    p.one_class_nu = nu
    p.solver, p.ws_blocks = 2, 1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_oneclass_gpu_start_and_rounds_compose(C):
    """a solve stopped in its first rounds: the gradient is K alpha of the alpha it returns — the start read
    from the Gram plus the rounds' updates — within 1e-3, K recomputed in float64"""
    X = big_problem()
    n = len(X)
    solver = C.GpuSolver(native_params(C, max_iter=200, **BIG), None, 0)
    solver.setup(X, n, np.zeros(n, np.float32))
    alpha, info = solver.solve()
    assert info["status"] == 2 and 0 < info["outer"] < 10
    start = np.zeros(n, np.float32)
    start[:1500] = 1.0
    assert np.count_nonzero(alpha != start) >= 2   # the rounds moved it
    assert abs(float(alpha.astype(np.float64).sum()) - 1500.0) < 1e-2
    x = X.astype(np.float64)
    sq = (x * x).sum(1)
    K = np.exp(-BIG["gamma"] * np.maximum(sq[:, None] + sq[None, :] - 2.0 * (x @ x.T), 0.0))
    want = K @ alpha.astype(np.float64)
    f = solver.gradient()
    err = float(np.max(np.abs(f - want)))
    print(f"max |gradient - K alpha| = {err:.3g} (|f| up to {np.abs(want).max():.4g}); rounds {info['outer']} steps "
          f"{info['iters']}")
    assert f.shape == (n,) and err < 1e-3


def test_oneclass_gpu_nu_path_reuses_the_gram(fx):
    from dpsvm_amd import OneClassSVM

    nus = [0.1, 0.3003, 0.05]
    m = OneClassSVM(gamma=0.5, eps=EPS, device="cuda")
    path = m.nu_path(fx["X"], nus)
    assert [st["gram_reused"] for st in m.path_stats_] == [False, True, True]
    assert m.path_stats_[0]["t_gram"] > 0
    assert all(st["t_gram"] == 0.0 for st in m.path_stats_[1:])   # a solve after set_nu
    assert all(st["t_start"] > 0 and st["converged"] for st in m.path_stats_)
    for i, nu in enumerate(nus):
        fresh = OneClassSVM(nu=nu, gamma=0.5, eps=EPS, device="cuda").fit(fx["X"])
        np.testing.assert_array_equal(m.path_alpha_[i], fresh.alpha_)
        assert path["rho"][i] == fresh.offset_ and m.path_stats_[i]["iters"] == fresh.n_iter_
        assert path["n_support"][i] == fresh.n_support_
        assert path["outlier_fraction"][i] == float(np.mean(fresh.train_decision_ < 0))
    assert note() in m.path_setup_info_["engine_note"]


@pytest.mark.parametrize("kw,msg", [
    (dict(one_class_nu=1.0), r"\(0, 1\)"), (dict(one_class_nu=-0.1), r"\(0, 1\)"), (dict(C=2.0), "C must be 1"),
    (dict(clip=0), "box"), (dict(ws_blocks=8), "ws_blocks"), (dict(solver=1), "solver"),
    (dict(force_cache=True), "cache"), (dict(x_mode=2), "partitioned"), (dict(checkpoint_every=5), "checkpoints"),
    (dict(problem=1), "problem")])
def test_oneclass_gpu_native_setup_refuses(fx, C, kw, msg):
    """refused by setup() before it allocates or uploads anything, with a message naming one-class"""
    if "clip" in kw:
        kw = dict(clip=C.ClipMode.independent)
    n = len(fx["X"])
    free0 = torch.cuda.mem_get_info()[0]
    solver = C.GpuSolver(native_params(C, **kw), None, 0)
    with pytest.raises(RuntimeError, match="one-class.*" + msg):
        solver.setup(fx["X"], n, np.zeros(n, np.float32))
    del solver
    assert torch.cuda.mem_get_info()[0] >= free0 - (8 << 20)


def test_oneclass_gpu_nu_zero_is_a_plain_classifier(fx, C):
    """one_class_nu = 0 is off, not an error: the labels count and nothing of one-class runs"""
    n = len(fx["X"])
    y = np.where(fx["X"][:, 0] > 0, 1.0, -1.0).astype(np.float32)
    free0 = torch.cuda.mem_get_info()[0]
    solver = C.GpuSolver(native_params(C, nu=0.0), None, 0)
    info = solver.setup(fx["X"], n, y)
    assert "one-class" not in info["engine_note"]
    alpha, res = solver.solve()
    assert res["converged"] and res["t_start"] == 0.0
    assert solver.train_accuracy(alpha, res["b"]) > 0.9
    with pytest.raises(RuntimeError, match="one-class"):
        solver.set_nu(0.2)
    del solver
    assert torch.cuda.mem_get_info()[0] >= free0 - (8 << 20)


def test_oneclass_gpu_refuses_resume_and_classifier_only_calls(fx, C):
    n = len(fx["X"])
    solver = C.GpuSolver(native_params(C), None, 0)
    solver.setup(fx["X"], n, np.zeros(n, np.float32))
    alpha, info = solver.solve()
    assert info["converged"]
    for call in (lambda: solver.solve(C.Checkpoint()),
                 lambda: solver.set_row_C(np.ones(n, np.float32)),
                 lambda: solver.train_accuracy(alpha, info["b"]),
                 lambda: solver.holdout_decisions(np.arange(5, dtype=np.int32), 0.0, 0),
                 lambda: solver.platt_fit(0),
                 lambda: solver.set_labels(np.ones(n, np.float32)),
                 lambda: solver.set_nu(1.0)):
        with pytest.raises(RuntimeError, match="one-class"):
            call()
    # gradient() and decision() serve as they are: f - rho on the training rows is the decision
    f = solver.gradient()
    dec = solver.decision(alpha, info["b"], fx["X"])
    assert float(np.max(np.abs((f.astype(np.float64) - info["b"]) - dec))) < PRED_TOL
    # the solver is as it was: the same solve again (the Gram rebuilt: nothing asked to keep it)
    again, info2 = solver.solve()
    np.testing.assert_array_equal(again, alpha)
    assert not info2["gram_reused"]


def test_oneclass_gpu_save_load(fx, tmp_path):
    from dpsvm_amd import OneClassSVM, load_one_class

    m = OneClassSVM(nu=0.1, gamma=0.5, eps=EPS, device="cuda").fit(fx["X"])
    path = str(tmp_path / "oneclass.model")
    m.save(path)
    back = load_one_class(path, device="cuda")
    np.testing.assert_array_equal(back.decision_function(fx["X_test"]), m.decision_function(fx["X_test"]))
    np.testing.assert_array_equal(back.predict(fx["X_test"]), m.predict(fx["X_test"]))
    assert back.n_support == m.n_support_


@pytest.mark.parametrize("kw", [dict(clip="independent"), dict(ws_blocks=8), dict(solver="smo")])
def test_oneclass_gpu_estimator_refuses(kw):
    from dpsvm_amd import OneClassSVM

    with pytest.raises(NotImplementedError):
        OneClassSVM(device="cuda", **kw)
