"""epsilon-SVR end to end on the GPU: the folded 2n-row dual on one-block working-set rounds over the resident
n x n Gram (ws_select_fold_kernel, ws_gather_kernel<true>, init_f_svr), against scikit-learn
(tests/data/sklearn_svr.json, bench/make_svr_fixture.py) and the CPU solver.

Bounds: predictions and threshold within 1e-2 (tests/test_weights_gpu.py's for two solvers at stop tolerance
1e-3); R^2 on held-out rows within 0.01 of scikit-learn's.
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


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "sklearn_svr.json")) as f:
        d = json.load(f)
    for k in ("X", "z", "X_test", "z_test"):
        d[k] = np.array(d[k], dtype=np.float32)
    return d


@pytest.fixture(scope="module")
def cpu_fits(fx):
    from dpsvm_amd import SVR

    return [SVR(C=s["C"], gamma=s["gamma"], epsilon=s["epsilon"], eps=EPS, device="cpu").fit(fx["X"], fx["z"])
            for s in fx["settings"]]


def big_problem(n=3000, nt=500, d=20, seed=11):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, size=(n + nt, d)).astype(np.float32)
    x = X.astype(np.float64)
    z = np.sin(2 * x[:, 0]) + x[:, 1] * x[:, 2] + 0.5 * np.cos(2 * x[:, 3] + x[:, 4]) - 0.3 * x[:, 5] ** 2
    z = (z + 0.1 * rng.standard_normal(n + nt)).astype(np.float32)
    return X[:n], z[:n], X[n:], z[n:]


def check_setup(m):
    si = m.setup_info_
    assert si["iteration"] == "ws-dense" and si["ws_rows"] == "gram"
    assert si["ws_blocks"] == 1
    from dpsvm_amd._native import load

    p = load().SolverParams()
    p.problem = 1
    assert load().problem_note(p) and load().problem_note(p) in si["engine_note"]
    assert si["n"] == m.alpha_.shape[1]  # the Gram's rows: n, not 2n


@pytest.mark.parametrize("wss", [1, 2])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_svr_gpu_matches_sklearn_and_cpu(fx, cpu_fits, k, wss):
    from dpsvm_amd import SVR

    s, ref = fx["settings"][k], cpu_fits[k]
    m = SVR(C=s["C"], gamma=s["gamma"], epsilon=s["epsilon"], eps=EPS, device="cuda", ws_wss=wss)
    m.fit(fx["X"], fx["z"])
    assert m.converged_ and m.status_ == 1
    check_setup(m)
    assert m.setup_info_["ws_wss"] == wss
    p_train, p_test = m.predict(fx["X"]), m.predict(fx["X_test"])
    d_train = float(np.max(np.abs(p_train - np.array(s["pred_train"]))))
    d_test = float(np.max(np.abs(p_test - np.array(s["pred_test"]))))
    d_b = abs(m.intercept_ - s["intercept"])
    c_train = float(np.max(np.abs(p_train - ref.predict(fx["X"]))))
    c_test = float(np.max(np.abs(p_test - ref.predict(fx["X_test"]))))
    print(f"setting {k} wss {wss}: vs sklearn max |d pred| {d_train:.3g} / {d_test:.3g} |d intercept| {d_b:.3g}; "
          f"vs cpu {c_train:.3g} / {c_test:.3g} |d b| {abs(m.b_ - ref.b_):.3g}; rounds {m.n_rounds_} steps "
          f"{m.n_iter_} n_sv {m.n_support_} (sklearn {s['n_sv']}, cpu {ref.n_support_})")
    assert p_train.dtype == np.float32
    assert d_train < PRED_TOL and d_test < PRED_TOL and d_b < B_TOL
    assert c_train < PRED_TOL and c_test < PRED_TOL and abs(m.b_ - ref.b_) < B_TOL
    # the invariants of the dual
    C = s["C"]
    n = len(fx["z"])
    assert m.alpha_.shape == (2, n)
    assert np.all(m.alpha_ >= 0) and np.all(m.alpha_ <= np.float32(C))
    assert not np.any((m.alpha_[0] > 0) & (m.alpha_[1] > 0))
    if s["epsilon"] > EPS:  # the solver's raw output: nothing for SVR to remove (epsilon = 0: the exception)
        assert m.n_common_ == 0
    assert abs(float(np.sum(m.alpha_[0].astype(np.float64) - m.alpha_[1]))) < 1e-2 * C
    assert abs(m.n_support_ - s["n_sv"]) <= 0.02 * s["n_sv"]


def test_svr_gpu_larger_shape_turns_the_working_set_over():
    """n = 3,000, d = 20: ~1,900 support vectors (the 192-row set turns over many times) and 2n = 6,000 state
    rows on 12 selection workgroups of the n columns"""
    from sklearn.svm import SVR as SkSVR

    from dpsvm_amd import SVR

    X, z, Xt, zt = big_problem()
    kw = dict(C=1.0, gamma=0.1, epsilon=0.1, eps=EPS)
    g = SVR(device="cuda", **kw).fit(X, z)
    c = SVR(device="cpu", **kw).fit(X, z)
    assert g.converged_ and c.converged_
    check_setup(g)
    assert g.setup_info_["groups"] == 12 and g.setup_info_["rows_per_group"] == 256
    assert g.n_support_ > 192 and g.n_rounds_ > 10
    d_pred = float(np.max(np.abs(g.predict(Xt) - c.predict(Xt))))
    print(f"gpu vs cpu: max |d pred| {d_pred:.3g} |d b| {abs(g.b_ - c.b_):.3g}; rounds {g.n_rounds_} steps "
          f"{g.n_iter_} (cpu {c.n_iter_}) n_sv {g.n_support_} (cpu {c.n_support_})")
    assert d_pred < PRED_TOL and abs(g.b_ - c.b_) < B_TOL
    sk = SkSVR(kernel="rbf", C=1.0, gamma=0.1, epsilon=0.1, tol=1e-3).fit(X.astype(np.float64), z.astype(np.float64))
    r2_sk = sk.score(Xt.astype(np.float64), zt.astype(np.float64))
    r2 = g.score(Xt, zt)
    print(f"R^2 held-out: gpu {r2:.5f} sklearn {r2_sk:.5f}")
    assert abs(r2 - r2_sk) < 0.01
    assert g.n_common_ == 0 and c.n_common_ == 0
    assert not hasattr(g, "_solver")  # the estimator does not keep the solver, and with it the Gram, alive


@pytest.mark.parametrize("wss", [1, 2])
@pytest.mark.parametrize("k", [0, 1])
def test_svr_gpu_raw_alphas_of_the_native_solve(fx, C, k, wss):
    """GpuSolver.solve() itself, with epsilon > eps: the eta = 0 pairs (j, j + n) that the sub-problem's joint
    box resolves leave no row with alpha_j and alpha*_j both positive, the box holds, and the gradient's halves
    keep f[j] - f[j + n] = 2 epsilon (every round adds one value to both)."""
    s = fx["settings"][k]
    n = len(fx["z"])
    solver = C.GpuSolver(native_params(C, s, ws_wss=wss), None, 0)
    solver.setup(fx["X"], n, fx["z"])
    raw, info = solver.solve()
    assert info["converged"] and raw.shape == (2 * n,)
    assert not np.any((raw[:n] > 0) & (raw[n:] > 0))
    assert np.all(raw >= 0) and np.all(raw <= np.float32(s["C"]))
    assert abs(float(np.sum(raw[:n].astype(np.float64) - raw[n:]))) < 1e-2 * s["C"]
    f = solver.gradient()
    assert f.shape == (2 * n,)
    assert float(np.max(np.abs((f[:n].astype(np.float64) - f[n:]) - 2 * s["epsilon"]))) < 1e-4


def native_params(C, s, **kw):
    p = C.SolverParams()
    p.C, p.gamma, p.eps, p.clip = s["C"], s["gamma"], EPS, C.ClipMode.box
    p.problem, p.svr_epsilon = 1, s["epsilon"]
    p.solver, p.ws_blocks = 2, 1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_svr_gpu_target_swap_keeps_the_gram(fx, C):
    s = fx["settings"][0]
    X, z = fx["X"], fx["z"]
    z2 = (np.cos(3.0 * X[:, 0]) - 0.5 * X[:, 1]).astype(np.float32)
    n = len(z)
    a = C.GpuSolver(native_params(C, s), None, 0)
    a.setup(X, n, z)
    alpha1, info1 = a.solve()
    assert alpha1.shape == (2 * n,) and info1["converged"] and not info1["gram_reused"]
    a.set_labels(z2)
    alpha2, info2 = a.solve()
    assert info2["converged"] and info2["gram_reused"] and info2["t_gram"] == 0.0
    b = C.GpuSolver(native_params(C, s), None, 0)
    b.setup(X, n, z2)
    alpha_fresh, info_fresh = b.solve()
    np.testing.assert_array_equal(alpha2, alpha_fresh)
    assert info2["b"] == info_fresh["b"] and info2["iters"] == info_fresh["iters"]
    assert np.any(alpha2 != alpha1)
    # a solve without a swap builds the Gram again and repeats itself
    alpha3, info3 = a.solve()
    assert not info3["gram_reused"]
    np.testing.assert_array_equal(alpha3, alpha2)


def test_svr_gpu_save_load_predict(fx, tmp_path):
    from dpsvm_amd import SVR, load_svr

    s = fx["settings"][0]
    m = SVR(C=s["C"], gamma=s["gamma"], epsilon=s["epsilon"], eps=EPS, device="cuda").fit(fx["X"], fx["z"])
    path = str(tmp_path / "svr.model")
    m.save(path)
    back = load_svr(path, device="cuda")
    np.testing.assert_array_equal(back.predict(fx["X_test"]), m.predict(fx["X_test"]))
    assert back.n_support == m.n_support_


@pytest.mark.parametrize("kw,msg", [
    (dict(clip=0), "box"), (dict(ws_blocks=8), "ws_blocks"), (dict(ws_blocks=0), "ws_blocks"),
    (dict(solver=1), "solver"), (dict(solver=0), "solver"), (dict(svr_epsilon=-1.0), "svr_epsilon"),
    (dict(force_cache=True), "cache"), (dict(cache_lines=1000), "cache"), (dict(exchange=2), "peer exchange"),
    (dict(force_collectives=True), "collectives"), (dict(x_mode=2), "partitioned"),
    (dict(checkpoint_every=5), "checkpoints"), (dict(problem=2), "problem")])
def test_svr_gpu_native_setup_refuses(fx, C, kw, msg):
    """refused by setup() before it allocates or uploads anything"""
    s = fx["settings"][0]
    if "clip" in kw:
        kw = dict(clip=C.ClipMode.independent)
    free0 = torch.cuda.mem_get_info()[0]
    solver = C.GpuSolver(native_params(C, s, **kw), None, 0)
    with pytest.raises(RuntimeError, match=msg):
        solver.setup(fx["X"], len(fx["z"]), fx["z"])
    del solver
    assert torch.cuda.mem_get_info()[0] >= free0 - (8 << 20)


def test_svr_gpu_refuses_classifier_only_calls(fx, C):
    s = fx["settings"][0]
    n = len(fx["z"])
    solver = C.GpuSolver(native_params(C, s), None, 0)
    solver.setup(fx["X"], n, fx["z"])
    alpha, info = solver.solve()
    for call in (lambda: solver.set_row_C(np.ones(n, np.float32)),
                 lambda: solver.train_accuracy(alpha[:n], info["b"]),
                 lambda: solver.decision(alpha[:n], info["b"], fx["X_test"]),
                 lambda: solver.holdout_decisions(np.arange(5, dtype=np.int32), 0.0, 0),
                 lambda: solver.platt_fit(0),
                 lambda: solver.set_nu(0.2),
                 lambda: solver.solve(C.Checkpoint())):
        with pytest.raises(RuntimeError, match="regression|epsilon-SVR"):
            call()
    # the solver is as it was: the same solve again
    again, _ = solver.solve()
    np.testing.assert_array_equal(again, alpha)


@pytest.mark.parametrize("kw", [dict(clip="independent"), dict(ws_blocks=8), dict(solver="smo")])
def test_svr_gpu_estimator_refuses(kw):
    from dpsvm_amd import SVR

    with pytest.raises(NotImplementedError):
        SVR(device="cuda", **kw)
