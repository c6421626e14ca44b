"""kernel="precomputed" end to end on the GPU: the caller's Gram copied into the solver's lines (setup_gram), the
one-block working-set rounds with the general-diagonal sub-problem kernels, decisions from K(test, train) by
gram_rows_dot — against scikit-learn (tests/data/sklearn_precomputed.json, bench/make_precomputed_fixture.py)
and the CPU solver (solve_cpu_gram).

Bounds: decisions and intercept within PRED_TOL = B_TOL = 1e-2 on the positive definite Grams (the bound of
tests/test_svr_gpu.py / test_oneclass_gpu.py: 10 x the fixture's recorded ``dev`` <= 1e-3, scikit-learn at tol 1e-3
against tol 1e-7); on the polynomial Gram, whose decisions reach 10, 10 x that setting's own ``dev``.
"""
import numpy as np
import pytest
import torch

from test_precomputed_cpu import (B_TOL, EPS, PRED_TOL, REFUSALS, bound, check_against_fixture, decisions, fit,
                                  fixture_script, load_fixture, make)

pytestmark = pytest.mark.gpu

NOTE = "precomputed Gram: general diagonal, one block"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def cpu_fits(fx):
    return [fit(make(s["kind"], device="cpu"), s["kind"], fx["grams"][s["gram"]][0], fx) for s in fx["settings"]]


def check_setup(m, wss=None, q=None):
    si = m.setup_info_
    assert si["kernel"] == "precomputed" and si["gram"] == "precomputed"
    assert si["iteration"] == "ws-dense" and si["ws_rows"] == "gram" and si["ws_blocks"] == 1
    assert NOTE in si["engine_note"]
    if wss is not None:
        assert si["ws_wss"] == wss
    if q is not None:
        assert si["ws_q_max"] == q
    for st in (m.stats_ if isinstance(m.stats_, list) else [m.stats_]):
        assert st["t_gram"] == 0 and st["gram_reused"] is True


# ---------------------------------------------------------------- 1. parity, 2. setup and reuse
@pytest.mark.parametrize("ws_size", [192, 48])
@pytest.mark.parametrize("wss", [1, 2])
@pytest.mark.parametrize("k", range(7))
def test_precomputed_gpu_matches_sklearn_and_cpu(fx, cpu_fits, k, wss, ws_size):
    s, ref = fx["settings"][k], cpu_fits[k]
    K, Kt = fx["grams"][s["gram"]]
    m = fit(make(s["kind"], device="cuda", ws_wss=wss, ws_size=ws_size), s["kind"], K, fx)
    assert m.converged_ and m.status_ == 1
    check_setup(m, wss, ws_size)
    check_against_fixture(m, s, K, Kt, f"gpu wss {wss} q {ws_size}")
    tol = bound(s)
    c_train = float(np.max(np.abs(decisions(m, s["kind"], K) - decisions(ref, s["kind"], K))))
    c_test = float(np.max(np.abs(decisions(m, s["kind"], Kt) - decisions(ref, s["kind"], Kt))))
    c_b = abs(float(m.b_) - float(ref.b_))
    print(f"  vs cpu max |d decision| {c_train:.3g} / {c_test:.3g} |d b| {c_b:.3g}; rounds {m.n_rounds_}")
    assert c_train < tol and c_test < tol and c_b < tol
    assert m.gamma_ is None and not hasattr(m, "support_vectors_") and m.intercept_ == -m.b_
    if s["kind"] == "svc":
        acc = float(np.mean(np.where(decisions(m, "svc", K) >= 0, 1.0, -1.0) == fx["y"][:fx["n"]]))
        assert abs(m.train_accuracy() - acc) <= 0.02  # from the gradient: rows within the band may differ
    if s["kind"] == "oneclass":
        assert float(np.max(np.abs(m.train_decision_ - m.decision_function(K)))) < PRED_TOL
        assert abs(float(np.sum(m.alpha_.astype(np.float64))) - 0.2 * fx["n"]) < 1e-2
    if s["kind"] == "svr":
        assert m.score(Kt, fx["z"][fx["n"]:]) > 0.5


def test_oneclass_nu_path_on_one_upload(fx):
    K, _ = fx["grams"]["scaled"]
    m = make("oneclass", device="cuda")
    path = m.nu_path(K, [0.1, 0.2, 0.4])
    assert [st["gram_reused"] for st in m.path_stats_] == [True, True, True]
    assert m.path_setup_info_["kernel"] == "precomputed"
    one = fit(make("oneclass", device="cuda"), "oneclass", K, fx)
    np.testing.assert_array_equal(m.path_alpha_[1].view(np.uint32), one.alpha_.view(np.uint32))
    assert path["rho"][1] == one.offset_ and path["n_support"][0] < path["n_support"][2]


# ---------------------------------------------------------------- 3. strided input
def test_strided_and_device_input_are_bit_equal(fx):
    """n = 601 rows (no multiple of 4) with ld = n + 3 and NaN in the padding, as a GPU tensor view; the same Gram
    contiguous on the GPU and as a numpy array: bit-equal fits"""
    X = fx["X"][:601]
    y = fx["y"][:601]
    K = fixture_script().grams(X, 601)["scaled"][0]
    n = 601
    base = torch.full((n, n + 3), float("nan"), dtype=torch.float32, device="cuda")
    base[:, :n] = torch.from_numpy(K).cuda()
    view = base[:, :n]
    assert view.stride(0) == n + 3 and not view.is_contiguous()
    fits = [make("svc", device="cuda").fit(Kin, y) for Kin in (K, torch.from_numpy(K).cuda(), view)]
    for m in fits:
        assert m.converged_
        check_setup(m)
    for m in fits[1:]:
        np.testing.assert_array_equal(m.alpha_.view(np.uint32), fits[0].alpha_.view(np.uint32))
        assert m.b_ == fits[0].b_
    # decisions straight from a GPU tensor (strided) and from the host copy: the same kernel, the same bits
    Kt = K[:50]
    dev_view = base[:50, :n]
    np.testing.assert_array_equal(fits[0].decision_function(dev_view).view(np.uint32),
                                  fits[0].decision_function(Kt).view(np.uint32))
    with pytest.raises(ValueError, match="float32"):
        make("svc", device="cuda").fit(torch.from_numpy(K).cuda().double(), y)


# ---------------------------------------------------------------- 4. one-vs-rest on one upload
def test_one_vs_rest_on_one_upload(fx):
    n = fx["n"]
    K, Kt = fx["grams"]["scaled"]
    X = fx["X"]
    protos = X[[0, 1, 2]]
    y3 = np.argmin(((X[:, None, :] - protos[None]) ** 2).sum(-1), axis=1)
    m = make("svc", device="cuda").fit(torch.from_numpy(K).cuda(), y3[:n])
    assert m.alpha_.shape == (3, n) and len(m.stats_) == 3 and m.converged_
    check_setup(m)
    for c in range(3):
        one = make("svc", device="cuda").fit(K, np.where(y3[:n] == c, 1.0, -1.0))
        np.testing.assert_array_equal(one.alpha_.view(np.uint32), m.alpha_[c].view(np.uint32))
        assert one.b_ == m.b_[c]
    dec = m.decision_function(Kt)
    assert dec.shape == (200, 3) and dec.dtype == np.float32
    ref = Kt.astype(np.float64) @ (m.alpha_ * m._Ys).astype(np.float64).T - m.b_.astype(np.float64)
    assert float(np.max(np.abs(dec - ref))) < 1e-5
    assert m.score(Kt, y3[n:]) > 0.8
    assert abs(m.train_accuracy() - m.score(K, y3[:n])) <= 0.02


# ---------------------------------------------------------------- 5. weights, cross-validation, probabilities
def test_weights_match_cpu(fx):
    n = fx["n"]
    K, Kt = fx["grams"]["scaled"]
    y = fx["y"][:n]
    rng = np.random.default_rng(5)
    w = rng.uniform(0.25, 2.0, size=n)
    w[[4, 40]] = 0.0
    g = make("svc", device="cuda", class_weight="balanced").fit(K, y, sample_weight=w)
    c = make("svc", device="cpu", class_weight="balanced").fit(K, y, sample_weight=w)
    check_setup(g)
    assert g.alpha_[4] == 0 and g.alpha_[40] == 0 and np.all(g.alpha_ <= g.row_C_)
    np.testing.assert_array_equal(g.row_C_, c.row_C_)
    e = float(np.max(np.abs(g.decision_function(Kt) - c.decision_function(Kt))))
    print(f"weighted: gpu vs cpu max |d decision| {e:.3g} |d b| {abs(g.b_ - c.b_):.3g}")
    assert e < PRED_TOL and abs(g.b_ - c.b_) < B_TOL


def test_cross_val_decision_equals_fits_on_sub_grams(fx):
    n = fx["n"]
    K, _ = fx["grams"]["scaled"]
    y = fx["y"][:n]
    est = make("svc", device="cuda")
    dec = est.cross_val_decision(K, y, cv=3)
    assert [st["gram_reused"] for st in est.cv_stats_] == [True] * 3 and est.cv_setup_info_["kernel"] == "precomputed"
    for te in est.cv_folds_:
        tr = np.setdiff1d(np.arange(n), te)
        sub = make("svc", device="cuda").fit(np.ascontiguousarray(K[np.ix_(tr, tr)]), y[tr])
        ref = sub.decision_function(np.ascontiguousarray(K[np.ix_(te, tr)]))
        e = float(np.max(np.abs(dec[te] - ref)))
        print(f"fold of {len(te)}: cross_val_decision vs a fit on the sub-Gram max |d decision| {e:.3g}")
        assert e < PRED_TOL
    assert est.cross_val_score(K, y, cv=3) > 0.75


def test_probability_fit(fx):
    n = fx["n"]
    K, Kt = fx["grams"]["rbf"]
    y = fx["y"][:n]
    m = make("svc", device="cuda").fit(K, y, probability=3)
    P = m.predict_proba(Kt)
    assert P.shape == (200, 2) and P.dtype == np.float32 and np.allclose(P.sum(axis=1), 1.0, atol=1e-6)
    plain = make("svc", device="cuda").fit(K, y)
    np.testing.assert_array_equal(m.alpha_.view(np.uint32), plain.alpha_.view(np.uint32))
    assert m.b_ == plain.b_ and m.cv_decision_.shape == (n,)
    # the sigmoid of the decisions, and the class it favours agrees with predict where the model is decided
    d = m.decision_function(Kt).astype(np.float64)
    np.testing.assert_allclose(P[:, 1], 1.0 / (1.0 + np.exp(m.probA_ * d + m.probB_)), atol=1e-5)
    assert m.train_accuracy() == plain.train_accuracy()


# ---------------------------------------------------------------- 6. errors
def test_refusals_and_errors_gpu(fx, C):
    K, Kt = fx["grams"]["rbf"]
    y = fx["y"][:fx["n"]]
    for kw, names in REFUSALS:
        with pytest.raises(NotImplementedError, match=names):
            make("svc", device="cuda", **kw).fit(K, y)
    for kw in (dict(comm=object()), dict(resume="ck.bin"), dict(rank_rows=10)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            make("svc", device="cuda").fit(K, y, **kw)
    with pytest.raises(ValueError, match="square"):
        make("svc", device="cuda").fit(K[:, :-1], y)
    # one entry changed by one ulp — one of the pairs of setup's fixed sample (symmetry is a precondition: the
    # sample is a tripwire, not a proof)
    i, j = next((int(a), int(b)) for a, b in C.gram_sym_pairs(len(K)) if a != b)
    bad = K.copy()
    bad[i, j] = np.nextafter(bad[i, j], np.float32(2))
    with pytest.raises(ValueError, match="symmetric"):
        make("svc", device="cuda").fit(bad, y)
    bad = K.copy()
    bad[9, 9] = np.nan
    with pytest.raises(ValueError, match="diagonal"):
        make("svc", device="cuda").fit(torch.from_numpy(bad).cuda(), y)
    m = make("svc", device="cuda").fit(K, y)
    with pytest.raises(ValueError, match="columns"):
        m.decision_function(Kt[:, :-1])
    with pytest.raises(NotImplementedError, match="precomputed"):
        m.save("model.txt")
    # the native solver: the X-based calls, release_cache, plain setup() and a multi-block request refuse
    p = C.SolverParams()
    p.kernel, p.clip, p.eps = 1, C.ClipMode.box, EPS
    s = C.GpuSolver(p, None, 0)
    with pytest.raises(RuntimeError, match="setup_gram"):
        s.setup(fx["X"][:fx["n"]], fx["n"], y)
    s = C.GpuSolver(p, None, 0)
    info = s.setup_gram(K, y)
    assert info["kernel"] == "precomputed" and info["ws_wss"] == 2 and info["ws_blocks"] == 1
    alpha, st = s.solve()
    assert st["converged"] and st["gram_reused"] and st["t_gram"] == 0
    np.testing.assert_array_equal(np.asarray(alpha).view(np.uint32), m.alpha_.view(np.uint32))
    for call, what in ((lambda: s.release_cache(), "release_cache"), (lambda: s.train_accuracy(alpha, st["b"]), "X"),
                       (lambda: s.decision(alpha, st["b"], fx["X"][:4]), "X")):
        with pytest.raises(RuntimeError, match=what):
            call()
    p.ws_blocks = 4
    with pytest.raises(RuntimeError, match="ws_blocks"):
        C.GpuSolver(p, None, 0).setup_gram(K, y)
