"""kernel="precomputed" on the CPU: solve_cpu_gram (the CPU solver's loop on the caller's Gram, eta from the pair's
own diagonal entries) against scikit-learn (tests/data/sklearn_precomputed.json, bench/make_precomputed_fixture.py),
gram_decision_cpu against numpy float64, the general-diagonal pair_update overloads against the unit-diagonal
ones, and the refusals and value errors with device="cpu".

Bounds: decisions and intercept within 1e-2 on the positive definite Grams (PRED_TOL / B_TOL of
tests/test_svr_gpu.py, 10 x the fixture's recorded ``dev`` <= 1e-3), on the polynomial Gram 10 x its own ``dev``.
"""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 1e-3
PRED_TOL = 1e-2   # the project's bound for two solvers at stop tolerance 1e-3 (tests/test_svr_gpu.py): 10 x dev
B_TOL = 1e-2
BAND = 1e-2       # decisions within BAND of 0 are undecided at these tolerances
POSITIVE_DEFINITE = ("rbf", "scaled")


@functools.lru_cache(maxsize=1)
def fixture_script():
    path = os.path.join(HERE, "..", "bench", "make_precomputed_fixture.py")
    spec = importlib.util.spec_from_file_location("make_precomputed_fixture", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=1)
def load_fixture() -> dict:
    """the fixture with X / y / z as arrays, ``n`` training rows and ``grams``: name -> (K (n, n), K(test, train))"""
    with open(os.path.join(HERE, "data", "sklearn_precomputed.json")) as f:
        d = json.load(f)
    d["X"] = fixture_script().features(d["seed"])
    d["y"] = np.array(d["y"], dtype=np.float32)
    d["z"] = np.array(d["z"], dtype=np.float32)
    d["n"] = int(d["n_train"])
    d["grams"] = fixture_script().grams(d["X"], d["n"])
    for s in d["settings"]:
        s["dec_train"] = np.array(s["dec_train"])
        s["dec_test"] = np.array(s["dec_test"])
    return d


def bound(s: dict) -> float:
    """PRED_TOL on the positive definite Grams; on the polynomial one 10 x the setting's recorded dev"""
    return PRED_TOL if s["gram"] in POSITIVE_DEFINITE else 10.0 * s["dev"]


def make(kind: str, **kw):
    """the estimator of a fixture setting (C = 1; epsilon = 0.1; nu = 0.2), kernel="precomputed" """
    from dpsvm_amd import SVC, SVR, OneClassSVM

    kw = dict(kernel="precomputed", eps=EPS, **kw)
    if kind == "svc":
        return SVC(C=1.0, **kw)
    if kind == "svr":
        return SVR(C=1.0, epsilon=0.1, **kw)
    return OneClassSVM(nu=0.2, **kw)


def fit(m, kind: str, K, fx: dict):
    n = fx["n"]
    if kind == "svc":
        return m.fit(K, fx["y"][:n])
    if kind == "svr":
        return m.fit(K, fx["z"][:n])
    return m.fit(K)


def decisions(m, kind: str, Kt):
    return m.predict(Kt) if kind == "svr" else m.decision_function(Kt)


def check_against_fixture(m, s: dict, K, Kt, what: str) -> None:
    """decisions on the training and held-out rows and the intercept within bound(s) of scikit-learn's (printed
    first); predictions equal the reference's sign where it is decided"""
    tol = bound(s)
    d_train, d_test = decisions(m, s["kind"], K), decisions(m, s["kind"], Kt)
    e_train = float(np.max(np.abs(d_train - s["dec_train"])))
    e_test = float(np.max(np.abs(d_test - s["dec_test"])))
    e_b = abs(float(m.intercept_) - s["intercept"])
    print(f"{what} {s['kind']} on {s['gram']}: vs sklearn max |d decision| {e_train:.3g} / {e_test:.3g} "
          f"|d intercept| {e_b:.3g} (bound {tol:.3g}); steps {m.n_iter_} n_sv {m.n_support_} (sklearn {s['n_sv']})")
    assert d_train.dtype == np.float32 and d_train.shape == (len(K),) and d_test.shape == (len(Kt),)
    assert e_train < tol and e_test < tol and e_b < tol
    if s["kind"] != "svr":
        sure = np.abs(s["dec_test"]) >= BAND
        assert np.mean(~sure) <= 0.05
        want = np.where(s["dec_test"][sure] >= 0, 1, -1)
        np.testing.assert_array_equal(np.asarray(m.predict(Kt))[sure].astype(np.int64), want)


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.mark.parametrize("k", range(7))
def test_solve_cpu_gram_matches_sklearn(fx, k):
    s = fx["settings"][k]
    K, Kt = fx["grams"][s["gram"]]
    m = fit(make(s["kind"], device="cpu"), s["kind"], K, fx)
    assert m.converged_ and m.status_ == 1
    assert m.setup_info_["kernel"] == "precomputed" and m.setup_info_["iteration"] == "cpu"
    assert "precomputed Gram: general diagonal, one block" in m.setup_info_["engine_note"]
    assert m.gamma_ is None and not hasattr(m, "support_vectors_")
    check_against_fixture(m, s, K, Kt, "cpu")
    if s["kind"] == "svc":
        acc = float(np.mean(np.where(s["dec_train"] >= 0, 1.0, -1.0) == fx["y"][:fx["n"]]))
        assert abs(m.train_accuracy() - acc) <= 0.02  # the rows within the band may flip
    if s["kind"] == "oneclass":
        assert float(np.max(np.abs(m.train_decision_ - m.decision_function(K)))) < 1e-4
        assert abs(float(np.sum(m.alpha_.astype(np.float64))) - 0.2 * fx["n"]) < 1e-2


def test_native_solve_cpu_gram_row_C(fx, C):
    """per-row C for the classifier: a zero-bound row keeps alpha = 0, the others stay inside their boxes"""
    K, _ = fx["grams"]["scaled"]
    n = fx["n"]
    y = fx["y"][:n]
    p = C.SolverParams()
    p.kernel, p.clip, p.eps = 1, C.ClipMode.box, EPS
    rc = np.where(np.arange(n) % 3 == 0, 0.5, 2.0).astype(np.float32)
    rc[[5, 17]] = 0.0
    alpha, info = C.solve_cpu_gram(K, y, p, None, rc)
    assert info["converged"] and info["gram_reused"] and info["t_gram"] == 0
    assert np.all(alpha >= 0) and np.all(alpha <= rc) and alpha[5] == 0 and alpha[17] == 0
    assert abs(float(np.sum(alpha.astype(np.float64) * y))) < 1e-4
    # the gradient it returns is consistent with alpha: f = K (alpha y) - y
    f = K.astype(np.float64) @ (alpha.astype(np.float64) * y) - y
    assert float(np.max(np.abs(np.asarray(info["f"]) - f))) < 1e-3


@pytest.mark.parametrize("nt,n,k", [(1, 1, 1), (5, 3, 3), (7, 1025, 9), (300, 4099, 2)])
def test_gram_decision_cpu_matches_numpy(C, nt, n, k):
    rng = np.random.default_rng(nt * 131 + n + k)
    Kt = rng.standard_normal((nt, n)).astype(np.float32)
    coef = rng.standard_normal((k, n)).astype(np.float32)
    b = rng.standard_normal(k).astype(np.float32)
    ref = Kt.astype(np.float64) @ coef.astype(np.float64).T - b.astype(np.float64)
    mag = np.abs(Kt.astype(np.float64)) @ np.abs(coef.astype(np.float64)).T
    out = np.asarray(C.gram_decision_cpu(Kt, coef, b, 0))
    assert out.shape == (nt, k) and out.dtype == np.float32
    # one rounding to float32 of a float64 sum: half an ulp of the reference, plus the float64 accumulation
    tol = 0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 1e-12 * mag + 1e-45
    assert np.all(np.abs(out.astype(np.float64) - ref) <= tol)


def test_pair_update_general_diagonal_unit_is_bit_equal(C):
    """with k_hh = k_ll = 1 the new overloads are the old ones bit for bit, on random operands: every clip mode,
    both label geometries, the same-row case, steps that land on either bound"""
    rng = np.random.default_rng(7)
    bits = lambda t: np.array(t, dtype=np.float32).view(np.uint32).tolist()  # noqa: E731
    for i in range(4000):
        Cs = float(np.float32(rng.choice([0.5, 1.0, 10.0])))
        C_hi, C_lo = (Cs, Cs) if i % 2 else (float(np.float32(rng.uniform(0.1, 3))), float(np.float32(rng.uniform(0.1, 3))))
        a_hi = float(np.float32(rng.choice([0.0, C_hi, rng.uniform(0, C_hi)])))
        a_lo = float(np.float32(rng.choice([0.0, C_lo, rng.uniform(0, C_lo)])))
        y_hi, y_lo = float(rng.choice([-1.0, 1.0])), float(rng.choice([-1.0, 1.0]))
        b_hi = float(np.float32(rng.normal()))
        b_lo = float(np.float32(b_hi + abs(rng.normal()) * rng.choice([1e-3, 1.0, 30.0])))
        k_hl = float(np.float32(rng.choice([1.0, rng.uniform(-0.2, 1.0)])))
        clip, same = int(rng.integers(0, 2)), bool(i % 17 == 0)
        if same:
            a_lo, y_lo, C_lo, k_hl = a_hi, y_hi, C_hi, 1.0
        old_w = C.pair_update_w(a_hi, a_lo, y_hi, y_lo, b_hi, b_lo, k_hl, C_hi, C_lo, 1e-12, clip, same)
        new_w = C.pair_update_w_diag(a_hi, a_lo, y_hi, y_lo, b_hi, b_lo, k_hl, 1.0, 1.0, C_hi, C_lo, 1e-12, clip, same)
        assert bits(old_w) == bits(new_w)
        old = C.pair_update(a_hi, a_lo, y_hi, y_lo, b_hi, b_lo, k_hl, C_hi, 1e-12, clip, same)
        new = C.pair_update_diag(a_hi, a_lo, y_hi, y_lo, b_hi, b_lo, k_hl, 1.0, 1.0, C_hi, 1e-12, clip, same)
        assert bits(old) == bits(new)


def test_pair_update_general_diagonal_eta(C):
    """eta = k_hh + k_ll - 2 k_hl: an unclipped step is y_lo (b_hi - b_lo) / eta; eta <= 0 is floored at tau"""
    a_hi, a_lo, c_hi, c_lo = C.pair_update_diag(0.5, 0.5, 1.0, -1.0, -0.25, 0.25, 0.5, 4.0, 2.0, 10.0, 1e-12, 1, False)
    step = np.float32(-1.0) * (np.float32(-0.25) - np.float32(0.25)) / np.float32(5.0)
    assert a_lo == np.float32(0.5) + step and a_hi == np.float32(0.5) + step
    # a duplicated row scaled alike: eta = 4 + 4 - 2 * 4 = 0 exactly -> tau, the step runs into the box
    a_hi, a_lo, _, _ = C.pair_update_diag(0.5, 0.5, 1.0, -1.0, -0.25, 0.25, 4.0, 4.0, 4.0, 10.0, 1e-12, 1, False)
    assert a_lo == 10.0 and a_hi == 10.0


REFUSALS = [
    (dict(solver="smo"), "solver"), (dict(engines="all"), "engines"), (dict(ws_blocks=4), "ws_blocks"),
    (dict(force_cache=True), "force_cache"), (dict(cache_lines=64), "cache_lines"),
    (dict(host_cache_lines=8), "host_cache_lines"), (dict(ws_recompute="on"), "ws_recompute"),
    (dict(shrink="on"), "shrink"), (dict(x_mode="partitioned"), "x_mode"), (dict(dp="shard"), "dp="),
    (dict(exchange="peer"), "exchange"), (dict(force_collectives=True), "force_collectives"),
    (dict(checkpoint_path="ck.bin"), "checkpoint"), (dict(checkpoint_every=10), "checkpoint"),
    (dict(clip="independent"), "clip"),
]


@pytest.mark.parametrize("kind", ["svc", "svr", "oneclass"])
@pytest.mark.parametrize("kw,names", REFUSALS)
def test_refusals_name_the_setting_cpu(kind, kw, names):
    with pytest.raises(NotImplementedError, match=names):
        make(kind, device="cpu", **kw)


def test_fit_argument_refusals_cpu(fx):
    K, _ = fx["grams"]["rbf"]
    y = fx["y"][:fx["n"]]
    for kw in (dict(comm=object()), dict(resume="ck.bin"), dict(rank_rows=10)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            make("svc", device="cpu").fit(K, y, **kw)


def test_value_errors_cpu(fx):
    from dpsvm_amd import SVC

    K, Kt = fx["grams"]["rbf"]
    y = fx["y"][:fx["n"]]
    with pytest.raises(ValueError, match="rbf.*precomputed"):
        SVC(kernel="linear")
    with pytest.raises(ValueError, match="square"):
        make("svc", device="cpu").fit(K[:, :-1], y)
    bad = K.copy()
    bad[3, 11] = np.nextafter(bad[3, 11], np.float32(2))
    with pytest.raises(ValueError, match="symmetric"):
        make("svc", device="cpu").fit(bad, y)
    bad = K.copy()
    bad[9, 9] = np.nan
    with pytest.raises(ValueError, match="diagonal"):
        make("svc", device="cpu").fit(bad, y)
    m = make("svc", device="cpu").fit(K, y)
    with pytest.raises(ValueError, match="columns"):
        m.decision_function(Kt[:, :-1])
    for call in (lambda: m.save("model.txt"), m.to_model):
        with pytest.raises(NotImplementedError, match="precomputed"):
            call()
    assert m.support_.ndim == 1 and m.dual_coef_.shape == m.support_.shape and m.gamma_ is None


def test_multiclass_weights_cv_proba_cpu(fx):
    """one-vs-rest, weights, cross-validation and probabilities through the CPU solver"""
    n = fx["n"]
    K, Kt = fx["grams"]["scaled"]
    X = fx["X"]
    protos = X[[0, 1, 2]]
    y3 = np.argmin(((X[:, None, :] - protos[None]) ** 2).sum(-1), axis=1)[:n]
    m = make("svc", device="cpu").fit(K, y3)
    assert m.alpha_.shape == (3, n) and m.decision_function(Kt).shape == (len(Kt), 3)
    for c in range(3):
        one = make("svc", device="cpu").fit(K, np.where(y3 == c, 1.0, -1.0))
        np.testing.assert_array_equal(one.alpha_.view(np.uint32), m.alpha_[c].view(np.uint32))
    assert m.train_accuracy() == pytest.approx(float(np.mean(m.predict(K) == y3)), abs=0.02)
    y = fx["y"][:n]
    w = np.ones(n)
    w[[4, 40]] = 0.0
    mw = make("svc", device="cpu", class_weight="balanced").fit(K, y, sample_weight=w)
    assert mw.alpha_[4] == 0 and mw.alpha_[40] == 0 and np.all(mw.alpha_ <= mw.row_C_)
    mp = make("svc", device="cpu").fit(K, y, probability=3)
    P = mp.predict_proba(Kt)
    assert P.shape == (len(Kt), 2) and np.allclose(P.sum(axis=1), 1.0, atol=1e-6)
    np.testing.assert_array_equal(mp.alpha_.view(np.uint32), make("svc", device="cpu").fit(K, y).alpha_.view(np.uint32))
