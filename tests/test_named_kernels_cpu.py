"""Linear, polynomial and sigmoid kernels as kernel spec objects (docs/DESIGN.md §21), on the CPU: the specs'
validation, kernel_gram_cpu against the formula in float64, a spec fit against kernel="precomputed" on
kernel_gram_cpu(X) bit for bit, against scikit-learn's own kernels (tests/data/sklearn_named_kernels.json,
bench/make_named_kernels_fixture.py), the model files, and the precomputed table's refusals under a spec.

Bounds against scikit-learn: 10 x the setting's recorded ``dev`` (scikit-learn at tol 1e-3 against tol 1e-7), the
project's rule for two solvers at stop tolerance 1e-3, on the decisions and on the intercept.
"""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def fixture_script():
    path = os.path.join(HERE, "..", "bench", "make_named_kernels_fixture.py")
    spec = importlib.util.spec_from_file_location("make_named_kernels_fixture", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=1)
def load_fixture() -> dict:
    """the fixture with X / y / z as arrays and ``n`` training rows (shared, read-only)"""
    with open(os.path.join(HERE, "data", "sklearn_named_kernels.json")) as f:
        d = json.load(f)
    d["X"] = fixture_script().features(d["seed"])
    d["y"] = np.asarray(d["y"], dtype=np.float32)
    d["z"] = np.asarray(d["z"], dtype=np.float32)
    d["n"] = int(d["n_train"])
    for s in d["settings"]:
        s["dec_train"] = np.asarray(s["dec_train"], dtype=np.float64)
        s["dec_test"] = np.asarray(s["dec_test"], dtype=np.float64)
    for a in (d["X"], d["y"], d["z"]):
        a.setflags(write=False)
    return d


def spec_of(s: dict):
    from dpsvm_amd import Linear, Poly, Sigmoid

    return {"linear": lambda: Linear(), "poly": lambda: Poly(s["degree"], s["coef0"]),
            "sigmoid": lambda: Sigmoid(s["coef0"])}[s["kernel"]]()


def make(kind: str, kernel, gamma, **kw):
    """the estimator of a fixture setting (C = 1; epsilon = 0.1; nu = 0.2) under ``kernel``"""
    from dpsvm_amd import SVC, SVR, OneClassSVM

    if kind == "svc":
        return SVC(C=1.0, kernel=kernel, gamma=gamma, **kw)
    if kind == "svr":
        return SVR(C=1.0, epsilon=0.1, kernel=kernel, gamma=gamma, **kw)
    return OneClassSVM(nu=0.2, kernel=kernel, gamma=gamma, **kw)


def fit(m, kind: str, X, fx: dict, **kw):
    n = fx["n"]
    if kind == "svc":
        return m.fit(X, fx["y"][:n], **kw)
    if kind == "svr":
        return m.fit(X, fx["z"][:n], **kw)
    return m.fit(X, **kw)


def decisions(m, kind: str, X, **kw):
    return m.predict(X, **kw) if kind == "svr" else m.decision_function(X, **kw)


def check_against_fixture(m, s: dict, fx: dict, what: str) -> None:
    """decisions on the training and held-out rows and the intercept within 10 x dev of scikit-learn's (printed
    first)"""
    n, tol = fx["n"], 10.0 * s["dev"]
    d_train, d_test = decisions(m, s["kind"], fx["X"][:n]), decisions(m, s["kind"], fx["X"][n:])
    e_train = float(np.max(np.abs(d_train - s["dec_train"])))
    e_test = float(np.max(np.abs(d_test - s["dec_test"])))
    e_b = abs(float(m.intercept_) - s["intercept"])
    print(f"{what} {s['kind']} {s['kernel']}: vs sklearn max |d decision| {e_train:.3g} / {e_test:.3g} "
          f"|d intercept| {e_b:.3g} (bound {tol:.3g}); steps {m.n_iter_} n_sv {m.n_support_} (sklearn {s['n_sv']})")
    assert d_train.dtype == np.float32 and d_train.shape == (n,) and d_test.shape == (len(fx["X"]) - n,)
    assert e_train < tol and e_test < tol and e_b < tol


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


# ------------------------------------------------------------------ the specs
def test_spec_validation():
    from dpsvm_amd import SVC, SVR, Linear, OneClassSVM, Poly, Sigmoid

    for bad in (0, 33, 2.5, -1, True, "3", None):
        with pytest.raises(ValueError, match="degree"):
            Poly(bad, 1.0)
    for bad in (float("nan"), float("inf"), 1e39, "x"):
        with pytest.raises(ValueError, match="coef0"):
            Poly(2, bad)
        with pytest.raises(ValueError, match="coef0"):
            Sigmoid(bad)
    p = Poly(degree=np.int64(3), coef0=1)
    assert (p.name, p.degree, p.coef0) == ("poly", 3, 1.0) and isinstance(p.degree, int) and isinstance(p.coef0, float)
    assert Poly(32).degree == 32 and Poly(1).degree == 1
    assert (Linear().name, Sigmoid(-0.5).name, Sigmoid(-0.5).coef0) == ("linear", "sigmoid", -0.5)
    assert Poly(3, 1.0) == Poly(3, 1.0) and Poly(3, 1.0) != Poly(2, 1.0) and hash(Poly(3, 1.0)) == hash(Poly(3, 1.0))
    with pytest.raises(Exception):  # frozen
        p.degree = 4
    # the strings stay "rbf" and "precomputed"
    for name in ("poly", "linear", "sigmoid"):
        with pytest.raises(ValueError, match="rbf.*precomputed"):
            SVC(kernel=name)
    with pytest.raises(ValueError, match="kernel"):
        SVC(kernel=3)
    for est in (SVC(kernel=Poly(3, 1.0)), SVR(kernel=Poly(3, 1.0)), OneClassSVM(kernel=Poly(3, 1.0))):
        assert est.get_params()["kernel"] == "poly" and est.config.clip == "box"
    assert SVC(kernel=Linear()).get_params()["kernel"] == "linear"
    assert "kernel" not in SVC().get_params()


# ------------------------------------------------------------------ kernel_gram_cpu
def formula64(X, Y, spec, gamma):
    dot = X.astype(np.float64) @ Y.astype(np.float64).T
    if spec.name == "linear":
        return dot
    u = gamma * dot + spec.coef0
    return np.tanh(u) if spec.name == "sigmoid" else u ** spec.degree


def test_kernel_gram_cpu_formula_and_symmetry(C, fx):
    """against the formula in float64: the dot is rounded once to float32 (2^-24 relative), u once more, the
    power by p - 1 float32 multiplications (powi's intermediates are powers of u too), tanh within a few ulp"""
    from dpsvm_amd import Linear, Poly, Sigmoid

    X = np.ascontiguousarray(fx["X"][:257])
    Y = np.ascontiguousarray(fx["X"][300:431])
    u24 = 2.0 ** -24
    for spec, gamma in ((Linear(), 1.0), (Poly(3, 1.0), 0.1), (Poly(7, -0.5), 0.3), (Sigmoid(0.25), 0.02)):
        K = np.asarray(C.kernel_gram_cpu(X, None, *spec.native(), gamma, 0))
        assert K.dtype == np.float32 and K.shape == (257, 257)
        np.testing.assert_array_equal(bits(K), bits(K.T))
        np.testing.assert_array_equal(bits(K), bits(C.kernel_gram_cpu(X, None, *spec.native(), gamma, 1)))
        R = np.asarray(C.kernel_gram_cpu(X, Y, *spec.native(), gamma, 0))
        assert R.shape == (257, 131)
        np.testing.assert_array_equal(bits(R[:, :5]), bits(C.kernel_gram_cpu(X, np.ascontiguousarray(Y[:5]),
                                                                             *spec.native(), gamma, 0)))
        for got, ref, dot in ((K, formula64(X, X, spec, gamma), formula64(X, X, Linear(), 1.0)),
                              (R, formula64(X, Y, spec, gamma), formula64(X, Y, Linear(), 1.0))):
            if spec.name == "linear":
                tol = u24 * np.abs(ref)
            else:
                au = np.abs(gamma * dot) + abs(spec.coef0)
                if spec.name == "sigmoid":
                    tol = 2 * u24 * au + 8 * u24  # |tanh'| <= 1; a few ulp of a value <= 1
                else:
                    p, u = spec.degree, np.abs(gamma * dot + spec.coef0)
                    tol = 2 * (p * u ** (p - 1) * 2 * u24 * au + p * u24 * u ** p)
            err = np.abs(got.astype(np.float64) - ref)
            print(f"{spec.name} {spec.degree}: max err / bound {float(np.max(err / np.maximum(tol, 1e-300))):.3g}")
            assert np.all(err <= tol)
    # (1 x.y + 0)^1 is the dot product itself, bit for bit
    np.testing.assert_array_equal(bits(C.kernel_gram_cpu(X, Y, *Poly(1, 0.0).native(), 1.0, 0)),
                                  bits(C.kernel_gram_cpu(X, Y, *Linear().native(), 1.0, 0)))
    with pytest.raises(ValueError):
        C.kernel_gram_cpu(X, Y, 1, 33, 0.0, 1.0, 0)
    with pytest.raises(ValueError):
        C.kernel_gram_cpu(X, np.ascontiguousarray(Y[:, :5]), 0, 1, 0.0, 1.0, 0)


# ------------------------------------------------------------------ spec fit == precomputed fit on kernel_gram_cpu(X)
def gram_of(C, X, spec, gamma):
    return np.asarray(C.kernel_gram_cpu(np.ascontiguousarray(X), None, *spec.native(), gamma, 0))


@pytest.mark.parametrize("k", range(5))
def test_spec_fit_equals_precomputed_fit_cpu(C, fx, k):
    s = fx["settings"][k]
    n, spec, gamma = fx["n"], spec_of(s), s["gamma"]
    X = fx["X"][:n]
    a = fit(make(s["kind"], spec, gamma, device="cpu"), s["kind"], X, fx)
    b = fit(make(s["kind"], "precomputed", None, device="cpu"), s["kind"], gram_of(C, X, spec, gamma), fx)
    np.testing.assert_array_equal(bits(a.alpha_), bits(b.alpha_))
    assert np.float32(a.b_).view(np.uint32) == np.float32(b.b_).view(np.uint32)
    assert a.converged_ and a.setup_info_["kernel"] == s["kernel"] and a.setup_info_["iteration"] == "cpu"
    assert "precomputed Gram: general diagonal, one block" in a.setup_info_["engine_note"]
    assert a.n_features_in_ == X.shape[1] and a.support_vectors_.shape == (a.n_support_, X.shape[1])
    np.testing.assert_array_equal(a.support_, b.support_)
    np.testing.assert_array_equal(a.support_vectors_, X[a.support_])
    assert a.gamma_ is None if s["kernel"] == "linear" else a.gamma_ == pytest.approx(gamma)
    # the model predicts from rows what the precomputed one predicts from K(test, train)
    Kt = np.asarray(C.kernel_gram_cpu(np.ascontiguousarray(fx["X"][n:]), np.ascontiguousarray(X), *spec.native(),
                                      gamma, 0))
    np.testing.assert_array_equal(bits(decisions(a, s["kind"], fx["X"][n:])), bits(decisions(b, s["kind"], Kt)))
    np.testing.assert_array_equal(bits(decisions(a, s["kind"], fx["X"][n:], predict_chunk_rows=77)),
                                  bits(decisions(a, s["kind"], fx["X"][n:])))
    check_against_fixture(a, s, fx, "cpu")


def test_three_class_weighted_spec_fit_equals_precomputed_cpu(C, fx):
    from dpsvm_amd import Poly

    n, spec, gamma = 300, Poly(3, 1.0), 0.1
    X = fx["X"][:n]
    y3 = np.where(X[:, 0] < -0.3, 0, np.where(X[:, 0] < 0.3, 1, 2))
    w = 0.5 + (np.arange(n) % 4) * 0.5
    a = make("svc", spec, gamma, device="cpu").fit(X, y3, sample_weight=w, probability=3)
    b = make("svc", "precomputed", None, device="cpu").fit(gram_of(C, X, spec, gamma), y3, sample_weight=w,
                                                         probability=3)
    assert a.alpha_.shape == (3, n)
    np.testing.assert_array_equal(bits(a.alpha_), bits(b.alpha_))
    np.testing.assert_array_equal(bits(a.b_), bits(b.b_))
    np.testing.assert_array_equal(a.probA_, b.probA_)
    np.testing.assert_array_equal(a.probB_, b.probB_)
    Xt = fx["X"][600:700]
    Kt = np.asarray(C.kernel_gram_cpu(np.ascontiguousarray(Xt), np.ascontiguousarray(X), *spec.native(), gamma, 0))
    np.testing.assert_array_equal(bits(a.decision_function(Xt)), bits(b.decision_function(Kt)))
    pa = a.predict_proba(Xt, predict_chunk_rows=33)
    np.testing.assert_array_equal(bits(pa), bits(b.predict_proba(Kt)))
    assert np.max(np.abs(pa.sum(axis=1) - 1.0)) < 1e-5
    np.testing.assert_array_equal(a.predict(Xt), b.predict(Kt))
    assert a.train_accuracy() == b.train_accuracy() and a.score(X, y3) == pytest.approx(a.train_accuracy(), abs=0.02)
    # cross-validation and the nu path run on the same Gram
    y2 = np.where(X[:, 1] > 0, 1.0, -1.0)
    np.testing.assert_array_equal(
        bits(make("svc", spec, gamma, device="cpu").cross_val_decision(X, y2, cv=3)),
        bits(make("svc", "precomputed", None, device="cpu").cross_val_decision(gram_of(C, X, spec, gamma), y2, cv=3)))
    pa = make("oneclass", spec, gamma, device="cpu").nu_path(X, [0.1, 0.3])
    pb = make("oneclass", "precomputed", None, device="cpu").nu_path(gram_of(C, X, spec, gamma), [0.1, 0.3])
    assert pa == pb


# ------------------------------------------------------------------ model files
@pytest.mark.parametrize("kind", ["svc", "svc3", "svr", "oneclass"])
def test_model_file_round_trip_cpu(fx, tmp_path, kind):
    from dpsvm_amd import Poly, load_model, load_one_class, load_svr

    n, spec, gamma = 300, Poly(2, 1.0), 0.1
    X, Xt = fx["X"][:n], fx["X"][600:700]
    path = str(tmp_path / "m.txt")
    if kind == "svc3":
        y3 = np.where(X[:, 0] < -0.3, 0, np.where(X[:, 0] < 0.3, 1, 2))
        m = make("svc", spec, gamma, device="cpu").fit(X, y3, probability=3)
        m.save(path)
        back = load_model(path, device="cpu")
        assert open(path).readline() == "dpsvm-kernel poly 2 1\n" and open(path).readlines()[1].startswith("dpsvm-ovr 3 ")
        np.testing.assert_array_equal(bits(back.decision_function(Xt)), bits(m.decision_function(Xt)))
        np.testing.assert_array_equal(bits(back.predict_proba(Xt)), bits(m.predict_proba(Xt)))  # the .platt sidecar
        np.testing.assert_array_equal(back.predict(Xt), m.predict(Xt))
        return
    fxs = {"n": n, "y": fx["y"], "z": fx["z"]}
    m = fit(make(kind, spec, gamma, device="cpu"), kind, X, fxs)
    m.save(path)
    assert open(path).readline() == "dpsvm-kernel poly 2 1\n"
    back = {"svc": load_model, "svr": load_svr, "oneclass": load_one_class}[kind](path, device="cpu")
    assert (back.model.kernel, back.model.degree, back.model.coef0) == ("poly", 2, 1.0)
    np.testing.assert_array_equal(bits(decisions(back, kind, Xt)), bits(decisions(m, kind, Xt)))
    np.testing.assert_array_equal(bits(decisions(back, kind, Xt, predict_chunk_rows=7)), bits(decisions(m, kind, Xt)))


def test_linear_and_sigmoid_model_files_cpu(fx, tmp_path):
    from dpsvm_amd import Linear, Sigmoid, load_model

    n = 300
    X, Xt, y = fx["X"][:n], fx["X"][600:650], fx["y"][:n]
    for spec, gamma, head in ((Linear(), None, "dpsvm-kernel linear 1 0\n"),
                              (Sigmoid(0.125), 0.02, "dpsvm-kernel sigmoid 1 0.125\n")):
        path = str(tmp_path / f"{spec.name}.txt")
        m = make("svc", spec, gamma, device="cpu").fit(X, y)
        m.save(path)
        assert open(path).readline() == head
        np.testing.assert_array_equal(bits(load_model(path, device="cpu").decision_function(Xt)),
                                      bits(m.decision_function(Xt)))
        with pytest.raises(ValueError, match="legacy"):
            m.save(path, legacy=True)


def test_rbf_model_file_is_unchanged_and_unknown_kernel_is_an_error(C, fx, tmp_path):
    from dpsvm_amd import SVC, load_model

    n = 200
    X, y = fx["X"][:n], fx["y"][:n]
    m = SVC(C=1.0, gamma=0.5, device="cpu", solver="ws").fit(X, y)
    path = str(tmp_path / "rbf.txt")
    m.save(path)
    text = open(path).read()
    assert "dpsvm-kernel" not in text and float(text.split("\n")[0]) == pytest.approx(0.5)
    back = load_model(path, device="cpu")
    assert back.model.kernel == "rbf"
    np.testing.assert_array_equal(bits(back.decision_function(X[:20])), bits(m.decision_function(X[:20])))
    # a kernel line that says "rbf" reads as the same model; a name this build does not know is an error
    with open(str(tmp_path / "rbf2.txt"), "w") as f:
        f.write("dpsvm-kernel rbf 0 0\n" + text)
    np.testing.assert_array_equal(bits(load_model(str(tmp_path / "rbf2.txt"), device="cpu").decision_function(X[:20])),
                                  bits(m.decision_function(X[:20])))
    bad = str(tmp_path / "bad.txt")
    with open(bad, "w") as f:
        f.write("dpsvm-kernel laplace 1 0\n" + text)
    with pytest.raises(Exception, match="unknown kernel 'laplace'"):
        load_model(bad, device="cpu")
    with open(bad, "w") as f:
        f.write("dpsvm-kernel poly 40 0\n" + text)
    with pytest.raises(Exception, match="degree"):
        load_model(bad, device="cpu")
    # the RBF predictors refuse a model of another kernel by name
    md = C.read_model(path, False)
    md.kernel = "poly"
    with pytest.raises(ValueError, match="poly"):
        C.decision_cpu(md, np.ascontiguousarray(X[:4]), 0)


def test_svm_test_cli_names_the_kernel(fx, tmp_path, bin_dir):
    from conftest import run

    n = 100
    path = str(tmp_path / "poly.txt")
    from dpsvm_amd import Poly

    make("svc", Poly(2, 1.0), 0.1, device="cpu").fit(fx["X"][:n], fx["y"][:n]).save(path)
    r = run([os.path.join(bin_dir, "svmTest"), "-a", "20", "-x", "50", "--synthetic", "uniform", "-m", path, "--cpu"])
    assert r.returncode != 0 and "'poly' kernel" in (r.stdout + r.stderr)


# ------------------------------------------------------------------ refusals and value errors
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
def test_refusals_name_the_setting_under_a_spec(kind, kw, names):
    from dpsvm_amd import Poly

    with pytest.raises(NotImplementedError, match=names):
        make(kind, Poly(3, 1.0), 0.1, device="cpu", **kw)


def test_fit_argument_refusals_and_value_errors_under_a_spec(fx):
    from dpsvm_amd import Poly, Sigmoid

    n = 100
    X, y = fx["X"][:n], fx["y"][:n]
    for kw in (dict(comm=object()), dict(resume="ck.bin"), dict(rank_rows=10)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            make("svc", Poly(3, 1.0), 0.1, device="cpu").fit(X, y, **kw)
    with pytest.raises(ValueError, match="len"):
        make("svc", Poly(3, 1.0), 0.1, device="cpu").fit(X, y[:-1])
    m = make("svc", Poly(3, 1.0), 0.1, device="cpu").fit(X, y)
    with pytest.raises(ValueError, match="features"):
        m.decision_function(X[:, :5])
    with pytest.raises(ValueError, match="predict_chunk_rows"):
        m.decision_function(X, predict_chunk_rows=0)
    with pytest.raises(NotImplementedError):
        make("svc", "precomputed", None, device="cpu").fit(np.eye(4, dtype=np.float32), [1, -1, 1, -1]).to_model()
    # tanh(gamma x.x - 5) < 0 on rows near zero: the diagonal check of the precomputed path refuses the Gram
    for kind in ("svc", "svr", "oneclass"):
        with pytest.raises(ValueError, match="diagonal"):
            fit(make(kind, Sigmoid(-5.0), 0.02, device="cpu"), kind, X * np.float32(1e-3),
                {"n": n, "y": fx["y"], "z": fx["z"]})
