"""Probability estimates on the CPU: platt_fit_cpu against the numpy port
(tests/ref_platt.py) and the scikit-learn fixture (tests/data/platt_blobs.json),
and fit(probability=) / predict_proba / the .platt sidecar end to end.

Bound on A and B: 1e-6, at least 30 times the gap between the port and
scikit-learn on the fixture's runs (bench/make_platt_fixture.py prints it) — the
spread two correct minimisers of this strictly convex objective show.
"""
import os
import warnings

import numpy as np
import pytest

import ref_platt
from ref_smo_weighted import GAMMA, N, shared_data

AB_TOL = 1e-6


@pytest.fixture(scope="module")
def C():
    from dpsvm_amd._native import load

    return load()


@pytest.fixture(scope="module")
def runs():
    """the fixture's five decision sets: (name, float32 decisions, labels, scikit-learn's A, B)"""
    fx = ref_platt.load_fixture()
    cls = shared_data()[5]
    out = []
    for c, mach in enumerate(fx["machines"]):
        dec = (np.array(mach["cv_decision_e6"], dtype=np.float64) / fx["scale"]).astype(np.float32)
        out.append((f"machine {c}", dec, np.where(cls == c, 1.0, -1.0).astype(np.float32), mach["A"], mach["B"]))
    out.append(("binary",) + out[3][1:])
    assert all(len(r[1]) == N for r in out)
    return out


def test_fit_cpu_against_port_and_fixture(C, runs):
    for name, dec, y, A, B in runs:
        got, ref = C.platt_fit_cpu(dec, y), ref_platt.platt_fit(dec, y)
        print(f"{name}: A {got['A']:.9f} B {got['B']:.9f}  - port {got['A'] - ref['A']:.3g} {got['B'] - ref['B']:.3g}  "
              f"- scikit-learn {got['A'] - A:.3g} {got['B'] - B:.3g}  iters {got['iters']} evals {got['evals']}")
        assert abs(got["A"] - ref["A"]) <= AB_TOL and abs(got["B"] - ref["B"]) <= AB_TOL
        assert abs(got["A"] - A) <= AB_TOL and abs(got["B"] - B) <= AB_TOL
        assert (got["iters"], got["evals"], got["status"]) == (ref["iters"], ref["evals"], ref["status"])
        assert got["status"] == 0 and abs(got["fval"] - ref["fval"]) <= 1e-9 * abs(ref["fval"])


def test_proba_cpu_against_port(C):
    rng = np.random.default_rng(3)
    for k in (1, 2, 4):
        dec = rng.uniform(-3, 3, (37, k)).astype(np.float32)
        A, B = rng.uniform(-13, -1, k), rng.uniform(-1, 1, k)
        got = C.proba_cpu(dec, A, B)
        assert got.dtype == np.float32 and got.shape == (37, k)
        assert np.max(np.abs(got - ref_platt.proba(dec, A, B))) <= (2.0 ** -22 if k > 2 else 2.0 ** -23)
    zero = C.proba_cpu(np.full((2, 4), 1000.0, dtype=np.float32), np.ones(4), np.zeros(4))  # exp(-1000) == 0
    assert np.array_equal(zero, np.full((2, 4), 0.25, dtype=np.float32))


def _check_model(C, clf, plain, X, y_machines, Xq, k, tmp_path):
    n = len(X)
    multi = k > 2
    assert clf.cv_decision_.dtype == np.float32 and clf.cv_decision_.shape == ((n, k) if multi else (n,))
    assert np.shape(clf.probA_) == ((k,) if multi else ()) and np.asarray(clf.probA_).dtype == np.float64
    assert np.shape(clf.probB_) == np.shape(clf.probA_) and np.asarray(clf.probB_).dtype == np.float64
    assert all(np.array_equal(a, b) for a, b in zip(clf.cv_folds_, clf.cv_folds(n, 5, 0)))
    cvd = clf.cv_decision_ if multi else clf.cv_decision_[:, None]
    stats = clf.platt_stats_ if multi else [clf.platt_stats_]
    for c in range(cvd.shape[1]):  # the published sigmoids are platt_fit_cpu of the published decisions
        fit = C.platt_fit_cpu(np.ascontiguousarray(cvd[:, c]), y_machines[c])
        assert (fit["A"], fit["B"]) == (np.atleast_1d(clf.probA_)[c], np.atleast_1d(clf.probB_)[c])
        assert stats[c] == {key: fit[key] for key in ("iters", "evals", "fval", "status")} and fit["status"] == 0
    # the probability fit leaves the model alone
    assert np.array_equal(clf.alpha_, plain.alpha_) and np.array_equal(clf.b_, plain.b_)
    assert np.array_equal(clf.predict(Xq), plain.predict(Xq))
    P = clf.predict_proba(Xq)
    assert P.dtype == np.float32 and P.shape == (len(Xq), k)
    assert np.max(np.abs(P.astype(np.float64).sum(axis=1) - 1.0)) <= 2.0 ** -22
    dec = clf.decision_function(Xq)
    ref = ref_platt.proba(dec if multi else dec[:, None], np.atleast_1d(clf.probA_), np.atleast_1d(clf.probB_))
    if multi:  # columns in the order of classes_
        assert np.max(np.abs(P - ref)) <= 2.0 ** -22
    else:  # [1 - p, p], p = P(classes_[-1])
        assert np.max(np.abs(P[:, 1] - ref[:, 0])) <= 2.0 ** -23
        assert np.array_equal(P[:, 0], np.float32(1.0) - P[:, 1])
    agree = float(np.mean(clf.classes_[np.argmax(P, axis=1)] == clf.predict(Xq)))
    print(f"k = {k}: argmax of the probabilities agrees with predict on {agree:.3f} of the rows")
    with pytest.raises(RuntimeError):
        plain.predict_proba(Xq)
    # the sidecar round trip
    from dpsvm_amd.models.svc import load_model

    path = str(tmp_path / f"model{k}.txt")
    clf.save(path, precision=9)
    with open(path + ".platt") as f:
        lines = f.read().split("\n")
    m = k if multi else 1
    assert lines[0] == f"dpsvm-platt {m}" and len(lines[1].split(",")) == m and len(lines[2].split(",")) == m
    loaded = load_model(path, device="cpu")
    assert np.array_equal(np.atleast_1d(loaded.probA_), np.atleast_1d(clf.probA_))  # 17 digits: the same doubles
    assert np.array_equal(np.atleast_1d(loaded.probB_), np.atleast_1d(clf.probB_))
    # 9 digits hold a float32: the file's model is the fitted one, so the probabilities are the same bits
    assert np.array_equal(loaded.decision_function(Xq), dec)
    assert np.array_equal(loaded.predict_proba(Xq), P)
    plain_path = str(tmp_path / f"plain{k}.txt")
    plain.save(plain_path)
    assert not os.path.exists(plain_path + ".platt")
    with pytest.raises(RuntimeError):
        load_model(plain_path, device="cpu").predict_proba(Xq)
    os.remove(path + ".platt")  # the model file alone
    with pytest.raises(RuntimeError):
        load_model(path, device="cpu").predict_proba(Xq)


def test_end_to_end_binary_cpu(C, tmp_path):
    from dpsvm_amd.models.svc import SVC

    X, y, _, Xt, _, _ = shared_data()
    X, y, Xq = X[:300], y[:300], Xt[:50]
    cfg = dict(C=1.0, gamma=GAMMA, device="cpu", clip="box")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # a sigmoid fit that does not converge warns
        clf = SVC(**cfg).fit(X, y, probability=5)
    plain = SVC(**cfg).fit(X, y)
    assert len(clf.cv_stats_) == 5 and all(s["converged"] for s in clf.cv_stats_) and clf.stats_["converged"]
    assert np.array_equal(clf.cv_decision_, SVC(**cfg).cross_val_decision(X, y, cv=5, seed=0))
    _check_model(C, clf, plain, X, [y], Xq, 2, tmp_path)


def test_end_to_end_four_classes_cpu(C, tmp_path):
    from dpsvm_amd.models.svc import SVC

    X, _, _, Xt, _, cls = shared_data()
    X, cls, Xq = X[:300], cls[:300], Xt[:50]
    cfg = dict(C=1.0, gamma=GAMMA, device="cpu", clip="box")
    clf = SVC(**cfg).fit(X, cls, probability=5)
    plain = SVC(**cfg).fit(X, cls)
    assert np.array_equal(clf.classes_, np.arange(4))
    assert len(clf.stats_) == 4 and [len(s) for s in clf.cv_stats_] == [5, 5, 5, 5]
    ys = [np.where(cls == c, 1.0, -1.0).astype(np.float32) for c in range(4)]
    for c in range(4):  # each column is the binary out-of-fold call on that machine's labels
        assert np.array_equal(clf.cv_decision_[:, c], SVC(**cfg).cross_val_decision(X, ys[c], cv=5, seed=0))
    _check_model(C, clf, plain, X, ys, Xq, 4, tmp_path)


def test_probability_argument_and_refusals():
    from dpsvm_amd.models.svc import SVC

    X, y, _, _, _, _ = shared_data()
    X, y = X[:60], y[:60]
    for bad in (1, -1):
        with pytest.raises(ValueError):
            SVC(device="cpu").fit(X, y, probability=bad)
    # settings resolve as for a weighted fit: the same refusals
    for kw in (dict(solver="smo"), dict(shrink="on"), dict(ws_recompute="on"), dict(checkpoint_path="ck.bin")):
        with pytest.raises(NotImplementedError):
            SVC(device="cpu", **kw).fit(X, y, probability=2)
    with pytest.raises(NotImplementedError):
        SVC(device="cpu").fit(X, y, probability=2, resume="ck.bin")
    assert "probability" not in SVC().get_params()
