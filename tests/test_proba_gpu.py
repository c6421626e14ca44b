"""fit(probability=5) and predict_proba on the GPU, two and four classes on the 1500
blobs: the full-data solve and the folds of every machine on one resident Gram, the
held-out decisions and the sigmoid fit on the device, the probability epilogue of
the decision GEMM, the .platt sidecar.

Against the scikit-learn fixture's probabilities (tests/data/platt_blobs.json) the
bound is 1.3e-2: tests/test_cv_gpu.py allows the out-of-fold decisions 1e-2 from
scikit-learn's; a sigmoid of slope |A| / 4 with |A| about 2.54 turns that into
6.4e-3 (checked on the CPU: +-1e-2 noise on the decisions moved the probabilities
by at most 6.4e-3, the drift of A and B included); the bound doubles that.
"""
import os

import numpy as np
import pytest
import torch

import ref_platt
from ref_smo_weighted import GAMMA, N, NT, shared_data

pytestmark = pytest.mark.gpu

CFG = dict(C=1.0, gamma=GAMMA, device="cuda", solver="ws", clip="box")
PLAIN = dict(CFG, shrink="off", ws_recompute="off")  # what a probability fit resolves to
AB_TOL, FIXTURE_TOL = 1e-6, 1.3e-2


@pytest.fixture(scope="module")
def data():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return shared_data()


@pytest.fixture(scope="module")
def binary(data):
    from dpsvm_amd.models.svc import SVC

    X, y, _, Xt, _, _ = data
    return SVC(**CFG).fit(X, y, probability=5), SVC(**PLAIN).fit(X, y)


@pytest.fixture(scope="module")
def four(data):
    from dpsvm_amd.models.svc import SVC

    X, _, _, Xt, _, cls = data
    return SVC(**CFG).fit(X, cls, probability=5), SVC(**PLAIN).fit(X, cls)


def test_binary_solves_on_one_gram(binary):
    clf, plain = binary
    assert clf.stats_["gram_reused"] is False and clf.stats_["converged"]
    assert [s["gram_reused"] for s in clf.cv_stats_] == [True] * 5 and all(s["converged"] for s in clf.cv_stats_)
    assert clf.setup_info_["iteration"] == "ws-dense"
    assert np.array_equal(clf.alpha_, plain.alpha_) and clf.b_ == plain.b_  # bit-equal to the fit without
    assert clf.n_iter_ == plain.n_iter_


def test_binary_cv_decision_and_sigmoid(data, binary):
    from dpsvm_amd.models.svc import SVC

    X, y = data[0], data[1]
    clf, _ = binary
    assert clf.cv_decision_.dtype == np.float32 and clf.cv_decision_.shape == (N,)
    assert np.array_equal(clf.cv_decision_, SVC(**CFG).cross_val_decision(X, y, cv=5, seed=0))
    ref = ref_platt.platt_fit(clf.cv_decision_, y)
    print(f"binary: A {clf.probA_:.9f} B {clf.probB_:.9f}  - port {clf.probA_ - ref['A']:.3g} "
          f"{clf.probB_ - ref['B']:.3g}  {clf.platt_stats_}")
    assert abs(clf.probA_ - ref["A"]) <= AB_TOL and abs(clf.probB_ - ref["B"]) <= AB_TOL
    assert clf.platt_stats_["status"] == 0
    assert (clf.platt_stats_["iters"], clf.platt_stats_["evals"]) == (ref["iters"], ref["evals"])


def test_binary_predict_proba(data, binary, tmp_path):
    from dpsvm_amd.models.svc import load_model

    Xt = data[3]
    clf, plain = binary
    P = clf.predict_proba(Xt)
    assert P.dtype == np.float32 and P.shape == (NT, 2)
    dec = clf.decision_function(Xt)
    ref = ref_platt.proba(dec[:, None], [clf.probA_], [clf.probB_])[:, 0]
    assert np.max(np.abs(P[:, 1] - ref)) <= 2.0 ** -22 and np.array_equal(P[:, 0], np.float32(1.0) - P[:, 1])
    assert np.array_equal(clf.predict(Xt), plain.predict(Xt))
    fx = ref_platt.load_fixture()
    gap = float(np.max(np.abs(P[:, 1] - np.array(fx["binary_holdout_proba_e6"]) / fx["scale"])))
    print(f"binary: max |p - scikit-learn| on the held-out rows {gap:.3g}")
    assert gap <= FIXTURE_TOL
    with pytest.raises(RuntimeError):
        plain.predict_proba(Xt)
    path = str(tmp_path / "binary.txt")
    clf.save(path)
    loaded = load_model(path, device="cuda")
    assert np.array_equal(loaded.decision_function(Xt), dec) and np.array_equal(loaded.predict_proba(Xt), P)
    os.remove(path + ".platt")
    with pytest.raises(RuntimeError):
        load_model(path, device="cuda").predict_proba(Xt)


def test_four_classes_solves_and_decisions(data, four):
    from dpsvm_amd.models.svc import SVC

    X, cls = data[0], data[5]
    clf, plain = four
    assert [s["gram_reused"] for s in clf.stats_] == [False, True, True, True]
    assert all(s["converged"] for s in clf.stats_)
    assert [[s["gram_reused"] for s in m] for m in clf.cv_stats_] == [[True] * 5] * 4
    assert all(s["converged"] for m in clf.cv_stats_ for s in m)
    assert np.array_equal(clf.alpha_, plain.alpha_) and np.array_equal(clf.b_, plain.b_)
    assert clf.cv_decision_.dtype == np.float32 and clf.cv_decision_.shape == (N, 4)
    assert clf.probA_.shape == (4,) and clf.probA_.dtype == np.float64 and clf.probB_.shape == (4,)
    for c in range(4):
        yc = np.where(cls == c, 1.0, -1.0).astype(np.float32)
        assert np.array_equal(clf.cv_decision_[:, c], SVC(**CFG).cross_val_decision(X, yc, cv=5, seed=0))
        ref = ref_platt.platt_fit(clf.cv_decision_[:, c], yc)
        print(f"machine {c}: A {clf.probA_[c]:.9f} B {clf.probB_[c]:.9f}  - port {clf.probA_[c] - ref['A']:.3g} "
              f"{clf.probB_[c] - ref['B']:.3g}  {clf.platt_stats_[c]}")
        assert abs(clf.probA_[c] - ref["A"]) <= AB_TOL and abs(clf.probB_[c] - ref["B"]) <= AB_TOL
        assert clf.platt_stats_[c]["status"] == 0
        assert (clf.platt_stats_[c]["iters"], clf.platt_stats_[c]["evals"]) == (ref["iters"], ref["evals"])


def test_four_classes_predict_proba(data, four, tmp_path):
    from dpsvm_amd.models.svc import load_model

    Xt = data[3]
    clf, plain = four
    P = clf.predict_proba(Xt)
    assert P.dtype == np.float32 and P.shape == (NT, 4) and np.array_equal(clf.classes_, np.arange(4))
    dec = clf.decision_function(Xt)
    assert np.max(np.abs(P - ref_platt.proba(dec, clf.probA_, clf.probB_))) <= 2.0 ** -22
    assert np.max(np.abs(P.astype(np.float64).sum(axis=1) - 1.0)) <= 2.0 ** -22
    assert np.array_equal(clf.predict(Xt), plain.predict(Xt))
    fx = ref_platt.load_fixture()
    gap = float(np.max(np.abs(P - np.array(fx["multi_holdout_proba_e6"]).reshape(NT, 4) / fx["scale"])))
    print(f"four classes: max |p - scikit-learn| on the held-out rows {gap:.3g}")
    assert gap <= FIXTURE_TOL
    path = str(tmp_path / "four.txt")
    clf.save(path)
    loaded = load_model(path, device="cuda")
    assert np.array_equal(loaded.decision_function(Xt), dec) and np.array_equal(loaded.predict_proba(Xt), P)
