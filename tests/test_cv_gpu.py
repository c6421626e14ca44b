"""k-fold cross-validation as k solves on one resident Gram (SVC.cross_val_decision):
per fold set_row_C with the fold's weights zeroed, a cold solve, and the held-out
decision values f_i + y_i - b read from the solver's gradient.

Checked against the scikit-learn fixture's out-of-fold decisions
(tests/data/libsvm_weighted_blobs.json) and against five independent GPU fits on
X[train] with decision_function(X[fold]).  clip="box": the comparison is between
solutions of the same dual (tests/test_weights_gpu.py).
"""
import numpy as np
import pytest
import torch

from ref_smo_weighted import GAMMA, N, load_fixture, shared_data

pytestmark = pytest.mark.gpu

CFG = dict(C=1.0, gamma=GAMMA, device="cuda", solver="ws", shrink="off", clip="box")


@pytest.fixture(scope="module")
def cv():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dpsvm_amd.models.svc import SVC

    X, y, w, _, _, _ = shared_data()
    clf = SVC(**CFG)
    dec = clf.cross_val_decision(X, y, cv=5, seed=0, sample_weight=w)
    return X, y, w, clf, dec


def test_folds_and_gram_reuse(cv):
    X, y, w, clf, dec = cv
    folds = np.array_split(np.random.default_rng(0).permutation(N), 5)  # as documented
    assert all(np.array_equal(a, b) for a, b in zip(folds, clf.cv_folds_))
    assert dec.shape == (N,) and dec.dtype == np.float32
    assert [s["gram_reused"] for s in clf.cv_stats_] == [False, True, True, True, True]
    assert all(s["converged"] for s in clf.cv_stats_)
    assert clf.cv_setup_info_["iteration"] == "ws-dense"


def test_against_the_fixture(cv):
    X, y, w, clf, dec = cv
    run_ = load_fixture()["runs"]["1"]
    ref = np.array(run_["cv_decision"])
    dd = float(np.max(np.abs(dec - ref)))
    acc = float(np.mean(np.where(dec < 0, -1.0, 1.0) == y))
    print(f"out-of-fold against scikit-learn: max|ddec| {dd:.3g}  accuracy {acc:.4f} (fixture {run_['cv_accuracy']:.4f})")
    assert dd <= 1e-2 and abs(acc - run_["cv_accuracy"]) <= 0.01


def test_against_independent_fits(cv):
    from dpsvm_amd.models.svc import SVC

    X, y, w, clf, dec = cv
    ref = np.zeros(N, dtype=np.float32)
    for fold in clf.cv_folds_:
        tr = np.setdiff1d(np.arange(N), fold)
        ref[fold] = SVC(**CFG).fit(X[tr], y[tr], sample_weight=w[tr]).decision_function(X[fold])
    dd = float(np.max(np.abs(dec - ref)))
    acc, acc_ref = (float(np.mean(np.where(d < 0, -1.0, 1.0) == y)) for d in (dec, ref))
    print(f"out-of-fold against five subset fits: max|ddec| {dd:.3g}  accuracy {acc:.4f} vs {acc_ref:.4f}")
    assert dd <= 1e-2 and abs(acc - acc_ref) <= 0.01
    assert SVC(**CFG).cross_val_score(X, y, cv=5, seed=0, sample_weight=w) == acc
