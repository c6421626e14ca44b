"""Sample / class weights (per-row C_i = C w_i) on the CPU solver: the oracle's
counterpart of tests/test_weights_gpu.py.

Data, weights and oracles: tests/ref_smo_weighted.py (a float64 numpy model of the
pair rule with per-row bounds) and tests/data/libsvm_weighted_blobs.json
(scikit-learn with sample_weight, tol 1e-7; bench/make_weighted_fixture.py).
Tolerances are those of tests/test_ws_gpu.py: two eps-level solutions of this data
differ by about 1e-3 (scikit-learn tol 1e-3 against 1e-7: max |d dec| 5.1e-4,
|d intercept| <= 1e-4, max |d alpha| <= 1.9e-3 C).

The comparisons with another solver's solution use clip="box": the reference's
independent clipping does not keep sum(alpha y) = 0 (with these weights it drifts
to about -3.3 at C = 1 and the threshold moves by 0.1), so its solution is the
optimum of a different problem; it is checked by its own KKT gap and box.
"""
import json
import os

import numpy as np
import pytest

from conftest import run
from ref_smo import decision, rbf_gram
from ref_smo_weighted import GAMMA, N, kkt_gap_w, load_fixture, pair_step_w, shared_data, smo_reference_w

# The CPU solver follows the reference's do / while: the pair step of the selection that passes the stop test
# (b_lo <= b_hi + 2 eps, asserted below from the solver's own record) is still applied, and that step moves
# every f_j by up to 2 eps / sqrt(eta), so the float64 gap of the returned alphas is not bounded by 2 eps +
# drift as the working-set engines' is (they stop on a selection without a step).  Unweighted fits of this
# data end at 1.9e-3 .. 2.1e-3, the weighted ones at 1.9e-3 .. 2.3e-3; the bound allows one such step at
# eta >= 1 (K(hi, lo) <= 0.5: rows of different blobs, or far apart in one).
KKT_TOL = 2e-3 + 2e-3


@pytest.fixture(scope="module")
def data():
    X, y, w, Xt, yt, cls = shared_data()
    return dict(X=X, y=y, w=w, Xt=Xt, yt=yt, cls=cls, K=rbf_gram(X, GAMMA), fx=load_fixture())


def _svc(**kw):
    from dpsvm_amd.models.svc import SVC

    kw.setdefault("gamma", GAMMA)
    kw.setdefault("device", "cpu")
    return SVC(**kw)


def _close(clf, ay_ref, b_ref, dec_ref, y, Xt, Cv):
    ay = clf.alpha_ * y
    db, da = abs(clf.b_ - b_ref), float(np.max(np.abs(ay - ay_ref)))
    dec = clf.decision_function(Xt)
    dd = float(np.max(np.abs(dec - dec_ref)))
    sign = float(np.mean((dec >= 0) == (np.asarray(dec_ref) >= 0)))
    print(f"C={Cv}: |db| {db:.3g}  max|da| {da:.3g}  max|ddec| {dd:.3g}  signs {sign:.4f}")
    assert db < 1e-2 and da < 0.1 * Cv and dd <= 1e-2 and sign > 0.99


@pytest.mark.parametrize("Cv", [1.0, 10.0])
def test_fit_matches_fixture_and_numpy_model(data, Cv):
    X, y, w = data["X"], data["y"], data["w"]
    run_ = data["fx"]["runs"]["%g" % Cv]
    clf = _svc(C=Cv, clip="box").fit(X, y, sample_weight=w)
    assert clf.converged_
    rc = (np.float32(Cv) * w.astype(np.float32)).astype(np.float32)
    assert np.array_equal(clf.row_C_, rc)
    assert np.all(clf.alpha_ >= 0) and np.all(clf.alpha_ <= rc)
    assert clf.n_bounded_ == int(np.sum((clf.alpha_ == rc) & (rc > 0)))
    assert abs(clf.n_bounded_ - run_["n_bounded"]) <= 0.02 * N  # rows at their own bound, over the five bound values
    gap = kkt_gap_w(data["K"], y, clf.alpha_, rc)
    print(f"C={Cv}: weighted KKT gap {gap:.3g}, sum(alpha y) {float(np.sum(clf.alpha_ * y)):.3g}")
    assert gap < KKT_TOL and clf.stats_["b_lo"] - clf.stats_["b_hi"] <= 2e-3 * (1 + 1e-6)
    assert abs(float(np.sum(clf.alpha_.astype(np.float64) * y))) < 1e-2 * Cv
    _close(clf, np.array(run_["alpha_y"]), -run_["intercept"], np.array(run_["holdout_decision"]), y, data["Xt"], Cv)
    a, b, _ = smo_reference_w(X, y, Cv * w, GAMMA, clip="box", K=data["K"])
    _close(clf, a * y, b, decision(X, y, a, b, GAMMA, data["Xt"]), y, data["Xt"], Cv)


def test_fit_matches_sklearn(data):
    sk = pytest.importorskip("sklearn.svm")
    X, y, w = data["X"], data["y"], data["w"]
    m = sk.SVC(C=1.0, gamma=GAMMA, tol=1e-7).fit(X, y, sample_weight=w)
    ay = np.zeros(N)
    ay[m.support_] = m.dual_coef_[0]
    clf = _svc(C=1.0, clip="box").fit(X, y, sample_weight=w)
    _close(clf, ay, -float(m.intercept_[0]), m.decision_function(data["Xt"]), y, data["Xt"], 1.0)


@pytest.mark.parametrize("clip", ["independent", "box"])
def test_independent_and_box_meet_their_own_kkt(data, clip):
    X, y, w = data["X"], data["y"], data["w"]
    clf = _svc(C=1.0, clip=clip).fit(X, y, sample_weight=w)
    assert clf.converged_
    assert np.all(clf.alpha_ >= 0) and np.all(clf.alpha_ <= clf.row_C_)
    assert kkt_gap_w(data["K"], y, clf.alpha_, clf.row_C_) < KKT_TOL


@pytest.mark.parametrize("clip", ["independent", "box"])
def test_all_ones_bit_equal_to_unweighted(data, clip):
    X, y = data["X"], data["y"]
    u = _svc(C=1.0, clip=clip).fit(X, y)
    o = _svc(C=1.0, clip=clip).fit(X, y, sample_weight=np.ones(N))
    assert u.row_C_ is None and o.row_C_ is not None
    assert np.array_equal(u.alpha_, o.alpha_) and u.b_ == o.b_ and u.n_iter_ == o.n_iter_


def test_pair_update_w_bit_equal_and_geometry(C):
    """C_hi == C_lo: pair_update's values bit for bit; two bounds: the numpy pair rule"""
    rng = np.random.default_rng(3)
    for _ in range(4000):
        Ch, Cl = (float(np.float32(v)) for v in rng.choice([0.25, 0.5, 1, 2, 4], 2))
        frac = rng.choice([0.0, 1.0, rng.random()], 2)
        ah, al = float(np.float32(frac[0] * Ch)), float(np.float32(frac[1] * Cl))
        yh, yl = (float(v) for v in rng.choice([-1.0, 1.0], 2))
        bh, bl = float(np.float32(-rng.random())), float(np.float32(rng.random()))
        k = float(np.float32(rng.random()))
        for clip in (0, 1):
            assert C.pair_update(ah, min(al, Ch), yh, yl, bh, bl, k, Ch, 1e-12, clip, False) == \
                C.pair_update_w(ah, min(al, Ch), yh, yl, bh, bl, k, Ch, Ch, 1e-12, clip, False)
            got = C.pair_update_w(ah, al, yh, yl, bh, bl, k, Ch, Cl, 1e-12, clip, False)
            ref = pair_step_w(ah, al, yh, yl, bh, bl, k, Ch, Cl, "box" if clip else "independent")
            assert 0 <= got[0] <= Ch and 0 <= got[1] <= Cl
            assert abs(got[0] - ref[0]) < 1e-5 * (1 + Ch + Cl) and abs(got[1] - ref[1]) < 1e-5 * (1 + Ch + Cl)
            if clip and ref[0] in (0.0, Ch):
                assert got[0] == np.float32(ref[0])  # snapped exactly onto its own bound


def test_zero_weight_rows_are_out_of_the_problem(data):
    X, y, w = data["X"], data["y"], data["w"].copy()
    zero = np.random.default_rng(11).choice(N, 150, replace=False)
    w[zero] = 0.0
    keep = np.setdiff1d(np.arange(N), zero)
    clf = _svc(C=1.0, clip="box").fit(X, y, sample_weight=w)
    assert clf.converged_ and np.all(clf.alpha_[zero] == 0.0)
    sub = _svc(C=1.0, clip="box").fit(X[keep], y[keep], sample_weight=w[keep])
    ay = np.zeros(N)
    ay[keep] = sub.alpha_ * y[keep]
    _close(clf, ay, sub.b_, sub.decision_function(data["Xt"]), y, data["Xt"], 1.0)


def test_weight_two_equals_a_duplicated_row(data):
    X, y = data["X"], data["y"]
    dup = np.random.default_rng(12).choice(N, 100, replace=False)
    w = np.ones(N)
    w[dup] = 2.0
    a = _svc(C=1.0, clip="box").fit(X, y, sample_weight=w)
    b = _svc(C=1.0, clip="box").fit(np.concatenate([X, X[dup]]), np.concatenate([y, y[dup]]),
                                     sample_weight=np.ones(N + 100))
    dd = float(np.max(np.abs(a.decision_function(data["Xt"]) - b.decision_function(data["Xt"]))))
    print(f"weight 2 against duplicated rows: max|ddec| {dd:.3g}")
    assert dd <= 1e-2


def test_class_weight_balanced_and_dict(data):
    X, y = data["X"], data["y"]
    n_pos = int(np.sum(y > 0))
    sw = np.where(y > 0, N / (2.0 * n_pos), N / (2.0 * (N - n_pos)))
    a = _svc(C=1.0, class_weight="balanced").fit(X, y)
    b = _svc(C=1.0).fit(X, y, sample_weight=sw)
    assert np.array_equal(a.row_C_, b.row_C_) and np.array_equal(a.alpha_, b.alpha_) and a.b_ == b.b_
    d = _svc(C=1.0, class_weight={1.0: 3.0}).fit(X, y)  # missing labels: 1
    assert np.array_equal(d.row_C_, np.where(y > 0, 3.0, 1.0).astype(np.float32))
    # row weight = class weight x sample weight
    e = _svc(C=1.0, class_weight={1.0: 3.0}).fit(X, y, sample_weight=data["w"])
    assert np.array_equal(e.row_C_, (np.where(y > 0, 3.0, 1.0) * data["w"]).astype(np.float32))


def test_multiclass_weights(data):
    X, cls = data["X"][:600], data["cls"][:600]
    labels = np.array([3, 7, 8, 11])[cls]
    m = _svc(C=1.0, class_weight="balanced").fit(X, labels)
    assert m.row_C_.shape == (4, 600)
    for c, lab in enumerate(m.classes_):
        yc = np.where(labels == lab, 1.0, -1.0)
        n_c = int(np.sum(yc > 0))
        sw = np.where(yc > 0, 600 / (2.0 * n_c), 600 / (2.0 * (600 - n_c)))
        one = _svc(C=1.0).fit(X, yc, sample_weight=sw)
        assert np.array_equal(m.row_C_[c], one.row_C_)
        assert np.array_equal(m.alpha_[c], one.alpha_) and m.b_[c] == np.float32(one.b_)
    d = _svc(C=1.0, class_weight={7: 2.0}).fit(X, labels)  # a row's own label in every machine
    assert np.array_equal(d.row_C_, np.tile(np.where(labels == 7, 2.0, 1.0).astype(np.float32), (4, 1)))


def test_validation(data):
    X, y = data["X"][:200], data["y"][:200]
    for bad in (-np.ones(200), np.full(200, np.nan), np.ones(199), np.where(y > 0, 0.0, 1.0),
                np.where(y > 0, 1.0, 0.0)):
        with pytest.raises(ValueError):
            _svc().fit(X, y, sample_weight=bad)
    with pytest.raises(ValueError):
        _svc(class_weight="bogus").fit(X, y)
    w = np.ones(200)
    for kw in (dict(solver="smo"), dict(shrink="on"), dict(ws_recompute="on"), dict(checkpoint_path="ck.bin")):
        with pytest.raises(NotImplementedError):
            _svc(**kw).fit(X, y, sample_weight=w)
    for kw in (dict(comm=object()), dict(resume="ck.bin"), dict(rank_rows=100)):
        with pytest.raises(NotImplementedError):
            _svc().fit(X, y, sample_weight=w, **kw)


def test_native_solve_cpu_validates(C, data):
    from dpsvm_amd.models.svc import SVCConfig

    X, y = data["X"][:200], data["y"][:200]
    p = SVCConfig(gamma=GAMMA).to_native(X.shape[1])
    for bad in (-np.ones(200, np.float32), np.full(200, np.inf, np.float32), np.where(y > 0, 0, 1).astype(np.float32)):
        with pytest.raises(RuntimeError):
            C.solve_cpu(X, y, p, None, None, None, bad)
    with pytest.raises(ValueError):
        C.solve_cpu(X, y, p, None, None, None, np.ones(199, np.float32))


def test_cross_val_decision_cpu(data):
    X, y, w = data["X"], data["y"], data["w"]
    run_ = data["fx"]["runs"]["1"]
    clf = _svc(C=1.0, clip="box")
    dec = clf.cross_val_decision(X, y, cv=5, seed=0, sample_weight=w)
    folds = np.array_split(np.random.default_rng(0).permutation(N), 5)  # as documented
    assert all(np.array_equal(a, b) for a, b in zip(folds, clf.cv_folds_)) and len(clf.cv_stats_) == 5
    ref = np.array(run_["cv_decision"])
    dd = float(np.max(np.abs(dec - ref)))
    acc = float(np.mean(np.where(dec < 0, -1.0, 1.0) == y))
    print(f"out-of-fold: max|ddec| {dd:.3g}  accuracy {acc:.4f} (fixture {run_['cv_accuracy']:.4f})")
    assert dec.shape == (N,) and dd <= 1e-2 and abs(acc - run_["cv_accuracy"]) <= 0.01
    assert _svc(C=1.0, clip="box").cross_val_score(X, y, cv=5, seed=0, sample_weight=w) == acc


def test_cli_class_weight_cpu(tmp_path, bin_dir):
    from dpsvm_amd.utils import datasets

    X, y = datasets.synthetic("blobs", n=400, d=5, seed=7, sep=1.5)
    p = str(tmp_path / "train.csv")
    datasets.write_csv(p, X, y)
    js = str(tmp_path / "metrics.json")
    r = run([os.path.join(bin_dir, "svmTrain"), "-a", "5", "-x", "400", "-f", p, "-c", "2", "-g", "0.4", "-m",
             str(tmp_path / "m.txt"), "--cpu", "--class-weight", "3,0.5", "--metrics-json", js])
    assert r.returncode == 0, r.stderr
    met = json.load(open(js))
    assert met["class_weight"] == [3.0, 0.5] and met["converged"]
    clf = _svc(C=2.0, gamma=0.4, class_weight={1.0: 3.0, -1.0: 0.5}).fit(X, y)
    assert met["n_sv"] == clf.n_support_ and abs(met["b"] - clf.b_) < 1e-6
    u = _svc(C=2.0, gamma=0.4).fit(X, y)
    assert abs(u.b_ - clf.b_) > 1e-3  # the weights changed the model
    for bad in ("3", "3,", "0,1", "a,b"):
        assert run([os.path.join(bin_dir, "svmTrain"), "-a", "5", "-x", "400", "-f", p, "-m", str(tmp_path / "m.txt"),
                    "--cpu", "--class-weight", bad]).returncode != 0
    r = run([os.path.join(bin_dir, "svmTrain"), "-a", "5", "-x", "400", "-f", p, "-m", str(tmp_path / "m.txt"),
             "--cpu", "--ranks", "2", "--class-weight", "3,0.5"])
    assert r.returncode != 0 and "one rank" in r.stderr
    # svmSeq shares the flag: the same weighted model, and the same refusals
    js2 = str(tmp_path / "metrics_seq.json")
    seq = [os.path.join(bin_dir, "svmSeq"), "-a", "5", "-x", "400", "-f", p, "-c", "2", "-g", "0.4", "-m",
           str(tmp_path / "m_seq.txt"), "--class-weight", "3,0.5"]
    r = run(seq + ["--metrics-json", js2])
    assert r.returncode == 0, r.stderr
    met2 = json.load(open(js2))
    assert met2["class_weight"] == [3.0, 0.5] and met2["n_sv"] == met["n_sv"] and met2["b"] == met["b"]
    assert met2["iterations"] == met["iterations"]
    r = run(seq + ["--checkpoint", str(tmp_path / "ck.bin"), "--checkpoint-every", "10"])
    assert r.returncode != 0 and "--class-weight" in r.stderr
