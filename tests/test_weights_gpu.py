"""Sample / class weights (per-row C_i = C w_i) on the working-set engines: every
ws_solve load path (one block, gathered multi-block, direct_sub), both clipping
modes, both pair choices, ws-cache, GpuSolver.set_row_C on one resident Gram, and
one-vs-rest with class_weight.

Data, weights and oracles: tests/ref_smo_weighted.py and
tests/data/libsvm_weighted_blobs.json (scikit-learn, tol 1e-7).  Tolerances are
those of tests/test_ws_gpu.py; two eps-level solutions of this data differ by
about 1e-3.  clip="independent" (the reference's rule) does not keep
sum(alpha y) = 0, so the point it stops at depends on the trajectory: it is
checked by the stop test on the exact gradient and by its box; clip="box" also
against the fixture and the numpy model.
"""
import numpy as np
import pytest
import torch

from ref_smo import decision, rbf_gram
from ref_smo_weighted import GAMMA, N, D, kkt_gap_w, load_fixture, shared_data, smo_reference_w

pytestmark = pytest.mark.gpu

SHAPES = {
    "one": dict(ws_blocks=1, ws_size=192),      # one block: the sub-Gram gathered by ws_gather
    "gather": dict(ws_blocks=4, ws_size=96),    # multi-block, sub-Grams gathered
    "direct": dict(ws_blocks=8, ws_size=48),    # multi-block, blocks of <= 64 rows: direct_sub
}
CONFIGS = [(s, c, 1) for s in SHAPES for c in ("independent", "box")] + [("one", "independent", 2), ("one", "box", 2)]
KKT_TOL = 2e-3 + 2e-4


@pytest.fixture(scope="module")
def data():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    X, y, w, Xt, yt, cls = shared_data()
    wz = w.copy()
    zero = np.random.default_rng(11).choice(N, 150, replace=False)
    wz[zero] = 0.0
    return dict(X=X, y=y, w=w, wz=wz, zero=zero, Xt=Xt, cls=cls, K=rbf_gram(X, GAMMA), fx=load_fixture(), ref={})


def _svc(shape="one", clip="box", wss=1, C=1.0, **kw):
    from dpsvm_amd.models.svc import SVC

    cfg = dict(C=C, gamma=GAMMA, device="cuda", solver="ws", shrink="off", clip=clip, ws_wss=wss)
    cfg.update(SHAPES[shape])
    cfg.update(kw)
    return SVC(**cfg)


def _numpy_ref(data, Cv, w):
    """the float64 model with zero-weight rows, box clipping: once per C"""
    if Cv not in data["ref"]:
        a, b, _ = smo_reference_w(data["X"], data["y"], Cv * w, GAMMA, clip="box", K=data["K"])
        data["ref"][Cv] = (a, b, decision(data["X"], data["y"], a, b, GAMMA, data["Xt"]))
    return data["ref"][Cv]


def _check_solution(clf, data, w, Cv, shape, tag):
    y = data["y"]
    rc = (np.float32(Cv) * w.astype(np.float32)).astype(np.float32)
    info = clf.setup_info_
    assert info["iteration"] == "ws-dense" and clf.converged_
    assert info["ws_blocks"] == SHAPES[shape]["ws_blocks"] and info["ws_q_max"] == SHAPES[shape]["ws_size"]
    assert np.array_equal(clf.row_C_, rc)
    assert np.all(clf.alpha_ >= 0) and np.all(clf.alpha_ <= rc)  # exactly inside each row's own box
    assert np.all(clf.alpha_[rc == 0] == 0)
    gap = kkt_gap_w(data["K"], y, clf.alpha_, rc)
    print(f"{tag}: weighted KKT gap {gap:.3g}  pair steps {clf.n_iter_}  rounds {clf.n_rounds_}  "
          f"at bound {clf.n_bounded_}  sum(alpha y) {float(np.sum(clf.alpha_.astype(np.float64) * y)):.3g}")
    assert gap < KKT_TOL


def _close(clf, ay_ref, b_ref, dec_ref, data, Cv, tag):
    ay = clf.alpha_ * data["y"]
    db, da = abs(clf.b_ - b_ref), float(np.max(np.abs(ay - ay_ref)))
    dec = clf.decision_function(data["Xt"])
    dd = float(np.max(np.abs(dec - dec_ref)))
    sign = float(np.mean((dec >= 0) == (np.asarray(dec_ref) >= 0)))
    print(f"{tag}: |db| {db:.3g}  max|da| {da:.3g}  max|ddec| {dd:.3g}  signs {sign:.4f}")
    assert db < 1e-2 and da < 0.1 * Cv and dd <= 1e-2 and sign > 0.99


@pytest.mark.parametrize("Cv", [1.0, 10.0])
@pytest.mark.parametrize("shape,clip,wss", CONFIGS)
def test_weighted_fit(data, shape, clip, wss, Cv):
    X, y = data["X"], data["y"]
    tag = f"{shape}/{clip}/wss{wss}/C{Cv:g}"
    clf = _svc(shape, clip, wss, Cv).fit(X, y, sample_weight=data["w"])
    _check_solution(clf, data, data["w"], Cv, shape, tag)
    # 150 rows with weight 0: out of the problem, alpha == 0 exactly
    cz = _svc(shape, clip, wss, Cv).fit(X, y, sample_weight=data["wz"])
    _check_solution(cz, data, data["wz"], Cv, shape, tag + "/zeros")
    assert np.all(cz.alpha_[data["zero"]] == 0.0)
    if clip == "box":
        for c in (clf, cz):
            assert abs(float(np.sum(c.alpha_.astype(np.float64) * y))) < 1e-2 * Cv
        run_ = data["fx"]["runs"]["%g" % Cv]
        _close(clf, np.array(run_["alpha_y"]), -run_["intercept"], np.array(run_["holdout_decision"]), data, Cv,
               tag + " vs fixture")
        a, b, dec = _numpy_ref(data, Cv, data["wz"])
        _close(cz, a * y, b, dec, data, Cv, tag + "/zeros vs numpy model")


@pytest.mark.parametrize("shape,clip,wss", CONFIGS)
def test_all_ones_bit_equal_to_unweighted(data, shape, clip, wss):
    """the kRowC instantiations against the scalar ones on a whole solve"""
    X, y = data["X"], data["y"]
    u = _svc(shape, clip, wss).fit(X, y)
    o = _svc(shape, clip, wss).fit(X, y, sample_weight=np.ones(N))
    assert u.row_C_ is None and o.row_C_ is not None and u.converged_
    assert np.array_equal(u.alpha_, o.alpha_) and u.b_ == o.b_
    assert u.n_iter_ == o.n_iter_ and u.n_rounds_ == o.n_rounds_


def test_solver_auto_takes_the_working_set_engine(data):
    from dpsvm_amd.models.svc import SVC

    clf = SVC(C=1.0, gamma=GAMMA, device="cuda").fit(data["X"], data["y"], sample_weight=data["w"])
    assert clf.setup_info_["iteration"] == "ws-dense" and "per-row C" in clf.setup_info_["engine_note"]
    assert clf.converged_ and kkt_gap_w(data["K"], data["y"], clf.alpha_, clf.row_C_) < KKT_TOL
    # train_accuracy stays unweighted
    assert clf.train_accuracy() == pytest.approx(np.mean(clf.predict(data["X"]) == data["y"]), abs=1e-6)


@pytest.mark.parametrize("clip", ["independent", "box"])
def test_ws_cache_bit_identical_to_ws_dense_under_weights(data, clip):
    X, y, w = data["X"], data["y"], data["wz"]
    dense = _svc("one", clip, gram_adapt="off").fit(X, y, sample_weight=w)
    cache = _svc("one", clip, gram_adapt="off", force_cache=True, cache_lines=900, ws_recompute="off").fit(
        X, y, sample_weight=w)
    assert dense.setup_info_["iteration"] == "ws-dense"
    assert cache.setup_info_["iteration"] == "ws-cache" and cache.setup_info_["ws_rows"] == "cache"
    assert cache.converged_ and cache.n_iter_ == dense.n_iter_ and cache.n_rounds_ == dense.n_rounds_
    assert np.array_equal(cache.alpha_, dense.alpha_) and cache.b_ == dense.b_


def test_native_set_row_C(C, data):
    """GpuSolver: setup; solve; set_row_C; solve on the kept Gram; back to the scalar C; after release_cache()"""
    from dpsvm_amd.models.svc import SVCConfig

    X, y, w = data["X"], data["y"], data["wz"]
    cfg = dict(C=1.0, gamma=GAMMA, solver="ws", shrink="off", clip="box")
    p = SVCConfig(**cfg).to_native(D)
    rc = (np.float32(1.0) * w.astype(np.float32)).astype(np.float32)
    s = C.GpuSolver(p, None, 0)
    s.setup(X, N, y)
    a0, i0 = s.solve()
    assert i0["gram_reused"] is False and i0["t_gram"] > 0
    s.set_row_C(rc)
    a1, i1 = s.solve()
    assert i1["gram_reused"] is True and i1["t_gram"] == 0
    fresh = _svc("one", "box", 0, ws_blocks=0).fit(X, y, sample_weight=w)
    assert np.array_equal(a1, fresh.alpha_) and np.float32(i1["b"]) == np.float32(fresh.b_)
    assert i1["iters"] == fresh.n_iter_ and np.all(a1[rc == 0] == 0)
    # the gradient of the zero-weight rows is kept up to date: f_i + y_i - b is their decision value
    g = s.gradient()
    zero = data["zero"]
    dec = fresh.decision_function(X[zero])
    assert np.max(np.abs(g[zero] + y[zero] - i1["b"] - dec)) < 1e-3
    # a second call only copies (same device buffer): still the kept Gram, same result
    s.set_row_C(rc)
    a1b, i1b = s.solve()
    assert i1b["gram_reused"] is True and np.array_equal(a1b, a1)
    # a plain solve after it rebuilds the Gram, with the weights still set
    a1c, i1c = s.solve()
    assert i1c["gram_reused"] is False and np.array_equal(a1c, a1)
    s.set_row_C(None)
    a2, i2 = s.solve()
    assert i2["gram_reused"] is True and np.array_equal(a2, a0) and i2["b"] == i0["b"] and i2["iters"] == i0["iters"]
    s.release_cache()
    s.set_row_C(rc)
    a3, i3 = s.solve()
    assert i3["gram_reused"] is False and i3["t_gram"] > 0
    assert np.array_equal(a3, a1) and i3["b"] == i1["b"]
    for bad in (-rc, np.full(N, np.nan, np.float32), np.where(y > 0, 0, 1).astype(np.float32)):
        with pytest.raises(RuntimeError):
            s.set_row_C(bad)
    # a refused solve (resume with per-row C) changes no state: the requested Gram reuse survives it
    s.set_row_C(rc)
    with pytest.raises(RuntimeError):
        s.solve(C.Checkpoint())
    a4, i4 = s.solve()
    assert i4["gram_reused"] is True and np.array_equal(a4, a1)
    # bounds valid for the labels at set_row_C, then labels that leave the -1 side without a positive C_i
    ip, im = int(np.nonzero(y > 0)[0][0]), int(np.nonzero(y < 0)[0][0])
    two = np.zeros(N, np.float32)
    two[[ip, im]] = 1.0
    s.set_row_C(two)
    y2 = y.copy()
    y2[im] = 1.0
    s.set_labels(y2)
    with pytest.raises(RuntimeError):
        s.solve()
    s.set_labels(y)
    s.set_row_C(rc)
    a5, _ = s.solve()
    assert np.array_equal(a5, a1)
    with pytest.raises(ValueError):
        s.set_row_C(rc[:-1])
    smo = C.GpuSolver(SVCConfig(**dict(cfg, solver="smo")).to_native(D), None, 0)
    smo.setup(X, N, y)
    with pytest.raises(RuntimeError):
        smo.set_row_C(rc)


def test_cli_class_weight_gpu(data, tmp_path, bin_dir):
    """svmTrain --class-weight on the device: the settings it resolves (working-set engine, no shrinking, no
    recompute rounds) and set_row_C, against SVC.fit(class_weight=...)"""
    import json
    import os

    from conftest import run
    from dpsvm_amd.models.svc import SVC
    from dpsvm_amd.utils import datasets

    X, y = datasets.synthetic("blobs", n=2000, d=5, seed=7, sep=1.5)
    p = str(tmp_path / "train.csv")
    datasets.write_csv(p, X, y)
    js = str(tmp_path / "metrics.json")
    base = [os.path.join(bin_dir, "svmTrain"), "-a", "5", "-x", "2000", "-f", p, "-c", "2", "-g", "0.4", "-m",
            str(tmp_path / "m.txt")]
    r = run(base + ["--class-weight", "3,0.5", "--metrics-json", js])
    assert r.returncode == 0, r.stderr
    met = json.load(open(js))
    assert met["class_weight"] == [3.0, 0.5] and met["converged"] and met["engine"] == "ws-dense"
    clf = SVC(C=2.0, gamma=0.4, device="cuda", class_weight={1.0: 3.0, -1.0: 0.5}).fit(X, y)
    assert clf.setup_info_["iteration"] == "ws-dense"
    print(f"CLI b {met['b']:.7f} n_sv {met['n_sv']}  SVC b {clf.b_:.7f} n_sv {clf.n_support_}")
    assert abs(met["b"] - clf.b_) < 1e-4 and abs(met["n_sv"] - clf.n_support_) <= 2
    u = SVC(C=2.0, gamma=0.4, device="cuda", solver="ws").fit(X, y)
    assert abs(u.b_ - clf.b_) > 1e-3  # the weights changed the model
    for refused in (["--solver", "smo"], ["--shrink=on"]):
        r = run(base + ["--class-weight", "3,0.5"] + refused)
        assert r.returncode != 0 and "--class-weight" in r.stderr


def test_multiclass_balanced_on_one_gram(data):
    X, labels = data["X"], np.array([3, 7, 8, 11])[data["cls"]]
    multi = _svc("one", "independent", 0, C=10.0, ws_blocks=0, class_weight="balanced").fit(X, labels)
    assert multi.row_C_.shape == (4, N) and multi.converged_
    assert [s["gram_reused"] for s in multi.stats_] == [False, True, True, True]
    for c, lab in enumerate(multi.classes_):
        yc = np.where(labels == lab, 1.0, -1.0)
        n_c = int(np.sum(yc > 0))
        sw = np.where(yc > 0, N / (2.0 * n_c), N / (2.0 * (N - n_c)))
        one = _svc("one", "independent", 0, C=10.0, ws_blocks=0).fit(X, yc, sample_weight=sw)
        assert np.array_equal(multi.row_C_[c], one.row_C_)
        assert np.array_equal(multi.alpha_[c], one.alpha_) and multi.b_[c] == np.float32(one.b_)
