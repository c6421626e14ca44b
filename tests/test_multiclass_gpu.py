"""One-vs-rest multi-class SVC on the GPU: k solves of one GpuSolver on one resident Gram
(set_labels), the multi-output predictor, and the model file.

Four Gaussian blobs in d = 32 (n = 1500, unit variance, centres 2.5 apart: the classes
overlap and about half the rows of every machine are support vectors), labels 3 / 7 / 8 / 11,
C = 10, gamma = 1 / 32.  The Gram is the same values whether a solve builds or keeps it and the
engines are deterministic, so every machine must equal an independent binary fit bit for bit.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LABELS = np.array([3, 7, 8, 11])
N, D, NT = 1500, 32, 400
CFG = dict(C=10.0, gamma=1.0 / 32, device="cuda", shrink="off")


def _blobs(n, seed):
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 4, n)
    centres = np.zeros((4, D), dtype=np.float32)
    for c in range(4):
        centres[c, c] = 2.5 / np.sqrt(2.0)  # pairwise distance 2.5
    X = (centres[cls] + rng.standard_normal((n, D))).astype(np.float32)
    return X, LABELS[cls]


@pytest.fixture(scope="module")
def data():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    X, y = _blobs(N, 1)
    Xt, yt = _blobs(NT, 2)
    return X, y, Xt, yt


@pytest.fixture(scope="module", params=["ws", "smo"])
def fits(request, data):
    """the multi-class fit and the k independent binary fits of one solver setting"""
    from dpsvm_amd.models.svc import SVC

    X, y, Xt, yt = data
    multi = SVC(solver=request.param, **CFG).fit(X, y)
    binary = [SVC(solver=request.param, **CFG).fit(X, np.where(y == c, 1, -1)) for c in multi.classes_]
    return multi, binary


def test_machines_equal_independent_fits(fits, data):
    multi, binary = fits
    assert np.array_equal(multi.classes_, LABELS)
    assert multi.alpha_.shape == (4, N) and multi.b_.shape == (4,) and multi.intercept_.shape == (4,)
    assert multi.n_iter_.shape == (4,) and multi.converged_ and multi.status_ == 1
    for c, one in enumerate(binary):
        assert one.converged_
        assert np.array_equal(multi.alpha_[c], one.alpha_), c
        assert np.array_equal(multi.b_[c], np.float32(one.b_)), c
    union = np.nonzero((multi.alpha_ > 0).any(axis=0))[0]
    assert np.array_equal(multi.support_, union) and multi.n_support_ == len(union)
    assert multi.dual_coef_.shape == (4, len(union)) and multi.support_vectors_.shape == (len(union), D)
    assert multi.fit_time_ == pytest.approx(sum(s["t_solve"] for s in multi.stats_))


def test_gram_built_once(fits):
    multi, _ = fits
    assert len(multi.stats_) == 4
    assert multi.stats_[0]["gram_reused"] is False and multi.stats_[0]["t_gram"] > 0
    for s in multi.stats_[1:]:
        assert s["gram_reused"] is True and s["t_gram"] == 0


def test_predictions(fits, data, tmp_path):
    from dpsvm_amd.models.svc import load_model

    multi, binary = fits
    X, y, Xt, yt = data
    dec = multi.decision_function(Xt)
    assert dec.shape == (NT, 4)
    for c, one in enumerate(binary):
        ref = one.decision_function(Xt)
        atol = 1e-4 * (1 + np.abs(multi.dual_coef_[c]).sum() / 100)
        assert np.allclose(dec[:, c], ref, rtol=1e-4, atol=atol), c
    pred = multi.predict(Xt)
    assert np.array_equal(pred, multi.classes_[np.argmax(dec, axis=1)])
    assert multi.score(Xt, yt) == np.mean(pred == yt)
    assert multi.train_accuracy() == np.mean(multi.predict(X) == y)
    path = str(tmp_path / "ovr.model")
    multi.save(path)
    loaded = load_model(path, device="cuda")
    assert np.array_equal(loaded.classes_, LABELS)
    assert np.array_equal(loaded.predict(Xt), pred)


@pytest.mark.parametrize("solver", ["ws", "smo"])
def test_native_label_swap(C, data, solver):
    """GpuSolver: setup; solve; set_labels; solve — and what a plain second solve, and a solve after
    release_cache(), report"""
    from dpsvm_amd.models.svc import SVC, SVCConfig

    X, y, _, _ = data
    cfg = SVCConfig(solver=solver, **CFG)
    p = cfg.to_native(D)
    y0 = np.where(y == 3, 1, -1).astype(np.float32)
    y1 = np.where(y == 7, 1, -1).astype(np.float32)
    s = C.GpuSolver(p, None, 0)
    s.setup(X, N, y0)
    a0, i0 = s.solve()
    assert i0["gram_reused"] is False and i0["t_gram"] > 0
    # a plain second solve rebuilds the Gram in its timed region
    a0b, i0b = s.solve()
    assert i0b["gram_reused"] is False and i0b["t_gram"] > 0
    assert np.array_equal(a0, a0b) and i0["b"] == i0b["b"]
    s.set_labels(y1)
    a1, i1 = s.solve()
    assert i1["gram_reused"] is True and i1["t_gram"] == 0
    one = SVC(solver=solver, **CFG).fit(X, y1)
    assert np.array_equal(a1, one.alpha_) and np.float32(i1["b"]) == np.float32(one.b_)
    # the swap alone does not carry over: the next plain solve builds the Gram again
    a1b, i1b = s.solve()
    assert i1b["gram_reused"] is False and np.array_equal(a1b, a1)
    # no Gram in place: set_labels + solve rebuilds it, and still matches
    s.release_cache()
    s.set_labels(y0)
    a2, i2 = s.solve()
    assert i2["gram_reused"] is False and i2["t_gram"] > 0
    assert np.array_equal(a2, a0) and i2["b"] == i0["b"]


def test_binary_path_unchanged(C, data, tmp_path):
    from dpsvm_amd.models.svc import SVC

    X, y, Xt, _ = data
    two = SVC(**CFG).fit(X, np.where(y == 3, 3, 8))
    assert two.alpha_.shape == (N,) and isinstance(two.b_, float)
    assert two.decision_function(Xt).shape == (NT,)
    assert set(np.unique(two.predict(Xt))) <= {3, 8}
    assert two.stats_["gram_reused"] is False
    path = str(tmp_path / "binary.model")
    two.save(path)
    m = C.read_model(path)
    assert m.nsv == two.n_support_ and m.d == D
    assert not C.is_multi_model(path)
