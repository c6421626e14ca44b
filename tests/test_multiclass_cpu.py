"""One-vs-rest multi-class SVC on the CPU solver, the multi-class model file, and the limits
the multi-class fit states."""
import dataclasses

import numpy as np
import pytest

from dpsvm_amd.models.svc import SVC, SVCConfig, load_model

CFG = dict(C=10.0, gamma=1.0 / 8, device="cpu")


def _blobs(n, d, sep, seed, labels=(2, 5, 9)):
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, len(labels), n)
    centres = np.zeros((len(labels), d), dtype=np.float32)
    for c in range(len(labels)):
        centres[c, c] = sep / np.sqrt(2.0)  # pairwise distance sep
    X = (centres[cls] + rng.standard_normal((n, d))).astype(np.float32)
    return X, np.asarray(labels)[cls]


@pytest.fixture(scope="module")
def fits():
    X, y = _blobs(300, 8, 2.5, 3)
    multi = SVC(**CFG).fit(X, y)
    binary = [SVC(**CFG).fit(X, np.where(y == c, 1, -1)) for c in multi.classes_]
    return X, y, multi, binary


def test_machines_equal_independent_cpu_fits(fits):
    X, y, multi, binary = fits
    assert np.array_equal(multi.classes_, [2, 5, 9])
    assert multi.alpha_.shape == (3, 300) and multi.b_.shape == (3,) and multi.n_iter_.shape == (3,)
    assert len(multi.stats_) == 3 and multi.converged_
    for c, one in enumerate(binary):
        assert np.array_equal(multi.alpha_[c], one.alpha_), c
        assert multi.b_[c] == np.float32(one.b_), c
    union = np.nonzero((multi.alpha_ > 0).any(axis=0))[0]
    assert np.array_equal(multi.support_, union)
    assert multi.dual_coef_.shape == (3, len(union))
    assert np.array_equal(multi.intercept_, -multi.b_)


def test_predict_is_argmax_of_binary_decisions(fits):
    X, y, multi, binary = fits
    Xt, yt = _blobs(120, 8, 2.5, 4)
    dec = multi.decision_function(Xt)
    assert dec.shape == (120, 3)
    ref = np.stack([one.decision_function(Xt) for one in binary], axis=1)
    pred = multi.predict(Xt)
    assert np.array_equal(pred, multi.classes_[np.argmax(ref, axis=1)])
    assert np.array_equal(pred, multi.classes_[np.argmax(dec, axis=1)])
    assert multi.score(Xt, yt) == np.mean(pred == yt)


def test_separated_blobs_train_to_accuracy_one():
    # centres 10 apart at unit variance: separation is certain by construction
    X, y = _blobs(300, 8, 10.0, 5)
    m = SVC(**CFG).fit(X, y)
    assert m.train_accuracy() == 1.0
    assert np.array_equal(m.predict(X), y)


def test_model_file_round_trip(fits, tmp_path, C):
    X, y, multi, _ = fits
    path = str(tmp_path / "ovr.model")
    multi.save(path, precision=9)
    with open(path) as fh:
        head = fh.readline().split()
    assert head == ["dpsvm-ovr", "3", str(multi.n_support_), "8"]
    assert C.is_multi_model(path)
    m = C.read_multi_model(path)
    src = multi.to_model()
    assert m.k == 3 and m.nsv == multi.n_support_ and m.d == 8
    assert np.array_equal(m.classes, [2, 5, 9])
    assert m.gamma == np.float32(multi.gamma_)
    assert np.array_equal(m.b, multi.b_)
    assert np.array_equal(m.coef, src.coef) and np.array_equal(m.coef, multi.dual_coef_.T)
    assert np.array_equal(m.x, multi.support_vectors_)
    loaded = load_model(path, device="cpu")
    assert np.array_equal(loaded.classes_, [2, 5, 9])
    assert np.array_equal(loaded.predict(X), multi.predict(X))
    assert np.array_equal(loaded.decision_function(X), multi.decision_function(X))


def test_readers_reject_the_other_format(fits, tmp_path, C):
    X, y, multi, binary = fits
    mpath, bpath = str(tmp_path / "ovr.model"), str(tmp_path / "binary.model")
    multi.save(mpath)
    binary[0].save(bpath)
    with pytest.raises(RuntimeError, match="read_multi_model"):
        C.read_model(mpath)
    with pytest.raises(RuntimeError, match="not a multi-class"):
        C.read_multi_model(bpath)
    assert C.read_model(bpath).nsv == binary[0].n_support_


@pytest.mark.parametrize("kw", [{"comm": object()}, {"resume": "ck.bin"}, {"rank_rows": 100}])
def test_multi_rank_and_resume_not_implemented(kw):
    X, y = _blobs(60, 8, 2.5, 6)
    with pytest.raises(NotImplementedError, match=next(iter(kw))):
        SVC(**CFG).fit(X, y, **kw)


def test_config_round_trip_with_three_classes(fits):
    X, y, multi, _ = fits
    params = multi.get_params()
    assert params == dataclasses.asdict(SVCConfig(**CFG))
    again = SVC(**params)
    assert again.get_params() == params
    assert np.array_equal(again.fit(X, y).alpha_, multi.alpha_)


def test_two_classes_keep_the_binary_interface(fits, tmp_path, C):
    X, y, _, _ = fits
    two = SVC(**CFG).fit(X, np.where(y == 2, 2, 9))
    assert two.alpha_.shape == (300,) and isinstance(two.b_, float)
    assert two.decision_function(X).shape == (300,)
    path = str(tmp_path / "binary.model")
    two.save(path)
    assert not C.is_multi_model(path) and C.read_model(path).nsv == two.n_support_
