"""The public fitted attributes of every fit path, as one table (tests/fit_attributes.py): 3 kernels x binary /
one-vs-rest x weights x probability 0 / 3 on SVC, SVR and OneClassSVM per kernel, and Linear() — the exact set of
``name_`` attributes, each one's type, dtype and shape, the None values, and where ``setup_info_`` and
``support_vectors_`` exist.  n = 96, d = 6, device="cpu", clip="box"; the precomputed Gram is X X^T."""
import numpy as np
import pytest

import fit_attributes as fa

SVC_CASES = [(kernel, multi, weights, prob) for kernel in ("rbf", "precomputed", "poly")
             for multi in (False, True) for weights in (False, True) for prob in (0, fa.FOLDS)]


@pytest.fixture(scope="module")
def dat():
    return fa.data()


@pytest.mark.parametrize("kernel,multi,weights,prob", SVC_CASES)
def test_svc_attributes(dat, kernel, multi, weights, prob):
    est = fa.fit(dat, "svc", kernel, multi, weights, prob)
    fa.check_table(est, fa.expected("svc", kernel, multi, weights, prob))
    fa.check_consistency(est, dat, "svc", multi)
    if kernel != "rbf":
        assert est.setup_info_["iteration"] == "cpu" and set(est.setup_info_) == {"iteration", "kernel",
                                                                                  "engine_note"}


@pytest.mark.parametrize("kind", ["svr", "oneclass"])
@pytest.mark.parametrize("kernel", ["rbf", "precomputed", "poly"])
def test_one_block_attributes(dat, kind, kernel):
    est = fa.fit(dat, kind, kernel)
    fa.check_table(est, fa.expected(kind, kernel))
    fa.check_consistency(est, dat, kind, False)


def test_linear_has_no_gamma(dat):
    est = fa.fit(dat, "svc", "linear")
    fa.check_table(est, fa.expected("svc", "linear"))
    assert est.gamma_ is None and est.support_vectors_.shape == (len(est.support_), fa.D)


def test_refits_of_one_estimator(dat):
    """One SVC object refitted binary -> one-vs-rest -> binary and probability 3 -> 0: after each fit everything the
    fit sets is what a fresh object's fit sets, values included.  What a fit does not set stays from the fit before:
    ``cv_folds_`` and ``cv_stats_`` of the last probability fit survive a probability=0 refit (the other
    probability attributes are cleared to None) — recorded as found, stale as it is."""
    from dpsvm_amd import SVC

    est = SVC(C=fa.C_BOUND, gamma=0.5, device="cpu", clip="box")
    stale = {}
    for multi, prob in ((False, 3), (True, 0), (False, 0), (True, 3), (False, 0)):
        fa.fit(dat, "svc", "rbf", multi, False, prob, est=est)
        fresh = fa.fit(dat, "svc", "rbf", multi, False, prob)
        want = fa.expected("svc", "rbf", multi, False, prob)
        if prob:
            stale = {name: (want[name], 3 if multi else 1) for name in ("cv_folds_", "cv_stats_")}
        got = fa.table(est)
        fresh_t = fa.table(fresh)
        assert {k: v for k, v in got.items() if k in fresh_t} == fresh_t
        assert set(got) - set(fresh_t) == (set() if prob else set(stale))
        for name in set(got) - set(fresh_t):  # the stale ones keep the shape of the fit that set them
            spec, k = stale[name]
            assert got[name] == fa.resolve({name: spec}, est, k)[name]
        fa.check_table(fresh, want)
        fa.check_consistency(est, dat, "svc", multi)
        for name, v in vars(fresh).items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(getattr(est, name), v), name
        assert est.b_.tolist() == fresh.b_.tolist() if multi else est.b_ == fresh.b_
