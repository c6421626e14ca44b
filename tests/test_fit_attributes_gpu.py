"""The table of test_fit_attributes_cpu.py on the device: 3 kernels x binary / one-vs-rest x probability 0 / 3, the
same shapes.  On the GPU every kernel publishes ``setup_info_``; binary RBF keeps its solver for
``train_accuracy()``, the Gram fits answer it from the solves' gradients."""
import pytest

import fit_attributes as fa

pytestmark = pytest.mark.gpu

CASES = [(kernel, multi, prob) for kernel in ("rbf", "precomputed", "poly") for multi in (False, True)
         for prob in (0, fa.FOLDS)]


@pytest.fixture(scope="module")
def dat():
    return fa.data()


@pytest.mark.parametrize("kernel,multi,prob", CASES)
def test_svc_attributes(dat, kernel, multi, prob):
    est = fa.fit(dat, "svc", kernel, multi, False, prob, device="cuda")
    fa.check_table(est, fa.expected("svc", kernel, multi, False, prob, device="cuda"))
    fa.check_consistency(est, dat, "svc", multi)
    assert est.device_ == "cuda:0"
    assert isinstance(est.setup_info_, dict)
    if kernel == "rbf" and not multi:  # the kept solver's device pass against the predictor's
        assert est._solver is not None
        assert est.train_accuracy() == est.score(dat["X"], dat["y2"])
    if kernel == "precomputed" and not multi and not prob:  # from the solve's gradient against K(train, train)
        assert est.train_accuracy() == est.score(dat["K"], dat["y2"])
