"""The chunked host loop behind GpuPredictor.decision / decision_multi and GpuSolver.decision: a host
matrix goes through the device in chunks of 2^20 rows, so 2^20 + 300 rows is the smallest input with
a second chunk (and a tail with a partial 128-row tile).  The split count of a launch depends on its
row count, so a chunked result is not bit-equal to one big launch; it is bit-equal to the same rows
passed as a call of their own, which is what is asserted.  Also: zero rows in, and a model without
support vectors (every decision value is exactly -b)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK, TAIL = 2 ** 20, 300
NSV = 200


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dpsvm_amd._native import load

    return load()


def _rows(d, seed):
    """2^20 + 300 rows: a 1,024-row random block tiled"""
    block = np.random.default_rng(seed).random((1024, d), dtype=np.float32)
    return np.ascontiguousarray(np.tile(block, (CHUNK // 1024 + 1, 1))[:CHUNK + TAIL])


def _binary_model(C, d, nsv, b=0.25, seed=1):
    rng = np.random.default_rng(seed)
    m = C.Model()
    m.gamma, m.b, m.d = 1.0 / d, b, d
    m.x = rng.random((nsv, d), dtype=np.float32)
    m.alpha = rng.random(nsv, dtype=np.float32)
    m.y = np.where(rng.random(nsv) < 0.5, -1.0, 1.0).astype(np.float32)
    return m


def _multi_model(C, d, nsv, k=3, seed=2):
    rng = np.random.default_rng(seed)
    m = C.MultiModel()
    m.gamma, m.d = 1.0 / d, d
    m.classes = np.arange(k, dtype=np.float32)
    m.b = np.array([0.5, -1.25, 2.0], dtype=np.float32)[:k]
    m.x = rng.random((nsv, d), dtype=np.float32)
    m.coef = rng.standard_normal((nsv, k)).astype(np.float32)
    return m


def _check_chunks(f, X):
    full = f(X)
    assert full.shape[0] == CHUNK + TAIL and np.all(np.isfinite(full))
    assert np.array_equal(full[:CHUNK], f(X[:CHUNK]))
    assert np.array_equal(full[CHUNK:], f(X[CHUNK:]))
    return full


def test_predictor_decision_second_chunk(C):
    """d = 16: the f32-input decision GEMM"""
    pred = C.GpuPredictor(_binary_model(C, 16, NSV), 0)
    full = _check_chunks(pred.decision, _rows(16, 3))
    assert full.shape == (CHUNK + TAIL,)
    assert np.array_equal(full[1024:2048], full[:1024])  # the tiled block, within one launch


def test_predictor_decision_multi_second_chunk(C):
    """d = 128, k = 3: the multi-output split kernel"""
    pred = C.GpuPredictor(_multi_model(C, 128, NSV), 0)
    full = _check_chunks(pred.decision_multi, _rows(128, 4))
    assert full.shape == (CHUNK + TAIL, 3)


@pytest.fixture(scope="module")
def solved(C):
    from dpsvm_amd.models.svc import SVCConfig
    from dpsvm_amd.utils.datasets import synthetic

    X, y = synthetic("blobs", n=512, d=16, seed=1, sep=2.0)
    s = C.GpuSolver(SVCConfig(C=1.0, gamma=1.0 / 16).to_native(16), None, 0)
    s.setup(X, 512, y)
    alpha, info = s.solve(None, None)
    assert info["converged"]
    return s, alpha, float(info["b"])


def test_solver_decision_second_chunk(solved):
    s, alpha, b = solved
    full = _check_chunks(lambda X: s.decision(alpha, b, X), _rows(16, 5))
    assert full.shape == (CHUNK + TAIL,)


def test_zero_rows(C):
    assert C.GpuPredictor(_binary_model(C, 16, NSV), 0).decision(np.zeros((0, 16), np.float32)).shape == (0,)
    assert C.GpuPredictor(_multi_model(C, 128, NSV), 0).decision_multi(np.zeros((0, 128), np.float32)).shape == (0, 3)


def test_solver_decision_zero_rows(solved):
    """GpuSolver.decision shares the predictors' loop and with it their zero-row return; its own copy of the
    loop sized a launch of zero rows first (an integer division by zero on the host)"""
    s, alpha, b = solved
    assert s.decision(alpha, b, np.zeros((0, 16), np.float32)).shape == (0,)


def test_zero_support_vectors(C):
    X = np.random.default_rng(6).random((300, 16), dtype=np.float32)
    one = C.GpuPredictor(_binary_model(C, 16, 0, b=0.25), 0).decision(X)
    assert one.shape == (300,) and np.all(one == np.float32(-0.25))
    multi = _multi_model(C, 16, 0)
    dec = C.GpuPredictor(multi, 0).decision_multi(X)
    assert dec.shape == (300, 3) and np.array_equal(dec, np.tile(-multi.b, (300, 1)))
