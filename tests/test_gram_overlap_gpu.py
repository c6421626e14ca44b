"""The one-product Gram pass across tiles (rbf_gemm_split_h1s_kernel,
docs/DESIGN.md §13) and the solver-owned operand prep (GramAdaptPrep).

The adaptive-Gram tests of test_gram_adapt_gpu.py run fewer tiles than the GPU
has CUs, so every persistent workgroup computes one tile.  Here a workgroup
walks a first, middle and last tile (n = 6990: 784 upper tiles of 256 x 128,
unequal counts per workgroup, partial last row and column tiles), with an odd
(d = 784), an even (d = 768) and the minimal (d = 160: 5) k-block count.  The
oracle is the same Gram by column slabs of 1024 (28 x 8 tiles: one per
workgroup, nothing mirrored): the bits must be equal.
Reference: the kernel rows these replace, svmTrain.cu:212-249 (cuBLAS Sgemv + exp).
"""
import numpy as np
import pytest
import torch

from test_gram_adapt_gpu import TAU, _data

pytestmark = pytest.mark.gpu

N = 6990
SLAB = 1024


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dpsvm_amd.ops import kernels

    return kernels


_cache = {}


def _case(K, d):
    """x [N, d] on the device and its adaptive Gram by one-tile-a-workgroup column slabs (computed once)."""
    if d not in _cache:
        X = _data(N)
        if d != X.shape[1]:
            X = np.ascontiguousarray(np.resize(X, (N, d)))
        x = torch.from_numpy(X).cuda()
        slabs = []
        for c0 in range(0, N, SLAB):
            s = K.rbf_gram(x, x[c0:c0 + SLAB].contiguous(), 0.25, split=True, cold_tau=TAU)
            tiles, _ = K.gram_adapt_last()
            assert 0 < tiles <= 224, tiles  # at most one tile a workgroup
            slabs.append(s)
        _cache[d] = (x, torch.cat(slabs, dim=1))
    return _cache[d]


@pytest.mark.parametrize("d", [784, 768, 160])
def test_symmetric_multi_tile_equals_slabs(K, d):
    x, ref = _case(K, d)
    ka = K.rbf_gram(x, None, 0.25, split=True, cold_tau=TAU)  # (into a NaN-filled output)
    tiles, hot = K.gram_adapt_last()
    assert tiles == 784 and 0 < hot <= tiles, (tiles, hot)
    assert not torch.isnan(ka).any()
    assert torch.equal(ka, ka.T)
    assert torch.equal(ka, ref)


def test_rectangular_multi_tile_equals_slabs(K):
    x, ref = _case(K, 784)
    kb = K.rbf_gram(x, x[:3000].contiguous(), 0.25, split=True, cold_tau=TAU)
    tiles, _ = K.gram_adapt_last()
    assert tiles == 28 * 24, tiles
    assert not torch.isnan(kb).any()
    assert torch.equal(kb, ref[:, :3000])


def test_solver_prep_once_repeated_solves_equal_fresh():
    """ws-dense with the adaptive resident Gram: setup builds the split rows, h planes and log2 norms once; a
    second solve() of the same solver (hot buffer re-zeroed) and a fresh solver's first compute the same bits."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dpsvm_amd import SVCConfig
    from dpsvm_amd._native import load
    from dpsvm_amd.utils.datasets import synthetic

    C = load()
    X, y = synthetic("mnist", n=3000, seed=11)
    cfg = SVCConfig(C=10.0, gamma=0.25, eps=1e-3, solver="ws", gram_adapt="on")

    def solver():
        s = C.GpuSolver(cfg.to_native(X.shape[1]), None, 0)
        info = s.setup(X, X.shape[0], y)
        assert info["iteration"] == "ws-dense" and info["gram"] == "split-f16-adaptive", info
        return s

    s = solver()
    a1, r1 = s.solve()
    a2, r2 = s.solve()
    a3, r3 = solver().solve()
    assert r1["converged"]
    for a, r in ((a2, r2), (a3, r3)):
        assert np.array_equal(np.asarray(a), np.asarray(a1))
        assert np.array_equal(np.float64(r["b"]), np.float64(r1["b"]))
        for k in ("iters", "gram_tiles", "gram_hot_tiles"):
            assert r[k] == r1[k], (k, r[k], r1[k])
    assert r1["gram_tiles"] > 0 and r1["gram_hot_tiles"] >= 0
