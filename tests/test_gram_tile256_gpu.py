"""The one-product Gram pass's stored bits at the shapes where its tile's edges are (rbf_gemm_split.hip:
rbf_gemm_split_h1_kernel, 256 x 256 tiles, plus the hot-tile pass; docs/DESIGN.md §13).

tests/data/gram_onepass_bits.json (bench/make_gram_bits_fixture.py, recorded on the build whose one-product pass
ran 256 x 128 tiles over row-major h planes) holds, per case, the sha256 of the adaptive Gram's bytes and
gram_adapt_last()'s (tiles, hot).  A change to the pass's tile, ring, plane layout or epilogue must store the
same bits and report the same 256 x 128 tiles: a 256 x 256 tile with both halves partial (n = 300), an odd count
of 128-column tiles (n = 600: the last tile has a left half only, 88 wide), a right half of 10 columns (n = 650),
tiles that mirror beside diagonal ones (n = 1100), 5 / 6 / 7 k blocks (d = 160 / 192 / 224), rectangular Grams
with M != N, and more tiles than workgroups (n = 6990).
Reference: the kernel rows these replace, svmTrain.cu:212-249 (cuBLAS Sgemv + exp).
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from test_gram_adapt_gpu import TAU, _data

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "gram_onepass_bits.json")) as _f:
    FIX = json.load(_f)
GAMMA = FIX["gamma"]
SYM = [c for c in FIX["cases"] if c["kind"] == "sym"]
RECT = [c for c in FIX["cases"] if c["kind"] == "rect"]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dpsvm_amd.ops import kernels

    return kernels


_rows = {}
_sym = {}


def _x(n, d):
    if (n, d) not in _rows:
        X = _data(n)
        if d != X.shape[1]:
            X = np.ascontiguousarray(np.resize(X, (n, d)))
        _rows[(n, d)] = torch.from_numpy(X).cuda()
    return _rows[(n, d)]


def _sym_gram(K, n, d):
    """(adaptive symmetric Gram, tiles, hot), computed once (n = 6990 is not kept: 195 MB)."""
    if (n, d) in _sym:
        return _sym[(n, d)]
    k = K.rbf_gram(_x(n, d), None, GAMMA, split=True, cold_tau=TAU)  # (into a NaN-filled output)
    r = (k,) + tuple(K.gram_adapt_last())
    if n <= 2048:
        _sym[(n, d)] = r
    return r


def _sha(k):
    return hashlib.sha256(np.ascontiguousarray(k.cpu().numpy()).tobytes()).hexdigest()


def test_fixture_holds_the_cases():
    assert FIX["tau_log2"] == -22 and TAU == 2.0 ** -22
    assert sorted((c["n"], c["d"]) for c in SYM) == sorted(
        [(n, d) for n in (300, 600, 650, 700, 1100) for d in (160, 192, 224)] + [(6990, 160)])
    assert sorted((c["m"], c["n"], c["d"]) for c in RECT) == [(300, 700, 160), (700, 130, 160), (700, 300, 160)]


@pytest.mark.parametrize("case", SYM, ids=lambda c: f"n{c['n']}-d{c['d']}")
def test_symmetric_bits_equal_fixture(K, case):
    k, tiles, hot = _sym_gram(K, case["n"], case["d"])
    assert (tiles, hot) == (case["tiles"], case["hot"]), (tiles, hot)
    assert tiles > 0  # the adaptive plan ran
    assert not torch.isnan(k).any()
    assert torch.equal(k, k.T)
    assert _sha(k) == case["sha256"]


@pytest.mark.parametrize("case", RECT, ids=lambda c: f"m{c['m']}-n{c['n']}-d{c['d']}")
def test_rectangular_bits_equal_fixture_and_symmetric(K, case):
    m, n, d = case["m"], case["n"], case["d"]
    big = max(m, n)
    x = _x(big, d)
    k = K.rbf_gram(x[:m].contiguous(), x[:n].contiguous(), GAMMA, split=True, cold_tau=TAU)
    tiles, hot = K.gram_adapt_last()
    assert (tiles, hot) == (case["tiles"], case["hot"]), (tiles, hot)
    assert tiles > 0
    assert not torch.isnan(k).any()
    assert _sha(k) == case["sha256"]
    ks, _, _ = _sym_gram(K, big, d)
    assert torch.equal(k, ks[:m, :n])
