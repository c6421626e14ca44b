"""The multi-output decision GEMM (launch::rbf_predict_multi, ops.kernels.rbf_decision_multi):
dec[i, c] = sum_s coef[s, c] K(x_i, sv_s) - b[c] against a float64 torch reference, column by
column, within the single-output GEMM's own tolerance (test_kernels_gpu.py::test_rbf_decision_gemm)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dpsvm_amd.ops import kernels

    return kernels


def _rbf_ref(x, w, gamma):
    x64, w64 = x.double(), w.double()
    d2 = (x64 * x64).sum(1)[None, :] + (w64 * w64).sum(1)[:, None] - 2 * w64 @ x64.T
    return torch.exp(-gamma * d2.clamp_min(0))


def _close(got, ref, coef):
    """column by column: rtol 1e-4, atol 1e-4 (1 + sum |coef[:, c]| / 100)"""
    assert got.shape == ref.shape
    for c in range(ref.shape[1]):
        atol = 1e-4 * (1 + coef[:, c].abs().sum().item() / 100)
        err = (got[:, c].double() - ref[:, c]).abs().max().item()
        assert torch.allclose(got[:, c].double(), ref[:, c], rtol=1e-4, atol=atol), (c, err, atol)


def _case(n, nsv, d, k, seed=0):
    g = torch.Generator(device="cuda").manual_seed(1000 * n + 10 * nsv + k + seed)
    x = torch.rand(n, d, device="cuda", generator=g)
    sv = torch.rand(nsv, d, device="cuda", generator=g)
    coef = torch.randn(nsv, k, device="cuda", generator=g)
    b = torch.randn(k, device="cuda", generator=g)
    return x, sv, coef, b, 1.0 / d


# (n, nsv, d, k), each the smallest shape at its boundary
SHAPES = [
    (130, 129, 128, 3),     # row and SV tile edges, the split path
    (100, 1, 128, 1),       # one SV, one column
    (257, 3000, 784, 10),   # several SV splits, the headline's d and k
    (300, 400, 160, 8),     # pass boundaries of an 8-, 16- or 32-column pass
    (300, 400, 160, 9),
    (300, 400, 160, 16),
    (300, 400, 160, 17),
    (300, 400, 160, 33),
    (200, 257, 54, 4),      # fewer than 128 padded features: the loop of single-output launches
]


@pytest.mark.parametrize("n,nsv,d,k", SHAPES)
def test_rbf_decision_multi(K, n, nsv, d, k):
    x, sv, coef, b, gamma = _case(n, nsv, d, k)
    got = K.rbf_decision_multi(x, sv, coef, gamma, b)
    ref = _rbf_ref(sv, x, gamma) @ coef.double() - b.double()[None, :]
    _close(got, ref, coef)


@pytest.mark.parametrize("n,nsv,d", [(100, 1, 128), (130, 129, 128), (200, 257, 54)])
def test_one_column_is_rbf_decision(K, n, nsv, d):
    x, sv, coef, b, gamma = _case(n, nsv, d, 1)
    got = K.rbf_decision_multi(x, sv, coef, gamma, b)
    one = K.rbf_decision(x, sv, coef[:, 0], gamma, float(b[0]))
    assert torch.equal(got[:, 0], one)


def test_zero_column_is_minus_b(K):
    x, sv, coef, b, gamma = _case(300, 400, 160, 10)
    coef[:, 4] = 0.0
    got = K.rbf_decision_multi(x, sv, coef, gamma, b)
    assert torch.equal(got[:, 4], (-b[4]).expand(300))
    ref = _rbf_ref(sv, x, gamma) @ coef.double() - b.double()[None, :]
    _close(got, ref, coef)


def test_integer_case_columns_not_crossed(K):
    """X and SV in {0, 1, 2}, coef in {-1, 0, 1}: every column agrees with the single-output kernel on that
    column, and a permutation of the columns permutes the output bit for bit."""
    n, nsv, d, k = 260, 390, 128, 10
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randint(0, 3, (n, d), device="cuda", generator=g).float()
    sv = torch.randint(0, 3, (nsv, d), device="cuda", generator=g).float()
    coef = (torch.randint(0, 3, (nsv, k), device="cuda", generator=g) - 1).float()
    b = torch.arange(k, device="cuda").float() / 4
    gamma = 1.0 / d
    got = K.rbf_decision_multi(x, sv, coef, gamma, b)
    for c in range(k):
        one = K.rbf_decision(x, sv, coef[:, c], gamma, float(b[c]))
        atol = 1e-4 * (1 + coef[:, c].abs().sum().item() / 100)
        assert torch.allclose(got[:, c], one, rtol=1e-4, atol=atol), c
    perm = torch.randperm(k, device="cuda", generator=g)
    assert not torch.equal(perm, torch.arange(k, device="cuda"))
    got_p = K.rbf_decision_multi(x, sv, coef[:, perm].contiguous(), gamma, b[perm].contiguous())
    assert torch.equal(got_p, got[:, perm])
