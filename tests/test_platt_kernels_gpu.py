"""The probability kernels (dpsvm_amd/csrc/kernels/platt.hip), one launch each,
against the float64 numpy port (tests/ref_platt.py).

Shapes: the smallest at which each kernel can go wrong — platt_fit_kernel's wave
edge (63 / 64 / 65), its stride edge (1023 / 1024 / 1025: one workgroup of 1024
threads), n = 2, several machines in one launch (the grid index), decisions far
into the exponent guards; holdout_decision_kernel's one-row and whole-array folds
and a slot past the first; proba_rows_kernel's one-row and 1025-row arrays (more
than one block) for k = 1, 2, 4, 33.

Bounds: 1e-6 on A and B (tests/test_platt_cpu.py says why) with the same steps and
evaluations — the counts are what a float32 accumulator fails; 2^-23 on a
probability (one float32 ulp at 1: the kernel computes in fp64 and rounds once),
2^-22 after the k > 2 normalisation.
"""
import numpy as np
import pytest
import torch

import ref_platt
from ref_smo_weighted import shared_data

pytestmark = pytest.mark.gpu

AB_TOL = 1e-6


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dpsvm_amd.ops import kernels

    return kernels


def overlapping(n, seed, scale=1.0):
    """decisions of two overlapping classes (not separable: the fit has a finite optimum), both labels present"""
    rng = np.random.default_rng(seed)
    y = np.where(rng.random(n) < 0.4, 1.0, -1.0).astype(np.float32)
    y[0], y[-1] = 1.0, -1.0
    dec = (scale * (0.8 * y + rng.standard_normal(n))).astype(np.float32)
    return dec, y


def check_fit(got, dec, y, what):
    ref = ref_platt.platt_fit(dec, y)
    print(f"{what}: A {got['A']:.9g} B {got['B']:.9g}  - port {got['A'] - ref['A']:.3g} {got['B'] - ref['B']:.3g}  "
          f"iters {got['iters']}/{ref['iters']} evals {got['evals']}/{ref['evals']} status {got['status']}")
    assert abs(got["A"] - ref["A"]) <= AB_TOL and abs(got["B"] - ref["B"]) <= AB_TOL
    assert (got["iters"], got["evals"], got["status"]) == (ref["iters"], ref["evals"], ref["status"])
    assert abs(got["fval"] - ref["fval"]) <= 1e-9 * max(1.0, abs(ref["fval"]))


@pytest.mark.parametrize("n", [2, 63, 64, 65, 1023, 1024, 1025])
def test_platt_fit_sizes(K, n):
    if n == 2:  # one row a class
        dec, y = np.array([0.7, -0.4], dtype=np.float32), np.array([1.0, -1.0], dtype=np.float32)
    else:
        dec, y = overlapping(n, n)
    (got,) = K.platt_fit(dec[None, :], y[None, :])
    check_fit(got, dec, y, f"n = {n}")


def test_platt_fit_fixture_and_machines(K):
    """the 1500 fixture decisions; three machines with different labels in one launch"""
    fx = ref_platt.load_fixture()
    cls = shared_data()[5]
    decs = np.stack([(np.array(fx["machines"][c]["cv_decision_e6"]) / fx["scale"]).astype(np.float32)
                     for c in (3, 0, 1)])
    ys = np.stack([np.where(cls == c, 1.0, -1.0).astype(np.float32) for c in (3, 0, 1)])
    (one,) = K.platt_fit(decs[:1], ys[:1])
    check_fit(one, decs[0], ys[0], "fixture, binary")
    assert abs(one["A"] - fx["machines"][3]["A"]) <= AB_TOL and abs(one["B"] - fx["machines"][3]["B"]) <= AB_TOL
    three = K.platt_fit(decs, ys)
    assert len(three) == 3 and three[0] == one  # the same bits from another grid
    for c in range(3):
        check_fit(three[c], decs[c], ys[c], f"machine {c} of 3")
    assert len({(r["A"], r["B"]) for r in three}) == 3


def test_platt_fit_exponent_guards(K):
    """separated decisions, |d| from 2 to 40: |A d + B| beyond 25 at the optimum, where 1 + exp(-|x|) rounds to 1
    — both branches of every two-branch form, far out.  (The smoothed targets keep the optimum finite.)"""
    rng = np.random.default_rng(5)
    y = np.where(rng.random(1025) < 0.4, 1.0, -1.0).astype(np.float32)
    dec = (y * rng.uniform(2.0, 40.0, 1025)).astype(np.float32)
    dec[:2], y[:2] = [40.0, -40.0], [1.0, -1.0]
    (got,) = K.platt_fit(dec[None, :], y[None, :])
    check_fit(got, dec, y, "separated, |d| <= 40")
    assert float(np.max(np.abs(got["A"] * dec + got["B"]))) > 25.0


def test_platt_fit_reproducible(K):
    dec, y = overlapping(1500, 11)
    a = K.platt_fit(np.stack([dec, dec]), np.stack([y, y]))
    b = K.platt_fit(np.stack([dec, dec]), np.stack([y, y]))
    assert a == b and a[0] == a[1]
    assert np.float64(a[0]["A"]).tobytes() == np.float64(b[0]["A"]).tobytes()


def test_platt_fit_degenerate(K):
    """all decisions equal: the system is singular up to the ridge, so no values are compared"""
    y = np.where(np.arange(200) % 3 == 0, 1.0, -1.0).astype(np.float32)
    dec = np.full(200, 0.5, dtype=np.float32)
    (got,) = K.platt_fit(dec[None, :], y[None, :])
    n_pos = float(np.sum(y > 0))
    t = np.where(y > 0, (n_pos + 1) / (n_pos + 2), 1.0 / (200 - n_pos + 2))
    start = ref_platt.objective(dec.astype(np.float64), t, 0.0, float(np.log((200 - n_pos + 1) / (n_pos + 1))))
    print(f"degenerate: A {got['A']:.6g} B {got['B']:.6g} fval {got['fval']:.12g} start {start:.12g} "
          f"status {got['status']} iters {got['iters']} evals {got['evals']}")
    assert np.isfinite(got["A"]) and np.isfinite(got["B"]) and np.isfinite(got["fval"])
    assert got["fval"] <= start * (1 + 200 * 2.0 ** -52)  # two summation orders of the 200 starting terms
    assert got["iters"] <= 100 and got["evals"] <= 1 + 100 * 34


@pytest.mark.parametrize("case", ["one row", "all rows", "any order", "slot 2"])
def test_holdout_decision(K, case):
    n = 1025
    rng = np.random.default_rng(17)
    f = rng.standard_normal(n).astype(np.float32) * 3
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(np.float32)
    b = float(np.float32(0.3141592))
    slots, slot = (3, 2) if case == "slot 2" else (1, 0)
    rows = {"one row": np.array([n - 1]), "all rows": np.arange(n), "any order": rng.permutation(n)[:300],
            "slot 2": rng.permutation(n)[:511]}[case]
    before = rng.standard_normal((slots, n)).astype(np.float32)
    got = K.holdout_decision(f, y, rows, b, before, slot)
    want = before.copy()
    want[slot, rows] = (f[rows].astype(np.float64) + y[rows] - b).astype(np.float32)  # the host line it replaces
    assert got.dtype == np.float32 and got.shape == before.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))  # the rest of the buffer untouched


@pytest.mark.parametrize("k", [1, 2, 4, 33])
@pytest.mark.parametrize("n", [1, 1025])
def test_proba_rows(K, n, k):
    rng = np.random.default_rng(100 * k + n)
    A, B = rng.uniform(-8.0, -0.5, k), rng.uniform(-2.0, 2.0, k)
    dec = rng.uniform(-4.5, 4.5, (n, k)).astype(np.float32)
    dec[0, 0] = 4.75  # |A d + B| up to 40
    A[0], B[0] = -8.0, -2.0
    if n > 1:
        dec[1, 0] = -4.75
        assert np.max(np.abs(dec * A + B)) >= 39.0
    got = K.proba_rows(dec, A, B)
    ref = ref_platt.proba(dec, A, B)
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    print(f"n = {n} k = {k}: max |p - float64| {err:.3g}")
    assert got.dtype == np.float32 and got.shape == (n, k)
    assert err <= (2.0 ** -22 if k > 2 else 2.0 ** -23)
    if k > 2:  # k roundings to float32 of values below 1, half an ulp (<= 2^-25) each
        assert np.max(np.abs(got.astype(np.float64).sum(axis=1) - 1.0)) <= k * 2.0 ** -25


def test_proba_rows_zero_sum(K):
    """every sigmoid of a row underflows to 0 (exp(-1000)): 1 / k each; the row beside it is normal"""
    dec = np.array([[1000.0] * 4, [0.5, -0.5, 0.25, 0.0]], dtype=np.float32)
    A, B = np.ones(4), np.zeros(4)
    got = K.proba_rows(dec, A, B)
    assert np.array_equal(got[0], np.full(4, 0.25, dtype=np.float32))
    assert np.max(np.abs(got[1] - ref_platt.proba(dec, A, B)[1])) <= 2.0 ** -22
