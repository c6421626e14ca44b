"""gram_rows_wsum (gram_wsum.hip): a weighted sum of Gram rows accumulated in fp64 and rounded to fp32 once,
against a numpy fp64 sum over the same fp32 Gram values.

Bound: |out - ref| <= 1 ulp_fp32(ref) for every element.  Derived, not measured: the terms are exact in fp64 (a
product of two fp32 values), so the kernel's and the reference's sums each carry at most m 2^-53 sum|terms| of
rounding, many orders below half an fp32 ulp of the result; only the final rounding to fp32 can then differ, by at
most one place.  The coefficients have mixed signs and magnitudes from 1e-3 to 1e3, so an fp32 accumulator
misses the bound (checked below on the reference's own terms).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# name -> (n, ldg, L, m, lines kind)
CASES = {
    "one_row": (1000, 1024, 8, 1, "shuffled"),
    "dup_lines": (1025, 1028, 200, 300, "shuffled"),      # 300 lines into 200 rows: duplicates; n % 4 == 1
    "identity_slices": (4100, 4100, 4100, 4100, None),    # 5 column groups, several row slices
}


@functools.lru_cache(maxsize=None)
def problem(name):
    n, ldg, L, m, kind = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    gram = rng.random(size=(L, ldg), dtype=np.float32)
    coef = (10.0 ** rng.uniform(-3, 3, size=m) * rng.choice([-1.0, 1.0], size=m)).astype(np.float32)
    lines = None if kind is None else rng.integers(0, L, size=m).astype(np.int32)
    base = (1e3 * rng.standard_normal(n)).astype(np.float32)
    rows = gram[:m] if lines is None else gram[lines]
    ref = coef.astype(np.float64) @ rows[:, :n].astype(np.float64)
    for a in (gram, coef, base, ref):
        a.setflags(write=False)
    return gram, coef, lines, base, ref


def ulp32(ref):
    return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def check(out, ref, what):
    assert out.dtype == np.float32 and out.shape == ref.shape
    err = np.abs(out.astype(np.float64) - ref) / ulp32(ref)
    print(f"{what}: max |out - ref| = {err.max():.3f} ulp_fp32(ref), {np.mean(err > 0.5):.4f} of the elements "
          "beyond half an ulp")
    assert np.all(err <= 1.0)


def check_pad(r):
    assert len(r["pad"]) >= 64 and np.all(r["pad"] == np.float32(r["fill"]))


@pytest.mark.parametrize("name", list(CASES))
def test_gram_wsum_matches_fp64_sum(name):
    from dpsvm_amd.ops import kernels as K

    n = CASES[name][0]
    gram, coef, lines, base, ref = problem(name)
    r = K.gram_rows_wsum(gram, n, coef, lines=lines)
    print(f"{name}: S = {r['S']}")
    check(r["out"], ref, name)
    check_pad(r)  # columns >= n of the padded out are untouched
    if name == "identity_slices":
        assert r["S"] > 1
        # the test's power: the same terms summed in fp32, in order, miss the bound
        terms = coef[:, None] * gram[:, :n]
        seq = np.cumsum(terms, axis=0, dtype=np.float32)[-1]
        assert np.any(np.abs(seq.astype(np.float64) - ref) > ulp32(ref))
    else:
        assert r["S"] >= 1


def test_gram_wsum_base_is_added_before_the_one_rounding():
    from dpsvm_amd.ops import kernels as K

    n = CASES["dup_lines"][0]
    gram, coef, lines, base, ref = problem("dup_lines")
    r = K.gram_rows_wsum(gram, n, coef, lines=lines, base=base)
    check(r["out"], ref + base.astype(np.float64), "with base")
    check_pad(r)
    # a sum rounded first and base added in fp32 afterwards is a different number somewhere
    twice = (ref.astype(np.float32) + base).astype(np.float32)
    assert np.any(twice != (ref + base.astype(np.float64)).astype(np.float32))


@pytest.mark.parametrize("with_base", [False, True])
def test_gram_wsum_empty_list_yields_base_or_zeros(with_base):
    from dpsvm_amd.ops import kernels as K

    n = CASES["dup_lines"][0]
    gram, _, _, base, _ = problem("dup_lines")
    for lines in (None, np.zeros(0, np.int32)):
        r = K.gram_rows_wsum(gram, n, np.zeros(0, np.float32), lines=lines, base=base if with_base else None)
        assert r["S"] == 0
        np.testing.assert_array_equal(r["out"], base if with_base else np.zeros(n, np.float32))
        check_pad(r)


@pytest.mark.parametrize("name", ["dup_lines", "identity_slices"])
def test_gram_wsum_two_runs_are_bit_equal(name):
    from dpsvm_amd.ops import kernels as K

    n = CASES[name][0]
    gram, coef, lines, base, _ = problem(name)
    a = K.gram_rows_wsum(gram, n, coef, lines=lines, base=base)
    b = K.gram_rows_wsum(gram, n, coef, lines=lines, base=base, reps=2)  # the third launch of this call
    assert a["S"] == b["S"] and len(b["us"]) == 2
    np.testing.assert_array_equal(a["out"], b["out"])


def test_gram_wsum_refuses_bad_shapes(C):
    g = np.zeros(4 * 1026, np.float32)
    one = np.ones(1, np.float32)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        C.k_gram_rows_wsum(g, 4, 1026, 1000, None, one)          # ldg % 4 != 0
    with pytest.raises(RuntimeError, match="ldg >= n"):
        C.k_gram_rows_wsum(g, 4, 1026, 1030, None, one)          # ldg < n
    with pytest.raises(RuntimeError, match="out of range"):
        C.k_gram_rows_wsum(np.zeros(4 * 1024, np.float32), 4, 1024, 1000, np.array([4], np.int32), one)
    with pytest.raises(RuntimeError, match="m <= L"):
        C.k_gram_rows_wsum(np.zeros(4 * 1024, np.float32), 4, 1024, 1000, None, np.ones(5, np.float32))
