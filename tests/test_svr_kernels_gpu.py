"""The epsilon-SVR kernels, one launch each on crafted state (ws_kernel_entry.hip probes with fold = n):

  ws_select_fold_kernel   the folded one-pass f update and selection: f against the plain one-pass kernel on the
                          explicitly unfolded input (bit-equal), the candidates against tests/ref_svr.py
  ws_gather_kernel<true>  the one-block gather with Gram access modulo n
  ws_solve                (existing code) on the eta = 0 pair (j, j + n) of a folded sub-problem

Shapes: column counts that do not divide the 256-thread selection group, so the state rows j and j + n sit in
different lanes of the unfolded launch; 66,000 columns reach two columns per thread.
"""
import numpy as np
import pytest
import torch

from ref_svr import KC, KC1, NONE, fold_candidates, fold_f_update, fold_geometry, fold_labels
from test_ws_kernels_gpu import extremes, lists_from_state, merge1_model, padded_block, solve_model

pytestmark = pytest.mark.gpu

C_BOX = 1.0


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dpsvm_amd.ops import kernels

    return kernels


def fold_state(n, L, seed):
    """L Gram lines of n columns, f / alpha of the 2n state rows.  Crafted parts: rows at either bound in both
    halves; workgroup 1's columns all bounded on the up side (alpha_j = C, alpha*_j = 0: its up list is empty);
    columns t1, t2 of workgroup 0 duplicate each other's Gram values and all four of their state rows start at
    the same, lowest f with free alphas (ties across columns and across halves, resolved by the row index)."""
    rng = np.random.default_rng(seed)
    gram = rng.uniform(0.0, 1.0, size=(L, n)).astype(np.float32)
    y = fold_labels(n)
    u = rng.random(2 * n)
    alpha = np.where(u < 0.4, 0.0, np.where(u < 0.6, C_BOX, rng.uniform(0.1, 0.9, 2 * n))).astype(np.float32)
    f = rng.normal(size=2 * n).astype(np.float32)
    G, rpt = fold_geometry(n)
    lo, hi = rpt * 256, min(n, 2 * rpt * 256)  # workgroup 1
    alpha[lo:hi] = C_BOX      # y = +1 at C: not in I_up
    alpha[n + lo:n + hi] = 0  # y = -1 at 0: not in I_up
    t1, t2 = 3, 200
    gram[:, t2] = gram[:, t1]
    for r in (t1, t2, t1 + n, t2 + n):
        alpha[r] = 0.5
        f[r] = -50.0
    return gram, f, alpha, y, (t1, t2)


def apply_list(rng, L, na):
    """na apply rows over L lines: a state row j and its twin j + n share a line, so lines repeat (with
    coefficients of opposite sign: d_alpha_j (+1) and d_alpha*_j (-1)); the coefficients nearly cancel"""
    lines = rng.integers(0, L, size=na).astype(np.int32)
    coef = rng.normal(scale=0.3, size=na).astype(np.float32)
    if na >= 2:
        lines[1] = lines[0]        # j together with j + n
        coef[1] = -coef[0] * np.float32(0.75)
    if na >= 4:
        lines[3] = lines[2]
        coef[3] = -coef[2]         # cancels exactly
    return lines, coef


@pytest.fixture(scope="module")
def select_runs(K):
    """every (shape, list) case run once: the folded kernel, and the plain one-pass kernel on the unfolded input"""
    out = {}
    for n, L in ((300, 24), (700, 24), (66000, 8)):
        gram, f, alpha, y, ties = fold_state(n, L, seed=n)
        unfolded = np.concatenate([gram, gram], axis=1)
        for na in (1, 5, 192):
            lines, coef = apply_list(np.random.default_rng(n + na), L, na)
            zeros = np.zeros(2 * n, np.float32)
            got = K.ws_select(gram, f, alpha, y, zeros, lines, coef, [na], C_BOX, fold=n)
            plain = K.ws_select(unfolded, f, alpha, y, zeros, lines, coef, [na], C_BOX)
            out[(n, na)] = dict(gram=gram, f=f, alpha=alpha, y=y, ties=ties, lines=lines, coef=coef, got=got,
                                plain=plain)
    return out


CASES = [(n, na) for n in (300, 700, 66000) for na in (1, 5, 192)]


@pytest.mark.parametrize("n,na", CASES)
def test_fold_select_f_is_the_plain_kernels_on_the_unfolded_input(select_runs, n, na):
    r = select_runs[(n, na)]
    got, plain = r["got"], r["plain"]
    G, rpt = fold_geometry(n)
    assert (got["G"], got["rpt"]) == (G, rpt) and rpt == (2 if n == 66000 else 1)
    assert got["nonfinite"] == 0
    np.testing.assert_array_equal(got["f"], plain["f"])
    np.testing.assert_array_equal(got["alpha"], r["alpha"])
    # the model of the summation order: the same bits
    np.testing.assert_array_equal(got["f"], fold_f_update(r["gram"][r["lines"]], r["coef"], r["f"], n))
    # f[j] - f[j + n] keeps its value: each half rounds its own add (half an ulp of the result each)
    d0 = r["f"][:n].astype(np.float64) - r["f"][n:]
    d1 = got["f"][:n].astype(np.float64) - got["f"][n:]
    ulp = 2.0 ** -24 * (np.abs(got["f"][:n]) + np.abs(got["f"][n:]) + np.abs(r["f"][:n]) + np.abs(r["f"][n:]))
    assert np.all(np.abs(d1 - d0) <= ulp)


@pytest.mark.parametrize("n,na", CASES)
def test_fold_select_candidates_match_model(select_runs, n, na):
    r = select_runs[(n, na)]
    got = r["got"]
    G, rpt = fold_geometry(n)
    cand = np.asarray(got["cand"], dtype=np.uint64).reshape(G, 2, KC)[:, :, :KC1]
    want = fold_candidates(got["f"], r["alpha"], r["y"], C_BOX, n)
    np.testing.assert_array_equal(cand, want)
    # the crafted parts reached their branches: an empty up list, ties by index, rows of both halves listed
    assert np.all(cand[1, 0] == NONE) and np.all(cand[1, 1] != NONE)
    t1, t2 = r["ties"]
    assert [int(k) & 0xFFFFFFFF for k in cand[0, 0]] == [t1, t2, t1 + n, t2 + n]
    rows = (cand[cand != NONE] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert np.any(rows < n) and np.any(rows >= n)


def test_fold_select_halves_get_the_same_increment(K):
    """equal halves stay equal bit for bit: one accumulated value is added to both"""
    n, L, na = 700, 24, 192
    gram, f, alpha, y, _ = fold_state(n, L, seed=5)
    f[n:] = f[:n]
    lines, coef = apply_list(np.random.default_rng(9), L, na)
    got = K.ws_select(gram, f, alpha, y, np.zeros(2 * n, np.float32), lines, coef, [na], C_BOX, fold=n)
    np.testing.assert_array_equal(got["f"][:n], got["f"][n:])
    assert np.any(got["f"][:n] != f[:n])


def test_fold_select_after_the_stop_updates_f_and_writes_no_candidates(K):
    n, L, na = 300, 24, 5
    gram, f, alpha, y, _ = fold_state(n, L, seed=11)
    lines, coef = apply_list(np.random.default_rng(12), L, na)
    zeros = np.zeros(2 * n, np.float32)
    run = K.ws_select(gram, f, alpha, y, zeros, lines, coef, [na], C_BOX, fold=n)
    for done in (1, 2):  # converged, max_iter: the last round's changes still reach f
        got = K.ws_select(gram, f, alpha, y, zeros, lines, coef, [na], C_BOX, fold=n, done=done)
        np.testing.assert_array_equal(got["f"], run["f"])
        assert not np.any(np.asarray(got["cand"], dtype=np.uint64))  # the probe's buffer starts zeroed
    # as the plain one-pass kernel does
    plain = K.ws_select(np.concatenate([gram, gram], axis=1), f, alpha, y, zeros, lines, coef, [na], C_BOX, done=1)
    np.testing.assert_array_equal(plain["f"], run["f"])
    assert not np.any(np.asarray(plain["cand"], dtype=np.uint64))


def test_fold_select_refuses_what_it_does_not_run(K):
    n, L = 300, 4
    gram, f, alpha, y, _ = fold_state(n, L, seed=2)
    zeros = np.zeros(2 * n, np.float32)
    with pytest.raises(RuntimeError, match="fold"):  # per-row C
        K.ws_select(gram, f, alpha, y, zeros, [0], [0.1], [1], C_BOX, fold=n, row_C=np.ones(2 * n, np.float32))
    with pytest.raises(RuntimeError, match="fold"):  # state rows != 2 fold
        K.ws_select(gram, f[:-1], alpha[:-1], y[:-1], zeros[:-1], [0], [0.1], [1], C_BOX, fold=n)


# ---------------------------------------------------------------- gather
@pytest.mark.parametrize("q_max", [192, 48])
def test_fold_gather_reads_the_gram_modulo_n(K, q_max):
    n, G = 300, 32
    rng = np.random.default_rng(40 + q_max)
    gram = rng.uniform(0.0, 1.0, size=(n, n + 4)).astype(np.float32)  # ldg > n: rows do not alias
    y = fold_labels(n)
    alpha = np.where(rng.random(2 * n) < 0.5, 0.0, rng.uniform(0.1, 0.9, 2 * n)).astype(np.float32)
    f = rng.normal(size=2 * n).astype(np.float32)
    # row 7 and its twin 7 + n lead both sides: the set holds j and j + n
    f[7], f[7 + n] = -9.0, 9.0
    alpha[7] = alpha[7 + n] = 0.5
    f[n + 11], f[11] = -8.0, 8.0
    alpha[11] = alpha[11 + n] = 0.25
    cand = lists_from_state(f, alpha, y, C_BOX, G)
    got = K.ws_gather(gram, cand, [], f, alpha, y, q_max, q_max, 1e-3, fold=n)
    ref = merge1_model(cand, [], q_max, q_max, 1e-3)
    assert got["done"] == 0 and got["q"] == ref["q"] and q_max // 2 < got["q"] <= q_max
    idx = np.asarray(got["idx"])
    assert idx.tolist() == ref["idx"]
    assert {7, 7 + n} <= set(idx.tolist())  # the global extremes of the two sides: always in the set
    q = got["q"]
    line = idx % n
    np.testing.assert_array_equal(np.asarray(got["line"]), line)  # what ws_solve copies into apply_line
    assert np.any(idx >= n) and np.any(idx != line)
    np.testing.assert_array_equal(got["subg"][:q, :q], gram[line][:, line])
    np.testing.assert_array_equal(got["aux"][0, :q], f[idx])
    np.testing.assert_array_equal(got["aux"][1, :q], alpha[idx])
    np.testing.assert_array_equal(got["aux"][2, :q], y[idx])


def test_fold_gather_pads_with_zeros_and_records_the_lines(K):
    """fewer candidates than q_max: the rows past q are zeroed; the recorded lines (WsCtrl::line, which the solve
    copies into the apply list) are idx mod n"""
    n, G, q_max = 300, 2, 48
    rng = np.random.default_rng(77)
    gram = rng.uniform(0.0, 1.0, size=(n, n)).astype(np.float32)
    y = fold_labels(n)
    alpha = np.full(2 * n, 0.5, np.float32)
    f = rng.normal(size=2 * n).astype(np.float32)
    cand = lists_from_state(f, alpha, y, C_BOX, G)
    got = K.ws_gather(gram, cand, [], f, alpha, y, q_max, q_max, 1e-3, fold=n)
    q = got["q"]
    assert got["done"] == 0 and 2 <= q < q_max
    idx = np.asarray(got["idx"])
    line = idx % n
    np.testing.assert_array_equal(np.asarray(got["line"]), line)
    assert np.any(idx >= n)
    np.testing.assert_array_equal(got["subg"][:q, :q], gram[line][:, line])
    assert not np.any(got["subg"][q:, :]) and not np.any(got["subg"][:q, q:])
    assert not np.any(got["aux"][0, q:q_max])


# ---------------------------------------------------------------- solve on the degenerate pair
@pytest.mark.parametrize("wss", [1, 2])
def test_ws_solve_on_the_eta_zero_pair_of_a_folded_sub_problem(K, wss):
    """rows 0 and 4 are the state rows (j, j + n) of one training row: K = 1 between them, labels +1 / -1, both
    alphas positive and f[0] - f[4] = 2 epsilon > 2 eps.  The pair is the maximal violating one; eta = 0 takes
    the tau floor and the joint box removes the common part (the smaller alpha goes to 0 exactly)."""
    rng = np.random.default_rng(3)
    m, C = 4, 1.0
    X = rng.normal(size=(m, 3))
    Kc = np.exp(-0.5 * ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)).astype(np.float32)
    np.fill_diagonal(Kc, 1.0)
    Kq = np.tile(Kc, (2, 2))
    y = fold_labels(m)
    a = np.array([0.4, 0.0, 0.3, 1.0, 0.25, 0.2, 0.0, 0.0], np.float32)
    f = np.array([0.5, 0.41, 0.38, 0.44, 0.3, 0.36, 0.43, 0.39], np.float32)
    bh, bl = extremes(f, a, y, C)
    assert (bh, bl) == (np.float32(0.3), np.float32(0.5))
    eps, rel = 1e-3, 0.3
    eps_floor = np.float32(rel * eps)
    eps_in = max(eps_floor, np.float32(np.float32(rel * np.float32(0.5)) * np.float32(bl - bh)))
    q_max = 8
    Kp, fp, ap, yp = padded_block(Kq, f, a, y, q_max)
    for cap in (1, 3, 8):
        got = K.ws_solve(Kp, fp, ap, yp, [8], q_max, C, clip="box", eps=eps, rel=rel, eps_floor=eps_floor, b_hi=bh,
                         b_lo=bl, inner_max=cap, wss=wss)
        ref_a, ref_steps, _ = solve_model(Kq, f, a, y, C, True, eps_in, 1e-12, cap, w2=wss == 2)
        an = got["alpha"][:8]
        assert np.all(np.isfinite(an)) and np.all((an >= 0) & (an <= C))
        assert got["steps"] == [ref_steps]
        np.testing.assert_allclose(an, ref_a, rtol=2e-6, atol=2e-6 * C)
        if cap == 1:  # the first step is the degenerate pair's: the common part 0.25 leaves both
            assert an[4] == 0.0 and abs(float(an[0]) - 0.15) < 1e-6
            np.testing.assert_array_equal(an[[1, 2, 3, 5, 6, 7]], a[[1, 2, 3, 5, 6, 7]])
