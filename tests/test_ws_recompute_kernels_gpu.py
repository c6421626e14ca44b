"""Kernel-level tests of the one-block merge (ws_merge.hpp) and of the recompute
rounds' two kernels (ws_recompute.hip), one launch each on crafted state
(dpsvm_amd.ops.kernels.ws_gather / ws_subgram_split / ws_fupdate_split):

  the merge      through ws_gather, against merge1_model (test_ws_kernels_gpu.py;
                 its invariants: test_ws_merge1_model_cpu.py) — set, order, stop
                 codes exactly; the gathered sub-Gram and aux exactly;
  ws_subgram     the same set as ws_gather on the same state, and the sub-Gram
                 bit-identical to the resident split Gram's entries, zeros in
                 the columns past q;
  ws_fupdate     f bit-identical to the documented summation order over the
                 split Gram's bits (and within a derived bound of float64), the
                 candidate lists, the stop states;
  one round      composed from the probes: the recompute path and the resident-
                 Gram path take the same sub-problem step.

The end-to-end fits (test_ws_recompute_gpu.py) bound only the optimum reached;
a skipped column block, a counted padding row or a wrong merge passes them."""
import functools

import numpy as np
import pytest
import torch

import test_ws_kernels_gpu as W
from test_ws_kernels_gpu import K  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

KC, KC1, NONE = W.KC, W.KC1, W.NONE
RUNNING, CONVERGED, MAX_ITER = 0, 1, 2


def f32_same(a, b):
    """float32 equality that takes NaN == NaN (an empty side reports NaN)"""
    return np.array_equal(np.asarray([a], np.float32), np.asarray([b], np.float32), equal_nan=True)


@pytest.fixture(scope="module")
def noise_gram():
    """a 'Gram' of distinct values: a gathered entry identifies its (row, column)"""
    return np.random.default_rng(7).random((3600, 3600), dtype=np.float32)


def probe_consts():
    from dpsvm_amd._native import load

    C = load()
    return C.kWsProbeApply, np.uint64(C.kWsProbeKey)


def check_merge(got, ref):
    assert got["done"] == ref["done"]
    assert f32_same(got["b_hi"], ref["b_hi"]) and f32_same(got["b_lo"], ref["b_lo"])
    if ref["done"] != RUNNING:
        assert got["n_apply"] == 0  # nothing may be applied twice
        return
    assert got["n_apply"] == probe_consts()[0]  # a running round leaves the apply list to the solve
    assert got["q"] == ref["q"] and got["idx"] == ref["idx"]


def check_set_state(got, st, sub_want, q_max):
    """subg == sub_want on the set, exact zeros in its rows' columns past q, no
    sentinel (NaN) left in rows < q; aux = f / alpha / y of the set"""
    q, idx = got["q"], np.asarray(got["idx"], dtype=np.int64)
    sub = got["subg"]
    assert sub.shape == (q_max, q_max) and not np.isnan(sub[:q]).any()
    np.testing.assert_array_equal(sub[:q, :q], sub_want)
    assert np.all(sub[:q, q:].view(np.uint32) == 0)  # +0.0 exactly
    for r, name in enumerate(("f", "alpha", "y")):
        np.testing.assert_array_equal(got["aux"][r, :q], st[name][idx])


# ---------------------------------------------------------------- the merge, through ws_gather
@pytest.mark.parametrize("name", sorted(W.MERGE1_CASES))
def test_ws_gather_merge_matches_model(K, noise_gram, name):  # noqa: F811
    st, q_max, n_new, prev = W.merge1_case(name)
    ref = W.merge1_model(st["cand"], prev, q_max, n_new, W.MERGE1_EPS)
    W.merge1_case_reaches_its_branch(name, st, prev, ref)
    n = st["n"]
    gram = np.ascontiguousarray(noise_gram[:n, :n])
    got = K.ws_gather(gram, st["cand"], prev, st["f"], st["alpha"], st["y"], q_max, n_new, W.MERGE1_EPS)
    check_merge(got, ref)
    idx = np.asarray(got["idx"], dtype=np.int64)
    check_set_state(got, st, gram[np.ix_(idx, idx)], q_max)
    assert np.all(got["subg"][got["q"]:] == 0)  # rows past q are zeroed (ws_gather_row)
    # the other round parity reads and writes the other halves of the control record
    odd = K.ws_gather(gram, st["cand"], prev, st["f"], st["alpha"], st["y"], q_max, n_new, W.MERGE1_EPS, outer=2)
    assert odd["idx"] == got["idx"] and odd["q"] == got["q"]


@pytest.mark.parametrize("name", sorted(W.merge1_stop_cases()))
def test_ws_gather_stop_codes(K, name):  # noqa: F811
    f, alpha, y, eps, it, max_iter, nonfinite, done = W.merge1_stop_cases()[name]
    cand = W.lists_from_state(f, alpha, y, W.MERGE1_C, 1)
    ref = W.merge1_model(cand, [], 2, 2, eps, iteration=it, max_iter=max_iter, nonfinite=nonfinite)
    assert ref["done"] == done
    gram = np.array([[1.0, 0.25], [0.25, 1.0]], np.float32)
    x = np.array([[0.0, 1.0], [1.0, 0.0]], np.float32)
    for got in (K.ws_gather(gram, cand, [], f, alpha, y, 2, 2, eps, iteration=it, max_iter=max_iter,
                            nonfinite=nonfinite),
                K.ws_subgram_split(x, cand, [], f, alpha, y, 0.5, 2, 2, eps, iteration=it, max_iter=max_iter,
                                   nonfinite=nonfinite)):
        check_merge(got, ref)
        if done != RUNNING:  # a stopped round writes no set
            assert got["q"] == 0 and np.isnan(got["subg"]).all() and np.isnan(got["aux"]).all()


# ---------------------------------------------------------------- ws_subgram_split
# set sizes at the edges of the 64 x 64 tiles and of the tiles that return early: (state, q_max, n_new,
# previous rows, of them picked again) -> q = n_new + previous rows not picked again
_G256 = dict(n=3072, G=256, fgen=W._normal)
SUBGRAM_Q_CASES = {
    "q1": (_G256, 192, 1, 1, 1),
    "q63": (_G256, 192, 40, 23, 0),
    "q64": (_G256, 192, 40, 24, 0),
    "q65": (_G256, 192, 48, 17, 0),
    "q128": (_G256, 192, 96, 32, 0),
    "q150": (_G256, 192, 144, 6, 0),
    "q192": (_G256, 192, 192, 0, 0),
    "q33of40": (_G256, 40, 20, 13, 0),
    "q40of40": (_G256, 40, 30, 10, 0),
    "q65of96": (_G256, 96, 50, 15, 0),
    "q96of96": (_G256, 96, 72, 24, 0),
}
SUBGRAM_Q = dict(q1=1, q63=63, q64=64, q65=65, q128=128, q150=150, q192=192, q33of40=33, q40of40=40, q65of96=65,
                 q96of96=96)


def subgram_x(n, d, seed):
    """rows of different scales (different split shifts), two of them equal"""
    rng = np.random.default_rng(300 + seed)
    X = (rng.normal(size=(n, d)) * rng.choice([0.25, 0.5, 1.0, 2.0], size=(n, 1))).astype(np.float32)
    X[1] = X[0]
    return X


def run_subgram_case(K, noise_gram, st, q_max, n_new, prev, d):  # noqa: F811
    n = st["n"]
    X = subgram_x(n, d, n + d)
    gamma = 0.5 / d
    ref = W.merge1_model(st["cand"], prev, q_max, n_new, W.MERGE1_EPS)
    got = K.ws_subgram_split(X, st["cand"], prev, st["f"], st["alpha"], st["y"], gamma, q_max, n_new, W.MERGE1_EPS)
    check_merge(got, ref)
    dense = K.ws_gather(np.ascontiguousarray(noise_gram[:n, :n]), st["cand"], prev, st["f"], st["alpha"], st["y"],
                        q_max, n_new, W.MERGE1_EPS)
    for k in ("done", "q", "idx", "b_hi", "b_lo", "n_apply"):
        assert got[k] == dense[k], k
    idx = torch.as_tensor(got["idx"], dtype=torch.long, device="cuda")
    gram = K.rbf_gram(torch.from_numpy(X).cuda(), None, gamma, split=True)  # the resident split Gram of the same X
    sub_want = gram[idx][:, idx].cpu().numpy()
    assert np.isfinite(sub_want).all()
    check_set_state(got, st, sub_want, q_max)
    return got


@pytest.mark.parametrize("d", [54, 20])
@pytest.mark.parametrize("name", sorted(SUBGRAM_Q_CASES))
def test_ws_subgram_split_set_sizes_bit_identical_to_the_split_gram(K, noise_gram, name, d):  # noqa: F811
    st, q_max, n_new, prev = W.merge1_case(name, SUBGRAM_Q_CASES)
    got = run_subgram_case(K, noise_gram, st, q_max, n_new, prev, d)
    assert got["q"] == SUBGRAM_Q[name]


@pytest.mark.parametrize("d", [54, 20])
@pytest.mark.parametrize("name", sorted(W.MERGE1_CASES))
def test_ws_subgram_split_merge_cases_match_ws_gather(K, noise_gram, name, d):  # noqa: F811
    st, q_max, n_new, prev = W.merge1_case(name)
    run_subgram_case(K, noise_gram, st, q_max, n_new, prev, d)


# ---------------------------------------------------------------- ws_fupdate_split
FUP_C = 2.0


@functools.lru_cache(maxsize=2)
def fup_state(n, d):
    rng = np.random.default_rng(n + d)
    X = (rng.normal(size=(n, d)) * rng.choice([0.5, 1.0, 2.0], size=(n, 1))).astype(np.float32)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(np.float32)
    u = rng.random(n)
    alpha = np.where(u < 0.4, 0.0, np.where(u < 0.6, FUP_C, rng.uniform(0.1, 1.9, n))).astype(np.float32)
    f = rng.normal(size=n).astype(np.float32)
    assert (alpha == 0).any() and (alpha == np.float32(FUP_C)).any() and ((alpha > 0) & (alpha < FUP_C)).any()
    return X, f, alpha, y


def fup_apply(n, M, seed=0):
    """M changed rows among the columns (the first and the last column among
    them: the diagonal at both ends) and their coefficients"""
    rng = np.random.default_rng(10 * M + seed)
    rows = rng.choice(np.arange(1, n - 1), size=max(0, M - 2), replace=False).tolist()
    rows = ([n - 1] + rows + [0])[:M] if M >= 2 else [n - 1][:M]
    return np.asarray(rows, dtype=np.int32), rng.normal(scale=0.3, size=M).astype(np.float32)


def split_rows_of_gram(K, X, rows, gamma):  # noqa: F811
    """Kb[k] = the split Gram's row rows[k] (rbf_rows_indexed, split; d <= 64
    here, so the small-K kernel: pinned bit-identical to the split Gram by
    test_ws_cache_kernels_gpu.py::test_rbf_rows_miss_bit_identical_to_the_gram_rows;
    test_split_gemm_gpu.py pins only the LDS-DMA kernels, d = 784)"""
    return K.rbf_rows_indexed(torch.from_numpy(X).cuda(), [int(r) for r in rows], gamma, split=True).cpu().numpy()


def k64_rows(X, rows, gamma):
    X64 = X.astype(np.float64)
    sq = (X64 ** 2).sum(1)
    d2 = sq[rows][:, None] + sq[None, :] - 2.0 * (X64[rows] @ X64.T)
    return np.exp(-gamma * np.maximum(d2, 0.0))


def fupdate_model(f, Kb, coef):
    """ws_recompute.hip's order, float32, products rounded before they are added
    (no fused multiply-add): per column, half-wave 0 sums c_k K(k, j) over the
    rows k with k mod 32 in 0-3, 8-11, 16-19, 24-27, half-wave 1 over the others,
    each in row order; f' = f + (acc0 + acc1)"""
    acc = np.zeros((2, len(f)), np.float32)
    for k in range(len(coef)):
        h = 0 if (k % 32) % 8 < 4 else 1
        acc[h] = acc[h] + np.float32(coef[k]) * Kb[k]
    return f + (acc[0] + acc[1])


def f64_bound(f, Kb, K64, coef):
    """(f + sum_k c_k K64(k, j), the bound on |f' - it|) with the bound
    sum|c_k| e_K + (M + 2) 2^-24 (|f_j| + sum|c_k|): e_K = max |Kb - K64| is the
    kernel values' own error on those rows; a term then passes through its
    product, at most M / 2 additions of its chain, the add of the two chains and
    the add to f_j — fewer than M + 2 roundings of relative 2^-24, on partial
    sums no larger than |f_j| + sum|c_k| (K <= 1).  Nothing in it is measured
    from the kernel under test."""
    M = len(coef)
    S = float(np.abs(coef.astype(np.float64)).sum())
    e_K = float(np.abs(Kb.astype(np.float64) - K64).max()) if M else 0.0
    want = f.astype(np.float64) + coef.astype(np.float64) @ K64 if M else f.astype(np.float64)
    return want, S * e_K + (M + 2) * 2.0 ** -24 * (np.abs(f.astype(np.float64)) + S)


def geometry(n):
    G = min(256, (n + 255) // 256)
    return G, (n + G * 256 - 1) // (G * 256)


def check_lists(cand, f, alpha, y, G, rpt):
    """the first kWsCand1 keys a side: the model's; the rest of a list is not written"""
    np.testing.assert_array_equal(cand[:, :, :KC1], W.candidates_model(f, alpha, y, FUP_C, G, rpt, nc=KC1))
    assert np.all(cand[:, :, KC1:] == probe_consts()[1])


FUP_SHAPES = {777: (54, 4, 1), 2500: (20, 10, 1), 70000: (54, 256, 2), 140001: (54, 256, 3)}


@pytest.mark.parametrize("n,M", [(777, 1), (777, 31), (777, 32), (777, 33), (777, 100), (777, 192), (2500, 33),
                                 (2500, 192), (70000, 100), (140001, 192)])
def test_ws_fupdate_split_bit_exact_against_the_summation_order_model(K, n, M):  # noqa: F811
    """777: the last group holds 9 columns (seven idle waves); 2500 x 20: one k
    block; 70000: rpt 2, 16 column blocks a group = 2 W exactly; 140001: rpt 3,
    24 blocks (the loop's second half runs past the end), a partial last group."""
    d, G, rpt = FUP_SHAPES[n]
    assert geometry(n) == (G, rpt)
    X, f, alpha, y = fup_state(n, d)
    gamma = 0.5 / d
    rows, coef = fup_apply(n, M)
    got = K.ws_fupdate_split(X, f, alpha, y, rows, coef, gamma, FUP_C)
    assert (got["G"], got["rpt"]) == (G, rpt)
    assert got["rows_computed"] == M and got["nonfinite"] == 0
    Kb = split_rows_of_gram(K, X, rows, gamma)
    want64, bound = f64_bound(f, Kb, k64_rows(X, rows, gamma), coef)
    ratio = float((np.abs(got["f"].astype(np.float64) - want64) / bound).max())
    model = fupdate_model(f, Kb, coef)
    exact = np.array_equal(got["f"], model)
    print(f"ws_fupdate_split n={n} d={d} M={M}: bit-exact {exact}, "
          f"max |f - f64| / bound = {ratio:.4f}, differing columns {int((got['f'] != model).sum())}")
    np.testing.assert_array_equal(got["f"], model)
    assert ratio <= 1.0
    check_lists(got["cand"], got["f"], alpha, y, G, rpt)


def test_ws_fupdate_split_stop_states(K):  # noqa: F811
    n, (d, G, rpt) = 777, FUP_SHAPES[777]
    X, f, alpha, y = fup_state(n, d)
    gamma = 0.5 / d
    rows, coef = fup_apply(n, 33, seed=1)
    none = (np.zeros(0, np.int32), np.zeros(0, np.float32))
    sentinel = probe_consts()[1]
    # nothing to apply while running: f keeps its bits, the lists are built from it
    got = K.ws_fupdate_split(X, f, alpha, y, *none, gamma, FUP_C)
    assert np.array_equal(got["f"].view(np.uint32), f.view(np.uint32)) and got["rows_computed"] == 0
    check_lists(got["cand"], f, alpha, y, G, rpt)
    # the run ended in the solve (max_iter): its last changes are applied, no lists
    got = K.ws_fupdate_split(X, f, alpha, y, rows, coef, gamma, FUP_C, done=MAX_ITER)
    np.testing.assert_array_equal(got["f"], fupdate_model(f, split_rows_of_gram(K, X, rows, gamma), coef))
    assert got["rows_computed"] == 33 and np.all(got["cand"] == sentinel)
    # ended and nothing to apply: nothing is touched
    got = K.ws_fupdate_split(X, f, alpha, y, *none, gamma, FUP_C, done=CONVERGED)
    assert np.array_equal(got["f"].view(np.uint32), f.view(np.uint32))
    assert got["rows_computed"] == 0 and got["nonfinite"] == 0 and np.all(got["cand"] == sentinel)
    # one infinite f: flagged (and only then)
    g = f.copy()
    g[400] = np.inf
    got = K.ws_fupdate_split(X, g, alpha, y, rows, coef, gamma, FUP_C)
    assert got["nonfinite"] == 1 and got["f"][400] == np.inf
    assert K.ws_fupdate_split(X, f, alpha, y, rows, coef, gamma, FUP_C)["nonfinite"] == 0


def test_probes_reject_malformed_calls(K):  # noqa: F811
    """a malformed call raises before anything is launched"""
    n, d = 300, 20
    X, f, alpha, y = fup_state(n, d)
    ok = (np.asarray([1, 2], np.int32), np.asarray([0.1, -0.1], np.float32))
    with pytest.raises(RuntimeError):  # a row past n
        K.ws_fupdate_split(X, f, alpha, y, np.asarray([1, n], np.int32), ok[1], 0.1, FUP_C)
    with pytest.raises(RuntimeError):  # more than 192 rows
        K.ws_fupdate_split(X, f, alpha, y, np.arange(193, dtype=np.int32), np.zeros(193, np.float32), 0.1, FUP_C)
    with pytest.raises(RuntimeError):  # dp > 64
        K.ws_fupdate_split(np.zeros((n, 65), np.float32), f, alpha, y, *ok, 0.1, FUP_C)
    with pytest.raises(RuntimeError):  # f of another length
        K.ws_fupdate_split(X, f[:-1], alpha, y, *ok, 0.1, FUP_C)
    cand = W.lists_from_state(f, alpha, y, FUP_C, 2)
    with pytest.raises(RuntimeError):  # q_max > 192
        K.ws_subgram_split(X, cand, [], f, alpha, y, 0.1, 194, 194, 1e-3)
    with pytest.raises(RuntimeError):  # a previous-set row past n
        K.ws_subgram_split(X, cand, [n], f, alpha, y, 0.1, 192, 144, 1e-3)
    bad = cand.copy()
    bad[0, 0, 0] = W.make_key(np.float32(-9.0), n)[0]  # a candidate row past n
    with pytest.raises(RuntimeError):
        K.ws_subgram_split(X, bad, [], f, alpha, y, 0.1, 192, 144, 1e-3)
    with pytest.raises(RuntimeError):
        K.ws_gather(np.zeros((n, n), np.float32), bad, [], f, alpha, y, 192, 144, 1e-3)
    with pytest.raises(RuntimeError):  # a Gram of fewer rows than f
        K.ws_gather(np.zeros((n - 1, n), np.float32), cand, [], f, alpha, y, 192, 144, 1e-3)


# ---------------------------------------------------------------- one round, composed from the probes
@pytest.mark.parametrize("clip", ["independent", "box"])
def test_one_round_recompute_path_takes_the_resident_gram_path_step(K, clip):  # noqa: F811
    """ws_subgram_split -> ws_solve -> ws_fupdate_split against ws_gather ->
    ws_solve -> ws_select on the resident split Gram of the same X, q = 150 in
    q_max = 192.  The sub-Gram rows past q differ (never written: the sentinel /
    zeroed) and the apply lists are bit-identical: those rows never reach the
    solve."""
    n, d, q_max, n_new, q_want = 1500, 54, 192, 144, 150
    rng = np.random.default_rng(77)
    X = subgram_x(n, d, 5)
    gamma = 0.5 / d
    gram = K.rbf_gram(torch.from_numpy(X).cuda(), None, gamma, split=True).cpu().numpy()
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(np.float32)
    u = rng.random(n)
    alpha = np.where(u < 0.5, 0.0, np.where(u < 0.65, FUP_C, rng.uniform(0.1, 1.9, n))).astype(np.float32)
    f = (gram.astype(np.float64) @ (alpha.astype(np.float64) * y) - y).astype(np.float32)
    G, rpt = geometry(n)
    cand = W.candidates_model(f, alpha, y, FUP_C, G, rpt)
    st = dict(n=n, cand=cand, f=f, alpha=alpha, y=y)
    held = set(int(k) & 0xFFFFFFFF for k in cand[:, :, :KC1].ravel() if k != NONE)
    free = [r for r in range(n) if r not in held]
    n_chosen = W.merge1_model(cand, free[:1], q_max, n_new, 1e-3)["n_chosen"]
    prev = [int(r) for r in rng.permutation(free)[: q_want - n_chosen]]
    ref = W.merge1_model(cand, prev, q_max, n_new, 1e-3)
    assert ref["done"] == RUNNING and ref["q"] == q_want
    rec = K.ws_subgram_split(X, cand, prev, f, alpha, y, gamma, q_max, n_new, 1e-3)
    res = K.ws_gather(gram, cand, prev, f, alpha, y, q_max, n_new, 1e-3)
    idx = np.asarray(ref["idx"], dtype=np.int64)
    for got in (rec, res):
        check_merge(got, ref)
        check_set_state(got, st, gram[np.ix_(idx, idx)], q_max)
    assert np.isnan(rec["subg"][q_want:]).all() and np.all(res["subg"][q_want:] == 0)

    def solve(r):
        aux = np.where(np.arange(q_max) < q_want, r["aux"], 0.0).astype(np.float32)  # the probe takes q_max entries
        return K.ws_solve(r["subg"], aux[0], aux[1], aux[2], [q_want], q_max, FUP_C, clip=clip, eps=1e-3,
                          b_hi=r["b_hi"], b_lo=r["b_lo"])

    s_rec, s_res = solve(rec), solve(res)
    assert len(s_rec["apply_idx"]) > 2 and s_rec["steps"][0] > 0
    assert s_rec["apply_idx"] == s_res["apply_idx"] and s_rec["steps"] == s_res["steps"]
    assert np.array_equal(s_rec["apply_coef"].view(np.uint32), s_res["apply_coef"].view(np.uint32))
    assert np.array_equal(s_rec["alpha"][:q_want].view(np.uint32), s_res["alpha"][:q_want].view(np.uint32))
    rows = idx[np.asarray(s_rec["apply_idx"], dtype=np.int64)].astype(np.int32)
    coef = s_rec["apply_coef"]
    a_new = alpha.copy()
    a_new[idx] = s_rec["alpha"][:q_want]
    f_rec = K.ws_fupdate_split(X, f, a_new, y, rows, coef, gamma, FUP_C)
    f_res = K.ws_select(gram, f, a_new, y, np.zeros(n, np.float32), rows, coef, [len(rows)], FUP_C, q_max=q_max)
    assert (f_rec["G"], f_rec["rpt"]) == (f_res["G"], f_res["rpt"]) == (G, rpt)
    # both within the derived bound of the float64 update (hence within twice it of each other)
    want64, bound = f64_bound(f, gram[rows], k64_rows(X, rows, gamma), coef)
    for name, got in (("recompute", f_rec), ("resident", f_res)):
        ratio = float((np.abs(got["f"].astype(np.float64) - want64) / bound).max())
        print(f"one round ({clip}), {name}: {len(rows)} changed rows, max |f - f64| / bound = {ratio:.4f}")
        assert ratio <= 1.0
    np.testing.assert_array_equal(f_rec["f"], fupdate_model(f, gram[rows], coef))
    check_lists(f_rec["cand"], f_rec["f"], a_new, y, G, rpt)
    res_cand = np.asarray(f_res["cand"], dtype=np.uint64).reshape(G, 2, KC)[:, :, :KC1]
    np.testing.assert_array_equal(res_cand, W.candidates_model(f_res["f"], a_new, y, FUP_C, G, rpt, nc=KC1))
