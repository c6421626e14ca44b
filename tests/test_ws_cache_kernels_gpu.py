"""Kernel-level tests of the cache-mode rounds (ws-cache), one or two launches
each on crafted state (dpsvm_amd.ops.kernels.ws_merge_cache /
ws_merge_multi_cache / ws_pack_rows / rbf_rows_miss):

  ws_merge_kernel    the one-block merge through its third instantiation (the
                     merge case table and stop codes of test_ws_kernels_gpu.py),
                     and the line plan against ws_cache_model.line_plan: the
                     whole state after the launch, by array equality;
  ws_gather_lines    the sub-Gram gathered from the planned lines, bit for bit
                     what ws_gather reads from a resident Gram;
  multi-block merge  the cache branch of ws_merge_multi_body: the same union as
                     without a cache, the line plan of the union, ws_gather_multi
                     on WsCtrl::line;
  ws_pack_rows       the misses' X rows of a shard;
  the miss-row GEMM  in the solver's calling shape (launch sized by m_max, the
                     device count m, a column shard): the lines bit-identical
                     to the Gram's rows through all three split kernels and the
                     f32 kernel, nothing written outside them.

The end-to-end ws-cache fits see only the cache states their trajectories
reach, and cannot say which kernel broke."""
import functools

import numpy as np
import pytest
import torch

import test_ws_kernels_gpu as W
import test_ws_recompute_kernels_gpu as R
import ws_cache_model as M
from test_ws_kernels_gpu import K  # noqa: F401  (the module fixture)
from test_ws_recompute_kernels_gpu import check_merge, check_set_state, noise_gram  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED = 0, 1
WIN1, WINM = M.WINDOW1, M.WINDOW_MULTI


@functools.lru_cache(maxsize=1)
def consts():
    from dpsvm_amd._native import load

    C = load()
    return C.kWsProbeMiss, C.kWsProbeRowsComputed, C.kWsProbeRowHits


def empty_cache(n, L):
    return np.full(n, -1, np.int32), np.full(L, -1, np.int32)


def merge_cache(K, st, q_max, n_new, prev, L, hand, maps, **kw):  # noqa: F811
    return K.ws_merge_cache(st["cand"], prev, st["f"], st["alpha"], st["y"], q_max, n_new, W.MERGE1_EPS, L, hand,
                            maps[0], maps[1], **kw)


def check_plan(got, members, maps, hand, L, window):
    """the whole cache state after the launch equals the model's"""
    lines, mrow, mline, hand2, s1, k1 = M.line_plan(members, maps[0], maps[1], hand, L, window)
    nm = len(mrow)
    assert got["n_miss"] == nm
    np.testing.assert_array_equal(got["miss_row"][:nm], mrow)
    np.testing.assert_array_equal(got["miss_line"][:nm], mline)
    assert np.all(got["miss_row"][nm:] == -1) and np.all(got["miss_line"][nm:] == -1)
    assert got["hand"] == hand2
    np.testing.assert_array_equal(got["slot_of"], s1)
    np.testing.assert_array_equal(got["key_of"], k1)
    assert got["rows_computed"] - consts()[1] == nm and got["row_hits"] - consts()[2] == len(members) - nm
    return lines, s1, k1


def check_untouched(got, maps, hand):
    """a round that stops (or finds the run ended) leaves the cache as it was uploaded"""
    miss0, rows0, hits0 = consts()
    assert got["hand"] == hand and got["n_miss"] == miss0
    assert got["rows_computed"] == rows0 and got["row_hits"] == hits0
    assert np.all(got["miss_row"] == -1) and np.all(got["miss_line"] == -1)
    np.testing.assert_array_equal(got["slot_of"], maps[0])
    np.testing.assert_array_equal(got["key_of"], maps[1])


def lines_of(noise, key_of, n, device="cuda"):
    """lines[l] = noise[key_of[l]][:n], NaN in every line that holds no row"""
    key_of = np.asarray(key_of)
    out = np.full((len(key_of), n), np.nan, np.float32)
    held = np.nonzero(key_of >= 0)[0]
    out[held] = noise[key_of[held], :n]
    return torch.from_numpy(out).to(device)


# ---------------------------------------------------------------- the merge through ws_merge_kernel
@pytest.mark.parametrize("name", sorted(W.MERGE1_CASES))
def test_ws_merge_cache_merge_matches_model_and_ws_gather(K, noise_gram, name):  # noqa: F811
    st, q_max, n_new, prev = W.merge1_case(name)
    ref = W.merge1_model(st["cand"], prev, q_max, n_new, W.MERGE1_EPS)
    n, L = st["n"], 896
    maps = empty_cache(n, L)
    dense = K.ws_gather(np.ascontiguousarray(noise_gram[:n, :n]), st["cand"], prev, st["f"], st["alpha"], st["y"],
                        q_max, n_new, W.MERGE1_EPS)
    for outer, hand in ((1, 0), (2, 700)):  # both round parities
        got = merge_cache(K, st, q_max, n_new, prev, L, hand, maps, outer=outer)
        check_merge(got, ref)
        for k in ("done", "q", "idx", "b_hi", "b_lo", "n_apply"):
            assert got[k] == dense[k], k
        assert np.isnan(got["subg"]).all() and np.isnan(got["aux"]).all()  # no lines: no gather
        lines, _, _ = check_plan(got, got["idx"], maps, hand, L, WIN1)
        assert got["line"] == lines == [(hand + k) % L for k in range(got["q"])]  # a cold cache: all misses


@pytest.mark.parametrize("name", sorted(W.merge1_stop_cases()))
def test_ws_merge_cache_stop_codes_leave_the_cache_alone(K, name):  # noqa: F811
    f, alpha, y, eps, it, max_iter, nonfinite, done = W.merge1_stop_cases()[name]
    cand = W.lists_from_state(f, alpha, y, W.MERGE1_C, 1)
    ref = W.merge1_model(cand, [], 2, 2, eps, iteration=it, max_iter=max_iter, nonfinite=nonfinite)
    assert ref["done"] == done
    L, hand = 896, 895
    maps = M.place(2, L, hand, {0: 3})  # row 0 cached inside the window
    lines = torch.zeros(L, 4, device="cuda")  # a gather that ran would leave zeros, not the NaN fill
    dense = K.ws_gather(np.array([[1.0, 0.25], [0.25, 1.0]], np.float32), cand, [], f, alpha, y, 2, 2, eps,
                        iteration=it, max_iter=max_iter, nonfinite=nonfinite)
    for outer in (1, 2):
        got = K.ws_merge_cache(cand, [], f, alpha, y, 2, 2, eps, L, hand, *maps, lines=lines, iteration=it,
                               max_iter=max_iter, nonfinite=nonfinite, outer=outer)
        check_merge(got, ref)
        for k in ("done", "q", "idx", "b_hi", "b_lo", "n_apply"):
            assert R.f32_same(got[k], dense[k]) if k in ("b_hi", "b_lo") else got[k] == dense[k], k
        if done != RUNNING:
            assert got["q"] == 0 and np.isnan(got["subg"]).all() and np.isnan(got["aux"]).all()
            check_untouched(got, maps, hand)
        else:
            check_plan(got, got["idx"], maps, hand, L, WIN1)
            assert not np.isnan(got["subg"]).any()


@pytest.mark.parametrize("outer", [1, 2])
def test_ws_merge_cache_run_already_ended_changes_nothing(K, outer):  # noqa: F811
    st, q_max, n_new, prev = W.merge1_case("g256-prev-overlap")
    n, L, hand = st["n"], 896, 100
    maps = M.random_cache(np.random.default_rng(3), n, L, 0.7)
    lines = torch.zeros(L, n, device="cuda")
    got = merge_cache(K, st, q_max, n_new, prev, L, hand, maps, lines=lines, outer=outer, done=CONVERGED)
    assert got["done"] == CONVERGED and got["n_apply"] == 0 and got["q"] == 0 and got["idx"] == []
    assert np.isnan(got["subg"]).all() and np.isnan(got["aux"]).all()
    check_untouched(got, maps, hand)


# ---------------------------------------------------------------- the one-block line plan
@functools.lru_cache(maxsize=4)
def plan_members(q_max):
    """(state, n_new, prev, the set the merge builds) at n = 3072: q = q_max members"""
    st, qm, n_new, prev = W.merge1_case({192: "g256-d0", 40: "g256-q40"}[q_max])
    ref = W.merge1_model(st["cand"], prev, qm, n_new, W.MERGE1_EPS)
    assert qm == q_max and st["n"] == 3072 and ref["done"] == RUNNING and ref["q"] == q_max
    return st, n_new, tuple(prev), tuple(ref["idx"])


def wrap_offsets(hand, L, W_):
    """window offsets of pins on both sides of the point where the window wraps past line L - 1 (none: 0, 3)"""
    w = L - hand  # offset of line 0
    return sorted({0, 3} | ({w - 2, w - 1, w, w + 1} & set(range(W_))))


def named_plan_state(name, mem, n, L, hand):
    """(maps, what the case promises) of a named one-block case; mem: the members in set order"""
    q, W_ = len(mem), min(L, WIN1)
    if name == "cold":
        return empty_cache(n, L), dict(n_miss=q)
    if name == "hits-outside":  # every member cached past the window; a third of the window holds other rows
        return M.place(n, L, hand, {r: W_ + k for k, r in enumerate(mem)}, occupied=range(0, W_, 3), avoid=mem), \
            dict(n_miss=0)
    if name == "hits-inside":
        return M.place(n, L, hand, {r: 2 * k + 1 for k, r in enumerate(mem)}, occupied=range(0, W_, 2), avoid=mem), \
            dict(n_miss=0)
    if name == "pins-edges":
        return M.place(n, L, hand, dict(zip(mem[:4], (0, 1, W_ - 2, W_ - 1)))), dict(n_miss=q - 4, first=2)
    if name == "pins-even":
        return M.place(n, L, hand, {r: 2 * k for k, r in enumerate(mem[: q // 2])}), dict(n_miss=q - q // 2, first=1)
    if name == "pins-odd":
        return M.place(n, L, hand, {r: 2 * k + 1 for k, r in enumerate(mem[: q // 2])}), \
            dict(n_miss=q - q // 2, first=0)
    if name == "pins-pairs":  # both slots of the thread pairs 1, 2, 3 and 7
        offs = [2, 3, 4, 5, 6, 7, 14, 15]
        return M.place(n, L, hand, dict(zip(mem[:8], offs))), dict(n_miss=q - 8, first=0)
    if name == "pinned-run":  # q - 1 pinned lines in a run at the window start: the one victim sits behind them
        return M.place(n, L, hand, {r: k for k, r in enumerate(mem[:-1])}), dict(n_miss=1, first=q - 1)
    if name == "window-full":  # every window line holds a row that is no member
        return M.place(n, L, hand, {}, occupied=range(W_), avoid=mem), dict(n_miss=q, first=0, evicted=q)
    if name == "behind-hand":  # cached at offset L - 1: a hit outside the window
        return M.place(n, L, hand, {mem[0]: L - 1}, occupied=range(0, W_, 5), avoid=mem), dict(n_miss=q - 1, first=0)
    if name == "wrap":  # pins on both sides of the wrap, members cached past the window, other rows in between
        offs = wrap_offsets(hand, L, W_)
        at = dict(zip(mem, offs))
        at.update({r: W_ + 7 * k for k, r in enumerate(mem[len(offs): len(offs) + 5])})
        return M.place(n, L, hand, at, occupied=range(1, W_, 4), avoid=mem), dict(n_miss=q - len(offs) - 5)
    raise KeyError(name)


PLAN_CASES = [(name, 896, 37) for name in ("cold", "hits-outside", "hits-inside", "pins-edges", "pins-even",
                                           "pins-odd", "pins-pairs", "pinned-run", "window-full", "behind-hand")]
PLAN_CASES += [("wrap", L, h) for L in (896,) for h in (0, 1, L - 512, L - 511, L - 2, L - 1)]
PLAN_CASES += [(name, L, h) for L in (1000, 4096) for name, h in (("wrap", L - 300), ("pins-edges", L - 1),
                                                                  ("window-full", L - 511), ("cold", 0))]


@pytest.mark.parametrize("q_max", [192, 40])
@pytest.mark.parametrize("name,L,hand", PLAN_CASES)
def test_ws_merge_cache_line_plan_matches_model(K, name, L, hand, q_max):  # noqa: F811
    st, n_new, prev, mem = plan_members(q_max)
    n = st["n"]
    maps, want = named_plan_state(name, mem, n, L, hand)
    M.check_maps(*maps)
    got = merge_cache(K, st, q_max, n_new, list(prev), L, hand, maps)
    assert got["done"] == RUNNING and tuple(got["idx"]) == mem
    lines, s1, _ = check_plan(got, mem, maps, hand, L, WIN1)
    assert got["line"] == lines and len(set(lines)) == len(lines)
    # the case is the one its name says
    assert got["n_miss"] == want["n_miss"]
    if want["n_miss"] == 0:
        assert got["hand"] == hand and got["row_hits"] - consts()[2] == len(mem)
    if "first" in want:
        assert got["miss_line"][0] == (hand + want["first"]) % L
    if "evicted" in want:  # exactly n_miss rows lost their line, and nothing else changed
        lost = np.nonzero((maps[0] >= 0) & (got["slot_of"] < 0))[0]
        assert len(lost) == want["evicted"] and int((maps[0] != got["slot_of"]).sum()) == 2 * want["evicted"]
    if name == "behind-hand":
        assert got["line"][0] == (hand - 1) % L


def fresh_state(seed):
    """n = 3072 rows, 256 lists, a new f / alpha / y per seed"""
    return W.merge1_state("chain", 3072, 256, W._normal, seed=seed)


@pytest.mark.parametrize("seed", range(8))
def test_ws_merge_cache_chained_rounds_match_model(K, noise_gram, seed):  # noqa: F811
    """six rounds from a random consistent cache, the maps and the hand a round returns fed into the next one, the
    previous set its set, fresh lists every round; the last round's sub-Gram gathered from the planned lines"""
    rng = np.random.default_rng(40 + seed)
    n = 3072
    L = int([896, 896, 1000, 4096, 897, 2000, 896, 1300][seed])
    q_max, n_new = (192, 144) if seed % 2 == 0 else (40, 30)
    maps = M.random_cache(rng, n, L, [0.0, 0.5, 1.0, 0.9][seed % 4])
    hand = int(rng.integers(0, L))
    prev, outer = [], 1
    for rnd in range(6):
        st = fresh_state(100 * seed + rnd)
        ref = W.merge1_model(st["cand"], prev, q_max, n_new, W.MERGE1_EPS)
        assert ref["done"] == RUNNING
        last = rnd == 5
        lines_dev = None
        if last:  # the lines as they stand once the misses' rows are computed: the model's map
            k1 = M.line_plan(ref["idx"], maps[0], maps[1], hand, L, WIN1)[5]
            lines_dev = lines_of(noise_gram, k1, n)
        got = merge_cache(K, st, q_max, n_new, prev, L, hand, maps, outer=outer, lines=lines_dev)
        check_merge(got, ref)
        check_plan(got, ref["idx"], maps, hand, L, WIN1)
        M.check_maps(got["slot_of"], got["key_of"])
        if last:
            idx = np.asarray(got["idx"], dtype=np.int64)
            check_set_state(got, st, noise_gram[np.ix_(idx, idx)], q_max)
        maps, hand, prev, outer = (got["slot_of"], got["key_of"]), got["hand"], got["idx"], outer + 1


# ---------------------------------------------------------------- ws_gather_lines
@pytest.mark.parametrize("name,L,hand", [("cold", 896, 37), ("wrap", 896, 895), ("wrap", 1000, 700),
                                         ("hits-outside", 896, 500)])
@pytest.mark.parametrize("q_max", [192, 40])
def test_ws_gather_lines_reads_the_planned_lines(K, noise_gram, name, L, hand, q_max):  # noqa: F811
    st, n_new, prev, mem = plan_members(q_max)
    n = st["n"]
    maps, _ = named_plan_state(name, mem, n, L, hand)
    k1 = M.line_plan(mem, maps[0], maps[1], hand, L, WIN1)[5]
    got = merge_cache(K, st, q_max, n_new, list(prev), L, hand, maps, lines=lines_of(noise_gram, k1, n))
    check_plan(got, mem, maps, hand, L, WIN1)
    gram = np.ascontiguousarray(noise_gram[:n, :n])
    dense = K.ws_gather(gram, st["cand"], list(prev), st["f"], st["alpha"], st["y"], q_max, n_new, W.MERGE1_EPS)
    idx = np.asarray(got["idx"], dtype=np.int64)
    check_set_state(got, st, gram[np.ix_(idx, idx)], q_max)
    q = got["q"]
    assert np.array_equal(got["subg"].view(np.uint32), dense["subg"].view(np.uint32))  # rows past q: zeros too
    assert np.array_equal(got["aux"][:, :q].view(np.uint32), dense["aux"][:, :q].view(np.uint32))


# ---------------------------------------------------------------- the multi-block line plan
def crafted_candidates_in(rng, G, n_rows, n):
    """W.crafted_candidates with the rows drawn below n (the cache maps cover n rows)"""
    rows = rng.choice(n, size=n_rows, replace=False)
    f = rng.normal(size=n_rows).astype(np.float32)
    f[: n_rows // 10] = f[0]
    kind = rng.integers(0, 3, size=n_rows)
    owner = rng.integers(0, G, size=n_rows)
    cand = np.full((G, 2, W.KC), W.NONE, dtype=np.uint64)
    for g in range(G):
        sel = np.nonzero(owner == g)[0]
        ups = np.sort(W.make_key(f[sel][kind[sel] != 2], rows[sel][kind[sel] != 2]))[: W.KC]
        lows = np.sort(W.make_key(-f[sel][kind[sel] != 1], rows[sel][kind[sel] != 1]))[: W.KC]
        cand[g, 0, : len(ups)] = ups
        cand[g, 1, : len(lows)] = lows
    return cand, rows


def multi_pins(mem, L):
    """row -> window offset: a run (1,024 lines from unions of 3,072 rows on), all eight slots of thread 5, slots
    8 t of threads 10-12, slots 8 t + 7 of threads 20-22, the window's first and last slot; then members cached past
    the window"""
    Q, W_ = len(mem), min(L, WINM)
    run = min(1024, Q // 3)
    offs = list(range(3000, 3000 + run)) + list(range(40, 48)) + [80, 88, 96, 167, 175, 183, 0, W_ - 1]
    offs = offs[: max(0, Q - 4)]  # small unions: keep some misses
    at = dict(zip(mem, offs))
    rest = mem[len(offs):]
    at.update({r: W_ + 3 * k for k, r in enumerate(rest[: min(len(rest) // 4, (L - W_) // 3)])})
    return at


# (blocks, q_max, p_act, n_new, previous rows, L above the minimum, hand, union size bracket)
MULTI_CASES = [
    (2, 96, 2, 96, 0, 0, "0", (1, 192)),
    (2, 96, 2, 60, 40, 37, "L-1", (1, 192)),
    (4, 96, 4, 48, 150, 37, "L-8191", (193, 384)),
    (32, 96, 8, 96, 100, 0, "L-1", (512, 1023)),
    (32, 96, 32, 30, 140, 37, "L-8191", (1025, 2047)),
    (32, 96, 32, 60, 100, 0, "0", (1025, 2047)),
    (32, 96, 32, 64, 60, 37, "L-1", (2049, 3071)),
    (32, 96, 32, 90, 150, 0, "L-8191", (2049, 3071)),
    (64, 48, 64, 15, 50, 0, "L-8191", (512, 1023)),
    (64, 48, 64, 47, 30, 37, "0", (2049, 3071)),
    (32, 128, 32, 127, 20, 0, "L-1", (3073, 4095)),
    (32, 128, 32, 100, 700, 37, "L-8191", (3073, 4095)),
]


def multi_inputs(blocks, q_max, n_prev, n, n_rows, seed):
    rng = np.random.default_rng(seed)
    cand, rows = crafted_candidates_in(rng, 256, n_rows, n)
    others = np.setdiff1d(np.arange(n), rows)
    prev = np.concatenate([rng.choice(rows, size=n_prev // 2, replace=False),
                           rng.choice(others, size=n_prev - n_prev // 2, replace=False)])
    return cand, [int(v) for v in rng.permutation(prev)]


def check_multi(K, got, plain, cand, blocks, q_max, maps, hand, L):  # noqa: F811
    for k in ("uidx", "idx", "qb", "b_hi", "b_lo", "done", "p_round"):  # the cache does not change the selection
        assert got[k] == plain[k], k
    mem = got["uidx"]
    lines, s1, k1 = check_plan(got, mem, maps, hand, L, WINM)
    M.check_maps(got["slot_of"], got["key_of"])
    line_of = dict(zip(mem, lines))
    want = np.asarray([line_of[r] if r >= 0 else -1 for r in got["idx"]], dtype=np.int32)
    np.testing.assert_array_equal(got["line"], want)  # at idx's [b][la] positions, -1 where idx is unused
    return mem, k1


@pytest.mark.parametrize("blocks,q_max,p_act,n_new,n_prev,extra,hand_at,bracket", MULTI_CASES)
def test_ws_merge_multi_cache_line_plan_matches_model(K, blocks, q_max, p_act, n_new, n_prev, extra,  # noqa: F811
                                                      hand_at, bracket):
    n = 20000
    L = 2 * blocks * q_max + WINM + extra
    hand = {"0": 0, "L-1": L - 1, "L-8191": L - 8191}[hand_at]
    cand, prev = multi_inputs(blocks, q_max, n_prev, n, 12000, 7 * blocks + q_max + n_new + n_prev)
    plain = K.ws_merge_multi(cand, blocks, q_max, n_new, 1e-3, prev, p_act=p_act)
    assert plain["done"] == RUNNING
    mem = plain["uidx"]
    Q = len(mem)
    assert bracket[0] <= Q <= bracket[1] and Q % 1024 != 0, Q
    rng = np.random.default_rng(Q)
    at = multi_pins(mem, L)
    maps = M.place(n, L, hand, at, occupied=rng.choice(WINM, size=WINM // 2, replace=False), avoid=mem)
    M.check_maps(*maps)
    assert 0 < len(at) < Q  # hits and misses
    got = K.ws_merge_multi_cache(cand, blocks, q_max, n_new, 1e-3, L, hand, maps[0], maps[1], prev_union=prev,
                                 p_act=p_act)
    check_multi(K, got, plain, cand, blocks, q_max, maps, hand, L)
    assert got["n_miss"] == Q - len(at)
    # a cold cache at the same hand: every union row takes the window's lines in order
    cold = empty_cache(n, L)
    got = K.ws_merge_multi_cache(cand, blocks, q_max, n_new, 1e-3, L, hand, cold[0], cold[1], prev_union=prev,
                                 p_act=p_act)
    check_multi(K, got, plain, cand, blocks, q_max, cold, hand, L)
    np.testing.assert_array_equal(got["miss_line"][:Q], (hand + np.arange(Q)) % L)
    assert got["hand"] == (hand + Q) % L


def test_ws_merge_multi_cache_stopped_round_leaves_the_cache_alone(K):  # noqa: F811
    n, blocks, q_max = 2000, 2, 96
    L, hand = 2 * blocks * q_max + WINM, 5
    cand, prev = multi_inputs(blocks, q_max, 20, n, 600, 1)
    maps = M.random_cache(np.random.default_rng(2), n, L, 0.2)
    got = K.ws_merge_multi_cache(cand, blocks, q_max, 96, 1e-3, L, hand, *maps, prev_union=prev, iteration=50,
                                 max_iter=50)
    assert got["done"] == 2 and got["uidx"] == []
    check_untouched(got, maps, hand)


@pytest.mark.parametrize("hand_at,n_new,n_prev", [("L-1", 96, 0), ("L-8191", 70, 40)])
def test_ws_gather_multi_reads_the_planned_lines(K, noise_gram, hand_at, n_new, n_prev):  # noqa: F811
    n, blocks, q_max = 1024, 2, 96
    L = 2 * blocks * q_max + WINM
    hand = {"L-1": L - 1, "L-8191": L - 8191}[hand_at]
    cand, prev = multi_inputs(blocks, q_max, n_prev, n, 600, 11 + n_prev)
    rng = np.random.default_rng(12)
    f, alpha = rng.normal(size=n).astype(np.float32), rng.uniform(0, 2, n).astype(np.float32)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(np.float32)
    plain = K.ws_merge_multi(cand, blocks, q_max, n_new, 1e-3, prev)
    mem = plain["uidx"]
    maps = M.place(n, L, hand, multi_pins(mem, L), occupied=range(0, 400, 3), avoid=mem)
    k1 = M.line_plan(mem, maps[0], maps[1], hand, L, WINM)[5]
    got = K.ws_merge_multi_cache(cand, blocks, q_max, n_new, 1e-3, L, hand, maps[0], maps[1], prev_union=prev,
                                 lines=lines_of(noise_gram, k1, n), f=f, alpha=alpha, y=y)
    check_multi(K, got, plain, cand, blocks, q_max, maps, hand, L)
    assert 0 < got["n_miss"] < len(mem)
    idx = np.asarray(got["idx"], dtype=np.int64).reshape(blocks, q_max)
    for p in range(blocks):
        q = int(got["qb"][p])
        rows = idx[p, :q]
        assert q > 0 and np.all(rows >= 0)
        sub = got["subg"][p]
        assert not np.isnan(sub).any()
        np.testing.assert_array_equal(sub[:q, :q], noise_gram[np.ix_(rows, rows)])
        assert np.all(sub[:q, q:].view(np.uint32) == 0) and np.all(sub[q:].view(np.uint32) == 0)
        for r, v in enumerate((f, alpha, y)):
            np.testing.assert_array_equal(got["aux"][r, p, :q], v[rows])


# ---------------------------------------------------------------- ws_pack_rows
@pytest.mark.parametrize("d", [20, 54, 784])
@pytest.mark.parametrize("n_miss", [0, 1, 5, 192])
def test_ws_pack_rows_packs_the_owned_rows(K, d, n_miss):  # noqa: F811
    """ws_pack_rows_kernel's comment: row i of the pack is X row miss_row[i] when this rank owns it, else zeros; rows
    past n_miss are zeroed; xsq is global, so the packed norm is the row's whoever owns it (0 past n_miss)"""
    n, off, nl, q_max = 900, 300, 479, 192
    dp = (d + 15) // 16 * 16
    rng = np.random.default_rng(d + n_miss)
    X = np.zeros((n, dp), np.float32)
    X[:, :d] = rng.normal(size=(n, d))
    X[off + 7] = -0.0  # an owned row of negative zeros keeps its sign bits
    xsq = rng.random(n).astype(np.float32) + 1.0  # its own values: a norm identifies its row
    # misses on both sides of the shard's ends, the first and the last owned row among them
    edge = [off, off + nl - 1, off - 1, off + nl, off + 7, 0, n - 1]
    miss = (edge + [int(r) for r in rng.permutation(n) if r not in edge])[:n_miss]
    stale = [int(r) for r in rng.integers(off, off + nl, size=40)]  # an earlier round's rows past n_miss
    got = K.ws_pack_rows(X[off:off + nl], off, xsq, miss + stale, n_miss, q_max)
    out, out_sq = got["out"], got["out_sq"]
    assert out.shape == (q_max, dp) and not np.isnan(out).any() and not np.isnan(out_sq).any()
    for i, r in enumerate(miss):
        own = off <= r < off + nl
        want = X[r] if own else np.zeros(dp, np.float32)
        assert np.array_equal(out[i].view(np.uint32), want.view(np.uint32)), (i, r)
        assert out_sq[i] == xsq[r]
    assert np.all(out[n_miss:].view(np.uint32) == 0) and np.all(out_sq[n_miss:].view(np.uint32) == 0)
    if n_miss >= 5:
        assert sum(off <= r < off + nl for r in miss) not in (0, n_miss)  # owned and foreign rows


# ---------------------------------------------------------------- the miss-row GEMM in the solver's calling shape
# (d, m, m_max, n, shard, split): every d, m, m_max kind, n, shard and split value at least once; every (k blocks,
# miss-count class) pair of the split kernels — k blocks 1 (d 16) and 2 (d 54, 64): the small-K kernel, whose wave
# layout goes by m <= 64, <= 128, more; 3 (d 80): the LDS-DMA kernels, persistent where m_max <= 192
ROWS_CASES = [
    (16, 0, 192, 777, False, True), (16, 1, 1, 1300, True, True), (16, 64, 3072, 777, True, True),
    (16, 65, 192, 1300, False, True), (16, 128, 128, 777, True, True), (16, 129, 3072, 1300, True, True),
    (16, 192, 192, 777, False, True), (16, 193, 193, 1300, True, True), (16, 400, 3072, 777, False, True),
    (54, 0, 3072, 1300, True, True), (64, 1, 192, 777, False, True), (54, 64, 64, 1300, True, True),
    (64, 65, 3072, 777, True, True), (54, 128, 192, 1300, False, True), (64, 129, 129, 777, True, True),
    (64, 193, 3072, 777, True, True), (80, 0, 192, 777, True, True), (80, 1, 3072, 1300, False, True),
    (80, 65, 65, 1300, True, True), (80, 128, 3072, 777, False, True), (80, 192, 192, 777, True, True),
    (80, 193, 3072, 1300, True, True), (80, 400, 400, 777, False, True),
    (16, 0, 192, 777, True, False), (54, 1, 3072, 1300, False, False), (64, 64, 192, 777, True, False),
    (80, 65, 65, 1300, True, False), (54, 193, 3072, 777, False, False), (80, 400, 400, 1300, True, False),
]


@functools.lru_cache(maxsize=None)
def rows_problem(n, d):
    X = R.subgram_x(n, d, n + d)  # rows of mixed scales, two of them equal
    return X, 0.5 / d


_GRAMS = {}


def gram_of(K, n, d, split):  # noqa: F811
    """the resident Gram of rows_problem(n, d), computed once and left unchanged"""
    if (n, d, split) not in _GRAMS:
        X, gamma = rows_problem(n, d)
        _GRAMS[n, d, split] = K.rbf_gram(torch.from_numpy(X).cuda(), None, gamma, split=split).cpu().numpy()
    return _GRAMS[n, d, split]


@pytest.mark.parametrize("d,m,m_max,n,shard,split", ROWS_CASES)
def test_rbf_rows_miss_bit_identical_to_the_gram_rows(K, d, m, m_max, n, shard, split):  # noqa: F811
    X, gamma = rows_problem(n, d)
    off, nl = (300, n - 421) if shard else (0, n)
    rng = np.random.default_rng(d + m + m_max + n)
    # rows inside and outside the shard, its first and last among them; the two equal rows 0 and 1
    first = [off, off + nl - 1, 0, 1, n - 1]
    pick = first + [int(r) for r in rng.permutation(n) if r not in first]
    rows = pick[:m]
    n_lines = m + 9
    out_lines = [int(v) for v in rng.permutation(n_lines)[:m]]  # scattered
    x = torch.from_numpy(X).cuda()
    out = K.rbf_rows_miss(x, rows, gamma, m_max=m_max, off=off, nl=nl, out_lines=out_lines, n_lines=n_lines,
                          split=split).cpu().numpy()
    ld = (nl + 127) // 128 * 128
    assert out.shape == (n_lines, ld)
    written = np.zeros(n_lines, bool)
    written[out_lines] = True
    assert np.isnan(out[~written]).all()  # m = 0: nothing at all
    # pad columns [nl, ld) of a written line keep the fill: the split kernels guard col < N (the small-K one diverts
    # the store), and the f32 kernel's epilogue stores under `orow >= 0 && col < N`
    assert np.isnan(out[:, nl:]).all()
    if m == 0:
        return
    gram = gram_of(K, n, d, split)
    want = gram[np.asarray(rows)][:, off:off + nl]
    got = out[np.asarray(out_lines)][:, :nl]
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    if split:  # against float64: the rule of test_split_gram_matches_float64_like_f32_kernel on these rows
        ref = R.k64_rows(X, np.asarray(rows), gamma)[:, off:off + nl]
        e32 = float(np.abs(gram_of(K, n, d, False)[np.asarray(rows)][:, off:off + nl] - ref).max())
        e16 = float(np.abs(got - ref).max())
        print(f"rbf_rows_miss d={d} m={m} m_max={m_max} n={n} shard={shard}: split error {e16:.3e}, f32 {e32:.3e}")
        assert e16 <= max(3 * e32, 2e-6), (e16, e32)


# ---------------------------------------------------------------- argument checks
def test_cache_probes_reject_malformed_calls(K):  # noqa: F811
    """a malformed call raises before anything is launched"""
    st, q_max, n_new, prev = W.merge1_case("g256-q40")
    n, L = st["n"], 896
    s0, k0 = empty_cache(n, L)

    def one(L_=L, hand=0, s=s0, k=k0, **kw):
        return K.ws_merge_cache(st["cand"], prev, st["f"], st["alpha"], st["y"], q_max, n_new, 1e-3, L_, hand, s, k,
                                **kw)

    with pytest.raises(RuntimeError):  # fewer lines than ws_cache_min_lines(40) = 592
        one(L_=591, k=k0[:591])
    with pytest.raises(RuntimeError):  # the hand is no line
        one(hand=L)
    with pytest.raises(RuntimeError):
        one(hand=-1)
    s, k = s0.copy(), k0.copy()
    s[5] = 9  # row 5 claims line 9, line 9 holds nothing
    with pytest.raises(RuntimeError):
        one(s=s)
    k[9] = 6  # ... or another row
    with pytest.raises(RuntimeError):
        one(s=s, k=k)
    k = k0.copy()
    k[3] = 5  # a line claims a row that has no line
    with pytest.raises(RuntimeError):
        one(k=k)
    s = s0.copy()
    s[5] = L  # a line past L
    with pytest.raises(RuntimeError):
        one(s=s)
    k = k0.copy()
    k[3] = n  # a row past n
    with pytest.raises(RuntimeError):
        one(k=k)
    with pytest.raises(RuntimeError):  # maps of other lengths
        one(s=s0[:-1])
    with pytest.raises(RuntimeError):
        one(k=k0[:-1])
    with pytest.raises(RuntimeError):  # lines narrower than n
        one(lines=torch.zeros(L, n - 1, device="cuda"))
    with pytest.raises(ValueError):  # lines of fewer than L rows
        one(lines=torch.zeros(L - 1, n, device="cuda"))
    with pytest.raises(RuntimeError):  # a DoneCode
        one(done=99)
    # the multi-block probe: what launch::ws_merge_multi refuses, and rows the maps do not cover
    nm, blocks, qm = 2000, 2, 96
    cand, prevm = multi_inputs(blocks, qm, 20, nm, 600, 3)
    Lm = 2 * blocks * qm + WINM
    sm, km = empty_cache(nm, Lm)

    def multi(blocks_=blocks, qm_=qm, L_=Lm, s=sm, k=km, cand_=cand, prev_=prevm, **kw):
        return K.ws_merge_multi_cache(cand_, blocks_, qm_, 96, 1e-3, L_, 0, s, k, prev_union=prev_, **kw)

    with pytest.raises(RuntimeError):  # one line short of ws_cache_multi_min_lines
        multi(L_=Lm - 1, k=km[:-1])
    with pytest.raises(RuntimeError):  # 6,144 union rows: more than the cache-mode merge's 4,096
        multi(blocks_=32, qm_=192, L_=2 * 32 * 192 + WINM, k=np.full(2 * 32 * 192 + WINM, -1, np.int32))
    with pytest.raises(RuntimeError):  # a previous-union row past n
        multi(prev_=prevm + [nm])
    with pytest.raises(RuntimeError):  # ... twice
        multi(prev_=prevm + prevm[:1])
    bad = cand.copy()
    bad[3, 1, 15] = W.make_key(np.float32(0.5), nm)[0]  # a candidate row past n, in the last slot of a list
    with pytest.raises(RuntimeError):
        multi(cand_=bad)
    with pytest.raises(RuntimeError):  # lines without f / alpha / y
        multi(lines=torch.zeros(Lm, nm, device="cuda"))
    # ws_pack_rows
    X = np.zeros((100, 32), np.float32)
    xsq = np.zeros(300, np.float32)
    with pytest.raises(RuntimeError):  # a miss row past n
        K.ws_pack_rows(X, 50, xsq, [300], 1, 192)
    with pytest.raises(RuntimeError):  # the shard past n
        K.ws_pack_rows(X, 201, xsq, [1], 1, 192)
    with pytest.raises(RuntimeError):  # more misses than rows in the pack
        K.ws_pack_rows(X, 50, xsq, list(range(10)), 10, 8)
    with pytest.raises(RuntimeError):  # fewer rows listed than n_miss
        K.ws_pack_rows(X, 50, xsq, [1, 2], 3, 192)
    with pytest.raises(RuntimeError):  # dp no multiple of 16
        K.ws_pack_rows(np.zeros((100, 20), np.float32), 50, xsq, [1], 1, 192)
    # rbf_rows_miss
    x = torch.zeros(500, 16, device="cuda")
    for split in (False, True):
        with pytest.raises(RuntimeError):  # a row past n
            K.rbf_rows_miss(x, [500], 0.1, split=split)
        with pytest.raises(RuntimeError):  # m_max below the count
            K.rbf_rows_miss(x, [1, 2, 3], 0.1, m_max=2, split=split)
        with pytest.raises(RuntimeError):  # the shard past n
            K.rbf_rows_miss(x, [1], 0.1, off=400, nl=101, split=split)
        with pytest.raises(RuntimeError):  # two rows into one line
            K.rbf_rows_miss(x, [1, 2], 0.1, out_lines=[0, 0], split=split)
        with pytest.raises(RuntimeError):  # a line past n_lines
            K.rbf_rows_miss(x, [1, 2], 0.1, out_lines=[0, -1], n_lines=2, split=split)
        with pytest.raises(RuntimeError):  # more rows than a round can miss
            K.rbf_rows_miss(x, [1], 0.1, m_max=6145, split=split)
