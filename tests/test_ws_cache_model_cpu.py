"""The line-plan model of the kernel-row cache (ws_cache_model.line_plan) on its
own: the invariants every round must keep, on seeded random consistent states
chained over several rounds, and hand-worked cases pinned by literal values.
test_ws_cache_kernels_gpu.py holds ws_merge_kernel and the multi-block merge's
cache branch to this model."""
import numpy as np
import pytest

from ws_cache_model import WINDOW1, WINDOW_MULTI, check_maps, line_plan, place, random_cache


def check_round(members, before, after, hand, L, window):
    """what a round must keep, whatever the state"""
    slot0, key0 = before
    lines, miss_row, miss_line, hand2, slot1, key1 = after
    W = min(L, window)
    check_maps(slot1, key1)
    assert len(set(lines)) == len(lines) == len(members)  # no two members share a line
    assert all(0 <= ln < L for ln in lines)
    assert [int(slot1[r]) for r in members] == lines
    prior = {int(slot0[r]) for r in members if slot0[r] >= 0}
    assert not prior & set(miss_line)  # a member's line is never a victim
    hits = [r for r in members if slot0[r] >= 0]
    assert [int(slot1[r]) for r in hits] == [int(slot0[r]) for r in hits]  # a hit keeps its line
    assert miss_row == [r for r in members if slot0[r] < 0]
    offs = [(ln - hand) % L for ln in miss_line]
    assert offs == sorted(offs) and all(o < W for o in offs)  # victims in window order, inside the window
    evicted = {int(key0[ln]) for ln in miss_line if key0[ln] >= 0}
    changed = {int(r) for r in np.nonzero(slot0 != slot1)[0]}
    assert changed == evicted | set(miss_row)  # nothing else moves
    assert all(slot1[r] == -1 for r in evicted)
    assert hand2 == ((hand + offs[-1] + 1) % L if miss_row else hand)
    assert 0 <= hand2 < L


@pytest.mark.parametrize("seed", range(6))
def test_line_plan_keeps_its_invariants_on_random_chained_states(seed):
    rng = np.random.default_rng(500 + seed)
    n = 3072
    for trial in range(60):
        L = 896 if trial % 2 == 0 else int(rng.integers(896, 5000))
        slot_of, key_of = random_cache(rng, n, L, rng.choice([0.0, 0.3, 0.9, 1.0]))
        hand = int(rng.integers(0, L))
        members = []
        for _ in range(4):
            q = int(rng.integers(1, 193))
            keep = [r for r in members if rng.random() < 0.4][: q // 2]  # part of the last set stays
            kept = set(keep)
            fresh = [int(r) for r in rng.permutation(n)[: q + len(keep)] if int(r) not in kept][: q - len(keep)]
            members = fresh + keep
            out = line_plan(members, slot_of, key_of, hand, L, WINDOW1)
            check_round(members, (slot_of, key_of), out, hand, L, WINDOW1)
            hand, slot_of, key_of = out[3], out[4], out[5]


def test_line_plan_multi_window_random_states():
    rng = np.random.default_rng(9)
    n = 20000
    for trial in range(6):
        q = int(rng.integers(1000, 4097))
        L = 2 * 4096 + WINDOW_MULTI + int(rng.integers(0, 100))
        slot_of, key_of = random_cache(rng, n, L, 0.8)
        hand = int(rng.choice([0, L - 1, L - 8191, rng.integers(0, L)]))
        members = [int(r) for r in rng.choice(n, size=q, replace=False)]
        out = line_plan(members, slot_of, key_of, hand, L, WINDOW_MULTI)
        check_round(members, (slot_of, key_of), out, hand, L, WINDOW_MULTI)


def test_hand_worked_small_cases():
    e = -1
    # L = 8, window 4, hand 6: the window is lines 6, 7, 0, 1.  Rows 0 and 1 are cached at lines 6 and 0 (offsets 0
    # and 2: pinned), row 2 at line 3 (offset 5: outside the window), row 5 — no member — at line 7.
    slot_of = np.array([6, 0, 3, e, e, 7, e, e, e, e], np.int32)
    key_of = np.array([1, e, e, 2, e, e, 0, 5], np.int32)
    lines, mrow, mline, hand, s1, k1 = line_plan([0, 7, 1, 8, 2], slot_of, key_of, 6, 8, 4)
    assert lines == [6, 7, 0, 1, 3]
    assert mrow == [7, 8] and mline == [7, 1]  # the free offsets 1 and 3; row 5 is evicted from line 7
    assert hand == 2  # (6 + 3 + 1) mod 8
    assert s1.tolist() == [6, 0, 3, e, e, e, e, 7, 1, e]
    assert k1.tolist() == [1, 8, e, 2, e, e, 0, 7]
    # the inputs are not written
    assert slot_of.tolist() == [6, 0, 3, e, e, 7, e, e, e, e] and key_of.tolist() == [1, e, e, 2, e, e, 0, 5]
    # all hits: nothing moves
    lines, mrow, mline, hand, s2, k2 = line_plan([2, 0, 1], slot_of, key_of, 6, 8, 4)
    assert (lines, mrow, mline, hand) == ([3, 6, 0], [], [], 6)
    assert np.array_equal(s2, slot_of) and np.array_equal(k2, key_of)
    # fewer lines than the window: W = L = 6, so the line just behind the hand (offset 5) is pinned too
    slot_of = np.array([e, e, e, 4, e, e, e, e, e, e], np.int32)
    key_of = np.array([e, e, e, e, 3, e], np.int32)
    lines, mrow, mline, hand, _, _ = line_plan([3, 9], slot_of, key_of, 5, 6, 8)
    assert (lines, mrow, mline, hand) == ([4, 5], [9], [5], 0)
    # L = 8 > W = 4: a member just behind the hand (line 1, offset 7) is a hit outside the window and keeps its line
    slot_of = np.array([e, e, e, e, 1, e, e, e, e, e], np.int32)
    key_of = np.array([e, 4, e, e, e, e, e, e], np.int32)
    lines, mrow, mline, hand, _, _ = line_plan([4, 6], slot_of, key_of, 2, 8, 4)
    assert (lines, mrow, mline, hand) == ([1, 2], [6], [2], 3)
    # three misses, two free lines in the window
    with pytest.raises(ValueError):
        line_plan([0, 1, 2, 3, 4], np.array([0, 1, e, e, e], np.int32), np.array([0, 1, e, e, e, e, e, e], np.int32),
                  0, 8, 4)


def test_hand_worked_cases_at_the_one_block_window():
    """the named cases of test_ws_cache_kernels_gpu.py at L = 896, W = 512, by literal values"""
    n, L, W = 3072, 896, 512
    members = list(range(100, 292))  # 192 rows
    cold = (np.full(n, -1, np.int32), np.full(L, -1, np.int32))
    # cold cache: the first 192 window lines, the hand moves past them
    lines, mrow, mline, hand, _, _ = line_plan(members, *cold, 0, L, WINDOW1)
    assert lines == mline == list(range(192)) and mrow == members and hand == 192
    # the window wraps at the end of the lines
    lines, _, mline, hand, _, _ = line_plan(members, *cold, L - 2, L, WINDOW1)
    assert mline == [894, 895] + list(range(190)) and hand == 190
    lines, _, mline, hand, _, _ = line_plan(members[:1], *cold, L - 1, L, WINDOW1)
    assert mline == [895] and hand == 0
    # pins at the window's offsets 0, 1, W - 2, W - 1 (hand 700: lines 700, 701, 314, 315) and five misses
    hand0 = 700
    maps = place(n, L, hand0, {100: 0, 101: 1, 102: W - 2, 103: W - 1})
    assert [int(maps[0][r]) for r in (100, 101, 102, 103)] == [700, 701, 314, 315]
    lines, mrow, mline, hand, _, _ = line_plan(members[:9], *maps, hand0, L, WINDOW1)
    assert lines == [700, 701, 314, 315, 702, 703, 704, 705, 706] and hand == 707
    # 191 pinned lines in a run at the window start: the one victim is at offset 191
    maps = place(n, L, 5, {r: r - 100 for r in members[:191]})
    lines, mrow, mline, hand, _, _ = line_plan(members, *maps, 5, L, WINDOW1)
    assert mrow == [291] and mline == [196] and hand == 197
    # pins on the even slots 0, 2, .., 20 only: the victims are the odd ones; on the odd slots: the even ones
    maps = place(n, L, 0, {100 + k: 2 * k for k in range(11)})
    _, _, mline, hand, _, _ = line_plan(members[:16], *maps, 0, L, WINDOW1)
    assert mline == [1, 3, 5, 7, 9] and hand == 10
    maps = place(n, L, 0, {100 + k: 2 * k + 1 for k in range(11)})
    _, _, mline, hand, _, _ = line_plan(members[:16], *maps, 0, L, WINDOW1)
    assert mline == [0, 2, 4, 6, 8] and hand == 9
    # both slots of the pairs (3, 4, 5): victims 0 .. 5, then 12, 13
    maps = place(n, L, 0, {100 + k: 6 + k for k in range(6)})
    _, _, mline, hand, _, _ = line_plan(members[:14], *maps, 0, L, WINDOW1)
    assert mline == [0, 1, 2, 3, 4, 5, 12, 13] and hand == 14
    # every window line holds a non-member: each miss evicts exactly one row
    maps = place(n, L, 300, {}, occupied=range(W), avoid=members)
    _, mrow, mline, hand, s1, k1 = line_plan(members, *maps, 300, L, WINDOW1)
    assert mline == list(range(300, 492)) and hand == 492
    assert int((maps[0] >= 0).sum()) == 512 and int((s1 >= 0).sum()) == 512
    assert sorted(np.nonzero((maps[0] >= 0) & (s1 < 0))[0].tolist()) == sorted(int(maps[1][ln]) for ln in mline)
    # a member cached just behind the hand (offset L - 1) keeps its line
    maps = place(n, L, 40, {100: L - 1})
    lines, mrow, mline, hand, _, _ = line_plan(members[:3], *maps, 40, L, WINDOW1)
    assert lines == [39, 40, 41] and mrow == [101, 102] and hand == 42
