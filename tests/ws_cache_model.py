"""The line plan of the kernel-row cache (ws-cache rounds), written from the rule
in the comments above ws_merge_kernel and the cache branch of the multi-block
merge (kernels/ws_merge.hip), not from their scans:

  a member's row is cached (slot_of) or takes a victim line; victims come from
  the window of up to `window` lines after the CLOCK hand, skipping lines that
  hold a member (pinned while the round uses them); the evicted row loses its
  line; the hand moves past the last victim.

Its invariants and hand-worked cases: test_ws_cache_model_cpu.py; the kernels
against it: test_ws_cache_kernels_gpu.py."""
import numpy as np

WINDOW1 = 512      # the one-block merge's window (device_state.hpp kWsCacheWindow)
WINDOW_MULTI = 8192  # the multi-block merge's (kWsWindowMulti)


def check_maps(slot_of, key_of):
    """slot_of [n] and key_of [L] are mutual inverses (-1: none)"""
    slot_of, key_of = np.asarray(slot_of), np.asarray(key_of)
    rows = np.nonzero(slot_of >= 0)[0]
    lines = np.nonzero(key_of >= 0)[0]
    assert len(rows) == len(lines)
    assert np.array_equal(key_of[slot_of[rows]], rows) and np.array_equal(slot_of[key_of[lines]], lines)


def line_plan(members, slot_of, key_of, hand, L, window):
    """(lines, miss_row, miss_line, hand', slot_of', key_of') of one round whose
    set is `members` (distinct rows, in set order).  The window is the W =
    min(L, window) lines hand, hand + 1, ... (mod L); a cached member's line is
    pinned when its offset (line - hand) mod L is below W; the k-th miss in member
    order takes the k-th line of the window, in window order, that is not pinned;
    the row that line held loses its slot_of; hand' = (hand + offset of the last
    victim + 1) mod L, unchanged without a miss."""
    slot_of = np.array(slot_of, dtype=np.int32)
    key_of = np.array(key_of, dtype=np.int32)
    assert len(key_of) == L and 0 <= hand < L
    members = [int(r) for r in members]
    assert len(set(members)) == len(members)
    W = min(L, window)
    lines = [int(slot_of[r]) for r in members]
    pinned = {(ln - hand) % L for ln in lines if ln >= 0 and (ln - hand) % L < W}
    free = [o for o in range(W) if o not in pinned]
    miss_row = [r for r, ln in zip(members, lines) if ln < 0]
    if len(miss_row) > len(free):
        raise ValueError("the window holds fewer free lines than the round has misses")
    miss_line = [(hand + o) % L for o in free[: len(miss_row)]]
    for r, ln in zip(miss_row, miss_line):
        old = int(key_of[ln])
        if old >= 0:
            slot_of[old] = -1
        key_of[ln] = r
        slot_of[r] = ln
    lines = [int(slot_of[r]) for r in members]
    hand2 = (hand + free[len(miss_row) - 1] + 1) % L if miss_row else hand
    return lines, miss_row, miss_line, hand2, slot_of, key_of


def random_cache(rng, n, L, fill):
    """consistent maps with about fill * L lines holding random distinct rows"""
    slot_of = np.full(n, -1, np.int32)
    key_of = np.full(L, -1, np.int32)
    k = min(int(fill * L), n, L)
    lines = rng.choice(L, size=k, replace=False)
    rows = rng.choice(n, size=k, replace=False)
    key_of[lines] = rows
    slot_of[rows] = lines
    return slot_of, key_of


def place(n, L, hand, at, occupied=(), avoid=()):
    """maps with row r at window offset o (line (hand + o) mod L) for every (r, o)
    of the dict `at`, and rows that are neither keys of `at` nor in `avoid`
    (ascending from the top of the row range) in the lines at the offsets
    `occupied`"""
    slot_of = np.full(n, -1, np.int32)
    key_of = np.full(L, -1, np.int32)
    for r, o in at.items():
        ln = (hand + o) % L
        assert key_of[ln] < 0 and slot_of[r] < 0
        key_of[ln], slot_of[r] = r, ln
    taken = set(at) | {int(r) for r in avoid}
    spare = (r for r in range(n - 1, -1, -1) if r not in taken)
    for o in occupied:
        ln = (hand + o) % L
        if key_of[ln] < 0:
            r = next(spare)
            key_of[ln], slot_of[r] = r, ln
    return slot_of, key_of
