"""The models of tests/ws_shard_model.py against their own rules, without a GPU: a kernel test that agrees with
them (test_ws_shard_kernels_gpu.py) agrees with something that cannot be vacuous."""
import numpy as np
import pytest

import ws_shard_model as M
from test_ws_kernels_gpu import KC, KC1, NONE, candidates_model

SHAPES = [(3000, 3), (2050, 8), (1027, 2), (5, 2), (70000, 4)]


@pytest.mark.parametrize("n,W", SHAPES)
def test_shards_partition_the_rows_and_the_shapes_are_the_awkward_ones(n, W):
    sh = [M.shard_of(n, r, W) for r in range(W)]
    assert sh[0][0] == 0 and sh[-1][0] + sh[-1][1] == n
    assert all(a[0] + a[1] == b[0] for a, b in zip(sh, sh[1:]))
    assert max(m for _, m in sh) - min(m for _, m in sh) <= 1 and max(m for _, m in sh) == -(-n // W)
    G, rpt = M.geometry(n, W)
    assert G * W <= 1024 and G * rpt * 256 >= -(-n // W)


def test_the_gpu_shapes_cover_unequal_unaligned_shards():
    sh = [M.shard_of(n, r, W) for n, W in SHAPES[:4] for r in range(W)]
    assert any(m % 4 for _, m in sh) and any(o % 4 for o, _ in sh)
    assert any(m % 256 for _, m in sh) and all(m % 1024 for _, m in sh)
    assert len({M.shard_of(2050, r, 8)[1] for r in range(8)}) == 2  # 257 and 256 rows


@pytest.mark.parametrize("n,W", SHAPES[:4])
def test_owner_masks_partition_every_entry_and_every_f_once(n, W):
    rng = np.random.default_rng(n)
    q_max = min(48, n - 1)
    for q in (q_max, q_max // 2, 1, 0):
        idx = rng.permutation(n)[:q_max]
        sub = np.zeros((q_max, q_max), int)
        fm = np.zeros(q_max, int)
        for r in range(W):
            s, f = M.owner_mask(idx, q, q_max, *M.shard_of(n, r, W))
            sub += s
            fm += f
        live = np.arange(q_max) < q
        assert np.array_equal(sub, (live[:, None] & live[None, :]).astype(int))
        assert np.array_equal(fm, live.astype(int))


def test_gather_model_sums_to_the_picked_sub_gram():
    n, W, q_max, q = 101, 3, 12, 9
    rng = np.random.default_rng(1)
    gram = rng.uniform(0.1, 1.0, (n, n)).astype(np.float32)
    f, a, y = (rng.uniform(0.5, 1.5, n).astype(np.float32) for _ in range(3))
    idx = rng.permutation(n)[:q_max]
    sub = np.zeros((q_max, q_max), np.float32)
    aux0 = np.zeros(q_max, np.float32)
    for r in range(W):
        s, x = M.gather_model(gram, f, a, y, idx, q, q_max, *M.shard_of(n, r, W))
        sub += s
        aux0 += x[0]
        assert np.array_equal(x[1, :q], a[idx[:q]]) and np.array_equal(x[2, :q], y[idx[:q]])
    assert np.array_equal(sub[:q, :q], gram[np.ix_(idx[:q], idx[:q])]) and not sub[q:].any() and not sub[:, q:].any()
    assert np.array_equal(aux0[:q], f[idx[:q]]) and not aux0[q:].any()
    # cache lines: the row comes from its line, the columns stay global
    lines = gram[idx[::-1]]
    s, _ = M.gather_model(lines, f, a, y, idx, q, q_max, 0, n, lines=np.arange(q_max)[::-1])
    assert np.array_equal(s[:q, :q], gram[np.ix_(idx[:q], idx[:q])])


@pytest.mark.parametrize("n,W,nc", [(1024, 2, KC), (3072, 3, KC1), (2048, 8, 8)])
def test_rank_lists_concatenate_to_the_one_rank_lists_when_groups_coincide(n, W, nc):
    """shards of whole 256-row groups at rpt 1: the ranks' workgroups are the one-rank workgroups, in rank order"""
    rng = np.random.default_rng(n + W)
    f = rng.normal(size=n).astype(np.float32)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(np.float32)
    a = rng.choice(np.asarray([0.0, 0.7, 2.0], np.float32), size=n)
    G, rpt = M.geometry(n, W)
    assert rpt == 1 and G * 256 * W == n
    want = candidates_model(f, a, y, 2.0, n // 256, 1, nc=nc)
    got = M.all_candidates(f, a, y, 2.0, W, nc=nc)
    assert np.array_equal(got[:, :, :nc], want) and np.all(got[:, :, nc:] == NONE)
    rows = (got[got != NONE] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert rows.max() >= n - 256  # the keys carry global rows


def test_rank_lists_with_per_row_bounds_use_the_compare_form():
    a = np.asarray([0.0, 1.0, 1.0, 0.0, 0.5], np.float32)
    y = np.asarray([1, 1, -1, -1, 1], np.float32)
    up, lo = M.in_sets(a, y, np.asarray([1.0, 1.0, 1.0, 0.0, 1.0], np.float32))
    assert up.tolist() == [True, False, True, False, True] and lo.tolist() == [False, True, False, False, True]
    up1, lo1 = M.in_sets(a, y, 1.0)
    assert up1.tolist() == [True, False, True, False, True] and lo1.tolist() == [False, True, False, True, True]


def test_part_slots_partition_the_all_gathered_array():
    for W, p1G, ks in ((3, 1, 1), (8, 2, 3), (2, 69, 16)):
        s = np.concatenate([M.part_slots(r, p1G, ks) for r in range(W)])
        assert np.array_equal(s, np.arange(2 * W * p1G * ks))


def test_xtag_is_never_zero_and_has_period_65535():
    T = np.arange(1, 3 * 65535 + 2)
    tags = np.asarray([M.xtag(int(t)) for t in T], dtype=np.uint64)
    assert np.all(tags >> np.uint64(48) >= 1) and np.all(tags >> np.uint64(48) <= 65535)
    assert np.all(tags & np.uint64(M.M48) == 0)
    assert np.array_equal(tags[65535:], tags[:-65535])
    assert len(set(tags[:65535].tolist())) == 65535  # no shorter period
    assert np.all(tags[2:] != tags[:-2])  # T and T - 2 differ: the only older publication a slot can hold
    # the rounds the GPU tests run: (R + 1) % 65535 = 65534, 0 and 1
    assert [M.xtag(R + 1) >> 48 for R in (65533, 65534, 65535)] == [65535, 1, 2]


def test_put64_round_trips_and_leaves_the_tag_bits_to_the_tag():
    rng = np.random.default_rng(3)
    for v in [0, (1 << 64) - 1, 0xFFFF, 0x10000] + [int(x) for x in rng.integers(0, 1 << 63, 50)]:
        g0, g1 = M.put64(M.xtag(7), v)
        assert M.get64(g0, g1) == v and g0 >> 48 == g1 >> 48 == 8


@pytest.mark.parametrize("blocks,G_all,W,p1G,ks,q_max", [(1, 8, 2, 4, 1, 192), (4, 12, 3, 1, 3, 96), (128, 16, 8, 1, 1, 48)])
def test_exchange_slots_do_not_overlap_and_fill_the_region(blocks, G_all, W, p1G, ks, q_max):
    xcw, xpart, xsub, rows, words = M.xlayout(blocks, G_all, W, p1G, ks, q_max)
    nk = KC if blocks > 1 else KC1
    used = np.zeros(words, int)
    for par in (0, 1):
        for slot in range(G_all):
            for side in (0, 1):
                for r in range(nk):
                    at = M.xcand_at(par, slot, side, r, G_all, xcw)
                    used[at:at + 2] += 1
        if blocks > 1:
            for k in range(W * p1G * ks):
                at = M.xpart_at(par, k, xpart, W * p1G * ks)
                used[at:at + 4] += 1
        for row in range(rows):
            at = M.xrow_at(par, row, 0, xsub, rows, q_max)
            used[at:at + q_max + 1] += 1
    assert used.max() == 1 and used.min() == 1
