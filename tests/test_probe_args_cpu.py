"""The kernel probes (kernel_entry.hip, ws_kernel_entry.hip) check their arguments before they touch the device:
a malformed call raises the check's own RuntimeError.  On a host without a GPU that proves the check ran before every
HIP call (the first of which would fail there with another message); on a GPU host the calls raise the same way."""
import numpy as np
import pytest

NONE = np.uint64((1 << 64) - 1)
KC = 16  # kWsCand


@pytest.fixture(scope="module")
def K():
    from dpsvm_amd.ops import kernels

    return kernels


def f32(*v):
    return np.asarray(v, np.float32)


def lists(C, G, rows=(0, 1)):
    """[G][2][KC] candidate lists: list 0 holds rows[0] (up) and rows[1] (low), the rest is empty"""
    c = np.full((G, 2, KC), NONE, np.uint64)
    c[0, 0, 0] = C.make_key(-1.0, rows[0])
    c[0, 1, 0] = C.make_key(-1.0, rows[1])
    return c


def state(n):
    return np.zeros(n, np.float32), np.zeros(n, np.float32), np.where(np.arange(n) % 2, -1, 1).astype(np.float32)


def test_ws_merge_multi(K, C):
    with pytest.raises(RuntimeError, match="2 <= blocks <= 128"):
        K.ws_merge_multi(lists(C, 1), 1, 4, 2, 1e-3)
    with pytest.raises(RuntimeError, match="G <= 256"):
        K.ws_merge_multi(lists(C, 257), 2, 4, 2, 1e-3)


def test_ws_solve(K):
    q = 4
    with pytest.raises(RuntimeError, match=r"qb\[p\] <= q_max"):
        K.ws_solve(np.eye(q), *state(q), [q + 1], q, 1.0)
    with pytest.raises(RuntimeError, match="blocks x q_max <= 6144"):  # 128 x 64 rows overrun the control record
        K.ws_solve(np.zeros((128, 64, 64), np.float32), *state(128 * 64), [2] * 128, 64, 1.0)
    with pytest.raises(RuntimeError, match="diag runs one block"):
        K.ws_solve(np.stack([np.eye(q)] * 2), *state(2 * q), [2, 2], q, 1.0, clip="box", diag=True)


def test_ws_solve_direct(K):
    n, q = 8, 4
    gram = np.zeros((n, n), np.float32)
    run = lambda idx, qb, q_max=q, g=gram: K.ws_solve_direct(g, *state(n), idx, qb, q_max, 1.0)  # noqa: E731
    with pytest.raises(RuntimeError, match="2 <= q_max <= 64"):
        run(np.zeros((1, 65), np.int32), [2], q_max=65)
    with pytest.raises(RuntimeError, match=r"qb\[p\] <= q_max"):
        run([[0, 1, 2, 3]], [q + 1])
    with pytest.raises(RuntimeError, match="row out of range"):  # a row the load reads
        run([[0, n, -1, -1]], [2])
    with pytest.raises(RuntimeError, match="row out of range"):  # -1 inside the block's q rows
        run([[0, -1, -1, -1]], [2])
    with pytest.raises(RuntimeError, match="listed twice"):
        run([[0, 1, -1, -1], [2, 1, -1, -1]], [2, 2])
    with pytest.raises(RuntimeError, match=r"idx \[P\]\[q_max\]"):
        run([[0, 1, 2]], [2])
    with pytest.raises(RuntimeError, match="blocks x q_max <= 6144"):
        run(np.zeros((128, 64), np.int32), [0] * 128, q_max=64)
    with pytest.raises(RuntimeError, match=r"gram \[n\]\[ldg >= n\]"):
        run([[0, 1, -1, -1]], [2], g=np.zeros((n, n - 1), np.float32))


def shard(K, stage, n=8, W=2, exchange="collectives", **kw):
    f, alpha, y = state(n)
    args = dict(blocks=1, q_max=4, gram=np.zeros((n, n), np.float32))
    args.update(kw)
    return K.ws_shard_round(stage, args.pop("gram"), f, alpha, y, W, exchange=exchange, **args)


def test_ws_shard_round(K, C):
    apply = dict(apply_idx=[1], apply_line=[1], apply_coef=[0.5], nab=[1])
    with pytest.raises(RuntimeError, match="1 <= world <= 32"):
        shard(K, "select", W=33, n=40, **apply)
    with pytest.raises(RuntimeError, match="at least one row each"):
        shard(K, "select", W=9, **apply)
    with pytest.raises(RuntimeError, match="apply line out of range"):
        shard(K, "select", **dict(apply, apply_line=[8]))
    with pytest.raises(RuntimeError, match="apply row out of range"):
        shard(K, "select", **dict(apply, apply_idx=[8]))
    with pytest.raises(RuntimeError, match="run one block"):
        shard(K, "select", blocks=2, **dict(apply, nab=[1, 0]))
    with pytest.raises(RuntimeError, match="run one block"):
        shard(K, "pass1", **apply)
    with pytest.raises(RuntimeError, match=r"nab\[p\] <= q_max"):
        shard(K, "pass1", blocks=2, nab=[5, 0], apply_idx=[0] * 5, apply_line=[0] * 5, apply_coef=[0.5] * 5)
    with pytest.raises(RuntimeError, match=r"part \[world p1G\]\[ks\]\[2\]"):
        shard(K, "pass2", blocks=2, part=np.zeros(3), dfs=np.zeros(8), **dict(apply, nab=[1, 0]))
    with pytest.raises(RuntimeError, match=r"dfs \[ks\]\[n\]"):
        shard(K, "pass2", blocks=2, part=np.zeros(4), dfs=np.zeros(7), **dict(apply, nab=[1, 0]))
    with pytest.raises(RuntimeError, match="ldg_extra a multiple of 4"):
        shard(K, "select", ldg_extra=2, **apply)
    with pytest.raises(RuntimeError, match=r"cand \[world G\]\[2\]"):
        shard(K, "gather", cand=lists(C, 1), prev_set=[])
    with pytest.raises(RuntimeError, match="candidate row out of range"):
        shard(K, "gather", cand=lists(C, 2, rows=(0, 8)), prev_set=[])
    sets = dict(idx=[[0, 1, -1, -1]], line=[[0, 1, -1, -1]], qb=[2], cache=1)
    with pytest.raises(RuntimeError, match="set row or line out of range"):
        shard(K, "gather_lines", **dict(sets, line=[[0, 8, -1, -1]]))
    with pytest.raises(RuntimeError, match="set row or line out of range"):
        shard(K, "gather_lines", **dict(sets, idx=[[0, -1, -1, -1]]))
    with pytest.raises(RuntimeError, match="listed twice"):
        shard(K, "gather_lines", **dict(sets, idx=[[1, 1, -1, -1]]))
    with pytest.raises(RuntimeError, match="GatherLines is the cache form"):
        shard(K, "gather_lines", **dict(sets, cache=0))
    with pytest.raises(RuntimeError, match="a dense gather reads"):
        shard(K, "gather_multi", blocks=2, gram=np.zeros((4, 8), np.float32), idx=np.zeros((2, 4)),
              line=np.zeros((2, 4)), qb=[0, 0])
    # the peer form never waits long: a poll bound above 0.1 s is refused, before any buffer is allocated
    for ticks in (0, 10**7 + 1):
        with pytest.raises(RuntimeError, match="xtimeout_ticks in"):
            shard(K, "select", exchange="peer", xtimeout_ticks=ticks, **apply)
    assert C.kWsProbeXTimeout == 10**7
    with pytest.raises(ValueError, match="unknown field"):
        shard(K, "select", q_maxx=4, **apply)


def test_ws_select(K):
    L, n = 4, 8
    gram = np.zeros((L, n), np.float32)
    f, alpha, y = state(n)
    with pytest.raises(RuntimeError, match="fold needs 2 fold state rows"):
        K.ws_select(gram, f[:6], alpha[:6], y[:6], alpha[:6], [0], [0.5], [1], 1.0, fold=4)
    with pytest.raises(RuntimeError, match="apply line out of range"):
        K.ws_select(gram, f, alpha, y, alpha, [L], [0.5], [1], 1.0)
    for done in (-1, 6):
        with pytest.raises(RuntimeError, match="done is a DoneCode"):
            K.ws_select(gram, f, alpha, y, alpha, [0], [0.5], [1], 1.0, done=done)


@pytest.mark.parametrize("probe", ["ws_gather", "ws_subgram_split"])
def test_one_block_merge_probes(K, C, probe):
    n = 8
    f, alpha, y = state(n)
    first = np.zeros((n, n), np.float32) if probe == "ws_gather" else np.zeros((n, 4), np.float32)
    extra = () if probe == "ws_gather" else (0.5,)  # gamma
    run = getattr(K, probe)
    with pytest.raises(RuntimeError, match="previous set longer than q_max"):
        run(first, lists(C, 1), [2, 3, 4], f, alpha, y, *extra, 2, 2, 1e-3)
    with pytest.raises(RuntimeError, match="candidate row out of range"):
        run(first, lists(C, 1, rows=(0, n)), [], f, alpha, y, *extra, 2, 2, 1e-3)


def cache(n, L, pairs=()):
    """slot_of [n] / key_of [L] with row r in line l for every (r, l)"""
    s, k = np.full(n, -1, np.int32), np.full(L, -1, np.int32)
    for r, ln in pairs:
        s[r], k[ln] = ln, r
    return s, k


def test_ws_merge_cache(K, C):
    n, L = 8, 520  # ws_cache_min_lines(2) = 516
    f, alpha, y = state(n)

    def run(L_=L, hand=0, maps=None, rows=(0, 1), prev=(), **kw):
        s, k = cache(n, L_, [(2, 7)]) if maps is None else maps
        return K.ws_merge_cache(lists(C, 1, rows=rows), list(prev), f, alpha, y, 2, 2, 1e-3, L_, hand, s, k, **kw)

    with pytest.raises(RuntimeError, match="L below ws_cache_min_lines"):
        run(L_=515)
    for hand in (-1, L):
        with pytest.raises(RuntimeError, match="the hand must be a line"):
            run(hand=hand)
    s, k = cache(n, L, [(2, 7)])
    with pytest.raises(RuntimeError, match="not inverses"):  # the line holds another row
        run(maps=(s, np.where(np.arange(L) == 7, 3, k).astype(np.int32)))
    with pytest.raises(RuntimeError, match="not inverses"):  # a line claims a row that has no line
        run(maps=(s, np.where(np.arange(L) == 9, 4, k).astype(np.int32)))
    with pytest.raises(RuntimeError, match="slot_of entry out of range"):
        run(maps=(np.where(np.arange(n) == 5, L, s).astype(np.int32), k))
    with pytest.raises(RuntimeError, match="key_of entry out of range"):
        run(maps=(s, np.where(np.arange(L) == 9, n, k).astype(np.int32)))
    with pytest.raises(RuntimeError, match="slot_of of n rows, key_of of L lines"):
        run(maps=(s[:-1], k))
    with pytest.raises(RuntimeError, match="candidate row out of range"):
        run(rows=(0, n))
    with pytest.raises(RuntimeError, match="previous set longer than q_max"):
        run(prev=(2, 3, 4))
    with pytest.raises(RuntimeError, match="done a DoneCode"):
        run(done=99)


def test_ws_merge_multi_cache(K, C):
    n, blocks, q_max = 64, 2, 4
    L = 2 * blocks * q_max + 8192

    def run(blocks_=blocks, q_=q_max, L_=L, rows=(0, 1), prev=(), maps=None):
        s, k = cache(n, L_, [(2, 7)]) if maps is None else maps
        return K.ws_merge_multi_cache(lists(C, 1, rows=rows), blocks_, q_, 2, 1e-3, L_, 0, s, k, prev_union=prev)

    with pytest.raises(RuntimeError, match="<= 4096 union rows and L >="):
        run(L_=L - 1)
    with pytest.raises(RuntimeError, match="<= 4096 union rows and L >="):
        run(blocks_=32, q_=192, L_=2 * 32 * 192 + 8192)
    with pytest.raises(RuntimeError, match="2 <= blocks <= 128"):
        run(blocks_=1)
    with pytest.raises(RuntimeError, match="candidate row out of range"):
        run(rows=(0, n))
    with pytest.raises(RuntimeError, match="distinct, below n"):
        run(prev=(3, n))
    with pytest.raises(RuntimeError, match="distinct, below n"):
        run(prev=(3, 5, 3))
    s, k = cache(n, L, [(2, 7)])
    with pytest.raises(RuntimeError, match="not inverses"):
        run(maps=(np.where(np.arange(n) == 4, 7, s).astype(np.int32), k))


def test_ws_pack_rows(K):
    X, xsq = np.zeros((100, 32), np.float32), np.zeros(300, np.float32)
    with pytest.raises(RuntimeError, match="miss row out of range"):
        K.ws_pack_rows(X, 50, xsq, [300], 1, 192)
    with pytest.raises(RuntimeError, match=r"the shard \[off, off \+ nl\) inside"):
        K.ws_pack_rows(X, 201, xsq, [1], 1, 192)
    with pytest.raises(RuntimeError, match="the shard"):  # dp no multiple of 16
        K.ws_pack_rows(np.zeros((100, 20), np.float32), 50, xsq, [1], 1, 192)
    with pytest.raises(RuntimeError, match="n_miss <= q_max"):
        K.ws_pack_rows(X, 50, xsq, list(range(10)), 10, 8)
    with pytest.raises(RuntimeError, match="n_miss <= q_max"):  # fewer rows listed than n_miss
        K.ws_pack_rows(X, 50, xsq, [1, 2], 3, 192)


def test_rbf_rows_miss(C):
    """device addresses: nothing may be read before the checks pass (the addresses here are null)"""
    def run(rows=(1, 2), out_lines=(0, 1), x_rows=1024, n=500, ld=16, off=0, nl=500, m_max=192, n_lines=4,
            out_ld=512, split=False):
        return C.k_rbf_rows_miss(0, 0, x_rows, n, ld, off, nl, np.asarray(rows, np.int32), m_max, 0.5, 0, n_lines,
                                 out_ld, np.asarray(out_lines, np.int32), 0, split)

    for split in (False, True):
        with pytest.raises(RuntimeError, match="row out of range"):
            run(rows=(1, 500), split=split)
        with pytest.raises(RuntimeError, match="lines must be distinct"):
            run(out_lines=(1, 1), split=split)
        with pytest.raises(RuntimeError, match="lines must be distinct"):
            run(out_lines=(1, 4), split=split)
        with pytest.raises(RuntimeError, match="m <= m_max <= 6144"):
            run(m_max=1, split=split)
        with pytest.raises(RuntimeError, match="m <= m_max <= 6144"):
            run(m_max=6145, split=split)
        with pytest.raises(RuntimeError, match="the shard"):
            run(off=400, nl=101, split=split)
        with pytest.raises(RuntimeError, match="whole column tiles"):
            run(x_rows=511, split=split)
        with pytest.raises(RuntimeError, match="whole column tiles"):  # off + round_up(nl, 256) rows are read
            run(x_rows=600, off=200, nl=300, split=split)
        with pytest.raises(RuntimeError, match="out_ld >= nl"):
            run(out_ld=499, split=split)
        with pytest.raises(RuntimeError, match="ld a multiple of 16"):
            run(ld=20, split=split)


def test_ws_fupdate_split(K):
    n = 200
    f, alpha, y = state(n)
    X = np.zeros((n, 4), np.float32)
    with pytest.raises(RuntimeError, match="<= 192 apply rows"):
        K.ws_fupdate_split(X, f, alpha, y, np.arange(193), np.zeros(193), 0.5, 1.0)
    with pytest.raises(RuntimeError, match="dp <= 64"):
        K.ws_fupdate_split(np.zeros((n, 65), np.float32), f, alpha, y, [1], [0.5], 0.5, 1.0)


def test_gram_rows_wsum(K):
    L, ldg = 4, 8
    gram = np.zeros((L, ldg), np.float32)
    with pytest.raises(RuntimeError, match="ldg >= n"):
        K.gram_rows_wsum(gram, ldg + 1, [1.0])
    with pytest.raises(RuntimeError, match="line out of range"):
        K.gram_rows_wsum(gram, ldg, [1.0], lines=[L])
    with pytest.raises(RuntimeError, match="identity lines need m <= L"):
        K.gram_rows_wsum(gram, ldg, np.ones(L + 1))


def test_gram_rows_dot(C):
    nt, n, k = 2, 8, 3
    with pytest.raises(RuntimeError, match=r"b \[k\]"):
        C.k_gram_rows_dot(np.zeros(nt * n, np.float32), nt, n, n, np.zeros(k * n, np.float32), n, k,
                          np.zeros(k + 1, np.float32))


def test_platt_probes(K):
    with pytest.raises(RuntimeError, match=r"platt_fit: dec and y \[m\]\[n\]"):
        K.platt_fit(np.zeros((2, 8)), np.ones((2, 9)))
    with pytest.raises(RuntimeError, match="slot < slots"):
        K.holdout_decision(np.zeros(8), np.ones(8), [0, 1], 0.0, np.zeros((2, 8)), slot=2)
    with pytest.raises(RuntimeError, match="A and B of k values"):
        K.proba_rows(np.zeros((4, 3)), np.zeros(2), np.zeros(3))
