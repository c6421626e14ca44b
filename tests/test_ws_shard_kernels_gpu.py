"""What a rank does differently when it owns a shard, one kernel at a time (ops.kernels.ws_shard_round: one stage of
a round launched once per rank on crafted state, every rank with its own control record, f shard, Gram panel and
copies of the global vectors).  The collectives form is checked against the one-rank kernels bit for bit and
against the models of ws_shard_model.py, the test doing in numpy what the communicator does (concatenate for the
all-gathers, add in rank order for the sum all-reduce); the peer form against what the collectives form produced.
The end-to-end multi-rank solves compare one exchange mode with the other: a defect both share passes them while
the solve converges.  Shapes: shards of unequal length, lengths that are no multiple of 4 / 256 / 1024, offsets
that are no multiple of 4."""
import functools

import numpy as np
import pytest
import torch

import ws_shard_model as M
from test_ws_kernels_gpu import KC, KC1, NONE, extremes

pytestmark = pytest.mark.gpu

SHAPES = [(3000, 3), (2050, 8), (1027, 2), (5, 2)]
PEER_SHAPES = [(1027, 2), (3000, 3), (2050, 8)]
OUTERS = [0, 1, 65533, 65534, 65535]  # (R + 1) % 65535 = 1, 2, 65534, 0, 1: the tag's wrap, both parities
C = 2.0
PROBE_KEY = np.uint64(0xABCDABCDFFFFFFFF)  # kWsProbeKey: what cand holds before a launch


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dpsvm_amd.ops import kernels

    return kernels


def peer_cases():
    """(n, W, outer): every round number on the small shapes, one of each parity on the largest"""
    return [(n, W, o) for n, W in PEER_SHAPES for o in (OUTERS if n != 3000 else [1, 65534])]


@functools.lru_cache(maxsize=None)
def state(n):
    """a bitwise-symmetric Gram with every entry > 0, f != 0 everywhere (in a gather "zero" means "not owned"),
    alphas at 0, inside and at C"""
    rng = np.random.default_rng(n)
    X = rng.normal(size=(n, 5))
    sq = (X ** 2).sum(1)
    d2 = sq[:, None] + sq[None, :] - 2 * X @ X.T
    gram = np.exp(-0.3 * np.maximum((d2 + d2.T) / 2, 0)).astype(np.float32)
    np.fill_diagonal(gram, 1.0)
    assert gram.min() > 0 and np.array_equal(gram, gram.T)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(np.float32)
    u = rng.random(n)
    alpha = np.where(u < 0.4, 0.0, np.where(u < 0.55, C, rng.uniform(0.2 * C, 0.8 * C, n))).astype(np.float32)
    f = rng.normal(size=n).astype(np.float32)
    f[f == 0] = 1.0
    row_C = (C * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    for v in (gram, y, alpha, f, row_C):
        v.setflags(write=False)
    return dict(n=n, gram=gram, y=y, alpha=alpha, f=f, row_C=row_C)


def pad4(gram):
    """the one-rank two-pass kernels load 16 bytes: columns padded to a multiple of 4 with NaN"""
    n = gram.shape[1]
    return np.concatenate([gram, np.full((gram.shape[0], (n + 3) // 4 * 4 - n), np.nan, np.float32)], axis=1)


def changes(st, W, P, owner=None, bound=None):
    """a round's alpha changes over P blocks (an empty segment among them): rows ch, alpha after them, d_alpha,
    coefficients d_alpha y, rows per block.  owner: None (anywhere), "last" (every changed row in the last rank's
    shard: rank 0 owns none) or "not0" (none in rank 0's).  bound: per-row bounds the new alphas respect."""
    n = st["n"]
    rng = np.random.default_rng(7 * n + P)
    nab = ([40, 0, 40, 2] if P == 4 else [150]) if n > 200 else ([1, 0, 1, 0] if P == 4 else [3])
    lo = {None: 0, "last": M.shard_of(n, W - 1, W)[0], "not0": M.shard_of(n, 1, W)[0]}[owner]
    ch = lo + rng.choice(n - lo, size=sum(nab), replace=False)
    cb = np.full(n, C, np.float32) if bound is None else bound
    a_old = st["alpha"].copy()
    a_old[ch] = (cb[ch] * rng.uniform(0.2, 0.8, len(ch))).astype(np.float32)
    a_new = a_old.copy()
    a_new[ch] = (a_old[ch] + cb[ch] * rng.uniform(0.05, 0.15, len(ch)) * rng.choice([-1, 1], len(ch))).astype(np.float32)
    a_new[ch[::4]] = cb[ch[::4]]  # steps that end on the bound
    dal = np.zeros(n, np.float32)
    dal[ch] = a_new[ch] - a_old[ch]
    assert np.all(dal[ch] != 0)
    return dict(ch=ch.astype(np.int32), a_new=a_new, dal=dal, coef=(dal[ch] * st["y"][ch]).astype(np.float32), nab=nab)


def apply_kw(cg):
    return dict(apply_idx=cg["ch"], apply_line=cg["ch"], apply_coef=cg["coef"], nab=cg["nab"])


def u64(x):
    return np.ascontiguousarray(x).view(np.uint64)


# ---------------------------------------------------------------- collectives form
@pytest.mark.parametrize("n,W", SHAPES)
def test_one_pass_select_of_a_shard(K, n, W):
    st = state(n)
    cg = changes(st, W, 1)
    one = K.ws_select(st["gram"], st["f"], st["alpha"], st["y"], np.zeros(n, np.float32), cg["ch"], cg["coef"],
                      cg["nab"], C)
    got = K.ws_shard_round("select", st["gram"], st["f"], st["alpha"], st["y"], W, blocks=1, q_max=192, C=C,
                           ldg_extra=4, **apply_kw(cg))
    assert (got["G"], got["rpt"]) == M.geometry(n, W)
    assert not np.array_equal(one["f"], st["f"])
    for r, k in enumerate(got["ranks"]):
        off, nl = M.shard_of(n, r, W)
        assert (k["off"], k["nl"], k["done"]) == (off, nl, 0) and k["ldg"] == (nl + 3) // 4 * 4 + 4
        np.testing.assert_array_equal(k["f"], one["f"][off:off + nl])
        np.testing.assert_array_equal(k["alpha"], st["alpha"])
        want = M.rank_candidates(k["f"], st["alpha"], st["y"], C, off, got["G"], got["rpt"], nc=KC1)
        np.testing.assert_array_equal(k["cand_out"][:, :, :KC1], want[:, :, :KC1])


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("n,W", SHAPES)
def test_pass1_of_a_shard(K, n, W, ks):
    st = state(n)
    cg = changes(st, W, 4)
    got = K.ws_shard_round("pass1", st["gram"], st["f"], cg["a_new"], st["y"], W, dalpha=cg["dal"], blocks=4,
                           q_max=96, p_round=4, p_act=4, ks=ks, C=C, ldg_extra=4, **apply_kw(cg))
    p1G = got["p1G"]
    assert p1G == M.pass1_groups(n, W)
    sentinel = u64(np.array([K.load().kWsProbePart]))[0]
    tq = tg = 0.0
    for r, k in enumerate(got["ranks"]):
        own = np.zeros(2 * W * p1G * ks, bool)
        own[M.part_slots(r, p1G, ks)] = True
        assert np.all(u64(k["part"])[~own] == sentinel)  # no other rank's slot touched
        assert np.all(np.isfinite(k["part"][own])) and np.all(u64(k["part"])[own] != sentinel)
        tq += k["part"][own][0::2].sum()
        tg += k["part"][own][1::2].sum()
    c = cg["dal"].astype(np.float64) * st["y"]
    d_f = st["gram"].astype(np.float64).T @ c
    ch = cg["ch"]
    assert tq == pytest.approx(float(np.sum(c[ch] * d_f[ch])), rel=1e-4)
    assert tg == pytest.approx(-float(np.sum(c[ch] * st["f"].astype(np.float64)[ch])), rel=1e-6, abs=1e-9)
    if ks == 1:
        one = K.ws_select(pad4(st["gram"]), st["f"], cg["a_new"], st["y"], cg["dal"], ch, cg["coef"], cg["nab"], C,
                          q_max=96)
        for k in got["ranks"]:
            np.testing.assert_array_equal(k["dfs"][0], one["dfs"][k["off"]:k["off"] + k["nl"]])


def steered(st, cg, target):
    """f with one changed row's value set so that g'd / d'Qd = target (test_ws_select_two_pass_line_search...)"""
    c = cg["dal"].astype(np.float64) * st["y"]
    ch = cg["ch"]
    d_f = st["gram"].astype(np.float64).T @ c
    q = float(np.sum(c[ch] * d_f[ch]))
    j0 = ch[int(np.argmax(np.abs(c[ch])))]
    rest = ch[ch != j0]
    f = st["f"].copy()
    f[j0] = np.float32((target * q + float(np.sum(c[rest] * f[rest].astype(np.float64)))) / -c[j0])
    return f


def pass2_round(K, n, W, target, owner, rowc, exchange="collectives", outer=1, ncand=0):
    """pass 1 on every rank, the all-gather of the partials and the shards' d_f in numpy, pass 2 on every rank; the
    one-rank kernels on the same state"""
    st = state(n)
    bound = st["row_C"] if rowc else None
    cg = changes(st, W, 4, owner, bound)
    f = steered(st, cg, target)
    kw = dict(dalpha=cg["dal"], blocks=4, q_max=96, p_round=4, p_act=4, C=C, ldg_extra=4, row_C=bound, outer=outer,
              **apply_kw(cg))
    p1 = K.ws_shard_round("pass1", st["gram"], f, cg["a_new"], st["y"], W, **kw)
    p1G = p1["p1G"]
    part = np.concatenate([k["part"][M.part_slots(r, p1G, 1)] for r, k in enumerate(p1["ranks"])])
    dfs = np.concatenate([k["dfs"][0] for k in p1["ranks"]])
    p2 = K.ws_shard_round("pass2", st["gram"], f, cg["a_new"], st["y"], W, exchange=exchange, part=part, dfs=dfs,
                          ncand=ncand, **kw)
    one = K.ws_select(pad4(st["gram"]), f, cg["a_new"], st["y"], cg["dal"], cg["ch"], cg["coef"], cg["nab"], C,
                      q_max=96, row_C=bound, outer=outer)
    return st, cg, p1, p2, one


@pytest.mark.parametrize("target,owner,rowc", [(0.5, None, False), (2.0, None, False), (0.5, "last", False),
                                               (0.5, "not0", False), (2.0, "last", False), (0.5, None, True)],
                         ids=["damped", "full", "damped-one-owner", "damped-rank0-owns-none", "full-one-owner",
                              "damped-rowC"])
@pytest.mark.parametrize("n,W", SHAPES)
def test_pass2_of_a_shard(K, n, W, target, owner, rowc):
    st, cg, _, p2, one = pass2_round(K, n, W, target, owner, rowc)
    if owner is not None:
        off1, _ = M.shard_of(n, 1, W)
        assert np.all(cg["ch"] >= off1)  # rank 0 owns no changed row: workgroup 0's loop fixes them all there
    t = p2["ranks"][0]["t"]
    if n > 200:
        assert (t < 1.0) == (target < 0.9) and t > 0
        if t < 1:
            assert not np.array_equal(one["alpha"], cg["a_new"])
    bound = st["row_C"] if rowc else C
    for k in p2["ranks"]:
        off, nl = k["off"], k["nl"]
        assert k["t"] == one["t"] == t  # the same bits on every rank
        np.testing.assert_array_equal(k["alpha"], one["alpha"])
        assert not np.any(k["dalpha"])
        np.testing.assert_array_equal(k["f"], one["f"][off:off + nl])
        assert (k["p_act"], k["n_damped"], k["done"]) == (one["p_act"], one["n_damped"], 0)
        want = M.rank_candidates(k["f"], k["alpha"], st["y"], bound, off, p2["G"], p2["rpt"])
        np.testing.assert_array_equal(k["cand_out"], want)


def crafted_set(st, P, q_max, seed=0):
    """P blocks of distinct rows, uneven (a full block, a partial one, an empty one when P >= 3)"""
    n = st["n"]
    rng = np.random.default_rng(50 + seed + n)
    qb = [q_max, max(1, q_max // 2 - 1), 0][:P] if n > 200 else [2, 2, 0][:P]
    rows = rng.permutation(n)[:sum(qb)]
    idx = -np.ones((P, q_max), np.int32)
    at = 0
    for p, q in enumerate(qb):
        idx[p, :q] = rows[at:at + q]
        at += q
    return idx, qb


def cache_lines(st, idx, qb, seed=0):
    """a kernel-row cache holding the set's rows at shuffled lines: (lines [L][n], line [P][q_max])"""
    rows = np.concatenate([idx[p, :q] for p, q in enumerate(qb)])
    L = len(rows) + 5
    at = np.random.default_rng(60 + seed).permutation(L)[:len(rows)]
    lines = np.full((L, st["n"]), 0.25, np.float32)  # a line that holds no member: a wrong line shows
    lines[at] = st["gram"][rows]
    line = -np.ones_like(idx)
    k = 0
    for p, q in enumerate(qb):
        line[p, :q] = at[k:k + q]
        k += q
    return lines, line


def check_gather(st, got, W, idx, qb, q_max, line=None, gram=None):
    """per rank the model's rows exactly (so: zero wherever the rank is not the owner), alpha / y rows the same on
    every rank, rows past q zero; returns the rank-order sum (the sum all-reduce) of subg and of the f row"""
    n, P = st["n"], len(qb)
    gram = st["gram"] if gram is None else gram
    sub = np.zeros((P, q_max, q_max), np.float32)
    fr = np.zeros((P, q_max), np.float32)
    for r, k in enumerate(got["ranks"]):
        off, nl = M.shard_of(n, r, W)
        for p, q in enumerate(qb):
            ws, wa = M.gather_model(gram, st["f"], st["alpha"], st["y"], idx[p], q, q_max, off, nl,
                                    None if line is None else line[p])
            m_sub, m_f = M.owner_mask(idx[p], q, q_max, off, nl)
            assert not np.any(k["subg"][p][~m_sub]) and not np.any(k["aux"][0, p, :q_max][~m_f])
            assert np.all(k["subg"][p][m_sub] != 0) and np.all(k["aux"][0, p, :q_max][m_f] != 0)
            np.testing.assert_array_equal(k["subg"][p], ws)
            np.testing.assert_array_equal(k["aux"][:, p, :q], wa[:, :q])
            assert not np.any(k["aux"][0, p, q:q_max])
        sub += k["subg"]
        fr += k["aux"][0, :, :q_max]
    return sub, fr


@pytest.mark.parametrize("n,W", SHAPES)
def test_gather_of_a_shard(K, n, W):
    """ws_gather_kernel: every rank merges the all-gathered lists to the same set, then fills what it owns"""
    st = state(n)
    q_max, n_new = (40, 30) if n > 200 else (4, 4)
    cand = M.all_candidates(st["f"], st["alpha"], st["y"], C, W, nc=KC1)
    prev = [int(v) for v in np.random.default_rng(n).permutation(n)[:q_max // 2]]
    one = K.ws_gather(st["gram"], cand, prev, st["f"], st["alpha"], st["y"], q_max, n_new, 1e-4)
    got = K.ws_shard_round("gather", st["gram"], st["f"], st["alpha"], st["y"], W, blocks=1, q_max=q_max, C=C,
                           cand=cand, prev_set=prev, n_new=n_new, eps=1e-4, ldg_extra=4)
    q = one["q"]
    assert one["done"] == 0 and 2 <= q <= q_max
    for k in got["ranks"]:
        assert (k["done"], k["q"], k["idx"]) == (0, q, one["idx"])
        assert (k["b_hi"], k["b_lo"]) == (one["b_hi"], one["b_lo"])
    idx = np.asarray(one["idx"] + [-1] * (q_max - q), np.int32)[None, :]
    sub, fr = check_gather(st, got, W, idx, [q], q_max)
    np.testing.assert_array_equal(sub[0], one["subg"])
    np.testing.assert_array_equal(fr[0], one["aux"][0, :q_max])
    np.testing.assert_array_equal(got["ranks"][W - 1]["aux"][1:, 0, :q_max], one["aux"][1:, :q_max])


@pytest.mark.parametrize("stage,cache", [("gather_multi", 0), ("gather_multi", 1), ("gather_lines", 1)])
@pytest.mark.parametrize("n,W", SHAPES)
def test_gather_of_a_crafted_set_of_a_shard(K, n, W, stage, cache):
    """ws_gather_multi_kernel (dense, and reading WsCtrl::line) and ws_gather_lines_kernel: the one-rank gather is
    the same probe at world 1"""
    st = state(n)
    P = 1 if stage == "gather_lines" else 3
    q_max = 24 if n > 200 else 2
    idx, qb = crafted_set(st, P, q_max)
    gram, line = cache_lines(st, idx, qb) if cache else (st["gram"], idx)
    kw = dict(blocks=P, q_max=q_max, C=C, idx=idx, line=line, qb=qb, cache=cache, ldg_extra=4, p_round=P, p_act=P)
    got = K.ws_shard_round(stage, gram, st["f"], st["alpha"], st["y"], W, **kw)
    one = K.ws_shard_round(stage, gram, st["f"], st["alpha"], st["y"], 1, **kw)["ranks"][0]
    sub, fr = check_gather(st, got, W, idx, qb, q_max, line if cache else None, gram)
    np.testing.assert_array_equal(sub, one["subg"])
    np.testing.assert_array_equal(fr, one["aux"][0, :, :q_max])
    for k in got["ranks"]:
        np.testing.assert_array_equal(k["aux"][1:, :, :q_max], one["aux"][1:, :, :q_max])
        assert k["done"] == 0


# ---------------------------------------------------------------- peer-exchange form
def check_collected(peer, coll, nk):
    """a.cand after ws_xcollect_cand on every rank: the ranks' lists concatenated in rank order, kKeyNone past nk"""
    want = np.concatenate([k["cand_out"] for k in coll["ranks"]])
    want[:, :, nk:] = NONE
    assert not np.any(want == PROBE_KEY) and np.any(want != NONE)
    for k in peer["ranks"]:
        np.testing.assert_array_equal(k["cand"], want)
        assert k["done"] == 0


@pytest.mark.parametrize("n,W,outer", peer_cases())
def test_peer_select_publishes_every_list_to_every_rank(K, n, W, outer):
    st = state(n)
    cg = changes(st, W, 1)
    kw = dict(blocks=1, q_max=192, C=C, outer=outer, **apply_kw(cg))
    args = ("select", st["gram"], st["f"], st["alpha"], st["y"], W)
    peer = K.ws_shard_round(*args, exchange="peer", **kw)
    assert peer["xch_words"] == M.xlayout(1, W * peer["G"], W, peer["p1G"], 1, 192)[4]
    check_collected(peer, K.ws_shard_round(*args, **kw), KC1)


@pytest.mark.parametrize("ncand", [0, 8])
@pytest.mark.parametrize("n,W,outer", peer_cases())
def test_peer_pass1_and_pass2_publish_partials_and_lists(K, n, W, outer, ncand):
    st = state(n)
    cg = changes(st, W, 4)
    kw = dict(dalpha=cg["dal"], blocks=4, q_max=96, p_round=4, p_act=4, C=C, outer=outer, **apply_kw(cg))
    args = ("pass1", st["gram"], st["f"], cg["a_new"], st["y"], W)
    if ncand == 0:  # the partials do not depend on ncand
        coll, peer = K.ws_shard_round(*args, **kw), K.ws_shard_round(*args, exchange="peer", **kw)
        p1G = coll["p1G"]
        assert peer["xch_words"] == M.xlayout(4, W * peer["G"], W, p1G, 1, 96)[4]
        part = np.concatenate([k["part"][M.part_slots(r, p1G, 1)] for r, k in enumerate(coll["ranks"])])
        for k in peer["ranks"]:
            np.testing.assert_array_equal(u64(k["part"]), u64(part))
            assert k["done"] == 0
    _, _, _, p2, _ = pass2_round(K, n, W, 0.5, None, False, outer=outer, ncand=ncand)
    _, _, _, p2x, _ = pass2_round(K, n, W, 0.5, None, False, exchange="peer", outer=outer, ncand=ncand)
    check_collected(p2x, p2, 8 if ncand == 8 else KC)
    for a, b in zip(p2x["ranks"], p2["ranks"]):  # the exchange changes nothing else
        np.testing.assert_array_equal(a["f"], b["f"])
        np.testing.assert_array_equal(a["alpha"], b["alpha"])


def check_peer_solve(K, st, peer, coll, idx, qb, q_max, outer, skw):
    """ws_solve on the pushed rows, on every rank, against ws_solve on the summed subg / aux of the collectives form"""
    P = len(qb)
    sub = sum(k["subg"] for k in coll["ranks"])
    fr = sum(k["aux"][0, :, :q_max] for k in coll["ranks"])
    aux = coll["ranks"][0]["aux"]
    ref = K.ws_solve(sub, fr, aux[1, :, :q_max], aux[2, :, :q_max], qb, q_max, C, **skw)
    assert sum(ref["steps"]) > 0 and ref["done"] == 0
    want = st["alpha"].copy()
    flat = idx.reshape(-1)
    for p, q in enumerate(qb):
        want[idx[p, :q]] = ref["alpha"][p * q_max:p * q_max + q]
    for k in peer["ranks"]:
        np.testing.assert_array_equal(k["alpha"], want)
        assert k["steps"] == ref["steps"] and k["nab"] == ref["nab"]
        assert k["apply_idx"] == [int(flat[i]) for i in ref["apply_idx"]]
        np.testing.assert_array_equal(k["apply_coef"], ref["apply_coef"])
        assert (k["iter"], k["done"], k["outer"]) == (ref["iter"], 0, outer + 1)


@pytest.mark.parametrize("stage,cache", [("gather", 0), ("gather_multi", 0), ("gather_multi", 1), ("gather_lines", 1)])
@pytest.mark.parametrize("n,W,outer", peer_cases())
def test_peer_gather_pushes_the_rows_ws_solve_reads(K, n, W, outer, stage, cache):
    st = state(n)
    # (the merge's eps and the solve's are one field of the arguments)
    skw = dict(clip="box", eps=1e-4 if stage == "gather" else 1e-3, rel=0.3, eps_floor=3e-4, inner_max=64)
    args = lambda g: (stage, g, st["f"], st["alpha"], st["y"], W)  # noqa: E731
    if stage == "gather":
        q_max = 40
        cand = M.all_candidates(st["f"], st["alpha"], st["y"], C, W, nc=KC1)
        prev = [int(v) for v in np.random.default_rng(n).permutation(n)[:q_max // 2]]
        kw = dict(blocks=1, q_max=q_max, C=C, cand=cand, prev_set=prev, n_new=30, outer=outer, **skw)
        coll = K.ws_shard_round(*args(st["gram"]), **kw)
        r0 = coll["ranks"][0]
        q = r0["q"]
        idx, qb = np.asarray(r0["idx"] + [-1] * (q_max - q), np.int32)[None, :], [q]
        skw.update(b_hi=r0["b_hi"], b_lo=r0["b_lo"])  # the merge's own selection: what the solve finds in the record
        peer = K.ws_shard_round(*args(st["gram"]), exchange="peer", **kw)
    else:
        P = 1 if stage == "gather_lines" else 3
        q_max = 24
        idx, qb = crafted_set(st, P, q_max, seed=1)
        gram, line = cache_lines(st, idx, qb) if cache else (st["gram"], idx)
        rows = np.concatenate([idx[p, :q] for p, q in enumerate(qb)])
        bh, bl = extremes(st["f"][rows], st["alpha"][rows], st["y"][rows], C)
        skw.update(b_hi=bh, b_lo=bl)
        kw = dict(blocks=P, q_max=q_max, C=C, idx=idx, line=line, qb=qb, cache=cache, p_round=P, p_act=P, outer=outer,
                  **skw)
        coll = K.ws_shard_round(*args(gram), **kw)
        peer = K.ws_shard_round(*args(gram), exchange="peer", **kw)
    check_peer_solve(K, st, peer, coll, idx, qb, q_max, outer, skw)
