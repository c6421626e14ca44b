"""The sub-Gram load of the headline round (ws_solve_kernel with WsArgs::direct_sub, ws_solve.hip): each block
reads the upper triangle of its sub-Gram straight from the resident Gram, mirrors it in LDS, zero-fills the columns
past q, and takes f / alpha / y / C_i by global row.  One launch on crafted state (ops.kernels.ws_solve_direct)
against the gathered path (ws_solve on a sub-Gram picked in numpy: the same pair loop, so every difference is the
load's) and against the float32 pair-rule model.  A whole solve converges through a wrong sub-Gram entry, only
more slowly; these cannot."""
import numpy as np
import pytest
import torch

from test_ws_kernels_gpu import extremes, solve_model

pytestmark = pytest.mark.gpu

N, LDG = 700, 704  # ldg = n + 4: the padding columns hold NaN


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dpsvm_amd.ops import kernels

    return kernels


@pytest.fixture(scope="module")
def problem():
    """a bitwise-symmetric Gram [N][LDG] (NaN padding), and a state with alphas at 0, inside and at the bound"""
    rng = np.random.default_rng(11)
    X = rng.normal(size=(N, 6)).astype(np.float32)
    d2 = ((X[:, None, :].astype(np.float64) - X[None, :, :]) ** 2).sum(-1)
    g = np.exp(-0.7 * d2).astype(np.float32)
    np.fill_diagonal(g, 1.0)
    assert np.array_equal(g, g.T)
    gram = np.concatenate([g, np.full((N, LDG - N), np.nan, np.float32)], axis=1)
    C = 2.0
    y = np.where(rng.random(N) < 0.5, 1.0, -1.0).astype(np.float32)
    row_C = (C * rng.uniform(0.5, 1.5, N)).astype(np.float32)
    u = rng.random(N)
    frac = np.where(u < 0.3, 0.0, np.where(u < 0.45, 1.0, rng.random(N))).astype(np.float32)
    f = (g.astype(np.float64) @ (C * frac * y) - y + rng.normal(scale=0.3, size=N)).astype(np.float32)
    return dict(g=g, gram=gram, C=C, y=y, row_C=row_C, frac=frac, f=f)


def alphas(pb, rowc):
    """alpha = frac x the row's bound: exactly 0, exactly at the bound, or inside"""
    return (pb["frac"] * (pb["row_C"] if rowc else np.float32(pb["C"]))).astype(np.float32)


def layout(name, q_max, seed=0, descending=False):
    """(idx [P][q_max] with -1 past qb[p], qb): uneven blocks of distinct rows.  p2: q_max and 37 rows; p3: 2,
    q_max, 1; p128: a full block, 37 rows, then blocks of 0 .. 6 rows up to the union's capacity of 6,144 rows
    (kWsMaxAll: 128 blocks of 48 rows, 96 of 64; block 2 is empty: the merge leaves qb = 0 for a block past its NP
    pairs or past p_act, ws_merge_multi_body)"""
    qb = {"p2": [q_max, 37], "p3": [2, q_max, 1],
          "p128": [q_max, 37] + [(3 * k) % 7 for k in range(6144 // q_max - 2)]}[name]
    assert sum(qb) <= N and len(qb) * q_max <= 6144 and (name != "p128" or (qb[2] == 0 and len(qb) >= 96))
    rows = np.random.default_rng(100 + seed).permutation(N)
    idx = -np.ones((len(qb), q_max), np.int32)
    at = 0
    for p, q in enumerate(qb):
        r = np.sort(rows[at:at + q])
        idx[p, :q] = r[::-1] if descending else r
        at += q
    return idx, qb, rows[at:]  # the rows no block holds


def gathered(pb, idx, qb, q_max, rowc, a):
    """subg / aux of the gathered path, picked in numpy: block p's K[ra][col] = gram[idx[ra]][idx[col]]"""
    P = len(qb)
    Kall = np.zeros((P, q_max, q_max), np.float32)
    f, al, y = (np.zeros((P, q_max), np.float32) for _ in range(3))
    y[:] = 1.0
    rc = np.full((P, q_max), pb["C"], np.float32)
    for p, q in enumerate(qb):
        r = idx[p, :q]
        Kall[p, :q, :q] = pb["g"][np.ix_(r, r)]
        f[p, :q], al[p, :q], y[p, :q], rc[p, :q] = pb["f"][r], a[r], pb["y"][r], pb["row_C"][r]
    return Kall, f, al, y, (rc if rowc else None)


def poison_lds(K, qb, q_max):
    """A launch of the same grid that fills every block's LDS sub-Gram with NaN and takes no step: LDS keeps what
    the last workgroup on the CU left, and the gathered run of the same block leaves exactly the entries a missing
    mirror store would have to write — a dropped store then reads NaN, not the right value by inheritance."""
    P = len(qb)
    z = np.zeros(P * q_max, np.float32)
    r = K.ws_solve(np.full((P, q_max, q_max), np.nan, np.float32), z, z, z + 1, [q_max] * P, q_max, 1.0, inner_max=0)
    assert sum(r["steps"]) == 0


def solve_kw(pb, idx, qb, a, clip, wss, inner_max):
    r = np.concatenate([idx[p, :q] for p, q in enumerate(qb)])
    bh, bl = extremes(pb["f"][r], a[r], pb["y"][r], pb["C"])  # the round's global selection: over every block
    return dict(clip=clip, eps=1e-3, rel=0.3, eps_floor=3e-4, b_hi=bh, b_lo=bl, inner_max=inner_max, wss=wss)


def same_as_gathered(direct, ref, idx, qb, q_max, a):
    """alpha, steps, apply_idx, apply_coef, iter, done of the direct load against the gathered path's, bit for bit
    (the gathered probe numbers block p's row ra as p q_max + ra: mapped through idx)"""
    want = a.copy()
    for p, q in enumerate(qb):
        want[idx[p, :q]] = ref["alpha"][p * q_max:p * q_max + q]
    np.testing.assert_array_equal(direct["alpha"], want)
    assert direct["steps"] == ref["steps"] and direct["nab"] == ref["nab"]
    assert direct["apply_idx"] == [int(idx.reshape(-1)[i]) for i in ref["apply_idx"]]
    np.testing.assert_array_equal(direct["apply_coef"], ref["apply_coef"])
    assert (direct["iter"], direct["done"], direct["outer"]) == (ref["iter"], ref["done"], ref["outer"])


@pytest.mark.parametrize("rowc", [False, True], ids=["C", "rowC"])
@pytest.mark.parametrize("wss", [1, 2])
@pytest.mark.parametrize("clip", ["independent", "box"])
@pytest.mark.parametrize("name", ["p2", "p3", "p128"])
@pytest.mark.parametrize("q_max", [48, 64])
def test_direct_load_is_the_gathered_path_bit_for_bit(K, problem, q_max, name, clip, wss, rowc):
    """Case 1, and case 2 on the same blocks: the rows of every block in descending order and every entry below the
    block's diagonal BY POSITION — gram[idx[ra]][idx[col]], ra > col, which in descending order are the entries
    with the smaller row number first — replaced by NaN.  The kernel reads gram[idx[ra]][idx[col]] for ra <= col
    only and mirrors it, so the NaNs are never loaded and the result is that of the clean Gram: the rule goes by
    position in the block, not by row number, and it needs the Gram bitwise symmetric."""
    pb = problem
    a = alphas(pb, rowc)
    rc = pb["row_C"] if rowc else None
    for descending in (False, True):
        idx, qb, _ = layout(name, q_max, descending=descending)
        kw = solve_kw(pb, idx, qb, a, clip, wss, 4 * q_max)
        gk = gathered(pb, idx, qb, q_max, rowc, a)
        ref = K.ws_solve(*gk[:4], qb, q_max, pb["C"], row_C=gk[4], **kw)
        assert sum(ref["steps"]) > 0 and len(ref["apply_idx"]) > 0  # the blocks really step
        gram = pb["gram"]
        if descending:
            gram = gram.copy()
            for p, q in enumerate(qb):
                r = idx[p, :q]
                lower = np.tril_indices(q, -1)
                gram[r[lower[0]], r[lower[1]]] = np.nan
                assert q < 2 or np.any(r[lower[0]] < r[lower[1]])  # a row-number rule would read these
        poison_lds(K, qb, q_max)
        got = K.ws_solve_direct(gram, pb["f"], a, pb["y"], idx, qb, q_max, pb["C"], row_C=rc, **kw)
        same_as_gathered(got, ref, idx, qb, q_max, a)


@pytest.mark.parametrize("clip", ["independent", "box"])
@pytest.mark.parametrize("q_max", [48, 64])
def test_direct_load_matches_the_pair_rule_model(K, problem, q_max, clip):
    """Case 3: the first 1, 3 and 8 pair steps of every block against the float32 model on Gram entries picked in
    numpy, to the tolerances of test_ws_solve_matches_pair_rule_model (a step is ~1 ulp from IEEE division)."""
    pb = problem
    C, a = pb["C"], alphas(pb, False)
    idx, qb, _ = layout("p2", q_max, seed=3)
    for cap in (1, 3, 8):
        kw = solve_kw(pb, idx, qb, a, clip, 1, cap)
        eps_in = max(np.float32(kw["eps_floor"]),
                     np.float32(np.float32(kw["rel"] * np.float32(0.5)) * np.float32(kw["b_lo"] - kw["b_hi"])))
        poison_lds(K, qb, q_max)
        got = K.ws_solve_direct(pb["gram"], pb["f"], a, pb["y"], idx, qb, q_max, C, **kw)
        assert sum(got["steps"]) >= cap  # at least the block holding the global pair steps to the cap
        for p, q in enumerate(qb):
            r = idx[p, :q]
            ref_a, ref_steps, _ = solve_model(pb["g"][np.ix_(r, r)], pb["f"][r], a[r], pb["y"][r], C, clip == "box",
                                              eps_in, 1e-12, cap)
            assert got["steps"][p] == ref_steps
            np.testing.assert_allclose(got["alpha"][r], ref_a, rtol=2e-6, atol=2e-6 * C)


@pytest.mark.parametrize("q_max", [48, 64])
def test_direct_load_zero_fills_the_columns_past_q(K, problem, q_max):
    """Case 4: the positions q .. q_max - 1 of idx name rows in a strongly violating state (alpha 0, y +1,
    f = -100: the smallest f of I_up by far; and alpha C, y +1, f = +100 for I_low).  A load that took them in
    would pair them at once: they must not move, and the blocks' result is that of idx with -1 there."""
    pb = problem
    C, a, f, y = pb["C"], alphas(pb, False).copy(), pb["f"].copy(), pb["y"].copy()
    idx, qb, free = layout("p3", q_max, seed=5)
    at = 0
    planted = idx.copy()
    for p, q in enumerate(qb):
        planted[p, q:] = free[at:at + q_max - q]
        at += q_max - q
    extra = planted[idx < 0]
    assert len(extra) == sum(q_max - q for q in qb) > 0
    a[extra[::2]], y[extra[::2]], f[extra[::2]] = 0.0, 1.0, -100.0
    a[extra[1::2]], y[extra[1::2]], f[extra[1::2]] = C, 1.0, 100.0
    kw = solve_kw(dict(pb, f=f, y=y), idx, qb, a, "box", 1, 4 * q_max)
    clean = K.ws_solve_direct(pb["gram"], f, a, y, idx, qb, q_max, C, **kw)
    got = K.ws_solve_direct(pb["gram"], f, a, y, planted, qb, q_max, C, **kw)
    assert sum(got["steps"]) > 0
    np.testing.assert_array_equal(got["alpha"][extra], a[extra])
    np.testing.assert_array_equal(got["alpha"], clean["alpha"])
    assert got["steps"] == clean["steps"] and got["apply_idx"] == clean["apply_idx"]
    assert not set(got["apply_idx"]) & set(int(v) for v in extra)
