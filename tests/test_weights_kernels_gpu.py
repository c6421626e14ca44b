"""Kernel-level tests of the per-row-C instantiations of ws_solve / ws_select
(WsArgs::c_row): one launch each on crafted state through the extended probes,
against float32 numpy models of the same rule (the scalar models of
tests/test_ws_kernels_gpu.py with a bound per row and the compare-form sets)."""
import numpy as np
import pytest
import torch

import test_ws_kernels_gpu as base

pytestmark = pytest.mark.gpu

KC = base.KC
f32 = np.float32


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dpsvm_amd.ops import kernels

    return kernels


def up_w(a, y, Cr):
    return np.where(np.asarray(y) > 0, np.asarray(a) < Cr, np.asarray(a) > 0)


def low_w(a, y, Cr):
    return np.where(np.asarray(y) > 0, np.asarray(a) > 0, np.asarray(a) < Cr)


def pair_step_model_w(a_hi, a_lo, y_hi, y_lo, bh, bl, khl, C_hi, C_lo, tau, box, same):
    eta = f32(2.0) - f32(2.0) * f32(khl)
    eta = eta if eta >= f32(tau) else f32(tau)
    s = f32(y_lo * y_hi)
    a_lo_new = f32(a_lo + f32(f32(y_lo * f32(bh - bl)) / eta))
    if box and not same:
        if y_hi != y_lo:
            dl = f32(a_lo - a_hi)
            L, hL = (dl, f32(0)) if dl > 0 else (f32(0), f32(-1))
            H, hH = (f32(C_hi + dl), f32(C_hi)) if f32(C_hi + dl) < C_lo else (f32(C_lo), f32(-1))
        else:
            sm = f32(a_lo + a_hi)
            L, hL = (f32(sm - C_hi), f32(C_hi)) if f32(sm - C_hi) > 0 else (f32(0), f32(-1))
            H, hH = (sm, f32(0)) if sm < C_lo else (f32(C_lo), f32(-1))
        atL = a_lo_new <= L
        atH = (not atL) and a_lo_new >= H
        a_lo_new = L if atL else (H if atH else a_lo_new)
        snap = hL if atL else (hH if atH else f32(-1))
        a_hi_new = snap if snap >= 0 else f32(a_hi + f32(s * f32(a_lo - a_lo_new)))
        a_hi_new = f32(min(max(a_hi_new, 0), C_hi))
    else:
        a_hi_new = f32(a_hi + f32(s * f32(a_lo - a_lo_new)))
        a_lo_new = f32(min(max(a_lo_new, 0), C_lo))
        a_hi_new = f32(min(max(a_hi_new, 0), C_hi))
    return a_hi_new, a_lo_new, f32(f32(a_hi_new - a_hi) * y_hi), f32(f32(a_lo_new - a_lo) * y_lo)


def solve_model_w(Kq, f, a, y, Cr, box, eps_in, tau, cap):
    """the first-order ws_solve loop in float32 with per-row bounds; also the (hi, lo) pairs taken"""
    Kq = Kq.astype(np.float32)
    a = a.astype(np.float32).copy()
    fu = np.where(up_w(a, y, Cr), f, np.inf).astype(np.float32)
    fl = np.where(low_w(a, y, Cr), -f, np.inf).astype(np.float32)
    pairs = []
    while len(pairs) < cap:
        mu, ml = fu.min(), fl.min()
        bh, bl = mu, f32(-ml)
        if not (mu < np.inf and ml < np.inf and bl > f32(bh + f32(f32(2.0) * f32(eps_in)))):
            break
        ph, pl = int(np.argmin(fu)), int(np.argmin(fl))
        ahn, aln, c_hi, c_lo = pair_step_model_w(a[ph], a[pl], y[ph], y[pl], bh, bl, Kq[ph, pl], Cr[ph], Cr[pl], tau,
                                                 box, ph == pl)
        dl = (c_hi * Kq[ph, :]).astype(np.float32) + (c_lo * Kq[pl, :]).astype(np.float32)
        fu = (fu + dl).astype(np.float32)
        fl = (fl - dl).astype(np.float32)
        f_lo_new = f32(bl + f32(f32(c_hi * Kq[ph, pl]) + f32(c_lo * Kq[pl, pl])))
        f_hi_new = f32(bh + f32(f32(c_hi * Kq[ph, ph]) + f32(c_lo * Kq[pl, ph])))
        for pos, an, fp in ((pl, aln, f_lo_new), (ph, ahn, f_hi_new)):  # hi placed last
            fu[pos] = fp if up_w(an, y[pos], Cr[pos]) else np.inf
            fl[pos] = -fp if low_w(an, y[pos], Cr[pos]) else np.inf
        a[pl] = aln
        a[ph] = ahn
        pairs.append((ph, pl))
    return a, pairs


def weighted_blocks(rng, q=48):
    """two blocks of q rows with bounds from five values, alphas inside their own boxes; block 0 carries the
    crafted rows: 0 / 1 with C_i = 0 at alpha 0 and the most extreme f of either side, 2 (y +1, C 0.25) / 3
    (y -1, C 4) the most violating real pair, whose step reaches row 2's bound first"""
    blocks = []
    for _ in range(2):
        Kq, f, a, y = base.sub_problem(rng, q, 1.0)
        Cr = rng.choice([0.25, 0.5, 1.0, 2.0, 4.0], q).astype(np.float32)
        a = (a * Cr).astype(np.float32)  # 0 stays 0, C stays on the row's own bound
        blocks.append([Kq, f, a, y, Cr])
    Kq, f, a, y, Cr = blocks[0]
    y[0], a[0], Cr[0], f[0] = 1.0, 0.0, 0.0, -100.0   # in_up would make it b_hi
    y[1], a[1], Cr[1], f[1] = -1.0, 0.0, 0.0, 100.0   # in_low would make it b_lo
    y[2], a[2], Cr[2], f[2] = 1.0, 0.0, 0.25, -30.0
    y[3], a[3], Cr[3], f[3] = -1.0, 0.0, 4.0, 30.0
    return blocks


def run_blocks(K, blocks, clip, cap, row_c=True, wss=1, C=1.0):
    q = len(blocks[0][1])
    cat = lambda i: np.concatenate([b[i] for b in blocks])  # noqa: E731
    fa, aa, ya, ca = cat(1), cat(2), cat(3), cat(4)
    bh = f32(fa[up_w(aa, ya, ca)].min())
    bl = f32(fa[low_w(aa, ya, ca)].max())
    eps, rel = 1e-3, 1e-4  # the crafted rows open a gap of 60: a small rel keeps the sub-problem tolerance tight
    eps_floor = f32(3e-4)
    eps_in = max(eps_floor, f32(f32(rel * f32(0.5)) * f32(bl - bh)))
    got = K.ws_solve(np.stack([b[0] for b in blocks]), fa, aa, ya, [q] * len(blocks), q, C, clip=clip, eps=eps,
                     rel=rel, eps_floor=eps_floor, b_hi=bh, b_lo=bl, inner_max=cap, wss=wss,
                     row_C=ca if row_c else None)
    return got, eps_in


@pytest.mark.parametrize("clip", ["independent", "box"])
def test_ws_solve_rows_keep_their_own_bounds(K, clip):
    blocks = weighted_blocks(np.random.default_rng(5))
    q, box = 48, clip == "box"
    Kq, f, a, y, Cr = blocks[0]
    # step by step against the pair rule (a step is ~1 ulp from the model's IEEE division)
    for cap in (1, 2, 3, 5, 8):
        got, eps_in = run_blocks(K, blocks, clip, cap)
        for p, (Kp, fp, ap, yp, cp) in enumerate(blocks):
            ref_a, pairs = solve_model_w(Kp, fp, ap, yp, cp, box, eps_in, 1e-12, cap)
            assert got["steps"][p] == len(pairs)
            np.testing.assert_allclose(got["alpha"][p * q:(p + 1) * q], ref_a, rtol=2e-6, atol=2e-6)
            if p == 0:
                assert pairs[0] == (2, 3)  # the C_i = 0 rows 0 / 1 are in neither set: never chosen
                assert all(2 not in pr[:1] for pr in pairs[1:])  # row 2 sits on its bound: out of I_up
        an = got["alpha"][:q]
        assert an[0] == 0.0 and an[1] == 0.0 and 0 not in got["apply_idx"] and 1 not in got["apply_idx"]
        # row 2 stopped on its own bound 0.25 (its partner's is 4), exactly
        assert an[2] == f32(0.25)
        if cap == 1:
            assert an[3] == (f32(0.25) if box else f32(4.0))  # box: the line; independent: clipped on its own
    # a whole sub-problem: every row inside its own box, the zero rows untouched
    got, eps_in = run_blocks(K, blocks, clip, 4 * q)
    for p, (Kp, fp, ap, yp, cp) in enumerate(blocks):
        an = got["alpha"][p * q:(p + 1) * q]
        assert np.all((an >= 0) & (an <= cp))
        assert np.all(an[cp == 0] == 0)
        if box:
            assert abs(float(np.sum((an.astype(np.float64) - ap) * yp))) < 1e-4 * 4.0 * q
        fn = fp + Kp.astype(np.float64) @ ((an.astype(np.float64) - ap) * yp)
        if got["steps"][p] < 4 * q:  # the sub-problem's stop test on the float64 sub-gradient, per-row sets
            assert fn[low_w(an, yp, cp)].max() <= fn[up_w(an, yp, cp)].min() + 2 * eps_in + 1e-4


@pytest.mark.parametrize("wss", [1, 2])
@pytest.mark.parametrize("clip", ["independent", "box"])
@pytest.mark.parametrize("q,P", [(48, 2), (96, 2), (150, 1), (192, 1)])
def test_ws_solve_uniform_row_c_bit_equal_to_scalar(K, clip, wss, q, P):
    """C_i = C everywhere: the kRowC instantiations against the scalar ones, every load path's shape"""
    rng = np.random.default_rng(q + P)
    C = 2.0
    blocks = [list(base.sub_problem(rng, q, C)) + [np.full(q, C, np.float32)] for _ in range(P)]
    a, _ = run_blocks(K, blocks, clip, 4 * q, row_c=True, wss=wss, C=C)
    b, _ = run_blocks(K, blocks, clip, 4 * q, row_c=False, wss=wss, C=C)
    assert sum(a["steps"]) > 0
    for k in ("steps", "apply_idx", "nab", "iter", "outer", "done", "p_act", "p1_round"):
        assert a[k] == b[k], k
    np.testing.assert_array_equal(a["alpha"], b["alpha"])
    np.testing.assert_array_equal(a["apply_coef"], b["apply_coef"])


def candidates_model_w(f, a, y, Cr, G, rpt, nc):
    out = np.full((G, 2, nc), base.NONE, dtype=np.uint64)
    for b in range(G):
        j = np.arange(b * rpt * 256, min(len(f), (b + 1) * rpt * 256))
        if len(j) == 0:
            continue
        u, l_ = up_w(a[j], y[j], Cr[j]), low_w(a[j], y[j], Cr[j])
        ku, kl = np.sort(base.make_key(f[j][u], j[u]))[:nc], np.sort(base.make_key(-f[j][l_], j[l_]))[:nc]
        out[b, 0, :len(ku)] = ku
        out[b, 1, :len(kl)] = kl
    return out


def weighted_select_state(rng, n, C):
    """select_state with a bound per row; crafted rows (none of them changed this round): z, C_i = 0 at alpha 0
    with the smallest f; big, at the scalar C with y +1 and C_i = 2 C and the next smallest f"""
    gram, f, a_new, y, dal, ch = base.select_state(rng, n, C, 160)
    Cr = (C * rng.choice([1.0, 2.0, 4.0], n)).astype(np.float32)  # every alpha inside its own box
    free = np.setdiff1d(np.arange(n), ch)
    z, big = int(free[0]), int(free[1])
    y[z], a_new[z], Cr[z], f[z] = 1.0, 0.0, 0.0, -60.0
    y[big], a_new[big], Cr[big], f[big] = 1.0, f32(C), f32(2 * C), -50.0
    return gram, f, a_new, y, dal, ch, Cr, z, big


def test_ws_select_pass2_clips_to_own_bound_and_classifies_per_row(K):
    rng = np.random.default_rng(9)
    n, C, q_max, P = 3000, 1.0, 96, 4
    gram, f, a_new, y, dal, ch, Cr, z, big = weighted_select_state(rng, n, C)
    # two changed rows whose damped value leaves their own box (it stays inside the scalar one's widest, 4 C):
    # j_hi ends above its C_i = 0.5, j_lo below 0
    j_hi, j_lo = int(ch[0]), int(ch[1])
    a_new[j_hi], dal[j_hi], Cr[j_hi] = 0.2, -2.0, 0.5
    a_new[j_lo], dal[j_lo], Cr[j_lo] = 0.1, 2.0, 1.0
    c = dal.astype(np.float64) * y
    d_f = gram.astype(np.float64).T @ c
    q = float(np.sum(c[ch] * d_f[ch]))
    j0 = ch[2 + int(np.argmax(np.abs(c[ch[2:]])))]  # steer g'd = 0.5 d'Qd through one changed row's f
    rest = ch[ch != j0]
    f[j0] = f32((0.5 * q + float(np.sum(c[rest] * f[rest]))) / -c[j0])
    nab = [40] * P
    got = K.ws_select(gram, f, a_new, y, dal, ch, c[ch].astype(np.float32), nab, 4 * C, q_max=q_max, row_C=Cr)
    t = f32(got["t"])
    assert 0 < t < 0.9
    want = a_new.copy()
    want[ch] = np.clip(a_new[ch] - f32(f32(1.0) - t) * dal[ch], 0, Cr[ch]).astype(np.float32)
    np.testing.assert_allclose(got["alpha"], want, rtol=1e-6, atol=1e-7)
    assert got["alpha"][j_hi] == f32(0.5) and got["alpha"][j_lo] == 0.0
    assert np.all(got["alpha"] <= Cr)
    scalar = K.ws_select(gram, f, a_new, y, dal, ch, c[ch].astype(np.float32), nab, 4 * C, q_max=q_max)
    assert scalar["alpha"][j_hi] > 0.5  # the scalar kernel's bound is 4 C
    G, rpt = got["G"], got["rpt"]
    cand = np.asarray(got["cand"], dtype=np.uint64).reshape(G, 2, KC)
    np.testing.assert_array_equal(cand, candidates_model_w(got["f"], got["alpha"], y, Cr, G, rpt, KC))
    idx = cand & np.uint64(0xFFFFFFFF)
    listed = set(idx[cand != base.NONE].tolist())
    assert z not in listed  # C_i = 0: in neither list, whatever its f
    grp = big // (rpt * 256)
    assert int(idx[grp, 0, 0]) == big or int(idx[grp, 0, 1]) == big  # alpha = C < C_i: still in I_up
    sidx = np.asarray(scalar["cand"], dtype=np.uint64).reshape(G, 2, KC)[z // (rpt * 256), 0] & np.uint64(0xFFFFFFFF)
    assert z in sidx.tolist()  # the scalar classification lists the alpha = 0 row


def test_ws_select_one_pass_per_row_and_uniform_bit_equal(K):
    rng = np.random.default_rng(10)
    n, C = 3000, 1.0
    gram, f, a, y, dal, ch, Cr, z, big = weighted_select_state(rng, n, C)
    coef = rng.normal(scale=0.2, size=len(ch)).astype(np.float32)
    zero = np.zeros(n, np.float32)
    got = K.ws_select(gram, f, a, y, zero, ch, coef, [len(ch)], C, row_C=Cr)
    G, rpt = got["G"], got["rpt"]
    np.testing.assert_array_equal(got["alpha"], a)
    cand = np.asarray(got["cand"], dtype=np.uint64).reshape(G, 2, KC)[:, :, :base.KC1]
    np.testing.assert_array_equal(cand, candidates_model_w(got["f"], a, y, Cr, G, rpt, base.KC1))
    listed = set((cand & np.uint64(0xFFFFFFFF))[cand != base.NONE].tolist())
    assert z not in listed and big in listed
    # C_i = C everywhere (alphas inside [0, C]): the scalar kernel's outputs bit for bit, both modes
    a1 = np.minimum(a, f32(C))
    uni = np.full(n, C, np.float32)
    for nab, d in (([len(ch)], zero), ([40] * 4, dal)):
        q_max = 192 if len(nab) == 1 else 96
        x = K.ws_select(gram, f, a1, y, d, ch, coef, nab, C, q_max=q_max, row_C=uni)
        s = K.ws_select(gram, f, a1, y, d, ch, coef, nab, C, q_max=q_max)
        for k in ("f", "alpha", "dalpha"):
            np.testing.assert_array_equal(x[k], s[k])
        assert x["cand"] == s["cand"] and x["t"] == s["t"]
