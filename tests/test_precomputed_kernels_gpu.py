"""Kernel-level tests of the precomputed-kernel path: the general-diagonal sub-problem kernels (ws_solve's kDiag
instantiations: eta = K(hi,hi) + K(lo,lo) - 2 K(hi,lo) from the sub-Gram's own diagonal) and gram_rows_dot
(gram_dot.hip: decisions from a rectangular Gram, accumulated in fp64).

1. On a sub-Gram whose diagonal is exactly 1.0f the kDiag kernels return the bits of the RBF kernels: the operands
   of eta keep their order, (khh + kll) - 2 khl against (1 + 1) - 2 khl.
2. On D K D they follow the pair-rule model below (pair_step_model / solve_model of tests/test_ws_kernels_gpu.py,
   copied, with the general eta), the tau floor included: a duplicated row scaled alike has eta = 0 exactly.
3. gram_rows_dot against numpy float64: half an ulp of float32 plus the float64 accumulation's bound, the padding
   of Kt / coef never read (NaN there), nothing written outside out, two runs bit-equal.
"""
import numpy as np
import pytest
import torch

from test_ws_kernels_gpu import extremes, in_low, in_up, padded_block, sub_problem

pytestmark = pytest.mark.gpu

SHAPES = [(40, 40), (100, 128), (150, 192), (192, 192)]  # (q, q_max): NS 1, 2, 3 and kFull


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dpsvm_amd.ops import kernels

    return kernels


def tolerances(f, a, y, C, eps=1e-3, rel=0.3):
    bh, bl = extremes(f, a, y, C)
    eps_floor = np.float32(rel * eps)
    eps_in = max(eps_floor, np.float32(np.float32(rel * np.float32(0.5)) * np.float32(bl - bh)))
    return bh, bl, eps_floor, eps_in


# ---------------------------------------------------------------- 1. unit diagonal: bit equality
@pytest.mark.parametrize("rowc", [False, True])
@pytest.mark.parametrize("wss", [1, 2])
@pytest.mark.parametrize("q,q_max", SHAPES)
def test_ws_solve_diag_unit_diagonal_is_bit_equal(K, q, q_max, wss, rowc):
    rng = np.random.default_rng(q * 5 + q_max + wss)
    C = 2.0
    Kq, f, a, y = sub_problem(rng, q, C, gamma=0.7 if wss == 1 else 0.05)
    assert np.all(np.diagonal(Kq) == np.float32(1.0))
    row_C = None
    if rowc:  # bounds per row at or above the rows' alphas
        rc = np.maximum(a, rng.uniform(0.5, C, size=q).astype(np.float32)).astype(np.float32)
        row_C = np.concatenate([rc, np.zeros(q_max - q, np.float32)])
    bh, bl, eps_floor, _ = tolerances(f, a, y, C)
    Kp, fp, ap, yp = padded_block(Kq, f, a, y, q_max)
    kw = dict(clip="box", eps=1e-3, rel=0.3, eps_floor=eps_floor, b_hi=bh, b_lo=bl, inner_max=4 * q_max, wss=wss,
              row_C=row_C)
    ref = K.ws_solve(Kp, fp, ap, yp, [q], q_max, C, **kw)
    got = K.ws_solve(Kp, fp, ap, yp, [q], q_max, C, diag=True, **kw)
    assert ref["steps"][0] > 0
    assert got["steps"] == ref["steps"] and got["apply_idx"] == ref["apply_idx"] and got["done"] == ref["done"]
    np.testing.assert_array_equal(got["alpha"].view(np.uint32), ref["alpha"].view(np.uint32))
    np.testing.assert_array_equal(np.asarray(got["apply_coef"]).view(np.uint32),
                                  np.asarray(ref["apply_coef"]).view(np.uint32))


# ---------------------------------------------------------------- 2. general diagonal: the pair-rule model
def pair_step_model(a_hi, a_lo, y_hi, y_lo, bh, bl, khl, khh, kll, C, tau, same):
    """tests/test_ws_kernels_gpu.py's pair_step_model (box clipping) with eta = (khh + kll) - 2 khl"""
    f32 = np.float32
    eta = f32(f32(khh) + f32(kll)) - f32(2.0) * f32(khl)
    eta = eta if eta >= f32(tau) else f32(tau)
    s = f32(y_lo * y_hi)
    a_lo_new = f32(a_lo + f32(f32(y_lo * f32(bh - bl)) / eta))
    if not same:
        if y_hi != y_lo:
            dl = f32(a_lo - a_hi)
            L, hL = (dl, f32(0)) if dl > 0 else (f32(0), f32(-1))
            H, hH = (f32(C + dl), f32(C)) if f32(C + dl) < C else (f32(C), f32(-1))
        else:
            sm = f32(a_lo + a_hi)
            L, hL = (f32(sm - C), f32(C)) if f32(sm - C) > 0 else (f32(0), f32(-1))
            H, hH = (sm, f32(0)) if sm < C else (f32(C), f32(-1))
        atL = a_lo_new <= L
        atH = (not atL) and a_lo_new >= H
        a_lo_new = L if atL else (H if atH else a_lo_new)
        snap = hL if atL else (hH if atH else f32(-1))
        a_hi_new = snap if snap >= 0 else f32(a_hi + f32(s * f32(a_lo - a_lo_new)))
        a_hi_new = f32(min(max(a_hi_new, 0), C))
    else:
        a_hi_new = f32(a_hi + f32(s * f32(a_lo - a_lo_new)))
        a_lo_new = f32(min(max(a_lo_new, 0), C))
        a_hi_new = f32(min(max(a_hi_new, 0), C))
    return a_hi_new, a_lo_new, f32(f32(a_hi_new - a_hi) * y_hi), f32(f32(a_lo_new - a_lo) * y_lo)


def solve_model(Kq, f, a, y, C, eps_in, tau, cap, w2=False):
    """tests/test_ws_kernels_gpu.py's solve_model (box clipping) on a Gram with any diagonal; w2: the low row by
    the gain (f_lo - b_hi)^2 / eta(hi, lo) with eta = (K(hi,hi) + K(lo,lo)) - 2 K(hi,lo).  Also returns how often
    eta was floored at tau."""
    f32 = np.float32
    Kq = Kq.astype(np.float32)
    kd = np.diagonal(Kq).copy()
    a = a.astype(np.float32).copy()
    y = y.astype(np.float32)
    fu = np.where(in_up(a, y, C), f, np.inf).astype(np.float32)
    fl = np.where(in_low(a, y, C), -f, np.inf).astype(np.float32)
    steps, floored = 0, 0
    while steps < cap:
        mu, ml = fu.min(), fl.min()
        bh, bl = mu, f32(-ml)
        if not (mu < np.inf and ml < np.inf and bl > f32(bh + f32(f32(2.0) * f32(eps_in)))):
            break
        ph, pl = int(np.argmin(fu)), int(np.argmin(fl))
        if w2:
            dv = (-fl - bh).astype(np.float32)
            eta = ((kd[ph] + kd).astype(np.float32) - np.float32(2.0) * Kq[ph, :]).astype(np.float32)
            eta = np.maximum(eta, np.float32(tau)).astype(np.float32)
            g = np.where(np.isfinite(fl) & (dv > 0), -(dv * dv) / eta, np.inf)
            pl = int(np.argmin(g))
            bl = f32(-fl[pl])
        floored += bool(f32(kd[ph] + kd[pl]) - f32(2.0) * Kq[ph, pl] < f32(tau))
        a_hi_new, a_lo_new, c_hi, c_lo = pair_step_model(a[ph], a[pl], y[ph], y[pl], bh, bl, Kq[ph, pl], kd[ph],
                                                         kd[pl], C, tau, ph == pl)
        dl = (c_hi * Kq[ph, :]).astype(np.float32) + (c_lo * Kq[pl, :]).astype(np.float32)
        fu = (fu + dl).astype(np.float32)
        fl = (fl - dl).astype(np.float32)
        f_lo_new = f32(bl + f32(f32(c_hi * Kq[ph, pl]) + f32(c_lo * Kq[pl, pl])))
        f_hi_new = f32(bh + f32(f32(c_hi * Kq[ph, ph]) + f32(c_lo * Kq[pl, ph])))
        for pos, an, fp in ((pl, a_lo_new, f_lo_new), (ph, a_hi_new, f_hi_new)):  # hi placed last
            fu[pos] = fp if in_up(an, y[pos], C) else np.inf
            fl[pos] = -fp if in_low(an, y[pos], C) else np.inf
        a[pl] = a_lo_new
        a[ph] = a_hi_new
        steps += 1
    return a, steps, floored


def scaled_problem(rng, q, C, gamma, dup):
    """sub_problem's Gram scaled to D K D, D = diag(u), u uniform in [0.6, 3] (float32), rounded to float32; dup:
    rows 0 and 1 are the same point scaled alike, so K(0,0) = K(1,1) = K(0,1) and their eta is 0 exactly"""
    Kq, _, a, y = sub_problem(rng, q, C, gamma=gamma, dup=dup)
    u = rng.uniform(0.6, 3.0, size=q).astype(np.float32)
    if dup:
        u[1] = u[0]
    Kd = (Kq.astype(np.float64) * np.outer(u.astype(np.float64), u.astype(np.float64))).astype(np.float32)
    f = (Kd.astype(np.float64) @ (a * y) - y + rng.normal(scale=0.3, size=q)).astype(np.float32)
    if dup:  # the pair (0, 1) is the first the rule picks: 0 the lowest of I_up, 1 the highest of I_low
        a[0], a[1], y[0], y[1] = np.float32(0.5 * C), np.float32(0.5 * C), 1.0, 1.0
        f[0], f[1] = np.float32(f.min() - 1.0), np.float32(f.max() + 1.0)
        assert Kd[0, 0] == Kd[1, 1] == Kd[0, 1]
    return Kd, f, a, y


@pytest.mark.parametrize("wss", [1, 2])
@pytest.mark.parametrize("q,q_max,dup", [(40, 40, False), (100, 128, False), (150, 192, False), (192, 192, False),
                                         (100, 128, True)])
def test_ws_solve_diag_matches_general_pair_rule_model(K, q, q_max, dup, wss):
    rng = np.random.default_rng(q * 7 + q_max + (3 if dup else 0) + wss)
    C = 2.0
    Kd, f, a, y = scaled_problem(rng, q, C, 0.7 if wss == 1 else 0.05, dup)
    assert np.diagonal(Kd).min() < 0.5 and np.diagonal(Kd).max() > 4.0  # far from a unit diagonal
    bh, bl, eps_floor, eps_in = tolerances(f, a, y, C)
    Kp, fp, ap, yp = padded_block(Kd, f, a, y, q_max)
    kw = dict(clip="box", eps=1e-3, rel=0.3, eps_floor=eps_floor, b_hi=bh, b_lo=bl, wss=wss, diag=True)
    w2 = wss == 2
    for cap in (1, 3, 8):
        got = K.ws_solve(Kp, fp, ap, yp, [q], q_max, C, inner_max=cap, **kw)
        ref_a, ref_steps, floored = solve_model(Kd, f, a, y, C, eps_in, 1e-12, cap, w2=w2)
        assert got["steps"] == [ref_steps] and got["iter"] == ref_steps
        np.testing.assert_allclose(got["alpha"][:q], ref_a, rtol=2e-6, atol=2e-6 * C)
        if dup and not w2:
            assert floored >= 1  # the first pair is the duplicated one: its step runs into the box on the tau floor
    if not dup:  # the RBF kernels take other steps on this Gram: the case tells the two etas apart (the
        # duplicated pair's step ends on the box under either eta)
        rbf = K.ws_solve(Kp, fp, ap, yp, [q], q_max, C, inner_max=8, **{**kw, "diag": False})
        assert not np.array_equal(rbf["alpha"], got["alpha"])
    got = K.ws_solve(Kp, fp, ap, yp, [q], q_max, C, inner_max=4 * q_max, **kw)
    _, ref_steps, _ = solve_model(Kd, f, a, y, C, eps_in, 1e-12, 4 * q_max, w2=w2)
    an = got["alpha"][:q]
    print(f"q {q} q_max {q_max} dup {dup} wss {wss}: steps {got['steps'][0]} (model {ref_steps})")
    assert np.all((an >= 0) & (an <= C))
    assert abs(float(np.sum((an.astype(np.float64) - a) * y))) < 1e-4 * C * q
    assert abs(got["steps"][0] - ref_steps) <= max(3, ref_steps // 5)
    ch = np.nonzero(an != a)[0]
    assert got["apply_idx"] == ch.tolist()
    np.testing.assert_array_equal(got["apply_coef"], ((an[ch] - a[ch]) * y[ch]).astype(np.float32))


# ---------------------------------------------------------------- 3. gram_rows_dot
def check_dot(K, nt, n, k, ld, ldc, seed):
    rng = np.random.default_rng(seed)
    Kt = np.full((nt, ld), np.nan, np.float32)
    Kt[:, :n] = rng.standard_normal((nt, n)).astype(np.float32)
    coef = np.full((k, ldc), np.nan, np.float32)
    coef[:, :n] = (rng.standard_normal((k, n)) * rng.choice([0.0, 1.0], size=(k, n), p=[0.4, 0.6])).astype(np.float32)
    b = rng.standard_normal(k).astype(np.float32)
    k64, c64 = Kt[:, :n].astype(np.float64), coef[:, :n].astype(np.float64)
    ref = k64 @ c64.T - b.astype(np.float64)
    mag = np.abs(k64) @ np.abs(c64).T
    r = K.gram_rows_dot(Kt, n, coef, b)
    out = r["out"]
    assert out.shape == (nt, k) and out.dtype == np.float32
    assert np.all(r["pad"] == np.float32(r["fill"])), "written outside out"
    # float(sum): half an ulp of float32 at the reference; the fp64 accumulation in any order: n 2^-53 < 1e-12 of
    # sum |Kt coef| for n <= 4,099
    tol = 0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 1e-12 * mag + 1e-45
    err = np.abs(out.astype(np.float64) - ref)
    assert np.all(np.isfinite(out)) and np.all(err <= tol), (nt, n, k, float(np.max(err - tol)))
    again = K.gram_rows_dot(Kt, n, coef, b)["out"]
    np.testing.assert_array_equal(again.view(np.uint32), out.view(np.uint32))


@pytest.mark.parametrize("n", [1, 3, 4, 1023, 1024, 1025, 4099])
def test_gram_rows_dot_matches_numpy_fp64(K, n):
    ld = (n + 3) // 4 * 4 + 4
    for nt in (1, 5, 300):
        for k in (1, 3, 8, 9, 33):
            check_dot(K, nt, n, k, ld, ld, seed=n * 1000 + nt * 37 + k)


@pytest.mark.parametrize("n,ld,ldc", [(1025, 1027, 1028), (1025, 1028, 1025), (6, 7, 9)])
def test_gram_rows_dot_unaligned_rows(K, n, ld, ldc):
    """row strides that are no multiple of 4 floats take the loads by elements: the same bound"""
    for nt, k in ((5, 1), (3, 9)):
        check_dot(K, nt, n, k, ld, ldc, seed=n + ld + k)
