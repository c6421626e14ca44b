"""Plain numpy model of the reference's pair rule (svmTrainMain.cpp:235-310) with a
bound per row, 0 <= alpha_i <= C_i: the independent oracle of the weighted tests,
and the data they share.

float64 throughout; ties go to the lowest index.  Sets in the compare form
(up: y > 0 ? a < C_i : a > 0; low: y > 0 ? a > 0 : a < C_i), so a row with
C_i = 0 is in neither.  The box is LIBSVM's two-bound geometry.
"""
import json
import os

import numpy as np

from ref_smo import rbf_gram

N, D, NT = 1500, 32, 400
GAMMA = 1.0 / 32
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "libsvm_weighted_blobs.json")


def blobs(n, seed):
    """the blobs of tests/test_multiclass_gpu.py: four centres 2.5 apart, unit variance; classes 0..3"""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 4, n)
    centres = np.zeros((4, D), dtype=np.float32)
    for c in range(4):
        centres[c, c] = 2.5 / np.sqrt(2.0)
    X = (centres[cls] + rng.standard_normal((n, D))).astype(np.float32)
    return X, cls


def shared_data():
    """X, y (class 3 against the rest), the weights, the held-out X / y, the four-class labels"""
    X, cls = blobs(N, 1)
    Xt, clst = blobs(NT, 2)
    y = np.where(cls == 3, 1.0, -1.0).astype(np.float32)
    yt = np.where(clst == 3, 1.0, -1.0).astype(np.float32)
    w = np.random.default_rng(7).choice([0.25, 0.5, 1, 2, 4], N)
    return X, y, w, Xt, yt, cls


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def sets_w(a, y, Cr):
    up = np.where(y > 0, a < Cr, a > 0)
    low = np.where(y > 0, a > 0, a < Cr)
    return up, low


def pair_step_w(a_hi, a_lo, y_hi, y_lo, b_hi, b_lo, k_hl, C_hi, C_lo, clip="independent", same=False, tau=1e-12):
    """one pair update with two bounds -> (a_hi_new, a_lo_new)"""
    eta = max(2.0 - 2.0 * k_hl, tau)
    s = y_lo * y_hi
    aln = a_lo + y_lo * (b_hi - b_lo) / eta
    if clip == "box" and not same:
        if y_hi != y_lo:
            dl = a_lo - a_hi
            L, hL = (dl, 0.0) if dl > 0 else (0.0, None)
            H, hH = (C_hi + dl, C_hi) if C_hi + dl < C_lo else (C_lo, None)
        else:
            sm = a_lo + a_hi
            L, hL = (sm - C_hi, C_hi) if sm - C_hi > 0 else (0.0, None)
            H, hH = (sm, 0.0) if sm < C_lo else (C_lo, None)
        snap = None
        if aln <= L:
            aln, snap = L, hL
        elif aln >= H:
            aln, snap = H, hH
        ahn = snap if snap is not None else min(max(a_hi + s * (a_lo - aln), 0.0), C_hi)
    else:
        ahn = a_hi + s * (a_lo - aln)
        aln, ahn = min(max(aln, 0.0), C_lo), min(max(ahn, 0.0), C_hi)
    return ahn, aln


def smo_reference_w(X, y, Cr, gamma, eps=1e-3, max_iter=150000, clip="independent", K=None):
    y = np.where(np.asarray(y) > 0, 1.0, -1.0)
    Cr = np.asarray(Cr, dtype=np.float64)
    K = rbf_gram(X, gamma) if K is None else K
    a = np.zeros(len(y))
    f = -y.copy()
    it = 0
    while True:
        up, low = sets_w(a, y, Cr)
        ih, il = int(np.argmin(np.where(up, f, np.inf))), int(np.argmin(np.where(low, -f, np.inf)))
        bh, bl = f[ih], f[il]
        ahn, aln = pair_step_w(a[ih], a[il], y[ih], y[il], bh, bl, K[ih, il], Cr[ih], Cr[il], clip, ih == il)
        dh, dl = ahn - a[ih], aln - a[il]
        a[il] = aln
        a[ih] = ahn
        f += dh * y[ih] * K[ih] + dl * y[il] * K[il]
        it += 1
        if not (bl > bh + 2 * eps) or it >= max_iter:
            break
    return a, (bl + bh) / 2.0, it


def kkt_gap_w(K, y, alpha, Cr):
    """float64 b_lo - b_hi of alpha over the per-row sets (K: the float64 Gram)"""
    y = np.where(np.asarray(y) > 0, 1.0, -1.0)
    a = np.asarray(alpha, dtype=np.float64)
    f = K @ (a * y) - y
    up, low = sets_w(a, y, np.asarray(Cr, dtype=np.float64))
    return float(np.max(f[low]) - np.min(f[up]))
