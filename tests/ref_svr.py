"""Plain numpy models of epsilon-SVR on the folded 2n-row dual (docs/DESIGN.md §17), the oracles of
tests/test_svr_cpu.py, tests/test_svr_kernels_gpu.py and tests/test_svr_gpu.py.

State rows j < n hold alpha_j (label +1), rows j + n hold alpha*_j (label -1); the kernel matrix of the state
rows is K(a mod n, b mod n); the start is alpha = 0, f[j] = eps - z_j, f[j + n] = -eps - z_j.  Everything else
is the classifier's algorithm (tests/ref_smo.py).

  svr_reference     first-order SMO on the folded dual, float64
  fold_f_update     one folded round's f update in the kernel's float32 summation order
  fold_candidates   the per-workgroup candidate lists of the folded selection
"""
import numpy as np

NONE = np.uint64((1 << 64) - 1)
SEL_THREADS = 256  # kWsSelThreads
PARTS = 4          # list partitions of the one-pass kernels at <= 4 rows per thread (ws_parts)
KC = 16            # kWsCand: the lists' stride
KC1 = 4            # kWsCand1: keys per side a one-block round writes


# ---------------------------------------------------------------- key model (common.hpp)
def f32_order(f):
    u = np.asarray(f, dtype=np.float32).reshape(-1).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def make_key(f, idx):
    return (f32_order(f).astype(np.uint64) << np.uint64(32)) | np.asarray(idx, dtype=np.uint64).reshape(-1)


def in_up(a, y, C):
    a, y = np.asarray(a, np.float32), np.asarray(y, np.float32)
    return np.where(a == 0, y == 1, np.where(a == np.float32(C), y != 1, True))


def in_low(a, y, C):
    a, y = np.asarray(a, np.float32), np.asarray(y, np.float32)
    return np.where(a == 0, y != 1, np.where(a == np.float32(C), y == 1, True))


def fold_labels(n):
    return np.concatenate([np.ones(n, np.float32), -np.ones(n, np.float32)])


def fold_start(z, epsilon):
    """f of the folded dual at alpha = 0: y o p with p = [eps - z, eps + z], in float32 as init_f computes it"""
    z = np.asarray(z, np.float32)
    e = np.float32(epsilon)
    return np.concatenate([e - z, -e - z]).astype(np.float32)


# ---------------------------------------------------------------- one folded round
def fold_f_update(lines, coef, f, n):
    """f after the folded round's update.  ``lines`` [na][>= n]: the changed rows' Gram lines in list order,
    ``coef`` their (alpha_new - alpha_old) y.  Column j's sum acc_j = sum_k coef_k lines[k][j] is formed as the
    kernel forms it — the list cut into PARTS contiguous slices of ceil(na / PARTS), each summed from 0 in list
    order with a rounded product and a rounded add (no fma), the slices' sums added in slice order — and the
    same acc_j goes to f[j] and f[j + n]."""
    lines = np.asarray(lines, np.float32)[:, :n]
    coef = np.asarray(coef, np.float32)
    f = np.asarray(f, np.float32).copy()
    na = len(coef)
    if na == 0:
        return f
    per = (na + PARTS - 1) // PARTS
    acc = None
    for p in range(PARTS):
        part = np.zeros(n, np.float32)
        for k in range(min(na, p * per), min(na, p * per + per)):
            part = (part + (coef[k] * lines[k]).astype(np.float32)).astype(np.float32)
        acc = part if acc is None else (acc + part).astype(np.float32)
    f[:n] = (f[:n] + acc).astype(np.float32)
    f[n:] = (f[n:] + acc).astype(np.float32)
    return f


def fold_geometry(n):
    """selection workgroups and columns per thread over the n Gram columns (launch::ws_geometry at one rank)"""
    G = max(1, min(256, (n + SEL_THREADS - 1) // SEL_THREADS))
    rpt = max(1, (n + G * SEL_THREADS - 1) // (G * SEL_THREADS))
    return G, rpt


def fold_candidates(f, alpha, y, C, n, nc=KC1):
    """[G][2][nc] u64: workgroup b owns columns [b rpt 256, (b + 1) rpt 256) and classifies the state rows j and
    j + n of each; per side its nc smallest keys (f, row) ascending — ties on f go to the lower row — and
    kKeyNone past the side's rows."""
    G, rpt = fold_geometry(n)
    out = np.full((G, 2, nc), NONE, dtype=np.uint64)
    f, alpha, y = (np.asarray(v, np.float32) for v in (f, alpha, y))
    for b in range(G):
        cols = np.arange(b * rpt * SEL_THREADS, min(n, (b + 1) * rpt * SEL_THREADS))
        rows = np.concatenate([cols, cols + n])
        if len(rows) == 0:
            continue
        up, lo = in_up(alpha[rows], y[rows], C), in_low(alpha[rows], y[rows], C)
        u = np.sort(make_key(f[rows][up], rows[up]))[:nc]
        l_ = np.sort(make_key(-f[rows][lo], rows[lo]))[:nc]
        out[b, 0, : len(u)] = u
        out[b, 1, : len(l_)] = l_
    return out


# ---------------------------------------------------------------- the whole solve
def rbf_gram(X, gamma):
    X = X.astype(np.float64)
    sq = (X * X).sum(1)
    return np.exp(-gamma * np.maximum(sq[:, None] + sq[None, :] - 2.0 * X @ X.T, 0.0))


def svr_reference(X, z, C, gamma, epsilon, eps=1e-3, max_iter=150000, tau=1e-12):
    """first-order SMO with the joint box on the folded dual; returns (alpha [2n], b, steps)"""
    n = len(z)
    K = rbf_gram(X, gamma)
    y = fold_labels(n).astype(np.float64)
    z = np.asarray(z, np.float64)
    a = np.zeros(2 * n)
    f = np.concatenate([epsilon - z, -epsilon - z])
    it = 0
    while True:
        up = ((a == 0) & (y == 1)) | ((a == C) & (y != 1)) | ((a > 0) & (a < C))
        lo = ((a == 0) & (y != 1)) | ((a == C) & (y == 1)) | ((a > 0) & (a < C))
        ih, il = int(np.argmin(np.where(up, f, np.inf))), int(np.argmin(np.where(lo, -f, np.inf)))
        bh, bl = f[ih], f[il]
        eta = max(2.0 - 2.0 * K[ih % n, il % n], tau)
        aln = a[il] + y[il] * (bh - bl) / eta
        if y[ih] != y[il]:
            dl = a[il] - a[ih]
            L, hL = (dl, 0.0) if dl > 0 else (0.0, None)
            H, hH = (C + dl, C) if dl < 0 else (C, None)
        else:
            sm = a[il] + a[ih]
            L, hL = (sm - C, C) if sm > C else (0.0, None)
            H, hH = (sm, 0.0) if sm < C else (C, None)
        snap = None
        if aln <= L:
            aln, snap = L, hL
        elif aln >= H:
            aln, snap = H, hH
        ahn = snap if snap is not None else min(max(a[ih] + y[il] * y[ih] * (a[il] - aln), 0.0), C)
        d = (ahn - a[ih]) * y[ih] * K[ih % n] + (aln - a[il]) * y[il] * K[il % n]
        a[il], a[ih] = aln, ahn
        f[:n] += d
        f[n:] += d
        it += 1
        if not (bl > bh + 2 * eps) or it >= max_iter:
            break
    return a, (bl + bh) / 2.0, it


def svr_predict(Xtr, alpha, b, gamma, Xte):
    n = len(Xtr)
    Xtr, Xte = Xtr.astype(np.float64), Xte.astype(np.float64)
    d2 = np.maximum((Xte * Xte).sum(1)[:, None] + (Xtr * Xtr).sum(1)[None, :] - 2 * Xte @ Xtr.T, 0)
    return np.exp(-gamma * d2) @ (alpha[:n] - alpha[n:]) - b
