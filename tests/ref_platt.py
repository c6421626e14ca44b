"""Plain numpy float64 port of Platt scaling as Lin, Lin and Weng's note gives it
("A note on Platt's probabilistic outputs for support vector machines", 2007; the
method of LIBSVM's sigmoid_train), and of the probability formula: the independent
oracle of the probability tests, and the fixture they share.

P(y = +1 | d) = 1 / (1 + exp(A d + B)).  Targets (n+ + 1) / (n+ + 2) for y > 0, else
1 / (n- + 2); start A = 0, B = log((n- + 1) / (n+ + 1)); Newton steps with a 1e-12
ridge, backtracking from 1 by halving while the step is >= 1e-10 (sufficient
decrease 1e-4 step g'd); stop when both gradient components are below 1e-5, or
after 100 steps.
"""
import json
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "platt_blobs.json")
C, CV, CV_SEED = 1.0, 5, 0


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def objective(d, t, A, B):
    x = d * A + B
    return float(np.sum(np.where(x >= 0, t * x, (t - 1.0) * x) + np.log1p(np.exp(-np.abs(x)))))


def platt_fit(dec, y):
    """-> dict A, B, iters (Newton steps taken), evals (objective evaluations, the start's included), fval,
    status (0 converged, 1 line search failed, 2 stopped at 100 steps)"""
    d = np.asarray(dec, dtype=np.float64)
    pos = np.asarray(y) > 0
    n_pos = float(np.sum(pos))
    n_neg = float(len(d)) - n_pos
    t = np.where(pos, (n_pos + 1.0) / (n_pos + 2.0), 1.0 / (n_neg + 2.0))
    A, B = 0.0, float(np.log((n_neg + 1.0) / (n_pos + 1.0)))
    fval = objective(d, t, A, B)
    evals, status, it = 1, 2, 0
    while it < 100:
        x = d * A + B
        e = np.exp(-np.abs(x))
        u = 1.0 / (1.0 + e)
        w = e * u
        p = np.where(x >= 0, w, u)
        q = np.where(x >= 0, u, w)
        d2 = p * q
        d1 = t - p
        h11 = float(np.sum(d * d * d2)) + 1e-12
        h22 = float(np.sum(d2)) + 1e-12
        h21 = float(np.sum(d * d2))
        g1 = float(np.sum(d * d1))
        g2 = float(np.sum(d1))
        if abs(g1) < 1e-5 and abs(g2) < 1e-5:
            status = 0
            break
        det = h11 * h22 - h21 * h21
        with np.errstate(all="ignore"):
            dA = np.float64(-(h22 * g1 - h21 * g2)) / np.float64(det)
            dB = np.float64(-(-h21 * g1 + h11 * g2)) / np.float64(det)
            gd = g1 * dA + g2 * dB
            step, moved = 1.0, False
            while step >= 1e-10:
                nA, nB = A + step * dA, B + step * dB
                nf = objective(d, t, nA, nB)
                evals += 1
                if nf < fval + 1e-4 * step * gd:
                    A, B, fval, moved = float(nA), float(nB), nf, True
                    break
                step *= 0.5
        if not moved:
            status = 1
            break
        it += 1
    return {"A": A, "B": B, "iters": it, "evals": evals, "fval": fval, "status": status}


def sigmoid(x):
    """1 / (1 + exp(x)) in the two-branch form, float64"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        e = np.exp(-np.abs(x))
    return np.where(x >= 0, e / (1.0 + e), 1.0 / (1.0 + e))


def proba(dec, A, B):
    """decisions (n, k) -> probabilities (n, k) in float64: the k sigmoids, for k > 2 divided by the row's sum
    (a sum of 0: 1 / k each)"""
    d = np.asarray(dec, dtype=np.float64)
    p = sigmoid(d * np.asarray(A, dtype=np.float64)[None, :] + np.asarray(B, dtype=np.float64)[None, :])
    k = p.shape[1]
    if k <= 2:
        return p
    s = p.sum(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(s > 0, p / s, 1.0 / k)
