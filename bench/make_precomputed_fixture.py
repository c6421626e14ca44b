#!/usr/bin/env python3
"""tests/data/sklearn_precomputed.json: scikit-learn on precomputed Grams, the reference of
tests/test_precomputed_cpu.py and tests/test_precomputed_gpu.py.

One X: 600 training and 200 held-out rows, d = 8, float32, uniform on [-0.875, 0.875)^8, rebuilt from an integer
LCG by ``features()`` rather than stored.  Three Grams, built in float64 by
``grams()`` (the tests import it) and rounded to float32, bitwise symmetric:

    rbf     exp(-1.5 |x - y|^2), unit diagonal, strictly positive definite
    scaled  D rbf D with d_i = 0.6 + |x_i|^2: the same, with a diagonal d_i^2 from 1.3 to 25
    poly    (0.5 x.y + 1)^3

Settings: SVC C = 1 on all three; SVR (C = 1, epsilon = 0.1) and one-class nu = 0.2 on the two positive definite
ones (a rank-deficient Gram's SVR / one-class dual is not unique).  Stored per setting: scikit-learn's decisions
on the training and held-out rows at tol = 1e-7, the intercept, n_sv, and ``dev``: the largest difference of
those decisions and the intercept to scikit-learn at tol = 1e-3 — the distance two correct solvers at the
project's stop tolerance may have.  The script asserts dev <= 1e-3 on the positive definite settings and that at
most 5% of the held-out rows lie within 1e-2 of 0, and writes nothing otherwise.

    python bench/make_precomputed_fixture.py [--out tests/data/sklearn_precomputed.json]
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

N_TRAIN, N_TEST, D = 600, 200, 8
GAMMA = 1.5
BAND = 1e-2
SETTINGS = [
    {"kind": "svc", "gram": "rbf"}, {"kind": "svc", "gram": "scaled"}, {"kind": "svc", "gram": "poly"},
    {"kind": "svr", "gram": "rbf"}, {"kind": "svr", "gram": "scaled"},
    {"kind": "oneclass", "gram": "rbf"}, {"kind": "oneclass", "gram": "scaled"},
]
POSITIVE_DEFINITE = ("rbf", "scaled")


def short(v) -> float:
    return float(str(np.float32(v)))


def uniform24(count: int, seed: int) -> np.ndarray:
    """count values k / 2^24 in [0, 1) from a 64-bit LCG in integer arithmetic: the same on every machine, each
    exact in float32 (the fixture stores y and z, the tests rebuild X with this)"""
    s, out = seed, np.empty(count, np.float64)
    for i in range(count):
        s = (s * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        out[i] = (s >> 40) / float(1 << 24)
    return out


def features(seed: int = 23) -> np.ndarray:
    """X (800, 8) float32, uniform on [-0.875, 0.875)^8 (the variance of 0.5 N(0, 1))"""
    u = uniform24((N_TRAIN + N_TEST) * D, seed).reshape(N_TRAIN + N_TEST, D)
    return ((2.0 * u - 1.0) * 0.875).astype(np.float32)


def problem(seed: int = 23):
    """X, labels y in {-1, +1} and regression targets z (float32) of all 800 rows"""
    X = features(seed)
    x = X.astype(np.float64)
    noise = 2.0 * uniform24(2 * len(X), seed + 1).reshape(2, -1) - 1.0
    score = x[:, 0] + 0.7 * x[:, 1] * x[:, 2] - 0.5 * x[:, 3] ** 2 + 0.25 + 0.25 * noise[0]
    y = np.where(score > 0, 1.0, -1.0).astype(np.float32)
    z = np.sin(2.0 * x[:, 0]) + 0.5 * x[:, 1] - 0.3 * x[:, 4] * x[:, 5] + 0.17 * noise[1]
    return X, y, z.astype(np.float32)


def grams(X: np.ndarray, n_train: int = N_TRAIN) -> dict:
    """name -> (K(train, train) (n, n), K(rest, train)) in float32, from float64; the square ones are bitwise
    symmetric (a + b and a * b commute; a BLAS product alone need not be)"""
    x = X.astype(np.float64)
    dot = x @ x.T
    dot = 0.5 * (dot + dot.T)
    sq = np.diagonal(dot).copy()
    d2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * dot, 0.0)
    np.fill_diagonal(d2, 0.0)
    rbf = np.exp(-GAMMA * d2)
    d = 0.6 + sq
    full = {"rbf": rbf, "scaled": rbf * np.outer(d, d), "poly": (0.5 * dot + 1.0) ** 3}
    out = {}
    for name, K in full.items():
        K = K.astype(np.float32)
        out[name] = (np.ascontiguousarray(K[:n_train, :n_train]), np.ascontiguousarray(K[n_train:, :n_train]))
    return out


def fit(kind: str, K: np.ndarray, Kt: np.ndarray, y: np.ndarray, z: np.ndarray, tol: float):
    """scikit-learn on the float64 copy of the float32 Gram -> (decisions train, decisions test, intercept, n_sv)"""
    from sklearn.svm import SVC, SVR, OneClassSVM

    K64, Kt64 = K.astype(np.float64), Kt.astype(np.float64)
    if kind == "svc":
        m = SVC(kernel="precomputed", C=1.0, tol=tol, cache_size=500).fit(K64, y)
        f = m.decision_function
    elif kind == "svr":
        m = SVR(kernel="precomputed", C=1.0, epsilon=0.1, tol=tol, cache_size=500).fit(K64, z.astype(np.float64))
        f = m.predict
    else:
        m = OneClassSVM(kernel="precomputed", nu=0.2, tol=tol, cache_size=500).fit(K64)
        f = m.decision_function
    return f(K64), f(Kt64), float(np.ravel(m.intercept_)[0]), int(len(m.support_))


def main() -> int:
    import sklearn

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument("--out", default=os.path.join(here, "..", "tests", "data", "sklearn_precomputed.json"))
    a = ap.parse_args()
    X, y, z = problem()
    G = grams(X)
    for name, (K, _) in G.items():
        assert np.array_equal(K.view(np.uint32), K.T.view(np.uint32)), f"{name}: not bitwise symmetric"
        dg = np.diagonal(K)
        print(f"gram {name}: diagonal {dg.min():.4g} .. {dg.max():.4g}, smallest eigenvalue "
              f"{np.linalg.eigvalsh(K.astype(np.float64)).min():.3g}")
    out = {
        "sklearn": sklearn.__version__, "tol": 1e-7, "tol_dev": 1e-3, "gamma": GAMMA, "n_train": N_TRAIN,
        # float32 values by their shortest round-trip text, decisions to 8 significant digits (bounds: 1e-2)
        "seed": 23, "y": [int(v) for v in y], "z": [short(v) for v in z],
        "settings": [],
    }
    for s in SETTINGS:
        K, Kt = G[s["gram"]]
        ytr, ztr = y[:N_TRAIN], z[:N_TRAIN]
        d_train, d_test, icpt, n_sv = fit(s["kind"], K, Kt, ytr, ztr, 1e-7)
        l_train, l_test, l_icpt, _ = fit(s["kind"], K, Kt, ytr, ztr, 1e-3)
        dev = float(max(np.max(np.abs(d_train - l_train)), np.max(np.abs(d_test - l_test)), abs(icpt - l_icpt)))
        near = float(np.mean(np.abs(d_test) < BAND))
        print(f"{s['kind']} on {s['gram']}: n_sv={n_sv} intercept={icpt:.6f} max|dec|={np.max(np.abs(d_train)):.3g} "
              f"dev={dev:.3g} near_zero_test={near:.3f}")
        if s["gram"] in POSITIVE_DEFINITE:
            assert dev <= 1e-3, f"{s}: scikit-learn at tol 1e-3 is {dev:.3g} from tol 1e-7 (> 1e-3)"
        if s["kind"] != "svr":
            assert near <= 0.05, f"{s}: {near:.3f} of the held-out rows lie within {BAND} of 0"
        out["settings"].append({**s, "dec_train": [float("%.8g" % v) for v in d_train],
                                "dec_test": [float("%.8g" % v) for v in d_test], "intercept": icpt, "n_sv": n_sv,
                                "dev": float("%.3g" % dev)})
    with open(a.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"wrote {os.path.normpath(a.out)} ({os.path.getsize(a.out)} bytes)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
