#!/usr/bin/env python3
"""tests/data/sklearn_named_kernels.json: scikit-learn on its own linear, polynomial and sigmoid kernels, the
reference of tests/test_named_kernels_cpu.py and tests/test_named_kernels_gpu.py.

One X: 600 training and 200 held-out rows, d = 20, float32, uniform on [-0.875, 0.875)^20, rebuilt from an integer
LCG by ``features()`` (the tests import it) rather than stored.  scikit-learn evaluates the kernels itself, in
float64, from the rows (kernel="linear" / "poly" / "sigmoid" with the setting's gamma, coef0 and degree): nothing
of this project computes the reference.

Settings (``SETTINGS``): SVC linear; SVC (0.1 x.y + 1)^3; SVC tanh(0.02 x.y); SVR (0.1 x.y + 1)^2, epsilon 0.1;
one-class (0.1 x.y + 1)^2, nu 0.2; C = 1 throughout.  Stored per setting: scikit-learn's decisions on the training
and held-out rows at tol = 1e-7, the intercept, n_sv, and ``dev``: the largest difference of those decisions and
the intercept to scikit-learn at tol = 1e-3 — the distance two correct solvers at the project's stop tolerance may
have.  The script asserts that every fit converged without a warning and that dev <= 1% of the setting's largest
|decision|, and writes nothing otherwise.

    python bench/make_named_kernels_fixture.py [--out tests/data/sklearn_named_kernels.json]
"""
from __future__ import annotations

import argparse
import json
import os
import warnings

import numpy as np

N_TRAIN, N_TEST, D = 600, 200, 20
SETTINGS = [
    {"kind": "svc", "kernel": "linear", "degree": 1, "coef0": 0.0, "gamma": 1.0},
    {"kind": "svc", "kernel": "poly", "degree": 3, "coef0": 1.0, "gamma": 0.1},
    {"kind": "svc", "kernel": "sigmoid", "degree": 1, "coef0": 0.0, "gamma": 0.02},
    {"kind": "svr", "kernel": "poly", "degree": 2, "coef0": 1.0, "gamma": 0.1},
    {"kind": "oneclass", "kernel": "poly", "degree": 2, "coef0": 1.0, "gamma": 0.1},
]
C_, EPSILON, NU = 1.0, 0.1, 0.2


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


def features(seed: int = 41) -> np.ndarray:
    """X (800, 20) float32, uniform on [-0.875, 0.875)^20"""
    u = uniform24((N_TRAIN + N_TEST) * D, seed).reshape(N_TRAIN + N_TEST, D)
    return ((2.0 * u - 1.0) * 0.875).astype(np.float32)


def problem(seed: int = 41):
    """X, labels y in {-1, +1} and regression targets z (float32) of all 800 rows"""
    X = features(seed)
    x = X.astype(np.float64)
    noise = 2.0 * uniform24(2 * len(X), seed + 1).reshape(2, -1) - 1.0
    score = x[:, 0] + 0.6 * x[:, 1] - 0.8 * x[:, 2] + 0.7 * x[:, 3] * x[:, 4] + 0.1 + 0.25 * noise[0]
    y = np.where(score > 0, 1.0, -1.0).astype(np.float32)
    z = x[:, 0] - 0.5 * x[:, 1] + 0.8 * x[:, 2] * x[:, 3] - 0.4 * x[:, 5] ** 2 + 0.1 * noise[1]
    return X, y, z.astype(np.float32)


def fit(s: dict, X: np.ndarray, Xt: np.ndarray, y: np.ndarray, z: np.ndarray, tol: float):
    """scikit-learn on the float64 copy of the float32 rows -> (decisions train, decisions test, intercept, n_sv);
    any warning (ConvergenceWarning among them) is an error"""
    from sklearn.svm import SVC, SVR, OneClassSVM

    kw = dict(kernel=s["kernel"], gamma=s["gamma"], coef0=s["coef0"], degree=s["degree"], tol=tol, cache_size=500)
    X64, Xt64 = X.astype(np.float64), Xt.astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        if s["kind"] == "svc":
            m = SVC(C=C_, **kw).fit(X64, y)
            f = m.decision_function
        elif s["kind"] == "svr":
            m = SVR(C=C_, epsilon=EPSILON, **kw).fit(X64, z.astype(np.float64))
            f = m.predict
        else:
            m = OneClassSVM(nu=NU, **kw).fit(X64)
            f = m.decision_function
    assert m.fit_status_ == 0, f"{s}: scikit-learn did not converge at tol {tol}"
    return f(X64), f(Xt64), float(np.ravel(m.intercept_)[0]), int(len(m.support_))


def main() -> int:
    import sklearn

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument("--out", default=os.path.join(here, "..", "tests", "data", "sklearn_named_kernels.json"))
    a = ap.parse_args()
    X, y, z = problem()
    Xtr, Xte, ytr, ztr = X[:N_TRAIN], X[N_TRAIN:], y[:N_TRAIN], z[:N_TRAIN]
    out = {
        "sklearn": sklearn.__version__, "tol": 1e-7, "tol_dev": 1e-3, "n_train": N_TRAIN, "C": C_,
        "epsilon": EPSILON, "nu": NU,
        # float32 values by their shortest round-trip text, decisions to 8 significant digits
        "seed": 41, "y": [int(v) for v in y], "z": [short(v) for v in z],
        "settings": [],
    }
    for s in SETTINGS:
        d_train, d_test, icpt, n_sv = fit(s, Xtr, Xte, ytr, ztr, 1e-7)
        l_train, l_test, l_icpt, _ = fit(s, Xtr, Xte, ytr, ztr, 1e-3)
        dev = float(max(np.max(np.abs(d_train - l_train)), np.max(np.abs(d_test - l_test)), abs(icpt - l_icpt)))
        top = float(max(np.max(np.abs(d_train)), np.max(np.abs(d_test))))
        print(f"{s['kind']} {s['kernel']} degree {s['degree']} coef0 {s['coef0']} gamma {s['gamma']}: n_sv={n_sv} "
              f"intercept={icpt:.6f} max|dec|={top:.3g} dev={dev:.3g} ({100 * dev / top:.2f}%)")
        assert dev <= 0.01 * top, f"{s}: dev {dev:.3g} is more than 1% of the largest |decision| {top:.3g}"
        out["settings"].append({**s, "dec_train": [float("%.8g" % v) for v in d_train],
                                "dec_test": [float("%.8g" % v) for v in d_test], "intercept": icpt, "n_sv": n_sv,
                                "dev": float("%.3g" % dev)})
    with open(a.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"wrote {os.path.normpath(a.out)} ({os.path.getsize(a.out)} bytes)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
