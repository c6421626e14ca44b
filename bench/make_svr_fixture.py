#!/usr/bin/env python3
"""tests/data/sklearn_svr.json: scikit-learn's epsilon-SVR on a small smooth regression problem, the reference
of tests/test_svr_cpu.py and tests/test_svr_gpu.py.

500 x 8 float32 training rows in [-1, 1], 200 held-out rows, target = a smooth function of the features plus
noise; three settings (C, gamma, epsilon), each solved by sklearn.svm.SVR(kernel="rbf", tol=1e-7) in float64.
Stored per setting: the predictions on the training rows and on the held-out rows, the intercept and the
number of support vectors.

    python bench/make_svr_fixture.py [--out tests/data/sklearn_svr.json]
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

SETTINGS = [
    {"C": 1.0, "gamma": 0.5, "epsilon": 0.1},
    {"C": 10.0, "gamma": 0.125, "epsilon": 0.05},
    {"C": 1.0, "gamma": 0.5, "epsilon": 0.0},
]


def problem(n: int = 500, n_test: int = 200, d: int = 8, seed: int = 7):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, size=(n + n_test, d)).astype(np.float32)
    x = X.astype(np.float64)
    z = np.sin(2.0 * x[:, 0]) + 0.5 * x[:, 1] * x[:, 2] + 0.3 * np.cos(3.0 * x[:, 3]) - 0.4 * x[:, 4] ** 2
    z = (z + 0.1 * rng.standard_normal(n + n_test)).astype(np.float32)
    return X[:n], z[:n], X[n:], z[n:]


def main() -> int:
    import sklearn
    from sklearn.svm import SVR

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument("--out", default=os.path.join(here, "..", "tests", "data", "sklearn_svr.json"))
    a = ap.parse_args()
    X, z, Xt, zt = problem()
    out = {
        "sklearn": sklearn.__version__,
        "tol": 1e-7,
        "X": [[float(v) for v in r] for r in X],
        "z": [float(v) for v in z],
        "X_test": [[float(v) for v in r] for r in Xt],
        "z_test": [float(v) for v in zt],
        "settings": [],
    }
    for s in SETTINGS:
        m = SVR(kernel="rbf", C=s["C"], gamma=s["gamma"], epsilon=s["epsilon"], tol=1e-7, cache_size=500)
        m.fit(X.astype(np.float64), z.astype(np.float64))
        out["settings"].append({
            **s,
            "pred_train": [float(v) for v in m.predict(X.astype(np.float64))],
            "pred_test": [float(v) for v in m.predict(Xt.astype(np.float64))],
            "intercept": float(m.intercept_[0]),
            "n_sv": int(len(m.support_)),
            "r2_test": float(m.score(Xt.astype(np.float64), zt.astype(np.float64))),
        })
        print(f"C={s['C']} gamma={s['gamma']} epsilon={s['epsilon']}: n_sv={len(m.support_)} "
              f"intercept={m.intercept_[0]:.6f} r2_test={out['settings'][-1]['r2_test']:.4f}")
    with open(a.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"wrote {os.path.normpath(a.out)} ({os.path.getsize(a.out)} bytes)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
