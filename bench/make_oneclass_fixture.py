#!/usr/bin/env python3
"""tests/data/sklearn_oneclass.json: scikit-learn's one-class SVM on a small novelty-detection problem, the
reference of tests/test_oneclass_cpu.py and tests/test_oneclass_gpu.py.

500 training and 200 held-out rows, d = 8, float32: 660 rows 0.5 N(0, I) and 40 rows uniform on [-3, 3]^8,
shuffled; four settings (nu, gamma), each solved by sklearn.svm.OneClassSVM(kernel="rbf", tol=1e-7) in float64.
Stored per setting: the decisions on the training rows and on the held-out rows, rho (= -intercept_ = offset_),
the number of support vectors and sum(alpha) (= nu n).

    python bench/make_oneclass_fixture.py [--out tests/data/sklearn_oneclass.json]
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

SETTINGS = [
    {"nu": 0.1, "gamma": 0.5},
    {"nu": 0.5, "gamma": 0.125},
    {"nu": 0.05, "gamma": 1.0},
    {"nu": 0.3003, "gamma": 0.5},   # nu n = 150.15: a fractional alpha in the start
]


def problem(n: int = 500, n_test: int = 200, d: int = 8, seed: int = 11, n_out: int = 40):
    rng = np.random.default_rng(seed)
    inl = 0.5 * rng.standard_normal(size=(n + n_test - n_out, d))
    out = rng.uniform(-3.0, 3.0, size=(n_out, d))
    X = np.concatenate([inl, out], axis=0)
    X = X[rng.permutation(n + n_test)].astype(np.float32)
    return X[:n], X[n:]


def main() -> int:
    import sklearn
    from sklearn.svm import OneClassSVM

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    here = os.path.dirname(os.path.abspath(__file__))
    ap.add_argument("--out", default=os.path.join(here, "..", "tests", "data", "sklearn_oneclass.json"))
    a = ap.parse_args()
    X, Xt = problem()
    out = {
        "sklearn": sklearn.__version__,
        "tol": 1e-7,
        "X": [[float(v) for v in r] for r in X],
        "X_test": [[float(v) for v in r] for r in Xt],
        "settings": [],
    }
    for s in SETTINGS:
        m = OneClassSVM(kernel="rbf", nu=s["nu"], gamma=s["gamma"], tol=1e-7, cache_size=500)
        m.fit(X.astype(np.float64))
        dec_train = m.decision_function(X.astype(np.float64))
        dec_test = m.decision_function(Xt.astype(np.float64))
        out["settings"].append({
            **s,
            "dec_train": [float(v) for v in dec_train],
            "dec_test": [float(v) for v in dec_test],
            "rho": float(m.offset_[0]),
            "n_sv": int(len(m.support_)),
            "sum_alpha": float(np.sum(m.dual_coef_)),
        })
        print(f"nu={s['nu']} gamma={s['gamma']}: n_sv={len(m.support_)} rho={m.offset_[0]:.6f} "
              f"sum_alpha={np.sum(m.dual_coef_):.4f} near_zero_test={np.mean(np.abs(dec_test) < 1e-2):.3f} "
              f"outliers_train={np.mean(dec_train < 0):.3f}")
    with open(a.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"wrote {os.path.normpath(a.out)} ({os.path.getsize(a.out)} bytes)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
