#!/usr/bin/env python3
"""LIBSVM (scikit-learn's libsvm, CPU) reference for the sample-weight tests
(tests/test_weights_cpu.py, test_weights_gpu.py, test_cv_gpu.py): trains
sklearn.svm.SVC with sample_weight on the four-blob set of
tests/test_multiclass_gpu.py (class 3 against the rest, n = 1500, d = 32,
gamma = 1/32) with weights rng(7).choice([0.25, 0.5, 1, 2, 4], n), for C = 1 and
C = 10, and stores alpha y of every row, the intercept, the decision values on
400 held-out rows (seed 2) and, for 5-fold cross-validation over the folds
np.array_split(rng(0).permutation(n), 5), each row's out-of-fold decision value.

  python bench/make_weighted_fixture.py [--tol 1e-7]

The fixture is generated here (scikit-learn is not needed where the GPU tests run)
and checked in.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, NT, GAMMA, W_SEED, CV, CV_SEED = 1500, 32, 400, 1.0 / 32, 7, 5, 0


def blobs(n, seed):
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 4, n)
    centres = np.zeros((4, D), dtype=np.float32)
    for c in range(4):
        centres[c, c] = 2.5 / np.sqrt(2.0)  # pairwise distance 2.5
    return (centres[cls] + rng.standard_normal((n, D))).astype(np.float32), cls


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tol", type=float, default=1e-7)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "data", "libsvm_weighted_blobs.json"))
    a = ap.parse_args()
    from sklearn.svm import SVC

    X, cls = blobs(N, 1)
    Xh, _ = blobs(NT, 2)
    y = np.where(cls == 3, 1.0, -1.0)
    w = np.random.default_rng(W_SEED).choice([0.25, 0.5, 1, 2, 4], N)
    folds = np.array_split(np.random.default_rng(CV_SEED).permutation(N), CV)
    rec = {"generator": "blobs of tests/test_multiclass_gpu.py, seeds 1 (train) / 2 (held out); class 3 vs rest",
           "n": N, "d": D, "holdout": NT, "gamma": GAMMA, "tol": a.tol, "weights_seed": W_SEED,
           "weights": "rng(weights_seed).choice([0.25, 0.5, 1, 2, 4], n)", "cv": CV, "cv_seed": CV_SEED,
           "folds": "np.array_split(rng(cv_seed).permutation(n), cv)", "runs": {}}
    for C in (1.0, 10.0):
        m = SVC(C=C, gamma=GAMMA, kernel="rbf", tol=a.tol, cache_size=1000).fit(X, y, sample_weight=w)
        ay = np.zeros(N)
        ay[m.support_] = m.dual_coef_[0]
        bound = np.abs(ay) >= C * w * (1 - 1e-9)
        cvd = np.zeros(N)
        for fold in folds:
            tr = np.setdiff1d(np.arange(N), fold)
            mf = SVC(C=C, gamma=GAMMA, kernel="rbf", tol=a.tol, cache_size=1000).fit(X[tr], y[tr], sample_weight=w[tr])
            cvd[fold] = mf.decision_function(X[fold])
        run = {"C": C, "intercept": float(m.intercept_[0]), "n_support": int(m.n_support_.sum()),
               "n_bounded": int(bound.sum()), "n_free": int(np.sum((ay != 0) & ~bound)),
               "alpha_y": [round(float(v), 7) for v in ay],
               "holdout_decision": [round(float(v), 6) for v in m.decision_function(Xh)],
               "cv_decision": [round(float(v), 6) for v in cvd],
               "cv_accuracy": float(np.mean(np.where(cvd < 0, -1.0, 1.0) == y))}
        rec["runs"]["%g" % C] = run
        print({k: v for k, v in run.items() if not isinstance(v, list)})
    with open(a.out, "w") as f:
        json.dump(rec, f)
    print(a.out, os.path.getsize(a.out), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
