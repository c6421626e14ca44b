#!/usr/bin/env python3
"""scikit-learn reference for the probability tests (tests/test_platt_cpu.py,
test_platt_kernels_gpu.py, test_proba_gpu.py): on the four-blob set of
tests/ref_smo_weighted.shared_data() (n = 1500, d = 32, 400 held-out rows), C = 1,
gamma = 1/32, unweighted, folds SVC.cv_folds(1500, 5, 0), for the four one-vs-rest
machines (machine 3 is also the binary problem "class 3 against the rest"):

  cv_decision_e6   sklearn.svm.SVC's out-of-fold decisions, rounded to 6 decimals (as integers, x 1e6)
  A, B             sklearn.calibration._sigmoid_calibration on those rounded decisions: the same objective,
                   targets and sign convention (p = 1 / (1 + exp(A d + B))) by another optimiser

and the probabilities of the 400 held-out rows (x 1e6): the binary model's P(class 3)
and the four-class model's normalised (400, 4).  Prints the gap between
tests/ref_platt.py's port and scikit-learn on the five runs.

  python bench/make_platt_fixture.py [--tol 1e-7]

The fixture is generated here (scikit-learn is not needed where the GPU tests run)
and checked in; it stays under 64 KB.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tol", type=float, default=1e-7)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "data", "platt_blobs.json"))
    a = ap.parse_args()
    from sklearn.calibration import _sigmoid_calibration
    from sklearn.svm import SVC

    import ref_platt
    from ref_smo_weighted import GAMMA, N, NT, shared_data

    X, y3, _, Xt, _, cls = shared_data()
    folds = np.array_split(np.random.default_rng(ref_platt.CV_SEED).permutation(N), ref_platt.CV)  # SVC.cv_folds
    svc = lambda: SVC(C=ref_platt.C, gamma=GAMMA, kernel="rbf", tol=a.tol, cache_size=1000)  # noqa: E731
    e6 = lambda v: [int(round(float(x) * 1e6)) for x in np.asarray(v).reshape(-1)]  # noqa: E731
    rec = {"generator": "tests/ref_smo_weighted.shared_data(); machine c: class c against the rest; binary: machine 3",
           "n": N, "holdout": NT, "C": ref_platt.C, "gamma": GAMMA, "tol": a.tol, "cv": ref_platt.CV,
           "cv_seed": ref_platt.CV_SEED, "scale": 1e6, "machines": []}
    gapA = gapB = 0.0
    hold = np.zeros((NT, 4))
    for c in range(4):
        y = np.where(cls == c, 1.0, -1.0)
        cvd = np.zeros(N)
        for fold in folds:
            tr = np.setdiff1d(np.arange(N), fold)
            cvd[fold] = svc().fit(X[tr], y[tr]).decision_function(X[fold])
        cvd = np.round(cvd, 6)  # what the fixture stores
        A, B = (float(v) for v in _sigmoid_calibration(cvd, y))
        runs = [("machine %d" % c, cvd)] + ([("binary", cvd)] if c == 3 else [])
        for name, d in runs:  # the port on what the tests will see: the rounded decisions as float32
            port = ref_platt.platt_fit(d.astype(np.float32), y)
            gapA, gapB = max(gapA, abs(port["A"] - A)), max(gapB, abs(port["B"] - B))
            print(f"{name}: A {A:.9f} B {B:.9f}  port - sklearn: dA {port['A'] - A:.3g} dB {port['B'] - B:.3g}  "
                  f"iters {port['iters']} evals {port['evals']} status {port['status']}")
        hold[:, c] = ref_platt.sigmoid(A * svc().fit(X, y).decision_function(Xt) + B)
        rec["machines"].append({"A": A, "B": B, "cv_decision_e6": e6(cvd)})
    assert np.array_equal(np.where(cls == 3, 1.0, -1.0), y3)
    rec["binary_holdout_proba_e6"] = e6(hold[:, 3])
    rec["multi_holdout_proba_e6"] = e6(hold / hold.sum(axis=1, keepdims=True))
    print(f"port against scikit-learn over the five runs: max |dA| {gapA:.3g}  max |dB| {gapB:.3g}")
    with open(a.out, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
    size = os.path.getsize(a.out)
    print(a.out, size, "bytes")
    return 0 if size <= 64 * 1024 else 1


if __name__ == "__main__":
    sys.exit(main())
