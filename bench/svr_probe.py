#!/usr/bin/env python3
"""epsilon-SVR probes (docs/DESIGN.md §17), one JSON line each.

  --select   what the fold buys: the folded one-pass kernel (ws_select_fold_kernel: n Gram columns, each
             value loaded once for the state rows j and j + n) against the plain one-pass kernel on the
             explicitly unfolded lines (2n columns: each value stored and loaded twice), event-timed over
             192 apply rows.  Every repetition reads another 192 lines of a Gram several times the last-level
             cache, so the rows come from HBM as a solve's do.
  --fit      one SVR.fit on the GPU: wall time, rounds, pair steps.

    python bench/svr_probe.py --select --cols 20000 60000
    python bench/svr_probe.py --fit --samples 20000 --features 20
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

NA = 192


def select_probe(n: int, reps: int, cache_mb: float) -> dict:
    from dpsvm_amd.ops import kernels as K

    rng = np.random.default_rng(n)
    groups = max(2, int(np.ceil(2 * cache_mb * (1 << 20) / (NA * n * 4.0))))
    L = NA * groups
    gram = rng.uniform(0.0, 1.0, size=(L, n)).astype(np.float32)
    y = np.concatenate([np.ones(n, np.float32), -np.ones(n, np.float32)])
    alpha = np.where(rng.random(2 * n) < 0.5, 0.0, 0.5).astype(np.float32)
    f = rng.normal(size=2 * n).astype(np.float32)
    coef = (rng.normal(scale=1e-3, size=NA) * np.where(np.arange(NA) % 2, 1.0, -1.0)).astype(np.float32)
    zeros = np.zeros(2 * n, np.float32)
    lines = np.arange(NA, dtype=np.int32)
    fold = K.ws_select(gram, f, alpha, y, zeros, lines, coef, [NA], 1.0, fold=n, reps=reps)
    plain = K.ws_select(np.concatenate([gram, gram], axis=1), f, alpha, y, zeros, lines, coef, [NA], 1.0, reps=reps)
    same = bool(np.array_equal(fold["f"], plain["f"]))  # after reps timed launches and the returned one each
    tf, tp = np.array(fold["select_us"][2:]), np.array(plain["select_us"][2:])  # the first launches load the code
    byt = NA * n * 4.0
    return {"probe": "svr_select", "cols": n, "apply_rows": NA, "lines": L, "reps": reps,
            "fold_us_median": float(np.median(tf)), "fold_us_min": float(tf.min()),
            "plain_us_median": float(np.median(tp)), "plain_us_min": float(tp.min()),
            "fold_gram_bytes": byt, "plain_gram_bytes": 2 * byt,
            "fold_gbs": byt / (float(np.median(tf)) * 1e-6) / 1e9,
            "plain_gbs": 2 * byt / (float(np.median(tp)) * 1e-6) / 1e9,
            "ratio_plain_over_fold": float(np.median(tp) / np.median(tf)), "f_bit_equal": same}


def fit_probe(n: int, d: int, C: float, gamma: float, epsilon: float, eps: float) -> dict:
    from dpsvm_amd import SVR

    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, size=(n, d)).astype(np.float32)
    x = X.astype(np.float64)
    z = np.sin(2 * x[:, 0]) + x[:, 1] * x[:, 2] + 0.5 * np.cos(2 * x[:, 3] + x[:, 4]) - 0.3 * x[:, 5] ** 2
    z = (z + 0.1 * rng.standard_normal(n)).astype(np.float32)
    out = None
    for rep in range(2):  # the first fit loads the code objects
        t0 = time.perf_counter()
        m = SVR(C=C, gamma=gamma, epsilon=epsilon, eps=eps, device="cuda").fit(X, z)
        wall = time.perf_counter() - t0
        out = {"probe": "svr_fit", "n": n, "d": d, "C": C, "gamma": gamma, "epsilon": epsilon, "eps": eps,
               "wall_s": wall, "fit_s": m.fit_time_, "setup_s": m.setup_time_, "gram_s": m.stats_["t_gram"],
               "rounds": m.n_rounds_, "pair_steps": m.n_iter_, "converged": m.converged_, "n_sv": m.n_support_,
               "gram_bytes": 4.0 * n * n, "engine": m.setup_info_["iteration"], "gram": m.setup_info_["gram"],
               "ws_wss": m.setup_info_["ws_wss"], "note": m.setup_info_["engine_note"],
               "r2_train": m.score(X[:2000], z[:2000])}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--select", action="store_true")
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--cols", type=int, nargs="+", default=[20000, 60000])
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--cache-mb", type=float, default=256.0, help="last-level cache the Gram must exceed twice")
    ap.add_argument("--samples", type=int, default=20000)
    ap.add_argument("--features", type=int, default=20)
    ap.add_argument("--C", type=float, default=1.0)
    ap.add_argument("--gamma", type=float, default=0.1)
    ap.add_argument("--epsilon", type=float, default=0.1)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    if a.select:
        lines += [select_probe(n, a.reps, a.cache_mb) for n in a.cols]
    if a.fit:
        lines.append(fit_probe(a.samples, a.features, a.C, a.gamma, a.epsilon, a.eps))
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
