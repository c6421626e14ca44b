#!/usr/bin/env python3
"""One-class probes (docs/DESIGN.md §18), one JSON line each.

  --wsum   gram_rows_wsum at m = n / 2 (the start of nu = 0.5), identity lines, event-timed: bytes read
           (m n 4), the achieved rate beside the project's measured stream-read rate (6.0 TB/s, README), and
           the alternative the kernel replaces — f of the same start recomputed from X by the predict GEMM
           (ops.kernels.rbf_decision: row norms, GEMM, fused exp and row reduce; --features 128 and up run the
           split-operand GEMM).  The Gram passed holds just the rows the sum reads, but never fewer than a
           GiB of them, so the row loads are the non-temporal ones a solver's whole Gram of this n gets.
  --fit    one OneClassSVM.fit and a five-value nu_path on one shape: wall time, rounds, the start's event time,
           the Gram GEMM's, and what the sweep's later solves cost without it.

    python bench/oneclass_probe.py --wsum --cols 20000 60000
    python bench/oneclass_probe.py --fit --samples 20000 --features 20
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

STREAM_READ_TBS = 6.0  # the project's measured stream-read rate (README: pass 1 at the stream roofline)


def wsum_probe(n: int, reps: int, d: int, gamma: float) -> dict:
    import torch

    from dpsvm_amd.ops import kernels as K

    rng = np.random.default_rng(n)
    m = n // 2
    ldg = (n + 3) // 4 * 4
    L = max(m, ((1 << 30) // (4 * ldg)) + 1)
    gram = rng.random(size=(L, ldg), dtype=np.float32)
    coef = np.ones(m, np.float32)
    r = K.gram_rows_wsum(gram, n, coef, reps=reps)
    us = np.array(r["us"][2:])  # the first launches load the code
    ref = gram[:m, :n].sum(axis=0, dtype=np.float64)
    ulp = float(np.max(np.abs(r["out"].astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32))))
    del gram
    byt = 4.0 * m * n
    # the alternative: f = K(X, X[:m]) 1 from X
    X = torch.from_numpy(rng.standard_normal(size=(n, d)).astype(np.float32) * 0.5).cuda()
    ones = torch.ones(m, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    gemm = []
    for _ in range(max(3, reps // 4)):
        e0.record()
        K.rbf_decision(X, X[:m], ones, gamma, 0.0)
        e1.record()
        e1.synchronize()
        gemm.append(1e3 * e0.elapsed_time(e1))
    gemm = np.array(gemm[1:])
    return {"probe": "gram_rows_wsum", "cols": n, "rows": m, "slices": r["S"], "reps": reps,
            "us_median": float(np.median(us)), "us_min": float(us.min()), "bytes": byt,
            "tbs_median": byt / (float(np.median(us)) * 1e-6) / 1e12, "stream_read_tbs": STREAM_READ_TBS,
            "max_err_ulp": ulp, "features": d, "predict_gemm_us_median": float(np.median(gemm)),
            "predict_gemm_us_min": float(gemm.min()),
            "ratio_gemm_over_wsum": float(np.median(gemm) / np.median(us))}


def fit_probe(n: int, d: int, nu: float, gamma: float, eps: float) -> dict:
    from dpsvm_amd import OneClassSVM

    rng = np.random.default_rng(5)
    n_out = n // 20
    X = np.concatenate([0.5 * rng.standard_normal(size=(n - n_out, d)), rng.uniform(-2, 2, size=(n_out, d))])
    X = X[rng.permutation(n)].astype(np.float32)
    out = None
    for rep in range(2):  # the first fit loads the code objects
        t0 = time.perf_counter()
        m = OneClassSVM(nu=nu, gamma=gamma, eps=eps, device="cuda").fit(X)
        wall = time.perf_counter() - t0
        out = {"probe": "oneclass_fit", "n": n, "d": d, "nu": nu, "gamma": gamma, "eps": eps, "wall_s": wall,
               "fit_s": m.fit_time_, "setup_s": m.setup_time_, "gram_s": m.stats_["t_gram"],
               "start_s": m.stats_["t_start"], "rounds": m.n_rounds_, "pair_steps": m.n_iter_,
               "converged": m.converged_, "n_sv": m.n_support_, "rho": m.offset_,
               "outlier_fraction": float(np.mean(m.train_decision_ < 0)), "gram_bytes": 4.0 * n * n,
               "engine": m.setup_info_["iteration"], "gram": m.setup_info_["gram"],
               "ws_wss": m.setup_info_["ws_wss"], "note": m.setup_info_["engine_note"]}
    nus = [0.05, 0.1, 0.2, 0.3, 0.5]
    t0 = time.perf_counter()
    path = m.nu_path(X, nus)
    out["path"] = {"nus": nus, "wall_s": time.perf_counter() - t0, "rho": path["rho"], "n_sv": path["n_support"],
                   "outlier_fraction": path["outlier_fraction"],
                   "gram_reused": [s["gram_reused"] for s in m.path_stats_],
                   "fit_s": [s["t_solve"] for s in m.path_stats_], "gram_s": [s["t_gram"] for s in m.path_stats_],
                   "start_s": [s["t_start"] for s in m.path_stats_], "rounds": [s["outer"] for s in m.path_stats_]}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--wsum", action="store_true")
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--cols", type=int, nargs="+", default=[20000, 60000])
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--samples", type=int, default=20000)
    ap.add_argument("--features", type=int, default=20)
    ap.add_argument("--gemm-features", type=int, default=128, help="d of the --wsum alternative's predict GEMM")
    ap.add_argument("--nu", type=float, default=0.1)
    ap.add_argument("--gamma", type=float, default=0.05)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    if a.wsum:
        lines += [wsum_probe(n, a.reps, a.gemm_features, a.gamma) for n in a.cols]
    if a.fit:
        lines.append(fit_probe(a.samples, a.features, a.nu, a.gamma, a.eps))
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
