#!/usr/bin/env python3
"""Named-kernel probes (docs/DESIGN.md §21), one JSON line each (profiles/named_kernels/probes.jsonl).

  --builder  the symmetric Gram of (0.05 x.y + 1)^3 at n x d = 20000 x 20 and 60000 x 784 (synthetic rows),
             event-timed, median of --reps after two warm-ups, three ways on the same device rows:
               dot      ops' k_dot_gram_split: the GEMM alone (its own event pair around each launch, split rows
                        prepared once) and the whole call (split rows + GEMM)
               rbf      the RBF Gram's whole call (split rows + GEMM) forced onto its Glds path (variant 3: the same
                        tiling and ring, so the epilogue is what differs), and on the path it takes by default
               torch    X @ X.T in fp32, the elementwise epilogue in place, and the symmetrisation 0.5 (K + K.T)
  --fit      SVC(kernel=Poly(3, 1.0)).fit on 20000 x 20 blobs against kernel="precomputed" on the torch-built Gram
             of the same rows: wall time (the torch build included), peak memory (torch.cuda.max_memory_allocated
             plus the solver's bytes_device), rounds and pair steps (max_iter raised to 5,000,000 pair steps).
  --tanh     the device tanhf inside the sigmoid epilogue against float64 tanh of the same float32 u, in ulp, over
             the values of tests/test_dot_gemm_gpu.py's shapes.

    python bench/named_kernels_probe.py --builder --fit --tanh --out profiles/named_kernels/probes.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn, reps: int) -> np.ndarray:
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(reps + 2):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    return np.array(us[2:])  # the first launches load the code


def stats(us) -> dict:
    us = np.asarray(us, dtype=np.float64)
    return {"us_median": float(np.median(us)), "us_min": float(us.min()), "us_max": float(us.max())}


def builder_probe(n: int, d: int, data: str, reps: int) -> dict:
    import torch

    from dpsvm_amd import Poly
    from dpsvm_amd._native import load
    from dpsvm_amd.utils.datasets import synthetic

    C = load()
    spec, gamma = Poly(3, 1.0), 0.05
    X, _ = synthetic(data, n=n, d=d, seed=1)
    n, d = X.shape
    s = torch.cuda.current_stream().cuda_stream
    x = torch.from_numpy(X).cuda()
    ld = (n + 127) // 128 * 128
    out = torch.empty((n, ld), device="cuda")
    kind, degree, coef0 = spec.native()

    def dot(reps_=0):
        return C.k_dot_gram_split(x.data_ptr(), n, x.data_ptr(), n, d, d, d, kind, degree, coef0, gamma,
                                  out.data_ptr(), ld, True, s, reps_)

    dot()
    dot()
    gemm_us = dot(reps)
    whole_us = timed(dot, reps)
    sub = np.random.default_rng(0).choice(n, 512, replace=False)
    got = out[torch.from_numpy(sub).cuda()][:, :n].double().cpu().numpy()
    ref = (gamma * (X[sub].astype(np.float64) @ X.astype(np.float64).T) + 1.0) ** 3
    rel = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))  # (u^3 crosses 0: no per-element relative error)
    # the RBF Gram of the same rows (its operands padded as ops.rbf_gram pads them)
    dp = (d + 15) // 16 * 16
    rows = (n + 255) // 256 * 256 + 512
    xp = torch.zeros(rows, dp, device="cuda")
    xp[:n, :d] = x
    xsq = torch.zeros(rows, device="cuda")
    C.k_row_sqnorm(xp.data_ptr(), rows, dp, dp, xsq.data_ptr(), s)

    def rbf():
        C.k_rbf_gram_split(xp.data_ptr(), xsq.data_ptr(), n, xp.data_ptr(), xsq.data_ptr(), n, dp, gamma,
                           out.data_ptr(), ld, True, s)

    res = {"probe": "builder", "n": n, "d": d, "data": data, "reps": reps, "kernel": "poly 3 coef0 1 gamma 0.05",
           "dot_gemm": stats(gemm_us), "dot_whole": stats(whole_us), "max_abs_err_over_max_abs_value_vs_fp64_512rows": rel}
    keep = C.k_split_gemm_variant()
    try:
        C.k_set_split_gemm_variant(3)
        res["rbf_glds_path"] = C.k_split_gram_path(n, n, dp, ld, True, False)
        res["rbf_glds_whole"] = stats(timed(rbf, reps))
        C.k_set_split_gemm_variant(0)
        res["rbf_default_path"] = C.k_split_gram_path(n, n, dp, ld, True, False)
        res["rbf_default_whole"] = stats(timed(rbf, reps))
    finally:
        C.k_set_split_gemm_variant(keep)
    del xp

    def torch_gram():
        K = x @ x.t()
        K.mul_(gamma).add_(1.0)
        K.pow_(3)
        return (K + K.t()).mul_(0.5)

    res["torch"] = stats(timed(torch_gram, reps))
    return res


def fit_probe(n: int, d: int, reps: int = 2) -> dict:
    import torch

    from dpsvm_amd import SVC, Poly
    from dpsvm_amd.utils.datasets import synthetic

    spec, gamma, C_, max_iter = Poly(3, 1.0), 0.05, 1.0, 5000000  # (150,000 pair steps do not close the gap here)
    X, y = synthetic("blobs", n=n, d=d, seed=1, sep=2.0)
    out = {"probe": "poly_fit", "n": n, "d": d, "gamma": gamma, "C": C_, "kernel": "poly 3 coef0 1",
           "max_iter": max_iter}

    def run(named: bool):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        if named:
            m = SVC(C=C_, gamma=gamma, kernel=spec, device="cuda", max_iter=max_iter).fit(X, y)
        else:
            Xd = torch.from_numpy(X).cuda()
            K = Xd @ Xd.t()
            K.mul_(gamma).add_(1.0)
            K.pow_(3)
            K = (K + K.t()).mul_(0.5)
            m = SVC(C=C_, kernel="precomputed", device="cuda", max_iter=max_iter).fit(K, y)
        wall = time.perf_counter() - t0
        st = m.stats_
        return {"wall_s": wall, "torch_peak_bytes": int(torch.cuda.max_memory_allocated() - base),
                "bytes_device": int(m.setup_info_["bytes_device"]),
                "peak_bytes": int(torch.cuda.max_memory_allocated() - base) + int(m.setup_info_["bytes_device"]),
                "t_gram_build_s": m.setup_info_.get("t_gram_build", 0.0), "setup_s": m.setup_time_,
                "solve_s": st["t_solve"], "rounds": int(m.n_rounds_), "pair_steps": int(m.n_iter_),
                "converged": bool(m.converged_), "n_sv": int(m.n_support_), "b": float(m.b_),
                "train_accuracy": m.train_accuracy()}

    for rep in range(reps):  # the first fits load the code objects
        out["named"] = run(True)
        out["precomputed_torch"] = run(False)
    out["gram_bytes"] = 4 * n * ((n + 127) // 128 * 128)
    return out


def tanh_probe() -> dict:
    import torch

    from dpsvm_amd import Linear, Sigmoid
    from dpsvm_amd.ops import kernels as ops

    worst, count = 0.0, 0
    gamma, c0 = np.float32(0.1), np.float32(0.25)
    for n, d, seed in ((130, 20, 120), (130, 200, 300), (300, 200, 500), (257, 100, 1899)):
        x = torch.from_numpy(np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)).cuda()
        L = ops.kernel_gram(x, None, kernel=Linear()).cpu().numpy().astype(np.float64)
        K = ops.kernel_gram(x, None, kernel=Sigmoid(float(c0)), gamma=float(gamma)).cpu().numpy()
        u = (float(gamma) * L + float(c0)).astype(np.float32).astype(np.float64)  # the fma's single rounding
        t = np.tanh(u)
        ulp = np.abs(K.astype(np.float64) - t) / np.spacing(np.abs(t).astype(np.float32)).astype(np.float64)
        worst, count = max(worst, float(ulp.max())), count + ulp.size
    return {"probe": "device_tanhf", "values": count, "max_ulp_vs_fp64_tanh_of_f32_u": worst,
            "bound_used_by_the_tests_ulp": 5}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--builder", action="store_true")
    ap.add_argument("--big", action="store_true", help="--builder: also 60000 x 784")
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--tanh", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()

    def emit(ln):
        print(json.dumps(ln), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(ln) + "\n")

    if a.tanh:
        emit(tanh_probe())
    if a.builder:
        emit(builder_probe(20000, 20, "blobs", a.reps))
        if a.big:
            emit(builder_probe(60000, 784, "mnist", a.reps))
    if a.fit:
        emit(fit_probe(20000, 20))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
