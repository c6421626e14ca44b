"""The multi-output decision GEMM (rbf_predict_multi_kernel) against k single-output
launches (rbf_predict_split_kernel, the kernel every binary prediction runs) at the
headline shape: 60000 queries x 60000 SVs x k = 10 columns, d = 784 and d = 128.  Both
sides include what a production call includes (operands split per launch, the reduce);
they alternate in one process, one event-timed launch each, after one warm-up each; the
report is the medians and their ratio.  One JSON line.

    python bench/predict_multi_probe.py [--n 60000] [--nsv 60000] [--k 10] [--d 784 128] [--reps 7]

--train: one-vs-rest training instead — the ten-class mnist-parity-shape problem (the
generator's ten prototypes recovered as labels: ten greedily picked far-apart rows, label =
nearest) fitted once as a multi-class SVC (one setup, one Gram) and as ten independent
binary fits in the same process: solve seconds, rounds per machine, the one t_gram.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpsvm_amd._native import load  # noqa: E402


def predict_shape(C, n, nsv, d, k, reps):
    dp = (d + 15) // 16 * 16
    g = torch.Generator(device="cuda").manual_seed(d)
    s = torch.cuda.current_stream().cuda_stream

    def padded(rows):
        pad = (rows + 127) // 128 * 128 + 128
        t = torch.zeros(pad, dp, device="cuda")
        t[:rows, :d] = torch.rand(rows, d, device="cuda", generator=g)
        sq = torch.zeros(pad, device="cuda")
        C.k_row_sqnorm(t.data_ptr(), pad, dp, dp, sq.data_ptr(), s)
        return t, sq

    x, xsq = padded(n)
    sv, svsq = padded(nsv)
    coef = torch.randn(nsv, k, device="cuda", generator=g)
    cols = torch.zeros(k, sv.shape[0], device="cuda")  # column c's coefficients, zero on the padding rows
    cols[:, :nsv] = coef.T
    b = torch.zeros(k, device="cuda")
    dec = torch.zeros(n, k, device="cuda")
    one = torch.zeros(n * k, device="cuda")
    torch.cuda.synchronize()

    def run(multi, out):
        return C.k_predict_multi_bench(x.data_ptr(), xsq.data_ptr(), n, dp, sv.data_ptr(), svsq.data_ptr(),
                                       coef.data_ptr(), cols.data_ptr(), cols.shape[1], k, nsv, 1.0 / d, b.data_ptr(),
                                       out.data_ptr(), multi, 1, s)[0]

    run(True, dec), run(False, one)  # warm-up
    t_multi, t_single = [], []
    for _ in range(reps):
        t_multi.append(run(True, dec))
        t_single.append(run(False, one))
    # the last single-output launch left column k - 1 in one[:n]
    diff = float((dec[:, k - 1] - one[:n]).abs().max())
    m, s1 = float(np.median(t_multi)), float(np.median(t_single))
    return {"d": d, "multi_ms": round(m, 3), "single_x_k_ms": round(s1, 3), "ratio": round(m / s1, 4),
            "multi_ms_all": [round(v, 3) for v in t_multi], "single_x_k_ms_all": [round(v, 3) for v in t_single],
            "max_abs_diff_last_column": diff}


def ten_class_labels(X):
    centres = [0]
    d0 = ((X - X[0]) ** 2).sum(1)
    near = d0.copy()
    while len(centres) < 10:
        i = int(np.argmax(near))  # the row farthest from every centre so far
        centres.append(i)
        near = np.minimum(near, ((X - X[i]) ** 2).sum(1))
    dist = np.stack([((X - X[i]) ** 2).sum(1) for i in centres], axis=1)
    return np.argmin(dist, axis=1).astype(np.int64)


def train(n, d):
    from dpsvm_amd.models.svc import SVC
    from dpsvm_amd.utils.datasets import synthetic

    X, _ = synthetic("mnist-parity", n=n, d=d, seed=0)
    y = ten_class_labels(X)
    cfg = dict(C=10.0, gamma=0.25, eps=1e-3, device="cuda", solver="ws")
    SVC(**cfg).fit(X[:4096], np.where(y[:4096] == y[0], 1, -1))  # warm-up: module load, first launches
    multi = SVC(**cfg).fit(X, y)
    binary = [SVC(**cfg).fit(X, np.where(y == c, 1, -1)) for c in multi.classes_]
    same = all(np.array_equal(multi.alpha_[c], one.alpha_) for c, one in enumerate(binary))
    return {"mode": "train", "n": n, "d": d, "k": int(len(multi.classes_)),
            "class_counts": np.bincount(y).tolist(),
            "multi_fit_s": round(multi.fit_time_, 6), "multi_wall_s": round(multi.wall_time_, 4),
            "multi_t_gram_s": [round(s["t_gram"], 6) for s in multi.stats_],
            "multi_t_solve_s": [round(s["t_solve"], 6) for s in multi.stats_],
            "multi_rounds": [int(s["outer"]) for s in multi.stats_],
            "multi_gram_reused": [bool(s["gram_reused"]) for s in multi.stats_],
            "binary_fit_s": round(sum(o.fit_time_ for o in binary), 6),
            "binary_wall_s": round(sum(o.wall_time_ for o in binary), 4),
            "binary_t_gram_s": [round(o.stats_["t_gram"], 6) for o in binary],
            "binary_t_solve_s": [round(o.stats_["t_solve"], 6) for o in binary],
            "binary_rounds": [int(o.stats_["outer"]) for o in binary],
            "alphas_bit_equal": bool(same), "train_accuracy": round(multi.train_accuracy(), 5),
            "n_support": int(multi.n_support_), "engine": multi.setup_info_["iteration"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--nsv", type=int, default=60000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--d", type=int, nargs="+", default=[784, 128])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.train:
        res = train(a.n, a.d[0])
    else:
        C = load()
        res = {"mode": "predict", "n": a.n, "nsv": a.nsv, "k": a.k, "reps": a.reps,
               "shapes": [predict_shape(C, a.n, a.nsv, d, a.k, a.reps) for d in a.d]}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
