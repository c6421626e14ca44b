#!/usr/bin/env python3
"""Precomputed-kernel probes (docs/DESIGN.md §20), one JSON line each (profiles/precomputed/probes.jsonl).

  --dot    gram_rows_dot on a device-resident K(test, train) of (nt, n) = (20000, 20000) and (60000, 60000) for
           k = 1 and k = 10 machines, event-timed (median of --reps launches after two warm-ups): the bytes of Kt
           read once per group of 8 machines, the achieved rate beside the project's measured stream-read rate
           (6.0 TB/s, README), and torch.mv / torch.mm in fp32 on the same tensors.
  --fit    SVC(kernel="precomputed") on the RBF Gram of n x d synthetic rows (built with torch on the device,
           passed without a host copy) against the RBF fit of the same rows at solver="ws", ws_blocks=1,
           clip="box": solve time without the Gram, rounds and pair steps of each — the rounds differ by one add a
           pair step.

    python bench/precomputed_probe.py --dot --fit --out profiles/precomputed/probes.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

STREAM_READ_TBS = 6.0  # the project's measured stream-read rate (README: pass 1 at the stream roofline)


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


def dot_probe(nt: int, n: int, k: int, reps: int) -> dict:
    import torch

    from dpsvm_amd._native import load

    C = load()
    g = torch.Generator(device="cuda").manual_seed(nt + n + k)
    Kt = torch.rand((nt, n), dtype=torch.float32, device="cuda", generator=g)
    coef = torch.randn((k, n), dtype=torch.float32, device="cuda", generator=g)
    b = torch.zeros(k, dtype=torch.float32, device="cuda")
    out = torch.empty((nt, k), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def ours():
        C.k_gram_rows_dot_device(Kt.data_ptr(), nt, Kt.stride(0), n, coef.data_ptr(), coef.stride(0), k, b.data_ptr(),
                                 out.data_ptr(), k, stream)

    coef_t = coef.t().contiguous()
    ref_fn = (lambda: torch.mv(Kt, coef[0])) if k == 1 else (lambda: torch.mm(Kt, coef_t))
    us, us_ref = timed(ours, reps), timed(ref_fn, reps)
    ref = (Kt[:256].double() @ coef.double().t()).float()
    ours()
    err = float((out[:256] - ref).abs().max())
    passes = 1 if k == 1 else (k + 7) // 8
    byt = 4.0 * nt * n
    return {"probe": "gram_rows_dot", "nt": nt, "n": n, "k": k, "reps": reps, "us_median": float(np.median(us)),
            "us_min": float(us.min()), "kt_bytes": byt, "passes": passes,
            "gbs_kt_once": byt / (float(np.median(us)) * 1e-6) / 1e9,
            "gbs_read": passes * byt / (float(np.median(us)) * 1e-6) / 1e9, "stream_read_tbs": STREAM_READ_TBS,
            "torch": "mv" if k == 1 else "mm", "torch_us_median": float(np.median(us_ref)),
            "torch_gbs_kt_once": byt / (float(np.median(us_ref)) * 1e-6) / 1e9,
            "ratio_ours_over_torch": float(np.median(us) / np.median(us_ref)), "max_abs_err_vs_fp64_256rows": err}


def fit_probe(n: int, d: int, gamma: float, eps: float, C_: float) -> dict:
    import torch

    from dpsvm_amd import SVC
    from dpsvm_amd.utils.datasets import synthetic

    X, y = synthetic("blobs", n=n, d=d, seed=1, sep=2.0)
    Xd = torch.from_numpy(X).cuda()
    sq = (Xd * Xd).sum(1)
    dot = Xd @ Xd.t()
    d2 = (sq[:, None] + sq[None, :] - 2.0 * dot).clamp_(min=0)
    K = torch.exp(-gamma * 0.5 * (d2 + d2.t()))  # a + b commutes: bitwise symmetric
    K.fill_diagonal_(1.0)
    del dot, d2
    out = {"probe": "precomputed_fit", "n": n, "d": d, "gamma": gamma, "eps": eps, "C": C_}
    for rep in range(2):  # the first fits load the code objects
        pre = SVC(C=C_, eps=eps, kernel="precomputed", device="cuda").fit(K, y)
        rbf = SVC(C=C_, gamma=gamma, eps=eps, device="cuda", solver="ws", ws_blocks=1, clip="box",
                  ws_wss=pre.setup_info_["ws_wss"]).fit(X, y)
    for name, m in (("precomputed", pre), ("rbf", rbf)):
        st = m.stats_
        out[name] = {"solve_without_gram_s": st["t_solve"] - st["t_gram"], "gram_s": st["t_gram"],
                     "setup_s": m.setup_time_, "rounds": m.n_rounds_, "pair_steps": m.n_iter_,
                     "converged": m.converged_, "n_sv": m.n_support_, "b": m.b_, "ws_wss": m.setup_info_["ws_wss"],
                     "gram": m.setup_info_["gram"], "note": m.setup_info_["engine_note"]}
    out["train_accuracy"] = {"precomputed": pre.train_accuracy(), "rbf": rbf.train_accuracy()}
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dot", action="store_true")
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    lines = [dot_probe(n, n, k, a.reps) for n in (20000, 60000) for k in (1, 10)] if a.dot else []
    if a.fit:
        lines.append(fit_probe(20000, 20, 0.05, 1e-3, 1.0))
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
