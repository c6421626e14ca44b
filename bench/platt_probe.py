"""The Platt sigmoid fit on the device against the host path it replaces.

  fit   n = 60000 decisions x k = 10 machines (overlapping classes, resident in device memory as the solver's
        held-out buffer is): one platt_fit_kernel launch, event-timed, against downloading the decisions and
        k calls of platt_fit_cpu (plain C++ double, the same algorithm).
  e2e   the headline shape (mnist 60000 x 784, C = 10, gamma = 0.25): wall seconds of fit(probability=5)
        against fit + cross_val_decision + platt_fit_cpu on the host.

Fresh child processes, alternating the two arms --reps times; every child warms up, then reports its
median over --fits timed runs.  One JSON line (medians over the processes) appended to --out.

    python bench/platt_probe.py [--reps 3] [--fits 5] [--out profiles/platt/fit_probe.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(C=10.0, gamma=0.25, eps=1e-3, solver="ws", device="cuda")


def decisions(n, k, seed=0):
    rng = np.random.default_rng(seed)
    y = np.where(rng.random((k, n)) < 0.1, 1.0, -1.0).astype(np.float32)  # one-vs-rest: a tenth positive
    return (0.9 * y + 0.6 * rng.standard_normal((k, n))).astype(np.float32), y


def child_fit(a):
    sys.path.insert(0, HERE)
    from dpsvm_amd._native import load

    C = load()
    dec, y = decisions(a.n, a.k)
    out = {"arm": "fit", "n": a.n, "k": a.k}
    host = []
    if a.device == "cuda":
        import torch

        dd = torch.from_numpy(dec).cuda()
        torch.cuda.synchronize()
        ms = C.k_platt_fit_bench(dec, y, a.fits + 1)[1:]  # the first launch loads the code object
        out["device_fit_ms"] = float(np.median(ms))
        fits = C.k_platt_fit(dec, y)
    for _ in range(a.fits + 1):
        t0 = time.perf_counter()
        h = dd.cpu().numpy() if a.device == "cuda" else dec.copy()  # the download the host fit needs
        ref = [C.platt_fit_cpu(h[c], y[c]) for c in range(a.k)]
        host.append((time.perf_counter() - t0) * 1e3)
    out["host_download_and_fit_ms"] = float(np.median(host[1:]))
    out["host_iters"] = [r["iters"] for r in ref]
    if a.device == "cuda":
        out["max_abs_dA"] = max(abs(f["A"] - r["A"]) for f, r in zip(fits, ref))
        out["max_abs_dB"] = max(abs(f["B"] - r["B"]) for f, r in zip(fits, ref))
        out["device_iters"] = [f["iters"] for f in fits]
    print(json.dumps(out), flush=True)


def child_e2e(a):
    sys.path.insert(0, HERE)
    from dpsvm_amd._native import load
    from dpsvm_amd.models.svc import SVC
    from dpsvm_amd.utils.datasets import synthetic

    C = load()
    cfg = dict(CFG, device=a.device)
    X, y = synthetic("mnist", n=a.n, d=a.d, seed=0)
    SVC(**cfg).fit(X[:4096], y[:4096], probability=5)  # module load, first launches
    one, parts = [], []
    for _ in range(a.fits + 1):
        t0 = time.perf_counter()
        clf = SVC(**cfg).fit(X, y, probability=5)
        one.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ref = SVC(**cfg)
        ref.fit(X, y)
        dec = ref.cross_val_decision(X, y, cv=5, seed=0)
        fit = C.platt_fit_cpu(dec, ref._y_train)
        parts.append(time.perf_counter() - t0)
    print(json.dumps({"arm": "e2e", "n": a.n, "d": a.d, "fit_probability5_wall_s": float(np.median(one[1:])),
                      "fit_cv_hostfit_wall_s": float(np.median(parts[1:])),
                      "dA": clf.probA_ - fit["A"], "dB": clf.probB_ - fit["B"],
                      "same_decisions": bool(np.array_equal(clf.cv_decision_, dec)),
                      "platt_stats": clf.platt_stats_}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--d", type=int, default=784)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fits", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="", choices=["", "fit", "e2e"])
    ap.add_argument("--device", default="cuda", help="cpu: a rehearsal of the script at a small --n, not a measurement")
    a = ap.parse_args()
    if a.child:
        return child_fit(a) if a.child == "fit" else child_e2e(a)
    runs = {"fit": [], "e2e": []}
    for _ in range(a.reps):
        for arm in runs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", arm, "--n", str(a.n), "--d",
                                str(a.d), "--k", str(a.k), "--fits", str(a.fits), "--device", a.device],
                               capture_output=True, text=True, timeout=600, cwd=HERE)
            if r.returncode != 0:
                raise RuntimeError(f"{arm} child failed ({r.returncode}): {r.stderr[-2000:]}")
            runs[arm].append(json.loads(r.stdout.strip().splitlines()[-1]))
    med = lambda rs, key: float(np.median([r[key] for r in rs])) if key in rs[0] else None  # noqa: E731
    res = {"n": a.n, "d": a.d, "k": a.k, "reps": a.reps, "fits": a.fits, "device": a.device,
           "fit": {"device_fit_ms": med(runs["fit"], "device_fit_ms"),
                   "host_download_and_fit_ms": med(runs["fit"], "host_download_and_fit_ms"),
                   "per_process": runs["fit"]},
           "e2e": {"fit_probability5_wall_s": med(runs["e2e"], "fit_probability5_wall_s"),
                   "fit_cv_hostfit_wall_s": med(runs["e2e"], "fit_cv_hostfit_wall_s"), "per_process": runs["e2e"]}}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
