"""Per-row C (sample weights) at the headline shape, mnist 60000 x 784, C = 10, gamma = 0.25.

  --mode ones   sample_weight = ones against no weights.  Fresh child processes, alternating
                [baseline tree, no weights | this tree, no weights | this tree, ones] --reps times; every
                child warms up, then runs --fits timed fits and reports each t_solve with the trajectory
                (pair steps, rounds, a digest of alpha).  --baseline-tree: a built checkout of the commit
                to compare against (omit: this tree only).  The three must run one trajectory.
  --mode cv     5-fold SVC.cross_val_decision (one setup, one Gram, set_row_C per fold, decisions from the
                gradient) against five fits on X[train] plus five decision_function(X[fold]) calls, solver
                "ws" on both sides, alternating --reps times in one process: wall seconds, the sums of
                t_solve, and the largest difference of the out-of-fold decisions.

    python bench/weights_probe.py --mode ones [--baseline-tree PATH] [--reps 3] [--fits 5] [--out FILE]
    python bench/weights_probe.py --mode cv [--reps 3] [--out FILE]

One JSON line per run (appended to --out).
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(C=10.0, gamma=0.25, eps=1e-3, device="cuda")


def child(tree, weights, n, d, fits, device):
    CFG["device"] = device
    sys.path.insert(0, tree)
    from dpsvm_amd.models.svc import SVC
    from dpsvm_amd.utils.datasets import synthetic

    X, y = synthetic("mnist", n=n, d=d, seed=0)
    kw = {"sample_weight": np.ones(n)} if weights == "ones" else {}
    kw_warm = {"sample_weight": np.ones(4096)} if weights == "ones" else {}
    SVC(solver="ws", **CFG).fit(X[:4096], y[:4096], **kw_warm)  # module load, first launches
    SVC(**CFG).fit(X, y, **kw)  # the timed shape once
    runs = [SVC(**CFG).fit(X, y, **kw) for _ in range(fits)]
    c = runs[-1]
    info = getattr(c, "setup_info_", {"iteration": "cpu"})  # the CPU rehearsal has no device setup
    print(json.dumps({"tree": tree, "weights": weights, "t_solve_s": [round(r.fit_time_, 6) for r in runs],
                      "t_gram_s": [round(r.stats_["t_gram"], 6) for r in runs],
                      "n_iter": int(c.n_iter_), "n_rounds": int(c.n_rounds_), "engine": info["iteration"],
                      "engine_note": info.get("engine_note", ""),
                      "alpha_sha256": hashlib.sha256(np.ascontiguousarray(c.alpha_).tobytes()).hexdigest()[:16],
                      "b": float(c.b_)}), flush=True)


def mode_ones(a):
    arms = ([("baseline", a.baseline_tree, "none")] if a.baseline_tree else []) + [("new", HERE, "none"),
                                                                                   ("new-ones", HERE, "ones")]
    runs = {k: [] for k, _, _ in arms}
    for _ in range(a.reps):
        for name, tree, weights in arms:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--weights", weights,
                                "--n", str(a.n), "--d", str(a.d), "--fits", str(a.fits), "--device", a.device],
                               capture_output=True,
                               text=True, timeout=600, cwd=tree)
            if r.returncode != 0:
                raise RuntimeError(f"{name} child failed ({r.returncode}): {r.stderr[-2000:]}")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    res = {"mode": "ones", "n": a.n, "d": a.d, "reps": a.reps, "fits": a.fits, **CFG}
    for name, rs in runs.items():
        ts = [t for r in rs for t in r["t_solve_s"]]
        res[name] = {"t_solve_median_s": round(float(np.median(ts)), 6), "t_solve_min_s": min(ts),
                     "t_solve_max_s": max(ts), "per_process_median_s": [float(np.median(r["t_solve_s"])) for r in rs],
                     "n_iter": rs[0]["n_iter"], "n_rounds": rs[0]["n_rounds"], "alpha_sha256": rs[0]["alpha_sha256"],
                     "engine": rs[0]["engine"], "engine_note": rs[0]["engine_note"]}
    res["same_trajectory"] = len({(v["n_iter"], v["n_rounds"], v["alpha_sha256"]) for k, v in res.items()
                                  if isinstance(v, dict)}) == 1
    return res


def mode_cv(a):
    sys.path.insert(0, HERE)
    from dpsvm_amd.models.svc import SVC
    from dpsvm_amd.utils.datasets import synthetic

    X, y = synthetic("mnist", n=a.n, d=a.d, seed=0)
    cfg = dict(solver="ws", **CFG)
    SVC(**cfg).fit(X[:4096], y[:4096])  # module load, first launches
    folds = SVC.cv_folds(a.n, 5, 0)
    one, sub = [], []
    for _ in range(a.reps):
        clf = SVC(**cfg)
        t0 = time.perf_counter()
        dec = clf.cross_val_decision(X, y, cv=5, seed=0)
        one.append({"wall_s": time.perf_counter() - t0, "t_solve_s": sum(s["t_solve"] for s in clf.cv_stats_),
                    "t_gram_s": sum(s["t_gram"] for s in clf.cv_stats_),
                    "gram_reused": [bool(s["gram_reused"]) for s in clf.cv_stats_]})
        t0 = time.perf_counter()
        ref = np.zeros(a.n, dtype=np.float32)
        ts = tg = 0.0
        for fold in folds:
            tr = np.setdiff1d(np.arange(a.n), fold)
            m = SVC(**cfg).fit(X[tr], y[tr])
            ref[fold] = m.decision_function(X[fold])
            ts += m.fit_time_
            tg += m.stats_["t_gram"]
        sub.append({"wall_s": time.perf_counter() - t0, "t_solve_s": ts, "t_gram_s": tg})
    med = lambda rs, k: round(float(np.median([r[k] for r in rs])), 6)  # noqa: E731
    return {"mode": "cv", "n": a.n, "d": a.d, "reps": a.reps, "cv": 5, **cfg,
            "one_gram": {"wall_median_s": med(one, "wall_s"), "t_solve_sum_median_s": med(one, "t_solve_s"),
                         "t_gram_sum_median_s": med(one, "t_gram_s"), "gram_reused": one[0]["gram_reused"],
                         "wall_s": [round(r["wall_s"], 4) for r in one]},
            "subset_fits": {"wall_median_s": med(sub, "wall_s"), "t_solve_sum_median_s": med(sub, "t_solve_s"),
                            "t_gram_sum_median_s": med(sub, "t_gram_s"), "wall_s": [round(r["wall_s"], 4) for r in sub]},
            "max_abs_decision_diff": float(np.max(np.abs(dec - ref))),
            "accuracy": [float(np.mean(np.where(v < 0, -1.0, 1.0) == y)) for v in (dec, ref)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["ones", "cv"], default="ones")
    ap.add_argument("--baseline-tree", default="")
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--d", type=int, default=784)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fits", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--weights", default="none")
    ap.add_argument("--device", default="cuda", help="cpu: a rehearsal of the script at a small --n, not a measurement")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.weights, a.n, a.d, a.fits, a.device)
    CFG["device"] = a.device
    if a.baseline_tree:
        a.baseline_tree = os.path.abspath(a.baseline_tree)
    res = mode_ones(a) if a.mode == "ones" else mode_cv(a)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
