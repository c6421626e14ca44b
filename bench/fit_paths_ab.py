#!/usr/bin/env python3
"""A/B digests of the model layer: every fit path's published attributes and predictions, as SHA-256.

  python bench/fit_paths_ab.py --device cpu|cuda [--out FILE] [--detail]

Runs the matrix 3 kernels (rbf, precomputed, Poly) x binary / one-vs-rest x weights x probability 0 / 3 on SVC,
plus SVR and OneClassSVM per kernel (30 fits, n = 96, d = 6, clip="box"), and prints one JSON line per case:

  attrs     {name: digest} of every public fitted attribute (``name_``): arrays (and lists of arrays) as
            "dtype shape sha256(bytes)", scalars / None by repr, dicts and lists of dicts by their sorted keys;
            the time fields are left out
  predict   digests of decision_function / predict (/ predict_proba) on 200 seeded test rows, train_accuracy()
            and, where the kernel has a model file, of the saved file's bytes and the loaded model's predictions
  params    sha256 of get_params() and of SVCConfig.to_native(d).to_json() for the case's config

and a first line for the default config's native params.  Each group is printed as one SHA-256 over its sorted
entries; ``--detail`` prints the entries themselves, to find the attribute behind a differing line.  Two builds
given the same device print the same lines when the model layer computes the same thing: CPU fits repeat bitwise,
and the GPU solves are deterministic.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, D, NT = 96, 6, 200
TIMES = ("fit_time_", "setup_time_", "wall_time_", "cv_wall_time_")


def sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def digest(v) -> str:
    if isinstance(v, np.ndarray):
        return f"{v.dtype} {v.shape} {sha(np.ascontiguousarray(v).tobytes())}"
    if isinstance(v, dict):
        return "dict " + ",".join(sorted(v))
    if isinstance(v, (list, tuple)) and v and all(isinstance(e, np.ndarray) for e in v):
        return f"{type(v).__name__}[{len(v)}] " + sha(b"".join(digest(e).encode() for e in v))
    if isinstance(v, (list, tuple)) and v and all(isinstance(e, dict) for e in v):
        return f"{type(v).__name__}[{len(v)}] of " + digest(v[0])
    if isinstance(v, (list, tuple)) and v and all(isinstance(e, (list, tuple)) for e in v):
        return f"{type(v).__name__}[{len(v)}] of " + digest(v[0])
    return f"{type(v).__name__} {v!r}"


def data():
    rng = np.random.default_rng(7)
    X = rng.standard_normal((N, D)).astype(np.float32)
    Xt = rng.standard_normal((NT, D)).astype(np.float32)
    w = rng.standard_normal(D)
    y2 = np.where(X @ w + 0.3 * rng.standard_normal(N) > 0, 1.0, -1.0).astype(np.float32)
    y3 = np.digitize(X @ w, [-0.8, 0.8]).astype(np.int64)  # three classes, all present
    assert set(y2.tolist()) == {-1.0, 1.0} and set(y3.tolist()) == {0, 1, 2}
    z = (np.sin(X @ w) + 0.1 * rng.standard_normal(N)).astype(np.float32)
    sw = rng.uniform(0.5, 2.0, N)
    K = X.astype(np.float64) @ X.astype(np.float64).T
    K = (0.5 * (K + K.T)).astype(np.float32)
    K = np.ascontiguousarray(np.triu(K) + np.triu(K, 1).T)  # symmetric bitwise
    Kt = np.ascontiguousarray((Xt.astype(np.float64) @ X.astype(np.float64).T).astype(np.float32))
    return dict(X=X, Xt=Xt, y2=y2, y3=y3, z=z, sw=sw, K=K, Kt=Kt)


def kernels():
    from dpsvm_amd import Poly

    return {"rbf": "rbf", "precomputed": "precomputed", "poly": Poly(2, 1.0)}


def cases():
    for kname in ("rbf", "precomputed", "poly"):
        for multi in (False, True):
            for weights in (False, True):
                for prob in (0, 3):
                    yield ("svc", kname, multi, weights, prob)
        yield ("svr", kname, False, False, 0)
        yield ("oneclass", kname, False, False, 0)


def attrs_of(est) -> dict:
    return {k: digest(v) for k, v in sorted(vars(est).items())
            if k.endswith("_") and not k.startswith("_") and k not in TIMES}


def run_case(case, dat, device: str, tmp: str) -> dict:
    from dpsvm_amd import SVC, SVR, OneClassSVM, SVCConfig, load_model, load_one_class, load_svr

    kind, kname, multi, weights, prob = case
    kernel = kernels()[kname]
    train, test = (dat["K"], dat["Kt"]) if kname == "precomputed" else (dat["X"], dat["Xt"])
    kw = dict(gamma=0.5, eps=1e-3, device=device, clip="box", kernel=kernel)
    pred = {}
    if kind == "svc":
        kw["C"] = 2.0
        est = SVC(**kw)
        est.fit(train, dat["y3"] if multi else dat["y2"], sample_weight=dat["sw"] if weights else None,
                probability=prob)
        pred["decision_function"] = digest(est.decision_function(test))
        pred["predict"] = digest(np.asarray(est.predict(test)))
        if prob:
            pred["predict_proba"] = digest(est.predict_proba(test))
        pred["train_accuracy"] = repr(est.train_accuracy())
        loader = load_model
    elif kind == "svr":
        kw["C"] = 2.0
        est = SVR(epsilon=0.05, **kw)
        est.fit(train, dat["z"])
        pred["predict"] = digest(est.predict(test))
        loader = load_svr
    else:
        est = OneClassSVM(nu=0.3, **kw)
        est.fit(train)
        pred["decision_function"] = digest(est.decision_function(test))
        pred["score_samples"] = digest(est.score_samples(test))
        path = est.nu_path(train, [0.2, 0.4])
        pred["nu_path"] = sha(json.dumps(path, sort_keys=True).encode())
        loader = load_one_class
    if kname != "precomputed":  # a model file: its bytes, and the loaded model's predictions
        path = os.path.join(tmp, "m.txt")
        for side in (path, path + ".platt"):
            if os.path.exists(side):
                os.remove(side)
        est.save(path)
        with open(path, "rb") as f:
            pred["file"] = sha(f.read())
        if os.path.exists(path + ".platt"):
            with open(path + ".platt", "rb") as f:
                pred["platt_file"] = sha(f.read())
        lm = loader(path, device)
        pred["loaded"] = digest(np.asarray(lm.decision_function(test)))
        if prob:
            pred["loaded_proba"] = digest(lm.predict_proba(test))
    cfg_kw = {k: v for k, v in kw.items()}
    params = {
        "get_params": sha(json.dumps(est.get_params(), sort_keys=True, default=str).encode()),
        "to_native": sha(SVCConfig(**cfg_kw).to_native(D).to_json().encode()),
        "fitted_to_native": sha(est.config.to_native(D).to_json().encode()),
    }
    name = f"{kind}-{kname}-{'ovr' if multi else 'bin'}-{'w' if weights else 'u'}-p{prob}"
    return {"case": name, "attrs": attrs_of(est), "predict": pred, "params": params}


def compact(rec: dict) -> dict:
    """each group of a case's record as one digest over its sorted entries"""
    return {k: v if isinstance(v, str) else sha(json.dumps(v, sort_keys=True).encode()) for k, v in rec.items()}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--out", default=None)
    ap.add_argument("--detail", action="store_true", help="every entry's digest instead of one per group")
    a = ap.parse_args()
    from dpsvm_amd import SVCConfig

    lines = [json.dumps({"case": "default-config", "to_native": sha(SVCConfig().to_native(D).to_json().encode())},
                        sort_keys=True)]
    dat = data()
    with tempfile.TemporaryDirectory() as tmp:
        for case in cases():
            rec = run_case(case, dat, a.device, tmp)
            lines.append(json.dumps(rec if a.detail else compact(rec), sort_keys=True))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
