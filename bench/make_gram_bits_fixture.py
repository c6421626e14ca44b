#!/usr/bin/env python3
"""tests/data/gram_onepass_bits.json: the adaptive split Gram's stored bits, recorded on the build BEFORE a
change to the one-product pass (rbf_gemm_split.hip) — the reference of tests/test_gram_tile256_gpu.py.

Per case: the sha256 of the adaptive Gram's bytes (row-major float32, the n or M x N values) and
gram_adapt_last()'s (tiles, hot).  The data is test_gram_adapt_gpu._data (MNIST-shape rows plus near-duplicates,
so some off-diagonal tiles are hot), np.resize'd to d columns as test_gram_overlap_gpu.py does; gamma 0.25,
tau 2^-22.  A rectangular case (M, N) is K(X[:M], X[:N]) of X = _data(max(M, N)).  The shapes sit where a
one-product tile's edges are: partial row and column tiles, an odd count of 128-column tiles, mirrored
tiles beside diagonal ones, odd and even k-block counts, and more tiles than workgroups.

Needs a GPU.  Run it on the parent build of the change under test:

    python bench/make_gram_bits_fixture.py [--out tests/data/gram_onepass_bits.json]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

GAMMA = 0.25
SYM = [(n, d) for n in (300, 600, 650, 700, 1100) for d in (160, 192, 224)] + [(6990, 160)]
RECT = [(700, 130, 160), (700, 300, 160), (300, 700, 160)]


def rows(n: int, d: int) -> np.ndarray:
    from test_gram_adapt_gpu import _data

    X = _data(n)
    if d != X.shape[1]:
        X = np.ascontiguousarray(np.resize(X, (n, d)))
    return X


def gram(K, a, b, tau):
    """(adaptive Gram of a [and b], tiles, hot); the output buffer starts NaN-filled (ops.kernels.rbf_gram)."""
    k = K.rbf_gram(a, b, GAMMA, split=True, cold_tau=tau)
    tiles, hot = K.gram_adapt_last()
    return k, int(tiles), int(hot)


def digest(k) -> str:
    return hashlib.sha256(np.ascontiguousarray(k.cpu().numpy()).tobytes()).hexdigest()


def main() -> int:
    import torch
    from test_gram_adapt_gpu import TAU

    from dpsvm_amd.ops import kernels as K

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "tests", "data", "gram_onepass_bits.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    out = {"gamma": GAMMA, "tau_log2": -22, "cases": []}
    for n, d in SYM:
        x = torch.from_numpy(rows(n, d)).cuda()
        k, tiles, hot = gram(K, x, None, TAU)
        out["cases"].append({"kind": "sym", "n": n, "d": d, "sha256": digest(k), "tiles": tiles, "hot": hot})
        print(out["cases"][-1], flush=True)
    for m, n, d in RECT:
        x = torch.from_numpy(rows(max(m, n), d)).cuda()
        k, tiles, hot = gram(K, x[:m].contiguous(), x[:n].contiguous(), TAU)
        out["cases"].append({"kind": "rect", "m": m, "n": n, "d": d, "sha256": digest(k), "tiles": tiles,
                             "hot": hot})
        print(out["cases"][-1], flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {os.path.normpath(a.out)} ({os.path.getsize(a.out)} bytes)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
