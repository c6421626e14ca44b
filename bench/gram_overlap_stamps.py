"""The adaptive Gram at the headline shape: event times of the whole call (both
passes and the per-call operand prep) and a checksum of the stored bits, the
figures profiles/gram_overlap/ and profiles/gram_tile256/ compare builds by.

No longer reported: the per-tile s_memtime stamps (compute wave: stage 0 landed
/ k loop / values / store issue; DMA wave: barrier and landing waits).  They
belonged to the stamped build of rbf_gemm_split_h1s_kernel, which went with
that kernel: the 256 x 256 one-product kernel (rbf_gemm_split_h1_kernel) has
no stamped build and no DMA waves.  profiles/gram_overlap/h1s_before.txt keeps
the last stamps taken.

    python bench/gram_overlap_stamps.py [--n 60000] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpsvm_amd._native import load  # noqa: E402
from dpsvm_amd.utils.datasets import synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tau", type=float, default=2.0 ** -22)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    C = load()
    X, _ = synthetic("mnist", n=a.n, seed=0)
    n, d = X.shape
    dp = (d + 15) // 16 * 16
    rows = (n + 255) // 256 * 256 + 512
    x = torch.zeros(rows, dp, device="cuda")
    x[:n, :d] = torch.from_numpy(X).cuda()
    s = torch.cuda.current_stream().cuda_stream
    xsq = torch.zeros(rows, device="cuda")
    C.k_row_sqnorm(x.data_ptr(), rows, dp, dp, xsq.data_ptr(), s)
    ld = (n + 127) // 128 * 128
    out = torch.full((n, ld), float("nan"), device="cuda")

    def gram():
        C.k_rbf_gram_split(x.data_ptr(), xsq.data_ptr(), n, x.data_ptr(), xsq.data_ptr(), n, dp, 0.25,
                           out.data_ptr(), ld, True, s, a.tau)

    gram()  # warm
    torch.cuda.synchronize()
    tiles, hot = C.k_gram_adapt_last()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gram()
        e1.record()
        torch.cuda.synchronize()
        ms.append(round(e0.elapsed_time(e1), 3))
    bits = out[:, :n].contiguous().view(torch.int32)
    checksum = int(bits.to(torch.int64).sum().item())
    nan = int(torch.isnan(out[:, :n]).sum().item())
    res = {"n": n, "tiles": tiles, "hot_tiles": hot, "adaptive_gram_ms": ms, "checksum": checksum, "nan": nan}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
