"""Where a tile of the one-product Gram pass (rbf_gemm_split_h1s_kernel) spends
its time, on both kinds of wave: the stamped build of the kernel
(C.k_set_gram_stamps, 16 words a tile) records, for a workgroup's first
compute wave, s_memtime at the tile's start / stage 0 landed / k loop done /
values done / stores issued, and for its first DMA wave the cycles spent at the
barrier of the tile's stage 0 (waiting out the previous tile's epilogue), at
the other stages' barriers, waiting for its own DMA to land, and in all.

Also times the unstamped adaptive Gram (events, both passes and the per-call
operand prep) and prints a checksum of the stored bits.

    python bench/gram_overlap_stamps.py [--n 60000] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
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
    stamps = torch.zeros(tiles * 16, dtype=torch.int64, device="cuda")
    C.k_set_gram_stamps(stamps.data_ptr())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    gram()
    e1.record()
    torch.cuda.synchronize()
    C.k_set_gram_stamps(0)
    st = stamps.view(-1, 16).cpu().numpy().astype(np.int64)
    cw = (np.diff(st[:, :5], axis=1) & 0xffffffff)  # low words: differences mod 2^32
    first, loop, values, store = cw.T
    tile_us = ((st[:, 6] - st[:, 5]) & 0xffffffff) / 100.0
    clk = float(np.median((first + loop + values + store) / np.maximum(tile_us, 1e-9)))  # cycles per us
    bar0, bar, land, total = st[:, 8], st[:, 9], st[:, 10], st[:, 11]
    G = 256
    later = np.arange(len(st)) >= G  # a workgroup's tiles after its first (whose stage-0 wait is the prologue)
    med = lambda v: float(np.median(v))  # noqa: E731
    res = {
        "n": n, "tiles": tiles, "hot_tiles": hot,
        "adaptive_gram_ms_unstamped": ms, "adaptive_gram_ms_stamped": round(e0.elapsed_time(e1), 3),
        "checksum": checksum, "nan": nan, "memtime_cycles_per_us": round(clk, 1),
        "compute_wave_cycles_median": {"stage0_wait": med(first[later]), "k_loop_rest": med(loop[later]),
                                       "values": med(values[later]), "store_issue": med(store[later]),
                                       "tile": med((first + loop + values + store)[later])},
        "compute_wave_epilogue_share": round(med((values + store)[later]) /
                                             med((first + loop + values + store)[later]), 3),
        "dma_wave_cycles_median": {"barrier_stage0": med(bar0[later]), "barrier_other_stages": med(bar[later]),
                                   "own_dma_landing": med(land[later]), "tile": med(total[later])},
        "dma_wave_blocked_at_stage0_share": round(med(bar0[later]) / med(total[later]), 3),
        "tile_us_median": med(tile_us[later]),
    }
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
