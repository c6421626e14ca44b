"""The timed paths of the kernel probes (reps > 0; the tables of bench/ are built on them): each of the seven
timed entries returns one finite, positive time per repetition, and the repetitions leave what the entry returns as
the untimed call does — bit for bit where the repeated launch only reads its inputs.  The one-block ws_select
updates f on every repetition, on rotated apply lines: there the count, and that the returned launch runs on the
caller's lines again.  Shapes are the smallest of the entries' own tests; no bound on a time is asserted."""
import numpy as np
import pytest
import torch

import test_ws_kernels_gpu as W
from test_ws_kernels_gpu import K  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

REPS = 3


def check_times(t):
    t = np.asarray(list(t), np.float64)
    assert t.shape == (REPS,) and np.all(np.isfinite(t)) and np.all(t > 0), t


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_gram_rows_wsum_reps(K):  # noqa: F811
    rng = np.random.default_rng(1)
    n, ldg, L, m = 1025, 1028, 20, 30  # n % 4 == 1, duplicate lines
    gram = rng.random(size=(L, ldg), dtype=np.float32)
    coef = rng.standard_normal(m).astype(np.float32)
    lines = rng.integers(0, L, size=m).astype(np.int32)
    base = rng.standard_normal(n).astype(np.float32)
    once = K.gram_rows_wsum(gram, n, coef, lines=lines, base=base)
    timed = K.gram_rows_wsum(gram, n, coef, lines=lines, base=base, reps=REPS)
    check_times(timed["us"])
    assert once["us"] == [] and timed["S"] == once["S"]
    same_bits(timed["out"], once["out"])
    same_bits(timed["pad"], once["pad"])


def test_gram_rows_dot_reps(K):  # noqa: F811
    rng = np.random.default_rng(2)
    nt, n, k, ld = 5, 1025, 3, 1032
    Kt = np.full((nt, ld), np.nan, np.float32)
    Kt[:, :n] = rng.standard_normal((nt, n)).astype(np.float32)
    coef = np.full((k, ld), np.nan, np.float32)
    coef[:, :n] = rng.standard_normal((k, n)).astype(np.float32)
    b = rng.standard_normal(k).astype(np.float32)
    once = K.gram_rows_dot(Kt, n, coef, b)
    timed = K.gram_rows_dot(Kt, n, coef, b, reps=REPS)
    check_times(timed["us"])
    assert once["us"] == []
    same_bits(timed["out"], once["out"])
    same_bits(timed["pad"], once["pad"])


@pytest.mark.parametrize("sym", [True, False])
def test_kernel_gram_reps(K, sym):  # noqa: F811
    from dpsvm_amd import Poly

    g = torch.Generator(device="cuda").manual_seed(3)
    a = torch.rand(130, 20, device="cuda", generator=g)
    b = None if sym else torch.rand(70, 20, device="cuda", generator=g)
    once = K.kernel_gram(a, b, kernel=Poly(3, 1.0), gamma=0.1)
    timed, us = K.kernel_gram(a, b, kernel=Poly(3, 1.0), gamma=0.1, reps=REPS)
    check_times(us)
    assert torch.equal(timed, once)


def test_ws_select_pass1_reps(K):  # noqa: F811
    """blocks > 1: the repeated launch is pass 1, which only reads the state"""
    rng = np.random.default_rng(4)
    n, ldg, C, nab = 1027, 1028, 2.0, [40] * 4  # two column groups, the last 3 columns wide
    gram, f, a_new, y, dal, ch = W.select_state(rng, n, C, sum(nab))
    gram = np.concatenate([gram, np.full((n, ldg - n), np.nan, np.float32)], axis=1)
    coef = (dal.astype(np.float64) * y)[ch].astype(np.float32)
    once = K.ws_select(gram, f, a_new, y, dal, ch, coef, nab, C, q_max=96)
    timed = K.ws_select(gram, f, a_new, y, dal, ch, coef, nab, C, q_max=96, reps=REPS)
    check_times(timed["pass1_us"])
    assert once["pass1_us"] == [] and timed["select_us"] == [] and set(timed) == set(once)
    for key in sorted(set(once) - {"pass1_us"}):
        same_bits(timed[key], once[key])


def test_ws_select_one_block_reps(K):  # noqa: F811
    """blocks == 1: repetition i runs on the lines apply_lines + (i mod (L // na)) na and updates f; the launch
    whose state is returned runs on the caller's lines again.  With L = 3 na lines of distinct values, f after
    three repetitions and the returned launch is f + (2 G0 + G1 + G2)' coef, Gi the rows apply_lines + i na; lines
    left rotated would give G0 + G1 + 2 G2.  Bound: four passes, each at most na + 1 additions per column in
    float32 on partial sums no larger than |f| + 4 sum |coef| (0 <= gram < 1)."""
    rng = np.random.default_rng(5)
    n, na, C = 1027, 8, 1.0
    L = 3 * na
    gram = rng.random(size=(L, n), dtype=np.float32)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(np.float32)
    alpha = np.zeros(n, np.float32)
    f = rng.standard_normal(n).astype(np.float32)
    lines = np.arange(na, dtype=np.int32)
    coef = rng.normal(scale=0.2, size=na).astype(np.float32)
    args = (gram, f, alpha, y, np.zeros(n, np.float32), lines, coef, [na], C)
    fresh = K.ws_select(*args)
    timed = K.ws_select(*args, reps=REPS)
    check_times(timed["select_us"])
    assert timed["pass1_us"] == [] and fresh["select_us"] == []
    g64, c64 = gram.astype(np.float64), coef.astype(np.float64)
    rows = [c64 @ g64[i * na:(i + 1) * na] for i in range(3)]
    want = f.astype(np.float64) + 2 * rows[0] + rows[1] + rows[2]
    bound = 4 * (na + 1) * 2.0 ** -24 * (np.abs(f).max() + 4 * np.abs(c64).sum())
    err = np.abs(timed["f"].astype(np.float64) - want).max()
    rotated = np.abs(rows[0] - rows[2]).max()
    print(f"one-block reps: max |f - model| = {err:.3e}, bound {bound:.3e}, lines left rotated would miss by "
          f"{rotated:.3e}")
    assert rotated > 100 * bound and err <= bound
    again = K.ws_select(*args)
    for key in sorted(set(fresh) - {"select_us", "pass1_us"}):
        same_bits(again[key], fresh[key])


def test_predict_multi_bench_reps(K):  # noqa: F811
    from dpsvm_amd._native import load

    C = load()
    n, nsv, d, k = 130, 129, 128, 3  # row and SV tile edges, the multi-output split path
    g = torch.Generator(device="cuda").manual_seed(6)
    x = torch.rand(n, d, device="cuda", generator=g)
    sv = torch.rand(nsv, d, device="cuda", generator=g)
    coef = torch.randn(nsv, k, device="cuda", generator=g).contiguous()
    b = torch.randn(k, device="cuda", generator=g)
    want = K.rbf_decision_multi(x, sv, coef, 1.0 / d, b)
    s = torch.cuda.current_stream().cuda_stream
    xp, dp = K._pad_rows_cols(x)
    svp, _ = K._pad_rows_cols(sv)
    xsq = torch.zeros(xp.shape[0], device="cuda")
    svsq = torch.zeros(svp.shape[0], device="cuda")
    C.k_row_sqnorm(xp.data_ptr(), xp.shape[0], dp, dp, xsq.data_ptr(), s)
    C.k_row_sqnorm(svp.data_ptr(), svp.shape[0], dp, dp, svsq.data_ptr(), s)
    cols = torch.zeros(k, svp.shape[0], device="cuda")  # column c's coefficients, zero on the padding rows
    cols[:, :nsv] = coef.T
    dec = torch.zeros(n, k, device="cuda")
    ms = C.k_predict_multi_bench(xp.data_ptr(), xsq.data_ptr(), n, dp, svp.data_ptr(), svsq.data_ptr(),
                                 coef.data_ptr(), cols.data_ptr(), cols.shape[1], k, nsv, 1.0 / d, b.data_ptr(),
                                 dec.data_ptr(), True, REPS, s)
    torch.cuda.synchronize()
    check_times(ms)
    assert torch.equal(dec, want)


def test_rows_split_bench_reps(K):  # noqa: F811
    from dpsvm_amd._native import load

    C = load()
    n, d, gamma = 700, 20, 0.05
    rows = [3, 699, 0, 128, 511]
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.rand(n, d, device="cuda", generator=g)
    want = K.rbf_rows_indexed(x, rows, gamma, split=True)
    s = torch.cuda.current_stream().cuda_stream
    xp, dp = K._pad_rows_cols(x, row_mult=512)  # as rbf_rows_indexed: the GEMM reads whole 512-column tiles
    xsq = torch.zeros(xp.shape[0], device="cuda")
    C.k_row_sqnorm(xp.data_ptr(), xp.shape[0], dp, dp, xsq.data_ptr(), s)
    rd = torch.tensor(rows, dtype=torch.int32, device="cuda")
    od = torch.arange(len(rows), dtype=torch.int32, device="cuda")
    ld = (n + 127) // 128 * 128
    out = torch.full((len(rows), ld), float("nan"), device="cuda")
    ms = C.k_rows_split_bench(xp.data_ptr(), xsq.data_ptr(), n, dp, rd.data_ptr(), len(rows), gamma, out.data_ptr(),
                              ld, od.data_ptr(), REPS, s)
    torch.cuda.synchronize()
    check_times(ms)
    assert torch.equal(out[:, :n], want)


def test_platt_fit_bench_reps():
    from dpsvm_amd._native import load

    rng = np.random.default_rng(8)
    y = np.where(rng.random((2, 300)) < 0.3, 1.0, -1.0).astype(np.float32)
    dec = (0.9 * y + 0.6 * rng.standard_normal((2, 300))).astype(np.float32)
    check_times(load().k_platt_fit_bench(dec, y, REPS))
