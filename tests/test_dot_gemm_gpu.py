"""The Gram builder of the dot-product kernels (kernels/dot_gemm_split.hip) alone, through ops.kernel_gram, at
the smallest shapes at which it can go wrong.

k blocks: d in {20, 33, 96, 100, 130, 200} gives 1, 2, 3, 4, 5, 7 blocks of 32 columns — every count of blocks
in flight ahead of the one being multiplied (0, 1, 2), the ring's wrap past its four buffers, padded last blocks.
Tiles: symmetric n = 130 (an edge tile, one mirrored tile) and 300 (three tile rows: the lower tiles exist only
through the mirror), non-symmetric 257 x 131 and 5 x 300.

Linear against the dot product in float64: per element
    |K - dot64| <= (d + 16) 2^-24 sum_k |a_k| |b_k|
fp32 accumulation of d products that are exact in fp32: d 2^-24; the dropped l.l term: 2^-22 = 4 2^-24; the
truncation of each operand to 22 bits: 2 x 2^-22 = 8 2^-24; H + (P + Q), the scaling (exact) and the split's own
roundings: 4 2^-24 more.  Worst case; the measured maximum is printed.

Poly and sigmoid against the formula in float64 applied to the op's OWN linear output L (the same dot bits, so
the GEMM's error is not in it): with u = gamma L + coef0 (gamma and coef0 as the float32 values the kernel gets),
    poly     |K - u^p|     <= 2 (p |u|^(p-1) 2^-23 (|gamma L| + |coef0|) + p 2^-24 |u|^p)
    sigmoid  |K - tanh(u)| <= 2^-23 (|gamma L| + |coef0|) + 5 ulp
tanhf: no device-libs document with an accuracy table was found with the toolchain, so the bound is the one the
device math library is written against — OpenCL 3.0 full profile, single precision tanh <= 5 ulp — with
1 ulp <= 2^-23 |tanh u|.  The measured maximum against float64 tanh of the float32 u is printed (and recorded in
profiles/named_kernels/probes.jsonl by bench/named_kernels_probe.py).
"""
import functools

import numpy as np
import pytest
import torch

from dpsvm_amd import Linear, Poly, Sigmoid

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
GAMMA, POLY, SIG = 0.1, Poly(3, 1.0), Sigmoid(0.25)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def rows(n: int, d: int, seed: int) -> np.ndarray:
    x = np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)
    x.setflags(write=False)
    return x


def gram(a, b=None, kernel=Linear(), gamma=1.0):
    from dpsvm_amd.ops import kernels as ops

    ta = torch.tensor(a, dtype=torch.float32, device="cuda")
    tb = None if b is None else torch.tensor(b, dtype=torch.float32, device="cuda")
    return ops.kernel_gram(ta, tb, kernel=kernel, gamma=gamma)


def bits(t) -> np.ndarray:
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def check_linear(K: np.ndarray, a: np.ndarray, b: np.ndarray, what: str) -> None:
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    bound = (a.shape[1] + 16) * U24 * (np.abs(a64) @ np.abs(b64).T)
    err = np.abs(K.astype(np.float64) - a64 @ b64.T)
    ratio = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{what}: linear max err / bound {ratio:.3g}")
    assert np.all(np.isfinite(K)) and np.all(err <= bound)


def check_padding(Kt: torch.Tensor, m: int, n: int) -> None:
    """the view's base is (m, round_up(n, 128)) pre-filled with NaN: columns >= n still NaN, the rest finite"""
    base = Kt._base
    assert base is not None and tuple(base.shape) == (m, (n + 127) // 128 * 128) and tuple(Kt.shape) == (m, n)
    assert bool(torch.isfinite(Kt).all())
    if base.shape[1] > n:
        assert bool(torch.isnan(base[:, n:]).all())


def check_poly_sigmoid(a, b, L: np.ndarray, what: str) -> None:
    """poly and sigmoid of the same operands against float64 on the op's own linear output L"""
    g, L64 = float(np.float32(GAMMA)), L.astype(np.float64)
    Kp = gram(a, b, POLY, GAMMA).cpu().numpy()
    p, c0 = POLY.degree, float(np.float32(POLY.coef0))
    u = g * L64 + c0
    au = np.abs(g * L64) + abs(c0)
    tol = 2 * (p * np.abs(u) ** (p - 1) * 2 * U24 * au + p * U24 * np.abs(u) ** p)
    err = np.abs(Kp.astype(np.float64) - u ** p)
    print(f"{what}: poly max err / bound {float(np.max(err / np.maximum(tol, 1e-300))):.3g}")
    assert np.all(err <= tol)
    Ks = gram(a, b, SIG, GAMMA).cpu().numpy()
    c0 = float(np.float32(SIG.coef0))
    u = g * L64 + c0
    au = np.abs(g * L64) + abs(c0)
    tol = 2 * U24 * au + 5 * 2 * U24 * np.abs(np.tanh(u))
    err = np.abs(Ks.astype(np.float64) - np.tanh(u))
    u32 = u.astype(np.float32).astype(np.float64)  # the kernel's u: the fma's single rounding of g L + c0
    ulp = np.abs(Ks.astype(np.float64) - np.tanh(u32)) / np.spacing(np.abs(np.tanh(u32)).astype(np.float32))
    print(f"{what}: sigmoid max err / bound {float(np.max(err / np.maximum(tol, 1e-300))):.3g}; against float64 "
          f"tanh of the float32 u: {float(np.max(ulp)):.2f} ulp")
    assert np.all(err <= tol)


@pytest.mark.parametrize("d", [20, 33, 96, 100, 130, 200])
def test_k_blocks_symmetric_130(d):
    """nkb = 1, 2, 3, 4, 5, 7 on the two-tile symmetric Gram: values, symmetry, padding, the three kernels"""
    a = rows(130, d, 100 + d)
    Kt = gram(a)
    check_padding(Kt, 130, 130)
    K = Kt.cpu().numpy()
    check_linear(K, a, a, f"sym 130 x {d}")
    np.testing.assert_array_equal(bits(Kt), bits(Kt.t()))
    np.testing.assert_array_equal(bits(Kt), bits(gram(a, a)))  # the non-symmetric launch computes every tile
    np.testing.assert_array_equal(bits(gram(a, None, Poly(1, 0.0), 1.0)), bits(Kt))
    check_poly_sigmoid(a, None, K, f"sym 130 x {d}")
    for spec in (POLY, SIG):
        Ks = gram(a, None, spec, GAMMA)
        np.testing.assert_array_equal(bits(Ks), bits(Ks.t()))
        np.testing.assert_array_equal(bits(Ks), bits(gram(a, a, spec, GAMMA)))


@pytest.mark.parametrize("d", [20, 200])
def test_three_tile_rows_symmetric_300(d):
    a = rows(300, d, 300 + d)
    Kt = gram(a)
    check_padding(Kt, 300, 300)
    check_linear(Kt.cpu().numpy(), a, a, f"sym 300 x {d}")
    np.testing.assert_array_equal(bits(Kt), bits(Kt.t()))
    np.testing.assert_array_equal(bits(Kt), bits(gram(a, a)))
    Kp = gram(a, None, POLY, GAMMA)
    check_padding(Kp, 300, 300)
    np.testing.assert_array_equal(bits(Kp), bits(Kp.t()))
    np.testing.assert_array_equal(bits(Kp), bits(gram(a, a, POLY, GAMMA)))


@pytest.mark.parametrize("m,n,d", [(257, 131, 100), (5, 300, 33), (257, 131, 20)])
def test_rectangular(m, n, d):
    a, b = rows(m, d, 7 * m + d), rows(n, d, 11 * n + d)
    Kt = gram(a, b)
    check_padding(Kt, m, n)
    K = Kt.cpu().numpy()
    check_linear(K, a, b, f"{m} x {n} x {d}")
    np.testing.assert_array_equal(bits(gram(b, a)), bits(Kt.t()))  # the dot is bit-identical under operand swap
    np.testing.assert_array_equal(bits(gram(a, b, Poly(1, 0.0), 1.0)), bits(Kt))
    check_poly_sigmoid(a, b, K, f"{m} x {n} x {d}")
    check_padding(gram(a, b, SIG, GAMMA), m, n)


def test_extreme_rows():
    """row scales 2^-20 .. 2^20 and a zero row: the per-row shifts keep the linear bound (scaling by a power of two
    is exact); the zero row's dot products are 0, so its poly values are powi(coef0, p) and its sigmoid tanh(coef0)"""
    base = rows(140, 40, 5)
    scale = np.ldexp(1.0, np.linspace(-20, 20, 140).round().astype(np.int32)).astype(np.float32)
    a = (base * scale[:, None]).astype(np.float32)
    a[77] = 0.0
    Kt = gram(a)
    K = Kt.cpu().numpy()
    check_linear(K, a, a, "extreme rows")
    np.testing.assert_array_equal(bits(Kt), bits(Kt.t()))
    assert np.all(K[77] == 0.0) and np.all(K[:, 77] == 0.0)
    spec = Poly(5, -1.5)
    Kp = gram(a, None, spec, 2.0 ** -30).cpu().numpy()
    c = np.float32(-1.5)
    want = c * (c * c) * (c * c)  # powi(c, 5): ret = c, tmp = c^2; tmp = c^4; ret = c * c^4 — exact here
    assert np.all(Kp[77] == want) and np.all(Kp[:, 77] == want) and float(want) == (-1.5) ** 5
    Ks = gram(a, None, Sigmoid(0.75), 2.0 ** -30).cpu().numpy()
    t = np.tanh(0.75)
    assert np.all(np.abs(Ks[77].astype(np.float64) - t) <= 5 * 2 * U24 * t) and len(np.unique(Ks[77])) == 1
    np.testing.assert_array_equal(Ks.view(np.uint32), Ks.T.view(np.uint32))


def test_ring_wrap_repeats_bit_for_bit():
    """n = 300, d = 200 (7 k blocks: the ring wraps) on two inputs interleaved over two streams: every launch of
    an input gives the same bits"""
    a, b = rows(300, 200, 500), rows(300, 200, 501)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    out = []
    for x, s in ((a, s1), (b, s2), (a, s2), (b, s1)):
        with torch.cuda.stream(s):
            out.append(gram(x, None, POLY, GAMMA))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(out[0]), bits(out[2]))
    np.testing.assert_array_equal(bits(out[1]), bits(out[3]))
    assert not np.array_equal(bits(out[0]), bits(out[1]))


def test_argument_errors():
    from dpsvm_amd.ops import kernels as ops

    a = torch.zeros(4, 8, device="cuda")
    with pytest.raises(ValueError, match="kernel spec"):
        ops.kernel_gram(a, None, kernel="poly")
    with pytest.raises(ValueError):
        ops.kernel_gram(a, torch.zeros(4, 7, device="cuda"), kernel=Linear())
    assert tuple(ops.kernel_gram(a[:0], a, kernel=Linear()).shape) == (0, 4)
