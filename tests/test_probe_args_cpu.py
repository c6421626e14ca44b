"""The kernel probes (kernel_entry.hip, ws_kernel_entry.hip) check their arguments before they touch the device:
a malformed call raises the check's own RuntimeError.  On a host without a GPU that proves the check ran before every
HIP call (the first of which would fail there with another message); on a GPU host the calls raise the same way."""
import numpy as np
import pytest

NONE = np.uint64((1 << 64) - 1)
KC = 16  # kWsCand


@pytest.fixture(scope="module")
def K():
    from dpsvm_amd.ops import kernels

    return kernels


def f32(*v):
    return np.asarray(v, np.float32)


def lists(C, G, rows=(0, 1)):
    """[G][2][KC] candidate lists: list 0 holds rows[0] (up) and rows[1] (low), the rest is empty"""
    c = np.full((G, 2, KC), NONE, np.uint64)
    c[0, 0, 0] = C.make_key(-1.0, rows[0])
    c[0, 1, 0] = C.make_key(-1.0, rows[1])
    return c


def state(n):
    return np.zeros(n, np.float32), np.zeros(n, np.float32), np.where(np.arange(n) % 2, -1, 1).astype(np.float32)


def test_ws_merge_multi(K, C):
    with pytest.raises(RuntimeError, match="2 <= blocks <= 128"):
        K.ws_merge_multi(lists(C, 1), 1, 4, 2, 1e-3)
    with pytest.raises(RuntimeError, match="G <= 256"):
        K.ws_merge_multi(lists(C, 257), 2, 4, 2, 1e-3)


def test_ws_solve(K):
    q = 4
    with pytest.raises(RuntimeError, match=r"qb\[p\] <= q_max"):
        K.ws_solve(np.eye(q), *state(q), [q + 1], q, 1.0)
    with pytest.raises(RuntimeError, match="diag runs one block"):
        K.ws_solve(np.stack([np.eye(q)] * 2), *state(2 * q), [2, 2], q, 1.0, clip="box", diag=True)


def test_ws_select(K):
    L, n = 4, 8
    gram = np.zeros((L, n), np.float32)
    f, alpha, y = state(n)
    with pytest.raises(RuntimeError, match="fold needs 2 fold state rows"):
        K.ws_select(gram, f[:6], alpha[:6], y[:6], alpha[:6], [0], [0.5], [1], 1.0, fold=4)
    with pytest.raises(RuntimeError, match="apply line out of range"):
        K.ws_select(gram, f, alpha, y, alpha, [L], [0.5], [1], 1.0)
    for done in (-1, 6):
        with pytest.raises(RuntimeError, match="done is a DoneCode"):
            K.ws_select(gram, f, alpha, y, alpha, [0], [0.5], [1], 1.0, done=done)


@pytest.mark.parametrize("probe", ["ws_gather", "ws_subgram_split"])
def test_one_block_merge_probes(K, C, probe):
    n = 8
    f, alpha, y = state(n)
    first = np.zeros((n, n), np.float32) if probe == "ws_gather" else np.zeros((n, 4), np.float32)
    extra = () if probe == "ws_gather" else (0.5,)  # gamma
    run = getattr(K, probe)
    with pytest.raises(RuntimeError, match="previous set longer than q_max"):
        run(first, lists(C, 1), [2, 3, 4], f, alpha, y, *extra, 2, 2, 1e-3)
    with pytest.raises(RuntimeError, match="candidate row out of range"):
        run(first, lists(C, 1, rows=(0, n)), [], f, alpha, y, *extra, 2, 2, 1e-3)


def test_ws_fupdate_split(K):
    n = 200
    f, alpha, y = state(n)
    X = np.zeros((n, 4), np.float32)
    with pytest.raises(RuntimeError, match="<= 192 apply rows"):
        K.ws_fupdate_split(X, f, alpha, y, np.arange(193), np.zeros(193), 0.5, 1.0)
    with pytest.raises(RuntimeError, match="dp <= 64"):
        K.ws_fupdate_split(np.zeros((n, 65), np.float32), f, alpha, y, [1], [0.5], 0.5, 1.0)


def test_gram_rows_wsum(K):
    L, ldg = 4, 8
    gram = np.zeros((L, ldg), np.float32)
    with pytest.raises(RuntimeError, match="ldg >= n"):
        K.gram_rows_wsum(gram, ldg + 1, [1.0])
    with pytest.raises(RuntimeError, match="line out of range"):
        K.gram_rows_wsum(gram, ldg, [1.0], lines=[L])
    with pytest.raises(RuntimeError, match="identity lines need m <= L"):
        K.gram_rows_wsum(gram, ldg, np.ones(L + 1))


def test_gram_rows_dot(C):
    nt, n, k = 2, 8, 3
    with pytest.raises(RuntimeError, match=r"b \[k\]"):
        C.k_gram_rows_dot(np.zeros(nt * n, np.float32), nt, n, n, np.zeros(k * n, np.float32), n, k,
                          np.zeros(k + 1, np.float32))


def test_platt_probes(K):
    with pytest.raises(RuntimeError, match=r"platt_fit: dec and y \[m\]\[n\]"):
        K.platt_fit(np.zeros((2, 8)), np.ones((2, 9)))
    with pytest.raises(RuntimeError, match="slot < slots"):
        K.holdout_decision(np.zeros(8), np.ones(8), [0, 1], 0.0, np.zeros((2, 8)), slot=2)
    with pytest.raises(RuntimeError, match="A and B of k values"):
        K.proba_rows(np.zeros((4, 3)), np.zeros(2), np.zeros(3))
