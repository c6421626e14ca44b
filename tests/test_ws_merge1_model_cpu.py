"""The numpy model of the one-block merge (merge1_model, beside merge_model in
test_ws_kernels_gpu.py) on every crafted input the GPU tests feed the kernels
(tests/test_ws_recompute_kernels_gpu.py): the model's own invariants, and that
each input reaches the branch it is named for — so a kernel test that agrees
with the model agrees with something that cannot be vacuous."""
import numpy as np
import pytest

import test_ws_kernels_gpu as W


def _held(cand):
    c = cand[:, :, : W.KC1].ravel()
    return set(int(k) & 0xFFFFFFFF for k in c[c != W.NONE])


@pytest.mark.parametrize("name", sorted(W.MERGE1_CASES))
def test_merge1_model_invariants_on_every_crafted_input(name):
    st, q_max, n_new, prev = W.merge1_case(name)
    ref = W.merge1_model(st["cand"], prev, q_max, n_new, W.MERGE1_EPS)
    W.merge1_case_reaches_its_branch(name, st, prev, ref)
    idx, nc = ref["idx"], ref["n_chosen"]
    assert ref["q"] == len(idx) <= q_max
    assert len(set(idx)) == len(idx)  # no row twice
    keys = st["cand"][:, :, : W.KC1]
    up, low = np.sort(keys[:, 0].ravel()), np.sort(keys[:, 1].ravel())
    up0, low0 = int(up[0]) & 0xFFFFFFFF, int(low[0]) & 0xFFFFFFFF
    assert idx[0] == up0 and ref["src"][0] == "u"  # the global extremes first: the round makes progress
    if ref["want"] >= 2 and low0 != up0:
        assert ref["src"].index("l") == 1 and idx[1] == low0
    assert ref["b_hi"] == W.key_value(up[:1])[0] and ref["b_lo"] == -W.key_value(low[:1])[0]
    assert set(idx[:nc]) <= _held(st["cand"])  # every new row is a candidate
    assert nc <= ref["want"] and set(ref["src"][:nc]) <= {"u", "l"}
    kept = [p for p in prev if p not in idx[:nc]]
    assert ref["q"] == min(q_max, nc + len(kept))
    assert idx[nc:] == kept[: q_max - nc]  # retained rows keep their order (newest first)
    # the keys past kWsCand1 in a list are not read: the same result without them
    trimmed = st["cand"].copy()
    trimmed[:, :, W.KC1:] = W.NONE
    assert (st["cand"][:, :, W.KC1:] != W.NONE).any() or st["n"] <= W.KC1 * st["G"]
    assert W.merge1_model(trimmed, prev, q_max, n_new, W.MERGE1_EPS)["idx"] == idx


@pytest.mark.parametrize("name", sorted(W.merge1_stop_cases()))
def test_merge1_model_stop_codes(name):
    f, alpha, y, eps, it, max_iter, nonfinite, done = W.merge1_stop_cases()[name]
    cand = W.lists_from_state(f, alpha, y, W.MERGE1_C, 1)
    ref = W.merge1_model(cand, [], 2, 2, eps, iteration=it, max_iter=max_iter, nonfinite=nonfinite)
    assert ref["done"] == done
    if done:
        assert ref["q"] == 0 and ref["idx"] == [] and ref["n_apply"] == 0
    else:
        assert ref["idx"] == [0, 1]
    if name != "empty-low-side":  # b is reported on a stop too
        assert ref["b_hi"] == 0.0 and ref["b_lo"] == f[1]
