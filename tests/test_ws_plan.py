"""The working-set round's shape is decided by one pure host function
(dpsvm/ws_plan.hpp ws_round_plan + ws_round_shape; gpu_setup.hip gathers the
facts and runs the two device steps between them; docs/DESIGN.md §2b).  CPU
only.  Unless stated: 60,000 rows, ws_size 192, ws_blocks auto, one rank, 256
CUs, ws-dense, every rank eligible, the peer exchange's self test passes."""
import pytest

C = pytest.importorskip("dpsvm_amd._C")

CACHE = dict(ws_dense=False, ws_cache=True)


def plan(n=60000, **facts):
    return C.ws_round_plan(n, **facts)


@pytest.mark.parametrize("facts,blocks,q_max", [
    (dict(uncoupled=True), 128, 48),
    (dict(), 32, 96),
    (dict(uncoupled=True, L=14336, **CACHE), 64, 48),   # L = 2 x 64 x 48 + the 8192-line window
    (dict(uncoupled=True, L=14335, **CACHE), 1, 192),
    (dict(L=2 * 3072 + 8192, **CACHE), 32, 96),
    (dict(L=2 * 3072 + 8191, **CACHE), 1, 192),
    (dict(n=49999, uncoupled=True), 1, 192),
    (dict(n=50000, uncoupled=True), 128, 48),
    (dict(ws_size=64), 32, 64),
    (dict(ws_size=32, uncoupled=True), 128, 32),
    (dict(ws_size=33, uncoupled=True), 128, 32),        # an even q
    (dict(ws_size=250), 32, 96),                        # clamped to 192
    (dict(ws_blocks=8), 8, 192),
    (dict(ws_blocks=1, uncoupled=True), 1, 192),
    (dict(ws_blocks=4, ws_size=95), 1, 95),
    (dict(ws_blocks=32, ws_size=192), 32, 192),         # 6,144 rows: the capacity itself
    (dict(ws_blocks=32, ws_size=192, L=10 ** 6, **CACHE), 1, 192),  # ws-cache unions stay <= 3,072 rows
    (dict(uncoupled=True, world=4, share=4), 64, 48),
    (dict(uncoupled=True, world=8, share=8), 32, 48),
    (dict(uncoupled=True, world=2, share=1), 128, 48),
    (dict(uncoupled=True, world=8, share=1), 128, 48),
    (dict(uncoupled=True, world=4, share=4, cus=304), 128, 48),  # 9,472 waves fit 9,728 slots
    (dict(uncoupled=True, world=4, share=4, force_collectives=True, device_comm=True), 128, 48),
    (dict(uncoupled=True, world=4, share=4, exchange=1), 128, 48),  # allreduce: nothing spins
    (dict(uncoupled=True, world=2, selftest_ok=False), 1, 192),     # no exchange, host communicator
    (dict(uncoupled=True, world=2, selftest_ok=False, device_comm=True), 128, 48),
    (dict(uncoupled=True, world=2, peers_eligible=False), 1, 192),
    (dict(uncoupled=True, world=2, ws_G=129), 1, 192),  # 258 candidate lists: more than the merge reads
])
def test_round_shape(facts, blocks, q_max):
    p = plan(**facts)
    assert p["error"] == ""
    assert (p["blocks"], p["q_max"]) == (blocks, q_max), p


def test_headline_and_coupled_shapes_in_full():
    p = plan(uncoupled=True)
    assert (p["ncand"], p["direct_sub"], p["n_new"], p["inner_max"]) == (C.kWsCand, 1, 48, 192)
    assert (p["p1G"], p["ks"]) == (59, 4) and p["note"] == ""
    p = plan()
    assert (p["ncand"], p["direct_sub"], p["n_new"], p["inner_max"]) == (C.kWsCandStd, 0, 96, 384)
    # ws_new / ws_inner given: kept; one-block rounds below 128 padded features replace 3/4 of the set
    p = plan(uncoupled=True, ws_new=20, ws_inner=77)
    assert (p["n_new"], p["inner_max"]) == (20, 77)
    assert plan(n=3000, dp=64)["n_new"] == 144 and plan(n=3000, dp=128)["n_new"] == 192
    # the solve gathers its sub-Gram itself only at one rank, on the resident Gram, without an exchange
    assert plan(uncoupled=True, exchange=2)["direct_sub"] == 0
    assert plan(uncoupled=True, L=14336, **CACHE)["direct_sub"] == 0
    assert plan(uncoupled=True, world=2)["direct_sub"] == 0


def test_refusals_and_notes():
    p = plan(ws_blocks=64, ws_size=192)
    assert "must be <= 6144 (the round's union capacity)" in p["error"]
    assert plan(ws_blocks=64, ws_size=96)["error"] == ""
    # solver=smo / a small problem on the pair engines ignores ws_blocks
    assert plan(ws_blocks=64, ws_size=192, ws_dense=False)["error"] == ""
    p = plan(ws_blocks=4, ws_size=95)
    assert "one block per round" in p["note"] and plan(ws_blocks=4, ws_size=96)["note"] == ""
    assert plan(n=3000, ws_size=95)["note"] == ""  # nothing asked for, nothing to explain
    # ranks sharing a device whose consumers would starve the producers: collectives, with the reason
    p = plan(n=3000, world=8, share=8, cus=40)
    assert not p["xch_resident"] and not p["peer_one"] and p["xch_waves"] == 8 * 80 + 1024
    assert "8 ranks share a device (1664 spinning + producer waves > 1280 wave slots)" in p["note"]
    p = plan(n=3000, world=8, share=8, cus=40, exchange=2)  # exchange=peer insists
    assert p["peer_one"] and p["note"] == ""


def test_exchange_region_words():
    """candidates + line-search partials + sub-Gram rows, both parities (device_state.hpp ws_xch_words*)"""
    p = plan(uncoupled=True, world=2)
    G_all, P, q = 2 * 118, 128, 48
    assert (p["p1G"], p["ks"]) == (30, 8)
    assert p["xch_words_multi"] == 2 * G_all * 4 * 16 + 2 * (2 * 30) * 8 * 4 + 2 * max(P * q * (q + 1), 192 * 193)
    assert p["xch_words_one"] == 2 * G_all * 4 * 4 + 2 * 192 * 193
