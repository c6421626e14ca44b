"""The Python surface of the kernel probes is frozen: every ``k_*`` function of the built module has the pybind11
signature line (name, argument names, order, types, defaults, return type) and every ``kWsProbe*`` constant the
value that tests/data/probe_surface.json holds, recorded by bench/make_probe_surface_fixture.py: the entries of the
build before the probes' host code was consolidated, unchanged since, plus those of the cache-mode probes
(k_ws_merge_cache, k_ws_merge_multi_cache, k_ws_pack_rows, k_rbf_rows_miss and their three constants) as they were
added.  No name missing, none added: a new probe is recorded in the fixture by the change that adds it."""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def test_probe_surface_matches_the_fixture(C):
    spec = importlib.util.spec_from_file_location(
        "make_probe_surface_fixture", os.path.join(HERE, "..", "bench", "make_probe_surface_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(HERE, "data", "probe_surface.json")) as fh:
        want = json.load(fh)
    got = mod.surface(C)
    assert len(want) >= 39 and "kWsProbeKey" in want and "k_ws_select" in want
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
