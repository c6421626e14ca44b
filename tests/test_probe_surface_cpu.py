"""The Python surface of the kernel probes is frozen: every ``k_*`` function of the built module has the pybind11
signature line (name, argument names, order, types, defaults, return type) and the two ``kWsProbe*`` constants the
value that tests/data/probe_surface.json holds, recorded by bench/make_probe_surface_fixture.py on the build before
the probes' host code was consolidated.  No name missing, none added."""
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
