#!/usr/bin/env python3
"""tests/data/probe_surface.json: the Python surface of the kernel probes, the reference of
tests/test_probe_surface_cpu.py.

For every attribute of ``dpsvm_amd._C`` whose name starts with ``k_`` or ``kWsProbe``: the pybind11 signature line
(the first line of ``__doc__``: name, argument names, types, defaults, return type) of a function, the value of a
constant.  Record it on the build whose surface is to be kept (the parent of a change to the probes' host code);
needs no GPU.

    python bench/make_probe_surface_fixture.py [--out tests/data/probe_surface.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def surface(C) -> dict:
    out = {}
    for name in sorted(dir(C)):
        if not name.startswith(("k_", "kWsProbe")):
            continue
        v = getattr(C, name)
        out[name] = v.__doc__.splitlines()[0] if callable(v) else v
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "data", "probe_surface.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from dpsvm_amd._native import load

    s = surface(load(build_if_missing=False))
    with open(a.out, "w") as fh:
        json.dump(s, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{a.out}: {len(s)} names")
    return 0


if __name__ == "__main__":
    sys.exit(main())
