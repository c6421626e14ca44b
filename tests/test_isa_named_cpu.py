"""Register-spill guard for the dot-product kernels' Gram builder (CPU only: hipcc cross-compiles gfx950 here),
in the manner of test_isa_cpu.py: kernels/dot_gemm_split.hip is compiled to gfx950 assembly and each of its three
instantiations (linear, poly, sigmoid) must have a zero private (scratch) segment — the 96 accumulator registers
stay live through an epilogue that inlines tanhf / the powi loop."""
import os

import pytest

from test_isa_cpu import HIPCC, kernel_scratch

TU = "kernels/dot_gemm_split.hip"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_dot_gemm_kernels_do_not_spill(tmp_path):
    res, n_scratch = kernel_scratch(TU, tmp_path)
    names = [k for k in res if "dot_gemm_split_glds_kernel" in k]
    assert len(names) == 3, f"expected the linear, poly and sigmoid instantiations, found {sorted(res)}"
    spilled = {k: v for k, v in res.items() if v != 0}
    assert not spilled and n_scratch == 0, f"{TU}: scratch segments {spilled}, {n_scratch} scratch instructions"
