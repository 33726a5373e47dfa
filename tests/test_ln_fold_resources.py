"""The folded instantiations of the fp32 edge kernels (edge_encode.hip, conv_edge.hip, conv_edge_small.hip: the last template
argument `true`) use no scratch memory and at most 256 registers, in the release and in the checked library; the general
instantiations are still there beside them.  Parses the amdhsa metadata of the embedded gfx950 code objects
(tools/kernel_resources.py); CPU only, runs wherever the ROCm LLVM tools are installed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

FOLDED = ["k_conv_edge<false, false, true>", "k_conv_edge<false, true, true>",
          "k_conv_edge_small<1, 1, false, false, true>", "k_conv_edge_small<1, 1, false, true, true>",
          "k_edge_encode<44, true>", "k_edge_encode<45, true>", "k_edge_encode_small<44, true>", "k_edge_encode_small<45, true>"]
GENERAL = ["k_conv_edge<false, false, false>", "k_conv_edge<false, true, false>",
           "k_conv_edge_small<1, 1, false, false, false>", "k_conv_edge_small<1, 1, false, true, false>",
           "k_edge_encode<44, false>", "k_edge_encode<45, false>", "k_edge_encode_small<44, false>", "k_edge_encode_small<45, false>"]


@pytest.mark.parametrize("which", ["release", "checked"])
def test_folded_instantiations_have_no_scratch_and_at_most_256_registers(which):
    from gamd_amd import _lib
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    path = _lib.LIB_PATH if which == "release" else os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")
    res = kr.kernel_resources(path)
    for k in FOLDED + GENERAL:
        hit = [v for n, v in res.items() if k + "(" in n]
        assert len(hit) == 1, (k, sorted(res))
        if k in FOLDED:
            v = hit[0]
            assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0, (k, v)
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= 256, (k, v)
