"""The classical observer's kernels (gamd_amd/csrc/classical.hip) use no scratch memory, in the release and in the checked
library: the pair kernel keeps an atom, six double accumulators and a pair term in registers, and a spill would put the
accumulators of the N^2 loop into memory.  Parses the amdhsa metadata of the embedded gfx950 code objects
(tools/kernel_resources.py); CPU only, runs wherever the ROCm LLVM tools are installed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402


def test_classical_kernels_use_no_scratch_in_the_release_and_the_checked_library():
    from gamd_amd import _lib
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kr.kernel_resources(path).items() if "k_classical_" in n}
        assert len(res) == 3, sorted(res)
        for n, v in res.items():
            assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0, (n, v)
            assert v.get("group_segment_fixed_size", 0) <= 8 * 1024, (n, v)          # one staged tile of 256 x 3 doubles
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= 128, (n, v)           # four waves per SIMD at the least
