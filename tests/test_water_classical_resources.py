"""The water classical observer's kernels (gamd_amd/csrc/water_classical.hip) use no scratch memory and spill no register, in
the release and in the checked library: the pair kernel keeps an atom, six double accumulators and a pair term with erfc, erf
and exp in double in registers, the reciprocal kernels an atom (or a k-vector) and their accumulators, and a spill would put
the accumulators of the N^2 and N K loops into memory.  Parses the amdhsa metadata of the embedded gfx950 code objects
(tools/kernel_resources.py); CPU only, runs wherever the ROCm LLVM tools are installed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

KERNELS = ("k_water_pairs", "k_water_rho", "k_water_sk", "k_water_recip", "k_water_atoms", "k_water_final")
# LDS: k_water_recip stages 256 k-vectors as six doubles each (n, Re S, Im S, A: 12 KiB), k_water_rho 256 atoms as four (s and
# the charge) plus the 4 KiB of its wave sums; the pair kernel 256 atoms as three doubles and a flag.
LDS_CAP = 12 * 1024
# registers: the pair kernel holds the polynomial evaluations of erfc / erf / exp in double next to the pair term and may take
# up to 168 (three waves per SIMD at the least, of 512 registers per lane); every other kernel stays at four waves or more.
VGPR_CAP = {"k_water_pairs": 168}


def test_water_kernels_use_no_scratch_and_spill_nothing_in_the_release_and_the_checked_library():
    from gamd_amd import _lib
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kr.kernel_resources(path).items() if "k_water_" in n}
        assert len(res) == len(KERNELS) and all(any(k + "(" in n for n in res) for k in KERNELS), sorted(res)
        for n, v in res.items():
            short = next(k for k in KERNELS if k + "(" in n)
            assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
            assert v.get("group_segment_fixed_size", 0) <= LDS_CAP, (n, v)
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= VGPR_CAP.get(short, 128), (n, v)
