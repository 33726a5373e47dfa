"""The cell-table kernels (gamd_amd/csrc/water_cells.hip) are exactly the documented nine, in the release and in the checked
library, use no scratch memory and spill no register, vector or scalar: the pair pass keeps the table's addresses and the inner
loops' geometry in vector registers and gives the same-molecule terms (erf) a wave of their own, because the potential's constants
with those of erf and erfc in one path do not fit the scalar file.  Parses the amdhsa metadata of the embedded gfx950 code
objects (tools/kernel_resources.py); CPU only, runs wherever the ROCm LLVM tools are installed.  No kernel's name carries one of
the prefixes the other resource tests count."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

KERNELS = ("k_wcell_clear", "k_wcell_count", "k_wcell_scan", "k_wcell_fill", "k_wcell_rank", "k_wcell_pairs", "k_wcell_force",
           "k_wcell_pairs4", "k_wcell_force4")
# LDS: the scan its 256 sums (1 KiB); the pair pass the partial rows of the five x entries, 5 x NOUT x 64 doubles: 15 KiB with
# every accumulator, 7.5 KiB with the forces alone — ten and more workgroups per CU of 160 KiB, registers bind first.
LDS_CAP = {"k_wcell_scan": 1024, "k_wcell_pairs": 15 * 1024, "k_wcell_pairs4": 15 * 1024, "k_wcell_force": 7680, "k_wcell_force4": 7680}
# registers: the table build took 18 or fewer when this was written.  The pair pass is gamd_water_walk's body (k_water_pairs took
# 164) and stays under the all-pairs walk's bar of 168: three waves per SIMD (512 per lane).
VGPR_CAP = {k: 168 if k in LDS_CAP and k != "k_wcell_scan" else 32 for k in KERNELS}
OTHER_PREFIXES = ("k_water_", "k_w4_", "k_wvir_", "k_wsrc_", "k_wmin_", "k_pme_")


def test_cell_kernels_are_the_documented_set_without_scratch_or_spills_in_the_release_and_the_checked_library():
    from gamd_amd import _lib
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kr.kernel_resources(path).items() if "k_wcell_" in n}
        assert len(res) == len(KERNELS) and all(any(k + "(" in n for n in res) for k in KERNELS), sorted(res)
        for n, v in res.items():
            short = next(k for k in KERNELS if k + "(" in n)
            assert not any(p in n for p in OTHER_PREFIXES), n
            assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
            assert v.get("group_segment_fixed_size", 0) <= LDS_CAP.get(short, 0), (n, v)
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= VGPR_CAP[short], (n, v)
            print(os.path.basename(path), short, "vgpr", v["vgpr_count"], "sgpr", v.get("sgpr_count"), "lds", v.get("group_segment_fixed_size", 0))
