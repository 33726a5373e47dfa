"""The cell-table kernels of the Lennard-Jones classical potential (gamd_amd/csrc/classical_cells.hip) are exactly the documented
eight, in the release and in the checked library, use no scratch memory and spill no register, vector or scalar, and the pair
pass stays under the all-pairs kernels' bar of 128 vector registers (four waves per SIMD).  Parses the amdhsa metadata of the
embedded gfx950 code objects (tools/kernel_resources.py) and nothing else; CPU only, runs wherever the ROCm LLVM tools are
installed.  No kernel's name carries one of the prefixes the other resource tests count."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

BUILD = ("k_ljcell_clear", "k_ljcell_count", "k_ljcell_scan", "k_ljcell_fill", "k_ljcell_rank")
PASS = ("k_ljcell_pairs", "k_ljcell_force", "k_ljcell_min")
KERNELS = BUILD + PASS
# LDS: the scan its 256 sums (1 KiB); the pair pass none (the lanes' partial rows meet by shuffles)
LDS_CAP = {"k_ljcell_scan": 1024}
# registers: the table build took 18 or fewer when this was written; the pair pass holds a batch of four table entries (32
# registers) on top of gamd_lj_walk's body and must leave four waves per SIMD: 512 / 4 = 128 per lane
VGPR_CAP = {k: 128 if k in PASS else 32 for k in KERNELS}
OTHER_PREFIXES = ("k_classical_", "k_drive_", "k_min_", "k_wcell_", "k_water_", "k_w4_", "k_wvir_", "k_wsrc_", "k_wmin_", "k_pme_")


def test_cell_kernels_are_the_documented_set_without_scratch_or_spills_in_the_release_and_the_checked_library():
    from gamd_amd import _lib
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kr.kernel_resources(path).items() if "k_ljcell_" in n}
        assert len(res) == len(KERNELS) and all(any(k + "(" in n for n in res) for k in KERNELS), sorted(res)
        for n, v in res.items():
            short = next(k for k in KERNELS if k + "(" in n)
            assert not any(p in n for p in OTHER_PREFIXES), n
            assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
            assert v.get("group_segment_fixed_size", 0) <= LDS_CAP.get(short, 0), (n, v)
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= VGPR_CAP[short], (n, v)
            print(os.path.basename(path), short, "vgpr", v["vgpr_count"], "sgpr", v.get("sgpr_count"), "lds", v.get("group_segment_fixed_size", 0))
