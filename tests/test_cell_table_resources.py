"""The cell-table kernels of the classical potentials — the table's builder (gamd_amd/csrc/cell_table.hip) and the pair passes over
the table (water_cells.hip, classical_cells.hip) — are exactly the documented twelve, family by family, in the release and in the
checked library, use no scratch memory and spill no register, vector or scalar.  The water pair pass keeps the table's addresses
and the inner loops' geometry in vector registers and gives the same-molecule terms (erf) a wave of their own, because the
potential's constants with those of erf and erfc in one path do not fit the scalar file; the Lennard-Jones pair pass stays under
the all-pairs kernels' bar of 128 vector registers (four waves per SIMD).  Parses the amdhsa metadata of the embedded gfx950 code
objects (tools/kernel_resources.py) and nothing else; CPU only, runs wherever the ROCm LLVM tools are installed.  No kernel's name
carries one of the prefixes the other families or the other resource tests count."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

# family: (kernels, LDS cap per kernel (0 where none is named), VGPR cap)
FAMILIES = {
    # the builder.  LDS: the scan its 256 sums (1 KiB).  Registers: the table build took 18 or fewer when this was written.
    "k_celltab_": (("k_celltab_clear", "k_celltab_count", "k_celltab_scan", "k_celltab_fill", "k_celltab_rank"),
                   {"k_celltab_scan": 1024}, 32),
    # LDS: the pair pass the partial rows of the five x entries, 5 x NOUT x 64 doubles: 15 KiB with every accumulator, 7.5 KiB with
    # the forces alone — ten and more workgroups per CU of 160 KiB, registers bind first.  Registers: the pair pass is
    # gamd_water_walk's body (k_water_pairs took 164) and stays under the all-pairs walk's bar of 168: three waves per SIMD (512
    # per lane).
    "k_wcell_": (("k_wcell_pairs", "k_wcell_force", "k_wcell_pairs4", "k_wcell_force4"),
                 {"k_wcell_pairs": 15 * 1024, "k_wcell_pairs4": 15 * 1024, "k_wcell_force": 7680, "k_wcell_force4": 7680}, 168),
    # LDS: none (the lanes' partial rows meet by shuffles).  Registers: the pair pass holds a batch of four table entries (32
    # registers) on top of gamd_lj_walk's body and must leave four waves per SIMD: 512 / 4 = 128 per lane
    "k_ljcell_": (("k_ljcell_pairs", "k_ljcell_force", "k_ljcell_min"), {}, 128),
}
OTHER_PREFIXES = ("k_celltab_", "k_wcell_", "k_ljcell_", "k_classical_", "k_drive_", "k_min_", "k_water_", "k_w4_", "k_wvir_", "k_wsrc_",
                  "k_wmin_", "k_pme_")


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_cell_kernels_are_the_documented_set_without_scratch_or_spills_in_the_release_and_the_checked_library(family):
    from gamd_amd import _lib
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    KERNELS, LDS_CAP, VGPR_CAP = FAMILIES[family]
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kr.kernel_resources(path).items() if family in n}
        assert len(res) == len(KERNELS) and all(any(k + "(" in n for n in res) for k in KERNELS), sorted(res)
        for n, v in res.items():
            short = next(k for k in KERNELS if k + "(" in n)
            assert not any(p in n for p in OTHER_PREFIXES if p != family), n
            assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
            assert v.get("group_segment_fixed_size", 0) <= LDS_CAP.get(short, 0), (n, v)
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= VGPR_CAP, (n, v)
            print(os.path.basename(path), short, "vgpr", v["vgpr_count"], "sgpr", v.get("sgpr_count"), "lds", v.get("group_segment_fixed_size", 0))
