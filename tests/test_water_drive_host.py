"""The water classical force source (gamd_md_force_source with GAMD_FORCE_WATER_CLASSICAL, gamd_amd/csrc/water_drive.hip) as
far as it can be seen without a GPU: the entry refuses a null handle by name for the new value, the binding tables carry it
next to the unchanged LJ table, and its two kernels are in the release and the checked library under names of their own —
tests/test_water_classical_resources.py counts exactly six kernels with `k_water_` in the name, tests/test_classical_drive_host.py
two with `k_drive_` — without scratch and without a spilled register, with one staged tile of 256 x 3 doubles plus flags in LDS
(at most 8 KiB), the pair kernel within the observer's own bar for k_water_pairs (168 registers: the polynomial evaluations of
erfc / erf / exp in double sit next to the pair term) and the per-atom kernel within 128.  Parses the amdhsa metadata of the
embedded gfx950 code objects (tools/kernel_resources.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

VGPR_CAP = {"k_wsrc_pairs": 168, "k_wsrc_atoms": 128}


@pytest.fixture(scope="module")
def lib():
    from gamd_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_the_tables_carry_the_water_source_next_to_the_unchanged_lj_table(lib):
    from gamd_amd import _lib
    assert hasattr(lib, "gamd_md_force_source") and "gamd_md_force_source" in _lib.SYMBOLS
    assert _lib.WATER_FORCE_SOURCE == {"water_classical": 2}
    assert _lib.FORCE_SOURCE == {"network": 0, "classical": 1}


def test_a_null_handle_is_refused_by_name_for_the_water_source(lib):
    assert lib.gamd_md_force_source(None, 2) == -22
    assert b"null handle" in lib.gamd_last_error()


def test_water_drive_kernels_are_in_both_libraries_within_their_bars(lib):
    from gamd_amd import _lib
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kr.kernel_resources(path).items() if "k_wsrc_" in n}
        assert len(res) == 2 and all(any(k + "(" in n for n in res) for k in VGPR_CAP), sorted(res)
        for n, v in res.items():
            short = next(k for k in VGPR_CAP if k + "(" in n)
            assert "k_water_" not in n and "k_drive_" not in n and "k_classical_" not in n
            assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
            assert v.get("group_segment_fixed_size", 0) <= 8 * 1024, (n, v)
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= VGPR_CAP[short], (n, v)
            print(os.path.basename(path), short, "vgpr", v["vgpr_count"], "sgpr", v.get("sgpr_count"), "lds", v.get("group_segment_fixed_size", 0))
