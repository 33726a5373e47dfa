"""The classical force source (gamd_md_force_source, gamd_amd/csrc/drive.hip) as far as it can be seen without a GPU: the entry
is exported and refuses a null handle by name, and its two kernels are in the release and the checked library under names of
their own — tests/test_classical_resources.py counts exactly three kernels with `k_classical_` in the name — within the bar
that test sets for the observer: no scratch, at most 128 registers, at most 8 KiB LDS.  Parses the amdhsa metadata of the
embedded gfx950 code objects (tools/kernel_resources.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from gamd_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_the_entry_is_exported_and_in_the_binding_table(lib):
    from gamd_amd import _lib
    assert hasattr(lib, "gamd_md_force_source") and "gamd_md_force_source" in _lib.SYMBOLS
    assert _lib.FORCE_SOURCE == {"network": 0, "classical": 1}


def test_a_null_handle_is_refused_by_name(lib):
    assert lib.gamd_md_force_source(None, 1) == -22
    assert b"null handle" in lib.gamd_last_error()
    assert lib.gamd_md_force_source(None, 0) == -22


def test_drive_kernels_are_in_both_libraries_within_the_observers_bars(lib):
    from gamd_amd import _lib
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kr.kernel_resources(path).items() if "k_drive_" in n}
        assert len(res) == 2 and any("k_drive_lj_pairs" in n for n in res) and any("k_drive_lj_atoms" in n for n in res), sorted(res)
        for n, v in res.items():
            assert "k_classical_" not in n
            assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0, (n, v)
            assert v.get("group_segment_fixed_size", 0) <= 8 * 1024, (n, v)          # one staged tile of 256 x 3 doubles
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= 128, (n, v)           # four waves per SIMD at the least
