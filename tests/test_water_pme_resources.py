"""The particle-mesh Ewald kernels (gamd_amd/csrc/water_pme.hip) are exactly the documented seven, in the release and in the
checked library, use no scratch memory and spill no register: spread and gather keep an atom's 6 p spline weights in
registers and pick the z weight of their lane by selects (an indexed access would move the atom into scratch), the line pass
holds its points in LDS.  Parses the amdhsa metadata of the embedded gfx950 code objects (tools/kernel_resources.py); CPU only,
runs wherever the ROCm LLVM tools are installed.  No kernel's name carries one of the prefixes the other resource tests count."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

KERNELS = ("k_pme_clear", "k_pme_spread4", "k_pme_spread6", "k_pme_fft", "k_pme_conv", "k_pme_gather4", "k_pme_gather6")
# LDS: the line pass holds 1024 complex points as two arrays of doubles (16 KiB) and the 64 twiddles (1 KiB): 17 KiB, nine
# workgroups per CU of 160 KiB; the convolution its four wave sums; nothing else uses any.
LDS_CAP = {"k_pme_fft": 17 * 1024, "k_pme_conv": 32}
# registers: 128 keeps four waves per SIMD (512 per lane).  The gather of order 6 holds 36 doubles of weights and derivatives,
# three accumulators and the stencil's indices and took 98 when this was written; every other kernel took 70 or fewer.
VGPR_CAP = 128
OTHER_PREFIXES = ("k_water_", "k_w4_", "k_wvir_", "k_wsrc_", "k_wmin_")


def test_pme_kernels_are_the_documented_set_without_scratch_or_spills_in_the_release_and_the_checked_library():
    from gamd_amd import _lib
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kr.kernel_resources(path).items() if "k_pme_" in n}
        assert len(res) == len(KERNELS) and all(any(k + "(" in n for n in res) for k in KERNELS), sorted(res)
        for n, v in res.items():
            short = next(k for k in KERNELS if k + "(" in n)
            assert not any(p in n for p in OTHER_PREFIXES), n
            assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
            assert v.get("group_segment_fixed_size", 0) <= LDS_CAP.get(short, 0), (n, v)
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= VGPR_CAP, (n, v)
            print(os.path.basename(path), short, "vgpr", v["vgpr_count"], "sgpr", v.get("sgpr_count"), "lds", v.get("group_segment_fixed_size", 0))
