"""Molecular virial of the water classical potential, host side (no device): the float64 reference of
tests/water_virial_ref.py against the volume derivative of the existing references' energy and against the Coulomb identity,
the long-range dispersion correction against a quadrature and its closed form, the C ABI of the three new entry points, the
resources of the k_wvir_* kernels, and RunWaterClassical's virial columns and pressure on synthetic arrays."""
import os
import re
import sys

import numpy as np
import pytest

import water_classical_ref as wr
import water_virial_ref as vr
from gamd_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W4 = 0.106676721
BOXES = {"cubic": np.array([13.75, 13.75, 13.75]), "ortho": np.array([13.75, 15.0, 16.25])}


def water86(box):
    """the 86-molecule jittered lattice of test_water_classical_host.py (unwrapped: molecules whole), its molecules moved
    rigidly so that their centres fill `box`"""
    pos, b0, species, _ = wl.water_box(86, seed=5, jitter=0.02, wrap=False)
    x, _ = vr.scaled(pos, b0, np.asarray(box, dtype=np.float64) / float(np.float32(b0)))
    return x, species


@pytest.fixture(scope="module")
def lib():
    from gamd_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- the formulas against the volume derivative of the existing references' energy ---------------------------------------
@pytest.mark.parametrize("w", [0.0, W4], ids=["3site", "4site"])
@pytest.mark.parametrize("shape", ["cubic", "ortho"])
def test_molecular_virial_is_the_volume_derivative_of_the_reference_energy(shape, w):
    """W_mol = -dE/d lambda at lambda = 1 (box edges and molecular centres scaled, molecules rigid; r_cut, alpha, k_cut fixed),
    central differences at h = 2^-10 and 2^-12, Richardson-extrapolated.  L (1 +- h) is exact in fp32 for these edges; the
    Lennard-Jones term is switched (a truncated one jumps when a pair crosses the cutoff); ewald_tol = 1e-12.  Bound
    1e-8 |W_mol|: 1.5e-10 .. 1.9e-10 are measured in these four cases (printed), on one configuration; the margin of 50
    covers others."""
    box = BOXES[shape]
    x, species = water86(box)
    wat = wr.Water(r_cut=6.8, r_switch=5.8, ewald_tol=1e-12)
    ref = vr.virial(x, box, species, wat, w)
    fd, D = vr.volume_derivative(x, box, species, wat, w)
    err = abs(fd - ref["w_mol"]) / abs(ref["w_mol"])
    print(f"{shape} w = {w}: W_mol {ref['w_mol']:.9f} kJ/mol, -dE/dlambda {fd:.9f} (h = 2^-10: {D[0]:.9f}, 2^-12: {D[1]:.9f}), "
          f"|difference| / |W_mol| = {err:.3e} (bound 1e-8); terms " + ", ".join(f"{c} {ref[c]:.6f}" for c in vr.COLUMNS[:4]))
    assert abs(ref["w_mol"]) > 1.0 and err <= 1e-8


def test_coulomb_virial_equals_the_coulomb_energy_up_to_the_ewald_truncation():
    """W_coul,pair + W_recip = U_real + U_excl + U_recip + U_self (the Coulomb energy is homogeneous of degree -1): measured
    3.2e-12, 2.2e-14, 1.9e-16 of the sum of absolute terms at ewald_tol 1e-10, 1e-12, 1e-14 (printed).  Asserted: <= 1e-12 at 1e-12, and
    falling from one tolerance to the next."""
    box = BOXES["cubic"]
    x, species = water86(box)
    dev = []
    for tol in (1e-10, 1e-12, 1e-14):
        ref = vr.virial(x, box, species, wr.Water(r_cut=6.8, r_switch=5.8, ewald_tol=tol), 0.0)
        ev = ref["ev"]
        lhs = ref["w_coul"] + ref["w_recip"]
        rhs = ((ev["u_real"] + ev["u_excl"]) + ev["u_recip"]) + ev["u_self"]
        scale = ref["abs_w_coul"] + ref["abs_w_recip"] + ev["abs_real"] + ev["abs_recip"] + abs(ev["u_self"])
        dev.append(abs(lhs - rhs) / scale)
        print(f"ewald_tol {tol:.0e}: W_coul + W_recip = {lhs:.9f}, U_coul = {rhs:.9f}, |difference| / abs terms = {dev[-1]:.2e}")
    assert dev[1] <= 1e-12 and dev[0] > dev[1] > dev[2]


def test_intramolecular_term_ignores_periodic_images_bit_for_bit():
    """positions on a grid of 2^-10 A: x + k L is exact in fp32, atom-wise shifts tear the molecules across images"""
    box = BOXES["ortho"]
    x, _ = water86(box)
    x32 = (np.rint(x / 2.0 ** -10) * 2.0 ** -10).astype(np.float32)
    k = np.random.default_rng(3).integers(-2, 3, size=x.shape)
    moved = (x32.astype(np.float64) + k * box).astype(np.float32)
    assert np.array_equal(moved.astype(np.float64), x32.astype(np.float64) + k * box) and (k != 0).any()
    assert np.array_equal(vr.molecule_offsets(moved, box), vr.molecule_offsets(x32, box))


# ---- long-range dispersion correction -------------------------------------------------------------------------------------
def test_dispersion_correction_against_quadrature_and_the_closed_form():
    from scipy.integrate import quad
    from gamd_amd.engine import lj_dispersion_correction
    n, vol, sig, eps, rc, rs = 86, 2.6, 0.315075, 0.635968, 0.68, 0.58
    u_lj = lambda r: 4.0 * eps * ((sig / r) ** 12 - (sig / r) ** 6)

    def one_minus_s(r):
        t = (r - rs) / (rc - rs)
        return t ** 3 * ((6.0 * t - 15.0) * t + 10.0)
    inner = quad(lambda r: u_lj(r) * one_minus_s(r) * r * r, rs, rc, epsabs=0.0, epsrel=2e-14)[0]
    outer = quad(lambda r: u_lj(r) * r * r, rc, np.inf, epsabs=0.0, epsrel=2e-14)[0]
    want = 2.0 * np.pi * n * n / vol * (inner + outer)
    u, w = lj_dispersion_correction(n, vol, sig, eps, rc, rs)
    print(f"U_lrc {u:.12e} kJ/mol, quadrature {want:.12e}, relative difference {abs(u - want) / abs(want):.2e}")
    assert abs(u - want) <= 1e-12 * abs(want) and w == 3.0 * u and u < 0.0
    closed = 2.0 * np.pi * n * n / vol * 4.0 * eps * (sig ** 12 / (9.0 * rc ** 9) - sig ** 6 / (3.0 * rc ** 3))
    for no_switch in (0.0, rc, 2.0 * rc):
        u0, w0 = lj_dispersion_correction(n, vol, sig, eps, rc, no_switch)
        assert abs(u0 - closed) <= 1e-15 * abs(closed) and w0 == 3.0 * u0
    assert abs(u) > abs(closed)                               # the switch takes attraction away inside the cutoff as well
    with pytest.raises(ValueError):
        lj_dispersion_correction(n, 0.0, sig, eps, rc, rs)


# ---- RunWaterClassical / RunClassical -------------------------------------------------------------------------------------
def _synthetic(virial=True):
    from gamd_amd.engine import RunWaterClassical
    rows = np.zeros((3, 2, 12))
    rows[:, :, 0] = 10.0
    v = np.zeros((3, 2, 6))
    v[:, :, 0] = [[300.0, 30.0], [310.0, 31.0], [320.0, 32.0]]
    v[:, :, 1] = -900.0
    v[:, :, 2] = 50.0
    v[:, :, 3] = [[-20.0, 5.0], [-21.0, 6.0], [-22.0, 7.0]]
    v[:, :, 4] = [[320.0, 33.0], [321.0, 34.0], [322.0, 35.0]]
    v[:, :, 5] = ((v[:, :, 0] + v[:, :, 1]) + v[:, :, 2]) - v[:, :, 3]
    return RunWaterClassical([2, 4, 6], rows, 258, virial_rows=v if virial else None), v


def test_virial_columns_and_pressure_on_synthetic_rows():
    from gamd_amd.engine import BAR_PER_KJ_MOL_NM3, RunWaterClassical, lj_dispersion_correction
    rc, v = _synthetic()
    assert np.array_equal(rc.virial, v[:, :, 5]) and np.array_equal(rc.ke_com, v[:, :, 4])
    assert list(rc.virial_terms) == ["w_lj", "w_coul", "w_recip", "w_intra"]
    for k, name in enumerate(rc.virial_terms):
        assert np.array_equal(rc.virial_terms[name], v[:, :, k])
    vol = np.array([2.6, 3.3])
    want = BAR_PER_KJ_MOL_NM3 * (2.0 * v[:, :, 4] + v[:, :, 5]) / (3.0 * vol[None, :])
    assert np.array_equal(rc.pressure(None, vol), want)
    assert np.array_equal(rc.pressure(np.zeros((3, 2)), vol), BAR_PER_KJ_MOL_NM3 * v[:, :, 5] / (3.0 * vol[None, :]))
    # the dispersion correction: the oxygens, the potential's parameters in the engine's length unit
    with pytest.raises(ValueError, match="parameters"):
        rc.pressure(None, vol, dispersion=True)
    rc.lj = dict(sigma=3.15075, epsilon=0.635968, r_cut=6.8, r_switch=5.8, shift=False, length_per_nm=0.0)
    w_lrc = np.array([lj_dispersion_correction(86, x, 3.15075 / 10.0, 0.635968, 6.8 / 10.0, 5.8 / 10.0)[1] for x in vol])
    assert np.array_equal(rc.pressure(None, vol, dispersion=True), want + BAR_PER_KJ_MOL_NM3 * w_lrc[None, :] / (3.0 * vol[None, :]))
    rc.lj = dict(rc.lj, shift=True)
    with pytest.raises(ValueError, match="shift"):
        rc.pressure(None, vol, dispersion=True)
    # without virial rows: as before
    bare, _ = _synthetic(virial=False)
    assert bare.virial is None and bare.virial_terms is None and bare.ke_com is None
    with pytest.raises(NotImplementedError, match="virial"):
        bare.pressure(None, vol)
    with pytest.raises(ValueError, match="virial_rows"):
        RunWaterClassical([2, 4, 6], np.zeros((3, 2, 12)), 258, virial_rows=np.zeros((3, 2, 5)))


def test_lj_pressure_is_unchanged_by_default_and_takes_the_correction_for_all_atoms():
    from gamd_amd.engine import BAR_PER_KJ_MOL_NM3, RunClassical, lj_dispersion_correction
    rows = np.zeros((2, 1, 9))
    rows[:, 0, 1] = [30.0, 33.0]
    rc = RunClassical([4, 8], rows, 258)
    ke = np.array([[300.0], [310.0]])
    base = BAR_PER_KJ_MOL_NM3 * (2.0 * ke + rows[:, :, 1]) / (3.0 * 10.0)
    assert np.array_equal(rc.pressure(ke, 10.0), base) and np.array_equal(rc.pressure(ke, 10.0, dispersion=False), base)
    rc.lj = dict(sigma=3.4, epsilon=0.995792, r_cut=10.2, r_switch=6.8, shift=False, length_per_nm=10.0)
    w = lj_dispersion_correction(258, 10.0, 3.4 / 10.0, 0.995792, 10.2 / 10.0, 6.8 / 10.0)[1]
    assert np.array_equal(rc.pressure(ke, 10.0, dispersion=True), base + BAR_PER_KJ_MOL_NM3 * w / (3.0 * 10.0))
    rc.lj = dict(rc.lj, shift=True)
    with pytest.raises(ValueError, match="shift"):
        rc.pressure(ke, 10.0, dispersion=True)


# ---- ABI and resources ----------------------------------------------------------------------------------------------------
def test_virial_entry_points_are_declared_bound_and_exported(lib):
    from gamd_amd import _lib
    src = open(os.path.join(ROOT, "include", "gamd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gamd_water_virial", "gamd_water_virial_read", "gamd_water_virial_eval"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in _lib.SYMBOLS and hasattr(lib, name)
    assert re.search(r"GAMD_WATER_VIRIAL_ROW\s*=\s*6\b", src) and _lib.WATER_VIRIAL_ROW == 6 == len(vr.COLUMNS)
    # answered before any device work
    assert lib.gamd_water_virial(None, 1) == -22 and b"null handle" in lib.gamd_last_error()
    assert lib.gamd_water_virial_read(None, None, None, 0, None) == -22
    assert lib.gamd_water_virial_eval(None, None, None, None, None, 0.0, 16.0, 1.0, None, None, None) == -22
    assert lib.gamd_water_virial_eval(None, None, None, None, None, 0.0, 16.0, 0.0, None, None, None) == -22


KERNELS = ("k_wvir_pairs", "k_wvir_pairs4", "k_wvir_lj4", "k_wvir_sk", "k_wvir_mols", "k_wvir_final")
# LDS: the pair walks stage 256 atoms as three doubles and a flag (6400 B).  Registers: the two pair walks hold the polynomial
# evaluations of erfc / erf / exp in double like k_water_pairs and share its bar of 168 (three waves per SIMD at the least);
# every other kernel stays at four waves or more.
LDS_CAP = 6400
VGPR_CAP = {"k_wvir_pairs": 168, "k_wvir_pairs4": 168}


def test_virial_kernels_use_no_scratch_and_spill_nothing_in_the_release_and_the_checked_library():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    from gamd_amd import _lib
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kr.kernel_resources(path).items() if "k_wvir_" in n}
        assert len(res) == len(KERNELS) and all(any(k + "(" in n for n in res) for k in KERNELS), sorted(res)
        for n, v in res.items():
            short = next(k for k in KERNELS if k + "(" in n)
            assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
            assert v.get("group_segment_fixed_size", 0) <= LDS_CAP, (n, v)
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= VGPR_CAP.get(short, 128), (n, v)
