"""Water classical observer, host side (no device): the float64 Ewald reference of tests/water_classical_ref.py against known
results and against itself (the Madelung constant of rock salt, independence of the splitting parameter, central differences,
Newton's third law, translation and periodic-image invariance), the ABI of gamd_water_params as a C99 compiler sees it, the
argument checks of gamd_water_configure that are answered before any device work, and RunWaterClassical's arithmetic and file
layout on synthetic arrays.  Nothing here claims parity with OpenMM or with a particle-mesh sum: the default parameters are
unverified."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import water_classical_ref as wr
from gamd_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ["interval", "max_samples", "q_h", "sigma_o", "epsilon_o", "r_cut", "r_switch", "shift", "reserved", "alpha", "k_cut",
          "coulomb_const"]

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "gamd_hip.h"
int main(void) {
    printf("sizeof %lu\n", (unsigned long)sizeof(gamd_water_params));
    printf("row %d\n", (int)GAMD_WATER_ROW);
@OFFSETS@
    return 0;
}
"""


@pytest.fixture(scope="module")
def lib():
    from gamd_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- the reference against a known result ----------------------------------------------------------------------------
def test_rock_salt_madelung_constant_and_vanishing_forces():
    """64 ions of charge +-1 on a simple cubic lattice of spacing 1 (L = 4), C = 1, no exclusions: E = -N M / 2 with
    M = 1.747564594633.  r_cut = 2 and alpha = 3 leave erfc(6) = 2e-17 of a term outside the real-space sum, and k_cut with
    exp(-k_cut^2 / 4 alpha^2) = 1e-15 that much outside the reciprocal one; by symmetry every force vanishes."""
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    q = np.where(g.sum(axis=1) % 2 == 0, 1.0, -1.0)
    alpha = 3.0
    k_cut = 2.0 * alpha * np.sqrt(-np.log(1e-15))
    out = wr.ewald(g.astype(np.float64), 4.0, q, np.zeros((64, 64), dtype=bool), alpha, 2.0, k_cut)
    e = out["u_real"] + out["u_excl"] + out["u_recip"] + out["u_self"]
    madelung = -2.0 * e / 64.0
    print(f"Madelung constant {madelung:.13f} ({out['n_k']} k-vectors, weight outside {out['tail']:.1e}), max |F| {np.abs(out['forces']).max():.2e}")
    assert out["u_excl"] == 0.0 and out["sum_q"] == 0.0 and out["tail"] <= 1e-15
    assert abs(madelung - 1.747564594633) <= 1e-10
    assert np.abs(out["forces"]).max() <= 1e-12


# ---- the reference against itself ------------------------------------------------------------------------------------
L86, RC86 = float(np.float32(13.7)), 6.8        # the reference holds the box as the library does: the fp32 value, widened


@pytest.fixture(scope="module")
def water86():
    """86 TIP3P molecules, jittered by 0.02 A per atom, scaled into a 13.7 A box (unwrapped: molecules are whole)"""
    pos, box, species, _ = wl.water_box(86, seed=5, jitter=0.02, wrap=False)
    return pos * (L86 / box), species


def _eval(x, species, alpha, n2max):
    # k_cut = 2 pi sqrt(n2max) / L: the whole list carries weight
    w = wr.Water(r_cut=RC86, alpha=alpha, k_cut=2.0 * np.pi * np.sqrt(n2max) / L86 * (1.0 + 1e-9))
    return wr.evaluate(x, L86, species, w, n2max=n2max)


@pytest.fixture(scope="module")
def two_alphas(water86):
    x, species = water86
    return _eval(x, species, 0.80, 400), _eval(x, species, 0.92, 520)


def test_energy_and_forces_do_not_depend_on_the_splitting_parameter(two_alphas):
    """(alpha, n2max) = (0.80, 400) and (0.92, 520): erfc(alpha r_cut) <= 1.5e-14 and exp(-k_max^2 / 4 alpha^2) <= 6e-15 of a
    term are left out by either, so the totals agree to 1e-11 of the sum of the absolute terms while every Ewald term by
    itself moves by more than 10 %."""
    a, b = two_alphas
    bound_e = 1e-11 * max(a["abs_energy"], b["abs_energy"])
    d_e = abs(a["energy"] - b["energy"])
    ratio_f = (np.abs(a["forces"] - b["forces"]) / (1e-11 * np.maximum(a["abs_f"], b["abs_f"])[:, None])).max()
    print(f"E {a['energy']:.9f} / {b['energy']:.9f}, |dE| {d_e:.2e} (bound {bound_e:.2e}), max |dF| / bound {ratio_f:.3e}; "
          f"K {a['n_k']} / {b['n_k']}")
    for name in ("u_coul", "u_recip", "u_self"):
        assert abs(a[name] - b[name]) > 0.1 * min(abs(a[name]), abs(b[name])), name
    assert a["u_lj"] == b["u_lj"] and a["pairs"] == b["pairs"] > 0 and a["near"] == 0
    assert d_e <= bound_e and ratio_f <= 1.0


def test_central_differences_of_the_energy_reproduce_the_forces(water86):
    """F = -dE/dx with h = 1e-5 A on every component of six atoms (O and H, first and last molecule included).  E carries a
    rounding error of at most 1e-12 of the sum of its absolute terms (the project's bound for such sums), which the
    difference quotient divides by 2 h for each of its two energies; the truncation h^2 E''' / 6 is below 1e-7 of the largest
    force component for any length scale above 0.03 A."""
    x, species = water86
    w = wr.Water(r_cut=RC86, ewald_tol=1e-12)
    ref = wr.evaluate(x, L86, species, w)
    f = ref["forces"] / 10.0                                  # kJ/mol/A
    h, atoms = 1e-5, [0, 1, 2, 100, 128, 257]
    fd = np.zeros((len(atoms), 3))
    for k, i in enumerate(atoms):
        for c in range(3):
            xp, xm = x.copy(), x.copy()
            xp[i, c] += h
            xm[i, c] -= h
            fd[k, c] = -(wr.evaluate(xp, L86, species, w)["energy"] - wr.evaluate(xm, L86, species, w)["energy"]) / (2 * h)
    scale = np.abs(f[atoms]).max()
    err = np.abs(fd - f[atoms]).max()
    bound = 1e-12 * ref["abs_energy"] / h + 1e-7 * scale
    print(f"central difference: max |F_fd - F| = {err:.3e} kJ/mol/A = {err / scale:.2e} of max |F| = {scale:.2f} (bound {bound:.3e})")
    assert scale > 0 and err <= bound


def test_forces_sum_to_zero_and_the_energy_ignores_translations_and_image_shifts(water86, two_alphas):
    x, species = water86
    a = two_alphas[0]
    assert a["sum_q"] == 0.0
    assert np.abs(a["forces"].sum(axis=0)).max() <= 1e-11 * a["abs_f"].sum()
    assert np.abs(a["f_pair"].sum(axis=0)).max() <= 1e-12 * a["abs_f"].sum()
    bound = 1e-11 * a["abs_energy"]
    moved = _eval(x + np.array([1.2345, -7.75, 20.5]), species, 0.80, 400)
    k = np.random.default_rng(3).integers(-2, 3, size=x.shape)
    image = _eval(x + k * L86, species, 0.80, 400)
    print(f"|dE| translation {abs(moved['energy'] - a['energy']):.2e}, image shifts {abs(image['energy'] - a['energy']):.2e} (bound {bound:.2e})")
    assert (k != 0).any() and moved["pairs"] == image["pairs"] == a["pairs"]
    assert abs(moved["energy"] - a["energy"]) <= bound and abs(image["energy"] - a["energy"]) <= bound


def test_kvector_list_is_a_sorted_half_space():
    kv = wr.kvectors(9)
    assert kv.shape == (61, 3)                                # include/gamd_hip.h: K = 61 for |n|^2 <= 9
    n2 = (kv * kv).sum(axis=1)
    keys = [(int(a), int(b), int(c), int(d)) for a, (b, c, d) in zip(n2, kv)]
    assert keys == sorted(keys) and n2.min() == 1 and n2.max() == 9
    both = {tuple(v) for v in kv} | {tuple(-v) for v in kv}
    assert len(both) == 2 * 61


# ---- ABI -------------------------------------------------------------------------------------------------------------
def test_water_params_layout_matches_a_c99_translation_unit(tmp_path):
    from gamd_amd._lib import WATER_ROW, GamdWaterParams
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed to read the header's layout"
    lines = "\n".join(f'    printf("{f} %lu\\n", (unsigned long)offsetof(gamd_water_params, {f}));' for f in FIELDS)
    src = tmp_path / "probe.c"
    src.write_text(PROBE.replace("@OFFSETS@", lines))
    exe = tmp_path / "probe"
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(GamdWaterParams) == int(out.pop("sizeof")) == 88
    assert int(out.pop("row")) == WATER_ROW == 12
    assert [n for n, _ in GamdWaterParams._fields_] == FIELDS and sorted(out) == sorted(FIELDS)
    for f in FIELDS:
        assert getattr(GamdWaterParams, f).offset == int(out[f]), f


def test_water_entry_points_are_declared_bound_and_exported(lib):
    from gamd_amd import _lib
    src = open(os.path.join(ROOT, "include", "gamd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gamd_water_configure", "gamd_water_reset", "gamd_water_read", "gamd_water_eval"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in _lib.SYMBOLS and hasattr(lib, name)


def test_configure_checks_its_parameter_block_before_it_needs_a_device(lib):
    from gamd_amd._lib import GamdWaterParams as P
    good = dict(interval=4, max_samples=0, q_h=0.417, sigma_o=3.15075, epsilon_o=0.635968, r_cut=9.5, r_switch=0.0, shift=0,
                reserved=0, alpha=0.5, k_cut=4.8, coulomb_const=138.935456)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(interval=-1), b"interval"), (dict(max_samples=-1), b"max_samples"), (dict(q_h=nan), b"q_h"),
             (dict(sigma_o=0.0), b"sigma_o"), (dict(sigma_o=-3.0), b"sigma_o"), (dict(sigma_o=nan), b"sigma_o"),
             (dict(epsilon_o=inf), b"epsilon_o"), (dict(r_cut=0.0), b"r_cut"), (dict(r_cut=-1.0), b"r_cut"),
             (dict(r_switch=-0.5), b"r_switch"), (dict(alpha=0.0), b"alpha"), (dict(alpha=nan), b"alpha"),
             (dict(k_cut=0.0), b"k_cut"), (dict(k_cut=inf), b"k_cut"), (dict(coulomb_const=nan), b"coulomb_const"),
             (dict(), b"null handle"),                         # a good block gets as far as the handle
             (dict(interval=0), b"null handle")]
    for change, word in cases:
        p = P(**{**good, **change})
        assert lib.gamd_water_configure(None, ctypes.byref(p)) == -22
        assert word in lib.gamd_last_error(), (word, lib.gamd_last_error())
    assert lib.gamd_water_configure(None, None) == -22
    assert lib.gamd_water_reset(None) == -22
    assert lib.gamd_water_read(None, None, None, None, 0, None, None, None, 0) == -22
    assert lib.gamd_water_eval(None, None, None, None, 0.0, None, None, None) == -22


# ---- RunWaterClassical -----------------------------------------------------------------------------------------------
def _synthetic():
    from gamd_amd.engine import RunWaterClassical
    steps = np.array([4, 8, 12])
    rows = np.zeros((3, 2, 12))
    rows[:, :, 0] = [[10.0, 5.0], [11.0, 6.0], [12.5, 7.0]]                   # u_lj
    rows[:, :, 1] = [[-80.0, -40.0], [-81.0, -41.0], [-82.0, -42.0]]          # u_real + u_excl
    rows[:, :, 2] = 3.0                                                       # u_recip
    rows[:, :, 3] = -33.0                                                     # u_self
    rows[:, :, 4] = 45.0
    rows[:, :, 5] = 60.0          # sum |D_ic| over 10 atoms x 3: mae 2
    rows[:, :, 6] = 270.0         # sum |D_i|^2: rmse 3
    rows[:, :, 7] = 4.0           # sum cos over 10 - 2 atoms: 0.5
    rows[:, :, 8] = 80.0          # sum |f_cl|: mean 8, relative mae 0.25
    rows[:, :, 9] = 70.0
    rows[:, :, 10] = 2.0
    rows[:, :, 11] = 0.0
    return RunWaterClassical(steps, rows, 10, dropped=1), rows


def test_columns_energy_and_force_errors_on_synthetic_rows():
    rc, rows = _synthetic()
    assert rc.dropped == 1 and len(rc.COLUMNS) == 12
    for k, name in enumerate(rc.COLUMNS):
        assert np.array_equal(getattr(rc, name), rows[:, :, k]), name
    assert np.array_equal(rc.energy, [[-100.0, -65.0], [-100.0, -65.0], [-99.5, -65.0]])
    fe = rc.force_errors()
    assert np.array_equal(fe["mae"], np.full((3, 2), 2.0)) and np.array_equal(fe["rmse"], np.full((3, 2), 3.0))
    assert np.array_equal(fe["cosine"], np.full((3, 2), 0.5)) and np.array_equal(fe["relative_mae"], np.full((3, 2), 0.25))
    ev = rc.force_errors(unit=0.0010364)
    assert np.allclose(ev["mae"], 2.0 * 0.0010364, rtol=1e-15) and np.array_equal(ev["cosine"], fe["cosine"])
    with pytest.raises(NotImplementedError, match="virial"):
        rc.pressure(np.zeros((3, 2)), 1.0)
    with pytest.raises(ValueError, match="rows"):
        type(rc)(rc.steps, rows[:, :, :9], 10)


def test_state_data_file_has_openmms_six_columns(tmp_path):
    from gamd_amd.engine import RunReport
    rc, _ = _synthetic()
    ke = np.array([[300.0, 30.0], [310.0, 31.0], [320.0, 32.0]])
    rep = RunReport(rc.steps, ke, ke / 3.0, np.zeros((2, 1, 0)), 0, 0)
    path = tmp_path / "log.txt"
    rc.write_state_data(rep, path, 0.0005, box=1)
    lines = path.read_text().splitlines()
    assert lines[0] == '#"Step"\t"Time (ps)"\t"Potential Energy (kJ/mole)"\t"Kinetic Energy (kJ/mole)"\t"Total Energy (kJ/mole)"\t"Temperature (K)"'
    got = np.array([[float(v) for v in l.split("\t")] for l in lines[1:]])
    assert got.shape == (3, 6)
    assert np.array_equal(got[:, 0], [4, 8, 12]) and np.allclose(got[:, 1], [0.002, 0.004, 0.006], rtol=1e-15)
    assert np.array_equal(got[:, 2], [-65.0, -65.0, -65.0]) and np.array_equal(got[:, 3], ke[:, 1])
    assert np.array_equal(got[:, 4], got[:, 2] + got[:, 3]) and np.array_equal(got[:, 5], ke[:, 1] / 3.0)
    other = RunReport(rc.steps + 1, ke, ke, np.zeros((2, 1, 0)), 0, 0)
    with pytest.raises(ValueError, match="step"):
        rc.write_state_data(other, path, 0.0005)
