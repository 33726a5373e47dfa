"""Classical observer, host side (no device): the float64 reference of tests/classical_ref.py against itself (finite
differences, Newton's third law, continuity at r_switch and r_cut), the ABI of gamd_classical_params as a C99 compiler sees
it, the argument checks of gamd_classical_configure that are answered before any device work, and RunClassical's arithmetic
and file layout on synthetic arrays.  Nothing here claims parity with OpenMM: the default parameters are unverified."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import classical_ref as cr
from gamd_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ["interval", "max_samples", "sigma", "epsilon", "r_cut", "r_switch", "shift", "reserved"]

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "gamd_hip.h"
int main(void) {
    printf("sizeof %lu\n", (unsigned long)sizeof(gamd_classical_params));
    printf("row %d\n", (int)GAMD_CLASSICAL_ROW);
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


# ---- the reference against itself ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box300():
    pos, box = wl.lj_box(300, seed=4)
    return pos.astype(np.float32), box


def test_central_difference_of_the_energy_reproduces_the_forces(box300):
    """F = -dE/dx: a central difference with h = 1e-3 A on every component of 8 atoms spread over the box, within 1e-4 of the
    largest force component among them (truncation h^2 u''' / 6 and the rounding of E / h are both far below that)."""
    x32, box = box300
    lj = cr.LJ()
    assert 2 * lj.r_cut <= np.float32(box)
    x = x32.astype(np.float64)
    f = cr.evaluate(x, box, lj)["forces"] / 10.0                       # kJ/mol/A
    h, atoms = 1e-3, [0, 37, 74, 111, 148, 185, 255, 299]
    fd = np.zeros((len(atoms), 3))
    for a, i in enumerate(atoms):
        for c in range(3):
            xp, xm = x.copy(), x.copy()
            xp[i, c] += h
            xm[i, c] -= h
            fd[a, c] = -(cr.evaluate(xp, box, lj)["energy"] - cr.evaluate(xm, box, lj)["energy"]) / (2 * h)
    scale = np.abs(f[atoms]).max()
    err = np.abs(fd - f[atoms]).max() / scale
    print(f"central difference: max |F_fd - F| / max |F| = {err:.3e} (max |F| = {scale:.4f} kJ/mol/A)")
    assert scale > 0 and err <= 1e-4


@pytest.mark.parametrize("kw", [dict(), dict(shift=False), dict(r_switch=0.0), dict(shift=False, r_switch=0.0)])
def test_forces_sum_to_zero_and_virial_is_the_pair_sum(box300, kw):
    x, box = box300
    lj = cr.LJ(**kw)
    out = cr.evaluate(x, box, lj)
    assert out["pairs"] > 0 and out["near"] == 0
    assert np.abs(out["forces"].sum(axis=0)).max() <= 1e-12 * out["abs_f"].sum()
    # W = sum_{i<j} d . F_ij from the forces' own pair terms
    d, r2 = cr.min_image(x, box)
    np.fill_diagonal(r2, np.inf)
    inside = r2 < lj.rc2
    _, ru = lj.terms(np.where(inside, r2, 1.0))
    assert abs(out["virial"] - 0.5 * (-np.where(inside, ru, 0.0)).sum()) <= 1e-12 * out["abs_ru"]
    assert out["abs_u"] >= abs(out["energy"]) and out["abs_ru"] >= abs(out["virial"])


def test_u_and_du_are_continuous_at_r_switch_and_vanish_at_r_cut():
    lj = cr.LJ()
    assert lj.switching and lj.r_cut == pytest.approx(10.2) and lj.r_switch == pytest.approx(6.8)
    d = 1e-9
    (ua, ub), (dua, dub) = lj.u([lj.r_switch - d, lj.r_switch + d])
    # |u(rs + d) - u(rs - d)| <= 2 d max |u'| and the same for u' with u'': both ~1e-2 kJ/mol/A^k there
    assert abs(ua - ub) <= 1e-9 and abs(dua - dub) <= 1e-8
    (uc, uo), (duc, duo) = lj.u([lj.r_cut - d, lj.r_cut + d])
    assert uo == 0.0 and duo == 0.0
    # S ~ 10 (1 - t)^3 and S' ~ -30 (1 - t)^2 / w near t = 1: both vanish faster than d
    assert abs(uc) <= 1e-12 and abs(duc) <= 1e-12
    # unswitched and shifted: u vanishes at r_cut, u' does not; unshifted: neither does
    plain = cr.LJ(r_switch=0.0)
    (up,), (dup,) = plain.u([plain.r_cut - d])
    assert abs(up) <= 1e-9 and abs(dup) > 1e-5
    raw = cr.LJ(r_switch=0.0, shift=False)
    assert abs(raw.u([raw.r_cut - d])[0][0]) > 1e-4
    # the minimum sits at 2^(1/6) sigma with depth epsilon (inside r_switch nothing is switched; the shift lifts it by -u0)
    rm = 2.0 ** (1.0 / 6.0) * lj.sigma
    (um,), (dum,) = lj.u([rm])
    assert um == pytest.approx(-lj.epsilon - lj.u0, rel=1e-12) and abs(dum) <= 1e-12


# ---- ABI -------------------------------------------------------------------------------------------------------------
def test_classical_params_layout_matches_a_c99_translation_unit(tmp_path):
    from gamd_amd._lib import CLASSICAL_ROW, GamdClassicalParams
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed to read the header's layout"
    lines = "\n".join(f'    printf("{f} %lu\\n", (unsigned long)offsetof(gamd_classical_params, {f}));' for f in FIELDS)
    src = tmp_path / "probe.c"
    src.write_text(PROBE.replace("@OFFSETS@", lines))
    exe = tmp_path / "probe"
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(GamdClassicalParams) == int(out.pop("sizeof")) == 56
    assert int(out.pop("row")) == CLASSICAL_ROW == 9
    assert [n for n, _ in GamdClassicalParams._fields_] == FIELDS and sorted(out) == sorted(FIELDS)
    for f in FIELDS:
        assert getattr(GamdClassicalParams, f).offset == int(out[f]), f


def test_classical_entry_points_are_declared_bound_and_exported(lib):
    from gamd_amd import _lib
    src = open(os.path.join(ROOT, "include", "gamd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gamd_classical_configure", "gamd_classical_reset", "gamd_classical_read", "gamd_classical_eval"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in _lib.SYMBOLS and hasattr(lib, name)


def test_configure_checks_its_parameter_block_before_it_needs_a_device(lib):
    from gamd_amd._lib import GamdClassicalParams as P
    cases = [(P(-1, 0, 3.4, 1.0, 10.2, 6.8, 1, 0), b"interval"),
             (P(4, -1, 3.4, 1.0, 10.2, 6.8, 1, 0), b"max_samples"),
             (P(4, 0, 0.0, 1.0, 10.2, 6.8, 1, 0), b"sigma"),
             (P(4, 0, -3.4, 1.0, 10.2, 6.8, 1, 0), b"sigma"),
             (P(4, 0, float("nan"), 1.0, 10.2, 6.8, 1, 0), b"sigma"),
             (P(4, 0, 3.4, float("inf"), 10.2, 6.8, 1, 0), b"epsilon"),
             (P(4, 0, 3.4, 1.0, 0.0, 6.8, 1, 0), b"r_cut"),
             (P(4, 0, 3.4, 1.0, -1.0, 6.8, 1, 0), b"r_cut"),
             (P(4, 0, 3.4, 1.0, 10.2, -0.5, 1, 0), b"r_switch"),
             (P(4, 0, 3.4, 1.0, 10.2, 6.8, 1, 0), b"null handle"),      # a good block gets as far as the handle
             (P(0, 0, 3.4, 1.0, 10.2, 0.0, 0, 0), b"null handle")]
    for p, word in cases:
        assert lib.gamd_classical_configure(None, ctypes.byref(p)) == -22
        assert word in lib.gamd_last_error(), (word, lib.gamd_last_error())
    assert lib.gamd_classical_configure(None, None) == -22
    assert lib.gamd_classical_reset(None) == -22
    assert lib.gamd_classical_read(None, None, None, None, 0, None, None, None, 0) == -22
    assert lib.gamd_classical_eval(None, None, None, 0.0, None, None, None, None, None) == -22


# ---- RunClassical ----------------------------------------------------------------------------------------------------
def _synthetic():
    from gamd_amd.engine import RunClassical
    steps = np.array([4, 8, 12])
    rows = np.zeros((3, 2, 9))
    n = 10
    rows[:, :, 0] = [[-100.0, -50.0], [-101.0, -51.0], [-102.5, -52.0]]       # energy
    rows[:, :, 1] = [[30.0, 6.0], [33.0, 9.0], [36.0, 12.0]]                  # virial
    rows[:, :, 2] = 45.0
    rows[:, :, 3] = 60.0          # sum |D_ic| over 10 atoms x 3: mae 2
    rows[:, :, 4] = 270.0         # sum |D_i|^2: rmse sqrt(270 / 30) = 3
    rows[:, :, 5] = 4.0           # sum cos over 10 - 2 atoms: 0.5
    rows[:, :, 6] = 80.0          # sum |f_cl|: mean 8, relative mae 0.25
    rows[:, :, 7] = 70.0
    rows[:, :, 8] = 2.0
    return RunClassical(steps, rows, n, dropped=1), rows


def test_force_errors_are_the_notebooks_figures():
    rc, rows = _synthetic()
    assert rc.dropped == 1 and rc.energy.shape == (3, 2) and np.array_equal(rc.pairs, rows[:, :, 2])
    fe = rc.force_errors()
    assert np.array_equal(fe["mae"], np.full((3, 2), 2.0)) and np.array_equal(fe["rmse"], np.full((3, 2), 3.0))
    assert np.array_equal(fe["cosine"], np.full((3, 2), 0.5)) and np.array_equal(fe["relative_mae"], np.full((3, 2), 0.25))
    ev = rc.force_errors(unit=0.0010364)
    assert np.allclose(ev["mae"], 2.0 * 0.0010364, rtol=1e-15) and np.allclose(ev["rmse"], 3.0 * 0.0010364, rtol=1e-15)
    assert np.array_equal(ev["cosine"], fe["cosine"]) and np.array_equal(ev["relative_mae"], fe["relative_mae"])
    # the notebook's own arithmetic on explicit vectors (lj.ipynb cell 3), through classical_ref's sums
    rng = np.random.default_rng(0)
    gt, net = rng.normal(size=(7, 3)), rng.normal(size=(7, 3)).astype(np.float32)
    sums, _ = cr.force_error_sums(net, gt)
    from gamd_amd.engine import RunClassical
    one = RunClassical([1], np.concatenate([[0.0, 0.0, 0.0], sums])[None, None, :], 7).force_errors(unit=0.5)
    d = (net.astype(np.float64) - gt) * 0.5
    assert one["mae"][0, 0] == pytest.approx(np.abs(d).mean(axis=1).sum() / 7, rel=1e-14)
    assert one["rmse"][0, 0] == pytest.approx(np.sqrt((d ** 2).mean(axis=1).sum() / 7), rel=1e-14)
    cos = (net * gt).sum(axis=1) / (np.linalg.norm(net.astype(np.float64), axis=1) * np.linalg.norm(gt, axis=1))
    assert one["cosine"][0, 0] == pytest.approx(cos.mean(), rel=1e-13)
    assert one["relative_mae"][0, 0] == pytest.approx(np.abs(d).mean(axis=1).sum() / 7 / (0.5 * np.linalg.norm(gt, axis=1).mean()), rel=1e-13)


def test_pressure_is_the_virial_expression_in_bar():
    rc, _ = _synthetic()
    ke = np.array([[300.0, 30.0], [300.0, 30.0], [300.0, 30.0]])
    p = rc.pressure(ke, [20.0, 2.0])
    assert p.shape == (3, 2)
    assert p[0, 0] == pytest.approx(16.6053906717 * (600.0 + 30.0) / 60.0, rel=1e-15)
    assert p[2, 1] == pytest.approx(16.6053906717 * (60.0 + 12.0) / 6.0, rel=1e-15)
    # 1 kJ/mol/nm^3 in bar from the constants
    assert 16.6053906717 == pytest.approx(1e3 / 6.02214076e23 / 1e-27 / 1e5, rel=1e-10)
    assert np.array_equal(rc.pressure(ke, 20.0)[:, 0], p[:, 0])


def test_state_data_file_has_openmms_six_columns(tmp_path):
    from gamd_amd.engine import RunReport
    rc, _ = _synthetic()
    ke = np.array([[300.0, 30.0], [310.0, 31.0], [320.0, 32.0]])
    rep = RunReport(rc.steps, ke, ke / 3.0, np.zeros((2, 1, 0)), 0, 0)
    path = tmp_path / "log.txt"
    rc.write_state_data(rep, path, 0.002, box=1)
    lines = path.read_text().splitlines()
    assert lines[0] == '#"Step"\t"Time (ps)"\t"Potential Energy (kJ/mole)"\t"Kinetic Energy (kJ/mole)"\t"Total Energy (kJ/mole)"\t"Temperature (K)"'
    got = np.array([[float(v) for v in l.split("\t")] for l in lines[1:]])
    assert got.shape == (3, 6)
    assert np.array_equal(got[:, 0], [4, 8, 12]) and np.allclose(got[:, 1], [0.008, 0.016, 0.024], rtol=1e-15)
    assert np.array_equal(got[:, 2], [-50.0, -51.0, -52.0]) and np.array_equal(got[:, 3], ke[:, 1])
    assert np.array_equal(got[:, 4], got[:, 2] + got[:, 3]) and np.array_equal(got[:, 5], ke[:, 1] / 3.0)
    rc.write_state_data(rep, path, 0.002, separator=",", driver_step_convention=True)
    first = path.read_text().splitlines()[1].split(",")
    assert first[0] == "8" and float(first[1]) == 8 * 0.002 and float(first[2]) == -100.0
    # the reporter's own four-column file is unchanged
    rep.write_state_data(path, 0.002)
    assert len(path.read_text().splitlines()[1].split("\t")) == 4
    other = RunReport(rc.steps + 1, ke, ke, np.zeros((2, 1, 0)), 0, 0)
    with pytest.raises(ValueError, match="step"):
        rc.write_state_data(other, path, 0.002)
    short = RunReport(rc.steps[:2], ke[:2], ke[:2], np.zeros((2, 1, 0)), 0, 0)
    with pytest.raises(ValueError, match="step"):
        rc.write_state_data(short, path, 0.002)
