"""The TIP4P M-site of the water classical potential (gamd_water_msite, gamd_amd/csrc/water_msite.hip) as far as it can be
seen without a GPU.

The host reference (tests/water_msite_ref.py) is judged on its own: with w = 0 it is water_classical_ref.evaluate; the
redistributed forces sum to zero over the box; they are the negative gradient of the reference's OWN energy with respect to
the three real atoms (central finite differences, independent of any device code); and the site of a hand-built molecule is
where the closed form puts it.  86 molecules from wl.water_box(86, seed=5, jitter=0.02, wrap=False), TIP4P-Ew parameters, r_cut
6.8, ewald_tol 1e-10.  Bars: the finite-difference bar 1e-7 of max |F| at h = 1e-4 Angstrom stands for truncation
h^2 U''' / 6 plus rounding eps U / h of an energy of a few 1e3 kJ/mol, with a margin for other seeds (a scratch version of
this reference gave 6.2e-9 on its coordinates; the eight drawn here give 1.3e-8).  The O-M
distance: 2 w r_OH cos(theta / 2) to 1e-12, and 0.125 Angstrom to 1e-9 — w is stated with nine decimals, so the distance it
implies is 0.125 only to 5e-10 * 2 r_OH cos(theta / 2) = 5.9e-10 (it comes out 3.2e-10 above).

The library: the entry point exists, the binding table carries it, a null handle is refused by name, and the seven new kernels
are in the release and the checked library under the prefix k_w4_ — tests/test_water_classical_resources.py counts exactly six
kernels with `k_water_` in the name — without scratch or a spilled register, within 16 KiB of LDS, the pair kernel within
k_water_pairs' bar of 168 vector registers and every other one within 128 (tools/kernel_resources.py)."""
import os
import sys

import numpy as np
import pytest

import water_classical_ref as wr
import water_msite_ref as w4
from gamd_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

VGPR_CAP = {"k_w4_sites": 128, "k_w4_pairs": 168, "k_w4_lj": 128, "k_w4_rho": 128, "k_w4_recip": 128, "k_w4_atoms": 128, "k_w4_drive": 128}


@pytest.fixture(scope="module")
def box86():
    pos, box, species, _ = wl.water_box(86, seed=5, jitter=0.02, wrap=False)
    wat, w = w4.tip4pew(r_cut=6.8, ewald_tol=1e-10)
    assert 2 * wat.r_cut <= np.float32(box)
    x = pos.astype(np.float32)
    return x, np.float32(box), species, wat, w, w4.evaluate(x, box, species, wat, w)


def test_weight_zero_is_the_three_site_reference(box86):
    x, box, species, wat, _, _ = box86
    a, b = w4.evaluate(x, box, species, wat, 0.0), wr.evaluate(x, box, species, wat)
    for name in ("energy", "u_lj", "u_coul", "u_recip", "u_self", "pairs", "sum_q"):
        assert a[name] == b[name], name
    print("w = 0: max |F - F_3site| =", np.abs(a["forces"] - b["forces"]).max())
    assert np.abs(a["forces"] - b["forces"]).max() <= 1e-11
    assert np.abs(a["abs_f"] - b["abs_f"]).max() <= 1e-11 * b["abs_f"].max()


def test_the_weight_changes_the_potential_and_the_forces_sum_to_zero(box86):
    x, box, species, wat, w, ref = box86
    three = wr.evaluate(x, box, species, wat)
    assert abs(ref["energy"] - three["energy"]) > 1e-3 * abs(three["energy"]) and ref["u_self"] == three["u_self"]
    assert ref["near"] == 0 and ref["near_lj"] == 0 and ref["sum_q"] == 0.0 and ref["pairs"] > 0
    total = np.abs(ref["forces"].sum(axis=0)).max()
    print(f"|sum F| = {total:.3e}, max |F| = {np.abs(ref['forces']).max():.3e}, sum abs_f = {ref['abs_f'].sum():.3e}")
    assert total <= 1e-12 * ref["abs_f"].sum()


def test_the_forces_are_the_negative_gradient_of_the_energy(box86):
    x, box, species, wat, w, ref = box86
    xd = x.astype(np.float64)
    fmax = np.abs(ref["forces"]).max()
    h, worst = 1e-4, 0.0
    rng = np.random.default_rng(17)
    # seeded coordinates, oxygens and both hydrogens.  Neither term is shifted, so U jumps where a pair crosses its cutoff (an
    # O-O pair by 0.03 kJ/mol: 1e3 kJ/mol/nm over 2 h): a coordinate whose two displaced frames do not hold the same pairs has
    # no derivative to compare with and the next draw takes its place
    done, skipped, k, seen = 0, 0, 0, set()
    while done < 8:
        i, c, k = int(3 * rng.integers(86) + k % 3), int(rng.integers(3)), k + 1
        if (i, c) in seen:
            continue
        seen.add((i, c))
        e, masks = [], []
        for s in (+1.0, -1.0):
            y = xd.copy()
            y[i, c] += s * h
            r = w4.evaluate(y, box, species, wat, w)
            e.append(r["energy"])
            masks.append((r["real_mask"], r["lj_mask"]))
        if not all(np.array_equal(a, b) for a, b in zip(*masks)):
            skipped += 1
            assert skipped <= 8
            continue
        done += 1
        fd = -(e[0] - e[1]) / (2.0 * h) * 10.0                                  # kJ/mol/Angstrom -> kJ/mol/nm
        worst = max(worst, abs(fd - ref["forces"][i, c]) / fmax)
        print(f"atom {i} ({'OHH'[i % 3]}) component {c}: F {ref['forces'][i, c]:+.9e}, -dU/dx {fd:+.9e}")
    print(f"largest |F + dU/dx| / max |F| = {worst:.3e} ({skipped} draws skipped: a pair crossed a cutoff)")
    assert worst <= 1e-7


def test_the_site_of_a_hand_built_molecule():
    r_oh, half = wl.TIP3P_R_OH, 0.5 * np.deg2rad(104.52)
    t, c = r_oh * np.cos(half), r_oh * np.sin(half)
    w = w4.TIP4PEW_W
    L = 20.0
    o1, o2 = np.array([3.0, 4.0, 5.0]), np.array([19.9, 0.2, 10.0])            # the second molecule straddles two faces of the box
    x = np.array([o1, o1 + [c, t, 0.0], o1 + [-c, t, 0.0],
                  o2, o2 + [0.0, -c, t] + np.array([0.0, L, 0.0]), o2 + [0.0, c, t] - np.array([L, 0.0, 0.0])])   # hydrogens in other images
    s = w4.sites(x, L, w)
    assert np.array_equal(s[[1, 2, 4, 5]], x[[1, 2, 4, 5]])
    assert np.abs(s[0] - (o1 + [0.0, 2.0 * w * t, 0.0])).max() <= 1e-12
    assert np.abs(s[3] - (o2 + [0.0, 0.0, 2.0 * w * t])).max() <= 1e-12          # in the oxygen's image
    for m in (0, 1):
        d_om = np.linalg.norm(s[3 * m] - x[3 * m])
        print(f"molecule {m}: |OM| = {d_om!r}")
        assert abs(d_om - 2.0 * w * t) <= 1e-12 and abs(d_om - 0.125) <= 1e-9
    # ... and the potential does not care which image an atom is given in
    wat, _ = w4.tip4pew(r_cut=6.8, ewald_tol=1e-10)
    y = x.copy()
    y[4] -= [0.0, L, 0.0]
    y[5] += [L, 0.0, 0.0]
    sp = np.array([1, 0, 0, 1, 0, 0])
    a, b = w4.evaluate(x, L, sp, wat, w), w4.evaluate(y, L, sp, wat, w)
    assert abs(a["energy"] - b["energy"]) <= 1e-12 * a["abs_energy"] and (np.abs(a["forces"] - b["forces"]) <= 1e-12 * a["abs_f"][:, None]).all()


# ---- the library -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from gamd_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_the_entry_point_is_exported_and_bound_and_refuses_a_null_handle_by_name(lib):
    from gamd_amd import _lib, engine
    assert hasattr(lib, "gamd_water_msite") and "gamd_water_msite" in _lib.SYMBOLS
    assert lib.gamd_water_msite(None, 0.106676721) == -22
    assert b"null handle" in lib.gamd_last_error()
    assert _lib.WATER_FORCE_SOURCE == {"water_classical": 2}                  # the M-site is no force source
    assert engine.TIP4PEW == dict(q_h=0.52422, sigma_o=3.16435, epsilon_o=0.680946, m_site=0.106676721)


def test_msite_kernels_are_in_both_libraries_within_their_bars(lib):
    from gamd_amd import _lib
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kr.kernel_resources(path).items() if "k_w4_" in n}
        assert len(res) == len(VGPR_CAP) and all(any(k + "(" in n for n in res) for k in VGPR_CAP), sorted(res)
        for n, v in res.items():
            short = next(k for k in VGPR_CAP if k + "(" in n)
            assert not any(p in n for p in ("k_water_", "k_wsrc_", "k_wmin_", "k_drive_", "k_classical_"))
            assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
            assert v.get("group_segment_fixed_size", 0) <= 16 * 1024, (n, v)
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= VGPR_CAP[short], (n, v)
            print(os.path.basename(path), short, "vgpr", v["vgpr_count"], "sgpr", v.get("sgpr_count"), "lds", v.get("group_segment_fixed_size", 0))
