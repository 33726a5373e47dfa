"""The water energy minimiser (gamd_water_minimize, gamd_amd/csrc/water_minimize.hip) as far as it can be seen without a GPU.

* The closed-form unit-weight SETTLE of the float64 replay (tests/water_minimize_ref.py, the arithmetic of gamd_wmin_dev.h)
  against the oracle's iterated SHAKE with unit weights.  The oracle stops when every |d^2 - r^2| / d^2 is below 1e-13, i.e.
  when a bond is within 0.5e-13 of its length relative; both solve the same equations (displacements along the reference
  bonds), so the positions may differ by that residual: the bar is ten times 1e-13 times the longest bond (r_hh), 1.5e-12 A.
  The replay's own bond lengths are exact to 1e-14 relative.
* The 3x3 projection against the oracle's iterated RATTLE with unit weights, which stops when every |r . (u_a - u_b)| is below
  1e-14: a component along a bond of at most 1e-14 / |r|.  The bar is ten times that for the shortest bond, 10 * 1e-14 / r_oh,
  on vectors of unit scale; after the projection r . (u_a - u_b) is zero to rounding on every bond (1e-14 for |r|, |u| ~ 1).
* The replay on the 86-molecule lattice start (seed 5, r_cut 6.5 A, ewald_tol 1e-8): U never increases from one evaluation
  to the next, it converges to tolerance 10 after exactly 100 position updates (the count the issue's prototype reached), and
  rms at the stop (9.743) and at the evaluation before it (11.050) are both far more than 1e-6 relative from the tolerance,
  so the device's count can be required to be equal.  (The 258-molecule start at r_cut 9.5 A takes 86 updates, rms 8.524
  after 11.019; a minute of replay, so it is pinned in tests/test_gpu_water_minimize.py and not replayed here.)
* The k_wmin_* kernels, in the release and the checked library: no scratch, no VGPR or SGPR spill, the pair kernel within the
  168 registers k_water_pairs is allowed, the others within 128, LDS within 12 KiB.
* The entry is exported and bound, and refuses bad parameter blocks, a bad geometry and a null handle by name."""
import ctypes
import os
import sys

import numpy as np
import pytest

import gamd_oracle as orc
import water_classical_ref as wr
import water_minimize_ref as wm
from gamd_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

DELTA = 1e-8                                                    # ewald_tol of tests/test_gpu_water_classical.py
R_OH, R_HH = wl.TIP3P_R_OH, wl.TIP3P_R_HH
ITER_86 = 100                                                   # the replay's count at tolerance 10 (asserted below)


@pytest.fixture(scope="module")
def lib():
    from gamd_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _displaced(n_mol, seed, amplitude):
    pos, _, _, _ = wl.water_box(n_mol, seed=seed, jitter=0.0, wrap=False)
    rng = np.random.default_rng(seed)
    return pos, pos + rng.uniform(-amplitude, amplitude, pos.shape)


# ---- SETTLE and the projection ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amplitude", [1e-3, 0.05, 0.1])
def test_settle_agrees_with_the_oracles_shake_with_unit_weights(amplitude):
    x0, x1 = _displaced(64, 11, amplitude)
    pairs, lengths = orc.water_constraints(x0.shape[0], R_OH, R_HH)
    ref = orc.shake_positions(x0, x1, np.ones(x0.shape[0]), pairs, lengths)
    got = wm.settle(x0, x1, R_OH, R_HH)
    bl = wm.bond_lengths(got)
    worst = np.abs(got - ref).max()
    print(f"amplitude {amplitude}: |SETTLE - SHAKE| max {worst:.3e} A (bar {10 * 1e-13 * R_HH:.3e}); bond lengths off by "
          f"{np.abs(bl[:, :2] / R_OH - 1).max():.3e}, {np.abs(bl[:, 2] / R_HH - 1).max():.3e} relative")
    assert worst <= 10 * 1e-13 * R_HH
    assert np.abs(bl[:, :2] / R_OH - 1).max() <= 1e-14 and np.abs(bl[:, 2] / R_HH - 1).max() <= 1e-14
    # unit weights: the centroid of every molecule stays where the unconstrained positions put it
    assert np.abs(got.reshape(-1, 3, 3).mean(axis=1) - x1.reshape(-1, 3, 3).mean(axis=1)).max() <= 1e-14


def test_settle_with_reference_equal_to_new_puts_an_fp32_start_on_the_geometry():
    pos, _, _, _ = wl.water_box(86, seed=5, jitter=0.0, wrap=False)
    x = pos.astype(np.float32).astype(np.float64)
    got = wm.settle(x, x, R_OH, R_HH)
    bl = wm.bond_lengths(got)
    assert np.abs(bl[:, :2] / R_OH - 1).max() <= 1e-14 and np.abs(bl[:, 2] / R_HH - 1).max() <= 1e-14
    assert np.abs(got - x).max() < 1e-5                        # the fp32 rounding of the start and no more
    bad = x.copy()
    bad[1] = bad[0]                                            # a hydrogen on its oxygen: not placeable
    assert not np.isfinite(wm.settle(bad, bad, R_OH, R_HH)[:3]).all() and np.isfinite(wm.settle(bad, bad, R_OH, R_HH)[3:]).all()


def test_projection_agrees_with_the_oracles_rattle_with_unit_weights():
    pos, _, _, _ = wl.water_box(64, seed=12, jitter=0.0, wrap=False)
    u = np.random.default_rng(12).normal(0.0, 1.0, pos.shape)
    pairs, _ = orc.water_constraints(pos.shape[0], R_OH, R_HH)
    ref = orc.rattle_velocities(pos, u, np.ones(pos.shape[0]), pairs)
    got = wm.project(pos, u)
    along = np.abs(((pos[pairs[:, 0]] - pos[pairs[:, 1]]) * (got[pairs[:, 0]] - got[pairs[:, 1]])).sum(axis=1)).max()
    print(f"|projection - RATTLE| max {np.abs(got - ref).max():.3e} (bar {10 * 1e-14 / R_OH:.3e}); r . du max {along:.3e}")
    assert np.abs(got - ref).max() <= 10 * 1e-14 / R_OH
    assert along <= 1e-14
    assert np.abs(wm.project(pos, got) - got).max() <= 1e-14   # a projection


# ---- the replay ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def replay86():
    pos, box, species, _ = wl.water_box(86, seed=5, jitter=0.0, wrap=False)
    w = wr.Water(r_cut=6.5, ewald_tol=DELTA)
    trace = []
    r = wm.minimize(pos.astype(np.float32), np.float32(box), species, w, 10.0, trace=trace)
    return dict(r=r, trace=trace, box=np.float32(box), species=species, w=w, x0=pos.astype(np.float32))


def test_replay_converges_on_the_86_molecule_lattice_start_and_u_never_increases(replay86):
    r, trace = replay86["r"], replay86["trace"]
    print(f"86 molecules: {r['iterations']} iterations, U {r['u0']:.6f} -> {r['u']:.6f}, rms {r['rms0']:.6f} -> {r['rms']:.6f} "
          f"(before the stop {trace[-2][1]:.6f}), dt {r['dt']:.6f}")
    assert r["state"] == wm.CONVERGED and r["iterations"] == ITER_86 == len(trace) - 1
    assert r["u"] < r["u0"] and all(b[0] <= a[0] for a, b in zip(trace, trace[1:]))
    assert r["rms"] <= 10.0 < trace[-2][1]
    for rms in (trace[-1][1], trace[-2][1]):                    # the device's count can be required to be equal
        assert abs(rms - 10.0) > 1e-6 * 10.0
    bl = wm.bond_lengths(r["x"])
    assert np.abs(bl[:, :2] / R_OH - 1).max() <= 1e-12 and np.abs(bl[:, 2] / R_HH - 1).max() <= 1e-12


def test_the_fp32_rounding_of_the_result_moves_the_projected_rms_by_less_than_the_gpu_tests_margin(replay86):
    """tests/test_gpu_water_minimize.py allows tolerance + 5.6e-4 on the returned fp32 x: ten times the largest
    |rms on fp32 x - rms on x64| of the replay, 5.6e-5 kJ/mol/nm on this start (8.2e-6 on the 258-molecule start)"""
    r, box, species, w = replay86["r"], replay86["box"], replay86["species"], replay86["w"]
    xf = wm.wrap_fp32(r["x"], box)
    rms32, _ = wm.projected_rms(xf, box, species, w)
    print(f"rms on the fp32 x {rms32:.9f}, on x64 {r['rms']:.9f}: |difference| {abs(rms32 - r['rms']):.3e}")
    assert abs(rms32 - r["rms"]) <= 5.6e-5
    o = xf.reshape(-1, 3, 3)[:, 0]
    assert (o >= 0).all() and (o < box).all()


def test_replay_stops_and_fails_as_the_header_says(replay86):
    x0, box, species, w = replay86["x0"], replay86["box"], replay86["species"], replay86["w"]
    r = wm.minimize(x0, box, species, w, 10.0, max_iter=5)
    assert r["state"] == wm.MAX_ITER and r["iterations"] == 5
    x1 = x0.copy()
    x1[6:9] = x1[3:6]                                           # atoms of different molecules at one point: a molecule on another
    r = wm.minimize(x1, box, species, w, 10.0)                  # (the same bits in, the same bits out of the first SETTLE)
    assert r["state"] == wm.FAILED and r["iterations"] == 0
    x1 = x0.copy()
    x1[4] = x1[3]                                               # a hydrogen on its oxygen
    r = wm.minimize(x1, box, species, w, 10.0)
    assert r["state"] == wm.FAILED and r["iterations"] == 0


def test_wrap_keeps_molecules_whole_and_sends_an_oxygen_that_rounds_up_to_the_edge_to_zero():
    box = np.float32(20.0)
    mol = np.array([[0.0, 0.0, 0.0], [0.9, 0.1, 0.0], [-0.3, 0.9, 0.0]])
    x = np.concatenate([mol + np.array([-0.5, 20.0, 45.25]), mol + np.array([-1e-9, 19.9999999, 20.0 - 1e-20])])
    wp = wm.wrap_fp32(x, box)
    assert wp.dtype == np.float32
    assert np.array_equal(wp[0], np.array([19.5, 0.0, 5.25], dtype=np.float32))
    assert np.array_equal(wp[3], np.zeros(3, dtype=np.float32))            # each component rounds up to L in fp32
    d = wp.reshape(2, 3, 3).astype(np.float64) - wp.reshape(2, 3, 3)[:, :1]
    assert np.abs(d - (mol - mol[:1])[None]).max() < 2e-6       # both hydrogens went with their oxygen
    o = wp.reshape(2, 3, 3)[:, 0]
    assert (o >= 0).all() and (o < box).all()


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_exported_bound_and_refuses_by_name(lib):
    from gamd_amd import _lib
    from gamd_amd._lib import GamdMinimizeParams as P
    assert hasattr(lib, "gamd_water_minimize") and "gamd_water_minimize" in _lib.SYMBOLS
    call = lambda p, r_oh=0.0, r_hh=0.0: lib.gamd_water_minimize(None, None, None, None, 0.0, r_oh, r_hh, None, None,
                                                                 None if p is None else ctypes.byref(p), None, None)
    assert call(P(tolerance=10.0)) == -22 and b"null handle" in lib.gamd_last_error()
    assert call(None) == -22 and b"null argument" in lib.gamd_last_error()
    for p, word in ((P(tolerance=0.0), b"tolerance"), (P(tolerance=1.0, max_iter=-1), b"max_iter"), (P(tolerance=1.0, f_dec=1.0), b"f_dec"),
                    (P(tolerance=1.0, max_step=-0.1), b"max_step")):
        assert call(p) == -22 and word in lib.gamd_last_error()
    assert call(P(tolerance=10.0), 1.0, 2.0) == -22 and b"2 r_oh" in lib.gamd_last_error()
    assert call(P(tolerance=10.0), 1.0, 2.5) == -22 and b"2 r_oh" in lib.gamd_last_error()
    assert call(P(tolerance=10.0), -1.0, 1.0) == -22 and b"not positive" in lib.gamd_last_error()
    assert call(P(tolerance=10.0), 1.0, float("nan")) == -22 and b"not positive" in lib.gamd_last_error()


# ---- kernels ---------------------------------------------------------------------------------------------------------------
KERNELS = ("k_wmin_init", "k_wmin_pairs", "k_wmin_rho", "k_wmin_recip", "k_wmin_mols", "k_wmin_update", "k_wmin_store_x")
VGPR_CAP = {"k_wmin_pairs": 168}                               # three waves per SIMD, as k_water_pairs; the others four or more
LDS_CAP = 12 * 1024


def test_wmin_kernels_use_no_scratch_and_spill_nothing_in_the_release_and_the_checked_library(lib):
    from gamd_amd import _lib
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kr.kernel_resources(path).items() if "k_wmin_" in n}
        assert len(res) == len(KERNELS) and all(any(k + "(" in n for n in res) for k in KERNELS), sorted(res)
        for n, v in res.items():
            short = next(k for k in KERNELS if k + "(" in n)
            assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
            assert v.get("group_segment_fixed_size", 0) <= LDS_CAP, (n, v)
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= VGPR_CAP.get(short, 128), (n, v)
