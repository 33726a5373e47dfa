"""The water L-BFGS energy minimiser (gamd_water_minimize_lbfgs, gamd_amd/csrc/water_lbfgs.hip) as far as it can be seen without
a GPU: the float64 replay of its recipe (tests/water_lbfgs_ref.py) converges from the 86-molecule lattice start at the
tolerances 10 and 1 on the default potential with no more evaluations than the FIRE replay (tests/water_minimize_ref.py) needs
iterations, keeps the line search's promises and the rigid geometry at every evaluation, takes the same count under molecule
permutations, and stops in each of its four states; with a switched Lennard-Jones term it converges to 1e-3; on the default
(truncated) term it does not get to 1e-4; the entry is exported, bound and refuses a null handle and bad parameter blocks by
name before it looks at the handle; the k_wlb_* kernels are in the release and the checked library without scratch and
without spills.

The start is wl.water_box(86, seed=5, jitter=0, wrap=False) rounded to fp32, r_cut 6.5, ewald_tol 1e-8 (the start, the
potential and the FIRE counts of tests/test_water_minimize_host.py and tests/test_gpu_water_minimize.py).  One run at tolerance
1 serves tolerance 10 as well: the tolerance only ends a run.

Numbers of the replay on this start (default potential, m = 6): 78 evaluations to tolerance 10 (rms 8.665 at the stop, 10.068 at
the accepted point before it), 188 to tolerance 1, one rejected trial, no reset; FIRE's replay takes 100 and 378 iterations.

The step bound: step 3 clamps every atom's displacement to max_step IN FRONT of SETTLE.  SETTLE then moves the atoms of a
molecule by a correction that is second order in the displacement: three points at most max_step from a rigid triangle miss its
bond lengths by O(max_step^2 / r), r the shortest bond.  With max_step = 0.1 A and r = r_oh = 0.9572 A that is about 0.0104 A;
the bar is max_step + 2 max_step^2 / r_oh = 0.1209 A, and the replay's largest |x_t - x| is printed (0.1105 A on this run)."""
import ctypes
import os
import sys

import numpy as np
import pytest

import water_classical_ref as wr
import water_lbfgs_ref as wlr
import water_minimize_ref as wm
from gamd_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

DELTA = 1e-8                                                    # ewald_tol of the water minimiser's tests
R_OH, R_HH = wm.TIP3P_R_OH, wm.TIP3P_R_HH
COUNT_AT_10 = 78                                                # evaluations to tolerance 10, the same under molecule permutations
FIRE_COUNT = {10.0: 100, 1.0: 378}                              # the FIRE replay's iterations on this start


@pytest.fixture(scope="module")
def lib():
    from gamd_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _start():
    pos, box, species, _ = wl.water_box(86, seed=5, jitter=0.0, wrap=False)
    return pos.astype(np.float32), np.float32(box), species


def _rigid(x):
    bl = wm.bond_lengths(x)
    return max(np.abs(bl[:, :2] / R_OH - 1).max(), np.abs(bl[:, 2] / R_HH - 1).max())


# ---- the replay ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run1():
    """the replay to tolerance 1 on the default potential with its trace"""
    x0, box, species = _start()
    trace = []
    r = wlr.minimize(x0, box, species, wr.Water(r_cut=6.5, ewald_tol=DELTA), 1.0, trace=trace)
    return dict(r=r, trace=trace)


def _count_to(trace, tol):
    """evaluations until the first accepted point with rms <= tol"""
    return next(k + 1 for k, e in enumerate(trace) if e["accepted"] and e["rms"] <= tol)


def test_replay_converges_at_10_and_1_with_at_most_fires_counts(run1):
    r, trace = run1["r"], run1["trace"]
    assert r["state"] == wlr.CONVERGED and r["rms"] <= 1.0 and r["evaluations"] == len(trace)
    assert r["accepted"] == sum(e["accepted"] for e in trace) and r["u"] < r["u0"]
    counts = {tol: _count_to(trace, tol) for tol in (10.0, 1.0)}
    acc = [e for e in trace[:counts[10.0]] if e["accepted"]]
    print(f"evaluations to 10 / 1: {counts[10.0]} / {counts[1.0]} (FIRE's replay {FIRE_COUNT[10.0]} / {FIRE_COUNT[1.0]}); accepted {r['accepted']}, "
          f"skipped {r['skipped']}, resets {r['resets']}; U {r['u0']:.6f} -> {r['u']:.6f}; rms at the tolerance-10 stop {acc[-1]['rms']:.6f}, "
          f"before it {acc[-2]['rms']:.6f}")
    assert counts[1.0] == r["evaluations"]
    assert counts[10.0] == COUNT_AT_10
    for tol in (10.0, 1.0):
        assert counts[tol] <= FIRE_COUNT[tol]
    assert acc[-1]["rms"] <= 10.0 < acc[-2]["rms"]
    for rms in (acc[-1]["rms"], acc[-2]["rms"]):                # the device's count can be required to be equal
        assert abs(rms - 10.0) > 1e-6 * 10.0


def test_every_evaluation_keeps_the_line_searchs_promises_and_the_geometry(run1):
    r, trace = run1["r"], run1["trace"]
    par = wlr.DEFAULTS
    bar = par["max_step"] + 2.0 * par["max_step"] ** 2 / R_OH   # the module's docstring
    u = r["u0"]
    worst_s = worst_b = 0.0
    for k, e in enumerate(trace):
        assert e["smax"] <= par["max_step"] * (1.0 + 1e-15), k  # in front of SETTLE no atom moves further than max_step
        assert e["smax_settled"] <= bar, k
        worst_s = max(worst_s, e["smax_settled"])
        assert e["u_from"] == u, k
        if e["accepted"]:
            assert e["fs"] > 0.0 and np.isfinite(e["u"]) and e["u"] <= u - par["c1"] * e["fs"], k     # step 5's inequality
            assert e["u"] <= u, k                               # U never rises from one accepted point to the next
            worst_b = max(worst_b, _rigid(e["x"]))
            u = e["u"]
    print(f"largest per-atom |x_t - x| {worst_s:.6f} A (bar {bar:.6f}); bonds of the accepted points off by {worst_b:.3e} relative at most")
    assert u == r["u"] and worst_b <= 1e-12


def test_the_count_at_tolerance_10_is_the_same_under_molecule_permutations():
    x0, box, species = _start()
    w = wr.Water(r_cut=6.5, ewald_tol=DELTA)
    for seed in (1, 2, 3):
        p = np.random.default_rng(seed).permutation(86)
        a = (3 * p[:, None] + np.arange(3)[None, :]).reshape(-1)
        r = wlr.minimize(x0[a], box, species, w, 10.0)
        assert r["state"] == wlr.CONVERGED and r["evaluations"] == COUNT_AT_10, seed


def test_replay_stops_in_each_of_its_states():
    x0, box, species = _start()
    w = wr.Water(r_cut=6.5, ewald_tol=DELTA)
    r = wlr.minimize(x0, box, species, w, 10.0, max_iter=5)
    assert r["state"] == wlr.MAX_ITER and r["evaluations"] == 5 and r["u"] < r["u0"] and _rigid(r["x"]) <= 1e-12
    x1 = x0.copy()
    x1[6:9] = x1[3:6]                                           # a molecule copied onto another (the same bits out of the first SETTLE)
    r = wlr.minimize(x1, box, species, w, 10.0)
    assert r["state"] == wlr.FAILED and r["evaluations"] == 0 and np.array_equal(r["x"], x1.astype(np.float64))
    r = wlr.minimize(x0, box, species, w, 1e12)                 # already below the tolerance
    assert r["state"] == wlr.CONVERGED and r["evaluations"] == 0 and r["u"] == r["u0"] and _rigid(r["x"]) <= 1e-12
    # the potential is convex along the first steepest step: the decrease falls short of 0.9 of the linear prediction, and one
    # rejection with an empty history ends the search.  The margin is far from rounding.
    trace = []
    r = wlr.minimize(x0, box, species, w, 10.0, max_ls=1, c1=0.9, trace=trace)
    e = trace[0]
    print(f"c1 = 0.9: U_t - U = {e['u'] - e['u_from']:.6f}, -c1 F.s = {-0.9 * e['fs']:.6f}")
    assert r["state"] == wlr.LINE_SEARCH and r["evaluations"] == 1 and r["accepted"] == 0
    assert e["fs"] > 0.0 and (e["u"] - e["u_from"]) - (-0.9 * e["fs"]) > 1e-6 * abs(e["fs"])


def test_a_switched_potential_converges_to_1e_3():
    """tolerances below about 1 need a continuous potential: with r_switch = 5.5 the replay converges to 1e-3 within 2 000
    evaluations (about 45 s on the CPU)"""
    x0, box, species = _start()
    r = wlr.minimize(x0, box, species, wr.Water(r_cut=6.5, r_switch=5.5, ewald_tol=DELTA), 1e-3, max_iter=2000)
    print(f"r_switch = 5.5, tolerance 1e-3: {r['evaluations']} evaluations, accepted {r['accepted']}, skipped {r['skipped']}, resets {r['resets']}; "
          f"rms {r['rms']:.3e}")
    assert r["state"] == wlr.CONVERGED and r["rms"] <= 1e-3 and r["evaluations"] <= 2000 and _rigid(r["x"]) <= 1e-12


def test_the_default_truncated_potential_does_not_get_to_1e_4():
    """the default Lennard-Jones term is cut at r_cut without a switch or a shift: an O-O pair that crosses 6.5 A changes U by
    about 0.03 kJ/mol, and once the steps gain less than that the sufficient-decrease test rejects every trial across the jump.
    The replay stops as line_search at rms 0.33 after 932 evaluations and 6 resets; the rejected trials of its last search all
    raise U by 0.0326 kJ/mol while F.s has fallen to 1e-5: nine orders of magnitude above rounding.  (90 s on the CPU.)"""
    x0, box, species = _start()
    trace = []
    r = wlr.minimize(x0, box, species, wr.Water(r_cut=6.5, ewald_tol=DELTA), 1e-4, max_iter=2000, trace=trace)
    last = trace[-1]
    print(f"default potential, tolerance 1e-4: state {r['state']}, {r['evaluations']} evaluations, accepted {r['accepted']}, resets {r['resets']}, "
          f"rms {r['rms']:.6f}; the last rejected trial: U_t - U = {last['u'] - last['u_from']:.6f} at F.s = {last['fs']:.3e}")
    assert r["state"] in (wlr.LINE_SEARCH, wlr.MAX_ITER) and r["rms"] > 1e-4
    if r["state"] == wlr.LINE_SEARCH:
        assert not last["accepted"] and last["u"] - last["u_from"] > 1e-3 > 100.0 * last["fs"]


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def _call(lib, p, r_oh=0.0, r_hh=0.0):
    return lib.gamd_water_minimize_lbfgs(None, None, None, None, 0.0, r_oh, r_hh, None, None, None if p is None else ctypes.byref(p), None, None)


def test_the_entry_is_exported_and_in_the_binding_table(lib):
    from gamd_amd import _lib
    from gamd_amd.engine import GamdForce
    assert hasattr(lib, "gamd_water_minimize_lbfgs") and "gamd_water_minimize_lbfgs" in _lib.SYMBOLS
    assert callable(GamdForce.water_minimize_lbfgs)


def test_a_null_handle_and_a_bad_parameter_block_are_refused_by_name_before_the_handle(lib):
    from gamd_amd._lib import GamdLbfgsParams as P
    assert _call(lib, P(tolerance=10.0)) == -22 and b"null handle" in lib.gamd_last_error()
    assert _call(lib, None) == -22 and b"null argument" in lib.gamd_last_error()
    cases = [(P(tolerance=0.0), b"tolerance"), (P(tolerance=float("nan")), b"tolerance"), (P(tolerance=1.0, max_iter=-1), b"max_iter"),
             (P(tolerance=1.0, check_every=-1), b"check_every"), (P(tolerance=1.0, m=-1), b"m is outside"),
             (P(tolerance=1.0, m=9), b"m is outside"), (P(tolerance=1.0, c1=1.0), b"c1"), (P(tolerance=1.0, curv=-1e-3), b"curv"),
             (P(tolerance=1.0, max_ls=-1), b"max_ls"), (P(tolerance=1.0, max_step=-0.1), b"max_step"), (P(tolerance=1.0, reserved=1), b"reserved")]
    for p, word in cases:
        assert _call(lib, p) == -22
        msg = lib.gamd_last_error()
        assert word in msg and msg.startswith(b"gamd_water_minimize_lbfgs:"), (word, msg)
    for m in (1, 8):                                            # the ends of the range pass the block's checks
        assert _call(lib, P(tolerance=1.0, m=m)) == -22 and b"null handle" in lib.gamd_last_error()
    # the geometry, as gamd_water_minimize refuses it, under this entry's name
    assert _call(lib, P(tolerance=10.0), 1.0, 2.0) == -22 and b"gamd_water_minimize_lbfgs: r_hh" in lib.gamd_last_error()
    assert _call(lib, P(tolerance=10.0), -1.0, 1.0) == -22 and b"not positive" in lib.gamd_last_error()
    # the Lennard-Jones entry's texts keep its own name
    assert lib.gamd_minimize_lbfgs(None, None, None, 0.0, None, None, ctypes.byref(P(tolerance=1.0, m=9)), None, None) == -22
    assert lib.gamd_last_error().startswith(b"gamd_minimize_lbfgs: m is outside")


# ---- kernels -------------------------------------------------------------------------------------------------------------
KERNELS = ("k_wlb_init", "k_wlb_mols", "k_wlb_update", "k_wlb_store_x")


def test_wlb_kernels_are_in_both_libraries_without_scratch_or_spills(lib):
    """the molecule pass carries 35 double accumulators per thread beside three atoms' positions, forces, s and y, and the
    decide/update pass the recursion's coefficients and SETTLE: both stay in registers (no private segment, no spilled vector
    or scalar register) inside the 256 registers a 256-thread workgroup may have with two waves per SIMD"""
    from gamd_amd import _lib
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kr.kernel_resources(path).items() if "k_wlb_" in n}
        assert len(res) == len(KERNELS) and all(any(k + "(" in n for n in res) for k in KERNELS), sorted(res)
        for n, v in res.items():
            assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
            assert v.get("group_segment_fixed_size", 0) <= 2 * 1024, (n, v)
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= 256, (n, v)
