"""The water L-BFGS energy minimiser on the device (gamd_water_minimize_lbfgs, gamd_amd/csrc/water_lbfgs.hip): the limited-memory
quasi-Newton direction and the backtracking line search of gamd_minimize_lbfgs on rigid 3-site molecules in double under the
water potential, leaving x and f as a water-source md_run / md_run_nhc expects them.  gamd_water_minimize (FIRE) is the yardstick
for the counts and is itself left alone.

What is asserted, and why the bars are what they are
* The f contract is bit equality (test_gpu_water_minimize._assert_f_contract): the returned f viewed as int32 equals
  water_classical_forces(x, species)[0].float() viewed as int32.  No tolerance is involved.
* Evaluation counts at tolerance 10 equal the float64 replay's (tests/water_lbfgs_ref.py): 78 at 86 molecules / r_cut 6.5
  (replayed in tests/test_water_lbfgs_host.py: rms 8.665 at the stop, 10.068 before it) and 61 at 258 molecules / r_cut 9.5 (rms
  8.852 at the stop, 10.782 before it; half a minute of replay on the CPU, so pinned here).  Neither rms is within 1e-6
  relative of the tolerance.  FIRE takes 100 and 86 iterations on these starts.
* Convergence is judged on the RETURNED fp32 positions: the rms of the projected classical force on x is at most tolerance +
  5.6e-4 kJ/mol/nm, the margin of tests/test_gpu_water_minimize.py.  Re-derived from this replay it would be ten times
  1.58e-5 (86 molecules; 5.5e-6 at 258, 5.9e-6 at tolerance 1) = 1.6e-4; the larger of the two is kept.
* Molecules of x64 are rigid to 1e-12 relative; x is the replay's wrap of x64 bit for bit, every oxygen in [0, L).
* Parity with the replay after K = 1 and K = 32 evaluations at 86 molecules, for the ring lengths 1, 6 and 8: the bars are 100
  times the replay's own spread under three molecule permutations (another summation order) and under a relative perturbation
  of every force component by 2^-50 xi, xi uniform in [-1, 1], with floors of 1e-13 A on x64 and 1e-13 relative on U and rms:
  the rule of tests/test_gpu_water_minimize.py.  The spreads come from the replay in this session, never from the device.
  State and the evaluation / accepted / skipped / reset counts at K are the replay's, exactly.
* Tolerance 1e-3 with r_switch = 5.5 at 86 molecules: converged within max_iter 2 000, and wm.projected_rms on the returned x64
  (the float64 reference potential) is at most tolerance (1 + 1e-3): the potential's parity bound of 1e-12 of the sums of
  absolute terms is about 1e-8 kJ/mol/nm here, 1e-5 of the tolerance, and the bar is a hundred times that.  No count is
  pinned: paths diverge at this depth.
* Same bits from two calls, a fresh handle, check_every = 1, 64 and 1000, the checked library, and for each box of a two-box
  handle whose boxes stop at different evaluations against that box alone.  x, x64 and the rows are compared across handles; f
  is held to its contract on each handle, because the k-vector list of a handle is built for the longest edge of all its boxes
  and the force source's k slices go by the list's length (tests/test_gpu_water_minimize.py).
* Nothing else moves: the network path's bits, a following FIRE call's bits, a following gamd_minimize_lbfgs on an LJ handle.

A frozen handle's refusal is not exercised: it would take a provoked neighbour-buffer overflow.  Starts are
wl.water_box(n_mol, seed, jitter=0, wrap=False) rounded to fp32; ewald_tol is test_gpu_water_classical.py's DELTA."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import water_classical_ref as wr
import water_lbfgs_ref as wlr
import water_minimize_ref as wm
from gamd_amd import workloads as wl
from test_gpu_classical_drive import _i32, _i64
from test_gpu_report import _state
from test_gpu_water_classical import _Water, DELTA
from test_gpu_water_drive import _assert_frames_carry_the_classical_force, _rattled
from test_gpu_water_minimize import (EDGES, MARGIN, _assert_f_contract, _assert_rigid_whole_and_wrapped, _projected_rms, _start,
                                     _water_engine)
from test_gpu_water_minimize import _bits as _fire_bits, _minimize as _fire_minimize

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHK = os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")
TOL = 10.0
STATES = ("converged", "max_iter", "failed", "line_search")
COUNT = {86: 78, 258: 61}                                       # the float64 replay's evaluations to tolerance 10
FIRE_COUNT = {86: 100, 258: 86}


def _lbfgs(eng, x0, species, box=None, **kw):
    """one call on a copy of x0: (result, x, f, x64) with the arrays on the host"""
    x = torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float32)).cuda()
    res = eng.water_minimize_lbfgs(x, species, box=box, return_x64=True, **kw)
    return res, x.cpu().numpy(), res.f.cpu().numpy(), res.x64.cpu().numpy()


def _bits(res, x, f, x64):
    return _i32(x).tolist(), _i32(f).tolist(), _i64(x64).tolist(), _i64(res.rows).tolist()


def _counts(res, b=0):
    return res.state[b], int(res.evaluations[b]), int(res.accepted[b]), int(res.skipped[b]), int(res.resets[b])


def _replay_counts(r):
    return STATES[r["state"]], r["evaluations"], r["accepted"], r["skipped"], r["resets"]


# ---- 1: convergence and contracts ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def minimized774():
    x0, box, species = _start(258)                              # two 256-molecule tiles with a tail of two; 774 atoms: four atom tiles
    eng = _water_engine(258, box, 9.5)
    res, x, f, x64 = _lbfgs(eng, x0, species, tolerance=TOL)
    fcl = _assert_f_contract(eng, x, f, species)
    eng.close()
    return dict(x0=x0, box=box, species=species, res=res, x=x, f=f, x64=x64, fcl=fcl)


def _check_converged(n_mol, m, tol=TOL):
    res = m["res"]
    rms32 = _projected_rms(m["x"], m["fcl"])
    print(f"{n_mol} molecules: {res!r}; U {res.energy_start[0]:.6f} -> {res.energy[0]:.6f}, rms {res.rms_start[0]:.6f} -> {res.rms[0]:.6f}, "
          f"fmax {res.fmax[0]:.4f}; counts {_counts(res)}; projected rms on the fp32 x {rms32:.6f} (|difference| {abs(rms32 - res.rms[0]):.3e})")
    assert res.status == 0 and res.converged and res.state == ["converged"]
    assert res.energy[0] < res.energy_start[0] and res.rms[0] <= tol < res.rms_start[0]
    _assert_rigid_whole_and_wrapped(m["x"], m["x64"], m["box"])
    assert rms32 <= tol + MARGIN
    # fmax is the largest per-atom norm of the projected force: at least the rms, at most sqrt(3N) times it
    assert res.rms[0] <= res.fmax[0] <= res.rms[0] * np.sqrt(9.0 * n_mol)


def test_86_molecules_converge_in_the_replays_count_and_meet_every_contract():
    x0, box, species = _start(86)                               # one molecule tile; 258 atoms: one 256-atom tile plus 2
    eng = _water_engine(86, box, 6.5)
    res, x, f, x64 = _lbfgs(eng, x0, species, tolerance=TOL)
    fcl = _assert_f_contract(eng, x, f, species)
    eng.close()
    _check_converged(86, dict(res=res, x=x, f=f, x64=x64, fcl=fcl, box=box))
    assert res.evaluations[0] == COUNT[86] <= FIRE_COUNT[86]


def test_258_molecules_converge_in_the_replays_count_and_meet_every_contract(minimized774):
    _check_converged(258, minimized774)                         # two molecule tiles with a tail of two
    assert minimized774["res"].evaluations[0] == COUNT[258] <= FIRE_COUNT[258]


def test_tolerance_1_converges_in_at_most_fires_count():
    x0, box, species = _start(86)
    eng = _water_engine(86, box, 6.5)
    res, x, f, x64 = _lbfgs(eng, x0, species, tolerance=1.0)
    fcl = _assert_f_contract(eng, x, f, species)
    eng.close()
    _check_converged(86, dict(res=res, x=x, f=f, x64=x64, fcl=fcl, box=box), tol=1.0)
    assert 0 < res.evaluations[0] <= 378                        # the FIRE replay's iterations (the L-BFGS replay: 188)


def test_a_switched_potential_converges_to_1e_3():
    x0, box, species = _start(86)
    eng = _water_engine(86, box, 6.5, r_switch=5.5)
    res, x, f, x64 = _lbfgs(eng, x0, species, tolerance=1e-3, max_iter=2000)
    _assert_f_contract(eng, x, f, species)
    eng.close()
    rms64, _ = wm.projected_rms(x64, box, species, wr.Water(r_cut=6.5, r_switch=5.5, ewald_tol=DELTA))
    print(f"r_switch = 5.5, tolerance 1e-3: {res!r}; counts {_counts(res)}; the float64 reference's projected rms on x64 {rms64:.6e} "
          f"(the device's {res.rms[0]:.6e})")
    assert res.status == 0 and res.state == ["converged"] and res.evaluations[0] <= 2000 and res.rms[0] <= 1e-3
    assert rms64 <= 1e-3 * (1.0 + 1e-3)
    _assert_rigid_whole_and_wrapped(x, x64, box)


# ---- 2: a run from the minimised start -------------------------------------------------------------------------------
def test_a_water_source_nhc_run_starts_from_the_minimised_box(minimized774):
    case = _Water("nhc")
    assert np.array_equal(case.pos.astype(np.float32), minimized774["x0"])
    eng, _, _, _ = case.make()
    eng.water_classical_configure(0, ewald_tol=DELTA)
    eng.md_force_source("water_classical")
    x, f = torch.from_numpy(minimized774["x"]).cuda(), torch.from_numpy(minimized774["f"]).cuda()
    v = torch.from_numpy(_rattled(minimized774["x"].astype(np.float64), case.species, 6)).float().cuda()
    steps = 12
    eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
    case.run(eng, x, v, f, steps)
    assert eng.last_status == 0
    tr = eng.traj_read()
    assert all(np.isfinite(a).all() for a in (tr.x, tr.v, tr.f))
    _assert_frames_carry_the_classical_force(eng, tr, x, f, case.species, steps)
    eng.close()


# ---- 3: parity with the float64 replay -------------------------------------------------------------------------------
_REPLAYS = {}


def _replay(K, m):
    """the replay after K evaluations from the 86-molecule start with a ring of m: as it is, under three molecule permutations,
    and with every force component perturbed by 2^-50 relative (computed once)"""
    if (K, m) not in _REPLAYS:
        x0, box, species = _start(86)
        w = wr.Water(r_cut=6.5, ewald_tol=DELTA)
        runs = []
        for kind, seed in (("base", None), ("perm", 1), ("perm", 2), ("perm", 3), ("perturb", 4)):
            p = np.random.default_rng(seed).permutation(86) if kind == "perm" else np.arange(86)
            a = (3 * p[:, None] + np.arange(3)[None, :]).reshape(-1)
            r = wlr.minimize(x0[a], box, species, w, 1e-300, max_iter=K, m=m,
                             perturb=np.random.default_rng(seed) if kind == "perturb" else None)
            xs = np.empty_like(r["x"])
            xs[a] = r["x"]
            runs.append(dict(x=xs, u=r["u"], rms=r["rms"], counts=_replay_counts(r)))
        base = runs[0]
        assert all(r["counts"] == base["counts"] for r in runs)
        spread_x = max(np.abs(r["x"] - base["x"]).max() for r in runs[1:])
        spread_u = max(abs(r["u"] - base["u"]) for r in runs[1:])
        spread_r = max(abs(r["rms"] - base["rms"]) for r in runs[1:])
        _REPLAYS[(K, m)] = dict(base=base, spread=(spread_x, spread_u, spread_r),
                                bar=(max(100.0 * spread_x, 1e-13), max(100.0 * spread_u, 1e-13 * abs(base["u"])),
                                     max(100.0 * spread_r, 1e-13 * base["rms"])))
    return _REPLAYS[(K, m)]


@pytest.mark.parametrize("K,m", [(1, 1), (1, 6), (1, 8), (32, 1), (32, 6), (32, 8)])
def test_positions_energy_and_rms_agree_with_the_float64_replay(K, m):
    x0, box, species = _start(86)
    rp = _replay(K, 6 if K == 1 else m)                         # the first evaluation has no history: one replay serves every m
    base, (spread_x, spread_u, spread_r), (bar_x, bar_u, bar_r) = rp["base"], rp["spread"], rp["bar"]
    eng = _water_engine(86, box, 6.5)
    res, x, f, x64 = _lbfgs(eng, x0, species, tolerance=1e-300, max_iter=K, m=m)
    _assert_f_contract(eng, x, f, species)
    eng.close()
    dx, du, dr = np.abs(x64 - base["x"]).max(), abs(res.energy[0] - base["u"]), abs(res.rms[0] - base["rms"])
    print(f"K = {K}, m = {m}: device against the replay: |dx| max {dx:.3e} A (replay's spread {spread_x:.3e}, bar {bar_x:.3e}); "
          f"|dU| {du:.3e} (spread {spread_u:.3e}, bar {bar_u:.3e}) at U = {base['u']:.9e}; "
          f"|drms| {dr:.3e} (spread {spread_r:.3e}, bar {bar_r:.3e}) at rms = {base['rms']:.9e}; counts {_counts(res)}")
    assert res.status == 1 and _counts(res) == base["counts"] and base["counts"][:2] == ("max_iter", K)
    assert dx <= bar_x
    assert du <= bar_u
    assert dr <= bar_r


# ---- 4: reproducibility and gating -----------------------------------------------------------------------------------
def test_two_calls_a_fresh_handle_and_every_check_every_give_the_same_bits():
    x0, box, species = _start(86)
    eng = _water_engine(86, box, 6.5)
    first = _lbfgs(eng, x0, species, tolerance=TOL)             # 78 evaluations: two chunks of 64
    assert first[0].status == 0 and first[0].evaluations[0] > 64
    ref = _bits(*first)
    assert _bits(*_lbfgs(eng, x0, species, tolerance=TOL)) == ref, "second call"
    eng.close()
    eng = _water_engine(86, box, 6.5)
    for every in (1, 64, 1000):
        assert _bits(*_lbfgs(eng, x0, species, tolerance=TOL, check_every=every)) == ref, f"check_every = {every}"
    eng.close()


def test_each_box_of_a_two_box_handle_gets_the_bits_it_gets_alone():
    (xa, ba, species), (xb, bb, _) = _start(86), _start(86, seed=6, edges=EDGES)
    boxes = np.stack([np.full(3, ba, dtype=np.float32), bb]).astype(np.float32)
    eng = _water_engine(86, float(ba), 6.5, n_boxes=2)
    res, x, f, x64 = _lbfgs(eng, np.concatenate([xa, xb]), species, box=boxes, tolerance=TOL)
    _assert_f_contract(eng, x, f, species, box=boxes)
    eng.close()
    print(f"two boxes: {res!r}")
    assert res.status == 0 and res.evaluations.tolist() == [COUNT[86], 67]    # one box stops first (the replay's counts)
    for b, (xs, box) in enumerate(((xa, ba), (xb, bb))):
        one = _water_engine(86, box, 6.5)
        r1, x1, f1, x641 = _lbfgs(one, xs, species, box=box, tolerance=TOL)
        _assert_f_contract(one, x1, f1, species, box=box)
        one.close()
        sl = slice(258 * b, 258 * (b + 1))
        assert np.array_equal(_i64(x64[sl]), _i64(x641)) and np.array_equal(_i64(res.rows[b]), _i64(r1.rows[0])), f"box {b}"
        assert np.array_equal(_i32(x[sl]), _i32(x1)), f"box {b}"


CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_water_lbfgs as t
from gamd_amd import _lib
print("RESULT", json.dumps(dict(version=_lib.load().gamd_version().decode(), bits=t._w86_bits())))
"""


def _w86_bits():
    x0, box, species = _start(86)
    eng = _water_engine(86, box, 6.5)
    out = _lbfgs(eng, x0, species, tolerance=TOL, max_iter=40, m=2)      # a ring of 2 wraps round many times in 40 evaluations
    eng.close()
    return [out[0].status, *_bits(*out)]


def test_checked_build_gives_the_same_bits():
    """the only values a k_wlb_* kernel reads from memory and then addresses with are the ring's two numbers in the state; the
    checked library range-checks them, finds nothing and must give the same bits (a failed check would come back as -35)"""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    env = {k: v for k, v in os.environ.items() if k not in ("GAMD_LIB", "GAMD_CHK_INJECT")}
    env["GAMD_LIB"] = CHK
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert p.returncode == 0 and "RESULT" in p.stdout, (p.stdout[-800:], p.stderr[-1500:])
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got["version"].endswith("checked")
    assert got["bits"] == _w86_bits() and got["bits"][0] == 1


# ---- 5: stops --------------------------------------------------------------------------------------------------------
def test_max_iter_stops_with_its_own_state_at_the_last_accepted_x():
    x0, box, species = _start(86)
    eng = _water_engine(86, box, 6.5)
    res, x, f, x64 = _lbfgs(eng, x0, species, tolerance=TOL, max_iter=5)
    _assert_f_contract(eng, x, f, species)
    eng.close()
    assert res.status == 1 and _counts(res) == ("max_iter", 5, 5, 0, 0) and not res.converged
    assert res.rms[0] > TOL and res.energy[0] < res.energy_start[0] and not np.array_equal(x, x0)
    _assert_rigid_whole_and_wrapped(x, x64, box)


def test_a_start_that_is_not_finite_fails_and_leaves_x_f_and_x64_alone():
    good, box, species = _start(86)
    x0 = good - np.float32(3.0)                                  # not wrapped: "as given" means as given
    x0[6:9] = x0[3:6]                                           # a molecule on another (tests/test_gpu_water_minimize.py)
    eng = _water_engine(86, box, 6.5)
    x = torch.from_numpy(x0).cuda()
    f = torch.full_like(x, 7.0)
    res = eng.water_minimize_lbfgs(x, species, f, tolerance=TOL, return_x64=True)
    assert res.status == 2 and _counts(res) == ("failed", 0, 0, 0, 0)
    assert np.array_equal(_i32(x.cpu().numpy()), _i32(x0))
    assert np.array_equal(f.cpu().numpy(), np.full_like(x0, 7.0))
    assert np.array_equal(res.x64.cpu().numpy(), x0.astype(np.float64))
    # the handle goes on: the same call on a sound start converges
    assert _lbfgs(eng, good, species, tolerance=TOL)[0].status == 0
    eng.close()


def test_a_start_below_the_tolerance_takes_no_evaluation():
    x0, box, species = _start(86)
    eng = _water_engine(86, box, 6.5)
    res, x, f, x64 = _lbfgs(eng, x0, species, tolerance=1e12)
    _assert_f_contract(eng, x, f, species)
    eng.close()
    assert res.status == 0 and _counts(res) == ("converged", 0, 0, 0, 0)
    assert res.energy[0] == res.energy_start[0] and res.rms[0] == res.rms_start[0]
    _assert_rigid_whole_and_wrapped(x, x64, box)                # the start put on the exact geometry, and nothing else
    assert np.abs(x64 - x0.astype(np.float64)).max() < 1e-5


# The first steepest step gains 0.093 of its linear prediction, so c1 above that rejects it.  In the replay every decision of
# these runs has |U_t - (U - c1 F.s)| >= 9e-4 |F.s|: far from rounding.
LINE_SEARCH_CASES = [(dict(max_ls=1, c1=0.9), ("line_search", 1, 0, 0, 0)),        # the first rejection, no history: stops at the start
                     (dict(max_ls=3, c1=0.3), ("line_search", 3, 0, 0, 0)),        # t = 1, 1/2, 1/4, then the stop
                     (dict(max_ls=1, c1=0.08), ("line_search", 15, 10, 0, 4)),     # four resets, then a rejection with the ring empty
                     (dict(max_ls=1, c1=0.08, max_iter=12), ("max_iter", 12, 9, 0, 2))]    # max_iter used up on a rejected trial


@pytest.mark.parametrize("kw,expect", LINE_SEARCH_CASES)
def test_line_search_failures_reset_the_history_and_stop_as_the_replay_does(kw, expect):
    x0, box, species = _start(86)
    r = wlr.minimize(x0, box, species, wr.Water(r_cut=6.5, ewald_tol=DELTA), 1e-300, **kw)
    assert _replay_counts(r) == expect
    eng = _water_engine(86, box, 6.5)
    res, x, f, x64 = _lbfgs(eng, x0, species, tolerance=1e-300, **kw)
    _assert_f_contract(eng, x, f, species)
    eng.close()
    dx = np.abs(x64 - r["x"]).max()
    print(f"{kw}: device {_counts(res)}, replay {_replay_counts(r)}; |dx| max {dx:.3e} A")
    assert _counts(res) == _replay_counts(r) and res.status == r["state"]
    assert dx <= _replay(32, 6)["bar"][0]
    _assert_rigid_whole_and_wrapped(x, x64, box)


# ---- 6: nothing else moves -------------------------------------------------------------------------------------------
def test_the_network_path_and_a_following_fire_call_are_untouched():
    case = _Water("baoab")
    ref_eng, xr, vr, fr = case.make()
    out0 = ref_eng.forward(xr, species=case.species).clone()
    x0 = xr.cpu().numpy()
    ref_eng.water_classical_configure(0, ewald_tol=DELTA)
    fire_ref = _fire_bits(*_fire_minimize(ref_eng, x0, case.species, tolerance=TOL, max_iter=20))   # a handle that never ran L-BFGS
    case.run(ref_eng, xr, vr, fr, 6)
    ref = _state(xr, vr, fr)
    ref_eng.close()

    eng, x, v, f = case.make()
    eng.water_classical_configure(0, ewald_tol=DELTA)
    other = x.clone()
    res = eng.water_minimize_lbfgs(other, case.species, tolerance=TOL, max_iter=20)
    assert res.status == 1 and not torch.equal(other, x)
    assert torch.equal(eng.forward(x, species=case.species), out0) and eng.force_source == "network"
    assert _fire_bits(*_fire_minimize(eng, x0, case.species, tolerance=TOL, max_iter=20)) == fire_ref
    case.run(eng, x, v, f, 6)
    for name, a, b in zip("xvf", ref, _state(x, v, f)):
        assert np.array_equal(_i32(a), _i32(b)), name
    eng.close()


def test_a_following_lennard_jones_lbfgs_call_gives_the_same_bits():
    from test_gpu_classical_drive import _seeded_engine
    from test_gpu_lbfgs import _bits as _lj_bits, _lbfgs as _lj_lbfgs
    from test_gpu_minimize import _golden_start

    def lj():
        x0, box = _golden_start()
        eng = _seeded_engine(258, box)
        out = _lj_bits(*_lj_lbfgs(eng, x0, tolerance=TOL))
        eng.close()
        return out

    before = lj()
    x0, box, species = _start(86)
    eng = _water_engine(86, box, 6.5)
    assert _lbfgs(eng, x0, species, tolerance=TOL, max_iter=10)[0].status == 1
    eng.close()
    assert lj() == before


# ---- 7: refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    import ctypes as C
    from gamd_amd._lib import GamdError, GamdLbfgsParams
    from gamd_amd.engine import GamdForce
    from gamd_amd.weights import SHIPPED_SCALERS
    from helpers import load_golden
    from test_gpu_report import _Case

    def raw(eng, x, f, flags):
        p = GamdLbfgsParams(tolerance=TOL)
        st = eng._lib.gamd_water_minimize_lbfgs(eng._h, C.c_void_p(x.data_ptr()), C.c_void_p(flags.data_ptr()) if flags is not None else None,
                                                eng._box_arg(None), 0.0, 0.0, 0.0, C.c_void_p(f.data_ptr()), None, C.byref(p), None, eng._stream())
        return st, eng._lib.gamd_last_error()

    # an LJ handle
    eng, x, v, f = _Case("lj").make()
    st, msg = raw(eng, x, f, None)
    assert st == -22 and b"GAMD_KIND_LJ" in msg and b"gamd_water_minimize_lbfgs" in msg
    eng.close()
    # an atom count that is no multiple of 3
    _, _, sd = load_golden("tip3p774_seed3")
    _, box, _, bonds = wl.water_box(85, seed=5, jitter=0.0, wrap=False)
    eng = GamdForce(sd, 257, box, 4.2, bond=bonds, scaler=SHIPPED_SCALERS["tip3p"])
    xx = torch.zeros((257, 3), dtype=torch.float32, device="cuda")
    st, msg = raw(eng, xx, xx.clone(), torch.ones(257, dtype=torch.uint8, device="cuda"))
    assert st == -22 and b"multiple of 3" in msg
    eng.close()

    case = _Water("baoab")
    eng, x, v, f = case.make()
    flags = torch.from_numpy(case.species).cuda()
    st, msg = raw(eng, x, f, flags)                                           # no parameters yet
    assert st == -22 and b"gamd_water_configure" in msg
    eng.water_classical_configure(0, ewald_tol=DELTA)
    case.run(eng, x, v, f, 2, sync=False)
    with pytest.raises(GamdError, match="-22.*enqueued.*gamd_water_minimize_lbfgs"):      # a run is pending
        eng.water_minimize_lbfgs(x, case.species, f, tolerance=TOL)
    assert eng.sync_status() == 0
    before = _state(x, v, f)
    with pytest.raises(GamdError, match="-22.*species"):
        eng.water_minimize_lbfgs(x, None, f, tolerance=TOL)
    with pytest.raises(GamdError, match="-22.*r_cut"):                       # a box edge below 2 r_cut
        eng.water_minimize_lbfgs(x, case.species, f, tolerance=TOL, box=0.9 * case.box)
    for bad, word in ((dict(r_oh=1.0, r_hh=2.0), "2 r_oh"), (dict(r_oh=1.0, r_hh=2.5), "2 r_oh"), (dict(r_oh=-1.0), "not positive"),
                      (dict(tolerance=0.0), "tolerance"), (dict(max_iter=-1), "max_iter"), (dict(check_every=-1), "check_every"),
                      (dict(m=9), "gamd_water_minimize_lbfgs: m is outside"), (dict(c1=1.0), "gamd_water_minimize_lbfgs: c1"),
                      (dict(max_step=-0.1), "max_step")):
        with pytest.raises(GamdError, match="-22.*" + word):
            eng.water_minimize_lbfgs(x, case.species, f, **{"tolerance": TOL, **bad})
    with pytest.raises(TypeError):
        eng.water_minimize_lbfgs(x, case.species, f, tolerance=TOL, dt_start=0.002)
    # the three forms of the potential that have no minimiser keep their status here, under this entry's name
    for kw, word in ((dict(m_site=0.128), "gamd_water_minimize_lbfgs: the TIP4P M-site is set"),
                     (dict(pme=(16, 32, 8)),"gamd_water_minimize_lbfgs: particle-mesh Ewald is on"),
                     (dict(cells=True), "gamd_water_minimize_lbfgs: the cell table is on")):
        eng.water_classical_configure(0, ewald_tol=DELTA, **kw)
        with pytest.raises(GamdError, match="-22.*" + word):
            eng.water_minimize_lbfgs(x, case.species, f, tolerance=TOL)
    for a, b in zip(before, _state(x, v, f)):                               # a refused call changed nothing
        assert np.array_equal(_i32(a), _i32(b))
    eng.close()
