"""The L-BFGS energy minimiser on the device (gamd_minimize_lbfgs, gamd_amd/csrc/lbfgs.hip): a limited-memory quasi-Newton
direction, a backtracking line search and FIRE's per-atom clamp, in double under the classical Lennard-Jones potential, leaving
x and f as a classical-source md_run / md_run_nhc expects them.  gamd_minimize (FIRE) is the yardstick for the counts and is
itself left alone.

What is asserted, and why the bars are what they are
* The f contract is bit equality: the returned f viewed as int32 equals classical_forces(x)[0].float() viewed as int32, for
  every size, start and ring length.  No tolerance is involved.
* Parity with the float64 replay (tests/lbfgs_ref.py) after K = 8 and K = 32 evaluations from lj258_seed0, for the ring lengths
  1, 6 and 8: the bar is 100 times the replay's own spread under three atom permutations (another summation order), with a
  floor of 1e-13 A on the positions and a relative floor of 1e-13 on U and rms — factor and floors of
  test_gpu_minimize.py::test_positions_energy_and_rms_agree_with_the_float64_replay.  The device's slice, thread and block
  order differs from numpy's by more than a permutation does, and the device runs the recursion on the ring's inner products
  where the replay runs it on the vectors (tests/test_lbfgs_host.py bounds that difference on the CPU by the same bar).
  State and the evaluation / accepted / skipped / reset counts at K are the replay's, exactly.
* Convergence: tolerance 10 in the replay's 23 evaluations; tolerances 1 and 1e-6 in at most the FIRE replay's 363 and 2 430
  iterations; no pair closer than 3.0 A; rms of classical_forces on the RETURNED fp32 positions at most tolerance + 1e-3
  kJ/mol/nm for the tolerances 10 and 1 (the margin of test_gpu_minimize.py: fp32 rounding of the positions).
* Same bits from two calls, a fresh handle, check_every = 1, 7 and 64, the checked library, and for each box of a two-box
  handle whose boxes stop at different evaluations.
* With the cell table on, states and counts at tolerance 10 are the all-pairs run's and the positions are within the parity
  bar of K = 32; the sums take another order there, so bits are not promised.
* Nothing else moves: the network forces of the handle, and the bits of a following FIRE call.

Random starts are uniform points in the box of wl.lj_box(n, seed=4), drawn with numpy's default_rng(4).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import classical_ref as cr
import lbfgs_ref as lr
import minimize_ref as mr
from gamd_amd import workloads as wl
from test_gpu_report import _Case, _state
from test_gpu_classical_drive import _assert_frames_carry_the_classical_force, _i32, _i64, _seeded_engine
from test_gpu_minimize import _assert_f_contract, _golden_start, _lattice_start, _nearest, _rms
from test_gpu_minimize import _bits as _fire_bits, _minimize as _fire_minimize

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHK = os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")
TOL = 10.0
STATES = ("converged", "max_iter", "failed", "line_search")
FIRE_COUNT = {1.0: 363, 1e-6: 2430}                             # the FIRE replay's iterations from lj258_seed0


def _lbfgs(eng, x0, box=None, **kw):
    """one call on a copy of x0: (result, x, f, x64) with the arrays on the host"""
    x = torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float32)).cuda()
    res = eng.minimize_lbfgs(x, box=box, return_x64=True, **kw)
    return res, x.cpu().numpy(), res.f.cpu().numpy(), res.x64.cpu().numpy()


def _bits(res, x, f, x64):
    return _i32(x).tolist(), _i32(f).tolist(), _i64(x64).tolist(), _i64(res.rows).tolist()


def _counts(res, b=0):
    return res.state[b], int(res.evaluations[b]), int(res.accepted[b]), int(res.skipped[b]), int(res.resets[b])


def _replay_counts(r):
    return STATES[r["state"]], r["evaluations"], r["accepted"], r["skipped"], r["resets"]


# ---- 1: parity with the float64 replay -------------------------------------------------------------------------------
_REPLAYS = {}


def _replay(K, m):
    """the replay after K evaluations from lj258_seed0 with a ring of m, and the same under three permutations (computed once)"""
    if (K, m) not in _REPLAYS:
        x0, box = _golden_start()
        runs = []
        for seed in (None, 1, 2, 3):
            p = np.arange(258) if seed is None else np.random.default_rng(seed).permutation(258)
            r = lr.minimize(x0[p], box, cr.LJ(), 1e-300, max_iter=K, m=m)
            xs = np.empty_like(r["x"])
            xs[p] = r["x"]
            runs.append(dict(x=xs, u=r["u"], rms=r["rms"], counts=_replay_counts(r)))
        base = runs[0]
        spread_x = max(np.abs(r["x"] - base["x"]).max() for r in runs[1:])
        spread_u = max(abs(r["u"] - base["u"]) for r in runs[1:])
        spread_r = max(abs(r["rms"] - base["rms"]) for r in runs[1:])
        _REPLAYS[(K, m)] = dict(base=base, spread=(spread_x, spread_u, spread_r),
                                bar=(max(100.0 * spread_x, 1e-13), max(100.0 * spread_u, 1e-13 * abs(base["u"])),
                                     max(100.0 * spread_r, 1e-13 * base["rms"])))
    return _REPLAYS[(K, m)]


@pytest.mark.parametrize("K,m", [(8, 6), (32, 6), (32, 1), (32, 8)])
def test_positions_energy_and_rms_agree_with_the_float64_replay(K, m):
    x0, box = _golden_start()
    rp = _replay(K, m)
    base, (spread_x, spread_u, spread_r), (bar_x, bar_u, bar_r) = rp["base"], rp["spread"], rp["bar"]
    eng = _seeded_engine(258, box)
    res, x, f, x64 = _lbfgs(eng, x0, tolerance=1e-300, max_iter=K, m=m)
    _assert_f_contract(eng, x, f)
    eng.close()
    dx, du, dr = np.abs(x64 - base["x"]).max(), abs(res.energy[0] - base["u"]), abs(res.rms[0] - base["rms"])
    print(f"K = {K}, m = {m}: device against the replay: |dx| max {dx:.3e} A (replay's spread {spread_x:.3e}, bar {bar_x:.3e}); "
          f"|dU| {du:.3e} (spread {spread_u:.3e}, bar {bar_u:.3e}) at U = {base['u']:.9e}; "
          f"|drms| {dr:.3e} (spread {spread_r:.3e}, bar {bar_r:.3e}) at rms = {base['rms']:.9e}; counts {_counts(res)}")
    assert res.status == 1 and _counts(res) == base["counts"] and base["counts"][:2] == ("max_iter", K)
    assert dx <= bar_x
    assert du <= bar_u
    assert dr <= bar_r


# ---- 2, 3: convergence, the start of a classical run, the forces -------------------------------------------------------
@pytest.fixture(scope="module")
def minimized():
    x0, box = _golden_start()
    eng = _seeded_engine(258, box)
    res, x, f, x64 = _lbfgs(eng, x0, tolerance=TOL)
    fcl = _assert_f_contract(eng, x, f)
    energy0 = eng.classical_forces(x0)[1]
    eng.close()
    return dict(x0=x0, box=box, res=res, x=x, f=f, x64=x64, fcl=fcl, energy0=energy0)


def test_lj258_seed0_converges_at_tolerance_10_in_the_replays_count(minimized):
    m, res = minimized, minimized["res"]
    print(f"lj258_seed0: {res!r}; U0 {res.energy_start[0]:.6e} rms0 {res.rms_start[0]:.6e} fmax {res.fmax[0]:.4f}; counts {_counts(res)}; "
          f"nearest pair {_nearest(m['x0'], m['box']):.3f} -> {_nearest(m['x'], m['box']):.3f} A; rms on the fp32 x {_rms(m['fcl']):.6f}")
    assert res.status == 0 and res.converged and res.state == ["converged"]
    assert res.evaluations[0] == 23                             # the float64 replay's count (tests/test_lbfgs_host.py)
    assert res.energy_start[0] > 1.0e7 and res.rms_start[0] > 3.0e7 and _nearest(m["x"], m["box"]) > 3.0
    assert res.energy[0] < res.energy_start[0] and res.rms[0] <= TOL and _rms(m["fcl"]) <= TOL + 1e-3
    assert 0.0 <= m["x"].min() and m["x"].max() < np.float32(m["box"])
    assert np.array_equal(m["x"], mr.wrap_fp32(m["x64"], m["box"]))
    # the start's pair pass is k_classical_pairs' walk and the sums above it take the same order
    assert np.array_equal(_i64(res.energy_start), _i64(m["energy0"]))


@pytest.mark.parametrize("tol", [1.0, 1e-6])
def test_tolerances_1_and_1e_6_converge_in_at_most_fires_counts(tol):
    x0, box = _golden_start()
    eng = _seeded_engine(258, box)
    res, x, f, x64 = _lbfgs(eng, x0, tolerance=tol)
    fcl = _assert_f_contract(eng, x, f)
    eng.close()
    print(f"tolerance {tol:g}: {res!r}; counts {_counts(res)}; FIRE's replay {FIRE_COUNT[tol]}; rms on the fp32 x {_rms(fcl):.6f}")
    assert res.status == 0 and res.state == ["converged"] and res.rms[0] <= tol
    assert 0 < res.evaluations[0] <= FIRE_COUNT[tol]
    assert _nearest(x, box) > 3.0
    if tol == 1.0:
        assert _rms(fcl) <= tol + 1e-3


def test_a_classical_nhc_run_starts_from_the_minimised_snapshot(minimized):
    case = _Case("lj", "nhc")
    eng, _, v, _ = case.make()
    x, f = torch.from_numpy(minimized["x"]).cuda(), torch.from_numpy(minimized["f"]).cuda()
    eng.classical_configure(0)
    eng.md_force_source("classical")
    steps = 12
    eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
    case.run(eng, x, v, f, steps)
    assert eng.last_status == 0
    tr = eng.traj_read()
    assert all(np.isfinite(a).all() for a in (tr.x, tr.v, tr.f))
    _assert_frames_carry_the_classical_force(eng, tr, x, f, steps)
    eng.close()


@pytest.mark.parametrize("n,m", [(64, 8), (300, 1)])
def test_a_tile_with_a_tail_and_more_than_one_tile(n, m):
    """64 atoms: below one 256-atom tile (box 17.1 A, r_cut 8.5); 300: one full tile plus 44, two block rows"""
    box = np.float32(wl.lj_box(n, seed=4)[1])
    lj = cr.LJ(r_cut=8.5, r_switch=5.1) if n == 64 else cr.LJ()
    assert 2 * lj.r_cut <= box
    x0 = (np.random.default_rng(4).random((n, 3)) * np.float64(box)).astype(np.float32)
    eng = _seeded_engine(n, float(box), cutoff=5.0 if n == 64 else 7.5)
    eng.classical_configure(0, **lj.kwargs())
    res, x, f, x64 = _lbfgs(eng, x0, tolerance=TOL, m=m)
    fcl = _assert_f_contract(eng, x, f)
    eng.close()
    r = lr.minimize(x0, float(box), lj, TOL, m=m)
    print(f"n = {n}, m = {m}: {res!r}; counts {_counts(res)}, the replay's {_replay_counts(r)}; rms on the fp32 x {_rms(fcl):.6f}")
    assert res.status == 0 and _counts(res) == _replay_counts(r)
    assert res.energy[0] < res.energy_start[0] and _rms(fcl) <= TOL + 1e-3
    assert np.array_equal(x, mr.wrap_fp32(x64, box)) and (x >= 0).all() and (x < box).all()


# ---- 4: reproducibility and gating -----------------------------------------------------------------------------------
def test_two_calls_a_fresh_handle_and_every_check_every_give_the_same_bits():
    x0, box = _golden_start()
    eng = _seeded_engine(258, box)
    first = _lbfgs(eng, x0, tolerance=1.0)                      # 195 evaluations in the replay: four chunks of 64
    assert first[0].status == 0 and first[0].evaluations[0] > 128
    ref = _bits(*first)
    assert _bits(*_lbfgs(eng, x0, tolerance=1.0)) == ref, "second call"
    eng.close()
    eng = _seeded_engine(258, box)
    for every in (1, 7, 64):
        assert _bits(*_lbfgs(eng, x0, tolerance=1.0, check_every=every)) == ref, f"check_every = {every}"
    eng.close()


def test_each_box_of_a_two_box_handle_gets_the_bits_it_gets_alone():
    (xa, ba), (xb, bb) = _golden_start(), _lattice_start()
    boxes = np.array([[ba] * 3, [bb] * 3], dtype=np.float32)
    eng = _seeded_engine(258, float(ba), n_boxes=2)
    res, x, f, x64 = _lbfgs(eng, np.concatenate([xa, xb]), box=boxes, tolerance=TOL)
    _assert_f_contract(eng, x, f, box=boxes)
    eng.close()
    assert res.status == 0 and res.evaluations.tolist() == [23, 3]      # one box stops first
    for b, (xs, box) in enumerate(((xa, ba), (xb, bb))):
        one = _seeded_engine(258, box)
        r1, x1, f1, x641 = _lbfgs(one, xs, tolerance=TOL)
        one.close()
        sl = slice(258 * b, 258 * (b + 1))
        assert np.array_equal(_i32(x[sl]), _i32(x1)) and np.array_equal(_i32(f[sl]), _i32(f1)), f"box {b}"
        assert np.array_equal(_i64(x64[sl]), _i64(x641)) and np.array_equal(_i64(res.rows[b]), _i64(r1.rows[0])), f"box {b}"


CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_lbfgs as t
from gamd_amd import _lib
print("RESULT", json.dumps(dict(version=_lib.load().gamd_version().decode(), bits=t._lj258_bits())))
"""


def _lj258_bits():
    x0, box = _golden_start()
    eng = _seeded_engine(258, box)
    out = _lbfgs(eng, x0, tolerance=TOL, m=2)                   # a ring of 2 wraps round many times in 23 evaluations
    eng.close()
    return [out[0].status, *_bits(*out)]


def test_checked_build_gives_the_same_bits():
    """the only values a k_lbfgs_* kernel reads from memory and then addresses with are the ring's two numbers in the state;
    the checked library range-checks them, finds nothing and must give the same bits (a failed check would come back as -35)"""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    env = {k: v for k, v in os.environ.items() if k not in ("GAMD_LIB", "GAMD_CHK_INJECT")}
    env["GAMD_LIB"] = CHK
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert p.returncode == 0 and "RESULT" in p.stdout, (p.stdout[-800:], p.stderr[-1500:])
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got["version"].endswith("checked")
    assert got["bits"] == _lj258_bits() and got["bits"][0] == 0


# ---- 5: the cell table -------------------------------------------------------------------------------------------------
def test_the_cell_table_gives_the_all_pairs_counts_and_positions_within_the_parity_bar():
    x0, box = _golden_start()
    bar_x = _replay(32, 6)["bar"][0]
    out = {}
    for cells in (False, True):
        eng = _seeded_engine(258, box)
        eng.classical_configure(0, cells=cells)
        res, x, f, x64 = _lbfgs(eng, x0, tolerance=TOL)
        _assert_f_contract(eng, x, f)
        eng.close()
        out[cells] = (res, x64)
    dx = np.abs(out[True][1] - out[False][1]).max()
    print(f"cells against all pairs at tolerance 10: counts {_counts(out[True][0])} / {_counts(out[False][0])}; |dx| max {dx:.3e} A (bar {bar_x:.3e})")
    assert out[True][0].status == 0 and _counts(out[True][0]) == _counts(out[False][0]) == ("converged", 23, 23, 0, 0)
    assert dx <= bar_x


# ---- 6: stops --------------------------------------------------------------------------------------------------------
def test_max_iter_stops_with_its_own_state():
    x0, box = _golden_start()
    eng = _seeded_engine(258, box)
    res, x, f, x64 = _lbfgs(eng, x0, tolerance=TOL, max_iter=5)
    _assert_f_contract(eng, x, f)
    eng.close()
    assert res.status == 1 and _counts(res) == ("max_iter", 5, 5, 0, 0) and not res.converged
    assert res.rms[0] > TOL and res.energy[0] < res.energy_start[0] and not np.array_equal(x, x0)


def test_two_atoms_at_one_point_fail_and_leave_x_and_f_alone():
    x0, box = _golden_start()
    x0 = x0 - np.float32(3.0)                                    # not wrapped: "as given" means as given
    x0[7] = x0[3]
    eng = _seeded_engine(258, box)
    x = torch.from_numpy(x0).cuda()
    f = torch.full_like(x, 7.0)
    res = eng.minimize_lbfgs(x, f, tolerance=TOL, return_x64=True)
    assert res.status == 2 and _counts(res) == ("failed", 0, 0, 0, 0)
    assert np.array_equal(_i32(x.cpu().numpy()), _i32(x0))
    assert np.array_equal(f.cpu().numpy(), np.full_like(x0, 7.0))
    assert np.array_equal(res.x64.cpu().numpy(), x0.astype(np.float64))
    # the handle goes on: the same call on a sound start converges
    good, _ = _golden_start()
    assert _lbfgs(eng, good, tolerance=TOL)[0].status == 0
    eng.close()


def test_a_start_below_the_tolerance_takes_no_evaluation():
    x0, box = _golden_start()
    eng = _seeded_engine(258, box)
    res, x, f, x64 = _lbfgs(eng, x0, tolerance=1e12)
    _assert_f_contract(eng, x, f)
    eng.close()
    assert res.status == 0 and _counts(res) == ("converged", 0, 0, 0, 0)
    assert np.array_equal(x64, x0.astype(np.float64)) and res.energy[0] == res.energy_start[0] and res.rms[0] == res.rms_start[0]


@pytest.mark.parametrize("start,kw", [("lj258_seed0", dict(max_ls=1, c1=0.9)),      # the first rejection, no history: stops at the start
                                      ("lattice", dict(max_ls=1, c1=0.07)),         # two resets, then a rejection with the ring empty
                                      ("lattice", dict(max_ls=1, c1=0.06, max_iter=32))])   # one reset on the way to max_iter
def test_line_search_failures_reset_the_history_and_stop_as_the_replay_does(start, kw):
    x0, box = _golden_start() if start == "lj258_seed0" else _lattice_start()
    r = lr.minimize(x0, box, cr.LJ(), 1e-300, **kw)
    eng = _seeded_engine(258, box)
    res, x, f, x64 = _lbfgs(eng, x0, tolerance=1e-300, **kw)
    _assert_f_contract(eng, x, f)
    eng.close()
    dx = np.abs(x64 - r["x"]).max()
    print(f"{start}, {kw}: device {_counts(res)}, replay {_replay_counts(r)}; |dx| max {dx:.3e} A")
    assert _counts(res) == _replay_counts(r) and res.status == r["state"]
    if "max_iter" not in kw:
        assert res.state == ["line_search"] and res.status == 3
        assert r["resets"] == (0 if start == "lj258_seed0" else 2)
    else:
        assert res.state == ["max_iter"] and r["resets"] == 1
    assert dx <= _replay(32, 6)["bar"][0]
    if r["accepted"] == 0:
        assert np.array_equal(x64, x0.astype(np.float64))


# ---- 7: nothing else moves -------------------------------------------------------------------------------------------
def test_the_network_path_and_a_following_fire_call_are_untouched():
    case = _Case("lj")
    ref_eng, xr, vr, fr = case.make()
    out0 = ref_eng.forward(xr).clone()
    fire_ref = _fire_bits(*_fire_minimize(ref_eng, xr.cpu().numpy(), tolerance=TOL))    # a handle that never ran L-BFGS
    ref_eng.close()

    eng, x, v, f = case.make()
    other = x.clone()
    res = eng.minimize_lbfgs(other, tolerance=TOL)
    assert res.status == 0 and not torch.equal(other, x)
    assert torch.equal(eng.forward(x), out0) and eng.force_source == "network"
    assert _fire_bits(*_fire_minimize(eng, x.cpu().numpy(), tolerance=TOL)) == fire_ref
    eng.close()


# ---- 8: refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    import ctypes as C
    from gamd_amd._lib import GamdError, GamdLbfgsParams

    def raw(eng, x, f, tolerance=TOL):
        p = GamdLbfgsParams(tolerance=tolerance)
        return eng._lib.gamd_minimize_lbfgs(eng._h, C.c_void_p(x.data_ptr()), eng._box_arg(None), 0.0, C.c_void_p(f.data_ptr()), None,
                                            C.byref(p), None, eng._stream()), eng._lib.gamd_last_error()

    water = _Case("water")
    eng, x, v, f = water.make()
    st, msg = raw(eng, x, f)
    assert st == -22 and b"GAMD_KIND_WATER" in msg
    eng.close()
    case = _Case("lj")
    eng, x, v, f = case.make()
    st, msg = raw(eng, x, f)                                                 # no parameters yet
    assert st == -22 and b"gamd_classical_configure" in msg
    eng.classical_configure(0)
    case.run(eng, x, v, f, 2, sync=False)
    with pytest.raises(GamdError, match="-22.*enqueued"):                   # a run is pending
        eng.minimize_lbfgs(x, f, tolerance=TOL)
    assert eng.sync_status() == 0
    before = _state(x, v, f)
    with pytest.raises(GamdError, match="-22.*r_cut"):                      # a box edge below 2 r_cut
        eng.minimize_lbfgs(x, f, tolerance=TOL, box=0.74 * case.box)
    for bad, word in ((dict(tolerance=0.0), "tolerance"), (dict(tolerance=float("nan")), "tolerance"), (dict(tolerance=float("inf")), "tolerance"),
                      (dict(max_iter=-1), "max_iter"), (dict(check_every=-1), "check_every"), (dict(m=-1), "m is outside"),
                      (dict(m=9), "m is outside"), (dict(c1=1.0), "c1"), (dict(c1=-0.1), "c1"), (dict(curv=-1e-3), "curv"),
                      (dict(max_ls=-1), "max_ls"), (dict(max_step=-0.1), "max_step")):
        with pytest.raises(GamdError, match="-22.*" + word):
            eng.minimize_lbfgs(x, f, **{"tolerance": TOL, **bad})
    with pytest.raises(TypeError):
        eng.minimize_lbfgs(x, f, tolerance=TOL, f_grow=1.1)
    for a, b in zip(before, _state(x, v, f)):                               # a refused call changed nothing
        assert np.array_equal(_i32(a), _i32(b))
    eng.close()
