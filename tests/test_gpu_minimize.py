"""The energy minimiser on the device (gamd_minimize, gamd_amd/csrc/minimize.hip): FIRE in double under the classical
Lennard-Jones potential, leaving x and f as a classical-source md_run / md_run_nhc expects them.

What is asserted, and why the bars are what they are
* The f contract is bit equality: the returned f viewed as int32 equals classical_forces(x)[0].float() viewed as int32, for
  every size, start and potential form.  No tolerance is involved.
* Convergence is judged on the RETURNED fp32 positions: the RMS of classical_forces(x) is at most tolerance + 1e-3 kJ/mol/nm.
  The 1e-3 covers the rounding of the double positions to fp32: the floor of the RMS force of fp32-rounded minima seen on the
  CPU is 1e-4, and the margin is ten times that.
* Parity with the float64 replay (tests/minimize_ref.py) after K = 1 and K = 64 iterations: the bar is 100 times the replay's
  own spread under three atom permutations (another summation order), with a floor of 1e-13 A on the positions.  The device's
  slice, thread and block order differs from numpy's by more than a permutation does, hence the factor; sqrt, division and
  rint are correctly rounded on both sides.  U and rms get the same factor with a relative floor of 1e-13: about 1000 ulp, for
  sums of 3e4 terms whose order differs (a permutation can leave a sum's rounded value unchanged, i.e. a spread of zero).
* The minimised lj258_seed0 snapshot starts the classical-source runs that tests/test_gpu_classical_drive.py had to start from
  a lattice: every frame of 12 steps carries fp32(classical_forces(x)) bit for bit, and three steps agree with the oracle's
  float64 integrators within that file's bars (1e-5 on x, 1e-4 on v) after the same CPU pre-check (an fp32 emulation against
  the float64 replay), which passes on the minimised start: rel_err x 1.6e-7 / v 2.5e-7 (BAOAB), 8.4e-8 / 1.7e-7 (NHC).
* energy_start equals the energy classical_forces gives on the same fp32 start, bit for bit (258 atoms; a two-box handle): the
  minimiser's pair pass and the observer's are one walk, and the sums above it take the same order.  No tolerance is involved.
* Same bits from two calls, a fresh handle, check_every = 1, 64 and 1000, the checked library, and for each box of a two-box
  handle whose boxes stop at different iterations.

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
import minimize_ref as mr
from gamd_amd import workloads as wl
from gamd_amd.weights import SHIPPED_SCALERS
from helpers import load_golden, rel_err
from test_gpu_report import _Case, _state
from test_gpu_classical_drive import (_assert_frames_carry_the_classical_force, _emulate_f32, _i32, _i64, _replay_f64,
                                      _seeded_engine, DT, MASS, GAMMA, FREQ, CHAIN)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHK = os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")
TOL = 10.0


def _golden_start():
    g, _, _ = load_golden("lj258_seed0")
    box = float(g["box"])
    return np.mod(g["pos"], box).astype(np.float32), box


def _lattice_start():
    pos, box = wl.lj_box(258)
    return pos.astype(np.float32), box


def _nearest(x, box):
    _, r2 = cr.min_image(x, box)
    return float(np.sqrt(r2[np.triu_indices(x.shape[0], 1)].min()))


def _rms(f):
    f = np.asarray(f, dtype=np.float64)
    return float(np.sqrt((f * f).sum() / f.size))


def _minimize(eng, x0, box=None, **kw):
    """one call on a copy of x0: (result, x, f, x64) with the arrays on the host"""
    x = torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float32)).cuda()
    res = eng.minimize(x, box=box, return_x64=True, **kw)
    return res, x.cpu().numpy(), res.f.cpu().numpy(), res.x64.cpu().numpy()


def _assert_f_contract(eng, x, f, box=None):
    fcl = eng.classical_forces(x, box=box)[0]
    assert torch.isfinite(fcl).all() and float(fcl.abs().max()) > 0.0
    assert np.array_equal(_i32(f), _i32(fcl.float().cpu().numpy()))
    return fcl.cpu().numpy()


def _bits(res, x, f, x64):
    return _i32(x).tolist(), _i32(f).tolist(), _i64(x64).tolist(), _i64(res.rows).tolist()


# ---- 1: the snapshot a classical run could not start from ------------------------------------------------------------
@pytest.fixture(scope="module")
def minimized():
    x0, box = _golden_start()
    eng = _seeded_engine(258, box)
    res, x, f, x64 = _minimize(eng, x0, tolerance=TOL)
    fcl = _assert_f_contract(eng, x, f)
    eng.close()
    return dict(x0=x0, box=box, res=res, x=x, f=f, x64=x64, fcl=fcl)


def test_lj258_seed0_converges_to_a_start_without_overlaps(minimized):
    m, res = minimized, minimized["res"]
    print(f"lj258_seed0: {res!r}; U0 {res.energy_start[0]:.6e} rms0 {res.rms_start[0]:.6e} fmax {res.fmax[0]:.4f} dt {res.dt[0]:.5f}; "
          f"nearest pair {_nearest(m['x0'], m['box']):.3f} -> {_nearest(m['x'], m['box']):.3f} A; rms on the fp32 x {_rms(m['fcl']):.6f}")
    assert res.status == 0 and res.converged and res.state == ["converged"]
    assert _nearest(m["x0"], m["box"]) < 1.2 and res.energy_start[0] > 1.0e7 and res.rms_start[0] > 3.0e7
    assert _nearest(m["x"], m["box"]) > 3.0
    assert res.energy[0] < res.energy_start[0] and res.rms[0] <= TOL
    assert _rms(m["fcl"]) <= TOL + 1e-3
    assert res.iterations[0] == 17                              # the float64 replay's count (tests/test_minimize_host.py)
    assert 0.0 <= m["x"].min() and m["x"].max() < np.float32(m["box"])
    assert np.array_equal(m["x"], mr.wrap_fp32(m["x64"], m["box"]))


@pytest.mark.parametrize("integrator", ["nhc", "baoab"])
def test_a_classical_run_starts_from_the_minimised_snapshot(minimized, integrator):
    """the test the classical force source had to move to a lattice: 12 steps from the minimised lj258_seed0 with the golden
    snapshot's weights, velocities and integrator settings (BAOAB: gamma = 25 / ps, 100 K, noise on)"""
    case = _Case("lj", integrator)
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


@pytest.mark.parametrize("integrator", ["baoab", "nhc"])
def test_three_steps_from_the_minimised_snapshot_match_the_oracle_integrators(minimized, integrator):
    x0, box, lj, steps = minimized["x"], minimized["box"], cr.LJ(), 3
    v0 = np.random.default_rng(1).normal(0, 1.4, x0.shape).astype(np.float32)
    f0 = cr.evaluate(x0, box, lj)["forces"].astype(np.float32)
    xr, vr = _replay_f64(integrator, x0, v0, f0, box, steps)
    xe, ve = _emulate_f32(integrator, x0, v0, f0, box, steps)    # on the CPU first: fp32 state can stay inside the bars at all
    print(f"{integrator}: fp32 emulation against the float64 replay: rel_err x {rel_err(xe, xr):.3e}, v {rel_err(ve, vr):.3e}")
    assert rel_err(xe, xr) < 1e-5 and rel_err(ve, vr) < 1e-4
    from gamd_amd.engine import GamdForce
    _, _, sd = load_golden("lj258_seed0")
    eng = GamdForce(sd, 258, box, 7.5, scaler=SHIPPED_SCALERS["lj"])
    x, v, f = torch.from_numpy(x0).cuda(), torch.from_numpy(v0).cuda(), torch.from_numpy(minimized["f"]).cuda()
    eng.classical_configure(0)
    eng.md_force_source("classical")
    assert rel_err(minimized["f"], f0) < 1e-6
    if integrator == "baoab":
        eng.md_run(x, v, f, steps, dt_ps=DT, mass_amu=MASS, temperature_k=0.0, gamma_per_ps=GAMMA)
    else:
        eng.md_run_nhc(x, v, f, steps, dt_ps=DT, mass_amu=MASS, temperature_k=100.0, frequency_per_ps=FREQ, chain_length=CHAIN)
    ex, ev = rel_err(x.cpu().numpy(), xr), rel_err(v.cpu().numpy(), vr)
    print(f"{integrator}: device against the float64 replay: rel_err x {ex:.3e}, v {ev:.3e}")
    assert ex < 1e-5
    assert ev < 1e-4
    eng.close()


# ---- 3: parity with the float64 replay -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def replay64():
    """the replay at K = 64 from lj258_seed0 with the state behind iteration 1 kept, and the same under three permutations"""
    x0, box = _golden_start()
    runs = []
    for seed in (None, 1, 2, 3):
        p = np.arange(258) if seed is None else np.random.default_rng(seed).permutation(258)
        out = {}
        for K in (1, 64):                                       # (K = 1 costs two evaluations)
            r = mr.minimize(x0[p], box, cr.LJ(), 1e-300, max_iter=K)
            xs = np.empty_like(r["x"])
            xs[p] = r["x"]
            out[K] = dict(x=xs, u=r["u"], rms=r["rms"], state=r["state"], iterations=r["iterations"])
        runs.append(out)
    return runs


@pytest.mark.parametrize("K", [1, 64])
def test_positions_energy_and_rms_agree_with_the_float64_replay(replay64, K):
    x0, box = _golden_start()
    base = replay64[0][K]
    spread_x = max(np.abs(r[K]["x"] - base["x"]).max() for r in replay64[1:])
    spread_u = max(abs(r[K]["u"] - base["u"]) for r in replay64[1:])
    spread_r = max(abs(r[K]["rms"] - base["rms"]) for r in replay64[1:])
    bar_x = max(100.0 * spread_x, 1e-13)
    bar_u, bar_r = max(100.0 * spread_u, 1e-13 * abs(base["u"])), max(100.0 * spread_r, 1e-13 * base["rms"])
    eng = _seeded_engine(258, box)
    res, x, f, x64 = _minimize(eng, x0, tolerance=1e-300, max_iter=K)
    _assert_f_contract(eng, x, f)
    eng.close()
    dx, du, dr = np.abs(x64 - base["x"]).max(), abs(res.energy[0] - base["u"]), abs(res.rms[0] - base["rms"])
    print(f"K = {K}: device against the replay: |dx| max {dx:.3e} A (replay's spread {spread_x:.3e}, bar {bar_x:.3e}); "
          f"|dU| {du:.3e} (spread {spread_u:.3e}, bar {bar_u:.3e}) at U = {base['u']:.9e}; "
          f"|drms| {dr:.3e} (spread {spread_r:.3e}, bar {bar_r:.3e}) at rms = {base['rms']:.9e}")
    assert res.status == 1 and res.state == ["max_iter"] and res.iterations[0] == K == base["iterations"]
    assert dx <= bar_x
    assert du <= bar_u
    assert dr <= bar_r


# ---- 4: reproducibility and gating -----------------------------------------------------------------------------------
def test_two_calls_a_fresh_handle_and_every_check_every_give_the_same_bits():
    x0, box = _golden_start()
    eng = _seeded_engine(258, box)
    first = _minimize(eng, x0, tolerance=1.0)                   # 363 iterations in the replay: six chunks of 64
    assert first[0].status == 0 and first[0].iterations[0] > 128
    ref = _bits(*first)
    assert _bits(*_minimize(eng, x0, tolerance=1.0)) == ref, "second call"
    eng.close()
    eng = _seeded_engine(258, box)
    for every in (1, 64, 1000):
        assert _bits(*_minimize(eng, x0, tolerance=1.0, check_every=every)) == ref, f"check_every = {every}"
    eng.close()


def test_each_box_of_a_two_box_handle_gets_the_bits_it_gets_alone():
    (xa, ba), (xb, bb) = _golden_start(), _lattice_start()
    boxes = np.array([[ba] * 3, [bb] * 3], dtype=np.float32)
    eng = _seeded_engine(258, float(ba), n_boxes=2)
    res, x, f, x64 = _minimize(eng, np.concatenate([xa, xb]), box=boxes, tolerance=TOL)
    _assert_f_contract(eng, x, f, box=boxes)
    eng.close()
    assert res.status == 0 and res.iterations.tolist() == [17, 26]      # one box stops first
    for b, (xs, box) in enumerate(((xa, ba), (xb, bb))):
        one = _seeded_engine(258, box)
        r1, x1, f1, x641 = _minimize(one, xs, tolerance=TOL)
        one.close()
        sl = slice(258 * b, 258 * (b + 1))
        assert np.array_equal(_i32(x[sl]), _i32(x1)) and np.array_equal(_i32(f[sl]), _i32(f1)), f"box {b}"
        assert np.array_equal(_i64(x64[sl]), _i64(x641)) and np.array_equal(_i64(res.rows[b]), _i64(r1.rows[0])), f"box {b}"


def test_energy_start_is_the_classical_energy_of_the_same_fp32_start_bit_for_bit():
    """k_min_pairs and k_classical_pairs are one walk (gamd_lj_walk): on the same fp32 start — widened by the one, by k_min_init
    for the other — the same slices, atom-to-thread assignment, block count and tree, and 0.5 * the in-order block sum give the
    same double.  258 atoms (two row tiles, the second partial) alone and in a two-box handle with different edges."""
    (xa, ba), (xb, bb) = _golden_start(), _lattice_start()
    boxes = np.array([[ba] * 3, [bb] * 3], dtype=np.float32)
    for x0, box, nb in ((xa, None, 1), (np.concatenate([xa, xb]), boxes, 2)):
        eng = _seeded_engine(258, float(ba), n_boxes=nb)
        energy = eng.classical_forces(x0, box=box)[1]
        res = _minimize(eng, x0, box=box, tolerance=TOL, max_iter=1)[0]
        eng.close()
        print(f"{nb} box(es): energy_start {res.energy_start.tolist()}, classical_forces {np.asarray(energy).tolist()}")
        assert np.isfinite(energy).all() and len(energy) == nb
        assert np.array_equal(_i64(res.energy_start), _i64(energy))


CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_minimize as t
from gamd_amd import _lib
print("RESULT", json.dumps(dict(version=_lib.load().gamd_version().decode(), bits=t._lj258_bits())))
"""


def _lj258_bits():
    x0, box = _golden_start()
    eng = _seeded_engine(258, box)
    out = _minimize(eng, x0, tolerance=TOL)
    eng.close()
    return [out[0].status, *_bits(*out)]


def test_checked_build_gives_the_same_bits():
    """no k_min_* kernel uses a value it read from memory as an address: the checked library has nothing to range-check in
    them, runs the same code and must give the same bits (a failed check of any other kernel would come back as -35)"""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    env = {k: v for k, v in os.environ.items() if k not in ("GAMD_LIB", "GAMD_CHK_INJECT")}
    env["GAMD_LIB"] = CHK
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert p.returncode == 0 and "RESULT" in p.stdout, (p.stdout[-800:], p.stderr[-1500:])
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got["version"].endswith("checked")
    assert got["bits"] == _lj258_bits() and got["bits"][0] == 0


# ---- 5: shapes and potential forms -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,scale,kw", [
    (300, (1.0, 1.0, 1.0), dict()),                                       # one full tile plus 44, 32 slices of 10
    (64, (1.0, 1.0, 1.0), dict(r_cut=8.5, r_switch=5.1)),                 # below one tile; box 17.1 A
    (1500, (1.0, 0.9, 1.15), dict()),                                     # six tiles, three different edges, six block rows
    (300, (1.0, 1.0, 1.0), dict(shift=False)),
    (300, (1.0, 1.0, 1.0), dict(r_switch=0.0)),
])
def test_shapes_and_potential_forms(n, scale, kw):
    L = wl.lj_box(n, seed=4)[1]
    box = (np.float32(L) * np.asarray(scale, dtype=np.float32)).astype(np.float32)
    lj = cr.LJ(**kw)
    assert 2 * lj.r_cut <= box.min()
    x0 = (np.random.default_rng(4).random((n, 3)) * box.astype(np.float64)).astype(np.float32)
    eng = _seeded_engine(n, box, cutoff=5.0 if n == 64 else 7.5)
    eng.classical_configure(0, **lj.kwargs())
    res, x, f, x64 = _minimize(eng, x0, box=box, tolerance=TOL)
    fcl = _assert_f_contract(eng, x, f, box=box)
    eng.close()
    print(f"n = {n}, {kw}: {res!r}; U0 {res.energy_start[0]:.3e} rms0 {res.rms_start[0]:.3e}; rms on the fp32 x {_rms(fcl):.6f}")
    assert res.status == 0 and res.state == ["converged"] and 0 < res.iterations[0] <= 400
    assert res.energy[0] < res.energy_start[0] and _rms(fcl) <= TOL + 1e-3
    assert np.array_equal(x, mr.wrap_fp32(x64, box)) and (x >= 0).all() and (x < box).all()


# ---- 6: stops --------------------------------------------------------------------------------------------------------
def test_max_iter_stops_with_its_own_state():
    x0, box = _golden_start()
    eng = _seeded_engine(258, box)
    res, x, f, x64 = _minimize(eng, x0, tolerance=TOL, max_iter=5)
    _assert_f_contract(eng, x, f)
    eng.close()
    assert res.status == 1 and res.state == ["max_iter"] and res.iterations[0] == 5 and not res.converged
    assert res.rms[0] > TOL and res.energy[0] < res.energy_start[0] and not np.array_equal(x, x0)


def test_two_atoms_at_one_point_fail_and_leave_x_and_f_alone():
    x0, box = _golden_start()
    x0 = x0 - np.float32(3.0)                                    # not wrapped: "as given" means as given
    x0[7] = x0[3]
    eng = _seeded_engine(258, box)
    x = torch.from_numpy(x0).cuda()
    f = torch.full_like(x, 7.0)
    res = eng.minimize(x, f, tolerance=TOL, return_x64=True)
    assert res.status == 2 and res.state == ["failed"] and res.iterations[0] == 0
    assert np.array_equal(_i32(x.cpu().numpy()), _i32(x0))
    assert np.array_equal(f.cpu().numpy(), np.full_like(x0, 7.0))
    assert np.array_equal(res.x64.cpu().numpy(), x0.astype(np.float64))
    # the handle goes on: the same call on a sound start converges
    good, _ = _golden_start()
    assert _minimize(eng, good, tolerance=TOL)[0].status == 0
    eng.close()


def test_the_network_path_is_untouched_by_a_minimisation():
    case = _Case("lj")
    ref_eng, xr, vr, fr = case.make()
    out0 = ref_eng.forward(xr).clone()
    case.run(ref_eng, xr, vr, fr, 6)
    ref = _state(xr, vr, fr)
    ref_eng.close()

    eng, x, v, f = case.make()
    other = x.clone()
    res = eng.minimize(other, tolerance=TOL)
    assert res.status == 0 and not torch.equal(other, x)
    assert torch.equal(eng.forward(x), out0) and eng.force_source == "network"
    case.run(eng, x, v, f, 6)
    for name, a, b in zip("xvf", ref, _state(x, v, f)):
        assert np.array_equal(_i32(a), _i32(b)), name
    eng.close()


def test_refusals_name_their_reason():
    import ctypes as C
    from gamd_amd._lib import GamdError, GamdMinimizeParams

    def raw(eng, x, f, tolerance=TOL):
        p = GamdMinimizeParams(tolerance=tolerance)
        return eng._lib.gamd_minimize(eng._h, C.c_void_p(x.data_ptr()), eng._box_arg(None), 0.0, C.c_void_p(f.data_ptr()), None,
                                      C.byref(p), None, eng._stream()), eng._lib.gamd_last_error()

    water = _Case("water")
    eng, x, v, f = water.make()
    st, msg = raw(eng, x, f)
    assert st == -22 and b"GAMD_KIND_WATER" in msg
    eng.close()
    case = _Case("lj")
    eng, x, v, f = case.make()
    before = _state(x, v, f)
    st, msg = raw(eng, x, f)                                                 # no parameters yet
    assert st == -22 and b"gamd_classical_configure" in msg
    eng.classical_configure(0)
    case.run(eng, x, v, f, 2, sync=False)
    with pytest.raises(GamdError, match="-22.*enqueued"):                   # a run is pending
        eng.minimize(x, f, tolerance=TOL)
    assert eng.sync_status() == 0
    before = _state(x, v, f)
    with pytest.raises(GamdError, match="-22.*r_cut"):                      # a box edge below 2 r_cut
        eng.minimize(x, f, tolerance=TOL, box=0.74 * case.box)
    for bad, word in ((dict(tolerance=0.0), "tolerance"), (dict(tolerance=float("nan")), "tolerance"), (dict(tolerance=float("inf")), "tolerance"),
                      (dict(max_iter=-1), "max_iter"), (dict(check_every=-1), "check_every"), (dict(n_min=-1), "n_min"),
                      (dict(f_dec=1.5), "f_dec"), (dict(f_alpha=1.0), "f_alpha"), (dict(alpha_start=-0.1), "alpha_start"),
                      (dict(f_inc=1.0), "f_inc"), (dict(dt_start=0.05), "dt_max"), (dict(dt_start=-1.0), "dt_start"),
                      (dict(max_step=-0.1), "max_step")):
        with pytest.raises(GamdError, match="-22.*" + word):
            eng.minimize(x, f, **{"tolerance": TOL, **bad})
    with pytest.raises(TypeError):
        eng.minimize(x, f, tolerance=TOL, f_grow=1.1)
    for a, b in zip(before, _state(x, v, f)):                               # a refused call changed nothing
        assert np.array_equal(_i32(a), _i32(b))
    eng.close()
