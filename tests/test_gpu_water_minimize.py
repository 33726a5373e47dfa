"""The water energy minimiser on the device (gamd_water_minimize, gamd_amd/csrc/water_minimize.hip): rigid-molecule FIRE in
double under the 3-site water potential, leaving x and f as a water-source md_run / md_run_nhc expects them.

What is asserted, and why the bars are what they are
* The f contract is bit equality: the returned f viewed as int32 equals water_classical_forces(x, species)[0].float() viewed as
  int32, for every size, start, unit and potential form.  No tolerance is involved.
* Iteration counts at tolerance 10 equal the float64 replay's (tests/water_minimize_ref.py): 100 at 86 molecules / r_cut 6.5
  (replayed in tests/test_water_minimize_host.py: rms 9.743 at the stop, 11.050 before it) and 86 at 258 molecules / r_cut 9.5
  (rms 8.524 at the stop, 11.019 before it; a minute of replay on the CPU, so pinned here).  Neither rms is within 1e-6
  relative of the tolerance, so the count does not hang on rounding.
* Convergence is judged on the RETURNED fp32 positions: the rms of the projected classical force on x is at most tolerance +
  5.6e-4 kJ/mol/nm.  The margin is ten times the largest |rms on fp32 x - rms on x64| the replay shows on these starts on the
  CPU: 5.57e-5 at 86 molecules, 8.2e-6 at 258.
* Molecules of x64 are rigid to 1e-12 relative; x is the replay's wrap of x64 bit for bit (every oxygen in [0, L), hydrogens
  moved by the same lattice vector), so its bonds are off by at most the fp32 rounding of three coordinates per atom,
  2 sqrt(3) ulp(32) / 2 < 7e-6 A.
* Parity with the replay after K = 1 and K = 32 iterations at 86 molecules: the bars are 100 times the replay's own spread
  under three molecule permutations (another summation order) and under a relative perturbation of every force component by
  2^-50 xi, xi uniform in [-1, 1] (device erfc / exp / sincospi are not correctly rounded; numpy's and scipy's are others),
  with floors of 1e-13 A on x64 and 1e-13 relative on U and rms.  The factor is the LJ minimiser's test's: the device's slice,
  thread and block order differs from numpy's by more than a permutation does.  The five replays (one run to K = 32 each, the
  state behind iteration 1 kept) take about 25 s on the CPU, once per session.
* Same bits from two calls, a fresh handle, check_every = 1, 64 and 1000, the checked library, and for each box of a two-box
  handle whose boxes stop at different iterations (100 and 87 in the replay) against the same box alone.  x, x64 and the rows
  are compared across handles; f is held to its contract on each handle, because the k-vector list of a handle is built for
  the longest edge of all its boxes and the force source's k slices go by the list's length.
* The bohr case scales positions, box, r_cut, sigma_O, r_oh, r_hh and max_step by u = 1.88972613 and dt_start, dt_max by
  sqrt(u): F is in kJ/mol/nm in every unit and dr = dt v with v built from dt F, so the step is quadratic in dt and sqrt(u)
  makes the bohr run the Angstrom run scaled (the replay: 100 iterations in both; scaled by u itself it takes 108).  The count
  is therefore required to equal the Angstrom case's within 1.

* The start with two atoms of different molecules at one point is a molecule copied onto another: the call first puts every
  molecule on the exact geometry, which moves an fp32 atom by 1e-7 A, so a single atom moved onto another would no longer
  coincide with it (and would be put back on its own molecule's geometry); two molecules with the same bits come out of
  SETTLE with the same bits.  A frozen handle's refusal is not exercised: it would take a provoked neighbour-buffer overflow.

Starts are wl.water_box(n_mol, seed, jitter=0, wrap=False) rounded to fp32; ewald_tol is test_gpu_water_classical.py's DELTA.
Nothing here claims parity with OpenMM, whose minimiser is L-BFGS with restraints."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import water_classical_ref as wr
import water_minimize_ref as wm
from gamd_amd import workloads as wl
from test_gpu_classical_drive import _i32, _i64
from test_gpu_report import _state
from test_gpu_water_classical import _Water, _engine, DELTA
from test_gpu_water_drive import _assert_frames_carry_the_classical_force, _rattled, _scale_centres

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHK = os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")
TOL = 10.0
MARGIN = 5.6e-4
ITERS = {86: 100, 258: 86}                                      # the float64 replay's counts at tolerance 10
EDGES = (1.0, 1.05, 1.02)


def _start(n_mol, seed=5, edges=None):
    """(x0 fp32, box fp32 scalar or [3], species)"""
    pos, box, species, _ = wl.water_box(n_mol, seed=seed, jitter=0.0, wrap=False)
    if edges is None:
        return pos.astype(np.float32), np.float32(box), species
    return _scale_centres(pos, edges).astype(np.float32), (np.float32(box) * np.asarray(edges, dtype=np.float32)).astype(np.float32), species


def _water_engine(n_mol, box, r_cut, n_boxes=1, length_per_nm=0.0, **kw):
    eng, _ = _engine(n_mol, box, n_boxes=n_boxes)
    eng.water_classical_configure(0, ewald_tol=DELTA, r_cut=r_cut, length_per_nm=length_per_nm, **kw)
    return eng


def _minimize(eng, x0, species, box=None, **kw):
    """one call on a copy of x0: (result, x, f, x64) with the arrays on the host"""
    x = torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float32)).cuda()
    res = eng.water_minimize(x, species, box=box, return_x64=True, **kw)
    return res, x.cpu().numpy(), res.f.cpu().numpy(), res.x64.cpu().numpy()


def _assert_f_contract(eng, x, f, species, box=None, length_per_nm=0.0):
    fcl = eng.water_classical_forces(x, species, box=box, length_per_nm=length_per_nm)[0]
    assert torch.isfinite(fcl).all() and float(fcl.abs().max()) > 0.0
    assert np.array_equal(_i32(f), _i32(fcl.float().cpu().numpy()))
    return fcl.cpu().numpy()


def _projected_rms(x, fcl):
    F = wm.project(np.asarray(x, dtype=np.float64), fcl)
    return float(np.sqrt((F * F).sum() / F.size))


def _assert_rigid_whole_and_wrapped(x, x64, box, r_oh=wl.TIP3P_R_OH, r_hh=wl.TIP3P_R_HH, unit=1.0):
    bl = wm.bond_lengths(x64)
    assert np.abs(bl[:, :2] / r_oh - 1).max() <= 1e-12 and np.abs(bl[:, 2] / r_hh - 1).max() <= 1e-12
    assert np.array_equal(_i32(x), _i32(wm.wrap_fp32(x64, box)))
    o = x.reshape(-1, 3, 3)[:, 0]
    assert (o >= 0).all() and (o < np.asarray(box, dtype=np.float32)).all()
    assert np.abs(wm.bond_lengths(x) - np.array([r_oh, r_oh, r_hh])).max() <= 7e-6 * unit     # whole: fp32 rounding and no more


def _bits(res, x, f, x64):
    return _i32(x).tolist(), _i32(f).tolist(), _i64(x64).tolist(), _i64(res.rows).tolist()


# ---- 1: convergence and contracts ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def minimized774():
    x0, box, species = _start(258)
    eng = _water_engine(258, box, 9.5)
    res, x, f, x64 = _minimize(eng, x0, species, tolerance=TOL)
    fcl = _assert_f_contract(eng, x, f, species)
    eng.close()
    return dict(x0=x0, box=box, species=species, res=res, x=x, f=f, x64=x64, fcl=fcl)


def _check_converged(n_mol, m):
    res = m["res"]
    rms32 = _projected_rms(m["x"], m["fcl"])
    print(f"{n_mol} molecules: {res!r}; U {res.energy_start[0]:.6f} -> {res.energy[0]:.6f}, rms {res.rms_start[0]:.6f} -> {res.rms[0]:.6f}, "
          f"fmax {res.fmax[0]:.4f}, dt {res.dt[0]:.6f}; projected rms on the fp32 x {rms32:.6f} (|difference| {abs(rms32 - res.rms[0]):.3e})")
    assert res.status == 0 and res.converged and res.state == ["converged"]
    assert res.iterations[0] == ITERS[n_mol]
    assert res.energy[0] < res.energy_start[0] and res.rms[0] <= TOL < res.rms_start[0]
    _assert_rigid_whole_and_wrapped(m["x"], m["x64"], m["box"])
    assert rms32 <= TOL + MARGIN


def test_258_molecules_converge_to_the_replays_count_and_meet_every_contract(minimized774):
    _check_converged(258, minimized774)


def test_86_molecules_converge_to_the_replays_count_and_meet_every_contract():
    x0, box, species = _start(86)                              # one 256-atom tile plus 2: the last molecule split O | H,H
    eng = _water_engine(86, box, 6.5)
    res, x, f, x64 = _minimize(eng, x0, species, tolerance=TOL)
    fcl = _assert_f_contract(eng, x, f, species)
    eng.close()
    _check_converged(86, dict(res=res, x=x, f=f, x64=x64, fcl=fcl, box=box))


# ---- 2: a run from the minimised start -------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", ["nhc", "baoab"])
def test_a_water_source_run_starts_from_the_minimised_box(minimized774, integrator):
    case = _Water(integrator)
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
@pytest.fixture(scope="module")
def replay32():
    """the replay to K = 32 from the 86-molecule start with the state behind iteration 1 kept: as it is, under three molecule
    permutations, and with every force component perturbed by 2^-50 relative"""
    x0, box, species = _start(86)
    w = wr.Water(r_cut=6.5, ewald_tol=DELTA)
    runs = []
    for kind, seed in (("base", None), ("perm", 1), ("perm", 2), ("perm", 3), ("perturb", 4)):
        p = np.random.default_rng(seed).permutation(86) if kind == "perm" else np.arange(86)
        a = (3 * p[:, None] + np.arange(3)[None, :]).reshape(-1)
        snaps = {1: None}
        r = wm.minimize(x0[a], box, species, w, 1e-300, max_iter=32, snapshots=snaps,
                        perturb=np.random.default_rng(seed) if kind == "perturb" else None)
        assert r["state"] == wm.MAX_ITER and r["iterations"] == 32
        out = {}
        for K, s in ((1, snaps[1]), (32, r)):
            xs = np.empty_like(s["x"])
            xs[a] = s["x"]
            out[K] = dict(x=xs, u=s["u"], rms=s["rms"])
        runs.append(out)
    return runs


@pytest.mark.parametrize("K", [1, 32])
def test_positions_energy_and_rms_agree_with_the_float64_replay(replay32, K):
    x0, box, species = _start(86)
    base = replay32[0][K]
    spread_x = max(np.abs(r[K]["x"] - base["x"]).max() for r in replay32[1:])
    spread_u = max(abs(r[K]["u"] - base["u"]) for r in replay32[1:])
    spread_r = max(abs(r[K]["rms"] - base["rms"]) for r in replay32[1:])
    bar_x = max(100.0 * spread_x, 1e-13)
    bar_u, bar_r = max(100.0 * spread_u, 1e-13 * abs(base["u"])), max(100.0 * spread_r, 1e-13 * base["rms"])
    eng = _water_engine(86, box, 6.5)
    res, x, f, x64 = _minimize(eng, x0, species, tolerance=1e-300, max_iter=K)
    _assert_f_contract(eng, x, f, species)
    eng.close()
    dx, du, dr = np.abs(x64 - base["x"]).max(), abs(res.energy[0] - base["u"]), abs(res.rms[0] - base["rms"])
    print(f"K = {K}: device against the replay: |dx| max {dx:.3e} A (replay's spread {spread_x:.3e}, bar {bar_x:.3e}); "
          f"|dU| {du:.3e} (spread {spread_u:.3e}, bar {bar_u:.3e}) at U = {base['u']:.9e}; "
          f"|drms| {dr:.3e} (spread {spread_r:.3e}, bar {bar_r:.3e}) at rms = {base['rms']:.9e}")
    assert res.status == 1 and res.state == ["max_iter"] and res.iterations[0] == K
    assert dx <= bar_x
    assert du <= bar_u
    assert dr <= bar_r


# ---- 4: reproducibility and gating -----------------------------------------------------------------------------------
def test_two_calls_a_fresh_handle_and_every_check_every_give_the_same_bits():
    x0, box, species = _start(86)
    eng = _water_engine(86, box, 6.5)
    first = _minimize(eng, x0, species, tolerance=TOL)          # 100 iterations: two chunks of 64
    assert first[0].status == 0 and first[0].iterations[0] > 64
    ref = _bits(*first)
    assert _bits(*_minimize(eng, x0, species, tolerance=TOL)) == ref, "second call"
    eng.close()
    eng = _water_engine(86, box, 6.5)
    for every in (1, 64, 1000):
        assert _bits(*_minimize(eng, x0, species, tolerance=TOL, check_every=every)) == ref, f"check_every = {every}"
    eng.close()


def test_each_box_of_a_two_box_handle_gets_the_bits_it_gets_alone():
    (xa, ba, species), (xb, bb, _) = _start(86), _start(86, seed=6, edges=EDGES)
    boxes = np.stack([np.full(3, ba, dtype=np.float32), bb]).astype(np.float32)
    eng = _water_engine(86, float(ba), 6.5, n_boxes=2)
    res, x, f, x64 = _minimize(eng, np.concatenate([xa, xb]), species, box=boxes, tolerance=TOL)
    _assert_f_contract(eng, x, f, species, box=boxes)
    eng.close()
    print(f"two boxes: {res!r}")
    assert res.status == 0 and res.iterations.tolist() == [100, 87]       # one box stops first (the replay's counts)
    for b, (xs, box) in enumerate(((xa, ba), (xb, bb))):
        one = _water_engine(86, box, 6.5)
        r1, x1, f1, x641 = _minimize(one, xs, species, box=box, tolerance=TOL)
        _assert_f_contract(one, x1, f1, species, box=box)
        one.close()
        sl = slice(258 * b, 258 * (b + 1))
        assert np.array_equal(_i64(x64[sl]), _i64(x641)) and np.array_equal(_i64(res.rows[b]), _i64(r1.rows[0])), f"box {b}"
        assert np.array_equal(_i32(x[sl]), _i32(x1)), f"box {b}"


CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_water_minimize as t
from gamd_amd import _lib
print("RESULT", json.dumps(dict(version=_lib.load().gamd_version().decode(), bits=t._w86_bits())))
"""


def _w86_bits():
    x0, box, species = _start(86)
    eng = _water_engine(86, box, 6.5)
    out = _minimize(eng, x0, species, tolerance=TOL, max_iter=40)
    eng.close()
    return [out[0].status, *_bits(*out)]


def test_checked_build_gives_the_same_bits():
    """no k_wmin_* kernel uses a value it read from memory as an address: the checked library has nothing to range-check in
    them, runs the same code and must give the same bits (a failed check of any other kernel would come back as -35)"""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    env = {k: v for k, v in os.environ.items() if k not in ("GAMD_LIB", "GAMD_CHK_INJECT")}
    env["GAMD_LIB"] = CHK
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert p.returncode == 0 and "RESULT" in p.stdout, (p.stdout[-800:], p.stderr[-1500:])
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got["version"].endswith("checked")
    assert got["bits"] == _w86_bits() and got["bits"][0] == 1


# ---- 5: forms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edges,kw", [(EDGES, dict()), (None, dict(r_switch=8.0, shift=True))])
def test_three_edges_and_switch_with_shift_on_774_atoms(edges, kw):
    x0, box, species = _start(258, edges=edges)
    assert 2 * 9.5 <= np.min(box) and (edges is None or len(set(np.asarray(box).tolist())) == 3)
    eng = _water_engine(258, box, 9.5, **kw)
    res, x, f, x64 = _minimize(eng, x0, species, box=box, tolerance=TOL)
    fcl = _assert_f_contract(eng, x, f, species, box=box)
    eng.close()
    rms32 = _projected_rms(x, fcl)
    print(f"774 atoms, edges {edges}, {kw}: {res!r}; U {res.energy_start[0]:.6f} -> {res.energy[0]:.6f}; projected rms on the fp32 x {rms32:.6f}")
    assert res.status == 0 and res.state == ["converged"] and 0 < res.iterations[0] <= 400
    assert res.energy[0] < res.energy_start[0] and rms32 <= TOL + MARGIN
    _assert_rigid_whole_and_wrapped(x, x64, box)


def test_bohr_units_take_the_angstrom_cases_iterations():
    pos, box, species, _ = wl.water_box(86, seed=5, jitter=0.0, wrap=False)
    ln = wl.BOHR_PER_NM
    u = float(np.float32(ln)) / 10.0
    x0, bx = (pos * u).astype(np.float32), np.float32(box * u)
    eng = _water_engine(86, bx, 6.5 * u, length_per_nm=ln)      # sigma_O's default goes with length_per_nm
    su = float(np.sqrt(u))
    res, x, f, x64 = _minimize(eng, x0, species, tolerance=TOL, length_per_nm=ln, r_oh=wl.TIP3P_R_OH * u, r_hh=wl.TIP3P_R_HH * u,
                               dt_start=0.002 * su, dt_max=0.02 * su, max_step=0.1 * u)
    fcl = _assert_f_contract(eng, x, f, species, length_per_nm=ln)
    eng.close()
    rms32 = _projected_rms(x, fcl)
    print(f"bohr: {res!r}; U {res.energy_start[0]:.6f} -> {res.energy[0]:.6f}; projected rms on the fp32 x {rms32:.6f}")
    assert res.status == 0 and res.state == ["converged"] and abs(int(res.iterations[0]) - ITERS[86]) <= 1
    assert res.energy[0] < res.energy_start[0] and rms32 <= TOL + MARGIN
    _assert_rigid_whole_and_wrapped(x, x64, bx, wl.TIP3P_R_OH * u, wl.TIP3P_R_HH * u, unit=u)


# ---- 6: stops --------------------------------------------------------------------------------------------------------
def test_max_iter_stops_with_its_own_state():
    x0, box, species = _start(86)
    eng = _water_engine(86, box, 6.5)
    res, x, f, x64 = _minimize(eng, x0, species, tolerance=TOL, max_iter=5)
    _assert_f_contract(eng, x, f, species)
    eng.close()
    assert res.status == 1 and res.state == ["max_iter"] and res.iterations[0] == 5 and not res.converged
    assert res.rms[0] > TOL and res.energy[0] < res.energy_start[0] and not np.array_equal(x, x0)


@pytest.mark.parametrize("what", ["a molecule on another", "a hydrogen on its oxygen"])
def test_a_start_that_is_not_finite_fails_and_leaves_x_f_and_x64_alone(what):
    good, box, species = _start(86)
    x0 = good - np.float32(3.0)                                  # not wrapped: "as given" means as given
    if what == "a molecule on another":
        x0[6:9] = x0[3:6]                                       # atoms of different molecules at one point (the same bits
    else:                                                       # in, the same bits out of the first SETTLE)
        x0[4] = x0[3]                                           # SETTLE cannot place it
    eng = _water_engine(86, box, 6.5)
    x = torch.from_numpy(x0).cuda()
    f = torch.full_like(x, 7.0)
    res = eng.water_minimize(x, species, f, tolerance=TOL, return_x64=True)
    assert res.status == 2 and res.state == ["failed"] and res.iterations[0] == 0
    assert np.array_equal(_i32(x.cpu().numpy()), _i32(x0))
    assert np.array_equal(f.cpu().numpy(), np.full_like(x0, 7.0))
    assert np.array_equal(res.x64.cpu().numpy(), x0.astype(np.float64))
    # the handle goes on: the same call on a sound start converges
    assert _minimize(eng, good, species, tolerance=TOL)[0].status == 0
    eng.close()


# ---- 7: the network path ---------------------------------------------------------------------------------------------
def test_the_network_path_is_untouched_by_a_minimisation():
    case = _Water("baoab")
    ref_eng, xr, vr, fr = case.make()
    out0 = ref_eng.forward(xr, species=case.species).clone()
    case.run(ref_eng, xr, vr, fr, 6)
    ref = _state(xr, vr, fr)
    ref_eng.close()

    eng, x, v, f = case.make()
    other = x.clone()
    res = eng.water_minimize(other, case.species, tolerance=TOL, max_iter=20)
    assert res.status == 1 and not torch.equal(other, x)
    assert torch.equal(eng.forward(x, species=case.species), out0) and eng.force_source == "network"
    case.run(eng, x, v, f, 6)
    for name, a, b in zip("xvf", ref, _state(x, v, f)):
        assert np.array_equal(_i32(a), _i32(b)), name
    eng.close()


# ---- 8: refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    import ctypes as C
    from gamd_amd._lib import GamdError, GamdMinimizeParams
    from gamd_amd.engine import GamdForce
    from gamd_amd.weights import SHIPPED_SCALERS
    from helpers import load_golden
    from test_gpu_report import _Case

    def raw(eng, x, f, flags, entry="gamd_water_minimize"):
        p = GamdMinimizeParams(tolerance=TOL)
        if entry == "gamd_minimize":
            st = eng._lib.gamd_minimize(eng._h, C.c_void_p(x.data_ptr()), eng._box_arg(None), 0.0, C.c_void_p(f.data_ptr()), None,
                                        C.byref(p), None, eng._stream())
        else:
            st = eng._lib.gamd_water_minimize(eng._h, C.c_void_p(x.data_ptr()), C.c_void_p(flags.data_ptr()) if flags is not None else None,
                                              eng._box_arg(None), 0.0, 0.0, 0.0, C.c_void_p(f.data_ptr()), None, C.byref(p), None, eng._stream())
        return st, eng._lib.gamd_last_error()

    # an LJ handle
    eng, x, v, f = _Case("lj").make()
    st, msg = raw(eng, x, f, None)
    assert st == -22 and b"GAMD_KIND_LJ" in msg
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
    st, msg = raw(eng, x, f, flags, entry="gamd_minimize")                    # the LJ minimiser still refuses a water handle
    assert st == -22 and b"GAMD_KIND_WATER" in msg
    st, msg = raw(eng, x, f, flags)                                           # no parameters yet
    assert st == -22 and b"gamd_water_configure" in msg
    eng.water_classical_configure(0, ewald_tol=DELTA)
    case.run(eng, x, v, f, 2, sync=False)
    with pytest.raises(GamdError, match="-22.*enqueued"):                    # a run is pending
        eng.water_minimize(x, case.species, f, tolerance=TOL)
    assert eng.sync_status() == 0
    before = _state(x, v, f)
    with pytest.raises(GamdError, match="-22.*species"):
        eng.water_minimize(x, None, f, tolerance=TOL)
    with pytest.raises(GamdError, match="-22.*r_cut"):                       # a box edge below 2 r_cut
        eng.water_minimize(x, case.species, f, tolerance=TOL, box=0.9 * case.box)
    for bad, word in ((dict(r_oh=1.0, r_hh=2.0), "2 r_oh"), (dict(r_oh=1.0, r_hh=2.5), "2 r_oh"), (dict(r_oh=-1.0), "not positive"),
                      (dict(r_hh=-0.5), "not positive"), (dict(tolerance=0.0), "tolerance"), (dict(tolerance=float("nan")), "tolerance"),
                      (dict(max_iter=-1), "max_iter"), (dict(check_every=-1), "check_every"), (dict(f_dec=1.5), "f_dec"),
                      (dict(dt_start=0.05), "dt_max"), (dict(max_step=-0.1), "max_step")):
        with pytest.raises(GamdError, match="-22.*" + word):
            eng.water_minimize(x, case.species, f, **{"tolerance": TOL, **bad})
    with pytest.raises(TypeError):
        eng.water_minimize(x, case.species, f, tolerance=TOL, f_grow=1.1)
    for a, b in zip(before, _state(x, v, f)):                               # a refused call changed nothing
        assert np.array_equal(_i32(a), _i32(b))
    eng.close()
