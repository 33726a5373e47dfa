"""The water classical force source on the device (gamd_md_force_source with GAMD_FORCE_WATER_CLASSICAL,
gamd_amd/csrc/water_drive.hip): enqueued rigid-water md_run / md_run_nhc calls whose forces come from the 3-site water potential
of the water classical observer (O-O Lennard-Jones plus a plain Ewald sum, in double) instead of the network.

What is asserted, and why the bars are what they are
* The force contract is bit equality: on every recorded frame, and in the final buffer, f viewed as int32 equals
  water_classical_forces(x, species)[0].float() viewed as int32 (the observer's kernels on the same fp32 positions, rounded to
  nearest).  No tolerance is involved.
* The integrator chain is judged against the oracle's float64 rigid integrators (SHAKE / RATTLE iterated to convergence) driven
  by tests/water_classical_ref.py, with the bars tests/test_gpu_round4.py sets for the same chain under network forces:
  rel_err(x) < 1e-5, rel_err(v) < 1e-4.  The device keeps molecules whole but wraps them by their oxygen, so a whole-molecule
  lattice vector is taken off the device's x first (asserted to be one vector per molecule).  Before the device runs, the same
  three steps with x, v, f rounded to fp32 after every half-step are checked against the float64 replay with the same bars on
  the CPU: the bars are reachable by fp32 state at all.  Every replayed frame is asserted to hold no pair within 1e-12 r_cut of
  the cutoff.
* The observer on a driven run: f = RN_fp32(f_cl) per component, so |D_ic| <= 2^-24 |f_cl,ic| and
    sum_abs      = sum_i sum_c |D_ic|  <= 2^-24 sqrt(3) sum_i |f_cl,i|  (Cauchy-Schwarz over the three components),
    sum_sq       = sum_i |D_i|^2       <= 2^-48 sum_i |f_cl,i|^2,
    sum_norm_cl  = sum_i |f_cl,i|      (the host's sum of the device's f_cl, to 1e-12),
    |sum_norm - sum_norm_cl|           <= sum_i |D_i| <= 2^-24 sum_i |f_cl,i|,
    N - sum_cos  : the angle between f_i and f_cl,i is at most |D_i| / |f_cl,i| <= 2^-24, so 1 - cos <= 2^-49 per atom, next to
                   a few 2^-53 of double rounding in the quotient: |N - sum_cos| <= N 1e-13.
  (1 + 1e-12) covers the rounding of the device's sums (774 double terms each, test_gpu_classical.py's argument).  No component
  comes near the fp32 range (asserted).

Shapes: 774 atoms (258 molecules: three 256-atom row tiles plus a tail of 6, molecules straddling tile edges; r_cut 9.5,
ewald_tol 1e-8, 3 940 k-vectors), one 774-atom box with three different edges, and two boxes of 258 atoms (the last molecule of
a tile split O | H,H) with different positions and edges.  Every start is whole rigid molecules with rattled 300 K velocities.
Nothing here claims parity with OpenMM: the default parameters are unverified."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gamd_oracle as orc
import water_classical_ref as wr
from gamd_amd import workloads as wl
from gamd_amd.weights import SHIPPED_SCALERS
from helpers import load_golden, rel_err
from test_gpu_classical_drive import _i32, _i64
from test_gpu_report import _Case, _state, _f32
from test_gpu_water_classical import _Water, DELTA

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHK = os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")
SKIN = 0.7                                                 # cutoff / 6 of the 4.2 A network cutoff
MODES = [("baoab", 0.0), ("baoab", SKIN), ("nhc", 0.0), ("nhc", SKIN)]


def _scale_centres(pos, scale):
    """every molecule moved with its oxygen to O * scale: the geometry of a molecule stays exactly rigid"""
    o = np.repeat(pos[0::3], 3, axis=0)
    return o * np.asarray(scale)[None, :] + (pos - o)


def _rattled(pos, species, seed):
    pairs, _ = orc.water_constraints(pos.shape[0], wl.TIP3P_R_OH, wl.TIP3P_R_HH)
    mm = np.where(species == 1, wl.MASS_O, wl.MASS_H).astype(np.float64).reshape(-1, 1)
    v0 = np.random.default_rng(seed).normal(0, 1.0, pos.shape) * 10.0 * np.sqrt(wl.KB * 300.0 / mm)
    return orc.rattle_velocities(pos, v0, (1.0 / mm).reshape(-1), pairs)


class _WaterIn(_Water):
    """_Water in another length unit (bohr: positions, box, velocities, network cutoff, skin and the rigid geometry scaled),
    or with its molecules moved to a box with three different edges"""

    def __init__(self, integrator="baoab", skin=0.0, length_per_nm=0.0, edges=None, **kw):
        super().__init__(integrator, skin=skin, **kw)
        if edges is not None:
            self.pos = _scale_centres(self.pos, edges)
            self.box = (np.float32(self.box) * np.asarray(edges, dtype=np.float32)).astype(np.float32)
        self.unit = 1.0
        if length_per_nm:
            u = self.unit = float(_f32(length_per_nm)) / 10.0
            self.len = length_per_nm
            self.pos, self.v0, self.box = self.pos * u, self.v0 * u, float(np.float32(self.box * u))
            self.rc, self.skin = self.rc * u, self.skin * u
            self.md = dict(self.md, length_per_nm=length_per_nm, r_oh=wl.TIP3P_R_OH * u, r_hh=wl.TIP3P_R_HH * u)


def _water_start(eng, x, species, box=None, length_per_nm=0.0, **kw):
    """parameters (interval 0), the water source, and the forces a water-source run must find in f"""
    eng.water_classical_configure(0, **{"ewald_tol": DELTA, "length_per_nm": length_per_nm, **kw})
    eng.md_force_source("water_classical")
    assert eng.force_source == "water_classical"
    return eng.water_classical_forces(x, species, box=box, length_per_nm=length_per_nm)[0].float().contiguous()


def _make(case, **kw):
    eng, x, v, f = case.make()
    f = _water_start(eng, x, case.species, length_per_nm=case.len, **kw)
    return eng, x, v, f


def _assert_frames_carry_the_classical_force(eng, tr, x, f, species, n_frames, box=None, length_per_nm=0.0):
    """every recorded frame and the final state: f == fp32(f_cl(x)) bit for bit"""
    assert tr.dropped == 0 and np.array_equal(tr.steps, np.arange(1, n_frames + 1))
    frames = [(tr.x[t].reshape(-1, 3), tr.f[t].reshape(-1, 3)) for t in range(n_frames)] + [(x.cpu().numpy(), f.cpu().numpy())]
    assert np.array_equal(frames[-1][0], frames[-2][0]) and np.array_equal(_i32(frames[-1][1]), _i32(frames[-2][1]))
    for t, (xs, fs) in enumerate(frames[:-1]):
        fcl = eng.water_classical_forces(xs, species, box=box, length_per_nm=length_per_nm)[0]
        assert torch.isfinite(fcl).all() and float(fcl.abs().max()) > 0.0
        assert np.array_equal(_i32(fs), _i32(fcl.float().cpu().numpy())), f"frame {t}"
    assert not np.array_equal(frames[0][0], frames[-1][0])                 # it moved


# ---- 1: forces on every frame ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator,skin", MODES)
def test_water774_every_frame_carries_the_classical_force_of_its_positions(integrator, skin):
    case = _Water(integrator, skin=skin)                                 # BAOAB at 300 K with gamma = 25: noise on
    eng, x, v, f = _make(case)
    steps = 12
    eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
    case.run(eng, x, v, f, steps)
    assert eng.last_status == 0
    _assert_frames_carry_the_classical_force(eng, eng.traj_read(), x, f, case.species, steps)
    eng.close()


@pytest.mark.parametrize("integrator,skin,length_per_nm,kw", [               # the observer's own test parameters
    ("nhc", SKIN, 0.0, dict(r_switch=8.0, shift=True)),
    ("baoab", 0.0, wl.BOHR_PER_NM, dict()),
    ("nhc", SKIN, wl.BOHR_PER_NM, dict(r_switch=8.0, shift=True)),
])
def test_switch_shift_and_bohr_units(integrator, skin, length_per_nm, kw):
    case = _WaterIn(integrator, skin=skin, length_per_nm=length_per_nm)
    w = wr.Water(sigma_o=3.15075 * case.unit, r_cut=9.5 * case.unit, r_switch=kw.get("r_switch", 0.0) * case.unit,
                 shift=kw.get("shift", False), ewald_tol=DELTA)
    assert 2 * w.r_cut <= np.float32(case.box)
    eng, x, v, f = _make(case, **{k: (val * case.unit if k == "r_switch" else val) for k, val in kw.items()})
    ref = wr.evaluate(x.cpu().numpy(), case.box, case.species, w, length_per_nm)      # the parameters are the ones meant
    assert ref["near"] == 0 and (not kw or ref["abs_lj"] > 0)
    assert (np.abs(f.cpu().numpy() - ref["forces"]) <= 1e-12 * ref["abs_f"][:, None] + 2.0 ** -24 * np.abs(ref["forces"])).all()
    steps = 6
    eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
    case.run(eng, x, v, f, steps)
    assert eng.last_status == 0
    _assert_frames_carry_the_classical_force(eng, eng.traj_read(), x, f, case.species, steps, length_per_nm=length_per_nm)
    eng.close()


@pytest.mark.parametrize("integrator,skin", [("baoab", SKIN), ("nhc", 0.0)])
def test_three_different_edges(integrator, skin):
    case = _WaterIn(integrator, skin=skin, edges=(1.0, 1.05, 1.02))
    assert 2 * 9.5 <= case.box.min() and len(set(case.box.tolist())) == 3
    eng, x, v, f = _make(case)
    steps = 6
    eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
    case.run(eng, x, v, f, steps)
    assert eng.last_status == 0
    _assert_frames_carry_the_classical_force(eng, eng.traj_read(), x, f, case.species, steps)
    eng.close()


# ---- 2: the chain against the oracle's rigid integrators -------------------------------------------------------------
DT, GAMMA, FREQ, CHAIN, T_NHC = 0.0005, 25.0, 25.0, 10, 300.0


@functools.lru_cache(maxsize=None)
def _chain_reference(integrator, steps=3):
    """(x0, v0, f0 as fp32, the float64 replay (x, v), the replay with x, v, f rounded to fp32 after every half-step (x, v),
    the largest force component met): computed once per integrator on the CPU, never changed"""
    case = _Water(integrator)
    x0, v0 = case.pos.astype(np.float32), case.v0.astype(np.float32)
    w, box, n = wr.Water(ewald_tol=DELTA), np.float32(case.box), case.n
    pairs, lengths = orc.water_constraints(n, wl.TIP3P_R_OH, wl.TIP3P_R_HH)
    mass = np.where(case.species == 1, float(_f32(wl.MASS_O)), float(_f32(wl.MASS_H))).reshape(-1, 1)   # as the device holds them
    kT, ndf, a = wl.KB * T_NHC, 2.0 * n - 3.0, np.exp(-GAMMA * DT)
    fmax = [0.0]

    def force(x):
        ref = wr.evaluate(x, box, case.species, w)
        assert ref["near"] == 0, "ill-posed: a pair sits on the cutoff"
        fmax[0] = max(fmax[0], float(np.abs(ref["forces"]).max()))
        return ref["forces"]

    def replay(r32):
        rd = (lambda t: t.astype(np.float32).astype(np.float64)) if r32 else (lambda t: t)
        xr, vr, fr = x0.astype(np.float64), v0.astype(np.float64), f_start.astype(np.float32).astype(np.float64)   # f as the run finds it
        st = orc.nhc_init(CHAIN, FREQ)
        for _ in range(steps):
            if integrator == "baoab":
                vr = orc.remove_cm_motion(vr, mass)
                xr, vr = orc.baoab_first_half_rigid(xr, vr, fr, 1.0 / mass, DT, a, 0.0, 0.0, pairs, lengths)
            else:
                xr, vr = orc.nhc_first_half_rigid(st, xr, vr, fr, mass, DT, kT, FREQ, ndf, pairs, lengths, remove_com=True)
            xr, vr = rd(xr), rd(vr)
            fr = rd(force(xr))
            if integrator == "baoab":
                vr = orc.baoab_second_half_rigid(xr, vr, fr, 1.0 / mass, DT, pairs)
            else:
                vr = orc.nhc_second_half_rigid(st, xr, vr, fr, mass, DT, kT, FREQ, ndf, pairs)
            vr = rd(vr)
        return xr, vr

    f_start = force(x0)
    return x0, v0, f_start.astype(np.float32), replay(False), replay(True), fmax[0]


@pytest.mark.parametrize("integrator", ["baoab", "nhc"])
def test_three_deterministic_rigid_steps_match_the_oracle_integrators(integrator):
    """Measured on one MI355X, device against the float64 replay: BAOAB rel_err x 1.99e-7, v 1.94e-5; NHC x 1.29e-7, v 7.1e-6.
    The bar on v needs the rigid integrators' velocity correction of the position constraint, v += (xc - x1) / dt, formed
    relative to the molecule's old oxygen (settle_step, gamd_md_dev.h): taken from two fp32 absolute positions it carries
    ulp(x) / dt = 4e-3 A/ps at this 0.5 fs step, and the same run gave v 4.75e-4 (BAOAB) and 1.99e-4 (NHC)."""
    steps = 3
    x0, v0, f0, (xr, vr), (xe, ve), fmax = _chain_reference(integrator)
    # on the CPU first: fp32 state can stay inside the bars at all
    print(f"{integrator}: fp32-rounded replay against the float64 replay: rel_err x {rel_err(xe, xr):.3e}, v {rel_err(ve, vr):.3e}; "
          f"largest force component {fmax:.3e} kJ/mol/nm")
    assert rel_err(xe, xr) < 1e-5 and rel_err(ve, vr) < 1e-4
    case = _Water(integrator)
    eng, x, v, f = case.make()
    assert np.array_equal(x.cpu().numpy(), x0) and np.array_equal(v.cpu().numpy(), v0)
    f = _water_start(eng, x, case.species)
    assert rel_err(f.cpu().numpy(), f0) < 1e-6                               # (the force itself is judged bit for bit above)
    if integrator == "baoab":
        eng.md_run(x, v, f, steps, gamma_per_ps=GAMMA, seed=1, **{**case.md, "temperature_k": 0.0})
    else:
        eng.md_run_nhc(x, v, f, steps, frequency_per_ps=FREQ, chain_length=CHAIN, **case.md)
    assert eng.last_status == 0 and case.md["dt_ps"] == DT and case.md["temperature_k"] == T_NHC
    xd, vd = x.cpu().double().numpy(), v.cpu().double().numpy()
    # the device keeps molecules whole but may translate them by a lattice vector
    shift = np.round((xd - xr) / case.box) * case.box
    assert np.abs(shift.reshape(-1, 3, 3) - shift.reshape(-1, 3, 3)[:, :1]).max() == 0.0
    ex, ev = rel_err(xd - shift, xr), rel_err(vd, vr)
    print(f"{integrator}: device against the float64 replay: rel_err x {ex:.3e}, v {ev:.3e}")
    assert ex < 1e-5
    assert ev < 1e-4
    eng.close()


# ---- 3: the same bits ------------------------------------------------------------------------------------------------
def _driven(case, calls, observers=False):
    """a water-source run of the case in `calls` calls of K steps each (first_step and the chain carried on)"""
    eng, x, v, f = _make(case)
    if observers:
        eng.report_configure(3, rdf_bins=32, **case.report_kw())
        eng.traj_configure(3, max_frames=8, fields=("x", "v", "f", "image"), n_lags=3)
        eng.structure_configure(3, rdf_bins=32, sk_n2max=4)
        eng.water_classical_configure(3, ewald_tol=DELTA)
    chain = None
    for c, k in enumerate(calls):
        chain = case.run(eng, x, v, f, k, first_step=sum(calls[:c]), chain=chain)
        assert eng.last_status == 0
    out = _state(x, v, f)
    rows = eng.water_classical_read().steps if observers else None
    eng.close()
    return out, rows


@pytest.mark.parametrize("integrator,skin", MODES)
def test_chunked_runs_fresh_handles_and_armed_observers_give_the_same_bits(integrator, skin):
    K = 6
    case = _Water(integrator, skin=skin, K=K)
    one, _ = _driven(case, [2 * K])
    two, _ = _driven(case, [K, K])
    again, _ = _driven(case, [2 * K])
    armed, rows = _driven(case, [2 * K], observers=True)
    assert np.array_equal(rows, 3 * np.arange(1, 5))
    for name, other in (("two calls", two), ("second handle", again), ("observers armed", armed)):
        for a, b in zip(one, other):
            assert np.array_equal(_i32(a), _i32(b)), name
    assert not np.array_equal(one[0], case.pos.astype(np.float32))


# ---- 4: the observer on a driven run ---------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator,skin", [("baoab", SKIN), ("nhc", 0.0)])
def test_observer_rows_on_a_driven_run(integrator, skin, tmp_path):
    case = _Water(integrator, skin=skin)
    eng, x, v, f = _make(case)
    steps, n = 8, case.n
    eng.water_classical_configure(2, ewald_tol=DELTA)
    eng.report_configure(2, **case.report_kw())
    eng.traj_configure(1, max_frames=steps, fields=("x", "f"))
    case.run(eng, x, v, f, steps)
    rd, rep, tr = eng.water_classical_read(forces=True), eng.report_read(), eng.traj_read()
    assert rd.dropped == 0 and np.array_equal(rd.steps, [2, 4, 6, 8]) and np.array_equal(rep.steps, rd.steps)
    for q, g in enumerate(rd.steps):
        xs = tr.x[g - 1].reshape(-1, 3)
        fcl, one = eng.water_classical_forces(xs, case.species)
        fcl = fcl.cpu().numpy()
        assert np.abs(fcl).max() < 1e30                                  # nowhere near the fp32 range
        for name in ("u_lj", "u_real", "u_recip", "u_self", "pairs", "sum_q", "energy"):
            assert _i64(getattr(rd, name)[q])[0] == _i64(getattr(one, name)[0])[0], name
        assert rd.pairs[q, 0] > 0 and rd.sum_q[q, 0] == 0.0
        norms = np.sqrt((fcl * fcl).sum(axis=1))
        norm, eps = norms.sum(), 2.0 ** -24
        bound = eps * np.sqrt(3.0) * norm * (1.0 + 1e-12)
        print(f"{integrator} step {g}: sum |D_ic| = {rd.sum_abs[q, 0]:.6e}, bound {bound:.6e}, sum |D_i|^2 = {rd.sum_sq[q, 0]:.6e}, "
              f"bound {eps * eps * (norms * norms).sum():.6e}, N - sum cos = {n - rd.sum_cos[q, 0]:.3e}, "
              f"sum |f_cl| = {rd.sum_norm_cl[q, 0]:.9e}, sum |f| - sum |f_cl| = {rd.sum_norm[q, 0] - rd.sum_norm_cl[q, 0]:.3e}")
        assert abs(rd.sum_norm_cl[q, 0] - norm) <= 1e-12 * norm
        assert 0.0 < rd.sum_abs[q, 0] <= bound
        assert 0.0 < rd.sum_sq[q, 0] <= eps * eps * (norms * norms).sum() * (1.0 + 1e-12)
        assert abs(rd.sum_norm[q, 0] - rd.sum_norm_cl[q, 0]) <= eps * norm * (1.0 + 1e-12)
        assert rd.excluded[q, 0] == 0 and abs(n - rd.sum_cos[q, 0]) <= n * 1e-13
    assert np.array_equal(_i64(rd.forces), _i64(eng.water_classical_forces(tr.x[-1].reshape(-1, 3), case.species)[0].cpu().numpy()))
    path = tmp_path / "log_nvt_tip3p_0.txt"
    rd.write_state_data(rep, path, DT)
    cols = [ln.split("\t") for ln in open(path).read().splitlines()[1:]]
    assert len(cols) == 4 and [float(c[2]) for c in cols] == [float(e) for e in rd.energy[:, 0]]
    eng.close()


# ---- 5: overflow in the middle of a run ------------------------------------------------------------------------------
def test_overflow_in_the_middle_of_a_driven_run_gives_the_bits_of_an_ample_buffer():
    """The scheme of the observer's overflow test (tests/test_gpu_water_classical.py) with rigid molecules: every molecule
    translates towards the centre of the box (one velocity per molecule: on the constraint manifold), a capacity that holds
    the first edge list but not a later one.  The run freezes on the device, gamd_sync_status regrows the buffer and enqueues
    the rest: the library's designed recovery."""
    from gamd_amd.engine import GamdForce
    case = _Water()
    steps = 30
    x0 = torch.from_numpy(case.pos).float().cuda()
    o = np.repeat(case.pos[0::3], 3, axis=0)
    v0 = torch.from_numpy(-(o - case.box / 2) * 6.0).float().cuda()
    probe, _, _, _ = case.make()
    e_now = probe.counts()[0]
    probe.close()
    md = {**case.md, "temperature_k": 0.0}
    res = []
    for cap in (0, e_now + 60):
        eng = GamdForce(case.sd, case.n, case.box, case.rc, edge_capacity=cap, **case.eng_kw)
        x, v = x0.clone(), v0.clone()
        eng.forward(x, species=case.species)
        assert eng.last_status == 0
        f = _water_start(eng, x, case.species)
        eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
        eng.md_run(x, v, f, steps, gamma_per_ps=0.0, seed=1, sync=False, **md)
        status = eng.sync_status()
        assert status == (1 if cap else 0), "the run was meant to outgrow its edge buffer"
        res.append((_state(x, v, f), eng.traj_read()))
        eng.close()
    (sa, ta), (sb, tb) = res
    for a, b in zip(sa, sb):
        assert np.array_equal(_i32(a), _i32(b))
    assert ta.dropped == tb.dropped == 0 and np.array_equal(ta.steps, np.arange(1, steps + 1)) and np.array_equal(tb.steps, ta.steps)
    for name in ("x", "v", "f"):
        assert np.array_equal(_i32(getattr(ta, name)), _i32(getattr(tb, name))), name
    assert np.isfinite(sa[2]).all() and not np.array_equal(sa[0], x0.cpu().numpy())


# ---- 6: two boxes ----------------------------------------------------------------------------------------------------
# The k-vector list of a handle is the list of the longest edge of ALL its boxes; vectors beyond a box's own k_cut carry weight
# zero there, but a longer list moves the borders of the k slices, and with them the order of the reciprocal sum.  A box whose
# own list is the common one gives the same bits alone and in the pair; a box with a shorter list of its own agrees only to the
# bound of tests/test_gpu_water_classical.py on the force (1e-12 of the sum of the absolute terms, then one fp32 rounding).
# Edges (1, 1.03, 0.99) are those of test_gpu_water_classical._two_boxes (box 0's own list is shorter); (1, 0.985, 0.99) leave
# both boxes with the common list.
@pytest.mark.parametrize("scale", [(1.0, 1.03, 0.99), (1.0, 0.985, 0.99)])
@pytest.mark.parametrize("integrator,skin", [("baoab", 0.0), ("nhc", SKIN)])
def test_two_boxes_are_the_two_boxes_run_one_by_one(integrator, skin, scale):
    from gamd_amd.engine import GamdForce
    n_mol, n, steps = 86, 258, 4
    scale = np.array(scale)
    pos, L, species, bonds = wl.water_box(n_mol, seed=5, jitter=0.0, wrap=False)
    other, _, _, _ = wl.water_box(n_mol, seed=7, jitter=0.0, wrap=False)
    second = _scale_centres(other, scale)
    boxes = np.array([[L, L, L], L * scale]).astype(np.float32)
    w = wr.Water(r_cut=6.8, ewald_tol=DELTA)
    assert 2 * w.r_cut <= boxes.min()
    x0 = np.concatenate([pos, second]).astype(np.float32)
    v0 = np.concatenate([_rattled(pos, species, 6), _rattled(second, species, 8)]).astype(np.float32)
    _, _, sd = load_golden("tip3p774_seed3")
    md = dict(dt_ps=DT, mass_amu=wl.MASS_O, mass_h_amu=wl.MASS_H, temperature_k=300.0, rigid_water=True, r_oh=wl.TIP3P_R_OH,
              r_hh=wl.TIP3P_R_HH, remove_cm_motion=True)

    def run(nb, xs, vs, box):
        eng = GamdForce(sd, n, box if nb == 1 else float(L), 4.2, bond=bonds, scaler=SHIPPED_SCALERS["tip3p"], n_boxes=nb, neighbor_skin=skin)
        sp = np.tile(species, nb)
        x, v = torch.from_numpy(xs).cuda(), torch.from_numpy(vs).cuda()
        f = _water_start(eng, x, sp, box=box, **w.kwargs())
        first = f.cpu().numpy().copy()
        if integrator == "baoab":
            # T = 0: no noise (the noise stream of a box is seeded by seed + its index in the handle)
            eng.md_run(x, v, f, steps, gamma_per_ps=25.0, seed=11, box=box, species=sp, **{**md, "temperature_k": 0.0})
        else:
            eng.md_run_nhc(x, v, f, steps, frequency_per_ps=25.0, box=box, species=sp, **md)
        assert eng.last_status == 0
        fcl = eng.water_classical_forces(x, sp, box=box)[0].float().cpu().numpy()
        out = _state(x, v, f)
        assert np.array_equal(_i32(out[2]), _i32(fcl))                       # the force contract, in this handle
        eng.close()
        return out, first

    both, first = run(2, x0, v0, boxes)
    own_is_common = [wr.list_n2max(w.k_cut, boxes[b].max()) == wr.list_n2max(w.k_cut, boxes.max()) for b in range(2)]
    assert own_is_common == ([False, True] if scale[1] > 1.0 else [True, True])
    for b in range(2):
        sl = slice(b * n, (b + 1) * n)
        one, first_one = run(1, x0[sl], v0[sl], boxes[b])
        ref = wr.evaluate(x0[sl], boxes[b], species, w)
        assert ref["near"] == 0
        for got in (first[sl], first_one):                                   # either handle's forces at the start: the reference's
            assert (np.abs(got.astype(np.float64) - ref["forces"]) <= 1e-12 * ref["abs_f"][:, None] + 2.0 ** -24 * np.abs(ref["forces"])).all()
        if own_is_common[b]:
            for name, a, c in zip("xvf", both, one):
                assert np.array_equal(_i32(a[sl]), _i32(c)), f"box {b} {name}"
    assert not np.array_equal(both[2][:n], both[2][n:])


# ---- 7: refusals and no side effects ---------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    from gamd_amd._lib import GamdError, load
    lib = load()
    assert lib.gamd_md_force_source(None, 2) == -22 and b"null handle" in lib.gamd_last_error()
    lj = _Case("lj")
    eng, x, v, f = lj.make()
    with pytest.raises(GamdError, match="-22.*GAMD_KIND_LJ"):              # source 2 on an LJ handle
        eng.md_force_source("water_classical")
    assert eng.force_source == "network"
    eng.close()
    case = _Water()
    eng, x, v, f = case.make()
    with pytest.raises(GamdError, match="-22.*GAMD_KIND_WATER.*GAMD_FORCE_WATER_CLASSICAL"):   # source 1 still refuses water
        eng.md_force_source("classical")
    with pytest.raises(GamdError, match="-22.*gamd_water_configure"):      # no parameters yet
        eng.md_force_source("water_classical")
    assert eng.force_source == "network"
    eng.md_force_source("network")                                          # the default is always accepted
    with pytest.raises(ValueError):
        eng.md_force_source("openmm")
    assert lib.gamd_md_force_source(eng._h, 7) == -22
    assert b"unknown force source 7" in lib.gamd_last_error() and b"GAMD_FORCE_WATER_CLASSICAL" in lib.gamd_last_error()
    eng.water_classical_configure(0, ewald_tol=DELTA)
    case.run(eng, x, v, f, 2, sync=False)
    with pytest.raises(GamdError, match="-22.*enqueued"):                   # a run is pending
        eng.md_force_source("water_classical")
    assert eng.sync_status() == 0 and eng.force_source == "network"
    eng.md_force_source("water_classical")
    eng.md_force_source("network")
    assert eng.force_source == "network"
    eng.close()


@pytest.mark.parametrize("integrator", ["baoab", "nhc"])
def test_refused_runs_leave_x_v_f_untouched(integrator):
    from gamd_amd._lib import GamdError
    case = _Water(integrator)
    half = float(np.float32(0.5) * np.float32(case.box))
    eng, x, v, f = _make(case)
    before = _state(x, v, f)
    run = eng.md_run if integrator == "baoab" else eng.md_run_nhc
    with pytest.raises(GamdError, match="-22.*rigid_water"):                # the potential has no bond or angle term
        run(x, v, f, 4, **{**case.md, "rigid_water": False})
    with pytest.raises(GamdError, match="-22.*species"):
        run(x, v, f, 4, **{**case.md, "species": None})
    eng.water_classical_configure(0, r_cut=half * 1.001, ewald_tol=DELTA)   # the source stays; the box is known at the run
    assert eng.force_source == "water_classical"
    with pytest.raises(GamdError, match="-22.*r_cut"):
        case.run(eng, x, v, f, 4)
    eng.water_classical_configure(0, ewald_tol=DELTA)
    with pytest.raises(GamdError, match="-22.*r_cut"):                      # a smaller box than the constructor's
        run(x, v, f, 4, box=0.9 * case.box, **case.md)
    assert eng.sync_status() == 0
    for a, b in zip(before, _state(x, v, f)):
        assert np.array_equal(_i32(a), _i32(b))
    # the network source minds neither the potential's cutoff nor rigid_water
    eng.water_classical_configure(0, r_cut=half * 1.001, ewald_tol=DELTA)
    eng.md_force_source("network")
    run(x, v, f, 2, **{**case.md, "rigid_water": False, "remove_cm_motion": False})
    assert eng.last_status == 0
    eng.close()


# ---- 8: the network path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skin", [0.0, SKIN])
def test_the_network_path_is_untouched_by_the_source(skin):
    case = _Water(skin=skin)
    sp = case.species
    ref_eng, xr, vr, fr = case.make()
    f_start = fr.clone()
    case.run(ref_eng, xr, vr, fr, 6)
    ref = _state(xr, vr, fr)
    ref_eng.close()

    eng, x, v, f = case.make()
    x0, v0 = x.clone(), v.clone()
    assert torch.equal(f, f_start)
    out0 = eng.forward(x0, species=sp).clone()
    fc = _water_start(eng, x0, sp)
    assert torch.equal(eng.forward(x0, species=sp), out0)                   # forward evaluates the network whatever the source
    xc, vc = x0.clone(), v0.clone()
    case.run(eng, xc, vc, fc, 5, sync=False)
    assert eng.sync_status() == 0
    assert not torch.equal(xc, x0)
    assert torch.equal(eng.forward(x0, species=sp), out0)                   # the source is still the water potential here
    assert eng.force_source == "water_classical"
    eng.md_force_source("network")
    assert torch.equal(eng.forward(x0, species=sp), out0)
    f = eng.forward(x0, species=sp, denormalize=True).clone()
    assert torch.equal(f, f_start)
    case.run(eng, x, v, f, 6)
    for name, a, b in zip("xvf", ref, _state(x, v, f)):
        assert np.array_equal(_i32(a), _i32(b)), name
    eng.close()


# ---- 9: checked build ------------------------------------------------------------------------------------------------
def _frames_of_the_skin_case():
    case = _Water("nhc", skin=SKIN)
    eng, x, v, f = _make(case)
    steps = 8
    eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
    case.run(eng, x, v, f, steps, sync=False)
    status = eng.sync_status()
    tr = eng.traj_read()
    out = _state(x, v, f)
    eng.close()
    return status, tr, out


CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_water_drive as t
from gamd_amd import _lib
status, tr, out = t._frames_of_the_skin_case()
print("RESULT", json.dumps(dict(version=_lib.load().gamd_version().decode(), status=status, steps=tr.steps.tolist(),
                                frames=[t._i32(a).tolist() for a in (tr.x, tr.v, tr.f)], final=[t._i32(a).tolist() for a in out])))
"""


def test_checked_build_gives_the_same_bits():
    """a driven 774-atom skin-mode run under libgamd_hip_chk.so in a child process: a failed device-side range check of any
    kernel of the run would come back as -35; the source's kernels index with nothing they read from memory and give the same
    bits."""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    env = {k: v for k, v in os.environ.items() if k not in ("GAMD_LIB", "GAMD_CHK_INJECT")}
    env["GAMD_LIB"] = CHK
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert p.returncode == 0 and "RESULT" in p.stdout, (p.stdout[-800:], p.stderr[-1500:])
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got["version"].endswith("checked") and got["status"] == 0
    status, tr, out = _frames_of_the_skin_case()
    assert status == 0 and got["steps"] == tr.steps.tolist() == list(range(1, 9))
    for a, b in zip(got["frames"], (tr.x, tr.v, tr.f)):
        assert a == _i32(b).tolist()
    for a, b in zip(got["final"], out):
        assert a == _i32(b).tolist()
