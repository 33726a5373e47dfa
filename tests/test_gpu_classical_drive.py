"""The classical force source on the device (gamd_md_force_source, gamd_amd/csrc/drive.hip): enqueued md_run / md_run_nhc calls
whose forces come from the switched, shifted Lennard-Jones potential of the classical observer instead of the network.

What is asserted, and why the bars are what they are
* The force contract is bit equality: on every recorded frame, and in the final buffer, f viewed as int32 equals
  classical_forces(x)[0].float() viewed as int32 (the observer's kernels on the same fp32 positions, rounded to nearest).  No
  tolerance is involved.
* The integrator chain is judged against the oracle's float64 integrators driven by tests/classical_ref.py, with the bars
  tests/test_gpu_md.py sets for the same chain under network forces: rel_err(x) < 1e-5, rel_err(v) < 1e-4.  The force is not
  judged there (a Lennard-Jones force amplifies a position difference about 13-fold).  Before the device runs, an fp32 numpy
  emulation of the same three steps is checked against the float64 replay with the same bars on the CPU: the bars are
  reachable by fp32 state at all.
* The observer on a driven run: f = RN_fp32(f_cl) per component, so |D_ic| <= 2^-24 |f_cl,ic| and the row's
  sum_i sum_c |D_ic| <= 2^-24 sqrt(3) sum_i |f_cl,i| (Cauchy-Schwarz over the three components); (1 + 1e-12) covers the
  rounding of the two device sums (258 double terms each, test_gpu_classical.py's argument).  No component comes near the fp32
  range (asserted), so no rounding is to infinity or into the subnormals' coarser grid.

The start of every driven 258-atom run is the workload's own box, wl.lj_box(258): the lattice start at the reference's reduced
density, edge 27.2706 A (the golden snapshot's is 27.27), nearest pair 3.07 A, largest classical force component 4.0e2
kJ/mol/nm.  The positions of the lj258_seed0 golden snapshot are NOT used for driven runs: they are uniform random points made
for the network kernels, with 24 pairs below 2.5 A and one at 1.107 A, where the classical force is 2.9e8 kJ/mol/nm.  One
2 fs step under that force moves an atom by more than 100 A; the CPU check of test 2 fails on it (fp32 emulation against the
float64 replay of three BAOAB steps: rel_err x 2.1e-4, v 1.7e-3 against bars of 1e-5 and 1e-4), and the oracle's float64
Nose-Hoover chain itself overflows to NaN in the first step.  A run like that checks nothing about the integrator chain, and
non-finite positions must never reach the neighbour kernels.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import classical_ref as cr
import gamd_oracle as orc
from gamd_amd import workloads as wl
from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
from helpers import load_golden, rel_err
from test_gpu_report import _Case, _state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHK = os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")
SKIN = 1.25                                                # cutoff / 6 of the 7.5 A network cutoff
MODES = [("baoab", 0.0), ("baoab", SKIN), ("nhc", 0.0), ("nhc", SKIN)]


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _seeded_engine(n, box, cutoff=7.5, **kw):
    from gamd_amd.engine import GamdForce
    sd = make_state_dict(ModelConfig(kind="lj", conv_layer=2), 2, 5.0, 1.7)
    return GamdForce(sd, n, box, cutoff, scaler=SHIPPED_SCALERS["lj"], **kw)


class _Lj258(_Case):
    """_Case("lj") (258 atoms, the golden snapshot's weights, velocities and integrator settings) started from the workload's
    lattice box instead of the snapshot's random points (see the module docstring)"""

    def __init__(self, integrator="baoab", **kw):
        super().__init__("lj", integrator, **kw)
        self.pos, self.box = wl.lj_box(self.n)
        assert 2 * cr.LJ().r_cut <= np.float32(self.box)


def _classical_start(eng, x, box=None, length_per_nm=0.0, **lj_kw):
    """parameters (interval 0), the classical source, and the forces a classical-source run must find in f"""
    eng.classical_configure(0, **lj_kw)
    eng.md_force_source("classical")
    assert eng.force_source == "classical"
    return eng.classical_forces(x, box=box, length_per_nm=length_per_nm)[0].float().contiguous()


def _make(case, **lj_kw):
    eng, x, v, f = case.make()
    f = _classical_start(eng, x, length_per_nm=case.len, **lj_kw)
    return eng, x, v, f


def _assert_frames_carry_the_classical_force(eng, tr, x, f, n_frames, box=None, length_per_nm=0.0):
    """every recorded frame and the final state: f == fp32(f_cl(x)) bit for bit"""
    assert tr.dropped == 0 and np.array_equal(tr.steps, np.arange(1, n_frames + 1))
    frames = [(tr.x[t].reshape(-1, 3), tr.f[t].reshape(-1, 3)) for t in range(n_frames)] + [(x.cpu().numpy(), f.cpu().numpy())]
    assert np.array_equal(frames[-1][0], frames[-2][0]) and np.array_equal(_i32(frames[-1][1]), _i32(frames[-2][1]))
    for t, (xs, fs) in enumerate(frames[:-1]):
        fcl = eng.classical_forces(xs, box=box, length_per_nm=length_per_nm)[0]
        assert torch.isfinite(fcl).all() and float(fcl.abs().max()) > 0.0
        assert np.array_equal(_i32(fs), _i32(fcl.float().cpu().numpy())), f"frame {t}"
    assert not np.array_equal(frames[0][0], frames[-1][0])                 # it moved


# ---- 1: forces on every frame ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator,skin", MODES)
def test_lj258_every_frame_carries_the_classical_force_of_its_positions(integrator, skin):
    case = _Lj258(integrator, skin=skin)                                 # BAOAB at 100 K with gamma = 25: noise on
    eng, x, v, f = _make(case)
    steps = 12
    eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
    case.run(eng, x, v, f, steps)
    assert eng.last_status == 0
    _assert_frames_carry_the_classical_force(eng, eng.traj_read(), x, f, steps)
    eng.close()


@pytest.mark.parametrize("n,scale,kw", [
    (300, (1.0, 1.0, 1.0), dict()),                                       # one full tile plus 44, 32 slices of 10
    (64, (1.0, 1.0, 1.0), dict(r_cut=8.5, r_switch=5.1)),                 # below one tile; box 17.1 A
    (1500, (1.0, 0.9, 1.15), dict()),                                     # six tiles, three different edges
    (300, (1.0, 1.0, 1.0), dict(shift=False)),
    (300, (1.0, 1.0, 1.0), dict(r_switch=0.0)),
])
@pytest.mark.parametrize("integrator,skin", [("baoab", SKIN), ("nhc", 0.0)])
def test_shapes_and_potential_forms(n, scale, kw, integrator, skin):
    pos, L = wl.lj_box(n, seed=4)
    s = np.asarray(scale)
    box = (np.float32(L) * s.astype(np.float32)).astype(np.float32)
    lj = cr.LJ(**kw)
    assert 2 * lj.r_cut <= box.min()
    cutoff = 5.0 if n == 64 else 7.5
    if skin and n == 64:
        skin = 0.6                                                        # three cells of cutoff + skin per edge still
    eng = _seeded_engine(n, box, cutoff=cutoff, neighbor_skin=skin)
    x = torch.from_numpy(np.mod(pos * s[None, :], box.astype(np.float64))).float().cuda()
    v = torch.from_numpy(wl.maxwell_boltzmann(n, 100.0, seed=91)).float().cuda()
    f = _classical_start(eng, x, box=box, **lj.kwargs())
    steps = 4
    eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
    md = dict(dt_ps=0.002, mass_amu=39.9, temperature_k=100.0, box=box)
    if integrator == "baoab":
        eng.md_run(x, v, f, steps, gamma_per_ps=25.0, seed=11, **md)
    else:
        eng.md_run_nhc(x, v, f, steps, frequency_per_ps=25.0, **md)
    assert eng.last_status == 0
    _assert_frames_carry_the_classical_force(eng, eng.traj_read(), x, f, steps, box=box)
    eng.close()


# ---- 2: the chain against the oracle's integrators -------------------------------------------------------------------
DT, MASS, GAMMA, FREQ, CHAIN = 0.002, 39.9, 25.0, 25.0, 10


def _chain_start():
    pos, box = wl.lj_box(258)
    x = pos.astype(np.float32)
    v = np.random.default_rng(1).normal(0, 1.4, x.shape).astype(np.float32)
    return x, v, box


def _replay_f64(integrator, x, v, f, box, steps):
    """the oracle's integrators in float64 around the float64 reference of the potential"""
    lj, boxw = cr.LJ(), float(np.float32(box))
    xr, vr, fr = x.astype(np.float64), v.astype(np.float64), f.astype(np.float64)
    st = orc.nhc_init(CHAIN, FREQ)
    kT, ndf = wl.KB * 100.0, 3.0 * x.shape[0]
    for _ in range(steps):
        if integrator == "baoab":
            xr, vr = orc.baoab_first_half(xr, vr, fr, 10.0 / MASS, DT, np.exp(-GAMMA * DT), 0.0, 0.0)
        else:
            xr, vr = orc.nhc_first_half(st, xr, vr, fr, MASS, DT, kT, FREQ, ndf)
        xr = np.mod(xr, boxw)
        fr = cr.evaluate(xr, box, lj)["forces"]
        vr = orc.baoab_second_half(vr, fr, 10.0 / MASS, DT) if integrator == "baoab" else orc.nhc_second_half(st, vr, fr, MASS, DT, kT, FREQ, ndf)
    return xr, vr


def _emulate_f32(integrator, x, v, f, box, steps):
    """the same three steps with x, v, f held in fp32 and every integrator operation rounded to fp32 (the chain variables
    and the kinetic-energy sum stay in double, as on the device); the force is the fp32 rounding of the float64 reference on
    the fp32 positions"""
    f32 = np.float32
    lj, boxw = cr.LJ(), f32(box)
    x, v, f = x.astype(f32), v.astype(f32), f.astype(f32)
    h, inv_m, a = f32(0.5 * DT), f32(10.0) * (f32(1.0) / f32(MASS)), f32(np.exp(-GAMMA * DT))
    st = orc.nhc_init(CHAIN, FREQ)
    kT, ndf, m = wl.KB * 100.0, 3.0 * x.shape[0], float(f32(MASS))

    def scale(vv):
        ke2 = float(np.sum(m * (0.1 * vv.astype(np.float64)) ** 2))
        return f32(orc.nhc_propagate(st, ke2, DT, kT, FREQ, ndf))

    for _ in range(steps):
        if integrator == "baoab":
            v = v + (h * f) * inv_m
            x = x + h * v
            v = a * v
            x = x + h * v
        else:
            v = v * scale(v)
            v = v + (h * f) * inv_m
            x = x + f32(DT) * v
        x = np.mod(x, boxw).astype(f32)
        f = cr.evaluate(x, box, lj)["forces"].astype(f32)
        v = v + (h * f) * inv_m
        if integrator == "nhc":
            v = v * scale(v)
    return x, v


@pytest.mark.parametrize("integrator", ["baoab", "nhc"])
def test_three_deterministic_steps_match_the_oracle_integrators(integrator):
    x0, v0, box = _chain_start()
    steps, lj = 3, cr.LJ()
    f0 = cr.evaluate(x0, box, lj)["forces"].astype(np.float32)
    xr, vr = _replay_f64(integrator, x0, v0, f0, box, steps)
    # on the CPU first: fp32 state can stay inside the bars at all
    xe, ve = _emulate_f32(integrator, x0, v0, f0, box, steps)
    print(f"{integrator}: fp32 emulation against the float64 replay: rel_err x {rel_err(xe, xr):.3e}, v {rel_err(ve, vr):.3e}")
    assert rel_err(xe, xr) < 1e-5 and rel_err(ve, vr) < 1e-4
    from gamd_amd.engine import GamdForce
    _, _, sd = load_golden("lj258_seed0")
    eng = GamdForce(sd, 258, box, 7.5, scaler=SHIPPED_SCALERS["lj"])
    assert 2 * lj.r_cut <= np.float32(box)
    x, v = torch.from_numpy(x0).cuda(), torch.from_numpy(v0).cuda()
    f = _classical_start(eng, x)
    assert rel_err(f.cpu().numpy(), f0) < 1e-6                               # (the force itself is judged bit for bit above)
    if integrator == "baoab":
        eng.md_run(x, v, f, steps, dt_ps=DT, mass_amu=MASS, temperature_k=0.0, gamma_per_ps=GAMMA)
    else:
        eng.md_run_nhc(x, v, f, steps, dt_ps=DT, mass_amu=MASS, temperature_k=100.0, frequency_per_ps=FREQ, chain_length=CHAIN)
    ex, ev = rel_err(x.cpu().numpy(), xr), rel_err(v.cpu().numpy(), vr)
    print(f"{integrator}: device against the float64 replay: rel_err x {ex:.3e}, v {ev:.3e}")
    assert ex < 1e-5
    assert ev < 1e-4
    eng.close()


# ---- 3: the same bits ------------------------------------------------------------------------------------------------
def _driven(case, calls, observers=False):
    """a classical-source run of the case in `calls` calls of K steps each (first_step and the chain carried on)"""
    eng, x, v, f = _make(case)
    if observers:                                                       # all five configurable observers; water's is not this kind's
        eng.report_configure(3, rdf_bins=32)
        eng.traj_configure(3, max_frames=8, fields=("x", "v", "f", "image"), n_lags=3)
        eng.structure_configure(3, rdf_bins=32, sk_n2max=4)
        eng.classical_configure(3)
    chain = None
    for c, k in enumerate(calls):
        chain = case.run(eng, x, v, f, k, first_step=sum(calls[:c]), chain=chain)
        assert eng.last_status == 0
    out = _state(x, v, f)
    rows = eng.classical_read().steps if observers else None
    eng.close()
    return out, rows


@pytest.mark.parametrize("integrator,skin", MODES)
def test_chunked_runs_fresh_handles_and_armed_observers_give_the_same_bits(integrator, skin):
    K = 6
    case = _Lj258(integrator, skin=skin, K=K)
    one, _ = _driven(case, [2 * K])
    two, _ = _driven(case, [K, K])
    again, _ = _driven(case, [2 * K])
    armed, rows = _driven(case, [2 * K], observers=True)
    assert np.array_equal(rows, 3 * np.arange(1, 5))
    for name, other in (("two calls", two), ("second handle", again), ("observers armed", armed)):
        for a, b in zip(one, other):
            assert np.array_equal(_i32(a), _i32(b)), name
    assert not np.array_equal(one[0], np.mod(case.pos, case.box).astype(np.float32))


# ---- 4: the observer on a driven run ---------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator,skin", [("baoab", SKIN), ("nhc", 0.0)])
def test_observer_rows_on_a_driven_run(integrator, skin, tmp_path):
    case = _Lj258(integrator, skin=skin)
    eng, x, v, f = _make(case)
    steps = 8
    eng.classical_configure(2)
    eng.report_configure(2)
    eng.traj_configure(1, max_frames=steps, fields=("x", "f"))
    case.run(eng, x, v, f, steps)
    rd, rep, tr = eng.classical_read(forces=True), eng.report_read(), eng.traj_read()
    assert rd.dropped == 0 and np.array_equal(rd.steps, [2, 4, 6, 8]) and np.array_equal(rep.steps, rd.steps)
    for q, g in enumerate(rd.steps):
        xs = tr.x[g - 1].reshape(-1, 3)
        fcl, e, w, c = eng.classical_forces(xs)
        fcl = fcl.cpu().numpy()
        assert np.abs(fcl).max() < 1e30                                  # nowhere near the fp32 range
        assert _i64(rd.energy[q])[0] == _i64(e)[0] and _i64(rd.virial[q])[0] == _i64(w)[0] and rd.pairs[q, 0] == c[0] > 0
        norm = np.sqrt((fcl * fcl).sum(axis=1)).sum()
        bound = 2.0 ** -24 * np.sqrt(3.0) * norm * (1.0 + 1e-12)
        print(f"{integrator} step {g}: sum |D_ic| = {rd.sum_abs[q, 0]:.6e}, bound {bound:.6e}, sum |f_cl| = {rd.sum_norm_cl[q, 0]:.9e}")
        assert abs(rd.sum_norm_cl[q, 0] - norm) <= 1e-12 * norm
        assert 0.0 < rd.sum_abs[q, 0] <= bound
        assert rd.excluded[q, 0] == 0
    assert np.array_equal(_i64(rd.forces), _i64(eng.classical_forces(tr.x[-1].reshape(-1, 3))[0].cpu().numpy()))
    path = tmp_path / "log_nvt_lj_gt.txt"
    rd.write_state_data(rep, path, 0.002)
    lines = open(path).read().splitlines()
    assert lines[0].count("\t") == 5 and "Potential Energy" in lines[0].split("\t")[2]
    cols = [ln.split("\t") for ln in lines[1:]]
    assert len(cols) == 4 and all(len(c) == 6 for c in cols)
    assert [float(c[2]) for c in cols] == [float(e) for e in rd.energy[:, 0]]
    assert [float(c[4]) for c in cols] == [float(rd.energy[q, 0]) + float(rep.ke[q, 0]) for q in range(4)]
    eng.close()


# ---- 5: overflow in the middle of a run ------------------------------------------------------------------------------
def test_overflow_in_the_middle_of_a_driven_run_gives_the_bits_of_an_ample_buffer():
    """The scheme of test_overflow_in_the_middle_of_a_run_writes_every_row_once_with_the_bits_of_an_ample_buffer
    (tests/test_gpu_classical.py): five contracting boxes, a capacity that holds the first edge list but not a later one.  The
    run freezes on the device, gamd_sync_status regrows the buffer and enqueues the rest: the library's designed recovery."""
    nb, n, rc, steps = 5, 258, 7.5, 30
    base, box = wl.lj_box(n)
    assert 2 * cr.LJ().r_cut <= np.float32(box)
    kw = dict(n_boxes=nb)
    rng = np.random.default_rng(2)
    pos = np.concatenate([base + (rng.normal(0, 0.3, base.shape) if b else 0.0) for b in range(nb)])
    x0 = torch.from_numpy(pos).float().cuda()
    v0 = (-(torch.remainder(x0, box) - box / 2)).contiguous() * 1.5
    probe = _seeded_engine(n, box, cutoff=rc, **kw)
    probe.forward(x0)
    e_now = probe.counts()[0]
    probe.close()
    res = []
    for cap in (0, e_now + 40):
        eng = _seeded_engine(n, box, cutoff=rc, edge_capacity=cap, **kw)
        x, v = x0.clone(), v0.clone()
        eng.forward(x)
        assert eng.last_status == 0
        f = _classical_start(eng, x)
        eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
        eng.md_run(x, v, f, steps, temperature_k=0.0, gamma_per_ps=0.0, seed=1, sync=False)
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
@pytest.mark.parametrize("skin", [0.0, SKIN])
def test_two_boxes_are_the_two_boxes_run_one_by_one(skin):
    n, steps = 300, 4
    pos, L = wl.lj_box(n, seed=4)
    boxes = np.array([[L, L, L], [L, 1.05 * L, 0.97 * L]], dtype=np.float32)
    assert 2 * cr.LJ().r_cut <= boxes.min()
    rng = np.random.default_rng(8)
    second = np.mod(pos * np.array([1.0, 1.05, 0.97]) + rng.normal(0, 0.3, pos.shape), boxes[1].astype(np.float64))
    x0 = np.concatenate([pos, second]).astype(np.float32)
    v0 = np.concatenate([wl.maxwell_boltzmann(n, 100.0, seed=90 + b) for b in range(2)]).astype(np.float32)
    md = dict(dt_ps=0.002, mass_amu=39.9, temperature_k=0.0, gamma_per_ps=25.0)

    def run(eng, xs, vs, box):
        x, v = torch.from_numpy(xs).cuda(), torch.from_numpy(vs).cuda()
        f = _classical_start(eng, x, box=box)
        eng.md_run(x, v, f, steps, box=box, **md)
        assert eng.last_status == 0
        out = _state(x, v, f)
        eng.close()
        return out

    both = run(_seeded_engine(n, float(L), n_boxes=2, neighbor_skin=skin), x0, v0, boxes)
    for b in range(2):
        sl = slice(b * n, (b + 1) * n)
        one = run(_seeded_engine(n, boxes[b], neighbor_skin=skin), x0[sl], v0[sl], boxes[b])
        for a, c in zip(both, one):
            assert np.array_equal(_i32(a[sl]), _i32(c)), f"box {b}"
    assert not np.array_equal(both[2][:n], both[2][n:])


# ---- 7: refusals and no side effects ---------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    from gamd_amd._lib import GamdError, load
    lib = load()
    assert lib.gamd_md_force_source(None, 1) == -22 and b"null handle" in lib.gamd_last_error()
    water = _Case("water")
    eng, x, v, f = water.make()
    with pytest.raises(GamdError, match="-22.*GAMD_KIND_WATER"):
        eng.md_force_source("classical")
    eng.md_force_source("network")                                          # the default is always accepted
    assert eng.force_source == "network"
    eng.close()
    case = _Case("lj")
    eng, x, v, f = case.make()
    with pytest.raises(GamdError, match="-22.*gamd_classical_configure"):   # no parameters yet
        eng.md_force_source("classical")
    assert eng.force_source == "network"
    with pytest.raises(ValueError):
        eng.md_force_source("openmm")
    assert lib.gamd_md_force_source(eng._h, 7) == -22 and b"unknown force source 7" in lib.gamd_last_error()
    eng.classical_configure(0)
    case.run(eng, x, v, f, 2, sync=False)
    with pytest.raises(GamdError, match="-22.*enqueued"):                   # a run is pending
        eng.md_force_source("classical")
    assert eng.sync_status() == 0 and eng.force_source == "network"
    eng.md_force_source("classical")
    eng.close()


@pytest.mark.parametrize("integrator", ["baoab", "nhc"])
def test_a_box_below_two_cutoffs_refuses_the_run_before_anything_is_enqueued(integrator):
    case = _Lj258(integrator)
    half = float(np.float32(0.5) * np.float32(case.box))
    eng, x, v, f = _make(case)
    before = _state(x, v, f)
    from gamd_amd._lib import GamdError
    eng.classical_configure(0, r_cut=half * 1.001)                          # the source stays; the box is known at the run
    assert eng.force_source == "classical"
    with pytest.raises(GamdError, match="-22.*r_cut"):
        case.run(eng, x, v, f, 4)
    eng.classical_configure(0)
    with pytest.raises(GamdError, match="-22.*r_cut"):                      # a smaller box than the constructor's
        (eng.md_run if integrator == "baoab" else eng.md_run_nhc)(x, v, f, 4, box=0.74 * case.box, **case.md)
    assert eng.sync_status() == 0
    for a, b in zip(before, _state(x, v, f)):
        assert np.array_equal(_i32(a), _i32(b))
    # the network source does not mind the potential's cutoff
    eng.classical_configure(0, r_cut=half * 1.001)
    eng.md_force_source("network")
    case.run(eng, x, v, f, 2)
    eng.close()


@pytest.mark.parametrize("skin", [0.0, SKIN])
def test_the_network_path_is_untouched_by_the_source(skin):
    case = _Lj258(skin=skin)
    ref_eng, xr, vr, fr = case.make()
    f_start = fr.clone()
    case.run(ref_eng, xr, vr, fr, 6)
    ref = _state(xr, vr, fr)
    ref_eng.close()

    eng, x, v, f = case.make()
    x0, v0 = x.clone(), v.clone()
    assert torch.equal(f, f_start)
    out0 = eng.forward(x0).clone()
    fc = _classical_start(eng, x0)
    assert torch.equal(eng.forward(x0), out0)                               # forward evaluates the network whatever the source
    xc, vc = x0.clone(), v0.clone()
    case.run(eng, xc, vc, fc, 5)
    assert not torch.equal(xc, x0)
    assert torch.equal(eng.forward(x0), out0)
    eng.md_force_source("network")
    assert torch.equal(eng.forward(x0), out0)
    f = eng.forward(x0, denormalize=True).clone()
    assert torch.equal(f, f_start)
    case.run(eng, x, v, f, 6)
    for name, a, b in zip("xvf", ref, _state(x, v, f)):
        assert np.array_equal(_i32(a), _i32(b)), name
    eng.close()


# ---- 8: checked build ------------------------------------------------------------------------------------------------
def _frames_of_the_skin_case():
    case = _Lj258("baoab", skin=SKIN)
    eng, x, v, f = _make(case)
    steps = 12
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
import test_gpu_classical_drive as t
from gamd_amd import _lib
status, tr, out = t._frames_of_the_skin_case()
print("RESULT", json.dumps(dict(version=_lib.load().gamd_version().decode(), status=status, steps=tr.steps.tolist(),
                                frames=[t._i32(a).tolist() for a in (tr.x, tr.v, tr.f)], final=[t._i32(a).tolist() for a in out])))
"""


def test_checked_build_gives_the_same_bits():
    """test 1's 258-atom skin case under libgamd_hip_chk.so in a child process: a failed device-side range check of any kernel
    of the run would come back as -35; the drive kernels index with nothing they read from memory and give the same bits."""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    env = {k: v for k, v in os.environ.items() if k not in ("GAMD_LIB", "GAMD_CHK_INJECT")}
    env["GAMD_LIB"] = CHK
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert p.returncode == 0 and "RESULT" in p.stdout, (p.stdout[-800:], p.stderr[-1500:])
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got["version"].endswith("checked") and got["status"] == 0
    status, tr, out = _frames_of_the_skin_case()
    assert status == 0 and got["steps"] == tr.steps.tolist() == list(range(1, 13))
    for a, b in zip(got["frames"], (tr.x, tr.v, tr.f)):
        assert a == _i32(b).tolist()
    for a, b in zip(got["final"], out):
        assert a == _i32(b).tolist()
