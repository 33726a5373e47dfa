"""The TIP4P M-site in the water classical potential on the device (gamd_water_msite, gamd_amd/csrc/water_msite.hip): given
positions, the observer inside enqueued runs and the water classical force source, with TIP4P-Ew parameters, against the
float64 host reference of tests/water_msite_ref.py.

Shapes: 86 molecules (258 atoms, L = 13.87 A, r_cut 6.8: one full 256-atom tile and a second one of 2 atoms, the last molecule
of the first tile split O | H,H across the tile edge; 86 oxygens in the Lennard-Jones pass) nearly everywhere, and one case at
258 molecules (774 atoms, r_cut 9.5: three full tiles, a tail of 6, several slices; 258 oxygens = one full tile of the
Lennard-Jones pass plus 2).

Tolerances are those of tests/test_gpu_water_classical.py, for the same reason: the device and the reference evaluate a term
with the same operations and differ in the order of the sums, in erfc / erf / exp / sincospi and — here — in the image a site
is held in (the device wraps O and H into the box before it forms M, the reference does not: one rounding of a minimum-image
difference).  Each energy term and each force component lies within 1e-12 of the sum of the absolute values of its terms, the
redistribution included: abs_F[O] = (1 - 2 w) abs_f_site[M] + abs_f_LJ[O], abs_F[H] = abs_f_site[H] + w abs_f_site[M].  Pair
counts are exact (no charge-site pair and no O-O pair within 1e-12 r_cut of the cutoff, asserted) and the charge sum is exactly
0.  The force contract of the source is bit equality with water_classical_forces rounded to fp32.  Nothing here claims parity
with OpenMM: the TIP4P-Ew parameters are unverified."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import classical_ref as cr
import water_classical_ref as wr
import water_msite_ref as w4
from gamd_amd import workloads as wl
from test_gpu_classical_drive import _i32
from test_gpu_report import _Case, _state, _f32
from test_gpu_water_classical import _Water, _engine, _bits, _rows, DELTA, TOL
from test_gpu_water_drive import _assert_frames_carry_the_classical_force, _rattled, _scale_centres, SKIN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHK = os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")
W = w4.TIP4PEW_W
RC = 6.8                                                   # 2 r_cut <= 13.66, the shortest edge any 86-molecule case here has
Q_H, SIGMA, EPS = 0.52422, 3.16435, 0.680946


def _water(unit=1.0, r_cut=RC, **kw):
    return wr.Water(q_h=Q_H, sigma_o=SIGMA * unit, epsilon_o=EPS, r_cut=r_cut * unit, ewald_tol=DELTA, **kw)


def _conf(eng, interval=0, m_site=W, wat=None, **kw):
    eng.water_classical_configure(interval, m_site=m_site, **{**(wat or _water()).kwargs(), **kw})


def _check_box(tag, row, x_box, box, species, wat, w, length_per_nm, fcl_dev, f_run=None):
    """one box of one frame against water_msite_ref: row [12] from the device, fcl_dev [n, 3] the device's forces"""
    ref = w4.evaluate(x_box, box, species, wat, w, length_per_nm)
    fr = dict(lj=abs(row[0] - ref["u_lj"]) / (TOL * ref["abs_lj"]), coul=abs(row[1] - ref["u_coul"]) / (TOL * ref["abs_real"]),
              recip=abs(row[2] - ref["u_recip"]) / (TOL * ref["abs_recip"]), self=abs(row[3] - ref["u_self"]) / (TOL * abs(ref["u_self"])),
              force=(np.abs(fcl_dev - ref["forces"]) / (TOL * ref["abs_f"][:, None])).max())
    print(f"{tag}: pairs {row[4]:.0f} (ref {ref['pairs']:.0f}, {ref['near']} + {ref['near_lj']} at the cutoff), K {ref['n_k']}, U_LJ {row[0]:.9e} "
          f"U_coul {row[1]:.9e} U_recip {row[2]:.9e} U_self {row[3]:.9e}, sum q {row[11]!r}; |dev - ref| / bound: "
          + ", ".join(f"{k} {v:.3e}" for k, v in fr.items()))
    assert ref["near"] == 0 and ref["near_lj"] == 0, "ill-posed: a pair sits on a cutoff"
    assert ref["pairs"] > 0 and row[4] == ref["pairs"] and ref["abs_lj"] > 0
    assert row[11] == 0.0 and ref["sum_q"] == 0.0
    assert all(v <= 1.0 for v in fr.values()) and np.isfinite(fcl_dev).all()
    if f_run is not None:
        sums, ab = cr.force_error_sums(f_run, fcl_dev)
        ratio = np.abs(row[5:10] - sums[:5]) / (TOL * ab)
        print(f"{tag}: force-error sums {row[5:10]}, |dev - host| / bound {ratio}, left out of the cosine {row[10]:.0f}")
        assert (ab > 0).all() and (ratio <= 1.0).all() and row[10] == sums[5]
    else:
        assert (row[5:11] == 0.0).all()
    return ref


# ---- 1: given positions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mol,r_cut,length_per_nm", [(86, RC, 0.0), (86, RC, wl.BOHR_PER_NM), (258, 9.5, 0.0)])
def test_forces_on_given_positions(n_mol, r_cut, length_per_nm):
    unit = _f32(length_per_nm) / 10.0 if length_per_nm else 1.0
    pos, box, _, _ = wl.water_box(n_mol, seed=5, jitter=0.02, wrap=False)
    x, box = (pos * unit).astype(np.float32), np.float32(box * unit)
    wat = _water(unit, r_cut)
    assert 2 * wat.r_cut <= box
    eng, species = _engine(n_mol, float(box))
    _conf(eng, wat=wat, length_per_nm=length_per_nm)
    f, rd = eng.water_classical_forces(x, species, length_per_nm=length_per_nm)
    assert f.dtype == torch.float64 and tuple(f.shape) == (3 * n_mol, 3)
    fh = f.cpu().numpy()
    ref = _check_box(f"{3 * n_mol} atoms, len {length_per_nm}", _rows(rd)[0], x, box, species, wat, W, length_per_nm, fh)
    assert abs(rd.energy[0, 0] - ref["energy"]) <= TOL * ref["abs_energy"]
    # it is another potential than the 3-site one with the same parameters
    three = wr.evaluate(x, box, species, wat, length_per_nm)
    assert np.abs(fh - three["forces"]).max() > 1e-3 * np.abs(fh).max() and abs(rd.u_real[0, 0] - three["u_coul"]) > 1e-3 * abs(three["u_coul"])
    eng.close()


# ---- 2: two boxes ----------------------------------------------------------------------------------------------------
def test_two_boxes_with_different_positions_and_edges_are_the_boxes_alone():
    """edges (1, 0.985, 0.99) of the second box leave both boxes with the handle's common k-vector list (the longest edge is
    the first box's), so a box alone in a one-box handle has the same slices and gives the same bits"""
    scale = np.array([1.0, 0.985, 0.99])
    pos, L, _, _ = wl.water_box(86, seed=5, jitter=0.02, wrap=False)
    other, _, _, _ = wl.water_box(86, seed=7, jitter=0.02, wrap=False)
    x = np.concatenate([pos, _scale_centres(other, scale)]).astype(np.float32)
    boxes = np.array([[L, L, L], L * scale]).astype(np.float32)
    wat = _water()
    assert 2 * wat.r_cut <= boxes.min()
    eng, species = _engine(86, float(boxes[0, 0]), n_boxes=2)
    _conf(eng)
    f, rd = eng.water_classical_forces(x, species, box=boxes)
    fh, rows = f.cpu().numpy(), _rows(rd)
    assert rd.u_real[0, 0] != rd.u_real[0, 1] and rd.u_recip[0, 0] != rd.u_recip[0, 1]
    for b in range(2):
        sl = slice(b * 258, (b + 1) * 258)
        _check_box(f"box {b}", rows[b], x[sl], boxes[b], species, wat, W, 0.0, fh[sl])
        one, _ = _engine(86, boxes[b])
        _conf(one)
        f1, r1 = one.water_classical_forces(x[sl], species, box=boxes[b])
        assert np.array_equal(_bits(f1.cpu().numpy()), _bits(fh[sl])), b
        assert np.array_equal(_bits(_rows(r1)[0]), _bits(rows[b])), b
        one.close()
    eng.close()


# ---- 3: periodic images ----------------------------------------------------------------------------------------------
def test_atoms_in_other_periodic_images_and_a_second_call_give_the_same_bits():
    """Positions and box edges on a grid of 2^-10 A (edges 13.875, 13.75, 14.0): x + k L is exact in fp32, so the O -> H vectors,
    the wrapped O and H, M, every site difference and every O-O difference are the same doubles for every image.  Atom-wise
    shifts: every molecule is torn across images — M must be built from minimum-image O -> H vectors."""
    q = 2.0 ** -10
    pos, L, _, _ = wl.water_box(86, seed=5, jitter=0.02, wrap=False)
    box = np.array([13.875, 13.75, 14.0], dtype=np.float32)
    x = (np.rint(_scale_centres(pos, box.astype(np.float64) / L) / q) * q).astype(np.float32)
    k = np.random.default_rng(3).integers(-2, 3, size=x.shape)
    xs = (x.astype(np.float64) + k * box.astype(np.float64)[None, :]).astype(np.float32)
    assert np.array_equal(xs.astype(np.float64), x.astype(np.float64) + k * box.astype(np.float64)[None, :])
    assert (k.reshape(-1, 3, 3) != k.reshape(-1, 3, 3)[:, :1]).any(axis=(1, 2)).sum() > 80         # torn molecules
    eng, species = _engine(86, box)
    _conf(eng)
    a = eng.water_classical_forces(x, species, box=box)
    b = eng.water_classical_forces(xs, species, box=box)
    c = eng.water_classical_forces(x, species, box=box)
    for other in (b, c):
        assert np.array_equal(_bits(a[0].cpu().numpy()), _bits(other[0].cpu().numpy()))
        assert np.array_equal(_bits(_rows(a[1])), _bits(_rows(other[1])))
    _check_box("on the grid", _rows(a[1])[0], x, box, species, _water(), W, 0.0, a[0].cpu().numpy())
    _check_box("torn across images", _rows(b[1])[0], xs, box, species, _water(), W, 0.0, b[0].cpu().numpy())
    eng.close()


# ---- 4: weight zero --------------------------------------------------------------------------------------------------
def test_weight_zero_is_the_three_site_potential_bit_for_bit():
    from gamd_amd._lib import GamdWaterParams
    pos, box, _, _ = wl.water_box(86, seed=5, jitter=0.02, wrap=False)
    x, wat = pos.astype(np.float32), _water()
    # a handle that never heard of the M-site: gamd_water_configure alone
    eng, species = _engine(86, float(box))
    p = GamdWaterParams(0, 0, wat.q_h, wat.lj.sigma, wat.lj.epsilon, wat.r_cut, 0.0, 0, 0, wat.alpha, wat.k_cut, wat.coulomb_const)
    assert eng._lib.gamd_water_configure(eng._h, C.byref(p)) == 0
    eng._water_set = True
    f0, r0 = eng.water_classical_forces(x, species)
    eng.close()
    eng, species = _engine(86, float(box))
    _conf(eng, m_site=0.0)
    f1, r1 = eng.water_classical_forces(x, species)
    _conf(eng, m_site=W)
    f2, r2 = eng.water_classical_forces(x, species)
    _conf(eng, interval=0)                                                     # the weight holds across the C configure call ...
    assert eng._lib.gamd_water_configure(eng._h, C.byref(p)) == 0
    f3, r3 = eng.water_classical_forces(x, species)
    _conf(eng, m_site=0.0)                                                     # ... until it is set again
    f4, r4 = eng.water_classical_forces(x, species)
    eng.close()
    for f, r in ((f1, r1), (f4, r4)):
        assert np.array_equal(_bits(f.cpu().numpy()), _bits(f0.cpu().numpy())) and np.array_equal(_bits(_rows(r)), _bits(_rows(r0)))
    assert np.array_equal(_bits(f3.cpu().numpy()), _bits(f2.cpu().numpy())) and np.array_equal(_bits(_rows(r3)), _bits(_rows(r2)))
    assert np.abs((f2 - f0).cpu().numpy()).max() > 1e-3 * np.abs(f0.cpu().numpy()).max()
    assert r2.u_real[0, 0] != r0.u_real[0, 0] and r2.u_recip[0, 0] != r0.u_recip[0, 0] and r2.u_self[0, 0] == r0.u_self[0, 0]


# ---- 5: the observer in a run ----------------------------------------------------------------------------------------
def _reference_frames(case, chunks):
    """observer-off run (a handle that was never configured) cut into `chunks` calls of K steps: final state, (x, f) at every
    cut, and afterwards the device's 4-site forces on every frame"""
    eng, x, v, f = case.make()
    chain, frames = None, []
    for c in range(chunks):
        chain = case.run(eng, x, v, f, case.K, first_step=c * case.K, chain=chain)
        xs, _, fs = _state(x, v, f)
        frames.append((xs, fs))
    out = _state(x, v, f)
    _conf(eng)
    fcl = [eng.water_classical_forces(xs, case.species, box=case.box)[0].cpu().numpy() for xs, _ in frames]
    eng.close()
    return out, frames, fcl


def _sampled_run(case, chunks):
    eng, x, v, f = case.make()
    _conf(eng, interval=case.K)
    eng.report_configure(case.K, **case.report_kw())
    case.run(eng, x, v, f, chunks * case.K)
    rd, rep = eng.water_classical_read(forces=True), eng.report_read()
    out = _state(x, v, f)
    eng.close()
    return out, rd, rep


@pytest.mark.parametrize("integrator,skin", [("baoab", 0.0), ("nhc", SKIN)])
def test_rows_are_the_reference_on_the_frames_of_an_observer_off_run(integrator, skin):
    chunks = 2
    case = _Water(integrator, skin=skin, n_mol=86, K=3)
    (xr, vr, fr), frames, fcl = _reference_frames(case, chunks)
    (x, v, f), rd, rep = _sampled_run(case, chunks)
    assert np.array_equal(x, xr) and np.array_equal(v, vr) and np.array_equal(f, fr)        # the observer does not perturb the run
    assert rd.dropped == 0 and np.array_equal(rd.steps, case.K * np.arange(1, chunks + 1)) and np.array_equal(rd.steps, rep.steps)
    for q, (xs, fs) in enumerate(frames):
        _check_box(f"{integrator} skin {skin} frame {q}", _rows(rd, q)[0], xs, case.box, case.species, _water(), W, 0.0, fcl[q], fs)
    assert np.array_equal(_bits(rd.forces), _bits(fcl[-1]))


# ---- 6: the force source ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _minimised_start():
    """the documented start recipe, once: the 86-molecule lattice minimised with w = 0 (tolerance 10 kJ/mol/nm), rattled 300 K
    velocities on the minimised geometry"""
    case = _Water(n_mol=86)
    eng, x, v, f = case.make()
    _conf(eng, m_site=0.0)
    m = eng.water_minimize(x, case.species, tolerance=10.0, r_oh=wl.TIP3P_R_OH, r_hh=wl.TIP3P_R_HH)
    assert m.status == 0
    xm = x.cpu().numpy().copy()
    eng.close()
    return xm, _rattled(xm.astype(np.float64), case.species, 6).astype(np.float32)


def _start(case, m_site=W, eng=None):
    """the weight set behind the minimiser, f = fp32(water_classical_forces(x))"""
    xm, vm = _minimised_start()
    if eng is None:
        eng, _, _, _ = case.make()
    x, v = torch.from_numpy(xm).cuda(), torch.from_numpy(vm).cuda()
    _conf(eng, m_site=m_site)
    eng.md_force_source("water_classical")
    f = eng.water_classical_forces(x, case.species)[0].float().contiguous()
    return eng, x, v, f


def _driven(case, calls, observers=False, m_site=W):
    eng, x, v, f = _start(case, m_site)
    if observers:
        eng.report_configure(2, **case.report_kw())
        _conf(eng, interval=2, m_site=m_site)
    chain = None
    for c, k in enumerate(calls):
        chain = case.run(eng, x, v, f, k, first_step=sum(calls[:c]), chain=chain)
        assert eng.last_status == 0
    out = _state(x, v, f)
    rd = eng.water_classical_read() if observers else None
    eng.close()
    return out, rd


@pytest.mark.parametrize("integrator,skin", [("baoab", SKIN), ("nhc", 0.0)])
def test_every_frame_of_a_driven_run_carries_the_four_site_force_of_its_positions(integrator, skin):
    case = _Water(integrator, skin=skin, n_mol=86)
    eng, x, v, f = _start(case)
    x0 = x.cpu().numpy().copy()
    ref = w4.evaluate(x0, case.box, case.species, _water(), W)                # the start forces are the potential meant
    assert (np.abs(f.cpu().numpy() - ref["forces"]) <= TOL * ref["abs_f"][:, None] + 2.0 ** -24 * np.abs(ref["forces"])).all()
    steps = 8
    eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
    case.run(eng, x, v, f, steps)
    assert eng.last_status == 0
    _assert_frames_carry_the_classical_force(eng, eng.traj_read(), x, f, case.species, steps)
    eng.close()


@pytest.mark.parametrize("integrator,skin", [("baoab", 0.0), ("nhc", SKIN)])
def test_chunked_runs_fresh_handles_and_an_armed_observer_give_the_same_bits(integrator, skin):
    K = 4
    case = _Water(integrator, skin=skin, n_mol=86, K=K)
    one, _ = _driven(case, [2 * K])
    two, _ = _driven(case, [K, K])
    again, _ = _driven(case, [2 * K])
    armed, rd = _driven(case, [2 * K], observers=True)
    three, _ = _driven(case, [2 * K], m_site=0.0)
    assert np.array_equal(rd.steps, 2 * np.arange(1, 5)) and (rd.pairs > 0).all() and (rd.sum_q == 0.0).all()
    # f = RN_fp32(f_cl): the observer's error sums of a driven step are those of one rounding
    assert (rd.sum_abs[:, 0] > 0).all() and (rd.sum_abs[:, 0] <= 2.0 ** -24 * np.sqrt(3.0) * rd.sum_norm_cl[:, 0] * (1.0 + 1e-12)).all()
    for name, other in (("two calls", two), ("second handle", again), ("observer armed", armed)):
        for a, b in zip(one, other):
            assert np.array_equal(_i32(a), _i32(b)), name
    assert not np.array_equal(_i32(one[0]), _i32(three[0])) and not np.array_equal(_i32(one[2]), _i32(three[2]))


def test_overflow_in_the_middle_of_a_driven_run_gives_the_bits_of_an_ample_buffer():
    """the recipe of tests/test_gpu_water_drive.py at 86 molecules: every molecule translates towards the centre of the box, a
    capacity that holds the first edge list but not a later one; the run freezes, gamd_sync_status regrows and resumes"""
    from gamd_amd.engine import GamdForce
    case = _Water(n_mol=86)
    steps = 30
    xm, _ = _minimised_start()
    o = np.repeat(xm[0::3].astype(np.float64), 3, axis=0)
    v0 = (-(o - case.box / 2) * 6.0).astype(np.float32)
    probe = GamdForce(case.sd, case.n, case.box, case.rc, **case.eng_kw)
    probe.forward(torch.from_numpy(xm).cuda(), species=case.species)
    e_now = probe.counts()[0]
    probe.close()
    md = {**case.md, "temperature_k": 0.0}
    res = []
    for cap in (0, e_now + 60):
        eng = GamdForce(case.sd, case.n, case.box, case.rc, edge_capacity=cap, **case.eng_kw)
        eng.forward(torch.from_numpy(xm).cuda(), species=case.species)
        assert eng.last_status == 0
        eng, x, _, f = _start(case, eng=eng)
        v = torch.from_numpy(v0).cuda()
        eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
        eng.md_run(x, v, f, steps, gamma_per_ps=0.0, seed=1, sync=False, **md)
        status = eng.sync_status()
        assert status == (1 if cap else 0), "the run was meant to outgrow its edge buffer"
        tr = eng.traj_read()
        if cap:
            _assert_frames_carry_the_classical_force(eng, tr, x, f, case.species, steps)
        res.append((_state(x, v, f), tr))
        eng.close()
    (sa, ta), (sb, tb) = res
    for a, b in zip(sa, sb):
        assert np.array_equal(_i32(a), _i32(b))
    assert ta.dropped == tb.dropped == 0 and np.array_equal(ta.steps, np.arange(1, steps + 1)) and np.array_equal(tb.steps, ta.steps)
    for name in ("x", "v", "f"):
        assert np.array_equal(_i32(getattr(ta, name)), _i32(getattr(tb, name))), name
    assert np.isfinite(sa[2]).all() and not np.array_equal(sa[0], xm)


# ---- 7: refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    from gamd_amd._lib import GamdError, check
    lj = _Case("lj")
    eng, x, v, f = lj.make()
    assert eng._lib.gamd_water_msite(eng._h, W) == -22 and b"GAMD_KIND_LJ" in eng._lib.gamd_last_error()
    eng.close()
    case = _Water(n_mol=86)
    eng, x, v, f = case.make()
    assert eng._lib.gamd_water_msite(eng._h, W) == -22 and b"gamd_water_configure" in eng._lib.gamd_last_error()   # before configure
    for bad in (-0.1, 0.5, 0.75, float("nan"), float("inf")):
        with pytest.raises(GamdError, match="-22.*w_h"):
            _conf(eng, m_site=bad)
    _conf(eng, m_site=0.0)                                                     # the refused weights left 0 in force
    xm = x.clone()
    m = eng.water_minimize(xm, case.species, tolerance=1e3, max_iter=2)
    assert m.status in (0, 1)
    _conf(eng)
    x1 = x.clone()
    with pytest.raises(GamdError, match="-22.*M-site"):
        eng.water_minimize(x1, case.species, tolerance=1e3, max_iter=2)
    assert torch.equal(x1, x)                                                  # nothing was enqueued
    _conf(eng, interval=4)
    case.run(eng, x, v, f, 4, sync=False)
    assert eng._lib.gamd_water_msite(eng._h, 0.0) == -22 and b"enqueued" in eng._lib.gamd_last_error()          # a run is pending
    assert eng.sync_status() == 0
    rd = eng.water_classical_read(forces=True)
    assert np.array_equal(rd.steps, [4])
    _check_box("after the refusals", _rows(rd)[0], x.cpu().numpy(), case.box, case.species, _water(), W, 0.0, rd.forces, f.cpu().numpy())
    check(eng._lib.gamd_water_msite(eng._h, 0.0), "gamd_water_msite")
    eng.close()


# ---- 8: checked build ------------------------------------------------------------------------------------------------
CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_water_msite as t
from gamd_amd import _lib
print("RESULT", json.dumps(dict(version=_lib.load().gamd_version().decode(), **t._checked_payload())))
"""


def _checked_payload():
    """a sampled skin-mode run (rows and the last sample's forces) and a driven run (final x, v, f) at 86 molecules"""
    case = _Water("nhc", skin=SKIN, n_mol=86)
    _, rd, _ = _sampled_run(case, 2)
    rows = np.stack([getattr(rd, name) for name in rd.COLUMNS], axis=-1)
    (x, v, f), _ = _driven(case, [4])
    return dict(steps=rd.steps.tolist(), dropped=rd.dropped, rows=_bits(rows).tolist(), forces=_bits(rd.forces).tolist(),
                driven=[_i32(a).tolist() for a in (x, v, f)])


def test_checked_build_gives_the_same_rows_and_forces():
    """under libgamd_hip_chk.so in a fresh child process (nothing preloaded): a failed device-side range check of any kernel of
    the runs would come back as -35; the 4-site kernels index with nothing they read from memory and give the same bits"""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    env = {k: v for k, v in os.environ.items() if k not in ("GAMD_LIB", "GAMD_CHK_INJECT")}
    env["GAMD_LIB"] = CHK
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert p.returncode == 0 and "RESULT" in p.stdout, (p.stdout[-800:], p.stderr[-1500:])
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got.pop("version").endswith("checked")
    mine = _checked_payload()
    assert got["steps"] == mine["steps"] == [4, 8] and got["dropped"] == 0
    assert got == mine
