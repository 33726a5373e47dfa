"""Smooth particle-mesh Ewald in the water classical potential on the device (gamd_water_pme, gamd_amd/csrc/water_pme.hip):
given positions, the observer inside enqueued runs and the water classical force source, for the 3-site form and the M-site
form (TIP4P-Ew's weight), against the float64 host reference of tests/water_pme_ref.py.

Shapes (tests/test_water_pme_host.py CASES, whose references are shared and whose bounds are shown there not to be vacuous): 86
molecules in the box 13.66 x 14.2 x 15.1 with the grids 16^3 and 16 x 32 x 8 (a line of 8 points with order 6: the stencil
wraps over most of the axis; three different line lengths), in Angstrom and in bohr; 258 molecules (three full 256-atom tiles
and a tail) with 32^3; and 86 molecules with 8 x 64 x 128, so that every line length runs.  r_cut 6.8, ewald_tol 1e-8, both
orders.  The atoms sit in several periodic images, some three box lengths away, some negative, molecules torn.

Bounds, as the issue sets them: U_recip within 1e-12 abs_recip and every force component within 1e-12 abs_f, with
abs_recip = (C / 2 pi V) sum |G| (sum |q|)^2 and abs_f = |q_i| (n_d / L_d) sum |theta' theta theta| (C / pi V) sum |G| sum |q|
from the reference alone; the row's other columns, the pair count and the charge sum are the plain path's bit for bit.  The
device and the reference differ in the order of the transform's additions, in exp, and in the order of the pair sums.
Everything else is bit equality.  No test feeds a non-finite position (tools/pme_host_check.cpp covers that on the host)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import water_classical_ref as wr
import water_msite_ref as w4
import water_pme_ref as pr
import test_water_pme_host as ph
from gamd_amd import workloads as wl
from test_gpu_classical_drive import _i32
from test_gpu_report import _Case, _state
from test_gpu_water_classical import _Water, _engine, _bits, _rows
from test_gpu_water_drive import _assert_frames_carry_the_classical_force, SKIN
from test_gpu_water_msite import _minimised_start

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHK = os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")
W = w4.TIP4PEW_W
TOL = 1e-12
WORST = {}                              # the largest observed fraction of each bound (printed; profiles/run_water_pme.md)
PLAIN_COLUMNS = [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11]          # every column of the row but U_recip


def _conf(eng, interval=0, msite=False, pme=(16, 32, 8), order=6, unit=1.0, length_per_nm=0.0, **kw):
    wat = ph.water4(unit) if msite else ph.water3(unit)
    eng.water_classical_configure(interval, m_site=W if msite else 0.0, pme=pme, pme_order=order, length_per_nm=length_per_nm,
                                  **{**wat.kwargs(), **kw})


def _check(tag, row, f_dev, ref):
    fr = dict(recip=abs(row[2] - ref["u_recip"]) / (TOL * ref["abs_recip"]), force=(np.abs(f_dev - ref["forces"]) / (TOL * ref["abs_f"])).max())
    print(f"{tag}: U_recip {row[2]:.12e} (ref {ref['u_recip']:.12e}); |dev - ref| / bound: recip {fr['recip']:.3e}, force {fr['force']:.3e}")
    for k, v in fr.items():
        WORST[k] = max(WORST.get(k, 0.0), float(v))
    assert np.isfinite(f_dev).all() and np.isfinite(row).all()
    assert fr["recip"] <= 1.0 and fr["force"] <= 1.0
    assert row[4] == ref["pairs"] and row[11] == 0.0 and ref["near"] == 0


# ---- 1: against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ph.CASES, ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[2]))}-{'bohr' if c[3] else 'A'}")
def test_energy_and_forces_are_the_reference_s_and_the_other_columns_the_plain_path_s(case):
    n_mol, cubic, grid, length_per_nm = case
    x, box, species, unit = ph.configuration(n_mol, cubic, length_per_nm)
    eng, sp = _engine(n_mol, float(box) if cubic else box)
    assert np.array_equal(sp, species)
    box = None if cubic else box                                                # (the handle's own)
    for msite in (False, True):
        _conf(eng, msite=msite, pme=None, unit=unit, length_per_nm=length_per_nm)
        _, r0 = eng.water_classical_forces(x, species, box=box, length_per_nm=length_per_nm)
        for order in (4, 6):
            _conf(eng, msite=msite, pme=grid, order=order, unit=unit, length_per_nm=length_per_nm)
            f, rd = eng.water_classical_forces(x, species, box=box, length_per_nm=length_per_nm)
            row = _rows(rd)[0]
            _check(f"{n_mol} molecules {grid} order {order} {'M-site' if msite else '3-site'} len {length_per_nm}", row, f.cpu().numpy(),
                   ph.reference(n_mol, cubic, grid, length_per_nm, order, msite))
            assert np.array_equal(_bits(row[PLAIN_COLUMNS]), _bits(_rows(r0)[0][PLAIN_COLUMNS]))
            assert row[2] != _rows(r0)[0][2]
    eng.close()


# ---- 2: the same bits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msite,order,grid", [(False, 6, (16, 32, 8)), (True, 4, (16, 16, 16))])
def test_a_repeated_call_a_fresh_handle_and_each_box_of_two_give_the_same_bits(msite, order, grid):
    x0, box0, species, _ = ph.configuration(86, False, 0.0)
    scale = np.array([1.0, 0.985, 0.99])
    box1 = (box0 * scale).astype(np.float32)
    pos7, L7, _, _ = wl.water_box(86, seed=7, jitter=0.02, wrap=False)
    x1 = ph.images(ph.move(pos7, L7, box1.astype(np.float64)), box1, 4)
    x, boxes = np.concatenate([x0, x1]), np.stack([box0, box1])
    eng, _ = _engine(86, float(box0[0]), n_boxes=2)
    _conf(eng, msite=msite, pme=grid, order=order)
    f, rd = eng.water_classical_forces(x, species, box=boxes)
    f2, rd2 = eng.water_classical_forces(x, species, box=boxes)                 # the grid is cleared at the head of every sample
    fh, rows = f.cpu().numpy(), _rows(rd)
    assert np.array_equal(_bits(fh), _bits(f2.cpu().numpy())) and np.array_equal(_bits(rows), _bits(_rows(rd2)))
    assert rows[0][2] != rows[1][2]
    _check("box 0 of two", rows[0], fh[:258], ph.reference(86, False, grid, 0.0, order, msite))
    for b, (xb, bb) in enumerate(((x0, box0), (x1, box1))):
        for fresh in range(2):                                                  # the box alone, on two fresh handles
            one, _ = _engine(86, bb)
            _conf(one, msite=msite, pme=grid, order=order)
            f1, r1 = one.water_classical_forces(xb, species, box=bb)
            assert np.array_equal(_bits(f1.cpu().numpy()), _bits(fh[b * 258:(b + 1) * 258])), (b, fresh)
            assert np.array_equal(_bits(_rows(r1)[0]), _bits(rows[b])), (b, fresh)
            one.close()
    eng.close()


def _start(case, msite, pme, order, eng=None):
    """the documented recipe: the lattice minimised under the plain sum (once, tests/test_gpu_water_msite.py), PME switched on,
    f = fp32(water_classical_forces(x))"""
    xm, vm = _minimised_start()
    if eng is None:
        eng, _, _, _ = case.make()
    x, v = torch.from_numpy(xm).cuda(), torch.from_numpy(vm).cuda()
    _conf(eng, msite=msite, pme=pme, order=order)
    eng.md_force_source("water_classical")
    f = eng.water_classical_forces(x, case.species)[0].float().contiguous()
    return eng, x, v, f


def _driven(case, calls, msite=False, pme=(16, 32, 8), order=6, observers=False):
    eng, x, v, f = _start(case, msite, pme, order)
    if observers:
        eng.report_configure(2, **case.report_kw())
        _conf(eng, interval=2, msite=msite, pme=pme, order=order)
    chain = None
    for c, k in enumerate(calls):
        chain = case.run(eng, x, v, f, k, first_step=sum(calls[:c]), chain=chain)
        assert eng.last_status == 0
    out = _state(x, v, f)
    rd = eng.water_classical_read(forces=True) if observers else None
    eng.close()
    return out, rd


@pytest.mark.parametrize("integrator,skin,msite,order", [("baoab", 0.0, False, 6), ("nhc", SKIN, True, 4)])
def test_chunked_runs_fresh_handles_and_an_armed_observer_give_the_same_bits(integrator, skin, msite, order):
    K = 4
    case = _Water(integrator, skin=skin, n_mol=86, K=K)
    one, _ = _driven(case, [2 * K], msite, order=order)
    two, _ = _driven(case, [K, K], msite, order=order)
    again, _ = _driven(case, [2 * K], msite, order=order)
    armed, rd = _driven(case, [2 * K], msite, order=order, observers=True)
    plain, _ = _driven(case, [2 * K], msite, pme=None)
    assert np.array_equal(rd.steps, 2 * np.arange(1, 5)) and (rd.pairs > 0).all() and (rd.sum_q == 0.0).all()
    # f = RN_fp32(f_cl): the observer's error sums of a driven step are those of one rounding
    assert (rd.sum_abs[:, 0] > 0).all() and (rd.sum_abs[:, 0] <= 2.0 ** -24 * np.sqrt(3.0) * rd.sum_norm_cl[:, 0] * (1.0 + 1e-12)).all()
    assert np.array_equal(_i32(armed[2]), _i32(rd.forces.astype(np.float32)))     # the last sample is the last step's force
    for name, other in (("two calls", two), ("second handle", again), ("observer armed", armed)):
        for a, b in zip(one, other):
            assert np.array_equal(_i32(a), _i32(b)), name
    assert not np.array_equal(_i32(one[0]), _i32(plain[0])) and not np.array_equal(_i32(one[2]), _i32(plain[2]))    # another potential


def test_overflow_in_the_middle_of_a_driven_run_gives_the_bits_of_an_ample_buffer():
    """the recipe of tests/test_gpu_water_msite.py: every molecule translates towards the centre of the box, a capacity that
    holds the first edge list but not a later one; the run freezes (every PME kernel returns, the grid is cleared again when the
    step is evaluated again), gamd_sync_status regrows and resumes"""
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
        eng, x, _, f = _start(case, False, (16, 32, 8), 6, eng=eng)
        v = torch.from_numpy(v0).cuda()
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
    assert np.isfinite(sa[2]).all() and not np.array_equal(sa[0], xm)


# ---- 3: driven runs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator,msite,order,grid", [("baoab", False, 6, (16, 32, 8)), ("nhc", True, 6, (16, 16, 16)),
                                                         ("nhc", False, 4, (16, 16, 16)), ("baoab", True, 4, (16, 32, 8))])
def test_every_frame_of_a_driven_skin_mode_run_carries_the_pme_force_of_its_positions(integrator, msite, order, grid):
    case = _Water(integrator, skin=SKIN, n_mol=86)
    eng, x, v, f = _start(case, msite, grid, order)
    steps = 6
    eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
    case.run(eng, x, v, f, steps)
    assert eng.last_status == 0
    _assert_frames_carry_the_classical_force(eng, eng.traj_read(), x, f, case.species, steps)
    eng.close()


# ---- 4: off is off -----------------------------------------------------------------------------------------------------
def test_order_zero_restores_the_bits_of_a_handle_that_never_had_pme():
    from gamd_amd._lib import GamdWaterParams, GamdWaterPmeParams
    case = _Water("nhc", skin=SKIN, n_mol=86)
    wat = ph.water3()
    xm, vm = _minimised_start()
    p = GamdWaterParams(0, 0, wat.q_h, wat.lj.sigma, wat.lj.epsilon, wat.r_cut, 0.0, 0, 0, wat.alpha, wat.k_cut, wat.coulomb_const)

    def run(eng):
        eng._water_set = True
        eng.md_force_source("water_classical")
        x, v = torch.from_numpy(xm).cuda(), torch.from_numpy(vm).cuda()
        f64, rd = eng.water_classical_forces(x, case.species)
        f = f64.float().contiguous()
        eng.traj_configure(1, max_frames=4, fields=("x", "f"))
        case.run(eng, x, v, f, 4)
        tr = eng.traj_read()
        return _bits(f64.cpu().numpy()), _bits(_rows(rd)), _i32(tr.x), _i32(tr.f), *[_i32(a) for a in _state(x, v, f)]

    eng, _, _, _ = case.make()                                                  # gamd_water_configure alone: PME never called
    assert eng._lib.gamd_water_configure(eng._h, C.byref(p)) == 0
    never = run(eng)
    eng.close()
    eng, _, _, _ = case.make()
    _conf(eng, pme=(16, 32, 8), order=6)
    on, _ = eng.water_classical_forces(torch.from_numpy(xm).cuda(), case.species)
    assert eng._lib.gamd_water_configure(eng._h, C.byref(p)) == 0               # sticky across the C configure call ...
    on2, _ = eng.water_classical_forces(torch.from_numpy(xm).cuda(), case.species)
    assert np.array_equal(_bits(on.cpu().numpy()), _bits(on2.cpu().numpy()))
    off = GamdWaterPmeParams(0, 0, 0, 0)                                        # ... until order 0
    assert eng._lib.gamd_water_pme(eng._h, C.byref(off)) == 0
    after = run(eng)
    eng.close()
    assert not np.array_equal(never[0], _bits(on.cpu().numpy()))
    for a, b in zip(never, after):
        assert np.array_equal(a, b)


# ---- 5: the limit is lifted --------------------------------------------------------------------------------------------
def test_a_k_cut_the_plain_sum_refuses_is_served_with_pme_on():
    from gamd_amd._lib import GamdError
    x, box, species, _ = ph.configuration(86, False, 0.0)
    eng, _ = _engine(86, box)
    with pytest.raises(GamdError, match="-22.*k_cut"):                          # about 1.7e5 triples
        _conf(eng, pme=None, k_cut=20.0)
        eng.water_classical_forces(x, species, box=box)
    _conf(eng, pme=(16, 32, 8), order=6, k_cut=20.0)
    f, rd = eng.water_classical_forces(x, species, box=box)
    _check("k_cut 20", _rows(rd)[0], f.cpu().numpy(), ph.reference(86, False, (16, 32, 8), 0.0, 6, False))
    eng.close()
    # ... and so is a tolerance whose OWN k_cut (2 alpha sqrt(-ln tol) = 16.9 / A) the plain sum refuses, on a handle that
    # never had PME: the parameters are accepted in front of gamd_water_pme whatever k_cut they carry
    tight = dict(ewald_tol=1e-25, alpha=None, k_cut=None)
    eng, _ = _engine(86, box)
    with pytest.raises(GamdError, match="-22.*k_cut"):
        _conf(eng, pme=None, **tight)
        eng.water_classical_forces(x, species, box=box)
    _conf(eng, pme=(16, 32, 8), order=6, **tight)
    f, rd = eng.water_classical_forces(x, species, box=box)
    wat = wr.Water(r_cut=ph.RC, ewald_tol=1e-25)
    _check("ewald_tol 1e-25", _rows(rd)[0], f.cpu().numpy(), pr.evaluate(x, box, species, wat, (16, 32, 8), 6))
    eng.close()


# ---- 6: refusals -------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_handle_usable():
    from gamd_amd._lib import GamdError, GamdWaterPmeParams
    pme = lambda e, *a: e._lib.gamd_water_pme(e._h, C.byref(GamdWaterPmeParams(*a)))
    err = lambda e: e._lib.gamd_last_error()
    lj = _Case("lj")
    eng, _, _, _ = lj.make()
    assert pme(eng, 6, 16, 16, 16) == -22 and b"GAMD_KIND_LJ" in err(eng)
    eng.close()
    case = _Water(n_mol=86)
    eng, x, v, f = case.make()
    assert eng._lib.gamd_water_pme(eng._h, None) == -22 and b"null" in err(eng)
    assert pme(eng, 6, 16, 16, 16) == -22 and b"gamd_water_configure" in err(eng)                      # before configure
    _conf(eng, pme=None)
    for order in (1, 2, 3, 5, 7, 8, -4):
        assert pme(eng, order, 16, 16, 16) == -22 and b"order" in err(eng)
    for grid in ((12, 16, 16), (16, 256, 16), (16, 16, 0), (4, 16, 16), (16, -8, 16), (16, 16, 100)):
        assert pme(eng, 6, *grid) == -22 and b"grid length" in err(eng)
    for kw in (dict(pme=12), dict(pme=(16, 16)), dict(pme=(16, 16, 24)), dict(pme=16, pme_order=5), dict(pme=16, virial=True)):
        with pytest.raises(ValueError):
            eng.water_classical_configure(0, **kw)
    # the virial log and the minimiser are not built for PME
    assert eng._lib.gamd_water_virial(eng._h, 1) == 0
    assert pme(eng, 6, 16, 16, 16) == -22 and b"virial" in err(eng) and b"PME" in err(eng)
    assert eng._lib.gamd_water_virial(eng._h, 0) == 0
    _conf(eng, pme=(16, 32, 8), order=6)
    assert eng._lib.gamd_water_virial(eng._h, 1) == -22 and b"PME" in err(eng)
    with pytest.raises(GamdError, match="-22.*PME"):
        eng.water_classical_virial(x, case.species)
    x1 = x.clone()
    with pytest.raises(GamdError, match="-22.*PME"):
        eng.water_minimize(x1, case.species, tolerance=1e3, max_iter=2)
    assert torch.equal(x1, x)                                                   # nothing was enqueued
    # a pending run
    _conf(eng, interval=4, pme=(16, 32, 8), order=6)
    case.run(eng, x, v, f, 4, sync=False)
    assert pme(eng, 0, 0, 0, 0) == -22 and b"enqueued" in err(eng)
    assert eng.sync_status() == 0
    rd = eng.water_classical_read(forces=True)
    assert np.array_equal(rd.steps, [4])
    # the handle is as usable as before: the sample of the run is the potential on its frame
    f2, r2 = eng.water_classical_forces(x, case.species)
    assert np.array_equal(_bits(f2.cpu().numpy()), _bits(rd.forces)) and _rows(r2)[0][2] == _rows(rd)[0][2]
    ref = pr.evaluate(x.cpu().numpy(), case.box, case.species, ph.water3(), (16, 32, 8), 6)
    _check("after the refusals", _rows(r2)[0], f2.cpu().numpy(), ref)
    eng.close()


# ---- 7: checked build --------------------------------------------------------------------------------------------------
CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_water_pme as t
from gamd_amd import _lib
print("RESULT", json.dumps(dict(version=_lib.load().gamd_version().decode(), **t._checked_payload())))
"""


def _checked_payload():
    """given positions in several images (both orders, both site models, three line lengths) and a driven skin-mode run with the
    observer armed (rows, the last sample's forces, final x, v, f) at 86 molecules"""
    x, box, species, _ = ph.configuration(86, False, 0.0)
    eng, _ = _engine(86, box)
    evals = []
    for msite, order in ((False, 6), (True, 4)):
        _conf(eng, msite=msite, pme=(16, 32, 8), order=order)
        f, rd = eng.water_classical_forces(x, species, box=box)
        evals.append([_bits(f.cpu().numpy()).tolist(), _bits(_rows(rd)).tolist()])
    eng.close()
    case = _Water("nhc", skin=SKIN, n_mol=86)
    (xs, vs, fs), rd = _driven(case, [4], msite=True, order=6, observers=True)
    rows = np.stack([getattr(rd, name) for name in rd.COLUMNS], axis=-1)
    return dict(evals=evals, steps=rd.steps.tolist(), dropped=rd.dropped, rows=_bits(rows).tolist(), forces=_bits(rd.forces).tolist(),
                driven=[_i32(a).tolist() for a in (xs, vs, fs)])


def test_checked_build_gives_the_same_rows_and_forces():
    """under libgamd_hip_chk.so in a fresh child process (nothing preloaded): a failed device-side range check of any kernel of
    the runs would come back as -35; the PME kernels form their grid addresses by gamd_pme_index / gamd_pme_wrap and give the
    same bits"""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    env = {k: v for k, v in os.environ.items() if k not in ("GAMD_LIB", "GAMD_CHK_INJECT")}
    env["GAMD_LIB"] = CHK
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert p.returncode == 0 and "RESULT" in p.stdout, (p.stdout[-800:], p.stderr[-1500:])
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got.pop("version").endswith("checked")
    mine = _checked_payload()
    assert got["steps"] == mine["steps"] == [2, 4] and got["dropped"] == 0
    assert got == mine


def test_print_the_largest_observed_fractions_of_the_bounds():
    print("largest |dev - ref| / bound over this session:", {k: f"{v:.3e}" for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())
