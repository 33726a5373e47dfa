"""The real-space pairs of the water classical potential over a cell table on the device (gamd_water_cells,
gamd_amd/csrc/water_cells.hip): given positions, the observer inside enqueued runs and the water classical force source, for the
3-site form and the M-site form (TIP4P-Ew's weight), with the plain reciprocal sum and with particle-mesh Ewald, against the
float64 host references (tests/water_classical_ref.py, water_msite_ref.py, water_pme_ref.py) and against the all-pairs path.

Shapes (tests/test_water_cells_host.py CASES, shown there to keep every pair inside the cutoff within two cells; the
configurations of tests/test_water_pme_host.py, atoms in several periodic images, some three box lengths away, molecules torn):

    86 molecules, box 13.66 x 14.2 x 15.1   r_cut 6.8   nc (4, 4, 4)    every cell of every axis is visited
    86 molecules, same box                  r_cut 4.2   nc (6, 6, 7)    the wrap, unequal axes, an odd count (also in bohr)
    86 molecules, same box                  r_cut 3.0   nc (9, 9, 10)   600 of 810 cells empty
    258 molecules, cubic box of 20          r_cut 6.8   nc (5, 5, 5)    exactly 2 R + 1: offsets -2 .. +2 are all the cells
    258 molecules, same box                 r_cut 4.5   nc (8, 8, 8)    the wrap; 13 workgroups of 64 slots and a tail of 6
    258 molecules, same box                 r_cut 9.5   nc (4, 4, 4)    occupancy up to 21

ewald_tol 1e-8 throughout; PME at order 6 on 16 x 32 x 8 (86 molecules) and 32^3 (258).

Exact: the pair count and the charge sum are the all-pairs path's, U_recip and U_self its bits, the table is the numpy
restatement's (tests/water_cells_ref.py).  Bounds, the ones tests/test_gpu_water_classical.py, test_gpu_water_msite.py and
test_gpu_water_pme.py apply to the all-pairs path: U_LJ and U_real + U_excl within 1e-12 of the sums of their absolute terms,
every force component within 1e-12 abs_f of the reference in force.  The device and the references differ in the order of the
sums and in erfc / erf / exp.  Everything else is bit equality — except across periodic images, which is not promised (an image
may sit in the neighbouring cell at a face)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import water_cells_ref as cf
import water_classical_ref as wr
import water_msite_ref as w4
import water_pme_ref as pr
import water_virial_ref as vr
import test_water_pme_host as ph
import test_water_cells_host as ch
import test_gpu_water_virial as tv
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
WORST = {}                              # the largest observed fraction of each bound (printed; profiles/run_water_cells.md)
GRID = {86: (16, 32, 8), 258: (32, 32, 32)}
CASES = [c[:3] + (0.0,) for c in ch.CASES] + [(86, False, 4.2, wl.BOHR_PER_NM)]
IDS = [f"{c[0]}-rc{c[2]}-{'bohr' if c[3] else 'A'}" for c in CASES]


def _wat(r_cut, msite, unit=1.0):
    if msite:
        return wr.Water(q_h=ph.Q_H4, sigma_o=ph.SIGMA4 * unit, epsilon_o=ph.EPS4, r_cut=r_cut * unit, ewald_tol=ph.DELTA)
    return wr.Water(r_cut=r_cut * unit, sigma_o=3.15075 * unit, ewald_tol=ph.DELTA)


def _conf(eng, interval=0, msite=False, pme=None, cells=True, r_cut=ph.RC, unit=1.0, length_per_nm=0.0, **kw):
    eng.water_classical_configure(interval, m_site=W if msite else 0.0, pme=pme, pme_order=6, cells=cells, length_per_nm=length_per_nm,
                                  **{**_wat(r_cut, msite, unit).kwargs(), **kw})


@functools.lru_cache(maxsize=None)
def _reference(n_mol, cubic, r_cut, length_per_nm, msite, pme):
    """the float64 reference of one configuration (computed once, shared, never modified)"""
    x, box, species, unit = ph.configuration(n_mol, cubic, length_per_nm)
    wat = _wat(r_cut, msite, unit)
    if pme:
        return pr.evaluate(x, box, species, wat, GRID[n_mol], 6, W if msite else None, length_per_nm)
    return w4.evaluate(x, box, species, wat, W, length_per_nm) if msite else wr.evaluate(x, box, species, wat, length_per_nm)


def _check(tag, row, f_dev, ref):
    abs_f = ref["abs_f"] if ref["abs_f"].ndim == 2 else ref["abs_f"][:, None]
    fr = dict(lj=abs(row[0] - ref["u_lj"]) / (TOL * ref["abs_lj"]), coul=abs(row[1] - ref["u_coul"]) / (TOL * ref["abs_real"]),
              force=(np.abs(f_dev - ref["forces"]) / (TOL * abs_f)).max())
    print(f"{tag}: pairs {row[4]:.0f} (ref {ref['pairs']:.0f}), U_LJ {row[0]:.12e} U_coul {row[1]:.12e}; |dev - ref| / bound: "
          + ", ".join(f"{k} {v:.3e}" for k, v in fr.items()))
    for k, v in fr.items():
        WORST[k] = max(WORST.get(k, 0.0), float(v))
    assert ref["near"] == 0 and ref.get("near_lj", 0) == 0, "ill-posed: a pair sits on a cutoff"
    assert np.isfinite(f_dev).all() and np.isfinite(row).all()
    assert row[4] == ref["pairs"] and ref["pairs"] > 0 and row[11] == 0.0 and ref["abs_lj"] > 0
    assert all(v <= 1.0 for v in fr.values())


def _assert_table(eng, x64, box, r_cut, b=0):
    nc, start, order = eng.water_cells_table(b)
    rnc, rstart, rorder = cf.table(x64, box, r_cut)
    assert np.array_equal(nc, rnc) and np.array_equal(start, rstart) and np.array_equal(order, rorder)
    return tuple(int(v) for v in nc)


# ---- 1: against the references, the all-pairs path and the numpy table ----------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_energies_and_forces_are_the_references_pairs_and_the_other_columns_the_all_pairs_path_s_and_the_table_numpy_s(case):
    n_mol, cubic, r_cut, length_per_nm = case
    x, box, species, unit = ph.configuration(n_mol, cubic, length_per_nm)
    eng, sp = _engine(n_mol, float(box) if cubic else box)
    assert np.array_equal(sp, species)
    hb = None if cubic else box                                                 # (the handle's own)
    for msite in (False, True):
        xw = cf.charge_sites(x.astype(np.float64), box, W) if msite else x.astype(np.float64)
        for pme in (None, GRID[n_mol]):
            kw = dict(msite=msite, pme=pme, r_cut=r_cut, unit=unit, length_per_nm=length_per_nm)
            _conf(eng, cells=False, **kw)
            f0, r0 = eng.water_classical_forces(x, species, box=hb, length_per_nm=length_per_nm)
            _conf(eng, cells=True, **kw)
            f, rd = eng.water_classical_forces(x, species, box=hb, length_per_nm=length_per_nm)
            row, off = _rows(rd)[0], _rows(r0)[0]
            tag = f"{n_mol} molecules r_cut {r_cut} {'M-site' if msite else '3-site'} {'PME' if pme else 'plain'} len {length_per_nm}"
            _check(tag, row, f.cpu().numpy(), _reference(n_mol, cubic, r_cut, length_per_nm, msite, bool(pme)))
            assert row[4] == off[4] and _bits(row[11]) == _bits(off[11])        # pairs, sum q
            assert _bits(row[2]) == _bits(off[2]) and _bits(row[3]) == _bits(off[3])        # U_recip, U_self
            assert (row[5:11] == 0.0).all()
            nc = _assert_table(eng, xw * 1.0, box, r_cut * unit)
            if not length_per_nm:
                assert nc == ch.CASES[CASES.index(case)][3]
            d = np.abs(f.cpu().numpy() - f0.cpu().numpy()).max()
            print(f"{tag}: nc {nc}; largest |f_cells - f_all_pairs| {d:.3e} kJ/mol/nm")
    eng.close()


# ---- 2: atoms on cell faces, and a lattice whose distances tie on the cutoff ------------------------------------------------
@pytest.mark.parametrize("r_cut,nc", [(6.8, 5), (4.5, 8)])
def test_atoms_on_cell_faces_at_zero_and_at_the_edge_fall_into_the_numpy_table_s_cells(r_cut, nc):
    x, box, species, _ = ph.configuration(258, True, 0.0)
    assert float(box) == 20.0
    face = (np.float32(20.0) * np.arange(nc + 1, dtype=np.float32) / np.float32(nc)).astype(np.float32)     # exact: 4 i, 2.5 i; 0 and L
    assert np.array_equal(face.astype(np.float64), 20.0 * np.arange(nc + 1) / nc)
    x = x.copy()
    hyd = np.flatnonzero(species == 0)[:6 * (nc + 1)]                            # hydrogens only: no Lennard-Jones core is moved
    for k, i in enumerate(hyd):
        x[i, k % 3] = face[(k // 3) % (nc + 1)] + np.float32(20.0) * np.float32((k // (3 * (nc + 1))) * -1)     # in the box, and one image below
    eng, _ = _engine(258, 20.0)
    for msite in (False, True):
        _conf(eng, msite=msite, cells=False, r_cut=r_cut)
        _, r0 = eng.water_classical_forces(x, species)
        _conf(eng, msite=msite, cells=True, r_cut=r_cut)
        f, rd = eng.water_classical_forces(x, species)
        xw = cf.charge_sites(x.astype(np.float64), box, W) if msite else x.astype(np.float64)
        assert _assert_table(eng, xw, box, r_cut) == (nc, nc, nc)
        cell = cf.cell_axis(x[hyd[:3 * (nc + 1)], 0].astype(np.float64)[0::3], 20.0, nc) if not msite else None
        if cell is not None:
            assert np.array_equal(cell, np.r_[np.arange(nc), 0])                # x = 0 and x = L are cell 0, face i is cell i
        assert _rows(rd)[0][4] == _rows(r0)[0][4] > 0 and torch.isfinite(f).all()
    eng.close()


@pytest.mark.parametrize("n_mol,r_cut", [(86, 6.8), (86, 4.2), (258, 4.5)])
def test_on_a_lattice_whose_distances_tie_at_the_cutoff_the_pair_count_is_the_all_pairs_path_s(n_mol, r_cut):
    pos, L, species, _ = wl.water_box(n_mol, seed=5, jitter=0, wrap=False)
    x = pos.astype(np.float32)
    eng, _ = _engine(n_mol, float(L))
    assert 2 * r_cut <= L
    for msite in (False, True):
        _conf(eng, msite=msite, cells=False, r_cut=r_cut)
        _, r0 = eng.water_classical_forces(x, species)
        _conf(eng, msite=msite, cells=True, r_cut=r_cut)
        _, rd = eng.water_classical_forces(x, species)
        print(f"lattice of {n_mol} molecules, r_cut {r_cut}, {'M-site' if msite else '3-site'}: pairs {_rows(rd)[0][4]:.0f}")
        assert _rows(rd)[0][4] == _rows(r0)[0][4] > 0
        xw = cf.charge_sites(x.astype(np.float64), np.float32(L), W) if msite else x.astype(np.float64)
        _assert_table(eng, xw, np.float32(L), r_cut)
    eng.close()


# ---- 3: the same bits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("msite,pme,r_cut", [(False, (16, 32, 8), 4.2), (True, (16, 16, 16), 6.8), (False, None, 4.2)])
def test_a_repeated_call_a_fresh_handle_and_each_box_of_two_give_the_same_bits(msite, pme, r_cut):
    """with PME every bit; with the plain sum the handle's common k-vector list is longer than the shorter box's own (tests/
    test_gpu_water_classical.py: the surplus carries weight zero but changes the order of the reciprocal sums), so there the real-space
    columns are the same bits and the forces agree within the references' bound"""
    x0, box0, species, _ = ph.configuration(86, False, 0.0)
    scale = np.array([1.0, 0.985, 0.99])
    box1 = (box0 * scale).astype(np.float32)                                    # 13.66 x 13.99 x 14.95: nc (6, 6, 7) and (4, 4, 4) again
    pos7, L7, _, _ = wl.water_box(86, seed=7, jitter=0.02, wrap=False)
    x1 = ph.images(ph.move(pos7, L7, box1.astype(np.float64)), box1, 4)
    x, boxes = np.concatenate([x0, x1]), np.stack([box0, box1])
    eng, _ = _engine(86, float(box0[0]), n_boxes=2)
    _conf(eng, msite=msite, pme=pme, r_cut=r_cut)
    f, rd = eng.water_classical_forces(x, species, box=boxes)
    f2, rd2 = eng.water_classical_forces(x, species, box=boxes)                 # the tables are cleared at the head of every sample
    fh, rows = f.cpu().numpy(), _rows(rd)
    assert np.array_equal(_bits(fh), _bits(f2.cpu().numpy())) and np.array_equal(_bits(rows), _bits(_rows(rd2)))
    assert rows[0][1] != rows[1][1]
    tables = [eng.water_cells_table(b) for b in range(2)]
    for b, (xb, bb) in enumerate(((x0, box0), (x1, box1))):
        xw = cf.charge_sites(xb.astype(np.float64), bb, W) if msite else xb.astype(np.float64)
        _assert_table(eng, xw, bb, r_cut, b)
        for fresh in range(2):                                                  # the box alone, on two fresh handles
            one, _ = _engine(86, bb)
            _conf(one, msite=msite, pme=pme, r_cut=r_cut)
            f1, r1 = one.water_classical_forces(xb, species, box=bb)
            if pme:
                assert np.array_equal(_bits(f1.cpu().numpy()), _bits(fh[b * 258:(b + 1) * 258])), (b, fresh)
                assert np.array_equal(_bits(_rows(r1)[0]), _bits(rows[b])), (b, fresh)
            else:
                assert np.array_equal(_bits(_rows(r1)[0][[0, 1, 3, 4, 11]]), _bits(rows[b][[0, 1, 3, 4, 11]])), (b, fresh)
                ref = wr.evaluate(xb, bb, species, _wat(r_cut, msite))
                assert (np.abs(f1.cpu().numpy() - fh[b * 258:(b + 1) * 258]) <= TOL * ref["abs_f"][:, None]).all(), (b, fresh)
            for got, want in zip(one.water_cells_table(0), tables[b]):
                assert np.array_equal(got, want)
            one.close()
    eng.close()


def _start(case, msite, pme, r_cut, eng=None, cells=True):
    """the documented recipe: the lattice minimised with the cells off (once, tests/test_gpu_water_msite.py), the cells switched
    on, f = fp32(water_classical_forces(x))"""
    xm, vm = _minimised_start()
    if eng is None:
        eng, _, _, _ = case.make()
    x, v = torch.from_numpy(xm).cuda(), torch.from_numpy(vm).cuda()
    _conf(eng, msite=msite, pme=pme, r_cut=r_cut, cells=cells)
    eng.md_force_source("water_classical")
    f = eng.water_classical_forces(x, case.species)[0].float().contiguous()
    return eng, x, v, f


def _driven(case, calls, msite=False, pme=None, r_cut=4.2, observers=False, cells=True):
    eng, x, v, f = _start(case, msite, pme, r_cut, cells=cells)
    if observers:
        eng.report_configure(2, **case.report_kw())
        _conf(eng, interval=2, msite=msite, pme=pme, r_cut=r_cut, cells=cells)
    chain = None
    for c, k in enumerate(calls):
        chain = case.run(eng, x, v, f, k, first_step=sum(calls[:c]), chain=chain)
        assert eng.last_status == 0
    out = _state(x, v, f)
    rd = eng.water_classical_read(forces=True) if observers else None
    eng.close()
    return out, rd


@pytest.mark.parametrize("integrator,skin,msite,pme,r_cut", [("baoab", 0.0, False, None, 4.2), ("nhc", SKIN, True, (16, 32, 8), 6.8)])
def test_chunked_runs_fresh_handles_and_an_armed_observer_give_the_same_bits(integrator, skin, msite, pme, r_cut):
    K = 4
    case = _Water(integrator, skin=skin, n_mol=86, K=K)
    one, _ = _driven(case, [2 * K], msite, pme, r_cut)
    two, _ = _driven(case, [K, K], msite, pme, r_cut)
    again, _ = _driven(case, [2 * K], msite, pme, r_cut)
    armed, rd = _driven(case, [2 * K], msite, pme, r_cut, observers=True)
    assert np.array_equal(rd.steps, 2 * np.arange(1, 5)) and (rd.pairs > 0).all() and (rd.sum_q == 0.0).all()
    # f = RN_fp32(f_cl): the observer's error sums of a driven step are those of one rounding
    assert (rd.sum_abs[:, 0] > 0).all() and (rd.sum_abs[:, 0] <= 2.0 ** -24 * np.sqrt(3.0) * rd.sum_norm_cl[:, 0] * (1.0 + 1e-12)).all()
    assert np.array_equal(_i32(armed[2]), _i32(rd.forces.astype(np.float32)))     # the last sample is the last step's force
    for name, other in (("two calls", two), ("second handle", again), ("observer armed", armed)):
        for a, b in zip(one, other):
            assert np.array_equal(_i32(a), _i32(b)), name


def test_overflow_in_the_middle_of_a_driven_run_gives_the_bits_of_an_ample_buffer():
    """the recipe of tests/test_gpu_water_msite.py: every molecule translates towards the centre of the box, a capacity that
    holds the first edge list but not a later one; the run freezes (every cell kernel returns, the tables are cleared again when
    the step is evaluated again), gamd_sync_status regrows and resumes"""
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
        eng, x, _, f = _start(case, False, None, 4.2, eng=eng)
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


# ---- 4: driven runs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator,msite,pme,r_cut", [("baoab", False, None, 4.2), ("nhc", True, (16, 32, 8), 4.2),
                                                        ("nhc", False, (16, 16, 16), 6.8), ("baoab", True, None, 6.8)])
def test_every_frame_of_a_driven_skin_mode_run_carries_the_cells_force_of_its_positions(integrator, msite, pme, r_cut):
    case = _Water(integrator, skin=SKIN, n_mol=86)
    eng, x, v, f = _start(case, msite, pme, r_cut)
    steps = 6
    eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
    case.run(eng, x, v, f, steps)
    assert eng.last_status == 0
    _assert_frames_carry_the_classical_force(eng, eng.traj_read(), x, f, case.species, steps)
    eng.close()


# ---- 5: the virial log with the cells on -------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0.0, tv.W4], ids=["3site", "4site"])
def test_the_virial_rows_stay_within_the_reference_s_bound_with_the_cells_on(w):
    shape = "ortho"
    x, vel, species = tv._config(tv.BOXES[shape])
    box = tv.BOXES[shape].astype(np.float32)
    wat = tv._water()
    eng, _ = _engine(86, box)
    eng.water_classical_configure(0, m_site=w, cells=True, **wat.kwargs())
    rc = eng.water_classical_virial(x, species, vel, box=box, mass_o_amu=tv.MASS_O, mass_h_amu=tv.MASS_H)
    ref = vr.virial(x, box, species, wat, w, vel, tv.MASS_O, tv.MASS_H, 0.0)
    tv._check_row(f"cells on, {shape} w {w}", tv._vrows(rc)[0], ref)
    # the observer's own row of the same call is gamd_water_eval's with the cells on
    f, rd = eng.water_classical_forces(x, species, box=box)
    assert np.array_equal(_bits(_rows(rd)), _bits(_rows(rc)))
    # ... and armed in a run the log takes its rows behind the cells' f_cl
    eng.close()
    case = _Water("nhc", skin=SKIN, n_mol=86)
    eng, xs, v, f = _start(case, w != 0.0, None, 6.8)
    eng.water_classical_configure(2, m_site=w, cells=True, virial=True, **_wat(6.8, w != 0.0).kwargs())
    eng.traj_configure(2, max_frames=2, fields=("x", "v"))
    case.run(eng, xs, v, f, 4)
    assert eng.last_status == 0
    rd, tr = eng.water_classical_read(), eng.traj_read()
    assert np.array_equal(rd.steps, [2, 4])
    for q in range(2):
        ref = vr.virial(tr.x[q].reshape(-1, 3), np.float32(case.box), case.species, _wat(6.8, w != 0.0), w, tr.v[q].reshape(-1, 3),
                        tv.MASS_O, tv.MASS_H, 0.0)
        tv._check_row(f"cells on, run sample {q} w {w}", tv._vrows(rd, q)[0], ref)
    eng.close()


# ---- 6: off is off -----------------------------------------------------------------------------------------------------
def test_switching_the_cells_off_restores_the_bits_of_a_handle_that_never_had_them():
    from gamd_amd._lib import GamdWaterParams
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

    eng, _, _, _ = case.make()                                                  # gamd_water_configure alone: the switch never touched
    assert eng._lib.gamd_water_configure(eng._h, C.byref(p)) == 0
    never = run(eng)
    eng.close()
    eng, _, _, _ = case.make()
    assert eng._lib.gamd_water_configure(eng._h, C.byref(p)) == 0
    eng._water_set = True                                                       # (the package: the parameters are the C call's)
    assert eng._lib.gamd_water_cells(eng._h, 1) == 0
    on, r_on = eng.water_classical_forces(torch.from_numpy(xm).cuda(), case.species)
    assert eng._lib.gamd_water_configure(eng._h, C.byref(p)) == 0               # sticky across the C configure call ...
    on2, _ = eng.water_classical_forces(torch.from_numpy(xm).cuda(), case.species)
    assert np.array_equal(_bits(on.cpu().numpy()), _bits(on2.cpu().numpy()))
    assert eng._lib.gamd_water_cells(eng._h, 0) == 0                            # ... until it is switched off
    assert eng._lib.gamd_water_cells_read(eng._h, None, 0, (C.c_int32 * 3)(), None, 0, None, 0) == -22
    after = run(eng)
    eng.close()
    assert not np.array_equal(never[0], _bits(on.cpu().numpy()))                # another order of the sums
    assert _rows(r_on)[0][4] == never[1].view(np.float64)[0][4]
    for a, b in zip(never, after):
        assert np.array_equal(a, b)


# ---- 7: refusals -------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_handle_usable():
    from gamd_amd._lib import GamdError
    cells = lambda e, on: e._lib.gamd_water_cells(e._h, on)
    err = lambda e: e._lib.gamd_last_error()
    read = lambda e, b=0: e._lib.gamd_water_cells_read(e._h, None, b, (C.c_int32 * 3)(), None, 0, None, 0)
    lj = _Case("lj")
    eng, _, _, _ = lj.make()
    assert cells(eng, 1) == -22 and b"GAMD_KIND_LJ" in err(eng)
    eng.close()
    case = _Water(n_mol=86)
    eng, x, v, f = case.make()
    assert cells(eng, 1) == -22 and b"gamd_water_configure" in err(eng)                                # before configure
    _conf(eng, cells=False)
    for on in (2, -1, 7):
        assert cells(eng, on) == -22 and b"not 0" in err(eng)
    assert read(eng) == -22 and b"off" in err(eng)
    assert cells(eng, 1) == 0
    assert read(eng) == -22 and b"nothing has been sampled" in err(eng)
    # the minimiser's f is the all-pairs force
    x1 = x.clone()
    with pytest.raises(GamdError, match="-22.*cell table.*cells off"):
        eng.water_minimize(x1, case.species, tolerance=1e3, max_iter=2)
    assert torch.equal(x1, x)                                                   # nothing was enqueued
    # a pending run
    _conf(eng, interval=4, cells=True)
    eng.md_force_source("water_classical")
    f = eng.water_classical_forces(x, case.species)[0].float().contiguous()
    case.run(eng, x, v, f, 4, sync=False)
    assert cells(eng, 0) == -22 and b"enqueued" in err(eng)
    assert eng.sync_status() == 0
    assert read(eng) == 0 and read(eng, 1) == -22 and b"outside" in err(eng)
    rd = eng.water_classical_read(forces=True)
    assert np.array_equal(rd.steps, [4])
    # the handle is as usable as before: the sample of the run is the potential on its frame, the table that frame's
    f2, r2 = eng.water_classical_forces(x, case.species)
    assert np.array_equal(_bits(f2.cpu().numpy()), _bits(rd.forces)) and np.array_equal(_bits(_rows(r2)[0][:5]), _bits(_rows(rd)[0][:5]))
    _assert_table(eng, x.cpu().numpy().astype(np.float64), np.float32(case.box), ph.RC)
    ref = wr.evaluate(x.cpu().numpy(), np.float32(case.box), case.species, ph.water3())
    _check("after the refusals", _rows(r2)[0], f2.cpu().numpy(), ref)
    eng.close()


# ---- 8: checked build --------------------------------------------------------------------------------------------------
CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_water_cells as t
from gamd_amd import _lib
print("RESULT", json.dumps(dict(version=_lib.load().gamd_version().decode(), **t._checked_payload())))
"""


def _checked_payload():
    """given positions in several images (both site models, plain and PME, nc (6, 6, 7)) with their tables, and a driven
    skin-mode run with the observer armed (rows, the last sample's forces, final x, v, f) at 86 molecules"""
    x, box, species, _ = ph.configuration(86, False, 0.0)
    eng, _ = _engine(86, box)
    evals = []
    for msite, pme in ((False, None), (True, (16, 32, 8))):
        _conf(eng, msite=msite, pme=pme, r_cut=4.2)
        f, rd = eng.water_classical_forces(x, species, box=box)
        evals.append([_bits(f.cpu().numpy()).tolist(), _bits(_rows(rd)).tolist(), [a.tolist() for a in eng.water_cells_table(0)]])
    eng.close()
    case = _Water("nhc", skin=SKIN, n_mol=86)
    (xs, vs, fs), rd = _driven(case, [4], msite=True, pme=None, r_cut=4.2, observers=True)
    rows = np.stack([getattr(rd, name) for name in rd.COLUMNS], axis=-1)
    return dict(evals=evals, steps=rd.steps.tolist(), dropped=rd.dropped, rows=_bits(rows).tolist(), forces=_bits(rd.forces).tolist(),
                driven=[_i32(a).tolist() for a in (xs, vs, fs)])


def test_checked_build_gives_the_same_rows_forces_and_tables():
    """under libgamd_hip_chk.so in a fresh child process (nothing preloaded): a failed device-side range check of any kernel of
    the runs — an atom's cell, a cell's start, a slot, a table entry's atom — would come back as -35"""
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
