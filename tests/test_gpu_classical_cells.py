"""The Lennard-Jones classical potential over a cell table on the device (gamd_classical_cells, gamd_amd/csrc/classical_cells.hip):
classical_configure(cells=True) on given positions.  Runs and the minimiser: tests/test_gpu_classical_cells_runs.py.

What is asserted
* Exact: the pair count equals the all-pairs path's and the reference's; the table (nc, start, order) read back equals the numpy
  restatement water_cells_ref.table on the same doubles.
* Bounded: the bounds tests/test_gpu_classical.py derives for the all-pairs path (N eps against 1e-12; the cell walk adds an
  atom's terms in another order, no more of them), against tests/classical_ref.py, as that file's _check_box applies them: |E - E_ref| <=
  1e-12 sum |u|, |W - W_ref| <= 1e-12 sum |r u'|, every force component within 1e-12 sum_j |F_ij|.  _check_box prints the
  observed fraction of every bound.  Periodic images are judged against their OWN reference: bit equality across images is not
  promised (an image may fall into the neighbouring cell at a face).
  The fourth bound, the five force-error sums of an observer's row within 1e-12 of their absolute terms, needs a run's forces:
  tests/test_gpu_classical_cells_runs.py asserts it through this file's _check_box on sampled, network-driven runs.
* Bit equality: a second call, a fresh handle, each box of a two-box handle against that box alone.
* Off is untouched: a handle toggled on and off again gives the bits of a handle that never had cells.
* The refusals name their reason and leave the handle usable.
* One builder, one table (gamd_amd/csrc/cell_table.hip): an LJ handle and a water handle given the same positions hold equal
  tables, both the numpy restatement's.

The shapes are those of tests/classical_cells_cases.py; tests/test_classical_cells_host.py checks on the CPU that each is well
posed (no pair within 1e-12 r_cut of the cutoff, 2 r_cut <= the shortest edge) and has the cells per axis it is meant to have."""
import ctypes as C

import numpy as np
import pytest
import torch

import classical_cells_cases as cc
import classical_ref as cr
import water_cells_ref as cf
from gamd_amd import workloads as wl
from test_gpu_classical import _bits, _engine, TOL
from test_gpu_report import _Case

pytestmark = pytest.mark.gpu


def _check_box(tag, row, x_box, box, lj, length_per_nm, fcl_dev, f_run=None):
    """tests/test_gpu_classical.py's _check_box — the same reference and the same bounds — with the force bound compared as
    |df| <= TOL sum_j |F_ij| instead of through their quotient: at r_cut = 4 A most atoms have no partner, and 0 <= 0 holds where
    0 / 0 is not a number.  With f_run (the run's forces on the frame, row [9] an observer's row): the five force-error sums within
    TOL of the sums of their absolute terms and the left-out count, recomputed on the host (classical_ref.force_error_sums) from
    the device's f_cl and f_run, as there.  Prints the largest observed fraction of every bound."""
    ref = cr.evaluate(x_box, box, lj, length_per_nm)
    e_err, w_err = abs(row[0] - ref["energy"]), abs(row[1] - ref["virial"])
    f_err, f_bound = np.abs(fcl_dev - ref["forces"]), TOL * ref["abs_f"][:, None] * np.ones((1, 3))
    some = f_bound > 0
    print(f"{tag}: pairs {row[2]:.0f} (ref {ref['pairs']:.0f}, {ref['near']} at the cutoff), E {row[0]:.9e} |dE| / bound "
          f"{e_err / (TOL * ref['abs_u']):.3e}, W {row[1]:.9e} |dW| / bound {w_err / (TOL * ref['abs_ru']):.3e}, max |df| / bound "
          f"{(f_err[some] / f_bound[some]).max():.3e}, {int((~some[:, 0]).sum())} atoms without a partner")
    assert ref["near"] == 0, "ill-posed: a pair sits on the cutoff"
    assert ref["pairs"] > 0 and row[2] == ref["pairs"]
    assert e_err <= TOL * ref["abs_u"] and w_err <= TOL * ref["abs_ru"]
    assert (f_err <= f_bound).all() and np.isfinite(fcl_dev).all()
    if f_run is not None:
        sums, ab = cr.force_error_sums(f_run, fcl_dev)
        ratio = np.abs(row[3:8] - sums[:5]) / (TOL * ab)
        print(f"{tag}: force-error sums {row[3:8]}, |dev - host| / bound {ratio}, left out of the cosine {row[8]:.0f}")
        assert (ab > 0).all() and (ratio <= 1.0).all() and row[8] == sums[5]
    return ref


def _eval(eng, x, box, **kw):
    f, e, w, c = eng.classical_forces(x, box=box, **kw)
    return f.cpu().numpy(), e, w, c


def _same(a, b):
    return all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a, b))


def _assert_table(eng, x_box, box, r_cut, b=0):
    nc, start, order = eng.classical_cells_table(b)
    rn, rs, ro = cf.table(np.asarray(x_box, dtype=np.float32).astype(np.float64), box, r_cut)
    assert np.array_equal(nc, rn) and np.array_equal(start, rs) and np.array_equal(order, ro)
    return tuple(int(v) for v in nc)


# ---- 1: given positions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.CASES))
def test_pairs_and_table_are_exact_and_energy_virial_and_forces_stay_inside_the_all_pairs_bounds(name):
    x, box, lj, want = cc.build(name)
    n = len(x)
    eng = _engine(n, box, cutoff=5.0 if n == 64 else 7.5)
    eng.classical_configure(0, cells=True, **lj.kwargs())
    on = _eval(eng, x, box)
    ref = _check_box(f"cells {name}", np.array([on[1][0], on[2][0], on[3][0]]), x, box, lj, 0.0, on[0])
    assert _assert_table(eng, x, box, lj.r_cut) == want
    assert _same(on, _eval(eng, x, box)), "second call"
    # the all-pairs path on the same handle: the same pairs, and the same values inside the same bounds
    eng.classical_configure(0, **lj.kwargs())
    off = _eval(eng, x, box)
    assert off[3][0] == on[3][0] == ref["pairs"]
    assert abs(off[1][0] - on[1][0]) <= 2e-12 * ref["abs_u"] and (np.abs(off[0] - on[0]) <= 2e-12 * ref["abs_f"][:, None]).all()
    eng.close()
    fresh = _engine(n, box, cutoff=5.0 if n == 64 else 7.5)
    fresh.classical_configure(0, cells=True, **lj.kwargs())
    assert _same(on, _eval(fresh, x, box)), "fresh handle"
    fresh.close()


@pytest.mark.parametrize("second,ncs", [((1.0, 1.05, 0.97), [(5, 5, 5), (5, 5, 5)]),     # test_two_boxes_with_different_positions_in_bohr's boxes
                                        ((1.0, 1.1, 1.25), [(5, 5, 5), (5, 6, 7)])])      # ... and two with different cells per axis
def test_two_boxes_in_bohr_have_their_own_cells_and_each_is_that_box_alone(second, ncs):
    n = 300
    pos, L = wl.lj_box(n, seed=4)
    rng = np.random.default_rng(8)
    x = np.concatenate([pos, np.mod(pos + rng.normal(0, 0.4, pos.shape), L)]).astype(np.float32)
    boxes = np.array([[L, L, L], [L * second[0], L * second[1], L * second[2]]], dtype=np.float32)
    lj = cr.LJ()
    eng = _engine(n, float(L), n_boxes=2)
    eng.classical_configure(0, cells=True, **lj.kwargs())
    f, e, w, c = _eval(eng, x, boxes, length_per_nm=wl.BOHR_PER_NM)
    for b in range(2):
        sl = slice(b * n, (b + 1) * n)
        _check_box(f"cells box {b}", np.array([e[b], w[b], c[b]]), x[sl], boxes[b], lj, wl.BOHR_PER_NM, f[sl])
        assert _assert_table(eng, x[sl], boxes[b], lj.r_cut, b) == ncs[b]
    assert c[0] != c[1]
    eng.close()
    for b in range(2):
        sl = slice(b * n, (b + 1) * n)
        one = _engine(n, boxes[b])
        one.classical_configure(0, cells=True, **lj.kwargs())
        f1, e1, w1, c1 = _eval(one, x[sl], boxes[b], length_per_nm=wl.BOHR_PER_NM)
        assert _same((f1, e1, w1, c1), (f[sl], e[b:b + 1], w[b:b + 1], c[b:b + 1])), f"box {b}"
        one.close()


# ---- 2: off is untouched ---------------------------------------------------------------------------------------------
def test_a_handle_toggled_on_and_off_gives_the_bits_of_a_handle_that_never_had_cells():
    x, box, lj, _ = cc.build("300")
    n = len(x)
    x0 = np.mod(x, box)
    v0 = wl.maxwell_boltzmann(n, 100.0, seed=91).astype(np.float32)
    md = dict(dt_ps=0.002, mass_amu=39.9, temperature_k=100.0, box=box, gamma_per_ps=25.0, seed=11)

    def everything(eng):
        out = list(_eval(eng, x, box))
        xm = torch.from_numpy(x0).cuda()
        res = eng.minimize(xm, box=box, tolerance=1e-300, max_iter=8, return_x64=True)
        out += [res.rows, res.x64.cpu().numpy(), xm.cpu().numpy(), res.f.cpu().numpy()]
        eng.md_force_source("classical")
        eng.classical_configure(2, **lj.kwargs())
        xr, vr = torch.from_numpy(x0).cuda(), torch.from_numpy(v0).cuda()
        fr = eng.classical_forces(xr, box=box)[0].float().contiguous()
        eng.md_run(xr, vr, fr, 6, **md)
        rd = eng.classical_read(forces=True)
        out += [xr.cpu().numpy(), vr.cpu().numpy(), fr.cpu().numpy(), rd.forces] + [getattr(rd, name) for name in rd.COLUMNS]
        return out

    never = _engine(n, box)
    never.classical_configure(0, **lj.kwargs())
    want = everything(never)
    never.close()
    eng = _engine(n, box)
    eng.classical_configure(0, cells=True, **lj.kwargs())
    on = _eval(eng, x, box)
    eng.classical_configure(0, cells=False, **lj.kwargs())
    got = everything(eng)
    eng.close()
    assert len(got) == len(want) and _same(got, want)
    assert not np.array_equal(_bits(on[0]), _bits(want[0]))                 # (the cells did run: another order of the sums)


# ---- 3: refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_handle_usable():
    from gamd_amd._lib import GamdError, load
    lib = load()
    err = lambda: lib.gamd_last_error()
    water = _Case("water")
    eng, x, v, f = water.make()
    assert lib.gamd_classical_cells(eng._h, 1) == -22 and b"GAMD_KIND_WATER" in err() and b"gamd_water_cells" in err()
    eng.close()
    xs, box, lj, _ = cc.build("300")
    eng = _engine(len(xs), box)
    assert lib.gamd_classical_cells(eng._h, 1) == -22 and b"gamd_classical_configure" in err()      # no parameters yet
    nc = (C.c_int32 * 3)()
    eng.classical_configure(0, **lj.kwargs())
    assert lib.gamd_classical_cells_read(eng._h, None, 0, nc, None, 0, None, 0) == -22 and b"off" in err()
    for on in (2, -1):
        assert lib.gamd_classical_cells(eng._h, on) == -22 and b"not 0" in err()
    eng.classical_configure(0, cells=True, **lj.kwargs())
    with pytest.raises(GamdError, match="-22.*nothing has been sampled"):
        eng.classical_cells_table()
    # a pending run
    x = torch.from_numpy(np.mod(xs, box)).cuda()
    v = torch.from_numpy(wl.maxwell_boltzmann(len(xs), 100.0, seed=91)).float().cuda()
    f = eng.forward(x, box=box, denormalize=True).clone()
    eng.md_run(x, v, f, 2, dt_ps=0.002, mass_amu=39.9, temperature_k=100.0, box=box, gamma_per_ps=25.0, seed=11, sync=False)
    assert lib.gamd_classical_cells(eng._h, 0) == -22 and b"enqueued" in err()
    with pytest.raises(GamdError, match="-22.*enqueued"):
        eng.classical_configure(0, cells=False, **lj.kwargs())
    assert eng.sync_status() == 0
    # the switch is still on, and the handle evaluates inside the bounds
    fc, e, w, c = _eval(eng, xs, box)
    _check_box("after the refusals", np.array([e[0], w[0], c[0]]), xs, box, lj, 0.0, fc)
    _assert_table(eng, xs, box, lj.r_cut)
    with pytest.raises(GamdError, match="-22.*box = 1"):
        eng.classical_cells_table(1)
    # the read call describes the table the device holds: that of the last evaluation, whatever was configured since
    eng.classical_configure(0, cells=True, r_cut=6.0, r_switch=4.0)
    _assert_table(eng, xs, box, lj.r_cut)
    _eval(eng, xs, box)
    assert _assert_table(eng, xs, box, 6.0) == (9, 8, 10)
    eng.close()


# ---- 4: one builder, one table -----------------------------------------------------------------------------------------
def _shared_positions(box, seed):
    """192 fp32 positions in the box `box`: a third moved by -3 .. +3 box edges, and 40 coordinates put ON faces of the cells of
    both cutoffs below (the fp32 edge times i / nc, rounded to fp32), zero and the edge itself among them"""
    rng = np.random.default_rng(seed)
    b = box.astype(np.float64)
    x = rng.uniform(0.0, 1.0, (192, 3)) * b[None, :]
    x[::3] += rng.integers(-3, 4, size=(64, 3)) * b[None, :]
    for k, i in enumerate(rng.choice(192, 40, replace=False)):
        d, rc = k % 3, (6.8, 3.0)[(k // 3) % 2]
        nc = int(cf.ncells(box, rc)[d])
        x[i, d] = b[d] * ((k // 6) % (nc + 1)) / nc + (b[d] if k >= 30 else 0.0)
    return x.astype(np.float32)


@pytest.mark.parametrize("n_boxes", [1, 2])
def test_the_lj_and_the_water_handle_build_the_same_table_from_the_same_positions_and_it_is_numpy_s(n_boxes):
    """cell_table.hip serves both potentials: an LJ handle of 192 atoms and a water handle of 64 molecules, given the same 192
    fp32 positions per box, hold equal tables, both the numpy restatement's, with no allowance.  r_cut = 6.8: (4, 5, 6) cells, one
    axis below five, the scan walks one cell per thread; r_cut = 3.0: (10, 11, 14) = 1540 cells, every axis wraps, seven cells per
    thread, most of them empty.  The second box of the two-box handles has other edges (and other cells per axis).  Only the
    tables are judged: the positions are no molecules, and the water handle's reciprocal sum is cut short (k_cut) because
    nothing of it is read."""
    from test_gpu_water_classical import _engine as _water_engine
    import water_classical_ref as wr
    boxes = np.array([[15.1, 17.5, 21.2], [16.4, 13.7, 19.3]], dtype=np.float32)[:n_boxes]
    want = {6.8: [(4, 5, 6), (4, 4, 5)], 3.0: [(10, 11, 14), (10, 9, 12)]}
    x = np.concatenate([_shared_positions(boxes[b], 21 + b) for b in range(n_boxes)])
    hb = boxes if n_boxes > 1 else boxes[0]
    lj = _engine(192, hb[0] if n_boxes > 1 else hb, n_boxes=n_boxes, cutoff=6.5)
    wat, species = _water_engine(64, hb[0] if n_boxes > 1 else hb, n_boxes=n_boxes)
    for r_cut in (6.8, 3.0):
        assert (2.0 * r_cut <= boxes).all()
        lj.classical_configure(0, cells=True, r_cut=r_cut, r_switch=0.8 * r_cut)
        lj.classical_forces(x, box=hb)
        wat.water_classical_configure(0, cells=True, **wr.Water(r_cut=r_cut, k_cut=2.0).kwargs())
        wat.water_classical_forces(x, species, box=hb)
        for b in range(n_boxes):
            xb = x[192 * b:192 * (b + 1)]
            ref = cf.table(xb.astype(np.float64), boxes[b], r_cut)
            tl, tw = lj.classical_cells_table(b), wat.water_cells_table(b)
            assert tuple(int(v) for v in ref[0]) == want[r_cut][b]
            for name, r, a, w in zip(("nc", "start", "order"), ref, tl, tw):
                assert np.array_equal(a, w) and np.array_equal(a, r), (r_cut, b, name)
            print(f"r_cut {r_cut} box {b}: nc {want[r_cut][b]}, {int((np.diff(ref[1]) == 0).sum())} of {len(ref[1]) - 1} cells empty, "
                  f"occupancy up to {int(np.diff(ref[1]).max())}")
    lj.close()
    wat.close()
