"""Molecular virial of the water classical potential on the device (gamd_water_virial, gamd_amd/csrc/water_virial.hip) against
the float64 reference tests/water_virial_ref.py.  86 molecules are 258 atoms: two row tiles (molecule 85 straddles the 256-atom
boundary) and 32 pair slices of 9 atoms, which split molecules.

Tolerances: every column of a row (W_LJ, W_coul,pair, W_recip, W_intra, KE_com, W_mol) is within 1e-12 of the reference's sum of
the absolute terms of that column — the project's standing bound for sums of this kind in double.  The Coulomb identity
W_coul,pair + W_recip = U_coul on device rows at ewald_tol = 1e-12 is held to 3e-12 of the absolute terms: 1e-12 of rounding on
either side plus the truncation the host test measures (below 1e-13 there).  Everything else is bit for bit."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import water_classical_ref as wr
import water_virial_ref as vr
from gamd_amd import workloads as wl
from test_gpu_report import _Case, _state, _f32
from test_gpu_water_classical import _Water, _engine, _bits, _rows, DELTA

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHK = os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")
TOL = 1e-12
W4 = 0.106676721
BOXES = {"cubic": np.array([13.75, 13.75, 13.75]), "ortho": np.array([13.75, 15.0, 16.25])}
MASS_O, MASS_H = float(_f32(wl.MASS_O)), float(_f32(wl.MASS_H))          # the fp32 values a run holds
POT = dict(r_cut=6.8, r_switch=5.8)


def _config(box, seed=5, grid=0.0, unit=1.0):
    """86 jittered molecules moved rigidly into `box` (whole molecules), fp32 velocities of a few length units per ps"""
    pos, b0, species, _ = wl.water_box(86, seed=seed, jitter=0.02, wrap=False)
    x, _ = vr.scaled(pos, b0, np.asarray(box, dtype=np.float64) / float(np.float32(b0)))
    if grid:
        x = np.rint(x / grid) * grid
    vel = np.random.default_rng(seed + 40).normal(0.0, 4.0, x.shape)
    return (x * unit).astype(np.float32), (vel * unit).astype(np.float32), species


def _vrows(rc, q=0):
    return np.stack([rc.virial_terms[c][q] for c in ("w_lj", "w_coul", "w_recip", "w_intra")] + [rc.ke_com[q], rc.virial[q]], axis=-1)


def _water(unit=1.0, tol=DELTA):
    return wr.Water(sigma_o=3.15075 * unit, r_cut=POT["r_cut"] * unit, r_switch=POT["r_switch"] * unit, ewald_tol=tol)


def _check_row(tag, row, ref):
    fr = {c: abs(row[k] - ref[c]) / (TOL * ref["abs_" + c]) for k, c in enumerate(vr.COLUMNS) if ref["abs_" + c] > 0.0}
    print(f"{tag}: " + ", ".join(f"{c} {row[k]:.9e}" for k, c in enumerate(vr.COLUMNS)) + "; |dev - ref| / (1e-12 abs terms): "
          + ", ".join(f"{c} {v:.3e}" for c, v in fr.items()))
    assert ref["ev"]["near"] == 0 and ref["ev"]["near_lj"] == 0, "ill-posed: a pair sits on the cutoff"
    assert all(ref["abs_" + c] > 0.0 for c in vr.COLUMNS[:4]) and np.isfinite(row).all()
    assert all(v <= 1.0 for v in fr.values()), fr
    if ref["abs_ke_com"] == 0.0:
        assert row[4] == 0.0


# ---- 1: given positions against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("length_per_nm", [0.0, wl.BOHR_PER_NM], ids=["angstrom", "bohr"])
@pytest.mark.parametrize("w", [0.0, W4], ids=["3site", "4site"])
@pytest.mark.parametrize("shape", ["cubic", "ortho"])
def test_every_column_is_the_reference_on_given_positions_and_velocities(shape, w, length_per_nm):
    unit = float(_f32(length_per_nm)) / 10.0 if length_per_nm else 1.0
    x, vel, species = _config(BOXES[shape], unit=unit)
    box = (BOXES[shape] * unit).astype(np.float32)
    wat = _water(unit)
    assert 2 * wat.r_cut <= box.min()
    eng, _ = _engine(86, box)
    eng.water_classical_configure(0, m_site=w, **wat.kwargs())
    rc = eng.water_classical_virial(x, species, vel, box=box, length_per_nm=length_per_nm, mass_o_amu=MASS_O, mass_h_amu=MASS_H)
    ref = vr.virial(x, box, species, wat, w, vel, MASS_O, MASS_H, length_per_nm)
    _check_row(f"{shape} w {w} len {length_per_nm}", _vrows(rc)[0], ref)
    assert rc.ke_com[0, 0] > 0.0 and rc.virial.shape == (1, 1)
    # the observer's own row of the same call is gamd_water_eval's, and without velocities KE_com is 0
    f, rd = eng.water_classical_forces(x, species, box=box, length_per_nm=length_per_nm)
    assert np.array_equal(_bits(_rows(rd)), _bits(_rows(rc)))
    still = eng.water_classical_virial(x, species, None, box=box, length_per_nm=length_per_nm, mass_o_amu=MASS_O, mass_h_amu=MASS_H)
    assert still.ke_com[0, 0] == 0.0 and np.array_equal(_bits(_vrows(still)[0, :4]), _bits(_vrows(rc)[0, :4]))
    vol = float(np.prod(box.astype(np.float64) / (10.0 * unit)))
    from gamd_amd.engine import BAR_PER_KJ_MOL_NM3
    assert rc.pressure(None, vol)[0, 0] == BAR_PER_KJ_MOL_NM3 * (2.0 * rc.ke_com[0, 0] + rc.virial[0, 0]) / (3.0 * vol)
    eng.close()


# ---- 2: the same bits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0.0, W4], ids=["3site", "4site"])
def test_images_boxes_of_a_batch_repeated_calls_and_fresh_handles_give_the_same_bits(w):
    """Positions on a grid of 2^-10 A in the (13.75, 15.0, 16.25) box: x + k L is exact in fp32, so every minimum-image vector
    and every wrapped coordinate is the same double for every image; atom-wise shifts tear the molecules across images.  The
    two boxes of the batch have the same edges (the k-vector list, and with it the tree of the k sums, goes by the longest edge
    of a handle's boxes) and different positions and velocities."""
    box = BOXES["ortho"].astype(np.float32)
    xa, va, species = _config(BOXES["ortho"], seed=5, grid=2.0 ** -10)
    xb, vb, _ = _config(BOXES["ortho"], seed=7, grid=2.0 ** -10)
    k = np.random.default_rng(3).integers(-2, 3, size=xa.shape)
    xs = (xa.astype(np.float64) + k * BOXES["ortho"]).astype(np.float32)
    assert np.array_equal(xs.astype(np.float64), xa.astype(np.float64) + k * BOXES["ortho"]) and (k != 0).any()
    kw = dict(mass_o_amu=MASS_O, mass_h_amu=MASS_H)

    def handle(n_boxes=1):
        eng, _ = _engine(86, box, n_boxes=n_boxes)
        eng.water_classical_configure(0, m_site=w, ewald_tol=DELTA, **POT)
        return eng
    eng = handle()
    a = _vrows(eng.water_classical_virial(xa, species, va, box=box, **kw))
    shifted = _vrows(eng.water_classical_virial(xs, species, va, box=box, **kw))
    b = _vrows(eng.water_classical_virial(xb, species, vb, box=box, **kw))
    again = _vrows(eng.water_classical_virial(xa, species, va, box=box, **kw))
    eng.close()
    fresh = handle()
    c = _vrows(fresh.water_classical_virial(xa, species, va, box=box, **kw))
    fresh.close()
    two = handle(2)
    both = _vrows(two.water_classical_virial(np.concatenate([xa, xb]), species, np.concatenate([va, vb]), box=np.stack([box, box]), **kw))
    two.close()
    assert a.shape == (1, 6) and both.shape == (2, 6) and not np.array_equal(a, b)
    for name, other in (("image shifts", shifted), ("second call", again), ("fresh handle", c), ("box 0 of two", both[0:1])):
        assert np.array_equal(_bits(a), _bits(other)), (name, a, other)
    assert np.array_equal(_bits(b), _bits(both[1:2]))


def test_two_boxes_with_different_edges_against_the_boxes_alone():
    """The cubic and the (13.75, 15.0, 16.25) box in one handle: the k-vector list is built for the longest edge, so the cubic
    box alone has a shorter list of its own and adds its k sums in another tree — as U_recip does in the observer's row.  The
    pair terms and KE_com have the same bits; W_recip, W_intra (through the reciprocal part of f_cl) and W_mol agree within
    1e-12 of the reference's absolute terms."""
    kw = dict(mass_o_amu=MASS_O, mass_h_amu=MASS_H)
    cfg = [_config(BOXES[s], seed=sd) for s, sd in (("cubic", 5), ("ortho", 7))]
    boxes = np.stack([BOXES["cubic"], BOXES["ortho"]]).astype(np.float32)
    species = cfg[0][2]
    two, _ = _engine(86, boxes[1], n_boxes=2)
    two.water_classical_configure(0, m_site=W4, ewald_tol=DELTA, **POT)
    both = _vrows(two.water_classical_virial(np.concatenate([c[0] for c in cfg]), species, np.concatenate([c[1] for c in cfg]), box=boxes, **kw))
    two.close()
    for b in range(2):
        one, _ = _engine(86, boxes[b])
        one.water_classical_configure(0, m_site=W4, ewald_tol=DELTA, **POT)
        alone = _vrows(one.water_classical_virial(cfg[b][0], species, cfg[b][1], box=boxes[b], **kw))[0]
        one.close()
        ref = vr.virial(cfg[b][0], boxes[b], species, _water(), W4, cfg[b][1], MASS_O, MASS_H)
        _check_row(f"box {b} of two", both[b], ref)
        for k in (0, 1, 4):
            assert _bits(alone[k:k + 1])[0] == _bits(both[b, k:k + 1])[0], (b, vr.COLUMNS[k])
        for k in (2, 3, 5):
            assert abs(alone[k] - both[b, k]) <= TOL * ref["abs_" + vr.COLUMNS[k]], (b, vr.COLUMNS[k])
    assert both[0, 2] != both[1, 2]


# ---- 3: the Coulomb identity on device rows --------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0.0, W4], ids=["3site", "4site"])
def test_coulomb_virial_equals_the_coulomb_energy_on_the_device(w):
    box = BOXES["cubic"].astype(np.float32)
    x, _, species = _config(BOXES["cubic"])
    wat = _water(tol=1e-12)
    eng, _ = _engine(86, box)
    eng.water_classical_configure(0, m_site=w, **wat.kwargs())
    rc = eng.water_classical_virial(x, species, None, box=box)
    eng.close()
    ref = vr.virial(x, box, species, wat, w)
    ev = ref["ev"]
    lhs = rc.virial_terms["w_coul"][0, 0] + rc.virial_terms["w_recip"][0, 0]
    rhs = (rc.u_real[0, 0] + rc.u_recip[0, 0]) + rc.u_self[0, 0]
    scale = ref["abs_w_coul"] + ref["abs_w_recip"] + ev["abs_real"] + ev["abs_recip"] + abs(ev["u_self"])
    print(f"w {w}: W_coul + W_recip = {lhs:.9f}, U_coul = {rhs:.9f} kJ/mol, |difference| / abs terms = {abs(lhs - rhs) / scale:.3e} (bound 3e-12)")
    assert abs(rhs) > 1.0 and abs(lhs - rhs) <= 3e-12 * scale


# ---- 4, 5: inside runs -------------------------------------------------------------------------------------------------------
def _run(case, calls, virial, source, w=0.0, interval=2, record=True, **cfg):
    """a rigid run of sum(calls) steps in len(calls) calls with the observer (and the virial log) at `interval`, the recorder
    beside it: (rows, virial rows or None, steps, recorded x, recorded v, final state)"""
    eng, x, v, f = case.make()
    eng.water_classical_configure(interval, ewald_tol=DELTA, m_site=w, virial=virial, **{**POT, **cfg})
    if source == "water":
        eng.md_force_source("water_classical")
        f = eng.water_classical_forces(x, case.species)[0].float().contiguous()
    if record:
        eng.traj_configure(interval, max_frames=sum(calls) // interval, fields=("x", "v"))
    chain, done = None, 0
    for n in calls:
        chain = case.run(eng, x, v, f, n, first_step=done, chain=chain)
        done += n
    assert eng.last_status == 0
    rd = eng.water_classical_read(forces=True)
    tr = eng.traj_read() if record else None
    out = dict(rows=np.stack([_rows(rd, q) for q in range(rd.steps.shape[0])]), steps=rd.steps,
               vrows=None if rd.virial is None else np.stack([_vrows(rd, q) for q in range(rd.steps.shape[0])]),
               forces=rd.forces, state=_state(x, v, f), rd=rd,
               x=None if tr is None else [tr.x[t].reshape(-1, 3) for t in range(tr.steps.shape[0])],
               v=None if tr is None else [tr.v[t].reshape(-1, 3) for t in range(tr.steps.shape[0])])
    return eng, out


@pytest.mark.parametrize("source", ["network", "water"])
@pytest.mark.parametrize("integrator", ["baoab", "nhc"])
def test_nothing_else_moves_when_the_virial_is_armed(integrator, source):
    """forces on given positions, the rows of gamd_water_read, the last sample's f_cl and the trajectory of a short rigid run"""
    res = []
    for virial in (False, True):
        case = _Water(integrator, n_mol=86)
        eng, out = _run(case, [6], virial, source, record=False)
        f, rd = eng.water_classical_forces(case.pos.astype(np.float32), case.species)
        out["eval"] = (f.cpu().numpy(), _rows(rd))
        eng.close()
        res.append(out)
    off, on = res
    assert off["vrows"] is None and on["vrows"] is not None and on["vrows"].shape == (3, 1, 6) and np.isfinite(on["vrows"]).all()
    assert np.array_equal(off["steps"], [2, 4, 6]) and np.array_equal(on["steps"], off["steps"])
    assert np.array_equal(_bits(on["rows"]), _bits(off["rows"])) and np.array_equal(_bits(on["forces"]), _bits(off["forces"]))
    for a, b in zip(on["state"], off["state"]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert np.array_equal(_bits(on["eval"][0]), _bits(off["eval"][0])) and np.array_equal(_bits(on["eval"][1]), _bits(off["eval"][1]))
    assert (on["rows"][:, :, 4] > 0).all()


def _ke_com_host(v, length=10.0):
    p = (MASS_O * v[0::3].astype(np.float64) / length + MASS_H * v[1::3].astype(np.float64) / length) + MASS_H * v[2::3].astype(np.float64) / length
    return 0.5 * ((p * p).sum(axis=1) / (MASS_O + (MASS_H + MASS_H))).sum()


@pytest.mark.parametrize("w", [0.0, W4], ids=["3site", "4site"])
def test_rows_of_a_water_source_run_are_the_eval_call_on_the_recorded_frames(w):
    case = _Water("baoab", n_mol=86)
    eng, one = _run(case, [8], True, "water", w=w)
    assert np.array_equal(one["steps"], [2, 4, 6, 8]) and len(one["x"]) == 4 and one["vrows"].shape == (4, 1, 6)
    for q in range(4):
        ev = eng.water_classical_virial(one["x"][q], case.species, one["v"][q], mass_o_amu=MASS_O, mass_h_amu=MASS_H)
        assert np.array_equal(_bits(_vrows(ev)), _bits(one["vrows"][q])), (q, _vrows(ev), one["vrows"][q])
        assert np.array_equal(_bits(_rows(ev)[:, :5]), _bits(one["rows"][q][:, :5]))
        ke = _ke_com_host(one["v"][q])
        print(f"w {w} sample {q}: " + ", ".join(f"{c} {one['vrows'][q, 0, k]:.6f}" for k, c in enumerate(vr.COLUMNS))
              + f"; |KE_com - host| / KE_com = {abs(one['vrows'][q, 0, 4] - ke) / ke:.3e}")
        assert ke > 0.0 and abs(one["vrows"][q, 0, 4] - ke) <= TOL * ke
    # the first frame against the float64 reference as well
    ref = vr.virial(one["x"][0], case.box, case.species, _water(), w, one["v"][0], MASS_O, MASS_H)
    _check_row(f"w {w} sample 0", one["vrows"][0, 0], ref)
    rd = one["rd"]
    vol = float(np.float32(case.box)) ** 3 / 1000.0
    from gamd_amd.engine import BAR_PER_KJ_MOL_NM3, lj_dispersion_correction
    p = rd.pressure(None, vol)
    assert np.array_equal(p, BAR_PER_KJ_MOL_NM3 * (2.0 * rd.ke_com + rd.virial) / (3.0 * vol)) and np.isfinite(p).all()
    w_lrc = lj_dispersion_correction(86, vol, 3.15075 / 10.0, 0.635968, 6.8 / 10.0, 5.8 / 10.0)[1]
    assert np.array_equal(rd.pressure(None, vol, dispersion=True), p + BAR_PER_KJ_MOL_NM3 * w_lrc / (3.0 * vol))
    print(f"w {w}: pressure {p[:, 0]} bar, dispersion correction {BAR_PER_KJ_MOL_NM3 * w_lrc / (3.0 * vol):.3f} bar")
    eng.close()
    # the same bits from a chunked run
    eng, two = _run(case, [3, 5], True, "water", w=w)
    eng.close()
    assert np.array_equal(two["steps"], one["steps"]) and np.array_equal(_bits(two["vrows"]), _bits(one["vrows"]))
    assert np.array_equal(_bits(two["rows"]), _bits(one["rows"]))


def _overflow_run(cap, virial=True):
    """tests/test_gpu_water_classical.py's scheme: flexible molecules contracting towards the centre of the box"""
    from gamd_amd.engine import GamdForce
    case = _Water()
    x = torch.from_numpy(case.pos).float().cuda()
    v = (-(x - case.box / 2)).contiguous() * 6.0
    md = dict(dt_ps=0.0005, mass_amu=wl.MASS_O, mass_h_amu=wl.MASS_H, temperature_k=0.0, gamma_per_ps=0.0, seed=1, species=case.species)
    eng = GamdForce(case.sd, case.n, case.box, case.rc, edge_capacity=cap, **case.eng_kw)
    f = eng.forward(x, species=case.species, denormalize=True).clone()
    e_now = eng.counts()[0]
    eng.water_classical_configure(3, ewald_tol=DELTA, virial=virial)
    eng.md_run(x, v, f, 30, **md)
    status, rd = eng.last_status, eng.water_classical_read()
    eng.close()
    return status, e_now, rd


def test_overflow_in_the_middle_of_a_run_writes_every_virial_row_with_the_bits_of_an_ample_buffer():
    s0, e_now, a = _overflow_run(0)
    s1, _, b = _overflow_run(e_now + 60)
    assert s0 == 0 and s1 == 1, "the run was meant to outgrow its edge buffer"
    assert np.array_equal(a.steps, 3 * np.arange(1, 11)) and np.array_equal(b.steps, a.steps) and a.dropped == b.dropped == 0
    va, vb = np.stack([_vrows(a, q) for q in range(10)]), np.stack([_vrows(b, q) for q in range(10)])
    assert np.array_equal(_bits(va), _bits(vb)) and np.isfinite(va).all() and (va[:, :, 4] > 0).all()
    for name in a.COLUMNS:
        assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name


CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_water_virial as t
from gamd_amd import _lib
eng, out = t._run(t._Water("baoab", n_mol=86), [4], True, "water", w=t.W4)
eng.close()
print("RESULT", json.dumps(dict(version=_lib.load().gamd_version().decode(), steps=out["steps"].tolist(),
                                vrows=t._bits(out["vrows"]).tolist(), rows=t._bits(out["rows"]).tolist())))
"""


def test_checked_build_gives_the_same_virial_rows():
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    env = {k: v for k, v in os.environ.items() if k not in ("GAMD_LIB", "GAMD_CHK_INJECT")}
    env["GAMD_LIB"] = CHK
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    assert p.returncode == 0 and "RESULT" in p.stdout, (p.stdout[-800:], p.stderr[-1500:])
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got["version"].endswith("checked")
    eng, out = _run(_Water("baoab", n_mol=86), [4], True, "water", w=W4)
    eng.close()
    assert got["steps"] == out["steps"].tolist() == [2, 4]
    assert got["vrows"] == _bits(out["vrows"]).tolist() and got["rows"] == _bits(out["rows"]).tolist()


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------
def test_the_setter_refuses_an_lj_handle_and_a_pending_run_and_leaves_the_state():
    from gamd_amd._lib import GamdError, load
    lib = load()
    lj = _Case("lj")
    eng, x, v, f = lj.make()
    assert lib.gamd_water_virial(eng._h, 1) == -22 and b"GAMD_KIND_LJ" in lib.gamd_last_error()
    assert lib.gamd_water_virial_read(eng._h, None, None, 0, None) == -22
    eng.close()
    case = _Water("baoab", n_mol=86)
    eng, x, v, f = case.make()
    assert lib.gamd_water_virial(eng._h, 1) == -22 and b"gamd_water_configure" in lib.gamd_last_error()      # no parameters yet
    eng.water_classical_configure(2, ewald_tol=DELTA, **POT)
    bare = eng.water_classical_read()
    assert bare.virial is None
    with pytest.raises(NotImplementedError, match="virial"):
        bare.pressure(None, 1.0)
    eng.water_classical_configure(2, ewald_tol=DELTA, virial=True, **POT)
    case.run(eng, x, v, f, 4, sync=False)
    assert lib.gamd_water_virial(eng._h, 0) == -22 and b"enqueued" in lib.gamd_last_error()                 # a run is pending
    with pytest.raises(GamdError, match="-22.*enqueued"):
        eng.water_classical_virial(case.pos.astype(np.float32), case.species)
    assert eng.sync_status() == 0
    rd = eng.water_classical_read()                                                                         # still armed: both rows
    assert np.array_equal(rd.steps, [2, 4]) and rd.virial.shape == (2, 1) and (rd.ke_com > 0).all() and np.isfinite(rd.virial).all()
    with pytest.raises(GamdError, match="-22.*mass"):
        eng.water_classical_virial(case.pos.astype(np.float32), case.species, mass_h_amu=0.0)
    # off again: what was logged stays readable through the C call, and further samples leave the rows alone
    assert lib.gamd_water_virial(eng._h, 0) == 0
    case.run(eng, x, v, f, 2, first_step=4)
    keep = np.zeros((3, 1, 6))
    n_rows = ctypes.c_int64()
    assert lib.gamd_water_virial_read(eng._h, None, keep.ctypes.data_as(ctypes.c_void_p), 3, ctypes.byref(n_rows)) == 0
    assert n_rows.value == 3 and np.array_equal(_bits(keep[:2, :, 5]), _bits(rd.virial)) and (keep[2] == 0.0).all()
    eng.close()
