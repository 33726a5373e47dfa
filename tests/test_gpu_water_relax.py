"""The water minimisers under the configured potential on the device (gamd_water_minimize_potential,
gamd_amd/csrc/water_relax.hip): FIRE (water_minimize) and L-BFGS (water_minimize_lbfgs) with the TIP4P M-site, particle-mesh Ewald
and the cell table in every combination.  Every case runs for both minimisers unless it says otherwise.

Shapes: the 86-molecule lattice start (258 atoms: one full 256-atom tile and a tail of 2, the last molecule across the tiles;
L = 13.87 Angstrom, r_cut 6.8: four cells per axis), PME grid (16, 16, 16) order 6; the same molecules in the box
[13.875, 13.75, 14.0] with the grid (16, 32, 8), orders 6 and 4; 258 molecules at r_cut 9.5 (a full tile of 256 oxygens plus 2
for k_wrx_lj, several pair slices) with the grid (32, 32, 32).  ewald_tol is the minimisers' tests' 1e-8; the M-site weight is
TIP4P-Ew's 0.106676721 on the handle's default charges.

What is asserted, and where the bars come from
* The switch: off by default; on and off again the three refusals are back with their words and nothing is enqueued; its own
  refusals (LJ handle, no configure, on not 0 / 1, a pending run) are -22 by name.
* Reduction: with the switch on and no form set, x, f, x64 and the row are the switch-off bits, at tolerance 10 and at
  max_iter = 5.  (This cannot pass without the feature: the symbol does not exist.)
* The contract of every one of the seven non-empty combinations of {M-site, PME, cells} from the lattice start to tolerance
  10: converged; f is water_classical_forces(x, species)[0].float() bit for bit under that configuration; oxygens in [0, L),
  molecules whole, x64 rigid to 1e-12 (tests/test_gpu_water_minimize.py's _assert_rigid_whole_and_wrapped); the returned U and
  rms agree with tests/water_relax_ref.py's form on the returned x64 within the bar of
  test_gpu_water_minimize.py::test_positions_energy_and_rms_agree_with_the_float64_replay — max(100 x the reference's own
  spread under three molecule permutations and a 2^-50 perturbation of every force component, 1e-13 relative) — the spread
  measured here at that x64; and the reference's rms there is at most tolerance (1 + bar / rms).
* Replay parity at 86 molecules (M-site; PME order 6; M-site + PME + cells) after 32 iterations (FIRE) and 32 evaluations
  (L-BFGS, m = 6 and m = 1): |x64 - replay| within 100 x the replay's spread under the same permutations and perturbation
  (floor 1e-13 Angstrom), the factor and floor of tests/test_gpu_water_lbfgs.py.  The counts to tolerance 10 are the replay's,
  which are the same under every permutation and perturbation tried (a CPU study of five replays per case; COUNTS below; the
  rms at the stop is nowhere within 1e-3 relative of the tolerance).
* Cells against all pairs (3-site and M-site, plain and PME): the same state and counts to tolerance 10, positions after 32
  evaluations within the parity bar of the form.
* 258 molecules, M-site + cells + PME: max_iter = 8, the f contract, and U does not rise from one accepted L-BFGS point to the
  next (the API returns no trace: the calls with max_iter = 1 .. 8 are its prefixes, bit for bit, and give U per evaluation).
* Bits: two calls, a fresh handle, check_every 1, 7, 64, the checked library (status as the release library's, no -35), each
  box of a two-box handle against the box alone — the boxes start differently, one stops earlier, and its x64 and row are what
  it had when it stopped.
* A start for a run: after water_minimize_lbfgs under M-site + PME a rigid water-source md_run_nhc of 4 steps with the observer
  at interval 4 samples the potential of its frame: the row's terms are water_classical_forces' on that frame bit for bit and
  the force-error sums are within fp32 rounding of f_cl (tests/test_gpu_water_drive.py::test_observer_rows_on_a_driven_run).
* A failed box: under M-site + PME a box with a NaN coordinate fails with its x untouched and the other box converges."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import water_classical_ref as wr
import water_minimize_ref as wm
import water_relax_ref as rr
from gamd_amd import workloads as wl
from test_gpu_classical_drive import _i32, _i64
from test_gpu_water_classical import _Water, DELTA
from test_gpu_water_drive import _rattled, _scale_centres
from test_gpu_water_lbfgs import _lbfgs
from test_gpu_water_minimize import _assert_f_contract, _assert_rigid_whole_and_wrapped, _minimize, _start, _water_engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHK = os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")
TOL = 10.0
W = rr.TIP4PEW_W
R_CUT = 6.8
GRID = (16, 16, 16)
NONCUBIC = np.array([13.875, 13.75, 14.0], dtype=np.float32)
MINIMISERS = ("fire", "lbfgs")
COMBOS = [(m, p, c) for m in (False, True) for p in (False, True) for c in (False, True) if m or p or c]
# the float64 replay's counts to tolerance 10 from the 86-molecule start at r_cut 6.8 (FIRE: iterations; L-BFGS: evaluations
# with m = 6 / m = 1), the same under three molecule permutations and a 2^-50 force perturbation; cells change no value
COUNTS = {("msite", "fire"): 81, ("msite", "lbfgs", 6): 47, ("msite", "lbfgs", 1): 50,
          ("pme", "fire"): 101, ("pme", "lbfgs", 6): 87, ("pme", "lbfgs", 1): 65,
          ("msite+pme", "fire"): 85, ("msite+pme", "lbfgs", 6): 50, ("msite+pme", "lbfgs", 1): 42,
          ("plain", "fire"): 100, ("plain", "lbfgs", 6): 73, ("plain", "lbfgs", 1): 67}


def _kw(msite=False, pme=False, cells=False, on=True, grid=GRID, order=6):
    """the configure arguments of a form"""
    kw = dict(minimize_configured=on, cells=cells)
    if msite:
        kw["m_site"] = W
    if pme:
        kw.update(pme=grid, pme_order=order)
    return kw


def _form(msite=False, pme=False, grid=GRID, order=6):
    return rr.Form(w=W if msite else 0.0, pme=tuple(grid) if pme else None, order=order)


def _name(msite, pme):
    return "+".join((["msite"] if msite else []) + (["pme"] if pme else [])) or "plain"


def _run(mini, eng, x0, species, box=None, **kw):
    """(result, x, f, x64) of one call of either minimiser on a copy of x0"""
    if mini == "fire":
        kw.pop("m", None)
        return _minimize(eng, x0, species, box=box, **kw)
    return _lbfgs(eng, x0, species, box=box, **kw)


def _count(res, b=0):
    return int(res.iterations[b] if hasattr(res, "iterations") else res.evaluations[b])


def _bits(out):
    res, x, f, x64 = out
    return _i32(x).tolist(), _i32(f).tolist(), _i64(x64).tolist(), _i64(res.rows).tolist()


# ---- 1: the switch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mini", MINIMISERS)
def test_the_switch_is_off_by_default_and_off_again_brings_the_refusals_back(mini):
    from gamd_amd._lib import GamdError
    x0, box, species = _start(86)
    eng = _water_engine(86, box, R_CUT)
    words = ((dict(msite=True), "M-site.*gamd_water_minimize_potential"), (dict(pme=True), "PME.*gamd_water_minimize_potential"),
             (dict(cells=True), "cell table.*gamd_water_minimize_potential.*cells off"))
    for form, word in words:                                    # never switched on
        eng.water_classical_configure(0, ewald_tol=DELTA, r_cut=R_CUT, **{k: v for k, v in _kw(on=False, **form).items() if k != "minimize_configured"})
        with pytest.raises(GamdError, match="-22.*" + word):
            _run(mini, eng, x0, species, tolerance=TOL)
    eng.water_classical_configure(0, ewald_tol=DELTA, r_cut=R_CUT, **_kw(msite=True))
    assert _run(mini, eng, x0, species, tolerance=TOL, max_iter=2)[0].status == 1
    for form, word in words:                                    # on, then off
        eng.water_classical_configure(0, ewald_tol=DELTA, r_cut=R_CUT, **_kw(on=False, **form))
        x = torch.from_numpy(x0).cuda()
        with pytest.raises(GamdError, match="-22.*" + word):
            (eng.water_minimize if mini == "fire" else eng.water_minimize_lbfgs)(x, species, tolerance=TOL)
        assert np.array_equal(_i32(x.cpu().numpy()), _i32(x0))  # nothing was enqueued
    eng.close()


def test_the_switchs_own_refusals_name_their_reason():
    from test_gpu_report import _Case
    eng, x, v, f = _Case("lj").make()
    assert eng._lib.gamd_water_minimize_potential(eng._h, 1) == -22
    msg = eng._lib.gamd_last_error()
    assert b"GAMD_KIND_LJ" in msg and b"gamd_water_minimize_potential" in msg
    eng.close()
    case = _Water("nhc", n_mol=86)
    eng, x, v, f = case.make()
    assert eng._lib.gamd_water_minimize_potential(eng._h, 1) == -22 and b"gamd_water_configure" in eng._lib.gamd_last_error()
    eng.water_classical_configure(0, ewald_tol=DELTA, r_cut=R_CUT)
    for bad in (2, -1):
        assert eng._lib.gamd_water_minimize_potential(eng._h, bad) == -22 and b"is not 0" in eng._lib.gamd_last_error()
    case.run(eng, x, v, f, 2, sync=False)
    assert eng._lib.gamd_water_minimize_potential(eng._h, 1) == -22
    msg = eng._lib.gamd_last_error()
    assert b"enqueued" in msg and b"gamd_water_minimize_potential" in msg
    assert eng.sync_status() == 0
    assert eng._lib.gamd_water_minimize_potential(eng._h, 1) == 0 and eng._lib.gamd_water_minimize_potential(eng._h, 0) == 0
    eng.close()


# ---- 2: reduction ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mini", MINIMISERS)
@pytest.mark.parametrize("stop", [dict(tolerance=TOL), dict(tolerance=TOL, max_iter=5)], ids=["tolerance 10", "max_iter 5"])
def test_with_no_form_set_the_switch_changes_no_bit(mini, stop):
    x0, box, species = _start(86)
    eng = _water_engine(86, box, R_CUT)
    off = _run(mini, eng, x0, species, **stop)
    eng.close()
    eng = _water_engine(86, box, R_CUT, minimize_configured=True)
    on = _run(mini, eng, x0, species, **stop)
    _assert_f_contract(eng, on[1], on[2], species)
    eng.close()
    print(f"{mini}, {stop}: off {off[0]!r}, on {on[0]!r}")
    assert on[0].status == off[0].status == (1 if "max_iter" in stop else 0)
    assert _bits(on) == _bits(off)


# ---- 3: the contract per form ------------------------------------------------------------------------------------------------
def _reference_bars(form, x64, box, species, wat):
    """the form's U and projected rms on x64, and the bars of test_positions_energy_and_rms_agree_with_the_float64_replay
    (tests/test_gpu_water_minimize.py) with the reference's spread measured at this point"""
    _, rms, u = rr.projected(form, x64, box, species, wat)
    du = dr = 0.0
    n_mol = x64.shape[0] // 3
    for kind, seed in (("perm", 1), ("perm", 2), ("perm", 3), ("perturb", 4)):
        p = np.random.default_rng(seed).permutation(n_mol) if kind == "perm" else np.arange(n_mol)
        a = (3 * p[:, None] + np.arange(3)[None, :]).reshape(-1)
        ev = rr.evaluate(form, x64[a], box, species, wat)
        F = ev["forces"]
        if kind == "perturb":
            F = F * (1.0 + 2.0 ** -50 * np.random.default_rng(seed).uniform(-1.0, 1.0, F.shape))
        F = wm.project(x64[a], F)
        du, dr = max(du, abs(ev["energy"] - u)), max(dr, abs(float(np.sqrt((F * F).sum() / F.size)) - rms))
    return u, rms, max(100.0 * du, 1e-13 * abs(u)), max(100.0 * dr, 1e-13 * rms), du, dr


@pytest.mark.parametrize("mini", MINIMISERS)
@pytest.mark.parametrize("msite,pme,cells", COMBOS)
def test_every_form_converges_and_meets_the_contract(mini, msite, pme, cells):
    x0, box, species = _start(86)
    eng = _water_engine(86, box, R_CUT, **_kw(msite, pme, cells))
    res, x, f, x64 = _run(mini, eng, x0, species, tolerance=TOL)
    _assert_f_contract(eng, x, f, species)
    eng.close()
    u, rms, bar_u, bar_r, du, dr = _reference_bars(_form(msite, pme), x64, box, species, wr.Water(r_cut=R_CUT, ewald_tol=DELTA))
    print(f"{mini}, {_name(msite, pme)}{' + cells' if cells else ''}: {res!r}; the reference on x64: U {u:.9e} (device off by "
          f"{abs(res.energy[0] - u):.3e}, spread {du:.3e}, bar {bar_u:.3e}), rms {rms:.9e} (device off by {abs(res.rms[0] - rms):.3e}, "
          f"spread {dr:.3e}, bar {bar_r:.3e})")
    assert res.status == 0 and res.state == ["converged"] and res.rms[0] <= TOL < res.rms_start[0] and res.energy[0] < res.energy_start[0]
    _assert_rigid_whole_and_wrapped(x, x64, box)
    assert abs(res.energy[0] - u) <= bar_u
    assert abs(res.rms[0] - rms) <= bar_r
    assert rms <= TOL * (1.0 + bar_r / rms)
    key = (_name(msite, pme), mini) + ((6,) if mini == "lbfgs" else ())
    if COUNTS.get(key) is not None:
        assert _count(res) == COUNTS[key]


@pytest.mark.parametrize("mini", MINIMISERS)
@pytest.mark.parametrize("order", [6, 4])
def test_three_different_edges_with_the_non_cubic_grid(mini, order):
    x0, box, species = _start(86)
    edges = NONCUBIC / np.float32(box)
    xs = _scale_centres(x0.astype(np.float64), edges).astype(np.float32)
    eng = _water_engine(86, NONCUBIC, R_CUT, **_kw(True, True, True, grid=(16, 32, 8), order=order))
    res, x, f, x64 = _run(mini, eng, xs, species, box=NONCUBIC, tolerance=TOL)
    _assert_f_contract(eng, x, f, species, box=NONCUBIC)
    eng.close()
    form = _form(True, True, grid=(16, 32, 8), order=order)
    u, rms, bar_u, bar_r, du, dr = _reference_bars(form, x64, NONCUBIC, species, wr.Water(r_cut=R_CUT, ewald_tol=DELTA))
    print(f"{mini}, order {order}: {res!r}; reference U {u:.9e} (off by {abs(res.energy[0] - u):.3e}, bar {bar_u:.3e}), rms {rms:.9e} "
          f"(off by {abs(res.rms[0] - rms):.3e}, bar {bar_r:.3e})")
    assert res.status == 0 and res.state == ["converged"]
    _assert_rigid_whole_and_wrapped(x, x64, NONCUBIC)
    assert abs(res.energy[0] - u) <= bar_u and abs(res.rms[0] - rms) <= bar_r and rms <= TOL * (1.0 + bar_r / rms)


# ---- 4: parity with the float64 replay ---------------------------------------------------------------------------------------
_REPLAYS = {}


def _replay32(msite, pme, mini, m):
    """the replay after 32 iterations / evaluations from the 86-molecule start: as it is, under three molecule permutations and
    with every force component perturbed by 2^-50 relative (computed once per case)"""
    key = (msite, pme, mini, m)
    if key not in _REPLAYS:
        x0, box, species = _start(86)
        wat, form = wr.Water(r_cut=R_CUT, ewald_tol=DELTA), _form(msite, pme)
        xs = []
        for kind, seed in (("base", None), ("perm", 1), ("perm", 2), ("perm", 3), ("perturb", 4)):
            p = np.random.default_rng(seed).permutation(86) if kind == "perm" else np.arange(86)
            a = (3 * p[:, None] + np.arange(3)[None, :]).reshape(-1)
            pert = np.random.default_rng(seed) if kind == "perturb" else None
            if mini == "fire":
                r = rr.minimize(form, x0[a], box, species, wat, 1e-300, max_iter=32, perturb=pert)
            else:
                r = rr.minimize_lbfgs(form, x0[a], box, species, wat, 1e-300, max_iter=32, m=m, perturb=pert)
            out = np.empty_like(r["x"])
            out[a] = r["x"]
            xs.append(out)
        spread = max(np.abs(x - xs[0]).max() for x in xs[1:])
        _REPLAYS[key] = dict(x=xs[0], spread=spread, bar=max(100.0 * spread, 1e-13))
    return _REPLAYS[key]


PARITY = [(True, False, False), (False, True, False), (True, True, True)]


@pytest.mark.parametrize("mini,m", [("fire", 0), ("lbfgs", 6), ("lbfgs", 1)])
@pytest.mark.parametrize("msite,pme,cells", PARITY)
def test_positions_after_32_agree_with_the_float64_replay_and_the_counts_are_its(msite, pme, cells, mini, m):
    x0, box, species = _start(86)
    rp = _replay32(msite, pme, mini, m)
    eng = _water_engine(86, box, R_CUT, **_kw(msite, pme, cells))
    res, x, f, x64 = _run(mini, eng, x0, species, tolerance=1e-300, max_iter=32, m=m)
    _assert_f_contract(eng, x, f, species)
    full = _run(mini, eng, x0, species, tolerance=TOL, m=m)[0]
    eng.close()
    dx = np.abs(x64 - rp["x"]).max()
    print(f"{mini} m = {m}, {_name(msite, pme)}{' + cells' if cells else ''}: after 32: |dx| max {dx:.3e} A (the replay's spread "
          f"{rp['spread']:.3e}, bar {rp['bar']:.3e}); to tolerance 10: {full!r}")
    assert res.status == 1 and _count(res) == 32
    assert dx <= rp["bar"]
    key = (_name(msite, pme), mini) + ((m,) if mini == "lbfgs" else ())
    assert full.status == 0
    if COUNTS.get(key) is not None:
        assert _count(full) == COUNTS[key]


# ---- 5: cells against all pairs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mini", MINIMISERS)
@pytest.mark.parametrize("msite,pme", [(False, False), (False, True), (True, False), (True, True)])
def test_cells_and_all_pairs_take_the_same_path(mini, msite, pme):
    x0, box, species = _start(86)
    out = {}
    for cells in (False, True):
        eng = _water_engine(86, box, R_CUT, **_kw(msite, pme, cells))
        out[cells] = (_run(mini, eng, x0, species, tolerance=TOL)[0], _run(mini, eng, x0, species, tolerance=1e-300, max_iter=32)[3])
        eng.close()
    bar = _replay32(msite, pme, mini, 6 if mini == "lbfgs" else 0)["bar"]
    dx = np.abs(out[True][1] - out[False][1]).max()
    print(f"{mini}, {_name(msite, pme)}: all pairs {out[False][0]!r}; cells {out[True][0]!r}; after 32: |dx| max {dx:.3e} A (bar {bar:.3e})")
    assert out[True][0].state == out[False][0].state == ["converged"] and _count(out[True][0]) == _count(out[False][0])
    assert dx <= bar


# ---- 6: 258 molecules ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mini", MINIMISERS)
def test_258_molecules_under_msite_cells_and_pme(mini):
    x0, box, species = _start(258)
    eng = _water_engine(258, box, 9.5, **_kw(True, True, True, grid=(32, 32, 32)))
    res, x, f, x64 = _run(mini, eng, x0, species, tolerance=1e-300, max_iter=8)
    _assert_f_contract(eng, x, f, species)
    _assert_rigid_whole_and_wrapped(x, x64, box)
    assert res.status == 1 and _count(res) == 8 and res.energy[0] < res.energy_start[0]
    if mini == "lbfgs":                                         # the calls with max_iter = k are the prefixes of this one
        u, acc = float(res.energy_start[0]), 0
        for k in range(1, 9):
            r = _run(mini, eng, x0, species, tolerance=1e-300, max_iter=k)[0]
            assert int(r.accepted[0]) >= acc and (r.energy[0] < u if int(r.accepted[0]) > acc else r.energy[0] == u), k
            u, acc = float(r.energy[0]), int(r.accepted[0])
        assert _i64(np.array([u]))[0] == _i64(res.energy[:1])[0] and acc == int(res.accepted[0])
    eng.close()


# ---- 7: bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mini", MINIMISERS)
def test_two_calls_a_fresh_handle_and_every_check_every_give_the_same_bits(mini):
    x0, box, species = _start(86)
    eng = _water_engine(86, box, R_CUT, **_kw(True, True, True))
    first = _run(mini, eng, x0, species, tolerance=TOL)
    assert first[0].status == 0
    ref = _bits(first)
    assert _bits(_run(mini, eng, x0, species, tolerance=TOL)) == ref, "second call"
    eng.close()
    eng = _water_engine(86, box, R_CUT, **_kw(True, True, True))
    for every in (1, 7, 64):
        assert _bits(_run(mini, eng, x0, species, tolerance=TOL, check_every=every)) == ref, f"check_every = {every}"
    eng.close()


@pytest.mark.parametrize("mini", MINIMISERS)
def test_each_box_of_a_two_box_handle_gets_the_bits_it_gets_alone(mini):
    (xa, ba, species), (xb, _, _) = _start(86), _start(86, seed=6)
    edges = NONCUBIC / np.float32(ba)
    xb = _scale_centres(xb.astype(np.float64), edges).astype(np.float32)
    boxes = np.stack([np.full(3, ba, dtype=np.float32), NONCUBIC]).astype(np.float32)
    kw = _kw(True, True, True)
    eng = _water_engine(86, float(ba), R_CUT, n_boxes=2, **kw)
    res, x, f, x64 = _run(mini, eng, np.concatenate([xa, xb]), species, box=boxes, tolerance=TOL)
    _assert_f_contract(eng, x, f, species, box=boxes)
    eng.close()
    print(f"{mini}, two boxes: {res!r}")
    assert res.status == 0 and _count(res, 0) != _count(res, 1)     # one box stops first
    for b, (xs, box) in enumerate(((xa, ba), (xb, NONCUBIC))):
        one = _water_engine(86, box, R_CUT, **kw)
        r1, x1, f1, x641 = _run(mini, one, xs, species, box=box, tolerance=TOL)
        one.close()
        sl = slice(258 * b, 258 * (b + 1))
        assert np.array_equal(_i64(x64[sl]), _i64(x641)) and np.array_equal(_i64(res.rows[b]), _i64(r1.rows[0])), f"box {b}"
        assert np.array_equal(_i32(x[sl]), _i32(x1)) and np.array_equal(_i32(f[sl]), _i32(f1)), f"box {b}"


CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_water_relax as t
from gamd_amd import _lib
print("RESULT", json.dumps(dict(version=_lib.load().gamd_version().decode(), bits=t._w86_bits())))
"""


def _w86_bits():
    x0, box, species = _start(86)
    eng = _water_engine(86, box, R_CUT, **_kw(True, True, True))
    out = []
    for mini in MINIMISERS:
        r = _run(mini, eng, x0, species, tolerance=TOL, max_iter=24)
        out.append([r[0].status, *_bits(r)])
    eng.close()
    return out


def test_checked_build_gives_the_same_bits():
    """the ring count k_wrx_lbmols reads and everything the reused table, cell and PME kernels address pass the checked library's
    range checks (a failed one would come back as -35), and the bits are the release library's"""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    env = {k: v for k, v in os.environ.items() if k not in ("GAMD_LIB", "GAMD_CHK_INJECT")}
    env["GAMD_LIB"] = CHK
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert p.returncode == 0 and "RESULT" in p.stdout, (p.stdout[-800:], p.stderr[-1500:])
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got["version"].endswith("checked")
    mine = _w86_bits()
    assert got["bits"] == mine and [b[0] for b in mine] == [1, 1]


# ---- 8: a start for a run ----------------------------------------------------------------------------------------------------------
def test_a_water_source_nhc_run_starts_from_the_box_minimised_under_msite_and_pme():
    case = _Water("nhc", n_mol=86)
    eng, _, _, _ = case.make()
    kw = dict(ewald_tol=DELTA, r_cut=R_CUT, **_kw(True, True, False))
    eng.water_classical_configure(0, **kw)
    x = torch.from_numpy(case.pos.astype(np.float32)).cuda()
    res = eng.water_minimize_lbfgs(x, case.species, tolerance=TOL)
    assert res.status == 0
    f = res.f
    eng.md_force_source("water_classical")
    v = torch.from_numpy(_rattled(x.cpu().numpy().astype(np.float64), case.species, 6)).float().cuda()
    eng.water_classical_configure(4, **kw)
    eng.traj_configure(1, max_frames=4, fields=("x", "f"))
    case.run(eng, x, v, f, 4)
    assert eng.last_status == 0
    rd, tr = eng.water_classical_read(forces=True), eng.traj_read()
    assert rd.dropped == 0 and np.array_equal(rd.steps, [4])
    fcl, one = eng.water_classical_forces(tr.x[3].reshape(-1, 3), case.species)
    fcl = fcl.cpu().numpy()
    for name in ("u_lj", "u_real", "u_recip", "u_self", "pairs", "sum_q", "energy"):
        assert _i64(getattr(rd, name)[0])[0] == _i64(getattr(one, name)[0])[0], name
    assert np.array_equal(_i64(rd.forces), _i64(fcl)) and np.array_equal(_i32(tr.f[3].reshape(-1, 3)), _i32(fcl.astype(np.float32)))
    norms = np.sqrt((fcl * fcl).sum(axis=1))
    norm, eps, n = norms.sum(), 2.0 ** -24, case.n
    assert rd.pairs[0, 0] > 0 and rd.sum_q[0, 0] == 0.0
    assert abs(rd.sum_norm_cl[0, 0] - norm) <= 1e-12 * norm
    assert 0.0 < rd.sum_abs[0, 0] <= eps * np.sqrt(3.0) * norm * (1.0 + 1e-12)
    assert 0.0 < rd.sum_sq[0, 0] <= eps * eps * (norms * norms).sum() * (1.0 + 1e-12)
    assert abs(rd.sum_norm[0, 0] - rd.sum_norm_cl[0, 0]) <= eps * norm * (1.0 + 1e-12)
    assert rd.excluded[0, 0] == 0 and abs(n - rd.sum_cos[0, 0]) <= n * 1e-13
    eng.close()


# ---- 9: a failed box ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mini", MINIMISERS)
def test_a_box_with_a_nan_coordinate_fails_untouched_and_the_other_converges(mini):
    good, box, species = _start(86)
    bad = good.copy()
    bad[100, 1] = np.nan
    eng = _water_engine(86, float(box), R_CUT, n_boxes=2, **_kw(True, True, False))
    x0 = np.concatenate([bad, good])
    x = torch.from_numpy(x0).cuda()
    f = torch.full_like(x, 7.0)
    res = (eng.water_minimize if mini == "fire" else eng.water_minimize_lbfgs)(x, species, f, tolerance=TOL, return_x64=True)
    xh, fh = x.cpu().numpy(), f.cpu().numpy()
    print(f"{mini}: {res!r}")
    assert res.status == 2 and res.state == ["failed", "converged"] and _count(res, 0) == 0
    assert np.array_equal(_i32(xh[:258]), _i32(x0[:258])) and np.array_equal(fh[:258], np.full((258, 3), 7.0, dtype=np.float32))
    one = _water_engine(86, box, R_CUT, **_kw(True, True, False))
    r1, x1, f1, x641 = _run(mini, one, good, species, tolerance=TOL)
    one.close()
    assert np.array_equal(_i32(xh[258:]), _i32(x1)) and np.array_equal(_i64(res.rows[1]), _i64(r1.rows[0]))
    eng.close()
