"""Float64 references for the water minimisers under the configured potential (gamd_water_minimize_potential,
gamd_amd/csrc/water_relax.hip): the FIRE replay of tests/water_minimize_ref.py and the L-BFGS replay of tests/water_lbfgs_ref.py
with the POTENTIAL as a parameter.

A `Form` names what the handle's three switches set:
    Form()                                   3-site, plain Ewald sum            water_classical_ref.evaluate
    Form(w=0.106676721)                      the TIP4P M-site, plain sum        water_msite_ref.evaluate
    Form(pme=(16, 16, 16), order=6)          3-site, particle-mesh Ewald        water_pme_ref.evaluate(w=None)
    Form(w=..., pme=..., order=...)          M-site and PME                     water_pme_ref.evaluate(w=w)
The cell table changes the order of the device's sums and no value in float64: a Form has no entry for it.

The two replay modules are NOT edited and their loops are NOT restated: both call `wr.evaluate(x, box, species, w, length_per_nm)`
through their module global `wr` and read `forces` and `energy` of the result, so `minimize` / `minimize_lbfgs` below hand them
another `evaluate` by putting a stand-in for that global in place for the duration of the call (and putting the module back).
With Form() the stand-in calls water_classical_ref.evaluate with the same arguments: the results are the existing replays'
exactly (tests/test_water_relax_host.py).

The forces every form returns are those on the three REAL atoms — with the M-site, M's force spread with the weights
1 - 2 w, w, w — so the replays' projection (water_minimize_ref.project) gives the device's projected force.  Not an oracle
module: nothing here was compared with OpenMM."""
import contextlib
import types
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import water_classical_ref as wr
import water_lbfgs_ref as wlr
import water_minimize_ref as wm
import water_msite_ref as w4
import water_pme_ref as wp

TIP4PEW_W = 0.106676721


@dataclass(frozen=True)
class Form:
    w: float = 0.0                                  # the hydrogens' weight of the M-site, 0 = 3-site
    pme: Optional[Tuple[int, int, int]] = None      # the PME grid, None = the plain sum
    order: int = 6

    def name(self):
        return "+".join(([f"msite({self.w:g})"] if self.w else []) + ([f"pme{self.pme}/{self.order}"] if self.pme else [])) or "3-site plain"


def evaluate(form, x, box, species, wat, length_per_nm=0.0):
    """the form's potential on x: the dict of water_classical_ref.evaluate (forces on the real atoms in kJ/mol/nm, energy)"""
    if form.pme is not None:
        return wp.evaluate(x, box, species, wat, tuple(form.pme), form.order, w=(form.w if form.w else None), length_per_nm=length_per_nm)
    if form.w:
        return w4.evaluate(x, box, species, wat, form.w, length_per_nm)
    return wr.evaluate(x, box, species, wat, length_per_nm)


@contextlib.contextmanager
def _potential(form, *modules):
    stand_in = types.SimpleNamespace(evaluate=lambda x, box, species, wat, length_per_nm=0.0: evaluate(form, x, box, species, wat, length_per_nm))
    try:
        for m in modules:
            m.wr = stand_in
        yield
    finally:
        for m in modules:
            m.wr = wr


def minimize(form, x, box, species, wat, tolerance, **kw):
    """water_minimize_ref.minimize (FIRE) under the form's potential: its arguments and its result"""
    with _potential(form, wm):
        return wm.minimize(x, box, species, wat, tolerance, **kw)


def minimize_lbfgs(form, x, box, species, wat, tolerance, **kw):
    """water_lbfgs_ref.minimize under the form's potential: its arguments and its result"""
    with _potential(form, wlr, wm):
        return wlr.minimize(x, box, species, wat, tolerance, **kw)


def projected(form, x, box, species, wat, length_per_nm=0.0):
    """(the projected force [N, 3], its rms over 3N components, U) of the form at x"""
    ev = evaluate(form, x, box, species, wat, length_per_nm)
    F = wm.project(np.asarray(x, dtype=np.float64), ev["forces"])
    return F, float(np.sqrt((F * F).sum() / F.size)), ev["energy"]


def tangent(x, rng):
    """a random direction of the rigid manifold at x [N, 3] (O,H,H): per molecule a translation plus a rotation about its
    centroid, d = t + omega x (r - c) — every bond length is stationary along it"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3, 3)
    t, om = rng.normal(size=(x.shape[0], 1, 3)), rng.normal(size=(x.shape[0], 1, 3))
    c = x.mean(axis=1, keepdims=True)
    return (t + np.cross(np.broadcast_to(om, x.shape), x - c)).reshape(-1, 3)


def move_rigid(x, d, h, r_oh=None, r_hh=None):
    """x carried along the tangent direction d by the step h and back onto the manifold: SETTLE(x, x + h d)"""
    x = np.asarray(x, dtype=np.float64)
    return wm.settle(x, x + h * d, wm.TIP3P_R_OH if r_oh is None else r_oh, wm.TIP3P_R_HH if r_hh is None else r_hh)
