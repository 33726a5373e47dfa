"""Float64 host replay of the water L-BFGS energy minimiser (gamd_amd/csrc/water_lbfgs.hip) on ONE
box: the recipe of gamd_water_minimize_lbfgs in include/gamd_hip.h decision by decision, with F and U from
tests/water_classical_ref.py, SETTLE, the projection and the wrap from tests/water_minimize_ref.py and the two-loop recursion
from tests/lbfgs_ref.py.  The iterate lives on the manifold of rigid molecules: F is the classical force projected onto the
tangent space of the bond constraints at x, a trial is x + t d carried back onto the manifold by SETTLE, s is the difference
of the positions SETTLE gives (with its second-order correction) and y = F - F_t, each projected at its own point.  The ring's
vectors are used as stored, without vector transport; the sufficient-decrease test guards descent.  The sums are numpy's (the
device adds slices, threads and blocks in its own fixed order): the tests bound that difference by the replay's own spread
under molecule permutations and under a 2^-50 relative perturbation of the force.  ``form``: "ring" or "gram", as in lbfgs_ref.
Not an oracle module: nothing here was compared with OpenMM, whose L-BFGS treats the constraints by restraints."""
import numpy as np

import lbfgs_ref as lr
import water_classical_ref as wr
import water_minimize_ref as wm

CONVERGED, MAX_ITER, FAILED, LINE_SEARCH = lr.CONVERGED, lr.MAX_ITER, lr.FAILED, lr.LINE_SEARCH
DEFAULTS = dict(lr.DEFAULTS)
_norms = lr._norms


def minimize(x, box, species, w, tolerance, max_iter=10000, length_per_nm=0.0, r_oh=None, r_hh=None, trace=None, perturb=None,
             form="ring", **par):
    """x [N, 3] (fp32 as the library reads it, or float64), atoms O,H,H; box scalar or [3]; w a water_classical_ref.Water.
    Returns a dict: x (float64, unwrapped, rigid: the last accepted point; the input widened for a failed box), state,
    evaluations (behind the first), accepted, skipped, resets, u0, rms0, u, rms, fmax (the largest per-atom |F_c,i|).
    ``trace``: a list that receives one dict per evaluation behind the first: u, rms (of the trial), accepted, fs (F.s), u_from,
    smax (the longest per-atom displacement behind the molecule's clamp, in front of SETTLE), smax_settled (the longest per-atom
    |x_t - x|), x (the trial positions, kept only where accepted, else None).  ``perturb``: a numpy Generator; every raw force
    component is multiplied by 1 + 2^-50 xi, xi uniform in [-1, 1]."""
    c = dict(DEFAULTS)
    c.update({k: v for k, v in par.items() if v})
    unknown = set(c) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown L-BFGS constants {sorted(unknown)}")
    direction = {"ring": lr._direction_ring, "gram": lr._direction_gram}[form]
    unit = (float(np.float32(length_per_nm)) / 10.0) if length_per_nm else 1.0
    r_oh = wm.TIP3P_R_OH * unit if not r_oh else float(r_oh)
    r_hh = wm.TIP3P_R_HH * unit if not r_hh else float(r_hh)
    x_in = np.array(x, dtype=np.float64)
    n = x_in.shape[0]

    def evaluate(p):
        """(F projected at p, U)"""
        with np.errstate(all="ignore"):
            ev = wr.evaluate(p, box, species, w, length_per_nm)
            F = ev["forces"]
            if perturb is not None:
                F = F * (1.0 + 2.0 ** -50 * perturb.uniform(-1.0, 1.0, F.shape))
            return wm.project(p, F), ev["energy"]

    # 0., 1. the start on the exact geometry
    x = wm.settle(x_in, x_in, r_oh, r_hh)
    F, U = evaluate(x)
    ff = float((F * F).sum())
    rms = float(np.sqrt(ff / (3.0 * n)))
    out = dict(u0=U, rms0=rms, evaluations=0, accepted=0, skipped=0, resets=0)

    def done(state):
        with np.errstate(all="ignore"):
            out.update(x=x_in if state == FAILED else x, state=state, u=U, rms=rms, fmax=float(_norms(F).max()))
        return out

    if not (np.isfinite(U) and np.isfinite(ff)):
        return done(FAILED)
    if rms <= tolerance:
        return done(CONVERGED)
    ring = []
    while True:
        # 2. the direction
        d = direction(F, ring) if ring else F * (c["max_step"] / float(_norms(F).max()))
        t, rejected = 1.0, 0
        while True:
            # 3. the trial: one clamp factor per molecule, SETTLE, and s as the positions give it
            s = t * d
            big = np.repeat(_norms(s).reshape(-1, 3).max(axis=1), 3)
            clamp = big > c["max_step"]
            scale = np.where(clamp, c["max_step"] / np.where(clamp, big, 1.0), 1.0)
            s = np.where(clamp[:, None], scale[:, None] * s, s)
            smax = float(_norms(s).max())
            xt = wm.settle(x, x + s, r_oh, r_hh)
            s = xt - x
            # 4. one evaluation, counted whatever follows
            Ft, Ut = evaluate(xt)
            out["evaluations"] += 1
            with np.errstate(all="ignore"):
                fs = float((F * s).sum())
                fft = float((Ft * Ft).sum())
                rms_t = float(np.sqrt(fft / (3.0 * n)))
            # 5. sufficient decrease
            ok = fs > 0.0 and bool(np.isfinite(Ut)) and Ut <= U - c["c1"] * fs
            if trace is not None:
                with np.errstate(all="ignore"):
                    trace.append(dict(u=Ut, rms=rms_t, accepted=ok, fs=fs, u_from=U, smax=smax, smax_settled=float(_norms(s).max()),
                                      x=xt if ok else None))
            if ok:
                break
            if out["evaluations"] == max_iter:                  # 7.
                return done(MAX_ITER)
            rejected += 1
            if rejected >= c["max_ls"] or not fs > 0.0:         # the search has failed
                if not ring:
                    return done(LINE_SEARCH)
                ring = []
                out["resets"] += 1
                d = F * (c["max_step"] / float(_norms(F).max()))
                t, rejected = 1.0, 0
            else:
                t = t / 2.0
        # 6. the step is taken
        y = F - Ft
        sy, ss, yy = float((s * y).sum()), float((s * s).sum()), float((y * y).sum())
        if sy > c["curv"] * float(np.sqrt(ss * yy)):
            ring.append((s, y))
            if len(ring) > c["m"]:
                ring.pop(0)
        else:
            out["skipped"] += 1
        x, F, U, rms = xt, Ft, Ut, rms_t
        out["accepted"] += 1
        if rms <= tolerance:
            return done(CONVERGED)
        if out["evaluations"] == max_iter:
            return done(MAX_ITER)
