"""Float64 host replay of the energy minimiser (gamd_amd/csrc/minimize.hip): FIRE in the semi-implicit
Euler form on ONE box, with F and U from tests/classical_ref.py and the scalar recipe of include/gamd_hip.h spelled out step by
step.  The sums are numpy's (the device adds slices, threads and blocks in its own fixed order): the tests bound that
difference by the replay's own spread under atom permutations.  Not an oracle module: nothing here was compared with OpenMM,
whose minimiser is L-BFGS."""
import numpy as np

import classical_ref as cr

CONVERGED, MAX_ITER, FAILED = 0, 1, 2
DEFAULTS = dict(dt_start=0.002, dt_max=0.02, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99, max_step=0.1)


def minimize(x, box, lj, tolerance, max_iter=10000, length_per_nm=0.0, trace=None, **fire):
    """x [N, 3] (fp32 as the library reads it, or float64), box scalar or [3].  Returns a dict: x (float64, unwrapped), state,
    iterations (position updates), u0, rms0, u, rms, fmax, dt.  ``trace``: a list that receives (U, rms) of every evaluation."""
    c = dict(DEFAULTS)
    c.update(fire)
    x = np.array(x, dtype=np.float64)
    n = x.shape[0]
    v = np.zeros_like(x)
    dt, alpha, n_pos = c["dt_start"], c["alpha_start"], 0
    out = dict(u0=None, rms0=None)
    it = 0
    while True:
        ev = cr.evaluate(x, box, lj, length_per_nm)
        F, U = ev["forces"], ev["energy"]
        ff, vf, vv = float((F * F).sum()), float((v * F).sum()), float((v * v).sum())
        rms = float(np.sqrt(ff / (3.0 * n)))
        if trace is not None:
            trace.append((U, rms))
        if it == 0:
            out.update(u0=U, rms0=rms)
        state = None
        if not (np.isfinite(U) and np.isfinite(ff)):
            state = FAILED
        elif rms <= tolerance:
            state = CONVERGED
        elif it == max_iter:
            state = MAX_ITER
        if state is not None:
            out.update(x=x, state=state, iterations=it, u=U, rms=rms, fmax=float(np.abs(F).max()), dt=dt)
            return out
        if vf > 0.0:
            v = (1.0 - alpha) * v + (alpha * np.sqrt(vv / ff)) * F
            if n_pos > c["n_min"]:
                dt = min(dt * c["f_inc"], c["dt_max"])
                alpha = alpha * c["f_alpha"]
            n_pos += 1
        else:
            v = np.zeros_like(x)
            alpha, dt, n_pos = c["alpha_start"], dt * c["f_dec"], 0
        v = v + dt * F
        dr = dt * v
        nrm = np.sqrt((dr[:, 0] * dr[:, 0] + dr[:, 1] * dr[:, 1]) + dr[:, 2] * dr[:, 2])
        big = nrm > c["max_step"]
        scale = np.where(big, c["max_step"] / np.where(big, nrm, 1.0), 1.0)
        dr = np.where(big[:, None], dr * scale[:, None], dr)
        x = x + dr
        it += 1


def wrap_fp32(x64, box):
    """the fp32 positions gamd_minimize returns: round to nearest, then the integrators' remainder (fmodf, sign of the edge)"""
    xf = np.asarray(x64, dtype=np.float64).astype(np.float32)
    L = np.broadcast_to(np.asarray(box, dtype=np.float32).reshape(-1), (3,))
    m = np.fmod(xf, L)
    return np.where((m != 0) & (m < 0), m + L, m).astype(np.float32)


def random_start(n, seed, box):
    """uniform random points in the box: what a user without a prepared start has"""
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) * float(box)).astype(np.float32)
