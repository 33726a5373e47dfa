"""Float64 host replay of the water energy minimiser (gamd_amd/csrc/water_minimize.hip): rigid-molecule
FIRE in the semi-implicit Euler form on ONE box, with F and U from tests/water_classical_ref.py, the closed-form unit-weight
SETTLE and the 3x3 projection of gamd_amd/csrc/gamd_wmin_dev.h in numpy (one molecule per row, the operations in the header's
order), the scalar recipe of include/gamd_hip.h step by step, and the wrap of the returned fp32 positions.  The sums are
numpy's (the device adds slices, threads and blocks in its own fixed order) and erfc / exp / sincospi are scipy's and numpy's:
the tests bound those differences by the replay's own spread under molecule permutations and under a 2^-50 relative
perturbation of the force.  Not an oracle module: nothing here was compared with OpenMM, whose minimiser is L-BFGS."""
import numpy as np

import water_classical_ref as wr

CONVERGED, MAX_ITER, FAILED = 0, 1, 2
DEFAULTS = dict(dt_start=0.002, dt_max=0.02, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99, max_step=0.1)
TIP3P_R_OH = 0.9572
TIP3P_R_HH = 2.0 * 0.9572 * float(np.sin(np.deg2rad(104.52) / 2.0))


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _unit(a):
    return (1.0 / np.sqrt(_dot(a, a)))[:, None] * a


def triangle(r_oh, r_hh):
    """the unit-weight canonical triangle of SETTLE: (ra, rb, rc)"""
    rc = 0.5 * r_hh
    t = float(np.sqrt(r_oh * r_oh - rc * rc))
    return (2.0 * t) / 3.0, t / 3.0, rc


def settle(x0, x1, r_oh, r_hh):
    """x0 [N, 3] the reference geometry, x1 [N, 3] the unconstrained new positions (atoms O,H,H): the constrained new positions
    with unit weights (the centroid of every molecule of x1 is kept).  A molecule it cannot place comes back not finite."""
    ra, rb, rc = triangle(r_oh, r_hh)
    x0, x1 = np.asarray(x0, dtype=np.float64).reshape(-1, 3, 3), np.asarray(x1, dtype=np.float64).reshape(-1, 3, 3)
    s = lambda v: v[:, None]
    with np.errstate(all="ignore"):
        b0, c0 = x0[:, 1] - x0[:, 0], x0[:, 2] - x0[:, 0]
        A1, B1, C1 = x1[:, 0] - x0[:, 0], x1[:, 1] - x0[:, 0], x1[:, 2] - x0[:, 0]
        d0 = (1.0 / 3.0) * ((A1 + B1) + C1)
        a1, b1, c1 = A1 - d0, B1 - d0, C1 - d0
        n0 = _cross(b0, c0)
        n1 = _cross(a1, n0)
        n2 = _cross(n0, n1)
        n0, n1, n2 = _unit(n0), _unit(n1), _unit(n2)
        b0x, b0y, c0x, c0y = _dot(b0, n1), _dot(b0, n2), _dot(c0, n1), _dot(c0, n2)
        a1z = _dot(a1, n0)
        b1x, b1y, b1z = _dot(b1, n1), _dot(b1, n2), _dot(b1, n0)
        c1x, c1y, c1z = _dot(c1, n1), _dot(c1, n2), _dot(c1, n0)
        sinphi = a1z / ra
        cosphi = np.sqrt(1.0 - sinphi * sinphi)
        sinpsi = (b1z - c1z) / ((2.0 * rc) * cosphi)
        cospsi = np.sqrt(1.0 - sinpsi * sinpsi)
        a2y, a2z = ra * cosphi, ra * sinphi
        b2x, b2y, b2z = -(rc * cospsi), -(rb * cosphi) - (rc * sinpsi) * sinphi, -(rb * sinphi) + (rc * sinpsi) * cosphi
        c2x, c2y, c2z = rc * cospsi, -(rb * cosphi) + (rc * sinpsi) * sinphi, -(rb * sinphi) - (rc * sinpsi) * cosphi
        alpha = (b2x * (b0x - c0x) + b0y * b2y) + c0y * c2y
        beta = (b2x * (c0y - b0y) + b0x * b2y) + c0x * c2y
        gamma = (b0x * b1y - b1x * b0y) + (c0x * c1y - c1x * c0y)
        a2b2 = alpha * alpha + beta * beta
        sint = (alpha * gamma - beta * np.sqrt(a2b2 - gamma * gamma)) / a2b2
        cost = np.sqrt(1.0 - sint * sint)
        a3x, a3y = -(a2y * sint), a2y * cost
        b3x, b3y = b2x * cost - b2y * sint, b2x * sint + b2y * cost
        c3x, c3y = c2x * cost - c2y * sint, c2x * sint + c2y * cost
        base = x0[:, 0] + d0
        out = np.stack([base + ((s(a3x) * n1 + s(a3y) * n2) + s(a2z) * n0),
                        base + ((s(b3x) * n1 + s(b3y) * n2) + s(b2z) * n0),
                        base + ((s(c3x) * n1 + s(c3y) * n2) + s(c2z) * n0)], axis=1)
    return out.reshape(-1, 3)


def project(x, u):
    """u [N, 3] (a force or a velocity per atom) without its components along the three bonds of every molecule of x: the
    orthogonal projection onto the tangent space of the constraints (unit weights)"""
    x, u = np.asarray(x, dtype=np.float64).reshape(-1, 3, 3), np.asarray(u, dtype=np.float64).reshape(-1, 3, 3)
    s = lambda v: v[:, None]
    with np.errstate(all="ignore"):
        r0, r1, r2 = x[:, 0] - x[:, 1], x[:, 0] - x[:, 2], x[:, 1] - x[:, 2]
        y0, y1, y2 = -_dot(r0, u[:, 0] - u[:, 1]), -_dot(r1, u[:, 0] - u[:, 2]), -_dot(r2, u[:, 1] - u[:, 2])
        a00, a01, a02 = 2.0 * _dot(r0, r0), _dot(r0, r1), -_dot(r0, r2)
        a11, a12, a22 = 2.0 * _dot(r1, r1), _dot(r1, r2), 2.0 * _dot(r2, r2)
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        inv_det = 1.0 / ((a00 * c00 + a01 * c01) + a02 * c02)
        g0 = ((c00 * y0 + c01 * y1) + c02 * y2) * inv_det
        g1 = ((c01 * y0 + c11 * y1) + c12 * y2) * inv_det
        g2 = ((c02 * y0 + c12 * y1) + c22 * y2) * inv_det
        out = np.stack([u[:, 0] + (s(g0) * r0 + s(g1) * r1), u[:, 1] + (s(g2) * r2 - s(g0) * r0), u[:, 2] - (s(g1) * r1 + s(g2) * r2)], axis=1)
    return out.reshape(-1, 3)


def projected_rms(x, box, species, w, length_per_nm=0.0):
    """(rms of the projected classical force over 3N components, U) at x"""
    ev = wr.evaluate(x, box, species, w, length_per_nm)
    F = project(x, ev["forces"])
    return float(np.sqrt((F * F).sum() / F.size)), ev["energy"]


def minimize(x, box, species, w, tolerance, max_iter=10000, length_per_nm=0.0, r_oh=None, r_hh=None, trace=None, perturb=None, snapshots=None,
             **fire):
    """x [N, 3] (fp32 as the library reads it, or float64), atoms O,H,H; box scalar or [3]; w a water_classical_ref.Water.
    Returns a dict: x (float64, unwrapped, rigid), state, iterations (position updates), u0, rms0, u, rms, fmax, dt.  ``trace``: a
    list that receives (U, rms) of every evaluation.  ``perturb``: a numpy Generator; every force component is multiplied by
    1 + 2^-50 xi, xi uniform in [-1, 1] (device erfc / exp / sincospi are not correctly rounded).  ``snapshots``: a dict whose
    keys are iteration numbers; each receives dict(x, u, rms) of the evaluation behind that many position updates."""
    c = dict(DEFAULTS)
    c.update(fire)
    unit = (float(np.float32(length_per_nm)) / 10.0) if length_per_nm else 1.0
    r_oh = TIP3P_R_OH * unit if not r_oh else float(r_oh)
    r_hh = TIP3P_R_HH * unit if not r_hh else float(r_hh)
    x = np.array(x, dtype=np.float64)
    x = settle(x, x, r_oh, r_hh)
    n = x.shape[0]
    v = np.zeros_like(x)
    dt, alpha, n_pos = c["dt_start"], c["alpha_start"], 0
    out = dict(u0=None, rms0=None)
    it = 0
    while True:
        with np.errstate(all="ignore"):
            ev = wr.evaluate(x, box, species, w, length_per_nm)
        F, U = ev["forces"], ev["energy"]
        if perturb is not None:
            F = F * (1.0 + 2.0 ** -50 * perturb.uniform(-1.0, 1.0, F.shape))
        F = project(x, F)
        v = project(x, v)
        ff, vf, vv = float((F * F).sum()), float((v * F).sum()), float((v * v).sum())
        rms = float(np.sqrt(ff / (3.0 * n)))
        if trace is not None:
            trace.append((U, rms))
        if it == 0:
            out.update(u0=U, rms0=rms)
        if snapshots is not None and it in snapshots:
            snapshots[it] = dict(x=x.copy(), u=U, rms=rms)
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
        big = np.repeat(nrm.reshape(-1, 3).max(axis=1), 3)      # one factor per molecule
        clamp = big > c["max_step"]
        scale = np.where(clamp, c["max_step"] / np.where(clamp, big, 1.0), 1.0)
        dr = np.where(clamp[:, None], scale[:, None] * dr, dr)
        x = settle(x, x + dr, r_oh, r_hh)
        it += 1


def wrap_fp32(x64, box):
    """the fp32 positions gamd_water_minimize returns (include/gamd_hip.h): per molecule and component, with the fp32 edge L,
    s = L floor(xO / L); xO - s < 0: s -= L; fp32(xO - s) >= L: s += L; O = max(fp32(xO - s), 0), H = fp32(xH - s)"""
    xm = np.asarray(x64, dtype=np.float64).reshape(-1, 3, 3)
    Lf = np.broadcast_to(np.asarray(box, dtype=np.float32).reshape(-1), (3,))
    L = Lf.astype(np.float64)
    xo = xm[:, 0]
    s = L * np.floor(xo / L)
    s = np.where(xo - s < 0.0, s - L, s)
    s = np.where((xo - s).astype(np.float32) >= Lf, s + L, s)
    out = (xm - s[:, None, :]).astype(np.float32)
    out[:, 0] = np.maximum(out[:, 0], np.float32(0.0))
    return out.reshape(-1, 3)


def bond_lengths(x):
    """[M, 3]: |O-H1|, |O-H2|, |H1-H2| of every molecule"""
    m = np.asarray(x, dtype=np.float64).reshape(-1, 3, 3)
    n = lambda d: np.sqrt((d * d).sum(axis=-1))
    return np.stack([n(m[:, 0] - m[:, 1]), n(m[:, 0] - m[:, 2]), n(m[:, 1] - m[:, 2])], axis=1)
