"""Float64 host replay of the L-BFGS energy minimiser (gamd_amd/csrc/lbfgs.hip) on ONE box, with F
and U from tests/classical_ref.py and the recipe of include/gamd_hip.h spelled out decision by decision: a limited-memory
quasi-Newton direction from a ring of at most m pairs (s, y), a backtracking line search on the sufficient-decrease condition,
FIRE's per-atom clamp on every trial displacement.  The sums are numpy's (the device adds slices, threads and blocks in its own
fixed order): the tests bound that difference by the replay's own spread under atom permutations.  ``form``: "ring" runs the
two-loop recursion on the ring's vectors; "gram" runs it on scalars alone, the inner products of the ring's vectors with each
other and with F, and forms d as one linear combination at the end — the arrangement of the device, the same numbers but for
rounding.  Not an oracle module: nothing here was compared with OpenMM, whose line search and stopping rule are its own."""
import numpy as np

import classical_ref as cr

CONVERGED, MAX_ITER, FAILED, LINE_SEARCH = 0, 1, 2, 3
DEFAULTS = dict(m=6, c1=1.0e-4, max_ls=20, curv=1.0e-10, max_step=0.1)


def _norms(a):
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def _direction_ring(F, ring):
    """d = H F by the two-loop recursion over the ring (oldest first), H0 = s.y / y.y of the newest pair"""
    q = F.copy()
    alpha = [0.0] * len(ring)
    for i in range(len(ring) - 1, -1, -1):
        s, y = ring[i]
        alpha[i] = float((s * q).sum()) / float((s * y).sum())
        q = q - alpha[i] * y
    s, y = ring[-1]
    r = (float((s * y).sum()) / float((y * y).sum())) * q
    for i in range(len(ring)):
        s, y = ring[i]
        beta = float((y * r).sum()) / float((s * y).sum())
        r = r + (alpha[i] - beta) * s
    return r


def _direction_gram(F, ring):
    """the same recursion on the coefficients of d over the basis {s_j}, {y_j}, F: only inner products are touched"""
    k = len(ring)
    S = [p[0] for p in ring]
    Y = [p[1] for p in ring]
    sy = np.array([[float((S[i] * Y[j]).sum()) for j in range(k)] for i in range(k)])
    yy = np.array([[float((Y[i] * Y[j]).sum()) for j in range(k)] for i in range(k)])
    fs = np.array([float((F * S[i]).sum()) for i in range(k)])
    fy = np.array([float((F * Y[i]).sum()) for i in range(k)])
    cy = np.zeros(k)                                            # q = F + sum cy_j y_j
    alpha = np.zeros(k)
    for i in range(k - 1, -1, -1):
        sq = fs[i]
        for j in range(k):
            sq = sq + cy[j] * sy[i, j]
        alpha[i] = sq / sy[i, i]
        cy[i] = cy[i] - alpha[i]
    h0 = sy[k - 1, k - 1] / yy[k - 1, k - 1]
    cf = h0                                                     # r = cf F + sum cy_j y_j + sum cs_j s_j
    cy = h0 * cy
    cs = np.zeros(k)
    for i in range(k):
        yr = cf * fy[i]
        for j in range(k):
            yr = yr + cy[j] * yy[i, j]
        for j in range(k):
            yr = yr + cs[j] * sy[j, i]
        beta = yr / sy[i, i]
        cs[i] = cs[i] + (alpha[i] - beta)
    d = cf * F
    for j in range(k):
        d = d + cs[j] * S[j]
    for j in range(k):
        d = d + cy[j] * Y[j]
    return d


def minimize(x, box, lj, tolerance, max_iter=10000, length_per_nm=0.0, trace=None, form="ring", **par):
    """x [N, 3] (fp32 as the library reads it, or float64), box scalar or [3].  Returns a dict: x (float64, unwrapped: the last
    accepted point), state, evaluations (pair evaluations behind the first), accepted, skipped (pairs the curvature test kept
    out of the ring), resets (line searches that failed with a history and emptied it), u0, rms0, u, rms, fmax (the largest
    per-atom |F_i|).  ``trace``: a list that receives one dict per evaluation behind the first: u, rms (of the trial), accepted,
    fs (F.s), u_from (U of the point the trial left), smax (the longest per-atom displacement as step 3 forms it, in front of
    the addition to x)."""
    c = dict(DEFAULTS)
    c.update({k: v for k, v in par.items() if v})
    unknown = set(c) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown L-BFGS constants {sorted(unknown)}")
    direction = {"ring": _direction_ring, "gram": _direction_gram}[form]
    x = np.array(x, dtype=np.float64)
    n = x.shape[0]
    ev = cr.evaluate(x, box, lj, length_per_nm)
    F, U = ev["forces"], ev["energy"]
    ff = float((F * F).sum())
    rms = float(np.sqrt(ff / (3.0 * n)))
    out = dict(u0=U, rms0=rms, evaluations=0, accepted=0, skipped=0, resets=0)

    def done(state):
        out.update(x=x, state=state, u=U, rms=rms, fmax=float(_norms(F).max()))
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
            # 3. the trial displacement, clamped per atom; s is what the evaluation sees: the difference of the positions
            s = t * d
            nrm = _norms(s)
            big = nrm > c["max_step"]
            scale = np.where(big, c["max_step"] / np.where(big, nrm, 1.0), 1.0)
            s = np.where(big[:, None], s * scale[:, None], s)
            smax = float(_norms(s).max())
            xt = x + s
            s = xt - x
            # 4. one evaluation, counted whatever follows
            ev = cr.evaluate(xt, box, lj, length_per_nm)
            Ft, Ut = ev["forces"], ev["energy"]
            out["evaluations"] += 1
            fs = float((F * s).sum())
            fft = float((Ft * Ft).sum())
            rms_t = float(np.sqrt(fft / (3.0 * n)))
            # 5. sufficient decrease
            ok = fs > 0.0 and bool(np.isfinite(Ut)) and Ut <= U - c["c1"] * fs
            if trace is not None:
                trace.append(dict(u=Ut, rms=rms_t, accepted=ok, fs=fs, u_from=U, smax=smax))
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
