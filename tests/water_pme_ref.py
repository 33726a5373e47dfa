"""Float64 host reference of smooth particle-mesh Ewald for the water classical potential (gamd_amd/csrc/water_pme.hip,
gamd_water_pme; Essmann et al. 1995): `recip` sums the reciprocal part of arbitrary charges z q_H on ONE box with numpy.fft —
B-spline weights by Essmann's recursion, the spread quantised to 2^-50 q_H per term as the device quantises it, the influence
function exp(-pi^2 |m~|^2 / alpha^2) / (|m~|^2 B(m)), the analytic gradient — and `evaluate` puts it in the place of the plain
sum's reciprocal part in water_classical_ref.evaluate (3-site) or water_msite_ref.evaluate (M-site, on its sites): pair,
exclusion, self and Lennard-Jones terms are theirs, only u_recip and the reciprocal force are replaced.  Besides every sum the
sums of the absolute terms that bound a difference in summation order, in the transform and in exp:
    abs_recip      = (C / 2 pi V) sum_m |G(m)| (sum_j |q_j|)^2
    abs_f[i, d]    = |q_i| (n_d / L_d) sum_stencil |theta'_d theta theta| (C / pi V) sum_m |G(m)| sum_j |q_j|
(through the M-site's redistribution for the 4-site form: abs_f[O] = (1 - 2 w) abs_f[M], abs_f[H] = abs_f[H] + w abs_f[M]).
Not an oracle module: nothing here was compared with OpenMM."""
import numpy as np

import classical_ref as cr
import water_classical_ref as wr
import water_msite_ref as w4

PI = wr.PI
QUANT = 2.0 ** 50
LENGTHS = (8, 16, 32, 64, 128)


def raise_order(w, th, k):
    """one step of Essmann's recursion, eq. 4.1: th [..., k - 1] of order k - 1 -> [..., k] of order k"""
    div = 1.0 / (k - 1)
    out = np.zeros(th.shape[:-1] + (k,))
    out[..., k - 1] = (div * w) * th[..., k - 2]
    for l in range(1, k - 1):
        out[..., k - l - 1] = div * ((w + l) * th[..., k - l - 2] + ((k - l) - w) * th[..., k - l - 1])
    out[..., 0] = (div * (1.0 - w)) * th[..., 0]
    return out


def spline(w, p):
    """theta [..., p] and d theta / du [..., p] of the cardinal B-spline of order p at the stencil of offset w in [0, 1):
    entry j belongs to the grid point floor(u) + j - (p - 1), theta_j = M_p(w + p - 1 - j)"""
    w = np.asarray(w, dtype=np.float64)
    th = np.stack([1.0 - w, w], axis=-1)
    for k in range(3, p):
        th = raise_order(w, th, k)
    dth = np.zeros(w.shape + (p,))
    dth[..., 0] = -th[..., 0]
    for l in range(1, p - 1):
        dth[..., l] = th[..., l - 1] - th[..., l]
    dth[..., p - 1] = th[..., p - 2]
    return raise_order(w, th, p), dth


def moduli(p, n):
    """|sum_{k=0}^{p-2} M_p(k + 1) exp(2 pi i m k / n)|^2, m in [0, n): positive for even p, zero at m = n / 2 for odd p"""
    th, _ = spline(np.float64(0.0), p)                       # th[j] = M_p(p - 1 - j)
    k = np.arange(p - 1)
    mk = th[p - 2 - k]
    arg = 2.0 * PI * ((np.arange(n)[:, None] * k[None, :]) % n) / n
    re, im = (mk * np.cos(arg)).sum(axis=1), (mk * np.sin(arg)).sum(axis=1)
    return re * re + im * im


def stencil(pos, box, grid, p):
    """per atom and axis: wrapped grid indices [N, 3, p], theta and theta' [N, 3, p]"""
    L, n = cr.edges(box), np.asarray(grid, dtype=np.int64)
    q = np.asarray(pos, dtype=np.float64) / L
    u = (q - np.floor(q)) * n
    u = np.where(u < n, u, 0.0)                              # s == 1: the image s = 0
    base = np.floor(u)
    th, dth = spline(u - base, p)
    idx = (base.astype(np.int64)[..., None] + np.arange(p) - (p - 1)) % n[None, :, None]
    return idx, th, dth


def influence(box, grid, p, alpha):
    """G(m) [nx, ny, nz], G(0) = 0; m_d taken in (-n/2, n/2]"""
    L = cr.edges(box)
    f = []
    for d, n in enumerate(grid):
        i = np.arange(n)
        f.append(np.where(i <= n // 2, i, i - n) / L[d])
    m2 = (f[0][:, None, None] ** 2 + f[1][None, :, None] ** 2) + f[2][None, None, :] ** 2
    B = (moduli(p, grid[0])[:, None, None] * moduli(p, grid[1])[None, :, None]) * moduli(p, grid[2])[None, None, :]
    m2s = np.where(m2 > 0, m2, 1.0)
    return np.where(m2 > 0, np.exp(-((PI * PI) / (alpha * alpha)) * m2s) / (m2s * B), 0.0)


def recip(pos, box, z, q_h, alpha, coul, grid, order):
    """One box: charges z q_h at pos [N, 3] (any image).  u_recip, f_recip [N, 3] per length unit, abs_recip, abs_f [N, 3], and
    the integer grid `quanta` the device must hold bit for bit after its spread."""
    if order not in (4, 6) or any(g not in LENGTHS for g in grid):
        raise ValueError("order 4 or 6, grid lengths in %r" % (LENGTHS,))
    L, n = cr.edges(box), np.asarray(grid, dtype=np.int64)
    z = np.asarray(z, dtype=np.float64)
    V = (L[0] * L[1]) * L[2]
    idx, th, dth = stencil(pos, box, grid, order)
    ix, iy, iz = idx[:, 0, :, None, None], idx[:, 1, None, :, None], idx[:, 2, None, None, :]
    tx, ty, tz = th[:, 0, :, None, None], th[:, 1, None, :, None], th[:, 2, None, None, :]
    dx, dy, dz = dth[:, 0, :, None, None], dth[:, 1, None, :, None], dth[:, 2, None, None, :]
    terms = (z[:, None, None, None] * tx) * (ty * tz)
    quanta = np.zeros(tuple(grid), dtype=np.int64)
    np.add.at(quanta, (ix, iy, iz), np.rint(terms * QUANT).astype(np.int64))
    Q = quanta.astype(np.float64) * (1.0 / QUANT)
    G = influence(box, grid, order, alpha)
    Qh = np.fft.fftn(Q)
    S = (G * (Qh.real * Qh.real + Qh.imag * Qh.imag)).sum()
    phi = np.fft.ifftn(G * Qh).real * float(np.prod(n))
    ph = phi[ix, iy, iz]                                     # [N, p, p, p]
    g = np.stack([((dx * ty) * tz * ph).sum(axis=(1, 2, 3)), ((tx * dy) * tz * ph).sum(axis=(1, 2, 3)),
                  ((tx * ty) * dz * ph).sum(axis=(1, 2, 3))], axis=1)
    ag = np.stack([np.abs((dx * ty) * tz).sum(axis=(1, 2, 3)), np.abs((tx * dy) * tz).sum(axis=(1, 2, 3)),
                   np.abs((tx * ty) * dz).sum(axis=(1, 2, 3))], axis=1)
    scale = n / L
    sum_abs_q = q_h * np.abs(z).sum()
    f = -((coul / (PI * V)) * (q_h * q_h)) * z[:, None] * scale[None, :] * g
    abs_f = (q_h * np.abs(z))[:, None] * scale[None, :] * ag * ((coul / (PI * V)) * np.abs(G).sum() * sum_abs_q)
    return dict(u_recip=(coul / (2.0 * PI * V)) * (q_h * q_h) * S, f_recip=f,
                abs_recip=(coul / (2.0 * PI * V)) * np.abs(G).sum() * sum_abs_q * sum_abs_q, abs_f=abs_f, quanta=quanta)


def evaluate(x, box, species, wat, grid, order, w=None, length_per_nm=0.0):
    """Water in ONE box with the reciprocal part by PME: w None the 3-site form of water_classical_ref.evaluate, else the M-site
    form of water_msite_ref.evaluate with the hydrogens' weight w (w = 0.0 takes the same path and gives the 3-site arrays).
    Returns that module's dict with u_recip, forces, energy replaced, and abs_recip, abs_f [N, 3] (per component) the PME sums
    above; f_recip [N, 3] is the PME reciprocal force on the atoms in kJ/mol/nm."""
    ln = float(np.float32(length_per_nm)) if length_per_nm else 10.0
    o = np.asarray(species).reshape(-1) != 0
    n = o.shape[0]
    z = np.where(o, -2.0, 1.0)
    mol = np.arange(n) // 3
    # the pair, exclusion, self and Lennard-Jones terms, with the shortest k-vector list there is: its reciprocal part is removed
    if w is None:
        out, pos, w_h = wr.evaluate(x, box, species, wat, length_per_nm, n2max=1), np.asarray(x, dtype=np.float64), 0.0
    else:
        out, pos, w_h = w4.evaluate(x, box, species, wat, w, length_per_nm, n2max=1), w4.sites(x, box, w), float(w)
    ew = wr.ewald(pos, box, z * wat.q_h, mol[:, None] == mol[None, :], wat.alpha, wat.r_cut, wat.k_cut, wat.coulomb_const * ln, 1)
    rec = recip(pos, box, z, wat.q_h, wat.alpha, wat.coulomb_const * ln, grid, order)

    def to_atoms(fs):                                        # the M-site's redistribution (the identity for w = 0)
        F = fs.copy()
        F[0::3] = (1.0 - 2.0 * w_h) * fs[0::3]
        for k in (1, 2):
            F[k::3] = fs[k::3] + w_h * fs[0::3]
        return F

    out["f_recip"] = to_atoms(rec["f_recip"]) * ln
    out["forces"] = out["forces"] + to_atoms(rec["f_recip"] - ew["f_recip"]) * ln
    out["u_recip"], out["abs_recip"] = rec["u_recip"], rec["abs_recip"]
    out["abs_f"] = to_atoms(rec["abs_f"]) * ln
    out["energy"] = ((out["u_coul"] + out["u_recip"]) + out["u_self"]) + out["u_lj"]
    out["abs_energy"] = out["abs_real"] + out["abs_recip"] + abs(out["u_self"]) + out["abs_lj"]
    out["quanta"] = rec["quanta"]
    return out
