"""Float64 host reference of the water classical observer (gamd_amd/csrc/water_classical.hip): a plain Ewald sum for
arbitrary point charges and an exclusion mask on ONE box (`ewald`), and on top of it the 3-site water potential of
include/gamd_hip.h (`evaluate`: charges q_H / -2 q_H by species, molecule = index / 3, O-O Lennard-Jones by
tests/classical_ref.py's pair term), with the operations of a term in the order DESIGN.md section 4.10 spells out.  The sums are
numpy's: the tests bound the difference by the sum of the absolute terms, which this module returns next to every sum.
erfc / erf are scipy's, sin / cos of 2 pi p are taken of p - rint(p) (the device calls sincospi(2 p)).  Not an oracle module:
nothing here was compared with OpenMM or with a particle-mesh sum."""
import numpy as np
from scipy.special import erf, erfc

import classical_ref as cr

PI = 3.141592653589793
CHUNK_BYTES = 100e6


class Water:
    """parameters as gamd_water_configure takes them"""

    def __init__(self, q_h=0.417, sigma_o=3.15075, epsilon_o=0.635968, r_cut=9.5, r_switch=0.0, shift=False, ewald_tol=1e-10,
                 alpha=None, k_cut=None, coulomb_const=138.935456):
        self.q_h, self.r_cut = float(q_h), float(r_cut)
        self.lj = cr.LJ(sigma=sigma_o, epsilon=epsilon_o, r_cut=r_cut, r_switch=r_switch, shift=shift)
        root = float(np.sqrt(-np.log(float(ewald_tol))))
        self.alpha = root / self.r_cut if alpha is None else float(alpha)
        self.k_cut = 2.0 * self.alpha * root if k_cut is None else float(k_cut)
        self.coulomb_const = float(coulomb_const)

    def kwargs(self):
        return dict(q_h=self.q_h, sigma_o=self.lj.sigma, epsilon_o=self.lj.epsilon, r_cut=self.r_cut, r_switch=self.lj.r_switch,
                    shift=self.lj.shift, alpha=self.alpha, k_cut=self.k_cut, coulomb_const=self.coulomb_const)


def kvectors(n2max):
    """one of each +-n with 0 < |n|^2 <= n2max (first non-zero component positive), sorted by (|n|^2, nx, ny, nz): int [K, 3]"""
    m = int(np.floor(np.sqrt(n2max)))
    g = np.stack(np.meshgrid(np.arange(0, m + 1), np.arange(-m, m + 1), np.arange(-m, m + 1), indexing="ij"), -1).reshape(-1, 3)
    n2 = (g * g).sum(axis=1)
    lead = np.where(g[:, 0] != 0, g[:, 0], np.where(g[:, 1] != 0, g[:, 1], g[:, 2]))
    g, n2 = g[(n2 > 0) & (n2 <= n2max) & (lead > 0)], n2[(n2 > 0) & (n2 <= n2max) & (lead > 0)]
    order = np.lexsort((g[:, 2], g[:, 1], g[:, 0], n2))
    return g[order].astype(np.int64)


def list_n2max(k_cut, lmax):
    """|n|^2 bound of the list the library builds for a longest edge lmax (a few ulp up; the weight decides per box)"""
    m = k_cut * float(lmax) / 6.283185307179586
    return int(np.floor(m * m * (1.0 + 1e-12)))


def ewald(x, box, q, excl, alpha, r_cut, k_cut=None, coul=1.0, n2max=None):
    """One box: x [N, 3], box scalar or [3], charges q [N], excl [N, N] bool (pairs that take the erf branch whatever r is;
    symmetric), Coulomb constant `coul` in energy * length / charge^2.  The k-vector list is every n with |n|^2 <= n2max (default:
    list_n2max(k_cut, longest edge)); k_cut None: the whole list carries weight.  Forces per length unit.  Returns a dict:
    forces [N, 3] (f_pair + f_recip), f_pair, f_recip, u_real, u_excl, u_recip, u_self, pairs (non-excluded pairs inside r_cut),
    sum_q, and the sums of absolute terms: abs_real = sum_{i<j} |u_real| + |u_excl|, abs_recip = (4 pi C / V) sum_k A (sum |q|)^2,
    abs_f [N] = sum_j |F_ij| + (8 pi C / V) |q_i| sum_k A |k| sum_j |q_j|; near = non-excluded pairs with |r - r_cut| <= 1e-12 r_cut;
    n_k, and tail = the largest weight exp(-k^2 / 4 alpha^2) just outside the weighted set (how far the k sum is converged)."""
    xd, L, q = np.asarray(x, dtype=np.float64), cr.edges(box), np.asarray(q, dtype=np.float64)
    n = xd.shape[0]
    d, r2 = cr.min_image(xd, box)
    off = ~np.eye(n, dtype=bool)
    ex = np.asarray(excl, dtype=bool) & off
    real = off & ~ex & (r2 < r_cut * r_cut)
    act = real | ex
    r2s = np.where(act, r2, 1.0)
    r, ir2 = np.sqrt(r2s), 1.0 / r2s
    qq = coul * (q[:, None] * q[None, :])
    ar = alpha * r
    gs = ((2.0 * alpha) / np.sqrt(PI)) * np.exp(-(ar * ar))
    t_ex, t_re = erf(ar) / r, erfc(ar) / r
    u = np.where(ex, -(qq * t_ex), np.where(real, qq * t_re, 0.0))
    fs = np.where(ex, (qq * (gs - t_ex)) * ir2, np.where(real, (qq * (t_re + gs)) * ir2, 0.0))
    fij = fs[..., None] * d
    f_pair = fij.sum(axis=1)
    abs_f = np.sqrt((fij * fij).sum(axis=-1)).sum(axis=1)
    iu = np.triu_indices(n, 1)
    rr = np.sqrt(r2[iu])
    near = int(((np.abs(rr - r_cut) <= 1e-12 * r_cut) & ~ex[iu]).sum())

    # reciprocal space
    V = (L[0] * L[1]) * L[2]
    if n2max is None:
        n2max = list_n2max(k_cut, L.max())
    kv = kvectors(n2max).astype(np.float64)
    s = (xd - L * np.floor(xd / L)) / L                      # wrapped into [0, L) first, as the device does
    sum_abs_q = np.abs(q).sum()
    u_rec, abs_rec, g, abs_g, tail = 0.0, 0.0, np.zeros((n, 3)), 0.0, 0.0
    step = max(1, int(CHUNK_BYTES / (8.0 * n)))
    inv_4a2 = 1.0 / (4.0 * (alpha * alpha))
    for c0 in range(0, kv.shape[0], step):
        nn = kv[c0:c0 + step]
        ph = (nn[:, 0:1] * s[None, :, 0] + nn[:, 1:2] * s[None, :, 1]) + nn[:, 2:3] * s[None, :, 2]      # [k, N]
        ph = ph - np.rint(ph)                                # exact: sincospi(2 p) has the period 1 in p
        sn, cs = np.sin((2.0 * PI) * ph), np.cos((2.0 * PI) * ph)
        s_re, s_im = (q[None, :] * cs).sum(axis=1), -(q[None, :] * sn).sum(axis=1)
        kk = (2.0 * PI) * (nn / L[None, :])
        k2 = (kk[:, 0] * kk[:, 0] + kk[:, 1] * kk[:, 1]) + kk[:, 2] * kk[:, 2]
        w = np.exp(-(k2 * inv_4a2))
        inside = np.ones(k2.shape, dtype=bool) if k_cut is None else k2 <= k_cut * k_cut
        A = np.where(inside, w / k2, 0.0)
        if (~inside).any():
            tail = max(tail, float(w[~inside].max()))
        u_rec += (A * (s_re * s_re + s_im * s_im)).sum()
        abs_rec += (A * (sum_abs_q * sum_abs_q)).sum()
        wk = A[:, None] * (s_re[:, None] * sn + s_im[:, None] * cs)                                      # [k, N]
        g += wk.T @ nn
        abs_g += (A * np.sqrt(k2)).sum()
    pref = ((8.0 * PI) * coul) / V
    f_rec = ((pref * q)[:, None] * ((2.0 * PI) / L)[None, :]) * g
    abs_f = abs_f + pref * np.abs(q) * sum_abs_q * abs_g
    return dict(forces=f_pair + f_rec, f_pair=f_pair, f_recip=f_rec,
                u_real=0.5 * np.where(real, u, 0.0).sum(), u_excl=0.5 * np.where(ex, u, 0.0).sum(),
                u_recip=(((4.0 * PI) * coul) / V) * u_rec, u_self=-(((coul * alpha) / np.sqrt(PI)) * (q * q).sum()),
                pairs=0.5 * float(real.sum()), sum_q=float(q.sum()), abs_real=0.5 * np.abs(u).sum(),
                abs_recip=(((4.0 * PI) * coul) / V) * abs_rec, abs_f=abs_f, near=near, n_k=int(kv.shape[0]), tail=tail, real_mask=real)


def evaluate(x, box, species, w, length_per_nm=0.0, n2max=None):
    """3-site water in ONE box: x [N, 3] (fp32 positions as the device reads them, or float64), species [N] (O != 0), w a Water.
    Energies kJ/mol, forces kJ/mol/nm.  Returns ewald()'s dict with u_coul = u_real + u_excl, u_lj, abs_lj, energy, abs_energy
    added and forces / abs_f including the O-O Lennard-Jones term and scaled by the length unit.  n2max: the list the LIBRARY
    built (the longest edge of all boxes of the call); default: this box's own."""
    ln = float(np.float32(length_per_nm)) if length_per_nm else 10.0
    o = np.asarray(species).reshape(-1) != 0
    n = o.shape[0]
    q = np.where(o, -2.0 * w.q_h, w.q_h)
    mol = np.arange(n) // 3
    out = ewald(x, box, q, mol[:, None] == mol[None, :], w.alpha, w.r_cut, w.k_cut, w.coulomb_const * ln, n2max)
    d, r2 = cr.min_image(x, box)
    m = out.pop("real_mask") & (o[:, None] & o[None, :])
    u, ru = w.lj.terms(np.where(m, r2, 1.0))
    u, ru = np.where(m, u, 0.0), np.where(m, ru, 0.0)
    fij = np.where(m, -(ru * (1.0 / np.where(m, r2, 1.0))), 0.0)[..., None] * d
    out["u_lj"], out["abs_lj"] = 0.5 * u.sum(), 0.5 * np.abs(u).sum()
    out["u_coul"] = out["u_real"] + out["u_excl"]
    out["forces"] = (out["forces"] + fij.sum(axis=1)) * ln
    out["f_pair"] = (out["f_pair"] + fij.sum(axis=1)) * ln
    out["f_recip"] = out["f_recip"] * ln
    out["abs_f"] = (out["abs_f"] + np.sqrt((fij * fij).sum(axis=-1)).sum(axis=1)) * ln
    out["energy"] = ((out["u_coul"] + out["u_recip"]) + out["u_self"]) + out["u_lj"]
    out["abs_energy"] = out["abs_real"] + out["abs_recip"] + abs(out["u_self"]) + out["abs_lj"]
    return out
