"""Float64 host reference of the classical observer (gamd_amd/csrc/classical.hip): the switched, shifted Lennard-Jones
potential of include/gamd_hip.h on all pairs of ONE box, with the pair term's operations in the order DESIGN.md section 4.9
spells out (the sums are numpy's: the tests bound the difference by the sum of the absolute terms, which this module returns
next to every sum).  Not an oracle module: nothing here was compared with OpenMM."""
import numpy as np


class LJ:
    """parameters as gamd_classical_configure takes them, and the constants the kernels derive from them"""

    def __init__(self, sigma=3.4, epsilon=0.238 * 4.184, r_cut=None, r_switch=None, shift=True):
        self.sigma, self.epsilon = float(sigma), float(epsilon)
        self.r_cut = 3.0 * self.sigma if r_cut is None else float(r_cut)
        self.r_switch = self.r_cut - self.sigma if r_switch is None else float(r_switch)
        self.shift = bool(shift)
        self.sig2 = self.sigma * self.sigma
        self.eps4, self.eps24 = 4.0 * self.epsilon, 24.0 * self.epsilon
        self.rc2 = self.r_cut * self.r_cut
        self.u0 = 0.0
        if self.shift:
            s2 = self.sig2 * (1.0 / self.rc2)
            s6 = (s2 * s2) * s2
            self.u0 = self.eps4 * (s6 * s6 - s6)
        self.switching = 0.0 < self.r_switch < self.r_cut
        self.inv_w = 1.0 / (self.r_cut - self.r_switch) if self.switching else 0.0

    def kwargs(self):
        return dict(sigma=self.sigma, epsilon=self.epsilon, r_cut=self.r_cut, r_switch=self.r_switch, shift=self.shift)

    def terms(self, r2):
        """(u, r u'(r)) of the squared distances r2 < r_cut^2 (array), by the kernel's operations"""
        r2 = np.asarray(r2, dtype=np.float64)
        ir2 = 1.0 / r2
        s2 = self.sig2 * ir2
        s6 = (s2 * s2) * s2
        s12 = s6 * s6
        u = self.eps4 * (s12 - s6) - self.u0
        ru = -(self.eps24 * ((s12 + s12) - s6))
        if self.switching:
            r = np.sqrt(r2)
            m = r > self.r_switch
            t = np.where(m, (r - self.r_switch) * self.inv_w, 0.0)
            t2, tm = t * t, t - 1.0
            S = 1.0 - (t2 * t) * ((6.0 * t - 15.0) * t + 10.0)
            dS = ((-30.0 * t2) * (tm * tm)) * self.inv_w
            ru = np.where(m, ru * S + ((u * dS) * r), ru)
            u = np.where(m, u * S, u)
        return u, ru

    def u(self, r):
        """u(r) and u'(r) of scalar or array distances, 0 at and beyond r_cut"""
        r = np.atleast_1d(np.asarray(r, dtype=np.float64))
        inside = r * r < self.rc2
        u, ru = self.terms(np.where(inside, r * r, 1.0))
        return np.where(inside, u, 0.0), np.where(inside, ru / r, 0.0)


def edges(box):
    """the fp32 box edges the library holds, widened: [3] float64"""
    return np.broadcast_to(np.asarray(box, dtype=np.float32).astype(np.float64).reshape(-1), (3,)).copy()


def min_image(x, box):
    """d [N, N, 3] = x_i - x_j - L rint((x_i - x_j) / L) and r2 [N, N] = (dx^2 + dy^2) + dz^2 in float64"""
    xd, L = np.asarray(x, dtype=np.float64), edges(box)
    d = xd[:, None, :] - xd[None, :, :]
    d = d - L * np.rint(d / L)
    return d, (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def evaluate(x, box, lj, length_per_nm=0.0):
    """One box: x [N, 3] (fp32 positions as the device reads them, or float64 for finite differences), box scalar or [3].
    Returns a dict: forces [N, 3] kJ/mol/nm, energy, virial, pairs, and the sums of absolute terms the tolerances refer to:
    abs_u = sum_{i<j} |u|, abs_ru = sum_{i<j} |r u'|, abs_f [N] = sum_j |F_ij| (kJ/mol/nm); near = pairs with
    |r - r_cut| <= 1e-12 r_cut (their side of the cutoff is not decided by the arithmetic)."""
    ln = float(np.float32(length_per_nm)) if length_per_nm else 10.0
    d, r2 = min_image(x, box)
    n = r2.shape[0]
    np.fill_diagonal(r2, np.inf)
    inside = r2 < lj.rc2
    u, ru = lj.terms(np.where(inside, r2, 1.0))
    u, ru = np.where(inside, u, 0.0), np.where(inside, ru, 0.0)
    fs = np.where(inside, -(ru * (1.0 / np.where(inside, r2, 1.0))), 0.0)
    fij = fs[..., None] * d                                  # per length unit
    r = np.sqrt(np.where(np.isfinite(r2), r2, 0.0))
    iu = np.triu_indices(n, 1)
    return dict(forces=fij.sum(axis=1) * ln, energy=0.5 * u.sum(), virial=0.5 * (-ru).sum(), pairs=0.5 * float(inside.sum()),
                abs_u=0.5 * np.abs(u).sum(), abs_ru=0.5 * np.abs(ru).sum(), abs_f=np.sqrt((fij * fij).sum(axis=-1)).sum(axis=1) * ln,
                near=int((np.abs(r[iu] - lj.r_cut) <= 1e-12 * lj.r_cut).sum()))


def force_error_sums(f, f_cl):
    """The five sums and the count of atoms left out of the cosine, as the device takes them, from f [N, 3] (fp32) and f_cl
    [N, 3] (float64) of ONE box: (sums [6], abs [5]) with abs the sums of the absolute terms of the first five."""
    g, c = np.asarray(f).astype(np.float64), np.asarray(f_cl, dtype=np.float64)
    dd = g - c
    a1 = (np.abs(dd[:, 0]) + np.abs(dd[:, 1])) + np.abs(dd[:, 2])
    sq = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
    nc = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    ng = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    out = (nc == 0.0) | (ng == 0.0)
    dot = (g[:, 0] * c[:, 0] + g[:, 1] * c[:, 1]) + g[:, 2] * c[:, 2]
    cos = np.where(out, 0.0, dot / np.where(out, 1.0, ng * nc))
    sums = np.array([a1.sum(), sq.sum(), cos.sum(), nc.sum(), ng.sum(), float(out.sum())])
    return sums, np.array([a1.sum(), sq.sum(), np.abs(cos).sum(), nc.sum(), ng.sum()])
