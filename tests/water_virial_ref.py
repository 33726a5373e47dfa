"""Float64 host reference of the molecular virial of the water classical potential (gamd_amd/csrc/water_virial.hip,
gamd_water_virial): the terms of include/gamd_hip.h on ONE box, on top of the existing references — forces, masks and sites
are water_msite_ref.evaluate's (which is water_classical_ref.evaluate for w = 0), the pair and k terms are formed by
water_classical_ref.ewald's operations.  Every sum comes with the sum of its absolute terms, which the tests' bounds refer
to.  `scaled` and `volume_derivative` are the independent check: W_mol = -dE/d lambda at lambda = 1 under a scaling of the box
edges and the molecules' centres of mass with the molecules kept rigid.  Not an oracle module: nothing here was compared with
OpenMM."""
import numpy as np
from scipy.special import erf, erfc

import classical_ref as cr
import water_classical_ref as wr
import water_msite_ref as wm

PI = wr.PI
COLUMNS = ("w_lj", "w_coul", "w_recip", "w_intra", "ke_com", "w_mol")
MASS_O, MASS_H = 15.99943, 1.007947


def molecule_offsets(x, box, mass_o=MASS_O, mass_h=MASS_H):
    """s_a = r_a - R_mol [N, 3] from the minimum-image vectors d_k = H_k - O alone: s_O = -(m_H / M)(d_1 + d_2), s_Hk = d_k + s_O"""
    xd, L = np.asarray(x, dtype=np.float64), cr.edges(box)
    o = xd[0::3]
    d1, d2 = xd[1::3] - o, xd[2::3] - o
    d1 = d1 - L * np.rint(d1 / L)
    d2 = d2 - L * np.rint(d2 / L)
    mu = mass_h / (mass_o + (mass_h + mass_h))
    s = np.zeros_like(xd)
    s[0::3] = -(mu * (d1 + d2))
    s[1::3] = d1 + s[0::3]
    s[2::3] = d2 + s[0::3]
    return s


def virial(x, box, species, wat, w=0.0, vel=None, mass_o=MASS_O, mass_h=MASS_H, length_per_nm=0.0, n2max=None):
    """ONE box: x [N, 3] (fp32 positions as the device reads them, or float64), atoms O,H,H; wat a water_classical_ref.Water;
    w the M-site's hydrogen weight (0: 3-site); vel [N, 3] in length unit / ps or None.  Returns a dict: the COLUMNS in kJ/mol,
    abs_<column> the sum of the absolute terms of each (abs_w_mol their sum over the four virial terms), and `ev`, the
    dictionary of water_msite_ref.evaluate (energies, forces)."""
    ln = float(np.float32(length_per_nm)) if length_per_nm else 10.0
    ev = wm.evaluate(x, box, species, wat, w, length_per_nm, n2max)
    xd, L = np.asarray(x, dtype=np.float64), cr.edges(box)
    o = np.asarray(species).reshape(-1) != 0
    n = o.shape[0]
    q = np.where(o, -2.0 * wat.q_h, wat.q_h)
    coul = wat.coulomb_const * ln
    mol = np.arange(n) // 3
    ex = (mol[:, None] == mol[None, :]) & ~np.eye(n, dtype=bool)
    real = ev["real_mask"]

    # pair terms on the charge sites, by ewald()'s operations: fs_coul r^2 is the bracket of its force scalar
    sx = wm.sites(x, box, w)
    _, r2 = cr.min_image(sx, box)
    r = np.sqrt(np.where(real | ex, r2, 1.0))
    qq = coul * (q[:, None] * q[None, :])
    ar = wat.alpha * r
    gs = ((2.0 * wat.alpha) / np.sqrt(PI)) * np.exp(-(ar * ar))
    wc = np.where(ex, qq * (gs - erf(ar) / r), np.where(real, qq * (erfc(ar) / r + gs), 0.0))

    # Lennard-Jones on the atoms' own O-O distances
    m = ev["lj_mask"]
    _, r2a = cr.min_image(x, box)
    _, ru = wat.lj.terms(np.where(m, r2a, 1.0))
    wl = np.where(m, -ru, 0.0)

    # reciprocal space: S(k), A(k) as ewald() forms them, times (1 - k^2 / (2 alpha^2))
    V = (L[0] * L[1]) * L[2]
    if n2max is None:
        n2max = wr.list_n2max(wat.k_cut, L.max())
    kv = wr.kvectors(n2max).astype(np.float64)
    s = (sx - L * np.floor(sx / L)) / L
    inv_4a2 = 1.0 / (4.0 * (wat.alpha * wat.alpha))
    sum_abs_q = np.abs(q).sum()
    w_rec, abs_rec = 0.0, 0.0
    step = max(1, int(wr.CHUNK_BYTES / (8.0 * n)))
    for c0 in range(0, kv.shape[0], step):
        nn = kv[c0:c0 + step]
        ph = (nn[:, 0:1] * s[None, :, 0] + nn[:, 1:2] * s[None, :, 1]) + nn[:, 2:3] * s[None, :, 2]
        ph = ph - np.rint(ph)
        sn, cs = np.sin((2.0 * PI) * ph), np.cos((2.0 * PI) * ph)
        s_re, s_im = (q[None, :] * cs).sum(axis=1), -(q[None, :] * sn).sum(axis=1)
        kk = (2.0 * PI) * (nn / L[None, :])
        k2 = (kk[:, 0] * kk[:, 0] + kk[:, 1] * kk[:, 1]) + kk[:, 2] * kk[:, 2]
        A = np.where(k2 <= wat.k_cut * wat.k_cut, np.exp(-(k2 * inv_4a2)) / k2, 0.0)
        fac = 1.0 - 2.0 * (k2 * inv_4a2)
        w_rec += ((A * (s_re * s_re + s_im * s_im)) * fac).sum()
        abs_rec += (A * (sum_abs_q * sum_abs_q) * np.abs(fac)).sum()
    pref = ((4.0 * PI) * coul) / V

    # the intramolecular correction about the centres of mass, and their kinetic energy
    so = molecule_offsets(x, box, mass_o, mass_h)
    sf = so * ev["forces"] / ln
    ke, M = 0.0, mass_o + (mass_h + mass_h)
    if vel is not None:
        v = np.asarray(vel, dtype=np.float64) / ln
        p = (mass_o * v[0::3] + mass_h * v[1::3]) + mass_h * v[2::3]
        ke = 0.5 * ((p * p).sum(axis=1) / M).sum()
    out = dict(w_lj=0.5 * wl.sum(), w_coul=0.5 * wc.sum(), w_recip=pref * w_rec, w_intra=sf.sum(), ke_com=float(ke),
               abs_w_lj=0.5 * np.abs(wl).sum(), abs_w_coul=0.5 * np.abs(wc).sum(), abs_w_recip=pref * abs_rec,
               abs_w_intra=np.abs(sf).sum(), abs_ke_com=float(ke), ev=ev)
    out["w_mol"] = ((out["w_lj"] + out["w_coul"]) + out["w_recip"]) - out["w_intra"]
    out["abs_w_mol"] = out["abs_w_lj"] + out["abs_w_coul"] + out["abs_w_recip"] + out["abs_w_intra"]
    return out


def scaled(x, box, lam, mass_o=MASS_O, mass_h=MASS_H):
    """the configuration under a scaling of the box edges and the molecules' centres of mass by lam, molecules rigid and whole
    (x unwrapped: every molecule in one image): (x', box')"""
    xd, L = np.asarray(x, dtype=np.float64), cr.edges(box)
    so = molecule_offsets(xd, box, mass_o, mass_h)
    return (xd - so) * lam + so, L * lam


def volume_derivative(x, box, species, wat, w=0.0, hs=(2.0 ** -10, 2.0 ** -12), **kw):
    """-dE/d lambda at lambda = 1 by central differences at the two steps hs (h, h / 4), Richardson-extrapolated
    ((16 D(h / 4) - D(h)) / 15 removes the h^2 term); r_cut, alpha and k_cut are held fixed.  The box edges L (1 +- h) must be
    exact in fp32: the reference rounds the box as the library does."""
    L = cr.edges(box)
    D = []
    for h in hs:
        e = []
        for lam in (1.0 + h, 1.0 - h):
            xs, bs = scaled(x, box, lam)
            if not np.array_equal(bs.astype(np.float32).astype(np.float64), bs):
                raise ValueError(f"box edge {L} times {lam} is not exact in fp32")
            e.append(wm.evaluate(xs, bs, species, wat, w, **kw)["energy"])
        D.append(-(e[0] - e[1]) / (2.0 * h))
    assert abs(hs[0] / hs[1] - 4.0) < 1e-15
    return (16.0 * D[1] - D[0]) / 15.0, D
