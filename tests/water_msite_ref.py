"""Float64 host reference of the water classical potential with the TIP4P M-site (gamd_amd/csrc/water_msite.hip,
gamd_water_msite), built on water_classical_ref.ewald, which takes arbitrary point charges and an exclusion mask: the charge
sites of ONE box (`sites`: M = O + w (d_1 + d_2) in the oxygen's row, the hydrogens in their own), the Ewald sum on the sites,
O-O Lennard-Jones on the oxygens with a cutoff test of its own, and the chain rule that takes M's force back to the atoms
(`evaluate`).  The device wraps O and H into [0, L) before it forms the sites and this module does not: the two differ by the
rounding of a minimum-image difference, which the sums of absolute terms returned here bound.  With w = 0 every array is
water_classical_ref.evaluate's, formed by the same operations.  Not an oracle module: nothing here was compared with OpenMM."""
import numpy as np

import classical_ref as cr
import water_classical_ref as wr

TIP4PEW_W = 0.106676721


def tip4pew(r_cut=9.5, **kw):
    """TIP4P-Ew as the package's TIP4PEW constant set states it (UNVERIFIED against OpenMM's tip4pew.xml): a Water and the weight"""
    return wr.Water(q_h=0.52422, sigma_o=3.16435, epsilon_o=0.680946, r_cut=r_cut, **kw), TIP4PEW_W


def sites(x, box, w):
    """charge-site positions [N, 3] of x [N, 3] (atoms O,H,H per molecule, any periodic image): row 3 m holds
    M = O + w (d_1 + d_2), d_k = H_k - O per component as d - L rint(d / L); the hydrogens' rows are their positions"""
    xd, L = np.asarray(x, dtype=np.float64), cr.edges(box)
    o = xd[0::3]
    d1, d2 = xd[1::3] - o, xd[2::3] - o
    d1 = d1 - L * np.rint(d1 / L)
    d2 = d2 - L * np.rint(d2 / L)
    s = xd.copy()
    s[0::3] = o + w * (d1 + d2)
    return s


def evaluate(x, box, species, wat, w, length_per_nm=0.0, n2max=None):
    """4-site water in ONE box: x [N, 3] (fp32 positions as the device reads them, or float64), species [N] (1,0,0 per molecule),
    wat a water_classical_ref.Water, w the hydrogens' weight of the M-site.  Energies kJ/mol, forces kJ/mol/nm on the three real
    atoms.  Returns water_classical_ref.evaluate's dict: ewald()'s terms on the SITES (pairs, near, sum_q, n_k, tail among
    them), u_coul, u_lj, abs_lj, energy, abs_energy, forces [N, 3] and abs_f [N] after the redistribution
        F_O = F_LJ(O) + (1 - 2 w) F_M,   F_Hk = F_site(Hk) + w F_M
        abs_f[O] = (1 - 2 w) abs_f_site[M] + abs_f_LJ[O],   abs_f[Hk] = abs_f_site[Hk] + w abs_f_site[M]
    and near_lj = O-O pairs with |r - r_cut| <= 1e-12 r_cut (the Lennard-Jones term has its own cutoff test); real_mask and
    lj_mask [N, N] are the pairs inside either cutoff (the potential jumps where one changes)."""
    ln = float(np.float32(length_per_nm)) if length_per_nm else 10.0
    o = np.asarray(species).reshape(-1) != 0
    n = o.shape[0]
    if n % 3 or not (o[0::3].all() and not o[1::3].any() and not o[2::3].any()):
        raise ValueError("atoms must be ordered O,H,H per molecule")
    q = np.where(o, -2.0 * wat.q_h, wat.q_h)
    mol = np.arange(n) // 3
    same = mol[:, None] == mol[None, :]
    out = wr.ewald(sites(x, box, w), box, q, same, wat.alpha, wat.r_cut, wat.k_cut, wat.coulomb_const * ln, n2max)
    # Lennard-Jones: the atoms' own minimum-image distances, oxygens of different molecules, r_OO^2 < r_cut^2
    d, r2 = cr.min_image(x, box)
    m = ~same & (o[:, None] & o[None, :]) & (r2 < wat.r_cut * wat.r_cut)
    u, ru = wat.lj.terms(np.where(m, r2, 1.0))
    u, ru = np.where(m, u, 0.0), np.where(m, ru, 0.0)
    fij = np.where(m, -(ru * (1.0 / np.where(m, r2, 1.0))), 0.0)[..., None] * d
    f_lj, abs_lj_f = fij.sum(axis=1), np.sqrt((fij * fij).sum(axis=-1)).sum(axis=1)
    iu = np.triu_indices(n, 1)
    oo = (~same & (o[:, None] & o[None, :]))[iu]
    out["near_lj"] = int(((np.abs(np.sqrt(r2[iu]) - wat.r_cut) <= 1e-12 * wat.r_cut) & oo).sum())
    out["lj_mask"] = m
    out["u_lj"], out["abs_lj"] = 0.5 * u.sum(), 0.5 * np.abs(u).sum()
    out["u_coul"] = out["u_real"] + out["u_excl"]
    # the chain rule: M = (1 - 2 w) O + w H1 + w H2 up to lattice vectors
    w_o = 1.0 - 2.0 * w
    fs, ab = out["forces"], out["abs_f"]
    out["f_site"], out["abs_f_site"] = fs * ln, ab * ln
    F, A = f_lj + fs, abs_lj_f + ab
    F[0::3] = f_lj[0::3] + w_o * fs[0::3]
    A[0::3] = abs_lj_f[0::3] + w_o * ab[0::3]
    for k in (1, 2):
        F[k::3] = fs[k::3] + w * fs[0::3]
        A[k::3] = ab[k::3] + w * ab[0::3]
    out["forces"], out["abs_f"] = F * ln, A * ln
    del out["f_pair"], out["f_recip"]
    out["energy"] = ((out["u_coul"] + out["u_recip"]) + out["u_self"]) + out["u_lj"]
    out["abs_energy"] = out["abs_real"] + out["abs_recip"] + abs(out["u_self"]) + out["abs_lj"]
    return out
