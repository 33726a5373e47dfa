// gamd_wrx_dev.h — the one body of the two per-molecule passes of water_relax.hip (k_wrx_mols for FIRE, k_wrx_lbmols for L-BFGS,
// DESIGN.md section 4.13.2): a molecule's three atom forces as the configured potential forms them, from the work buffers the
// force stage left.  3-site (w_h = 0): k_wmin_mols' statements — per atom the pair slices added in order from 0, the k slices
// added in order from 0, F = (t + (pq kf) g) len.  M-site: w4_atom_force's recipe (water_msite.hip) — the same sums give the
// SITE forces S (the oxygen's row is M's), the oxygen's Lennard-Jones row is added over its slices in order from 0, and
// F_O = (F_LJ + w_o S_M) len, F_Hk = (S_Hk + w_h S_M) len: M's force spread with the weights 1 - 2 w, w, w.  The energies: u_LJ
// from the pair rows (3-site) or the oxygen's Lennard-Jones row (M-site; the site walk stores 0 in that column), u_coul from
// the pair rows, each pair still counted twice.  Contraction is off from here on, as in the file that includes it.
#pragma once
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_wmin_dev.h"

namespace gamd_wrx {

using gamd_wmin::D3;

// the site model of the pass: the weights and the Lennard-Jones rows (w_h = 0: 3-site, nothing else is read)
struct Sites { double w_h, w_o; const double* ljpart; };

// the box's constants of the reciprocal force, as k_wmin_mols spells them
struct BoxK { double pref, kfx, kfy, kfz; };
__device__ __forceinline__ BoxK box_k(const WaterArgs& a, int box) {
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    const double pref = a.coul8pi / ((Lx * Ly) * Lz);
    return {pref, a.two_pi / Lx, a.two_pi / Ly, a.two_pi / Lz};
}

// molecule ml of box `box`: F[k] in kJ/mol/nm; the molecule's terms are added to ulj, uc and z2
__device__ __forceinline__ void mol_force(const WaterArgs& a, const Sites& q, const BoxK& c, int box, int npb, int ml, D3 (&F)[3],
                                          double& ulj, double& uc, double& z2) {
    const size_t mol = (size_t)box * (size_t)(npb / 3) + (size_t)ml;
    const bool msite = q.w_h != 0.0;                        // (uniform)
    D3 S[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int il = 3 * ml + k;
        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, t4 = 0.0;
        for (int s = 0; s < a.slices; ++s) {
            const double* p = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * WATER_PART;
            t0 += p[0]; t1 += p[1]; t2 += p[2]; t3 += p[3]; t4 += p[4];
        }
        double g0 = 0.0, g1 = 0.0, g2 = 0.0;
        for (int s = 0; s < a.kslices; ++s) {
            const double* p = a.rpart + (((size_t)box * (size_t)a.kslices + (size_t)s) * (size_t)npb + (size_t)il) * 3;
            g0 += p[0]; g1 += p[1]; g2 += p[2];
        }
        const bool o = a.species[3 * mol + k] != 0;
        const double pq = c.pref * (o ? a.q_o : a.q_h);
        S[k] = {t0 + (pq * c.kfx) * g0, t1 + (pq * c.kfy) * g1, t2 + (pq * c.kfz) * g2};
        if (!(msite && k == 0)) ulj += t3;                  // (M-site: the oxygen's u_LJ is its Lennard-Jones row's, below)
        uc += t4;
        const double z = o ? -2.0 : 1.0;                    // the charge in units of q_h: sums of these are exact
        z2 += z * z;
    }
    if (!msite) {
#pragma unroll
        for (int k = 0; k < 3; ++k) F[k] = {S[k].x * a.len, S[k].y * a.len, S[k].z * a.len};
        return;
    }
    double l0 = 0.0, l1 = 0.0, l2 = 0.0, l3 = 0.0;
    for (int s = 0; s < a.slices; ++s) {
        const double* p = q.ljpart + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)(npb / 3) + (size_t)ml) * W4_LJ;
        l0 += p[0]; l1 += p[1]; l2 += p[2]; l3 += p[3];
    }
    ulj += l3;
    F[0] = {(l0 + q.w_o * S[0].x) * a.len, (l1 + q.w_o * S[0].y) * a.len, (l2 + q.w_o * S[0].z) * a.len};
#pragma unroll
    for (int k = 1; k < 3; ++k)
        F[k] = {(S[k].x + q.w_h * S[0].x) * a.len, (S[k].y + q.w_h * S[0].y) * a.len, (S[k].z + q.w_h * S[0].z) * a.len};
}

}  // namespace gamd_wrx
