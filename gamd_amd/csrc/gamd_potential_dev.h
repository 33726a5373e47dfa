// gamd_potential_dev.h — the device terms the kernels of the two classical potentials share (DESIGN.md sections 4.9 - 4.13; the
// passes built from them are in gamd_passes_dev.h).  Every helper spells out one order of operations: the host computes
// u_LJ(r_cut) by gamd_lj_term's (potential_args, observe.hip), and tests/classical_ref.py mirrors them.  Contraction is off from
// here on, as in the files that include it.
#pragma once
#include "gamd_common.h"

#pragma clang fp contract(off)

// fp32 edge `c` of box `box`, widened: the eval call's edges, the run's one box, or the run's box table
template <typename Args>
__device__ __forceinline__ double gamd_box_edge(const Args& a, int box, int c) {
    if (a.box_edges) return (double)a.box_edges[3 * box + c];
    if (a.bx.n_boxes <= 1) return (double)a.box[c];
    const float4 b = a.bx.boxes[3 * box];
    return (double)(c == 0 ? b.x : (c == 1 ? b.y : b.z));
}

// one wave's part of the fixed tree of k_report_ke: shuffle-down 32 .. 1 (lane 0 holds the sum; the four waves of a
// 256-thread workgroup are then added as (w0 + w1) + (w2 + w3))
__device__ __forceinline__ double gamd_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// Lennard-Jones at 1 / r^2 = ir2: (u_LJ - u0, r u_LJ'(r)); eps24 = 24 epsilon (6 * eps4 is the same double)
__device__ __forceinline__ double2 gamd_lj_term(double sig2, double eps4, double eps24, double u0, double ir2) {
    const double s2 = sig2 * ir2;
    const double s6 = (s2 * s2) * s2;
    const double s12 = s6 * s6;
    return make_double2(eps4 * (s12 - s6) - u0, -(eps24 * ((s12 + s12) - s6)));
}

// the switch polynomial at r > rs, (S, dS / dr): S(t) = 1 - t^3 (6 t^2 - 15 t + 10), t = (r - rs) inv_w.  The caller applies it
// to (u, r u'): r u' <- r u' S + (u dS) r, then u <- u S.  (Both helpers return by value: written through references,
// k_classical_pairs orders its accumulators differently.)
__device__ __forceinline__ double2 gamd_lj_switch(double rs, double inv_w, double r) {
    const double t = (r - rs) * inv_w;
    const double t2 = t * t, tm = t - 1.0;
    const double S = 1.0 - (t2 * t) * ((6.0 * t - 15.0) * t + 10.0);
    const double dS = ((-30.0 * t2) * (tm * tm)) * inv_w;
    return make_double2(S, dS);
}

// The Lennard-Jones term of one pair in force: (u, r u') = ((u_LJ - u0) S, r d/dr of it) from the potential's constants in `a`
// (ClassicalArgs or WaterArgs; eps24 is the caller's: a.eps24, or 6.0 * a.eps4 where only 4 epsilon is carried — the same
// double).  Every pair kernel of either potential calls one of the two spellings, which differ in what the caller has at hand:
// _r2 takes r^2 and draws the square root only where a switch is configured (the Lennard-Jones walks, k_w4_lj); _r takes r (the
// water walk has it for the Coulomb term).  By value, like the helpers above.
__device__ __forceinline__ double2 gamd_lj_switched(double2 lj, double rs, double inv_w, double r) {
    const double2 sw = gamd_lj_switch(rs, inv_w, r);
    double u = lj.x, ru = lj.y;
    ru = ru * sw.x + ((u * sw.y) * r);                      // r u'(r), u = (u_LJ - u0) S.  (r u' first, then u: the values do
    u = u * sw.x;                                           // not depend on it, k_classical_pairs' inner loop schedule does)
    return make_double2(u, ru);
}
template <typename Args>
__device__ __forceinline__ double2 gamd_lj_pair_r2(const Args& a, double eps24, double ir2, double r2) {
    double2 lj = gamd_lj_term(a.sig2, a.eps4, eps24, a.u0, ir2);
    if (a.rs >= 0.0) {                                      // (the square root only where there is a switch)
        const double r = sqrt(r2);
        if (r > a.rs) lj = gamd_lj_switched(lj, a.rs, a.inv_w, r);
    }
    return lj;
}
template <typename Args>
__device__ __forceinline__ double2 gamd_lj_pair_r(const Args& a, double eps24, double ir2, double r) {
    double2 lj = gamd_lj_term(a.sig2, a.eps4, eps24, a.u0, ir2);
    if (a.rs >= 0.0 && r > a.rs) lj = gamd_lj_switched(lj, a.rs, a.inv_w, r);
    return lj;
}

// fractional coordinate of the reciprocal-space kernels (water_classical.hip, water_minimize.hip): the position wrapped into
// [0, L) first, s = (x - L floor(x / L)) / L.  Where x + k L is exact in fp32 the wrapped position is the same double for every
// image k, and so is every phase n.s (x / L alone is not: fl((x + k L) / L) and fl(x / L) + k differ in the last bits).
__device__ __forceinline__ double water_frac(double x, double L) { return (x - L * floor(x / L)) / L; }

// the TIP4P virtual site of one molecule (water_msite.hip; OpenMM's ThreeParticleAverageSite with weights 1 - 2 w, w, w):
// M = O' + w (d_1 + d_2), d_k = H_k - O per component as d - L rint(d / L), from the fp32 positions widened, and O' = O wrapped
// into [0, L) by water_wrap.  The hydrogens may be in any image; where x + k L is exact in fp32, d_k and O' — and so M — are the
// same doubles for every image of every atom.  The one place M is computed: every 4-site kernel reads its result.  T = float:
// the fp32 atoms widened (k_w4_sites); T = double: a minimiser's positions as they are (k_wrx_sites, water_relax.hip) — the
// same statements, the widening is then the identity.
__device__ __forceinline__ double water_wrap(double x, double L) { return x - L * floor(x / L); }

template <typename T>
__device__ __forceinline__ void water_msite(const T* o, const T* h1, const T* h2, double Lx, double Ly, double Lz, double w,
                                            double& mx, double& my, double& mz) {
    const double ox = (double)o[0], oy = (double)o[1], oz = (double)o[2];
    double ax = (double)h1[0] - ox, ay = (double)h1[1] - oy, az = (double)h1[2] - oz;
    double bx = (double)h2[0] - ox, by = (double)h2[1] - oy, bz = (double)h2[2] - oz;
    ax = ax - Lx * rint(ax / Lx); ay = ay - Ly * rint(ay / Ly); az = az - Lz * rint(az / Lz);
    bx = bx - Lx * rint(bx / Lx); by = by - Ly * rint(by / Ly); bz = bz - Lz * rint(bz / Lz);
    mx = water_wrap(ox, Lx) + w * (ax + bx); my = water_wrap(oy, Ly) + w * (ay + by); mz = water_wrap(oz, Lz) + w * (az + bz);
}

// one atom's terms of the force-error sums of the run's force g against the classical force c (both kJ/mol/nm):
// sum |D_c|, sum |D|^2, sum cos, sum |c|, sum |g|, and the atoms left out of the cosine because one of the two is zero
__device__ __forceinline__ void gamd_force_error(double gx, double gy, double gz, double cx, double cy, double cz, double& sum_abs,
                                                 double& sum_sq, double& sum_cos, double& sum_norm_cl, double& sum_norm, double& excluded) {
    const double dx = gx - cx, dy = gy - cy, dz = gz - cz;
    sum_abs += (fabs(dx) + fabs(dy)) + fabs(dz);
    sum_sq += (dx * dx + dy * dy) + dz * dz;
    const double nc = sqrt((cx * cx + cy * cy) + cz * cz), ng = sqrt((gx * gx + gy * gy) + gz * gz);
    if (nc == 0.0 || ng == 0.0) excluded += 1.0;
    else sum_cos += ((gx * cx + gy * cy) + gz * cz) / (ng * nc);
    sum_norm_cl += nc; sum_norm += ng;
}
