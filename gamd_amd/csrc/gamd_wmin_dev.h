// gamd_wmin_dev.h — the per-molecule double arithmetic of the water energy minimiser (water_minimize.hip, DESIGN.md section
// 4.13): SETTLE (Miyamoto & Kollman, J. Comput. Chem. 13, 952 (1992)) and the 3x3 projection onto the tangent space of the three
// bond constraints, both with UNIT weights for O, H and H — the orthogonal projection, so that the projected force is the
// gradient on the constraint manifold.  The formulas are those of gamd_md_dev.h's fp32 settle_positions / settle_velocities with
// m_O = m_H = 1, in double; tests/water_minimize_ref.py mirrors them operation for operation.  Contraction is off from here on, as in the
// file that includes it.
#pragma once
#include "gamd_common.h"

#pragma clang fp contract(off)

namespace gamd_wmin {

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 operator*(double s, D3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ D3 unit(D3 a) { return (1.0 / sqrt(dot(a, a))) * a; }

__device__ __forceinline__ void load_mol(const double* p, size_t m, D3 (&o)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = {p[9 * m + 3 * k], p[9 * m + 3 * k + 1], p[9 * m + 3 * k + 2]};
}
__device__ __forceinline__ void store_mol(double* p, size_t m, const D3 (&o)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { p[9 * m + 3 * k] = o[k].x; p[9 * m + 3 * k + 1] = o[k].y; p[9 * m + 3 * k + 2] = o[k].z; }
}

// x0: the reference geometry (rigid, or the raw input at the start); x1: the unconstrained new positions -> the constrained new
// positions, in place.  Unit weights: the centroid of x1 is kept.  ra = 2 t / 3, rb = t / 3, rc = r_hh / 2, t = sqrt(r_oh^2 - rc^2).
__device__ __forceinline__ void settle(const D3 (&x0)[3], D3 (&x1)[3], double ra, double rb, double rc) {
    const D3 b0 = x0[1] - x0[0], c0 = x0[2] - x0[0];
    const D3 A1 = x1[0] - x0[0], B1 = x1[1] - x0[0], C1 = x1[2] - x0[0];
    const D3 d0 = (1.0 / 3.0) * ((A1 + B1) + C1);
    const D3 a1 = A1 - d0, b1 = B1 - d0, c1 = C1 - d0;
    D3 n0 = cross(b0, c0), n1 = cross(a1, n0), n2 = cross(n0, n1);
    n0 = unit(n0); n1 = unit(n1); n2 = unit(n2);
    const double b0x = dot(b0, n1), b0y = dot(b0, n2), c0x = dot(c0, n1), c0y = dot(c0, n2);
    const double a1z = dot(a1, n0);
    const double b1x = dot(b1, n1), b1y = dot(b1, n2), b1z = dot(b1, n0);
    const double c1x = dot(c1, n1), c1y = dot(c1, n2), c1z = dot(c1, n0);
    const double sinphi = a1z / ra, cosphi = sqrt(1.0 - sinphi * sinphi);
    const double sinpsi = (b1z - c1z) / ((2.0 * rc) * cosphi), cospsi = sqrt(1.0 - sinpsi * sinpsi);
    const double a2y = ra * cosphi, a2z = ra * sinphi;
    const double b2x = -(rc * cospsi), b2y = -(rb * cosphi) - (rc * sinpsi) * sinphi, b2z = -(rb * sinphi) + (rc * sinpsi) * cosphi;
    const double c2x = rc * cospsi, c2y = -(rb * cosphi) + (rc * sinpsi) * sinphi, c2z = -(rb * sinphi) - (rc * sinpsi) * cosphi;
    const double alpha = (b2x * (b0x - c0x) + b0y * b2y) + c0y * c2y;
    const double beta = (b2x * (c0y - b0y) + b0x * b2y) + c0x * c2y;
    const double gamma = (b0x * b1y - b1x * b0y) + (c0x * c1y - c1x * c0y);
    const double a2b2 = alpha * alpha + beta * beta;
    const double sint = (alpha * gamma - beta * sqrt(a2b2 - gamma * gamma)) / a2b2, cost = sqrt(1.0 - sint * sint);
    const double a3x = -(a2y * sint), a3y = a2y * cost;
    const double b3x = b2x * cost - b2y * sint, b3y = b2x * sint + b2y * cost;
    const double c3x = c2x * cost - c2y * sint, c3y = c2x * sint + c2y * cost;
    const D3 base = x0[0] + d0;
    x1[0] = base + (((a3x * n1) + (a3y * n2)) + (a2z * n0));
    x1[1] = base + (((b3x * n1) + (b3y * n2)) + (b2z * n0));
    x1[2] = base + (((c3x * n1) + (c3y * n2)) + (c2z * n0));
}

// remove the components of u (a force or a velocity per atom) along the three bonds of the molecule at x:
// u_i += sum_k (+-) g_k r_k with A g = -r_k . (u_a - u_b), unit weights
__device__ __forceinline__ void project(const D3 (&x)[3], D3 (&u)[3]) {
    const D3 r0 = x[0] - x[1], r1 = x[0] - x[2], r2 = x[1] - x[2];
    const double y0 = -dot(r0, u[0] - u[1]), y1 = -dot(r1, u[0] - u[2]), y2 = -dot(r2, u[1] - u[2]);
    const double a00 = 2.0 * dot(r0, r0), a01 = dot(r0, r1), a02 = -dot(r0, r2);
    const double a11 = 2.0 * dot(r1, r1), a12 = dot(r1, r2), a22 = 2.0 * dot(r2, r2);
    // symmetric 3x3 solve by cofactors
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double inv_det = 1.0 / ((a00 * c00 + a01 * c01) + a02 * c02);
    const double g0 = ((c00 * y0 + c01 * y1) + c02 * y2) * inv_det;
    const double g1 = ((c01 * y0 + c11 * y1) + c12 * y2) * inv_det;
    const double g2 = ((c02 * y0 + c12 * y1) + c22 * y2) * inv_det;
    u[0] = u[0] + ((g0 * r0) + (g1 * r1));
    u[1] = u[1] + ((g2 * r2) - (g0 * r0));
    u[2] = u[2] - ((g1 * r1) + (g2 * r2));
}

// component d of molecule `mol` as the minimisers return it: x_io = fp32(x64 - s), s the lattice vector (edge L, an fp32 value)
// that brings the oxygen into [0, L); x64_out (may be null) = x64
__device__ __forceinline__ void store_wrapped(const double* x64, size_t mol, int d, double L, float* x_io, double* x64_out) {
    const float Lf = (float)L;                              // exact: the edge is an fp32 value
    const double xo = x64[9 * mol + d];
    double s = L * floor(xo / L);
    if (xo - s < 0.0) s = s - L;                            // the quotient rounded up to an integer
    if ((float)(xo - s) >= Lf) s = s + L;                   // the oxygen rounds up to L: it goes to 0 with its hydrogens
    float o = (float)(xo - s);
    if (o < 0.f) o = 0.f;
    x_io[9 * mol + d] = o;
    x_io[9 * mol + 3 + d] = (float)(x64[9 * mol + 3 + d] - s);
    x_io[9 * mol + 6 + d] = (float)(x64[9 * mol + 6 + d] - s);
    if (x64_out) {
        x64_out[9 * mol + d] = xo; x64_out[9 * mol + 3 + d] = x64[9 * mol + 3 + d]; x64_out[9 * mol + 6 + d] = x64[9 * mol + 6 + d];
    }
}

}  // namespace gamd_wmin
