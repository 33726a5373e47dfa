// drive.hip — the classical force source (gamd_md_force_source): the force evaluation of a step of an
// enqueued gamd_md_run / gamd_md_run_nhc whose forces come from the switched, shifted Lennard-Jones potential of classical.hip
// instead of the network.  Launched behind the neighbour stage of the step, where the edge encoder would start, on the run's
// fp32 positions in the CALLER's atom order:
//
//   k_drive_lj_pairs    the pair pass of k_classical_pairs — same grid (T * slices, boxes), same 256-atom row tiles, same
//                       slices, same staging, the same operations on d, r2, u and r u' in the same order — with the force
//                       accumulators only: per atom and slice {Fx, Fy, Fz} into the first three doubles of the observer's
//                       partial row (the row keeps its CLASSICAL_PART stride; e_i, w_i, pairs_i are not written).
//   k_drive_lj_atoms    one thread per atom: the slices' partials added in order from 0, f_cl = F * len in double to f_cl, and
//                       (float)f_cl (round to nearest) to the run's force buffer.
// No energy sums, no error sums, no final kernel.  The force bits are those of k_classical_pairs / k_classical_atoms on the same
// positions: f == fp32(f_cl of gamd_classical_eval) bit for bit.  `part` and `f_cl` are shared with the observer on one stream;
// a step that is driven and sampled evaluates twice and writes the same bits twice.  Fixed assignment, no floating-point
// atomics, contraction off, plain stores; every kernel returns while DEVFLAG_FROZEN is set, so a step enqueued again after a
// freeze writes the same bits.
// (No kernel uses a value it read from memory as an address: the checked build has nothing to range-check here.)
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_potential_dev.h"

namespace {

constexpr int DR_TILE = 256;

__global__ void __launch_bounds__(256) k_drive_lj_pairs(ClassicalArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;                 // a step that will be evaluated again
    __shared__ double sx[DR_TILE], sy[DR_TILE], sz[DR_TILE];
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)a.slices), s = (int)(blockIdx.x % (unsigned)a.slices);
    const int box = blockIdx.y;
    const int npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const size_t a0 = (size_t)box * (size_t)npb;            // the caller's order is box-major
    if (I >= a.tiles) return;                               // (uniform; cannot happen with the launcher's grid)
    const int il = I * DR_TILE + tid;                       // atom of this thread inside its box
    const bool vi = il < npb;
    const long long jb = (long long)s * a.chunk;
    const int je = (int)(jb + a.chunk < (long long)npb ? jb + a.chunk : (long long)npb);
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);

    double xi = 0.0, yi = 0.0, zi = 0.0;
    if (vi) {
        const float* p = a.x + 3 * (a0 + (size_t)il);
        xi = (double)p[0]; yi = (double)p[1]; zi = (double)p[2];
    }
    double fx = 0.0, fy = 0.0, fz = 0.0;
    for (long long base = jb; base < je; base += DR_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int nj = (int)(je - base < DR_TILE ? je - base : DR_TILE);
        if (tid < nj) {
            const float* p = a.x + 3 * (a0 + (size_t)base + (size_t)tid);
            sx[tid] = (double)p[0]; sy[tid] = (double)p[1]; sz[tid] = (double)p[2];
        }
        __syncthreads();
        if (!vi) continue;
        const int self = (int)((long long)il - base);       // this atom's own slot in the chunk, if it is there
        for (int jj = 0; jj < nj; ++jj) {
            double dx = xi - sx[jj], dy = yi - sy[jj], dz = zi - sz[jj];
            dx = dx - Lx * rint(dx / Lx);
            dy = dy - Ly * rint(dy / Ly);
            dz = dz - Lz * rint(dz / Lz);
            const double r2 = (dx * dx + dy * dy) + dz * dz;
            if (jj == self || !(r2 < a.rc2)) continue;
            const double ir2 = 1.0 / r2;
            const double2 lj = gamd_lj_term(a.sig2, a.eps4, a.eps24, a.u0, ir2);
            double ru = lj.y;                               // r u_LJ'(r)
            if (a.rs >= 0.0) {                              // (the square root only where there is a switch)
                const double r = sqrt(r2);
                if (r > a.rs) {
                    const double2 sw = gamd_lj_switch(a.rs, a.inv_w, r);
                    ru = ru * sw.x + ((lj.x * sw.y) * r);   // r u'(r), u = (u_LJ - u0) S
                }
            }
            const double fs = -(ru * ir2);                  // F_ij = -u'(r) d / r = fs d
            fx += fs * dx; fy += fs * dy; fz += fs * dz;
        }
    }
    if (vi) {
        double* out = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * CLASSICAL_PART;
        out[0] = fx; out[1] = fy; out[2] = fz;
    }
}

__global__ void __launch_bounds__(256) k_drive_lj_atoms(ClassicalArgs a, float* __restrict__ f_out) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    const int box = blockIdx.y;
    const int npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const int il = blockIdx.x * blockDim.x + threadIdx.x;   // one thread per atom
    if (il >= npb) return;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    for (int s = 0; s < a.slices; ++s) {
        const double* p = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * CLASSICAL_PART;
        t0 += p[0]; t1 += p[1]; t2 += p[2];
    }
    const size_t i = (size_t)box * (size_t)npb + (size_t)il;
    const double cx = t0 * a.len, cy = t1 * a.len, cz = t2 * a.len;                 // kJ/mol/nm
    a.f_cl[3 * i] = cx; a.f_cl[3 * i + 1] = cy; a.f_cl[3 * i + 2] = cz;
    f_out[3 * i] = (float)cx; f_out[3 * i + 1] = (float)cy; f_out[3 * i + 2] = (float)cz;
}

}  // namespace

int launch_classical_drive(const ClassicalArgs& a, float* f_out, hipStream_t st) {
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1, npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const long long T = (npb + DR_TILE - 1) / DR_TILE;
    if (npb < 1 || nb > 65535 || a.tiles != (int)T || a.slices < 1 || a.chunk < 1) return -1;
    if ((long long)a.slices * a.chunk < npb || T * a.slices > 0x7fffffll) return -1;   // the slices cover a row; grid.x * 256 threads stay below 2^31
    if (!a.x || !a.part || !a.f_cl || !a.devflags || !f_out) return -1;
    hipLaunchKernelGGL(k_drive_lj_pairs, dim3((unsigned)(T * a.slices), nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_drive_lj_atoms, dim3((unsigned)T, nb), dim3(256), 0, st, a, f_out); GAMD_CHECK_LAUNCH();
    return 0;
}
