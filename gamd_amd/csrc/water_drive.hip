// water_drive.hip — the water classical force source (gamd_md_force_source with GAMD_FORCE_WATER_CLASSICAL, DESIGN.md section
// 4.11.1): the force evaluation of a step of an enqueued gamd_md_run / gamd_md_run_nhc whose forces come from the 3-site water
// potential of water_classical.hip (O-O Lennard-Jones plus a plain Ewald sum, in double) instead of the network.  Launched
// behind the neighbour stage of the step, where the edge encoder would start, on the run's fp32 positions in the CALLER's atom
// order O,H,H.  Five launches:
//
//   k_wsrc_pairs        the pair pass of k_water_pairs — same grid (T * slices, boxes), same 256-atom row tiles, same slices,
//                       same staging (positions as doubles plus the species flag), the same operations on d, r2, qq, gs, t and
//                       fs in the same order, the same-molecule erf branch, the erfc branch and the O-O Lennard-Jones term —
//                       with the force accumulators only: per atom and slice {Fx, Fy, Fz} into the first three doubles of the
//                       observer's partial row (the row keeps its WATER_PART stride; u_LJ, u_coul, pairs are not written).
//   k_water_rho, k_water_sk, k_water_recip
//                       the observer's own reciprocal-space kernels, unchanged (launch_water_recip, water_classical.hip).
//   k_wsrc_atoms        one thread per atom: the pair slices added in order from 0, the k slices added in order from 0,
//                       f_cl = (t + (pq kf) g) len in double to f_cl, and (float)f_cl (round to nearest) to the run's force buffer.
// No energy sums, no error sums, no final kernel.  The force bits are those of k_water_pairs / k_water_atoms on the same
// positions: f == fp32(f_cl of gamd_water_eval) bit for bit.  `part`, `rpart`, `rho_partial`, `sk`, `ublk` and `f_cl` are shared
// with the observer on one stream; a step that is driven and sampled evaluates twice and writes the same bits twice.  Fixed
// assignment, no floating-point atomics, contraction off, plain stores; every kernel returns while DEVFLAG_FROZEN is set, so a
// step enqueued again after a freeze writes the same bits.
// (No kernel uses a value it read from memory as an address: the checked build has nothing to range-check here.)
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_potential_dev.h"

namespace {

constexpr int WD_TILE = 256;

__global__ void __launch_bounds__(256) k_wsrc_pairs(WaterArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;                 // a step that will be evaluated again
    __shared__ double sx[WD_TILE], sy[WD_TILE], sz[WD_TILE];
    __shared__ unsigned char so[WD_TILE];
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)a.slices), s = (int)(blockIdx.x % (unsigned)a.slices);
    const int box = blockIdx.y;
    const int npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const size_t a0 = (size_t)box * (size_t)npb;            // the caller's order is box-major
    if (I >= a.tiles) return;                               // (uniform; cannot happen with the launcher's grid)
    const int il = I * WD_TILE + tid;                       // atom of this thread inside its box
    const bool vi = il < npb;
    const long long jb = (long long)s * a.chunk;
    const int je = (int)(jb + a.chunk < (long long)npb ? jb + a.chunk : (long long)npb);
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);

    double xi = 0.0, yi = 0.0, zi = 0.0;
    bool oi = false;
    if (vi) {
        const float* p = a.x + 3 * (a0 + (size_t)il);
        xi = (double)p[0]; yi = (double)p[1]; zi = (double)p[2];
        oi = a.species[a0 + (size_t)il] != 0;
    }
    const double q_h = a.q_h, q_o = -(q_h + q_h);           // -2 q_h, exact
    const double qi = oi ? q_o : q_h;
    const int mi = il / 3;                                  // npb is a multiple of 3: molecules do not straddle boxes
    // the thread's output row, held in vector registers from here on, as in k_water_pairs: left to the compiler, its uniform
    // part stays in scalar registers across the loop, which the potential's constants fill already (four scalar spills otherwise)
    double* out = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * WATER_PART;
    asm volatile("" : "+v"(out));
    double fx = 0.0, fy = 0.0, fz = 0.0;
    for (long long base = jb; base < je; base += WD_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int nj = (int)(je - base < WD_TILE ? je - base : WD_TILE);
        if (tid < nj) {
            const size_t j = a0 + (size_t)base + (size_t)tid;
            const float* p = a.x + 3 * j;
            sx[tid] = (double)p[0]; sy[tid] = (double)p[1]; sz[tid] = (double)p[2];
            so[tid] = a.species[j] != 0 ? 1 : 0;
        }
        __syncthreads();
        if (!vi) continue;
        const int self = (int)((long long)il - base);       // this atom's own slot in the chunk, if it is there
        const int mol0 = (int)((long long)mi * 3 - base);   // ... and its molecule's first
        for (int jj = 0; jj < nj; ++jj) {
            double dx = xi - sx[jj], dy = yi - sy[jj], dz = zi - sz[jj];
            dx = dx - Lx * rint(dx / Lx);
            dy = dy - Ly * rint(dy / Ly);
            dz = dz - Lz * rint(dz / Lz);
            const double r2 = (dx * dx + dy * dy) + dz * dz;
            if (jj == self) continue;
            const bool same = jj >= mol0 && jj < mol0 + 3;
            if (!same && !(r2 < a.rc2)) continue;
            const bool oj = so[jj] != 0;
            const double qq = a.coul * (qi * (oj ? q_o : q_h));
            const double r = sqrt(r2);
            const double ir2 = 1.0 / r2;
            const double ar = a.alpha * r;
            const double gs = a.two_a_rpi * exp(-(ar * ar));        // -r d/dr of erfc(alpha r), over r
            double fs;
            if (same) {                                     // U_excl: -q_i q_j erf(alpha r) / r
                const double t = erf(ar) / r;
                fs = (qq * (gs - t)) * ir2;
            } else {                                        // U_real: q_i q_j erfc(alpha r) / r
                const double t = erfc(ar) / r;
                fs = (qq * (t + gs)) * ir2;
                if (oi && oj) {                             // k_classical_pairs' term
                    const double2 lj = gamd_lj_term(a.sig2, a.eps4, 6.0 * a.eps4, a.u0, ir2);   // 6 (4 epsilon) = 24 epsilon bit for bit
                    double ru = lj.y;
                    if (a.rs >= 0.0 && r > a.rs) {
                        const double2 sw = gamd_lj_switch(a.rs, a.inv_w, r);
                        ru = ru * sw.x + ((lj.x * sw.y) * r);
                    }
                    fs = fs + -(ru * ir2);
                }
            }
            fx += fs * dx; fy += fs * dy; fz += fs * dz;
        }
    }
    if (vi) { out[0] = fx; out[1] = fy; out[2] = fz; }
}

__global__ void __launch_bounds__(256) k_wsrc_atoms(WaterArgs a, float* __restrict__ f_out) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    const int box = blockIdx.y;
    const int npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const int il = blockIdx.x * blockDim.x + threadIdx.x;   // one thread per atom
    if (il >= npb) return;
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    const double pref = a.coul8pi / ((Lx * Ly) * Lz);
    const double kfx = a.two_pi / Lx, kfy = a.two_pi / Ly, kfz = a.two_pi / Lz;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    for (int s = 0; s < a.slices; ++s) {
        const double* p = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * WATER_PART;
        t0 += p[0]; t1 += p[1]; t2 += p[2];
    }
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
    for (int s = 0; s < a.kslices; ++s) {
        const double* p = a.rpart + (((size_t)box * (size_t)a.kslices + (size_t)s) * (size_t)npb + (size_t)il) * 3;
        g0 += p[0]; g1 += p[1]; g2 += p[2];
    }
    const size_t i = (size_t)box * (size_t)npb + (size_t)il;
    const bool o = a.species[i] != 0;
    const double pq = pref * (o ? a.q_o : a.q_h);
    const double cx = (t0 + (pq * kfx) * g0) * a.len, cy = (t1 + (pq * kfy) * g1) * a.len,
                 cz = (t2 + (pq * kfz) * g2) * a.len;                               // kJ/mol/nm
    a.f_cl[3 * i] = cx; a.f_cl[3 * i + 1] = cy; a.f_cl[3 * i + 2] = cz;
    f_out[3 * i] = (float)cx; f_out[3 * i + 1] = (float)cy; f_out[3 * i + 2] = (float)cz;
}

}  // namespace

int launch_water_drive(const WaterArgs& a, float* f_out, hipStream_t st) {
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1, npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const long long T = (npb + WD_TILE - 1) / WD_TILE;
    if (npb < 3 || npb % 3 || nb > 65535 || a.tiles != (int)T || a.slices < 1 || a.chunk < 1) return -1;
    if ((long long)a.slices * a.chunk < npb || T * a.slices > 0x7fffffll) return -1;   // the slices cover a row; grid.x * 256 threads stay below 2^31
    if (!a.x || !a.species || !a.part || !a.rpart || !a.f_cl || !a.devflags || !f_out) return -1;
    hipLaunchKernelGGL(k_wsrc_pairs, dim3((unsigned)(T * a.slices), nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    if (int r = launch_water_recip(a, st)) return r;
    hipLaunchKernelGGL(k_wsrc_atoms, dim3((unsigned)T, nb), dim3(256), 0, st, a, f_out); GAMD_CHECK_LAUNCH();
    return 0;
}
