// water_classical.hip — the water classical observer: the classical potential of 3-site water (O-O Lennard-Jones plus point
// charges, the reference's TIP3P labels: potential energy and getForces of dataset/generate_tip3p_data.py:91-103), with the
// electrostatics as a plain Ewald sum in double, on the device behind the second half of every interval-th step of an enqueued
// gamd_md_run / gamd_md_run_nhc, and the same kernels on given positions outside a run (gamd_water_eval).  Atoms in the CALLER's
// order O,H,H: molecule = index / 3, O = species != 0, q_O = -2 q_H.
//
//   k_water_pairs   the water tile walk (gamd_water_walk, gamd_passes_dev.h) on the fp32 positions widened, with the O-O
//                   Lennard-Jones term and every accumulator: per atom and slice one partial row
//                   {Fx, Fy, Fz, u_LJ, u_real + u_excl, pairs}.  FULL rows.
//   k_water_rho     the rho(k) pass (gamd_water_rho, same header) on the fp32 positions: one partial (re, im) per workgroup
//                   and k-vector.
//   k_water_sk      grid (K / 256, boxes), one thread per (box, k): S(k) = the block partials added in order, k and
//                   A(k) = exp(-k^2 / 4 alpha^2) / k^2 (0 beyond the box's k_cut); {Re S, Im S, A} stored, and the
//                   workgroup's sum of A |S|^2 by the fixed tree.
//   k_water_recip   the reciprocal force pass (gamd_water_recip, same header) on the fp32 positions, k slice ks walking the
//                   k-vectors [ks * kchunk, (ks + 1) * kchunk) in list order.
//   k_water_atoms   per atom: the pair slices added in order, the k slices added in order, f_cl; the atom's terms of the five
//                   force-error sums, its integer charge number z (-2, +1) and z^2; the fixed tree of k_classical_atoms.
//   k_water_final   one thread per box adds the block rows in order (and the k blocks' A |S|^2 in order) and writes the row
//                   the HOST chose.
// The arithmetic is spelled out in DESIGN.md section 4.10 (tests/water_classical_ref.py mirrors it).  d_ij = -d_ji bit for bit
// (rint is odd) and q_i q_j commutes, so F_ij = -F_ji bit for bit.  Fixed atom-to-thread and k-to-thread assignment, fixed
// slices and blocks per handle, no floating-point atomics, contraction off: the same bits run after run.  Every kernel returns
// while DEVFLAG_FROZEN is set; nothing is updated in place, so a sample that runs twice writes the same bits twice.
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_passes_dev.h"

namespace {

__global__ void __launch_bounds__(256) k_water_pairs(WaterArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;                 // a frame that will be evaluated again
    gamd_water_walk<WATER_PART, true>(a, GamdPosF32{a.x});
}

__global__ void __launch_bounds__(256) k_water_rho(WaterArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    gamd_water_rho(a, GamdPosF32{a.x});
}

__global__ void __launch_bounds__(256) k_water_sk(WaterArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    __shared__ double red[4];
    const int box = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;    // one thread per (box, k)
    double t = 0.0;
    if (k < a.n_k) {
        double re = 0.0, im = 0.0;
        for (int b = 0; b < a.rho_blocks; ++b) {
            const double* p = a.rho_partial + (((size_t)box * a.rho_blocks + b) * (size_t)a.n_k + (size_t)k) * 2;
            re += p[0]; im += p[1];
        }
        const double kx = a.two_pi * ((double)a.kvec[3 * (size_t)k] / gamd_box_edge(a, box, 0));
        const double ky = a.two_pi * ((double)a.kvec[3 * (size_t)k + 1] / gamd_box_edge(a, box, 1));
        const double kz = a.two_pi * ((double)a.kvec[3 * (size_t)k + 2] / gamd_box_edge(a, box, 2));
        const double k2 = (kx * kx + ky * ky) + kz * kz;
        const double A = k2 <= a.kc2 ? exp(-(k2 * a.inv_4a2)) / k2 : 0.0;     // beyond this box's k_cut: weight zero
        double* out = a.sk + ((size_t)box * (size_t)a.n_k + (size_t)k) * 3;
        out[0] = re; out[1] = im; out[2] = A;
        t = A * (re * re + im * im);
    }
    t = gamd_wave_sum(t);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) a.ublk[(size_t)box * (size_t)a.kblocks + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void __launch_bounds__(256) k_water_recip(WaterArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    gamd_water_recip(a, GamdPosF32{a.x});
}

__global__ void __launch_bounds__(256) k_water_atoms(WaterArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    __shared__ double red[4][WATER_ACC];
    const int box = blockIdx.y;
    const int npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const size_t a0 = (size_t)box * (size_t)npb;
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    const double pref = a.coul8pi / ((Lx * Ly) * Lz);
    const double kfx = a.two_pi / Lx, kfy = a.two_pi / Ly, kfz = a.two_pi / Lz;
    double acc[WATER_ACC];
#pragma unroll
    for (int q = 0; q < WATER_ACC; ++q) acc[q] = 0.0;
    for (int il = blockIdx.x * blockDim.x + threadIdx.x; il < npb; il += gridDim.x * blockDim.x) {
        double t[WATER_PART];
#pragma unroll
        for (int q = 0; q < WATER_PART; ++q) t[q] = 0.0;
        for (int s = 0; s < a.slices; ++s) {
            const double* p = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * WATER_PART;
#pragma unroll
            for (int q = 0; q < WATER_PART; ++q) t[q] += p[q];
        }
        double g[3] = {0.0, 0.0, 0.0};
        for (int s = 0; s < a.kslices; ++s) {
            const double* p = a.rpart + (((size_t)box * (size_t)a.kslices + (size_t)s) * (size_t)npb + (size_t)il) * 3;
            g[0] += p[0]; g[1] += p[1]; g[2] += p[2];
        }
        const size_t i = a0 + (size_t)il;
        const bool o = a.species[i] != 0;
        const double pq = pref * (o ? a.q_o : a.q_h);
        const double cx = (t[0] + (pq * kfx) * g[0]) * a.len, cy = (t[1] + (pq * kfy) * g[1]) * a.len,
                     cz = (t[2] + (pq * kfz) * g[2]) * a.len;                    // kJ/mol/nm
        a.f_cl[3 * i] = cx; a.f_cl[3 * i + 1] = cy; a.f_cl[3 * i + 2] = cz;
        acc[0] += t[3]; acc[1] += t[4]; acc[2] += t[5];
        const double z = o ? -2.0 : 1.0;                    // the charge in units of q_h: sums of these are exact
        acc[9] += z; acc[10] += z * z;
        if (a.f) {
            gamd_force_error((double)a.f[3 * i], (double)a.f[3 * i + 1], (double)a.f[3 * i + 2], cx, cy, cz, acc[3], acc[4], acc[5],
                             acc[6], acc[7], acc[8]);
        }
    }
#pragma unroll
    for (int q = 0; q < WATER_ACC; ++q) {
        const double v = gamd_wave_sum(acc[q]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < WATER_ACC) {
        const int q = threadIdx.x;
        a.blk[((size_t)box * (size_t)a.blocks + blockIdx.x) * WATER_ACC + q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
    }
}

__global__ void k_water_final(WaterArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1;
    const int box = blockIdx.x * blockDim.x + threadIdx.x;  // one thread per box
    if (box >= nb) return;
    double s[WATER_ACC];
#pragma unroll
    for (int q = 0; q < WATER_ACC; ++q) {
        s[q] = 0.0;
        for (int b = 0; b < a.blocks; ++b) s[q] += a.blk[((size_t)box * (size_t)a.blocks + b) * WATER_ACC + q];
    }
    double us = 0.0;
    for (int b = 0; b < a.kblocks; ++b) us += a.ublk[(size_t)box * (size_t)a.kblocks + b];
    const double V = (gamd_box_edge(a, box, 0) * gamd_box_edge(a, box, 1)) * gamd_box_edge(a, box, 2);
    double* row = a.rows + ((size_t)a.slot * (size_t)nb + (size_t)box) * WATER_ROW;
    row[0] = 0.5 * s[0];                                    // every pair sits in two rows
    row[1] = 0.5 * s[1];
    row[2] = (a.coul4pi / V) * us;
    row[3] = -(a.self_c * ((a.q_h * a.q_h) * s[10]));
    row[4] = 0.5 * s[2];
#pragma unroll
    for (int q = 3; q < 9; ++q) row[q + 2] = s[q];
    row[11] = a.q_h * s[9];
    if (box == 0 && a.steps) a.steps[a.slot] = a.g;
}

}  // namespace

// the reciprocal-space kernels alone, for the force source (water_drive.hip): rho, S(k) and the per-atom k sums of a.x into
// a.rpart (and the block sums of A |S|^2 into a.ublk, which the source does not read)
int launch_water_recip(const WaterArgs& a, hipStream_t st) {
    PassGeom g;
    if (pass_rows(a, 3, &g) || pass_k_geometry(a, g.T, true)) return -1;
    if (!a.x || !a.species || !a.kvec || !a.rho_partial || !a.sk || !a.ublk || !a.rpart || !a.devflags) return -1;
    hipLaunchKernelGGL(k_water_rho, dim3(a.rho_blocks, (a.n_k + 63) / 64, g.nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_water_sk, dim3(a.kblocks, g.nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_water_recip, dim3((unsigned)(g.T * a.kslices), g.nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_water_sk(const WaterArgs& a, hipStream_t st) {
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1;
    if (nb > 65535 || a.n_k < 1 || a.n_k > (1 << 17) || a.kblocks != (a.n_k + 255) / 256 || a.rho_blocks < 1) return -1;
    if (!a.kvec || !a.rho_partial || !a.sk || !a.ublk || !a.devflags) return -1;
    hipLaunchKernelGGL(k_water_sk, dim3(a.kblocks, nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_water_final(const WaterArgs& a, hipStream_t st) {
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1;
    if (nb > 65535 || a.blocks < 1 || a.blocks > 65535 || a.slot < 0 || a.kblocks < 1) return -1;
    if (!a.blk || !a.ublk || !a.rows || !a.devflags) return -1;
    hipLaunchKernelGGL(k_water_final, dim3((nb + 63) / 64), dim3(64), 0, st, a); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_water_classical(const WaterArgs& a, hipStream_t st, const PmeArgs* pme, const CellTabBufs* cells) {
    PassGeom g;
    if (pass_geometry(a, 3, &g) || (!pme && pass_k_geometry(a, g.T, true)) || a.blocks < 1 || a.blocks > 65535 || a.slot < 0) return -1;
    if (!a.x || !a.species || !a.part || !a.ublk || !a.rpart || !a.f_cl || !a.blk || !a.rows || !a.devflags) return -1;
    if (!pme && (!a.kvec || !a.rho_partial || !a.sk)) return -1;
    if (cells) {                                            // gamd_water_cells: the pair rows over the cell table, one slice
        if (int r = launch_water_cells(a, *cells, nullptr, WATER_PART, true, st)) return r;
    } else {
        hipLaunchKernelGGL(k_water_pairs, dim3((unsigned)(g.T * a.slices), g.nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    }
    if (int r = pme ? launch_water_pme(*pme, st) : launch_water_recip(a, st)) return r;        // (its checks are among those above)
    hipLaunchKernelGGL(k_water_atoms, dim3(a.blocks, g.nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_water_final, dim3((g.nb + 63) / 64), dim3(64), 0, st, a); GAMD_CHECK_LAUNCH();
    return 0;
}
