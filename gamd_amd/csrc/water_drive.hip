// water_drive.hip — the water classical force source (gamd_md_force_source with GAMD_FORCE_WATER_CLASSICAL, DESIGN.md section
// 4.11.1): the force evaluation of a step of an enqueued gamd_md_run / gamd_md_run_nhc whose forces come from the 3-site water
// potential of water_classical.hip (O-O Lennard-Jones plus a plain Ewald sum, in double) instead of the network.  Launched
// behind the neighbour stage of the step, where the edge encoder would start, on the run's fp32 positions in the CALLER's atom
// order O,H,H.  Five launches:
//
//   k_wsrc_pairs        k_water_pairs' walk (gamd_water_walk, gamd_passes_dev.h: the one body of both) with the force
//                       accumulators only: per atom and slice {Fx, Fy, Fz} into the first three doubles of the observer's
//                       partial row (the row keeps its WATER_PART stride; u_LJ, u_coul, pairs are not written).
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

#include "gamd_passes_dev.h"

namespace {

__global__ void __launch_bounds__(256) k_wsrc_pairs(WaterArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;                 // a step that will be evaluated again
    gamd_water_walk<3, true>(a, GamdPosF32{a.x});
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

int launch_water_drive(const WaterArgs& a, float* f_out, hipStream_t st, const PmeArgs* pme, const CellTabBufs* cells) {
    PassGeom g;
    if (pass_geometry(a, 3, &g)) return -1;
    if (!a.x || !a.species || !a.part || !a.rpart || !a.f_cl || !a.devflags || !f_out) return -1;
    if (cells) {                                            // gamd_water_cells: the force rows over the cell table, one slice
        if (int r = launch_water_cells(a, *cells, nullptr, 3, true, st)) return r;
    } else {
        hipLaunchKernelGGL(k_wsrc_pairs, dim3((unsigned)(g.T * a.slices), g.nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    }
    if (int r = pme ? launch_water_pme(*pme, st) : launch_water_recip(a, st)) return r;
    hipLaunchKernelGGL(k_wsrc_atoms, dim3((unsigned)g.T, g.nb), dim3(256), 0, st, a, f_out); GAMD_CHECK_LAUNCH();
    return 0;
}
