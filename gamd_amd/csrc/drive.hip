// drive.hip — the classical force source (gamd_md_force_source): the force evaluation of a step of an
// enqueued gamd_md_run / gamd_md_run_nhc whose forces come from the switched, shifted Lennard-Jones potential of classical.hip
// instead of the network.  Launched behind the neighbour stage of the step, where the edge encoder would start, on the run's
// fp32 positions in the CALLER's atom order:
//
//   k_drive_lj_pairs    k_classical_pairs' walk (gamd_lj_walk, gamd_passes_dev.h: the one body of both) with the force
//                       accumulators only: per atom and slice {Fx, Fy, Fz} into the first three doubles of the observer's
//                       partial row (the row keeps its CLASSICAL_PART stride; e_i, w_i, pairs_i are not written).
//   k_drive_lj_atoms    one thread per atom: the slices' partials added in order from 0, f_cl = F * len in double to f_cl, and
//                       (float)f_cl (round to nearest) to the run's force buffer.
// With gamd_classical_cells on, launch_classical_cells (cell_table.hip's table, then k_ljcell_force of classical_cells.hip) stands where
// k_drive_lj_pairs is, on ONE pair slice: the force terms and their order are those of the observer's cell pass, so the contract below holds there too.
// No energy sums, no error sums, no final kernel.  The force bits are those of k_classical_pairs / k_classical_atoms on the same
// positions: f == fp32(f_cl of gamd_classical_eval) bit for bit.  `part` and `f_cl` are shared with the observer on one stream;
// a step that is driven and sampled evaluates twice and writes the same bits twice.  Fixed assignment, no floating-point
// atomics, contraction off, plain stores; every kernel returns while DEVFLAG_FROZEN is set, so a step enqueued again after a
// freeze writes the same bits.
// (No kernel uses a value it read from memory as an address: the checked build has nothing to range-check here.)
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_passes_dev.h"

namespace {

__global__ void __launch_bounds__(256) k_drive_lj_pairs(ClassicalArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;                 // a step that will be evaluated again
    gamd_lj_walk<3>(a, GamdPosF32{a.x});
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

int launch_classical_drive(const ClassicalArgs& a, float* f_out, hipStream_t st, const CellTabBufs* cells) {
    PassGeom g;
    if (pass_geometry(a, 1, &g)) return -1;
    if (!a.x || !a.part || !a.f_cl || !a.devflags || !f_out) return -1;
    if (cells) {                                            // gamd_classical_cells: the force rows over the cell table, one slice
        if (int r = launch_classical_cells(a, *cells, nullptr, nullptr, 3, st)) return r;
    } else {
        hipLaunchKernelGGL(k_drive_lj_pairs, dim3((unsigned)(g.T * a.slices), g.nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_drive_lj_atoms, dim3((unsigned)g.T, g.nb), dim3(256), 0, st, a, f_out); GAMD_CHECK_LAUNCH();
    return 0;
}
