// classical.hip — the classical observer: the switched, shifted Lennard-Jones potential the reference's LJ data generators and
// rollout drivers evaluate with OpenMM (potentialEnergy / totalEnergy of dataset/generate_lj_data.py:87-90; gt_force of
// LJ/test_script/test_langevin.py:102-106), on the device behind the second half of every interval-th step of an enqueued
// gamd_md_run / gamd_md_run_nhc, and the same kernels on given positions outside a run (gamd_classical_eval).  r_cut (3 sigma)
// lies beyond the network's cutoff, so the edge list of the force evaluation cannot be walked: every ordered pair of a box is
// evaluated, N (N - 1) pair terms per box and sample, in double, from the caller's fp32 positions in the CALLER's atom order (the
// sorted order depends on the arrival order of the cell-fill atomics).
//
//   k_classical_pairs   the Lennard-Jones tile walk (gamd_lj_walk, gamd_passes_dev.h) on the fp32 positions widened, with every
//                       accumulator: per atom and slice one partial row {Fx, Fy, Fz, e_i, w_i, pairs_i}.  FULL rows: an atom's
//                       force is the sum of its own row, no atomics.
//   k_classical_atoms   grid (blocks per box, boxes): per atom, the slices' partial rows added in order from 0, f_cl = F * len;
//                       with f given, the atom's terms of the five force-error sums; per-thread sums over the thread's atoms
//                       (fixed assignment), then the fixed tree of k_report_ke (shuffle 32 .. 1, (w0 + w1) + (w2 + w3)).
//   k_classical_final   one thread per box adds the block rows in order and writes the row the HOST chose: E = sum e_i / 2,
//                       W = sum w_i / 2, pairs = sum pairs_i / 2 (halving is exact), the five sums, the atoms left out.
// With gamd_classical_cells on, launch_classical_cells (classical_cells.hip: cell_table.hip's per-box table and a pair pass over it, the
// same pairs in another order of the sums) stands where k_classical_pairs is, on ONE pair slice; the two kernels behind it are these.
// The arithmetic of a pair term is spelled out in DESIGN.md section 4.9 (tests/classical_ref.py mirrors it).  d_ij = -d_ji bit
// for bit (rint is odd), so u_ij = u_ji and F_ij = -F_ji bit for bit.  Fixed atom-to-thread assignment, fixed slices and
// blocks per handle, no floating-point atomics, contraction off: the same bits run after run.  Every kernel returns while
// DEVFLAG_FROZEN is set; nothing is updated in place, so a sample that runs twice writes the same bits twice.
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_passes_dev.h"

namespace {

__global__ void __launch_bounds__(256) k_classical_pairs(ClassicalArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;                 // a frame that will be evaluated again
    gamd_lj_walk<CLASSICAL_PART>(a, GamdPosF32{a.x});
}

__global__ void __launch_bounds__(256) k_classical_atoms(ClassicalArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    __shared__ double red[4][CLASSICAL_ROW];
    const int box = blockIdx.y;
    const int npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const size_t a0 = (size_t)box * (size_t)npb;
    double acc[CLASSICAL_ROW];
#pragma unroll
    for (int q = 0; q < CLASSICAL_ROW; ++q) acc[q] = 0.0;
    for (int il = blockIdx.x * blockDim.x + threadIdx.x; il < npb; il += gridDim.x * blockDim.x) {
        double t[CLASSICAL_PART];
#pragma unroll
        for (int q = 0; q < CLASSICAL_PART; ++q) t[q] = 0.0;
        for (int s = 0; s < a.slices; ++s) {
            const double* p = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * CLASSICAL_PART;
#pragma unroll
            for (int q = 0; q < CLASSICAL_PART; ++q) t[q] += p[q];
        }
        const size_t i = a0 + (size_t)il;
        const double cx = t[0] * a.len, cy = t[1] * a.len, cz = t[2] * a.len;      // kJ/mol/nm
        a.f_cl[3 * i] = cx; a.f_cl[3 * i + 1] = cy; a.f_cl[3 * i + 2] = cz;
        acc[0] += t[3]; acc[1] += t[4]; acc[2] += t[5];
        if (a.f) {
            gamd_force_error((double)a.f[3 * i], (double)a.f[3 * i + 1], (double)a.f[3 * i + 2], cx, cy, cz, acc[3], acc[4], acc[5],
                             acc[6], acc[7], acc[8]);
        }
    }
#pragma unroll
    for (int q = 0; q < CLASSICAL_ROW; ++q) {
        double v = acc[q];                                  // gamd_wave_sum, spelled out: the call moves this kernel's registers
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < CLASSICAL_ROW) {
        const int q = threadIdx.x;
        a.blk[((size_t)box * (size_t)a.blocks + blockIdx.x) * CLASSICAL_ROW + q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
    }
}

__global__ void k_classical_final(ClassicalArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1;
    const int box = blockIdx.x * blockDim.x + threadIdx.x;  // one thread per box
    if (box >= nb) return;
    double* row = a.rows + ((size_t)a.slot * (size_t)nb + (size_t)box) * CLASSICAL_ROW;
    for (int q = 0; q < CLASSICAL_ROW; ++q) {
        double s = 0.0;
        for (int b = 0; b < a.blocks; ++b) s += a.blk[((size_t)box * (size_t)a.blocks + b) * CLASSICAL_ROW + q];
        row[q] = q < 3 ? 0.5 * s : s;                       // every pair sits in two rows
    }
    if (box == 0 && a.steps) a.steps[a.slot] = a.g;
}

}  // namespace

int launch_classical(const ClassicalArgs& a, hipStream_t st, const CellTabBufs* cells) {
    PassGeom g;
    if (pass_geometry(a, 1, &g) || a.blocks < 1 || a.blocks > 65535 || a.slot < 0) return -1;
    if (!a.x || !a.part || !a.f_cl || !a.blk || !a.rows || !a.devflags) return -1;
    if (cells) {                                            // gamd_classical_cells: the pair rows over the cell table, one slice
        if (int r = launch_classical_cells(a, *cells, nullptr, nullptr, CLASSICAL_PART, st)) return r;
    } else {
        hipLaunchKernelGGL(k_classical_pairs, dim3((unsigned)(g.T * a.slices), g.nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_classical_atoms, dim3(a.blocks, g.nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_classical_final, dim3((g.nb + 63) / 64), dim3(64), 0, st, a); GAMD_CHECK_LAUNCH();
    return 0;
}
