// report.hip — the run reporter: what OpenMM's StateDataReporter logs in the reference's rollout drivers (step, kinetic
// energy, temperature; LJ/test_script/test_langevin.py:79-83 and the other five drivers) and the pair-distance histogram of
// a radial distribution function, taken on the device behind the second half of every interval-th step of an enqueued
// gamd_md_run / gamd_md_run_nhc.  No synchronisation, no host round trip, no copy inside the run (gamd_report_read fetches
// the results afterwards).
//
//   k_report_ke        per-block double sums of m |v|^2 over this block's share of box blockIdx.y (the layout of k_nhc_ke2 /
//                      k_com_partial of integrate.hip: fixed assignment of atoms to threads, fixed reduction tree)
//   k_report_ke_final  one thread per box adds the block sums in order and writes {g, KE} to the log row the HOST chose:
//                      a sample that is enqueued a second time after a freeze overwrites its own row with the same bits
//   k_report_rdf       one pass over the CSR edge slots of the force evaluation that has just run (positions do not move in
//                      the second half, so it is the pair list of the sampled frame): 32-bit bins in LDS per workgroup, one
//                      64-bit integer atomic per non-zero bin per workgroup.  Integer adds commute: the counts are exact
//                      and the same whatever the arrival order.
// Every kernel returns while DEVFLAG_FROZEN is set, like the integrator kernels: a frozen run adds nothing, the resumed run
// (gamd_sync_status -> enqueue_md_steps) enqueues the samples of the steps it replays.
#include "gamd_common.h"
#include "gamd_internal.h"

namespace {

__global__ void __launch_bounds__(256) k_report_ke(ReportArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    __shared__ double red[4];
    const int npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n, a0 = blockIdx.y * npb, a1 = a0 + npb;
    double s = 0.0;
    for (int i = a0 + blockIdx.x * blockDim.x + threadIdx.x; i < a1; i += gridDim.x * blockDim.x) {
#pragma clang fp contract(off)                              // the same bits whatever the compiler would like to fuse
        const double m = (a.species && a.mass_h > 0.0 && a.species[i] == 0) ? a.mass_h : a.mass;
        const double vx = (double)a.v[3 * i] / a.len, vy = (double)a.v[3 * i + 1] / a.len, vz = (double)a.v[3 * i + 2] / a.len;
        s += m * ((vx * vx + vy * vy) + vz * vz);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) a.partial[(size_t)blockIdx.y * a.blocks + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void k_report_ke_final(ReportArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1;
    const int box = blockIdx.x * blockDim.x + threadIdx.x;  // one thread per box
    if (box >= nb) return;
    double s = 0.0;
    for (int b = 0; b < a.blocks; ++b) s += a.partial[(size_t)box * a.blocks + b];
    a.ke[(size_t)a.slot * nb + box] = 0.5 * s;
    if (box == 0) a.steps[a.slot] = a.g;
}

__global__ void __launch_bounds__(256) k_report_rdf(ReportArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;                 // truncated CSR, or a frame that will be evaluated again
    __shared__ unsigned bins[GAMD_HIST_MAX_PAIRS * GAMD_HIST_MAX_BINS];
    const int n_slots = a.n_pairs * a.n_bins;               // <= 3072 (checked by gamd_report_configure)
    gamd_hist_zero(bins, n_slots);
    __syncthreads();

    const int box = blockIdx.y;
    const int npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n, a0 = box * npb, a1 = a0 + npb;
    // the CSR rows of a box are contiguous (its padding slots, source index n, sit behind its last row)
    long long E = a.counters[CNT_E];
    if (E > a.e_cap) E = a.e_cap;
    long long e0 = GAMD_CHK_RANGE(a.sticky, a.row_ptr[a0], 0, E, GAMD_CHK_REPORT_ROW);
    long long e1 = GAMD_CHK_RANGE(a.sticky, a.row_ptr[a1], 0, E, GAMD_CHK_REPORT_ROW);
    e0 = e0 < 0 ? 0 : (e0 > E ? E : e0);
    e1 = e1 < e0 ? e0 : (e1 > E ? E : e1);
    const BoxDims B = gamd_box_dims(a.bx, a.box, a.half, box);

    for (long long e = e0 + blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += (long long)gridDim.x * blockDim.x) {
        const int src = GAMD_CHK_RANGE(a.sticky, a.col[e], 0, a.n, GAMD_CHK_REPORT_SRC);
        const int dst = GAMD_CHK_RANGE(a.sticky, a.erow[e], 0, a.n, GAMD_CHK_REPORT_DST);
        if (src == a.n || dst == a.n || src == dst) continue;          // padding slot, self pair
        if (a.exclude_same_molecule) {
            const int is = GAMD_CHK_RANGE(a.sticky, a.perm[src], 0, a.n - 1, GAMD_CHK_REPORT_PERM);
            const int id = GAMD_CHK_RANGE(a.sticky, a.perm[dst], 0, a.n - 1, GAMD_CHK_REPORT_PERM);
            if (is / 3 == id / 3) continue;
        }
        gamd_hist_add(bins, a.pos_s[src], a.pos_s[dst], B, a.r_max, a.bin_scale, a.n_bins, a.n_pairs, a.all_edges, 1u);
    }
    __syncthreads();
    gamd_hist_flush(bins, a.counts + (size_t)box * n_slots, n_slots);
}

}  // namespace

int launch_report_ke(const ReportArgs& a, hipStream_t st) {
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1;
    hipLaunchKernelGGL(k_report_ke, dim3(a.blocks, nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_report_ke_final, dim3((nb + 63) / 64), dim3(64), 0, st, a); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_report_rdf(const ReportArgs& a, hipStream_t st) {
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1;
    if (a.n_bins < 1 || a.n_bins > GAMD_HIST_MAX_BINS || a.n_pairs < 1 || a.n_pairs > GAMD_HIST_MAX_PAIRS) return -1;
    hipLaunchKernelGGL(k_report_rdf, dim3(a.rdf_blocks, nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    return 0;
}
