// structure.hip — the structure sampler: the pair-distance histogram of a radial distribution function out to ANY r_max up
// to half the shortest box edge, and the partial static structure factors S_ab(k) on the box's reciprocal lattice, taken on
// the device behind the second half of every interval-th step of an enqueued gamd_md_run / gamd_md_run_nhc.  The run
// reporter's g(r) (report.hip) walks the edge list of the force evaluation and ends at the cutoff; this one evaluates every
// unordered pair of a box once, N (N - 1) / 2 distances per box and sample.
//
//   k_struct_pairs   grid (T (T + 1) / 2, boxes), T = 256-atom tiles per box: one workgroup per tile pair I <= J.  Tile J's
//                    rows of pos_s (and its molecule ids when intramolecular pairs are excluded) are staged in LDS; thread t
//                    keeps atom t of tile I in registers and walks tile J (every lane of a wave reads the same LDS address);
//                    the diagonal tile pairs count j > i only; tail tiles are masked.  A pair with r < r_max adds 2 (the
//                    reporter's directed-count convention) to a 32-bit LDS bin; every workgroup flushes its non-zero bins
//                    with one 64-bit integer atomic each.  Integer adds commute: the counts are exact and the same whatever
//                    the arrival order.
//   k_struct_rho     grid (blocks per box, K / 64, boxes): thread (w, l) owns k-vector l of its 64 and the atoms 4 m + w of
//                    every 256-atom chunk of its block (chunks staged in LDS as s = x / L in double); rho_c(n) = sum_i
//                    exp(-2 pi i n.s_i) per class in registers, the four waves added as (w0 + w1) + (w2 + w3), one partial row
//                    per workgroup.  Positions in the CALLER's order: the sorted order depends on atomics in the cell fill
//   k_struct_sk      one thread per (box, k): adds the block partials in order, then sk_sum[pair] += Re(rho_a conj(rho_b))
// Fixed atom-to-thread assignment, fixed number of blocks per box, no floating-point atomics, contraction off: the same
// bits run after run.  Every kernel returns while DEVFLAG_FROZEN is set; the counts and the in-place sk_sum update rely on a
// sample running exactly once unfrozen (the resumed run enqueues the samples of the steps it replays; the samples in front
// of the freeze are not enqueued again).
#include "gamd_common.h"
#include "gamd_internal.h"

namespace {

constexpr int STRUCT_TILE = 256;

__global__ void __launch_bounds__(256) k_struct_pairs(StructArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;                 // a frame that will be evaluated again
    __shared__ unsigned bins[GAMD_HIST_MAX_PAIRS * GAMD_HIST_MAX_BINS];
    __shared__ float4 tj[STRUCT_TILE];
    __shared__ int mj[STRUCT_TILE];
    const int tid = threadIdx.x;
    const int n_slots = a.n_pairs * a.n_bins;               // <= 3072 (checked by gamd_struct_configure)
    gamd_hist_zero(bins, n_slots);

    // tile pair p = J (J + 1) / 2 + I, I <= J < tiles
    const long long p = (long long)blockIdx.x;
    long long J = (long long)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while (J * (J + 1) / 2 > p) --J;
    while ((J + 1) * (J + 2) / 2 <= p) ++J;
    const long long I = p - J * (J + 1) / 2;
    if (I > J || J >= (long long)a.tiles) return;           // (uniform; cannot happen with the launcher's grid)

    const int box = blockIdx.y;
    const int npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const long long a0 = (long long)box * npb, a1 = a0 + npb;   // the sorted order is box-contiguous
    const long long i = a0 + I * STRUCT_TILE + tid, j0 = a0 + J * STRUCT_TILE;
    const bool vi = i < a1;
    const int nj = (int)(a1 - j0 < STRUCT_TILE ? a1 - j0 : STRUCT_TILE);
    const BoxDims B = gamd_box_dims(a.bx, a.box, a.half, box);

    float4 pi = make_float4(0.f, 0.f, 0.f, 0.f);
    int mi = -1;
    if (vi) {
        pi = a.pos_s[i];
        if (a.exclude_same_molecule) mi = GAMD_CHK_RANGE(a.sticky, a.perm[i], 0, a.n - 1, GAMD_CHK_STRUCT_PERM_I) / 3;
    }
    if (tid < nj) {
        tj[tid] = a.pos_s[j0 + tid];
        if (a.exclude_same_molecule) mj[tid] = GAMD_CHK_RANGE(a.sticky, a.perm[j0 + tid], 0, a.n - 1, GAMD_CHK_STRUCT_PERM_J) / 3;
    }
    __syncthreads();

    // diagonal tile pair: thread t takes j > t; the loop starts at the wave's first such j, so that the lanes of a wave stay
    // on one LDS address
    const bool diag = I == J;
    const int first = diag ? tid + 1 : 0;
    for (int jj = diag ? (tid & ~63) + 1 : 0; jj < nj; ++jj) {
        const float4 pj = tj[jj];
        if (!vi || jj < first) continue;
        if (a.exclude_same_molecule && mj[jj] == mi) continue;
        // r < r_max only; both directions of the pair (at most 2 * 256 * 256 per workgroup)
        gamd_hist_add(bins, pi, pj, B, a.r_max, a.bin_scale, a.n_bins, a.n_pairs, 0, 2u);
    }
    __syncthreads();
    gamd_hist_flush(bins, a.counts + (size_t)box * n_slots, n_slots);
}

// fp32 edge `c` of box `box`
__device__ __forceinline__ float struct_box_edge(const StructArgs& a, int box, int c) {
    if (a.bx.n_boxes <= 1) return a.box[c];
    const float4 b = a.bx.boxes[3 * box];
    return c == 0 ? b.x : (c == 1 ? b.y : b.z);
}

__global__ void __launch_bounds__(256) k_struct_rho(StructArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    __shared__ double sx[STRUCT_TILE], sy[STRUCT_TILE], sz[STRUCT_TILE];
    __shared__ unsigned char cls[STRUCT_TILE];
    __shared__ double red[4][4][64];                        // [wave][class re, class im][lane]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int box = blockIdx.z, npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n, a0 = box * npb, a1 = a0 + npb;
    const int k = blockIdx.y * 64 + lane;
    const bool vk = k < a.n_k;
    const double nx = vk ? (double)a.kvec[3 * k] : 0.0, ny = vk ? (double)a.kvec[3 * k + 1] : 0.0, nz = vk ? (double)a.kvec[3 * k + 2] : 0.0;
    const double Lx = (double)struct_box_edge(a, box, 0), Ly = (double)struct_box_edge(a, box, 1), Lz = (double)struct_box_edge(a, box, 2);
    double s[4] = {0.0, 0.0, 0.0, 0.0};                     // class 0: re, im; class 1: re, im
    for (int base = a0 + blockIdx.x * STRUCT_TILE; base < a1; base += gridDim.x * STRUCT_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int i = base + tid;
        if (i < a1) {
#pragma clang fp contract(off)
            sx[tid] = (double)a.x[3 * (size_t)i] / Lx;
            sy[tid] = (double)a.x[3 * (size_t)i + 1] / Ly;
            sz[tid] = (double)a.x[3 * (size_t)i + 2] / Lz;
            cls[tid] = (a.classes == 2 && a.species[i] == 0) ? 1 : 0;
        }
        __syncthreads();
        const int cnt = a1 - base < STRUCT_TILE ? a1 - base : STRUCT_TILE;
        for (int j = w; j < cnt; j += 4) {                  // (wave-uniform: one LDS address per wave)
#pragma clang fp contract(off)
            const double ph = (nx * sx[j] + ny * sy[j]) + nz * sz[j];
            double sn, cs;
            sincospi(2.0 * ph, &sn, &cs);
            const bool h = cls[j] != 0;
            s[0] += h ? 0.0 : cs; s[1] -= h ? 0.0 : sn;
            s[2] += h ? cs : 0.0; s[3] -= h ? sn : 0.0;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) red[w][q][lane] = s[q];
    __syncthreads();
    if (w == 0 && vk) {
        double* out = a.rho_partial + ((size_t)box * a.rho_blocks + blockIdx.x) * (size_t)a.classes * (size_t)a.n_k * 2;
        for (int c = 0; c < a.classes; ++c) {
            out[((size_t)c * a.n_k + k) * 2] = (red[0][2 * c][lane] + red[1][2 * c][lane]) + (red[2][2 * c][lane] + red[3][2 * c][lane]);
            out[((size_t)c * a.n_k + k) * 2 + 1] =
                (red[0][2 * c + 1][lane] + red[1][2 * c + 1][lane]) + (red[2][2 * c + 1][lane] + red[3][2 * c + 1][lane]);
        }
    }
}

__global__ void __launch_bounds__(64) k_struct_sk(StructArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    const int box = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;    // one thread per (box, k)
    if (k >= a.n_k) return;
    double re[2] = {0.0, 0.0}, im[2] = {0.0, 0.0};
    for (int b = 0; b < a.rho_blocks; ++b) {
        const double* p = a.rho_partial + ((size_t)box * a.rho_blocks + b) * (size_t)a.classes * (size_t)a.n_k * 2;
        for (int c = 0; c < a.classes; ++c) {
            re[c] += p[((size_t)c * a.n_k + k) * 2];
            im[c] += p[((size_t)c * a.n_k + k) * 2 + 1];
        }
    }
    double* out = a.sk_sum + (size_t)box * a.n_pairs * (size_t)a.n_k + k;
    {
#pragma clang fp contract(off)
        if (a.n_pairs == 1) {
            out[0] += re[0] * re[0] + im[0] * im[0];
        } else {
            out[0] += re[0] * re[0] + im[0] * im[0];
            out[(size_t)a.n_k] += re[0] * re[1] + im[0] * im[1];
            out[2 * (size_t)a.n_k] += re[1] * re[1] + im[1] * im[1];
        }
    }
}

}  // namespace

int launch_struct_pairs(const StructArgs& a, hipStream_t st) {
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1, npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    if (a.n_bins < 1 || a.n_bins > GAMD_HIST_MAX_BINS || a.n_pairs < 1 || a.n_pairs > GAMD_HIST_MAX_PAIRS || nb > 65535) return -1;
    const long long T = (npb + STRUCT_TILE - 1) / STRUCT_TILE, grid = T * (T + 1) / 2;
    if (a.tiles != (int)T || grid > 0xffffffll) return -1;          // grid.x * 256 threads must stay below 2^32
    hipLaunchKernelGGL(k_struct_pairs, dim3((unsigned)grid, nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_struct_sk(const StructArgs& a, hipStream_t st) {
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1;
    if (a.n_k < 1 || a.classes < 1 || a.classes > 2 || (a.classes == 2 && !a.species) || a.n_pairs != (a.classes == 2 ? 3 : 1) ||
        a.rho_blocks < 1 || nb > 65535)
        return -1;
    hipLaunchKernelGGL(k_struct_rho, dim3(a.rho_blocks, (a.n_k + 63) / 64, nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_struct_sk, dim3((a.n_k + 63) / 64, nb), dim3(64), 0, st, a); GAMD_CHECK_LAUNCH();
    return 0;
}
