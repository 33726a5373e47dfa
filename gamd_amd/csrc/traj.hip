// traj.hip — the run recorder: what the reference's data generators dump every 50 steps (pos / vel / forces,
// dataset/generate_lj_data.py:93-106) and the dynamical observables that need the UNWRAPPED displacement (mean-squared
// displacement, velocity autocorrelation), taken on the device behind the second half of every interval-th step of an
// enqueued gamd_md_run / gamd_md_run_nhc.  The integrators wrap positions into the box every step; the recorder keeps an
// exact integer image count per atom and component instead of touching them: u = x + image * L.
//
//   k_traj_sample      one pass over the 3 n degrees of freedom (a workgroup owns 256 atoms = 768 consecutive floats, read
//                      as three coalesced rows of 256): image update against x_prev, ambiguity count (one integer atomic
//                      per workgroup), x_prev, the frame row the HOST chose, the ring slot the HOST chose
//   k_traj_classes     first sample only: atoms per box and class (plain stores)
//   k_traj_com (+ final)   subtract_com: mass-weighted mean of u per box into the ring slot, the layout of k_com_partial
//   k_traj_corr        grid (blocks per box, lags with an origin in the ring, boxes): per-class double sums of |du|^2 and
//                      v(q).v(o) in registers, shuffle + LDS tree, one partial row per workgroup
//   k_traj_corr_final  one thread per (box, lag, class) adds the block partials in order, then adds into the running sum
// Fixed atom-to-thread assignment, fixed number of blocks per box, no floating-point atomics, contraction off: the same
// bits run after run.  Every kernel returns while DEVFLAG_FROZEN is set.  The image counters, x_prev, the ring and the
// running sums are updated in place: they rely on a sample running exactly once unfrozen (the resumed run enqueues the
// samples of the steps it replays; the samples in front of the freeze are not enqueued again).
#include "gamd_common.h"
#include "gamd_internal.h"

namespace {

// fp32 edge `c` of the box atom i lives in
__device__ __forceinline__ float traj_edge(const TrajArgs& a, int i, int c) {
    if (a.bx.n_boxes <= 1) return a.box[c];
    const float4 b = a.bx.boxes[3 * gamd_box_of(a.bx, i)];
    return c == 0 ? b.x : (c == 1 ? b.y : b.z);
}
__device__ __forceinline__ float traj_box_edge(const TrajArgs& a, int box, int c) {
    if (a.bx.n_boxes <= 1) return a.box[c];
    const float4 b = a.bx.boxes[3 * box];
    return c == 0 ? b.x : (c == 1 ? b.y : b.z);
}

__global__ void __launch_bounds__(256) k_traj_sample(TrajArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    __shared__ unsigned char amb[768];
    __shared__ int wcnt[4];
    const long long n3 = 3ll * a.n, base = 768ll * blockIdx.x;
    const size_t ring = (size_t)a.slot * (size_t)n3, frame = (size_t)(a.frame < 0 ? 0 : a.frame) * (size_t)n3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int l = threadIdx.x + 256 * k;
        const long long t = base + l;
        unsigned char flag = 0;
        if (t < n3) {
            const int i = (int)(t / 3), c = (int)(t - 3ll * i);
            const float x = a.x[t];
            int img = 0;
            if (a.q > 0) {
#pragma clang fp contract(off)
                const double L = (double)traj_edge(a, i, c), d = (double)x - (double)a.x_prev[t];
                const double kk = rint(d / L);
                img = a.image[t] - (int)kk;                 // the atom left through a face and came back a box edge lower: +1
                flag = fabs(d - kk * L) > 0.25 * L ? 1 : 0;
            }
            a.x_prev[t] = x;
            a.image[t] = img;
            if (a.frame >= 0) {
                if (a.fx) a.fx[frame + t] = x;
                if (a.fv) a.fv[frame + t] = a.v[t];
                if (a.ff) a.ff[frame + t] = a.f[t];
                if (a.fimg) a.fimg[frame + t] = img;
            }
            if (a.n_lags > 0) {
                a.ring_x[ring + t] = x;
                a.ring_img[ring + t] = img;
                a.ring_v[ring + t] = a.v[t];
            }
        }
        amb[l] = flag;
    }
    if (a.frame >= 0 && blockIdx.x == 0 && threadIdx.x == 0) a.steps[a.frame] = a.g;
    if (a.q == 0) return;                                   // (uniform) nothing to compare the first sample with
    __syncthreads();
    // thread j looks at atom j of this workgroup: a component beyond a quarter of the box edge makes the image choice doubtful
    const int mine = (amb[3 * threadIdx.x] | amb[3 * threadIdx.x + 1] | amb[3 * threadIdx.x + 2]) ? 1 : 0;
    const int w = __popcll(__ballot(mine));
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int c = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
        if (c) atomicAdd(a.ambiguous, (unsigned long long)c);        // integer adds commute
    }
}

__global__ void __launch_bounds__(256) k_traj_classes(TrajArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    __shared__ int wcnt[4];
    const int box = blockIdx.x, npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n, a0 = box * npb, a1 = a0 + npb;
    int c = 0;
    if (a.classes == 2)
        for (int i = a0 + threadIdx.x; i < a1; i += blockDim.x) c += a.species[i] != 0 ? 1 : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_down(c, d, 64);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int n_o = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
        if (a.classes == 2) { a.class_atoms[2 * box] = n_o; a.class_atoms[2 * box + 1] = npb - n_o; }
        else a.class_atoms[box] = npb;
    }
}

__global__ void __launch_bounds__(256) k_traj_com(TrajArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    __shared__ double red[4][4];
    const int box = blockIdx.y, npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n, a0 = box * npb, a1 = a0 + npb;
    const double Lx = (double)traj_box_edge(a, box, 0), Ly = (double)traj_box_edge(a, box, 1), Lz = (double)traj_box_edge(a, box, 2);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = a0 + blockIdx.x * blockDim.x + threadIdx.x; i < a1; i += gridDim.x * blockDim.x) {
#pragma clang fp contract(off)
        const double m = (a.species && a.mass_h > 0.0 && a.species[i] == 0) ? a.mass_h : a.mass;
        s[0] += m * ((double)a.x[3 * i] + (double)a.image[3 * i] * Lx);
        s[1] += m * ((double)a.x[3 * i + 1] + (double)a.image[3 * i + 1] * Ly);
        s[2] += m * ((double)a.x[3 * i + 2] + (double)a.image[3 * i + 2] * Lz);
        s[3] += m;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s[k] += __shfl_down(s[k], d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) red[threadIdx.x >> 6][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < 4)
        a.com_partial[((size_t)box * a.com_blocks + blockIdx.x) * 4 + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ void k_traj_com_final(TrajArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1;
    const int box = blockIdx.x * blockDim.x + threadIdx.x;  // one thread per box
    if (box >= nb) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < a.com_blocks; ++b) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += a.com_partial[((size_t)box * a.com_blocks + b) * 4 + k];
    }
    double* out = a.ring_com + ((size_t)a.slot * nb + box) * 3;
    out[0] = s[0] / s[3]; out[1] = s[1] / s[3]; out[2] = s[2] / s[3];
}

__global__ void __launch_bounds__(256) k_traj_corr(TrajArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    __shared__ double red[4][4];
    const int box = blockIdx.z, j = blockIdx.y, nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1;
    const int npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n, a0 = box * npb, a1 = a0 + npb;
    const int so = (a.slot - j + a.n_lags) % a.n_lags;      // ring slot of the origin q - j (j < n_lags)
    const size_t n3 = 3 * (size_t)a.n;
    const float* xq = a.ring_x + (size_t)a.slot * n3; const float* xo = a.ring_x + (size_t)so * n3;
    const int* iq = a.ring_img + (size_t)a.slot * n3; const int* io = a.ring_img + (size_t)so * n3;
    const float* vq = a.ring_v + (size_t)a.slot * n3; const float* vo = a.ring_v + (size_t)so * n3;
    const double Lx = (double)traj_box_edge(a, box, 0), Ly = (double)traj_box_edge(a, box, 1), Lz = (double)traj_box_edge(a, box, 2);
    double cx = 0.0, cy = 0.0, cz = 0.0;                    // displacement of the box's centre of mass
    if (a.subtract_com) {
        const double* cq = a.ring_com + ((size_t)a.slot * nb + box) * 3; const double* co = a.ring_com + ((size_t)so * nb + box) * 3;
        cx = cq[0] - co[0]; cy = cq[1] - co[1]; cz = cq[2] - co[2];
    }
    double s[4] = {0.0, 0.0, 0.0, 0.0};                     // class 0: |du|^2, v.v; class 1: |du|^2, v.v
    for (int i = a0 + blockIdx.x * blockDim.x + threadIdx.x; i < a1; i += gridDim.x * blockDim.x) {
#pragma clang fp contract(off)
        const size_t t = 3 * (size_t)i;
        const double dx = (((double)xq[t] - (double)xo[t]) + (double)(iq[t] - io[t]) * Lx) - cx;
        const double dy = (((double)xq[t + 1] - (double)xo[t + 1]) + (double)(iq[t + 1] - io[t + 1]) * Ly) - cy;
        const double dz = (((double)xq[t + 2] - (double)xo[t + 2]) + (double)(iq[t + 2] - io[t + 2]) * Lz) - cz;
        const double r2 = (dx * dx + dy * dy) + dz * dz;
        const double vv = ((double)vq[t] * (double)vo[t] + (double)vq[t + 1] * (double)vo[t + 1]) + (double)vq[t + 2] * (double)vo[t + 2];
        const bool h = a.classes == 2 && a.species[i] == 0;
        s[0] += h ? 0.0 : r2; s[1] += h ? 0.0 : vv;
        s[2] += h ? r2 : 0.0; s[3] += h ? vv : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s[k] += __shfl_down(s[k], d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) red[threadIdx.x >> 6][k] = s[k];
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * a.classes)
        a.corr_partial[(((size_t)box * a.n_lags + j) * a.corr_blocks + blockIdx.x) * (2 * a.classes) + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ void k_traj_corr_final(TrajArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1;
    const long long total = (long long)nb * a.active * a.classes;
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;     // one thread per (box, lag, class)
    if (k >= total) return;
    const int c = (int)(k % a.classes), j = (int)((k / a.classes) % a.active), box = (int)(k / ((long long)a.classes * a.active));
    const double* p = a.corr_partial + ((size_t)box * a.n_lags + j) * a.corr_blocks * (2 * a.classes) + 2 * c;
    double m = 0.0, v = 0.0;
    for (int b = 0; b < a.corr_blocks; ++b) { m += p[(size_t)b * 2 * a.classes]; v += p[(size_t)b * 2 * a.classes + 1]; }
    const size_t o = ((size_t)box * a.classes + c) * a.n_lags + j;
    a.msd[o] += m;
    a.vacf[o] += v;
}

}  // namespace

int launch_traj_sample(const TrajArgs& a, hipStream_t st) {
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1;
    if (a.classes < 1 || a.classes > 2 || (a.classes == 2 && !a.species)) return -1;
    hipLaunchKernelGGL(k_traj_sample, dim3((a.n + 255) / 256), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    if (a.n_lags <= 0) return 0;
    if (a.active < 1 || a.active > a.n_lags || a.slot < 0 || a.slot >= a.n_lags) return -1;
    if (a.q == 0) { hipLaunchKernelGGL(k_traj_classes, dim3(nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH(); }
    if (a.subtract_com) {
        hipLaunchKernelGGL(k_traj_com, dim3(a.com_blocks, nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_traj_com_final, dim3((nb + 63) / 64), dim3(64), 0, st, a); GAMD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_traj_corr, dim3(a.corr_blocks, a.active, nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    const long long total = (long long)nb * a.active * a.classes;
    hipLaunchKernelGGL(k_traj_corr_final, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, st, a); GAMD_CHECK_LAUNCH();
    return 0;
}
