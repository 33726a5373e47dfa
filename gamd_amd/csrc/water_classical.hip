// water_classical.hip — the water classical observer: the classical potential of 3-site water (O-O Lennard-Jones plus point
// charges, the reference's TIP3P labels: potential energy and getForces of dataset/generate_tip3p_data.py:91-103), with the
// electrostatics as a plain Ewald sum in double, on the device behind the second half of every interval-th step of an enqueued
// gamd_md_run / gamd_md_run_nhc, and the same kernels on given positions outside a run (gamd_water_eval).  Atoms in the CALLER's
// order O,H,H: molecule = index / 3, O = species != 0, q_O = -2 q_H.
//
//   k_water_pairs   k_classical_pairs' tiling: grid (T * slices, boxes), thread t of workgroup (I, s) keeps atom t of row tile I
//                   and walks the atoms [s * chunk, (s + 1) * chunk) of the box, staged 256 at a time in LDS as doubles plus
//                   their species flag.  FULL rows.  A same-molecule pair takes the erf branch (U_excl) whatever r is; a
//                   different-molecule pair with r^2 < r_cut^2 takes the erfc branch (U_real) and, O-O, the Lennard-Jones term
//                   of classical.hip.  Per atom and slice one partial row {Fx, Fy, Fz, u_LJ, u_real + u_excl, pairs}.
//   k_water_rho     k_struct_rho's scheme, charge-weighted: grid (blocks per box, K / 64, boxes), thread (w, l) owns k-vector l
//                   of its 64 and the atoms 4 m + w of every 256-atom chunk of its block (chunks staged in LDS as the wrapped
//                   fractional coordinate s and the charge, in double); one partial (re, im) per workgroup
//                   and k-vector, the four waves added as (w0 + w1) + (w2 + w3).
//   k_water_sk      grid (K / 256, boxes), one thread per (box, k): S(k) = the block partials added in order, k and
//                   A(k) = exp(-k^2 / 4 alpha^2) / k^2 (0 beyond the box's k_cut); {Re S, Im S, A} stored, and the
//                   workgroup's sum of A |S|^2 by the fixed tree.
//   k_water_recip   grid (T * kslices, boxes), thread t keeps atom t of row tile I (s = x / L) and walks the k-vectors
//                   [ks * kchunk, (ks + 1) * kchunk) in list order, staged 256 at a time in LDS {n, Re S, Im S, A}:
//                   g += A (Re S sin(k.r) + Im S cos(k.r)) n per component.
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

#include "gamd_potential_dev.h"

namespace {

constexpr int WC_TILE = 256;

__global__ void __launch_bounds__(256) k_water_pairs(WaterArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;                 // a frame that will be evaluated again
    __shared__ double sx[WC_TILE], sy[WC_TILE], sz[WC_TILE];
    __shared__ unsigned char so[WC_TILE];
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)a.slices), s = (int)(blockIdx.x % (unsigned)a.slices);
    const int box = blockIdx.y;
    const int npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const size_t a0 = (size_t)box * (size_t)npb;            // the caller's order is box-major
    if (I >= a.tiles) return;                               // (uniform; cannot happen with the launcher's grid)
    const int il = I * WC_TILE + tid;                       // atom of this thread inside its box
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
    // the thread's output row, held in vector registers from here on: left to the compiler, its uniform part stays in scalar
    // registers across the loop, which the potential's constants fill already (four scalar spills otherwise)
    double* out = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * WATER_PART;
    asm volatile("" : "+v"(out));
    double fx = 0.0, fy = 0.0, fz = 0.0, elj = 0.0, ec = 0.0, cnt = 0.0;
    for (long long base = jb; base < je; base += WC_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int nj = (int)(je - base < WC_TILE ? je - base : WC_TILE);
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
                ec += -(qq * t);
                fs = (qq * (gs - t)) * ir2;
            } else {                                        // U_real: q_i q_j erfc(alpha r) / r
                const double t = erfc(ar) / r;
                ec += qq * t;
                fs = (qq * (t + gs)) * ir2;
                cnt += 1.0;
                if (oi && oj) {                             // k_classical_pairs' term
                    const double2 lj = gamd_lj_term(a.sig2, a.eps4, 6.0 * a.eps4, a.u0, ir2);   // 6 (4 epsilon) = 24 epsilon bit for bit
                    double u = lj.x, ru = lj.y;
                    if (a.rs >= 0.0 && r > a.rs) {
                        const double2 sw = gamd_lj_switch(a.rs, a.inv_w, r);
                        ru = ru * sw.x + ((u * sw.y) * r);
                        u = u * sw.x;
                    }
                    elj += u;
                    fs = fs + -(ru * ir2);
                }
            }
            fx += fs * dx; fy += fs * dy; fz += fs * dz;
        }
    }
    if (vi) { out[0] = fx; out[1] = fy; out[2] = fz; out[3] = elj; out[4] = ec; out[5] = cnt; }
}

__global__ void __launch_bounds__(256) k_water_rho(WaterArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;
    __shared__ double sx[WC_TILE], sy[WC_TILE], sz[WC_TILE], sq[WC_TILE];
    __shared__ double red[4][2][64];                        // [wave][re, im][lane]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int box = blockIdx.z, npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n, a0 = box * npb, a1 = a0 + npb;
    const int k = blockIdx.y * 64 + lane;
    const bool vk = k < a.n_k;
    const double nx = vk ? (double)a.kvec[3 * (size_t)k] : 0.0, ny = vk ? (double)a.kvec[3 * (size_t)k + 1] : 0.0,
                 nz = vk ? (double)a.kvec[3 * (size_t)k + 2] : 0.0;
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    double re = 0.0, im = 0.0;
    for (int base = a0 + blockIdx.x * WC_TILE; base < a1; base += gridDim.x * WC_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int i = base + tid;
        if (i < a1) {
            sx[tid] = water_frac((double)a.x[3 * (size_t)i], Lx);
            sy[tid] = water_frac((double)a.x[3 * (size_t)i + 1], Ly);
            sz[tid] = water_frac((double)a.x[3 * (size_t)i + 2], Lz);
            sq[tid] = a.species[i] != 0 ? a.q_o : a.q_h;
        }
        __syncthreads();
        const int cnt = a1 - base < WC_TILE ? a1 - base : WC_TILE;
        for (int j = w; j < cnt; j += 4) {                  // (wave-uniform: one LDS address per wave)
            const double ph = (nx * sx[j] + ny * sy[j]) + nz * sz[j];
            double sn, cs;
            sincospi(2.0 * ph, &sn, &cs);
            re += sq[j] * cs; im -= sq[j] * sn;
        }
    }
    red[w][0][lane] = re; red[w][1][lane] = im;
    __syncthreads();
    if (w == 0 && vk) {
        double* out = a.rho_partial + (((size_t)box * a.rho_blocks + blockIdx.x) * (size_t)a.n_k + (size_t)k) * 2;
        out[0] = (red[0][0][lane] + red[1][0][lane]) + (red[2][0][lane] + red[3][0][lane]);
        out[1] = (red[0][1][lane] + red[1][1][lane]) + (red[2][1][lane] + red[3][1][lane]);
    }
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
    __shared__ double kn[3][WC_TILE], ks_re[WC_TILE], ks_im[WC_TILE], ks_a[WC_TILE];
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)a.kslices), s = (int)(blockIdx.x % (unsigned)a.kslices);
    const int box = blockIdx.y;
    const int npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const size_t a0 = (size_t)box * (size_t)npb;
    if (I >= a.tiles) return;                               // (uniform; cannot happen with the launcher's grid)
    const int il = I * WC_TILE + tid;
    const bool vi = il < npb;
    const long long kb = (long long)s * a.kchunk;
    const int ke = (int)(kb + a.kchunk < (long long)a.n_k ? kb + a.kchunk : (long long)a.n_k);
    double six = 0.0, siy = 0.0, siz = 0.0;
    if (vi) {
        const float* p = a.x + 3 * (a0 + (size_t)il);
        six = water_frac((double)p[0], gamd_box_edge(a, box, 0));
        siy = water_frac((double)p[1], gamd_box_edge(a, box, 1));
        siz = water_frac((double)p[2], gamd_box_edge(a, box, 2));
    }
    double gx = 0.0, gy = 0.0, gz = 0.0;
    for (long long base = kb; base < ke; base += WC_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int nk = (int)(ke - base < WC_TILE ? ke - base : WC_TILE);
        if (tid < nk) {
            const size_t k = (size_t)base + (size_t)tid;
            kn[0][tid] = (double)a.kvec[3 * k]; kn[1][tid] = (double)a.kvec[3 * k + 1]; kn[2][tid] = (double)a.kvec[3 * k + 2];
            const double* p = a.sk + ((size_t)box * (size_t)a.n_k + k) * 3;
            ks_re[tid] = p[0]; ks_im[tid] = p[1]; ks_a[tid] = p[2];
        }
        __syncthreads();
        if (!vi) continue;
        for (int kk = 0; kk < nk; ++kk) {
            const double nx = kn[0][kk], ny = kn[1][kk], nz = kn[2][kk];
            const double ph = (nx * six + ny * siy) + nz * siz;
            double sn, cs;
            sincospi(2.0 * ph, &sn, &cs);
            const double wk = ks_a[kk] * (ks_re[kk] * sn + ks_im[kk] * cs);
            gx += wk * nx; gy += wk * ny; gz += wk * nz;
        }
    }
    if (vi) {
        double* out = a.rpart + (((size_t)box * (size_t)a.kslices + (size_t)s) * (size_t)npb + (size_t)il) * 3;
        out[0] = gx; out[1] = gy; out[2] = gz;
    }
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
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1, npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const long long T = (npb + WC_TILE - 1) / WC_TILE;
    if (npb < 3 || npb % 3 || nb > 65535 || a.tiles != (int)T) return -1;
    if (a.n_k < 1 || a.n_k > (1 << 17) || a.kslices < 1 || a.kchunk < 1 || (long long)a.kslices * a.kchunk < a.n_k || T * a.kslices > 0x7fffffll) return -1;
    if (a.kblocks != (a.n_k + 255) / 256 || a.rho_blocks < 1 || a.rho_blocks > 65535) return -1;
    if (!a.x || !a.species || !a.kvec || !a.rho_partial || !a.sk || !a.ublk || !a.rpart || !a.devflags) return -1;
    hipLaunchKernelGGL(k_water_rho, dim3(a.rho_blocks, (a.n_k + 63) / 64, nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_water_sk, dim3(a.kblocks, nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_water_recip, dim3((unsigned)(T * a.kslices), nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
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

int launch_water_classical(const WaterArgs& a, hipStream_t st) {
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1, npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const long long T = (npb + WC_TILE - 1) / WC_TILE;
    if (npb < 3 || npb % 3 || nb > 65535 || a.tiles != (int)T || a.slices < 1 || a.chunk < 1 || a.blocks < 1 || a.blocks > 65535 || a.slot < 0) return -1;
    if ((long long)a.slices * a.chunk < npb || T * a.slices > 0x7fffffll) return -1;   // the slices cover a row; grid.x * 256 threads stay below 2^31
    if (a.n_k < 1 || a.n_k > (1 << 17) || a.kslices < 1 || a.kchunk < 1 || (long long)a.kslices * a.kchunk < a.n_k || T * a.kslices > 0x7fffffll) return -1;
    if (a.kblocks != (a.n_k + 255) / 256 || a.rho_blocks < 1 || a.rho_blocks > 65535) return -1;
    if (!a.x || !a.species || !a.kvec || !a.part || !a.rho_partial || !a.sk || !a.ublk || !a.rpart || !a.f_cl || !a.blk || !a.rows || !a.devflags) return -1;
    hipLaunchKernelGGL(k_water_pairs, dim3((unsigned)(T * a.slices), nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    if (int r = launch_water_recip(a, st)) return r;        // (its checks are among those above)
    hipLaunchKernelGGL(k_water_atoms, dim3(a.blocks, nb), dim3(256), 0, st, a); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_water_final, dim3((nb + 63) / 64), dim3(64), 0, st, a); GAMD_CHECK_LAUNCH();
    return 0;
}
