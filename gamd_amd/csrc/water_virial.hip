// water_virial.hip — the molecular virial of the water classical potential (gamd_water_virial): the
// terms of W_mol = W_LJ + W_coul,pair + W_recip - W_intra and the centre-of-mass kinetic energy of a box of rigid molecules,
// per box in double, in a log row of their own beside the observer's.  Launched BEHIND the observer's kernels of the same
// frame (launch_water_classical / launch_w4_classical), whose f_cl and S(k) table it reads; it writes into buffers of its own
// only, so the observer's rows, f_cl and every force source are what they are without it.  Atoms in the CALLER's order O,H,H.
//
//   k_wvir_pairs    k_water_pairs' walk (gamd_water_walk, gamd_passes_dev.h: the one body) with the virial's accumulators in
//                   place of the forces and energies: the same pairs by the same tests, per atom and slice
//                   {sum -(r u_LJ'(r)), sum fs_coul r^2} into `vpart`.
//   k_wvir_pairs4   the same on the charge sites with the Lennard-Jones term off (k_w4_pairs' walk): {0, sum fs_coul r^2}.
//   k_wvir_lj4      k_w4_lj's pass over oxygens, its cutoff test on the O-O distance: per molecule and slice sum -(r u_LJ'(r)).
//   k_wvir_sk       one thread per (box, k) reads {Re S, Im S, A} as k_water_sk left them, forms k^2 by k_water_sk's own
//                   operations and adds A |S|^2 (1 - k^2 / (2 alpha^2)) by k_water_sk's tree: one sum per workgroup.
//   k_wvir_mols     one thread per molecule (grid-stride over the box's molecules, whatever tile or slice its atoms sit in):
//                   the pair slices of its three rows added in order from 0 (O, H1, H2, then the molecule's Lennard-Jones
//                   slices with an M-site), d_k = H_k - O by the minimum image, s_O = -(m_H / M)(d_1 + d_2), s_Hk = d_k + s_O,
//                   sum_a s_a . F_a / len from f_cl, and |m_O v_O + m_H (v_H1 + v_H2)|^2 / M; the block tree of k_report_ke.
//   k_wvir_final    one thread per box adds the block rows in order (and the k blocks in order) and writes the row the HOST chose.
// Everything in double; fixed molecule-to-thread and k-to-thread assignment, fixed slices and blocks per handle, no
// floating-point atomics, contraction off, nothing updated in place: the same bits run after run.  Every kernel returns while
// DEVFLAG_FROZEN is set.  (No kernel uses a value it read from memory as an address.)
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_passes_dev.h"

namespace {

__global__ void __launch_bounds__(256) k_wvir_pairs(WVirArgs b) {
    if (b.w.devflags[DEVFLAG_FROZEN]) return;               // a frame that will be evaluated again
    gamd_water_walk<0, true, true>(b.w, GamdPosF32{b.w.x}, b.vpart);
}

__global__ void __launch_bounds__(256) k_wvir_pairs4(WVirArgs b) {
    if (b.w.devflags[DEVFLAG_FROZEN]) return;
    gamd_water_walk<0, false, true>(b.w, GamdPosF64{b.sites}, b.vpart);  // w_LJ: k_wvir_lj4's
}

// k_w4_lj's walk (water_msite.hip) with its one accumulator: thread t of workgroup (I, s) keeps the oxygen of molecule
// I * 256 + t and walks the molecules [s * mchunk, (s + 1) * mchunk), staged 256 at a time
__global__ void __launch_bounds__(256) k_wvir_lj4(WVirArgs b) {
    const WaterArgs& a = b.w;
    if (a.devflags[DEVFLAG_FROZEN]) return;
    __shared__ double sx[GAMD_PASS_TILE], sy[GAMD_PASS_TILE], sz[GAMD_PASS_TILE];
    __shared__ unsigned char so[GAMD_PASS_TILE];
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)a.slices), s = (int)(blockIdx.x % (unsigned)a.slices);
    const int box = blockIdx.y;
    const int npb = gamd_npb(a), nm = npb / 3;
    const size_t a0 = (size_t)box * (size_t)npb;
    const int ml = I * GAMD_PASS_TILE + tid;                // molecule of this thread inside its box
    if (I * GAMD_PASS_TILE >= nm) return;                   // (uniform; cannot happen with the launcher's grid)
    const bool vi = ml < nm;
    const long long jb = (long long)s * b.mchunk;
    const int je = (int)(jb + b.mchunk < (long long)nm ? jb + b.mchunk : (long long)nm);
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    double xi = 0.0, yi = 0.0, zi = 0.0;
    bool oi = false;
    if (vi) {
        const float* p = a.x + 3 * (a0 + 3 * (size_t)ml);
        xi = (double)p[0]; yi = (double)p[1]; zi = (double)p[2];
        oi = a.species[a0 + 3 * (size_t)ml] != 0;
    }
    double wlj = 0.0;
    for (long long base = jb; base < je; base += GAMD_PASS_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int nj = (int)(je - base < GAMD_PASS_TILE ? je - base : GAMD_PASS_TILE);
        if (tid < nj) {
            const size_t j = a0 + 3 * ((size_t)base + (size_t)tid);
            const float* p = a.x + 3 * j;
            sx[tid] = (double)p[0]; sy[tid] = (double)p[1]; sz[tid] = (double)p[2];
            so[tid] = a.species[j] != 0 ? 1 : 0;
        }
        __syncthreads();
        if (!vi || !oi) continue;
        const int self = (int)((long long)ml - base);       // this molecule's own slot in the chunk, if it is there
        for (int jj = 0; jj < nj; ++jj) {
            double dx = xi - sx[jj], dy = yi - sy[jj], dz = zi - sz[jj];
            dx = dx - Lx * rint(dx / Lx);
            dy = dy - Ly * rint(dy / Ly);
            dz = dz - Lz * rint(dz / Lz);
            const double r2 = (dx * dx + dy * dy) + dz * dz;
            if (jj == self || so[jj] == 0 || !(r2 < a.rc2)) continue;  // the cutoff test on the O-O distance
            const double ir2 = 1.0 / r2;
            const double2 lj = gamd_lj_pair_r2(a, 6.0 * a.eps4, ir2, r2);
            wlj += -lj.y;
        }
    }
    if (vi) b.vljpart[((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)nm + (size_t)ml] = wlj;
}

__global__ void __launch_bounds__(256) k_wvir_sk(WVirArgs b) {
    const WaterArgs& a = b.w;
    if (a.devflags[DEVFLAG_FROZEN]) return;
    __shared__ double red[4];
    const int box = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;    // one thread per (box, k)
    double t = 0.0;
    if (k < a.n_k) {
        const double* p = a.sk + ((size_t)box * (size_t)a.n_k + (size_t)k) * 3;
        const double re = p[0], im = p[1], A = p[2];
        const double kx = a.two_pi * ((double)a.kvec[3 * (size_t)k] / gamd_box_edge(a, box, 0));
        const double ky = a.two_pi * ((double)a.kvec[3 * (size_t)k + 1] / gamd_box_edge(a, box, 1));
        const double kz = a.two_pi * ((double)a.kvec[3 * (size_t)k + 2] / gamd_box_edge(a, box, 2));
        const double k2 = (kx * kx + ky * ky) + kz * kz;
        t = (A * (re * re + im * im)) * (1.0 - 2.0 * (k2 * a.inv_4a2));          // k^2 / (2 alpha^2) = 2 k^2 / (4 alpha^2)
    }
    t = gamd_wave_sum(t);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) b.vublk[(size_t)box * (size_t)a.kblocks + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void __launch_bounds__(256) k_wvir_mols(WVirArgs b) {
    const WaterArgs& a = b.w;
    if (a.devflags[DEVFLAG_FROZEN]) return;
    __shared__ double red[4][WATER_VIR_ACC];
    const int box = blockIdx.y;
    const int npb = gamd_npb(a), nm = npb / 3;
    const size_t a0 = (size_t)box * (size_t)npb;
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    const double M = b.mass_o + (b.mass_h + b.mass_h), mu = b.mass_h / M;
    double acc[WATER_VIR_ACC];
#pragma unroll
    for (int q = 0; q < WATER_VIR_ACC; ++q) acc[q] = 0.0;
    for (int ml = blockIdx.x * blockDim.x + threadIdx.x; ml < nm; ml += gridDim.x * blockDim.x) {
        const int il = 3 * ml;                              // the oxygen's row; npb is a multiple of 3: il + 2 < npb
        double wlj = 0.0, wc = 0.0;
        for (int k = 0; k < 3; ++k)
            for (int s = 0; s < a.slices; ++s) {
                const double* p = b.vpart + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)(il + k)) * WATER_VIR_PART;
                wlj += p[0]; wc += p[1];
            }
        if (b.vljpart)
            for (int s = 0; s < a.slices; ++s) wlj += b.vljpart[((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)nm + (size_t)ml];
        const size_t i = a0 + (size_t)il;
        const float* o = a.x + 3 * i;
        const double ox = (double)o[0], oy = (double)o[1], oz = (double)o[2];
        double ax = (double)o[3] - ox, ay = (double)o[4] - oy, az = (double)o[5] - oz;
        double bx = (double)o[6] - ox, by = (double)o[7] - oy, bz = (double)o[8] - oz;
        ax = ax - Lx * rint(ax / Lx); ay = ay - Ly * rint(ay / Ly); az = az - Lz * rint(az / Lz);
        bx = bx - Lx * rint(bx / Lx); by = by - Ly * rint(by / Ly); bz = bz - Lz * rint(bz / Lz);
        const double sox = -(mu * (ax + bx)), soy = -(mu * (ay + by)), soz = -(mu * (az + bz));     // s_O = O - R_mol
        const double* F = a.f_cl + 3 * i;                   // kJ/mol/nm, O, H1, H2
        const double wo = (sox * F[0] + soy * F[1]) + soz * F[2];
        const double w1 = ((ax + sox) * F[3] + (ay + soy) * F[4]) + (az + soz) * F[5];
        const double w2 = ((bx + sox) * F[6] + (by + soy) * F[7]) + (bz + soz) * F[8];
        acc[0] += wlj; acc[1] += wc;
        acc[2] += ((wo + w1) + w2) / a.len;
        if (b.v) {
            const float* v = b.v + 3 * i;
            const double px = (b.mass_o * ((double)v[0] / a.len) + b.mass_h * ((double)v[3] / a.len)) + b.mass_h * ((double)v[6] / a.len);
            const double py = (b.mass_o * ((double)v[1] / a.len) + b.mass_h * ((double)v[4] / a.len)) + b.mass_h * ((double)v[7] / a.len);
            const double pz = (b.mass_o * ((double)v[2] / a.len) + b.mass_h * ((double)v[5] / a.len)) + b.mass_h * ((double)v[8] / a.len);
            acc[3] += ((px * px + py * py) + pz * pz) / M;
        }
    }
#pragma unroll
    for (int q = 0; q < WATER_VIR_ACC; ++q) {
        const double v = gamd_wave_sum(acc[q]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < WATER_VIR_ACC) {
        const int q = threadIdx.x;
        b.vblk[((size_t)box * (size_t)a.blocks + blockIdx.x) * WATER_VIR_ACC + q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
    }
}

__global__ void k_wvir_final(WVirArgs b) {
    const WaterArgs& a = b.w;
    if (a.devflags[DEVFLAG_FROZEN]) return;
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1;
    const int box = blockIdx.x * blockDim.x + threadIdx.x;  // one thread per box
    if (box >= nb) return;
    double s[WATER_VIR_ACC];
#pragma unroll
    for (int q = 0; q < WATER_VIR_ACC; ++q) {
        s[q] = 0.0;
        for (int k = 0; k < a.blocks; ++k) s[q] += b.vblk[((size_t)box * (size_t)a.blocks + k) * WATER_VIR_ACC + q];
    }
    double us = 0.0;
    for (int k = 0; k < a.kblocks; ++k) us += b.vublk[(size_t)box * (size_t)a.kblocks + k];
    const double V = (gamd_box_edge(a, box, 0) * gamd_box_edge(a, box, 1)) * gamd_box_edge(a, box, 2);
    double* row = b.vrows + ((size_t)a.slot * (size_t)nb + (size_t)box) * WATER_VIR_ROW;
    const double wlj = 0.5 * s[0], wc = 0.5 * s[1];         // every pair sits in two rows
    const double wr = (a.coul4pi / V) * us;
    row[0] = wlj; row[1] = wc; row[2] = wr; row[3] = s[2];
    row[4] = 0.5 * s[3];
    row[5] = ((wlj + wc) + wr) - s[2];
}

}  // namespace

int launch_water_virial(const WVirArgs& b, hipStream_t st) {
    const WaterArgs& a = b.w;
    PassGeom g;
    if (pass_geometry(a, 3, &g) || pass_k_geometry(a, g.T, true) || a.blocks < 1 || a.blocks > 65535 || a.slot < 0) return -1;
    if (!a.x || !a.species || !a.kvec || !a.sk || !a.f_cl || !a.devflags) return -1;
    if (!b.vpart || !b.vublk || !b.vblk || !b.vrows) return -1;
    if (!(b.mass_o > 0.0) || !(b.mass_h > 0.0)) return -1;
    if (b.w_h != 0.0) {
        if (!b.sites || !b.vljpart || b.mchunk < 1 || (long long)a.slices * b.mchunk < g.npb / 3) return -1;
        const long long Tm = (g.npb / 3 + GAMD_PASS_TILE - 1) / GAMD_PASS_TILE;
        hipLaunchKernelGGL(k_wvir_pairs4, dim3((unsigned)(g.T * a.slices), g.nb), dim3(256), 0, st, b); GAMD_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_wvir_lj4, dim3((unsigned)(Tm * a.slices), g.nb), dim3(256), 0, st, b); GAMD_CHECK_LAUNCH();
    } else {
        if (b.vljpart) return -1;
        hipLaunchKernelGGL(k_wvir_pairs, dim3((unsigned)(g.T * a.slices), g.nb), dim3(256), 0, st, b); GAMD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_wvir_sk, dim3(a.kblocks, g.nb), dim3(256), 0, st, b); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_wvir_mols, dim3(a.blocks, g.nb), dim3(256), 0, st, b); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_wvir_final, dim3((g.nb + 63) / 64), dim3(64), 0, st, b); GAMD_CHECK_LAUNCH();
    return 0;
}
