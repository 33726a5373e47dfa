// water_minimize.hip — the water energy minimiser (gamd_water_minimize): FIRE (Bitzek et al., Phys. Rev.
// Lett. 97, 170201 (2006)) in the semi-implicit Euler form on RIGID 3-site molecules, per box, under the water potential of
// water_classical.hip (O-O Lennard-Jones plus a plain Ewald sum), with positions, velocities, forces and every scalar in double
// on the device.  Every water driver of the reference calls OpenMM's minimizeEnergy in front of its first step
// (dataset/generate_tip3p_data.py:85); this is not its L-BFGS, which treats the constraints by restraints — what is shared is
// the meaning of the tolerance.  Atoms in the CALLER's order O,H,H, molecule = index / 3.  The constraint arithmetic
// (gamd_wmin_dev.h) takes unit weights for the three atoms: the projection is the orthogonal one and the projected force F_c is
// the gradient on the constraint manifold.  One iteration is six launches:
//
//   k_wmin_pairs    the pair pass of k_water_pairs — same grid (T * slices, boxes), same 256-atom row tiles, same slices, same
//                   staging, the same operations on d, r2, qq, gs, t and fs in the same order, the same-molecule erf branch,
//                   the erfc branch and the O-O Lennard-Jones term — on the DOUBLE positions x64: per atom and slice
//                   {Fx, Fy, Fz, u_LJ, u_real + u_excl} into the first five doubles of the observer's partial row.
//   k_wmin_rho      k_water_rho on x64 (water_frac of the double position).
//   k_water_sk      the observer's own kernel, unchanged (launch_water_sk): it reads no positions.
//   k_wmin_recip    k_water_recip's term on x64; k slice s walks the 256-vector blocks s, s + kslices, ... of the list in
//                   order, so that a longer list only appends terms of weight zero to a slice.
//   k_wmin_mols     grid (blocks per box, boxes), one molecule at a time per thread: per atom the pair slices added in order
//                   from 0, the k slices added in order from 0, F as k_water_atoms forms f_cl (kJ/mol/nm); F and v projected
//                   onto the tangent space of the three bond constraints at x64, F_c to f64 and v to v64; the molecule's terms
//                   of ff = sum F_c.F_c, vf = sum v.F_c, vv = sum v.v, sum u_LJ, sum u_coul, sum z^2 and max |F_c|; per-thread
//                   sums over the thread's molecules (fixed assignment), then the tree of k_report_ke into one row per block.
//   k_wmin_update   grid (molecule tiles, boxes), one thread per molecule.  EVERY thread adds the block rows in order (and the
//                   k blocks' A |S|^2 in order) and takes the same decisions from the same bits: U = ((U_coul + U_recip) +
//                   U_self) + U_LJ with the terms of k_water_final, rms = sqrt(ff / 3N); then k_min_update's decisions and
//                   FIRE's mixing on F_c, v += dt F_c, dr = dt v, ONE factor per molecule so that the largest |dr| of its
//                   three atoms is at most max_step, and x64 <- SETTLE(reference x64, new x64 + dr).
//
// Scalar state, the two slots per box, the `stopped` gate and the rows are minimize.hip's.  Fixed assignment, no floating-point
// atomics, contraction off, plain stores: the same bits run after run, and a box gets the bits it gets alone.
// (No kernel uses a value it read from memory as an address: the checked build has nothing to range-check here.)
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_potential_dev.h"
#include "gamd_wmin_dev.h"

namespace {

using namespace gamd_wmin;

constexpr int WM_TILE = 256;

__device__ __forceinline__ int wmin_npb(const WaterArgs& a) { return a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n; }

// x64 = x widened and put on the exact rigid geometry (SETTLE with reference = new = the input), v = 0, the scalar state of
// iteration 0, the gate open, the row cleared
__global__ void __launch_bounds__(256) k_wmin_init(WMinArgs m, const float* __restrict__ x) {
    const int box = blockIdx.y, nmol = wmin_npb(m.w) / 3;
    const int ml = blockIdx.x * WM_TILE + threadIdx.x;
    if (ml == 0) {
        double* st = m.state + (size_t)box * 2 * MIN_STATE;
        st[0] = m.dt_start; st[1] = m.alpha_start; st[2] = 0.0; st[3] = 0.0;
        for (int q = 0; q < MIN_ROW; ++q) m.rows[(size_t)box * MIN_ROW + q] = 0.0;
        m.stopped[box] = 0;
    }
    if (ml >= nmol) return;
    const size_t mol = (size_t)box * (size_t)nmol + (size_t)ml;
    D3 x0[3], x1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x0[k] = {(double)x[9 * mol + 3 * k], (double)x[9 * mol + 3 * k + 1], (double)x[9 * mol + 3 * k + 2]};
        x1[k] = x0[k];
    }
    settle(x0, x1, m.ra, m.rb, m.rc);
    store_mol(m.x64, mol, x1);
    const D3 zero[3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    store_mol(m.v64, mol, zero);
}

__global__ void __launch_bounds__(256) k_wmin_pairs(WMinArgs m) {
    const WaterArgs& a = m.w;
    const int box = blockIdx.y;
    if (m.stopped[box]) return;                             // the box has stopped: its positions stay
    __shared__ double sx[WM_TILE], sy[WM_TILE], sz[WM_TILE];
    __shared__ unsigned char so[WM_TILE];
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)a.slices), s = (int)(blockIdx.x % (unsigned)a.slices);
    const int npb = wmin_npb(a);
    const size_t a0 = (size_t)box * (size_t)npb;            // the caller's order is box-major
    if (I >= a.tiles) return;                               // (uniform; cannot happen with the launcher's grid)
    const int il = I * WM_TILE + tid;                       // atom of this thread inside its box
    const bool vi = il < npb;
    const long long jb = (long long)s * a.chunk;
    const int je = (int)(jb + a.chunk < (long long)npb ? jb + a.chunk : (long long)npb);
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);

    double xi = 0.0, yi = 0.0, zi = 0.0;
    bool oi = false;
    if (vi) {
        const double* p = m.x64 + 3 * (a0 + (size_t)il);
        xi = p[0]; yi = p[1]; zi = p[2];
        oi = a.species[a0 + (size_t)il] != 0;
    }
    const double q_h = a.q_h, q_o = -(q_h + q_h);           // -2 q_h, exact
    const double qi = oi ? q_o : q_h;
    const int mi = il / 3;                                  // npb is a multiple of 3: molecules do not straddle boxes
    // the thread's output row, held in vector registers from here on, as in k_water_pairs: left to the compiler, its uniform
    // part stays in scalar registers across the loop, which the potential's constants fill already
    double* out = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * WATER_PART;
    asm volatile("" : "+v"(out));
    double fx = 0.0, fy = 0.0, fz = 0.0, elj = 0.0, ec = 0.0;
    for (long long base = jb; base < je; base += WM_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int nj = (int)(je - base < WM_TILE ? je - base : WM_TILE);
        if (tid < nj) {
            const size_t j = a0 + (size_t)base + (size_t)tid;
            const double* p = m.x64 + 3 * j;
            sx[tid] = p[0]; sy[tid] = p[1]; sz[tid] = p[2];
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
    if (vi) { out[0] = fx; out[1] = fy; out[2] = fz; out[3] = elj; out[4] = ec; }
}

__global__ void __launch_bounds__(256) k_wmin_rho(WMinArgs m) {
    const WaterArgs& a = m.w;
    const int box = blockIdx.z;
    if (m.stopped[box]) return;
    __shared__ double sx[WM_TILE], sy[WM_TILE], sz[WM_TILE], sq[WM_TILE];
    __shared__ double red[4][2][64];                        // [wave][re, im][lane]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int npb = wmin_npb(a), a0 = box * npb, a1 = a0 + npb;
    const int k = blockIdx.y * 64 + lane;
    const bool vk = k < a.n_k;
    const double nx = vk ? (double)a.kvec[3 * (size_t)k] : 0.0, ny = vk ? (double)a.kvec[3 * (size_t)k + 1] : 0.0,
                 nz = vk ? (double)a.kvec[3 * (size_t)k + 2] : 0.0;
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    double re = 0.0, im = 0.0;
    for (int base = a0 + blockIdx.x * WM_TILE; base < a1; base += gridDim.x * WM_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int i = base + tid;
        if (i < a1) {
            sx[tid] = water_frac(m.x64[3 * (size_t)i], Lx);
            sy[tid] = water_frac(m.x64[3 * (size_t)i + 1], Ly);
            sz[tid] = water_frac(m.x64[3 * (size_t)i + 2], Lz);
            sq[tid] = a.species[i] != 0 ? a.q_o : a.q_h;
        }
        __syncthreads();
        const int cnt = a1 - base < WM_TILE ? a1 - base : WM_TILE;
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

__global__ void __launch_bounds__(256) k_wmin_recip(WMinArgs m) {
    const WaterArgs& a = m.w;
    const int box = blockIdx.y;
    if (m.stopped[box]) return;
    __shared__ double kn[3][WM_TILE], ks_re[WM_TILE], ks_im[WM_TILE], ks_a[WM_TILE];
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)a.kslices), s = (int)(blockIdx.x % (unsigned)a.kslices);
    const int npb = wmin_npb(a);
    const size_t a0 = (size_t)box * (size_t)npb;
    if (I >= a.tiles) return;                               // (uniform; cannot happen with the launcher's grid)
    const int il = I * WM_TILE + tid;
    const bool vi = il < npb;
    double six = 0.0, siy = 0.0, siz = 0.0;
    if (vi) {
        const double* p = m.x64 + 3 * (a0 + (size_t)il);
        six = water_frac(p[0], gamd_box_edge(a, box, 0));
        siy = water_frac(p[1], gamd_box_edge(a, box, 1));
        siz = water_frac(p[2], gamd_box_edge(a, box, 2));
    }
    double gx = 0.0, gy = 0.0, gz = 0.0;
    // the 256-vector blocks s, s + kslices, ... of the list: which vectors a slice adds does not depend on the list's length
    for (long long base = (long long)s * WM_TILE; base < a.n_k; base += (long long)a.kslices * WM_TILE) {
        __syncthreads();                                    // the previous block has been read
        const int nk = (int)(a.n_k - base < WM_TILE ? a.n_k - base : WM_TILE);
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

__global__ void __launch_bounds__(256, 4) k_wmin_mols(WMinArgs m) {
    const WaterArgs& a = m.w;
    const int box = blockIdx.y;
    if (m.stopped[box]) return;
    __shared__ double red[4][WMIN_ACC];
    const int npb = wmin_npb(a), nmol = npb / 3;
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    const double pref = a.coul8pi / ((Lx * Ly) * Lz);
    const double kfx = a.two_pi / Lx, kfy = a.two_pi / Ly, kfz = a.two_pi / Lz;
    double ff = 0.0, vf = 0.0, vv = 0.0, ulj = 0.0, uc = 0.0, z2 = 0.0, mx = 0.0;
    for (int ml = blockIdx.x * blockDim.x + threadIdx.x; ml < nmol; ml += gridDim.x * blockDim.x) {
        const size_t mol = (size_t)box * (size_t)nmol + (size_t)ml;
        D3 F[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int il = 3 * ml + k;
            double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, t4 = 0.0;
            for (int s = 0; s < a.slices; ++s) {
                const double* p = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * WATER_PART;
                t0 += p[0]; t1 += p[1]; t2 += p[2]; t3 += p[3]; t4 += p[4];
            }
            double g0 = 0.0, g1 = 0.0, g2 = 0.0;
            for (int s = 0; s < a.kslices; ++s) {
                const double* p = a.rpart + (((size_t)box * (size_t)a.kslices + (size_t)s) * (size_t)npb + (size_t)il) * 3;
                g0 += p[0]; g1 += p[1]; g2 += p[2];
            }
            const bool o = a.species[3 * mol + k] != 0;
            const double pq = pref * (o ? a.q_o : a.q_h);
            F[k] = {(t0 + (pq * kfx) * g0) * a.len, (t1 + (pq * kfy) * g1) * a.len, (t2 + (pq * kfz) * g2) * a.len};   // kJ/mol/nm
            ulj += t3; uc += t4;
            const double z = o ? -2.0 : 1.0;                // the charge in units of q_h: sums of these are exact
            z2 += z * z;
        }
        D3 x[3], v[3];
        load_mol(m.x64, mol, x); load_mol(m.v64, mol, v);
        project(x, F);
        project(x, v);
        store_mol(m.f64, mol, F); store_mol(m.v64, mol, v);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ff += dot(F[k], F[k]);
            vf += dot(v[k], F[k]);
            vv += dot(v[k], v[k]);
            mx = fmax(mx, fmax(fmax(fabs(F[k].x), fabs(F[k].y)), fabs(F[k].z)));
        }
    }
    double acc[WMIN_ACC] = {ff, vf, vv, ulj, uc, z2, mx};
#pragma unroll
    for (int q = 0; q < WMIN_ACC; ++q) {
        double v = acc[q];
        if (q < WMIN_ACC - 1) v = gamd_wave_sum(v);
        else {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_down(v, d, 64));
        }
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < WMIN_ACC) {
        const int q = threadIdx.x;
        const double r = q < WMIN_ACC - 1 ? (red[0][q] + red[1][q]) + (red[2][q] + red[3][q])
                                          : fmax(fmax(red[0][q], red[1][q]), fmax(red[2][q], red[3][q]));
        a.blk[((size_t)box * (size_t)a.blocks + blockIdx.x) * WATER_ACC + q] = r;
    }
}

__global__ void __launch_bounds__(256) k_wmin_update(WMinArgs m) {
    const WaterArgs& a = m.w;
    const int box = blockIdx.y;
    if (m.stopped[box]) return;
    const int npb = wmin_npb(a), nmol = npb / 3;
    const int ml = blockIdx.x * WM_TILE + threadIdx.x;
    double ff = 0.0, vf = 0.0, vv = 0.0, ulj = 0.0, uc = 0.0, z2 = 0.0, mx = 0.0;
    for (int b = 0; b < a.blocks; ++b) {                    // the blocks in order: every thread gets the same bits
        const double* p = a.blk + ((size_t)box * (size_t)a.blocks + b) * WATER_ACC;
        ff += p[0]; vf += p[1]; vv += p[2]; ulj += p[3]; uc += p[4]; z2 += p[5]; mx = fmax(mx, p[6]);
    }
    double us = 0.0;
    for (int b = 0; b < a.kblocks; ++b) us += a.ublk[(size_t)box * (size_t)a.kblocks + b];
    const double V = (gamd_box_edge(a, box, 0) * gamd_box_edge(a, box, 1)) * gamd_box_edge(a, box, 2);
    // k_water_final's terms: every pair sits in two rows
    const double u_lj = 0.5 * ulj, u_coul = 0.5 * uc, u_recip = (a.coul4pi / V) * us, u_self = -(a.self_c * ((a.q_h * a.q_h) * z2));
    const double U = ((u_coul + u_recip) + u_self) + u_lj;
    const double rms = sqrt(ff / (3.0 * (double)npb));
    const double* cur = m.state + ((size_t)box * 2 + (size_t)(m.it & 1)) * MIN_STATE;
    double dt = cur[0], alpha = cur[1], n_pos = cur[2];
    const bool writer = ml == 0;
    double* row = m.rows + (size_t)box * MIN_ROW;
    if (writer && m.it == 0) { row[2] = U; row[3] = rms; }
    int stop = 0;
    if (!isfinite(U) || !isfinite(ff)) stop = 1 + MIN_FAILED;
    else if (rms <= m.tol) stop = 1 + MIN_CONVERGED;
    else if (m.last) stop = 1 + MIN_MAX_ITER;
    if (stop) {
        if (writer) {
            row[0] = (double)(stop - 1); row[1] = (double)m.it; row[4] = U; row[5] = rms; row[6] = mx; row[7] = dt;
            m.stopped[box] = stop;
        }
        return;
    }
    const bool mix = vf > 0.0;
    double c1 = 0.0, c2 = 0.0;
    if (mix) {
        c1 = 1.0 - alpha; c2 = alpha * sqrt(vv / ff);
        if (n_pos > (double)m.n_min) { dt = fmin(dt * m.f_inc, m.dt_max); alpha = alpha * m.f_alpha; }
        n_pos += 1.0;
    } else {
        alpha = m.alpha_start; dt = dt * m.f_dec; n_pos = 0.0;
    }
    if (writer) {
        double* nxt = m.state + ((size_t)box * 2 + (size_t)((m.it + 1) & 1)) * MIN_STATE;
        nxt[0] = dt; nxt[1] = alpha; nxt[2] = n_pos;
    }
    if (ml >= nmol) return;
    const size_t mol = (size_t)box * (size_t)nmol + (size_t)ml;
    D3 x[3], v[3], F[3], xn[3];
    load_mol(m.x64, mol, x); load_mol(m.v64, mol, v); load_mol(m.f64, mol, F);
    double big = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (mix) v[k] = (c1 * v[k]) + (c2 * F[k]);
        else v[k] = {0.0, 0.0, 0.0};
        v[k] = v[k] + (dt * F[k]);
        xn[k] = dt * v[k];                                  // dr
        big = fmax(big, sqrt(dot(xn[k], xn[k])));
    }
    store_mol(m.v64, mol, v);
    const bool clamp = big > m.max_step;
    const double sc = clamp ? m.max_step / big : 1.0;       // one factor for the molecule
#pragma unroll
    for (int k = 0; k < 3; ++k) xn[k] = x[k] + (clamp ? sc * xn[k] : xn[k]);
    settle(x, xn, m.ra, m.rb, m.rc);
    store_mol(m.x64, mol, xn);
}

// x = fp32(x64 - s) per molecule, s the lattice vector that brings the oxygen into [0, L); x64_out = x64.  A box that was not
// finite at the start keeps the x it was given, and x64_out is that x widened.
__global__ void __launch_bounds__(256) k_wmin_store_x(WMinArgs m, float* __restrict__ x_io, double* __restrict__ x64_out) {
    const WaterArgs& a = m.w;
    const int box = blockIdx.y, nmol = wmin_npb(a) / 3;
    const int ml = blockIdx.x * WM_TILE + threadIdx.x;
    if (ml >= nmol) return;
    const size_t mol = (size_t)box * (size_t)nmol + (size_t)ml;
    if (m.stopped[box] == 1 + MIN_FAILED && m.rows[(size_t)box * MIN_ROW + 1] == 0.0) {
        if (x64_out)
            for (int q = 0; q < 9; ++q) x64_out[9 * mol + q] = (double)x_io[9 * mol + q];
        return;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double L = gamd_box_edge(a, box, d);
        const float Lf = (float)L;                          // exact: the edge is an fp32 value
        const double xo = m.x64[9 * mol + d];
        double s = L * floor(xo / L);
        if (xo - s < 0.0) s = s - L;                        // the quotient rounded up to an integer
        if ((float)(xo - s) >= Lf) s = s + L;               // the oxygen rounds up to L: it goes to 0 with its hydrogens
        float o = (float)(xo - s);
        if (o < 0.f) o = 0.f;
        x_io[9 * mol + d] = o;
        x_io[9 * mol + 3 + d] = (float)(m.x64[9 * mol + 3 + d] - s);
        x_io[9 * mol + 6 + d] = (float)(m.x64[9 * mol + 6 + d] - s);
        if (x64_out) {
            x64_out[9 * mol + d] = xo; x64_out[9 * mol + 3 + d] = m.x64[9 * mol + 3 + d]; x64_out[9 * mol + 6 + d] = m.x64[9 * mol + 6 + d];
        }
    }
}

// what every launcher checks: the geometry covers a row and the grids stay inside their limits, every buffer is there
int wmin_check(const WMinArgs& m, long long* tiles, long long* mol_tiles, int* boxes) {
    const WaterArgs& a = m.w;
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1, npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const long long T = (npb + WM_TILE - 1) / WM_TILE;
    if (npb < 3 || npb % 3 || nb > 65535 || a.tiles != (int)T || a.slices < 1 || a.chunk < 1 || a.blocks < 1 || a.blocks > 65535) return -1;
    if ((long long)a.slices * a.chunk < npb || T * a.slices > 0x7fffffll) return -1;   // the slices cover a row; grid.x * 256 threads stay below 2^31
    if (a.n_k < 1 || a.n_k > (1 << 17) || a.kslices < 1 || T * a.kslices > 0x7fffffll) return -1;
    if (a.kblocks != (a.n_k + 255) / 256 || a.rho_blocks < 1 || a.rho_blocks > 65535) return -1;
    if (!a.species || !a.kvec || !a.part || !a.rho_partial || !a.sk || !a.ublk || !a.rpart || !a.blk || !a.box_edges || !a.devflags) return -1;
    if (!m.x64 || !m.v64 || !m.f64 || !m.state || !m.stopped || !m.rows || m.it < 0) return -1;
    if (!(m.ra > 0.0) || !(m.rb > 0.0) || !(m.rc > 0.0)) return -1;
    *tiles = T; *mol_tiles = (npb / 3 + WM_TILE - 1) / WM_TILE; *boxes = nb;
    return 0;
}

}  // namespace

int launch_wmin_init(const WMinArgs& m, const float* x, hipStream_t st) {
    long long T, M; int nb;
    if (wmin_check(m, &T, &M, &nb) || !x) return -1;
    hipLaunchKernelGGL(k_wmin_init, dim3((unsigned)M, nb), dim3(256), 0, st, m, x); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_wmin_iter(const WMinArgs& m, hipStream_t st) {
    long long T, M; int nb;
    if (wmin_check(m, &T, &M, &nb)) return -1;
    const WaterArgs& a = m.w;
    hipLaunchKernelGGL(k_wmin_pairs, dim3((unsigned)(T * a.slices), nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_wmin_rho, dim3(a.rho_blocks, (a.n_k + 63) / 64, nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    if (int r = launch_water_sk(a, st)) return r;
    hipLaunchKernelGGL(k_wmin_recip, dim3((unsigned)(T * a.kslices), nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_wmin_mols, dim3(a.blocks, nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_wmin_update, dim3((unsigned)M, nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_wmin_store_x(const WMinArgs& m, float* x_io, double* x64_out, hipStream_t st) {
    long long T, M; int nb;
    if (wmin_check(m, &T, &M, &nb) || !x_io) return -1;
    hipLaunchKernelGGL(k_wmin_store_x, dim3((unsigned)M, nb), dim3(256), 0, st, m, x_io, x64_out); GAMD_CHECK_LAUNCH();
    return 0;
}
