// water_minimize.hip — the water energy minimiser (gamd_water_minimize): FIRE (Bitzek et al., Phys. Rev.
// Lett. 97, 170201 (2006)) in the semi-implicit Euler form on RIGID 3-site molecules, per box, under the water potential of
// water_classical.hip (O-O Lennard-Jones plus a plain Ewald sum), with positions, velocities, forces and every scalar in double
// on the device.  Every water driver of the reference calls OpenMM's minimizeEnergy in front of its first step
// (dataset/generate_tip3p_data.py:85); this is not its L-BFGS, which treats the constraints by restraints — what is shared is
// the meaning of the tolerance.  Atoms in the CALLER's order O,H,H, molecule = index / 3.  The constraint arithmetic
// (gamd_wmin_dev.h) takes unit weights for the three atoms: the projection is the orthogonal one and the projected force F_c is
// the gradient on the constraint manifold.  One iteration is six launches:
//
//   k_wmin_pairs    k_water_pairs' walk on the DOUBLE positions x64: per atom and slice {Fx, Fy, Fz, u_LJ, u_real + u_excl}
//                   into the first five doubles of the observer's partial row.  The one pass written out here, not taken from
//                   gamd_passes_dev.h (see the kernel).
//   k_wmin_rho      k_water_rho's pass (gamd_water_rho) on x64.
//   k_water_sk      the observer's own kernel, unchanged (launch_water_sk): it reads no positions.
//   k_wmin_recip    k_water_recip's pass on x64 with a STRIDED k walk: k slice s walks the 256-vector blocks s, s + kslices, ...
//                   of the list in order, so that a longer list only appends terms of weight zero to a slice.  Written out
//                   here as well (see the kernel).
//   k_wmin_mols     grid (blocks per box, boxes), one molecule at a time per thread: per atom the pair slices added in order
//                   from 0, the k slices added in order from 0, F as k_water_atoms forms f_cl (kJ/mol/nm); F and v projected
//                   onto the tangent space of the three bond constraints at x64, F_c to f64 and v to v64; the molecule's terms
//                   of ff = sum F_c.F_c, vf = sum v.F_c, vv = sum v.v, sum u_LJ, sum u_coul, sum z^2 and max |F_c|; per-thread
//                   sums over the thread's molecules (fixed assignment), then gamd_fire_block_tree into one row per block.
//   k_wmin_update   grid (molecule tiles, boxes), one thread per molecule.  EVERY thread adds the block rows in order (and the
//                   k blocks' A |S|^2 in order) and takes the same decisions from the same bits: U = ((U_coul + U_recip) +
//                   U_self) + U_LJ with the terms of k_water_final; then k_min_update's decisions (gamd_fire_step) and
//                   FIRE's mixing on F_c, v += dt F_c, dr = dt v, ONE factor per molecule so that the largest |dr| of its
//                   three atoms is at most max_step, and x64 <- SETTLE(reference x64, new x64 + dr).
//
// launch_wmin_force enqueues the first four alone, on the positions and under the gate of the argument block it is handed: the
// water L-BFGS minimiser (water_lbfgs.hip) evaluates its trial positions through it.
// Scalar state, the two slots per box, the `stopped` gate and the rows are minimize.hip's.  Fixed assignment, no floating-point
// atomics, contraction off, plain stores: the same bits run after run, and a box gets the bits it gets alone.
// (No kernel uses a value it read from memory as an address: the checked build has nothing to range-check here.)
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_passes_dev.h"
#include "gamd_wmin_dev.h"

namespace {

using namespace gamd_wmin;

// x64 = x widened and put on the exact rigid geometry (SETTLE with reference = new = the input), v = 0, FIRE's state reset
__global__ void __launch_bounds__(256) k_wmin_init(WMinArgs m, const float* __restrict__ x) {
    const int box = blockIdx.y, nmol = gamd_npb(m.w) / 3;
    const int ml = blockIdx.x * GAMD_PASS_TILE + threadIdx.x;
    if (ml == 0) gamd_fire_reset(m.fire, box);
    if (ml >= nmol) return;
    const size_t mol = (size_t)box * (size_t)nmol + (size_t)ml;
    D3 x0[3], x1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x0[k] = {(double)x[9 * mol + 3 * k], (double)x[9 * mol + 3 * k + 1], (double)x[9 * mol + 3 * k + 2]};
        x1[k] = x0[k];
    }
    settle(x0, x1, m.ra, m.rb, m.rc);
    store_mol(m.fire.x64, mol, x1);
    const D3 zero[3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    store_mol(m.fire.v64, mol, zero);
}

// gamd_water_walk on x64, WRITTEN OUT.  Inlined from the header, the walk makes the compiler read the x64 pointer from the
// argument block once in front of the loop and spill it (163 VGPRs, two scalar spills); the same text in the kernel has 162 and
// none.  Statement for statement the walk of gamd_passes_dev.h with the forces, u_LJ and u_coul kept, LJ on and the loader
// GamdPosF64: a change there is made here too.  tests/test_gpu_water_minimize.py pins its forces to the force source's
// (k_wsrc_pairs) bit for bit; its two energy columns are pinned only through U against the float64 replay
// (test_positions_energy_and_rms_agree_with_the_float64_replay), to that test's tolerance.
__global__ void __launch_bounds__(256) k_wmin_pairs(WMinArgs m) {
    const WaterArgs& a = m.w;
    const int box = blockIdx.y;
    if (m.fire.stopped[box]) return;                        // the box has stopped: its positions stay
    __shared__ double sx[GAMD_PASS_TILE], sy[GAMD_PASS_TILE], sz[GAMD_PASS_TILE];
    __shared__ unsigned char so[GAMD_PASS_TILE];
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)a.slices), s = (int)(blockIdx.x % (unsigned)a.slices);
    const int npb = gamd_npb(a);
    const size_t a0 = (size_t)box * (size_t)npb;            // the caller's order is box-major
    if (I >= a.tiles) return;                               // (uniform; cannot happen with the launcher's grid)
    const int il = I * GAMD_PASS_TILE + tid;                // atom of this thread inside its box
    const bool vi = il < npb;
    const long long jb = (long long)s * a.chunk;
    const int je = (int)(jb + a.chunk < (long long)npb ? jb + a.chunk : (long long)npb);
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);

    double xi = 0.0, yi = 0.0, zi = 0.0;
    bool oi = false;
    if (vi) {
        const double* p = m.fire.x64 + 3 * (a0 + (size_t)il);
        xi = p[0]; yi = p[1]; zi = p[2];
        oi = a.species[a0 + (size_t)il] != 0;
    }
    const double q_h = a.q_h, q_o = -(q_h + q_h);           // -2 q_h, exact
    const double qi = oi ? q_o : q_h;
    const int mi = il / 3;                                  // npb is a multiple of 3: molecules do not straddle boxes
    // the thread's output row, held in vector registers from here on, as in the shared walk
    double* out = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * WATER_PART;
    asm volatile("" : "+v"(out));
    double fx = 0.0, fy = 0.0, fz = 0.0, elj = 0.0, ec = 0.0;
    for (long long base = jb; base < je; base += GAMD_PASS_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int nj = (int)(je - base < GAMD_PASS_TILE ? je - base : GAMD_PASS_TILE);
        if (tid < nj) {
            const size_t j = a0 + (size_t)base + (size_t)tid;
            const double* p = m.fire.x64 + 3 * j;
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
                if (oi && oj) {                             // the Lennard-Jones walk's term
                    const double2 lj = gamd_lj_pair_r(a, 6.0 * a.eps4, ir2, r);     // 6 (4 epsilon) = 24 epsilon bit for bit
                    elj += lj.x;
                    fs = fs + -(lj.y * ir2);
                }
            }
            fx += fs * dx; fy += fs * dy; fz += fs * dz;
        }
    }
    if (vi) { out[0] = fx; out[1] = fy; out[2] = fz; out[3] = elj; out[4] = ec; }
}

__global__ void __launch_bounds__(256) k_wmin_rho(WMinArgs m) {
    if (m.fire.stopped[blockIdx.z]) return;
    gamd_water_rho(m.w, GamdPosF64{m.fire.x64});
}

// gamd_water_recip on x64 with the STRIDED k walk, WRITTEN OUT: taken from the header the kernel is 0.6 % slower (1.7 us of 290
// at 4170 atoms, with the parent's registers and fewer instructions: block placement around the sincospi loop); the same text
// in the kernel is not.  Otherwise the pass of gamd_passes_dev.h statement for statement: a change there is made here too
// (the forces are pinned to the force source's bit for bit, as for k_wmin_pairs).
__global__ void __launch_bounds__(256) k_wmin_recip(WMinArgs m) {
    const WaterArgs& a = m.w;
    const int box = blockIdx.y;
    if (m.fire.stopped[box]) return;
    __shared__ double kn[3][GAMD_PASS_TILE], ks_re[GAMD_PASS_TILE], ks_im[GAMD_PASS_TILE], ks_a[GAMD_PASS_TILE];
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)a.kslices), s = (int)(blockIdx.x % (unsigned)a.kslices);
    const int npb = gamd_npb(a);
    const size_t a0 = (size_t)box * (size_t)npb;
    if (I >= a.tiles) return;                               // (uniform; cannot happen with the launcher's grid)
    const int il = I * GAMD_PASS_TILE + tid;
    const bool vi = il < npb;
    double six = 0.0, siy = 0.0, siz = 0.0;
    if (vi) {
        const double* p = m.fire.x64 + 3 * (a0 + (size_t)il);
        six = water_frac(p[0], gamd_box_edge(a, box, 0));
        siy = water_frac(p[1], gamd_box_edge(a, box, 1));
        siz = water_frac(p[2], gamd_box_edge(a, box, 2));
    }
    double gx = 0.0, gy = 0.0, gz = 0.0;
    // the 256-vector blocks s, s + kslices, ... of the list: which vectors a slice adds does not depend on the list's length
    for (long long base = (long long)s * GAMD_PASS_TILE; base < a.n_k; base += (long long)a.kslices * GAMD_PASS_TILE) {
        __syncthreads();                                    // the previous block has been read
        const int nk = (int)(a.n_k - base < GAMD_PASS_TILE ? a.n_k - base : GAMD_PASS_TILE);
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
    if (m.fire.stopped[box]) return;
    const int npb = gamd_npb(a), nmol = npb / 3;
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
        load_mol(m.fire.x64, mol, x); load_mol(m.fire.v64, mol, v);
        project(x, F);
        project(x, v);
        store_mol(m.fire.f64, mol, F); store_mol(m.fire.v64, mol, v);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ff += dot(F[k], F[k]);
            vf += dot(v[k], F[k]);
            vv += dot(v[k], v[k]);
            mx = fmax(mx, fmax(fmax(fabs(F[k].x), fabs(F[k].y)), fabs(F[k].z)));
        }
    }
    gamd_fire_block_tree<WATER_ACC>(a, box, ff, vf, vv, ulj, uc, z2, mx);
}

__global__ void __launch_bounds__(256) k_wmin_update(WMinArgs m) {
    const WaterArgs& a = m.w;
    const int box = blockIdx.y;
    if (m.fire.stopped[box]) return;
    const int npb = gamd_npb(a), nmol = npb / 3;
    const int ml = blockIdx.x * GAMD_PASS_TILE + threadIdx.x;
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
    gamd_fire_step(m.fire, box, npb, ml == 0, U, ff, vf, vv, mx, [&](bool mix, double c1, double c2, double dt) {
        if (ml >= nmol) return;
        const size_t mol = (size_t)box * (size_t)nmol + (size_t)ml;
        D3 x[3], v[3], F[3], xn[3];
        load_mol(m.fire.x64, mol, x); load_mol(m.fire.v64, mol, v); load_mol(m.fire.f64, mol, F);
        double big = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (mix) v[k] = (c1 * v[k]) + (c2 * F[k]);
            else v[k] = {0.0, 0.0, 0.0};
            v[k] = v[k] + (dt * F[k]);
            xn[k] = dt * v[k];                              // dr
            big = fmax(big, sqrt(dot(xn[k], xn[k])));
        }
        store_mol(m.fire.v64, mol, v);
        const bool clamp = big > m.fire.max_step;
        const double sc = clamp ? m.fire.max_step / big : 1.0;     // one factor for the molecule
#pragma unroll
        for (int k = 0; k < 3; ++k) xn[k] = x[k] + (clamp ? sc * xn[k] : xn[k]);
        settle(x, xn, m.ra, m.rb, m.rc);
        store_mol(m.fire.x64, mol, xn);
    });
}

// x = fp32(x64 - s) per molecule, s the lattice vector that brings the oxygen into [0, L); x64_out = x64.  A box that was not
// finite at the start keeps the x it was given, and x64_out is that x widened.
__global__ void __launch_bounds__(256) k_wmin_store_x(WMinArgs m, float* __restrict__ x_io, double* __restrict__ x64_out) {
    const WaterArgs& a = m.w;
    const int box = blockIdx.y, nmol = gamd_npb(a) / 3;
    const int ml = blockIdx.x * GAMD_PASS_TILE + threadIdx.x;
    if (ml >= nmol) return;
    const size_t mol = (size_t)box * (size_t)nmol + (size_t)ml;
    if (m.fire.stopped[box] == 1 + MIN_FAILED && m.fire.rows[(size_t)box * MIN_ROW + 1] == 0.0) {
        if (x64_out)
            for (int q = 0; q < 9; ++q) x64_out[9 * mol + q] = (double)x_io[9 * mol + q];
        return;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) store_wrapped(m.fire.x64, mol, d, gamd_box_edge(a, box, d), x_io, x64_out);
}

// what the force launches need: the geometry covers a row and the grids stay inside their limits, the potential's buffers, the
// positions and the gate are there
int wmin_force_check(const WMinArgs& m, PassGeom* g) {
    const WaterArgs& a = m.w;
    if (pass_geometry(a, 3, g) || pass_k_geometry(a, g->T, false) || a.blocks < 1 || a.blocks > 65535) return -1;
    if (!a.species || !a.kvec || !a.part || !a.rho_partial || !a.sk || !a.ublk || !a.rpart || !a.blk || !a.box_edges || !a.devflags) return -1;
    if (!m.fire.x64 || !m.fire.stopped) return -1;
    return 0;
}

// ... of a ROUTED block (gamd_water_minimize_potential, water_relax.hip): the k side is the route's and its launchers' to check
int wmin_routed_check(const WMinArgs& m, PassGeom* g) {
    const WaterArgs& a = m.w;
    if (pass_geometry(a, 3, g) || a.kblocks < 1 || a.blocks < 1 || a.blocks > 65535) return -1;
    if (!a.species || !a.part || !a.ublk || !a.rpart || !a.blk || !a.box_edges || !a.devflags) return -1;
    if (!m.fire.x64 || !m.fire.stopped) return -1;
    return 0;
}

// what every launcher of the minimiser checks: that, and every buffer of FIRE's
int wmin_check(const WMinArgs& m, PassGeom* g, long long* mol_tiles, bool routed = false) {
    const FireArgs& fi = m.fire;
    if (routed ? wmin_routed_check(m, g) : wmin_force_check(m, g)) return -1;
    if (!fi.x64 || !fi.v64 || !fi.f64 || !fi.state || !fi.stopped || !fi.rows || fi.it < 0) return -1;
    if (!(m.ra > 0.0) || !(m.rb > 0.0) || !(m.rc > 0.0)) return -1;
    *mol_tiles = (g->npb / 3 + GAMD_PASS_TILE - 1) / GAMD_PASS_TILE;
    return 0;
}

// pairs
int wmin_pairs(const WMinArgs& m, const PassGeom& g, hipStream_t st) {
    const WaterArgs& a = m.w;
    hipLaunchKernelGGL(k_wmin_pairs, dim3((unsigned)(g.T * a.slices), g.nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    return 0;
}

// rho, sk, recip
int wmin_recip(const WMinArgs& m, const PassGeom& g, hipStream_t st) {
    const WaterArgs& a = m.w;
    hipLaunchKernelGGL(k_wmin_rho, dim3(a.rho_blocks, (a.n_k + 63) / 64, g.nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    if (int r = launch_water_sk(a, st)) return r;
    hipLaunchKernelGGL(k_wmin_recip, dim3((unsigned)(g.T * a.kslices), g.nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    return 0;
}

// pairs; rho, sk, recip
int wmin_force(const WMinArgs& m, const PassGeom& g, hipStream_t st) {
    if (int r = wmin_pairs(m, g, st)) return r;
    return wmin_recip(m, g, st);
}

}  // namespace

int launch_wmin_init(const WMinArgs& m, const float* x, hipStream_t st) {
    PassGeom g; long long M;
    if (wmin_check(m, &g, &M) || !x) return -1;
    hipLaunchKernelGGL(k_wmin_init, dim3((unsigned)M, g.nb), dim3(256), 0, st, m, x); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_wmin_iter(const WMinArgs& m, hipStream_t st) {
    PassGeom g; long long M;
    if (wmin_check(m, &g, &M)) return -1;
    const WaterArgs& a = m.w;
    if (int r = wmin_force(m, g, st)) return r;
    hipLaunchKernelGGL(k_wmin_mols, dim3(a.blocks, g.nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_wmin_update, dim3((unsigned)M, g.nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_wmin_force(const WMinArgs& m, hipStream_t st) {
    PassGeom g;
    if (wmin_force_check(m, &g)) return -1;
    return wmin_force(m, g, st);
}

int launch_wmin_store_x(const WMinArgs& m, float* x_io, double* x64_out, hipStream_t st) {
    PassGeom g; long long M;
    if (wmin_check(m, &g, &M) || !x_io) return -1;
    hipLaunchKernelGGL(k_wmin_store_x, dim3((unsigned)M, g.nb), dim3(256), 0, st, m, x_io, x64_out); GAMD_CHECK_LAUNCH();
    return 0;
}

// ---- the pieces water_relax.hip puts its routes together from (gamd_water_minimize_potential) ----------------------------
// k_wmin_pairs alone: the pair side of the force launches' checks
int launch_wmin_pairs(const WMinArgs& m, hipStream_t st) {
    PassGeom g;
    if (wmin_routed_check(m, &g)) return -1;
    return wmin_pairs(m, g, st);
}

// k_wmin_rho, k_water_sk, k_wmin_recip alone: every check of the force launches (the strided k walk's geometry among them)
int launch_wmin_recip(const WMinArgs& m, hipStream_t st) {
    PassGeom g;
    if (wmin_force_check(m, &g)) return -1;
    return wmin_recip(m, g, st);
}

// k_wmin_update alone, behind a molecule pass that wrote k_wmin_mols' columns
int launch_wmin_update(const WMinArgs& m, hipStream_t st) {
    PassGeom g; long long M;
    if (wmin_check(m, &g, &M, true)) return -1;
    hipLaunchKernelGGL(k_wmin_update, dim3((unsigned)M, g.nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_wmin_init_routed(const WMinArgs& m, const float* x, hipStream_t st) {
    PassGeom g; long long M;
    if (wmin_check(m, &g, &M, true) || !x) return -1;
    hipLaunchKernelGGL(k_wmin_init, dim3((unsigned)M, g.nb), dim3(256), 0, st, m, x); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_wmin_store_x_routed(const WMinArgs& m, float* x_io, double* x64_out, hipStream_t st) {
    PassGeom g; long long M;
    if (wmin_check(m, &g, &M, true) || !x_io) return -1;
    hipLaunchKernelGGL(k_wmin_store_x, dim3((unsigned)M, g.nb), dim3(256), 0, st, m, x_io, x64_out); GAMD_CHECK_LAUNCH();
    return 0;
}
