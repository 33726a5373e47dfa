// minimize.hip — the energy minimiser (gamd_minimize): FIRE (Bitzek et al., Phys. Rev. Lett. 97, 170201
// (2006)) in the semi-implicit Euler form, per box, under the switched, shifted Lennard-Jones potential of classical.hip, with
// positions, velocities, forces and every scalar in double on the device.  The reference's drivers call OpenMM's
// minimizeEnergy in front of their first step (dataset/generate_lj_data.py:83, LJ/test_script/test_langevin.py:84); this is not
// its L-BFGS — what is shared is the meaning of the tolerance, the root mean square of all 3N force components in kJ/mol/nm.
// One iteration is three launches:
//
//   k_min_pairs     k_classical_pairs' walk on the DOUBLE positions x64: per atom and slice {Fx, Fy, Fz, u_i} into the first
//                   four doubles of the observer's partial row.  Written out here, not taken from gamd_passes_dev.h (see the
//                   kernel).
//   k_min_atoms     grid (blocks per box, boxes): per atom, the slices' partials added in order from 0, F = F * len
//                   (kJ/mol/nm) to f64; the atom's terms of ff = sum F.F, vf = sum v.F, vv = sum v.v, sum u_i and max |F_c|;
//                   per-thread sums over the thread's atoms (fixed assignment), then gamd_fire_block_tree into one row per block.
//   k_min_update    grid (T, boxes), one thread per atom.  EVERY thread adds the block rows in order, U = sum / 2, and takes
//                   the same decisions from the same bits (gamd_fire_step: stop, or FIRE's mixing coefficients and dt); a box
//                   that stops keeps its positions.  Then v = c1 v + c2 F (or 0), v += dt F, dr = dt v, |dr| clamped per atom
//                   to max_step, x64 += dr.
//
// With gamd_classical_cells on, launch_classical_cells (cell_table.hip's table rebuilt from x64, then k_ljcell_min of classical_cells.hip)
// stands where k_min_pairs is in every iteration, on ONE pair slice, and returns at once for a stopped box like the kernels here.
//
// F is in kJ/mol/nm and x, max_step in the handle's length unit: dt is a pseudo-time that absorbs the units (and the mass).
// Scalar state {dt, alpha, n_pos} sits in two slots per box: iteration `it` reads slot it & 1 in every thread and thread 0 of
// workgroup 0 writes slot (it + 1) & 1, so no thread reads what this launch writes.  `stopped[box]` is the gate: 0 while the box
// runs, 1 + state once it stopped; every kernel returns at once for a stopped box, which lets the host enqueue iterations
// without looking.  It is written by that one thread in k_min_update when the box stops — and a box that stops applies no
// update, so a thread of the same launch that already sees the flag and returns does what it would have done anyway.
// Fixed assignment, no floating-point atomics, contraction off, plain stores: the same bits run after run.
// (No kernel uses a value it read from memory as an address: the checked build has nothing to range-check here.)
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_passes_dev.h"

namespace {

// x64 = x widened, v = 0, FIRE's state reset
__global__ void __launch_bounds__(256) k_min_init(MinArgs m, const float* __restrict__ x) {
    const FireArgs& fi = m.fire;
    const int box = blockIdx.y, npb = gamd_npb(m.c);
    const int il = blockIdx.x * GAMD_PASS_TILE + threadIdx.x;
    if (il == 0) gamd_fire_reset(fi, box);
    if (il >= npb) return;
    const size_t i = (size_t)box * (size_t)npb + (size_t)il;
#pragma unroll
    for (int d = 0; d < 3; ++d) { fi.x64[3 * i + d] = (double)x[3 * i + d]; fi.v64[3 * i + d] = 0.0; }
}

// gamd_lj_walk on x64, WRITTEN OUT: taken from the header the kernel is 0.3 - 0.5 us slower at 258 atoms, where an iteration
// is launch latency (three scalar loads of the prologue end up behind the gate's branch); the same text in the kernel is not.
// Statement for statement the walk of gamd_passes_dev.h with the forces and u_i kept and the loader GamdPosF64: a change there
// is made here too.  tests/test_gpu_minimize.py pins both to each other bit for bit: the forces to the force source's
// (k_drive_lj_pairs), energy_start to classical_forces' energy (k_classical_pairs).
__global__ void __launch_bounds__(256) k_min_pairs(MinArgs m) {
    const ClassicalArgs& a = m.c;
    const int box = blockIdx.y;
    if (m.fire.stopped[box]) return;                             // the box has stopped: its positions stay
    __shared__ double sx[GAMD_PASS_TILE], sy[GAMD_PASS_TILE], sz[GAMD_PASS_TILE];
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)a.slices), s = (int)(blockIdx.x % (unsigned)a.slices);
    const int npb = gamd_npb(a);
    const size_t a0 = (size_t)box * (size_t)npb;            // the caller's order is box-major
    if (I >= a.tiles) return;                               // (uniform; cannot happen with the launcher's grid)
    const int il = I * GAMD_PASS_TILE + tid;                       // atom of this thread inside its box
    const bool vi = il < npb;
    const long long jb = (long long)s * a.chunk;
    const int je = (int)(jb + a.chunk < (long long)npb ? jb + a.chunk : (long long)npb);
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);

    double xi = 0.0, yi = 0.0, zi = 0.0;
    if (vi) {
        const double* p = m.fire.x64 + 3 * (a0 + (size_t)il);
        xi = p[0]; yi = p[1]; zi = p[2];
    }
    double fx = 0.0, fy = 0.0, fz = 0.0, e = 0.0;
    for (long long base = jb; base < je; base += GAMD_PASS_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int nj = (int)(je - base < GAMD_PASS_TILE ? je - base : GAMD_PASS_TILE);
        if (tid < nj) {
            const double* p = m.fire.x64 + 3 * (a0 + (size_t)base + (size_t)tid);
            sx[tid] = p[0]; sy[tid] = p[1]; sz[tid] = p[2];
        }
        __syncthreads();
        if (!vi) continue;
        const int self = (int)((long long)il - base);       // this atom's own slot in the chunk, if it is there
        for (int jj = 0; jj < nj; ++jj) {
            double dx = xi - sx[jj], dy = yi - sy[jj], dz = zi - sz[jj];
            dx = dx - Lx * rint(dx / Lx);
            dy = dy - Ly * rint(dy / Ly);
            dz = dz - Lz * rint(dz / Lz);
            const double r2 = (dx * dx + dy * dy) + dz * dz;
            if (jj == self || !(r2 < a.rc2)) continue;
            const double ir2 = 1.0 / r2;
            const double2 lj = gamd_lj_pair_r2(a, a.eps24, ir2, r2);   // (u, r u'(r)), u = (u_LJ - u0) S
            const double fs = -(lj.y * ir2);                // F_ij = -u'(r) d / r = fs d
            fx += fs * dx; fy += fs * dy; fz += fs * dz;
            e += lj.x;
        }
    }
    if (vi) {
        double* out = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * CLASSICAL_PART;
        out[0] = fx; out[1] = fy; out[2] = fz; out[3] = e;
    }
}

__global__ void __launch_bounds__(256) k_min_atoms(MinArgs m) {
    const ClassicalArgs& a = m.c;
    const FireArgs& fi = m.fire;
    const int box = blockIdx.y;
    if (fi.stopped[box]) return;
    const int npb = gamd_npb(a);
    const size_t a0 = (size_t)box * (size_t)npb;
    double ff = 0.0, vf = 0.0, vv = 0.0, us = 0.0, mx = 0.0;
    for (int il = blockIdx.x * blockDim.x + threadIdx.x; il < npb; il += gridDim.x * blockDim.x) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
        for (int s = 0; s < a.slices; ++s) {
            const double* p = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * CLASSICAL_PART;
            t0 += p[0]; t1 += p[1]; t2 += p[2]; t3 += p[3];
        }
        const size_t i = a0 + (size_t)il;
        const double cx = t0 * a.len, cy = t1 * a.len, cz = t2 * a.len;             // kJ/mol/nm
        fi.f64[3 * i] = cx; fi.f64[3 * i + 1] = cy; fi.f64[3 * i + 2] = cz;
        const double vx = fi.v64[3 * i], vy = fi.v64[3 * i + 1], vz = fi.v64[3 * i + 2];
        ff += (cx * cx + cy * cy) + cz * cz;
        vf += (vx * cx + vy * cy) + vz * cz;
        vv += (vx * vx + vy * vy) + vz * vz;
        us += t3;
        mx = fmax(mx, fmax(fmax(fabs(cx), fabs(cy)), fabs(cz)));
    }
    gamd_fire_block_tree<CLASSICAL_ROW>(a, box, ff, vf, vv, us, mx);
}

__global__ void __launch_bounds__(256) k_min_update(MinArgs m) {
    const ClassicalArgs& a = m.c;
    const FireArgs& fi = m.fire;
    const int box = blockIdx.y;
    if (fi.stopped[box]) return;
    const int npb = gamd_npb(a);
    const int il = blockIdx.x * GAMD_PASS_TILE + threadIdx.x;
    double ff = 0.0, vf = 0.0, vv = 0.0, us = 0.0, mx = 0.0;
    for (int b = 0; b < a.blocks; ++b) {                    // the blocks in order: every thread gets the same bits
        const double* p = a.blk + ((size_t)box * (size_t)a.blocks + b) * CLASSICAL_ROW;
        ff += p[0]; vf += p[1]; vv += p[2]; us += p[3]; mx = fmax(mx, p[4]);
    }
    const double U = 0.5 * us;                              // every pair sits in two rows
    gamd_fire_step(fi, box, npb, il == 0, U, ff, vf, vv, mx, [&](bool mix, double c1, double c2, double dt) {
        if (il >= npb) return;
        const size_t i = (size_t)box * (size_t)npb + (size_t)il;
        double dr[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double F = fi.f64[3 * i + d];
            double v = mix ? c1 * fi.v64[3 * i + d] + c2 * F : 0.0;
            v = v + dt * F;
            fi.v64[3 * i + d] = v;
            dr[d] = dt * v;
        }
        const double nrm = sqrt((dr[0] * dr[0] + dr[1] * dr[1]) + dr[2] * dr[2]);
        if (nrm > fi.max_step) {
            const double sc = fi.max_step / nrm;
            dr[0] *= sc; dr[1] *= sc; dr[2] *= sc;
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) fi.x64[3 * i + d] = fi.x64[3 * i + d] + dr[d];
    });
}

// x = fp32(x64), wrapped into the box by the integrators' expression; a box that was not finite at the start keeps what it was given
__global__ void __launch_bounds__(256) k_min_store_x(MinArgs m, float* __restrict__ x_out) {
    const ClassicalArgs& a = m.c;
    const int box = blockIdx.y, npb = gamd_npb(a);
    const int il = blockIdx.x * GAMD_PASS_TILE + threadIdx.x;
    if (il >= npb) return;
    if (m.fire.stopped[box] == 1 + MIN_FAILED && m.fire.rows[(size_t)box * MIN_ROW + 1] == 0.0) return;
    const size_t i = (size_t)box * (size_t)npb + (size_t)il;
#pragma unroll
    for (int d = 0; d < 3; ++d) x_out[3 * i + d] = gamd_remainder((float)m.fire.x64[3 * i + d], (float)gamd_box_edge(a, box, d));
}

// f = the force source's forces at the stored x; nothing is written for a failed box (its forces are not finite)
__global__ void __launch_bounds__(256) k_min_store_f(const int* __restrict__ stopped, int npb, const float* __restrict__ f_in,
                                                     float* __restrict__ f_out) {
    const int box = blockIdx.y;
    const int il = blockIdx.x * GAMD_PASS_TILE + threadIdx.x;
    if (il >= npb || stopped[box] == 1 + MIN_FAILED) return;
    const size_t i = (size_t)box * (size_t)npb + (size_t)il;
#pragma unroll
    for (int d = 0; d < 3; ++d) f_out[3 * i + d] = f_in[3 * i + d];
}

// what every launcher checks: the geometry covers a row and the grids stay inside their limits, every buffer is there
int min_check(const MinArgs& m, PassGeom* g) {
    const ClassicalArgs& a = m.c;
    const FireArgs& fi = m.fire;
    if (pass_geometry(a, 1, g) || a.blocks < 1 || a.blocks > 65535) return -1;
    if (!a.part || !a.blk || !a.box_edges || !fi.x64 || !fi.v64 || !fi.f64 || !fi.state || !fi.stopped || !fi.rows || fi.it < 0) return -1;
    return 0;
}

}  // namespace

int launch_minimize_init(const MinArgs& m, const float* x, hipStream_t st) {
    PassGeom g;
    if (min_check(m, &g) || !x) return -1;
    hipLaunchKernelGGL(k_min_init, dim3((unsigned)g.T, g.nb), dim3(256), 0, st, m, x); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_minimize_iter(const MinArgs& m, hipStream_t st, const CellTabBufs* cells) {
    PassGeom g;
    if (min_check(m, &g)) return -1;
    if (cells) {                                            // gamd_classical_cells: {F, u_i} over the cell table of x64, one slice
        if (!m.c.devflags) return -1;
        if (int r = launch_classical_cells(m.c, *cells, m.fire.x64, m.fire.stopped, 4, st)) return r;
    } else {
        hipLaunchKernelGGL(k_min_pairs, dim3((unsigned)(g.T * m.c.slices), g.nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_min_atoms, dim3(m.c.blocks, g.nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_min_update, dim3((unsigned)g.T, g.nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_minimize_store_x(const MinArgs& m, float* x_out, hipStream_t st) {
    PassGeom g;
    if (min_check(m, &g) || !x_out) return -1;
    hipLaunchKernelGGL(k_min_store_x, dim3((unsigned)g.T, g.nb), dim3(256), 0, st, m, x_out); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_minimize_store_f(const FireArgs& m, int n, const BoxRef& bx, const float* f_in, float* f_out, hipStream_t st) {
    const int nb = bx.n_boxes > 1 ? bx.n_boxes : 1, npb = bx.n_boxes > 1 ? bx.n_per_box : n;
    if (npb < 1 || nb > 65535 || !m.stopped || !f_in || !f_out) return -1;
    hipLaunchKernelGGL(k_min_store_f, dim3((unsigned)((npb + GAMD_PASS_TILE - 1) / GAMD_PASS_TILE), nb), dim3(256), 0, st, m.stopped, npb, f_in, f_out);
    GAMD_CHECK_LAUNCH();
    return 0;
}
