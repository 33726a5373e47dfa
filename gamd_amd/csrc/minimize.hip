// minimize.hip — the energy minimiser (gamd_minimize): FIRE (Bitzek et al., Phys. Rev. Lett. 97, 170201
// (2006)) in the semi-implicit Euler form, per box, under the switched, shifted Lennard-Jones potential of classical.hip, with
// positions, velocities, forces and every scalar in double on the device.  The reference's drivers call OpenMM's
// minimizeEnergy in front of their first step (dataset/generate_lj_data.py:83, LJ/test_script/test_langevin.py:84); this is not
// its L-BFGS — what is shared is the meaning of the tolerance, the root mean square of all 3N force components in kJ/mol/nm.
// One iteration is three launches:
//
//   k_min_pairs     the pair pass of k_classical_pairs — same grid (T * slices, boxes), same 256-atom row tiles, same slices,
//                   same staging, the same operations on d, r2, u and r u' in the same order — on the DOUBLE positions x64:
//                   per atom and slice {Fx, Fy, Fz, u_i} into the first four doubles of the observer's partial row (the row
//                   keeps its CLASSICAL_PART stride), summed over j in ascending order.
//   k_min_atoms     grid (blocks per box, boxes): per atom, the slices' partials added in order from 0, F = F * len
//                   (kJ/mol/nm) to f64; the atom's terms of ff = sum F.F, vf = sum v.F, vv = sum v.v, sum u_i and max |F_c|;
//                   per-thread sums over the thread's atoms (fixed assignment), then the tree of k_report_ke (gamd_wave_sum,
//                   (w0 + w1) + (w2 + w3)) into one row per block.
//   k_min_update    grid (T, boxes), one thread per atom.  EVERY thread adds the block rows in order and takes the same
//                   decisions from the same bits: U = sum / 2, rms = sqrt(ff / 3N); not finite -> the box stops as failed;
//                   rms <= tolerance -> converged; the pass behind the last iteration -> max_iter; a box that stops keeps
//                   its positions.  Otherwise FIRE's mixing (vf > 0: v = (1 - alpha) v + alpha sqrt(vv / ff) F, after n_min
//                   such steps dt = min(dt f_inc, dt_max), alpha = alpha f_alpha; else v = 0, alpha = alpha_start,
//                   dt = dt f_dec) and the step v += dt F, dr = dt v, |dr| clamped per atom to max_step, x64 += dr.
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

#include "gamd_potential_dev.h"

namespace {

constexpr int MN_TILE = 256;

__device__ __forceinline__ int min_npb(const ClassicalArgs& c) { return c.bx.n_boxes > 1 ? c.bx.n_per_box : c.n; }

// x64 = x widened, v = 0, the scalar state of iteration 0, the gate open, the row cleared
__global__ void __launch_bounds__(256) k_min_init(MinArgs m, const float* __restrict__ x) {
    const int box = blockIdx.y, npb = min_npb(m.c);
    const int il = blockIdx.x * MN_TILE + threadIdx.x;
    if (il == 0) {
        double* st = m.state + (size_t)box * 2 * MIN_STATE;
        st[0] = m.dt_start; st[1] = m.alpha_start; st[2] = 0.0; st[3] = 0.0;
        for (int q = 0; q < MIN_ROW; ++q) m.rows[(size_t)box * MIN_ROW + q] = 0.0;
        m.stopped[box] = 0;
    }
    if (il >= npb) return;
    const size_t i = (size_t)box * (size_t)npb + (size_t)il;
#pragma unroll
    for (int d = 0; d < 3; ++d) { m.x64[3 * i + d] = (double)x[3 * i + d]; m.v64[3 * i + d] = 0.0; }
}

__global__ void __launch_bounds__(256) k_min_pairs(MinArgs m) {
    const ClassicalArgs& a = m.c;
    const int box = blockIdx.y;
    if (m.stopped[box]) return;                             // the box has stopped: its positions stay
    __shared__ double sx[MN_TILE], sy[MN_TILE], sz[MN_TILE];
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)a.slices), s = (int)(blockIdx.x % (unsigned)a.slices);
    const int npb = min_npb(a);
    const size_t a0 = (size_t)box * (size_t)npb;            // the caller's order is box-major
    if (I >= a.tiles) return;                               // (uniform; cannot happen with the launcher's grid)
    const int il = I * MN_TILE + tid;                       // atom of this thread inside its box
    const bool vi = il < npb;
    const long long jb = (long long)s * a.chunk;
    const int je = (int)(jb + a.chunk < (long long)npb ? jb + a.chunk : (long long)npb);
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);

    double xi = 0.0, yi = 0.0, zi = 0.0;
    if (vi) {
        const double* p = m.x64 + 3 * (a0 + (size_t)il);
        xi = p[0]; yi = p[1]; zi = p[2];
    }
    double fx = 0.0, fy = 0.0, fz = 0.0, e = 0.0;
    for (long long base = jb; base < je; base += MN_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int nj = (int)(je - base < MN_TILE ? je - base : MN_TILE);
        if (tid < nj) {
            const double* p = m.x64 + 3 * (a0 + (size_t)base + (size_t)tid);
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
            const double2 lj = gamd_lj_term(a.sig2, a.eps4, a.eps24, a.u0, ir2);
            double u = lj.x, ru = lj.y;                     // u_LJ - u0 and r u_LJ'(r)
            if (a.rs >= 0.0) {                              // (the square root only where there is a switch)
                const double r = sqrt(r2);
                if (r > a.rs) {
                    const double2 sw = gamd_lj_switch(a.rs, a.inv_w, r);
                    ru = ru * sw.x + ((u * sw.y) * r);      // r u'(r), u = (u_LJ - u0) S
                    u = u * sw.x;
                }
            }
            const double fs = -(ru * ir2);                  // F_ij = -u'(r) d / r = fs d
            fx += fs * dx; fy += fs * dy; fz += fs * dz;
            e += u;
        }
    }
    if (vi) {
        double* out = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * CLASSICAL_PART;
        out[0] = fx; out[1] = fy; out[2] = fz; out[3] = e;
    }
}

__global__ void __launch_bounds__(256) k_min_atoms(MinArgs m) {
    const ClassicalArgs& a = m.c;
    const int box = blockIdx.y;
    if (m.stopped[box]) return;
    __shared__ double red[4][MIN_ACC];
    const int npb = min_npb(a);
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
        m.f64[3 * i] = cx; m.f64[3 * i + 1] = cy; m.f64[3 * i + 2] = cz;
        const double vx = m.v64[3 * i], vy = m.v64[3 * i + 1], vz = m.v64[3 * i + 2];
        ff += (cx * cx + cy * cy) + cz * cz;
        vf += (vx * cx + vy * cy) + vz * cz;
        vv += (vx * vx + vy * vy) + vz * vz;
        us += t3;
        mx = fmax(mx, fmax(fmax(fabs(cx), fabs(cy)), fabs(cz)));
    }
    double acc[MIN_ACC] = {ff, vf, vv, us, mx};
#pragma unroll
    for (int q = 0; q < MIN_ACC; ++q) {
        double v = acc[q];
        if (q < 4) v = gamd_wave_sum(v);
        else {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_down(v, d, 64));
        }
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < MIN_ACC) {
        const int q = threadIdx.x;
        const double r = q < 4 ? (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]) : fmax(fmax(red[0][q], red[1][q]), fmax(red[2][q], red[3][q]));
        a.blk[((size_t)box * (size_t)a.blocks + blockIdx.x) * CLASSICAL_ROW + q] = r;
    }
}

__global__ void __launch_bounds__(256) k_min_update(MinArgs m) {
    const ClassicalArgs& a = m.c;
    const int box = blockIdx.y;
    if (m.stopped[box]) return;
    const int npb = min_npb(a);
    const int il = blockIdx.x * MN_TILE + threadIdx.x;
    double ff = 0.0, vf = 0.0, vv = 0.0, us = 0.0, mx = 0.0;
    for (int b = 0; b < a.blocks; ++b) {                    // the blocks in order: every thread gets the same bits
        const double* p = a.blk + ((size_t)box * (size_t)a.blocks + b) * CLASSICAL_ROW;
        ff += p[0]; vf += p[1]; vv += p[2]; us += p[3]; mx = fmax(mx, p[4]);
    }
    const double U = 0.5 * us;                              // every pair sits in two rows
    const double rms = sqrt(ff / (3.0 * (double)npb));
    const double* cur = m.state + ((size_t)box * 2 + (size_t)(m.it & 1)) * MIN_STATE;
    double dt = cur[0], alpha = cur[1], n_pos = cur[2];
    const bool writer = il == 0;
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
    if (il >= npb) return;
    const size_t i = (size_t)box * (size_t)npb + (size_t)il;
    double dr[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double F = m.f64[3 * i + d];
        double v = mix ? c1 * m.v64[3 * i + d] + c2 * F : 0.0;
        v = v + dt * F;
        m.v64[3 * i + d] = v;
        dr[d] = dt * v;
    }
    const double nrm = sqrt((dr[0] * dr[0] + dr[1] * dr[1]) + dr[2] * dr[2]);
    if (nrm > m.max_step) {
        const double sc = m.max_step / nrm;
        dr[0] *= sc; dr[1] *= sc; dr[2] *= sc;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) m.x64[3 * i + d] = m.x64[3 * i + d] + dr[d];
}

// x = fp32(x64), wrapped into the box by the integrators' expression; a box that was not finite at the start keeps what it was given
__global__ void __launch_bounds__(256) k_min_store_x(MinArgs m, float* __restrict__ x_out) {
    const ClassicalArgs& a = m.c;
    const int box = blockIdx.y, npb = min_npb(a);
    const int il = blockIdx.x * MN_TILE + threadIdx.x;
    if (il >= npb) return;
    if (m.stopped[box] == 1 + MIN_FAILED && m.rows[(size_t)box * MIN_ROW + 1] == 0.0) return;
    const size_t i = (size_t)box * (size_t)npb + (size_t)il;
#pragma unroll
    for (int d = 0; d < 3; ++d) x_out[3 * i + d] = gamd_remainder((float)m.x64[3 * i + d], (float)gamd_box_edge(a, box, d));
}

// f = the force source's forces at the stored x; nothing is written for a failed box (its forces are not finite)
__global__ void __launch_bounds__(256) k_min_store_f(MinArgs m, const float* __restrict__ f_in, float* __restrict__ f_out) {
    const int box = blockIdx.y, npb = min_npb(m.c);
    const int il = blockIdx.x * MN_TILE + threadIdx.x;
    if (il >= npb || m.stopped[box] == 1 + MIN_FAILED) return;
    const size_t i = (size_t)box * (size_t)npb + (size_t)il;
#pragma unroll
    for (int d = 0; d < 3; ++d) f_out[3 * i + d] = f_in[3 * i + d];
}

// what every launcher checks: the geometry covers a row and the grids stay inside their limits, every buffer is there
int min_check(const MinArgs& m, long long* tiles, int* boxes) {
    const ClassicalArgs& a = m.c;
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1, npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const long long T = (npb + MN_TILE - 1) / MN_TILE;
    if (npb < 1 || nb > 65535 || a.tiles != (int)T || a.slices < 1 || a.chunk < 1 || a.blocks < 1 || a.blocks > 65535) return -1;
    if ((long long)a.slices * a.chunk < npb || T * a.slices > 0x7fffffll) return -1;   // the slices cover a row; grid.x * 256 threads stay below 2^31
    if (!a.part || !a.blk || !a.box_edges || !m.x64 || !m.v64 || !m.f64 || !m.state || !m.stopped || !m.rows || m.it < 0) return -1;
    *tiles = T; *boxes = nb;
    return 0;
}

}  // namespace

int launch_minimize_init(const MinArgs& m, const float* x, hipStream_t st) {
    long long T; int nb;
    if (min_check(m, &T, &nb) || !x) return -1;
    hipLaunchKernelGGL(k_min_init, dim3((unsigned)T, nb), dim3(256), 0, st, m, x); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_minimize_iter(const MinArgs& m, hipStream_t st) {
    long long T; int nb;
    if (min_check(m, &T, &nb)) return -1;
    hipLaunchKernelGGL(k_min_pairs, dim3((unsigned)(T * m.c.slices), nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_min_atoms, dim3(m.c.blocks, nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_min_update, dim3((unsigned)T, nb), dim3(256), 0, st, m); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_minimize_store_x(const MinArgs& m, float* x_out, hipStream_t st) {
    long long T; int nb;
    if (min_check(m, &T, &nb) || !x_out) return -1;
    hipLaunchKernelGGL(k_min_store_x, dim3((unsigned)T, nb), dim3(256), 0, st, m, x_out); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_minimize_store_f(const MinArgs& m, const float* f_in, float* f_out, hipStream_t st) {
    long long T; int nb;
    if (min_check(m, &T, &nb) || !f_in || !f_out) return -1;
    hipLaunchKernelGGL(k_min_store_f, dim3((unsigned)T, nb), dim3(256), 0, st, m, f_in, f_out); GAMD_CHECK_LAUNCH();
    return 0;
}
