// lbfgs.hip — the L-BFGS energy minimiser (gamd_minimize_lbfgs): a limited-memory BFGS direction from
// a ring of at most m pairs (s, y) (Nocedal, Math. Comp. 35, 773 (1980); Liu and Nocedal, Math. Programming 45, 503 (1989)), a
// backtracking line search on the sufficient-decrease condition and FIRE's per-atom clamp on every trial displacement, per box,
// under the switched, shifted Lennard-Jones potential of classical.hip, with positions, forces, the ring and every scalar in
// double on the device.  The reference's drivers call OpenMM's minimizeEnergy, which is L-BFGS too; the line search and the
// stopping rule here are this project's own (tests/lbfgs_ref.py states them decision by decision) and no parity is claimed.
// One evaluation is three launches, whatever m is:
//
//   k_lbfgs_pairs   k_min_pairs' walk (minimize.hip) on the TRIAL positions xt: per atom and slice {Fx, Fy, Fz, u_i} into the
//                   first four doubles of the observer's partial row.  Written out here as it is there.
//   k_lbfgs_dots    grid (blocks per box, boxes): per atom, the slices' partials added in order from 0, Ft = F * len
//                   (kJ/mol/nm) to ft, s = xt - x, y = F - Ft, and the atom's terms of every scalar the decision and the next
//                   direction need: sum u_i, Ft.Ft, F.s, s.s, s.y, y.y, s.Ft, y.Ft, max |Ft_i|, and for every ring slot k
//                   s.y_k, Ft.s_k, Ft.y_k.  Per-thread sums over the thread's atoms (fixed assignment), then the block tree of
//                   gamd_fire_block_tree (shuffle 32 .. 1, then (w0 + w1) + (w2 + w3)) into one row per block.
//   k_lbfgs_update  grid (T, boxes), one thread per atom.  Thread q of EVERY workgroup adds column q of the block rows in
//                   order, and every thread takes the same decisions from the same bits: the start, or accept / reject by
//                   U_t <= U - c1 F.s; on acceptance the curvature test, the push into the ring, x = xt, F = Ft, the stop
//                   tests; on rejection t / 2, or after max_ls of them the ring emptied, or the stop.  The two-loop recursion
//                   runs on SCALARS only: the inner products s_i.y_j, y_i.y_j, F.s_i, F.y_i of the ring, kept per box in the
//                   state and brought up to date from the new dots (y = F - Ft: y.v = F.v - Ft.v), give the coefficients of
//                   d = cf F + sum cs_j s_j + sum cy_j y_j, and every thread forms its atom's d from the ring.  Then the
//                   next trial: s = t d, |s_i| clamped to max_step, xt = x + s.  The decision, the ring's products and the
//                   recursion are gamd_lbfgs_dev.h's, shared with k_wlb_update (water_lbfgs.hip).
//
// With gamd_classical_cells on, launch_classical_cells (cell_table.hip's table rebuilt from xt, then k_ljcell_min of
// classical_cells.hip) stands where k_lbfgs_pairs is, on ONE pair slice.
//
// Pass `it` reads state slot it & 1 and the gates gates[it & 1] in every thread and writes slot and gates (it + 1) & 1 from one
// workgroup: no thread reads what its launch writes, so a box that stops in a pass is still finished by every thread of that
// pass (its accepted x is stored) — and the pass behind only hands the gate on.  A gate is 0 while the box runs and 1 + state
// once it stopped; every kernel returns at once for a stopped box, which lets the host enqueue evaluations without looking.
// Fixed assignment, no floating-point atomics, contraction off, plain stores: the same bits run after run.
// Checked build: the two ring numbers a thread reads from the state (pairs held, next slot) pass through GAMD_CHK_RANGE
// before they address the ring; nothing else read from memory is used as an address.
// Device memory besides the classical observer's work buffers: 24 (2 m + 5) + 12 B per atom.
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_passes_dev.h"
#include "gamd_lbfgs_dev.h"

namespace {

enum { LB_US = 0, LB_FTFT = 1, LB_FS = 2, LB_SS = 3, LB_SY = 4, LB_YY = 5, LB_SFT = 6, LB_YFT = 7,
       LB_SYK = 8, LB_FTSK = LB_SYK + LBFGS_M, LB_FTYK = LB_FTSK + LBFGS_M, LB_MAX = LBFGS_ACC - 1 };
static_assert(LB_FTYK + LBFGS_M == LB_MAX, "the columns of a block row");

__device__ __forceinline__ int lb_boxes(const ClassicalArgs& a) { return a.bx.n_boxes > 1 ? a.bx.n_boxes : 1; }
__device__ __forceinline__ const int* lb_gates_in(const LbfgsArgs& l) { return l.gates + (size_t)(l.it & 1) * (size_t)lb_boxes(l.c); }
__device__ __forceinline__ double lb_dot(const double* p, const double* q) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }
__device__ __forceinline__ void lb_load(const double* base, size_t i, double* v) { v[0] = base[3 * i]; v[1] = base[3 * i + 1]; v[2] = base[3 * i + 2]; }
__device__ __forceinline__ void lb_store(double* base, size_t i, const double* v) { base[3 * i] = v[0]; base[3 * i + 1] = v[1]; base[3 * i + 2] = v[2]; }
// ring vector: s of slot k (which = 0) or y of slot k (which = 1)
__device__ __forceinline__ double* lb_ring(const LbfgsArgs& l, int which, int k) {
    return l.ring + ((size_t)which * (size_t)l.m + (size_t)k) * 3 * (size_t)l.c.n;
}

// x = xt = the input widened, F = 0 (the start's pass reads it and uses none of it), the scalar state of the start, both gates open, the row cleared
__global__ void __launch_bounds__(256) k_lbfgs_init(LbfgsArgs l, const float* __restrict__ x) {
    const int box = blockIdx.y, npb = gamd_npb(l.c), nb = lb_boxes(l.c);
    const int il = blockIdx.x * GAMD_PASS_TILE + threadIdx.x;
    if (blockIdx.x == 0) {
        double* st = l.state + (size_t)box * 2 * LBFGS_SLOT;
        for (int q = threadIdx.x; q < 2 * LBFGS_SLOT; q += 256) st[q] = q == 0 ? 1.0 : 0.0;        // t = 1
        if (threadIdx.x < LBFGS_ROW) l.rows[(size_t)box * LBFGS_ROW + threadIdx.x] = 0.0;
        if (threadIdx.x == 0) { l.gates[box] = 0; l.gates[(size_t)nb + box] = 0; }
    }
    if (il >= npb) return;
    const size_t i = (size_t)box * (size_t)npb + (size_t)il;
#pragma unroll
    for (int d = 0; d < 3; ++d) { const double v = (double)x[3 * i + d]; l.x[3 * i + d] = v; l.xt[3 * i + d] = v; l.f[3 * i + d] = 0.0; }
}

// k_min_pairs (minimize.hip) on the trial positions, statement for statement: a change there is made here too.
// tests/test_gpu_lbfgs.py pins the energy at the start to classical_forces' (k_classical_pairs).
__global__ void __launch_bounds__(256) k_lbfgs_pairs(LbfgsArgs l) {
    const ClassicalArgs& a = l.c;
    const int box = blockIdx.y;
    if (lb_gates_in(l)[box]) return;                        // the box has stopped: its positions stay
    __shared__ double sx[GAMD_PASS_TILE], sy[GAMD_PASS_TILE], sz[GAMD_PASS_TILE];
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
    if (vi) {
        const double* p = l.xt + 3 * (a0 + (size_t)il);
        xi = p[0]; yi = p[1]; zi = p[2];
    }
    double fx = 0.0, fy = 0.0, fz = 0.0, e = 0.0;
    for (long long base = jb; base < je; base += GAMD_PASS_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int nj = (int)(je - base < GAMD_PASS_TILE ? je - base : GAMD_PASS_TILE);
        if (tid < nj) {
            const double* p = l.xt + 3 * (a0 + (size_t)base + (size_t)tid);
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

__global__ void __launch_bounds__(256) k_lbfgs_dots(LbfgsArgs l) {
    const ClassicalArgs& a = l.c;
    const int box = blockIdx.y;
    if (lb_gates_in(l)[box]) return;
    const int npb = gamd_npb(a);
    const size_t a0 = (size_t)box * (size_t)npb;
    const double* cur = l.state + ((size_t)box * 2 + (size_t)(l.it & 1)) * LBFGS_SLOT;
    const int cnt = GAMD_CHK_RANGE(l.sticky, (int)cur[2], 0, l.m, GAMD_CHK_LBFGS_COUNT);   // the slots 0 .. cnt - 1 hold pairs
    double acc[LBFGS_ACC];
#pragma unroll
    for (int q = 0; q < LBFGS_ACC; ++q) acc[q] = 0.0;
    for (int il = blockIdx.x * blockDim.x + threadIdx.x; il < npb; il += gridDim.x * blockDim.x) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
        for (int s = 0; s < a.slices; ++s) {
            const double* p = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * CLASSICAL_PART;
            t0 += p[0]; t1 += p[1]; t2 += p[2]; t3 += p[3];
        }
        const size_t i = a0 + (size_t)il;
        const double ft[3] = {t0 * a.len, t1 * a.len, t2 * a.len};                  // kJ/mol/nm
        lb_store(l.ft, i, ft);
        double x[3], xt[3], f[3];
        lb_load(l.x, i, x); lb_load(l.xt, i, xt); lb_load(l.f, i, f);
        const double s[3] = {xt[0] - x[0], xt[1] - x[1], xt[2] - x[2]};
        const double y[3] = {f[0] - ft[0], f[1] - ft[1], f[2] - ft[2]};
        const double ftft = lb_dot(ft, ft);
        acc[LB_US] += t3;
        acc[LB_FTFT] += ftft;
        acc[LB_FS] += lb_dot(f, s);
        acc[LB_SS] += lb_dot(s, s);
        acc[LB_SY] += lb_dot(s, y);
        acc[LB_YY] += lb_dot(y, y);
        acc[LB_SFT] += lb_dot(s, ft);
        acc[LB_YFT] += lb_dot(y, ft);
#pragma unroll
        for (int k = 0; k < LBFGS_M; ++k) {
            if (k < cnt) {                                  // (uniform)
                double sk[3], yk[3];
                lb_load(lb_ring(l, 0, k), i, sk); lb_load(lb_ring(l, 1, k), i, yk);
                acc[LB_SYK + k] += lb_dot(s, yk);
                acc[LB_FTSK + k] += lb_dot(ft, sk);
                acc[LB_FTYK + k] += lb_dot(ft, yk);
            }
        }
        acc[LB_MAX] = fmax(acc[LB_MAX], sqrt(ftft));
    }
    // gamd_fire_block_tree's tree on LBFGS_ACC accumulators: all but the last summed, the last maximised
    __shared__ double red[4][LBFGS_ACC];
#pragma unroll
    for (int q = 0; q < LBFGS_ACC; ++q) {
        double v = acc[q];
        if (q < LB_MAX) v = gamd_wave_sum(v);
        else {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_down(v, d, 64));
        }
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < LBFGS_ACC) {
        const int q = threadIdx.x;
        const double r = q < LB_MAX ? (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]) : fmax(fmax(red[0][q], red[1][q]), fmax(red[2][q], red[3][q]));
        l.blk[((size_t)box * (size_t)a.blocks + blockIdx.x) * LBFGS_ACC + q] = r;
    }
}

__global__ void __launch_bounds__(256) k_lbfgs_update(LbfgsArgs l) {
    const ClassicalArgs& a = l.c;
    const int box = blockIdx.y, nb = lb_boxes(a), tid = threadIdx.x;
    const bool writer = blockIdx.x == 0 && tid == 0;        // one thread per box
    int* gates_out = l.gates + (size_t)((l.it + 1) & 1) * (size_t)nb;
    const int gate = lb_gates_in(l)[box];
    if (gate) {                                             // stopped in an earlier pass: the gate goes on to the other set
        if (writer) gates_out[box] = gate;
        return;
    }
    __shared__ double sacc[LBFGS_ACC];
    __shared__ double g_sy[LBFGS_M * LBFGS_M], g_yy[LBFGS_M * LBFGS_M], g_fs[LBFGS_M], g_fy[LBFGS_M];   // the ring's products, oldest pair first
    const int npb = gamd_npb(a);
    if (tid < LBFGS_ACC) {                                  // the blocks in order: every workgroup gets the same bits
        double v = 0.0;
        for (int b = 0; b < a.blocks; ++b) {
            const double p = l.blk[((size_t)box * (size_t)a.blocks + b) * LBFGS_ACC + tid];
            v = tid < LB_MAX ? v + p : fmax(v, p);
        }
        sacc[tid] = v;
    }
    __syncthreads();
    const double* cur = l.state + ((size_t)box * 2 + (size_t)(l.it & 1)) * LBFGS_SLOT;
    double* nxt = l.state + ((size_t)box * 2 + (size_t)((l.it + 1) & 1)) * LBFGS_SLOT;
    double* row = l.rows + (size_t)box * LBFGS_ROW;
    gamd_lbfgs::Scalars sc = gamd_lbfgs::load_scalars(cur);
    const int cnt = GAMD_CHK_RANGE(l.sticky, (int)cur[2], 0, l.m, GAMD_CHK_LBFGS_COUNT);
    const int head = GAMD_CHK_RANGE(l.sticky, (int)cur[3], 0, l.m - 1, GAMD_CHK_LBFGS_SLOT);   // the slot a push writes
    const double Ut = 0.5 * sacc[LB_US];                    // every pair sits in two rows
    const double ftft = sacc[LB_FTFT], sy = sacc[LB_SY], yy = sacc[LB_YY];
    const double rms_t = sqrt(ftft / (3.0 * (double)npb));
    const bool start = l.it == 0;

    // ---- the decision, by every thread from the same bits ----
    if (start && writer) { row[3] = Ut; row[4] = rms_t; }
    const gamd_lbfgs::Decision dc = gamd_lbfgs::decide(l, start, cnt, Ut, ftft, sacc[LB_MAX], rms_t, sacc[LB_FS], sacc[LB_SS], sy, yy, sc);

    // ---- the accepted point: the ring's new pair, x = xt, F = Ft (a box that stops here still takes it) ----
    const int il = blockIdx.x * GAMD_PASS_TILE + tid;
    const bool vi = il < npb;
    const size_t i = (size_t)box * (size_t)npb + (size_t)(vi ? il : 0);
    double x[3] = {0.0, 0.0, 0.0}, f[3] = {0.0, 0.0, 0.0};
    if (vi && dc.stop != 1 + LBFGS_FAILED) {
        lb_load(l.x, i, x); lb_load(l.f, i, f);
        if (dc.accept) {
            double xt[3], ft[3];
            lb_load(l.xt, i, xt); lb_load(l.ft, i, ft);
            if (dc.push) {
                const double s[3] = {xt[0] - x[0], xt[1] - x[1], xt[2] - x[2]};
                const double y[3] = {f[0] - ft[0], f[1] - ft[1], f[2] - ft[2]};
                lb_store(lb_ring(l, 0, head), i, s); lb_store(lb_ring(l, 1, head), i, y);
            }
#pragma unroll
            for (int d = 0; d < 3; ++d) { x[d] = xt[d]; f[d] = ft[d]; }
            lb_store(l.x, i, x); lb_store(l.f, i, f);
        }
    }
    if (dc.stop) {
        if (writer) {
            row[0] = (double)(dc.stop - 1); row[1] = (double)l.it; row[2] = sc.n_acc; row[5] = sc.U; row[6] = sqrt(sc.FF / (3.0 * (double)npb));
            row[7] = sc.fm; row[8] = sc.n_skip; row[9] = sc.n_reset;
            gates_out[box] = dc.stop;
        }
        return;
    }

    // ---- the state of the next pass: the scalars, and the ring's products with the new pair in slot `head` ----
    const gamd_lbfgs::Ring rg = gamd_lbfgs::ring_next(l.m, cnt, head, dc, cur, nxt, blockIdx.x == 0, tid, sy, yy, sacc[LB_SFT], sacc[LB_YFT],
                                                     sacc + LB_SYK, sacc + LB_FTSK, sacc + LB_FTYK, g_sy, g_yy, g_fs, g_fy);
    if (writer) {
        nxt[0] = sc.t; nxt[1] = sc.ls; nxt[2] = (double)rg.cnt; nxt[3] = (double)rg.head; nxt[4] = sc.U; nxt[5] = sc.FF; nxt[6] = sc.fm;
        nxt[7] = sc.n_acc; nxt[8] = sc.n_skip; nxt[9] = sc.n_reset;
        gates_out[box] = 0;
    }
    __syncthreads();

    // ---- the direction: kept through a line search, new behind an accepted step or an emptied ring ----
    double d[3] = {0.0, 0.0, 0.0};
    if (dc.accept || dc.reset) {
        if (rg.cnt == 0) {                                  // steepest descent, the longest per-atom step max_step
            const double sd = l.max_step / sc.fm;
            if (vi) { d[0] = f[0] * sd; d[1] = f[1] * sd; d[2] = f[2] * sd; }
        } else {                                            // the two-loop recursion on the coefficients of d
            double cf, cs[LBFGS_M], cy[LBFGS_M];
            gamd_lbfgs::coefficients(rg.cnt, g_sy, g_yy, g_fs, g_fy, cf, cs, cy);
            if (vi) {
                d[0] = cf * f[0]; d[1] = cf * f[1]; d[2] = cf * f[2];
#pragma unroll
                for (int j = 0; j < LBFGS_M; ++j) {
                    if (j < rg.cnt) {
                        double v[3];
                        lb_load(lb_ring(l, 0, rg.slot_of(j)), i, v);
                        d[0] = d[0] + cs[j] * v[0]; d[1] = d[1] + cs[j] * v[1]; d[2] = d[2] + cs[j] * v[2];
                    }
                }
#pragma unroll
                for (int j = 0; j < LBFGS_M; ++j) {
                    if (j < rg.cnt) {
                        double v[3];
                        lb_load(lb_ring(l, 1, rg.slot_of(j)), i, v);
                        d[0] = d[0] + cy[j] * v[0]; d[1] = d[1] + cy[j] * v[1]; d[2] = d[2] + cy[j] * v[2];
                    }
                }
            }
        }
        if (vi) lb_store(l.d, i, d);
    } else if (vi) {
        lb_load(l.d, i, d);
    }
    if (!vi) return;

    // ---- the next trial ----
    double s[3] = {sc.t * d[0], sc.t * d[1], sc.t * d[2]};
    const double nrm = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    if (nrm > l.max_step) {
        const double sc = l.max_step / nrm;
        s[0] *= sc; s[1] *= sc; s[2] *= sc;
    }
    const double xt[3] = {x[0] + s[0], x[1] + s[1], x[2] + s[2]};
    lb_store(l.xt, i, xt);
}

// x = fp32(x64), wrapped into the box by the integrators' expression (k_min_store_x's rule); a box that failed keeps what it was given
__global__ void __launch_bounds__(256) k_lbfgs_store_x(LbfgsArgs l, const int* __restrict__ gates, float* __restrict__ x_out) {
    const ClassicalArgs& a = l.c;
    const int box = blockIdx.y, npb = gamd_npb(a);
    const int il = blockIdx.x * GAMD_PASS_TILE + threadIdx.x;
    if (il >= npb || gates[box] == 1 + LBFGS_FAILED) return;
    const size_t i = (size_t)box * (size_t)npb + (size_t)il;
#pragma unroll
    for (int d = 0; d < 3; ++d) x_out[3 * i + d] = gamd_remainder((float)l.x[3 * i + d], (float)gamd_box_edge(a, box, d));
}

// what every launcher checks: the geometry covers a row and the grids stay inside their limits, every buffer is there
int lbfgs_check(const LbfgsArgs& l, PassGeom* g) {
    const ClassicalArgs& a = l.c;
    if (pass_geometry(a, 1, g) || a.blocks < 1 || a.blocks > 65535) return -1;
    if (!a.part || !a.box_edges || !l.x || !l.xt || !l.f || !l.ft || !l.d || !l.ring || !l.blk || !l.state || !l.gates || !l.rows) return -1;
    if (l.m < 1 || l.m > LBFGS_M || l.max_ls < 1 || l.it < 0 || l.max_iter < 0) return -1;
    return 0;
}

}  // namespace

int launch_lbfgs_init(const LbfgsArgs& l, const float* x, hipStream_t st) {
    PassGeom g;
    if (lbfgs_check(l, &g) || !x) return -1;
    hipLaunchKernelGGL(k_lbfgs_init, dim3((unsigned)g.T, g.nb), dim3(256), 0, st, l, x); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_lbfgs_eval(const LbfgsArgs& l, hipStream_t st, const CellTabBufs* cells) {
    PassGeom g;
    if (lbfgs_check(l, &g)) return -1;
    if (cells) {                                            // gamd_classical_cells: {F, u_i} over the cell table of xt, one slice
        if (!l.c.devflags) return -1;
        if (int r = launch_classical_cells(l.c, *cells, l.xt, l.gates + (size_t)(l.it & 1) * (size_t)g.nb, 4, st)) return r;
    } else {
        hipLaunchKernelGGL(k_lbfgs_pairs, dim3((unsigned)(g.T * l.c.slices), g.nb), dim3(256), 0, st, l); GAMD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_lbfgs_dots, dim3(l.c.blocks, g.nb), dim3(256), 0, st, l); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_lbfgs_update, dim3((unsigned)g.T, g.nb), dim3(256), 0, st, l); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_lbfgs_store_x(const LbfgsArgs& l, const int* gates, float* x_out, hipStream_t st) {
    PassGeom g;
    if (lbfgs_check(l, &g) || !gates || !x_out) return -1;
    hipLaunchKernelGGL(k_lbfgs_store_x, dim3((unsigned)g.T, g.nb), dim3(256), 0, st, l, gates, x_out); GAMD_CHECK_LAUNCH();
    return 0;
}
