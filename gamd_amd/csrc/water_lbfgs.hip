// water_lbfgs.hip — the water L-BFGS energy minimiser (gamd_water_minimize_lbfgs): the limited-memory
// BFGS direction, the backtracking line search on the sufficient-decrease condition and the result row of lbfgs.hip, on the
// RIGID 3-site molecules and under the potential of water_minimize.hip, per box, with positions, forces, the ring and every
// scalar in double on the device.  The iterate lives on the manifold of rigid molecules: F is the classical force projected onto
// the tangent space of the three bond constraints at x (FIRE-water's F_c, gamd_wmin_dev.h, unit weights), a trial is x + t d
// carried back onto the manifold by SETTLE, s = x_t - x as the doubles give it and y = F - F_t, each projected at its own
// point.  The ring's vectors are used AS STORED, without vector transport to the new point's tangent space: d is then not
// exactly tangent, SETTLE removes the normal part of the step, and the sufficient-decrease test guards descent.
// tests/water_lbfgs_ref.py states the recipe decision by decision; no parity with OpenMM's L-BFGS is claimed.
// One evaluation is six launches, whatever m is:
//
//   k_wmin_pairs, k_wmin_rho, k_water_sk, k_wmin_recip
//                   the four force launches of the water minimiser (launch_wmin_force, water_minimize.hip), unchanged, handed
//                   the TRIAL positions xt and the gate set of this pass: there is no third copy of the pair and k walks.
//   k_wlb_mols      grid (blocks per box, boxes), one molecule at a time per thread: per atom the pair slices added in order
//                   from 0, the k slices added in order from 0, the raw force as k_wmin_mols forms it (kJ/mol/nm), projected
//                   at xt: Ft to ft; s = xt - x, y = F - Ft, and the molecule's terms of every scalar the decision and the next
//                   direction need: sum u_LJ, sum u_coul, sum z^2, Ft.Ft, F.s, s.s, s.y, y.y, s.Ft, y.Ft, max |Ft_i|, and for
//                   every ring slot k s.y_k, Ft.s_k, Ft.y_k.  Per-thread sums over the thread's molecules (fixed assignment),
//                   then the block tree of gamd_fire_block_tree into one row per block.
//   k_wlb_update    grid (molecule tiles, boxes), one thread per molecule.  Thread q of EVERY workgroup adds column q of the
//                   block rows in order (one more thread the k blocks' A |S|^2 in order); U = ((U_coul + U_recip) + U_self) +
//                   U_LJ as k_wmin_update spells it; every thread takes the same decision from the same bits and runs the
//                   two-loop recursion on the ring's inner products alone (gamd_lbfgs_dev.h); on acceptance the push into the
//                   ring, x = xt, F = Ft; then its molecule's d from the ring, s = t d with ONE factor per molecule so that
//                   the largest |s| of its three atoms is at most max_step, and xt = SETTLE(reference x, new x + s).
//
// The scalar body (decision, ring products, recursion) is gamd_lbfgs_dev.h's, shared with k_lbfgs_update (lbfgs.hip), which
// keeps its registers (81 VGPRs, no spill) and its bits on it.
// Pass `it`, the two state slots and the alternating gate sets are lbfgs.hip's: no thread reads what its launch writes, so a box
// that stops on an accepted step is still stored by every workgroup of that pass, and the pass behind only hands the gate on.
// Fixed assignment, no floating-point atomics, contraction off, plain stores: the same bits run after run, and a box gets the
// bits it gets alone.  Checked build: the two ring numbers a thread reads from the state (pairs held, next slot) pass through
// GAMD_CHK_RANGE before they address the ring; nothing else read from memory is used as an address.
// Device memory besides the water classical observer's work buffers: 24 (2 m + 5) + 12 B per atom.
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_passes_dev.h"
#include "gamd_wmin_dev.h"
#include "gamd_lbfgs_dev.h"

namespace {

using namespace gamd_wmin;

__device__ __forceinline__ int wlb_boxes(const WaterArgs& a) { return a.bx.n_boxes > 1 ? a.bx.n_boxes : 1; }
__device__ __forceinline__ const int* wlb_gates_in(const WLbfgsArgs& l) { return l.gates + (size_t)(l.it & 1) * (size_t)wlb_boxes(l.w); }
// ring vector: s of slot k (which = 0) or y of slot k (which = 1)
__device__ __forceinline__ double* wlb_ring(const WLbfgsArgs& l, int which, int k) {
    return l.ring + ((size_t)which * (size_t)l.m + (size_t)k) * 3 * (size_t)l.w.n;
}
__device__ __forceinline__ double dot3(const D3 (&p)[3], const D3 (&q)[3]) { return (dot(p[0], q[0]) + dot(p[1], q[1])) + dot(p[2], q[2]); }

// x = xt = the input widened and put on the exact rigid geometry (SETTLE with reference = new = the input), F = 0 (the start's
// pass reads it and uses none of it), the scalar state of the start, both gates open, the row cleared
__global__ void __launch_bounds__(256) k_wlb_init(WLbfgsArgs l, const float* __restrict__ x) {
    const int box = blockIdx.y, nmol = gamd_npb(l.w) / 3, nb = wlb_boxes(l.w);
    const int ml = blockIdx.x * GAMD_PASS_TILE + threadIdx.x;
    if (blockIdx.x == 0) {
        double* st = l.state + (size_t)box * 2 * LBFGS_SLOT;
        for (int q = threadIdx.x; q < 2 * LBFGS_SLOT; q += 256) st[q] = q == 0 ? 1.0 : 0.0;        // t = 1
        if (threadIdx.x < LBFGS_ROW) l.rows[(size_t)box * LBFGS_ROW + threadIdx.x] = 0.0;
        if (threadIdx.x == 0) { l.gates[box] = 0; l.gates[(size_t)nb + box] = 0; }
    }
    if (ml >= nmol) return;
    const size_t mol = (size_t)box * (size_t)nmol + (size_t)ml;
    D3 x0[3], x1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x0[k] = {(double)x[9 * mol + 3 * k], (double)x[9 * mol + 3 * k + 1], (double)x[9 * mol + 3 * k + 2]};
        x1[k] = x0[k];
    }
    settle(x0, x1, l.ra, l.rb, l.rc);
    store_mol(l.x, mol, x1); store_mol(l.xt, mol, x1);
    const D3 zero[3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    store_mol(l.f, mol, zero);
}

__global__ void __launch_bounds__(256) k_wlb_mols(WLbfgsArgs l) {
    const WaterArgs& a = l.w;
    const int box = blockIdx.y;
    if (wlb_gates_in(l)[box]) return;
    const int npb = gamd_npb(a), nmol = npb / 3;
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    const double pref = a.coul8pi / ((Lx * Ly) * Lz);
    const double kfx = a.two_pi / Lx, kfy = a.two_pi / Ly, kfz = a.two_pi / Lz;
    const double* cur = l.state + ((size_t)box * 2 + (size_t)(l.it & 1)) * LBFGS_SLOT;
    const int cnt = GAMD_CHK_RANGE(l.sticky, (int)cur[2], 0, l.m, GAMD_CHK_WLBFGS_COUNT);  // the slots 0 .. cnt - 1 hold pairs
    double acc[WLB_ACC];
#pragma unroll
    for (int q = 0; q < WLB_ACC; ++q) acc[q] = 0.0;
    for (int ml = blockIdx.x * blockDim.x + threadIdx.x; ml < nmol; ml += gridDim.x * blockDim.x) {
        const size_t mol = (size_t)box * (size_t)nmol + (size_t)ml;
        D3 ft[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {                       // the raw force, k_wmin_mols' statements
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
            ft[k] = {(t0 + (pq * kfx) * g0) * a.len, (t1 + (pq * kfy) * g1) * a.len, (t2 + (pq * kfz) * g2) * a.len};  // kJ/mol/nm
            acc[WLB_ULJ] += t3; acc[WLB_UC] += t4;
            const double z = o ? -2.0 : 1.0;                // the charge in units of q_h: sums of these are exact
            acc[WLB_Z2] += z * z;
        }
        D3 x[3], xt[3], f[3], s[3], y[3];
        load_mol(l.x, mol, x); load_mol(l.xt, mol, xt); load_mol(l.f, mol, f);
        project(xt, ft);
        store_mol(l.ft, mol, ft);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s[k] = xt[k] - x[k];
            y[k] = f[k] - ft[k];
            acc[WLB_MAX] = fmax(acc[WLB_MAX], sqrt(dot(ft[k], ft[k])));
        }
        acc[WLB_FTFT] += dot3(ft, ft);
        acc[WLB_FS] += dot3(f, s);
        acc[WLB_SS] += dot3(s, s);
        acc[WLB_SY] += dot3(s, y);
        acc[WLB_YY] += dot3(y, y);
        acc[WLB_SFT] += dot3(s, ft);
        acc[WLB_YFT] += dot3(y, ft);
        // the molecule's s and y of slot 0, stepped from slot to slot in vector registers: sixteen slot bases held as scalars
        // through the unrolled loop overflow the scalar file (five scalar spills)
        const double* rs = wlb_ring(l, 0, 0) + 9 * mol;
        const double* ry = wlb_ring(l, 1, 0) + 9 * mol;
#pragma unroll
        for (int k = 0; k < LBFGS_M; ++k) {
            if (k < cnt) {                                  // (uniform)
                D3 sk[3], yk[3];
                load_mol(rs, 0, sk); load_mol(ry, 0, yk);
                acc[WLB_SYK + k] += dot3(s, yk);
                acc[WLB_FTSK + k] += dot3(ft, sk);
                acc[WLB_FTYK + k] += dot3(ft, yk);
                rs += 3 * (size_t)a.n; ry += 3 * (size_t)a.n;
                asm volatile("" : "+v"(rs), "+v"(ry));
            }
        }
    }
    // gamd_fire_block_tree's tree on WLB_ACC accumulators: all but the last summed, the last maximised
    __shared__ double red[4][WLB_ACC];
#pragma unroll
    for (int q = 0; q < WLB_ACC; ++q) {
        double v = acc[q];
        if (q < WLB_MAX) v = gamd_wave_sum(v);
        else {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_down(v, d, 64));
        }
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < WLB_ACC) {
        const int q = threadIdx.x;
        const double r = q < WLB_MAX ? (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]) : fmax(fmax(red[0][q], red[1][q]), fmax(red[2][q], red[3][q]));
        l.blk[((size_t)box * (size_t)a.blocks + blockIdx.x) * WLB_ACC + q] = r;
    }
}

__global__ void __launch_bounds__(256) k_wlb_update(WLbfgsArgs l) {
    const WaterArgs& a = l.w;
    const int box = blockIdx.y, nb = wlb_boxes(a), tid = threadIdx.x;
    const bool writer = blockIdx.x == 0 && tid == 0;        // one thread per box
    int* gates_out = l.gates + (size_t)((l.it + 1) & 1) * (size_t)nb;
    const int gate = wlb_gates_in(l)[box];
    if (gate) {                                             // stopped in an earlier pass: the gate goes on to the other set
        if (writer) gates_out[box] = gate;
        return;
    }
    __shared__ double sacc[WLB_ACC + 1];                    // the block rows' columns, and the k blocks' sum behind them
    __shared__ double g_sy[LBFGS_M * LBFGS_M], g_yy[LBFGS_M * LBFGS_M], g_fs[LBFGS_M], g_fy[LBFGS_M];   // the ring's products, oldest pair first
    const int npb = gamd_npb(a), nmol = npb / 3;
    if (tid < WLB_ACC) {                                    // the blocks in order: every workgroup gets the same bits
        double v = 0.0;
        for (int b = 0; b < a.blocks; ++b) {
            const double p = l.blk[((size_t)box * (size_t)a.blocks + b) * WLB_ACC + tid];
            v = tid < WLB_MAX ? v + p : fmax(v, p);
        }
        sacc[tid] = v;
    } else if (tid == WLB_ACC) {
        double us = 0.0;
        for (int b = 0; b < a.kblocks; ++b) us += a.ublk[(size_t)box * (size_t)a.kblocks + b];
        sacc[WLB_ACC] = us;
    }
    __syncthreads();
    const double* cur = l.state + ((size_t)box * 2 + (size_t)(l.it & 1)) * LBFGS_SLOT;
    double* nxt = l.state + ((size_t)box * 2 + (size_t)((l.it + 1) & 1)) * LBFGS_SLOT;
    double* row = l.rows + (size_t)box * LBFGS_ROW;
    gamd_lbfgs::Scalars sc = gamd_lbfgs::load_scalars(cur);
    const int cnt = GAMD_CHK_RANGE(l.sticky, (int)cur[2], 0, l.m, GAMD_CHK_WLBFGS_COUNT);
    const int head = GAMD_CHK_RANGE(l.sticky, (int)cur[3], 0, l.m - 1, GAMD_CHK_WLBFGS_SLOT);  // the slot a push writes
    const double V = (gamd_box_edge(a, box, 0) * gamd_box_edge(a, box, 1)) * gamd_box_edge(a, box, 2);
    // k_water_final's terms, as k_wmin_update composes them: every pair sits in two rows
    const double u_lj = 0.5 * sacc[WLB_ULJ], u_coul = 0.5 * sacc[WLB_UC], u_recip = (a.coul4pi / V) * sacc[WLB_ACC];
    const double u_self = -(a.self_c * ((a.q_h * a.q_h) * sacc[WLB_Z2]));
    const double Ut = ((u_coul + u_recip) + u_self) + u_lj;
    const double ftft = sacc[WLB_FTFT], sy = sacc[WLB_SY], yy = sacc[WLB_YY];
    const double rms_t = sqrt(ftft / (3.0 * (double)npb));
    const bool start = l.it == 0;

    // ---- the decision, by every thread from the same bits ----
    if (start && writer) { row[3] = Ut; row[4] = rms_t; }
    const gamd_lbfgs::Decision dc = gamd_lbfgs::decide(l, start, cnt, Ut, ftft, sacc[WLB_MAX], rms_t, sacc[WLB_FS], sacc[WLB_SS], sy, yy, sc);

    // ---- the accepted point: the ring's new pair, x = xt, F = Ft (a box that stops here still takes it) ----
    const int ml = blockIdx.x * GAMD_PASS_TILE + tid;
    const bool vi = ml < nmol;
    const size_t mol = (size_t)box * (size_t)nmol + (size_t)(vi ? ml : 0);
    const D3 zero = {0.0, 0.0, 0.0};
    D3 x[3] = {zero, zero, zero}, f[3] = {zero, zero, zero};
    if (vi && dc.stop != 1 + LBFGS_FAILED) {
        load_mol(l.x, mol, x); load_mol(l.f, mol, f);
        if (dc.accept) {
            D3 xt[3], ft[3];
            load_mol(l.xt, mol, xt); load_mol(l.ft, mol, ft);
            if (dc.push) {
                const D3 s[3] = {xt[0] - x[0], xt[1] - x[1], xt[2] - x[2]};
                const D3 y[3] = {f[0] - ft[0], f[1] - ft[1], f[2] - ft[2]};
                store_mol(wlb_ring(l, 0, head), mol, s); store_mol(wlb_ring(l, 1, head), mol, y);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) { x[k] = xt[k]; f[k] = ft[k]; }
            store_mol(l.x, mol, x); store_mol(l.f, mol, f);
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
    const gamd_lbfgs::Ring rg = gamd_lbfgs::ring_next(l.m, cnt, head, dc, cur, nxt, blockIdx.x == 0, tid, sy, yy, sacc[WLB_SFT], sacc[WLB_YFT],
                                                     sacc + WLB_SYK, sacc + WLB_FTSK, sacc + WLB_FTYK, g_sy, g_yy, g_fs, g_fy);
    if (writer) {
        nxt[0] = sc.t; nxt[1] = sc.ls; nxt[2] = (double)rg.cnt; nxt[3] = (double)rg.head; nxt[4] = sc.U; nxt[5] = sc.FF; nxt[6] = sc.fm;
        nxt[7] = sc.n_acc; nxt[8] = sc.n_skip; nxt[9] = sc.n_reset;
        gates_out[box] = 0;
    }
    __syncthreads();

    // ---- the direction: kept through a line search, new behind an accepted step or an emptied ring ----
    D3 d[3] = {zero, zero, zero};
    if (dc.accept || dc.reset) {
        if (rg.cnt == 0) {                                  // steepest descent, the longest per-atom step max_step
            const double sd = l.max_step / sc.fm;
            if (vi) { d[0] = sd * f[0]; d[1] = sd * f[1]; d[2] = sd * f[2]; }
        } else {                                            // the two-loop recursion on the coefficients of d
            double cf, cs[LBFGS_M], cy[LBFGS_M];
            gamd_lbfgs::coefficients(rg.cnt, g_sy, g_yy, g_fs, g_fy, cf, cs, cy);
            if (vi) {
                d[0] = cf * f[0]; d[1] = cf * f[1]; d[2] = cf * f[2];
#pragma unroll
                for (int j = 0; j < LBFGS_M; ++j) {
                    if (j < rg.cnt) {
                        D3 v[3];
                        load_mol(wlb_ring(l, 0, rg.slot_of(j)), mol, v);
                        d[0] = d[0] + (cs[j] * v[0]); d[1] = d[1] + (cs[j] * v[1]); d[2] = d[2] + (cs[j] * v[2]);
                    }
                }
#pragma unroll
                for (int j = 0; j < LBFGS_M; ++j) {
                    if (j < rg.cnt) {
                        D3 v[3];
                        load_mol(wlb_ring(l, 1, rg.slot_of(j)), mol, v);
                        d[0] = d[0] + (cy[j] * v[0]); d[1] = d[1] + (cy[j] * v[1]); d[2] = d[2] + (cy[j] * v[2]);
                    }
                }
            }
        }
        if (vi) store_mol(l.d, mol, d);
    } else if (vi) {
        load_mol(l.d, mol, d);
    }
    if (!vi) return;

    // ---- the next trial: one factor for the molecule, then SETTLE back onto the rigid geometry ----
    D3 xn[3];
    double big = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        xn[k] = sc.t * d[k];                                // s
        big = fmax(big, sqrt(dot(xn[k], xn[k])));
    }
    const bool clamp = big > l.max_step;
    const double sf = clamp ? l.max_step / big : 1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) xn[k] = x[k] + (clamp ? sf * xn[k] : xn[k]);
    settle(x, xn, l.ra, l.rb, l.rc);
    store_mol(l.xt, mol, xn);
}

// k_wmin_store_x's store under the gates of the last pass: a box that failed keeps the x it was given, and x64_out is that x widened
__global__ void __launch_bounds__(256) k_wlb_store_x(WLbfgsArgs l, const int* __restrict__ gates, float* __restrict__ x_io, double* __restrict__ x64_out) {
    const WaterArgs& a = l.w;
    const int box = blockIdx.y, nmol = gamd_npb(a) / 3;
    const int ml = blockIdx.x * GAMD_PASS_TILE + threadIdx.x;
    if (ml >= nmol) return;
    const size_t mol = (size_t)box * (size_t)nmol + (size_t)ml;
    if (gates[box] == 1 + LBFGS_FAILED) {
        if (x64_out)
            for (int q = 0; q < 9; ++q) x64_out[9 * mol + q] = (double)x_io[9 * mol + q];
        return;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) store_wrapped(l.x, mol, d, gamd_box_edge(a, box, d), x_io, x64_out);
}

// what every launcher checks: the force launches' checks on the trial positions, and every buffer of the minimiser's own
// (`routed`: a block of gamd_water_minimize_potential, water_relax.hip — the k side is the route's and its launchers' to check)
int wlbfgs_check(const WLbfgsArgs& l, WMinArgs* force, PassGeom* g, long long* mol_tiles, bool routed = false) {
    const WaterArgs& a = l.w;
    if (pass_geometry(a, 3, g) || a.blocks < 1 || a.blocks > 65535) return -1;
    if (routed ? a.kblocks < 1 : pass_k_geometry(a, g->T, false)) return -1;
    if (!routed && (!a.kvec || !a.rho_partial || !a.sk)) return -1;
    if (!a.species || !a.part || !a.ublk || !a.rpart || !a.box_edges || !a.devflags) return -1;
    if (!l.x || !l.xt || !l.f || !l.ft || !l.d || !l.ring || !l.blk || !l.state || !l.gates || !l.rows) return -1;
    if (l.m < 1 || l.m > LBFGS_M || l.max_ls < 1 || l.it < 0 || l.max_iter < 0) return -1;
    if (!(l.ra > 0.0) || !(l.rb > 0.0) || !(l.rc > 0.0)) return -1;
    *mol_tiles = (g->npb / 3 + GAMD_PASS_TILE - 1) / GAMD_PASS_TILE;
    *force = WMinArgs{};
    force->w = a;
    force->fire.x64 = l.xt;
    force->fire.stopped = l.gates + (size_t)(l.it & 1) * (size_t)g->nb;
    force->ra = l.ra; force->rb = l.rb; force->rc = l.rc;
    return 0;
}

}  // namespace

int launch_wlbfgs_init(const WLbfgsArgs& l, const float* x, hipStream_t st) {
    PassGeom g; long long M; WMinArgs force;
    if (wlbfgs_check(l, &force, &g, &M) || !x) return -1;
    hipLaunchKernelGGL(k_wlb_init, dim3((unsigned)M, g.nb), dim3(256), 0, st, l, x); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_wlbfgs_eval(const WLbfgsArgs& l, hipStream_t st) {
    PassGeom g; long long M; WMinArgs force;
    if (wlbfgs_check(l, &force, &g, &M)) return -1;
    if (int r = launch_wmin_force(force, st)) return r;
    hipLaunchKernelGGL(k_wlb_mols, dim3(l.w.blocks, g.nb), dim3(256), 0, st, l); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_wlb_update, dim3((unsigned)M, g.nb), dim3(256), 0, st, l); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_wlbfgs_store_x(const WLbfgsArgs& l, const int* gates, float* x_io, double* x64_out, hipStream_t st) {
    PassGeom g; long long M; WMinArgs force;
    if (wlbfgs_check(l, &force, &g, &M) || !gates || !x_io) return -1;
    hipLaunchKernelGGL(k_wlb_store_x, dim3((unsigned)M, g.nb), dim3(256), 0, st, l, gates, x_io, x64_out); GAMD_CHECK_LAUNCH();
    return 0;
}

// ---- the pieces water_relax.hip puts its routes together from (gamd_water_minimize_potential) ----------------------------
// k_wlb_update alone, behind a molecule pass that wrote k_wlb_mols' columns
int launch_wlbfgs_update(const WLbfgsArgs& l, hipStream_t st) {
    PassGeom g; long long M; WMinArgs force;
    if (wlbfgs_check(l, &force, &g, &M, true)) return -1;
    hipLaunchKernelGGL(k_wlb_update, dim3((unsigned)M, g.nb), dim3(256), 0, st, l); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_wlbfgs_init_routed(const WLbfgsArgs& l, const float* x, hipStream_t st) {
    PassGeom g; long long M; WMinArgs force;
    if (wlbfgs_check(l, &force, &g, &M, true) || !x) return -1;
    hipLaunchKernelGGL(k_wlb_init, dim3((unsigned)M, g.nb), dim3(256), 0, st, l, x); GAMD_CHECK_LAUNCH();
    return 0;
}

int launch_wlbfgs_store_x_routed(const WLbfgsArgs& l, const int* gates, float* x_io, double* x64_out, hipStream_t st) {
    PassGeom g; long long M; WMinArgs force;
    if (wlbfgs_check(l, &force, &g, &M, true) || !gates || !x_io) return -1;
    hipLaunchKernelGGL(k_wlb_store_x, dim3((unsigned)M, g.nb), dim3(256), 0, st, l, gates, x_io, x64_out); GAMD_CHECK_LAUNCH();
    return 0;
}
