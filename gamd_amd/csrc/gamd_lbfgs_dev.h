// gamd_lbfgs_dev.h — the scalar body of an L-BFGS decide/update pass, as every thread of the pass runs it from the same bits:
// the accept / reject decision of the backtracking line search with the stop tests, the ring's inner products brought up to
// date behind the decision, and the two-loop recursion on those inner products alone, which gives the coefficients of
// d = cf F + sum cs_j s_j + sum cy_j y_j.  Nothing here touches a vector: the two kernels that include it (k_lbfgs_update,
// lbfgs.hip: one thread per atom; k_wlb_update, water_lbfgs.hip: one thread per molecule) load and store their own atoms or
// molecules.  Contraction is off from here on, as in the files that include it.
#pragma once
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

namespace gamd_lbfgs {

// the scalars of a state slot that a decision changes: cur[0], cur[1], cur[4] .. cur[9]
struct Scalars { double t, ls, U, FF, fm, n_acc, n_skip, n_reset; };
struct Decision { int stop; bool accept, push, reset; };    // stop: 0, or 1 + LBFGS_*

__device__ __forceinline__ Scalars load_scalars(const double* cur) { return {cur[0], cur[1], cur[4], cur[5], cur[6], cur[7], cur[8], cur[9]}; }

// l: an argument block with it, max_iter, tol, c1, curv, max_ls.  `start`: the pass of the start (nothing to compare with).
// cnt: pairs the ring holds.  Ut, ftft, fmax_t, rms_t: U, F.F, max |F_i| and the rms at the trial; fs = F.s, ss, sy, yy.
template <class L>
__device__ __forceinline__ Decision decide(const L& l, bool start, int cnt, double Ut, double ftft, double fmax_t, double rms_t,
                                           double fs, double ss, double sy, double yy, Scalars& s) {
    Decision d{0, false, false, false};
    if (start) {
        d.accept = true;
        if (!isfinite(Ut) || !isfinite(ftft)) { d.stop = 1 + LBFGS_FAILED; s.U = Ut; s.FF = ftft; s.fm = fmax_t; }
    } else {
        d.accept = fs > 0.0 && isfinite(Ut) && Ut <= s.U - l.c1 * fs;
    }
    if (!d.stop) {
        if (d.accept) {
            if (!start) {
                d.push = sy > l.curv * sqrt(ss * yy);
                s.n_acc += 1.0;
                if (!d.push) s.n_skip += 1.0;
            }
            s.U = Ut; s.FF = ftft; s.fm = fmax_t;
            if (rms_t <= l.tol) d.stop = 1 + LBFGS_CONVERGED;
            else if (l.it == l.max_iter) d.stop = 1 + LBFGS_MAX_ITER;
            s.t = 1.0; s.ls = 0.0;
        } else if (l.it == l.max_iter) {
            d.stop = 1 + LBFGS_MAX_ITER;
        } else {
            s.ls += 1.0;
            if (s.ls >= (double)l.max_ls || !(fs > 0.0)) {  // the search has failed
                if (cnt > 0) { d.reset = true; s.n_reset += 1.0; s.t = 1.0; s.ls = 0.0; }
                else d.stop = 1 + LBFGS_LINE_SEARCH;
            } else {
                s.t = s.t / 2.0;
            }
        }
    }
    return d;
}

// the ring behind a decision: pairs held, the slot the next push writes, the slot of the oldest pair
struct Ring {
    int m, cnt, head, oldest;
    __device__ __forceinline__ int slot_of(int j) const { const int p = oldest + j; return p >= m ? p - m : p; }   // pair j, oldest first
};

// The ring's inner products of the next pass: into nxt[LBFGS_SY ..] by ring slot where `store` (one workgroup per box), and
// into g_sy, g_yy [M][M], g_fs, g_fy [M] (shared memory of the caller) with the pairs counted from the oldest.  cur: the slot
// this pass reads.  sy, yy, sft, yft: s.y, y.y, s.Ft, y.Ft of the trial; syk, ftsk, ftyk [M]: s.y_k, Ft.s_k, Ft.y_k by ring slot
// (y = F - Ft: y.v = F.v - Ft.v).  Threads 0 .. M * M - 1 of the workgroup do the work; the caller synchronises behind it.
__device__ __forceinline__ Ring ring_next(int m, int cnt, int head, const Decision& dc, const double* cur, double* nxt, bool store, int tid,
                                          double sy, double yy, double sft, double yft, const double* syk, const double* ftsk, const double* ftyk,
                                          double* g_sy, double* g_yy, double* g_fs, double* g_fy) {
    const bool push = dc.push, accept = dc.accept;
    Ring r;
    r.m = m;
    r.cnt = dc.reset ? 0 : (push ? (cnt + 1 < m ? cnt + 1 : m) : cnt);
    r.head = dc.reset ? 0 : (push ? (head + 1 == m ? 0 : head + 1) : head);
    r.oldest = r.cnt < m ? 0 : r.head;
    auto n_sy = [&](int p, int q) -> double {               // s_p . y_q
        if (push && p == head) return q == head ? sy : syk[q];
        if (push && q == head) return cur[LBFGS_FS + p] - ftsk[p];         // s_p . (F - Ft)
        return cur[LBFGS_SY + p * LBFGS_M + q];
    };
    auto n_yy = [&](int p, int q) -> double {
        if (push && p == head) return q == head ? yy : cur[LBFGS_FY + q] - ftyk[q];
        if (push && q == head) return cur[LBFGS_FY + p] - ftyk[p];
        return cur[LBFGS_YY + p * LBFGS_M + q];
    };
    auto n_fs = [&](int p) -> double { return !accept ? cur[LBFGS_FS + p] : (push && p == head ? sft : ftsk[p]); };
    auto n_fy = [&](int p) -> double { return !accept ? cur[LBFGS_FY + p] : (push && p == head ? yft : ftyk[p]); };
    if (tid < LBFGS_M * LBFGS_M) {
        const int p = tid / LBFGS_M, q = tid % LBFGS_M;
        if (store) { nxt[LBFGS_SY + tid] = n_sy(p, q); nxt[LBFGS_YY + tid] = n_yy(p, q); }
        const bool in = p < r.cnt && q < r.cnt;             // here p, q count from the oldest pair
        g_sy[tid] = in ? n_sy(r.slot_of(p), r.slot_of(q)) : 0.0;
        g_yy[tid] = in ? n_yy(r.slot_of(p), r.slot_of(q)) : 0.0;
    }
    if (tid < LBFGS_M) {
        if (store) { nxt[LBFGS_FS + tid] = n_fs(tid); nxt[LBFGS_FY + tid] = n_fy(tid); }
        g_fs[tid] = tid < r.cnt ? n_fs(r.slot_of(tid)) : 0.0;
        g_fy[tid] = tid < r.cnt ? n_fy(r.slot_of(tid)) : 0.0;
    }
    return r;
}

// the two-loop recursion on the coefficients of d over the basis F, {s_j}, {y_j} (pairs oldest first), cnt >= 1 pairs held:
// d = cf F + sum cs_j s_j + sum cy_j y_j with H0 = s.y / y.y of the newest pair
__device__ __forceinline__ void coefficients(int cnt, const double* g_sy, const double* g_yy, const double* g_fs, const double* g_fy,
                                             double& cf, double (&cs)[LBFGS_M], double (&cy)[LBFGS_M]) {
    double al[LBFGS_M];
#pragma unroll
    for (int j = 0; j < LBFGS_M; ++j) { cy[j] = 0.0; cs[j] = 0.0; al[j] = 0.0; }
#pragma unroll
    for (int p = LBFGS_M - 1; p >= 0; --p) {
        if (p < cnt) {
            double sq = g_fs[p];
#pragma unroll
            for (int j = 0; j < LBFGS_M; ++j)
                if (j < cnt) sq = sq + cy[j] * g_sy[p * LBFGS_M + j];
            al[p] = sq / g_sy[p * LBFGS_M + p];
            cy[p] = cy[p] - al[p];
        }
    }
    const int nw = cnt - 1;                                 // the newest pair
    const double h0 = g_sy[nw * LBFGS_M + nw] / g_yy[nw * LBFGS_M + nw];
    cf = h0;
#pragma unroll
    for (int j = 0; j < LBFGS_M; ++j) cy[j] = h0 * cy[j];
#pragma unroll
    for (int p = 0; p < LBFGS_M; ++p) {
        if (p < cnt) {
            double yr = cf * g_fy[p];
#pragma unroll
            for (int j = 0; j < LBFGS_M; ++j)
                if (j < cnt) yr = yr + cy[j] * g_yy[p * LBFGS_M + j];
#pragma unroll
            for (int j = 0; j < LBFGS_M; ++j)
                if (j < cnt) yr = yr + cs[j] * g_sy[j * LBFGS_M + p];
            const double beta = yr / g_sy[p * LBFGS_M + p];
            cs[p] = cs[p] + (al[p] - beta);
        }
    }
}

}  // namespace gamd_lbfgs
