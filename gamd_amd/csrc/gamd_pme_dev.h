// gamd_pme_dev.h — what the smooth particle-mesh Ewald kernels (water_pme.hip) share with the host
// and with a plain C++ compiler: the grid index of a coordinate, the cardinal B-spline weights, the wrapped stencil index, and
// (host only) the tables that depend on the order and the grid length alone.  No ROCm header is needed to include it: a
// stand-alone host program (tools/pme_host_check.cpp) calls every function here under the address and undefined-behaviour
// sanitizers.
//
// Orders.  p = 4 and p = 6, compile-time.  Only EVEN orders are offered: for odd p the interpolation modulus
// |sum_k M_p(k + 1) exp(2 pi i m k / n)|^2 vanishes at m = n / 2, the convolution would divide by zero there, and the choice of
// a workaround (interpolating the neighbours, dropping the term) would become part of the potential.
//
// Safe addressing.  gamd_pme_index(x, L, n, &w) returns a base index in [0, n) for EVERY bit pattern of x: s = x / L -
// floor(x / L), u = s n, base = floor(u), w = u - base in [0, 1).  A negative x a rounding below zero gives s = 1 exactly; that
// is the image s = 0 and is taken as base 0, w = 0.  Exact multiples of L give base 0, w = 0; 1e30 is finite, x / L is an
// integer-valued double and s = 0.  A coordinate that is NaN or infinite gives u = NaN: base = 0 and w = NaN.  Such an atom
// SPREADS NOTHING (gamd_pme_quantum returns 0 for a term that is not finite: a 64-bit integer cannot carry a NaN), its weights
// are NaN, so the force gathered for it is NaN, and the only grid addresses its threads form are those of base 0 — inside the
// grid.  gamd_pme_wrap(base, j, n, p) = base + j - (p - 1), plus n if negative, is in [0, n) for base in [0, n), 0 <= j < p and
// n >= 8 > p - 1.
//
// The spread's domain.  One term z theta_x theta_y theta_z (|z| <= 2, every theta in [0, 1]) is quantised as
// llrint(term * 2^50), at most 2^-51 off; a grid point's sum is held in a signed 64-bit integer and so may reach 2^13 q_H in
// magnitude before it wraps — far beyond what any water configuration puts on one point (p^3 points share each charge).
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GAMD_PME_HD __host__ __device__ __forceinline__
#else
#define GAMD_PME_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

constexpr int GAMD_PME_MIN_N = 8, GAMD_PME_MAX_N = 128;     // grid lengths per axis: the powers of two in between
constexpr int GAMD_PME_TW = GAMD_PME_MAX_N / 2;             // twiddles of the longest line: exp(-2 pi i j / 128), j < 64
constexpr double GAMD_PME_QUANT = 1125899906842624.0;       // 2^50: quanta per q_H of the spread
constexpr double GAMD_PME_INV_QUANT = 1.0 / 1125899906842624.0;

GAMD_PME_HD bool gamd_pme_order_ok(int p) { return p == 4 || p == 6; }
GAMD_PME_HD bool gamd_pme_length_ok(int n) { return n == 8 || n == 16 || n == 32 || n == 64 || n == 128; }

// base index in [0, n) and the offset w of coordinate x in a box of edge L on a grid of n points (see "Safe addressing")
GAMD_PME_HD int gamd_pme_index(double x, double L, int n, double* w) {
    const double q = x / L;
    const double s = q - floor(q);
    const double u = s * (double)n;
    if (!(u >= 0.0 && u < (double)n)) {                     // s == 1 (the image s = 0), or not a number
        *w = u == u ? 0.0 : u;
        return 0;
    }
    const double b = floor(u);
    *w = u - b;
    return (int)b;
}

// grid index of stencil point j (0 <= j < p) of an atom with base index `base`: the point base + j - (p - 1), wrapped
GAMD_PME_HD int gamd_pme_wrap(int base, int j, int n, int p) {
    const int i = base + j - (p - 1);
    return i < 0 ? i + n : i;
}

// one step of Essmann's recursion (Essmann et al. 1995, eq. 4.1), in place: th[0 .. K-2] of order K - 1 become th[0 .. K-1] of
// order K (every loop bound is a compile-time constant: the arrays stay in registers)
template <int K>
GAMD_PME_HD void gamd_pme_raise(double w, double* th) {
    const double div = 1.0 / (double)(K - 1);
    th[K - 1] = (div * w) * th[K - 2];
#if defined(__clang__)
#pragma unroll
#endif
    for (int l = 1; l < K - 1; ++l)
        th[K - l - 1] = div * ((w + (double)l) * th[K - l - 2] + ((double)(K - l) - w) * th[K - l - 1]);
    th[0] = (div * (1.0 - w)) * th[0];
}

// the cardinal B-spline of order P at the P points of the stencil, th[j] = M_P(w + P - 1 - j), and its derivative in u,
// dth[j] = M_{P-1}(w + P - j) - M_{P-1}(w + P - 1 - j) (eq. 4.2), from the order-2 weights (1 - w, w)
template <int P>
GAMD_PME_HD void gamd_pme_spline(double w, double* th, double* dth) {
    static_assert(P == 4 || P == 6, "even orders only: see the header comment");
    th[0] = 1.0 - w; th[1] = w;
    gamd_pme_raise<3>(w, th);
    if (P == 6) { gamd_pme_raise<P == 6 ? 4 : 3>(w, th); gamd_pme_raise<P == 6 ? 5 : 3>(w, th); }
    dth[0] = -th[0];
#if defined(__clang__)
#pragma unroll
#endif
    for (int l = 1; l < P - 1; ++l) dth[l] = th[l - 1] - th[l];
    dth[P - 1] = th[P - 2];
    gamd_pme_raise<P>(w, th);
}

// one term of the spread in quanta of 2^-50 q_H; a term that is not finite spreads nothing
GAMD_PME_HD long long gamd_pme_quantum(double term) {
    if (!(fabs(term) <= 4.0)) return 0;                     // NaN, or outside what z theta^3 can be
    return llrint(term * GAMD_PME_QUANT);
}

#include <vector>
// ---- host only: the tables of one (order, length) ---------------------------------------------------------------------
// the interpolation modulus of order p on n points: mod[m] = |sum_{k=0}^{p-2} M_p(k + 1) exp(2 pi i m k / n)|^2, m in [0, n).
// Positive for even p.  Returns an empty vector for an order or length that is not offered.
inline std::vector<double> gamd_pme_moduli(int p, int n) {
    std::vector<double> mod;
    if (!gamd_pme_order_ok(p) || !gamd_pme_length_ok(n)) return mod;
    double th[6], dth[6];
    if (p == 4) gamd_pme_spline<4>(0.0, th, dth); else gamd_pme_spline<6>(0.0, th, dth);
    // w = 0: th[j] = M_p(p - 1 - j), so M_p(k + 1) = th[p - 2 - k] (th[p - 1] = M_p(0) = 0)
    mod.resize((size_t)n);
    const double two_pi = 6.283185307179586476925286766559;
    for (int m = 0; m < n; ++m) {
        double re = 0.0, im = 0.0;
        for (int k = 0; k <= p - 2; ++k) {
            const double arg = two_pi * (double)((m * k) % n) / (double)n;
            re += th[p - 2 - k] * std::cos(arg); im += th[p - 2 - k] * std::sin(arg);
        }
        mod[(size_t)m] = re * re + im * im;
    }
    return mod;
}

// the twiddles of the longest line, interleaved (cos, -sin)(2 pi j / 128), j < 64: a line of n points reads every (128 / n)-th
inline std::vector<double> gamd_pme_twiddles() {
    std::vector<double> tw(2 * (size_t)GAMD_PME_TW);
    const double two_pi = 6.283185307179586476925286766559;
    for (int j = 0; j < GAMD_PME_TW; ++j) {
        const double arg = two_pi * (double)j / (double)GAMD_PME_MAX_N;
        tw[2 * (size_t)j] = std::cos(arg); tw[2 * (size_t)j + 1] = -std::sin(arg);
    }
    tw[0] = 1.0; tw[1] = -0.0;
    tw[2 * 32] = 0.0; tw[2 * 32 + 1] = -1.0;                // exp(-i pi / 2), exactly
    return tw;
}
