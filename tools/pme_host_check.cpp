// pme_host_check.cpp — gamd_amd/csrc/gamd_pme_dev.h without a GPU and without ROCm: the grid index of a coordinate, the wrapped
// stencil, the B-spline recursion and the host's tables, called from a plain main() that tests/test_water_pme_host.py builds with
// the address and undefined-behaviour sanitizers.  Prints one line per property ("name ok count"); the first violation is
// printed as "name FAIL ..." and the exit status is 1.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../gamd_amd/csrc/gamd_pme_dev.h"

namespace {

int g_fail = 0;
const int LENGTHS[] = {8, 16, 32, 64, 128};

double ulp(double v) { return std::nextafter(std::fabs(v), INFINITY) - std::fabs(v); }

// every stencil point of x on every grid and both orders lies in [0, n); w is in [0, 1), or NaN exactly for a non-finite x
long check_index(double x, double L) {
    long n_checked = 0;
    for (int n : LENGTHS)
        for (int p : {4, 6}) {
            double w = -1.0;
            const int base = gamd_pme_index(x, L, n, &w);
            const bool finite = std::isfinite(x);
            if (base < 0 || base >= n || (finite ? !(w >= 0.0 && w < 1.0) : !std::isnan(w))) {
                std::printf("index FAIL x=%a L=%a n=%d base=%d w=%a\n", x, L, n, base, w);
                g_fail = 1;
            }
            for (int j = 0; j < p; ++j) {
                const int i = gamd_pme_wrap(base, j, n, p);
                if (i < 0 || i >= n) { std::printf("wrap FAIL x=%a L=%a n=%d p=%d j=%d i=%d\n", x, L, n, p, j, i); g_fail = 1; }
                ++n_checked;
            }
            // a coordinate that is not finite spreads nothing: every term of its stencil is quantised to 0
            if (!finite) {
                double th[6], dth[6];
                if (p == 4) gamd_pme_spline<4>(w, th, dth); else gamd_pme_spline<6>(w, th, dth);
                for (int j = 0; j < p; ++j)
                    if (gamd_pme_quantum((-2.0 * th[j]) * (th[0] * th[1])) != 0 || !std::isnan(dth[j])) {
                        std::printf("nonfinite FAIL x=%a p=%d j=%d\n", x, p, j); g_fail = 1;
                    }
            }
        }
    return n_checked;
}

template <int P>
long check_spline(std::mt19937_64& rng, int draws) {
    std::uniform_real_distribution<double> U(0.0, 1.0);
    long n_checked = 0;
    for (int k = 0; k < draws + 3; ++k) {
        const double w = k == draws ? 0.0 : (k == draws + 1 ? std::nextafter(1.0, 0.0) : (k == draws + 2 ? DBL_MIN : U(rng)));
        double th[P], dth[P];
        gamd_pme_spline<P>(w, th, dth);
        double s = 0.0, d = 0.0, ad = 0.0;
        for (int j = 0; j < P; ++j) {
            if (!(th[j] >= 0.0 && th[j] <= 1.0)) { std::printf("spline FAIL P=%d w=%a theta[%d]=%a\n", P, w, j, th[j]); g_fail = 1; }
            s += th[j]; d += dth[j]; ad += std::fabs(dth[j]);
        }
        if (std::fabs(s - 1.0) > 4.0 * ulp(1.0)) { std::printf("spline FAIL P=%d w=%a sum theta - 1 = %a\n", P, w, s - 1.0); g_fail = 1; }
        if (std::fabs(d) > 4.0 * ulp(ad)) { std::printf("spline FAIL P=%d w=%a sum theta' = %a of %a\n", P, w, d, ad); g_fail = 1; }
        ++n_checked;
    }
    return n_checked;
}

}  // namespace

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    long n_index = 0;
    for (float Lf : {13.66f, 14.2f, 15.1f, 1.0f, 52.0f, 7.3403244f}) {
        const double L = (double)Lf;
        std::vector<double> xs = {nan, -nan, inf, -inf, 1e30, -1e30, (double)1e30f, (double)-1e30f, 0.0, -0.0, DBL_MIN, -DBL_MIN, 4.9e-324,
                                  -4.9e-324, -1e-20, -1.0, -0.5 * L, -123.456, DBL_MAX, -DBL_MAX, (double)FLT_MAX, (double)-FLT_MAX,
                                  (double)std::nextafterf(Lf, 0.f), (double)std::nextafterf(Lf, 1e9f), std::nextafter(L, 0.0),
                                  std::nextafter(L, 1e9), -(double)std::nextafterf(Lf, 0.f), 0.5 * L, 0.999999 * L};
        for (int k = -5; k <= 5; ++k) {                     // exact multiples of L, and their neighbours in fp32 and in double
            const double m = (double)k * L;
            xs.push_back(m); xs.push_back((double)(float)m);
            xs.push_back(std::nextafter(m, inf)); xs.push_back(std::nextafter(m, -inf));
            xs.push_back((double)std::nextafterf((float)m, 1e9f)); xs.push_back((double)std::nextafterf((float)m, -1e9f));
        }
        for (int n : LENGTHS)                               // the grid lines themselves and their neighbours
            for (int i = 0; i <= n; ++i) {
                const double g = L * (double)i / (double)n;
                xs.push_back(g); xs.push_back(std::nextafter(g, inf)); xs.push_back(std::nextafter(g, -inf));
            }
        for (double x : xs) n_index += check_index(x, L);
    }
    std::printf("index %s %ld\n", g_fail ? "FAIL" : "ok", n_index);

    std::mt19937_64 rng(20240611);
    const long n4 = check_spline<4>(rng, 10000), n6 = check_spline<6>(rng, 10000);
    std::printf("spline %s %ld\n", g_fail ? "FAIL" : "ok", n4 + n6);

    long n_mod = 0;
    for (int p : {4, 6})
        for (int n : LENGTHS) {
            const std::vector<double> mod = gamd_pme_moduli(p, n);
            if ((int)mod.size() != n) { std::printf("moduli FAIL p=%d n=%d size %zu\n", p, n, mod.size()); g_fail = 1; continue; }
            double lo = mod[0];
            for (int m = 0; m < n; ++m) {
                lo = std::fmin(lo, mod[(size_t)m]);
                if (!(mod[(size_t)m] > 0.0 && mod[(size_t)m] <= 1.0 + 8.0 * DBL_EPSILON)) { std::printf("moduli FAIL p=%d n=%d m=%d %a\n", p, n, m, mod[(size_t)m]); g_fail = 1; }
                if (m && std::fabs(mod[(size_t)m] - mod[(size_t)(n - m)]) > 64.0 * DBL_EPSILON) { std::printf("moduli FAIL p=%d n=%d m=%d asymmetric\n", p, n, m); g_fail = 1; }
                ++n_mod;
            }
            if (std::fabs(mod[0] - 1.0) > 8.0 * DBL_EPSILON || lo != mod[(size_t)(n / 2)]) { std::printf("moduli FAIL p=%d n=%d ends\n", p, n); g_fail = 1; }
            std::printf("modulus p=%d n=%d min %.17g\n", p, n, lo);
        }
    for (int p : {0, 1, 2, 3, 5, 7, 8})
        if (!gamd_pme_moduli(p, 16).empty() || gamd_pme_order_ok(p)) { std::printf("moduli FAIL order %d offered\n", p); g_fail = 1; }
    for (int n : {0, 1, 4, 12, 24, 100, 256, -8})
        if (!gamd_pme_moduli(4, n).empty() || gamd_pme_length_ok(n)) { std::printf("moduli FAIL length %d offered\n", n); g_fail = 1; }
    std::printf("moduli %s %ld\n", g_fail ? "FAIL" : "ok", n_mod);

    const std::vector<double> tw = gamd_pme_twiddles();
    if (tw.size() != 2 * (size_t)GAMD_PME_TW) { std::printf("twiddles FAIL size\n"); g_fail = 1; }
    for (int j = 0; j < GAMD_PME_TW && !g_fail; ++j) {
        const double c = tw[2 * (size_t)j], s = tw[2 * (size_t)j + 1];
        const double arg = 6.283185307179586476925286766559 * (double)j / 128.0;
        if (std::fabs(c * c + s * s - 1.0) > 4.0 * DBL_EPSILON || std::fabs(c - std::cos(arg)) > 2.0 * DBL_EPSILON ||
            std::fabs(s + std::sin(arg)) > 2.0 * DBL_EPSILON || (j && !(s < 0.0))) { std::printf("twiddles FAIL j=%d\n", j); g_fail = 1; }
    }
    if (tw[0] != 1.0 || tw[1] != 0.0 || tw[64] != 0.0 || tw[65] != -1.0) { std::printf("twiddles FAIL exact entries\n"); g_fail = 1; }
    std::printf("twiddles %s %d\n", g_fail ? "FAIL" : "ok", GAMD_PME_TW);
    return g_fail;
}
