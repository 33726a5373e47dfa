// cells_host_check.cpp — gamd_amd/csrc/gamd_cells_dev.h without a GPU and without ROCm: the cells per axis and per box, the cell of a
// coordinate and the neighbour cells of a cell, called from a plain main() that tests/test_water_cells_host.py builds with the
// address and undefined-behaviour sanitizers.  Prints one line per property ("name ok count"); the first violation is printed as
// "name FAIL ..." and the exit status is 1.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../gamd_amd/csrc/gamd_cells_dev.h"

namespace {

int g_fail = 0;

// the cell of x lies in [0, nc) for every nc from 1 to 64, and indexes a table of nc entries
long check_index(double x, double L) {
    long n_checked = 0;
    for (int nc = 1; nc <= GAMD_CELLS_MAX; ++nc) {
        std::vector<int> count((size_t)nc, 0);
        const int c = gamd_cells_index(x, L, nc);
        if (c < 0 || c >= nc) { std::printf("index FAIL x=%a L=%a nc=%d cell=%d\n", x, L, nc, c); g_fail = 1; continue; }
        ++count[(size_t)c];                                 // (under the address sanitizer)
        if (!std::isfinite(x) && c != 0) { std::printf("index FAIL x=%a nc=%d: a coordinate that is not finite is not in cell 0\n", x, nc); g_fail = 1; }
        ++n_checked;
    }
    return n_checked;
}

}  // namespace

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    // ---- the cell of a coordinate ------------------------------------------------------------------------------------------
    long n_index = 0;
    for (float Lf : {13.66f, 14.2f, 15.1f, 20.0f, 1.0f, 52.0f, 7.3403244f}) {
        const double L = (double)Lf;
        std::vector<double> xs = {nan, -nan, inf, -inf, 1e30, -1e30, (double)1e30f, (double)-1e30f, 0.0, -0.0, DBL_MIN, -DBL_MIN, 4.9e-324,
                                  -4.9e-324, -1e-20, -1e-17 * L, -1.0, -0.5 * L, -123.456, DBL_MAX, -DBL_MAX, (double)FLT_MAX, (double)-FLT_MAX,
                                  (double)std::nextafterf(Lf, 0.f), (double)std::nextafterf(Lf, 1e9f), std::nextafter(L, 0.0),
                                  std::nextafter(L, 1e9), -(double)std::nextafterf(Lf, 0.f), 0.5 * L, 0.999999 * L};
        for (int k = -5; k <= 5; ++k) {                     // exact multiples of L, and their neighbours in fp32 and in double
            const double m = (double)k * L;
            xs.push_back(m); xs.push_back((double)(float)m);
            xs.push_back(std::nextafter(m, inf)); xs.push_back(std::nextafter(m, -inf));
            xs.push_back((double)std::nextafterf((float)m, 1e9f)); xs.push_back((double)std::nextafterf((float)m, -1e9f));
        }
        for (int nc = 3; nc <= GAMD_CELLS_MAX; ++nc)        // the cell faces themselves and their neighbours
            for (int i = 0; i <= nc; ++i) {
                const double g = L * (double)i / (double)nc;
                xs.push_back(g); xs.push_back(std::nextafter(g, inf)); xs.push_back(std::nextafter(g, -inf));
            }
        for (double x : xs) n_index += check_index(x, L);
        // negative values that round to s = 1: q - floor(q) = 1 exactly, the image s = 0, cell 0
        for (double x : {-DBL_MIN, -1e-20, -1e-17 * L}) {
            const double q = x / L, s = q - std::floor(q);
            if (s != 1.0) { std::printf("index FAIL x=%a L=%a: s=%a is not 1\n", x, L, s); g_fail = 1; }
            for (int nc = 3; nc <= GAMD_CELLS_MAX; ++nc)
                if (gamd_cells_index(x, L, nc) != 0) { std::printf("index FAIL x=%a nc=%d: s = 1 is not cell 0\n", x, nc); g_fail = 1; }
        }
        // a face that is exact: x = L i / nc for L = 20 and nc = 5, 8 is cell i (i < nc), and x = L is cell 0
        if (Lf == 20.0f)
            for (int nc : {5, 8})
                for (int i = 0; i <= nc; ++i) {
                    const int c = gamd_cells_index(20.0 * (double)i / (double)nc, L, nc);
                    if (c != (i < nc ? i : 0)) { std::printf("index FAIL face i=%d nc=%d cell=%d\n", i, nc, c); g_fail = 1; }
                }
    }
    std::printf("index %s %ld\n", g_fail ? "FAIL" : "ok", n_index);

    // ---- cells per axis ----------------------------------------------------------------------------------------------------
    long n_axis = 0;
    for (double rc : {3.0, 4.2, 4.5, 6.8, 9.5, 12.0, 0.1, 1e-300, 1e300})
        for (double L : {2.0 * rc, std::nextafter(2.0 * rc, inf), 13.66, 14.2, 15.1, 20.0, 53.0, 110.0, 1e6, 1e300, 0.0, -1.0, nan, inf, -inf}) {
            const int nc = gamd_cells_per_axis(L, rc);
            if (nc < 1 || nc > GAMD_CELLS_MAX) { std::printf("axis FAIL L=%a rc=%a nc=%d\n", L, rc, nc); g_fail = 1; }
            if (std::isfinite(L) && L >= 2.0 * rc && std::isfinite(2.0 * L) && std::isfinite(rc * GAMD_CELLS_MARGIN)) {
                // the potential's condition gives three cells at least, and a cell's edge is r_cut / 2 and the margin at least
                if (nc < 3) { std::printf("axis FAIL L=%a rc=%a nc=%d below 3\n", L, rc, nc); g_fail = 1; }
                if (!(L / (double)nc >= 0.5 * rc * (1.0 + 0.5 / 1048576.0))) { std::printf("axis FAIL L=%a rc=%a nc=%d edge too short\n", L, rc, nc); g_fail = 1; }
            }
            ++n_axis;
        }
    for (double bad : {nan, 0.0, -1.0, inf})
        if (gamd_cells_per_axis(10.0, bad) < 1 || gamd_cells_per_axis(10.0, bad) > GAMD_CELLS_MAX) { std::printf("axis FAIL r_cut=%a\n", bad); g_fail = 1; }
    if (gamd_cells_per_axis(13.66f, 6.8) != 4 || gamd_cells_per_axis(15.1f, 4.2) != 7 || gamd_cells_per_axis(20.0, 6.8) != 5 ||
        gamd_cells_per_axis(20.0, 4.5) != 8 || gamd_cells_per_axis(20.0, 9.5) != 4 || gamd_cells_per_axis(15.1f, 3.0) != 10) {
        std::printf("axis FAIL the documented shapes\n"); g_fail = 1;
    }
    std::printf("axis %s %ld\n", g_fail ? "FAIL" : "ok", n_axis);

    // ---- cells per box: the product of the three axes' counts over every triple of the edges above, never more than 64^3 ----------
    long n_count = 0;
    for (double rc : {3.0, 4.2, 4.5, 6.8, 9.5, 12.0, 0.1, 1e-300, 1e300}) {
        const double Ls[] = {2.0 * rc, std::nextafter(2.0 * rc, inf), 13.66, 14.2, 15.1, 20.0, 53.0, 110.0, 1e6, 1e300, 0.0, -1.0, nan, inf, -inf};
        for (double Lx : Ls)
            for (double Ly : Ls)
                for (double Lz : Ls) {
                    int nc[3] = {-1, -1, -1};
                    const int cells = gamd_cells_count(Lx, Ly, Lz, rc, nc);
                    const int px = gamd_cells_per_axis(Lx, rc), py = gamd_cells_per_axis(Ly, rc), pz = gamd_cells_per_axis(Lz, rc);
                    if (nc[0] != px || nc[1] != py || nc[2] != pz || (long long)cells != (long long)px * py * pz || cells < 1 ||
                        cells > GAMD_CELLS_MAX * GAMD_CELLS_MAX * GAMD_CELLS_MAX) {
                        std::printf("count FAIL L=%a %a %a rc=%a: %d cells, nc %d %d %d\n", Lx, Ly, Lz, rc, cells, nc[0], nc[1], nc[2]); g_fail = 1;
                    }
                    ++n_count;
                }
    }
    std::printf("count %s %ld\n", g_fail ? "FAIL" : "ok", n_count);

    // ---- neighbour cells: in range, no cell twice, every cell within two (wrapped) is there, the order is the documented one ----
    long n_nb = 0;
    for (int nc = 1; nc <= GAMD_CELLS_MAX; ++nc) {
        const int span = gamd_cells_span(nc);
        if (span != (nc >= 5 ? 5 : nc)) { std::printf("neighbour FAIL span nc=%d\n", nc); g_fail = 1; }
        for (int c = 0; c < nc; ++c) {
            std::vector<int> seen((size_t)nc, 0);
            for (int j = 0; j < span; ++j) {
                const int i = gamd_cells_neighbour(c, j, nc);
                if (i < 0 || i >= nc) { std::printf("neighbour FAIL nc=%d c=%d j=%d i=%d\n", nc, c, j, i); g_fail = 1; continue; }
                if (seen[(size_t)i]++) { std::printf("neighbour FAIL nc=%d c=%d: cell %d twice\n", nc, c, i); g_fail = 1; }
                const int want = nc >= 5 ? ((c + j - 2) % nc + nc) % nc : j;
                if (i != want) { std::printf("neighbour FAIL nc=%d c=%d j=%d: %d, documented %d\n", nc, c, j, i, want); g_fail = 1; }
                ++n_nb;
            }
            for (int o = -GAMD_CELLS_REACH; o <= GAMD_CELLS_REACH; ++o)
                if (!seen[(size_t)(((c + o) % nc + nc) % nc)]) { std::printf("neighbour FAIL nc=%d c=%d: offset %d missing\n", nc, c, o); g_fail = 1; }
        }
    }
    std::printf("neighbour %s %ld\n", g_fail ? "FAIL" : "ok", n_nb);

    // ---- reach: two coordinates less than r_cut apart (minimum image, as the walk computes it) are two cells apart at the most ----
    std::mt19937_64 rng(20240917);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    long n_reach = 0;
    for (int t = 0; t < 200000; ++t) {
        const double rc = 3.0 + 7.0 * U(rng), L = 2.0 * rc + 40.0 * U(rng) * U(rng);
        const int nc = gamd_cells_per_axis(L, rc);
        const double xi = (U(rng) * 7.0 - 3.0) * L;
        // a partner at a distance just inside the cutoff, on either side, in any image
        const double frac = t % 3 == 0 ? 1.0 - 1e-15 : (t % 3 == 1 ? 1.0 - 1e-9 : U(rng));
        const double xj = xi + (t & 1 ? 1.0 : -1.0) * frac * rc + (double)((int)(U(rng) * 7.0) - 3) * L;
        double d = xi - xj;
        d = d - L * rint(d / L);
        if (!(d * d < rc * rc)) continue;
        const int ci = gamd_cells_index(xi, L, nc), cj = gamd_cells_index(xj, L, nc);
        int dc = ci > cj ? ci - cj : cj - ci;
        if (nc - dc < dc) dc = nc - dc;
        if (dc > GAMD_CELLS_REACH) { std::printf("reach FAIL L=%a rc=%a nc=%d xi=%a xj=%a cells %d %d\n", L, rc, nc, xi, xj, ci, cj); g_fail = 1; }
        ++n_reach;
    }
    std::printf("reach %s %ld\n", g_fail ? "FAIL" : "ok", n_reach);
    return g_fail;
}
