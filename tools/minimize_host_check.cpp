// minimize_host_check.cpp — the device-free part of gamd_minimize (gamd_amd/csrc/gamd_minimize_host.h: the checks of the
// parameter block and the defaults a zero selects) exercised as a stand-alone host program, meant to be built with the host
// sanitizers.  No HIP header, no HIP call.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/minimize_host_check.cpp -o /tmp/mhc && /tmp/mhc
#include "../gamd_amd/csrc/gamd_minimize_host.h"

#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static char err[512];

static gamd_minimize_params good() {
    gamd_minimize_params p;
    std::memset(&p, 0, sizeof(p));
    p.tolerance = 10.0;
    return p;
}

// refused with -22, the reason named, and the output block untouched
static void refused(const gamd_minimize_params& p, const char* word) {
    gamd_minimize_params out;
    std::memset(&out, 0x5a, sizeof(out));
    gamd_minimize_params mark = out;
    err[0] = 0;
    REQUIRE(minimize_fill_params(&p, &out, err, sizeof(err)) == -22);
    if (!std::strstr(err, word)) { std::fprintf(stderr, "expected \"%s\" in \"%s\"\n", word, err); std::exit(1); }
    REQUIRE(std::memcmp(&out, &mark, sizeof(out)) == 0);
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    gamd_minimize_params out;

    // a zero selects the default, everything given stays
    gamd_minimize_params p = good();
    REQUIRE(minimize_fill_params(&p, &out, err, sizeof(err)) == 0);
    REQUIRE(out.tolerance == 10.0 && out.max_iter == 10000 && out.check_every == 64 && out.n_min == 5 && out.reserved == 0);
    REQUIRE(out.dt_start == 0.002 && out.dt_max == 0.02 && out.f_inc == 1.1 && out.f_dec == 0.5);
    REQUIRE(out.alpha_start == 0.1 && out.f_alpha == 0.99 && out.max_step == 0.1);
    p.max_iter = 7; p.check_every = 1000; p.n_min = 3; p.dt_start = 0.001; p.dt_max = 0.001; p.f_inc = 1.5; p.f_dec = 0.25;
    p.alpha_start = 0.2; p.f_alpha = 0.9; p.max_step = 0.05; p.tolerance = 1e-6; p.reserved = 77;
    REQUIRE(minimize_fill_params(&p, &out, err, sizeof(err)) == 0);
    REQUIRE(out.tolerance == 1e-6 && out.max_iter == 7 && out.check_every == 1000 && out.n_min == 3 && out.reserved == 0);
    REQUIRE(out.dt_start == 0.001 && out.dt_max == 0.001 && out.f_inc == 1.5 && out.f_dec == 0.25);
    REQUIRE(out.alpha_start == 0.2 && out.f_alpha == 0.9 && out.max_step == 0.05);
    REQUIRE(minimize_fill_params(&p, &p, err, sizeof(err)) == 0 && p.reserved == 0);      // in place

    // the refusals of include/gamd_hip.h, by name
    REQUIRE(minimize_fill_params(nullptr, &out, err, sizeof(err)) == -22 && std::strstr(err, "null argument"));
    for (double t : {0.0, -1.0, inf, nan}) { p = good(); p.tolerance = t; refused(p, "tolerance"); }
    p = good(); p.max_iter = -1; refused(p, "max_iter");
    p = good(); p.max_iter = (1ll << 30) + 1; refused(p, "max_iter");
    p = good(); p.check_every = -64; refused(p, "check_every");
    p = good(); p.n_min = -1; refused(p, "n_min");
    for (double v : {-0.002, inf, nan}) { p = good(); p.dt_start = v; refused(p, "dt_start"); }
    p = good(); p.dt_start = 0.05; refused(p, "dt_max");                                   // above the default dt_max
    p = good(); p.dt_max = 0.001; refused(p, "dt_max");                                    // below the default dt_start
    for (double v : {inf, nan}) { p = good(); p.dt_max = v; refused(p, "dt_max"); }
    for (double v : {1.0, 0.9, -1.1, inf, nan}) { p = good(); p.f_inc = v; refused(p, "f_inc"); }
    for (double v : {1.0, 1.5, -0.5, nan}) { p = good(); p.f_dec = v; refused(p, "f_dec"); }
    for (double v : {1.0, 2.0, -0.1, nan}) { p = good(); p.alpha_start = v; refused(p, "alpha_start"); }
    for (double v : {1.0, 1.01, -0.99, nan}) { p = good(); p.f_alpha = v; refused(p, "f_alpha"); }
    for (double v : {-0.1, inf, nan}) { p = good(); p.max_step = v; refused(p, "max_step"); }

    // a short error buffer is not overrun
    char tiny[8];
    p = good(); p.tolerance = -1.0;
    REQUIRE(minimize_fill_params(&p, &out, tiny, sizeof(tiny)) == -22 && std::strlen(tiny) == sizeof(tiny) - 1);
    std::printf("minimize_host_check: ok\n");
    return 0;
}
