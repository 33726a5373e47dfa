// gamd_minimize_host.h — the parameter block of gamd_minimize as the host takes it: the checks that need neither a handle nor
// a device, and the defaults a zero selects.  Plain C++ (no HIP header): tools/minimize_host_check.cpp builds it on its own
// under the host sanitizers.
#pragma once
#include "../../include/gamd_hip.h"

#include <cmath>
#include <cstdio>

// p as given -> *out with every zero replaced by its default.  0, or -22 with the reason in err (out is then left as it was).
inline int minimize_fill_params(const gamd_minimize_params* p, gamd_minimize_params* out, char* err, size_t err_len) {
    auto refuse = [&](const char* what, double v) { std::snprintf(err, err_len, "gamd_minimize: %s (%g)", what, v); return -22; };
    if (!p) { std::snprintf(err, err_len, "null argument"); return -22; }
    if (!(p->tolerance > 0.0) || !std::isfinite(p->tolerance)) return refuse("tolerance is not positive and finite", p->tolerance);
    if (p->max_iter < 0) return refuse("max_iter is negative", (double)p->max_iter);
    if (p->max_iter > (1ll << 30)) return refuse("max_iter exceeds 2^30", (double)p->max_iter);
    if (p->check_every < 0) return refuse("check_every is negative", (double)p->check_every);
    if (p->n_min < 0) return refuse("n_min is negative", (double)p->n_min);
    gamd_minimize_params q = *p;
    auto dflt = [](double& v, double d) { if (v == 0.0) v = d; };
    if (q.max_iter == 0) q.max_iter = 10000;
    if (q.check_every == 0) q.check_every = 64;
    if (q.n_min == 0) q.n_min = 5;
    dflt(q.dt_start, 0.002); dflt(q.dt_max, 0.02); dflt(q.f_inc, 1.1); dflt(q.f_dec, 0.5);
    dflt(q.alpha_start, 0.1); dflt(q.f_alpha, 0.99); dflt(q.max_step, 0.1);
    if (!(q.dt_start > 0.0) || !std::isfinite(q.dt_start)) return refuse("dt_start is not positive and finite", q.dt_start);
    if (!(q.dt_max >= q.dt_start) || !std::isfinite(q.dt_max)) return refuse("dt_max is below dt_start or not finite", q.dt_max);
    if (!(q.f_inc > 1.0) || !std::isfinite(q.f_inc)) return refuse("f_inc is not above 1 and finite", q.f_inc);
    if (!(q.f_dec > 0.0 && q.f_dec < 1.0)) return refuse("f_dec is outside (0, 1)", q.f_dec);
    if (!(q.alpha_start > 0.0 && q.alpha_start < 1.0)) return refuse("alpha_start is outside (0, 1)", q.alpha_start);
    if (!(q.f_alpha > 0.0 && q.f_alpha < 1.0)) return refuse("f_alpha is outside (0, 1)", q.f_alpha);
    if (!(q.max_step > 0.0) || !std::isfinite(q.max_step)) return refuse("max_step is not positive and finite", q.max_step);
    q.reserved = 0;
    *out = q;
    return 0;
}
