// gamd_lbfgs_host.h — the parameter block of gamd_minimize_lbfgs and gamd_water_minimize_lbfgs as the host takes it: the checks
// that need neither a handle nor a device, and the defaults a zero selects.  Plain C++ (no HIP header), after gamd_minimize_host.h.
#pragma once
#include "../../include/gamd_hip.h"

#include <cmath>
#include <cstdio>

// p as given -> *out with every zero replaced by its default.  0, or -22 with the reason in err (out is then left as it was);
// `api` is the entry the message names.
inline int lbfgs_fill_params(const gamd_lbfgs_params* p, gamd_lbfgs_params* out, char* err, size_t err_len, const char* api = "gamd_minimize_lbfgs") {
    auto refuse = [&](const char* what, double v) { std::snprintf(err, err_len, "%s: %s (%g)", api, what, v); return -22; };
    if (!p) { std::snprintf(err, err_len, "null argument"); return -22; }
    if (!(p->tolerance > 0.0) || !std::isfinite(p->tolerance)) return refuse("tolerance is not positive and finite", p->tolerance);
    if (p->max_iter < 0) return refuse("max_iter is negative", (double)p->max_iter);
    if (p->max_iter > (1ll << 30)) return refuse("max_iter exceeds 2^30", (double)p->max_iter);
    if (p->check_every < 0) return refuse("check_every is negative", (double)p->check_every);
    if (p->m < 0 || p->m > 8) return refuse("m is outside [1, 8]", (double)p->m);
    if (p->max_ls < 0) return refuse("max_ls is negative", (double)p->max_ls);
    if (p->reserved != 0) return refuse("reserved is not 0", (double)p->reserved);
    gamd_lbfgs_params q = *p;
    auto dflt = [](double& v, double d) { if (v == 0.0) v = d; };
    if (q.max_iter == 0) q.max_iter = 10000;
    if (q.check_every == 0) q.check_every = 64;
    if (q.m == 0) q.m = 6;
    if (q.max_ls == 0) q.max_ls = 20;
    dflt(q.max_step, 0.1); dflt(q.c1, 1.0e-4); dflt(q.curv, 1.0e-10);
    if (!(q.max_step > 0.0) || !std::isfinite(q.max_step)) return refuse("max_step is not positive and finite", q.max_step);
    if (!(q.c1 > 0.0 && q.c1 < 1.0)) return refuse("c1 is outside (0, 1)", q.c1);
    if (!(q.curv > 0.0) || !std::isfinite(q.curv)) return refuse("curv is negative or not finite", q.curv);
    *out = q;
    return 0;
}
