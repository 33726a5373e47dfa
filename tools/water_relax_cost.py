#!/usr/bin/env python3
"""What the water minimisers cost under the configured potential (gamd_water_minimize_potential, water_relax.hip) next to the
plain 3-site path of the same library: time per evaluation and whole calls, each form in a fresh process.

    python tools/water_relax_cost.py [--workloads w774 c3 big] [--forms plain pme cells msite msite+pme+cells]
                                     [--tolerances 10 1] [--r-switch 8.5] [--repeats 3] [--m 6] [--pme-tol 5e-4]

w774 is the 258-molecule lattice box (774 atoms), c3 the 1 390-molecule box of bench.py's C3 workload (4 170 atoms), big 17^3 =
4 913 molecules (14 739 atoms), all wl.water_box(jitter=0, wrap=False), seed 2345, r_cut 9.5 A, ewald_tol 1e-8: the boxes of
tools/water_lbfgs_cost.py and tools/water_pme_cost.py.  A form is a '+'-joined subset of msite (w = 0.106676721 on the default
charges), pme (order 6, the grid of pme_grid at --pme-tol) and cells; `plain` is none of them WITH THE SWITCH OFF: today's path.
Every form runs in a child process of its own (fresh handle, fresh allocator); every call is bracketed by HIP events on its
stream (it synchronises the stream itself: the bracket holds the enqueue, the device time and the host's looks at the states).
The first call of a kind (which allocates) is dropped and the median of --repeats further calls on the same start is printed.
  * per evaluation: two calls of K1 and K2 evaluations (tolerance 1e-300, check_every = K + 1); the slope is the time of one
    L-BFGS evaluation / FIRE iteration under the form, the intercept the fixed part of a call;
  * whole calls at --tolerances from the lattice start: tolerance >= 10 on the default (truncated) potential, lower ones with the
    Lennard-Jones term switched from --r-switch on (the truncated default stops in the line search below about 1).
A record, not a pass/fail bar."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_MOL = {"w774": 258, "c3": 1390, "big": 4913}
SLOPE_K = {"w774": (32, 160), "c3": (16, 80), "big": (8, 40)}
W = 0.106676721


def _child(workload, form, tolerances, r_switch, repeats, m, pme_tol):
    import numpy as np
    import torch
    from gamd_amd.engine import GamdForce, pme_grid
    from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
    from gamd_amd import workloads as wk
    sd = make_state_dict(ModelConfig(kind="water", use_bond=True, conv_layer=4), 3, 2.9, 1.1)
    pos, box, species, bonds = wk.water_box(N_MOL[workload], seed=2345, jitter=0.0, wrap=False)
    n = pos.shape[0]
    eng = GamdForce(sd, n, box, 4.2, bond=bonds, scaler=SHIPPED_SCALERS["tip3p"])
    parts = set() if form == "plain" else set(form.split("+"))
    alpha = float(np.sqrt(-np.log(1e-8))) / 9.5
    kw = dict(ewald_tol=1e-8, minimize_configured=bool(parts), cells="cells" in parts, m_site=W if "msite" in parts else 0.0)
    if "pme" in parts:
        kw.update(pme=pme_grid(alpha, box, pme_tol), pme_order=6)
    x0 = torch.from_numpy(pos).float().cuda()
    f = torch.zeros_like(x0)

    def timed(algo, tolerance, max_iter, check_every):
        call = ((lambda x: eng.water_minimize_lbfgs(x, species, f, tolerance=tolerance, max_iter=max_iter, check_every=check_every, m=m))
                if algo == "lbfgs" else (lambda x: eng.water_minimize(x, species, f, tolerance=tolerance, max_iter=max_iter, check_every=check_every)))
        ms, res = [], None
        for _ in range(1 + repeats):
            x = x0.clone()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = call(x)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        count = res.evaluations[0] if algo == "lbfgs" else res.iterations[0]
        return dict(first_ms=ms[0], warm_ms=float(np.median(ms[1:])), state=res.state[0], count=int(count), u=float(res.energy[0]), rms=float(res.rms[0]))

    out = dict(n=n, grid=list(kw["pme"]) if "pme" in kw else None, slopes={}, calls=[])
    eng.water_classical_configure(0, **kw)
    k1, k2 = SLOPE_K[workload]
    for algo in ("lbfgs", "fire"):
        a, b = timed(algo, 1e-300, k1, k1 + 1), timed(algo, 1e-300, k2, k2 + 1)
        assert a["count"] == k1 and b["count"] == k2
        s = (b["warm_ms"] - a["warm_ms"]) / (k2 - k1)
        out["slopes"][algo] = dict(us_per_evaluation=1e3 * s, fixed_ms=a["warm_ms"] - s * k1)
    for tol in tolerances:
        rs = 0.0 if tol >= 10.0 else r_switch
        eng.water_classical_configure(0, r_switch=rs, **kw)
        for algo in ("lbfgs", "fire"):
            out["calls"].append(dict(tolerance=tol, r_switch=rs, algo=algo, **timed(algo, tol, 0, 0)))
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def _measure(workload, form, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", workload, form, json.dumps(args.tolerances), repr(args.r_switch), str(args.repeats),
           str(args.m), repr(args.pme_tol)]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=900)
    if p.returncode != 0 or "RESULT" not in p.stdout:
        raise SystemExit(f"child failed ({p.returncode}): {p.stdout[-500:]} {p.stderr[-1500:]}")      # nothing more is started
    return json.loads(p.stdout.split("RESULT", 1)[1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        w, form, tols, rs, rep, m, pt = sys.argv[2:9]
        return _child(w, form, json.loads(tols), float(rs), int(rep), int(m), float(pt))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=["w774", "c3", "big"], choices=sorted(N_MOL))
    ap.add_argument("--forms", nargs="+", default=["plain", "pme", "cells", "msite", "msite+pme+cells"])
    ap.add_argument("--tolerances", nargs="*", type=float, default=[10.0, 1.0])
    ap.add_argument("--r-switch", type=float, default=8.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--m", type=int, default=6)
    ap.add_argument("--pme-tol", type=float, default=5e-4)
    args = ap.parse_args()
    out = {}
    for w in args.workloads:
        out[w] = {form: _measure(w, form, args) for form in args.forms}
        any_form = out[w][args.forms[0]]
        print(f"\n### {w.upper()} ({any_form['n']} atoms), m = {args.m}, slopes from {SLOPE_K[w][0]} / {SLOPE_K[w][1]} evaluations\n")
        print("| form | PME grid | L-BFGS us / evaluation | L-BFGS fixed ms | FIRE us / iteration | FIRE fixed ms |")
        print("|---|---|---|---|---|---|")
        for form, r in out[w].items():
            s = r["slopes"]
            print(f"| {form} | {r['grid'] or '-'} | {s['lbfgs']['us_per_evaluation']:.1f} | {s['lbfgs']['fixed_ms']:.3f} | "
                  f"{s['fire']['us_per_evaluation']:.1f} | {s['fire']['fixed_ms']:.3f} |")
        if args.tolerances:
            print("\n| form | tolerance kJ/mol/nm | r_switch | algorithm | state | count | U kJ/mol | rms kJ/mol/nm | first call ms | warm call ms |")
            print("|---|---|---|---|---|---|---|---|---|---|")
            for form, r in out[w].items():
                for c in r["calls"]:
                    print(f"| {form} | {c['tolerance']:g} | {c['r_switch']:g} | {c['algo']} | {c['state']} | {c['count']} | {c['u']:.4f} | {c['rms']:.3e} | "
                          f"{c['first_ms']:.2f} | {c['warm_ms']:.2f} |")
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
