#!/usr/bin/env python3
"""What a gamd_water_minimize_lbfgs call costs next to gamd_water_minimize (FIRE) on the same handle: time per evaluation and
whole calls, each figure from a fresh process.

    python tools/water_lbfgs_cost.py [--workloads w774 c3] [--tolerances 10 1] [--tight 1e-3] [--r-switch 8.5] [--repeats 3] [--m 6]

w774 is the 258-molecule lattice box (774 atoms), c3 the 1 390-molecule box of bench.py's C3 workload (4 170 atoms), both
wl.water_box(jitter=0, wrap=False), seed 2345, at the potential's defaults (r_cut 9.5 A, ewald_tol 1e-8): the boxes of
tools/water_minimize_cost.py.  Every measurement runs in a child process of its own (fresh handle, fresh allocator) and is
bracketed by HIP events on the call's stream; the call synchronises the stream itself, so the bracket holds the enqueue, the
device time and the host's looks at the states.  Per measurement the first call of the process (which allocates the work
buffers) and the median of --repeats further calls on the same start are printed.
  * per evaluation: two L-BFGS calls of K1 and K2 evaluations (tolerance 1e-300, check_every = K + 1: one look at the end); the
    slope (t(K2) - t(K1)) / (K2 - K1) is the time of one evaluation (six launches), the intercept the fixed part of a call; the
    same for FIRE's iterations (six launches);
  * whole calls at --tolerances with the default parameters on the default (truncated) potential, L-BFGS and FIRE one after the
    other on one handle: state, evaluations (FIRE: iterations), final U and rms, milliseconds;
  * one whole call at --tight with the Lennard-Jones term switched from --r-switch on (the default potential's jump at r_cut
    stops the line search below a tolerance of about 1), L-BFGS and FIRE alike.
A record, not a pass/fail bar."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_MOL = {"w774": 258, "c3": 1390}
SLOPE_K = {"w774": (32, 288), "c3": (16, 80)}


def _child(workload, tolerance, max_iter, check_every, repeats, m, r_switch):
    import numpy as np
    import torch
    from gamd_amd.engine import GamdForce
    from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
    from gamd_amd import workloads as wk
    sd = make_state_dict(ModelConfig(kind="water", use_bond=True, conv_layer=4), 3, 2.9, 1.1)
    pos, box, species, bonds = wk.water_box(N_MOL[workload], seed=2345, jitter=0.0, wrap=False)
    n = pos.shape[0]
    eng = GamdForce(sd, n, box, 4.2, bond=bonds, scaler=SHIPPED_SCALERS["tip3p"])
    eng.water_classical_configure(0, ewald_tol=1e-8, r_switch=r_switch)
    x0 = torch.from_numpy(pos).float().cuda()
    f = torch.zeros_like(x0)
    out = {}
    calls = {"lbfgs": lambda x: eng.water_minimize_lbfgs(x, species, f, tolerance=tolerance, max_iter=max_iter, check_every=check_every, m=m),
             "fire": lambda x: eng.water_minimize(x, species, f, tolerance=tolerance, max_iter=max_iter, check_every=check_every)}
    for name, call in calls.items():
        ms, res = [], None
        for _ in range(1 + repeats):
            x = x0.clone()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = call(x)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        count = res.evaluations[0] if name == "lbfgs" else res.iterations[0]
        out[name] = dict(first_ms=ms[0], warm_ms=float(np.median(ms[1:])), state=res.state[0], count=int(count), u0=float(res.energy_start[0]),
                         rms0=float(res.rms_start[0]), u=float(res.energy[0]), rms=float(res.rms[0]), fmax=float(res.fmax[0]))
        if name == "lbfgs":
            out[name].update(accepted=int(res.accepted[0]), skipped=int(res.skipped[0]), resets=int(res.resets[0]))
    eng.close()
    print("RESULT " + json.dumps(dict(n=n, **out)), flush=True)


def _measure(workload, tolerance, max_iter, check_every, repeats, m, r_switch=0.0):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", workload, repr(tolerance), str(max_iter), str(check_every), str(repeats), str(m),
           repr(r_switch)]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=400)
    if p.returncode != 0 or "RESULT" not in p.stdout:
        raise SystemExit(f"child failed ({p.returncode}): {p.stdout[-500:]} {p.stderr[-1500:]}")      # nothing more is started
    return json.loads(p.stdout.split("RESULT", 1)[1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        w, tol, it, every, rep, m, rs = sys.argv[2:9]
        return _child(w, float(tol), int(it), int(every), int(rep), int(m), float(rs))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=["w774", "c3"], choices=sorted(N_MOL))
    ap.add_argument("--tolerances", nargs="+", type=float, default=[10.0, 1.0])
    ap.add_argument("--tight", type=float, default=1e-3, help="one tolerance with the switched potential; 0: none")
    ap.add_argument("--r-switch", type=float, default=8.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--m", type=int, default=6)
    args = ap.parse_args()
    out = {}
    for w in args.workloads:
        k1, k2 = SLOPE_K[w]
        a, b = (_measure(w, 1e-300, k, k + 1, args.repeats, args.m) for k in (k1, k2))
        slopes = {}
        for algo in ("lbfgs", "fire"):
            assert a[algo]["count"] == k1 and b[algo]["count"] == k2
            s = (b[algo]["warm_ms"] - a[algo]["warm_ms"]) / (k2 - k1)
            slopes[algo] = dict(us_per_evaluation=1e3 * s, fixed_ms=a[algo]["warm_ms"] - s * k1)
        calls = [dict(tolerance=t, r_switch=0.0, **_measure(w, t, 0, 0, args.repeats, args.m)) for t in args.tolerances]
        if args.tight:
            calls.append(dict(tolerance=args.tight, r_switch=args.r_switch, **_measure(w, args.tight, 0, 0, args.repeats, args.m, args.r_switch)))
        out[w] = dict(n=a["n"], k=[k1, k2], slopes=slopes, calls=calls)
        print(f"\n### {w.upper()} ({a['n']} atoms), m = {args.m}\n")
        for algo in ("lbfgs", "fire"):
            print(f"{algo}: {k1} / {k2} evaluations in one chunk: {a[algo]['warm_ms']:.3f} / {b[algo]['warm_ms']:.3f} ms warm -> "
                  f"{slopes[algo]['us_per_evaluation']:.2f} us per evaluation, {slopes[algo]['fixed_ms']:.3f} ms fixed per call")
        print("\n| tolerance kJ/mol/nm | r_switch | algorithm | state | evaluations | accepted / resets | U kJ/mol | rms kJ/mol/nm | first call ms | warm call ms |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        for c in calls:
            for algo in ("lbfgs", "fire"):
                r = c[algo]
                extra = f"{r['accepted']} / {r['resets']}" if algo == "lbfgs" else "-"
                print(f"| {c['tolerance']:g} | {c['r_switch']:g} | {algo} | {r['state']} | {r['count']} | {extra} | {r['u']:.4f} | {r['rms']:.3e} | "
                      f"{r['first_ms']:.2f} | {r['warm_ms']:.2f} |")
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
