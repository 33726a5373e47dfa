#!/usr/bin/env python3
"""What a gamd_minimize_lbfgs call costs next to gamd_minimize (FIRE) on the same handle: time per evaluation and whole calls,
each figure from a fresh process.

    python tools/lbfgs_cost.py [--workloads c1 c2] [--tolerances 1 1e-6] [--cells 0 1] [--repeats 3] [--m 6]

C1 is the 258-atom lattice box of workloads.lj_box(258), C2 the 10 000-atom lattice box of bench.py's C2 workload (1e8 pair
terms per all-pairs evaluation).  --cells 1 switches the cell table on (classical_configure(cells=True)).  Every measurement
runs in a child process of its own (fresh handle, fresh allocator) and is bracketed by HIP events on the call's stream; the call
synchronises the stream itself, so the bracket holds the enqueue, the device time and the host's looks at the states.  Per
measurement the first call of the process (which allocates the work buffers) and the median of --repeats further calls on the
same start are printed.
  * per evaluation: two L-BFGS calls of K1 and K2 evaluations (tolerance 1e-300, check_every = K + 1: one look at the end); the
    slope (t(K2) - t(K1)) / (K2 - K1) is the time of one evaluation (three launches, nine with the cells), the intercept the
    fixed part of a call; the same for FIRE's iterations;
  * whole calls at --tolerances with the default parameters, L-BFGS and FIRE one after the other on one handle: state,
    evaluations (FIRE: iterations), final U and rms, milliseconds.
A record, not a pass/fail bar."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOPE_K = {"c1": (64, 576), "c2": (8, 40)}


def _child(workload, cells, tolerance, max_iter, check_every, repeats, m):
    import numpy as np
    import torch
    from gamd_amd.engine import GamdForce
    from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
    from gamd_amd import workloads as wk
    sd = make_state_dict(ModelConfig(kind="lj", conv_layer=2), 0, 7.0, 2.2)
    if workload == "c2":
        n, rc = 10000, 3.0 * wk.LJ_SIGMA
        pos, box = wk.lj_box(n, seed=1234)
    else:
        n, rc = 258, 7.5
        pos, box = wk.lj_box(n)
    eng = GamdForce(sd, n, box, rc, scaler=SHIPPED_SCALERS["lj"])
    eng.classical_configure(0, cells=bool(cells))
    x0 = torch.from_numpy(np.asarray(pos)).float().cuda()
    f = torch.zeros_like(x0)
    out = {}
    calls = {"lbfgs": lambda x: eng.minimize_lbfgs(x, f, tolerance=tolerance, max_iter=max_iter, check_every=check_every, m=m),
             "fire": lambda x: eng.minimize(x, f, tolerance=tolerance, max_iter=max_iter, check_every=check_every)}
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


def _measure(workload, cells, tolerance, max_iter, check_every, repeats, m):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", workload, str(cells), repr(tolerance), str(max_iter), str(check_every),
           str(repeats), str(m)]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=400)
    if p.returncode != 0 or "RESULT" not in p.stdout:
        raise SystemExit(f"child failed ({p.returncode}): {p.stdout[-500:]} {p.stderr[-1500:]}")      # nothing more is started
    return json.loads(p.stdout.split("RESULT", 1)[1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        w, cells, tol, it, every, rep, m = sys.argv[2:9]
        return _child(w, int(cells), float(tol), int(it), int(every), int(rep), int(m))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=["c1", "c2"], choices=["c1", "c2"])
    ap.add_argument("--tolerances", nargs="+", type=float, default=[1.0, 1e-6])
    ap.add_argument("--cells", nargs="+", type=int, default=[0, 1], choices=[0, 1])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--m", type=int, default=6)
    args = ap.parse_args()
    out = {}
    for w in args.workloads:
        for cells in args.cells:
            k1, k2 = SLOPE_K[w]
            a, b = (_measure(w, cells, 1e-300, k, k + 1, args.repeats, args.m) for k in (k1, k2))
            slopes = {}
            for algo in ("lbfgs", "fire"):
                assert a[algo]["count"] == k1 and b[algo]["count"] == k2
                s = (b[algo]["warm_ms"] - a[algo]["warm_ms"]) / (k2 - k1)
                slopes[algo] = dict(us_per_evaluation=1e3 * s, fixed_ms=a[algo]["warm_ms"] - s * k1)
            calls = [dict(tolerance=t, **_measure(w, cells, t, 0, 0, args.repeats, args.m)) for t in args.tolerances]
            out[f"{w}_cells{cells}"] = dict(n=a["n"], k=[k1, k2], slopes=slopes, calls=calls)
            print(f"\n### {w.upper()} ({a['n']} atoms), cells {'on' if cells else 'off'}, m = {args.m}\n")
            for algo in ("lbfgs", "fire"):
                print(f"{algo}: {k1} / {k2} evaluations in one chunk: {a[algo]['warm_ms']:.3f} / {b[algo]['warm_ms']:.3f} ms warm -> "
                      f"{slopes[algo]['us_per_evaluation']:.2f} us per evaluation, {slopes[algo]['fixed_ms']:.3f} ms fixed per call")
            print("\n| tolerance kJ/mol/nm | algorithm | state | evaluations | U kJ/mol | rms kJ/mol/nm | first call ms | warm call ms |")
            print("|---|---|---|---|---|---|---|---|")
            for c in calls:
                for algo in ("lbfgs", "fire"):
                    r = c[algo]
                    print(f"| {c['tolerance']:g} | {algo} | {r['state']} | {r['count']} | {r['u']:.4f} | {r['rms']:.3e} | {r['first_ms']:.2f} | {r['warm_ms']:.2f} |")
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
