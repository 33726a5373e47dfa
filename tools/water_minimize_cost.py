#!/usr/bin/env python3
"""What a gamd_water_minimize call costs: time per iteration and whole calls, each figure from a fresh process.

    python tools/water_minimize_cost.py [--workloads w774 c3] [--tolerances 10 1] [--repeats 3] [--ewald-tol 1e-8]

w774 is the 258-molecule lattice box (774 atoms, the reference generator's 2 nm box), c3 the 1 390-molecule box of bench.py's
C3 workload (4 170 atoms), both wl.water_box(jitter=0, wrap=False), seed 2345, at the potential's defaults (r_cut 9.5 A).  Every
measurement runs in a child process of its own (fresh handle, fresh allocator) and is bracketed by HIP events on the call's
stream; the call synchronises the stream itself, so the bracket holds the enqueue, the device time and the host's looks at the
states.  Per measurement the first call of the process (which allocates the work buffers) and the median of --repeats further
calls on the same start are printed.
  * per iteration: two calls of K1 and K2 position updates (tolerance 1e-300, check_every = K: one look at the end); the slope
    (t(K2) - t(K1)) / (K2 - K1) is the time of one iteration (six launches), the intercept the fixed part of a call (init, the
    last evaluation, the store of x, the force source's five kernels, the copies);
  * whole calls at --tolerances with the default parameters, from the lattice start: iterations, final U and rms, milliseconds.
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


def _child(workload, tolerance, max_iter, check_every, repeats, ewald_tol):
    import numpy as np
    import torch
    from gamd_amd.engine import GamdForce
    from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
    from gamd_amd import workloads as wk
    sd = make_state_dict(ModelConfig(kind="water", use_bond=True, conv_layer=4), 3, 2.9, 1.1)
    pos, box, species, bonds = wk.water_box(N_MOL[workload], seed=2345, jitter=0.0, wrap=False)
    n = pos.shape[0]
    eng = GamdForce(sd, n, box, 4.2, bond=bonds, scaler=SHIPPED_SCALERS["tip3p"])
    eng.water_classical_configure(0, ewald_tol=ewald_tol)
    x0 = torch.from_numpy(pos).float().cuda()
    f = torch.zeros_like(x0)
    ms, res = [], None
    for _ in range(1 + repeats):
        x = x0.clone()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = eng.water_minimize(x, species, f, tolerance=tolerance, max_iter=max_iter, check_every=check_every)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    eng.close()
    print("RESULT " + json.dumps(dict(n=n, first_ms=ms[0], warm_ms=float(np.median(ms[1:])), state=res.state[0], iterations=int(res.iterations[0]),
                                      u0=float(res.energy_start[0]), rms0=float(res.rms_start[0]), u=float(res.energy[0]), rms=float(res.rms[0]),
                                      fmax=float(res.fmax[0]), dt=float(res.dt[0]))), flush=True)


def _measure(workload, tolerance, max_iter, check_every, repeats, ewald_tol):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", workload, repr(tolerance), str(max_iter), str(check_every), str(repeats), repr(ewald_tol)]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=240)
    if p.returncode != 0 or "RESULT" not in p.stdout:
        raise SystemExit(f"child failed ({p.returncode}): {p.stdout[-500:]} {p.stderr[-1500:]}")      # nothing more is started
    return json.loads(p.stdout.split("RESULT", 1)[1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        w, tol, it, every, rep, et = sys.argv[2:8]
        return _child(w, float(tol), int(it), int(every), int(rep), float(et))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=["w774", "c3"], choices=sorted(N_MOL))
    ap.add_argument("--tolerances", nargs="+", type=float, default=[10.0, 1.0])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ewald-tol", type=float, default=1e-8)
    args = ap.parse_args()
    out = {}
    for w in args.workloads:
        k1, k2 = SLOPE_K[w]
        a, b = (_measure(w, 1e-300, k, k, args.repeats, args.ewald_tol) for k in (k1, k2))
        assert a["iterations"] == k1 and b["iterations"] == k2
        slope = (b["warm_ms"] - a["warm_ms"]) / (k2 - k1)
        fixed = a["warm_ms"] - slope * k1
        calls = [dict(tolerance=t, **_measure(w, t, 0, 0, args.repeats, args.ewald_tol)) for t in args.tolerances]
        out[w] = dict(n=a["n"], k=[k1, k2], warm_ms=[a["warm_ms"], b["warm_ms"]], first_ms=[a["first_ms"], b["first_ms"]],
                      us_per_iteration=1e3 * slope, fixed_ms=fixed, calls=calls)
        print(f"\n### {w.upper()} ({a['n']} atoms), ewald_tol {args.ewald_tol:g}\n")
        print(f"{k1} / {k2} iterations in one chunk: {a['warm_ms']:.3f} / {b['warm_ms']:.3f} ms warm ({a['first_ms']:.3f} / {b['first_ms']:.3f} ms "
              f"first call) -> {1e3 * slope:.2f} us per iteration, {fixed:.3f} ms fixed per call\n")
        print("| tolerance kJ/mol/nm | state | iterations | U kJ/mol | rms kJ/mol/nm | max abs F_c | first call ms | warm call ms |")
        print("|---|---|---|---|---|---|---|---|")
        for c in calls:
            print(f"| {c['tolerance']:g} | {c['state']} | {c['iterations']} | {c['u']:.4f} | {c['rms']:.3e} | {c['fmax']:.3e} | {c['first_ms']:.2f} | {c['warm_ms']:.2f} |")
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
