#!/usr/bin/env python3
"""What a gamd_minimize call costs: time per iteration and whole calls, each figure from a fresh process.

    python tools/minimize_cost.py [--workloads c1 c2] [--tolerances 10 1 1e-6] [--repeats 3]

C1 is the 258-atom lj258_seed0 snapshot (uniform random points: one pair at 1.107 A), C2 the 10 000-atom lattice box of
bench.py's C2 workload (1e8 pair terms per iteration).  Every measurement runs in a child process of its own (fresh handle,
fresh allocator) and is bracketed by HIP events on the call's stream; the call synchronises the stream itself, so the bracket
holds the enqueue, the device time and the host's looks at the states.  Per measurement the first call of the process (which
allocates the work buffers) and the median of --repeats further calls on the same start are printed.
  * per iteration: two calls of K1 and K2 position updates (tolerance 1e-300, check_every = K: one look at the end); the slope
    (t(K2) - t(K1)) / (K2 - K1) is the time of one iteration (three launches), the intercept the fixed part of a call (init,
    the last evaluation, the store of x, the force source's two kernels, the copies);
  * whole calls at --tolerances with the default parameters: iterations, final U and rms, milliseconds.
A record, not a pass/fail bar."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOPE_K = {"c1": (64, 576), "c2": (8, 40)}


def _child(workload, tolerance, max_iter, check_every, repeats):
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
        n, rc, box = 258, 7.5, 27.27
        pos = np.mod(np.load(os.path.join(ROOT, "tests", "golden", "lj258_seed0.npz"))["pos"].astype(np.float64), box)
    eng = GamdForce(sd, n, box, rc, scaler=SHIPPED_SCALERS["lj"])
    eng.classical_configure(0)
    x0 = torch.from_numpy(pos).float().cuda()
    f = torch.zeros_like(x0)
    ms, res = [], None
    for _ in range(1 + repeats):
        x = x0.clone()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = eng.minimize(x, f, tolerance=tolerance, max_iter=max_iter, check_every=check_every)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    eng.close()
    print("RESULT " + json.dumps(dict(n=n, first_ms=ms[0], warm_ms=float(np.median(ms[1:])), state=res.state[0], iterations=int(res.iterations[0]),
                                      u0=float(res.energy_start[0]), rms0=float(res.rms_start[0]), u=float(res.energy[0]), rms=float(res.rms[0]),
                                      fmax=float(res.fmax[0]), dt=float(res.dt[0]))), flush=True)


def _measure(workload, tolerance, max_iter, check_every, repeats):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", workload, repr(tolerance), str(max_iter), str(check_every), str(repeats)]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=240)
    if p.returncode != 0 or "RESULT" not in p.stdout:
        raise SystemExit(f"child failed ({p.returncode}): {p.stdout[-500:]} {p.stderr[-1500:]}")      # nothing more is started
    return json.loads(p.stdout.split("RESULT", 1)[1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        w, tol, it, every, rep = sys.argv[2:7]
        return _child(w, float(tol), int(it), int(every), int(rep))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=["c1", "c2"], choices=["c1", "c2"])
    ap.add_argument("--tolerances", nargs="+", type=float, default=[10.0, 1.0, 1e-6])
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    out = {}
    for w in args.workloads:
        k1, k2 = SLOPE_K[w]
        a, b = (_measure(w, 1e-300, k, k, args.repeats) for k in (k1, k2))
        assert a["iterations"] == k1 and b["iterations"] == k2
        slope = (b["warm_ms"] - a["warm_ms"]) / (k2 - k1)
        fixed = a["warm_ms"] - slope * k1
        calls = [dict(tolerance=t, **_measure(w, t, 0, 0, args.repeats)) for t in args.tolerances]
        out[w] = dict(n=a["n"], k=[k1, k2], warm_ms=[a["warm_ms"], b["warm_ms"]], first_ms=[a["first_ms"], b["first_ms"]],
                      us_per_iteration=1e3 * slope, fixed_ms=fixed, calls=calls)
        print(f"\n### {w.upper()} ({a['n']} atoms)\n")
        print(f"{k1} / {k2} iterations in one chunk: {a['warm_ms']:.3f} / {b['warm_ms']:.3f} ms warm ({a['first_ms']:.3f} / {b['first_ms']:.3f} ms "
              f"first call) -> {1e3 * slope:.2f} us per iteration, {fixed:.3f} ms fixed per call\n")
        print("| tolerance kJ/mol/nm | state | iterations | U kJ/mol | rms kJ/mol/nm | max abs F | first call ms | warm call ms |")
        print("|---|---|---|---|---|---|---|---|")
        for c in calls:
            print(f"| {c['tolerance']:g} | {c['state']} | {c['iterations']} | {c['u']:.4f} | {c['rms']:.3e} | {c['fmax']:.3e} | {c['first_ms']:.2f} | {c['warm_ms']:.2f} |")
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
