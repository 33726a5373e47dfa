#!/usr/bin/env python3
"""What the run recorder costs per MD step, and whether a build with it is as fast as one without when it is off.

    python tools/traj_cost.py [--parent-lib path/to/libgamd_hip.so of the commit before] [--steps 200] [--rounds 3]

On the C2 (10 000-atom LJ box, cutoff 10.2 A) and C1 (258-atom snapshot, cutoff 7.5 A) workloads of gamd_amd/workloads.py, in
skin mode as bench.py runs them, per-step device times come from gamd_timing_read_steps over warmed runs of --steps steps.
One process alternates the settings (recorder off; interval 100 and interval 1, both with fields x | v | f, 64 lags and a
frame buffer that holds every sample) --rounds times, every run on a fresh handle from the same start state (the recorder
does not change the trajectory, so all of them integrate the same steps), and prints the p50 and the mean of each.  The
interval-1 run fills the ring after 64 steps: the cost of a sampled step is the p50 of the steps behind that against the
p50 of the same steps of the off run.  Device bytes: what gamd_traj_configure allocates by the sizes documented in
include/gamd_hip.h, and the drop of free device memory across the call.

GAMD_LIB is read when gamd_amd._lib is imported, so every library runs in a child process of its own; with --parent-lib the
children are started alternately (parent, new, parent, new) and the recorder-off p50 of the new library is set against the
spread of the two parent runs.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_LAGS = 64
SETTINGS = [("off", 0), ("interval 100", 100), ("interval 1", 1)]


def _engine(workload, has_recorder):
    import numpy as np
    import torch
    from gamd_amd import _lib
    if not has_recorder:                       # a library of the commit before: bind what it exports
        for k in [k for k in _lib.SYMBOLS if k.startswith("gamd_traj_")]:
            del _lib.SYMBOLS[k]
    from gamd_amd.engine import GamdForce
    from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
    from gamd_amd import workloads as wk
    sd = make_state_dict(ModelConfig(kind="lj"), 0, 7.0, 2.2)
    if workload == "c2":
        n, rc = 10000, 3.0 * wk.LJ_SIGMA
        pos, box = wk.lj_box(n, seed=1234)
    else:
        n, rc, box = 258, 7.5, 27.27
        pos = np.mod(np.load(os.path.join(ROOT, "tests", "golden", "lj258_seed0.npz"))["pos"].astype(np.float64), box)
    eng = GamdForce(sd, n, box, rc, scaler=SHIPPED_SCALERS["lj"], neighbor_skin=rc / 6.0)
    x = torch.from_numpy(pos).float().cuda()
    v = torch.from_numpy(wk.maxwell_boltzmann(n, 100.0)).float().cuda()
    f = eng.forward(x, denormalize=True).clone()
    return eng, x, v, f, n


def worker(args):
    import numpy as np
    import torch
    has = not args.no_recorder
    out = {"lib": os.environ.get("GAMD_LIB", "default"), "label": args.label}
    for workload in ("c2", "c1"):
        res = {}
        for rnd in range(args.rounds):
            for slot, (name, interval) in enumerate(SETTINGS):
                eng, x, v, f, n = _engine(workload, has)
                eng.md_run(x, v, f, 50)                   # warm-up: allocations, first candidate build, clocks
                if has and interval:
                    frames = args.steps // interval
                    torch.cuda.synchronize()
                    free0 = torch.cuda.mem_get_info()[0]
                    eng.traj_configure(interval, max_frames=frames, fields=("x", "v", "f"), n_lags=N_LAGS)
                    free1 = torch.cuda.mem_get_info()[0]
                    blocks = max(1, min(16, (n + 1023) // 1024))
                    by_size = 24 * n + 8 + frames * (8 + 36 * n) + N_LAGS * 36 * n + 8 * N_LAGS * (2 * blocks + 2) + 8
                    out.setdefault(workload + "_bytes", {})[name] = {"by_size": by_size, "free_memory_drop": free0 - free1}
                elif not has and slot:
                    name = f"off #{slot + 1}"
                eng.timing_enable(True)
                eng.md_run(x, v, f, args.steps, first_step=50)
                ms = eng.timing_read_steps()
                eng.timing_enable(False)
                assert ms.shape[0] == args.steps
                if has and interval:
                    tr = eng.traj_read()
                    assert tr.n_samples == args.steps // interval and tr.dropped == 0 and tr.ambiguous == 0
                res.setdefault(name, []).append((float(np.percentile(ms, 50)), float(ms.mean()),
                                                 float(np.percentile(ms[N_LAGS:], 50))))
                out.setdefault(workload + "_edges", eng.counts()[0])
                eng.close()
        out[workload] = {k: {"p50_ms": [a for a, _, _ in val], "mean_ms": [b for _, b, _ in val],
                             "p50_full_ring_ms": [c for _, _, c in val]} for k, val in res.items()}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--no-recorder", action="store_true", help="the loaded library has no gamd_traj_* entry points")
    ap.add_argument("--label", default="new")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if args.steps < 200 or args.steps % 100:
        ap.error("--steps must be a multiple of 100, at least 200")
    order = [("parent", args.parent_lib), ("new", None)] * 2 if args.parent_lib else [("new", None)]
    results = []
    for label, lib in order:                   # one child per library, one at a time
        env = {k: v for k, v in os.environ.items() if k != "GAMD_LIB"}
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(args.steps), "--rounds", str(args.rounds),
               "--label", label]
        if lib:
            env["GAMD_LIB"] = os.path.abspath(lib)
            cmd.append("--no-recorder")
        p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
        if p.returncode != 0 or "RESULT " not in p.stdout:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"worker for the {label} library failed ({p.returncode})")
        results.append(json.loads(p.stdout.split("RESULT ", 1)[1].splitlines()[0]))
    med = lambda xs: sorted(xs)[len(xs) // 2]
    for workload in ("c2", "c1"):
        print(f"\n### {workload.upper()} ({results[-1][workload + '_edges']} directed edges), {args.steps} steps per run, {args.rounds} rounds\n")
        print("| process | setting | p50 ms/step per round | mean ms/step per round |")
        print("|---|---|---|---|")
        for r in results:
            for name, val in r[workload].items():
                print(f"| {r['label']} | {name} | {' '.join('%.4f' % a for a in val['p50_ms'])} | {' '.join('%.4f' % a for a in val['mean_ms'])} |")
        new = [r for r in results if r["label"] == "new"]
        off = med([a for r in new for a in r[workload]["off"]["p50_ms"]])
        d_mean = med([b - o for r in new for b, o in zip(r[workload]["interval 100"]["mean_ms"], r[workload]["off"]["mean_ms"])])
        on = med([a for r in new for a in r[workload]["interval 100"]["p50_ms"]])
        print(f"\ninterval 100: p50 {on:.4f} ms against {off:.4f} ms off ({1e3 * (on - off):+.1f} us); mean per step "
              f"{1e3 * d_mean:+.2f} us against off (median over rounds)")
        samp = med([a - o for r in new for a, o in zip(r[workload]["interval 1"]["p50_full_ring_ms"], r[workload]["off"]["p50_full_ring_ms"])])
        print(f"\na sampled step with the ring full ({N_LAGS} lags, frame of x | v | f): {1e3 * samp:+.1f} us (p50 of the steps behind "
              f"step {N_LAGS}, interval 1 against off, median over rounds)")
        for name, b in new[-1][workload + "_bytes"].items():
            print(f"\ndevice bytes, {name}: {b['by_size']} by the documented sizes, free device memory fell by {b['free_memory_drop']}")
        if args.parent_lib:
            pa, pb = [[a for k, val in r[workload].items() if k.startswith("off") for a in val["p50_ms"]]
                      for r in results if r["label"] == "parent"]
            spread = max(abs(a - b) for a, b in zip(pa, pb))
            par = med(pa + pb)
            print(f"\nrecorder off, new against parent (p50 ms/step): parent {par:.4f} (its two processes differ by up to "
                  f"{1e3 * spread:.2f} us on the same slot), new {off:.4f}; |new - parent| = {1e3 * abs(off - par):.2f} us "
                  f"-> {'within' if abs(off - par) <= spread else 'OUTSIDE'} the parent's own spread")


if __name__ == "__main__":
    main()
