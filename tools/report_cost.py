#!/usr/bin/env python3
"""What the run reporter costs per MD step, and whether a build with it is as fast as one without when it is off.

    python tools/report_cost.py [--parent-lib path/to/libgamd_hip.so of the commit before] [--steps 200] [--rounds 3]

On the C2 (10 000-atom LJ box, cutoff 10.2 A) and C1 (258-atom snapshot, cutoff 7.5 A) workloads of gamd_amd/workloads.py, in
skin mode as bench.py runs them, per-step device times come from gamd_timing_read_steps over warmed runs of --steps steps.
One process alternates the settings (reporter off, interval 100 with KE + 100-bin g(r), interval 1 with KE only, interval 1
with KE + 100-bin g(r)) --rounds times, every run on a fresh handle from the same start state (the reporter does not change
the trajectory, so all of them integrate the same steps), and prints the p50 and the mean of each.

GAMD_LIB is read when gamd_amd._lib is imported, so every library runs in a child process of its own; with --parent-lib the
children are started alternately (parent, new, parent, new) and the reporter-off p50 of the new library is set against the
spread of the two parent runs.

    --trace N    (worker mode for a kernel trace) run N steps of C2 with the given --interval / --bins and exit; used as
                 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/report_cost.py --trace 10 ...
    --compare-traces DIR_ON DIR_PARENT_OFF DIR_NEW_OFF
                 read three such trace directories: the reporter kernels' own times from the first, and whether the two
                 reporter-off runs launched the same kernels in the same order
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = [("off", 0, 0), ("interval 100, KE + g(r)", 100, 100), ("interval 1, KE", 1, 0), ("interval 1, KE + g(r)", 1, 100)]


def _engine(workload, has_reporter):
    import numpy as np
    import torch
    from gamd_amd import _lib
    if not has_reporter:                       # a library of the commit before: bind what it exports
        for k in [k for k in _lib.SYMBOLS if k.startswith("gamd_report_")]:
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
    return eng, x, v, f


def worker(args):
    import numpy as np
    has = not args.no_reporter
    out = {"lib": os.environ.get("GAMD_LIB", "default"), "label": args.label}
    for workload in ("c2", "c1"):
        res = {}
        for rnd in range(args.rounds):
            # a fresh handle and the same start state for every setting: the reporter does not change the trajectory, so
            # every timed run integrates the same 200 steps with the same handle history (rebuild steps included).  A library
            # without the reporter runs the same schedule with nothing configured (slots "off", "off #2", ...)
            for slot, (name, interval, bins) in enumerate(SETTINGS):
                eng, x, v, f = _engine(workload, has)
                eng.md_run(x, v, f, 50)                   # warm-up: allocations, first candidate build, clocks
                if has:
                    eng.report_configure(interval, rdf_bins=bins, max_samples=max(1, args.steps))
                elif slot:
                    name = f"off #{slot + 1}"
                eng.timing_enable(True)
                eng.md_run(x, v, f, args.steps, first_step=50)
                ms = eng.timing_read_steps()
                eng.timing_enable(False)
                assert ms.shape[0] == args.steps
                res.setdefault(name, []).append((float(np.percentile(ms, 50)), float(ms.mean())))
                out.setdefault(workload + "_edges", eng.counts()[0])
                eng.close()
        out[workload] = {k: {"p50_ms": [a for a, _ in val], "mean_ms": [b for _, b in val]} for k, val in res.items()}
    print("RESULT " + json.dumps(out), flush=True)


def trace(args):
    eng, x, v, f = _engine("c2", not args.no_reporter)
    eng.md_run(x, v, f, 5)
    if not args.no_reporter:
        eng.report_configure(args.interval, rdf_bins=args.bins)
    eng.md_run(x, v, f, args.trace, first_step=5)
    eng.close()


def compare_traces(dirs):
    import csv
    import glob
    import re
    import statistics

    def load(d):
        rows = []
        for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(p) as fh:
                rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
        return sorted(rows)
    on, parent_off, new_off = (load(d) for d in dirs)
    names_p, names_n = [r[2] for r in parent_off], [r[2] for r in new_off]
    print(f"reporter off: parent {len(names_p)} kernel launches, new {len(names_n)}; identical name sequences: {names_p == names_n}")
    for i, (a, b) in enumerate(zip(names_p, names_n)):
        if a != b:
            print(f"first difference at launch {i}: {a} | {b}")
            break
    print("reporter kernels in the reporter-off trace of the new library:", sum("k_report" in n for n in names_n))
    per = {}
    for s, e, n in on:
        m = re.search(r"k_report_\w+", n)
        if m:
            per.setdefault(m.group(0), []).append((e - s) / 1e3)
    for n, v in sorted(per.items()):
        print(f"{n}: {len(v)} launches, median {statistics.median(v):.2f} us, mean {statistics.mean(v):.2f} us, max {max(v):.2f} us")
    print(f"all kernels of the reporter-on run: {sum(e - s for s, e, _ in on) / 1e3:.0f} us in {len(on)} launches")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--no-reporter", action="store_true", help="the loaded library has no gamd_report_* entry points")
    ap.add_argument("--label", default="new")
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--interval", type=int, default=0)
    ap.add_argument("--bins", type=int, default=0)
    ap.add_argument("--compare-traces", nargs=3, metavar="DIR", default=None)
    args = ap.parse_args()
    if args.compare_traces:
        return compare_traces(args.compare_traces)
    if args.trace:
        return trace(args)
    if args.worker:
        return worker(args)
    if args.steps < 200:
        ap.error("--steps must be at least 200")
    order = [("parent", args.parent_lib), ("new", None)] * 2 if args.parent_lib else [("new", None)]
    results = []
    for label, lib in order:                   # one child per library, one at a time
        env = {k: v for k, v in os.environ.items() if k != "GAMD_LIB"}
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(args.steps), "--rounds", str(args.rounds),
               "--label", label]
        if lib:
            env["GAMD_LIB"] = os.path.abspath(lib)
            cmd.append("--no-reporter")
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
        for name, _, _ in SETTINGS[1:]:
            on_p50 = med([a for r in new for a in r[workload][name]["p50_ms"]])
            d_mean = med([b - o for r in new for b, o in zip(r[workload][name]["mean_ms"], r[workload]["off"]["mean_ms"])])
            print(f"\n{name}: p50 {on_p50:.4f} ms against {off:.4f} ms off ({1e3 * (on_p50 - off):+.1f} us); "
                  f"mean per step {1e3 * d_mean:+.2f} us against off (median over rounds)")
        if args.parent_lib:
            # every "off" slot of a parent process against the same slot of the other parent process: what two runs of one
            # library differ by; then all off slots of the new library against all of the parent's
            pa, pb = [[a for k, val in r[workload].items() if k.startswith("off") for a in val["p50_ms"]]
                      for r in results if r["label"] == "parent"]
            spread = max(abs(a - b) for a, b in zip(pa, pb))
            par = med(pa + pb)
            nw = med([a for r in new for a in r[workload]["off"]["p50_ms"]])
            print(f"\nreporter off, new against parent (p50 ms/step): parent {par:.4f} (its two processes differ by up to "
                  f"{1e3 * spread:.2f} us on the same slot), new {nw:.4f}; |new - parent| = {1e3 * abs(nw - par):.2f} us "
                  f"-> {'within' if abs(nw - par) <= spread else 'OUTSIDE'} the parent's own spread")

if __name__ == "__main__":
    main()
