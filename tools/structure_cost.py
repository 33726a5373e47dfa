#!/usr/bin/env python3
"""What the structure sampler costs per MD step, and whether a build with it is as fast as one without when it is off.

    python tools/structure_cost.py [--parent-lib path/to/libgamd_hip.so of the commit before] [--steps 200] [--rounds 3]
                                   [--workloads c1 c2 c3]

On the C1 (258-atom LJ snapshot), C2 (10 000-atom LJ box: 5e7 pairs per sample) and C3 (1 390 rigid TIP3P molecules, three
pair classes) workloads, in skin mode as bench.py runs them, per-step device times come from gamd_timing_read_steps over
warmed runs of --steps steps.  One process alternates the settings (sampler off; interval 100 and interval 1, both with a
200-bin g(r) out to half the box and S(k) for |n|^2 <= 16; interval 1 with the histogram alone and with S(k) alone)
--rounds times, every run on a fresh handle from the same start state (the sampler does not change the trajectory, so all
of them integrate the same steps), and prints the p50 and the mean of each.  The added time of a sampled step is the p50 of
an interval-1 run against the p50 of the off run; the per-step average at interval 100 is the difference of the means.

GAMD_LIB is read when gamd_amd._lib is imported, so every library runs in a child process of its own; with --parent-lib the
children are started alternately (parent, new, parent, new) and the sampler-off p50 of the new library is set against the
spread of the two parent runs.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BINS, N2MAX = 200, 16
# name, interval, rdf_bins, sk_n2max
SETTINGS = [("off", 0, 0, 0), ("interval 100, g(r) + S(k)", 100, BINS, N2MAX), ("interval 1, g(r) + S(k)", 1, BINS, N2MAX),
            ("interval 1, g(r)", 1, BINS, 0), ("interval 1, S(k)", 1, 0, N2MAX)]


def _engine(workload, has_sampler):
    import numpy as np
    import torch
    from gamd_amd import _lib
    if not has_sampler:                        # a library of the commit before: bind what it exports
        for k in [k for k in _lib.SYMBOLS if k.startswith("gamd_struct_")]:
            del _lib.SYMBOLS[k]
    from gamd_amd.engine import GamdForce
    from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
    from gamd_amd import workloads as wk
    md = {}
    if workload == "c3":
        pos, box, species, bonds = wk.water_box(1390, mol_per_20A3=258.0, seed=2345, jitter=0.0, wrap=False)
        sd = make_state_dict(ModelConfig(kind="water", use_bond=True), 3, 2.9, 1.1)
        eng = GamdForce(sd, pos.shape[0], box, 4.2, bond=bonds, scaler=SHIPPED_SCALERS["tip3p"], neighbor_skin=4.2 / 6.0)
        mass = wk.MASS_O
        md = dict(mass_amu=wk.MASS_O, mass_h_amu=wk.MASS_H, rigid_water=True, r_oh=wk.TIP3P_R_OH, r_hh=wk.TIP3P_R_HH, species=species,
                  dt_ps=0.0005)
    else:
        sd = make_state_dict(ModelConfig(kind="lj"), 0, 7.0, 2.2)
        species, mass = None, 39.9
        if workload == "c2":
            n, rc = 10000, 3.0 * wk.LJ_SIGMA
            pos, box = wk.lj_box(n, seed=1234)
        else:
            n, rc, box = 258, 7.5, 27.27
            pos = np.mod(np.load(os.path.join(ROOT, "tests", "golden", "lj258_seed0.npz"))["pos"].astype(np.float64), box)
        eng = GamdForce(sd, n, box, rc, scaler=SHIPPED_SCALERS["lj"], neighbor_skin=rc / 6.0)
    x = torch.from_numpy(pos).float().cuda()
    v = torch.from_numpy(wk.maxwell_boltzmann(pos.shape[0], 100.0, mass_amu=mass)).float().cuda()
    f = eng.forward(x, species=species, denormalize=True).clone()
    return eng, x, v, f, md


def worker(args):
    import numpy as np
    has = not args.no_sampler
    out = {"lib": os.environ.get("GAMD_LIB", "default"), "label": args.label}
    for workload in args.workloads:
        res = {}
        for rnd in range(args.rounds):
            for slot, (name, interval, bins, n2max) in enumerate(SETTINGS):
                eng, x, v, f, md = _engine(workload, has)
                eng.md_run(x, v, f, 50, **md)             # warm-up: allocations, first candidate build, clocks
                if has:
                    eng.structure_configure(interval, rdf_bins=bins, sk_n2max=n2max)
                elif slot:
                    name = f"off #{slot + 1}"
                eng.timing_enable(True)
                eng.md_run(x, v, f, args.steps, first_step=50, **md)
                ms = eng.timing_read_steps()
                eng.timing_enable(False)
                assert ms.shape[0] == args.steps
                if has and interval:
                    st = eng.structure_read()
                    assert st.frames == args.steps // interval
                    if bins:
                        out[workload + "_pairs_per_sample"] = int(st.rdf_counts.sum()) // (2 * st.frames)
                res.setdefault(name, []).append((float(np.percentile(ms, 50)), float(ms.mean())))
                out.setdefault(workload + "_atoms", int(x.shape[0]))
                eng.close()
        out[workload] = {k: {"p50_ms": [a for a, _ in val], "mean_ms": [b for _, b in val]} for k, val in res.items()}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workloads", nargs="+", default=["c1", "c2", "c3"], choices=["c1", "c2", "c3"])
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--no-sampler", action="store_true", help="the loaded library has no gamd_struct_* entry points")
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
               "--label", label, "--workloads"] + args.workloads
        if lib:
            env["GAMD_LIB"] = os.path.abspath(lib)
            cmd.append("--no-sampler")
        p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
        if p.returncode != 0 or "RESULT " not in p.stdout:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"worker for the {label} library failed ({p.returncode})")
        results.append(json.loads(p.stdout.split("RESULT ", 1)[1].splitlines()[0]))
    med = lambda xs: sorted(xs)[len(xs) // 2]
    for workload in args.workloads:
        new = [r for r in results if r["label"] == "new"]
        print(f"\n### {workload.upper()} ({new[-1][workload + '_atoms']} atoms, {new[-1].get(workload + '_pairs_per_sample', 0)} pairs "
              f"below r_max per sample), {args.steps} steps per run, {args.rounds} rounds\n")
        print("| process | setting | p50 ms/step per round | mean ms/step per round |")
        print("|---|---|---|---|")
        for r in results:
            for name, val in r[workload].items():
                print(f"| {r['label']} | {name} | {' '.join('%.4f' % a for a in val['p50_ms'])} | {' '.join('%.4f' % a for a in val['mean_ms'])} |")
        off = med([a for r in new for a in r[workload]["off"]["p50_ms"]])
        for name, interval, _, _ in SETTINGS[1:]:
            on_p50 = med([a for r in new for a in r[workload][name]["p50_ms"]])
            d_mean = med([b - o for r in new for b, o in zip(r[workload][name]["mean_ms"], r[workload]["off"]["mean_ms"])])
            what = "a sampled step" if interval == 1 else "p50"
            print(f"\n{name}: {what} {on_p50:.4f} ms against {off:.4f} ms off ({1e3 * (on_p50 - off):+.1f} us); "
                  f"mean per step {1e3 * d_mean:+.2f} us against off (median over rounds)")
        if args.parent_lib:
            pa, pb = [[a for k, val in r[workload].items() if k.startswith("off") for a in val["p50_ms"]]
                      for r in results if r["label"] == "parent"]
            spread = max(abs(a - b) for a, b in zip(pa, pb))
            par = med(pa + pb)
            print(f"\nsampler off, new against parent (p50 ms/step): parent {par:.4f} (its two processes differ by up to "
                  f"{1e3 * spread:.2f} us on the same slot), new {off:.4f}; |new - parent| = {1e3 * abs(off - par):.2f} us "
                  f"-> {'within' if abs(off - par) <= spread else 'OUTSIDE'} the parent's own spread")


if __name__ == "__main__":
    main()
