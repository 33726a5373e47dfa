#!/usr/bin/env python3
"""What a sample of the water classical observer costs: the per-step device times of sampled and unsampled steps of ONE run on ONE handle.

    python tools/water_classical_cost.py [--steps 200] [--interval 10] [--rounds 3] [--ewald-tol 1e-10] [--workloads c3 w774] [--plain]
                                           [--m-site W] [--virial]

On the C3 workload (1 390 rigid TIP3P molecules = 4 170 atoms) and the 774-atom box (258 molecules), in skin mode as bench.py
runs the water workloads, per-step device times come from gamd_timing_read_steps over a warmed run of --steps steps with the
observer at --interval (default parameters: q_H 0.417, r_cut 9.5 A, alpha and k_cut from --ewald-tol).  A step's interval runs
from the event in front of its first kernel to the event in front of the next step's, so the sample enqueued behind a step's
second half (and, in skin mode, that second half launched on its own) falls into the sampled step's time.  Printed per workload
and round: p50 of the unsampled steps, p50 of the sampled steps, their difference (the cost of one sample), and the same run's
p50 with the observer off on the same handle; then the medians over the rounds.  A record, not a pass/fail bar.
--m-site W (TIP4P-Ew: 0.106676721) samples the 4-site form of the potential with the package's TIP4PEW parameters instead.
--virial adds a third run per round with the molecular virial log armed (gamd_water_virial) and prints what a sampled step costs
with it against without it.
--plain times the same runs without touching the observer's entry points at all: the tool then also runs in a checkout of a
commit that does not have them (copy it into that checkout's tools/), which is how the unsampled steps of an armed run are set
against the parent commit's library on one machine.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _engine(workload):
    import torch
    from gamd_amd.engine import GamdForce
    from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
    from gamd_amd import workloads as wk
    sd = make_state_dict(ModelConfig(kind="water", use_bond=True), 3, 2.9, 1.1)
    n_mol = 1390 if workload == "c3" else 258
    pos, box, species, bonds = wk.water_box(n_mol, seed=2345, jitter=0.0, wrap=False)
    eng = GamdForce(sd, pos.shape[0], box, 4.2, bond=bonds, scaler=SHIPPED_SCALERS["tip3p"], neighbor_skin=4.2 / 6.0)
    x = torch.from_numpy(pos).float().cuda()
    v = torch.from_numpy(wk.maxwell_boltzmann(pos.shape[0], 100.0, mass_amu=wk.MASS_O)).float().cuda()
    f = eng.forward(x, species=species, denormalize=True).clone()
    md = dict(dt_ps=0.0005, mass_amu=wk.MASS_O, mass_h_amu=wk.MASS_H, temperature_k=100.0, gamma_per_ps=25.0, seed=7, species=species,
              rigid_water=True, r_oh=wk.TIP3P_R_OH, r_hh=wk.TIP3P_R_HH)
    return eng, x, v, f, md


def main():
    import numpy as np
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--interval", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ewald-tol", type=float, default=1e-10)
    ap.add_argument("--workloads", nargs="+", default=["c3", "w774"], choices=["c3", "w774"])
    ap.add_argument("--m-site", type=float, default=0.0, help="the hydrogens' weight of the TIP4P M-site with the TIP4PEW parameters; 0: 3-site water")
    ap.add_argument("--virial", action="store_true", help="a third run per round with the molecular virial log armed")
    ap.add_argument("--plain", action="store_true", help="observer-off runs only, without calling the observer's entry points")
    args = ap.parse_args()
    if args.interval < 2 or args.steps % args.interval:
        ap.error("--steps must be a multiple of --interval, and --interval at least 2")
    out = {}
    pot = {}
    if args.m_site:
        from gamd_amd.engine import TIP4PEW
        pot = dict(TIP4PEW, m_site=args.m_site)
    for workload in args.workloads:
        eng, x, v, f, md = _engine(workload)
        eng.md_run(x, v, f, 50, **md)                             # warm-up: allocations, first candidate build, clocks
        done, rows = 50, []
        for rnd in range(args.rounds):
            res = {}
            modes = (("off", 0),) if args.plain else (("off", 0), ("on", args.interval)) + ((("vir", args.interval),) if args.virial else ())
            for name, interval in modes:
                if not args.plain:
                    eng.water_classical_configure(interval, ewald_tol=args.ewald_tol, **pot, **(dict(virial=True) if name == "vir" else {}))
                eng.timing_enable(True)
                eng.md_run(x, v, f, args.steps, first_step=done, **md)
                ms = eng.timing_read_steps()
                eng.timing_enable(False)
                done += args.steps
                assert ms.shape[0] == args.steps
                if name == "vir":
                    rd = eng.water_classical_read()
                    assert rd.steps.shape[0] == args.steps // interval and np.isfinite(rd.virial).all()
                    sampled = (np.arange(1, args.steps + 1) % interval) == 0
                    res["vir_unsampled_p50_ms"] = float(np.percentile(ms[~sampled], 50))
                    res["vir_sampled_p50_ms"] = float(np.percentile(ms[sampled], 50))
                    res["w_mol_last"] = float(rd.virial[-1, 0])
                elif interval:
                    rd = eng.water_classical_read()
                    assert rd.steps.shape[0] == args.steps // interval and (rd.sum_q == 0.0).all()
                    sampled = (np.arange(1, args.steps + 1) % interval) == 0      # the clock restarts at every configure
                    res["pairs_per_sample"] = float(rd.pairs[-1, 0])
                    res["energy_last"] = float(rd.energy[-1, 0])
                    res["unsampled_p50_ms"] = float(np.percentile(ms[~sampled], 50))
                    res["sampled_p50_ms"] = float(np.percentile(ms[sampled], 50))
                    res["mean_ms"] = float(ms.mean())
                else:
                    res["off_p50_ms"] = float(np.percentile(ms, 50))
                    res["off_mean_ms"] = float(ms.mean())
            rows.append(res)
        eng.close()
        out[workload] = rows
        if args.plain:
            print(f"{workload.upper()} ({x.shape[0]} atoms) plain runs, p50 ms/step per round: " + " ".join(f"{r['off_p50_ms']:.4f}" for r in rows))
            continue
        med = lambda key: float(np.median([r[key] for r in rows]))
        print(f"\n### {workload.upper()} ({x.shape[0]} atoms, {rows[-1]['pairs_per_sample']:.0f} pairs inside r_cut), {args.steps} steps per run, "
              f"interval {args.interval}, ewald_tol {args.ewald_tol:g}, {args.rounds} rounds\n")
        print("| round | off p50 ms | unsampled p50 ms | sampled p50 ms | one sample us | mean on - mean off us/step |")
        print("|---|---|---|---|---|---|")
        for k, r in enumerate(rows):
            print(f"| {k} | {r['off_p50_ms']:.4f} | {r['unsampled_p50_ms']:.4f} | {r['sampled_p50_ms']:.4f} | "
                  f"{1e3 * (r['sampled_p50_ms'] - r['unsampled_p50_ms']):.1f} | {1e3 * (r['mean_ms'] - r['off_mean_ms']):+.2f} |")
        print(f"\nmedian over rounds: a sampled step {med('sampled_p50_ms'):.4f} ms against {med('unsampled_p50_ms'):.4f} ms unsampled "
              f"({1e3 * (med('sampled_p50_ms') - med('unsampled_p50_ms')):+.1f} us per sample); observer off {med('off_p50_ms'):.4f} ms")
        if args.virial:
            print(f"virial log armed: a sampled step {med('vir_sampled_p50_ms'):.4f} ms ({1e3 * (med('vir_sampled_p50_ms') - med('sampled_p50_ms')):+.1f} us "
                  f"against the observer alone), unsampled {med('vir_unsampled_p50_ms'):.4f} ms; per round sampled: "
                  + " ".join(f"{r['vir_sampled_p50_ms']:.4f}" for r in rows) + ", unsampled: " + " ".join(f"{r['vir_unsampled_p50_ms']:.4f}" for r in rows))
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
