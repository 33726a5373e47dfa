#!/usr/bin/env python3
"""What particle-mesh Ewald costs against the plain sum of the water classical potential, on ONE handle per process.

    python tools/water_pme_cost.py --workload {w774,c3,big} [--steps 100] [--interval 10] [--rounds 3] [--ewald-tol 1e-8]
                                   [--grid-tol 5e-4] [--order 6] [--drift]

Workloads: w774 (258 rigid TIP3P molecules), c3 (1 390 molecules = 4 170 atoms) and big (17^3 = 4 913 molecules = 14 739
atoms, the next lattice size of gamd_amd.workloads above 14 000 atoms), r_cut 9.5 A, alpha from --ewald-tol, in skin mode as
bench.py runs the water workloads.  Per-step device times are gamd_timing_read_steps' (HIP events around every step).  Per
round the modes are alternated on the same box and handle — the plain sum (skipped, with the library's message, where it is
refused), PME of --order on the grid pme_grid(alpha, box, --grid-tol) proposes, and on the grid one step finer per axis (capped
at 128) — and for each:
  sampled   a network-driven Langevin run with the observer at --interval: p50 of the sampled steps minus p50 of the
            unsampled ones = the cost of one sample;
  driven    a Nose-Hoover-chain run with the water classical force source: p50 of a step.
--drift adds, per mode, a gamma = 0 rigid water-source run of 1 ps (2 000 steps of 0.5 fs) from a start minimised under the
plain sum with 300 K velocities: E_tot = KE (reporter) + PE (observer) every 20 steps, its largest deviation from the first
sample and a least-squares slope.  A record, not a pass/fail bar.  Run one workload per process."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_MOL = {"w774": 258, "c3": 1390, "big": 4913}


def main():
    import numpy as np
    import torch
    from gamd_amd.engine import GamdForce, pme_grid
    from gamd_amd._lib import GamdError
    from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
    from gamd_amd import workloads as wk
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="w774", choices=sorted(N_MOL))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--interval", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ewald-tol", type=float, default=1e-8)
    ap.add_argument("--grid-tol", type=float, default=5e-4, help="the tolerance pme_grid's spacing rule is given")
    ap.add_argument("--order", type=int, default=6)
    ap.add_argument("--drift", action="store_true")
    args = ap.parse_args()
    if args.interval < 2 or args.steps % args.interval:
        ap.error("--steps must be a multiple of --interval, and --interval at least 2")

    sd = make_state_dict(ModelConfig(kind="water", use_bond=True), 3, 2.9, 1.1)
    pos, box, species, bonds = wk.water_box(N_MOL[args.workload], seed=2345, jitter=0.0, wrap=False)
    eng = GamdForce(sd, pos.shape[0], box, 4.2, bond=bonds, scaler=SHIPPED_SCALERS["tip3p"], neighbor_skin=4.2 / 6.0)
    n = pos.shape[0]
    md = dict(dt_ps=0.0005, mass_amu=wk.MASS_O, mass_h_amu=wk.MASS_H, species=species, rigid_water=True, r_oh=wk.TIP3P_R_OH, r_hh=wk.TIP3P_R_HH)
    alpha = float(np.sqrt(-np.log(args.ewald_tol))) / 9.5
    grid = pme_grid(alpha, box, args.grid_tol, args.order)
    fine = tuple(min(128, 2 * g) for g in grid)
    modes = [("plain", None), ("pme", grid)] + ([("pme_fine", fine)] if fine != grid else [])
    print(f"{args.workload}: {n} atoms, box {box:.3f} A, alpha {alpha:.4f} / A, grid {grid} (spacing {box / grid[0]:.3f} A), finer {fine}; "
          f"launches per sample: plain 6, PME 13 (pairs; clear, spread, 3 line passes, convolution, 3 line passes, gather; atoms, final)")

    def conf(interval, pme):
        eng.water_classical_configure(interval, ewald_tol=args.ewald_tol, pme=pme, pme_order=args.order)

    def fresh():
        x = torch.from_numpy(pos).float().cuda()
        v = torch.from_numpy(wk.maxwell_boltzmann(n, 100.0, mass_amu=wk.MASS_O)).float().cuda()
        return x, v

    def timed(run):
        eng.timing_enable(True)
        run()
        ms = eng.timing_read_steps()
        eng.timing_enable(False)
        assert ms.shape[0] == args.steps
        return ms

    out = {m: [] for m, _ in modes}
    refused = {}
    x, v = fresh()
    f = eng.forward(x, species=species, denormalize=True).clone()
    eng.md_run(x, v, f, 50, temperature_k=100.0, gamma_per_ps=25.0, seed=7, **md)        # warm-up
    done = 50
    for rnd in range(args.rounds):
        for name, pme in modes:
            if name in refused:
                continue
            try:
                conf(args.interval, pme)
                eng.water_classical_forces(torch.from_numpy(pos).float().cuda(), species)   # the k-vector list of this box, or its refusal
            except GamdError as e:
                refused[name] = str(e)
                print(f"{name}: refused: {e}")
                continue
            res = {}
            eng.md_force_source("network")
            ms = timed(lambda: eng.md_run(x, v, f, args.steps, temperature_k=100.0, gamma_per_ps=25.0, seed=7, first_step=done, **md))
            done += args.steps
            rd = eng.water_classical_read()
            assert rd.steps.shape[0] == args.steps // args.interval and np.isfinite(rd.energy).all()
            sampled = (np.arange(1, args.steps + 1) % args.interval) == 0
            res["unsampled_p50_ms"], res["sampled_p50_ms"] = float(np.percentile(ms[~sampled], 50)), float(np.percentile(ms[sampled], 50))
            res["u_recip_last"] = float(rd.u_recip[-1, 0])
            # driven: the water classical source, Nose-Hoover chain, from the lattice start (the network's run goes on from its
            # own state, which a classical potential need not survive)
            conf(0, pme)
            eng.md_force_source("water_classical")
            xd, vd = fresh()
            fd = eng.water_classical_forces(xd, species)[0].float().contiguous()
            ms = timed(lambda: eng.md_run_nhc(xd, vd, fd, args.steps, temperature_k=100.0, **md))
            res["driven_p50_ms"] = float(np.percentile(ms, 50))
            res["driven_finite"] = bool(torch.isfinite(fd).all())
            eng.md_force_source("network")
            out[name].append(res)
    med = lambda name, key: float(np.median([r[key] for r in out[name]]))
    print("\n| mode | grid | sampled p50 ms | unsampled p50 ms | one sample us | driven NHC step p50 ms | per round: sample us | per round: driven ms |")
    print("|---|---|---|---|---|---|---|---|")
    for name, pme in modes:
        if not out[name]:
            print(f"| {name} | {pme} | refused | | | | | |")
            continue
        print(f"| {name} | {pme} | {med(name, 'sampled_p50_ms'):.4f} | {med(name, 'unsampled_p50_ms'):.4f} | "
              f"{1e3 * (med(name, 'sampled_p50_ms') - med(name, 'unsampled_p50_ms')):.1f} | {med(name, 'driven_p50_ms'):.4f} | "
              + " ".join(f"{1e3 * (r['sampled_p50_ms'] - r['unsampled_p50_ms']):.1f}" for r in out[name]) + " | "
              + " ".join(f"{r['driven_p50_ms']:.4f}" for r in out[name]) + " |")

    drift = {}
    if args.drift:
        conf(0, None)
        x0, _ = fresh()
        m = eng.water_minimize(x0, species, tolerance=10.0, r_oh=wk.TIP3P_R_OH, r_hh=wk.TIP3P_R_HH)
        v0 = torch.from_numpy(wk.maxwell_boltzmann(n, 300.0, mass_amu=wk.MASS_O, seed=5)).float().cuda()
        print(f"\ndrift: start minimised under the plain sum (status {m.status}), 300 K velocities, gamma = 0, 2000 steps of 0.5 fs, E_tot every 20 steps")
        print("| mode | grid | E_tot first kJ/mol | max deviation kJ/mol | per atom | slope kJ/mol/ps | mean T K |")
        print("|---|---|---|---|---|---|---|")
        for name, pme in modes:
            if name in refused:
                continue
            conf(20, pme)
            eng.report_configure(20, rigid_water=True)
            eng.md_force_source("water_classical")
            xd, vd = x0.clone(), v0.clone()
            fd = eng.water_classical_forces(xd, species)[0].float().contiguous()
            eng.md_run(xd, vd, fd, 2000, temperature_k=300.0, gamma_per_ps=0.0, seed=3, **md)
            rd, rep = eng.water_classical_read(), eng.report_read()
            e = rep.ke[:, 0] + rd.energy[:, 0]
            t = rd.steps * 0.0005
            slope = float(np.polyfit(t, e, 1)[0])
            drift[name] = dict(first=float(e[0]), max_dev=float(np.abs(e - e[0]).max()), slope=slope, mean_t=float(rep.temperature[:, 0].mean()))
            print(f"| {name} | {pme} | {e[0]:.3f} | {drift[name]['max_dev']:.4f} | {drift[name]['max_dev'] / n:.2e} | {slope:+.4f} | {drift[name]['mean_t']:.1f} |")
            eng.md_force_source("network")
    eng.close()
    print("RESULT " + json.dumps(dict(workload=args.workload, atoms=n, box=box, grid=grid, fine=fine, modes=out, refused=refused, drift=drift)), flush=True)


if __name__ == "__main__":
    main()
