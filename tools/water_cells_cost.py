#!/usr/bin/env python3
"""What the cell table costs against the all-pairs walk of the water classical potential, on ONE handle per process.

    python tools/water_cells_cost.py --workload {w774,c3,big} [--steps 100] [--interval 10] [--rounds 3] [--ewald-tol 1e-8]
                                     [--grid-tol 5e-4] [--order 6] [--plain] [--evals 0]

Workloads as tools/water_pme_cost.py: w774 (258 rigid TIP3P molecules), c3 (1 390 molecules = 4 170 atoms) and big (17^3 =
4 913 molecules = 14 739 atoms), r_cut 9.5 A, alpha from --ewald-tol, in skin mode as bench.py runs the water workloads.  The
reciprocal part is PME of --order on the grid pme_grid(alpha, box, --grid-tol) proposes (the grids of profiles/run_water_pme.md);
--plain adds the plain reciprocal sum (where the library takes it).  Per-step device times are gamd_timing_read_steps' (HIP
events around every step).  Per round the cells are switched off and on, alternately, on the same box and handle, and for each:
  sampled   a network-driven Langevin run with the observer at --interval: p50 of the sampled steps minus p50 of the
            unsampled ones = the cost of one sample;
  driven    a Nose-Hoover-chain run with the water classical force source: p50 of a step;
  eval      water_classical_forces on the lattice, wall clock around the synchronous call, p50 of 20.
The two paths' pair counts must agree exactly and their energies to 1e-12 of their magnitude's sum, or the tool stops.
--evals K runs nothing of the above: K water_classical_forces calls with the cells off and K with them on, for a kernel trace
taken from outside (rocprofv3 --kernel-trace --stats -- python tools/water_cells_cost.py --workload big --evals 20): the
all-pairs pass is k_water_pairs, the cell path the k_wcell_ kernels.  A record, not a pass/fail bar.  One workload per process."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_MOL = {"w774": 258, "c3": 1390, "big": 4913}


def main():
    import numpy as np
    import torch
    from gamd_amd.engine import GamdForce, pme_grid
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
    ap.add_argument("--plain", action="store_true", help="also with the plain reciprocal sum")
    ap.add_argument("--evals", type=int, default=0, help="only this many eval calls per path, for a kernel trace taken from outside")
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
    nc = int(min(np.floor(2.0 * float(np.float32(box)) / (9.5 * (1.0 + 2.0 ** -20))), 64))
    print(f"{args.workload}: {n} atoms, box {box:.3f} A, alpha {alpha:.4f} / A, PME grid {grid}, {nc}^3 cells of {box / nc:.3f} A "
          f"({n / nc ** 3:.1f} atoms a cell); launches per sample with PME: all pairs 13, cells 18 (the pair launch becomes clear, "
          f"count, scan, fill, rank, pairs)")
    x_lat = torch.from_numpy(pos).float().cuda()

    def conf(interval, pme, cells):
        eng.water_classical_configure(interval, ewald_tol=args.ewald_tol, pme=pme, pme_order=args.order, cells=cells)

    if args.evals:
        for cells in (False, True):
            conf(0, grid, cells)
            for _ in range(args.evals):
                eng.water_classical_forces(x_lat, species)
        eng.close()
        return

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

    modes = [(f"{r}_{'cells' if c else 'all'}", p, c) for r, p in ([("pme", grid)] + ([("plain", None)] if args.plain else [])) for c in (False, True)]
    out = {m: [] for m, _, _ in modes}
    x, v = fresh()
    f = eng.forward(x, species=species, denormalize=True).clone()
    eng.md_run(x, v, f, 50, temperature_k=100.0, gamma_per_ps=25.0, seed=7, **md)        # warm-up
    done = 50
    for rnd in range(args.rounds):
        for name, pme, cells in modes:
            res = {}
            conf(args.interval, pme, cells)
            wall = []
            for _ in range(21):
                t0 = time.perf_counter()
                _, r0 = eng.water_classical_forces(x_lat, species)
                wall.append(1e3 * (time.perf_counter() - t0))
            res["eval_p50_ms"] = float(np.percentile(wall[1:], 50))
            res["pairs"], res["energy"], res["u_abs"] = float(r0.pairs[0, 0]), float(r0.energy[0, 0]), float(
                abs(r0.u_lj[0, 0]) + abs(r0.u_real[0, 0]) + abs(r0.u_recip[0, 0]) + abs(r0.u_self[0, 0]))
            eng.md_force_source("network")
            ms = timed(lambda: eng.md_run(x, v, f, args.steps, temperature_k=100.0, gamma_per_ps=25.0, seed=7, first_step=done, **md))
            done += args.steps
            rd = eng.water_classical_read()
            assert rd.steps.shape[0] == args.steps // args.interval and np.isfinite(rd.energy).all()
            sampled = (np.arange(1, args.steps + 1) % args.interval) == 0
            res["unsampled_p50_ms"], res["sampled_p50_ms"] = float(np.percentile(ms[~sampled], 50)), float(np.percentile(ms[sampled], 50))
            # driven: the water classical source, Nose-Hoover chain, from the lattice start
            conf(0, pme, cells)
            eng.md_force_source("water_classical")
            xd, vd = fresh()
            fd = eng.water_classical_forces(xd, species)[0].float().contiguous()
            ms = timed(lambda: eng.md_run_nhc(xd, vd, fd, args.steps, temperature_k=100.0, **md))
            res["driven_p50_ms"] = float(np.percentile(ms, 50))
            res["driven_finite"] = bool(torch.isfinite(fd).all())
            eng.md_force_source("network")
            out[name].append(res)
    for r in ("pme", "plain"):
        if f"{r}_all" in out:
            a, c = out[f"{r}_all"][0], out[f"{r}_cells"][0]
            assert a["pairs"] == c["pairs"] and abs(a["energy"] - c["energy"]) <= 1e-12 * a["u_abs"], (a, c)
    med = lambda name, key: float(np.median([r[key] for r in out[name]]))
    print("\n| mode | one sample us | driven NHC step p50 ms | eval call p50 ms (wall) | per round: sample us | per round: driven ms |")
    print("|---|---|---|---|---|---|")
    for name, _, _ in modes:
        print(f"| {name} | {1e3 * (med(name, 'sampled_p50_ms') - med(name, 'unsampled_p50_ms')):.1f} | {med(name, 'driven_p50_ms'):.4f} | "
              f"{med(name, 'eval_p50_ms'):.4f} | " + " ".join(f"{1e3 * (r['sampled_p50_ms'] - r['unsampled_p50_ms']):.1f}" for r in out[name])
              + " | " + " ".join(f"{r['driven_p50_ms']:.4f}" for r in out[name]) + " |")
    eng.close()
    print("RESULT " + json.dumps(dict(workload=args.workload, atoms=n, box=box, grid=grid, cells_per_axis=nc, modes=out)), flush=True)


if __name__ == "__main__":
    main()
