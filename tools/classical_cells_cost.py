#!/usr/bin/env python3
"""What the cell table costs against the all-pairs walk of the Lennard-Jones classical potential, on ONE handle per process.

    python tools/classical_cells_cost.py --atoms N [--steps 50] [--interval 10] [--rounds 2] [--minimize-to 0] [--evals 0]

The box is gamd_amd.workloads.lj_box(N) (the workloads' density rho* = 0.5, lattice plus jitter), the potential the default of
classical_configure (r_cut = 3 sigma, switched, shifted), the network the seeded two-layer LJ model in skin mode as bench.py runs
the LJ workloads.  Per-step device times are gamd_timing_read_steps' (HIP events around every step).  Per round the cells are
switched off and on, alternately, on the same box and handle, and for each:
  sampled   a network-driven Langevin run with the observer at --interval: p50 of the sampled steps minus p50 of the
            unsampled ones = the cost of one sample;
  driven    a Nose-Hoover-chain run with the "classical" force source: p50 of a step;
  eval      classical_forces on the start, wall clock around the synchronous call, p50 of 20;
  minimise  (wall of minimize(max_iter=300) - wall of minimize(max_iter=100)) / 200: one FIRE iteration, one look at the gates
            per call; --minimize-to T also times the whole call to tolerance T (first round only).
The two paths' pair counts must agree exactly and their energies to 1e-9 of the energy, or the tool stops (the tests hold
them to 1e-12 of the sum of the absolute pair terms against a float64 reference).  --evals K runs nothing of the above: K classical_forces calls with the cells off and K with them on, for a
kernel trace taken from outside (rocprofv3 --kernel-trace --stats -- python tools/classical_cells_cost.py --atoms N --evals 20):
the all-pairs pass is k_classical_pairs, the cell path the k_ljcell_ kernels.  A record, not a pass/fail bar."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    from gamd_amd.engine import GamdForce
    from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
    from gamd_amd import workloads as wk
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--atoms", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--interval", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--minimize-to", type=float, default=0.0, help="also the whole minimize call to this tolerance (kJ/mol/nm)")
    ap.add_argument("--evals", type=int, default=0, help="only this many eval calls per path, for a kernel trace taken from outside")
    args = ap.parse_args()
    if args.interval < 2 or args.steps % args.interval:
        ap.error("--steps must be a multiple of --interval, and --interval at least 2")

    n = args.atoms
    sd = make_state_dict(ModelConfig(kind="lj", conv_layer=2), 2, 5.0, 1.7)
    pos, box = wk.lj_box(n)
    eng = GamdForce(sd, n, box, 7.5, scaler=SHIPPED_SCALERS["lj"], neighbor_skin=7.5 / 6.0)
    r_cut = 3.0 * 3.4
    nc = int(min(np.floor(2.0 * float(np.float32(box)) / (r_cut * (1.0 + 2.0 ** -20))), 64))
    print(f"{n} atoms, box {box:.3f} A, r_cut {r_cut} A, {nc}^3 cells of {box / nc:.3f} A ({n / nc ** 3:.2f} atoms a cell); "
          f"launches per sample: all pairs 3, cells 8 (the pair launch becomes clear, count, scan, fill, rank, pairs)")
    x_start = torch.from_numpy(pos).float().cuda()
    md = dict(dt_ps=0.002, mass_amu=39.9)

    if args.evals:
        for cells in (False, True):
            eng.classical_configure(0, cells=cells)
            for _ in range(args.evals):
                eng.classical_forces(x_start)
        eng.close()
        return

    def fresh():
        return torch.from_numpy(pos).float().cuda(), torch.from_numpy(wk.maxwell_boltzmann(n, 100.0)).float().cuda()

    def timed(run):
        eng.timing_enable(True)
        run()
        ms = eng.timing_read_steps()
        eng.timing_enable(False)
        assert ms.shape[0] == args.steps
        return ms

    def wall(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        return 1e3 * (time.perf_counter() - t0), out

    modes = [("all", False), ("cells", True)]
    out = {m: [] for m, _ in modes}
    x, v = fresh()
    f = eng.forward(x, denormalize=True).clone()
    eng.md_run(x, v, f, 50, temperature_k=100.0, gamma_per_ps=25.0, seed=7, **md)        # warm-up
    done = 50
    for rnd in range(args.rounds):
        for name, cells in modes:
            res = {}
            eng.classical_configure(args.interval, cells=cells)
            ws = []
            for _ in range(21):
                t, r0 = wall(lambda: eng.classical_forces(x_start))
                ws.append(t)
            res["eval_p50_ms"] = float(np.percentile(ws[1:], 50))
            res["pairs"], res["energy"] = float(r0[3][0]), float(r0[1][0])
            eng.md_force_source("network")
            ms = timed(lambda: eng.md_run(x, v, f, args.steps, temperature_k=100.0, gamma_per_ps=25.0, seed=7, first_step=done, **md))
            done += args.steps
            rd = eng.classical_read()
            assert rd.steps.shape[0] == args.steps // args.interval and np.isfinite(rd.energy).all()
            sampled = (np.arange(1, args.steps + 1) % args.interval) == 0
            res["unsampled_p50_ms"], res["sampled_p50_ms"] = float(np.percentile(ms[~sampled], 50)), float(np.percentile(ms[sampled], 50))
            # driven: the classical source, Nose-Hoover chain, from the start
            eng.classical_configure(0, cells=cells)
            eng.md_force_source("classical")
            xd, vd = fresh()
            fd = eng.classical_forces(xd)[0].float().contiguous()
            ms = timed(lambda: eng.md_run_nhc(xd, vd, fd, args.steps, temperature_k=100.0, **md))
            res["driven_p50_ms"] = float(np.percentile(ms, 50))
            res["driven_finite"] = bool(torch.isfinite(fd).all())
            eng.md_force_source("network")
            # the minimiser: one iteration from two calls that differ by 200 iterations
            t = {}
            for k in (100, 300, 100, 300):
                t[k], _ = wall(lambda: eng.minimize(x_start.clone(), tolerance=1e-300, max_iter=k, check_every=1000))
            res["minimize_iter_us"] = 1e3 * (t[300] - t[100]) / 200.0
            if args.minimize_to > 0.0 and rnd == 0:
                tw, m = wall(lambda: eng.minimize(x_start.clone(), tolerance=args.minimize_to))
                res["minimize_call_ms"], res["minimize_iterations"], res["minimize_state"] = tw, int(m.iterations[0]), m.state[0]
            out[name].append(res)
    a, c = out["all"][0], out["cells"][0]
    assert a["pairs"] == c["pairs"] and abs(a["energy"] - c["energy"]) <= 1e-9 * abs(a["energy"]), (a, c)
    med = lambda name, key: float(np.median([r[key] for r in out[name]]))
    print("\n| pairs | one sample us | driven NHC step p50 ms | eval call p50 ms (wall) | minimise iteration us | per round: sample us | per round: driven ms |")
    print("|---|---|---|---|---|---|---|")
    for name, _ in modes:
        print(f"| {name} | {1e3 * (med(name, 'sampled_p50_ms') - med(name, 'unsampled_p50_ms')):.1f} | {med(name, 'driven_p50_ms'):.4f} | "
              f"{med(name, 'eval_p50_ms'):.4f} | {med(name, 'minimize_iter_us'):.1f} | "
              + " ".join(f"{1e3 * (r['sampled_p50_ms'] - r['unsampled_p50_ms']):.1f}" for r in out[name])
              + " | " + " ".join(f"{r['driven_p50_ms']:.4f}" for r in out[name]) + " |")
    eng.close()
    print("RESULT " + json.dumps(dict(atoms=n, box=box, cells_per_axis=nc, modes=out)), flush=True)


if __name__ == "__main__":
    main()
