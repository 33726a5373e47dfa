#!/usr/bin/env python3
"""The reference's LJ data generator (dataset/generate_lj_data.py:74-107: a Nose-Hoover-chain run under the classical force that
logs PE / KE / total energy and writes data_{seed}_{t}.npz) as ONE enqueued run, and what such a run costs.

    python tools/lj_ground_truth.py [--workloads c1 c2] [--steps 200] [--interval 50] [--frames 4] [--energy-ps 2.0]
                                    [--seed 0] [--out DIR] [--start lattice|random] [--minimize TOL]

For a seeded LJ box (C1: 258 atoms, C2: 10 000 atoms; the workload's own lattice box, or with --start random uniform random
points in it) on one handle in skin mode, as bench.py runs it:
  0. with --minimize TOL, the generator's minimizeEnergy (dataset/generate_lj_data.py:83, tolerance 1 there): the start relaxed
     on the device by GamdForce.minimize to an RMS force of TOL kJ/mol/nm (FIRE, not OpenMM's L-BFGS); --start random needs it;
  1. the generator: classical force source, traj_configure(interval, fields x v f), report_configure(interval),
     classical_configure(interval), one md_run_nhc of frames * interval steps, then RunTrajectory.write_dataset and
     RunClassical.write_state_data into --out (a temporary directory by default);
  2. ms per step (p50 of the per-step HIP-event times of gamd_timing_read_steps over --steps warmed steps), classical-driven and
     network-driven, from the same start;
  3. launches per step of both, counted from the launch lists of DESIGN.md sections 4.3 and 4.11 (not measured here: a
     rocprofv3 --kernel-trace run measures them);
  4. the series E_tot = KE + PE of a gamma = 0 BAOAB run (no friction, no noise: velocity Verlet) over --energy-ps at dt = 2 fs and
     at 1 fs, sampled every 10 fs: the maximum deviation from the first sample, for each.
Records, not pass/fail bars."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYERS = 4


def _engine(workload, seed, start="lattice"):
    import numpy as np
    import torch
    from gamd_amd.engine import GamdForce
    from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
    from gamd_amd import workloads as wk
    sd = make_state_dict(ModelConfig(kind="lj", conv_layer=LAYERS), 0, 7.0, 2.2)
    n, rc = (10000, 3.0 * wk.LJ_SIGMA) if workload == "c2" else (258, 7.5)
    pos, box = wk.lj_box(n, seed=1234 + seed)
    if start == "random":                                          # uniform points in the same box: overlaps, needs --minimize
        pos = np.random.default_rng(1234 + seed).random((n, 3)) * box
    eng = GamdForce(sd, n, box, rc, scaler=SHIPPED_SCALERS["lj"], neighbor_skin=rc / 6.0)
    x0 = torch.from_numpy(pos).float().cuda()
    v0 = torch.from_numpy(wk.maxwell_boltzmann(n, 100.0, seed=99 + seed)).float().cuda()
    return eng, x0, v0


def _start(eng, x0, v0, source):
    eng.md_force_source(source)
    x, v = x0.clone(), v0.clone()
    f = eng.classical_forces(x)[0].float().contiguous() if source == "classical" else eng.forward(x, denormalize=True).clone()
    return x, v, f


def _step_ms(eng, x0, v0, source, steps):
    import numpy as np
    x, v, f = _start(eng, x0, v0, source)
    chain = eng.md_run_nhc(x, v, f, 50)                            # warm-up: allocations, first candidate build, clocks
    eng.timing_enable(True)
    eng.md_run_nhc(x, v, f, steps, chain_state=chain)
    ms = eng.timing_read_steps()
    eng.timing_enable(False)
    assert ms.shape[0] == steps
    return float(np.percentile(ms, 50)), float(ms.mean())


def _launches(n, source, integrator):
    """per reuse step in skin mode, from the launch lists of DESIGN.md: the neighbour stage (3 launches up to 1024 atoms, 4
    above), the force path, and the integrator halves that do not ride in the neighbour stage's first kernel"""
    nbr = 3 if n <= 1024 else 4
    force = 2 if source == "classical" else 2 + 2 * LAYERS        # pairs + atoms | encoder, node(0), L x (conv, node)
    return nbr + force + (2 if integrator == "nhc" else 0)


def _energy_series(eng, x0, v0, dt_ps, total_ps):
    import numpy as np
    every = max(1, int(round(0.010 / dt_ps)))
    steps = int(round(total_ps / dt_ps)) // every * every
    x, v, f = _start(eng, x0, v0, "classical")
    eng.report_configure(every, max_samples=steps // every)
    eng.classical_configure(every, max_samples=steps // every)
    eng.md_run(x, v, f, steps, dt_ps=dt_ps, temperature_k=0.0, gamma_per_ps=0.0)
    rep, rd = eng.report_read(), eng.classical_read()
    eng.report_configure(0)
    eng.classical_configure(0)
    assert np.array_equal(rep.steps, rd.steps) and rd.dropped == 0
    e = rd.energy[:, 0] + rep.ke[:, 0]
    return dict(dt_fs=1e3 * dt_ps, steps=steps, samples=int(e.shape[0]), e_first=float(e[0]), max_dev=float(np.abs(e - e[0]).max()),
                ke_mean=float(rep.ke[:, 0].mean()), t_mean=float(rep.temperature[:, 0].mean()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=["c1", "c2"], choices=["c1", "c2"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--interval", type=int, default=50)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--energy-ps", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--start", choices=["lattice", "random"], default="lattice",
                    help="the workload's lattice box, or uniform random points in it (which overlap: give --minimize)")
    ap.add_argument("--minimize", type=float, default=None, metavar="TOL",
                    help="relax the start on the device to an RMS force of TOL kJ/mol/nm first (the generator's minimizeEnergy: 1)")
    args = ap.parse_args()
    if args.start == "random" and args.minimize is None:
        ap.error("--start random gives overlapping atoms: a classical run cannot start there without --minimize TOL")
    out_dir = args.out or tempfile.mkdtemp(prefix="lj_ground_truth_")
    out = {}
    for w in args.workloads:
        eng, x0, v0 = _engine(w, args.seed, args.start)
        n = x0.shape[0]
        eng.classical_configure(0)
        res = dict(n=n)
        # 0. the generator's minimizeEnergy (dataset/generate_lj_data.py:83), on the device
        if args.minimize is not None:
            m = eng.minimize(x0, tolerance=args.minimize)
            if m.status != 0:
                raise SystemExit(f"{w}: the minimiser stopped as {m.state[0]} after {int(m.iterations[0])} iterations (rms {m.rms[0]:.3e} kJ/mol/nm)")
            res["minimize"] = dict(tolerance=args.minimize, start=args.start, iterations=int(m.iterations[0]), u0=float(m.energy_start[0]),
                                   rms0=float(m.rms_start[0]), u=float(m.energy[0]), rms=float(m.rms[0]))
            print(f"{w}: {args.start} start minimised to rms {m.rms[0]:.3e} kJ/mol/nm in {int(m.iterations[0])} iterations: "
                  f"U {m.energy_start[0]:.6e} -> {m.energy[0]:.6f} kJ/mol")
        # 1. the generator loop as one enqueued run
        x, v, f = _start(eng, x0, v0, "classical")
        eng.traj_configure(args.interval, max_frames=args.frames, fields=("x", "v", "f"))
        eng.report_configure(args.interval, max_samples=args.frames)
        eng.classical_configure(args.interval, max_samples=args.frames)
        eng.md_run_nhc(x, v, f, args.frames * args.interval)
        tr, rep, rd = eng.traj_read(), eng.report_read(), eng.classical_read()
        wdir = os.path.join(out_dir, w)
        paths = tr.write_dataset(wdir, args.seed)
        log = os.path.join(wdir, "log_nvt_lj_gt.txt")
        rd.write_state_data(rep, log, 0.002)
        for ob in (eng.traj_configure, eng.report_configure, eng.classical_configure):
            ob(0)
        res["generator"] = dict(frames=len(paths), log=log, pe=[float(e) for e in rd.energy[:, 0]], temperature=[float(t) for t in rep.temperature[:, 0]])
        # 2., 3. cost
        for source in ("classical", "network"):
            p50, mean = _step_ms(eng, x0, v0, source, args.steps)
            res[source] = dict(p50_ms=p50, mean_ms=mean, launches_nhc=_launches(n, source, "nhc"), launches_baoab=_launches(n, source, "baoab"))
        # 4. energy conservation of the classical-driven run
        res["energy"] = [_energy_series(eng, x0, v0, dt, args.energy_ps) for dt in (0.002, 0.001)]
        eng.close()
        out[w] = res
        print(f"\n### {w.upper()} ({n} atoms), skin mode, Nose-Hoover chain, {args.steps} timed steps\n")
        print(f"generator: {len(paths)} frames and {log} written; PE {res['generator']['pe']}; T {res['generator']['temperature']}")
        print("\n| force source | p50 ms/step | mean ms/step | launches per reuse step (NHC) | (BAOAB, fused halves) |")
        print("|---|---|---|---|---|")
        for source in ("classical", "network"):
            r = res[source]
            print(f"| {source} | {r['p50_ms']:.4f} | {r['mean_ms']:.4f} | {r['launches_nhc']} | {r['launches_baoab']} |")
        print("\n| dt fs | steps | samples | E_tot first kJ/mol | max abs(E_tot - first) kJ/mol | per atom | mean KE | mean T K |")
        print("|---|---|---|---|---|---|---|---|")
        for e in res["energy"]:
            print(f"| {e['dt_fs']:.0f} | {e['steps']} | {e['samples']} | {e['e_first']:.6f} | {e['max_dev']:.6f} | {e['max_dev'] / n:.3e} | "
                  f"{e['ke_mean']:.3f} | {e['t_mean']:.2f} |")
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
