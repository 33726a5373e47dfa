#!/usr/bin/env python3
"""The reference's TIP3P data generator (dataset/generate_tip3p_data.py:76-103: a rigid-water Nose-Hoover-chain run under the
classical force that logs PE / KE / total energy every 50 steps and writes data_{seed}_{t}.npz) as ONE enqueued run, and what
such a run costs.

    python tools/water_ground_truth.py [--workloads w774 c3] [--steps 200] [--interval 50] [--frames 4] [--dt-fs 2.0]
                                       [--energy-ps 1.0] [--ewald-tol 1e-8] [--minimize-tolerance 10] [--lbfgs] [--relax-steps 0] [--seed 0]
                                       [--m-site W] [--out DIR]

For a seeded box of rigid 3-site water (w774: 258 molecules = 774 atoms, the generator's 2 nm box; c3: 1 390 molecules = 4 170
atoms) on one handle in skin mode, as bench.py runs the water workloads, each workload in a fresh process:
  1. the generator: water classical force source, traj_configure(interval, fields x v f), report_configure(interval),
     water_classical_configure(interval), one rigid md_run_nhc of frames * interval steps at 300 K (chain 10, 1 / ps, 5 x 5 as
     the generator's integrator), then RunTrajectory.write_dataset and RunWaterClassical.write_state_data into --out (a temporary
     directory by default): data_{seed}_{t}.npz and log_nvt_tip3p_{seed}.txt;
  2. ms per step (p50 of the per-step HIP-event times of gamd_timing_read_steps over --steps warmed steps), water-classical-driven
     and network-driven, from the same start;
  3. launches of the force path per step of both, from the launch lists of DESIGN.md sections 4.3 and 4.11 (not measured here);
  4. the series E_tot = KE + PE of a gamma = 0 rigid BAOAB run (no friction, no noise) over --energy-ps at --dt-fs and at half of
     it, sampled every 10 fs, from the end of the generator run: the maximum deviation from the first sample and a fitted
     slope, for each.
The start is the workload's lattice box (wl.water_box: whole rigid molecules on a cubic lattice, random orientations).  Left
alone, the lattice releases about 20 kJ/mol per molecule and heats a 300 K start past 1 000 K within 0.4 ps; so, as the
generator's minimizeEnergy (:85) does, step 0 minimises it on the device first: GamdForce.water_minimize to
--minimize-tolerance kJ/mol/nm (rigid-molecule FIRE, not OpenMM's L-BFGS; 0: not minimised), or with --lbfgs
GamdForce.water_minimize_lbfgs (this library's own L-BFGS on rigid molecules; "iterations" are then its evaluations, and
tolerances below about 1 need a switched or shifted Lennard-Jones term).  The earlier stand-in stays
available: --relax-steps steps of a strongly damped water-classical Langevin run at 300 K (--relax-dt-fs, --relax-gamma;
0 steps, the default: none), behind the minimiser when both are on.  Everything below starts from the end of step 0.  The
potential is the plain Ewald sum of
water_classical_configure, not OpenMM's PME, without long-range dispersion, and its default parameters are UNVERIFIED against
OpenMM: the files have the generator's layout, not its numbers.  Records, not pass/fail bars.

--m-site W (TIP4P-Ew: 0.106676721) runs all of it under the 4-site form of the potential — the reference's third generator,
dataset/generate_tip4p_data.py — with the package's TIP4PEW charges and Lennard-Jones parameters (UNVERIFIED as well) and the
weight W: step 0 minimises with the same parameters and the weight 0 (the minimiser is 3-site), then the weight is set and
every start takes its f from water_classical_forces.  The timings then stand next to those of a run without the option."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYERS = 4
N_MOL = {"w774": 258, "c3": 1390}


def _engine(workload, seed):
    import numpy as np
    import torch
    from gamd_amd.engine import GamdForce
    from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
    from gamd_amd import workloads as wk
    sd = make_state_dict(ModelConfig(kind="water", use_bond=True, conv_layer=LAYERS), 3, 2.9, 1.1)
    pos, box, species, bonds = wk.water_box(N_MOL[workload], seed=2345 + seed, jitter=0.0, wrap=False)
    eng = GamdForce(sd, pos.shape[0], box, 4.2, bond=bonds, scaler=SHIPPED_SCALERS["tip3p"], neighbor_skin=4.2 / 6.0)
    mass = np.where(species == 1, wk.MASS_O, wk.MASS_H).reshape(-1, 1)
    v = np.random.default_rng(99 + seed).normal(0.0, 1.0, pos.shape) * 10.0 * np.sqrt(wk.KB * 300.0 / mass)
    x0, v0 = torch.from_numpy(pos).float().cuda(), torch.from_numpy(v).float().cuda()   # (the first rigid half-step projects v)
    md = dict(mass_amu=wk.MASS_O, mass_h_amu=wk.MASS_H, temperature_k=300.0, species=species, rigid_water=True,
              r_oh=wk.TIP3P_R_OH, r_hh=wk.TIP3P_R_HH)
    return eng, x0, v0, species, md


def _start(eng, x0, v0, species, source):
    eng.md_force_source(source)
    x, v = x0.clone(), v0.clone()
    if source == "water_classical":
        f = eng.water_classical_forces(x, species)[0].float().contiguous()
    else:
        f = eng.forward(x, species=species, denormalize=True).clone()
    return x, v, f


def _step_ms(eng, x0, v0, species, md, source, steps, dt_ps):
    import numpy as np
    x, v, f = _start(eng, x0, v0, species, source)
    nhc = dict(dt_ps=dt_ps, frequency_per_ps=1.0, **md)
    chain = eng.md_run_nhc(x, v, f, 50, **nhc)                     # warm-up: allocations, first candidate build, clocks
    eng.timing_enable(True)
    eng.md_run_nhc(x, v, f, steps, chain_state=chain, **nhc)
    ms = eng.timing_read_steps()
    eng.timing_enable(False)
    # (last_status 1: a neighbour buffer overflowed and the run was resumed; its frozen steps are timed too, a few cheap
    #  intervals more that the median does not see)
    print(f"{source}: {ms.shape[0]} timed intervals for {steps} steps, run status {eng.last_status}")
    assert ms.shape[0] >= steps
    return float(np.percentile(ms, 50)), float(ms.mean())


def _potential(args, minimiser=False):
    """keyword arguments of water_classical_configure: the 3-site defaults, or TIP4P-Ew with the weight of --m-site"""
    from gamd_amd.engine import TIP4PEW
    if not args.m_site:
        return dict(ewald_tol=args.ewald_tol)
    return dict(TIP4PEW, m_site=0.0 if minimiser else args.m_site, ewald_tol=args.ewald_tol)


def _energy_series(eng, x0, v0, species, md, dt_ps, total_ps, pot):
    import numpy as np
    every = max(1, int(round(0.010 / dt_ps)))
    steps = int(round(total_ps / dt_ps)) // every * every
    x, v, f = _start(eng, x0, v0, species, "water_classical")
    eng.report_configure(every, max_samples=steps // every, rigid_water=True)
    eng.water_classical_configure(every, max_samples=steps // every, **pot)
    eng.md_run(x, v, f, steps, dt_ps=dt_ps, gamma_per_ps=0.0, **{**md, "temperature_k": 0.0})
    rep, rd = eng.report_read(), eng.water_classical_read()
    eng.report_configure(0)
    eng.water_classical_configure(0, **pot)
    assert np.array_equal(rep.steps, rd.steps) and rd.dropped == 0
    e = rd.energy[:, 0] + rep.ke[:, 0]
    slope = float(np.polyfit(dt_ps * rep.steps, e, 1)[0])             # kJ/mol per ps
    return dict(dt_fs=1e3 * dt_ps, steps=steps, samples=int(e.shape[0]), e_first=float(e[0]), max_dev=float(np.abs(e - e[0]).max()),
                drift_per_ps=slope, ke_mean=float(rep.ke[:, 0].mean()), t_mean=float(rep.temperature[:, 0].mean()))


def _one(args, w, out_dir):
    dt_ps = 1e-3 * args.dt_fs
    eng, x0, v0, species, md = _engine(w, args.seed)
    n = x0.shape[0]
    pot = _potential(args)
    eng.water_classical_configure(0, **_potential(args, minimiser=True))
    res = dict(n=n, m_site=args.m_site)
    # 0. the generator's minimizeEnergy: the lattice minimised on the device ...
    if args.minimize_tolerance > 0:
        x = x0.clone()
        minimise = eng.water_minimize_lbfgs if args.lbfgs else eng.water_minimize
        m = minimise(x, species, tolerance=args.minimize_tolerance, r_oh=md["r_oh"], r_hh=md["r_hh"])
        count = int(m.evaluations[0] if args.lbfgs else m.iterations[0])
        res["minimize"] = dict(tolerance=args.minimize_tolerance, algorithm="lbfgs" if args.lbfgs else "fire", state=m.state[0], iterations=count,
                               u0=float(m.energy_start[0]), u=float(m.energy[0]), rms0=float(m.rms_start[0]), rms=float(m.rms[0]))
        print(f"{w}: lattice minimised to tolerance {args.minimize_tolerance:g} kJ/mol/nm: {m.state[0]} after {count} "
              f"{'evaluations of L-BFGS' if args.lbfgs else 'iterations'}, "
              f"PE {res['minimize']['u0']:.3f} -> {res['minimize']['u']:.3f} kJ/mol, projected rms {res['minimize']['rms0']:.3f} -> {res['minimize']['rms']:.3f}")
        if m.status == 2:
            raise SystemExit(f"{w}: the minimiser failed (the start is not finite)")
        x0 = x
    eng.water_classical_configure(0, **pot)                                 # the weight, behind the minimiser
    # ... and / or relaxed by a strongly damped driven run
    if args.relax_steps > 0:
        x, v, f = _start(eng, x0, v0, species, "water_classical")
        eng.report_configure(args.relax_steps, max_samples=1, rigid_water=True)
        eng.water_classical_configure(args.relax_steps, max_samples=1, **pot)
        u0 = float(eng.water_classical_forces(x, species)[1].energy[0, 0])
        eng.md_run(x, v, f, args.relax_steps, dt_ps=1e-3 * args.relax_dt_fs, gamma_per_ps=args.relax_gamma, seed=args.seed, **md)
        rep, rd = eng.report_read(), eng.water_classical_read()
        eng.report_configure(0)
        eng.water_classical_configure(0, **pot)
        res["relax"] = dict(steps=args.relax_steps, dt_fs=args.relax_dt_fs, gamma_per_ps=args.relax_gamma, u0=u0, u=float(rd.energy[-1, 0]),
                            temperature=float(rep.temperature[-1, 0]))
        print(f"{w}: lattice relaxed by {args.relax_steps} Langevin steps of {args.relax_dt_fs:g} fs at gamma {args.relax_gamma:g} / ps: "
              f"PE {u0:.3f} -> {res['relax']['u']:.3f} kJ/mol, T {res['relax']['temperature']:.1f} K at the end")
        x0, v0 = x.clone(), v.clone()
    # 1. the generator loop as one enqueued run
    x, v, f = _start(eng, x0, v0, species, "water_classical")
    eng.traj_configure(args.interval, max_frames=args.frames, fields=("x", "v", "f"))
    eng.report_configure(args.interval, max_samples=args.frames, rigid_water=True)
    eng.water_classical_configure(args.interval, max_samples=args.frames, **pot)
    eng.md_run_nhc(x, v, f, args.frames * args.interval, dt_ps=dt_ps, frequency_per_ps=1.0, **md)
    tr, rep, rd = eng.traj_read(), eng.report_read(), eng.water_classical_read()
    wdir = os.path.join(out_dir, w)
    paths = tr.write_dataset(wdir, args.seed)
    log = os.path.join(wdir, f"log_nvt_tip3p_{args.seed}.txt")
    rd.write_state_data(rep, log, dt_ps)
    eng.traj_configure(0)
    eng.report_configure(0)
    eng.water_classical_configure(0, **pot)
    res["generator"] = dict(frames=len(paths), log=log, pe=[float(e) for e in rd.energy[:, 0]], temperature=[float(t) for t in rep.temperature[:, 0]],
                            pairs=float(rd.pairs[-1, 0]))
    x_end, v_end = x.clone(), v.clone()
    # 2., 3. cost
    for source in ("water_classical", "network"):
        p50, mean = _step_ms(eng, x0, v0, species, md, source, args.steps, dt_ps)
        res[source] = dict(p50_ms=p50, mean_ms=mean, force_launches=(7 if args.m_site else 5) if source == "water_classical" else 2 + 2 * LAYERS)
    # 4. energy conservation of the driven run, from the generator run's end
    res["energy"] = [_energy_series(eng, x_end, v_end, species, md, dt, args.energy_ps, pot) for dt in (dt_ps, 0.5 * dt_ps)]
    eng.close()
    print(f"\n### {w.upper()}{' M-site ' + format(args.m_site, 'g') if args.m_site else ''} ({n} atoms, {res['generator']['pairs']:.0f} pairs inside r_cut), skin mode, rigid Nose-Hoover chain, "
          f"dt {args.dt_fs:g} fs, ewald_tol {args.ewald_tol:g}, {args.steps} timed steps\n")
    print(f"generator: {len(paths)} frames and {log} written; PE {res['generator']['pe']}; T {res['generator']['temperature']}")
    print("\n| force source | p50 ms/step | mean ms/step | launches of the force path per step |")
    print("|---|---|---|---|")
    for source in ("water_classical", "network"):
        r = res[source]
        print(f"| {source} | {r['p50_ms']:.4f} | {r['mean_ms']:.4f} | {r['force_launches']} |")
    print("\n| dt fs | steps | samples | E_tot first kJ/mol | max abs(E_tot - first) kJ/mol | per atom | fitted drift kJ/mol/ps | mean KE | mean T K |")
    print("|---|---|---|---|---|---|---|---|---|")
    for e in res["energy"]:
        print(f"| {e['dt_fs']:g} | {e['steps']} | {e['samples']} | {e['e_first']:.6f} | {e['max_dev']:.6f} | {e['max_dev'] / n:.3e} | "
              f"{e['drift_per_ps']:+.6f} | {e['ke_mean']:.3f} | {e['t_mean']:.2f} |")
    print("RESULT " + json.dumps({w: res}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=["w774", "c3"], choices=sorted(N_MOL))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--interval", type=int, default=50)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--dt-fs", type=float, default=2.0, help="the generator's time step (dataset/generate_tip3p_data.py:51)")
    ap.add_argument("--energy-ps", type=float, default=1.0)
    ap.add_argument("--ewald-tol", type=float, default=1e-8)
    ap.add_argument("--minimize-tolerance", type=float, default=10.0,
                    help="step 0: GamdForce.water_minimize to this tolerance in kJ/mol/nm (0: the start is not minimised)")
    ap.add_argument("--lbfgs", action="store_true", help="step 0 with GamdForce.water_minimize_lbfgs in place of water_minimize (FIRE)")
    ap.add_argument("--relax-steps", type=int, default=0,
                    help="water-classical Langevin steps at 300 K in front of everything else, behind the minimiser (0: none)")
    ap.add_argument("--relax-dt-fs", type=float, default=1.0)
    ap.add_argument("--relax-gamma", type=float, default=25.0, help="friction of the relaxation run, 1 / ps")
    ap.add_argument("--m-site", type=float, default=0.0,
                    help="the hydrogens' weight of the TIP4P M-site (TIP4P-Ew: 0.106676721) with the TIP4PEW parameters; 0: 3-site water")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help=argparse.SUPPRESS)          # one workload, in this process
    args = ap.parse_args()
    out_dir = args.out or tempfile.mkdtemp(prefix="water_ground_truth_")
    if args.only:
        _one(args, args.only, out_dir)
        return
    out = {}
    for w in args.workloads:                                                # a fresh process per workload; this one opens no GPU
        cmd = [sys.executable, os.path.abspath(__file__), "--only", w, "--out", out_dir] + \
              [a for k in ("steps", "interval", "frames", "dt_fs", "energy_ps", "ewald_tol", "minimize_tolerance", "relax_steps", "relax_dt_fs", "relax_gamma", "m_site", "seed")
               for a in ("--" + k.replace("_", "-"), str(getattr(args, k)))] + (["--lbfgs"] if args.lbfgs else [])
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(p.stdout.split("RESULT ", 1)[0])
        if p.returncode != 0 or "RESULT " not in p.stdout:
            sys.stderr.write(p.stderr[-3000:])
            raise SystemExit(f"{w}: the child process ended with status {p.returncode}")
        out.update(json.loads(p.stdout.split("RESULT ", 1)[1]))
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
