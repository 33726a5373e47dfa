#!/usr/bin/env python3
"""What a sample of the classical observer costs: the per-step device times of sampled and unsampled steps of ONE run on ONE handle.

    python tools/classical_cost.py [--steps 200] [--interval 10] [--rounds 3] [--workloads c1 c2]

On the C1 (258-atom LJ snapshot) and C2 (10 000-atom LJ box: 1e8 pair terms per sample) workloads, in skin mode as bench.py runs
them, per-step device times come from gamd_timing_read_steps over a warmed run of --steps steps with the observer at
--interval (default parameters: sigma 3.4, r_cut 10.2, r_switch 6.8, shifted).  A step's interval runs from the event in front of
its first kernel to the event in front of the next step's, so the sample enqueued behind a step's second half (and, in skin
mode, that second half launched on its own) falls into the sampled step's time.  Printed per workload and round: p50 of the
unsampled steps, p50 of the sampled steps, their difference (the cost of one sample), and the same run's p50 with the observer
off on the same handle; then the medians over the rounds.  A record, not a pass/fail bar.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _engine(workload):
    import numpy as np
    import torch
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


def main():
    import numpy as np
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--interval", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workloads", nargs="+", default=["c1", "c2"], choices=["c1", "c2"])
    args = ap.parse_args()
    if args.interval < 2 or args.steps % args.interval:
        ap.error("--steps must be a multiple of --interval, and --interval at least 2")
    out = {}
    for workload in args.workloads:
        eng, x, v, f = _engine(workload)
        eng.md_run(x, v, f, 50)                                   # warm-up: allocations, first candidate build, clocks
        done, rows = 50, []
        for rnd in range(args.rounds):
            res = {}
            for name, interval in (("off", 0), ("on", args.interval)):
                eng.classical_configure(interval)
                eng.timing_enable(True)
                eng.md_run(x, v, f, args.steps, first_step=done)
                ms = eng.timing_read_steps()
                eng.timing_enable(False)
                done += args.steps
                assert ms.shape[0] == args.steps
                if interval:
                    rd = eng.classical_read()
                    assert rd.steps.shape[0] == args.steps // interval
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
        med = lambda key: float(np.median([r[key] for r in rows]))
        print(f"\n### {workload.upper()} ({x.shape[0]} atoms, {rows[-1]['pairs_per_sample']:.0f} pairs inside r_cut), {args.steps} steps per run, "
              f"interval {args.interval}, {args.rounds} rounds\n")
        print("| round | off p50 ms | unsampled p50 ms | sampled p50 ms | one sample us | mean on - mean off us/step |")
        print("|---|---|---|---|---|---|")
        for k, r in enumerate(rows):
            print(f"| {k} | {r['off_p50_ms']:.4f} | {r['unsampled_p50_ms']:.4f} | {r['sampled_p50_ms']:.4f} | "
                  f"{1e3 * (r['sampled_p50_ms'] - r['unsampled_p50_ms']):.1f} | {1e3 * (r['mean_ms'] - r['off_mean_ms']):+.2f} |")
        print(f"\nmedian over rounds: a sampled step {med('sampled_p50_ms'):.4f} ms against {med('unsampled_p50_ms'):.4f} ms unsampled "
              f"({1e3 * (med('sampled_p50_ms') - med('unsampled_p50_ms')):+.1f} us per sample); observer off {med('off_p50_ms'):.4f} ms")
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
