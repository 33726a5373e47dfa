#!/usr/bin/env python3
"""s_memtime breakdown of k_conv_edge at C2 (profiling build, GAMD_CONV_TIME=1): ticks per tile and segment, all waves / waves
0-3 / waves 4-7 (the two halves gather on different sides of the phase barriers).  --perwave adds one column per wave.
s_memtime ticks are not core cycles on this part: read the columns as proportions.  GPU box only."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("GAMD_LIB", os.path.join(ROOT, "gamd_amd", "libgamd_hip_prof.so"))
os.environ["GAMD_CONV_TIME"] = "1"
sys.path.insert(0, ROOT)
import numpy as np
import torch
from gamd_amd.engine import GamdForce
from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
from gamd_amd.workloads import lj_box

SEGMENTS = ["p1 bias init", "p1 gemm+post (+ piece stores, D gather, W2 copy)", "boundary 1 (late waves)", "S gather issue",
            "boundary 1 (early waves) + p2 gemm+post (+ W3 copy)", "boundary 2 (late waves)", "hn gather issue",
            "boundary 2 (early waves) + idx loads + bias", "p3 gemm+post (+ W4 copy)", "boundary 3",
            "p4 gemm+segment-sum (+ W1 copy)", "boundary 4 (late waves)", "e-prefetch issue", "boundary 4 (early waves)"]
n = int(os.environ.get("CV_ATOMS", "10000"))
pos, box = lj_box(n)
sd = make_state_dict(ModelConfig(kind="lj"), 0, 7.0, 2.2)
eng = GamdForce(sd, n, box, 3.0 * 3.4, scaler=SHIPPED_SCALERS["lj"])
p = torch.from_numpy(pos).float().cuda()
for _ in range(3):
    eng.forward(p, inplace=True)
torch.cuda.synchronize()
E = eng.counts()[0]
t = eng._dbg(5, (256, 8, 16), np.int64).astype(np.float64)
nseg = len(SEGMENTS)
tot = t[:, :, :nseg].sum(-1)
tiles_per_wave = (E + 31) // 32 / 8 / 256
print(f"E = {E}; s_memtime ticks per tile (last launch), all / waves 0-3 / waves 4-7; per-wave total {tot.mean():.0f}")
for i, nm in enumerate(SEGMENTS):
    a, o, y = t[:, :, i].mean(), t[:, :4, i].mean(), t[:, 4:, i].mean()
    print(f"    | {nm:52s} | {a / tiles_per_wave:8.0f} | {o / tiles_per_wave:8.0f} | {y / tiles_per_wave:8.0f} |")
print(f"    | sum | {tot.mean() / tiles_per_wave:8.0f} |   (ideal 4 x 2 x 256 MFMA x 64 = 131072)")
if "--perwave" in sys.argv:
    print("    per wave (columns = waves 0..7), ticks per tile:")
    for i, nm in enumerate(SEGMENTS):
        print(f"    | {nm[:40]:40s} | " + " | ".join(f"{t[:, wv, i].mean() / tiles_per_wave:7.0f}" for wv in range(8)) + " |")
