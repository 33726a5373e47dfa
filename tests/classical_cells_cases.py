"""The shapes of the tests of the Lennard-Jones potential's cell table (gamd_classical_cells): tests/test_gpu_classical_cells.py
runs them on the device, tests/test_classical_cells_host.py checks on the CPU that each is well posed — the cells per axis it
is meant to have, no pair within 1e-12 r_cut of the cutoff, 2 r_cut <= the shortest edge — and that a walk over the neighbour
cells finds exactly the all-pairs set.

All are wl.lj_box(n, seed=4) scaled per axis, as tests/test_gpu_classical.py scales it.  `skew` maps every fractional coordinate
s -> s^2 (the atoms crowd towards the origin: cells with tens of atoms next to empty ones, the rank kernel's and the lane
split's hard case; pairs far inside the core, energies of 1e8 kJ/mol and more, still judged by the relative bounds).  `images`
shifts every coordinate by -3 .. +3 box edges.  `lattice` is the jitter-free lattice moved by half a spacing, so that its
atoms sit ON the faces of the (4, 4, 4) cells up to the rounding of the fp32 positions."""
import numpy as np

import classical_ref as cr
from gamd_amd import workloads as wl

SCALE = (1.0, 0.9, 1.15)

# name -> (atoms, scale, LJ keywords, cells per axis, variant)
CASES = {
    "64": (64, (1.0, 1.0, 1.0), dict(r_cut=8.5, r_switch=5.1), (4, 4, 4), None),       # fewer than five cells per axis; below one workgroup
    "300": (300, SCALE, dict(), (5, 5, 6), None),                                      # exactly 2R + 1 on two axes, the wrap on the third
    "300-rc6": (300, SCALE, dict(r_cut=6.0, r_switch=4.0), (9, 8, 10), None),          # most cells empty, occupancy <= 1, unequal axes
    "300-rc4": (300, SCALE, dict(r_cut=4.0, r_switch=0.0, shift=False), (14, 12, 16), None),   # nearly all empty; no switch, no shift
    "1500": (1500, SCALE, dict(), (9, 8, 11), None),                                   # several workgroups and a tail
    "300-skew": (300, SCALE, dict(), (5, 5, 6), "skew"),
    "1500-skew": (1500, SCALE, dict(), (9, 8, 11), "skew"),
    "300-images": (300, SCALE, dict(), (5, 5, 6), "images"),
    "64-lattice": (64, (1.0, 1.0, 1.0), dict(r_cut=8.5, r_switch=5.1), (4, 4, 4), "lattice"),
}


def build(name):
    """(x fp32 [n, 3], box fp32 [3], cr.LJ, cells per axis) of case `name`"""
    n, scale, kw, nc, variant = CASES[name]
    pos, L = wl.lj_box(n, seed=4, jitter=0.0) if variant == "lattice" else wl.lj_box(n, seed=4)
    s = np.asarray(scale)
    box = (np.float32(L) * s.astype(np.float32)).astype(np.float32)
    xd = pos * s[None, :]
    if variant == "skew":
        b = box.astype(np.float64)[None, :]
        frac = xd / b
        xd = (frac * frac) * b
    elif variant == "images":
        k = np.random.default_rng(3).integers(-3, 4, size=xd.shape)
        xd = xd + k * box.astype(np.float64)[None, :]
    elif variant == "lattice":
        m = round(n ** (1.0 / 3.0))
        xd = xd - 0.5 * (L / m)
    return xd.astype(np.float32), box, cr.LJ(**kw), nc
