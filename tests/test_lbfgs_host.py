"""The L-BFGS energy minimiser (gamd_minimize_lbfgs, gamd_amd/csrc/lbfgs.hip) as far as it can be seen without a GPU: the float64
replay of its recipe (tests/lbfgs_ref.py) converges from the lj258_seed0 snapshot and from the workload's lattice at the
tolerances 10, 1 and 1e-6 with no more pair evaluations than the FIRE replay (tests/minimize_ref.py) needs iterations, keeps
the line search's promises at every evaluation, and stops in each of its four states; the arrangement the device uses (the
recursion on inner products alone, ``form="gram"``) gives the ring form's numbers within the replay's own spread; the entry is
exported, bound and refuses a null handle and bad parameter blocks by name; the parameter structure has the header's layout;
the k_lbfgs_* kernels are in the release and the checked library without scratch and without spills.

One run per start at tolerance 1e-6 serves the tolerances 10 and 1 as well: the tolerance only ends a run, so the run to 1e-6
passes through the points at which the larger tolerances would have stopped it (the first accepted evaluation at or below
each).  The same holds for the FIRE replay, which is run for as many iterations as L-BFGS needed evaluations and no further:
that it has not converged by then is what "at most FIRE's count" means."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import classical_ref as cr
import lbfgs_ref as lr
import minimize_ref as mr
from helpers import load_golden
from gamd_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

FIELDS = ["tolerance", "max_iter", "check_every", "max_step", "c1", "curv", "m", "max_ls", "reserved"]
COUNT_AT_10 = {"lj258_seed0": 23, "lattice": 3}                 # evaluations to tolerance 10, the same under atom permutations

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "gamd_hip.h"
int main(void) {
    printf("sizeof %lu\n", (unsigned long)sizeof(gamd_lbfgs_params));
    printf("row %d\n", (int)GAMD_LBFGS_ROW);
    printf("states %d%d%d%d\n", (int)GAMD_LBFGS_CONVERGED, (int)GAMD_LBFGS_MAX_ITER, (int)GAMD_LBFGS_FAILED, (int)GAMD_LBFGS_LINE_SEARCH);
@OFFSETS@
    return 0;
}
"""


@pytest.fixture(scope="module")
def lib():
    from gamd_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- the replay ----------------------------------------------------------------------------------------------------------
def _starts():
    g, _, _ = load_golden("lj258_seed0")
    box = float(g["box"])
    lat, lbox = wl.lj_box(258)
    return {"lj258_seed0": (np.mod(g["pos"], box).astype(np.float32), box), "lattice": (lat.astype(np.float32), lbox)}


@pytest.fixture(scope="module")
def runs():
    """per start: the L-BFGS replay to 1e-6 with its trace, and the FIRE replay's (U, rms) for as many iterations"""
    out = {}
    for name, (x0, box) in _starts().items():
        trace, fire = [], []
        r = lr.minimize(x0, box, cr.LJ(), 1e-6, trace=trace)
        mr.minimize(x0, box, cr.LJ(), 1e-6, max_iter=r["evaluations"] - 1, trace=fire)
        out[name] = dict(r=r, trace=trace, fire=fire)
    return out


def _count_to(trace, tol):
    """evaluations until the first accepted point with rms <= tol"""
    return next(k + 1 for k, e in enumerate(trace) if e["accepted"] and e["rms"] <= tol)


@pytest.mark.parametrize("name", ["lj258_seed0", "lattice"])
def test_replay_converges_at_10_1_and_1e_6_with_at_most_fires_counts(runs, name):
    r, trace, fire = runs[name]["r"], runs[name]["trace"], runs[name]["fire"]
    assert r["state"] == lr.CONVERGED and r["rms"] <= 1e-6 and r["evaluations"] == len(trace)
    assert r["accepted"] == sum(e["accepted"] for e in trace) and r["u"] < r["u0"]
    counts = {tol: _count_to(trace, tol) for tol in (10.0, 1.0, 1e-6)}
    print(f"{name}: evaluations to 10 / 1 / 1e-6: {counts[10.0]} / {counts[1.0]} / {counts[1e-6]}; accepted {r['accepted']}, "
          f"skipped {r['skipped']}, resets {r['resets']}; U {r['u0']:.6e} -> {r['u']:.9f}")
    assert counts[10.0] == COUNT_AT_10[name] and counts[1e-6] == r["evaluations"]
    # FIRE's iteration k is evaluation k of its trace (0: the start): within L-BFGS's count it has not got there
    for tol in (1.0, 1e-6):
        assert len(fire) >= counts[tol] and all(rms > tol for _, rms in fire[:counts[tol]]), tol
    if name == "lj258_seed0":
        _, r2 = cr.min_image(r["x"], _starts()[name][1])
        assert np.sqrt(r2[np.triu_indices(258, 1)].min()) > 3.0


@pytest.mark.parametrize("name", ["lj258_seed0", "lattice"])
def test_every_evaluation_keeps_the_line_searchs_promises(runs, name):
    r, trace = runs[name]["r"], runs[name]["trace"]
    par = lr.DEFAULTS
    u = r["u0"]
    for k, e in enumerate(trace):
        assert e["smax"] <= par["max_step"] * (1.0 + 1e-15), k          # no atom moves further than max_step in one trial
        assert e["u_from"] == u, k
        if e["accepted"]:
            assert e["fs"] > 0.0 and np.isfinite(e["u"]) and e["u"] <= u - par["c1"] * e["fs"], k      # step 5's inequality
            assert e["u"] <= u, k                                       # U never rises from one accepted point to the next
            u = e["u"]
    assert u == r["u"]


def test_the_count_at_tolerance_10_is_the_same_under_atom_permutations():
    for name, (x0, box) in _starts().items():
        for seed in (1, 2, 3):
            p = np.random.default_rng(seed).permutation(258)
            r = lr.minimize(x0[p], box, cr.LJ(), 10.0)
            assert r["state"] == lr.CONVERGED and r["evaluations"] == COUNT_AT_10[name], (name, seed)


def test_the_recursion_on_inner_products_gives_the_ring_forms_numbers():
    """the device keeps the ring's inner products and runs the two-loop recursion on them (form="gram"); after 32 evaluations
    from lj258_seed0 it is as far from the ring form as the ring form is from itself under an atom permutation, times 100 at most"""
    x0, box = _starts()["lj258_seed0"]
    base = lr.minimize(x0, box, cr.LJ(), 1e-300, max_iter=32)
    gram = lr.minimize(x0, box, cr.LJ(), 1e-300, max_iter=32, form="gram")
    spread = 0.0
    for seed in (1, 2, 3):
        p = np.random.default_rng(seed).permutation(258)
        rp = lr.minimize(x0[p], box, cr.LJ(), 1e-300, max_iter=32)
        xs = np.empty_like(rp["x"])
        xs[p] = rp["x"]
        spread = max(spread, np.abs(xs - base["x"]).max())
    dx = np.abs(gram["x"] - base["x"]).max()
    print(f"gram against ring after 32 evaluations: |dx| max {dx:.3e} A; the ring form's spread under permutations {spread:.3e} A")
    assert all(gram[k] == base[k] for k in ("state", "evaluations", "accepted", "skipped", "resets"))
    assert base["state"] == lr.MAX_ITER and base["evaluations"] == 32
    assert dx <= max(100.0 * spread, 1e-13)


def test_replay_stops_in_each_of_its_states():
    x0, box = _starts()["lj258_seed0"]
    x64 = x0.astype(np.float64)
    r = lr.minimize(x0, box, cr.LJ(), 10.0, max_iter=5)
    assert r["state"] == lr.MAX_ITER and r["evaluations"] == 5 and r["u"] < r["u0"]
    x1 = x0.copy()
    x1[7] = x1[3]                                               # two atoms at one point
    with np.errstate(all="ignore"):
        r = lr.minimize(x1, box, cr.LJ(), 10.0)
    assert r["state"] == lr.FAILED and r["evaluations"] == 0 and np.array_equal(r["x"], x1.astype(np.float64))
    r = lr.minimize(x0, box, cr.LJ(), 1e12)                     # already below the tolerance
    assert r["state"] == lr.CONVERGED and r["evaluations"] == 0 and np.array_equal(r["x"], x64) and r["u"] == r["u0"]
    # the potential is convex along the first steepest step: the decrease falls short of 0.9 of the linear prediction, and one
    # rejection with an empty history ends the search
    r = lr.minimize(x0, box, cr.LJ(), 10.0, max_ls=1, c1=0.9)
    assert r["state"] == lr.LINE_SEARCH and r["evaluations"] == 1 and r["accepted"] == 0 and np.array_equal(r["x"], x64)


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_the_entry_is_exported_and_in_the_binding_table(lib):
    from gamd_amd import _lib
    assert hasattr(lib, "gamd_minimize_lbfgs") and "gamd_minimize_lbfgs" in _lib.SYMBOLS
    assert _lib.LBFGS_ROW == 10 and _lib.LBFGS_STATE == ("converged", "max_iter", "failed", "line_search")
    from gamd_amd.engine import GamdForce, LbfgsResult
    assert callable(GamdForce.minimize_lbfgs)
    res = LbfgsResult(3, [[3, 7, 4, -1.0, 2.0, -3.0, 0.5, 0.25, 1, 2]])
    assert res.state == ["line_search"] and res.evaluations[0] == 7 and res.accepted[0] == 4 and res.skipped[0] == 1 and res.resets[0] == 2
    assert not res.converged and res.energy[0] == -3.0 and res.rms[0] == 0.5 and res.fmax[0] == 0.25


def test_a_null_handle_is_refused_by_name(lib):
    from gamd_amd._lib import GamdLbfgsParams as P
    p = P(tolerance=10.0)
    assert lib.gamd_minimize_lbfgs(None, None, None, 0.0, None, None, ctypes.byref(p), None, None) == -22
    assert b"null handle" in lib.gamd_last_error()


def test_the_parameter_block_is_checked_before_the_handle(lib):
    from gamd_amd._lib import GamdLbfgsParams as P
    cases = [(P(tolerance=0.0), b"tolerance"), (P(tolerance=-1.0), b"tolerance"), (P(tolerance=float("inf")), b"tolerance"),
             (P(tolerance=float("nan")), b"tolerance"), (P(tolerance=1.0, max_iter=-1), b"max_iter"),
             (P(tolerance=1.0, check_every=-1), b"check_every"), (P(tolerance=1.0, m=-1), b"m is outside"),
             (P(tolerance=1.0, m=9), b"m is outside"), (P(tolerance=1.0, c1=1.0), b"c1"), (P(tolerance=1.0, c1=-0.5), b"c1"),
             (P(tolerance=1.0, curv=-1e-3), b"curv"), (P(tolerance=1.0, max_ls=-1), b"max_ls"),
             (P(tolerance=1.0, max_step=-0.1), b"max_step"), (P(tolerance=1.0, reserved=1), b"reserved")]
    for p, word in cases:
        assert lib.gamd_minimize_lbfgs(None, None, None, 0.0, None, None, ctypes.byref(p), None, None) == -22
        assert word in lib.gamd_last_error() and b"gamd_minimize_lbfgs" in lib.gamd_last_error(), (word, lib.gamd_last_error())
    assert lib.gamd_minimize_lbfgs(None, None, None, 0.0, None, None, None, None, None) == -22
    assert b"null argument" in lib.gamd_last_error()
    for m in (1, 8):                                            # the ends of the range pass the block's checks
        assert lib.gamd_minimize_lbfgs(None, None, None, 0.0, None, None, ctypes.byref(P(tolerance=1.0, m=m)), None, None) == -22
        assert b"null handle" in lib.gamd_last_error()


def test_lbfgs_params_layout_matches_a_c99_translation_unit(tmp_path):
    from gamd_amd._lib import LBFGS_ROW, GamdLbfgsParams
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed to read the header's layout"
    lines = "\n".join(f'    printf("{f} %lu\\n", (unsigned long)offsetof(gamd_lbfgs_params, {f}));' for f in FIELDS)
    src = tmp_path / "probe.c"
    src.write_text(PROBE.replace("@OFFSETS@", lines))
    exe = tmp_path / "probe"
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(GamdLbfgsParams) == int(out.pop("sizeof")) == 64
    assert int(out.pop("row")) == LBFGS_ROW and out.pop("states") == "0123"
    assert [n for n, _ in GamdLbfgsParams._fields_] == FIELDS and sorted(out) == sorted(FIELDS)
    for f in FIELDS:
        assert getattr(GamdLbfgsParams, f).offset == int(out[f]), f


# ---- kernels -------------------------------------------------------------------------------------------------------------
def test_lbfgs_kernels_are_in_both_libraries_without_scratch_or_spills(lib):
    """the dots pass carries 33 double accumulators per thread and the decide/update pass the recursion's coefficients: both
    stay in registers (no private segment, no spilled register), and the pair pass stages what k_min_pairs stages"""
    from gamd_amd import _lib
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    names = ("k_lbfgs_init", "k_lbfgs_pairs", "k_lbfgs_dots", "k_lbfgs_update", "k_lbfgs_store_x")
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kr.kernel_resources(path).items() if "k_lbfgs_" in n}
        assert len(res) == len(names) and all(any(k in n for n in res) for k in names), sorted(res)
        for n, v in res.items():
            assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
            assert v.get("group_segment_fixed_size", 0) <= 8 * 1024, (n, v)          # one staged tile of 256 x 3 doubles
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= 128, (n, v)           # four waves per SIMD at the least
