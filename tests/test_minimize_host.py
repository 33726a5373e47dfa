"""The energy minimiser (gamd_minimize, gamd_amd/csrc/minimize.hip) as far as it can be seen without a GPU: the float64 replay
of its recipe (tests/minimize_ref.py) reaches the iteration counts an independent prototype of the same recipe reached, the
entry is exported, bound and refuses a null handle and bad parameter blocks by name, the parameter structure has the header's
layout, the k_min_* kernels are in the release and the checked library within the bars of the observer's pair kernel (no
scratch, at most 128 registers, at most 8 KiB LDS), and the device-free part of the host code passes a stand-alone program
built with the address and undefined-behaviour sanitizers (tools/minimize_host_check.cpp; nothing is loaded into Python)."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import classical_ref as cr
import minimize_ref as mr
from helpers import load_golden
from gamd_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

FIELDS = ["tolerance", "max_iter", "check_every", "dt_start", "dt_max", "f_inc", "f_dec", "alpha_start", "f_alpha", "max_step",
          "n_min", "reserved"]

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "gamd_hip.h"
int main(void) {
    printf("sizeof %lu\n", (unsigned long)sizeof(gamd_minimize_params));
    printf("row %d\n", (int)GAMD_MINIMIZE_ROW);
    printf("states %d%d%d\n", (int)GAMD_MIN_CONVERGED, (int)GAMD_MIN_MAX_ITER, (int)GAMD_MIN_FAILED);
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
    return {"lj258_seed0": (np.mod(g["pos"], box).astype(np.float32), box, 17), "lattice": (lat.astype(np.float32), lbox, 26)}


@pytest.mark.parametrize("name", ["lj258_seed0", "lattice"])
def test_replay_reaches_the_prototypes_iteration_count_at_tolerance_10(name):
    x0, box, want = _starts()[name]
    trace = []
    r = mr.minimize(x0, box, cr.LJ(), 10.0, trace=trace)
    assert r["state"] == mr.CONVERGED and r["iterations"] == want == len(trace) - 1
    assert r["rms"] <= 10.0 and r["u"] == trace[-1][0] and r["u0"] == trace[0][0]
    assert all(u < trace[0][0] for u, _ in trace[1:])           # U below the start from the first step on
    if name == "lj258_seed0":                                   # the snapshot a classical run could not start from
        assert r["u0"] > 1.0e7 and r["rms0"] > 3.0e7
        _, r2 = cr.min_image(r["x"], box)
        assert np.sqrt(r2[np.triu_indices(258, 1)].min()) > 3.0


def test_replay_stops_and_fails_as_the_header_says():
    x0, box, _ = _starts()["lj258_seed0"]
    r = mr.minimize(x0, box, cr.LJ(), 10.0, max_iter=5)
    assert r["state"] == mr.MAX_ITER and r["iterations"] == 5
    x1 = x0.copy()
    x1[7] = x1[3]                                               # two atoms at one point
    r = mr.minimize(x1, box, cr.LJ(), 10.0)
    assert r["state"] == mr.FAILED and r["iterations"] == 0 and np.array_equal(r["x"], x1.astype(np.float64))


def test_wrap_fp32_is_the_integrators_remainder():
    box = 27.25
    x = np.array([[-0.5, 27.25, 30.0], [0.0, -27.25, 54.75]])
    w = mr.wrap_fp32(x, box)
    assert w.dtype == np.float32 and np.array_equal(w, np.array([[26.75, 0.0, 2.75], [0.0, 0.0, 0.25]], dtype=np.float32))


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_the_entry_is_exported_and_in_the_binding_table(lib):
    from gamd_amd import _lib
    assert hasattr(lib, "gamd_minimize") and "gamd_minimize" in _lib.SYMBOLS
    assert _lib.MINIMIZE_ROW == 8 and _lib.MINIMIZE_STATE == ("converged", "max_iter", "failed")


def test_a_null_handle_is_refused_by_name(lib):
    from gamd_amd._lib import GamdMinimizeParams as P
    p = P(tolerance=10.0)
    assert lib.gamd_minimize(None, None, None, 0.0, None, None, ctypes.byref(p), None, None) == -22
    assert b"null handle" in lib.gamd_last_error()


def test_the_parameter_block_is_checked_before_the_handle(lib):
    from gamd_amd._lib import GamdMinimizeParams as P
    cases = [(P(tolerance=0.0), b"tolerance"), (P(tolerance=-1.0), b"tolerance"), (P(tolerance=float("inf")), b"tolerance"),
             (P(tolerance=float("nan")), b"tolerance"), (P(tolerance=1.0, max_iter=-1), b"max_iter"),
             (P(tolerance=1.0, check_every=-1), b"check_every"), (P(tolerance=1.0, n_min=-1), b"n_min"),
             (P(tolerance=1.0, dt_start=-0.1), b"dt_start"), (P(tolerance=1.0, dt_start=0.01, dt_max=0.005), b"dt_max"),
             (P(tolerance=1.0, f_inc=1.0), b"f_inc"), (P(tolerance=1.0, f_dec=1.0), b"f_dec"),
             (P(tolerance=1.0, alpha_start=1.5), b"alpha_start"), (P(tolerance=1.0, f_alpha=-0.5), b"f_alpha"),
             (P(tolerance=1.0, max_step=-0.1), b"max_step")]
    for p, word in cases:
        assert lib.gamd_minimize(None, None, None, 0.0, None, None, ctypes.byref(p), None, None) == -22
        assert word in lib.gamd_last_error(), (word, lib.gamd_last_error())
    assert lib.gamd_minimize(None, None, None, 0.0, None, None, None, None, None) == -22
    assert b"null argument" in lib.gamd_last_error()


def test_minimize_params_layout_matches_a_c99_translation_unit(tmp_path):
    from gamd_amd._lib import MINIMIZE_ROW, GamdMinimizeParams
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed to read the header's layout"
    lines = "\n".join(f'    printf("{f} %lu\\n", (unsigned long)offsetof(gamd_minimize_params, {f}));' for f in FIELDS)
    src = tmp_path / "probe.c"
    src.write_text(PROBE.replace("@OFFSETS@", lines))
    exe = tmp_path / "probe"
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(GamdMinimizeParams) == int(out.pop("sizeof")) == 88
    assert int(out.pop("row")) == MINIMIZE_ROW and out.pop("states") == "012"
    assert [n for n, _ in GamdMinimizeParams._fields_] == FIELDS and sorted(out) == sorted(FIELDS)
    for f in FIELDS:
        assert getattr(GamdMinimizeParams, f).offset == int(out[f]), f


# ---- kernels -------------------------------------------------------------------------------------------------------------
def test_min_kernels_are_in_both_libraries_within_the_observers_bars(lib):
    from gamd_amd import _lib
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    names = ("k_min_init", "k_min_pairs", "k_min_atoms", "k_min_update", "k_min_store_x", "k_min_store_f")
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kr.kernel_resources(path).items() if "k_min_" in n}
        assert len(res) == len(names) and all(any(k in n for n in res) for k in names), sorted(res)
        for n, v in res.items():
            assert "k_classical_" not in n and "k_drive_" not in n
            assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0, (n, v)
            assert v.get("group_segment_fixed_size", 0) <= 8 * 1024, (n, v)          # one staged tile of 256 x 3 doubles
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= 128, (n, v)           # four waves per SIMD at the least


# ---- host code under the sanitizers ----------------------------------------------------------------------------------------
def test_parameter_checks_and_defaults_pass_a_stand_alone_program_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a C++ compiler is needed to build tools/minimize_host_check.cpp"
    exe = tmp_path / "minimize_host_check"
    # the sanitizer runtimes linked into the program itself (clang's default): it needs nothing preloaded
    static = [] if "clang" in os.path.basename(os.path.realpath(cxx)) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                    os.path.join(ROOT, "tools", "minimize_host_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "minimize_host_check: ok" in run.stdout, run.stdout + run.stderr
