"""Run reporter, host side (no device): the ABI of gamd_report_params, the argument checks of gamd_report_configure that are
answered before any device work, and RunReport's log writer and g(r) normalisation on synthetic data."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ["interval", "max_samples", "ndf", "rdf_bins", "rdf_rmax", "exclude_same_molecule", "reserved"]

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "gamd_hip.h"
int main(void) {
    printf("sizeof %lu\n", (unsigned long)sizeof(gamd_report_params));
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


def test_report_params_layout_matches_a_c99_translation_unit(tmp_path):
    """sizeof / offsetof as a C99 compiler sees include/gamd_hip.h, against the ctypes mirror."""
    from gamd_amd._lib import GamdReportParams
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed to read the header's layout"
    lines = "\n".join(f'    printf("{f} %lu\\n", (unsigned long)offsetof(gamd_report_params, {f}));' for f in FIELDS)
    src = tmp_path / "probe.c"
    src.write_text(PROBE.replace("@OFFSETS@", lines))
    exe = tmp_path / "probe"
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(GamdReportParams) == int(out.pop("sizeof"))
    assert [n for n, _ in GamdReportParams._fields_] == FIELDS and sorted(out) == sorted(FIELDS)
    for f in FIELDS:
        assert getattr(GamdReportParams, f).offset == int(out[f]), f


def test_report_entry_points_are_declared_bound_and_exported(lib):
    from gamd_amd import _lib
    src = open(os.path.join(ROOT, "include", "gamd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gamd_report_configure", "gamd_report_reset", "gamd_report_read"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in _lib.SYMBOLS and hasattr(lib, name)


def test_configure_rejects_bad_arguments_before_any_device_work(lib):
    from gamd_amd._lib import GamdReportParams
    ok = GamdReportParams(100, 0, 0.0, 0, 0.0, 0, 0)
    assert lib.gamd_report_configure(None, ctypes.byref(ok)) == -22 and b"null handle" in lib.gamd_last_error()
    assert lib.gamd_report_configure(None, None) == -22 and b"null" in lib.gamd_last_error()
    bad = GamdReportParams(-1, 0, 0.0, 0, 0.0, 0, 0)
    assert lib.gamd_report_configure(None, ctypes.byref(bad)) == -22 and b"interval" in lib.gamd_last_error()
    bad = GamdReportParams(100, 0, 0.0, 1025, 0.0, 0, 0)
    assert lib.gamd_report_configure(None, ctypes.byref(bad)) == -22 and b"rdf_bins" in lib.gamd_last_error()
    bad = GamdReportParams(100, 0, 0.0, 64, -1.0, 0, 0)
    assert lib.gamd_report_configure(None, ctypes.byref(bad)) == -22 and b"rdf_rmax" in lib.gamd_last_error()
    assert lib.gamd_report_reset(None) == -22 and b"null handle" in lib.gamd_last_error()
    assert lib.gamd_report_read(None, None, None, None, None, 0, None, None, 0, None, None, None) == -22


def _synthetic_report():
    from gamd_amd.engine import RunReport
    steps = np.array([100, 200, 300, 400], dtype=np.int64)
    ke = np.array([[1.5, 2.5], [3.25, 4.0], [5.0, 6.0], [7.0, 8.125]])
    return RunReport(steps, ke, ke * 10.0, np.zeros((2, 1, 0), dtype=np.uint64), 0, 0)


def test_write_state_data_has_openmm_layout_under_both_step_conventions(tmp_path):
    rep = _synthetic_report()
    dt = 0.002
    for conv, k in ((False, 1), (True, 2)):
        path = tmp_path / f"log{k}.txt"
        rep.write_state_data(str(path), dt, driver_step_convention=conv)
        raw = path.read_bytes()
        head = b'#"Step"\t"Time (ps)"\t"Kinetic Energy (kJ/mole)"\t"Temperature (K)"\n'
        assert raw.startswith(head)
        rows = raw[len(head):].decode().splitlines()
        assert len(rows) == 4
        for row, g, kin in zip(rows, rep.steps, rep.ke[:, 0]):
            cols = row.split("\t")
            assert len(cols) == 4
            assert cols[0] == str(k * int(g)) and float(cols[1]) == k * int(g) * dt
            assert float(cols[2]) == kin and float(cols[3]) == kin * 10.0
    path = tmp_path / "log_box1.csv"
    rep.write_state_data(str(path), dt, separator=",", box=1)
    lines = path.read_text().splitlines()
    assert lines[0] == '#"Step","Time (ps)","Kinetic Energy (kJ/mole)","Temperature (K)"'
    assert [float(l.split(",")[2]) for l in lines[1:]] == list(rep.ke[:, 1])


@pytest.mark.parametrize("classes", [1, 3])
def test_rdf_of_ideal_gas_counts_is_one_in_every_bin(classes):
    """counts constructed as frames * m_ab * V_shell / V (what uncorrelated atoms give) normalise to g = 1."""
    from gamd_amd.engine import RunReport
    bins, r_max, box, frames = 80, 7.5, 23.7, 6
    vol = box ** 3
    edges = np.arange(bins + 1) * (r_max / bins)
    shell = 4.0 / 3.0 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
    if classes == 1:
        n_by = 258
        m = np.array([258.0 ** 2])
    else:
        n_by = (100, 200)
        m = np.array([100.0 ** 2, 2.0 * 100 * 200, 200.0 ** 2])
    scale = 1.0e6                                     # integer counts: make them large enough for the rounding not to show
    counts = np.rint(scale * frames * m[:, None] * shell[None, :] / vol).astype(np.uint64)[None]
    rep = RunReport(np.zeros(0, np.int64), np.zeros((0, 1)), np.zeros((0, 1)), counts, frames, 0, r_max=r_max, volumes=[vol])
    r_mid, g = rep.rdf(0, n_by)
    assert r_mid.shape == (bins,) and g.shape == (classes, bins)
    assert np.allclose(r_mid, 0.5 * (edges[1:] + edges[:-1]))
    assert np.allclose(g / scale, 1.0, rtol=1e-4, atol=0)


def test_reporter_kernels_use_no_scratch(lib):
    """the compiler reports neither spills nor a private segment for k_report_ke / k_report_ke_final / k_report_rdf"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    from gamd_amd import _lib
    res = {n: v for n, v in kernel_resources(_lib.LIB_PATH).items() if "k_report_" in n}
    assert len(res) == 3, sorted(res)
    for n, v in res.items():
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0, (n, v)
    rdf = next(v for n, v in res.items() if "k_report_rdf" in n)
    assert rdf["group_segment_fixed_size"] == 3 * 1024 * 4
