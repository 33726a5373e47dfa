"""Structure sampler, host side (no device): the ABI of gamd_struct_params as a C99 compiler sees it, the argument checks of
gamd_struct_configure that are answered before any device work, the wave-vector list, and RunStructure's g(r) and S(k)
normalisation on synthetic data."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ["interval", "rdf_bins", "rdf_rmax", "exclude_same_molecule", "sk_n2max", "reserved"]

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "gamd_hip.h"
int main(void) {
    printf("sizeof %lu\n", (unsigned long)sizeof(gamd_struct_params));
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


def test_struct_params_layout_matches_a_c99_translation_unit(tmp_path):
    """sizeof / offsetof as a C99 compiler sees include/gamd_hip.h, against the ctypes mirror."""
    from gamd_amd._lib import GamdStructParams
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed to read the header's layout"
    lines = "\n".join(f'    printf("{f} %lu\\n", (unsigned long)offsetof(gamd_struct_params, {f}));' for f in FIELDS)
    src = tmp_path / "probe.c"
    src.write_text(PROBE.replace("@OFFSETS@", lines))
    exe = tmp_path / "probe"
    subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(GamdStructParams) == int(out.pop("sizeof")) == 32
    assert [n for n, _ in GamdStructParams._fields_] == FIELDS and sorted(out) == sorted(FIELDS)
    for f in FIELDS:
        assert getattr(GamdStructParams, f).offset == int(out[f]), f


def test_struct_entry_points_are_declared_bound_and_exported(lib):
    from gamd_amd import _lib
    src = open(os.path.join(ROOT, "include", "gamd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gamd_struct_configure", "gamd_struct_reset", "gamd_struct_read"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in _lib.SYMBOLS and hasattr(lib, name)


def test_configure_checks_its_parameter_block_before_it_needs_a_device(lib):
    from gamd_amd._lib import GamdStructParams
    cases = [(GamdStructParams(-1, 0, 0.0, 0, 0), b"interval"),
             (GamdStructParams(4, 1025, 5.0, 0, 0), b"rdf_bins"),
             (GamdStructParams(4, -1, 5.0, 0, 0), b"rdf_bins"),
             (GamdStructParams(4, 64, 0.0, 0, 0), b"rdf_rmax"),
             (GamdStructParams(4, 64, float("nan"), 0, 0), b"rdf_rmax"),
             (GamdStructParams(4, 0, 0.0, 0, -1), b"sk_n2max"),
             (GamdStructParams(4, 0, 0.0, 0, 155), b"k-vectors"),          # K = 4108 (counted below)
             (GamdStructParams(4, 0, 0.0, 0, 1 << 30), b"k-vectors"),
             (GamdStructParams(4, 64, 5.0, 0, 154), b"null handle")]       # a good block gets as far as the handle
    for p, word in cases:
        assert lib.gamd_struct_configure(None, ctypes.byref(p)) == -22
        assert word in lib.gamd_last_error(), (word, lib.gamd_last_error())
    assert lib.gamd_struct_configure(None, None) == -22
    assert lib.gamd_struct_reset(None) == -22
    assert lib.gamd_struct_read(None, None, None, 0, None, 0, None, 0, None, None) == -22


# ---- the wave-vector list --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n2max,count", [(9, 61), (16, 128), (36, 462), (154, 4060), (155, 4108)])
def test_kvector_list_has_one_of_each_pair_in_the_stated_order(n2max, count):
    from gamd_amd.engine import structure_kvectors
    kv = structure_kvectors(n2max)
    assert kv.dtype == np.int32 and kv.shape == (count, 3)
    # independent count: all integer points of the ball but the origin, halved
    m = int(np.sqrt(n2max)) + 1
    r = np.arange(-m, m + 1)
    n2_all = (r[:, None, None] ** 2 + r[None, :, None] ** 2 + r[None, None, :] ** 2).reshape(-1)
    assert 2 * count == int(((n2_all > 0) & (n2_all <= n2max)).sum())
    n2 = (kv.astype(np.int64) ** 2).sum(axis=1)
    assert n2.min() >= 1 and n2.max() <= n2max
    keys = [(int(a), int(v[0]), int(v[1]), int(v[2])) for a, v in zip(n2, kv)]
    assert keys == sorted(keys) and len(set(keys)) == count                 # sorted by (|n|^2, nx, ny, nz), no repeat
    as_set = {tuple(int(c) for c in v) for v in kv}
    assert all((-a, -b, -c) not in as_set for a, b, c in as_set)             # no +-n duplicate
    for v in kv:                                                             # the first non-zero component is positive
        assert next(int(c) for c in v if c != 0) > 0
    if n2max == 9:
        assert [tuple(v) for v in kv[:4]] == [(0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 1, -1)]


def test_kvector_list_is_empty_for_zero():
    from gamd_amd.engine import structure_kvectors
    assert structure_kvectors(0).shape == (0, 3)


# ---- RunStructure ----------------------------------------------------------------------------------------------------
def test_rdf_of_uniform_counts_is_one():
    """an ideal gas: directed counts frames * N^2 * V_shell / V in every bin give g = 1 (one class), and with m_ab for three.
    The counts are integers: rounding the ideal value moves g by at most half a count, 0.5 / c relative."""
    from gamd_amd.engine import RunStructure
    bins, r_max, frames, L = 50, 10.0, 7, 20.0
    edges = np.arange(bins + 1) * (r_max / bins)
    shell = 4.0 / 3.0 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
    n = 10 ** 6
    c1 = np.rint(frames * float(n) * n * shell / L ** 3)
    rs = RunStructure(c1[None, None, :], np.zeros((1, 1, 0)), np.zeros((0, 3)), frames, r_max, [[L, L, L]])
    r_mid, g = rs.rdf(0, n)
    assert g.shape == (1, bins) and (np.abs(g[0] - 1.0) <= 0.51 / c1).all() and np.allclose(r_mid, 0.5 * (edges[1:] + edges[:-1]))
    n_o, n_h = 10 ** 5, 2 * 10 ** 5
    m = np.array([n_o ** 2, 2 * n_o * n_h, n_h ** 2], dtype=np.float64)
    c3 = np.rint(frames * m[:, None] * shell[None, :] / (L * 0.9 * L * 1.1 * L))
    rs3 = RunStructure(c3[None], np.zeros((1, 3, 0)), np.zeros((0, 3)), frames, r_max, [[L, 0.9 * L, 1.1 * L]])
    _, g3 = rs3.rdf(0, (n_o, n_h))
    assert g3.shape == (3, bins) and (np.abs(g3 - 1.0) <= 0.51 / c3).all()
    with pytest.raises(ValueError):
        rs3.rdf(0, 300)
    with pytest.raises(ValueError):
        RunStructure(np.zeros((1, 1, 0)), np.zeros((1, 1, 0)), np.zeros((0, 3)), 0).rdf(0, 10, volume=1.0)


def test_rdf_normalisation_is_the_reporters():
    from gamd_amd.engine import RunReport, RunStructure
    rng = np.random.default_rng(0)
    c = rng.integers(0, 1000, (2, 3, 40)).astype(np.uint64)
    rep = RunReport([], np.zeros((0, 2)), np.zeros((0, 2)), c, 5, 0, 6.0, [1000.0, 1200.0])
    rs = RunStructure(c, np.zeros((2, 3, 0)), np.zeros((0, 3)), 5, 6.0, [[10, 10, 10], [10, 10, 12]])
    for b in range(2):
        (r0, g0), (r1, g1) = rep.rdf(b, (30, 60)), rs.rdf(b, (30, 60))
        assert np.array_equal(r0, r1) and np.array_equal(g0, g1)


def test_sk_of_a_simple_cubic_lattice_is_n_at_reciprocal_lattice_vectors_and_zero_elsewhere():
    """m^3 atoms at spacing L / m: rho(n) = N when every component of n is a multiple of m, else 0.  Hand-made sums."""
    from gamd_amd.engine import RunStructure, structure_kvectors
    m, L, frames = 3, 12.0, 4
    n_at = m ** 3
    kv = structure_kvectors(18)
    bragg = np.all(kv % m == 0, axis=1)
    assert bragg.sum() == 3 + 6                                              # (0 0 3) and (0 3 3) families, one of each +-
    sums = np.where(bragg, frames * float(n_at) ** 2, 0.0)[None, None, :]
    rs = RunStructure(np.zeros((1, 1, 0)), sums, kv, frames, 0.0, [[L, L, L]])
    k, s = rs.sk(0, n_at)
    assert s.shape == (1, kv.shape[0]) and np.array_equal(s[0][bragg], np.full(9, float(n_at))) and not s[0][~bragg].any()
    assert np.allclose(k, 2.0 * np.pi * np.sqrt((kv.astype(np.float64) ** 2).sum(axis=1)) / L, rtol=1e-15)
    # the same sums from the lattice itself, to tie the hand-made ones to the definition
    g = (np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.25) / m
    rho = np.exp(-2j * np.pi * (kv.astype(np.float64) @ g.T)).sum(axis=1)
    assert np.allclose(np.abs(rho) ** 2, sums[0, 0] / frames, atol=1e-9)
    # shell average: |n|^2 = 9 holds (0 0 3) x 3 among 15 vectors, |n|^2 = 18 holds (0 3 3) x 6 among 18
    ks, ss = rs.sk(0, n_at, shell_average=True)
    n2 = np.unique((kv.astype(np.int64) ** 2).sum(axis=1))
    assert ks.shape == n2.shape and ss.shape == (1, n2.shape[0])
    assert np.allclose(ks, 2.0 * np.pi * np.sqrt(n2) / L)
    cnt9, cnt18 = int(((kv ** 2).sum(1) == 9).sum()), int(((kv ** 2).sum(1) == 18).sum())
    assert np.isclose(ss[0][n2 == 9][0], n_at * 3 / cnt9) and np.isclose(ss[0][n2 == 18][0], n_at * 6 / cnt18)
    assert not ss[0][(n2 != 9) & (n2 != 18)].any()


def test_sk_partial_normalisation_and_per_axis_k():
    from gamd_amd.engine import RunStructure, structure_kvectors
    kv = structure_kvectors(2)
    frames, n_o, n_h = 3, 10, 20
    sums = np.ones((1, 3, kv.shape[0])) * frames
    rs = RunStructure(np.zeros((1, 3, 0)), sums, kv, frames, 0.0, [[10.0, 9.0, 11.5]])
    k, s = rs.sk(0, (n_o, n_h))
    assert np.allclose(s[:, 0], [1.0 / n_o, 1.0 / np.sqrt(n_o * n_h), 1.0 / n_h], rtol=1e-15)
    assert np.allclose(k[:3], [2 * np.pi / 11.5, 2 * np.pi / 9.0, 2 * np.pi / 10.0], rtol=1e-15)   # (0 0 1), (0 1 0), (1 0 0)
    with pytest.raises(ValueError, match="cubic"):
        rs.sk(0, (n_o, n_h), shell_average=True)
    with pytest.raises(ValueError):
        rs.sk(0, 30)


def test_sampler_kernels_use_no_scratch_in_the_release_and_the_checked_library():
    import sys
    from gamd_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kernel_resources(path).items() if "k_struct_" in n}
        assert len(res) == 3, sorted(res)
        for n, v in res.items():
            assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0, (n, v)
            assert v.get("group_segment_fixed_size", 0) <= 64 * 1024, (n, v)        # 3 x 1024 bins + one staged tile
