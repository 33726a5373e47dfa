"""The cell table of the water classical potential (gamd_water_cells, gamd_amd/csrc/gamd_cells_dev.h, cell_table.hip,
water_cells.hip) as far as it can be seen without a GPU.

The numpy restatement (tests/water_cells_ref.py) on the shapes of tests/test_gpu_water_cells.py (CASES below: the configurations
of tests/test_water_pme_host.py, atoms in several periodic images):
  * every pair with computed r^2 < r_cut^2 (gamd_water_walk's minimum image on the same doubles) lies within two cells along
    every axis, so the walk over the neighbour cells meets it — for the atoms and for the M-site form's charge sites;
  * the neighbour list of every cell is in range, has no cell twice and, united over a cell's atoms, finds exactly the
    all-pairs set: the pair count by cells equals the all-pairs count;
  * the table is a permutation ordered by (cell, atom index) whose starts are the cells' offsets.

gamd_cells_dev.h is called by a stand-alone program (tools/cells_host_check.cpp) built with the host compiler and the address and
undefined-behaviour sanitizers: NaN, +-inf, +-1e30, +-0, exact multiples of L and their neighbours, negative values that round
to s = 1, every face of every nc from 3 to 64, cells per axis for edges and cutoffs that are not numbers, the cells per box of
every triple of those edges (the product of the axes' counts, 64^3 at the most), every neighbour list, and 2 10^5 random pairs
just inside the cutoff.  No Python code runs under a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

import water_cells_ref as cf
import water_msite_ref as w4
import test_water_pme_host as ph
from test_weights_host import ROOT, host_compiler

# (molecules, cubic?, r_cut, cells per axis): what each exercises is said in tests/test_gpu_water_cells.py
CASES = [(86, False, 6.8, (4, 4, 4)), (86, False, 4.2, (6, 6, 7)), (86, False, 3.0, (9, 9, 10)),
         (258, True, 6.8, (5, 5, 5)), (258, True, 4.5, (8, 8, 8)), (258, True, 9.5, (4, 4, 4))]
IDS = [f"{c[0]}-rc{c[2]}" for c in CASES]


def positions(n_mol, cubic, msite, length_per_nm=0.0):
    """the positions the walk reads, as doubles: the fp32 atoms widened, or the charge sites"""
    x, box, species, unit = ph.configuration(n_mol, cubic, length_per_nm)
    xd = x.astype(np.float64)
    return (cf.charge_sites(xd, box, w4.TIP4PEW_W) if msite else xd), box, species, unit


@pytest.mark.parametrize("msite", [False, True], ids=["3site", "4site"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_pair_inside_the_cutoff_lies_within_two_cells_and_the_cell_walk_finds_exactly_the_all_pairs_set(case, msite):
    n_mol, cubic, r_cut, want = case
    x, box, _, _ = positions(n_mol, cubic, msite)
    nc, start, order = cf.table(x, box, r_cut)
    assert tuple(nc) == want
    worst = cf.max_cell_distance(x, box, r_cut)
    inside = cf.pairs_inside(x, box, r_cut)
    print(f"{n_mol} molecules r_cut {r_cut} {'sites' if msite else 'atoms'}: nc {tuple(nc)}, largest cell distance of a pair inside the "
          f"cutoff {worst}, {inside.sum()} of {inside.size - len(x)} ordered pairs inside ({inside.sum() / (inside.size - len(x)):.1%}), "
          f"occupancy up to {np.diff(start).max()}, {int((np.diff(start) == 0).sum())} of {int(nc.prod())} cells empty")
    assert worst <= cf.REACH
    # the table: a permutation by (cell, index), starts = offsets
    cell = cf.cell_of(x, box, nc)
    assert np.array_equal(np.sort(order), np.arange(len(x))) and start[0] == 0 and start[-1] == len(x)
    key = cell[order].astype(np.int64) * len(x) + order
    assert (np.diff(key) > 0).all()
    for c in range(int(nc.prod())):
        assert (cell[order[start[c]:start[c + 1]]] == c).all()
    # the walk over the neighbour cells counts what the all-pairs walk counts, and no cell twice
    found = 0
    for c in range(int(nc.prod())):
        nb = cf.neighbour_cells(c, nc)
        assert len(set(nb)) == len(nb) and all(0 <= b < int(nc.prod()) for b in nb)
        mine = order[start[c]:start[c + 1]]
        if len(mine) == 0:
            continue
        theirs = np.concatenate([order[start[b]:start[b + 1]] for b in nb])
        found += int(inside[np.ix_(mine, theirs)].sum())
    assert found == int(inside.sum())


def test_neighbour_sets_have_no_duplicates_and_the_documented_order():
    for nc in range(1, 65):
        for c in range(nc):
            nb = cf.neighbour_axis(c, nc)
            assert len(set(nb)) == len(nb) == (5 if nc >= 5 else nc) and all(0 <= b < nc for b in nb)
            assert nb == ([(c + o) % nc for o in (-2, -1, 0, 1, 2)] if nc >= 5 else list(range(nc)))
    nc = np.array([4, 5, 7])
    nb = cf.neighbour_cells((1 * 5 + 0) * 7 + 6, nc)
    assert len(nb) == 4 * 5 * 5 and len(set(nb)) == len(nb)
    assert nb[:6] == [(0 * 5 + 3) * 7 + z for z in (4, 5, 6, 0, 1)] + [(0 * 5 + 4) * 7 + 4]       # x outermost, z innermost, wrapped


def test_cells_per_axis_and_faces_that_are_exact():
    assert tuple(cf.ncells(np.float32(20.0), 6.8)) == (5, 5, 5) and tuple(cf.ncells(np.float32(20.0), 4.5)) == (8, 8, 8)
    assert tuple(cf.ncells(ph.EDGES, 4.2)) == (6, 6, 7) and tuple(cf.ncells(ph.EDGES, 3.0)) == (9, 9, 10)
    assert tuple(cf.ncells(np.float32(13.6), 6.8)) == (3, 3, 3)                  # 2 r_cut = L: floor(4 / (1 + 2^-20)) = 3
    assert tuple(cf.ncells(np.float32(1e6), 3.0)) == (64, 64, 64)
    for nc in (5, 8):                                                           # L i / nc is exact in fp32: 4 i and 2.5 i
        face = np.float32(20.0) * np.arange(nc + 1, dtype=np.float32) / np.float32(nc)
        assert np.array_equal(face.astype(np.float64), 20.0 * np.arange(nc + 1) / nc)
        assert np.array_equal(cf.cell_axis(face, 20.0, nc), np.r_[np.arange(nc), 0])
        assert np.array_equal(cf.cell_axis(np.nextafter(face[1:], np.float32(0)), 20.0, nc), np.arange(nc))
        if nc == 8:                                                             # i / 8 - 2 and its fraction are exact; i / 5 - 2 is not:
            assert np.array_equal(cf.cell_axis(face - 40.0, 20.0, nc), np.r_[np.arange(nc), 0])
        else:                                                                   # an image of a face may sit in the cell below it
            assert np.array_equal(cf.cell_axis(face - 40.0, 20.0, nc), [0, 0, 1, 3, 4, 0])
    odd = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, -1e-20, 0.0, -0.0])
    assert np.array_equal(cf.cell_axis(odd, 13.66, 7), np.zeros(8, dtype=np.int64))


# ---- gamd_cells_dev.h under the sanitizers ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_out(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cells_host") / "cells_host_check"
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "cells_host_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-2000:] + run.stderr[-2000:]
    return run.stdout


def test_header_is_plain_cxx_without_a_rocm_include_path(tmp_path):
    src = tmp_path / "only_header.cpp"
    src.write_text('#include "gamd_cells_dev.h"\nint main() { return gamd_cells_index(1.0, 2.0, 8) - 4 + gamd_cells_per_axis(20.0, 4.5) - 8; }\n')
    run = subprocess.run([host_compiler(), "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                          "-I", os.path.join(ROOT, "gamd_amd", "csrc"), str(src)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr


def test_index_cells_per_axis_neighbours_and_reach_hold_for_every_input(check_out):
    lines = dict(l.split(" ", 1) for l in check_out.splitlines())
    assert "FAIL" not in check_out, check_out[-2000:]
    assert lines["index"].split()[0] == "ok" and int(lines["index"].split()[1]) > 2000000
    assert lines["axis"] == "ok 135"
    assert lines["count"] == f"ok {9 * 15 ** 3}"
    assert lines["neighbour"] == f"ok {sum((5 if n >= 5 else n) * n for n in range(1, 65))}"
    assert lines["reach"].split()[0] == "ok" and int(lines["reach"].split()[1]) > 150000


# ---- the library and the package ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from gamd_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_the_entry_points_are_exported_and_bound_and_refuse_a_null_handle_by_name(lib):
    import ctypes as C
    from gamd_amd import _lib
    for name in ("gamd_water_cells", "gamd_water_cells_read"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.gamd_water_cells(None, 1) == -22 and b"null handle" in lib.gamd_last_error()
    nc = (C.c_int32 * 3)()
    assert lib.gamd_water_cells_read(None, None, 0, nc, None, 0, None, 0) == -22 and b"null handle" in lib.gamd_last_error()
