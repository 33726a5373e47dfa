"""The cell table of the Lennard-Jones classical potential (gamd_classical_cells, gamd_amd/csrc/cell_table.hip and
classical_cells.hip) as far as it can be seen without a GPU.

On every shape of tests/classical_cells_cases.py (the shapes tests/test_gpu_classical_cells.py runs):
  * the case is well posed: the cells per axis it is meant to have, 2 r_cut <= the shortest edge, no pair within 1e-12 r_cut of
    the cutoff (tests/classical_ref.py's `near`);
  * a numpy walk over water_cells_ref.neighbour_cells meets every pair with computed r^2 < r_cut^2 (classical_ref.min_image on
    classical_ref.edges: gamd_lj_walk's operations on the same doubles) exactly once: the pair set by cells is the all-pairs set;
  * the pair pass's order, restated here (runs()): per (x entry, y entry) column the z entries' cells are one run of table slots,
    two when the z window wraps, the whole z line below five cells — and the columns' runs, concatenated in column order, are
    the slots of neighbour_cells in ITS order, x outermost and z innermost; the eight lanes' columns partition them.

gamd_cells_dev.h is covered by tools/cells_host_check.cpp (tests/test_water_cells_host.py)."""
import os

import numpy as np
import pytest

import classical_cells_cases as cc
import classical_ref as cr
import water_cells_ref as cf

LANES = 8                                                   # LJCELL_LANES


def runs(cell, nc, start):
    """the table-slot runs [(s0, s1), ...] of the columns q = 0, 1, ... of `cell`, two per column (the second may be empty), as
    k_ljcell_* take them from `start`"""
    cx, cy, cz = cell // (nc[1] * nc[2]), (cell // nc[2]) % nc[1], cell % nc[2]
    nz = int(nc[2])
    za0, za1, zb1 = 0, nz, 0
    if nz >= 2 * cf.REACH + 1:
        lo, hi = cz - cf.REACH, cz + cf.REACH
        if lo < 0:
            za0, zb1 = lo + nz, hi + 1
        elif hi >= nz:
            za0, zb1 = lo, hi - nz + 1
        else:
            za0, za1 = lo, hi + 1
    out = []
    for ix in cf.neighbour_axis(cx, nc[0]):
        for iy in cf.neighbour_axis(cy, nc[1]):
            cb = (ix * nc[1] + iy) * nz
            out.append([(int(start[cb + za0]), int(start[cb + za1])), (int(start[cb]), int(start[cb + zb1]))])
    return out


@pytest.mark.parametrize("name", list(cc.CASES))
def test_the_shape_is_well_posed_and_the_cell_walk_finds_exactly_the_all_pairs_set(name):
    x, box, lj, want = cc.build(name)
    n = len(x)
    assert 2 * lj.r_cut <= box.min()
    ref = cr.evaluate(x, box, lj)
    nc, start, order = cf.table(x.astype(np.float64), box, lj.r_cut)
    occ = np.diff(start)
    print(f"{name}: nc {tuple(nc)}, {ref['pairs']:.0f} pairs, {ref['near']} at the cutoff, occupancy up to {occ.max()}, "
          f"{int((occ == 0).sum())} of {int(nc.prod())} cells empty, E {ref['energy']:.3e}")
    assert tuple(nc) == want and ref["near"] == 0 and ref["pairs"] > 0
    _, r2 = cr.min_image(x, box)
    inside = r2 < lj.rc2
    np.fill_diagonal(inside, False)
    assert inside.sum() == 2 * ref["pairs"]
    visited = np.zeros((n, n), dtype=np.int32)
    for c in range(int(nc.prod())):
        mine = order[start[c]:start[c + 1]]
        if len(mine) == 0:
            continue
        nb = cf.neighbour_cells(c, nc)
        theirs = np.concatenate([order[start[b]:start[b + 1]] for b in nb])
        visited[np.ix_(mine, theirs)] += 1
        # the kernel's runs are the neighbour list's slots in the neighbour list's order, and the lanes' columns partition them
        cols = runs(c, nc, start)
        slots = [s for col in cols for (s0, s1) in col for s in range(s0, s1)]
        assert np.array_equal(order[slots], theirs) if slots else len(theirs) == 0
        assert len(cols) == cf.neighbour_axis(0, nc[0]).__len__() * cf.neighbour_axis(0, nc[1]).__len__() <= 25
        assert sorted(q for l in range(LANES) for q in range(l, len(cols), LANES)) == list(range(len(cols)))
    assert visited.max() == 1                               # no pair twice
    assert (visited[inside] == 1).all()                     # every pair inside the cutoff is met: found == all pairs
    found = int((visited.astype(bool) & inside).sum())
    assert found == int(inside.sum()) == 2 * int(ref["pairs"])


def test_the_skewed_and_lattice_shapes_are_the_hard_cases_they_are_meant_to_be():
    for name, most in (("300-skew", 20), ("1500-skew", 40)):
        x, box, lj, _ = cc.build(name)
        _, start, _ = cf.table(x.astype(np.float64), box, lj.r_cut)
        assert np.diff(start).max() >= most and (np.diff(start) == 0).sum() > 40
    x, box, lj, nc = cc.build("64-lattice")
    u = x.astype(np.float64) / box.astype(np.float64) * 4.0   # atoms on the faces of the (4, 4, 4) cells, up to fp32 rounding
    assert np.abs(u - np.rint(u)).max() < 1e-6
    x, box, lj, nc = cc.build("300-images")
    assert x.min() < -2 * box.max() and x.max() > 3 * box.min()


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
    import inspect
    from gamd_amd import _lib
    from gamd_amd.engine import GamdForce
    for name in ("gamd_classical_cells", "gamd_classical_cells_read"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.gamd_classical_cells(None, 1) == -22 and b"null handle" in lib.gamd_last_error()
    nc = (C.c_int32 * 3)()
    assert lib.gamd_classical_cells_read(None, None, 0, nc, None, 0, None, 0) == -22 and b"null handle" in lib.gamd_last_error()
    assert inspect.signature(GamdForce.classical_configure).parameters["cells"].default is False
    assert inspect.signature(GamdForce.classical_cells_table).parameters["box"].default == 0
