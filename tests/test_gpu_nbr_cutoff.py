"""Edge membership ON the cutoff and at the limit of the Verlet-skin rule, through the C ABI.

Every other neighbour test draws random positions, where a pair within an ulp of the cutoff is a 1e-7 event.  Here the
fixtures (tests/nbr_cases.py) put thousands of pairs ON the cutoff, atoms on the faces of the box and of its cells, and pairs
at the very limit of the skin rule; the expectation is the numpy restatement of the device's predicate (tests/nbr_ref.py,
shown equal to the oracle and sensitive to five wrong masks in tests/test_nbr_reference.py), compared as SETS with no
allowance near the cutoff.  Each fixture runs in exact mode and with neighbor_skin = rc / 6: a rebuild call, a reuse call on
the same positions, and a reuse call after a shift of 0.3 skin (new roundings of every wrapped coordinate).

Figures: profiles/nbr_cutoff_parity.md.
"""
import functools

import numpy as np
import pytest
import torch

import nbr_cases as cases
import nbr_ref as nr
from gamd_amd.weights import ModelConfig, make_state_dict

pytestmark = pytest.mark.gpu
F = np.float32
FLAVOURS = ["jaxmd", "torch"]
SHIFT_DIR = np.array([0.6, 0.64, 0.48])            # unit vector of the 0.3 skin shift


@functools.lru_cache(maxsize=None)
def _sd():
    return make_state_dict(ModelConfig(kind="lj"), 0)


def _engine(n, box, rc, **kw):
    from gamd_amd.engine import GamdForce
    return GamdForce(_sd(), n, box, rc, **kw)


def _keys(eng):
    return nr.edge_keys(eng.debug_edges(), eng.n_total)


def _check_csr(eng, flavour):
    edges = eng.debug_edges()
    row_ptr, col = eng.debug_csr()
    pad = int((col >= eng.n_total).sum())                      # the slots that align the boxes of a batch
    assert row_ptr[0] == 0 and row_ptr[-1] == edges.shape[1] + pad and np.all(np.diff(row_ptr) >= 0)
    assert pad <= 15 * (eng.n_boxes - 1)
    assert bool(np.any(edges[0] == edges[1])) == (flavour == "jaxmd")
    keys = edges[0].astype(np.int64) * eng.n_total + edges[1]
    assert np.unique(keys).size == keys.size                    # no pair twice


@functools.lru_cache(maxsize=None)
def _reference(name, offset, flavour, shifted):
    """(positions as handed to the engine, expected keys): computed once per module and left unchanged"""
    pos, box, rc = cases.tie_case(name, offset)
    if shifted:
        pos = (pos + (0.3 * (rc / 6.0) * SHIFT_DIR).astype(F)).astype(F)
    keys = nr.edge_keys(nr.edges(nr.wrap(pos, box), box, rc, flavour), pos.shape[0])
    keys.setflags(write=False)
    pos.setflags(write=False)
    return pos, keys


def _run_skin_sequence(skin_eng, exact_eng, flavour, calls, box=None):
    """calls: [(positions, expected keys, rebuilds expected after the call)].  Every call of the skin engine is compared
    with the restatement and with the exact-mode engine."""
    for pos, want, rebuilds in calls:
        p = torch.from_numpy(np.array(pos))
        skin_eng.forward(p, box=box)
        assert skin_eng.skin_stats()[0] == rebuilds
        exact_eng.build_neighbors(p, box=box)
        got, exact = _keys(skin_eng), _keys(exact_eng)
        assert np.array_equal(exact, want), f"exact mode: {np.setxor1d(exact, want).size} pairs differ"
        assert np.array_equal(got, want), f"skin mode, {rebuilds} rebuilds: {np.setxor1d(got, want).size} pairs differ"
        _check_csr(skin_eng, flavour)
        _check_csr(exact_eng, flavour)


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("name,offset", cases.TIE_CASES)
def test_pairs_on_the_cutoff_fall_on_the_restatements_side(name, offset, flavour):
    """sc216: one cell per axis, box = 2 rc, k_step_small / k_filter_fill_small; sc1728 and ties1600: the mid-size
    kernels (k_filter_count, k_filter_fill_scan), 3 cells per axis; ortho480: cells 3 / 5 / 2; sc17576: the multi-pass row
    scan above 16 384 rows; ties800 / ties1600: ties in general directions (all three squares inexact)."""
    pos, want = _reference(name, offset, flavour, False)
    pos_shift, want_shift = _reference(name, offset, flavour, True)
    _, box, rc = cases.tie_case(name, offset)
    n = pos.shape[0]
    pairs, _, _ = nr.cutoff_gap64(nr.wrap(pos, box), box, rc, window=cases.TIE_WINDOW)
    assert pairs.shape[1] >= 1000                                   # the fixture is about ties
    if name == "ortho480":
        assert cases.host_cell_counts(box, rc) == [3, 5, 2] and cases.host_cell_counts(box, rc + rc / 6.0) == [3, 5, 2]
    exact = _engine(n, box, rc, nbr_flavour=flavour)
    skin = _engine(n, box, rc, nbr_flavour=flavour, neighbor_skin=rc / 6.0)
    _run_skin_sequence(skin, exact, flavour, [(pos, want, 1), (pos, want, 1), (pos_shift, want_shift, 1)])
    exact.close(); skin.close()


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_pairs_on_the_cutoff_in_a_batch_of_different_boxes(flavour):
    """Three boxes of the 216-atom lattice, different offsets, [n_boxes, 3] boxes of different edges: the batch kernels
    against the restatement, and the batch against its boxes one by one -- same pairs in the same CSR order."""
    pos, boxes, rc = cases.batch_case()
    shift = (0.3 * (rc / 6.0) * SHIFT_DIR).astype(F)
    calls = []
    for p, rebuilds in ((pos, 1), (pos, 1), ((pos + shift).astype(F), 1)):
        calls.append((p, nr.edge_keys(nr.edges(nr.wrap(p, boxes, 3), boxes, rc, flavour, n_boxes=3), 648), rebuilds))
    pairs, _, _ = nr.cutoff_gap64(nr.wrap(pos, boxes, 3), boxes, rc, n_boxes=3, window=cases.TIE_WINDOW)
    assert pairs.shape[1] >= 1000
    exact = _engine(216, boxes[0], rc, nbr_flavour=flavour, n_boxes=3)             # the boxes arrive with every call
    skin = _engine(216, boxes[0], rc, nbr_flavour=flavour, n_boxes=3, neighbor_skin=rc / 6.0)
    _run_skin_sequence(skin, exact, flavour, calls, box=boxes)
    for eng, kw in ((exact, {}), (skin, dict(neighbor_skin=rc / 6.0))):
        batch = eng.debug_edges()
        for b in range(3):
            one = _engine(216, boxes[b], rc, nbr_flavour=flavour, **kw)
            p = torch.from_numpy(calls[2][0][216 * b:216 * (b + 1)].copy())
            if kw:
                one.forward(p)
            else:
                one.build_neighbors(p)
            mine = batch[:, (batch[0] >= 216 * b) & (batch[0] < 216 * (b + 1))] - 216 * b
            assert np.array_equal(mine, one.debug_edges()), (b, kw)
            one.close()
    exact.close(); skin.close()


def _faces_check(box, rc, nc, flavour, min_ties):
    pos = cases.faces_case(box, rc, nc)
    n = pos.shape[0]
    posw = nr.wrap(pos, box)
    want = nr.edge_keys(nr.edges(posw, box, rc, flavour), n)
    pairs, _, _ = nr.cutoff_gap64(posw, box, rc, window=cases.TIE_WINDOW)
    assert pairs.shape[1] >= min_ties
    exact = _engine(n, box, rc, nbr_flavour=flavour)
    skin = _engine(n, box, rc, nbr_flavour=flavour, neighbor_skin=rc / 6.0)
    _run_skin_sequence(skin, exact, flavour, [(pos, want, 1), (pos, want, 1)])
    exact.close(); skin.close()
    return n


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_atoms_on_the_faces_of_the_box_and_of_its_cells(flavour):
    """Per axis an atom on k L / nc and its two fp32 neighbours for every k, on L - ulp, L, -0.0, -1e-9 (remainder rounds up
    to L: the value cell_coord clamps), 37 L + x and -5 L + x, each with partners at rc -/+ one ulp across that face.  The
    expectation is the restatement on remainder(pos)."""
    box, rc = (10.0, 12.7, 9.3), 2.5
    nc = cases.host_cell_counts(box, rc)
    assert nc == [3, 5, 3] and cases.host_cell_counts(box, rc + rc / 6.0) == [3, 4, 3]
    assert 280 <= _faces_check(box, rc, nc, flavour, 100) <= 400


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("skin_on", [False, True])
def test_box_edges_where_the_cell_count_flips(skin_on, side):
    """Box edges on the two fp32 numbers around k x 1.0001 x (rc + skin), k = 3, 4: one cell more or less along that axis,
    the same edge set."""
    rc = 2.5
    radius = float(F(rc)) + (float(F(rc / 6.0)) if skin_on else 0.0)
    e3, e4 = cases.flip_edges(3, radius), cases.flip_edges(4, radius)
    box = (float(e3[side]), float(e4[side]), float(e3[1 - side]))
    assert cases.host_cell_counts(box, radius) == ([2, 3, 3] if side == 0 else [3, 4, 2])
    for flavour in FLAVOURS:
        pos = cases.faces_case(box, rc, (3, 4, 3))
        n = pos.shape[0]
        want = nr.edge_keys(nr.edges(nr.wrap(pos, box), box, rc, flavour), n)
        eng = _engine(n, box, rc, nbr_flavour=flavour, neighbor_skin=rc / 6.0 if skin_on else 0.0)
        p = torch.from_numpy(pos)
        for call in range(2 if skin_on else 1):
            eng.forward(p) if skin_on else eng.build_neighbors(p)
            assert np.array_equal(_keys(eng), want), (flavour, call)
        if skin_on:
            assert eng.skin_stats()[0] == 1
        _check_csr(eng, flavour)
        eng.close()


@pytest.mark.parametrize("n_boxes", [1, 2])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("L", [30.0, 150.0])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_reuse_at_the_limit_of_the_skin_rule_misses_no_edge(flavour, L, padded, n_boxes):
    """Pairs that are the first NON-candidates past rc + skin at the build, and whose atoms then move towards each other as
    far as the move test still calls "not moved" (tests/nbr_cases.py borderline_pairs; general 3-D directions).  The second
    call reuses the list, and its edge set is the exact search's.  With the candidate radius at exactly rc + skin the
    triangle inequality behind the reuse holds in exact arithmetic only, and this test fails by 70-80 directed edges per
    box (profiles/nbr_cutoff_parity.md); the candidate radius carries a margin derived from the fp32 roundings."""
    build, now, box, rc, skin = cases.skin_limit_case(flavour, L, n_boxes=n_boxes, padded=padded)
    n = build.shape[0] // n_boxes
    assert (n > 1024) == padded
    want = nr.edge_keys(nr.edges(nr.wrap(now, box, n_boxes), box, rc, flavour, n_boxes=n_boxes), n * n_boxes)
    kw = dict(nbr_flavour=flavour, n_boxes=n_boxes)
    skin_eng = _engine(n, box, rc, neighbor_skin=skin, **kw)
    exact = _engine(n, box, rc, **kw)
    skin_eng.forward(torch.from_numpy(build))
    assert skin_eng.skin_stats()[0] == 1
    skin_eng.forward(torch.from_numpy(now))
    assert skin_eng.skin_stats()[0] == 1                              # no atom counts as moved: the list is reused
    exact.build_neighbors(torch.from_numpy(now))
    got, ex = _keys(skin_eng), _keys(exact)
    print(f"{flavour} L {L} n {n} x {n_boxes}: reuse step misses {np.setdiff1d(want, got).size} directed edges, "
          f"has {np.setdiff1d(got, want).size} too many")
    assert np.array_equal(ex, want)
    assert np.array_equal(got, want)
    _check_csr(skin_eng, flavour)
    skin_eng.close(); exact.close()


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_reuse_at_the_limit_in_a_box_whose_grid_follows_the_enlarged_radius(flavour):
    """1006.48 x 30 x 30 with rc + skin = 8.75: the 1.0001 rule alone gives 115 cells of 8.7520 along x, narrower than the
    candidate radius with its margin (8.7529 at this box length), so the host takes 114.  Same construction and same checks
    as above, where the roundings are thirty times those of a 30-box."""
    build, now, box, rc, skin = cases.skin_limit_case(flavour, cases.LONG_BOX)
    assert cases.host_cell_counts(box, rc + skin) == [115, 3, 3] and cases.host_cell_counts(box, rc + skin, True) == [114, 3, 3]
    n = build.shape[0]
    want = nr.edge_keys(nr.edges(nr.wrap(now, box), box, rc, flavour), n)
    skin_eng = _engine(n, box, rc, neighbor_skin=skin, nbr_flavour=flavour)
    exact = _engine(n, box, rc, nbr_flavour=flavour)
    skin_eng.forward(torch.from_numpy(build))
    skin_eng.forward(torch.from_numpy(now))
    assert skin_eng.skin_stats()[0] == 1
    exact.build_neighbors(torch.from_numpy(now))
    assert np.array_equal(_keys(exact), want)
    assert np.array_equal(_keys(skin_eng), want)
    _check_csr(skin_eng, flavour)
    skin_eng.close(); exact.close()
