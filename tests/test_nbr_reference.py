"""The numpy restatement of the neighbour predicate (tests/nbr_ref.py) and the tie / borderline fixtures
(tests/nbr_cases.py), judged on the CPU:

  a. the restatement equals oracle.neighbor_edges pair for pair on fixtures whose pairs sit ON the cutoff (thousands of
     directed pairs within 2e-6 of it), where the float64 classification is off by thousands of pairs;
  b. each of five subtly wrong masks changes the edge set of at least one of those fixtures -- so the GPU tests on the same
     fixtures (tests/test_gpu_nbr_cutoff.py) would catch a kernel path that evaluated the mask that way;
  c. the skin-limit fixture is not vacuous: no atom counts as moved, and with the candidate radius rc + skin a reuse step
     misses edges in general 3-D directions; with the margin of forward.hip it misses none.

Figures: profiles/nbr_cutoff_parity.md."""
import numpy as np
import pytest
import torch

import gamd_oracle as orc
import nbr_cases as cases
import nbr_ref as nr

F = np.float32
FLAVOURS = ["jaxmd", "torch"]


def _oracle_keys(posw, box, rc, flavour, n):
    return nr.edge_keys(orc.neighbor_edges(torch.from_numpy(posw), box, rc, flavour).numpy(), n)


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("name,offset", cases.SMALL_TIE_CASES)
def test_restatement_equals_the_oracle_on_the_tie_fixtures(name, offset, flavour):
    pos, box, rc = cases.tie_case(name, offset)
    n = pos.shape[0]
    posw = nr.wrap(pos, box)
    mine = nr.edge_keys(nr.edges(posw, box, rc, flavour), n)
    assert np.array_equal(mine, _oracle_keys(posw, box, rc, flavour, n))
    # the fixture is about ties: directed pairs on the cutoff, and what a float64 search would make of them
    pairs, gap, inside64 = nr.cutoff_gap64(posw, box, rc, window=cases.TIE_WINDOW)
    assert pairs.shape[1] >= 1000
    in32 = np.isin(pairs[0] * n + pairs[1], mine)
    print(f"{name} offset {offset} {flavour}: n {n} edges {mine.size} on-cutoff pairs {pairs.shape[1]} "
          f"restatement != float64 on {int((in32 != inside64).sum())}")


def test_restatement_equals_the_oracle_box_by_box_and_on_the_faces():
    pos, boxes, rc = cases.batch_case()
    posw = nr.wrap(pos, boxes, 3)
    batch = nr.edges(posw, boxes, rc, "jaxmd", n_boxes=3)
    for b in range(3):
        sl = slice(216 * b, 216 * (b + 1))
        one = nr.edge_keys(nr.edges(posw[sl], boxes[b], rc, "jaxmd"), 216)
        assert np.array_equal(one, _oracle_keys(posw[sl], boxes[b], rc, "jaxmd", 216))
        mine = batch[:, (batch[0] >= 216 * b) & (batch[0] < 216 * (b + 1))] - 216 * b
        assert np.array_equal(nr.edge_keys(mine, 216), one)
    box, rc = (10.0, 12.7, 9.3), 2.5
    pos = cases.faces_case(box, rc, cases.host_cell_counts(box, rc))
    posw = nr.wrap(pos, box)
    for flavour in FLAVOURS:
        assert np.array_equal(nr.edge_keys(nr.edges(posw, box, rc, flavour), pos.shape[0]),
                              _oracle_keys(posw, box, rc, flavour, pos.shape[0]))


def test_remainder_equals_torch_remainder_bit_for_bit_on_the_face_values():
    box, rc = np.array([10.0, 12.7, 9.3], dtype=F), 2.5
    pos = cases.faces_case(box, rc, cases.host_cell_counts(box, rc))
    mine = nr.wrap(pos, box)
    theirs = torch.remainder(torch.from_numpy(pos), torch.from_numpy(box)).numpy()
    assert np.array_equal(mine.view(np.int32), theirs.view(np.int32))
    assert (mine == box).any() and (mine >= 0).all()          # -1e-9 rounds up to the box edge itself
    # and the branch form of the minimum image equals the remainder form on differences of wrapped coordinates
    d = (mine[:, None, :] - mine[None, :, :]).astype(F)
    half = (F(0.5) * box).astype(F)
    ref = (torch.remainder(torch.from_numpy(d + half), torch.from_numpy(box)) - torch.from_numpy(half)).numpy()
    assert np.array_equal(nr.min_image(d, box, half), ref)


def test_the_x_slab_prefilter_does_not_change_the_edge_set():
    pos, box, rc = cases.lattice_case("sc1728", 0.3337)
    posw = nr.wrap(pos, box)
    for flavour in FLAVOURS:
        assert np.array_equal(nr.edges(posw, box, rc, flavour, slab=False), nr.edges(posw, box, rc, flavour, slab=True))


# ---- b. wrong masks ---------------------------------------------------------------------------------------------------------
def _components(c, n, box, min_image=nr.min_image):
    c, n, box = (np.asarray(t, dtype=F) for t in (c, n, box))
    half = (F(0.5) * box).astype(F)
    return [min_image((c[..., k] - n[..., k]).astype(F), box[..., k], half[..., k]) for k in range(3)]


def _d2_contracted(c, n, box):
    """xx + yy contracted into one fused multiply-add: fma(rx, rx, yy), the product unrounded"""
    r = _components(c, n, box)
    yy, zz = (r[1] * r[1]).astype(F), (r[2] * r[2]).astype(F)
    s = (r[0].astype(np.float64) * r[0].astype(np.float64) + yy.astype(np.float64)).astype(F)
    return (s + zz).astype(F)


def _d2_neighbour_minus_centre(c, n, box):
    return nr.d2(n, c, box)


def _d2_other_association(c, n, box):
    r = _components(c, n, box)
    xx, yy, zz = (r[0] * r[0]).astype(F), (r[1] * r[1]).astype(F), (r[2] * r[2]).astype(F)
    return (xx + (yy + zz).astype(F)).astype(F)


def _d2_round_image(c, n, box):
    """d - L round(d / L) in place of the branch form"""
    def image(d, L, half):
        return (d - (L * np.rint((d / L).astype(F)).astype(F)).astype(F)).astype(F)
    r = _components(c, n, box, image)
    xx, yy, zz = (r[0] * r[0]).astype(F), (r[1] * r[1]).astype(F), (r[2] * r[2]).astype(F)
    return ((xx + yy).astype(F) + zz).astype(F)


def _rc2_from_the_rounded_cutoff(rc):
    return F(rc) * F(rc)


MUTATIONS = {
    "xx + yy contracted": dict(d2_fn=_d2_contracted),
    "neighbour minus centre": dict(d2_fn=_d2_neighbour_minus_centre),
    "x2 + (y2 + z2)": dict(d2_fn=_d2_other_association),
    "rc2 = fp32(rc) * fp32(rc)": dict(rc2=_rc2_from_the_rounded_cutoff),
    "round(d / L) minimum image": dict(d2_fn=_d2_round_image),
}


def _mutation_fixtures():
    """The tie fixtures below 2 000 atoms, plus one whose cutoff 10.2 = 3 a is no fp32 number (its square is rounded
    differently from the double and from the rounded cutoff; CPU only -- the C ABI carries the cutoff as a float)."""
    out = {f"{name} +{off}": cases.tie_case(name, off) for name, off in cases.SMALL_TIE_CASES
           if name != "sc1728" or off == 0.1}                # (one offset of the largest lattice: each costs a second)
    out["sc216 a=3.4 rc=10.2"] = ((cases.lattice((6, 6, 6), 1.0, 0.0) * F(3.4)).astype(F), 20.4, 10.2)
    return out


@pytest.fixture(scope="module")
def mutation_table():
    table = {}
    for fname, (pos, box, rc) in _mutation_fixtures().items():
        posw = nr.wrap(pos, box)
        n = pos.shape[0]
        for flavour in FLAVOURS:
            good = nr.edge_keys(nr.edges(posw, box, rc, flavour), n)
            for mname, kw in MUTATIONS.items():
                kw = dict(kw)
                if "rc2" in kw:
                    kw["rc2"] = kw["rc2"](rc)
                bad = nr.edge_keys(nr.edges(posw, box, rc, flavour, **kw), n)
                table[(mname, fname, flavour)] = int(np.setxor1d(good, bad).size)
    return table


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_each_wrong_mask_changes_the_edge_set_of_a_tie_fixture(mutation, mutation_table):
    hits = {k[1:]: v for k, v in mutation_table.items() if k[0] == mutation}
    print(mutation, {f"{f} {fl}": v for (f, fl), v in hits.items() if v})
    assert max(hits.values()) > 0
    if not mutation.startswith("rc2"):
        # ... and on a fixture the GPU tests run, not only on the CPU-only one
        assert max(v for (f, fl), v in hits.items() if "rc=10.2" not in f) > 0


# ---- c. the skin-limit fixture ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [30.0, 150.0, cases.LONG_BOX])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_skin_limit_fixture_is_not_vacuous(flavour, L):
    pb, pn, box, rc, skin = cases.skin_limit_case(flavour, L)
    n = pb.shape[0]
    wb, wn = nr.wrap(pb, box), nr.wrap(pn, box)
    b3 = nr.box3(box)[0]
    l_max, b64 = float(b3.max()), b3.astype(np.float64)
    assert not nr.moved_beyond(wn, wb, b3, skin).any()
    exact = nr.edge_keys(nr.edges(wn, box, rc, flavour), n)
    parent, rebuilt = nr.reuse_edges(wb, wn, box, rc, skin, flavour, nr.build_radius(rc, skin))
    assert not rebuilt
    parent = nr.edge_keys(parent, n)
    missed = np.setdiff1d(exact, parent)
    assert np.setdiff1d(parent, exact).size == 0
    assert missed.size >= 32
    i, j = missed // n, missed % n
    d = wn[i].astype(np.float64) - wn[j].astype(np.float64)
    d -= b64 * np.round(d / b64)
    general = (np.abs(d) > 0.2 * np.linalg.norm(d, axis=1, keepdims=True)).all(axis=1)
    assert 2 * int(general.sum()) >= missed.size
    # the derived margin (forward.hip) closes every one of them
    fixed, rebuilt = nr.reuse_edges(wb, wn, box, rc, skin, flavour, nr.build_radius(rc, skin, l_max))
    assert not rebuilt and np.array_equal(nr.edge_keys(fixed, n), exact)
    # how much of the margin the fixture needs: the largest float64 build distance among the missed pairs
    d0 = wb[i].astype(np.float64) - wb[j].astype(np.float64)
    d0 -= b64 * np.round(d0 / b64)
    need = float(np.linalg.norm(d0, axis=1).max()) - (rc + skin)
    print(f"{flavour} L {L}: parent's rule misses {missed.size} directed edges ({int(general.sum())} in general directions); "
          f"needs {need:.3e} of the margin {nr.skin_margin(l_max):.3e}")
    assert need < nr.skin_margin(l_max)
