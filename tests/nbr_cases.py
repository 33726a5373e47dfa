"""Fixtures of the cutoff-parity tests (test infrastructure): lattices and clouds whose pairs sit ON the cutoff, atoms on the
faces of the box and of its cells, and a seeded search for pairs at the limit of the Verlet-skin reuse rule.  Generators only: every
array is rebuilt from a few numbers.  Shared by tests/test_nbr_reference.py (CPU) and tests/test_gpu_nbr_cutoff.py."""
import functools

import numpy as np

import nbr_ref as nr

F = np.float32
TIE_WINDOW = 2e-6          # |d64 - rc| below this: the pair sits on the cutoff


def lattice(cells, a, offset):
    """Simple cubic lattice, spacing a (exactly representable, as is every k * a), plus an fp32 offset added in fp32 --
    the offset is what makes the wrapped coordinates, and with them every rounding of the mask, differ from pair to pair."""
    k = np.stack(np.meshgrid(*[np.arange(c) for c in cells], indexing="ij"), -1).reshape(-1, 3)
    base = (k.astype(F) * F(a)).astype(F)
    assert np.array_equal(base.astype(np.float64), k * float(a))
    return (base + np.asarray(offset, dtype=F)).astype(F)


# name -> (cells, a, box, rc, offsets): see the table in profiles/nbr_cutoff_parity.md
LATTICES = {
    "sc216": ((6, 6, 6), 2.5, 15.0, 7.5, (0.0, 0.1, 0.3337, (0.1, 0.3337, 0.7771))),   # 1 cell / axis, box = 2 rc
    "sc1728": ((12, 12, 12), 2.5, 30.0, 7.5, (0.0, 0.1, 0.3337)),                # 3 cells / axis (30 / (7.5 x 1.0001) = 3.9996)
    "ortho480": ((8, 12, 5), 2.5, (20.0, 30.0, 12.5), 5.0, (0.1, 0.3337)),       # cells 3 / 5 / 2 (also with rc / 6 skin)
    "sc17576": ((26, 26, 26), 2.5, 65.0, 5.0, (0.3337,)),                        # 12 cells / axis, > 16 384 rows: multi-pass row scan
}
LATTICE_CASES = [(name, off) for name, v in LATTICES.items() for off in v[4]]
SMALL_LATTICE_CASES = [c for c in LATTICE_CASES if c[0] != "sc17576"]


def lattice_case(name, offset):
    cells, a, box, rc, _ = LATTICES[name]
    return lattice(cells, a, offset), box, rc


# three boxes of the 216-atom lattice, different offsets, different edges (the lattice does not fill the longer ones)
BATCH_OFFSETS = (0.0, 0.1, 0.3337)
BATCH_BOXES = np.array([[15.0, 15.0, 15.0], [15.0, 17.5, 20.0], [20.0, 15.0, 17.5]])


def batch_case():
    pos = np.concatenate([lattice((6, 6, 6), 2.5, off) for off in BATCH_OFFSETS])
    return pos, BATCH_BOXES, 7.5


def host_cell_counts(box, radius, skin_on=False):
    """gamd_api.hip set_box: cells at least 1.0001 x radius wide and, with a skin, at least radius + 64 x 2^-24 x the longest
    edge (the second term decides beyond ~26 radii per edge)."""
    b = [float(F(x)) for x in np.broadcast_to(box, (3,))]
    width = max(float(radius) * 1.0001, float(radius) + 64 * 2.0 ** -24 * max(b) if skin_on else 0.0)
    return [max(1, int(np.floor(x / width))) for x in b]


# a box so long that the cell grid follows the enlarged candidate radius: 115 cells by the 1.0001 rule, 114 with the margin
LONG_BOX = (1006.48, 30.0, 30.0)


# ---- ties in general directions ------------------------------------------------------------------------------------------------
# On a lattice with a round spacing the three squares of a tie pair are (nearly) exact, so a mask that adds them in another
# order, or contracts a product into an add, lands on the same side almost always (profiles/nbr_cutoff_parity.md).  Here every
# centre has four partners a half ulp(L) apart, straddling the cutoff along a direction with three generic components.
TIE_CLOUDS = {"ties800": (160, 30.0, 7.5), "ties1600": (320, 30.0, 7.5)}       # n <= 1024 | mid-size kernels


@functools.lru_cache(maxsize=None)
def tie_cloud(name, seed=7):
    centres, L, rc = TIE_CLOUDS[name]
    rng = np.random.default_rng(seed)
    box = np.full(3, L, dtype=F)
    K = 24
    ks = np.arange(-K, K + 1) * (float(np.spacing(F(L))) / 2.0)
    u = rng.uniform(0.45, 1.0, (centres, 3)) * rng.choice([-1.0, 1.0], (centres, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    a0 = (rng.uniform(0.0, 1.0, (centres, 3)) * L).astype(F)
    grid = (a0.astype(np.float64)[:, None, :] + u[:, None, :] * (rc + ks)[None, :, None]).astype(F)
    inside = nr.d2(nr.wrap(np.broadcast_to(a0[:, None, :], grid.shape), L), nr.wrap(grid, L), box) < nr.rc2_of(rc)
    first_out = np.clip(np.argmax(~inside, axis=1), 2, 2 * K - 1)
    partners = [grid[np.arange(centres), first_out + s] for s in (-2, -1, 0, 1)]
    return np.concatenate([a0] + partners).astype(F), L, rc


TIE_CASES = LATTICE_CASES + [(name, None) for name in TIE_CLOUDS]
SMALL_TIE_CASES = SMALL_LATTICE_CASES + [(name, None) for name in TIE_CLOUDS]


def tie_case(name, offset):
    return tie_cloud(name) if name in TIE_CLOUDS else lattice_case(name, offset)


# ---- faces ---------------------------------------------------------------------------------------------------------------
def _face_values(L, nc, x):
    L = F(L)
    v = []
    for k in range(nc + 1):
        c = F(k * float(L) / nc)
        v += [np.nextafter(c, F(-np.inf)), c, np.nextafter(c, F(np.inf))]
    v += [np.nextafter(L, F(0)), L, F(-0.0), F(-1e-9), F(37.0 * float(L) + x), F(-5.0 * float(L) + x)]
    return [F(t) for t in v]


def faces_case(box, rc, nc, seed=5):
    """Per axis: an atom on every cell face k L / nc and its two fp32 neighbours, on L - ulp and L, on -0.0, on -1e-9 (its
    remainder rounds up to L: the value cell_coord clamps), on 37 L + x and -5 L + x -- each with four partners at
    rc -/+ one ulp on either side along that axis (across the face), the other two coordinates shared and generic."""
    rng = np.random.default_rng(seed)
    box = np.broadcast_to(np.asarray(box, dtype=F), (3,))
    lo, hi = np.nextafter(F(rc), F(0)), np.nextafter(F(rc), F(np.inf))
    pos = []
    for ax in range(3):
        for v in _face_values(box[ax], nc[ax], 1.2345 + ax):
            p = (rng.uniform(0.05, 0.95, 3) * box).astype(F)
            p[ax] = v
            pos.append(p.copy())
            for step in (-hi, -lo, lo, hi):
                q = p.copy()
                q[ax] = F(v + F(step))
                pos.append(q)
    return np.asarray(pos, dtype=F)


def flip_edges(k, radius):
    """The two fp32 numbers around k x 1.0001 x radius, where the host's cell count goes from k - 1 to k."""
    e = k * 1.0001 * float(radius)
    f = F(e)
    return (np.nextafter(f, F(0)), f) if float(f) > e else (f, np.nextafter(f, F(np.inf)))


# ---- the limit of the Verlet-skin reuse rule -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def borderline_pairs(flavour, L, rc, skin, seed, want):
    """Seeded search for pairs a, b in a box L (one edge, or a tuple of three), in general 3-D directions, written against nbr_ref:
      build    b is the first position along the direction from a that is NOT a candidate of radius rc + skin (either way round);
      now      both atoms have moved towards each other as far as moved_beyond still calls "not moved".
    In exact arithmetic such a pair is at least rc apart now; in fp32 it can pass the exact filter: an edge that the
    candidate rows of the parent's rule do not hold.  Returns (build [2, m, 3], now [2, m, 3]) raw fp32 positions (index 0:
    the a atoms), pairs whose two directed edges are both missed first; m <= want."""
    rng = np.random.default_rng(seed)
    T, K = 6000, 32
    box = nr.box3(L)[0]
    radius = nr.build_radius(rc, skin)
    step = float(np.spacing(box.max())) / 4.0
    ks = np.arange(-K, K + 1) * step
    L = box
    u = rng.uniform(0.45, 1.0, (T, 3)) * rng.choice([-1.0, 1.0], (T, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    a0 = (rng.uniform(0.0, 1.0, (T, 3)) * box.astype(np.float64)).astype(F)
    self_ = np.zeros((T, 1), dtype=bool)

    def in_rng(c, n, r):
        return nr.in_range(flavour, nr.d2(nr.wrap(c, L), nr.wrap(n, L), box), r, self_, nr.F(float(r) * float(r)))

    def pick(ok, last):
        """index of the first (or last) true per row, and whether there is one"""
        idx = (ok.shape[1] - 1 - np.argmax(ok[:, ::-1], axis=1)) if last else np.argmax(ok, axis=1)
        return idx, ok.any(axis=1)

    rows = np.arange(T)
    b_grid = (a0.astype(np.float64)[:, None, :] + u[:, None, :] * (float(radius) + ks)[None, :, None]).astype(F)
    a_rep = np.broadcast_to(a0[:, None, :], b_grid.shape)
    not_cand = ~in_rng(a_rep, b_grid, radius) & ~in_rng(b_grid, a_rep, radius)
    kb, ok_b = pick(not_cand, last=False)
    b0 = b_grid[rows, kb]
    s = 0.5 * float(skin) + ks
    a_grid = (a0.astype(np.float64)[:, None, :] + u[:, None, :] * s[None, :, None]).astype(F)
    c_grid = (b0.astype(np.float64)[:, None, :] - u[:, None, :] * s[None, :, None]).astype(F)
    ka, ok_a = pick(~nr.moved_beyond(nr.wrap(a_grid, L), nr.wrap(a_rep, L), box, skin), last=True)
    kc, ok_c = pick(~nr.moved_beyond(nr.wrap(c_grid, L), nr.wrap(np.broadcast_to(b0[:, None, :], c_grid.shape), L), box, skin), last=True)
    a1, b1 = a_grid[rows, ka], c_grid[rows, kc]
    hit_ab = in_rng(a1[:, None], b1[:, None], F(rc))[:, 0]
    hit_ba = in_rng(b1[:, None], a1[:, None], F(rc))[:, 0]
    good = ok_b & ok_a & ok_c & (hit_ab | hit_ba)
    order = np.argsort(~(hit_ab & hit_ba) + 2 * ~good, kind="stable")[:min(want, int(good.sum()))]
    return np.stack([a0[order], b0[order]]), np.stack([a1[order], b1[order]])


def padding_lattice(L, per_axis=10):
    """A frozen lattice that lifts the atom count above 1 024 (its atoms do not move between the two calls)."""
    return lattice((per_axis,) * 3, 1.0, 0.0) * F(L / per_axis) + F(0.37)


def skin_limit_case(flavour, L, n_boxes=1, padded=False, rc=7.5, skin=1.25, pairs=40):
    """(pos_build, pos_now, box, rc, skin) of n_boxes boxes: `pairs` borderline pairs per box (different ones in each box),
    behind them the frozen lattice when `padded`."""
    cubic = np.ndim(L) == 0
    assert cubic or not padded
    build, now = borderline_pairs(flavour, float(L) if cubic else tuple(float(x) for x in L), rc, skin, 11, pairs * 2)
    assert build.shape[1] >= pairs * n_boxes, "the search found too few borderline pairs"
    pb, pn = [], []
    for b in range(n_boxes):
        sl = slice(b * pairs, (b + 1) * pairs)
        extra = [padding_lattice(L)] if padded else []
        pb.append(np.concatenate([build[0, sl], build[1, sl]] + extra))
        pn.append(np.concatenate([now[0, sl], now[1, sl]] + extra))
    return np.concatenate(pb).astype(F), np.concatenate(pn).astype(F), float(L) if cubic else tuple(L), rc, skin
