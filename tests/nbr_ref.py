"""Restatement of the neighbour predicate of csrc/neighbor.hip in numpy, every intermediate held in np.float32 (test
infrastructure; owes nothing to torch).  One function per device function:

    remainder       gamd_remainder            fmod plus the sign fix
    min_image       gamd_min_image_wrapped    the branch form, for differences of wrapped coordinates
    d2              gamd_mask_d2              centre MINUS neighbour, every product rounded, (xx + yy) + zz
    in_range        in_range                  jaxmd: d2 < rc2, self pair kept; torch: sqrt(d2) <= rc, no self
    moved_beyond    d_moved_beyond            the move test of the Verlet-skin reuse
    edges           the exact search          blocked all-pairs mask (per-box boxes for batches)
    reuse_edges     a reuse step              candidates at the build positions, exact filter at the current ones

numpy evaluates `a * b + c` on float32 arrays as two rounded operations (no contraction), which is what the device code asks of
the compiler with `#pragma clang fp contract(off)`.
"""
import numpy as np

F = np.float32
TIE_WINDOW_DEFAULT = 2e-6


def _f(x):
    return np.asarray(x, dtype=F)


def box3(box, n_boxes=1):
    """Scalar, [3] or [n_boxes, 3] -> float32 [n_boxes, 3]."""
    b = np.asarray(box, dtype=np.float64).astype(F)
    if b.ndim == 0:
        b = np.full(3, b, dtype=F)
    if b.ndim == 1:
        b = np.broadcast_to(b.reshape(1, 3), (n_boxes, 3))
    assert b.shape == (n_boxes, 3)
    return np.ascontiguousarray(b)


def remainder(a, b):
    a, b = np.broadcast_arrays(_f(a), _f(b))
    m = np.fmod(a, b).astype(F)
    fix = (m != 0) & ((b < 0) != (m < 0))
    return np.where(fix, (m + b).astype(F), m).astype(F)


def wrap(pos, box, n_boxes=1):
    """remainder(pos, box of the atom's box) for [n_boxes * n_per_box, 3] positions, box-major."""
    pos = _f(pos)
    b = box3(box, n_boxes)
    if n_boxes == 1:
        return remainder(pos, b[0])                  # any leading shape
    return remainder(pos.reshape(n_boxes, -1, 3), b[:, None, :]).reshape(-1, 3)


def min_image(d, L, half):
    d, L, half = _f(d), _f(L), _f(half)
    t = (d + half).astype(F)
    t = np.where(t < 0, (t + L).astype(F), np.where(t >= L, (t - L).astype(F), t)).astype(F)
    return (t - half).astype(F)


def d2(centre, neighbour, box):
    """Squared minimum-image distance of wrapped positions; [..., 3] operands broadcast against each other, box [3]."""
    centre, neighbour, box = _f(centre), _f(neighbour), _f(box)
    half = (F(0.5) * box).astype(F)
    r = [min_image((centre[..., k] - neighbour[..., k]).astype(F), box[..., k], half[..., k]) for k in range(3)]
    xx, yy, zz = (r[0] * r[0]).astype(F), (r[1] * r[1]).astype(F), (r[2] * r[2]).astype(F)
    return ((xx + yy).astype(F) + zz).astype(F)


def rc2_of(rc):
    """graph_utils.py:59 `cutoff ** 2`: squared in double, rounded to fp32 once."""
    return F(float(rc) * float(rc))


def in_range(flavour, dd, rc, is_self, rc2=None):
    if flavour == "jaxmd":
        return dd < (rc2_of(rc) if rc2 is None else F(rc2))
    return (np.sqrt(_f(dd)).astype(F) <= F(rc)) & ~is_self


def skin_half2(skin):
    return F(F(0.25) * F(skin)) * F(skin)


def moved_beyond(p, r, box, skin):
    """Has the atom at wrapped position p moved more than skin / 2 from r?  (NaN counts as moved.)"""
    p, r, box = _f(p), _f(r), _f(box)
    half = (F(0.5) * box).astype(F)
    d = [min_image((p[..., k] - r[..., k]).astype(F), box[..., k], half[..., k]) for k in range(3)]
    s = (((d[0] * d[0]).astype(F) + (d[1] * d[1]).astype(F)).astype(F) + (d[2] * d[2]).astype(F)).astype(F)
    return ~(s <= skin_half2(skin))


MARGIN_ULPS = 48          # forward.hip GAMD_SKIN_MARGIN_EPS: the margin is 48 x 2^-24 x the longest box edge


def skin_margin(l_max):
    return MARGIN_ULPS * 2.0 ** -24 * float(F(l_max))


def build_radius(rc, skin, l_max=None):
    """The candidate radius as float32.  l_max None: rc + skin as a float32 sum, the rule without a margin (exact
    arithmetic's triangle inequality); l_max = the longest box edge: forward.hip's rc + skin + skin_margin(l_max), summed
    in double and rounded once."""
    if l_max is None:
        return F(F(rc) + F(skin))
    return F(float(F(rc)) + float(F(skin)) + skin_margin(l_max))


def _near_columns(p, rows, box, reach):
    """Columns whose float64 circular distance to the rows' bounding interval is at most reach along x AND along y (a
    superset prefilter: a pair closer than reach is closer than reach along every axis)."""
    keep = np.ones(p.shape[0], dtype=bool)
    for ax in (0, 1):
        x, L = p[:, ax].astype(np.float64), float(box[ax])
        lo, hi = float(x[rows].min()), float(x[rows].max())
        dx = np.mod(x - 0.5 * (lo + hi) + 0.5 * L, L) - 0.5 * L
        keep &= np.abs(dx) <= 0.5 * (hi - lo) + reach
    return np.nonzero(keep)[0]


def _blocks(p, box, reach, block):
    """(rows, columns) blocks that cover every pair of one box -- all columns, or with `reach` the rows in (x, y) order
    and the columns near them."""
    n = p.shape[0]
    if reach is None:
        for s in range(0, n, block):
            yield np.arange(s, min(n, s + block)), np.arange(n)
        return
    order = np.lexsort((p[:, 1], p[:, 0]))
    for s in range(0, n, 64):
        rows = order[s:s + 64]
        yield rows, _near_columns(p, rows, box, reach)


def pair_mask_edges(pos, box, n_boxes, mask_fn, block=256, slab_reach=None):
    """All directed pairs (centre i, neighbour j) of the same box with mask_fn(centre [b,1,3], neighbour [1,m,3], box [3],
    is_self [b,m]) true: int64 [2, E], centre-major, neighbours ascending, ids box-major over all boxes.  slab_reach (a
    length well above the largest radius mask_fn accepts): only the columns within that reach of a block of rows along x
    and y (float64, minimum image) are evaluated -- the same mask on fewer pairs."""
    pos = _f(pos)
    b3 = box3(box, n_boxes)
    npb = pos.shape[0] // n_boxes
    out_c, out_n = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for b in range(n_boxes):
        p = pos[b * npb:(b + 1) * npb]
        for rows, cols in _blocks(p, b3[b], slab_reach, block):
            m = mask_fn(p[rows][:, None, :], p[cols][None, :, :], b3[b], rows[:, None] == cols[None, :])
            i, j = np.nonzero(m)
            out_c.append(rows[i] + b * npb)
            out_n.append(cols[j] + b * npb)
    c, n = np.concatenate(out_c), np.concatenate(out_n)
    o = np.lexsort((n, c))
    return np.stack([c[o], n[o]]).astype(np.int64)


def edges(pos, box, rc, flavour, n_boxes=1, slab=None, d2_fn=d2, rc2=None):
    """The exact search on WRAPPED positions.  slab: use the x prefilter (default: above 4096 atoms per box)."""
    npb = np.asarray(pos).shape[0] // n_boxes
    if slab is None:
        slab = npb > 4096
    return pair_mask_edges(pos, box, n_boxes,
                           lambda c, n, b, self_: in_range(flavour, d2_fn(c, n, b), rc, self_, rc2),
                           slab_reach=float(rc) * 1.01 + 0.05 if slab else None)


def reuse_edges(pos_build, pos_now, box, rc, skin, flavour, radius, n_boxes=1):
    """A reuse step on wrapped positions: the candidates are the pairs in range of `radius` (float32) at pos_build, the
    exact filter runs over them at pos_now.  Returns (edges [2, E], rebuilt): when any atom counts as moved the device
    rebuilds, and the edges are the exact search's."""
    pos_build, pos_now = _f(pos_build), _f(pos_now)
    b3 = box3(box, n_boxes)
    npb = pos_now.shape[0] // n_boxes
    per_atom_box = np.repeat(b3, npb, axis=0)
    if bool(np.any(moved_beyond(pos_now, pos_build, per_atom_box, skin))):
        return edges(pos_now, box, rc, flavour, n_boxes), True
    radius = F(radius)
    r2 = F(float(radius) * float(radius))
    cand = pair_mask_edges(pos_build, box, n_boxes, lambda c, n, b, self_: in_range(flavour, d2(c, n, b), radius, self_, r2))
    keep = in_range(flavour, d2(pos_now[cand[0]], pos_now[cand[1]], per_atom_box[cand[0]]), rc, cand[0] == cand[1])
    return cand[:, keep], False


def cutoff_gap64(pos, box, rc, n_boxes=1, window=TIE_WINDOW_DEFAULT):
    """Float64 classification of the directed pairs (i != j, same box) with |d64 - rc| < window, d64 the float64
    minimum-image distance of the float32 positions: (pairs [2, k], gap [k], inside64 [k]).  It only counts how many pairs
    of a fixture sit on the cutoff, and how a float64 search would decide them."""
    pos = np.asarray(pos, dtype=np.float64)
    b3 = box3(box, n_boxes).astype(np.float64)
    npb = pos.shape[0] // n_boxes
    assert window <= 1.0
    P, G, I = [np.zeros((2, 0), dtype=np.int64)], [np.zeros(0)], [np.zeros(0, dtype=bool)]
    for b in range(n_boxes):
        p = pos[b * npb:(b + 1) * npb]
        for rows, cols in _blocks(p, b3[b], rc + window + 0.05, 64):
            r = p[rows][:, None, :] - p[cols][None, :, :]
            r -= b3[b] * np.round(r / b3[b])
            d = np.sqrt((r * r).sum(-1))
            gap = np.abs(d - rc)
            i, j = np.nonzero((gap < window) & (rows[:, None] != cols[None, :]))
            P.append(np.stack([rows[i] + b * npb, cols[j] + b * npb]))
            G.append(gap[i, j])
            I.append(d[i, j] < rc)
    return np.concatenate(P, axis=1), np.concatenate(G), np.concatenate(I)


def edge_keys(e, n):
    """Sorted int64 keys centre * n + neighbour of an edge list [2, E]."""
    e = np.asarray(e).astype(np.int64)
    return np.sort(e[0] * n + e[1])
