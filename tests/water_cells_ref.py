"""The cell table of the water classical potential (gamd_water_cells, gamd_amd/csrc/gamd_cells_dev.h and cell_table.hip) restated
in numpy: the header's operations in the header's order, in float64, so that every function agrees with the device bit for bit.

  ncells(box, r_cut)           cells per axis: min(floor(2 L / (r_cut (1 + 2^-20))), 64), at least 1, from the box's fp32 edges widened
  cell_axis(x, L, nc)          s = x / L - floor(x / L), u = s nc, floor(u); 0 where u is outside [0, nc) or not a number
  cell_of(x, box, nc)          (cx ny + cy) nz + cz
  table(x, box, r_cut)         nc, start (cells + 1 offsets) and order (the atoms by lexicographic (cell, index))
  neighbour_axis(c, nc)        the cells of an axis a cell visits, in order: c - 2 .. c + 2 wrapped when nc >= 5, else 0 .. nc - 1
  neighbour_cells(cell, nc)    the product of the three axes' lists, x outermost and z innermost
  charge_sites(x, box, w)      the M-site form's positions as k_w4_sites leaves them: M = O' + w (d_1 + d_2) with O' = O wrapped into
                               [0, L), the hydrogens wrapped into [0, L) (water_msite_ref.sites is the same potential's sites with
                               nothing wrapped: other doubles in another image, which at a cell face is another cell)
  max_cell_distance(...)       the largest per-axis cell distance (wrapped) over the pairs with computed r^2 < r_cut^2, by
                               gamd_water_walk's minimum image on the same doubles
"""
import numpy as np

MARGIN = 1.0 + 2.0 ** -20
MAX_CELLS = 64
REACH = 2


def edges(box):
    b = np.asarray(box, dtype=np.float32).astype(np.float64).reshape(-1)
    return np.repeat(b, 3) if b.size == 1 else b


def ncells(box, r_cut):
    v = np.floor((2.0 * edges(box)) / (float(r_cut) * MARGIN))
    v = np.where(v >= 1.0, v, 1.0)                          # (NaN compares false)
    return np.minimum(v, float(MAX_CELLS)).astype(np.int64)


def cell_axis(x, L, nc):
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.asarray(x, dtype=np.float64) / float(L)
        s = q - np.floor(q)
        u = s * float(nc)
        ok = (u >= 0.0) & (u < float(nc))
        return np.where(ok, np.floor(np.where(ok, u, 0.0)), 0.0).astype(np.int64)


def cell_of(x, box, nc):
    L = edges(box)
    x = np.asarray(x, dtype=np.float64)
    cx, cy, cz = (cell_axis(x[:, d], L[d], nc[d]) for d in range(3))
    return (cx * nc[1] + cy) * nc[2] + cz


def table(x, box, r_cut):
    nc = ncells(box, r_cut)
    cell = cell_of(x, box, nc)
    order = np.argsort(cell, kind="stable")                 # by (cell, atom index)
    start = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=int(nc.prod())))])
    return nc, start.astype(np.int32), order.astype(np.int32)


def neighbour_axis(c, nc):
    if nc < 2 * REACH + 1:
        return list(range(nc))
    return [(c + o) % nc for o in range(-REACH, REACH + 1)]


def neighbour_cells(cell, nc):
    cx, cy, cz = cell // (nc[1] * nc[2]), (cell // nc[2]) % nc[1], cell % nc[2]
    return [(ix * nc[1] + iy) * nc[2] + iz for ix in neighbour_axis(cx, nc[0]) for iy in neighbour_axis(cy, nc[1])
            for iz in neighbour_axis(cz, nc[2])]


def charge_sites(x, box, w):
    L = edges(box)
    xd = np.asarray(x, dtype=np.float64)
    o = xd[0::3]
    d1, d2 = xd[1::3] - o, xd[2::3] - o
    d1 = d1 - L * np.rint(d1 / L)
    d2 = d2 - L * np.rint(d2 / L)
    s = xd - L * np.floor(xd / L)                           # water_wrap
    s[0::3] = s[0::3] + w * (d1 + d2)
    return s


def pairs_inside(x, box, r_cut):
    """[N, N] bool: computed r^2 < r_cut^2 by gamd_water_walk's operations (the diagonal is False)"""
    L = edges(box)
    x = np.asarray(x, dtype=np.float64)
    d = x[:, None, :] - x[None, :, :]
    d = d - L * np.rint(d / L)
    r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    inside = r2 < float(r_cut) * float(r_cut)
    np.fill_diagonal(inside, False)
    return inside


def max_cell_distance(x, box, r_cut):
    nc = ncells(box, r_cut)
    L = edges(box)
    x = np.asarray(x, dtype=np.float64)
    inside = pairs_inside(x, box, r_cut)
    worst = 0
    for d in range(3):
        c = cell_axis(x[:, d], L[d], nc[d])
        dc = np.abs(c[:, None] - c[None, :])
        dc = np.minimum(dc, nc[d] - dc)
        worst = max(worst, int(dc[inside].max()))
    return worst
