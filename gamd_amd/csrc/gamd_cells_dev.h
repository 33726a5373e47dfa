// gamd_cells_dev.h — what the cell-table kernels of the classical potentials (the builder cell_table.hip and the walks
// water_cells.hip and classical_cells.hip) share with the host and with a plain C++ compiler: the cells
// per axis and per box, the cell of a coordinate, and the neighbour cells of a cell along one axis.  No ROCm header is needed to
// include it: a stand-alone host program (tools/cells_host_check.cpp) calls every function here under the address and
// undefined-behaviour sanitizers.
//
// Reach.  R = 2: a cell's edge is at least r_cut / 2, and a pair inside the cutoff lies at most two cells apart along every
// axis.  The 5^3 = 125 cells of that size cover 15.6 r_cut^3 against the sphere's 4.2 r_cut^3; R = 1 (27 cells of edge r_cut)
// would cover 27 r_cut^3.
//
// Cells per axis.  nc = min(floor(2 L / (r_cut (1 + 2^-20))), 64), from the box's OWN edge (the fp32 edge widened) and r_cut in
// double, by gamd_cells_per_axis wherever it is needed — host and device take the same operations in the same order.  The
// margin 2^-20 is there for the rounding of the cell index: two coordinates whose computed minimum-image distance is below
// r_cut have u = s nc (below) less than 2 / (1 + 2^-20) + a few 1e-14 apart, so their floors differ by two at most.  The cap of
// 64 only makes cells larger.  2 r_cut <= L (the potential's own condition) gives nc >= 3; an edge or a cutoff that is not a
// positive finite number gives nc = 1, so every count below stays a positive int.
//
// Cell of a coordinate.  gamd_pme_index's arithmetic: s = x / L - floor(x / L), u = s nc, cell = floor(u) — in [0, nc) for EVERY
// bit pattern of x: a negative x a rounding below zero gives s = 1 exactly, which is the image s = 0 and is cell 0; exact
// multiples of L give cell 0; 1e30 is finite, x / L is an integer-valued double and s = 0; NaN and the infinities give u = NaN
// and cell 0.
//
// Neighbour cells along one axis.  gamd_cells_span(nc) of them: 5 when nc >= 5, else nc.  gamd_cells_neighbour(c, j, nc), j in
// [0, span): with nc >= 5 the cell c + (j - 2) wrapped into [0, nc) — the offsets -2, -1, 0, +1, +2 in that order; with nc < 5
// the cell j — every cell of the axis once, in ascending order.  No cell comes twice.  A cell's neighbours in three dimensions
// are the product of the three axes' lists, x outermost and z innermost.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GAMD_CELLS_HD __host__ __device__ __forceinline__
#else
#define GAMD_CELLS_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

constexpr int GAMD_CELLS_REACH = 2;                         // R
constexpr int GAMD_CELLS_MAX = 64;                          // cells per axis at the most
constexpr double GAMD_CELLS_MARGIN = 1.0 + 1.0 / 1048576.0; // 1 + 2^-20

// cells along an axis of edge L under the cutoff r_cut (see "Cells per axis"): in [1, 64]
GAMD_CELLS_HD int gamd_cells_per_axis(double L, double r_cut) {
    const double v = floor((2.0 * L) / (r_cut * GAMD_CELLS_MARGIN));
    if (!(v >= 1.0)) return 1;                              // a ratio below 1, or not a number
    return v < (double)GAMD_CELLS_MAX ? (int)v : GAMD_CELLS_MAX;
}

// cells of a box with the edges Lx, Ly, Lz: nc = the three axes' gamd_cells_per_axis, returned their product, in [1, 64^3]
GAMD_CELLS_HD int gamd_cells_count(double Lx, double Ly, double Lz, double r_cut, int nc[3]) {
    nc[0] = gamd_cells_per_axis(Lx, r_cut); nc[1] = gamd_cells_per_axis(Ly, r_cut); nc[2] = gamd_cells_per_axis(Lz, r_cut);
    return (nc[0] * nc[1]) * nc[2];
}

// cell in [0, nc) of coordinate x along an axis of edge L (see "Cell of a coordinate")
GAMD_CELLS_HD int gamd_cells_index(double x, double L, int nc) {
    const double q = x / L;
    const double s = q - floor(q);
    const double u = s * (double)nc;
    if (!(u >= 0.0 && u < (double)nc)) return 0;            // s == 1 (the image s = 0), or not a number
    return (int)floor(u);
}

// how many cells of an axis of nc cells a cell's neighbour list visits
GAMD_CELLS_HD int gamd_cells_span(int nc) { return nc >= 2 * GAMD_CELLS_REACH + 1 ? 2 * GAMD_CELLS_REACH + 1 : nc; }

// entry j (0 <= j < gamd_cells_span(nc)) of the neighbour list of cell c (0 <= c < nc) along an axis of nc cells
GAMD_CELLS_HD int gamd_cells_neighbour(int c, int j, int nc) {
    if (nc < 2 * GAMD_CELLS_REACH + 1) return j;
    const int i = c + j - GAMD_CELLS_REACH;
    return i < 0 ? i + nc : (i >= nc ? i - nc : i);
}
