// classical_cells.hip — the pairs of the Lennard-Jones classical potential over a cell table (gamd_classical_cells, DESIGN.md
// section 4.9.1): a second producer of the pair rows `part`.  The kernels behind them (k_classical_atoms, k_classical_final,
// k_drive_lj_atoms, k_min_atoms, k_min_update) are launched as they are, on an argument block with ONE pair slice.  Positions
// are the consumer's — the fp32 atoms widened (the observer, gamd_classical_eval, the force source) or the minimiser's x64 — as
// they are given, never wrapped: a pair's d, minimum image and r^2 come from the same operations on the same two doubles as in
// gamd_lj_walk (gamd_passes_dev.h), so the set of pairs and the pair count are the all-pairs walk's by construction.
// Per box nx x ny x nz cells (gamd_cells_dev.h: cells per axis, cell of a coordinate, neighbour lists), cell = (cx ny + cy) nz + cz.
// The table — the box's atoms ordered by (cell, atom index), entries {x, y, z, atom index} and an O flag of 0 — is
// cell_table.hip's, built by launch_cell_table in front of the pair pass of every evaluation.
//
//   k_ljcell_pairs  the pair pass with every accumulator {Fx, Fy, Fz, e_i, w_i, pairs_i} (the observer, gamd_classical_eval)
//   k_ljcell_force  ... the force accumulators only (the force source, the minimiser's final force)
//   k_ljcell_min    ... {Fx, Fy, Fz, e_i} (an iteration of the minimiser, whose table was built from x64)
//                   256 threads: 32 consecutive table slots, LJCELL_LANES = 8 lanes per slot.  z is the table's innermost axis,
//                   so under one (x entry, y entry) of the neighbour lists the z entries' cells are ONE run of table slots — two
//                   when the z window wraps (the list's order: the run that ends at the axis' last cell first), the whole z line
//                   when nz < 5.  An atom has span_x span_y <= 25 such columns, q = (x entry) span_y + (y entry); lane l takes the
//                   columns q = l, l + 8, l + 16, ... in that order, a column's runs in list order, a run by table slot, and adds
//                   every term to its own partial row starting from zero; the atom itself is skipped by index.  The run
//                   boundaries are four loads of `start` per column, sixteen per lane (a lane without a fourth column loads column
//                   0's and drops them), all issued in front of the walk; a run is read four entries
//                   at a time (the loads of a batch are in flight together: the pass is bound by their latency, not by their
//                   number), and the terms of a batch are added in slot order.  The eight partial rows p_l meet by the fixed
//                   xor tree of k_pme_gather: ((p0 + p4) + (p2 + p6)) + ((p1 + p5) + (p3 + p7)), stored by lane 0.
//                   The body is gamd_lj_walk's statement for statement.  All three variants add the same force terms in the
//                   same order: a driven frame's force is fp32(f_cl of gamd_classical_eval) bit for bit, and so is the
//                   minimiser's f.
// No floating-point atomics; fixed slot-to-lane and column-to-lane assignment; contraction off: the same bits run after run.
// Every kernel returns while DEVFLAG_FROZEN is set, and for a box the minimiser has stopped.  Checked build: an atom's cell, a
// cell's start and a table entry's atom index pass through GAMD_CHK_RANGE before they are used as addresses.  A box whose cells
// exceed the tables' room (the host sizes them from the same boxes by the same function; cannot happen) is left alone by every
// kernel.
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_passes_dev.h"

namespace {

constexpr int LJCELL_LANES = 8;                                 // lanes of a table slot in the pair pass
constexpr int LJCELL_SLOTS = 256 / LJCELL_LANES;                // table slots of a workgroup
constexpr int LJCELL_ENTRIES = 2 * GAMD_CELLS_REACH + 1;        // entries of an axis' neighbour list at the most
constexpr int LJCELL_COLS = (LJCELL_ENTRIES * LJCELL_ENTRIES + LJCELL_LANES - 1) / LJCELL_LANES;    // columns of a lane at the most
constexpr int LJCELL_BATCH = 4;                                 // table entries in flight per lane

struct LjCellArgs {
    ClassicalArgs a;
    CellTabBufs c;
    const int* stopped;        // [n_boxes] the minimiser's gates, or null
};

// a frame that will be evaluated again, or a box whose positions stay
__device__ __forceinline__ bool ljcell_gated(const LjCellArgs& k, int box) {
    if (k.a.devflags[DEVFLAG_FROZEN]) return true;
    return k.stopped && k.stopped[box] != 0;
}

// a table entry in one 32-byte load: {x, y, z} and, in the low half of the fourth double, the atom inside its box
static_assert(sizeof(CellTabAtom) == sizeof(double4) && offsetof(CellTabAtom, idx) == 3 * sizeof(double), "a table entry is read as a double4");
__device__ __forceinline__ int ljcell_idx(const double4& t) { return (int)(unsigned)(unsigned long long)__double_as_longlong(t.w); }

template <int NOUT>
__device__ __forceinline__ void ljcell_walk(const LjCellArgs& k) {
    static_assert(NOUT == 3 || NOUT == 4 || NOUT == CLASSICAL_PART, "forces; + e_i; + w_i and pairs_i");
    const ClassicalArgs& a = k.a;
    const int l = threadIdx.x & (LJCELL_LANES - 1);
    const int box = blockIdx.y, npb = gamd_npb(a);
    const size_t a0 = (size_t)box * (size_t)npb;            // the caller's order is box-major
    const CellTabGeom g = gamd_celltab_geom(k.a, k.c, box);
    if (!g.ok) return;                                      // (uniform)
    const int sl = blockIdx.x * LJCELL_SLOTS + (int)(threadIdx.x / LJCELL_LANES);
    const bool vi = sl < npb;
    const int slot = vi ? sl : npb - 1;                     // a lane behind the last slot has no columns and stores nothing
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    const int* start = k.c.start + (size_t)box * ((size_t)k.c.cap + 1);
    const double4* table = reinterpret_cast<const double4*>(k.c.table + a0);
    const double4 me = table[slot];
    const int il = GAMD_CHK_RANGE(k.c.sticky, ljcell_idx(me), 0, npb - 1, GAMD_CHK_LJCELL_ATOM);
    const double xi = me.x, yi = me.y, zi = me.z;
    const int cell = GAMD_CHK_RANGE(k.c.sticky, k.c.cell_of[a0 + (size_t)il], 0, g.cells - 1, GAMD_CHK_LJCELL_CELL);
    const int cx = cell / (g.ny * g.nz), cy = (cell / g.nz) % g.ny, cz = cell % g.nz;
    const int span_y = gamd_cells_span(g.ny);
    const int ncols = vi ? gamd_cells_span(g.nx) * span_y : 0;
    // the z entries' cells of a column as cell runs [za0, za1) then [zb0, zb1) in the neighbour list's order
    int za0 = 0, za1 = g.nz, zb1 = 0;                       // fewer than five cells: the whole line (zb0 = 0 always)
    if (g.nz >= LJCELL_ENTRIES) {
        const int lo = cz - GAMD_CELLS_REACH, hi = cz + GAMD_CELLS_REACH;
        if (lo < 0) { za0 = lo + g.nz; zb1 = hi + 1; }      // ... the window wraps below: the cells lo + nz .. nz - 1, then 0 .. hi
        else if (hi >= g.nz) { za0 = lo; zb1 = hi - g.nz + 1; }     // ... above: lo .. nz - 1, then 0 .. hi - nz
        else { za0 = lo; za1 = hi + 1; }
    }
    // the run boundaries of the lane's columns, all in flight in front of the walk
    int r0[LJCELL_COLS][2], r1[LJCELL_COLS][2];
#pragma unroll
    for (int c = 0; c < LJCELL_COLS; ++c) {
        const int q = l + c * LJCELL_LANES;
        const bool vq = q < ncols;
        const int qq = vq ? q : 0;
        const int jx = qq / span_y, jy = qq - jx * span_y;
        const int cb = (gamd_cells_neighbour(cx, jx, g.nx) * g.ny + gamd_cells_neighbour(cy, jy, g.ny)) * g.nz;     // the column's first cell
        const int sa0 = GAMD_CHK_RANGE(k.c.sticky, start[cb + za0], 0, npb, GAMD_CHK_LJCELL_START);
        const int sa1 = GAMD_CHK_RANGE(k.c.sticky, start[cb + za1], 0, npb, GAMD_CHK_LJCELL_START);
        const int sb0 = GAMD_CHK_RANGE(k.c.sticky, start[cb], 0, npb, GAMD_CHK_LJCELL_START);
        const int sb1 = GAMD_CHK_RANGE(k.c.sticky, start[cb + zb1], 0, npb, GAMD_CHK_LJCELL_START);
        r0[c][0] = sa0; r1[c][0] = vq ? sa1 : sa0;
        r0[c][1] = sb0; r1[c][1] = vq ? sb1 : sb0;
    }
    double fx = 0.0, fy = 0.0, fz = 0.0, e = 0.0, w = 0.0, cnt = 0.0;
#pragma unroll
    for (int c = 0; c < LJCELL_COLS; ++c) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int s1 = r1[c][h];
            for (int s = r0[c][h]; s < s1; s += LJCELL_BATCH) {
                double4 t[LJCELL_BATCH];
#pragma unroll
                for (int u = 0; u < LJCELL_BATCH; ++u) t[u] = table[s + u < s1 ? s + u : s1 - 1];
#pragma unroll
                for (int u = 0; u < LJCELL_BATCH; ++u) {
                    // gamd_lj_walk's body (gamd_passes_dev.h), statement for statement
                    double dx = xi - t[u].x, dy = yi - t[u].y, dz = zi - t[u].z;
                    dx = dx - Lx * rint(dx / Lx);
                    dy = dy - Ly * rint(dy / Ly);
                    dz = dz - Lz * rint(dz / Lz);
                    const double r2 = (dx * dx + dy * dy) + dz * dz;
                    if (s + u >= s1 || ljcell_idx(t[u]) == il || !(r2 < a.rc2)) continue;
                    const double ir2 = 1.0 / r2;
                    const double2 lj = gamd_lj_pair_r2(a, a.eps24, ir2, r2);   // (u, r u'(r)), u = (u_LJ - u0) S
                    const double fs = -(lj.y * ir2);        // F_ij = -u'(r) d / r = fs d
                    fx += fs * dx; fy += fs * dy; fz += fs * dz;
                    if constexpr (NOUT >= 4) e += lj.x;
                    if constexpr (NOUT >= 6) {
                        w += -lj.y;                         // d . F_ij = -r u'(r)
                        cnt += 1.0;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int d = LJCELL_LANES / 2; d >= 1; d >>= 1) {       // (every lane of the wave is here)
        fx += __shfl_xor(fx, d, 64); fy += __shfl_xor(fy, d, 64); fz += __shfl_xor(fz, d, 64);
        if constexpr (NOUT >= 4) e += __shfl_xor(e, d, 64);
        if constexpr (NOUT >= 6) { w += __shfl_xor(w, d, 64); cnt += __shfl_xor(cnt, d, 64); }
    }
    if (vi && l == 0) {
        double* out = a.part + (a0 + (size_t)il) * CLASSICAL_PART;      // one pair slice: the box's rows
        out[0] = fx; out[1] = fy; out[2] = fz;
        if constexpr (NOUT >= 4) out[3] = e;
        if constexpr (NOUT >= 6) { out[4] = w; out[5] = cnt; }
    }
}

__global__ void __launch_bounds__(256) k_ljcell_pairs(LjCellArgs k) {
    if (ljcell_gated(k, blockIdx.y)) return;
    ljcell_walk<CLASSICAL_PART>(k);
}
__global__ void __launch_bounds__(256) k_ljcell_force(LjCellArgs k) {
    if (ljcell_gated(k, blockIdx.y)) return;
    ljcell_walk<3>(k);
}
__global__ void __launch_bounds__(256) k_ljcell_min(LjCellArgs k) {
    if (ljcell_gated(k, blockIdx.y)) return;
    ljcell_walk<4>(k);
}

}  // namespace

int launch_classical_cells(const ClassicalArgs& a, const CellTabBufs& c, const double* x64, const int* stopped, int nout, hipStream_t st) {
    PassGeom g;
    if (pass_rows(a, 1, &g) || a.slices != 1 || (nout != 3 && nout != 4 && nout != CLASSICAL_PART)) return -1;
    if ((!a.x && !x64) || !a.part || !a.devflags) return -1;
    if (((long long)g.npb + LJCELL_SLOTS - 1) / LJCELL_SLOTS > 0x7fffffll) return -1;
    if (int r = launch_cell_table(cell_tab_args(a, c, stopped, x64, nullptr, GAMD_CHK_LJCELL_CELL), st)) return r;
    const LjCellArgs k{a, c, stopped};
    const dim3 pg((unsigned)((g.npb + LJCELL_SLOTS - 1) / LJCELL_SLOTS), g.nb), b256(256);
    if (nout == 3) hipLaunchKernelGGL(k_ljcell_force, pg, b256, 0, st, k);
    else if (nout == 4) hipLaunchKernelGGL(k_ljcell_min, pg, b256, 0, st, k);
    else hipLaunchKernelGGL(k_ljcell_pairs, pg, b256, 0, st, k);
    GAMD_CHECK_LAUNCH();
    return 0;
}
