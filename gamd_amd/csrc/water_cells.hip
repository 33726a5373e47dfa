// water_cells.hip — the real-space pairs of the water classical potential over a cell table (gamd_water_cells, DESIGN.md section
// 4.10.4): a second producer of the pair rows `part`.  The kernels behind them (k_water_atoms, k_wsrc_atoms, k_w4_atoms,
// k_w4_drive, k_water_final), the reciprocal kernels (plain or particle-mesh), the M-site prepass and k_w4_lj are launched as they
// are, on an argument block with ONE pair slice.  Positions are the fp32 atoms widened (3-site) or the charge sites k_w4_sites
// left (M-site) — or, from the water minimisers under the configured potential (water_relax.hip), their double positions
// (3-site, the O-O term in the walk) or the sites k_wrx_sites left — never wrapped: a pair's d, minimum image and r^2 come from the same operations on the same two doubles as in
// gamd_water_walk (gamd_passes_dev.h), so the set of pairs and the pair count are the all-pairs walk's by construction.
// Per box nx x ny x nz cells (gamd_cells_dev.h: cells per axis, cell of a coordinate, neighbour lists), cell = (cx ny + cy) nz + cz.
// The table — the box's atoms ordered by (cell, atom index), entries {position, atom, O flag} — is cell_table.hip's, built by
// launch_cell_table in front of the pair pass of every evaluation.
//
//   k_wcell_pairs   the pair pass, 3-site, every accumulator (the observer, gamd_water_eval)       384 threads: six waves share
//   k_wcell_force   ... the force accumulators only (the force source)                             64 consecutive table slots,
//   k_wcell_pairs4  the pair pass on the charge sites, Lennard-Jones term off (k_w4_lj's)          lane l of every wave owns slot
//   k_wcell_force4  ... the force accumulators only                                                64 b + l
//                   Wave 1 + e walks entry e of the x axis' neighbour list (gamd_cells_neighbour: offsets -2 .. +2 wrapped, or
//                   every cell of an axis of fewer than five) and under it the y entries in order and under each the z entries
//                   in order; within a cell the table slots in order, that is by atom index; staged atoms of the lane's own
//                   molecule (index / 3) are skipped.  The body is gamd_water_walk's erfc branch statement for statement (gs, fs,
//                   the O-O Lennard-Jones term in the 3-site form).  Same-molecule pairs take the erf branch whatever r is: wave 0
//                   takes the lane's two partners by index from the caller-order positions, the lower index first: the row's
//                   first two terms, m.  (A wave of their own: erf's constants and erfc's in one path spill scalar registers.)
//                   The entries' partial rows meet in LDS (7.5 KiB or 15 KiB) and wave 0 adds them behind m in x-entry order,
//                   (((((m + p_0) + p_1) + p_2) + p_3) + p_4), and stores the atom's row of `part`.  Both variants add the same
//                   terms in the same order: a driven frame's force is fp32(f_cl of gamd_water_eval) bit for bit.
// No floating-point atomics; fixed slot-to-lane and cell-to-wave assignment; contraction off: the same bits run after run.  Every
// kernel returns while DEVFLAG_FROZEN is set.  Checked build: an atom's cell, a cell's start and a table entry's atom index pass
// through GAMD_CHK_RANGE before they are used as addresses.  A box whose cells exceed the tables' room (the host sizes them from
// the same boxes by the same function; cannot happen) is left alone by every kernel.
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_passes_dev.h"

namespace {

constexpr int WCELL_SLOTS = 64;                             // table slots of a workgroup of the pair pass
constexpr int WCELL_ENTRIES = 2 * GAMD_CELLS_REACH + 1;     // entries of an axis' neighbour list at the most
constexpr int WCELL_WAVES = 1 + WCELL_ENTRIES;              // its waves: the molecules' wave and one per entry of the x axis' list

struct WCellArgs {
    WaterArgs w;
    CellTabBufs c;
    const double* sites;       // [n][3] the charge sites k_w4_sites left, or null: the fp32 positions w.x
};

// atom i (all boxes) as the walk reads it
__device__ __forceinline__ void wcell_load(const WCellArgs& k, size_t i, double& px, double& py, double& pz) {
    if (k.sites) GamdPosF64{k.sites}.load(i, px, py, pz);
    else GamdPosF32{k.w.x}.load(i, px, py, pz);
}

// one term of gamd_water_walk's body (gamd_passes_dev.h), statement for statement: the pair's d is (dx, dy, dz) before the
// minimum image.  SAME: the erf branch whatever r is; else the cutoff test, the erfc branch, the count and (LJ) the O-O term.
template <int NOUT, bool LJ, bool SAME>
__device__ __forceinline__ void wcell_term(const WaterArgs& a, double Lx, double Ly, double Lz, double dx, double dy, double dz, double qi,
                                           double q_h, double q_o, bool oi, bool oj, double& fx, double& fy, double& fz, double& elj,
                                           double& ec, double& cnt) {
    dx = dx - Lx * rint(dx / Lx);
    dy = dy - Ly * rint(dy / Ly);
    dz = dz - Lz * rint(dz / Lz);
    const double r2 = (dx * dx + dy * dy) + dz * dz;
    if (!SAME && !(r2 < a.rc2)) return;
    const double qq = a.coul * (qi * (oj ? q_o : q_h));
    const double r = sqrt(r2);
    const double ir2 = 1.0 / r2;
    const double ar = a.alpha * r;
    const double gs = a.two_a_rpi * exp(-(ar * ar));        // -r d/dr of erfc(alpha r), over r
    double fs;
    if constexpr (SAME) {                                   // U_excl: -q_i q_j erf(alpha r) / r
        const double t = erf(ar) / r;
        if constexpr (NOUT >= 6) ec += -(qq * t);
        fs = (qq * (gs - t)) * ir2;
    } else {                                                // U_real: q_i q_j erfc(alpha r) / r
        const double t = erfc(ar) / r;
        if constexpr (NOUT >= 6) ec += qq * t;
        fs = (qq * (t + gs)) * ir2;
        if constexpr (NOUT >= 6) cnt += 1.0;
        if constexpr (LJ) {
            if (oi && oj) {                                 // the Lennard-Jones walk's term
                const double2 lj = gamd_lj_pair_r(a, 6.0 * a.eps4, ir2, r);     // 6 (4 epsilon) = 24 epsilon bit for bit
                if constexpr (NOUT >= 6) elj += lj.x;
                fs = fs + -(lj.y * ir2);
            }
        }
    }
    fx += fs * dx; fy += fs * dy; fz += fs * dz;
}

template <int NOUT, bool LJ>
__device__ __forceinline__ void wcell_walk(const WCellArgs& k) {
    static_assert(NOUT == 3 || NOUT == WATER_PART, "forces; + u_LJ, u_coul and pairs");
    __shared__ double red[WCELL_ENTRIES][NOUT][WCELL_SLOTS];
    const WaterArgs& a = k.w;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // (the wave: uniform)
    const int box = blockIdx.y, npb = gamd_npb(a);
    const size_t a0 = (size_t)box * (size_t)npb;            // the caller's order is box-major
    const CellTabGeom g = gamd_celltab_geom(k.w, k.c, box);
    if (!g.ok) return;                                      // (uniform)
    const bool vi = blockIdx.x * WCELL_SLOTS + lane < npb;
    // a lane behind the last slot walks the last slot's atom again and stores nothing: no branch on vi around the walk, whose
    // saved exec mask would be one more scalar pair alive across erf
    const int slot = vi ? blockIdx.x * WCELL_SLOTS + lane : npb - 1;
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    const int span_x = gamd_cells_span(g.nx);
    int span_y = gamd_cells_span(g.ny), span_z = gamd_cells_span(g.nz), ny = g.ny, nz = g.nz;
    const int* start = k.c.start + (size_t)box * ((size_t)k.c.cap + 1);
    const CellTabAtom* table = k.c.table + a0;
    // the table's and the output rows' addresses and the inner loops' geometry are held in vector registers from here on: left
    // to the compiler they stay in scalar registers across the walk, which the potential's constants and those of erf and erfc
    // fill already (eight scalar spills otherwise)
    double* rows = a.part + a0 * WATER_PART;                 // one pair slice: the box's rows
    asm volatile("" : "+v"(start), "+v"(table), "+v"(span_y), "+v"(span_z), "+v"(ny), "+v"(nz), "+v"(rows));
    const double q_h = a.q_h, q_o = -(q_h + q_h);           // -2 q_h, exact
    double fx = 0.0, fy = 0.0, fz = 0.0, elj = 0.0, ec = 0.0, cnt = 0.0;
    const CellTabAtom me = table[slot];
    const int il = GAMD_CHK_RANGE(k.c.sticky, me.idx, 0, npb - 1, GAMD_CHK_WCELL_ATOM);
    const double xi = me.x, yi = me.y, zi = me.z;
    const bool oi = me.o != 0;
    const double qi = oi ? q_o : q_h;
    const int mi = il / 3;                                  // npb is a multiple of 3: molecules do not straddle boxes
    if (wv == 0) {                                          // the molecule's other two atoms, the lower index first
        for (int q = 0; q < 3; ++q) {
            const int jl = 3 * mi + q;
            if (jl == il) continue;
            double xj, yj, zj;
            wcell_load(k, a0 + (size_t)jl, xj, yj, zj);
            const bool oj = a.species[a0 + (size_t)jl] != 0;
            wcell_term<NOUT, LJ, true>(a, Lx, Ly, Lz, xi - xj, yi - yj, zi - zj, qi, q_h, q_o, oi, oj, fx, fy, fz, elj, ec, cnt);
        }
    } else if (wv <= span_x) {                              // entry wv - 1 of the x axis' list
        const int cell = GAMD_CHK_RANGE(k.c.sticky, k.c.cell_of[a0 + (size_t)il], 0, g.cells - 1, GAMD_CHK_WCELL_CELL);
        const int cx = cell / (ny * nz), cy = (cell / nz) % ny, cz = cell % nz;
        const int ix = gamd_cells_neighbour(cx, wv - 1, g.nx);
        for (int jy = 0; jy < span_y; ++jy) {
            const int iy = gamd_cells_neighbour(cy, jy, ny);
            for (int jz = 0; jz < span_z; ++jz) {
                const int iz = gamd_cells_neighbour(cz, jz, nz);
                const int c2 = (ix * ny + iy) * nz + iz;
                const int s0 = GAMD_CHK_RANGE(k.c.sticky, start[c2], 0, npb, GAMD_CHK_WCELL_START);
                const int s1 = GAMD_CHK_RANGE(k.c.sticky, start[c2 + 1], 0, npb, GAMD_CHK_WCELL_START);
                for (int s = s0; s < s1; ++s) {
                    const CellTabAtom t = table[s];
                    if (t.idx / 3 == mi) continue;          // the atom itself and its molecule: wave 0's
                    wcell_term<NOUT, LJ, false>(a, Lx, Ly, Lz, xi - t.x, yi - t.y, zi - t.z, qi, q_h, q_o, oi, t.o != 0, fx, fy, fz, elj,
                                                ec, cnt);
                }
            }
        }
    }
    if (wv > 0) {
        red[wv - 1][0][lane] = fx; red[wv - 1][1][lane] = fy; red[wv - 1][2][lane] = fz;
        if constexpr (NOUT >= 6) { red[wv - 1][3][lane] = elj; red[wv - 1][4][lane] = ec; red[wv - 1][5][lane] = cnt; }
    }
    __syncthreads();
    if (wv == 0 && vi) {
        for (int w = 0; w < span_x; ++w) {                  // behind the molecule's terms the partial rows in x-entry order
            fx += red[w][0][lane]; fy += red[w][1][lane]; fz += red[w][2][lane];
            if constexpr (NOUT >= 6) { elj += red[w][3][lane]; ec += red[w][4][lane]; cnt += red[w][5][lane]; }
        }
        double* out = rows + (size_t)il * WATER_PART;
        out[0] = fx; out[1] = fy; out[2] = fz;
        if constexpr (NOUT >= 6) { out[3] = LJ ? elj : 0.0; out[4] = ec; out[5] = cnt; }
    }
}

__global__ void __launch_bounds__(WCELL_SLOTS * WCELL_WAVES) k_wcell_pairs(WCellArgs k) {
    if (k.w.devflags[DEVFLAG_FROZEN]) return;               // a frame that will be evaluated again
    wcell_walk<WATER_PART, true>(k);
}
__global__ void __launch_bounds__(WCELL_SLOTS * WCELL_WAVES) k_wcell_force(WCellArgs k) {
    if (k.w.devflags[DEVFLAG_FROZEN]) return;
    wcell_walk<3, true>(k);
}
__global__ void __launch_bounds__(WCELL_SLOTS * WCELL_WAVES) k_wcell_pairs4(WCellArgs k) {
    if (k.w.devflags[DEVFLAG_FROZEN]) return;
    wcell_walk<WATER_PART, false>(k);                       // u_LJ: k_w4_lj's
}
__global__ void __launch_bounds__(WCELL_SLOTS * WCELL_WAVES) k_wcell_force4(WCellArgs k) {
    if (k.w.devflags[DEVFLAG_FROZEN]) return;
    wcell_walk<3, false>(k);
}

}  // namespace

int launch_water_cells(const WaterArgs& w, const CellTabBufs& c, const double* sites, int nout, bool lj, hipStream_t st) {
    PassGeom g;
    // (lj with sites: the 3-site walk on a minimiser's double positions, water_relax.hip; the M-site form has no other positions)
    if (pass_rows(w, 3, &g) || w.slices != 1 || (nout != 3 && nout != WATER_PART) || (!lj && !sites)) return -1;
    if (!(sites || w.x) || !w.species || !w.part || !w.devflags) return -1;
    if (int r = launch_cell_table(cell_tab_args(w, c, nullptr, sites, w.species, GAMD_CHK_WCELL_CELL), st)) return r;
    const WCellArgs k{w, c, sites};
    const dim3 pg((unsigned)((g.npb + WCELL_SLOTS - 1) / WCELL_SLOTS), g.nb), pb(WCELL_SLOTS * WCELL_WAVES);
    if (lj) {
        if (nout == 3) hipLaunchKernelGGL(k_wcell_force, pg, pb, 0, st, k); else hipLaunchKernelGGL(k_wcell_pairs, pg, pb, 0, st, k);
    } else {
        if (nout == 3) hipLaunchKernelGGL(k_wcell_force4, pg, pb, 0, st, k); else hipLaunchKernelGGL(k_wcell_pairs4, pg, pb, 0, st, k);
    }
    GAMD_CHECK_LAUNCH();
    return 0;
}
