// cell_table.hip — the per-box cell table under the classical potentials' pair passes: ONE builder for
// every walk over it (water_cells.hip, classical_cells.hip).  Positions are the caller's as they are given, never wrapped: the
// fp32 atoms widened, or doubles (the minimiser's x64, the M-site pass's charge sites).  Per box nx x ny x nz cells
// (gamd_cells_dev.h: cells per axis, cell of a coordinate), cell = (cx ny + cy) nz + cz.  Five launches (launch_cell_table):
//
//   k_celltab_clear   one thread per cell: the counts and the fill cursors to zero.  They are the only buffers updated in place, so
//                     they are cleared at the head of EVERY evaluation: a sample that runs twice writes the same bits twice.
//   k_celltab_count   one thread per atom: its cell to cell_of, one integer atomicAdd on the cell's count.
//   k_celltab_scan    one workgroup per box: the exclusive scan of the counts in place — thread t sums its run of ceil(cells / 256)
//                     cells, the 256 sums are scanned in LDS, the thread writes its run's prefixes; start[cells] = the atoms.
//   k_celltab_fill    one thread per atom: slot start[cell] + atomicAdd(fill[cell], 1) of `members` takes the atom.  Which atom of a
//                     cell gets which slot depends on the arrival order; what the cell's run of slots holds as a SET does not.
//   k_celltab_rank    one thread per atom: its rank is the number of members of its cell with a lower atom index (a count over the
//                     cell's run: O(occupancy) whatever the positions are, no sort), its slot start[cell] + rank; `order` and the
//                     table entry {position, atom, O flag} of that slot.  The table is ordered by (cell, atom index): reproducible.
// No floating-point arithmetic on what is stored but the cell of a coordinate; integer atomics only.  Every kernel returns while
// DEVFLAG_FROZEN is set and for a box whose gate `stopped` is set.  Checked build: an atom's cell, a cell's start and a slot pass
// through GAMD_CHK_RANGE under the caller's codes chk, chk + 1, chk + 2 before they are used as addresses.  A box whose cells
// exceed the tables' room (the host sizes them from the same boxes by the same function; cannot happen) is left alone.
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_passes_dev.h"

namespace {

// a frame that will be evaluated again, or a box whose positions stay
__device__ __forceinline__ bool celltab_gated(const CellTabArgs& k, int box) {
    return k.devflags[DEVFLAG_FROZEN] || (k.stopped && k.stopped[box]);
}

// atom i (all boxes) as the walk reads it
__device__ __forceinline__ void celltab_load(const CellTabArgs& k, size_t i, double& px, double& py, double& pz) {
    if (k.x64) GamdPosF64{k.x64}.load(i, px, py, pz);
    else GamdPosF32{k.x}.load(i, px, py, pz);
}

__global__ void __launch_bounds__(256) k_celltab_clear(CellTabArgs k) {
    const int box = blockIdx.y;
    if (celltab_gated(k, box)) return;
    const CellTabGeom g = gamd_celltab_geom(k, k.c, box);
    if (!g.ok) return;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c <= g.cells) k.c.start[(size_t)box * ((size_t)k.c.cap + 1) + (size_t)c] = 0;
    if (c < g.cells) k.c.fill[(size_t)box * (size_t)k.c.cap + (size_t)c] = 0;
}

__global__ void __launch_bounds__(256) k_celltab_count(CellTabArgs k) {
    const int box = blockIdx.y, npb = gamd_npb(k);
    if (celltab_gated(k, box)) return;
    const CellTabGeom g = gamd_celltab_geom(k, k.c, box);
    const int il = blockIdx.x * 256 + threadIdx.x;          // one thread per atom
    if (!g.ok || il >= npb) return;
    const size_t i = (size_t)box * (size_t)npb + (size_t)il;
    double px, py, pz;
    celltab_load(k, i, px, py, pz);
    const int cx = gamd_cells_index(px, gamd_box_edge(k, box, 0), g.nx), cy = gamd_cells_index(py, gamd_box_edge(k, box, 1), g.ny),
              cz = gamd_cells_index(pz, gamd_box_edge(k, box, 2), g.nz);
    const int c = (cx * g.ny + cy) * g.nz + cz;             // in [0, cells): every factor is in its range for every bit pattern
    k.c.cell_of[i] = c;
    atomicAdd(k.c.start + (size_t)box * ((size_t)k.c.cap + 1) + (size_t)c, 1);
}

__global__ void __launch_bounds__(256) k_celltab_scan(CellTabArgs k) {
    __shared__ int sums[256];
    const int box = blockIdx.x, tid = threadIdx.x;
    if (celltab_gated(k, box)) return;                      // (uniform)
    const CellTabGeom g = gamd_celltab_geom(k, k.c, box);
    if (!g.ok) return;                                      // (uniform)
    int* start = k.c.start + (size_t)box * ((size_t)k.c.cap + 1);
    const int run = (g.cells + 255) / 256;
    const int c0 = tid * run < g.cells ? tid * run : g.cells, c1 = c0 + run < g.cells ? c0 + run : g.cells;
    int s = 0;
    for (int c = c0; c < c1; ++c) s += start[c];
    sums[tid] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                     // inclusive scan of the 256 sums
        const int v = tid >= d ? sums[tid - d] : 0;
        __syncthreads();
        sums[tid] += v;
        __syncthreads();
    }
    int at = sums[tid] - s;                                 // the atoms in front of this thread's run
    for (int c = c0; c < c1; ++c) {
        const int m = start[c];
        start[c] = at;
        at += m;
    }
    if (tid == 255) start[g.cells] = sums[255];
}

__global__ void __launch_bounds__(256) k_celltab_fill(CellTabArgs k) {
    const int box = blockIdx.y, npb = gamd_npb(k);
    if (celltab_gated(k, box)) return;
    const CellTabGeom g = gamd_celltab_geom(k, k.c, box);
    const int il = blockIdx.x * 256 + threadIdx.x;          // one thread per atom
    if (!g.ok || il >= npb) return;
    const size_t a0 = (size_t)box * (size_t)npb;
    const int c = GAMD_CHK_RANGE(k.c.sticky, k.c.cell_of[a0 + (size_t)il], 0, g.cells - 1, k.chk);
    const int s0 = GAMD_CHK_RANGE(k.c.sticky, k.c.start[(size_t)box * ((size_t)k.c.cap + 1) + (size_t)c], 0, npb, k.chk + 1);
    const int m = atomicAdd(k.c.fill + (size_t)box * (size_t)k.c.cap + (size_t)c, 1);
    const int slot = GAMD_CHK_RANGE(k.c.sticky, s0 + m, 0, npb - 1, k.chk + 2);
    k.c.members[a0 + (size_t)slot] = il;
}

__global__ void __launch_bounds__(256) k_celltab_rank(CellTabArgs k) {
    const int box = blockIdx.y, npb = gamd_npb(k);
    if (celltab_gated(k, box)) return;
    const CellTabGeom g = gamd_celltab_geom(k, k.c, box);
    const int il = blockIdx.x * 256 + threadIdx.x;          // one thread per atom
    if (!g.ok || il >= npb) return;
    const size_t a0 = (size_t)box * (size_t)npb;
    const int* start = k.c.start + (size_t)box * ((size_t)k.c.cap + 1);
    const int c = GAMD_CHK_RANGE(k.c.sticky, k.c.cell_of[a0 + (size_t)il], 0, g.cells - 1, k.chk);
    const int s0 = GAMD_CHK_RANGE(k.c.sticky, start[c], 0, npb, k.chk + 1);
    const int s1 = GAMD_CHK_RANGE(k.c.sticky, start[c + 1], 0, npb, k.chk + 1);
    int rank = 0;
    for (int s = s0; s < s1; ++s) rank += k.c.members[a0 + (size_t)s] < il ? 1 : 0;
    const int slot = GAMD_CHK_RANGE(k.c.sticky, s0 + rank, 0, npb - 1, k.chk + 2);
    k.c.order[a0 + (size_t)slot] = il;
    CellTabAtom t;
    celltab_load(k, a0 + (size_t)il, t.x, t.y, t.z);
    t.idx = il; t.o = k.species && k.species[a0 + (size_t)il] != 0 ? 1 : 0;
    k.c.table[a0 + (size_t)slot] = t;
}

}  // namespace

int launch_cell_table(const CellTabArgs& k, hipStream_t st) {
    const CellTabBufs& c = k.c;
    if ((!k.x && !k.x64) || !k.devflags) return -1;
    if (c.cap < 1 || c.cap > GAMD_CELLS_MAX * GAMD_CELLS_MAX * GAMD_CELLS_MAX || !(c.r_cut > 0.0)) return -1;
    if (!c.start || !c.fill || !c.cell_of || !c.members || !c.order || !c.table) return -1;
    const int nb = k.bx.n_boxes > 1 ? k.bx.n_boxes : 1, npb = k.bx.n_boxes > 1 ? k.bx.n_per_box : k.n;   // (the caller's pass_rows passed)
    const dim3 atoms((unsigned)((npb + 255) / 256), nb), b256(256);
    hipLaunchKernelGGL(k_celltab_clear, dim3((unsigned)((c.cap + 1 + 255) / 256), nb), b256, 0, st, k); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_celltab_count, atoms, b256, 0, st, k); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_celltab_scan, dim3(nb), b256, 0, st, k); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_celltab_fill, atoms, b256, 0, st, k); GAMD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_celltab_rank, atoms, b256, 0, st, k); GAMD_CHECK_LAUNCH();
    return 0;
}
