// gamd_passes_dev.h — the ONE body of every pass the classical potentials' consumers share (DESIGN.md sections 4.9 - 4.13): the
// Lennard-Jones tile walk (classical.hip, drive.hip), the water tile walk (water_classical.hip, water_drive.hip,
// water_msite.hip; water_virial.hip with the virial's accumulators), the rho(k) pass (water_classical.hip, water_minimize.hip, water_msite.hip), the reciprocal force pass
// (water_classical.hip, water_msite.hip), and FIRE's scalar part (minimize.hip, water_minimize.hip).  A kernel is its gate plus
// one call; what it chooses is a compile-time parameter: where positions come from (a loader below), which accumulators it
// keeps (NOUT), whether the O-O Lennard-Jones term is in the water walk.  Three kernels of the minimisers measured slower on
// these bodies than with the same text in the kernel and carry it written out, each saying so: k_min_pairs (minimize.hip),
// k_wmin_pairs and k_wmin_recip (water_minimize.hip).  The bit-for-bit contracts between the
// consumers (f == fp32(f_cl) on every driven frame, w_h = 0 equal to the 3-site potential, the minimisers' forces equal to the
// force sources') hold because there is one expression tree, not because copies agree.  Contraction is off from here on.
#pragma once
#include "gamd_common.h"
#include "gamd_internal.h"
#include "gamd_potential_dev.h"
#include "gamd_cells_dev.h"

#pragma clang fp contract(off)

constexpr int GAMD_PASS_TILE = 256;                         // atoms of a row tile, atoms and k-vectors of an LDS stage

// ---- position loaders: atom i of the caller's order as three doubles ------------------------------------------------
struct GamdPosF32 {                                         // fp32 positions, widened (exact)
    const float* x;
    __device__ __forceinline__ void load(size_t i, double& px, double& py, double& pz) const {
        const float* p = x + 3 * i;
        px = (double)p[0]; py = (double)p[1]; pz = (double)p[2];
    }
};
struct GamdPosF64 {                                         // double positions: a minimiser's x64, the M-site pass's sites
    const double* x;
    __device__ __forceinline__ void load(size_t i, double& px, double& py, double& pz) const {
        const double* p = x + 3 * i;
        px = p[0]; py = p[1]; pz = p[2];
    }
};

template <typename Args>
__device__ __forceinline__ int gamd_npb(const Args& a) { return a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n; }

// ---- the cell table's geometry of a box (cell_table.hip builds the table, water_cells.hip and classical_cells.hip walk it) ----
struct CellTabGeom { int nx, ny, nz, cells; bool ok; };     // ok: the tables have room for the box's cells
template <typename Args>
__device__ __forceinline__ CellTabGeom gamd_celltab_geom(const Args& a, const CellTabBufs& c, int box) {
    int nc[3];
    CellTabGeom g;
    g.cells = gamd_cells_count(gamd_box_edge(a, box, 0), gamd_box_edge(a, box, 1), gamd_box_edge(a, box, 2), c.r_cut, nc);   // <= 64^3
    g.nx = nc[0]; g.ny = nc[1]; g.nz = nc[2];
    g.ok = g.cells <= c.cap;
    return g;
}

// ---- the Lennard-Jones tile walk ------------------------------------------------------------------------------------
// grid (T * slices, boxes), T = 256-atom row tiles per box: workgroup (I, s) keeps atom t of tile I in the registers of thread t
// and walks the atoms [s * chunk, (s + 1) * chunk) of the box, staged 256 at a time in LDS as doubles (every lane of a wave
// reads the same LDS address).  FULL rows (j != i, both i < j and i > j), summed over j in ascending order.  Per atom and slice
// the first NOUT doubles of the partial row {Fx, Fy, Fz, e_i, w_i, pairs_i} (the row keeps its CLASSICAL_PART stride):
// NOUT = 3 the force source, 6 the observer.  (k_min_pairs, minimize.hip, carries this text written out with {F, e_i} kept.)
template <int NOUT, typename Pos>
__device__ __forceinline__ void gamd_lj_walk(const ClassicalArgs& a, const Pos pos) {
    static_assert(NOUT == 3 || NOUT == CLASSICAL_PART, "forces; + e_i, w_i and pairs_i");
    __shared__ double sx[GAMD_PASS_TILE], sy[GAMD_PASS_TILE], sz[GAMD_PASS_TILE];
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)a.slices), s = (int)(blockIdx.x % (unsigned)a.slices);
    const int box = blockIdx.y;
    const int npb = gamd_npb(a);
    const size_t a0 = (size_t)box * (size_t)npb;            // the caller's order is box-major
    if (I >= a.tiles) return;                               // (uniform; cannot happen with the launcher's grid)
    const int il = I * GAMD_PASS_TILE + tid;                // atom of this thread inside its box
    const bool vi = il < npb;
    const long long jb = (long long)s * a.chunk;
    const int je = (int)(jb + a.chunk < (long long)npb ? jb + a.chunk : (long long)npb);
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);

    double xi = 0.0, yi = 0.0, zi = 0.0;
    if (vi) pos.load(a0 + (size_t)il, xi, yi, zi);
    double fx = 0.0, fy = 0.0, fz = 0.0, e = 0.0, w = 0.0, cnt = 0.0;
    for (long long base = jb; base < je; base += GAMD_PASS_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int nj = (int)(je - base < GAMD_PASS_TILE ? je - base : GAMD_PASS_TILE);
        if (tid < nj) pos.load(a0 + (size_t)base + (size_t)tid, sx[tid], sy[tid], sz[tid]);
        __syncthreads();
        if (!vi) continue;
        const int self = (int)((long long)il - base);       // this atom's own slot in the chunk, if it is there
        for (int jj = 0; jj < nj; ++jj) {
            double dx = xi - sx[jj], dy = yi - sy[jj], dz = zi - sz[jj];
            dx = dx - Lx * rint(dx / Lx);
            dy = dy - Ly * rint(dy / Ly);
            dz = dz - Lz * rint(dz / Lz);
            const double r2 = (dx * dx + dy * dy) + dz * dz;
            if (jj == self || !(r2 < a.rc2)) continue;
            const double ir2 = 1.0 / r2;
            const double2 lj = gamd_lj_pair_r2(a, a.eps24, ir2, r2);   // (u, r u'(r)), u = (u_LJ - u0) S
            const double fs = -(lj.y * ir2);                // F_ij = -u'(r) d / r = fs d
            fx += fs * dx; fy += fs * dy; fz += fs * dz;
            if constexpr (NOUT >= 6) {
                e += lj.x;
                w += -lj.y;                                 // d . F_ij = -r u'(r)
                cnt += 1.0;
            }
        }
    }
    if (vi) {
        double* out = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * CLASSICAL_PART;
        out[0] = fx; out[1] = fy; out[2] = fz;
        if constexpr (NOUT >= 6) { out[3] = e; out[4] = w; out[5] = cnt; }
    }
}

// ---- the water tile walk --------------------------------------------------------------------------------------------
// The walk above plus the species flag of every staged atom.  A same-molecule pair takes the erf branch (U_excl) whatever r is;
// a different-molecule pair with r^2 < r_cut^2 takes the erfc branch (U_real), counts, and — LJ, both oxygens — adds the
// Lennard-Jones term.  Per atom and slice the first NOUT doubles of the partial row {Fx, Fy, Fz, u_LJ, u_real + u_excl, pairs}
// (WATER_PART stride): NOUT = 3 the force source, 6 the observer and the M-site pass, whose `pos` are the charge sites and
// whose Lennard-Jones term is k_w4_lj's (LJ = false: u_LJ is stored as 0).  (k_wmin_pairs, water_minimize.hip, carries this
// text written out with {F, u_LJ, u_coul} kept.)
// VIR (water_virial.hip) is the walk with the virial's accumulators INSTEAD of the others: the same pairs by the same tests,
// per atom and slice {w_LJ, w_coul} = {sum -(r u_LJ'(r)), sum fs_coul r^2} into `vpart` (WATER_VIR_PART stride), fs_coul r^2
// being the bracket the force scalar above is built from, on either branch.  Nothing of a.part is touched.
template <int NOUT, bool LJ, bool VIR = false, typename Pos>
__device__ __forceinline__ void gamd_water_walk(const WaterArgs& a, const Pos pos, double* vpart = nullptr) {
    static_assert(VIR ? NOUT == 0 : (NOUT == 3 || NOUT == WATER_PART), "forces; + u_LJ, u_coul and pairs; or the virial alone");
    __shared__ double sx[GAMD_PASS_TILE], sy[GAMD_PASS_TILE], sz[GAMD_PASS_TILE];
    __shared__ unsigned char so[GAMD_PASS_TILE];
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)a.slices), s = (int)(blockIdx.x % (unsigned)a.slices);
    const int box = blockIdx.y;
    const int npb = gamd_npb(a);
    const size_t a0 = (size_t)box * (size_t)npb;            // the caller's order is box-major
    if (I >= a.tiles) return;                               // (uniform; cannot happen with the launcher's grid)
    const int il = I * GAMD_PASS_TILE + tid;                // atom of this thread inside its box
    const bool vi = il < npb;
    const long long jb = (long long)s * a.chunk;
    const int je = (int)(jb + a.chunk < (long long)npb ? jb + a.chunk : (long long)npb);
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);

    double xi = 0.0, yi = 0.0, zi = 0.0;
    bool oi = false;
    if (vi) {
        pos.load(a0 + (size_t)il, xi, yi, zi);
        oi = a.species[a0 + (size_t)il] != 0;
    }
    const double q_h = a.q_h, q_o = -(q_h + q_h);           // -2 q_h, exact
    const double qi = oi ? q_o : q_h;
    const int mi = il / 3;                                  // npb is a multiple of 3: molecules do not straddle boxes
    // the thread's output row, held in vector registers from here on: left to the compiler, its uniform part stays in scalar
    // registers across the loop, which the potential's constants fill already (four scalar spills otherwise)
    double* out = VIR ? vpart + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * WATER_VIR_PART
                      : a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * WATER_PART;
    asm volatile("" : "+v"(out));
    double fx = 0.0, fy = 0.0, fz = 0.0, elj = 0.0, ec = 0.0, cnt = 0.0;
    double wlj = 0.0, wc = 0.0;                             // VIR only
    for (long long base = jb; base < je; base += GAMD_PASS_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int nj = (int)(je - base < GAMD_PASS_TILE ? je - base : GAMD_PASS_TILE);
        if (tid < nj) {
            const size_t j = a0 + (size_t)base + (size_t)tid;
            pos.load(j, sx[tid], sy[tid], sz[tid]);
            so[tid] = a.species[j] != 0 ? 1 : 0;
        }
        __syncthreads();
        if (!vi) continue;
        const int self = (int)((long long)il - base);       // this atom's own slot in the chunk, if it is there
        const int mol0 = (int)((long long)mi * 3 - base);   // ... and its molecule's first
        for (int jj = 0; jj < nj; ++jj) {
            double dx = xi - sx[jj], dy = yi - sy[jj], dz = zi - sz[jj];
            dx = dx - Lx * rint(dx / Lx);
            dy = dy - Ly * rint(dy / Ly);
            dz = dz - Lz * rint(dz / Lz);
            const double r2 = (dx * dx + dy * dy) + dz * dz;
            if (jj == self) continue;
            const bool same = jj >= mol0 && jj < mol0 + 3;
            if (!same && !(r2 < a.rc2)) continue;
            const bool oj = so[jj] != 0;
            const double qq = a.coul * (qi * (oj ? q_o : q_h));
            const double r = sqrt(r2);
            const double ir2 = 1.0 / r2;
            const double ar = a.alpha * r;
            const double gs = a.two_a_rpi * exp(-(ar * ar));        // -r d/dr of erfc(alpha r), over r
            double fs;
            if (same) {                                     // U_excl: -q_i q_j erf(alpha r) / r
                const double t = erf(ar) / r;
                if constexpr (NOUT >= 6) ec += -(qq * t);
                fs = (qq * (gs - t)) * ir2;
                if constexpr (VIR) wc += qq * (gs - t);
            } else {                                        // U_real: q_i q_j erfc(alpha r) / r
                const double t = erfc(ar) / r;
                if constexpr (NOUT >= 6) ec += qq * t;
                fs = (qq * (t + gs)) * ir2;
                if constexpr (VIR) wc += qq * (t + gs);
                if constexpr (NOUT >= 6) cnt += 1.0;
                if constexpr (LJ) {
                    if (oi && oj) {                         // the Lennard-Jones walk's term
                        const double2 lj = gamd_lj_pair_r(a, 6.0 * a.eps4, ir2, r);     // 6 (4 epsilon) = 24 epsilon bit for bit
                        if constexpr (NOUT >= 6) elj += lj.x;
                        fs = fs + -(lj.y * ir2);
                        if constexpr (VIR) wlj += -lj.y;    // gamd_lj_walk's w
                    }
                }
            }
            if constexpr (!VIR) { fx += fs * dx; fy += fs * dy; fz += fs * dz; }
        }
    }
    if (vi) {
        if constexpr (VIR) { out[0] = LJ ? wlj : 0.0; out[1] = wc; }
        else { out[0] = fx; out[1] = fy; out[2] = fz; }
        if constexpr (NOUT >= 6) { out[3] = LJ ? elj : 0.0; out[4] = ec; out[5] = cnt; }
    }
}

// ---- the rho(k) pass ------------------------------------------------------------------------------------------------
// k_struct_rho's scheme, charge-weighted: grid (blocks per box, K / 64, boxes), thread (w, l) owns k-vector l of its 64 and the
// atoms 4 m + w of every 256-atom chunk of its block (chunks staged in LDS as the wrapped fractional coordinate s and the charge,
// in double); one partial (re, im) per workgroup and k-vector, the four waves added as (w0 + w1) + (w2 + w3).
template <typename Pos>
__device__ __forceinline__ void gamd_water_rho(const WaterArgs& a, const Pos pos) {
    __shared__ double sx[GAMD_PASS_TILE], sy[GAMD_PASS_TILE], sz[GAMD_PASS_TILE], sq[GAMD_PASS_TILE];
    __shared__ double red[4][2][64];                        // [wave][re, im][lane]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int box = blockIdx.z, npb = gamd_npb(a), a0 = box * npb, a1 = a0 + npb;
    const int k = blockIdx.y * 64 + lane;
    const bool vk = k < a.n_k;
    const double nx = vk ? (double)a.kvec[3 * (size_t)k] : 0.0, ny = vk ? (double)a.kvec[3 * (size_t)k + 1] : 0.0,
                 nz = vk ? (double)a.kvec[3 * (size_t)k + 2] : 0.0;
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    double re = 0.0, im = 0.0;
    for (int base = a0 + blockIdx.x * GAMD_PASS_TILE; base < a1; base += gridDim.x * GAMD_PASS_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int i = base + tid;
        if (i < a1) {
            double px, py, pz;
            pos.load((size_t)i, px, py, pz);
            sx[tid] = water_frac(px, Lx);
            sy[tid] = water_frac(py, Ly);
            sz[tid] = water_frac(pz, Lz);
            sq[tid] = a.species[i] != 0 ? a.q_o : a.q_h;
        }
        __syncthreads();
        const int cnt = a1 - base < GAMD_PASS_TILE ? a1 - base : GAMD_PASS_TILE;
        for (int j = w; j < cnt; j += 4) {                  // (wave-uniform: one LDS address per wave)
            const double ph = (nx * sx[j] + ny * sy[j]) + nz * sz[j];
            double sn, cs;
            sincospi(2.0 * ph, &sn, &cs);
            re += sq[j] * cs; im -= sq[j] * sn;
        }
    }
    red[w][0][lane] = re; red[w][1][lane] = im;
    __syncthreads();
    if (w == 0 && vk) {
        double* out = a.rho_partial + (((size_t)box * a.rho_blocks + blockIdx.x) * (size_t)a.n_k + (size_t)k) * 2;
        out[0] = (red[0][0][lane] + red[1][0][lane]) + (red[2][0][lane] + red[3][0][lane]);
        out[1] = (red[0][1][lane] + red[1][1][lane]) + (red[2][1][lane] + red[3][1][lane]);
    }
}

// ---- the reciprocal force pass --------------------------------------------------------------------------------------
// grid (T * kslices, boxes), thread t keeps atom t of row tile I (s = the wrapped x / L) and walks its k slice in list order,
// staged 256 at a time in LDS {n, Re S, Im S, A}: g += A (Re S sin(k.r) + Im S cos(k.r)) n per component, into rpart.
// The k walk of slice s is contiguous: the vectors [s * kchunk, (s + 1) * kchunk).  (k_wmin_recip, water_minimize.hip, carries
// this text written out with a strided walk, the 256-vector blocks s, s + kslices, ...; see WMinArgs.)
template <typename Pos>
__device__ __forceinline__ void gamd_water_recip(const WaterArgs& a, const Pos pos) {
    __shared__ double kn[3][GAMD_PASS_TILE], ks_re[GAMD_PASS_TILE], ks_im[GAMD_PASS_TILE], ks_a[GAMD_PASS_TILE];
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)a.kslices), s = (int)(blockIdx.x % (unsigned)a.kslices);
    const int box = blockIdx.y;
    const int npb = gamd_npb(a);
    const size_t a0 = (size_t)box * (size_t)npb;
    if (I >= a.tiles) return;                               // (uniform; cannot happen with the launcher's grid)
    const int il = I * GAMD_PASS_TILE + tid;
    const bool vi = il < npb;
    const long long kb = (long long)s * a.kchunk;
    const int ke = (int)(kb + a.kchunk < (long long)a.n_k ? kb + a.kchunk : (long long)a.n_k);
    double six = 0.0, siy = 0.0, siz = 0.0;
    if (vi) {
        double px, py, pz;
        pos.load(a0 + (size_t)il, px, py, pz);
        six = water_frac(px, gamd_box_edge(a, box, 0));
        siy = water_frac(py, gamd_box_edge(a, box, 1));
        siz = water_frac(pz, gamd_box_edge(a, box, 2));
    }
    double gx = 0.0, gy = 0.0, gz = 0.0;
    for (long long base = kb; base < ke; base += GAMD_PASS_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int nk = (int)(ke - base < GAMD_PASS_TILE ? ke - base : GAMD_PASS_TILE);
        if (tid < nk) {
            const size_t k = (size_t)base + (size_t)tid;
            kn[0][tid] = (double)a.kvec[3 * k]; kn[1][tid] = (double)a.kvec[3 * k + 1]; kn[2][tid] = (double)a.kvec[3 * k + 2];
            const double* p = a.sk + ((size_t)box * (size_t)a.n_k + k) * 3;
            ks_re[tid] = p[0]; ks_im[tid] = p[1]; ks_a[tid] = p[2];
        }
        __syncthreads();
        if (!vi) continue;
        for (int kk = 0; kk < nk; ++kk) {
            const double nx = kn[0][kk], ny = kn[1][kk], nz = kn[2][kk];
            const double ph = (nx * six + ny * siy) + nz * siz;
            double sn, cs;
            sincospi(2.0 * ph, &sn, &cs);
            const double wk = ks_a[kk] * (ks_re[kk] * sn + ks_im[kk] * cs);
            gx += wk * nx; gy += wk * ny; gz += wk * nz;
        }
    }
    if (vi) {
        double* out = a.rpart + (((size_t)box * (size_t)a.kslices + (size_t)s) * (size_t)npb + (size_t)il) * 3;
        out[0] = gx; out[1] = gy; out[2] = gz;
    }
}

// ---- FIRE: what the two minimisers share besides the passes above -----------------------------------------------------
// x64, v64 widened / zeroed by the caller's init kernel; here the scalar state of iteration 0, the gate open, the row cleared
// (one thread per box calls it)
__device__ __forceinline__ void gamd_fire_reset(const FireArgs& m, int box) {
    double* st = m.state + (size_t)box * 2 * MIN_STATE;
    st[0] = m.dt_start; st[1] = m.alpha_start; st[2] = 0.0; st[3] = 0.0;
    for (int q = 0; q < MIN_ROW; ++q) m.rows[(size_t)box * MIN_ROW + q] = 0.0;
    m.stopped[box] = 0;
}

// the block tree of the per-atom / per-molecule pass: the thread's accumulators, all but the last summed and the last
// maximised over the 256 threads by the tree of k_report_ke (shuffle 32 .. 1, then (w0 + w1) + (w2 + w3)); thread q stores
// column q of this workgroup's STRIDE-double row of a.blk ([n_boxes][blocks][STRIDE]).  (The accumulators come as scalars:
// handed over as an array, k_wmin_mols spills a register.)
template <int STRIDE, typename Args, typename... Acc>
__device__ __forceinline__ void gamd_fire_block_tree(const Args& a, int box, Acc... sums_then_max) {
    constexpr int NACC = (int)sizeof...(Acc);
    __shared__ double red[4][NACC];
    double acc[NACC] = {sums_then_max...};
#pragma unroll
    for (int q = 0; q < NACC; ++q) {
        double v = acc[q];
        if (q < NACC - 1) v = gamd_wave_sum(v);
        else {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_down(v, d, 64));
        }
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < NACC) {
        const int q = threadIdx.x;
        const double r = q < NACC - 1 ? (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]) : fmax(fmax(red[0][q], red[1][q]), fmax(red[2][q], red[3][q]));
        a.blk[((size_t)box * (size_t)a.blocks + blockIdx.x) * STRIDE + q] = r;
    }
}

// The decision of one iteration, taken by EVERY thread from the same bits: U and the block sums ff, vf, vv, mx are known.
// rms = sqrt(ff / 3N); not finite -> the box stops as failed; rms <= tolerance -> converged; the pass behind the last
// iteration -> max_iter.  Otherwise FIRE's mixing coefficients (vf > 0: v = c1 v + c2 F with c1 = 1 - alpha,
// c2 = alpha sqrt(vv / ff), after n_min such steps dt = min(dt f_inc, dt_max), alpha = alpha f_alpha; else v = 0,
// alpha = alpha_start, dt = dt f_dec).  `writer` (one thread per box) writes the row's start columns at it == 0, the row and
// the gate when the box stops, and the next slot's {dt, alpha, n_pos}.  A box that goes on ends in move(mix, c1, c2, dt), the
// caller's update of its atom / molecule; a box that stops returns before it: nothing moves.
template <typename Move>
__device__ __forceinline__ void gamd_fire_step(const FireArgs& m, int box, int npb, bool writer, double U, double ff, double vf,
                                               double vv, double mx, Move move) {
    const double rms = sqrt(ff / (3.0 * (double)npb));
    const double* cur = m.state + ((size_t)box * 2 + (size_t)(m.it & 1)) * MIN_STATE;
    double dt = cur[0], alpha = cur[1], n_pos = cur[2];
    double* row = m.rows + (size_t)box * MIN_ROW;
    if (writer && m.it == 0) { row[2] = U; row[3] = rms; }
    int stop = 0;
    if (!isfinite(U) || !isfinite(ff)) stop = 1 + MIN_FAILED;
    else if (rms <= m.tol) stop = 1 + MIN_CONVERGED;
    else if (m.last) stop = 1 + MIN_MAX_ITER;
    if (stop) {
        if (writer) {
            row[0] = (double)(stop - 1); row[1] = (double)m.it; row[4] = U; row[5] = rms; row[6] = mx; row[7] = dt;
            m.stopped[box] = stop;
        }
        return;
    }
    const bool mix = vf > 0.0;
    double c1 = 0.0, c2 = 0.0;
    if (mix) {
        c1 = 1.0 - alpha; c2 = alpha * sqrt(vv / ff);
        if (n_pos > (double)m.n_min) { dt = fmin(dt * m.f_inc, m.dt_max); alpha = alpha * m.f_alpha; }
        n_pos += 1.0;
    } else {
        alpha = m.alpha_start; dt = dt * m.f_dec; n_pos = 0.0;
    }
    if (writer) {
        double* nxt = m.state + ((size_t)box * 2 + (size_t)((m.it + 1) & 1)) * MIN_STATE;
        nxt[0] = dt; nxt[1] = alpha; nxt[2] = n_pos;
    }
    move(mix, c1, c2, dt);
}
