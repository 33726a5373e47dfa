// water_relax.hip — the two water energy minimisers under the potential AS THE HANDLE IS CONFIGURED
// (gamd_water_minimize_potential): FIRE (water_minimize.hip) and L-BFGS (water_lbfgs.hip) on rigid
// molecules with the TIP4P M-site (gamd_water_msite), particle-mesh Ewald (gamd_water_pme) and the cell table (gamd_water_cells)
// in any combination, none of them included.  The reference's third ground-truth generator minimises TIP4P-Ew water under PME
// (dataset/generate_tip4p_data.py:85); with the switch off the minimisers know the 3-site, plain-sum, all-pairs form alone.
// Positions, forces and every sum in double; atoms in the CALLER's order O,H,H, molecule = index / 3.
//
// The force stage routes as WaterPotential::drive does, with the minimiser's double positions where the observer has its sites:
//
//   3-site   pairs       k_wmin_pairs (launch_wmin_pairs), or the table built from the positions and k_wcell_pairs
//                        (launch_water_cells, the O-O term in the walk)
//            reciprocal  k_wmin_rho, k_water_sk, k_wmin_recip — the minimiser's STRIDED k walk, checked by launch_wmin_recip —
//                        or the ten launches of launch_water_pme on the positions
//   M-site   k_wrx_sites one thread per atom, as k_w4_sites: the oxygen's row of `sites` takes M = O' + w (d_1 + d_2) by
//                        water_msite (gamd_potential_dev.h, the one place M is computed, here on doubles), a hydrogen's its
//                        own position wrapped into [0, L)
//            pairs       k_w4_pairs as it is (launch_w4_pairs: it reads the sites), or launch_water_cells on the sites
//            k_wrx_lj    k_w4_lj's O-O pass on the double positions: thread t of workgroup (I, s) keeps the oxygen of molecule
//                        I * 256 + t and walks the molecules of slice s, staged 256 at a time, with a cutoff test of its own on
//                        the O-O distance; {F_LJ, u_LJ} per molecule and slice into `ljpart`
//            reciprocal  k_w4_rho, k_water_sk, k_w4_recip — the observer's KCHUNK walk, checked by launch_w4_recip — or
//                        launch_water_pme on the sites
//
// and behind it one per-molecule pass and the minimiser's own update kernel, launched as it is:
//
//   k_wrx_mols      k_wmin_mols with the force of gamd_wrx_dev.h: the raw force of the molecule's three REAL atoms — with the
//                   M-site, M's force spread with the weights 1 - 2 w, w, w — projected onto the tangent space of the three
//                   bond constraints, v projected, the same seven columns into `blk`; then k_wmin_update.
//   k_wrx_lbmols    k_wlb_mols likewise: the same columns (WLB_ACC) into the L-BFGS's `blk`, formed in several walks over the thread's
//                   molecules (see the kernel); then k_wlb_update.
//
// Launches per iteration / evaluation: pairs 1 (cells 6), reciprocal 3 (PME 10), M-site + 2, molecules 1, update 1: 6 for the
// 3-site plain all-pairs form (today's six), 25 for M-site + PME + cells.
//
// Gates.  The k_wrx_ kernels, k_wmin_pairs / _rho / _recip and the update kernels skip a stopped box (fire.stopped, the L-BFGS's
// gate set of the pass).  The reused observer kernels — the table builder, k_wcell_*, k_pme_*, k_w4_pairs / _rho / _recip,
// k_water_sk — know DEVFLAG_FROZEN alone: they evaluate a stopped box again, on positions (or sites) that no longer change, and
// write work buffers (part, rpart, ublk, the grids, the tables) that no later kernel reads for that box, because every reader is
// gated.  A stopped box's x64, state and row do not change, and a box gets the bits it gets alone: every buffer is per box.
// Fixed assignment, no floating-point atomics (the spread's are integer, water_pme.hip), contraction off, plain stores: the same
// bits run after run.  Checked build: the ring count k_wrx_lbmols reads from the state passes through GAMD_CHK_RANGE, as in
// k_wlb_mols; no other value a k_wrx_ kernel reads from memory is used as an address.
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_passes_dev.h"
#include "gamd_wmin_dev.h"
#include "gamd_wrx_dev.h"

namespace {

using namespace gamd_wmin;

__global__ void __launch_bounds__(256) k_wrx_sites(WRxSiteArgs r) {
    const WaterArgs& a = r.b.w;
    const int box = blockIdx.y;
    if (r.stopped[box]) return;                             // the box has stopped: its sites stay
    const int npb = gamd_npb(a);
    const int il = blockIdx.x * blockDim.x + threadIdx.x;   // one thread per atom
    if (il >= npb) return;
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    const size_t a0 = (size_t)box * (size_t)npb, i = a0 + (size_t)il;
    const double* p = r.x64 + 3 * i;
    double sx, sy, sz;
    if (il % 3 == 0) {                                      // npb is a multiple of 3: il + 2 < npb
        water_msite(p, p + 3, p + 6, Lx, Ly, Lz, r.b.w_h, sx, sy, sz);
    } else {
        sx = water_wrap(p[0], Lx); sy = water_wrap(p[1], Ly); sz = water_wrap(p[2], Lz);
    }
    r.b.sites[3 * i] = sx; r.b.sites[3 * i + 1] = sy; r.b.sites[3 * i + 2] = sz;
}

// k_w4_lj (water_msite.hip) on the double positions, statement for statement: a change there is made here too
__global__ void __launch_bounds__(256) k_wrx_lj(WRxSiteArgs r) {
    const WaterArgs& a = r.b.w;
    const int box = blockIdx.y;
    if (r.stopped[box]) return;
    __shared__ double sx[GAMD_PASS_TILE], sy[GAMD_PASS_TILE], sz[GAMD_PASS_TILE];
    __shared__ unsigned char so[GAMD_PASS_TILE];
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)a.slices), s = (int)(blockIdx.x % (unsigned)a.slices);
    const int npb = gamd_npb(a), nm = npb / 3;
    const size_t a0 = (size_t)box * (size_t)npb;
    const int ml = I * GAMD_PASS_TILE + tid;                       // molecule of this thread inside its box
    if (I * GAMD_PASS_TILE >= nm) return;                          // (uniform; cannot happen with the launcher's grid)
    const bool vi = ml < nm;
    const long long jb = (long long)s * r.b.mchunk;
    const int je = (int)(jb + r.b.mchunk < (long long)nm ? jb + r.b.mchunk : (long long)nm);
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    double xi = 0.0, yi = 0.0, zi = 0.0;
    bool oi = false;
    if (vi) {
        const double* p = r.x64 + 3 * (a0 + 3 * (size_t)ml);
        xi = p[0]; yi = p[1]; zi = p[2];
        oi = a.species[a0 + 3 * (size_t)ml] != 0;
    }
    double lx = 0.0, ly = 0.0, lz = 0.0, elj = 0.0;
    for (long long base = jb; base < je; base += GAMD_PASS_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int nj = (int)(je - base < GAMD_PASS_TILE ? je - base : GAMD_PASS_TILE);
        if (tid < nj) {
            const size_t j = a0 + 3 * ((size_t)base + (size_t)tid);
            const double* p = r.x64 + 3 * j;
            sx[tid] = p[0]; sy[tid] = p[1]; sz[tid] = p[2];
            so[tid] = a.species[j] != 0 ? 1 : 0;
        }
        __syncthreads();
        if (!vi || !oi) continue;
        const int self = (int)((long long)ml - base);       // this molecule's own slot in the chunk, if it is there
        for (int jj = 0; jj < nj; ++jj) {
            double dx = xi - sx[jj], dy = yi - sy[jj], dz = zi - sz[jj];
            dx = dx - Lx * rint(dx / Lx);
            dy = dy - Ly * rint(dy / Ly);
            dz = dz - Lz * rint(dz / Lz);
            const double r2 = (dx * dx + dy * dy) + dz * dz;
            if (jj == self || so[jj] == 0 || !(r2 < a.rc2)) continue;  // the cutoff test on the O-O distance
            const double ir2 = 1.0 / r2;
            const double2 lj = gamd_lj_pair_r2(a, 6.0 * a.eps4, ir2, r2);               // 6 (4 epsilon) = 24 epsilon bit for bit
            elj += lj.x;
            const double fl = -(lj.y * ir2);
            lx += fl * dx; ly += fl * dy; lz += fl * dz;
        }
    }
    if (vi) {
        double* out = r.b.ljpart + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)nm + (size_t)ml) * W4_LJ;
        out[0] = lx; out[1] = ly; out[2] = lz; out[3] = elj;
    }
}

// k_wmin_mols (water_minimize.hip) with the force of gamd_wrx_dev.h; the projection, the inner products and the block tree are its
__global__ void __launch_bounds__(256, 4) k_wrx_mols(WRxMinArgs r) {
    const WMinArgs& m = r.m;
    const WaterArgs& a = m.w;
    const int box = blockIdx.y;
    if (m.fire.stopped[box]) return;
    const int npb = gamd_npb(a), nmol = npb / 3;
    const gamd_wrx::BoxK c = gamd_wrx::box_k(a, box);
    const gamd_wrx::Sites q{r.w_h, r.w_o, r.ljpart};
    double ff = 0.0, vf = 0.0, vv = 0.0, ulj = 0.0, uc = 0.0, z2 = 0.0, mx = 0.0;
    for (int ml = blockIdx.x * blockDim.x + threadIdx.x; ml < nmol; ml += gridDim.x * blockDim.x) {
        const size_t mol = (size_t)box * (size_t)nmol + (size_t)ml;
        D3 F[3];
        gamd_wrx::mol_force(a, q, c, box, npb, ml, F, ulj, uc, z2);
        D3 x[3], v[3];
        load_mol(m.fire.x64, mol, x); load_mol(m.fire.v64, mol, v);
        project(x, F);
        project(x, v);
        store_mol(m.fire.f64, mol, F); store_mol(m.fire.v64, mol, v);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ff += dot(F[k], F[k]);
            vf += dot(v[k], F[k]);
            vv += dot(v[k], v[k]);
            mx = fmax(mx, fmax(fmax(fabs(F[k].x), fabs(F[k].y)), fabs(F[k].z)));
        }
    }
    gamd_fire_block_tree<WATER_ACC>(a, box, ff, vf, vv, ulj, uc, z2, mx);
}

__device__ __forceinline__ double dot3(const D3 (&p)[3], const D3 (&q)[3]) { return (dot(p[0], q[0]) + dot(p[1], q[1])) + dot(p[2], q[2]); }

// one column of the block row on its way into the tree of gamd_fire_block_tree: the thread's accumulator summed (or maximised)
// over its wave, lane 0's result into the column's slot of the wave
__device__ __forceinline__ void wrx_column(double (&red)[4][WLB_ACC], int q, double v) {
    if (q < WLB_MAX) v = gamd_wave_sum(v);
    else {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_down(v, d, 64));
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v;
}

// k_wlb_mols (water_lbfgs.hip) with the force of gamd_wrx_dev.h, in SEVERAL walks over the thread's molecules so that the pass
// stays inside the 128 registers of four waves per SIMD (k_wlb_mols holds its 35 accumulators at once, in 226): the first walk
// forms and stores the projected force with the five columns that need nothing else, the second s = xt - x, y = F - Ft and their
// six columns, then one walk per ring slot that holds a pair; every column goes into the tree as soon as it is complete.  Ft
// is read back as the first walk stored it, by the thread that wrote it, and s is formed again by the same statement.  Every column is the sum of the same terms over the thread's molecules in the
// same order, then the same tree: k_wlb_mols' bits.
__global__ void __launch_bounds__(256, 4) k_wrx_lbmols(WRxLbArgs r) {
    const WLbfgsArgs& l = r.l;
    const WaterArgs& a = l.w;
    const int box = blockIdx.y;
    const int nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1;
    if (l.gates[(size_t)(l.it & 1) * (size_t)nb + box]) return;
    __shared__ double red[4][WLB_ACC];
    const int npb = gamd_npb(a), nmol = npb / 3;
    const double* cur = l.state + ((size_t)box * 2 + (size_t)(l.it & 1)) * LBFGS_SLOT;
    const int cnt = GAMD_CHK_RANGE(l.sticky, (int)cur[2], 0, l.m, GAMD_CHK_WLBFGS_COUNT);  // the slots 0 .. cnt - 1 hold pairs
    {
        const gamd_wrx::BoxK c = gamd_wrx::box_k(a, box);
        const gamd_wrx::Sites q{r.w_h, r.w_o, r.ljpart};
        double ulj = 0.0, uc = 0.0, z2 = 0.0, ftft = 0.0, mx = 0.0;
        for (int ml = blockIdx.x * blockDim.x + threadIdx.x; ml < nmol; ml += gridDim.x * blockDim.x) {
            const size_t mol = (size_t)box * (size_t)nmol + (size_t)ml;
            D3 ft[3], xt[3];
            gamd_wrx::mol_force(a, q, c, box, npb, ml, ft, ulj, uc, z2);
            load_mol(l.xt, mol, xt);
            project(xt, ft);
            store_mol(l.ft, mol, ft);
#pragma unroll
            for (int k = 0; k < 3; ++k) mx = fmax(mx, sqrt(dot(ft[k], ft[k])));
            ftft += dot3(ft, ft);
        }
        wrx_column(red, WLB_ULJ, ulj); wrx_column(red, WLB_UC, uc); wrx_column(red, WLB_Z2, z2); wrx_column(red, WLB_FTFT, ftft);
        wrx_column(red, WLB_MAX, mx);
    }
    {                                                       // s = xt - x, y = F - Ft and their six columns
        double fs = 0.0, ss = 0.0, sy = 0.0, yy = 0.0, sft = 0.0, yft = 0.0;
        for (int ml = blockIdx.x * blockDim.x + threadIdx.x; ml < nmol; ml += gridDim.x * blockDim.x) {
            const size_t mol = (size_t)box * (size_t)nmol + (size_t)ml;
            D3 x[3], f[3], ft[3], s[3], y[3];
            load_mol(l.x, mol, x); load_mol(l.xt, mol, s); load_mol(l.f, mol, f); load_mol(l.ft, mol, ft);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                s[k] = s[k] - x[k];
                y[k] = f[k] - ft[k];
            }
            fs += dot3(f, s);
            ss += dot3(s, s);
            sy += dot3(s, y);
            yy += dot3(y, y);
            sft += dot3(s, ft);
            yft += dot3(y, ft);
        }
        wrx_column(red, WLB_FS, fs); wrx_column(red, WLB_SS, ss); wrx_column(red, WLB_SY, sy); wrx_column(red, WLB_YY, yy);
        wrx_column(red, WLB_SFT, sft); wrx_column(red, WLB_YFT, yft);
    }
#pragma unroll 1
    for (int k = 0; k < LBFGS_M; ++k) {                     // the ring's slots, one at a time; an empty slot's columns are 0
        double syk = 0.0, ftsk = 0.0, ftyk = 0.0;
        if (k < cnt) {                                      // (uniform)
            const double* rs = l.ring + (size_t)k * 3 * (size_t)a.n;
            const double* ry = l.ring + ((size_t)l.m + (size_t)k) * 3 * (size_t)a.n;
            for (int ml = blockIdx.x * blockDim.x + threadIdx.x; ml < nmol; ml += gridDim.x * blockDim.x) {
                const size_t mol = (size_t)box * (size_t)nmol + (size_t)ml;
                D3 x[3], s[3], ft[3], v[3];
                load_mol(l.x, mol, x); load_mol(l.xt, mol, s); load_mol(l.ft, mol, ft);
#pragma unroll
                for (int i = 0; i < 3; ++i) s[i] = s[i] - x[i];
                load_mol(ry, mol, v);
                syk += dot3(s, v);
                ftyk += dot3(ft, v);
                load_mol(rs, mol, v);
                ftsk += dot3(ft, v);
            }
        }
        wrx_column(red, WLB_SYK + k, syk); wrx_column(red, WLB_FTSK + k, ftsk); wrx_column(red, WLB_FTYK + k, ftyk);
    }
    __syncthreads();
    if (threadIdx.x < WLB_ACC) {
        const int k = threadIdx.x;
        const double v = k < WLB_MAX ? (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]) : fmax(fmax(red[0][k], red[1][k]), fmax(red[2][k], red[3][k]));
        l.blk[((size_t)box * (size_t)a.blocks + blockIdx.x) * WLB_ACC + k] = v;
    }
}

// what the force stage checks itself: the rows and the slices, the buffers every route reads, the route's own; each reused
// launcher checks the geometry of its walk (the strided k walk in launch_wmin_recip, the kchunk walk in launch_w4_recip, the grid
// in launch_water_pme, one pair slice in launch_water_cells)
int wrx_force_check(const WaterArgs& a, const double* x64, const int* stopped, const WRxRoute& r, PassGeom* g) {
    if (pass_geometry(a, 3, g) || a.blocks < 1 || a.blocks > 65535) return -1;
    if (!a.species || !a.part || !a.ublk || !a.rpart || !a.box_edges || !a.devflags || !x64 || !stopped) return -1;
    if (r.cells && a.slices != 1) return -1;
    if (r.pme && (a.kslices != 1 || a.kblocks != pme_blocks(r.pme->nx, r.pme->ny, r.pme->nz))) return -1;
    if (r.w_h != 0.0) {
        if (!r.sites || !r.ljpart || !(r.w_h > 0.0) || !(r.w_h < 0.5) || r.mchunk < 1 || (long long)a.slices * r.mchunk < g->npb / 3) return -1;
        if ((g->npb / 3 + GAMD_PASS_TILE - 1) / GAMD_PASS_TILE * (long long)a.slices > 0x7fffffll) return -1;
    }
    return 0;
}

// the force stage on the positions x64 under the gates `stopped`
int wrx_force(const WaterArgs& a, const double* x64, const int* stopped, const WRxRoute& r, const PassGeom& g, hipStream_t st) {
    WMinArgs f{};                                           // what the minimiser's own force launches read
    f.w = a; f.fire.x64 = const_cast<double*>(x64); f.fire.stopped = const_cast<int*>(stopped);
    const bool msite = r.w_h != 0.0;
    const double* pos = msite ? r.sites : x64;              // what the pair and reciprocal passes walk
    const W4Args b{a, r.w_h, 1.0 - 2.0 * r.w_h, r.mchunk, r.sites, r.ljpart};
    const WRxSiteArgs sa{b, x64, stopped};
    if (msite) {
        hipLaunchKernelGGL(k_wrx_sites, dim3((unsigned)g.T, g.nb), dim3(256), 0, st, sa); GAMD_CHECK_LAUNCH();
    }
    if (r.cells) {
        if (int e = launch_water_cells(a, *r.cells, pos, WATER_PART, !msite, st)) return e;
    } else if (msite) {
        if (int e = launch_w4_pairs(b, st)) return e;
    } else {
        if (int e = launch_wmin_pairs(f, st)) return e;
    }
    if (msite) {
        const long long Tm = (g.npb / 3 + GAMD_PASS_TILE - 1) / GAMD_PASS_TILE;
        hipLaunchKernelGGL(k_wrx_lj, dim3((unsigned)(Tm * a.slices), g.nb), dim3(256), 0, st, sa); GAMD_CHECK_LAUNCH();
    }
    if (r.pme) {
        PmeArgs p = *r.pme;
        p.w = a; p.sites = pos;
        return launch_water_pme(p, st);
    }
    return msite ? launch_w4_recip(b, st) : launch_wmin_recip(f, st);
}

}  // namespace

int launch_wrx_iter(const WMinArgs& m, const WRxRoute& r, hipStream_t st) {
    PassGeom g;
    const FireArgs& fi = m.fire;
    if (wrx_force_check(m.w, fi.x64, fi.stopped, r, &g) || !m.w.blk) return -1;
    if (!fi.v64 || !fi.f64 || !fi.state || !fi.rows || fi.it < 0) return -1;
    if (int e = wrx_force(m.w, fi.x64, fi.stopped, r, g, st)) return e;
    const WRxMinArgs ma{m, r.w_h, 1.0 - 2.0 * r.w_h, r.ljpart};
    hipLaunchKernelGGL(k_wrx_mols, dim3(m.w.blocks, g.nb), dim3(256), 0, st, ma); GAMD_CHECK_LAUNCH();
    return launch_wmin_update(m, st);
}

int launch_wrx_eval(const WLbfgsArgs& l, const WRxRoute& r, hipStream_t st) {
    PassGeom g;
    if (!l.gates || l.it < 0) return -1;
    const int nb = l.w.bx.n_boxes > 1 ? l.w.bx.n_boxes : 1;
    const int* gates = l.gates + (size_t)(l.it & 1) * (size_t)nb;   // the gate set of this pass
    if (wrx_force_check(l.w, l.xt, gates, r, &g)) return -1;
    if (!l.x || !l.f || !l.ft || !l.d || !l.ring || !l.blk || !l.state || !l.rows || l.m < 1 || l.m > LBFGS_M) return -1;
    if (int e = wrx_force(l.w, l.xt, gates, r, g, st)) return e;
    const WRxLbArgs la{l, r.w_h, 1.0 - 2.0 * r.w_h, r.ljpart};
    hipLaunchKernelGGL(k_wrx_lbmols, dim3(l.w.blocks, g.nb), dim3(256), 0, st, la); GAMD_CHECK_LAUNCH();
    return launch_wlbfgs_update(l, st);
}
