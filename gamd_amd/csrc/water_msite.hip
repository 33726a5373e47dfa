// water_msite.hip — the TIP4P M-site in the water classical potential (gamd_water_msite): the
// potential of water_classical.hip with the negative charge of a molecule on a virtual site M instead of on the oxygen, the
// reference's third ground-truth generator (dataset/generate_tip4p_data.py, WaterBox(model='tip4pew')).  Handles, integrators
// and SETTLE see O,H,H; M lives inside the potential.  Atoms in the CALLER's order O,H,H: molecule = index / 3, the oxygen first.
//
//   k_w4_sites      the prepass: one thread per atom writes its charge-site position as doubles into `sites` — the oxygen's row
//                   holds M = O' + w (d_1 + d_2) (water_msite, gamd_potential_dev.h: the one place M is computed), a hydrogen's
//                   its own position wrapped into [0, L).  Every site is the same double whatever image its atoms are given in.
//   k_w4_pairs      k_water_pairs' walk (gamd_water_walk, gamd_passes_dev.h: the one body of both) on the site positions
//                   with the Lennard-Jones term off: a same-molecule pair (M-H1, M-H2, H1-H2) takes the erf branch, a
//                   different-molecule pair with site r^2 < r_cut^2 the erfc branch and counts.  Per atom and slice the row of
//                   k_water_pairs {F_site, 0, u_coul, pairs} into `part`.
//   k_w4_lj         the Lennard-Jones term in a pass of its own over oxygens (with it in the pair kernel that kernel needed 180
//                   vector registers, over the bar of 168): grid (Tm * slices, boxes), thread t keeps the oxygen of molecule t of
//                   its tile (atom 3 m, fp32 widened) and walks the oxygens of its slice of molecules, staged 256 at a time;
//                   k_classical_pairs' term on O-O distances with a cutoff test of its OWN on the O-O distance.  Per molecule
//                   and slice {F_LJ, u_LJ} into `ljpart`: kept apart from the site force, the two are spread differently.
//   k_w4_rho        k_water_rho's pass (gamd_water_rho) on the site positions.
//   k_w4_recip      k_water_recip's pass (gamd_water_recip, the same kchunk walk) on the site positions.
//   k_w4_atoms      k_water_atoms with the redistribution: a site's force F_s = pair slices in order from 0 + (pq kf) k slices in
//                   order from 0, as k_water_atoms forms it; F_O = F_LJ(O) + w_O F_M, F_Hk = F_s(Hk) + w F_M, then times len.  A
//                   hydrogen sums its molecule's oxygen row again in the same order (molecules straddle workgroups; the row is
//                   found by arithmetic on the thread's own index).  Error sums, z, z^2 and the fixed tree as k_water_atoms.
//   k_w4_drive      the force source's per-atom pass: the same forces to f_cl and (float)f_cl to the run's f, plain stores.
// k_water_sk and k_water_final read no positions and are launched as they are (launch_water_sk, launch_water_final).  The
// observer is eight launches, the force source seven (its pair passes are the observer's: energies computed and not read).
// Everything in double; fixed atom-to-thread and k-to-thread assignment, fixed slices and blocks per handle, no floating-point
// atomics, contraction off, nothing updated in place: the same bits run after run.  Every kernel returns while DEVFLAG_FROZEN
// is set.  (No kernel uses a value it read from memory as an address: the checked build has nothing to range-check here.)
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_passes_dev.h"

namespace {

__global__ void __launch_bounds__(256) k_w4_sites(W4Args b) {
    const WaterArgs& a = b.w;
    if (a.devflags[DEVFLAG_FROZEN]) return;
    const int box = blockIdx.y;
    const int npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const int il = blockIdx.x * blockDim.x + threadIdx.x;   // one thread per atom
    if (il >= npb) return;
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    const size_t a0 = (size_t)box * (size_t)npb, i = a0 + (size_t)il;
    const float* p = a.x + 3 * i;
    double sx, sy, sz;
    if (il % 3 == 0) {                                      // npb is a multiple of 3: il + 2 < npb
        water_msite(p, p + 3, p + 6, Lx, Ly, Lz, b.w_h, sx, sy, sz);
    } else {
        sx = water_wrap((double)p[0], Lx); sy = water_wrap((double)p[1], Ly); sz = water_wrap((double)p[2], Lz);
    }
    b.sites[3 * i] = sx; b.sites[3 * i + 1] = sy; b.sites[3 * i + 2] = sz;
}

__global__ void __launch_bounds__(256) k_w4_pairs(W4Args b) {
    if (b.w.devflags[DEVFLAG_FROZEN]) return;               // a frame that will be evaluated again
    gamd_water_walk<WATER_PART, false>(b.w, GamdPosF64{b.sites});       // u_LJ: k_w4_lj's
}

// the Lennard-Jones pass over oxygens: thread t of workgroup (I, s) keeps the oxygen of molecule I * 256 + t (atom 3 m of the
// box) and walks the molecules [s * mchunk, (s + 1) * mchunk), staged 256 at a time
__global__ void __launch_bounds__(256) k_w4_lj(W4Args b) {
    const WaterArgs& a = b.w;
    if (a.devflags[DEVFLAG_FROZEN]) return;
    __shared__ double sx[GAMD_PASS_TILE], sy[GAMD_PASS_TILE], sz[GAMD_PASS_TILE];
    __shared__ unsigned char so[GAMD_PASS_TILE];
    const int tid = threadIdx.x;
    const int I = (int)(blockIdx.x / (unsigned)a.slices), s = (int)(blockIdx.x % (unsigned)a.slices);
    const int box = blockIdx.y;
    const int npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n, nm = npb / 3;
    const size_t a0 = (size_t)box * (size_t)npb;
    const int ml = I * GAMD_PASS_TILE + tid;                       // molecule of this thread inside its box
    if (I * GAMD_PASS_TILE >= nm) return;                          // (uniform; cannot happen with the launcher's grid)
    const bool vi = ml < nm;
    const long long jb = (long long)s * b.mchunk;
    const int je = (int)(jb + b.mchunk < (long long)nm ? jb + b.mchunk : (long long)nm);
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    double xi = 0.0, yi = 0.0, zi = 0.0;
    bool oi = false;
    if (vi) {
        const float* p = a.x + 3 * (a0 + 3 * (size_t)ml);
        xi = (double)p[0]; yi = (double)p[1]; zi = (double)p[2];
        oi = a.species[a0 + 3 * (size_t)ml] != 0;
    }
    double lx = 0.0, ly = 0.0, lz = 0.0, elj = 0.0;
    for (long long base = jb; base < je; base += GAMD_PASS_TILE) {
        __syncthreads();                                    // the previous chunk has been read
        const int nj = (int)(je - base < GAMD_PASS_TILE ? je - base : GAMD_PASS_TILE);
        if (tid < nj) {
            const size_t j = a0 + 3 * ((size_t)base + (size_t)tid);
            const float* p = a.x + 3 * j;
            sx[tid] = (double)p[0]; sy[tid] = (double)p[1]; sz[tid] = (double)p[2];
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
        double* out = b.ljpart + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)nm + (size_t)ml) * W4_LJ;
        out[0] = lx; out[1] = ly; out[2] = lz; out[3] = elj;
    }
}

__global__ void __launch_bounds__(256) k_w4_rho(W4Args b) {
    if (b.w.devflags[DEVFLAG_FROZEN]) return;
    gamd_water_rho(b.w, GamdPosF64{b.sites});
}

__global__ void __launch_bounds__(256) k_w4_recip(W4Args b) {
    if (b.w.devflags[DEVFLAG_FROZEN]) return;
    gamd_water_recip(b.w, GamdPosF64{b.sites});
}

// the box's constants of the per-atom passes
struct W4Box { double pref, kfx, kfy, kfz; };
__device__ __forceinline__ W4Box w4_box(const WaterArgs& a, int box) {
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    return {a.coul8pi / ((Lx * Ly) * Lz), a.two_pi / Lx, a.two_pi / Ly, a.two_pi / Lz};
}

// the sums of row il of box `box`: t = the pair slices added in order from 0, F = t + (pq kf) g with g the k slices added in
// order from 0 — the site's complete force per length unit, as k_water_atoms forms it
__device__ __forceinline__ void w4_site_force(const WaterArgs& a, const W4Box& c, int box, int npb, int il, double t[WATER_PART], double F[3]) {
#pragma unroll
    for (int q = 0; q < WATER_PART; ++q) t[q] = 0.0;
    for (int s = 0; s < a.slices; ++s) {
        const double* p = a.part + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)npb + (size_t)il) * WATER_PART;
#pragma unroll
        for (int q = 0; q < WATER_PART; ++q) t[q] += p[q];
    }
    double g[3] = {0.0, 0.0, 0.0};
    for (int s = 0; s < a.kslices; ++s) {
        const double* p = a.rpart + (((size_t)box * (size_t)a.kslices + (size_t)s) * (size_t)npb + (size_t)il) * 3;
        g[0] += p[0]; g[1] += p[1]; g[2] += p[2];
    }
    const bool o = a.species[(size_t)box * (size_t)npb + (size_t)il] != 0;
    const double pq = c.pref * (o ? a.q_o : a.q_h);
    F[0] = t[0] + (pq * c.kfx) * g[0]; F[1] = t[1] + (pq * c.kfy) * g[1]; F[2] = t[2] + (pq * c.kfz) * g[2];
}

// atom il's force in kJ/mol/nm (and its own row's sums t): F_O = F_LJ(O) + w_O F_M, F_Hk = F_s(Hk) + w F_M, then times len
__device__ __forceinline__ void w4_atom_force(const W4Args& b, const W4Box& c, int box, int npb, int il, double t[WATER_PART], double F[3]) {
    const WaterArgs& a = b.w;
    double S[3];
    w4_site_force(a, c, box, npb, il, t, S);
    const int k = il % 3;
    if (k == 0) {                                           // the oxygen: its row is M's
        double l[W4_LJ] = {0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s < a.slices; ++s) {
            const double* p = b.ljpart + (((size_t)box * (size_t)a.slices + (size_t)s) * (size_t)(npb / 3) + (size_t)(il / 3)) * W4_LJ;
            l[0] += p[0]; l[1] += p[1]; l[2] += p[2]; l[3] += p[3];
        }
        t[3] = l[3];                                        // the row's u_LJ (k_w4_pairs stored 0)
#pragma unroll
        for (int d = 0; d < 3; ++d) F[d] = (l[d] + b.w_o * S[d]) * a.len;
    } else {                                                // a hydrogen: its molecule's M row, summed again in the same order
        double tm[WATER_PART], M[3];
        w4_site_force(a, c, box, npb, il - k, tm, M);
#pragma unroll
        for (int d = 0; d < 3; ++d) F[d] = (S[d] + b.w_h * M[d]) * a.len;
    }
}

__global__ void __launch_bounds__(256) k_w4_atoms(W4Args b) {
    const WaterArgs& a = b.w;
    if (a.devflags[DEVFLAG_FROZEN]) return;
    __shared__ double red[4][WATER_ACC];
    const int box = blockIdx.y;
    const int npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const size_t a0 = (size_t)box * (size_t)npb;
    const W4Box c = w4_box(a, box);
    double acc[WATER_ACC];
#pragma unroll
    for (int q = 0; q < WATER_ACC; ++q) acc[q] = 0.0;
    for (int il = blockIdx.x * blockDim.x + threadIdx.x; il < npb; il += gridDim.x * blockDim.x) {
        double t[WATER_PART], F[3];
        w4_atom_force(b, c, box, npb, il, t, F);
        const size_t i = a0 + (size_t)il;
        a.f_cl[3 * i] = F[0]; a.f_cl[3 * i + 1] = F[1]; a.f_cl[3 * i + 2] = F[2];
        acc[0] += t[3]; acc[1] += t[4]; acc[2] += t[5];
        const double z = a.species[i] != 0 ? -2.0 : 1.0;    // the charge in units of q_h: sums of these are exact
        acc[9] += z; acc[10] += z * z;
        if (a.f) {
            gamd_force_error((double)a.f[3 * i], (double)a.f[3 * i + 1], (double)a.f[3 * i + 2], F[0], F[1], F[2], acc[3], acc[4], acc[5],
                             acc[6], acc[7], acc[8]);
        }
    }
#pragma unroll
    for (int q = 0; q < WATER_ACC; ++q) {
        const double v = gamd_wave_sum(acc[q]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < WATER_ACC) {
        const int q = threadIdx.x;
        a.blk[((size_t)box * (size_t)a.blocks + blockIdx.x) * WATER_ACC + q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
    }
}

__global__ void __launch_bounds__(256) k_w4_drive(W4Args b, float* __restrict__ f_out) {
    const WaterArgs& a = b.w;
    if (a.devflags[DEVFLAG_FROZEN]) return;
    const int box = blockIdx.y;
    const int npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    const int il = blockIdx.x * blockDim.x + threadIdx.x;   // one thread per atom
    if (il >= npb) return;
    const W4Box c = w4_box(a, box);
    double t[WATER_PART], F[3];
    w4_atom_force(b, c, box, npb, il, t, F);
    const size_t i = (size_t)box * (size_t)npb + (size_t)il;
    a.f_cl[3 * i] = F[0]; a.f_cl[3 * i + 1] = F[1]; a.f_cl[3 * i + 2] = F[2];
    f_out[3 * i] = (float)F[0]; f_out[3 * i + 1] = (float)F[1]; f_out[3 * i + 2] = (float)F[2];
}

// what both launchers check, and the launches they share: sites, pairs, lj, rho, sk, recip — or, with `pme` (gamd_water_pme),
// launch_water_pme on the sites in place of the last three; with `cells` (gamd_water_cells, one pair slice) launch_water_cells on
// the sites in place of k_w4_pairs, `nout` accumulators; *gp = the rows' geometry
int w4_launch_passes(const W4Args& b, PassGeom* gp, hipStream_t st, const PmeArgs* pme, const CellTabBufs* cells, int nout) {
    const WaterArgs& a = b.w;
    if (pass_geometry(a, 3, gp) || (!pme && pass_k_geometry(a, gp->T, true))) return -1;
    const int nb = gp->nb, npb = gp->npb;
    const long long T = gp->T;
    if (!a.x || !a.species || !a.part || !a.ublk || !a.rpart || !a.f_cl || !a.devflags) return -1;
    if (!pme && (!a.kvec || !a.rho_partial || !a.sk)) return -1;
    if (!b.sites || !b.ljpart || !(b.w_h > 0.0) || !(b.w_h < 0.5) || b.mchunk < 1 || (long long)a.slices * b.mchunk < npb / 3) return -1;
    const long long Tm = (npb / 3 + GAMD_PASS_TILE - 1) / GAMD_PASS_TILE;
    hipLaunchKernelGGL(k_w4_sites, dim3((unsigned)T, nb), dim3(256), 0, st, b); GAMD_CHECK_LAUNCH();
    if (cells) {
        if (int r = launch_water_cells(a, *cells, b.sites, nout, false, st)) return r;
    } else {
        hipLaunchKernelGGL(k_w4_pairs, dim3((unsigned)(T * a.slices), nb), dim3(256), 0, st, b); GAMD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_w4_lj, dim3((unsigned)(Tm * a.slices), nb), dim3(256), 0, st, b); GAMD_CHECK_LAUNCH();
    if (pme) return launch_water_pme(*pme, st);             // (its `sites` are b.sites: the launchers below see to it)
    hipLaunchKernelGGL(k_w4_rho, dim3(a.rho_blocks, (a.n_k + 63) / 64, nb), dim3(256), 0, st, b); GAMD_CHECK_LAUNCH();
    if (int r = launch_water_sk(a, st)) return r;
    hipLaunchKernelGGL(k_w4_recip, dim3((unsigned)(T * a.kslices), nb), dim3(256), 0, st, b); GAMD_CHECK_LAUNCH();
    return 0;
}

}  // namespace

int launch_w4_classical(const W4Args& b, hipStream_t st, const PmeArgs* pme, const CellTabBufs* cells) {
    const WaterArgs& a = b.w;
    PassGeom g;
    if (a.blocks < 1 || a.blocks > 65535 || a.slot < 0 || !a.blk || !a.rows || (pme && pme->sites != b.sites)) return -1;
    if (int r = w4_launch_passes(b, &g, st, pme, cells, WATER_PART)) return r;
    hipLaunchKernelGGL(k_w4_atoms, dim3(a.blocks, g.nb), dim3(256), 0, st, b); GAMD_CHECK_LAUNCH();
    return launch_water_final(a, st);
}

int launch_w4_drive(const W4Args& b, float* f_out, hipStream_t st, const PmeArgs* pme, const CellTabBufs* cells) {
    PassGeom g;
    if (!f_out || (pme && pme->sites != b.sites)) return -1;
    if (int r = w4_launch_passes(b, &g, st, pme, cells, 3)) return r;
    hipLaunchKernelGGL(k_w4_drive, dim3((unsigned)g.T, g.nb), dim3(256), 0, st, b, f_out); GAMD_CHECK_LAUNCH();
    return 0;
}

// ---- the pieces water_relax.hip puts its routes together from (gamd_water_minimize_potential): the sites are its k_wrx_sites' --
// k_w4_pairs alone
int launch_w4_pairs(const W4Args& b, hipStream_t st) {
    const WaterArgs& a = b.w;
    PassGeom g;
    if (pass_geometry(a, 3, &g) || !a.species || !a.part || !a.devflags || !b.sites) return -1;
    hipLaunchKernelGGL(k_w4_pairs, dim3((unsigned)(g.T * a.slices), g.nb), dim3(256), 0, st, b); GAMD_CHECK_LAUNCH();
    return 0;
}

// k_w4_rho, k_water_sk, k_w4_recip alone: the kchunk walk's geometry
int launch_w4_recip(const W4Args& b, hipStream_t st) {
    const WaterArgs& a = b.w;
    PassGeom g;
    if (pass_rows(a, 3, &g) || pass_k_geometry(a, g.T, true)) return -1;
    if (!a.species || !a.kvec || !a.rho_partial || !a.sk || !a.ublk || !a.rpart || !a.devflags || !b.sites) return -1;
    hipLaunchKernelGGL(k_w4_rho, dim3(a.rho_blocks, (a.n_k + 63) / 64, g.nb), dim3(256), 0, st, b); GAMD_CHECK_LAUNCH();
    if (int r = launch_water_sk(a, st)) return r;
    hipLaunchKernelGGL(k_w4_recip, dim3((unsigned)(g.T * a.kslices), g.nb), dim3(256), 0, st, b); GAMD_CHECK_LAUNCH();
    return 0;
}
