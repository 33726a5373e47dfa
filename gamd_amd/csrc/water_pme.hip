// water_pme.hip — smooth particle-mesh Ewald (Essmann et al. 1995) as a second producer of the reciprocal-space buffers of the
// water classical potential (gamd_water_pme): `rpart`, the per-atom reciprocal force sums, and `ublk`,
// the block sums of the reciprocal energy.  The kernels behind them (k_water_atoms, k_w4_atoms, k_wsrc_atoms, k_w4_drive,
// k_water_final) are launched as they are.  Everything in double, no FFT library.  Per box a grid of nx x ny x nz points, z
// contiguous; charges in units of q_H (z = -2 on the oxygen or the M-site, +1 on a hydrogen).
//
//   k_pme_clear     one thread per grid point: the integer grid to zero.  The grid is the only buffer updated in place, so it
//                   is cleared at the head of EVERY sample: a sample that runs twice writes the same bits twice.
//   k_pme_spread4   grid (atoms / 32, boxes): eight lanes per atom, lane l < p owns stencil point l of the z axis — the contiguous
//   k_pme_spread6   axis, so an atom's z stencil sits on adjacent lanes — and walks the p x p points of x and y: the term
//                   z theta_x theta_y theta_z as llrint(term 2^50), added by a no-return atomicAdd on unsigned long long.
//                   Integer addition commutes and associates: the sums do not depend on the order of the additions.
//   k_pme_fft       one line pass of the 3-D transform: a workgroup holds up to 1024 points in LDS — 1024 / n lines of n points —
//                   loaded bit-reversed, log2 n radix-2 stages, stored in natural order.  Along z the lines are consecutive in
//                   memory; along y and x a workgroup takes lines of consecutive z, so every load and store is a run of
//                   min(1024 / n, nz) complex doubles (128 bytes at the least).  Twiddles from the host's table (double,
//                   uploaded once).  The first forward pass loads the integers, times 2^-50, as the real part.
//   k_pme_conv      grid (pme_blocks, boxes), grid-stride in a fixed order: G(m) = exp(-pi^2 |m~|^2 / alpha^2) / (|m~|^2 B(m)),
//                   m~_d = m_d / L_d with m_d in (-n/2, n/2], G(0) = 0; the thread's sum of G |Q^|^2, the fixed tree, times
//                   q_H^2 / 8 pi^2 into ublk (k_water_final's (4 pi C / V) * sum is then (C / 2 pi V) q_H^2 sum G |Q^|^2);
//                   Q^ <- G Q^.
//   k_pme_gather4   the spread's lanes: lane l sums theta'_d theta theta phi over the p x p points of x and y at its z point in
//   k_pme_gather6   index order, the eight lanes are added by the fixed tree (xor 4, 2, 1), and lane 0 stores
//                   -(q_H n_d / 16 pi^3) g_d into rpart: (8 pi C q_i / V)(2 pi / L_d) times that is
//                   -(C / pi V) q_i q_H (n_d / L_d) g_d, the PME force.
// Fixed atom-to-lane and point-to-thread assignment, integer accumulation where the order is not fixed, contraction off: the
// same bits run after run.  Every kernel returns while DEVFLAG_FROZEN is set.  Grid indices are computed from positions by
// gamd_pme_index / gamd_pme_wrap (gamd_pme_dev.h), which stay inside the grid for every bit pattern; no other value read from
// memory is used as an address.
#include "gamd_common.h"
#include "gamd_internal.h"

#pragma clang fp contract(off)

#include "gamd_passes_dev.h"
#include "gamd_pme_dev.h"

namespace {

constexpr int PME_LANES = 8;                                // lanes per atom of spread and gather
constexpr int PME_POINTS = 1024;                            // points a workgroup of the line pass holds

__device__ __forceinline__ size_t pme_points(const PmeArgs& p) { return ((size_t)p.nx * (size_t)p.ny) * (size_t)p.nz; }

__global__ void __launch_bounds__(256) k_pme_clear(PmeArgs p) {
    if (p.w.devflags[DEVFLAG_FROZEN]) return;
    const size_t G = pme_points(p), idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < G) p.gq[(size_t)blockIdx.y * G + idx] = 0ull;
}

// what spread and gather share: the lane's atom, its base indices, its weights
template <int P>
struct PmeAtom {
    int bx, by, bz;
    double tx[P], ty[P], tz[P], dx[P], dy[P], dz[P];
    double z;
};

template <int P, typename Pos>
__device__ __forceinline__ void pme_atom(const PmeArgs& p, const Pos pos, int box, size_t i, PmeAtom<P>& t) {
    const WaterArgs& a = p.w;
    double px, py, pz, wx, wy, wz;
    pos.load(i, px, py, pz);
    t.bx = gamd_pme_index(px, gamd_box_edge(a, box, 0), p.nx, &wx);
    t.by = gamd_pme_index(py, gamd_box_edge(a, box, 1), p.ny, &wy);
    t.bz = gamd_pme_index(pz, gamd_box_edge(a, box, 2), p.nz, &wz);
    gamd_pme_spline<P>(wx, t.tx, t.dx);
    gamd_pme_spline<P>(wy, t.ty, t.dy);
    gamd_pme_spline<P>(wz, t.tz, t.dz);
    t.z = a.species[i] != 0 ? -2.0 : 1.0;
}

// entry l of a register array by selects.  (Left alone, the compiler turns the chain back into an indexed load and the whole
// atom moves into scratch memory: every candidate passes through an empty asm, which it cannot see through.)
template <int P>
__device__ __forceinline__ double pme_pick(const double v[P], int l) {
    double r = v[0];
#pragma unroll
    for (int j = 1; j < P; ++j) {
        double c = v[j];
        asm volatile("" : "+v"(c));
        r = l == j ? c : r;
    }
    return r;
}

template <int P, typename Pos>
__device__ __forceinline__ void pme_spread(const PmeArgs& p, const Pos pos) {
    const WaterArgs& a = p.w;
    const int box = blockIdx.y, npb = gamd_npb(a);
    const int il = blockIdx.x * (256 / PME_LANES) + (threadIdx.x / PME_LANES), l = threadIdx.x % PME_LANES;
    if (il >= npb || l >= P) return;
    PmeAtom<P> t;
    pme_atom<P>(p, pos, box, (size_t)box * (size_t)npb + (size_t)il, t);
    const double thz = pme_pick<P>(t.tz, l);
    const int iz = gamd_pme_wrap(t.bz, l, p.nz, P);
    unsigned long long* g = p.gq + (size_t)box * pme_points(p);
#pragma unroll
    for (int jx = 0; jx < P; ++jx) {
        const int ix = gamd_pme_wrap(t.bx, jx, p.nx, P);
#pragma unroll
        for (int jy = 0; jy < P; ++jy) {
            const int iy = gamd_pme_wrap(t.by, jy, p.ny, P);
            const long long q = gamd_pme_quantum((t.z * t.tx[jx]) * (t.ty[jy] * thz));
            atomicAdd(g + ((size_t)ix * (size_t)p.ny + (size_t)iy) * (size_t)p.nz + (size_t)iz, (unsigned long long)q);
        }
    }
}

template <int P, typename Pos>
__device__ __forceinline__ void pme_gather(const PmeArgs& p, const Pos pos) {
    const WaterArgs& a = p.w;
    const int box = blockIdx.y, npb = gamd_npb(a);
    const int il = blockIdx.x * (256 / PME_LANES) + (threadIdx.x / PME_LANES), l = threadIdx.x % PME_LANES;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (il < npb && l < P) {
        PmeAtom<P> t;
        pme_atom<P>(p, pos, box, (size_t)box * (size_t)npb + (size_t)il, t);
        const double thz = pme_pick<P>(t.tz, l), dthz = pme_pick<P>(t.dz, l);
        const int iz = gamd_pme_wrap(t.bz, l, p.nz, P);
        const double* phi = p.gc + 2 * (size_t)box * pme_points(p);
#pragma unroll
        for (int jx = 0; jx < P; ++jx) {
            const int ix = gamd_pme_wrap(t.bx, jx, p.nx, P);
#pragma unroll
            for (int jy = 0; jy < P; ++jy) {
                const int iy = gamd_pme_wrap(t.by, jy, p.ny, P);
                const double f = phi[2 * (((size_t)ix * (size_t)p.ny + (size_t)iy) * (size_t)p.nz + (size_t)iz)];
                gx += ((t.dx[jx] * t.ty[jy]) * thz) * f;
                gy += ((t.tx[jx] * t.dy[jy]) * thz) * f;
                gz += ((t.tx[jx] * t.ty[jy]) * dthz) * f;
            }
        }
    }
#pragma unroll
    for (int d = PME_LANES / 2; d >= 1; d >>= 1) {          // (every lane of the wave is here)
        gx += __shfl_xor(gx, d, 64); gy += __shfl_xor(gy, d, 64); gz += __shfl_xor(gz, d, 64);
    }
    if (il < npb && l == 0) {
        const double c = a.q_h / (2.0 * ((a.two_pi * a.two_pi) * a.two_pi));        // q_H / 16 pi^3
        double* out = a.rpart + ((size_t)box * (size_t)npb + (size_t)il) * 3;       // kslices = 1
        out[0] = -((c * (double)p.nx) * gx); out[1] = -((c * (double)p.ny) * gy); out[2] = -((c * (double)p.nz) * gz);
    }
}

__global__ void __launch_bounds__(256) k_pme_spread4(PmeArgs p) {
    if (p.w.devflags[DEVFLAG_FROZEN]) return;
    if (p.sites) pme_spread<4>(p, GamdPosF64{p.sites}); else pme_spread<4>(p, GamdPosF32{p.w.x});
}
__global__ void __launch_bounds__(256) k_pme_spread6(PmeArgs p) {
    if (p.w.devflags[DEVFLAG_FROZEN]) return;
    if (p.sites) pme_spread<6>(p, GamdPosF64{p.sites}); else pme_spread<6>(p, GamdPosF32{p.w.x});
}
__global__ void __launch_bounds__(256) k_pme_gather4(PmeArgs p) {
    if (p.w.devflags[DEVFLAG_FROZEN]) return;
    if (p.sites) pme_gather<4>(p, GamdPosF64{p.sites}); else pme_gather<4>(p, GamdPosF32{p.w.x});
}
__global__ void __launch_bounds__(256) k_pme_gather6(PmeArgs p) {
    if (p.w.devflags[DEVFLAG_FROZEN]) return;
    if (p.sites) pme_gather<6>(p, GamdPosF64{p.sites}); else pme_gather<6>(p, GamdPosF32{p.w.x});
}

// lines of n points a workgroup of the pass along `axis` holds: 1024 / n, and no more than there are side by side (the lines
// of a box along z; the nz lines of consecutive z along y or x)
__host__ __device__ inline int pme_lines(int axis, int nx, int ny, int nz) {
    const int n = axis == 0 ? nx : (axis == 1 ? ny : nz);
    const int side = axis == 2 ? nx * ny : nz;
    return PME_POINTS / n < side ? PME_POINTS / n : side;
}

// one line pass.  axis 2: workgroup b holds the lines [b lpw, (b + 1) lpw) of the box's nx ny lines, 1024 points or the whole
// box in a row.  axis 1 (0): workgroup b holds, for one x (y), the lines along y (x) at lpw consecutive z.
__global__ void __launch_bounds__(256) k_pme_fft(PmeArgs p, int axis, int inverse, int first) {
    if (p.w.devflags[DEVFLAG_FROZEN]) return;
    __shared__ double sre[PME_POINTS], sim[PME_POINTS];
    __shared__ double twr[GAMD_PME_TW], twi[GAMD_PME_TW];
    const int tid = threadIdx.x;
    const int n = axis == 0 ? p.nx : (axis == 1 ? p.ny : p.nz);
    const int lgn = __ffs(n) - 1;
    const int lpw = pme_lines(axis, p.nx, p.ny, p.nz), lgl = __ffs(lpw) - 1;
    const int E = lpw << lgn;                               // points of this workgroup, <= 1024
    const size_t G = pme_points(p);
    if ((size_t)blockIdx.x * (size_t)E >= G) return;        // (uniform; cannot happen with the launcher's grid)
    if (tid < GAMD_PME_TW) { twr[tid] = p.tw[2 * tid]; twi[tid] = inverse ? -p.tw[2 * tid + 1] : p.tw[2 * tid + 1]; }
    // the first point of the workgroup and the stride between the points of a line
    size_t base, stride;
    if (axis == 2) { base = (size_t)blockIdx.x * (size_t)E; stride = 1; }
    else {
        const int gz = p.nz >> lgl;                         // workgroups per x (y)
        const size_t o = blockIdx.x / (unsigned)gz, z0 = (size_t)(blockIdx.x % (unsigned)gz) << lgl;
        if (axis == 1) { base = o * (size_t)p.ny * (size_t)p.nz + z0; stride = (size_t)p.nz; }
        else { base = o * (size_t)p.nz + z0; stride = (size_t)p.ny * (size_t)p.nz; }
    }
    const unsigned long long* gq = p.gq + (size_t)blockIdx.y * G;
    double* gc = p.gc + 2 * (size_t)blockIdx.y * G;
    for (int e = tid; e < E; e += 256) {
        int l, k; size_t addr;
        if (axis == 2) { l = e >> lgn; k = e & (n - 1); addr = base + (size_t)e; }
        else { l = e & (lpw - 1); k = e >> lgl; addr = base + (size_t)k * stride + (size_t)l; }
        const int slot = (l << lgn) + (int)(__brev((unsigned)k) >> (32 - lgn));
        if (first) { sre[slot] = (double)(long long)gq[addr] * GAMD_PME_INV_QUANT; sim[slot] = 0.0; }
        else { sre[slot] = gc[2 * addr]; sim[slot] = gc[2 * addr + 1]; }
    }
    for (int s = 1; s <= lgn; ++s) {
        __syncthreads();
        const int half = 1 << (s - 1);
        for (int b = tid; b < (E >> 1); b += 256) {
            const int l = b >> (lgn - 1), jb = b & ((n >> 1) - 1);
            const int pos = jb & (half - 1), grp = jb >> (s - 1);
            const int i0 = (l << lgn) + (grp << s) + pos, i1 = i0 + half;
            const int t = pos << (7 - s);                   // pos * (128 / 2^s)
            const double wr = twr[t], wi = twi[t];
            const double xr = sre[i1], xi = sim[i1];
            const double tr = wr * xr - wi * xi, ti = wr * xi + wi * xr;
            const double ur = sre[i0], ui = sim[i0];
            sre[i0] = ur + tr; sim[i0] = ui + ti;
            sre[i1] = ur - tr; sim[i1] = ui - ti;
        }
    }
    __syncthreads();
    for (int e = tid; e < E; e += 256) {
        int l, k; size_t addr;
        if (axis == 2) { l = e >> lgn; k = e & (n - 1); addr = base + (size_t)e; }
        else { l = e & (lpw - 1); k = e >> lgl; addr = base + (size_t)k * stride + (size_t)l; }
        const int slot = (l << lgn) + k;
        gc[2 * addr] = sre[slot]; gc[2 * addr + 1] = sim[slot];
    }
}

__global__ void __launch_bounds__(256) k_pme_conv(PmeArgs p) {
    const WaterArgs& a = p.w;
    if (a.devflags[DEVFLAG_FROZEN]) return;
    __shared__ double red[4];
    const int box = blockIdx.y;
    const size_t G = pme_points(p);
    const double Lx = gamd_box_edge(a, box, 0), Ly = gamd_box_edge(a, box, 1), Lz = gamd_box_edge(a, box, 2);
    const double pi = 0.5 * a.two_pi, pa2 = (pi * pi) / (a.alpha * a.alpha);
    double* gc = p.gc + 2 * (size_t)box * G;
    double t = 0.0;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < G; idx += (size_t)gridDim.x * 256) {
        const int iz = (int)(idx % (size_t)p.nz), iy = (int)((idx / (size_t)p.nz) % (size_t)p.ny), ix = (int)(idx / ((size_t)p.nz * (size_t)p.ny));
        const double fx = (double)(ix <= p.nx / 2 ? ix : ix - p.nx) / Lx, fy = (double)(iy <= p.ny / 2 ? iy : iy - p.ny) / Ly,
                     fz = (double)(iz <= p.nz / 2 ? iz : iz - p.nz) / Lz;
        const double m2 = (fx * fx + fy * fy) + fz * fz;
        const double B = (p.mod[ix] * p.mod[p.nx + iy]) * p.mod[p.nx + p.ny + iz];
        const double Gm = idx == 0 ? 0.0 : exp(-(pa2 * m2)) / (m2 * B);
        const double re = gc[2 * idx], im = gc[2 * idx + 1];
        t += Gm * (re * re + im * im);
        gc[2 * idx] = Gm * re; gc[2 * idx + 1] = Gm * im;
    }
    t = gamd_wave_sum(t);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double scale = (a.q_h * a.q_h) / (2.0 * (a.two_pi * a.two_pi));       // q_H^2 / 8 pi^2
        a.ublk[(size_t)box * (size_t)a.kblocks + blockIdx.x] = scale * ((red[0] + red[1]) + (red[2] + red[3]));
    }
}

}  // namespace

int launch_water_pme(const PmeArgs& p, hipStream_t st) {
    const WaterArgs& a = p.w;
    PassGeom g;
    if (pass_rows(a, 3, &g)) return -1;
    if (!gamd_pme_order_ok(p.order) || !gamd_pme_length_ok(p.nx) || !gamd_pme_length_ok(p.ny) || !gamd_pme_length_ok(p.nz)) return -1;
    if (a.kslices != 1 || a.kblocks != pme_blocks(p.nx, p.ny, p.nz)) return -1;
    if (!(p.sites || a.x) || !a.species || !a.ublk || !a.rpart || !a.devflags || !p.gq || !p.gc || !p.tw || !p.mod) return -1;
    const size_t G = ((size_t)p.nx * (size_t)p.ny) * (size_t)p.nz;
    const dim3 atoms((unsigned)((g.npb + 256 / PME_LANES - 1) / (256 / PME_LANES)), g.nb);
    hipLaunchKernelGGL(k_pme_clear, dim3((unsigned)(G / 256), g.nb), dim3(256), 0, st, p); GAMD_CHECK_LAUNCH();
    if (p.order == 4) hipLaunchKernelGGL(k_pme_spread4, atoms, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_pme_spread6, atoms, dim3(256), 0, st, p);
    GAMD_CHECK_LAUNCH();
    auto pass = [&](int axis, int inverse, int first) {
        const int n = axis == 0 ? p.nx : (axis == 1 ? p.ny : p.nz);
        const size_t wgs = G / ((size_t)pme_lines(axis, p.nx, p.ny, p.nz) * (size_t)n);
        hipLaunchKernelGGL(k_pme_fft, dim3((unsigned)wgs, g.nb), dim3(256), 0, st, p, axis, inverse, first);
        return (int)hipGetLastError();
    };
    for (int axis = 2; axis >= 0; --axis)
        if (int r = pass(axis, 0, axis == 2)) return r;
    hipLaunchKernelGGL(k_pme_conv, dim3((unsigned)a.kblocks, g.nb), dim3(256), 0, st, p); GAMD_CHECK_LAUNCH();
    for (int axis = 0; axis <= 2; ++axis)
        if (int r = pass(axis, 1, 0)) return r;
    if (p.order == 4) hipLaunchKernelGGL(k_pme_gather4, atoms, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_pme_gather6, atoms, dim3(256), 0, st, p);
    GAMD_CHECK_LAUNCH();
    return 0;
}
