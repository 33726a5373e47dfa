// conv_edge.hip — the edge side of one SmoothConvLayerNew, fully fused:
//
//   e (fragment order) -> edge_affine[Lin,SiLU,Lin] (+ S[src] + D[dst]) -> theta_edge[SiLU,Lin,SiLU,Lin]
//   -> multiply by hn[src] -> per-destination segment sum -> partial-sum pieces
//
// Replaces (reference, code/nn_module.py:135-142): six E-row Linears, two row gathers, two SiLU passes
// and DGL's u_mul_e -> sum SpMM, i.e. ~9 materialised [E,128] temporaries per layer.  src_affine /
// dst_affine are hoisted to node rows (S, D tables, computed by node.hip) — algebraically identical.
//
// Structure: persistent 512-thread workgroups (8 waves, 2 per SIMD), one per CU.  Each wave owns a
// 32-edge tile and carries its activations through four 128x128 fp32 MFMA GEMMs in registers
// (gamd_common.h).  The four weight matrices of the layer (4 x 64 KiB) are streamed L2 -> LDS with
// global_load_lds into a two-slot ring, one matrix ahead of the GEMM that consumes it; one
// workgroup barrier per GEMM phase.
//
// What the schedule is built around (profiles/r01_conv_edge_cycles.md, r02_ / r03_conv_edge_experiments.md):
// the two waves of a SIMD serialise their MFMA streams — whoever gets the matrix pipe first after a barrier keeps it
// until its GEMM is done, then the other one runs.  A phase therefore costs 2 GEMMs + whatever sits between the barrier
// and the first MFMA.  So:
// (1) everything a GEMM needs besides its LDS weights is loaded a phase ahead, into whichever of the three 64-register
// sets is free — by waves 0-3 BEFORE the barrier (the loads stay in flight across it: raw s_barrier + counted vmcnt),
// by waves 4-7 right AFTER it (see "Gather schedule" below);
// (2) nothing but the accumulator initialisation stands between a barrier and the first MFMA: the weight copy for the
// next phase, the piece stores of the previous tile and the D[dst] gather are issued 64 MFMAs INTO the GEMM (mid()
// hook).  In front of the GEMM they queued behind the other waves' gathers on the CU's address path, and the 8 x 3
// loop-invariant SGPRs of the per-copy addresses were restored from VGPR lanes (two v_readlane per copy) on that
// critical stretch; the copy now takes one base pair + immediate offsets (gamd_stage_weight_raw_contig);
// (3) element-wise post-ops (SiLU, message, segment sum) of output tile tp-1 are issued between the MFMA groups of tile
// tp.  fp32 MFMA and VALU share the SIMD's lanes, so this hides latency, not work: the kernel without any post-op runs
// at 0.87-0.89 of the matrix peak, with them at 0.81 (timing ablations in r03_conv_edge_experiments.md).
//
// The last GEMM runs in the F2 orientation so each lane ends up with 16 edges x 4 features: the
// multiply by hn[src] and the segment sum are in-lane, and every maximal run of edges (same
// destination, same 16-edge chunk) is written once as a "piece".  Pieces are summed per atom, in
// order, by the node kernel -> no atomics, bit-reproducible.
//
// Roofline: MFMA-bound.  8*128*128 = 131072 FLOP per edge per launch against ~1.6 KB of traffic.
//
// Layer-0 form (L0, LJ models only: every atom enters layer 0 with the same row hn0, so S[src] = S0, D[dst] = D0 and
// hn[src] = hn0 for every edge): the message is hn0 * (W4 T3 + b4), and phi_edge of its per-atom sum is
// M0 sum_j T3_j + d_i c0 with M0 = W_pe diag(hn0) W4, c0 = W_pe (hn0 * b4) (gamd_finalize_weights).  The kernel runs
// three GEMMs per tile instead of four (6*128*128 = 98304 FLOP per edge), the third in the F2 orientation with the segment
// sum of SiLU(W3 T2 + b3) over the REAL edges as its post-op, and the node kernel applies M0 and d_i c0 (node.hip).  S0 /
// D0 are row 0 of the layer's S / D tables; their sum is phase 2's accumulator start (wide.hip's order: (S + D), then the
// GEMM), kept in LDS.  Nothing is gathered per edge.
#include "gamd_common.h"
#include "gamd_internal.h"

#include <cstdlib>

namespace {

// two 64 KiB weight slots and b1, b3, b4 (L0: b1, b3, S0 + D0)
// (folded edge LayerNorm: + the weight fragment of phase 1's extra K step, 4 output blocks x 64 lanes)
constexpr int conv_lds_floats(bool l0, bool fold = false) { return 2 * GAMD_WFRAG_FLOATS + 3 * 128 + (fold ? 256 : 0); }

// 128x128 GEMM of the chain with a software-pipelined element-wise post-op: while output tile tp is being accumulated (64
// MFMAs in 16 groups of 4), post(tp-1, g) finishes element g of the previous, already complete, output tile.  Only tile 3's
// post-op trails the last MFMA.
// mid() runs once, between output tiles 0 and 1 (64 MFMAs into the GEMM): memory instructions that are due "some time
// during this phase" (the weight copy for the next phase, piece stores, C-in gathers) are issued there instead of in front
// of the first MFMA, where they would queue behind the other waves' gathers on the CU's address path and keep the matrix
// pipe idle after every barrier.
// tail(tp) runs behind the 64 MFMAs of output tile tp, before anything reads it: further K steps of that tile.
template <bool F2, typename Post, typename Mid, typename Tail>
__device__ __forceinline__ void gemm128_post(const f32x4* W, int lane, const f32x16 (&X)[4], f32x16 (&acc)[4], Post post, Mid mid, Tail tail) {
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) {
        if (tp == 1) mid();
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 w = W[((tp * 4 + t) * 4 + q) * 64 + lane];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float x = X[t][q * 4 + j];
                    acc[tp] = F2 ? mfma32(x, w[j], acc[tp]) : mfma32(w[j], x, acc[tp]);
                }
                if (tp > 0) post(tp - 1, t * 4 + q);
            }
        }
        tail(tp);
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) post(3, g);
}
template <bool F2, typename Post, typename Mid>
__device__ __forceinline__ void gemm128_post(const f32x4* W, int lane, const f32x16 (&X)[4], f32x16 (&acc)[4], Post post, Mid mid) {
    gemm128_post<F2>(W, lane, X, acc, post, mid, [](int) {});
}

// End of a phase: every wave has its own weight DMA (issued during the phase, before the N most
// recent VMEM loads) landed, then the workgroup meets.  The N prefetch loads stay in flight.
// vmcnt retires in order, so "at most N outstanding" proves the older DMA is done only if at least
// N loads really were issued after it: callers pass 0 on paths that skip the prefetch.
template <int N>
__device__ __forceinline__ void phase_barrier() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
    __builtin_amdgcn_s_barrier();
}

__device__ __forceinline__ void load_e_tile(const float* __restrict__ e_frag, int tile, int lane, f32x16 (&X)[4]) {
    const f32x4* ef = (const f32x4*)e_frag + (size_t)tile * 16 * 64;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 v = gamd_load_stream(&ef[(t * 4 + q) * 64 + lane]);
#pragma unroll
            for (int j = 0; j < 4; ++j) X[t][q * 4 + j] = v[j];
        }
}

// Gather schedule.  Of the two waves of a SIMD the one with the lower id is served first after a barrier (measured:
// waves 0-3 wait ~18 000 ticks at the barrier behind their own GEMM, waves 4-7 wait as long in front of theirs).  A gather
// (32 distinct rows per instruction) or a streaming prefetch occupies the CU's address path for thousands of cycles, and
// whatever a wave issues next queues behind it.  So:
//   * waves 0-3 issue the gathers for the next phase right after their GEMM, BEFORE the barrier: the address path is idle
//     then (waves 4-7 are in their GEMM) and the loads are long done when the barrier opens;
//   * waves 4-7 reach the barrier last; gathers issued there would sit in the queue in front of the next phase.  They issue
//     them AFTER the barrier, at the start of the phase, where they have a whole GEMM of waiting in front of them anyway;
//   * the weight copy of the phase after next is issued by every wave 64 MFMAs into its GEMM, behind the gathers.
// (Other schedules that were measured and dropped are recorded in profiles/r02_ / r03_conv_edge_experiments.md.)
// TIME (profiling build only, GAMD_CONV_TIME): per-segment s_memtime counters -> a.tdbg.
// L0: the layer-0 form of LJ models (see the top of the file; a.b3 and a.w3p are then packed in the F2 output order).
// FOLD: the folded edge LayerNorm (gamd_ln_fold_host.h).  The tile is x2' = rstd x2, a.w1p is A = W1 diag(gamma) B
// followed by the fragment (a, 0) of one extra K step, a.b1 = b1 + W1 beta; the step's other operand is the tile's rstd
// fragment (a.e_rstd: lanes 0-31 rstd, lanes 32-63 zero), loaded with the tile and held in one register through phase 1.
// Everything behind phase 1's accumulators is the general form's.
template <bool TIME, bool L0, bool FOLD = false>
__global__ void __launch_bounds__(512, 2) k_conv_edge(ConvEdgeArgs a) {
    if (a.devflags[DEVFLAG_FROZEN]) return;          // frozen run: nothing to compute until the host has regrown and resumed
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // L0: the three vectors (b1, b3, S0 + D0) in front of the weight slots, where every lane's address of them is one register
    // + an immediate offset (behind 128 KiB each needs registers of its own)
    float* buf0 = lds + (L0 ? 3 * 128 + (FOLD ? 256 : 0) : 0);
    float* buf1 = buf0 + GAMD_WFRAG_FLOATS;
    float* vb1 = L0 ? lds : buf1 + GAMD_WFRAG_FLOATS;
    float* vb3 = vb1 + 128;
    float* vb4 = vb3 + 128;
    float* vSD0 = vb4;                // L0: no W4, its slot holds S0 + D0
    float* vax = vb4 + 128;           // FOLD: (a, 0) per output block, lane order

    const int tid = threadIdx.x, lane = tid & 63, slot = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned lane16 = (unsigned)lane * 16u;
    int E = a.counters[CNT_E];
    if ((long long)E > a.e_cap) E = (int)a.e_cap;
    const int n_tiles = (E + GAMD_TILE - 1) / GAMD_TILE;
    // Work unit = 4 tiles, one per SIMD.  Waves 0-3 and 4-7 of the workgroup take successive units of its list, so
    // the work is balanced to half an iteration (an iteration with only waves 0-3 active takes about half the
    // time: the two waves of a SIMD serialise their MFMA streams anyway).
    const int n_units = (n_tiles + 3) / 4;
    int first, end, step;
    gamd_xcd_range(n_units, blockIdx.x, gridDim.x, first, end, step);
    if (first >= end) return;
    const int n_iter = ((end - first + step - 1) / step + 1) / 2;
    const int wsub = wave & 3, whalf = wave >> 2;
    const bool early = whalf == 0;                  // gathers before (true) / after (false) the barrier
    auto tile_of = [&](int it) {              // this wave's tile in iteration `it`, or n_tiles (inactive)
        const int u = first + (2 * it + whalf) * step;
        return (it < n_iter && u < end) ? u * 4 + wsub : n_tiles;
    };
    // L2 -> LDS copy of the next phase's weight matrix
    auto stage = [&](const float* gw, float* buf) { gamd_stage_weight_raw_contig<8>(gw, buf, wave, lane16); };

    long long tacc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) tacc[i] = 0;
    long long tprev = 0;
#define TMARK(i) do { if (TIME) { const long long tn__ = (long long)__builtin_readcyclecounter(); tacc[i] += tn__ - tprev; tprev = tn__; } } while (0)

    // (FOLD: the extra K step's fragment, loaded in front of the bias vectors and stored behind them: one round trip for all)
    float vax_t = 0.f;
    if (FOLD && tid < 256) vax_t = a.w1p[GAMD_WFRAG_FLOATS + tid];
    if (tid < 128) {
        vb1[tid] = a.b1[tid]; vb3[tid] = a.b3[tid];
        if (L0) vSD0[tid] = a.S[tid] + a.D[tid];
        else vb4[tid] = a.b4[tid];
    }
    if (FOLD && tid < 256) vax[tid] = vax_t;
    stage(a.w1p, buf0);

    // three 64-register sets rotate through the roles {GEMM input, GEMM output, prefetched gather}
    f32x16 RA[4], RB[4], RC[4];
    float rs = 0.f;                   // FOLD: the rstd fragment of the tile in RA
    // FOLD: phase 1's extra K step on output tile tp
    // (its weight fragment is read with the accumulator start, in front of the GEMM: read where it is used, each of the four
    // MFMAs waits out an LDS round trip -- measured +7 us per launch at C2 instead of +3)
    float wxr[4] = {0.f, 0.f, 0.f, 0.f};
    auto fold_head = [&]() {
        if constexpr (FOLD) {
#pragma unroll
            for (int tp = 0; tp < 4; ++tp) wxr[tp] = vax[tp * 64 + lane];
            asm volatile("" : "+v"(wxr[0]), "+v"(wxr[1]), "+v"(wxr[2]), "+v"(wxr[3]));      // (hipcc sinks the reads back otherwise)
        }
    };
    auto fold_tail = [&](int tp) { if constexpr (FOLD) RB[tp] = mfma32(wxr[tp], rs, RB[tp]); };
    auto init_b4 = [&]() {
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) {
            const float b = vb4[32 * tp + slot];
#pragma unroll
            for (int r = 0; r < 16; ++r) RC[tp][r] = b;
        }
    };

    // per-lane edge of the current tile (slot order) and prefetch for the first tile; padding slots of the last tile gather
    // the all-zero row n (their messages are exact zeros)
    int tile = tile_of(0);
    bool active = tile < n_tiles;
    int src = 0, dst = 0;
    {
        const int x = tile * GAMD_TILE + gamd_pi(slot);
        if (active && x < E) {
            src = GAMD_CHK_RANGE(a.sticky, a.col[x], 0, a.zero_row, GAMD_CHK_CONV_SRC);
            if (!L0) dst = GAMD_CHK_RANGE(a.sticky, a.erow[x], 0, a.zero_row, GAMD_CHK_CONV_DST);
        } else { src = a.zero_row; dst = a.zero_row; }
        if (FOLD && active) rs = a.e_rstd[(size_t)tile * 64 + lane];
        if (active) load_e_tile(a.e_frag, tile, lane, RA);
    }
    asm volatile("" ::"v"(src), "v"(dst));      // compiler-visible wait for the index loads (see phase 4)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (TIME) tprev = (long long)__builtin_readcyclecounter();
    unsigned pend_ends = 0;           // piece stores of the tile just finished (issued after its last barrier)
    int pend_p = 0;

    // S[src] rows, phase 2's post-op (chain layout, -> RA)
    auto gather_S = [&]() { load_row_chain(a.S + (size_t)src * GAMD_H, half, RA); };
    // hn[src] rows for phase 4 (-> RA; row layout: lane = features 4 slot .. 4 slot + 3 -- W4's output rows are packed in
    // that order, gamd_finalize_weights -- reg = edge): one 16-byte load per edge; the source index of edge (half, r)
    // lives in lane rho(r, half) = (r & 3) + 8 (r >> 2) + 4 half of `src`.  ONE index register: ds_bpermute's immediate
    // offset selects the lane (hipcc materialises the 16 lane indices of __shfl as 16 loop-invariant VGPRs), the byte offset
    // src * 512 is what travels, and the load takes the scalar base + 32-bit offset form (one v_add per edge instead of sign
    // extension + 64-bit shift + 64-bit add).
    auto gather_hn = [&]() {
        const unsigned soff = (unsigned)src << 9;
        const unsigned idx0 = 16u * (unsigned)half;                  // bpermute address = 4 * lane: lanes 4 half + ...
        const unsigned slot16 = 16u * (unsigned)slot;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            unsigned o0, o1, o2, o3;
            asm volatile("ds_bpermute_b32 %0, %4, %5 offset:%6\n\tds_bpermute_b32 %1, %4, %5 offset:%7\n\t"
                         "ds_bpermute_b32 %2, %4, %5 offset:%8\n\tds_bpermute_b32 %3, %4, %5 offset:%9\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(o0), "=&v"(o1), "=&v"(o2), "=&v"(o3)
                         : "v"(idx0), "v"(soff), "n"(4 * (0 + 8 * r4)), "n"(4 * (1 + 8 * r4)), "n"(4 * (2 + 8 * r4)), "n"(4 * (3 + 8 * r4)));
            const unsigned o[4] = {o0, o1, o2, o3};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const f32x4 hv = *(const f32x4*)((const char*)a.hn + (o[k] + slot16));
#pragma unroll
                for (int tp = 0; tp < 4; ++tp) RA[r4][k * 4 + tp] = hv[tp];
            }
        }
    };

    // Phase boundary of a wave that gathers early: barrier after its gathers (every wave's share of the weight copy issued
    // during the phase has landed: at most 16 younger VMEM loads -- the gathers -- may still be in flight).  Late waves pass
    // phase_barrier<0> BEFORE their gathers: the branch is around the barrier, not around the loads, so both groups run the
    // same gather code into the same registers.
    auto early_barrier = [&](bool gathered) { if (gathered) phase_barrier<16>(); else phase_barrier<0>(); };
    // the same behind the next tile's loads: FOLD adds the rstd fragment to the 16 loads of the tile
    auto early_barrier_e = [&](bool gathered) { if (gathered) phase_barrier<FOLD ? 17 : 16>(); else phase_barrier<0>(); };
    // one store per finished piece of the previous tile: closing edges (mask bits) and, if the chunk's last valid edge does
    // not close a segment, that edge too (the run continues in the next chunk as its own piece)
    auto piece_stores = [&]() {
        while (__any(pend_ends != 0)) {
            if (pend_ends != 0) {
                const int r = __builtin_ctz(pend_ends);
                pend_ends &= pend_ends - 1;
                f32x4 pv;
#pragma unroll
                for (int tp = 0; tp < 4; ++tp) {
                    float v = RC[tp][0];
#pragma unroll
                    for (int k = 1; k < 16; ++k) v = (r == k) ? RC[tp][k] : v;
                    pv[tp] = v;
                }
                *(f32x4*)(a.partial + (size_t)pend_p * GAMD_H + 4 * slot) = pv;
                ++pend_p;
            }
        }
    };
    // What a phase owes the memory system is issued 64 MFMAs into its GEMM (the mid() hook, fenced); inactive waves still
    // owe their share of the weight copy (the `else` branches below)
#define FENCE() __builtin_amdgcn_sched_barrier(0)

    if constexpr (L0) {
    // Layer-0 form: three phases per tile, three matrices through the two LDS slots, so the slot parity flips every tile
    // (W1 -> x, W2 -> y, W3 -> x, next tile's W1 -> y).  Registers: RA = e, then T2; RB = T1; RC = the pieces of the previous
    // tile until phase 1's mid(), then this tile's pieces.  The only per-edge loads are e and the 4-byte indices.
    for (int it = 0; it < n_iter; ++it) {
        const int x0 = tile * GAMD_TILE + 16 * half;
        int nvalid = E - x0;
        nvalid = !active ? 0 : (nvalid >= 16 ? 16 : (nvalid <= 0 ? 0 : nvalid));
        const int tile_n = tile_of(it + 1);
        const bool active_n = tile_n < n_tiles;
        int src_n = a.zero_row;
        float* const bx = (it & 1) ? buf1 : buf0;              // W1, then W3
        float* const by = (it & 1) ? buf0 : buf1;              // W2, then the next tile's W1

        // ===== phase 1: RB = SiLU(W1 e + b1)        in RA = e, RC = pieces of the previous tile =====
        if (active) {
            load_bias_chain(vb1, half, RB);
            fold_head();
            TMARK(0);
            gemm128_post<false>((const f32x4*)bx, lane, RA, RB,
                                [&](int tp, int g) { RB[tp][g] = gamd_silu_hw(RB[tp][g]); },
                                [&]() { FENCE(); piece_stores(); stage(a.w2p, by); FENCE(); }, fold_tail);
            TMARK(1);
        } else {
            piece_stores();
            stage(a.w2p, by);
        }
        // boundary 1: piece stores and the copy of W2 have landed (nothing younger is issued)
        phase_barrier<0>();
        TMARK(2);
        // ===== phase 2: RA = SiLU(W2 T1 + (S0 + D0))        in RB =====
        unsigned mask = 0;
        int p0 = 0;
        // accumulator start first (fenced: LDS reads behind the index loads would make hipcc wait for them), then the index
        // loads for phase 3 / the next tile: done long before boundary 2 needs vmcnt(0)
        if (active) { load_bias_chain(vSD0, half, RA); FENCE(); }
        if (active) {
            mask = a.chunk_mask[tile * 2 + half];
            p0 = GAMD_CHK_RANGE(a.sticky, a.chunk_piece[tile * 2 + half], 0, a.piece_cap - 17, GAMD_CHK_PIECE);
        }
        if (active_n) {
            const int xn = tile_n * GAMD_TILE + gamd_pi(slot);
            if (xn < E) src_n = GAMD_CHK_RANGE(a.sticky, a.col[xn], 0, a.zero_row, GAMD_CHK_CONV_SRC);
        }
        if (active) {
            gemm128_post<false>((const f32x4*)by, lane, RB, RA,
                                [&](int tp, int g) { RA[tp][g] = gamd_silu_hw(RA[tp][g]); },
                                [&]() { FENCE(); stage(a.w3p, bx); FENCE(); });
            TMARK(4);
        } else {
            stage(a.w3p, bx);
        }
        // boundary 2: the index loads and the copy of W3 have landed
        phase_barrier<0>();
        // (the compiler cannot see the wait written in assembly: naming the registers makes it emit its own here, where it
        // costs nothing, instead of in front of the piece-store loop or the next tile's ballot)
        asm volatile("" ::"v"(mask), "v"(p0), "v"(src_n));
        TMARK(5);
        // ===== phase 3: RC = T2 W3^T + b3 (F2: 16 edges x 4 features per lane), SiLU, segment sum over the real edges =====
        if (active) {
            // Padding slots -- the tail of the last tile, a box's padding in a batch -- have src == zero_row.  Nothing
            // multiplies them by hn[zero_row] = 0 any more: they start from GAMD_L0_PAD instead of b3 (F2 row r = CSR edge
            // x0 + r, whose index sits in chain lane rho(r, half) = (r & 3) + 8 (r >> 2) + 4 half) and add exactly -0.
            const unsigned bl = (unsigned)__ballot(src != a.zero_row) >> (4 * half);
            const unsigned real = (bl & 0xFu) | ((bl >> 4) & 0xF0u) | ((bl >> 8) & 0xF00u) | ((bl >> 12) & 0xF000u);
#pragma unroll
            for (int tp = 0; tp < 4; ++tp) {
                const float b = vb3[32 * tp + slot];
#pragma unroll
                for (int r = 0; r < 16; ++r) RC[tp][r] = ((real >> r) & 1u) ? b : GAMD_L0_PAD;
            }
            TMARK(7);
            const unsigned keep_bits = ~(mask << 1);          // bit r set: edge r continues edge r-1's piece
            gemm128_post<true>((const f32x4*)bx, lane, RA, RC, [&](int tp, int r) {
                RC[tp][r] = gamd_l0_acc(RC[tp][r], (r > 0 && ((keep_bits >> r) & 1u)) ? RC[tp][r - 1] : 0.f);
            }, [&]() { FENCE(); if (it + 1 < n_iter) stage(a.w1p, by); FENCE(); });
            pend_ends = mask;
            if (nvalid > 0 && !((mask >> (nvalid - 1)) & 1u)) pend_ends |= 1u << (nvalid - 1);
            pend_p = p0;
            TMARK(10);
        } else {
            if (it + 1 < n_iter) stage(a.w1p, by);
        }
        // boundary 3: the next tile's e -> RA.  Younger than the copy of W1: e (early waves)
        if (!early) phase_barrier<0>();
        TMARK(11);
        if (FOLD && active_n) rs = a.e_rstd[(size_t)tile_n * 64 + lane];      // (first: its wait is the tile's first)
        if (active_n) load_e_tile(a.e_frag, tile_n, lane, RA);
        TMARK(12);
        if (early) early_barrier_e(active_n);
        TMARK(13);
        tile = tile_n; active = active_n; src = src_n;
    }
    } else {
    for (int it = 0; it < n_iter; ++it) {
        const int x0 = tile * GAMD_TILE + 16 * half;            // this half's 16 CSR edges: x0 + r
        int nvalid = E - x0;
        nvalid = !active ? 0 : (nvalid >= 16 ? 16 : (nvalid <= 0 ? 0 : nvalid));
        // next tile of this wave (indices prefetched during phase 3)
        const int tile_n = tile_of(it + 1);
        const bool active_n = tile_n < n_tiles;
        int src_n = a.zero_row, dst_n = src_n;      // padding slots: the all-zero row

        // ===== phase 1: RB = SiLU(W1 e + b1)        in RA = e (prefetched), RC = pieces of the previous tile =====
        if (active) {
            load_bias_chain(vb1, half, RB);
            fold_head();
            TMARK(0);
            gemm128_post<false>((const f32x4*)buf0, lane, RA, RB,
                                [&](int tp, int g) { RB[tp][g] = gamd_silu_hw(RB[tp][g]); },
                                [&]() {                 // previous tile's pieces out of RC, then D[dst] (C-in of phase 2) into it, W2 -> buf1
                                    FENCE();
                                    piece_stores();
                                    load_row_chain(a.D + (size_t)dst * GAMD_H, half, RC);
                                    stage(a.w2p, buf1);
                                    FENCE();
                                }, fold_tail);
            TMARK(1);
        } else {
            piece_stores();
            stage(a.w2p, buf1);
        }
        // boundary 1: S[src] -> RA for phase 2's post-op.  Younger than the copy of W2: S (early waves)
        if (!early) phase_barrier<0>();
        TMARK(2);
        if (active) gather_S();
        TMARK(3);
        if (early) early_barrier(active);
        // ===== phase 2: RC = SiLU(W2 T1 + D[dst] + S[src])        in RB, S in RA =====
        if (active) {
            gemm128_post<false>((const f32x4*)buf1, lane, RB, RC,
                                [&](int tp, int g) { RC[tp][g] = gamd_silu_hw(RC[tp][g] + RA[tp][g]); },
                                [&]() { FENCE(); stage(a.w3p, buf0); FENCE(); });
            TMARK(4);
        } else {
            stage(a.w3p, buf0);
        }
        // boundary 2: hn[src] -> RA for phase 4.  Younger than the copy of W3: hn (early waves)
        if (!early) phase_barrier<0>();
        TMARK(5);
        if (active) gather_hn();
        TMARK(6);
        if (early) early_barrier(active);
        // ===== phase 3: RB = SiLU(W3 T3 + b3)        in RC =====
        unsigned mask = 0;
        int p0 = 0;
        // small index loads for phase 4 / the next tile go first: done long before the barrier needs vmcnt(0)
        if (active) {
            mask = a.chunk_mask[tile * 2 + half];
            p0 = GAMD_CHK_RANGE(a.sticky, a.chunk_piece[tile * 2 + half], 0, a.piece_cap - 17, GAMD_CHK_PIECE);
        }
        if (active_n) {
            const int xn = tile_n * GAMD_TILE + gamd_pi(slot);
            if (xn < E) { src_n = GAMD_CHK_RANGE(a.sticky, a.col[xn], 0, a.zero_row, GAMD_CHK_CONV_SRC); dst_n = GAMD_CHK_RANGE(a.sticky, a.erow[xn], 0, a.zero_row, GAMD_CHK_CONV_DST); }
        }
        if (active) {
            load_bias_chain(vb3, half, RB);
            TMARK(7);
            gemm128_post<false>((const f32x4*)buf0, lane, RC, RB,
                                [&](int tp, int g) { RB[tp][g] = gamd_silu_hw(RB[tp][g]); },
                                [&]() { FENCE(); stage(a.w4p, buf1); FENCE(); });
            TMARK(8);
        } else {
            stage(a.w4p, buf1);
        }
        // boundary 3 (nothing to gather): everything has landed behind it
        phase_barrier<0>();
        // The index loads of phase 3 are complete, but hipcc cannot see a wait written in assembly: it would keep them on
        // its scoreboard and later flush vmcnt(0) — in front of the piece-store loop, at the next tile's first use of src,
        // and before it re-initialises src_n.  Naming the registers here makes it emit its wait now, where it costs nothing.
        asm volatile("" ::"v"(mask), "v"(p0), "v"(src_n), "v"(dst_n));
        TMARK(9);
        // ===== phase 4: RC = T4 W4^T + b4 (F2: 16 edges x 4 features per lane), message, segment sum =====
        if (active) {
            init_b4();
            // e_emb for this lane's 16 edges x 4 features, then message + segment sum (nn_module.py:142
            // u_mul_e -> sum).  In-stream part is branch-free: RC[tp][r] becomes the running sum of the
            // messages of the current piece (reset after every edge that closes a destination segment).
            // Padding edges (r >= nvalid, last tile only) gathered hn[zero_row] = 0: their products are exact zeros.
            const unsigned keep_bits = ~(mask << 1);          // bit r set: edge r continues edge r-1's piece
            gemm128_post<true>((const f32x4*)buf1, lane, RB, RC, [&](int tp, int r) {
                RC[tp][r] = gamd_msg_acc(RA[r >> 2][(r & 3) * 4 + tp], RC[tp][r], (r > 0 && ((keep_bits >> r) & 1u)) ? RC[tp][r - 1] : 0.f);
            }, [&]() { FENCE(); if (it + 1 < n_iter) stage(a.w1p, buf0); FENCE(); });
            // piece stores are deferred past the boundary (vmcnt counts stores too: issued here they would sit in front of
            // the prefetch loads and a counted wait would wait for their write latency)
            pend_ends = mask;
            if (nvalid > 0 && !((mask >> (nvalid - 1)) & 1u)) pend_ends |= 1u << (nvalid - 1);
            pend_p = p0;
            TMARK(10);
        } else {
            if (it + 1 < n_iter) stage(a.w1p, buf0);
        }
        // boundary 4: the next tile's e -> RA.  Younger than the copy of W1: e (early waves)
        if (!early) phase_barrier<0>();
        TMARK(11);
        if (FOLD && active_n) rs = a.e_rstd[(size_t)tile_n * 64 + lane];      // (first: its wait is the tile's first)
        if (active_n) load_e_tile(a.e_frag, tile_n, lane, RA);
        TMARK(12);
        if (early) early_barrier_e(active_n);
        TMARK(13);
        tile = tile_n; active = active_n; src = src_n; dst = dst_n;
    }
    }
#undef FENCE
    piece_stores();            // the last tile's pieces
    if (TIME && a.tdbg && lane == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) a.tdbg[((size_t)blockIdx.x * 8 + wave) * 16 + i] = tacc[i];
    }
#undef TMARK
}

template <bool TIME, bool L0, bool FOLD = false>
int launch(const ConvEdgeArgs& a, int n_blocks, hipStream_t st) {
    const size_t lds = sizeof(float) * conv_lds_floats(L0, FOLD);
    static PerDeviceOnce once;
    if (int e = gamd_allow_dynamic_lds(once, (int)lds, k_conv_edge<TIME, L0, FOLD>)) return e;
    hipLaunchKernelGGL((k_conv_edge<TIME, L0, FOLD>), dim3(n_blocks), dim3(512), lds, st, a);
    GAMD_CHECK_LAUNCH();
    return 0;
}

}  // namespace

int launch_conv_edge(const ConvEdgeArgs& a, int n_blocks, hipStream_t st) {
#ifdef GAMD_PROFILING
    static const bool timed = getenv("GAMD_CONV_TIME") != nullptr;
    if (timed) return a.e_rstd ? launch<true, false, true>(a, n_blocks, st) : launch<true, false>(a, n_blocks, st);
#endif
    return a.e_rstd ? launch<false, false, true>(a, n_blocks, st) : launch<false, false>(a, n_blocks, st);
}

int launch_conv_edge_l0(const ConvEdgeArgs& a, int n_blocks, hipStream_t st) {
#ifdef GAMD_PROFILING
    static const bool timed = getenv("GAMD_CONV_TIME") != nullptr;
    if (timed) return a.e_rstd ? launch<true, true, true>(a, n_blocks, st) : launch<true, true>(a, n_blocks, st);
#endif
    return a.e_rstd ? launch<false, true, true>(a, n_blocks, st) : launch<false, true>(a, n_blocks, st);
}
