// gamd_internal.h — kernel argument blocks and launcher prototypes shared by the .hip translation
// units of libgamd_hip.so.  Not part of the public C ABI (that is include/gamd_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "gamd_common.h"

enum { CNT_E = 0, CNT_PIECES = 1, CNT_OVERFLOW = 2, CNT_TILES = 3, CNT_REBUILD = 4, CNT_NCAND = 5,
       CNT_CAND_MAX = 6,      // fixed-stride candidate rows: the longest row of the rebuild of this call
       CNT_COUNT = 8 };
// host-mapped, never cleared by the per-call memset: overflow must survive later steps of an enqueued MD run
enum { STICKY_EDGE_OVERFLOW = 0, STICKY_CAND_OVERFLOW = 1, STICKY_REBUILDS = 2, STICKY_NCAND = 3,
       STICKY_NONFINITE = 4,   // the decoder produced a non-finite force component (NaN / inf positions, or an operand
                               // beyond the fp16 range in the split-fp16 edge MLP, which turns into inf / NaN downstream)
       // checked build (-DGAMD_CHECKED, libgamd_hip_chk.so): the first device-side range check that failed — its code (the
       // GAMD_CHK_* ids below), the offending value and the source line.  Never written by the release build.
       STICKY_CHECK_CODE = 5, STICKY_CHECK_VALUE = 6, STICKY_CHECK_LINE = 7,
       STICKY_COUNT = 8 };
// ---- checked build ----------------------------------------------------------------------------------------------------
// SURVEY.md section 5 ("add a debug build with bounds checks"; the reference's only failure handling is the overflow test of
// graph_utils.py:41-42).  `make checked` compiles every kernel with -DGAMD_CHECKED: each index that a kernel READS FROM MEMORY and
// then uses as an address (CSR source / destination atoms, candidate rows, cell numbers, permutations, piece numbers, CSR write
// positions) passes through GAMD_CHK_RANGE, which records the first violation in the host-mapped sticky block and returns a safe
// value instead (no wild access, no trap: the process survives and gamd_sync_status / the synchronous entry points return -35
// with code, value and line).  In the release build the macro is the identity: same instructions as without it.
enum { GAMD_CHK_CELL = 101, GAMD_CHK_CAND = 102, GAMD_CHK_EDGE_POS = 103, GAMD_CHK_PERM = 104, GAMD_CHK_ENC_SRC = 111, GAMD_CHK_ENC_DST = 112,
       GAMD_CHK_CONV_SRC = 121, GAMD_CHK_CONV_DST = 122, GAMD_CHK_PIECE = 123, GAMD_CHK_NODE_PIECES = 131, GAMD_CHK_INJECTED = 199 };
#ifdef GAMD_CHECKED
template <typename T>
__device__ __forceinline__ T gamd_chk_range(int* sticky, T v, long long lo, long long hi, int code, int line) {
    if ((long long)v >= lo && (long long)v <= hi) return v;
    if (sticky && sticky[STICKY_CHECK_CODE] == 0) {          // first failure wins (a benign race between failing lanes)
        sticky[STICKY_CHECK_VALUE] = (int)v;
        sticky[STICKY_CHECK_LINE] = line;
        __threadfence_system();
        sticky[STICKY_CHECK_CODE] = code;
    }
    return (T)lo;
}
#define GAMD_CHK_RANGE(sticky, v, lo, hi, code) gamd_chk_range((sticky), (v), (long long)(lo), (long long)(hi), (code), __LINE__)
#else
#define GAMD_CHK_RANGE(sticky, v, lo, hi, code) (v)
#endif
// device-resident flags, cleared by the host only (gamd_create, after a regrow):
//   DEVFLAG_FROZEN     a neighbour buffer (edges or candidates) overflowed: the CSR of that call is truncated.  Node kernels
//                      and every integrator kernel return without touching their outputs while it is set, so an enqueued MD
//                      run stops at the last consistent state instead of integrating stale forces
//   DEVFLAG_FROZEN_AT  2 * (index of the step inside the md_run call) + (0: before its first half, 1: before its second
//                      half) of the first integrator kernel that found the flag set, -1 if none did: where to resume
//   DEVFLAG_REBUILDS   candidate rebuilds so far, counted HERE (device memory) and published to the host-mapped sticky block by a
//                      plain store: a read-modify-write on the host-mapped word is a PCIe read in the middle of a single-
//                      workgroup kernel — measured ~200 us per rebuild step (round 5).  Never cleared.
enum { DEVFLAG_FROZEN = 0, DEVFLAG_FROZEN_AT = 1, DEVFLAG_REBUILDS = 2, DEVFLAG_COUNT = 4 };

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a property of (kernel, DEVICE): a process that holds handles on several
// devices (gamd_config.device; SURVEY.md 8e "one stream per device from one process") must raise the limit on each of them, or
// the second device launches > 64 KiB of dynamic LDS without it.  One flag per device and kernel instantiation; launchers run
// under the handle's DeviceGuard, so the current device is the one the launch goes to.
// Different handles may be driven from different threads (include/gamd_hip.h): two threads can make their first launch of a
// kernel on one device at the same time, so the flags are atomics (relaxed: hipFuncSetAttribute is idempotent, a lost race
// only repeats it).
constexpr int GAMD_MAX_DEVICES = 64;
struct PerDeviceOnce { std::atomic<bool> done[GAMD_MAX_DEVICES] = {}; };
template <typename... Fn>
inline int gamd_allow_dynamic_lds(PerDeviceOnce& once, int bytes, Fn... fns) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (dev >= 0 && dev < GAMD_MAX_DEVICES && once.done[dev].load(std::memory_order_relaxed)) return 0;
    const void* list[] = {(const void*)fns...};
    for (const void* fn : list) {
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return (int)e;
    }
    if (dev >= 0 && dev < GAMD_MAX_DEVICES) once.done[dev].store(true, std::memory_order_relaxed);
    return 0;
}

// ---- several independent boxes in one set of launches (gamd_config.n_boxes > 1) -----------------------------------------
// Box b owns atoms [b * n_per_box, (b + 1) * n_per_box) in the caller's order AND in the sorted order (cells are numbered
// box-major: cell = first cell of box b + local cell, and every box holds exactly n_per_box atoms).  boxes[3 b] = (Lx, Ly, Lz, 0),
// boxes[3 b + 1] = (Lx / 2, Ly / 2, Lz / 2, 0), boxes[3 b + 2] = the bits of int4 (cells along x, y, z, first cell of box b):
// every box has the cell grid a single-box handle would give it, so its CSR rows come out in the same order.
// n_boxes <= 1: the by-value box of the argument block is used and nothing below is read.  The reference evaluates several graphs per forward through build_graph_batches + dgl.batch
// (nn_module.py:655-661, :520-527); here they share every launch.
struct BoxRef {
    int n_boxes, n_per_box;
    float inv_npb;             // 1 / n_per_box
    const float4* boxes;       // device, [n_boxes][3]
};
__device__ __forceinline__ int gamd_box_of(const BoxRef& r, int i) {
    int q = (int)(((float)i + 0.5f) * r.inv_npb);          // off by at most one for i < 2^23 (gamd_create's limit)
    const int rem = i - q * r.n_per_box;
    q += rem >= r.n_per_box ? 1 : (rem < 0 ? -1 : 0);
    return q;
}
struct BoxDims { float bx, by, bz, hx, hy, hz; };
__device__ __forceinline__ BoxDims gamd_box_dims(const BoxRef& r, const float (&box)[3], const float (&half)[3], int box_id) {
    if (r.n_boxes <= 1) return BoxDims{box[0], box[1], box[2], half[0], half[1], half[2]};
    const float4 b = r.boxes[3 * box_id], h = r.boxes[3 * box_id + 1];
    return BoxDims{b.x, b.y, b.z, h.x, h.y, h.z};
}

// ---- pair-distance histogram of a frame (k_report_rdf over the edge list, k_struct_pairs over all pairs): one binning, 32-bit
// bins in LDS per workgroup, one 64-bit integer atomic per non-zero bin per workgroup (exact whatever the arrival order) -----
constexpr int GAMD_HIST_MAX_BINS = 1024;       // per pair class (rdf_bins of gamd_report_params / gamd_struct_params)
constexpr int GAMD_HIST_MAX_PAIRS = 3;         // O-O, O-H, H-H
// Count the pair (p, q) of a box with dimensions B: its distance to a bin, its species flags (.w, O != 0) to a pair class, and
// `inc` onto that LDS bin — or nothing when the pair lies outside r_max.  accept_all: the caller's pair list IS the set
// r < r_max (no second test against a rounded sqrt).  (The add is in here: a slot handed back into the kernel's loop costs an
// exec-mask close and reopen in front of it.)
__device__ __forceinline__ void gamd_hist_add(unsigned* bins, float4 p, float4 q, const BoxDims& B, float r_max, float bin_scale,
                                              int n_bins, int n_pairs, int accept_all, unsigned inc) {
    float r;
    {
#pragma clang fp contract(off)
        const float rx = gamd_min_image_wrapped(p.x - q.x, B.bx, B.hx);
        const float ry = gamd_min_image_wrapped(p.y - q.y, B.by, B.hy);
        const float rz = gamd_min_image_wrapped(p.z - q.z, B.bz, B.hz);
        r = sqrtf((rx * rx + ry * ry) + rz * rz);
    }
    if (!(accept_all || r < r_max)) return;
    int bin = (int)(r * bin_scale / r_max);
    bin = bin < n_bins - 1 ? bin : n_bins - 1;
    bin = bin < 0 ? 0 : bin;
    int pair = 0;
    if (n_pairs == 3) {
        const bool po = p.w != 0.f, qo = q.w != 0.f;
        pair = (po && qo) ? 0 : ((po || qo) ? 1 : 2);
    }
    atomicAdd(&bins[pair * n_bins + bin], inc);
}
__device__ __forceinline__ void gamd_hist_zero(unsigned* bins, int n_slots) { for (int k = threadIdx.x; k < n_slots; k += blockDim.x) bins[k] = 0u; }
__device__ __forceinline__ void gamd_hist_flush(const unsigned* bins, unsigned long long* out, int n_slots) {
    for (int k = threadIdx.x; k < n_slots; k += blockDim.x) {
        const unsigned c = bins[k];
        if (c) atomicAdd(&out[k], (unsigned long long)c);
    }
}

// ---- neighbour build --------------------------------------------------------------------------
struct NbrArgs {
    int n;                 // atoms (all boxes together)
    BoxRef bx;             // n_boxes > 1: per-box dimensions and cell grids (nc[] below is then unused)
    int* box_shift;        // [n_boxes + 1] scratch of the row scan: padding in front of each box's first CSR row (see d_scan_deg)
    int flavour;           // 0: jax-md path (dr^2 < rc^2, self kept); 1: torch path (|dr| <= rc, no self)
    float box[3], half[3]; // box and 0.5*box in fp32 (nn_module.py:617-621)
    float rc, rc2;
    int nc[3], ncell;
    int ncell_cap;         // counters | cell_cnt[ncell_cap] | cell_fill[ncell_cap] are one allocation
    long long e_cap;       // edge capacity of col/erow/e_frag
    const float* pos;      // [n][3] caller positions (any image)
    const uint8_t* species;// [n] or null
    const float* feat;     // [n] float node feature (nn_module.py:554 node_encoder input) or null: then (float)species
    int self_loop;         // 1: append one self edge per atom at the end of its row (gamd_config.self_loop_mode)
    int* devflags;         // [DEVFLAG_COUNT]
    float4* pos_w;         // [n] wrapped, original order
    float4* pos_s;         // [n + 1] wrapped, sorted order; .w = species; row n stays zero (source of padding edges)
    int* cell_of;          // [n]
    int* cell_cnt;         // [ncell]
    int* cell_fill;        // [ncell]
    int* cell_start;       // [ncell+1]
    int* perm;             // [n + 1] sorted -> original; perm[n] = -2 (the zero row that padding edges point at)
    int* inv_perm;         // [n] original -> sorted
    int* deg;              // [n]
    int* row_ptr;          // [n+1]
    int* na_excl;          // [n+1]
    int* col;              // [e_cap] source (neighbour) atom, sorted index
    int* erow;             // [e_cap] destination (centre) atom, sorted index
    int* chunk_piece;      // [(e_cap+32)/16]
    unsigned* chunk_mask;  // [(e_cap+32)/16]
    int* counters;         // [CNT_COUNT]
    int* counters_next;    // skin path: the OTHER counter block of the ping-pong pair, cleared by k_skin_check / k_step_small
                           // for the next call (no per-call memset node in the stream); null otherwise
    int* sticky;           // [STICKY_COUNT] host-mapped
    // Verlet-skin reuse (graph_utils.py:21-25,36-44: build with cutoff + dr_threshold, rebuild when an atom has moved
    // dr_threshold / 2): candidate CSR built with rc + skin on the steps that need it, exact filter every step
    const int* gate;       // non-null: the kernel returns unless *gate != 0 (rebuild kernels of the skin mode)
    float skin_half2;      // (skin / 2)^2
    int force_rebuild;     // first call, box change, regrown buffers
    float4* ref_pos;       // [n] wrapped positions at the last candidate build (original order)
    int* cand_deg;         // [n]
    int* cand_ptr;         // [n+1]
    int* cand_col;         // [cand_cap] sorted index of the candidate neighbour
    long long cand_cap;
    int cand_stride;       // > 0 (n > 1024): candidate row c is cand_col[c * cand_stride ..][cand_deg[c]] — fixed-width rows as in
                           // jax-md's idx[N, max_occupancy] (graph_utils.py:21-25): one kernel fills them, no count / scan / fill
                           // passes.  0 (n <= 1024, k_step_small): CSR rows cand_col[cand_ptr[c] ..][cand_deg[c]]
    int use_small;         // the host's choice (gamd_api.hip: use_small, n <= 1024): k_step_small + k_filter_fill_small, CSR
                           // candidate rows.  Explicit, not inferred from cand_stride == 0 (an undersized candidate buffer must
                           // surface as an overflow on the grid-wide path, never send n > 1024 atoms into the one-workgroup kernel)
    int cells_one_wg;      // candidate rebuild: the four cell-list phases in one single-workgroup launch (rebuilds are rare: one
                           // gated launch per reuse step instead of four) or as four grid-wide kernels (rebuilds are frequent)
    float rc_build, rc2_build;   // rc + skin + the fp32 rounding margin (gamd_api.hip GAMD_SKIN_MARGIN_EPS)
};
struct MdArgs;
// Integrator work that the small-system skin path (n <= 1024, NbrArgs::counters_next set) folds into its first kernel:
// the second half (B) of the previous step and / or the first half (B A O A) of this one (plain BAOAB, no constraints).
struct MdFuse { const MdArgs* md; int do_second, do_first; };
int launch_neighbor_build(const NbrArgs& a, hipStream_t st);
// skin mode: check, gated candidate rebuild, exact filter.  fuse != null (small-system path only): see MdFuse
int launch_neighbor_skin(const NbrArgs& a, hipStream_t st, const MdFuse* fuse = nullptr);
// CSR from a caller-supplied directed edge list (centre[e], neigh[e]); atoms keep the caller's order.
// tmp_eid: [n_edges] scratch.  Rows keep the caller's edge order (deterministic).
int launch_csr_from_edges(const NbrArgs& a, const int* centre, const int* neigh, long long n_edges, int* tmp_eid,
                          hipStream_t st);

// ---- edge encoder -----------------------------------------------------------------------------
struct EncArgs {
    const int* counters;
    const int* devflags;       // DEVFLAG_FROZEN set: return at once (see ConvEdgeArgs)
    const float4* pos_s;
    const int* col;
    const int* erow;
    const int* bond_nbr;       // [n][4] original-index bonded partners (-1 pad) or null
    const int* perm;           // sorted -> original (bond lookup)
    const int* row_ptr;        // CSR rows (self_loop: the last edge of a row is the appended zero-feature loop)
    int self_loop;             // gamd_config.self_loop_mode
    int zero_row;              // = n (all boxes): the source index of the padding slots behind a box's last row
    float box[3], half[3];
    BoxRef bx;                 // n_boxes > 1: the box of an edge is the box of its destination atom
    float length_mean, length_std, gamma;
    // edge_layer_norm over the TRUE edge-embedding width: widths below the 128-blocks the kernels work in are zero-padded by
    // gamd_finalize_weights (padded outputs are exact zeros); 1 / width and the number of padded features
    float ln_inv_width, ln_n_pad;
    int n_feat;                // 44 or 45
    int n_ksteps;              // ceil(n_feat/2)
    const float* centers;      // [40]
    RbfGrid rbf;               // uniform centres: recurrence along the grid instead of one exponential per centre
    const float* w1p;          // packed [4][6][64][4]  (K padded to 48)
    const float* w2p;          // packed 128x128
    const float* w3p;          // packed 128x128
    const float* b1; const float* b2; const float* b3;   // [128]
    const float* ln_g; const float* ln_b;                // [128]
    float* e_frag;             // [tiles][4][4][64][4]
    long long e_cap;
    float* feat_dbg;           // optional [e_cap][48] raw features (debug/parity), or null
    int* sticky;               // host-mapped flags (checked build: GAMD_CHK_RANGE reports here)
    int e_format;              // generic-width encoder (wide.hip): 0 = fp32 fragments, 1 = bf16 fragments (wide_lp.hip), 2 = (hi, lo)
                               // fp16 operand images for the split-fp16 conv kernels (the layout edge_encode_f16x3.hip writes)
    float* rstd_out;           // folded edge LayerNorm (launch_edge_encode / _small, gamd_ln_fold_host.h): [tiles][64] in lane order,
                               // lanes 0-31 the edge's rstd, lanes 32-63 zero; e_frag then holds rstd x2, w3p the ten non-zero
                               // blocks of R, b3 = Q^T c, ln_g / ln_b are not read.  Null: e = LayerNorm(W3 x2 + b3)
};
// self_loop_mode 1: is CSR slot x (source src, destination dst) the loop that was appended behind the row's real edges?  It is the
// last slot of its row that is not a padding slot (padding follows only in the row of a box's last atom, n_boxes > 1).
__device__ __forceinline__ bool gamd_is_appended_loop(const EncArgs& a, long long x, int src, int dst) {
    if (!a.self_loop || src == a.zero_row) return false;
    const long long row_end = a.row_ptr[dst + 1];
    return x == row_end - 1 || (x + 1 < row_end && a.col[x + 1] == a.zero_row);
}

// dimensions of the box an edge lives in (the box of its destination atom, sorted index)
__device__ __forceinline__ BoxDims gamd_edge_box(const EncArgs& a, int dst) {
    return gamd_box_dims(a.bx, a.box, a.half, a.bx.n_boxes > 1 ? gamd_box_of(a.bx, dst) : 0);
}
int launch_edge_encode(const EncArgs& a, int n_blocks, hipStream_t st);
// small edge counts: one tile per 4-wave workgroup, weights straight from L2, bit-identical to launch_edge_encode
int launch_edge_encode_small(const EncArgs& a, int n_blocks, hipStream_t st);
int launch_edge_encode_bf16(const EncArgs& a, int n_blocks, hipStream_t st);   // w*p = bf16 packed fragments, e_frag bf16
int launch_edge_encode_f16x3(const EncArgs& a, int n_blocks, hipStream_t st);  // w*p = [hi | lo] fp16 fragments, e_frag pre-split
// generic widths (wide.hip): n_feat in {4, 5, 44, 45}; w3p = eht packed blocks W3[128 ob : 128 ob + 128, :],
// b3 / ln_g / ln_b are [128 eht]; e_frag is [tiles][eht][4][4][64][4]
int launch_edge_encode_wide(const EncArgs& a, int eht, int n_blocks, hipStream_t st);
// hidden_dim above 128 (wide_d.hip, fp32): D = 128 dt, dt = 2.  w1p points at 1 + dt^2 + eht dt contiguous 64 KiB blocks
// [W1: dt images of 24 KiB] | W2[ob][kb] | W3[ob][kb]; b1, b2 are [128 dt]
int launch_edge_encode_wide_d(const EncArgs& a, int eht, int dt, int n_blocks, hipStream_t st);

// ---- conv layer, edge side --------------------------------------------------------------------
struct ConvEdgeArgs {
    const int* counters;
    const int* devflags;       // DEVFLAG_FROZEN set (a neighbour buffer overflowed earlier in this enqueued run): return at once —
                               // the steps enqueued behind a frozen one cost their launches, not their GEMMs
    const int* col;
    const int* erow;
    const int* chunk_piece;
    const unsigned* chunk_mask;
    const float* e_frag;
    const float* hn;           // [n][128] LayerNorm'd node features
    const float* S;            // [n][128] src_affine(hn) + b_src + b_dst + b_edge_affine2
    const float* D;            // [n][128] dst_affine(hn) (no bias)
                               // (bf16 edge MLP: the three tables are fp16 rows of 256 B, NodeArgs::tab16, S and D pre-multiplied
                               //  by log2 e)
    const float* w1p; const float* w2p; const float* w3p; const float* w4p;   // packed 128x128
    const float* w16p;         // generic-width fp32 path: the same EHT + 2 + HT blocks packed for the 16-edge kernel (wide16.hip), or null
    const float* b1; const float* b3; const float* b4;                           // [128]
    float* partial;            // [pieces][128]
    long long e_cap;
    int zero_row;              // = n: hn / S / D have one extra all-zero row for the padding slots of the last tile
    long long* tdbg;           // profiling builds only: [blocks][8 waves][16] cycle sums, or null
    int* sticky;               // host-mapped flags (checked build: GAMD_CHK_RANGE reports here)
    long long piece_cap;       // rows of `partial` (checked build: every piece index is tested against it)
    float* emb_out;            // update_edge_emb (generic-width kernels only): e_emb = theta_edge(...) of every edge, [E][H] rows
                               // in CSR order, for launch_edge_update; null otherwise
    const float* e_rstd;       // folded edge LayerNorm (launch_conv_edge, _l0, _small, _small_l0): EncArgs::rstd_out; e_frag then
                               // holds rstd x2, w1p is A_l followed by the extra K step's fragment (a_l, 0) (lnf_pack_a), b1 = b1'_l.
                               // Null: the general form
};
int launch_conv_edge(const ConvEdgeArgs& a, int n_blocks, hipStream_t st);
// layer-0 form (LJ models, conv_edge.hip): three GEMMs per edge, pieces hold sums of SiLU(W3 T2 + b3) over the real edges;
// S0 / D0 = row 0 of a.S / a.D, a.w3p / a.b3 packed in the F2 output order; hn, erow, w4p, b4 unused
int launch_conv_edge_l0(const ConvEdgeArgs& a, int n_blocks, hipStream_t st);
int launch_conv_edge_bf16(const ConvEdgeArgs& a, int n_blocks, hipStream_t st);   // w*p = bf16 packed fragments, e_frag bf16
// small edge counts (conv_edge_small.hip): one tile per 4-wave workgroup, bit-identical to launch_conv_edge
int launch_conv_edge_small(const ConvEdgeArgs& a, int n_blocks, hipStream_t st);
int launch_conv_edge_small_l0(const ConvEdgeArgs& a, int n_blocks, hipStream_t st);    // bit-identical to launch_conv_edge_l0
int launch_conv_edge_small_wide(const ConvEdgeArgs& a, int eht, int ht, int n_blocks, hipStream_t st);   // = launch_conv_edge_wide
int launch_conv_edge_f16x3(const ConvEdgeArgs& a, int n_blocks, hipStream_t st);  // w*p = [hi | lo] fp16 fragments (64 KiB)
// generic widths (wide.hip): Eh = 128 eht, H = 128 ht.  w1p points at eht + 2 + ht contiguous packed blocks
// W1[:, kb] | W2 | W3 | W4[ob, :]; b4 is [H]; hn and partial rows are H wide, S and D stay 128 wide
int launch_conv_edge_wide(const ConvEdgeArgs& a, int eht, int ht, int n_blocks, hipStream_t st);
// the same on 16-edge work units (wide16.hip: v_mfma_f32_16x16x4_f32, one wave per SIMD, a.w16p), bit-identical to
// launch_conv_edge_wide; for launches whose 32-edge tiles leave the SIMDs between 1 and 1.5 (2 and 2.5, ...) quanta of work
int launch_conv_edge_wide16(const ConvEdgeArgs& a, int eht, int ht, int n_blocks, hipStream_t st);
// hidden_dim above 128 (wide_d.hip, fp32): w1p points at eht + dt + dt^2 + ht dt contiguous blocks
// W1[:, kb] | W2[db, :] | W3[ob][db] | W4[ob][db]; b3 is [128 dt]; S and D rows are 128 dt wide
int launch_conv_edge_wide_d(const ConvEdgeArgs& a, int eht, int ht, int dt, int n_blocks, hipStream_t st);
// the same on the fp16 matrix pipe by operand splitting (wide_lp.hip): w1p = eht + 2 + ht contiguous [hi | lo] fp16 images,
// e_frag in the encoder's e_format 2, hn rows in their natural [n][H] layout
int launch_conv_edge_f16x3_wide(const ConvEdgeArgs& a, int eht, int ht, int n_blocks, hipStream_t st);
// bf16 operands (wide_lp.hip): w1p = eht + 2 + ht contiguous 32 KiB bf16 images, e_frag in the encoder's e_format 1
int launch_conv_edge_bf16_wide(const ConvEdgeArgs& a, int eht, int ht, int n_blocks, hipStream_t st);

// update_edge_emb=True (SmoothConvLayerNew, nn_module.py:91-92, :140-146): the edge embedding the NEXT layers read is
// edge_layer_norm(e_emb) of this layer.  emb: [E][128 ht] rows written by the conv kernel (emb_out); e_frag_out: the same
// fragment-order tiles the edge encoder writes (Eh == H).
struct EdgeUpdateArgs {
    const int* counters;
    const int* devflags;
    long long e_cap;
    const float* emb;
    const float* ln_g; const float* ln_b;      // [128 ht], zero-padded
    float ln_inv_width, ln_n_pad;              // LayerNorm over the true width
    float* e_frag_out;
};
int launch_edge_update(const EdgeUpdateArgs& a, int ht, int n_blocks, hipStream_t st);

// ---- node side --------------------------------------------------------------------------------
struct NodeLayerW {            // one conv layer's node-side parameters (device pointers)
    const float* ln_g; const float* ln_b;
    const float* wsp; const float* wdp; const float* wpdp;   // packed src_affine, dst_affine, phi_dst
    const float* bS;           // b_src + b_dst + b_edge_affine.2
    const float* bP;           // b_phi_dst + b_phi_edge
    const float* wpep;         // packed phi_edge (layer-0 form, post(0) only: M0 = W_pe diag(hn0) W4, see conv_edge.hip)
    const float* c0;           // layer-0 form, post(0) only: W_pe (hn0 * b4), added d_i times (d_i = real incoming edges); else null
    const float* wphip;        // packed phi.mlp_layer.1
    const float* bphi;
};
struct NodeArgs {
    const int* counters;       // CNT_OVERFLOW set: the CSR is truncated and piece indices are meaningless -> do nothing
                               // (the host regrows the buffers and re-issues the call)
    const int* devflags;       // DEVFLAG_FROZEN set: same
    int* sticky;               // host-mapped; STICKY_NONFINITE is raised by the decoder
    int n;
    int mode;                  // 0: first (embed + pre(0)); 1: post(l-1) + pre(l); 2: post(L-1) + decoder
    int l0_gate;               // mode 0 inside an enqueued MD run: return at once unless this step rebuilt the candidate list
                               // (counters[CNT_REBUILD]) — layer 0's tables depend on species + weights only and are still valid
    // inputs
    const float4* pos_s;       // .w = species feature
    const float* node_emb;     // [128] (lj) or null
    const float* enc_w; const float* enc_b;   // node_encoder Linear(1->128): weight[:,0], bias (water)
    const int* row_ptr; const int* na_excl; const int* deg;
    const int* col;            // post.c0 set and several boxes: the CSR sources, to count each row's box padding (source n)
    const float* partial;
    long long piece_cap;       // rows of `partial` (checked build)
    const float* h_in;         // [n][128] residual stream before this layer's conv (mode 1,2)
    const float* P_in;         // [n][128] phi_dst(hn)+biases from pre()
    NodeLayerW post;           // layer being finished (mode 1,2)
    NodeLayerW pre;            // layer being prepared (mode 0,1)
    // decoder (mode 2)
    const float* dec_w1p; const float* dec_b1; const float* dec_w2; const float* dec_b2;   // w2: [3][128] plain
    float scale, shift;        // sqrt(var), mean of the force scaler (fp32 copy for the device path)
    float ln_inv_width, ln_n_pad;   // graph_conv.norm_layers over the TRUE node width (zero-padded to the 128-blocks): 1 / width, #pad
    int norm_bn;                    // 1: norm_layers are eval-mode BatchNorm1d (use_layer_norm=False), folded into ln_g / ln_b
    int f16x3;                      // 1 (node.hip, reduced-precision edge modes): node-side matrices are (hi | lo) fp16 images, GEMMs in split-fp16
    const int* perm;
    // outputs
    float* h_out;              // [n][128]
    float* hn_out; float* S_out; float* D_out; float* P_out;
    int hn_perm;               // 1: hn rows are stored feature-permuted, position (f & 31) * 4 + (f >> 5), so that the
                               // conv kernel's row-layout gather is one 16-byte load per edge (conv_edge_f16x3.hip)
    int tab16;                 // 1 (bf16 edge MLP, conv_edge_bf16.hip): hn, S, D are written as fp16 rows of 256 B instead of fp32
                               // rows — hn in natural feature order, S and D in the order gamd_tab16_pos() gives (the 64 features a
                               // lane of the chain layout owns come as 8 x 16 B, lanes slot and slot + 32 side by side)
    float* forces_norm;        // [n][3] normalised network output, ORIGINAL atom order (mode 2)
    float* forces;             // [n][3] denormalised fp32 (device MD loop), original order, or null
    long long* tdbg;           // profiling builds only (GAMD_NODE_TIME=1): [workgroup][wave][16] s_memtime marks of the mode-1 launches
};
int launch_node(const NodeArgs& a, hipStream_t st);
// generic widths (wide.hip): h / hn / partial rows and node_emb, enc_w, enc_b, ln_*, bphi are H = 128 ht wide;
// wsp, wdp, wpdp, wpep, dec_w1p are ht K-blocks, wphip is ht output blocks; S, D, P stay 128 wide
int launch_node_wide(const NodeArgs& a, int ht, hipStream_t st);
// hidden_dim above 128 (wide_d.hip, fp32): S, D, P rows, bS, bP, dec_b1 are 128 dt wide, dec_w2 is [3][128 dt]; wsp, wdp, wpdp, wpep,
// dec_w1p are dt x ht blocks (output block major), wphip is ht x dt
int launch_node_wide_d(const NodeArgs& a, int ht, int dt, hipStream_t st);

// ---- integrator -------------------------------------------------------------------------------
// rigid 3-site water (atoms O,H,H): masses and the SETTLE canonical triangle (Miyamoto & Kollman 1992):
// rc = d_HH/2, ra = distance O - centre of mass, rb = distance centre of mass - HH midpoint
struct RigidWater { float m_o, m_h, ra, rb, rc; };
// OpenMM's CMMotionRemover, which the first-half integrators run through addUpdateContextState() at the top of every step
// (hack_integrator.py:142, :272) when the System carries one (the water drivers' openmmtools WaterBox does; :226-235 takes 3
// degrees of freedom off for it): v_i -= sum_j m_j v_j / sum_j m_j, per box.  k_com_partial leaves per-block sums
// (sum m vx, sum m vy, sum m vz, sum m) in `partial`; every first-half thread adds up the `blocks` rows of its box in order.
struct MdCom {
    int enabled;
    int blocks;                // partial rows per box
    double* partial;           // [n_boxes][blocks][4]
};
struct MdArgs {
    int n;
    float* x; float* v;        // [n][3] length unit L (Angstrom | bohr), L/ps
    const float* f;            // [n][3] kJ/mol/nm
    const uint8_t* species;    // [n] or null: species-0 atoms use inv_mass_h when it is > 0
    float inv_mass, inv_mass_h;// 1/amu
    float len;                 // L per nm (10 for Angstrom)
    float dt;                  // ps
    float a, b_len_kT;         // exp(-gamma dt), sqrt(1-a^2)*len*sqrt(kT): O-step sigma = b_len_kT*sqrt(1/m)
    float box[3];
    BoxRef bx;                 // n_boxes > 1: per-box dimensions; box b draws its noise as a single box with seed + b would
    int use_rigid;             // 1: O,H,H triples are rigid (one thread per molecule)
    RigidWater rigid;
    unsigned long long seed; unsigned long long step;
    int* devflags;             // [DEVFLAG_COUNT]: frozen -> return, first kernel to see it records 2 * step_index + half
    int step_index;            // index of this step inside the gamd_md_run call
    MdCom com;                 // centre-of-mass motion removal at the start of the first half (hack_integrator.py:142)
};
int launch_baoab_first(const MdArgs& a, hipStream_t st);    // B A O A  (hack_integrator.py:141-165)
int launch_baoab_second(const MdArgs& a, hipStream_t st);   // B        (hack_integrator.py:175-178)
// B of the step a.step_index AND the per-block momentum sums (a.com) the NEXT step's CMMotionRemover needs, in one launch
int launch_baoab_second_com(const MdArgs& a, hipStream_t st);

// Nose-Hoover chain of the reference drivers (hack_integrator.py:182-330 first half, :334-493 second half;
// one chain state shared by both halves, as copy_state_from_integrator does every step)
struct NhcArgs {
    int n;
    float* x; float* v;        // [n][3] Angstrom, Angstrom/ps
    const float* f;            // [n][3] kJ/mol/nm
    const uint8_t* species;    // [n] or null
    float mass, mass_h;        // amu; species-0 atoms use mass_h when it is > 0
    float len;                 // length units per nm
    float dt;                  // ps
    float box[3];
    BoxRef bx;                 // n_boxes > 1: one chain per box (state / partial are per box), ndf is per box
    int use_rigid;
    RigidWater rigid;
    double kT, freq, ndf;      // kJ/mol, 1/ps, degrees of freedom
    int M, n_c, n_ys;          // chain length, multi-time-step count, Yoshida-Suzuki order
    double w[5];
    double* state;             // [n_boxes][3*M + 2]: xi[M], vxi[M], G[M], scale, KE2
    double* partial;           // [n_boxes][n_blocks] per-block sums of m v^2
    int n_blocks;              // blocks per box
    int* devflags;             // as in MdArgs
    int step_index;
    MdCom com;                 // as in MdArgs; in the first half the remover runs behind propagateNHC (hack_integrator.py:271-272):
                               // KE2 and the chain see the velocities as they are, the scaled velocities lose their COM part
};
// per-block momentum sums of the current velocities (first kernel of a step whose integrator removes the COM motion)
int launch_com_partial(const MdCom& com, const float* v, const uint8_t* species, float inv_mass, float inv_mass_h, int n,
                       const BoxRef& bx, const int* devflags, int by_molecule, hipStream_t st);
int launch_nhc_first(const NhcArgs& a, hipStream_t st);     // propagateNHC; v *= scale; v += dt/2 f/m; x += dt v
int launch_nhc_second(const NhcArgs& a, hipStream_t st);    // v += dt/2 f/m; propagateNHC; v *= scale

// ---- run reporter (report.hip) ------------------------------------------------------------------
// One sample of an enqueued MD run (gamd_report_configure): the kinetic-energy log row `slot` and / or the pair-distance
// histogram of the frame.  Slot and step number come from the host (the sample's ordinal), so a sample that is enqueued
// again after a freeze writes the same row; the histogram is protected by the freeze gate alone (a kernel that returned
// added nothing).
enum { GAMD_CHK_REPORT_SRC = 141, GAMD_CHK_REPORT_DST = 142, GAMD_CHK_REPORT_PERM = 143, GAMD_CHK_REPORT_ROW = 144 };
struct ReportArgs {
    int n;                     // atoms of all boxes
    BoxRef bx;
    const int* devflags;       // DEVFLAG_FROZEN set: every reporter kernel returns at once
    int* sticky;               // host-mapped (checked build)
    // kinetic energy
    const float* v;            // [n][3] length unit / ps
    const uint8_t* species;    // [n] or null
    double mass, mass_h;       // amu; species-0 atoms use mass_h when it is > 0
    double len;                // length units per nm
    double* partial;           // [n_boxes][blocks] per-block sums of m v^2
    int blocks;                // blocks per box
    long long* steps;          // [max_samples]
    double* ke;                // [max_samples][n_boxes]
    long long slot;            // log row of this sample, -1: the log is full (no kinetic-energy launch)
    long long g;               // completed MD steps at this sample
    // g(r)
    const int* counters;
    const float4* pos_s;
    const int* col; const int* erow; const int* row_ptr; const int* perm;
    long long e_cap;
    float box[3], half[3];
    int n_bins, n_pairs;       // n_bins == 0: no histogram
    float r_max, bin_scale;    // bin_scale = n_bins (as float): bin = (int)(r * bin_scale / r_max)
    int all_edges;             // r_max == cutoff: the edge list IS the set r < r_max (no second test against a rounded sqrt)
    int exclude_same_molecule;
    unsigned long long* counts;// [n_boxes][n_pairs][n_bins]
    int rdf_blocks;            // workgroups per box
};
int launch_report_ke(const ReportArgs& a, hipStream_t st);
int launch_report_rdf(const ReportArgs& a, hipStream_t st);

// ---- run recorder (traj.hip) --------------------------------------------------------------------
// One sample of an enqueued MD run (gamd_traj_configure): trajectory frame q, the periodic-image counters, and the
// MSD / VACF sums over the ring of the last n_lags samples.  Sample ordinal, frame slot and ring slot come from the host;
// the image counters, x_prev, the ring and the running sums are updated in place and rely on the freeze gate alone (a
// kernel that returned changed nothing, and a sample runs exactly once unfrozen).
// (No recorder kernel uses a value it read from memory as an address: the checked build has nothing to range-check here.)
struct TrajArgs {
    int n;                     // atoms of all boxes
    BoxRef bx;
    float box[3];              // n_boxes <= 1
    const int* devflags;       // DEVFLAG_FROZEN set: every recorder kernel returns at once
    const float* x; const float* v; const float* f;    // [n][3] the caller's buffers
    const uint8_t* species;    // [n] or null
    double mass, mass_h;       // amu; species-0 atoms use mass_h when it is > 0 (the COM of subtract_com)
    long long q;               // sample ordinal (g / interval - 1)
    long long g;               // completed MD steps at this sample
    // frames
    long long frame;           // q when q < max_frames, else -1
    long long* steps;          // [max_frames]
    float* fx; float* fv; float* ff; int* fimg;        // [max_frames][n][3] or null (field not recorded)
    // image bookkeeping
    float* x_prev;             // [n][3] positions at the previous sample
    int* image;                // [n][3]
    unsigned long long* ambiguous;
    // correlation functions
    int n_lags;                // 0: none
    int slot;                  // q % n_lags
    int active;                // min(q, n_lags - 1) + 1 lags have an origin in the ring
    int classes;               // 1, or 2 (O, H)
    int subtract_com;
    float* ring_x; int* ring_img; float* ring_v;       // [n_lags][n][3]
    double* ring_com;          // [n_lags][n_boxes][3] mass-weighted mean of the unwrapped positions
    double* com_partial;       // [n_boxes][com_blocks][4]
    int com_blocks;
    double* corr_partial;      // [n_boxes][n_lags][corr_blocks][classes][2]
    int corr_blocks;           // workgroups per box and lag (fixed per handle)
    double* msd; double* vacf; // [n_boxes][classes][n_lags] running sums
    long long* class_atoms;    // [n_boxes][classes]
};
int launch_traj_sample(const TrajArgs& a, hipStream_t st);     // frame, images, ring; with n_lags > 0 also COM and the sums

// ---- structure sampler (structure.hip) ------------------------------------------------------------
// One sample of an enqueued MD run (gamd_struct_configure): the all-pairs distance histogram of the frame out to r_max
// (any r_max up to half the shortest box edge: the edge list of the force evaluation cannot serve beyond the cutoff) and / or
// the partial structure-factor sums over the handle's k-vector list.  The integer counts commute; the S(k) sums are updated
// in place and rely on the freeze gate alone (a kernel that returned changed nothing, and a sample runs exactly once unfrozen).
enum { GAMD_CHK_STRUCT_PERM_I = 145, GAMD_CHK_STRUCT_PERM_J = 146 };
struct StructArgs {
    int n;                     // atoms of all boxes
    BoxRef bx;
    const int* devflags;       // DEVFLAG_FROZEN set: every sampler kernel returns at once
    int* sticky;               // host-mapped (checked build)
    float box[3], half[3];     // n_boxes <= 1
    // pair histogram: the wrapped positions of the force evaluation that has just run, sorted order (box-contiguous)
    const float4* pos_s;       // .w = species flag
    const int* perm;           // sorted -> caller order (exclude_same_molecule)
    int n_bins, n_pairs;       // n_bins == 0: no histogram
    float r_max, bin_scale;    // bin = (int)(r * bin_scale / r_max), bin_scale = n_bins as float
    int exclude_same_molecule;
    int tiles;                 // 256-atom tiles per box
    unsigned long long* counts;// [n_boxes][n_pairs][n_bins]
    // structure factors: the caller's positions in the caller's order (the sorted order is not the same run after run)
    const float* x;            // [n][3]
    const uint8_t* species;    // [n], classes == 2 only
    int n_k;                   // k-vectors, 0: none
    const int* kvec;           // [n_k][3] integer triples n
    int classes;               // 1, or 2 (O, H)
    int rho_blocks;            // workgroups per box and 64 k-vectors (fixed per handle: the summation tree never changes)
    double* rho_partial;       // [n_boxes][rho_blocks][classes][n_k][2] (re, im)
    double* sk_sum;            // [n_boxes][n_pairs][n_k] running sums of Re(rho_a conj(rho_b))
};
int launch_struct_pairs(const StructArgs& a, hipStream_t st);
int launch_struct_sk(const StructArgs& a, hipStream_t st);

// ---- the cell table under the classical potentials' pair passes (cell_table.hip) ---------------------------------------
// Per box a table of the atoms ordered by (cell, atom index), rebuilt at the head of every evaluation from the positions as they
// are given (gamd_cells_dev.h: the cells of a box, the cell of a coordinate).  One builder, five
// launches on `st`: clear, count, scan, fill, rank; the walks over the table are the potentials' own (water_cells.hip,
// classical_cells.hip).  Every kernel returns while DEVFLAG_FROZEN is set and for a box with stopped[box] != 0.
// Every value read from memory and then used as an address — an atom's cell, a cell's start, a slot — passes through
// GAMD_CHK_RANGE under the caller's codes chk, chk + 1, chk + 2 (a table entry's atom index: the walks', chk + 3).
struct CellTabAtom { double x, y, z; int idx, o; };   // a table entry: the position as the walk reads it, the atom inside its box, O != 0
struct CellTabBufs {
    double r_cut;              // the cutoff the cells per axis are computed from (gamd_cells_per_axis), length unit
    int cap;                   // cells per box the tables below have room for
    int* sticky;               // host-mapped (checked build)
    int* start;                // [n_boxes][cap + 1] the counts per cell, then (scan) the first slot of every cell and n_per_box behind the last
    int* fill;                 // [n_boxes][cap] members placed so far (cleared with the counts at the head of every sample)
    int* cell_of;              // [n] the atom's cell inside its box
    int* members;              // [n] per box and cell the atoms of the cell, in the order the atomics gave
    int* order;                // [n] per box the atoms in table order: by (cell, atom index)
    CellTabAtom* table;        // [n] the table-ordered copy
};
struct CellTabArgs {
    int n;                     // atoms of all boxes
    BoxRef bx;
    float box[3];              // n_boxes <= 1 and box_edges == null
    const float* box_edges;    // device [n_boxes][3], or null: box / bx.boxes of the run
    const int* devflags;
    const int* stopped;        // [n_boxes] a minimiser's gates, or null: no per-box gate
    const float* x;            // [n][3] positions, length unit, any periodic image
    const double* x64;         // [n][3] a minimiser's positions or the M-site pass's charge sites, or null: x widened
    const uint8_t* species;    // [n] O != 0, or null: every entry's O flag is 0
    int chk;                   // the caller's first range-check code
    CellTabBufs c;
};
// the builder's block from a potential's (ClassicalArgs, WaterArgs: its atoms, boxes, flags and fp32 positions)
template <typename Args>
inline CellTabArgs cell_tab_args(const Args& a, const CellTabBufs& c, const int* stopped, const double* x64, const uint8_t* species, int chk) {
    return CellTabArgs{a.n, a.bx, {a.box[0], a.box[1], a.box[2]}, a.box_edges, a.devflags, stopped, a.x, x64, species, chk, c};
}
int launch_cell_table(const CellTabArgs& k, hipStream_t st);

// ---- classical potential (classical.hip) ----------------------------------------------------------
// One sample of an enqueued MD run (gamd_classical_configure) or one gamd_classical_eval call: the switched, shifted
// Lennard-Jones potential of include/gamd_hip.h on every pair of every box in double, from the caller's fp32 positions in the
// caller's atom order: per-atom forces f_cl, per-box energy, virial and pair count, and (f != null) the force-error sums of f
// against f_cl.  Row number and step number come from the host (the sample's ordinal), so a sample that is enqueued again after
// a freeze writes the same row with the same bits; nothing is updated in place.
// (No kernel uses a value it read from memory as an address: the checked build has nothing to range-check here.)
enum { CLASSICAL_PART = 6,     // per atom and slice: Fx, Fy, Fz (per length unit), e_i, w_i, pairs of the atom's row
       CLASSICAL_ROW = 9 };    // per box: E, W, pairs, sum |D_ic|, sum |D_i|^2, sum cos, sum |f_cl,i|, sum |f_i|, atoms left out of cos
struct ClassicalArgs {
    int n;                     // atoms of all boxes
    BoxRef bx;
    const int* devflags;       // DEVFLAG_FROZEN set: every kernel returns at once
    float box[3];              // n_boxes <= 1 and box_edges == null
    const float* box_edges;    // device [n_boxes][3] (gamd_classical_eval), or null: box / bx.boxes of the run
    const float* x;            // [n][3] positions, length unit, any periodic image
    const float* f;            // [n][3] kJ/mol/nm to compare f_cl with, or null
    double sig2, eps4, eps24;  // sigma^2, 4 epsilon, 24 epsilon
    double rc2, u0;            // r_cut^2, u_LJ(r_cut) or 0
    double rs, inv_w;          // r_switch and 1 / (r_cut - r_switch); rs < 0: no switching
    double len;                // length units per nm
    int tiles, slices, chunk;  // 256-atom row tiles per box; J slices per row; atoms per slice
    int blocks;                // workgroups per box of the per-atom pass (fixed per handle: the summation tree never changes)
    double* part;              // [n_boxes][slices][n_per_box][CLASSICAL_PART]
    double* f_cl;              // [n][3] kJ/mol/nm
    double* blk;               // [n_boxes][blocks][CLASSICAL_ROW]
    double* rows;              // [...][n_boxes][CLASSICAL_ROW]
    long long* steps;          // [...] or null
    long long slot;            // row of this sample
    long long g;               // completed MD steps at this sample
};
// `cells` (gamd_classical_cells; `a` arrives with slices = 1): launch_classical_cells stands where the pair launch is; null: all pairs
int launch_classical(const ClassicalArgs& a, hipStream_t st, const CellTabBufs* cells = nullptr);

// ---- classical force source (drive.hip) -------------------------------------------------------------
// One force evaluation of a classical-source step of an enqueued MD run (gamd_md_force_source): the pair pass of classical.hip
// (tiles, slices and arithmetic of k_classical_pairs; forces only) into a.part, then per atom the slice partials added in order
// from 0, f_cl = F * len to a.f_cl and (float)f_cl to f_out ([n][3], the caller's atom order).  a.f, a.blk, a.rows, a.steps,
// a.slot and a.g are not used.  Two launches, plain stores.
int launch_classical_drive(const ClassicalArgs& a, float* f_out, hipStream_t st, const CellTabBufs* cells = nullptr);

// ---- water classical potential (water_classical.hip) ------------------------------------------------
// One sample of an enqueued MD run (gamd_water_configure) or one gamd_water_eval call: 3-site water in the caller's order
// O,H,H (molecule = index / 3, O = species != 0, q_O = -2 q_H), O-O Lennard-Jones as in classical.hip plus a plain Ewald sum
// (real space with the same-molecule exclusion, reciprocal space over the handle's k-vector list, self term), all in double
// (DESIGN.md section 4.10).  Rows, steps and the resume rule are those of ClassicalArgs: plain stores only.
// (No kernel uses a value it read from memory as an address: the checked build has nothing to range-check here.)
enum { WATER_PART = 6,         // per atom and pair slice: Fx, Fy, Fz (per length unit), u_LJ, u_real + u_excl, pairs of the atom's row
       WATER_ACC = 11,         // per box and block: sum u_LJ, sum u_coul, sum pairs, the five sums, atoms left out, sum z, sum z^2
       WATER_ROW = 12 };       // per box: U_LJ, U_real + U_excl, U_recip, U_self, pairs, the five sums, atoms left out, sum q
struct WaterArgs {
    int n;                     // atoms of all boxes
    BoxRef bx;
    const int* devflags;       // DEVFLAG_FROZEN set: every kernel returns at once
    float box[3];              // n_boxes <= 1 and box_edges == null
    const float* box_edges;    // device [n_boxes][3] (gamd_water_eval), or null: box / bx.boxes of the run
    const float* x;            // [n][3] positions, length unit, any periodic image
    const float* f;            // [n][3] kJ/mol/nm to compare f_cl with, or null
    const uint8_t* species;    // [n] O != 0
    double q_h, q_o;           // e; q_o = -2 q_h
    double sig2, eps4;         // O-O Lennard-Jones: sigma^2, 4 epsilon (24 epsilon is 6 * eps4 on the device, the same double)
    double rc2, u0;            // r_cut^2, u_LJ(r_cut) or 0
    double rs, inv_w;          // r_switch and 1 / (r_cut - r_switch); rs < 0: no switching
    double coul;               // C = coulomb_const * len: kJ/mol * length unit / e^2
    double alpha, two_a_rpi;   // alpha and 2 alpha / sqrt(pi)
    double kc2, inv_4a2;       // k_cut^2 and 1 / (4 alpha^2)
    double two_pi;             // 2 pi
    double coul4pi, coul8pi;   // 4 pi C and 8 pi C
    double self_c;             // C alpha / sqrt(pi)
    double len;                // length units per nm
    int tiles, slices, chunk;  // 256-atom row tiles per box; J slices per row; atoms per slice
    int blocks;                // workgroups per box of the per-atom pass (fixed per handle: the summation tree never changes)
    int n_k, kslices, kchunk;  // k-vectors of the list; k slices per atom; k-vectors per slice
    int kblocks;               // (n_k + 255) / 256: workgroups per box of k_water_sk
    int rho_blocks;            // workgroups per box and 64 k-vectors of k_water_rho (fixed per handle)
    const int* kvec;           // [n_k][3] integer triples n
    double* part;              // [n_boxes][slices][n_per_box][WATER_PART]
    double* rho_partial;       // [n_boxes][rho_blocks][n_k][2] (re, im)
    double* sk;                // [n_boxes][n_k][3]: Re S, Im S, A
    double* ublk;              // [n_boxes][kblocks]: block sums of A |S|^2
    double* rpart;             // [n_boxes][kslices][n_per_box][3]: sum_k A (Re S sin + Im S cos) n per component
    double* f_cl;              // [n][3] kJ/mol/nm
    double* blk;               // [n_boxes][blocks][WATER_ACC]
    double* rows;              // [...][n_boxes][WATER_ROW]
    long long* steps;          // [...] or null
    long long slot;            // row of this sample
    long long g;               // completed MD steps at this sample
};
// `pme` (gamd_water_pme; its w is `a` with kslices = 1 and kblocks = pme_blocks): launch_water_pme stands where the three
// reciprocal launches are; null: the plain sum, launch for launch as it was
// `cells` (gamd_water_cells; `a` arrives with slices = 1): launch_water_cells stands where the pair launch is; null: all pairs
struct PmeArgs;
int launch_water_classical(const WaterArgs& a, hipStream_t st, const PmeArgs* pme = nullptr, const CellTabBufs* cells = nullptr);
// k_water_rho, k_water_sk, k_water_recip alone, with launch_water_classical's checks for them: a.rpart (and a.sk, a.ublk) from a.x
int launch_water_recip(const WaterArgs& a, hipStream_t st);
// k_water_sk alone (it reads no positions): a.sk and a.ublk from a.rho_partial, for the water minimiser's own rho and force passes
int launch_water_sk(const WaterArgs& a, hipStream_t st);
// k_water_final alone (it reads no positions): the row of a.slot from a.blk and a.ublk, for the 4-site passes of water_msite.hip
int launch_water_final(const WaterArgs& a, hipStream_t st);

// ---- what every launcher of the tiled passes checks (gamd_passes_dev.h) --------------------------------------------------
// The rows: `unit` atoms at least and a multiple of it per box (1, or 3 for molecules), the box count inside grid.y, T = the
// 256-atom row tiles as the handle counted them (pass_rows: all a launcher without a pair pass needs); for the pair pass the
// slices cover a row, and grid.x * 256 threads stay below 2^31.
struct PassGeom { int nb, npb; long long T; };
template <typename Args>
inline int pass_rows(const Args& a, int unit, PassGeom* g) {
    g->nb = a.bx.n_boxes > 1 ? a.bx.n_boxes : 1; g->npb = a.bx.n_boxes > 1 ? a.bx.n_per_box : a.n;
    g->T = (g->npb + 255) / 256;
    return g->npb < unit || g->npb % unit || g->nb > 65535 || a.tiles != (int)g->T ? -1 : 0;
}
template <typename Args>
inline int pass_geometry(const Args& a, int unit, PassGeom* g) {
    if (pass_rows(a, unit, g) || a.slices < 1 || a.chunk < 1) return -1;
    if ((long long)a.slices * a.chunk < g->npb || g->T * a.slices > 0x7fffffll) return -1;
    return 0;
}
// ... and the k side of the water passes; `chunked`: the k slices are contiguous kchunk-vector pieces that cover the list
inline int pass_k_geometry(const WaterArgs& a, long long T, bool chunked) {
    if (a.n_k < 1 || a.n_k > (1 << 17) || a.kslices < 1 || T * a.kslices > 0x7fffffll) return -1;
    if (chunked && (a.kchunk < 1 || (long long)a.kslices * a.kchunk < a.n_k)) return -1;
    if (a.kblocks != (a.n_k + 255) / 256 || a.rho_blocks < 1 || a.rho_blocks > 65535) return -1;
    return 0;
}

// ---- water classical force source (water_drive.hip) -------------------------------------------------
// One force evaluation of a water-source step of an enqueued MD run (gamd_md_force_source, GAMD_FORCE_WATER_CLASSICAL): the pair
// pass of water_classical.hip (tiles, slices and arithmetic of k_water_pairs; forces only) into a.part, launch_water_recip, then
// per atom the pair slices and the k slices added in order from 0, f_cl to a.f_cl and (float)f_cl to f_out ([n][3], the
// caller's atom order).  a.f, a.blk, a.rows, a.steps, a.slot and a.g are not used.  Five launches, plain stores.
int launch_water_drive(const WaterArgs& a, float* f_out, hipStream_t st, const PmeArgs* pme = nullptr, const CellTabBufs* cells = nullptr);

// ---- the TIP4P M-site in the water classical potential (water_msite.hip) ------------------------------
// The potential of WaterArgs with the negative charge on a virtual site M = O' + w_h (d_1 + d_2) of every molecule
// (gamd_water_msite): the charge sites are M, H1, H2, the Lennard-Jones site is O, and M's force goes
// back to the atoms with the weights 1 - 2 w_h, w_h, w_h.  `w` is the 3-site argument block unchanged (w.x the fp32 atoms);
// molecule = index / 3 with the oxygen first.  w_h != 0: the 3-site launchers serve w_h = 0.
// (No kernel uses a value it read from memory as an address: the checked build has nothing to range-check here.)
enum { W4_LJ = 4 };            // per molecule and pair slice: the oxygen's Lennard-Jones Fx, Fy, Fz (per length unit) and u_LJ of its row
struct W4Args {
    WaterArgs w;
    double w_h, w_o;           // the hydrogens' weight and 1 - 2 w_h
    int mchunk;                // molecules per slice of the Lennard-Jones pass: slices * mchunk >= n_per_box / 3
    double* sites;             // [n][3] charge-site positions, length unit: M in the oxygen's row, the hydrogen wrapped into [0, L) in its own
    double* ljpart;            // [n_boxes][slices][n_per_box / 3][W4_LJ]
};
// k_w4_sites, k_w4_pairs, k_w4_lj, k_w4_rho, k_water_sk, k_w4_recip, k_w4_atoms, k_water_final: launch_water_classical's row and f_cl
int launch_w4_classical(const W4Args& a, hipStream_t st, const PmeArgs* pme = nullptr, const CellTabBufs* cells = nullptr);
// ... the first six and k_w4_drive: launch_water_drive's f_cl and f_out (the energies of the pair pass are computed and not read)
int launch_w4_drive(const W4Args& a, float* f_out, hipStream_t st, const PmeArgs* pme = nullptr, const CellTabBufs* cells = nullptr);

// ---- smooth particle-mesh Ewald for the water classical potential (water_pme.hip) -----------------------
// A second producer of w.rpart and w.ublk (gamd_water_pme): instead of k_water_rho, k_water_sk and
// k_water_recip (or their site twins) the charges z (-2, +1) of the positions — w.x, or `sites` for the M-site form — are spread
// on a grid of nx x ny x nz points per box in 64-bit integers, transformed, multiplied by the influence function and
// transformed back, and the per-atom gradient sums are gathered into w.rpart with w.kslices = 1, scaled so that k_water_atoms,
// k_wsrc_atoms, k_w4_atoms and k_w4_drive form the force with the arithmetic they have; the block sums of the reciprocal
// energy go to w.ublk with w.kblocks = pme_blocks(nx, ny, nz), scaled so that k_water_final reads them unchanged.  Nothing of
// w.kvec, w.rho_partial, w.sk, w.n_k, w.kchunk is read.  Ten launches on `st`: clear, spread, three line passes, the
// convolution, three line passes, gather.
struct PmeArgs {
    WaterArgs w;
    const double* sites;       // [n][3] the charge sites k_w4_sites left, or null: the fp32 positions w.x
    int order;                 // 4 or 6
    int nx, ny, nz;            // each of 8, 16, 32, 64, 128
    unsigned long long* gq;    // [n_boxes][nx][ny][nz] the spread, quanta of 2^-50 q_H as two's complement (cleared every sample)
    double* gc;                // [n_boxes][nx][ny][nz][2] the transform, (re, im)
    const double* tw;          // [64][2] (cos, -sin)(2 pi j / 128)
    const double* mod;         // [nx + ny + nz] the interpolation moduli of the three axes
};
inline int pme_blocks(int nx, int ny, int nz) { const long long g = (long long)nx * ny * nz / 256; return (int)(g < 128 ? g : 128); }
int launch_water_pme(const PmeArgs& p, hipStream_t st);

// ---- the real-space pairs of the water classical potential over a cell table (water_cells.hip) ------------
// A second producer of the pair rows w.part (gamd_water_cells): instead of k_water_pairs, k_wsrc_pairs
// or k_w4_pairs the table of CellTabBufs is built from the positions — w.x, or `sites` for the M-site form — with the O flags of
// w.species (launch_cell_table), and every atom walks the atoms of its cell's neighbour cells, gamd_water_walk's body on the same
// doubles.  The rows go to w.part as ONE pair slice: `w` arrives with w.slices = 1 and w.chunk = n_per_box, and k_water_atoms,
// k_wsrc_atoms, k_w4_atoms and k_w4_drive run on it as they are.  Six launches on `st`: the table's five, pairs.
// The first three codes are the builder's chk, chk + 1, chk + 2; the walk checks what it reads under the same ones and _ATOM.
enum { GAMD_CHK_WCELL_CELL = 151, GAMD_CHK_WCELL_START = 152, GAMD_CHK_WCELL_SLOT = 153, GAMD_CHK_WCELL_ATOM = 154 };
// nout = WATER_PART (the observer, gamd_water_eval) or 3 (the force source); lj: the O-O term in the walk (3-site: w.x, or
// `sites` = a minimiser's double positions), else the M-site form on `sites`
int launch_water_cells(const WaterArgs& w, const CellTabBufs& c, const double* sites, int nout, bool lj, hipStream_t st);

// ---- the pairs of the Lennard-Jones classical potential over a cell table (classical_cells.hip) ------------
// A second producer of the pair rows a.part (gamd_classical_cells): instead of k_classical_pairs,
// k_drive_lj_pairs or k_min_pairs the table of CellTabBufs (no species: the entries' O flag is 0) is built from the positions —
// a.x, or `x64` for the minimiser — and every atom walks the table's runs around its cell, gamd_lj_walk's body on the same
// doubles.  The rows go to a.part as ONE pair slice: `a` arrives with a.slices = 1 and a.chunk = n_per_box, and k_classical_atoms,
// k_drive_lj_atoms and k_min_atoms run on it as they are.  Six launches on `st`: the table's five, pairs.  `stopped` (the
// minimiser's gates, or null): a box with stopped[box] != 0 is left alone.  The codes: as the water walk's, of their own.
enum { GAMD_CHK_LJCELL_CELL = 155, GAMD_CHK_LJCELL_START = 156, GAMD_CHK_LJCELL_SLOT = 157, GAMD_CHK_LJCELL_ATOM = 158 };
// nout = CLASSICAL_PART (the observer, gamd_classical_eval), 3 (the force source) or 4 ({F, e_i}: an iteration of the minimiser)
int launch_classical_cells(const ClassicalArgs& a, const CellTabBufs& c, const double* x64, const int* stopped, int nout, hipStream_t st);

// ---- molecular virial of the water classical potential (water_virial.hip) ------------------------------
// The virial log of gamd_water_virial: launched BEHIND launch_water_classical / launch_w4_classical
// of the same frame and argument block `w`, whose f_cl (the atoms' total classical forces) and sk ({Re S, Im S, A}) it reads;
// nothing of theirs is written.  w_h = 0: the 3-site walk on w.x; else the charge-site walk on `sites` and the O-O pass with
// mchunk molecules per slice.  v (may be null: KE_com = 0) are the frame's velocities, length unit / ps; masses in amu.
// (No kernel uses a value it read from memory as an address: the checked build has nothing to range-check here.)
enum { WATER_VIR_PART = 2,     // per atom and pair slice: sum -(r u_LJ'(r)), sum fs_coul r^2 of the atom's row
       WATER_VIR_ACC = 4,      // per box and block: sum w_LJ, sum w_coul, sum s.F (kJ/mol), sum |P_mol|^2 / M (kJ/mol)
       WATER_VIR_ROW = 6 };    // per box: W_LJ, W_coul,pair, W_recip, W_intra, KE_com, W_mol = ((W_LJ + W_coul,pair) + W_recip) - W_intra
struct WVirArgs {
    WaterArgs w;
    double w_h;                // the M-site's hydrogen weight, 0 = 3-site
    int mchunk;                // w_h != 0: molecules per slice of the Lennard-Jones pass, as W4Args
    const double* sites;       // w_h != 0: [n][3] the charge sites k_w4_sites left
    const float* v;            // [n][3] or null
    double mass_o, mass_h;     // amu
    double* vpart;             // [n_boxes][slices][n_per_box][WATER_VIR_PART]
    double* vljpart;           // w_h != 0: [n_boxes][slices][n_per_box / 3] the oxygen's sum -(r u_LJ'(r))
    double* vublk;             // [n_boxes][kblocks]: block sums of A |S|^2 (1 - k^2 / 2 alpha^2)
    double* vblk;              // [n_boxes][blocks][WATER_VIR_ACC]
    double* vrows;             // [...][n_boxes][WATER_VIR_ROW], the row of w.slot
};
// k_wvir_pairs (or k_wvir_pairs4 and k_wvir_lj4), k_wvir_sk, k_wvir_mols, k_wvir_final
int launch_water_virial(const WVirArgs& a, hipStream_t st);

// ---- energy minimiser (minimize.hip) ----------------------------------------------------------------
// FIRE under the Lennard-Jones potential of classical.hip, per box, all state in double.  `c` carries
// the potential's constants, the geometry of the pair pass and its work buffers (part, blk) as for ClassicalArgs, with
// c.box_edges set; c.x, c.f, c.f_cl, c.rows, c.steps, c.slot, c.g and c.devflags are not used.  One iteration is three
// launches (pairs, atoms, update); every kernel returns at once for a box with stopped[box] != 0.
// (No kernel uses a value it read from memory as an address: the checked build has nothing to range-check here.)
enum { MIN_STATE = 4,          // per box and slot: dt, alpha, n_pos, unused
       MIN_ACC = 5,            // per box and block (the first doubles of a CLASSICAL_ROW-strided row of blk): ff, vf, vv, sum u_i, max |F_c|
       MIN_ROW = 8 };          // per box: state, iterations, U and rms at the start, U, rms and max |F_c| at the end, the final dt
enum { MIN_CONVERGED = 0, MIN_MAX_ITER = 1, MIN_FAILED = 2 };
// what the two minimisers share: FIRE's buffers, parameters and the position of this pass (gamd_passes_dev.h)
struct FireArgs {
    double* x64;               // [n][3] positions, length unit, unwrapped (water: every molecule on the rigid geometry)
    double* v64;               // [n][3] FIRE velocities (water: projected by the molecule pass)
    double* f64;               // [n][3] kJ/mol/nm at x64 (water: projected onto the constraint manifold)
    double* state;             // [n_boxes][2][MIN_STATE]: iteration `it` reads slot it & 1 and writes the other
    int* stopped;              // [n_boxes] 0: running, else 1 + MIN_*
    double* rows;              // [n_boxes][MIN_ROW]
    double tol;                // kJ/mol/nm
    double dt_start, dt_max, f_inc, f_dec, alpha_start, f_alpha, max_step;
    int n_min;
    int last;                  // the pass behind the last iteration: a box still running stops as MIN_MAX_ITER, nothing moves
    long long it;              // position updates enqueued in front of this pass
};
struct MinArgs {
    ClassicalArgs c;
    FireArgs fire;
};
int launch_minimize_init(const MinArgs& m, const float* x, hipStream_t st);
// `cells` (gamd_classical_cells; m.c arrives with slices = 1): launch_classical_cells (the table from x64, k_ljcell_min) stands where k_min_pairs is
int launch_minimize_iter(const MinArgs& m, hipStream_t st, const CellTabBufs* cells = nullptr);
// x_out = fp32(x64) wrapped (skipped for a box that failed at iteration 0); f_out = f_in for every box that did not fail
int launch_minimize_store_x(const MinArgs& m, float* x_out, hipStream_t st);
// (either minimiser's: n and bx are the handle's atoms and boxes)
int launch_minimize_store_f(const FireArgs& m, int n, const BoxRef& bx, const float* f_in, float* f_out, hipStream_t st);

// ---- L-BFGS energy minimiser (lbfgs.hip) --------------------------------------------------------------
// Limited-memory BFGS with a backtracking line search under the Lennard-Jones potential of classical.hip, per box, all state in
// double (tests/lbfgs_ref.py is the recipe).  `c` as for MinArgs.  One evaluation is three launches
// whatever m is (pairs on the trial positions, dots, decide/update); with gamd_classical_cells the table's five come on top.
// Pass `it` (0: the start, then one per evaluation) reads state slot it & 1 and the gates gates[it & 1], and writes the other of
// each: no thread reads what its launch writes, and a box that stops in a pass still finishes that pass in every thread.
// The ring's slot numbers live in the state: they pass through GAMD_CHK_RANGE before they address the ring.
enum { LBFGS_M = 8,            // ring slots the scalar state has room for: m <= LBFGS_M
       LBFGS_SC = 16,          // per box and slot, scalars: t, rejections, pairs held, next ring slot, U, F.F, max |F_i|, accepted, skipped, resets
       LBFGS_SY = LBFGS_SC,                             // [M][M] s_i . y_j by ring slot
       LBFGS_YY = LBFGS_SY + LBFGS_M * LBFGS_M,         // [M][M] y_i . y_j
       LBFGS_FS = LBFGS_YY + LBFGS_M * LBFGS_M,         // [M] F . s_i
       LBFGS_FY = LBFGS_FS + LBFGS_M,                   // [M] F . y_i
       LBFGS_SLOT = LBFGS_FY + LBFGS_M,
       LBFGS_ACC = 9 + 3 * LBFGS_M,                     // per box and block: sum u_i, Ft.Ft, F.s, s.s, s.y, y.y, s.Ft, y.Ft, [M] s.y_k, [M] Ft.s_k, [M] Ft.y_k, max |Ft_i|
       LBFGS_ROW = 10 };       // per box: state, evaluations, accepted steps, U and rms at the start, U, rms and max |F_i| at the end, pushes skipped, resets
enum { LBFGS_CONVERGED = 0, LBFGS_MAX_ITER = 1, LBFGS_FAILED = 2, LBFGS_LINE_SEARCH = 3 };
enum { GAMD_CHK_LBFGS_COUNT = 161, GAMD_CHK_LBFGS_SLOT = 162 };
struct LbfgsArgs {
    ClassicalArgs c;
    double* x;                 // [n][3] the accepted positions, length unit, unwrapped
    double* xt;                // [n][3] the trial positions
    double* f;                 // [n][3] kJ/mol/nm at x
    double* ft;                // [n][3] kJ/mol/nm at xt
    double* d;                 // [n][3] the direction of the running line search
    double* ring;              // [2 m][n][3]: s of slot 0 .. m - 1, then y of slot 0 .. m - 1
    double* blk;               // [n_boxes][blocks][LBFGS_ACC]
    double* state;             // [n_boxes][2][LBFGS_SLOT]
    int* gates;                // [2][n_boxes] 0: running, else 1 + LBFGS_*
    double* rows;              // [n_boxes][LBFGS_ROW]
    int* sticky;               // host-mapped (checked build)
    double tol;                // kJ/mol/nm
    double max_step, c1, curv;
    int m, max_ls;
    long long max_iter;
    long long it;              // evaluations enqueued in front of this pass's
};
int launch_lbfgs_init(const LbfgsArgs& l, const float* x, hipStream_t st);
// `cells` as for launch_minimize_iter
int launch_lbfgs_eval(const LbfgsArgs& l, hipStream_t st, const CellTabBufs* cells = nullptr);
// x_out = fp32(x) wrapped, for every box that did not fail; `gates`: the set the last pass wrote
int launch_lbfgs_store_x(const LbfgsArgs& l, const int* gates, float* x_out, hipStream_t st);

// ---- water energy minimiser (water_minimize.hip) ------------------------------------------------------
// Rigid-molecule FIRE under the 3-site water potential of water_classical.hip, per box, all state in double (DESIGN.md section
// 4.13).  `w` carries the potential's constants, the geometry of the pair and reciprocal passes and the observer's work buffers
// (part, rho_partial, sk, ublk, rpart, blk) as for WaterArgs, with w.box_edges and w.species set; w.x, w.f, w.f_cl, w.rows,
// w.steps, w.slot and w.g are not used, and w.kchunk is not either: slice s of the reciprocal force pass walks the 256-vector
// blocks s, s + kslices, ... of the list, so a longer list (another box of the handle has a longer edge) only appends terms of
// weight zero.  One iteration is six launches (pairs; rho, sk, recip; molecules; update); every k_wmin_* kernel returns at once
// for a box with stopped[box] != 0.  States, rows and the scalar slots are the minimiser's (MIN_*).
// (No kernel uses a value it read from memory as an address: the checked build has nothing to range-check here.)
enum { WMIN_ACC = 7 };         // per box and block (the first doubles of a WATER_ACC-strided row of blk): ff, vf, vv, sum u_LJ, sum u_coul, sum z^2, max |F_c|
struct WMinArgs {
    WaterArgs w;
    FireArgs fire;
    double ra, rb, rc;         // the unit-weight canonical triangle: rc = r_hh / 2, t = sqrt(r_oh^2 - rc^2), ra = 2 t / 3, rb = t / 3
};
int launch_wmin_init(const WMinArgs& m, const float* x, hipStream_t st);
int launch_wmin_iter(const WMinArgs& m, hipStream_t st);
// x_io = fp32(x64) with molecules whole and the oxygen in [0, L) (skipped for a box that failed at iteration 0); x64_out (may be
// null) = x64, or the input widened for such a box
int launch_wmin_store_x(const WMinArgs& m, float* x_io, double* x64_out, hipStream_t st);
// the four force launches of an iteration alone (k_wmin_pairs, k_wmin_rho, k_water_sk, k_wmin_recip) on m.fire.x64 under the gate
// m.fire.stopped, into m.w.part, m.w.rpart, m.w.sk and m.w.ublk: nothing else of m.fire is read (water_lbfgs.hip hands over its
// trial positions and the gate set of its pass)
int launch_wmin_force(const WMinArgs& m, hipStream_t st);

// ---- water L-BFGS energy minimiser (water_lbfgs.hip) ---------------------------------------------------
// Limited-memory BFGS with a backtracking line search on RIGID 3-site molecules under the water potential, per box, all state
// in double (tests/water_lbfgs_ref.py is the recipe).  `w`, ra, rb, rc as for WMinArgs; the L-BFGS
// members, the state slots (LBFGS_SLOT), the gates, the rows (LBFGS_ROW) and the states are LbfgsArgs'.  One evaluation is six
// launches whatever m is: launch_wmin_force on xt under the gates of the pass, k_wlb_mols, k_wlb_update.  Pass `it`, the two
// gate sets and the two state slots as for LbfgsArgs.
enum { WLB_ULJ = 0, WLB_UC = 1, WLB_Z2 = 2, WLB_FTFT = 3, WLB_FS = 4, WLB_SS = 5, WLB_SY = 6, WLB_YY = 7, WLB_SFT = 8, WLB_YFT = 9,
       WLB_SYK = 10, WLB_FTSK = WLB_SYK + LBFGS_M, WLB_FTYK = WLB_FTSK + LBFGS_M, WLB_MAX = WLB_FTYK + LBFGS_M,
       WLB_ACC = WLB_MAX + 1 };  // per box and block: sum u_LJ, sum u_coul, sum z^2, Ft.Ft, F.s, s.s, s.y, y.y, s.Ft, y.Ft, [M] s.y_k, [M] Ft.s_k, [M] Ft.y_k, max |Ft_i|
enum { GAMD_CHK_WLBFGS_COUNT = 163, GAMD_CHK_WLBFGS_SLOT = 164 };
struct WLbfgsArgs {
    WaterArgs w;
    double ra, rb, rc;         // the unit-weight canonical triangle, as WMinArgs
    double* x;                 // [n][3] the accepted positions, length unit, unwrapped, every molecule rigid
    double* xt;                // [n][3] the trial positions, rigid
    double* f;                 // [n][3] kJ/mol/nm at x, projected at x
    double* ft;                // [n][3] kJ/mol/nm at xt, projected at xt
    double* d;                 // [n][3] the direction of the running line search
    double* ring;              // [2 m][n][3]: s of slot 0 .. m - 1, then y of slot 0 .. m - 1
    double* blk;               // [n_boxes][blocks][WLB_ACC]
    double* state;             // [n_boxes][2][LBFGS_SLOT]
    int* gates;                // [2][n_boxes] 0: running, else 1 + LBFGS_*
    double* rows;              // [n_boxes][LBFGS_ROW]
    int* sticky;               // host-mapped (checked build)
    double tol;                // kJ/mol/nm
    double max_step, c1, curv;
    int m, max_ls;
    long long max_iter;
    long long it;              // evaluations enqueued in front of this pass's
};
int launch_wlbfgs_init(const WLbfgsArgs& l, const float* x, hipStream_t st);
int launch_wlbfgs_eval(const WLbfgsArgs& l, hipStream_t st);
// x_io = fp32(x) by k_wmin_store_x's wrap and x64_out (may be null) = x, for every box that did not fail (such a box keeps x_io,
// and x64_out is x_io widened); `gates`: the set the last pass wrote
int launch_wlbfgs_store_x(const WLbfgsArgs& l, const int* gates, float* x_io, double* x64_out, hipStream_t st);

// ---- the water minimisers under the configured potential (water_relax.hip) -----------------------------
// gamd_water_minimize_potential: an iteration of gamd_water_minimize or an evaluation of
// gamd_water_minimize_lbfgs whose force stage follows the three switches of the potential as WaterPotential::drive does, on the
// minimiser's DOUBLE positions.  The argument blocks arrive as the routed potential leaves them: w.slices = 1 and
// w.chunk = n_per_box under the cell table, w.kslices = 1 and w.kblocks = pme_blocks under particle-mesh Ewald.
//   3-site   pairs: k_wmin_pairs, or launch_water_cells on x64 with the O-O term in the walk;
//            reciprocal: k_wmin_rho, k_water_sk, k_wmin_recip (the strided k walk), or launch_water_pme on x64
//   M-site   k_wrx_sites; pairs: k_w4_pairs, or launch_water_cells on the sites; k_wrx_lj;
//            reciprocal: k_w4_rho, k_water_sk, k_w4_recip (the kchunk walk), or launch_water_pme on the sites
// then k_wrx_mols and k_wmin_update, or k_wrx_lbmols and k_wlb_update.  The k_wrx_ and k_wmin_ / k_wlb_ kernels skip a stopped
// box; the reused observer kernels know DEVFLAG_FROZEN alone and evaluate it again into work buffers nobody reads for it.
// (No k_wrx_ kernel uses a value it read from memory as an address but k_wrx_lbmols' ring count, which passes through
// GAMD_CHK_RANGE under GAMD_CHK_WLBFGS_COUNT as in k_wlb_mols.)
struct WRxRoute {
    double w_h;                // the M-site's hydrogen weight, 0 = 3-site
    int mchunk;                // w_h != 0: molecules per slice of the Lennard-Jones pass, as W4Args
    double* sites;             // w_h != 0: [n][3] the charge sites k_wrx_sites writes
    double* ljpart;            // w_h != 0: [n_boxes][slices][n_per_box / 3][W4_LJ]
    const PmeArgs* pme;        // particle-mesh Ewald in force (its w and sites are set here), or null: the plain sum
    const CellTabBufs* cells;  // the cell table in force, or null: all pairs
};
// what the three kinds of k_wrx_ kernels take
struct WRxSiteArgs { W4Args b; const double* x64; const int* stopped; };       // k_wrx_sites, k_wrx_lj: positions and gates of the pass
struct WRxMinArgs { WMinArgs m; double w_h, w_o; const double* ljpart; };      // k_wrx_mols
struct WRxLbArgs { WLbfgsArgs l; double w_h, w_o; const double* ljpart; };     // k_wrx_lbmols
int launch_wrx_iter(const WMinArgs& m, const WRxRoute& r, hipStream_t st);
int launch_wrx_eval(const WLbfgsArgs& l, const WRxRoute& r, hipStream_t st);
// pieces of the existing files the route is put together from, each with its launcher's own checks: k_wmin_pairs alone; k_wmin_rho,
// k_water_sk, k_wmin_recip alone; k_wmin_update / k_wlb_update alone; k_w4_pairs alone; k_w4_rho, k_water_sk, k_w4_recip alone.
// `routed` (also on the init and store-x launchers below): the block is a routed one, whose k side is not the plain sum's.
int launch_wmin_pairs(const WMinArgs& m, hipStream_t st);
int launch_wmin_recip(const WMinArgs& m, hipStream_t st);
int launch_wmin_update(const WMinArgs& m, hipStream_t st);
int launch_wlbfgs_update(const WLbfgsArgs& l, hipStream_t st);
int launch_w4_pairs(const W4Args& b, hipStream_t st);
int launch_w4_recip(const W4Args& b, hipStream_t st);
int launch_wmin_init_routed(const WMinArgs& m, const float* x, hipStream_t st);
int launch_wmin_store_x_routed(const WMinArgs& m, float* x_io, double* x64_out, hipStream_t st);
int launch_wlbfgs_init_routed(const WLbfgsArgs& l, const float* x, hipStream_t st);
int launch_wlbfgs_store_x_routed(const WLbfgsArgs& l, const int* gates, float* x_io, double* x64_out, hipStream_t st);
