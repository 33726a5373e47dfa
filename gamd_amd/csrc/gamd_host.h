// gamd_host.h — the handle and the host-side helpers shared by the host translation units of libgamd_hip.so (gamd_api.hip,
// forward.hip, observe.hip).  Not part of the C ABI (include/gamd_hip.h) and not exported: hidden visibility, the dynamic symbols stay as they were.
#pragma once
#include "../../include/gamd_hip.h"
#include "gamd_common.h"
#include "gamd_internal.h"
#include "gamd_weights_host.h"

#include <cstdarg>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)

inline thread_local char g_err[512] = "";          // gamd_last_error(), per thread

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess) return fail(-1000 - (int)e__, "%s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

// Initialising work — zeroing a fresh buffer, uploading a small table — goes to ONE stream and is waited for on THAT stream
// before the call returns: the caller's stream inside the entry points that take one, the handle's private non-blocking
// stream everywhere else (gamd_create, gamd_finalize_weights, gamd_set_bonds).  Nothing is ordered on, or waits for, the NULL
// stream: a hipMemset / hipMemcpy there is asynchronous to the host for device memory and not ordered with a non-blocking
// stream at all (round 5: the momentum sums of a run's first step, com_partial, were wiped after k_com_partial on the caller's
// non-blocking stream had written them, once in ~300 runs), and a NULL-stream synchronise inside a library stalls every
// blocking stream of the process.  InitStream is set by every entry point (RAII, per thread: different handles may be driven
// from different threads).
inline thread_local hipStream_t tl_init_stream = nullptr;
struct InitStream {
    hipStream_t prev;
    explicit InitStream(hipStream_t st) : prev(tl_init_stream) { tl_init_stream = st; }
    ~InitStream() { tl_init_stream = prev; }
    InitStream(const InitStream&) = delete;
    InitStream& operator=(const InitStream&) = delete;
};
// host -> device upload of a small table from pageable memory, landed before it returns
inline hipError_t init_upload(void* dst, const void* src, size_t bytes) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, tl_init_stream);
    return e != hipSuccess ? e : hipStreamSynchronize(tl_init_stream);
}

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t want, bool zero) {
        if (want <= bytes && p) return 0;
        if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return (int)e; p = nullptr; bytes = 0; }
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) return (int)e;
        bytes = want;
        if (zero) {
            // on the call's stream (InitStream) and waited for there: allocations are rare, and what a call allocates and
            // initialises has landed before it returns whatever stream the next call comes on
            e = hipMemsetAsync(p, 0, want, tl_init_stream);
            if (e == hipSuccess) e = hipStreamSynchronize(tl_init_stream);
            if (e != hipSuccess) return (int)e;
        }
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct LayerDev {
    // edge side
    const float *w1p, *w2p, *w3p, *w4p, *b1, *b3, *b4;
    const float *w16p = nullptr;                        // generic-width fp32: the blocks again, packed for wide16.hip
    const float *e_ln_g = nullptr, *e_ln_b = nullptr;   // update_edge_emb: this layer's edge_layer_norm
    const float *w3p_l0 = nullptr, *b3_l0 = nullptr;    // layer-0 form (gamd_handle::l0_hoist): W3, b3 in the F2 output order
                                                        // (gamd_handle::ln_fold: w1p = A_l + the extra K step's fragment, b1 = b1'_l)
    NodeLayerW node;
};

// every entry point runs on the handle's device and leaves the caller's current device as it found it
struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (changed) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// the gamd_md_run / gamd_md_run_nhc call whose steps are still in the stream: what gamd_sync_status needs to finish the
// run after a neighbour-buffer overflow froze it
struct MdPending {
    bool active = false;
    int kind = 0;                      // 0: split BAOAB, 1: split Nose-Hoover chain
    MdArgs m{};
    NhcArgs a{};
    unsigned long long first_step = 0;
    float mass = 0.f, mass_h = 0.f;    // BAOAB: mass_amu / mass_h_amu as given (MdArgs keeps their reciprocals)
    long long n_steps = 0;
    float* x = nullptr;
    float* f = nullptr;
    const uint8_t* species = nullptr;
    hipStream_t st = nullptr;
};

// ---- run observers (observe.hip: reporter, recorder, structure sampler, classical observer) as the MD driver sees them --------
struct Observers;
Observers* observers_new();
void observers_free(gamd_handle* h);           // releases their device buffers (under the caller's DeviceGuard)
// at the top of a run, in front of any device work (the first failing check decides the error text) ...
int observers_check_run(gamd_handle* h, const float* box, const uint8_t* species_dev);
// ... and once the run is certain to be enqueued
void observers_begin_run(gamd_handle* h, const float* box, const uint8_t* species_dev, long long n_steps);
// Does step s carry a sample?  Its second half must then be complete in front of observers_enqueue(h, s); both walk one list.
bool observers_sampled(const gamd_handle* h, long long s);
int observers_enqueue(gamd_handle* h, long long s);
// ---- the classical force source (gamd_md_force_source; observe.hip, drive.hip) ------------------------------------------------
// may this handle take `source`, GAMD_FORCE_CLASSICAL or GAMD_FORCE_WATER_CLASSICAL (the potential of its kind with parameters
// set)?  0, or -22 with the message
int drive_check_source(gamd_handle* h, int source);
// at the top of a run whose h->force_source is one of the two, in front of any device work: the potential's box rule and its
// work buffers (nothing is allocated inside a run), whether or not its observer is armed.  Water: species, and the k-vector
// list of these boxes built or swapped, which no pending run may still read (-22 while one is).
int drive_check_run(gamd_handle* h, const float* box, const uint8_t* species_dev);
// the force evaluation of one step of the pending run, behind the neighbour stage: the pending run's f from its x
int drive_enqueue(gamd_handle* h);

struct gamd_handle {
    gamd_config cfg{};
    int dev = 0;
    int n = 0, L = 0, n_cu = 256;               // n: atoms of ALL boxes together (n_boxes * n_per_box)
    int n_boxes = 1, n_per_box = 0;              // gamd_config.n_boxes: independent boxes evaluated in one set of launches
    bool use_small = false;                      // skin mode: the single-workgroup small-system path of neighbor.hip (decided once)
    DevBuf boxes_dev, box_shift;                 // n_boxes > 1: per-box dimensions (BoxRef::boxes), scratch of the row scan
    std::vector<float> boxes_host;               // [n_boxes][3] as last set
    Route rt;                                    // gamd_route_host.h: padded widths, family flags, one kernel enumerator per stage — set by
                                                 // gamd_create, again by gamd_finalize_weights once the state_dict says update_edge or not
    int norm_bn = 0;                             // graph_conv.norm_layers are BatchNorm1d (running statistics in the state_dict)
    long long small_tile_limit = 512;            // fp32 path: at most this many 32-edge tiles -> conv_edge_small.hip
    std::map<std::string, HostTensor> host_w;
    bool finalized = false;
    double scaler_mean = 0.0, scaler_var = 1.0;

    // packed weights on device
    DevBuf wblob;
    std::vector<LayerDev> layers;
    const float *enc_w1p = nullptr, *enc_w2p = nullptr, *enc_w3p = nullptr, *enc_b1 = nullptr, *enc_b2 = nullptr,
                *enc_b3 = nullptr, *enc_lng = nullptr, *enc_lnb = nullptr, *centers = nullptr;
    const float *node_emb = nullptr, *nenc_w = nullptr, *nenc_b = nullptr;
    const float *dec_w1p = nullptr, *dec_b1 = nullptr, *dec_w2 = nullptr, *dec_b2 = nullptr;
    float length_mean = 0.f, length_std = 1.f;
    RbfGrid rbf{};                               // set when edge_expand.centers is a uniform grid

    // per-atom buffers
    DevBuf pos_w, pos_s, cell_of, perm, inv_perm, deg, row_ptr, na_excl, bond_nbr;
    DevBuf hbuf, hn, S, D, P, f_norm, f_den;
    // Layer-0 node tables of their own (skin mode): h0 and pre(0)'s hn / S / D / P depend on the species and the weights only,
    // not on the positions — in sorted atom order they change when the candidate list is rebuilt (the atoms are renumbered), not
    // otherwise.  Inside an enqueued MD run the first node launch of a step therefore returns at once unless that step rebuilt
    // (NodeArgs::l0_gate): the other layers' tables are overwritten layer by layer, these are not.
    DevBuf l0_h, l0_hn, l0_S, l0_D, l0_P;
    // cells
    DevBuf cell_start;                           // (the per-cell counts and fill cursors live behind the counters: set_box)
    int ncell_cap = 0;
    // edges
    long long e_cap = 0;
    long long piece_cap = 0;        // rows of `partial`
    DevBuf col, erow, chunk_piece, chunk_mask, e_frag, partial, feat_dbg, e_emb, e_frag2;
    DevBuf e_rstd;                               // ln_fold: [tiles][64] rstd fragments beside e_frag (EncArgs::rstd_out)
    DevBuf counters, tdbg, tmp_eid, ke_partial, com_partial;
    DevBuf cnt2;                    // small systems in skin mode: two counter blocks used alternately (no per-call memset)
    int cnt_parity = 0;
    long long skin_calls = 0;       // skin-mode force evaluations so far (rebuild-frequency estimate)
    int* cur_counters = nullptr;    // the counter block of the call being enqueued
    int* counters_host = nullptr;   // pinned
    // gamd_forces_host: pinned staging buffers ([n][3] floats each) and the device copy of the positions, allocated on first use
    float* host_in = nullptr;
    float* host_out = nullptr;
    DevBuf pos_in;
    int* sticky_host = nullptr;     // pinned + mapped: overflow flags and rebuild count, written by kernels directly
    int* sticky_dev = nullptr;
    hipStream_t init_stream = nullptr;   // private non-blocking stream: initialising memsets / uploads of the entry points without a stream argument
    DevBuf devflags;                // [DEVFLAG_COUNT] device-resident freeze flag + where an MD run stopped
    const float* feat_dev = nullptr;   // gamd_set_node_features
    const uint8_t* rigid_checked = nullptr;   // species pointer whose O,H,H layout has been validated
    MdPending pending;
    int force_source = GAMD_FORCE_NETWORK;   // gamd_md_force_source: where the forces of gamd_md_run / gamd_md_run_nhc come from
    Observers* obs = nullptr;       // observe.hip (observers_new / observers_free)
    bool has_bonds = false;

    // Verlet-skin reuse (cfg.neighbor_skin > 0)
    float skin = 0.f;
    DevBuf ref_pos, cand_deg, cand_ptr, cand_col;
    long long cand_cap = 0;
    bool cand_valid = false;

    float box[3] = {0, 0, 0};
    float box_max = 0.f;            // longest edge of any box as last set: scale of the candidate radius' rounding margin
    int nc[3] = {1, 1, 1};
    int ncell = 1;                  // cells of all boxes together

    // live timing of the conv-edge kernel (gamd_timing_*)
    bool timing = false;
    std::vector<hipEvent_t> tev;     // pairs (start, stop)
    std::vector<int> tev_kind;       // per pair: l = the conv-layer edge kernel of layer l, 100 = the edge encoder (StageClock)
    size_t tev_used = 0;
    // one event at the top of every MD step of an enqueued run (and one behind the last): gamd_timing_read_steps
    std::vector<hipEvent_t> sev;
    std::vector<uint8_t> sev_closes; // per event: 1 = recorded BEHIND the last step of an enqueue (the interval to the next event
                                     // is the host's gap between two runs, not a step)
    size_t sev_used = 0;
    static constexpr size_t EVENT_POOL_CAP = 1u << 16;   // timing left on across a long run: recording stops here (never unbounded)
};

// ---- one force evaluation on a stream (forward.hip) ----------------------------------------------------------------------------
struct EdgeList { const int* centre; const int* neigh; long long n; };
struct ForwardCall {
    const float* pos = nullptr;
    const uint8_t* species = nullptr;
    float* out_norm = nullptr;                 // null: the handle's f_norm
    float* out_denorm = nullptr;               // null: not written
    hipStream_t st = nullptr;
    const EdgeList* edges = nullptr;           // the caller's edge list in place of a neighbour search
    const MdFuse* fuse = nullptr;              // skin mode: integrator halves that ride in the neighbour stage's first kernel
    bool copy_counters = true;                 // fetch this call's counter block behind the last launch
    bool l0_reuse = false;                     // NodeArgs::l0_gate: node(0) returns at once unless this call rebuilt the candidates
};
struct StageClock {
    gamd_handle* h;
    hipStream_t st;
    hipEvent_t* evs = nullptr;                 // gamd_profile: one event per mark, labels[i] names the stage in front of evs[i]
    int n_ev = 0;
    std::vector<std::string> labels;
    bool full = false;                         // the gamd_timing_* pool is full: the rest of the call is not timed
    void mark(const char* label);
    int begin(int kind);                       // 100: the edge encoder, l: the conv-layer edge kernel of layer l
    int end();
};
NbrArgs nbr_args(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev);
// neighbour stage, then the network — or, classical, drive_enqueue — then the counter copy
int enqueue_forward(gamd_handle* h, const ForwardCall& c, StageClock& clock, bool classical = false);

inline BoxRef box_ref(const gamd_handle* h) {
    BoxRef r{};
    r.n_boxes = h->n_boxes;
    r.n_per_box = h->n_per_box;
    r.inv_npb = 1.0f / (float)h->n_per_box;
    r.boxes = h->n_boxes > 1 ? h->boxes_dev.as<float4>() : nullptr;
    return r;
}

// checked build: a device-side range check (GAMD_CHK_RANGE) failed in some kernel since the last report
inline int check_traps(gamd_handle* h) {
    const int code = h->sticky_host[STICKY_CHECK_CODE];
    if (!code) return 0;
    const int value = h->sticky_host[STICKY_CHECK_VALUE], line = h->sticky_host[STICKY_CHECK_LINE];
    h->sticky_host[STICKY_CHECK_CODE] = 0;
    return fail(-35, "checked build: device-side range check %d failed (value %d, source line %d)", code, value, line);
}

#pragma GCC visibility pop
