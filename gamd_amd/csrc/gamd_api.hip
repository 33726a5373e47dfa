// gamd_api.hip — the handle's lifetime, the weight upload, the MD driver and the extern "C" entry points of include/gamd_hip.h
// (the handle itself is in gamd_host.h, the kernel route in gamd_route_host.h, weight packing in gamd_weights_host.h, the force
// evaluation in forward.hip; the run observers' entry points are in observe.hip).
#include "gamd_host.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <memory>
#include <optional>

static_assert(sizeof(gamd_config) == 96 && offsetof(gamd_config, n_boxes) == 88 && offsetof(gamd_config, edge_capacity) == 40,
              "gamd_config layout is part of the C ABI (gamd_amd/_lib.py mirrors it)");
static_assert(WH_FRAG_FLOATS == GAMD_WFRAG_FLOATS, "gamd_weights_host.h restates the size of a packed 128x128 weight");

namespace {

// centre-of-mass motion removal (MdCom): per-box, per-block momentum sums
int fill_com(gamd_handle* h, int enabled, MdCom* c) {
    c->enabled = enabled ? 1 : 0;
    c->blocks = std::max(1, std::min(16, (h->n_per_box + 1023) / 1024));
    c->partial = nullptr;
    if (!c->enabled) return 0;
    if (h->com_partial.ensure(sizeof(double) * 4 * (size_t)c->blocks * (size_t)h->n_boxes, true)) return fail(-12, "allocation failed");
    c->partial = h->com_partial.as<double>();
    return 0;
}

int alloc_candidates(gamd_handle* h, long long cap) {
    cap = std::max<long long>(cap, h->n);                         // fixed-width rows: at least one slot per atom
    if (h->cand_col.ensure(sizeof(int) * ((size_t)cap + 64), true)) return fail(-12, "candidate buffer allocation failed");
    h->cand_cap = cap;
    h->cand_valid = false;
    return 0;
}

int alloc_edges(gamd_handle* h, long long e_cap) {
    const size_t ec = (size_t)e_cap + 2 * GAMD_TILE;
    int r = 0;
    r |= h->col.ensure(sizeof(int) * ec, true);
    r |= h->erow.ensure(sizeof(int) * ec, true);
    r |= h->chunk_piece.ensure(sizeof(int) * (ec / GAMD_CHUNK + 2), true);
    r |= h->chunk_mask.ensure(sizeof(unsigned) * (ec / GAMD_CHUNK + 2), true);
    r |= h->e_frag.ensure(sizeof(float) * 4096 * (size_t)h->rt.EHT * (ec / GAMD_TILE + 1), false);
    if (h->rt.ln_fold) r |= h->e_rstd.ensure(sizeof(float) * 64 * (ec / GAMD_TILE + 1), false);
    r |= h->partial.ensure(sizeof(float) * (size_t)h->rt.H * (ec / GAMD_CHUNK + (size_t)h->n + 2), false);
    h->piece_cap = (long long)(ec / GAMD_CHUNK + (size_t)h->n + 2);
    if (h->rt.update_edge) {                        // e_emb rows of one layer and the updated embedding tiles (H == Eh)
        r |= h->e_emb.ensure(sizeof(float) * (size_t)h->rt.H * ec, false);
        r |= h->e_frag2.ensure(sizeof(float) * 4096 * (size_t)h->rt.EHT * (ec / GAMD_TILE + 1), false);
    }
    if (h->cfg.keep_stages) r |= h->feat_dbg.ensure(sizeof(float) * 48 * ec, true);
    if (r) return fail(-12, "edge buffer allocation failed for capacity %lld", e_cap);
    h->e_cap = e_cap;
    if (h->skin > 0.f) {
        const double grow = std::pow(((double)h->cfg.cutoff + h->skin) / (double)h->cfg.cutoff, 3.0);
        // candidate rows have a fixed width (capacity / n) on the grid-wide path AND on the small-system path (round 5), so what
        // must fit is the LONGEST row, not the total: ~2.5 x the mean row (e_cap is already 1.5 x the density estimate, x 1.7)
        const long long want = (long long)((double)e_cap * grow * 1.7) + 1024;
        if (want > h->cand_cap) return alloc_candidates(h, want);
    }
    return 0;
}

// The cell grid must hold the enlarged candidate radius (GAMD_SKIN_MARGIN_EPS, forward.hip: rc_build = rc + skin + 48 eps L, each
// fp32 predicate off by at most E = 10 eps L): a candidate pair is at most rc_build + E apart along every axis, and cell_coord
// (p * (nc / L), two roundings, |p nc / L| <= nc) places an atom up to 3 eps L from where it is, so two candidates land in the same
// or in adjacent cells when the cells are rc + skin + (48 + 10 + 6) eps L wide.  The 1.0001 factor gives more than that while
// 64 eps L <= 1e-4 (rc + skin), i.e. up to L = 26 (rc + skin); beyond that the second term takes over.  Without a skin the
// margin is zero and the grid is the 1.0001 rule alone.
constexpr double GAMD_CELL_MARGIN_EPS = 64.0 / 16777216.0;

// box: host [n_boxes][3].  Every box gets the cell grid a single-box handle would give it (cells at least cutoff + skin
// wide), cells numbered box after box; h->box / h->nc keep box 0 (what the single-box kernels' argument blocks carry).
int set_box(gamd_handle* h, const float* box, hipStream_t st = nullptr) {
    const int nb = h->n_boxes;
    bool changed = h->boxes_host.size() != (size_t)nb * 3;
    for (int b = 0; b < nb; ++b)
        for (int d = 0; d < 3; ++d) {
            const float v = box[3 * b + d];
            if (!(v > 0.f)) return fail(-22, "box[%d][%d] = %g is not positive", b, d, (double)v);
            if (!changed && h->boxes_host[(size_t)3 * b + d] != v) changed = true;
        }
    if (!changed) return 0;
    h->cand_valid = false;                                        // candidates were built for another box
    std::vector<int> grid((size_t)nb * 4);
    long long ncell = 0;
    float box_max = 0.f;
    for (int k = 0; k < 3 * nb; ++k) box_max = std::max(box_max, box[k]);
    // narrowest cell that holds the (candidate) radius: see GAMD_CELL_MARGIN_EPS; the first term decides up to 26 radii per edge
    const double radius = (double)h->cfg.cutoff + (double)h->skin;
    const double cell_min = std::max(radius * 1.0001, h->skin > 0.f ? radius + GAMD_CELL_MARGIN_EPS * (double)box_max : 0.0);
    for (int b = 0; b < nb; ++b) {
        long long nc_b = 1;
        for (int d = 0; d < 3; ++d) {
            const int nc = std::max(1, (int)std::floor((double)box[3 * b + d] / cell_min));
            grid[(size_t)4 * b + d] = nc;
            nc_b *= nc;
        }
        if (ncell + nc_b > (1ll << 30)) return fail(-22, "cell grid too large");
        grid[(size_t)4 * b + 3] = (int)ncell;
        ncell += nc_b;
    }
    for (int d = 0; d < 3; ++d) { h->box[d] = box[d]; h->nc[d] = grid[d]; }
    h->box_max = box_max;
    h->ncell = (int)ncell;
    if ((int)ncell > h->ncell_cap) {
        int r = 0;
        // counters | cell_cnt | cell_fill in one buffer so the per-call clear is a single memset
        r |= h->counters.ensure(sizeof(int) * (CNT_COUNT + 2 * (size_t)ncell), true);
        r |= h->cell_start.ensure(sizeof(int) * ((size_t)ncell + 1), true);
        if (r) return fail(-12, "cell buffer allocation failed");
        h->ncell_cap = (int)ncell;
    }
    h->boxes_host.assign(box, box + (size_t)nb * 3);
    if (nb > 1) {
        // kernels of earlier calls may still read the old dimensions: drain the stream before overwriting them (a box
        // change is rare: NPT-style drivers)
        HIP_TRY(hipStreamSynchronize(st));
        std::vector<float> img((size_t)nb * 12, 0.f);
        for (int b = 0; b < nb; ++b) {
            for (int d = 0; d < 3; ++d) { img[(size_t)12 * b + d] = box[3 * b + d]; img[(size_t)12 * b + 4 + d] = 0.5f * box[3 * b + d]; }
            memcpy(&img[(size_t)12 * b + 8], &grid[(size_t)4 * b], 4 * sizeof(int));
        }
        HIP_TRY(init_upload(h->boxes_dev.p, img.data(), sizeof(float) * img.size()));
    }
    return 0;
}

// rigid-water block shared by both integrators; returns 0 or an error code (message set)
int fill_rigid(const gamd_handle* h, int rigid_water, float mass_o, float mass_h, float r_oh, float r_hh,
               int* use_rigid, RigidWater* g) {
    *use_rigid = 0;
    if (!rigid_water) return 0;
    if (h->n_per_box % 3 != 0) return fail(-22, "rigid_water needs O,H,H triples: n_atoms = %d is not a multiple of 3", h->n_per_box);
    if (!(mass_h > 0.f) || !(mass_o > 0.f)) return fail(-22, "rigid_water needs mass_amu (O) and mass_h_amu (H)");
    if (!(r_oh > 0.f) || !(r_hh > 0.f) || !(r_hh < 2.f * r_oh)) return fail(-22, "rigid_water needs 0 < r_hh < 2 r_oh");
    const double rc = 0.5 * (double)r_hh, t = std::sqrt((double)r_oh * r_oh - rc * rc);
    const double ra = t * 2.0 * mass_h / ((double)mass_o + 2.0 * mass_h);
    g->m_o = mass_o; g->m_h = mass_h;
    g->rc = (float)rc; g->ra = (float)ra; g->rb = (float)(t - ra);
    *use_rigid = 1;
    return 0;
}

int check_ready(gamd_handle* h) {
    if (!h) return fail(-22, "null handle");
    if (!h->finalized) return fail(-22, "weights not finalized (call gamd_finalize_weights)");
    return 0;
}

// what every force evaluation needs besides positions and box (shared by the forces, md_run and profile entry points)
int check_model_inputs(gamd_handle* h, const uint8_t* species_dev) {
    if (h->cfg.kind == GAMD_KIND_WATER && !species_dev && !h->feat_dev)
        return fail(-22, "water model needs species (or gamd_set_node_features)");
    if (h->cfg.use_bond && !h->has_bonds) return fail(-22, "use_bond set but no bonds given (gamd_set_bonds)");
    return 0;
}

// rigid_water integrates O,H,H triples: check once per species buffer that the layout really is 1,0,0 per molecule
int check_rigid_layout(gamd_handle* h, const uint8_t* species_dev, hipStream_t st) {
    if (!species_dev) return fail(-22, "rigid_water needs species (O = 1, H = 0, atoms ordered O,H,H)");
    if (h->rigid_checked == species_dev) return 0;
    std::vector<uint8_t> sp((size_t)h->n);
    HIP_TRY(hipMemcpyAsync(sp.data(), species_dev, sp.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < h->n; ++i)
        if ((sp[(size_t)i] != 0) != (i % 3 == 0))
            return fail(-22, "rigid_water needs atoms ordered O,H,H per molecule: species[%d] = %d", i, (int)sp[(size_t)i]);
    h->rigid_checked = species_dev;
    return 0;
}

int clear_devflags(gamd_handle* h) {
    const int init[2] = {0, -1};                             // FROZEN, FROZEN_AT; the rebuild counter behind them stays
    HIP_TRY(init_upload(h->devflags.p, init, sizeof(init)));
    return 0;
}

// live timing: a HIP event on the launch stream in front of the first kernel of an MD step (and behind the last kernel of
// the run); consecutive events bracket one step.  Events are created outside the timed region (gamd_timing_enable).
int step_event(gamd_handle* h, hipStream_t st, bool closes = false) {
    if (!h->timing) return 0;
    if (h->sev_used == h->sev.size()) {
        if (h->sev.size() >= gamd_handle::EVENT_POOL_CAP) return 0;          // pool full: the rest of the run is not timed
        for (int k = 0; k < 256; ++k) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); h->sev.push_back(e); h->sev_closes.push_back(0); }
    }
    h->sev_closes[h->sev_used] = closes ? 1 : 0;
    HIP_TRY(hipEventRecord(h->sev[h->sev_used++], st));
    return 0;
}

// the force evaluation of step s of the pending MD run (of the steps enqueued from s_begin on): f from x, by the run's force source
int step_forces(gamd_handle* h, long long s, long long s_begin, const MdFuse* fuse = nullptr) {
    const MdPending& p = h->pending;
    ForwardCall c{p.x, p.species, nullptr, p.f, p.st, nullptr, fuse};
    c.copy_counters = s + 1 == p.n_steps;
    c.l0_reuse = s > s_begin;
    StageClock clock{h, p.st};
    return enqueue_forward(h, c, clock, h->force_source != GAMD_FORCE_NETWORK);     // (cannot change while the run is pending)
}

// steps [s_begin, n_steps) of the pending MD run; skip_first: the first half of step s_begin has already been done
int enqueue_md_steps(gamd_handle* h, long long s_begin, bool skip_first) {
    MdPending& p = h->pending;
    int r;
    // Skin mode, BAOAB (free atoms or rigid water): the B of step s-1 and the B A O A of step s ride in the first kernel of step s's force
    // evaluation (k_step_small / k_skin_check): 2 launches less per step; the last B is launched on its own.
    if (p.kind == 0 && h->skin > 0.f) {
        for (long long s = s_begin; s < p.n_steps; ++s) {
            if ((r = step_event(h, p.st))) return r;
            p.m.step = p.first_step + (unsigned long long)s;
            p.m.step_index = (int)s;
            // (the B of a step that carries an observer's sample has been launched on its own, in front of the sample)
            int do_second = (s > s_begin && !observers_sampled(h, s - 1)) ? 1 : 0;
            const int do_first = (skip_first && s == s_begin) ? 0 : 1;
            if (p.m.com.enabled) {
                // COM motion removal sits between the B of step s-1 and the first half of step s and needs a sum over all
                // atoms: the B is launched on its own, then the momentum sums; only the first half rides in the neighbour kernel
                if (do_second && do_first) {                      // B of step s - 1 + the momentum sums of step s: one launch
                    MdArgs prev = p.m;
                    prev.step_index = (int)(s - 1);
                    if ((r = launch_baoab_second_com(prev, p.st))) return fail(-1, "integrator launch failed (%d)", r);
                    do_second = 0;
                } else {
                    if (do_second) {
                        MdArgs prev = p.m;
                        prev.step_index = (int)(s - 1);
                        if ((r = launch_baoab_second(prev, p.st))) return fail(-1, "integrator launch failed (%d)", r);
                        do_second = 0;
                    }
                    if (do_first && (r = launch_com_partial(p.m.com, p.m.v, p.m.species, p.m.inv_mass, p.m.inv_mass_h, p.m.n, p.m.bx,
                                                            p.m.devflags, p.m.use_rigid, p.st)))
                        return fail(-1, "integrator launch failed (%d)", r);
                }
            }
            const MdFuse fuse{&p.m, do_second, do_first};
            if ((r = step_forces(h, s, s_begin, &fuse))) return r;
            if (s + 1 < p.n_steps && observers_sampled(h, s)) {        // a sampled step completes its B before the sample
                if ((r = launch_baoab_second(p.m, p.st))) return fail(-1, "integrator launch failed (%d)", r);
                if ((r = observers_enqueue(h, s))) return r;
            }
        }
        if (p.n_steps > s_begin) {
            p.m.step_index = (int)(p.n_steps - 1);
            if ((r = launch_baoab_second(p.m, p.st))) return fail(-1, "integrator launch failed (%d)", r);
            if ((r = observers_enqueue(h, p.n_steps - 1))) return r;
        }
        return step_event(h, p.st, true);
    }
    for (long long s = s_begin; s < p.n_steps; ++s) {
        if ((r = step_event(h, p.st))) return r;
        const bool first = !(skip_first && s == s_begin), baoab = p.kind == 0;
        if (baoab) { p.m.step = p.first_step + (unsigned long long)s; p.m.step_index = (int)s; }
        else p.a.step_index = (int)s;
        if (first && (r = baoab ? launch_baoab_first(p.m, p.st) : launch_nhc_first(p.a, p.st))) return fail(-1, "integrator launch failed (%d)", r);
        if ((r = step_forces(h, s, s_begin))) return r;
        if ((r = baoab ? launch_baoab_second(p.m, p.st) : launch_nhc_second(p.a, p.st))) return fail(-1, "integrator launch failed (%d)", r);
        if ((r = observers_enqueue(h, s))) return r;
    }
    return step_event(h, p.st, true);
}

// gamd_md_run / gamd_md_run_nhc (p: gamd_md_params / gamd_nhc_params, a: MdArgs / NhcArgs): atoms, units, rigid water, box,
// centre-of-mass motion removal and the freeze flags of the integrator's argument block
template <typename Params, typename Args>
int fill_run_args(gamd_handle* h, const Params* p, const float* box, const uint8_t* species_dev, hipStream_t st, Args* a) {
    int r;
    a->n = h->n; a->species = species_dev; a->dt = p->dt_ps;
    a->len = p->length_per_nm > 0.f ? p->length_per_nm : 10.0f;
    if ((r = fill_rigid(h, p->rigid_water, p->mass_amu, p->mass_h_amu, p->r_oh, p->r_hh, &a->use_rigid, &a->rigid))) return r;
    if (a->use_rigid && (r = check_rigid_layout(h, species_dev, st))) return r;
    for (int d = 0; d < 3; ++d) a->box[d] = box[d];
    a->bx = box_ref(h);
    if ((r = fill_com(h, p->remove_cm_motion, &a->com))) return r;
    a->devflags = h->devflags.as<int>();
    return 0;
}

// The top of gamd_md_run / gamd_md_run_nhc: every refusal the two share, in the order a bad call meets them (an integrator's own
// refusal texts `own_after_steps`, `own_after_inputs`, null when it has none to make, keep their places), then the guards of the
// entry point, which live in `scope` until it returns, and the box.
struct RunScope { std::optional<DeviceGuard> device; std::optional<InitStream> init; };
int begin_run(gamd_handle* h, bool pointers_given, long long n_steps, const uint8_t* species_dev, const float* box, int rigid_water,
              hipStream_t st, RunScope& scope, const char* own_after_steps = nullptr, const char* own_after_inputs = nullptr) {
    int r;
    if ((r = check_ready(h))) return r;
    if (!pointers_given) return fail(-22, "null argument");
    if (n_steps < 0 || n_steps > 0x3fffffff) return fail(-22, "n_steps out of range");
    if (own_after_steps) return fail(-22, "%s", own_after_steps);
    if ((r = check_model_inputs(h, species_dev))) return r;
    if (own_after_inputs) return fail(-22, "%s", own_after_inputs);
    if ((r = observers_check_run(h, box, species_dev))) return r;
    if (h->force_source == GAMD_FORCE_WATER_CLASSICAL && !rigid_water)
        return fail(-22, "the water classical force source needs rigid_water: the potential has no bond or angle term (same-molecule "
                         "pairs are excluded), so only the constraints hold a molecule together");
    if (h->force_source != GAMD_FORCE_NETWORK && (r = drive_check_run(h, box, species_dev))) return r;
    scope.device.emplace(h->dev);
    scope.init.emplace(st);
    return set_box(h, box, st);
}

// ... and once the run is certain to be enqueued (pending.kind and its argument block are set)
int start_run(gamd_handle* h, float* x_dev, float* f_dev, const uint8_t* species_dev, const float* box, long long n_steps, hipStream_t st) {
    MdPending& pd = h->pending;
    pd.active = true; pd.n_steps = n_steps;
    pd.x = x_dev; pd.f = f_dev; pd.species = species_dev; pd.st = st;
    observers_begin_run(h, box, species_dev, n_steps);
    return enqueue_md_steps(h, 0, false);
}

}  // namespace

extern "C" {

#ifdef GAMD_CHECKED
const char* gamd_version(void) { return "gamd_hip 0.1 (gfx950) checked"; }       // libgamd_hip_chk.so: device-side range checks
#else
const char* gamd_version(void) { return "gamd_hip 0.1 (gfx950)"; }
#endif
const char* gamd_last_error(void) { return g_err; }

int32_t gamd_create(const gamd_config* cfg, gamd_handle** out) {
    if (!cfg || !out) return fail(-22, "null argument");
    if (cfg->n_atoms <= 0) return fail(-22, "n_atoms must be positive");
    if (cfg->n_boxes < 0 || cfg->n_boxes > (1 << 20)) return fail(-22, "n_boxes out of range");
    const int n_boxes = cfg->n_boxes > 1 ? cfg->n_boxes : 1;
    // node-table rows are addressed with 32-bit byte offsets (row * 512 B, scalar base + offset loads) in the conv-layer edge
    // kernels: 2^23 - 1 rows including the zero row (a 288 GB device holds ~5e6 atoms of this model)
    if ((long long)cfg->n_atoms * n_boxes >= (1 << 23) - 1)
        return fail(-22, "n_atoms x n_boxes = %lld: at most %d atoms per handle", (long long)cfg->n_atoms * n_boxes, (1 << 23) - 2);
    if (cfg->n_layers <= 0 || cfg->n_layers > 16) return fail(-22, "n_layers out of range");
    if (!(cfg->cutoff > 0.f)) return fail(-22, "cutoff must be positive");
    if (cfg->edge_dtype != GAMD_EDGE_F32 && cfg->edge_dtype != GAMD_EDGE_BF16 && cfg->edge_dtype != GAMD_EDGE_F16X3)
        return fail(-22, "unknown edge_dtype");
    if (!(cfg->neighbor_skin >= 0.f)) return fail(-22, "neighbor_skin must be >= 0");
    if (cfg->self_loop_mode != GAMD_SELF_LOOP_DGL07_NOOP && cfg->self_loop_mode != GAMD_SELF_LOOP_APPEND_ZERO_FEATURE)
        return fail(-22, "unknown self_loop_mode %d", cfg->self_loop_mode);
    if (cfg->self_loop_mode != GAMD_SELF_LOOP_DGL07_NOOP && cfg->edge_dtype != GAMD_EDGE_F32)
        return fail(-22, "self_loop_mode 1 is built for the fp32 edge dtype only");
    if (cfg->kernel_select & ~(GAMD_KSEL_FORCE_GENERIC_WIDTH | GAMD_KSEL_FORCE_HALF_QUANTUM | GAMD_KSEL_NO_LAYER0_HOIST | GAMD_KSEL_NO_LN_FOLD))
        return fail(-22, "unknown kernel_select bits 0x%x", cfg->kernel_select);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(-19, "no HIP device available: libgamd_hip has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(-22, "device %d out of range (%d visible)", cfg->device, ndev);
    DeviceGuard guard(cfg->device);            // the caller's current device is restored on every return path
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
    // widths, kernel families and their refusals: gamd_route_host.h (update_edge is known once the weights are there)
    const Route rt = gamd_route(route_config(*cfg), false);
    if (rt.err) return fail(rt.err, "%s", rt.msg);
    if (!rt.f32 && rt.H == 256 && (long long)cfg->n_atoms * n_boxes > (1ll << 22) - 2)
        return fail(-22, "bf16 / split-fp16 with encoding_size > 128: at most 2^22 - 2 atoms per handle (32-bit byte offsets into hn)");
    std::unique_ptr<gamd_handle, int32_t (*)(gamd_handle*)> owner(new gamd_handle(), gamd_destroy);    // destroyed on every return but the last
    gamd_handle* const h = owner.get();
    h->obs = observers_new();
    h->cfg = *cfg;
    h->dev = cfg->device;
    if (hipStreamCreateWithFlags(&h->init_stream, hipStreamNonBlocking) != hipSuccess) {
        h->init_stream = nullptr;
        return fail(-12, "stream creation failed");
    }
    InitStream init(h->init_stream);
    h->n_boxes = n_boxes;
    h->n_per_box = cfg->n_atoms;
    h->n = cfg->n_atoms * n_boxes;
    h->L = cfg->n_layers;
    h->rt = rt;
    h->skin = cfg->neighbor_skin;
    h->small_tile_limit = route_tile_limit(cfg->small_tile_limit);
    h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const size_t n = (size_t)h->n;
    int r = 0;
    r |= h->pos_w.ensure(sizeof(float4) * n, true);
    // one extra row behind pos_s / perm for the padding edges that align the boxes of a batch (col = n): zero position,
    // original id -2 (matches no bond partner)
    r |= h->pos_s.ensure(sizeof(float4) * (n + 1), true);
    r |= h->cell_of.ensure(sizeof(int) * n, true);
    r |= h->perm.ensure(sizeof(int) * (n + 1), true);
    if (n_boxes > 1) {
        r |= h->boxes_dev.ensure(sizeof(float) * 12 * (size_t)n_boxes, true);
        r |= h->box_shift.ensure(sizeof(int) * ((size_t)n_boxes + 2), true);
    }
    r |= h->inv_perm.ensure(sizeof(int) * n, true);
    r |= h->deg.ensure(sizeof(int) * n, true);
    r |= h->row_ptr.ensure(sizeof(int) * (n + 1), true);
    r |= h->na_excl.ensure(sizeof(int) * (n + 1), true);
    const size_t nh = n * (size_t)rt.H * sizeof(float), nd = n * (size_t)rt.Dp * sizeof(float), zd = (size_t)rt.Dp * sizeof(float);
    r |= h->hbuf.ensure(nh * (cfg->keep_stages ? (size_t)h->L + 1 : 2), true);
    // one extra, all-zero row (index n) behind the node tables the conv-layer edge kernel gathers from: the padding
    // slots of the last 32-edge tile point at it, so their messages are exact zeros without a per-element mask
    r |= h->hn.ensure(nh + (size_t)rt.H * sizeof(float), true);
    r |= h->S.ensure(nd + zd, true);
    r |= h->D.ensure(nd + zd, true);
    r |= h->P.ensure(nd, true);
    if (cfg->neighbor_skin > 0.f) {
        r |= h->l0_hn.ensure(nh + (size_t)rt.H * sizeof(float), true);
        r |= h->l0_S.ensure(nd + zd, true);
        r |= h->l0_D.ensure(nd + zd, true);
        r |= h->l0_P.ensure(nd, true);
        if (!cfg->keep_stages) r |= h->l0_h.ensure(nh, true);
    }
    r |= h->f_norm.ensure(sizeof(float) * 3 * n, true);
    r |= h->f_den.ensure(sizeof(float) * 3 * n, true);
    r |= h->tdbg.ensure(sizeof(long long) * 16 * 8 * 1024, true);
    r |= h->devflags.ensure(sizeof(int) * DEVFLAG_COUNT, true);
    r |= h->cnt2.ensure(sizeof(int) * 2 * CNT_COUNT, true);
    if (r) return fail(-12, "device allocation failed");
    {
        const int no_atom = -2;
        if (init_upload(h->perm.as<int>() + n, &no_atom, sizeof(int)) != hipSuccess) return fail(-1, "device copy failed");
    }
    if ((r = clear_devflags(h))) return r;
    if (hipHostMalloc((void**)&h->counters_host, sizeof(int) * CNT_COUNT) != hipSuccess) return fail(-12, "pinned allocation failed");
    memset(h->counters_host, 0, sizeof(int) * CNT_COUNT);
    if (hipHostMalloc((void**)&h->sticky_host, sizeof(int) * STICKY_COUNT, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&h->sticky_dev, h->sticky_host, 0) != hipSuccess)
        return fail(-12, "mapped host allocation failed");
    memset(h->sticky_host, 0, sizeof(int) * STICKY_COUNT);
    if (h->skin > 0.f) {
        int rr = 0;
        rr |= h->ref_pos.ensure(sizeof(float4) * n, true);
        rr |= h->cand_deg.ensure(sizeof(int) * n, true);
        rr |= h->cand_ptr.ensure(sizeof(int) * (n + 1), true);
        if (rr) return fail(-12, "device allocation failed");
    }
    {
        std::vector<float> all((size_t)n_boxes * 3);              // every box starts with the constructor's box
        for (int b = 0; b < n_boxes; ++b)
            for (int d = 0; d < 3; ++d) all[(size_t)3 * b + d] = cfg->box[d];
        if ((r = set_box(h, all.data()))) return r;
    }
    {
        // Small-system path (k_step_small: skin check, integrator halves and — on the steps that need it — the cell build of a
        // candidate rebuild in ONE workgroup; the candidate rows are written by the count pass behind it).  Worth it while
        // rebuilds are rare and cheap: a box of 3 cells per axis (the 774-atom DFT-water configuration: every atom is a
        // candidate of every other, a rebuild every ~7 steps) is as fast on the grid-wide path (measured: 0.8825 against
        // 0.884 ms per step), and a dilute box with thousands of cells is walked faster by 32 workgroups than by one.
        const double per_atom = std::min<double>(h->n, 27.0 * h->n / std::max(1, h->ncell));
        h->use_small = h->n <= 1024 && n_boxes <= 1 && (double)h->n * per_atom <= 3.0e5 && h->ncell <= 4096;
    }
    long long ecap = cfg->edge_capacity;
    if (ecap <= 0) {
        const double vol = (double)cfg->box[0] * cfg->box[1] * cfg->box[2];
        const double per_atom = 4.18879 * std::pow((double)cfg->cutoff, 3) * (double)h->n_per_box / vol + 1.0;
        ecap = (long long)(1.5 * per_atom * (double)h->n) + 1024 + 16ll * n_boxes;
    }
    if (cfg->self_loop_mode) ecap += h->n;
    if ((r = alloc_edges(h, ecap))) return r;
    if (hipStreamSynchronize(h->init_stream) != hipSuccess) return fail(-1, "device synchronisation failed");
    *out = owner.release();                    // every initialising memset / copy has landed: any stream may use the handle
    return 0;
}

int32_t gamd_destroy(gamd_handle* h) {
    if (!h) return 0;
    DeviceGuard guard(h->dev);
    InitStream init(h->init_stream);
    h->devflags.release();
    h->cnt2.release();
    DevBuf* bufs[] = {&h->boxes_dev, &h->box_shift, &h->wblob, &h->pos_w, &h->pos_s, &h->cell_of, &h->perm, &h->inv_perm, &h->deg, &h->row_ptr,
                      &h->na_excl, &h->bond_nbr, &h->hbuf, &h->hn, &h->S, &h->D, &h->P, &h->l0_h, &h->l0_hn, &h->l0_S, &h->l0_D, &h->l0_P, &h->f_norm, &h->f_den,
                      &h->cell_start, &h->col, &h->erow, &h->chunk_piece,
                      &h->chunk_mask, &h->e_frag, &h->e_rstd, &h->e_emb, &h->e_frag2, &h->partial, &h->feat_dbg, &h->counters, &h->tdbg, &h->tmp_eid, &h->ke_partial, &h->com_partial,
                      &h->ref_pos, &h->cand_deg, &h->cand_ptr, &h->cand_col};
    for (DevBuf* b : bufs) b->release();
    observers_free(h);
    h->pos_in.release();
    if (h->host_in) (void)hipHostFree(h->host_in);
    if (h->host_out) (void)hipHostFree(h->host_out);
    if (h->counters_host) (void)hipHostFree(h->counters_host);
    if (h->sticky_host) (void)hipHostFree(h->sticky_host);
    for (hipEvent_t e : h->tev) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->sev) (void)hipEventDestroy(e);
    if (h->init_stream) (void)hipStreamDestroy(h->init_stream);
    delete h;
    return 0;
}

int32_t gamd_load_weight(gamd_handle* h, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
    if (!h || !name || !data || !shape || ndim < 1 || ndim > 2) return fail(-22, "bad argument to gamd_load_weight");
    HostTensor t;
    size_t cnt = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); cnt *= (size_t)shape[i]; }
    t.data.assign(data, data + cnt);
    h->host_w[name] = std::move(t);
    h->finalized = false;
    return 0;
}

// Transformation and packing are pack_weights (gamd_weights_host.h, host only); here: the route now that the state_dict is known,
// the upload, and the offset tables turned into the device pointers of the same names.
int32_t gamd_finalize_weights(gamd_handle* h) {
    if (!h) return fail(-22, "null handle");
    DeviceGuard guard(h->dev);
    InitStream init(h->init_stream);
    const RouteConfig rc = route_config(h->cfg);
    const Route rt = gamd_route(rc, route_update_edge(h->host_w));
    const PackedWeights pw = pack_weights(rc, rt, h->L, h->host_w);
    if (pw.err) return fail(pw.err, "%s", pw.msg);
    const bool regrow = rt.update_edge != h->rt.update_edge;     // e_emb / e_frag2 come and go with it
    h->rt = rt;
    if (regrow && alloc_edges(h, h->e_cap)) return -12;
    h->norm_bn = pw.norm_bn ? 1 : 0;
    h->length_mean = pw.length_mean;
    h->length_std = pw.length_std;
    h->rbf = RbfGrid{pw.rbf.uniform, pw.rbf.c0, pw.rbf.delta, pw.rbf.A, pw.rbf.B, pw.rbf.C};

    if (h->wblob.ensure(sizeof(float) * pw.blob.size(), false)) return fail(-12, "weight blob allocation failed");
    HIP_TRY(init_upload(h->wblob.p, pw.blob.data(), sizeof(float) * pw.blob.size()));
    const float* B = h->wblob.as<float>();
    auto at = [B](size_t off) { return off == WOFF_NONE ? nullptr : B + off; };
    h->layers.assign(pw.layers.size(), LayerDev{});
    for (size_t l = 0; l < pw.layers.size(); ++l) {
        const LayerOff& o = pw.layers[l];
        LayerDev& d = h->layers[l];
#define GAMD_W_SET(f) d.f = at(o.f);
        GAMD_W_LAYER_FIELDS(GAMD_W_SET)        // w16p stays null unless the blob carries the wide16.hip image
#undef GAMD_W_SET
#define GAMD_W_SET(f) d.node.f = at(o.node.f);
        GAMD_W_NODE_FIELDS(GAMD_W_SET)         // c0: null but in the layer-0 form ...
#undef GAMD_W_SET
        if (o.m0 != WOFF_NONE) d.node.wpep = at(o.m0);            // ... where post(0) multiplies by M0 in phi_edge's place
    }
#define GAMD_W_SET(f) h->f = at(pw.g.f);
    GAMD_W_GLOBAL_FIELDS(GAMD_W_SET)           // node_emb (LJ) or nenc_w / nenc_b (water): the other kind's stay null
#undef GAMD_W_SET
    h->finalized = true;
    return 0;
}

int32_t gamd_set_scaler(gamd_handle* h, double mean, double var) {
    if (!h) return fail(-22, "null handle");
    if (!(var >= 0.0)) return fail(-22, "scaler variance must be non-negative");
    h->scaler_mean = mean;
    h->scaler_var = var;
    return 0;
}

int32_t gamd_set_bonds(gamd_handle* h, const int32_t* bonds, int64_t n_bonds) {
    if (!h || (!bonds && n_bonds > 0)) return fail(-22, "bad argument to gamd_set_bonds");
    DeviceGuard guard(h->dev);
    InitStream init(h->init_stream);
    std::vector<int> tab((size_t)h->n * 4, -1);
    auto add = [&](int i, int j) -> int {
        for (int k = 0; k < 4; ++k) {
            if (tab[(size_t)i * 4 + k] == j) return 0;
            if (tab[(size_t)i * 4 + k] < 0) { tab[(size_t)i * 4 + k] = j; return 0; }
        }
        return -1;
    };
    // several boxes: the bond list names atoms of ONE box (every box has the same topology) and is applied to each of them
    for (int box = 0; box < h->n_boxes; ++box)
        for (int64_t b = 0; b < n_bonds; ++b) {
            int i = bonds[2 * b], j = bonds[2 * b + 1];
            if (i < 0 || j < 0 || i >= h->n_per_box || j >= h->n_per_box)
                return fail(-22, "bond %lld references atom out of range", (long long)b);
            i += box * h->n_per_box; j += box * h->n_per_box;
            if (add(i, j) || add(j, i)) return fail(-22, "more than 4 bonded partners for one atom is not supported");
        }
    if (h->bond_nbr.ensure(sizeof(int) * tab.size(), false)) return fail(-12, "bond table allocation failed");
    HIP_TRY(init_upload(h->bond_nbr.p, tab.data(), sizeof(int) * tab.size()));
    h->has_bonds = n_bonds > 0;
    return 0;
}

int32_t gamd_set_node_features(gamd_handle* h, const float* feat_dev) {
    if (!h) return fail(-22, "null handle");
    if (feat_dev && h->cfg.kind != GAMD_KIND_WATER) return fail(-22, "node features belong to the water models (the LJ model has node_emb)");
    h->feat_dev = feat_dev;
    return 0;
}

int32_t gamd_get_device_flags(gamd_handle* h, int32_t flags[4]) {
    if (!h || !flags) return fail(-22, "null argument");
    flags[0] = h->sticky_host[STICKY_NONFINITE] ? 1 : 0;
    flags[1] = flags[2] = flags[3] = 0;
    h->sticky_host[STICKY_NONFINITE] = 0;
    return 0;
}

int32_t gamd_build_neighbors(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, const float* box, void* stream) {
    int r;
    if ((r = check_ready(h))) return r;
    if (!pos_dev || !box) return fail(-22, "null argument");
    DeviceGuard guard(h->dev);
    InitStream init((hipStream_t)stream);
    hipStream_t st = (hipStream_t)stream;
    for (int attempt = 0; attempt < 4; ++attempt) {
        if ((r = set_box(h, box, st))) return r;
        h->cur_counters = h->counters.as<int>();
        NbrArgs na = nbr_args(h, pos_dev, species_dev);
        h->cand_valid = false;                                    // the exact build below reorders the atoms
        if ((r = launch_neighbor_build(na, st))) return fail(-1, "neighbor build launch failed (%d)", r);
        HIP_TRY(hipMemcpyAsync(h->counters_host, h->counters.p, sizeof(int) * CNT_COUNT, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        h->sticky_host[STICKY_EDGE_OVERFLOW] = 0;
        if (int t = check_traps(h)) return t;
        if (!h->counters_host[CNT_OVERFLOW]) return attempt ? 1 : 0;
        const long long need = (long long)(1.25 * (double)h->counters_host[CNT_E]) + 1024;
        if ((r = alloc_edges(h, need))) return r;
        if ((r = clear_devflags(h))) return r;
    }
    return fail(-34, "neighbor buffers still overflow after regrowing");
}

int32_t gamd_forces_async(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, const float* box,
                          float* out_norm_dev, float* out_denorm_dev, void* stream) {
    int r;
    if ((r = check_ready(h))) return r;
    if (!pos_dev || !box) return fail(-22, "null argument");
    if ((r = check_model_inputs(h, species_dev))) return r;
    DeviceGuard guard(h->dev);
    InitStream init((hipStream_t)stream);
    if ((r = set_box(h, box, (hipStream_t)stream))) return r;
    h->pending.active = false;
    const ForwardCall c{pos_dev, species_dev, out_norm_dev, out_denorm_dev, (hipStream_t)stream};
    StageClock clock{h, c.st};
    return enqueue_forward(h, c, clock);
}

int32_t gamd_sync_status(gamd_handle* h, void* stream) {
    if (!h) return fail(-22, "null handle");
    DeviceGuard guard(h->dev);
    InitStream init((hipStream_t)stream);
    bool resumed = false;
    for (int attempt = 0; attempt < 5; ++attempt) {
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        // the sticky flags catch an overflow in ANY step enqueued since the last check (gamd_md_run), not only the last
        const bool cand_ovf = h->sticky_host[STICKY_CAND_OVERFLOW] != 0;
        const bool edge_ovf = h->counters_host[CNT_OVERFLOW] || h->sticky_host[STICKY_EDGE_OVERFLOW];
        if (int t = check_traps(h)) { h->pending.active = false; return t; }
        if (!cand_ovf && !edge_ovf) {
            h->pending.active = false;
            if (h->cfg.edge_dtype != GAMD_EDGE_F32 && h->sticky_host[STICKY_NONFINITE])
                return fail(-33, "non-finite forces with a reduced-precision edge dtype: an MFMA operand left the fp16 range "
                                 "(|x| > 65504) or the input positions are not finite");
            return resumed ? 1 : 0;
        }
        int r;
        long long need = 0;
        if (cand_ovf) {
            const long long seen = std::max<long long>(h->sticky_host[STICKY_NCAND], h->cand_cap);
            need = (long long)(1.25 * (double)seen) + 1024;
            if ((r = alloc_candidates(h, need))) return r;
        }
        if (edge_ovf) {
            const long long seen = std::max<long long>(h->counters_host[CNT_E], h->e_cap);
            need = (long long)(1.25 * (double)seen) + 1024;
            if ((r = alloc_edges(h, need))) return r;
            h->cand_valid = false;
        }
        h->sticky_host[STICKY_CAND_OVERFLOW] = 0;
        h->sticky_host[STICKY_EDGE_OVERFLOW] = 0;
        h->counters_host[CNT_OVERFLOW] = 0;
        int flags[DEVFLAG_COUNT] = {0, -1, 0, 0};
        HIP_TRY(hipMemcpyAsync(flags, h->devflags.p, sizeof(flags), hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        if ((r = clear_devflags(h))) return r;
        if (!h->pending.active)
            return fail(-34, "%s neighbour buffers overflowed; regrown to %lld, re-issue the call", cand_ovf ? "candidate" : "edge", need);
        // an enqueued MD run froze at (step, half): forces at the frozen positions, the rest of that step, the remaining steps
        const int at = flags[DEVFLAG_FROZEN_AT];
        if (at < 0) {
            h->pending.active = false;
            return fail(-34, "neighbour buffers overflowed inside an MD run but no integrator kernel recorded where it stopped");
        }
        if ((r = enqueue_md_steps(h, at / 2, (at & 1) != 0))) return r;
        resumed = true;
    }
    h->pending.active = false;
    return fail(-34, "neighbour buffers still overflow after regrowing four times");
}

int32_t gamd_forces(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, const float* box,
                    float* out_norm_dev, float* out_denorm_dev, void* stream) {
    for (int attempt = 0; attempt < 4; ++attempt) {
        int r = gamd_forces_async(h, pos_dev, species_dev, box, out_norm_dev, out_denorm_dev, stream);
        if (r) return r;
        r = gamd_sync_status(h, stream);
        if (r == 0) return attempt ? 1 : 0;
        if (r != -34) return r;
    }
    return fail(-34, "neighbour buffers still overflow after regrowing");
}

// The reference's host-array boundary (predict_forces, LJ/train_network_lj.py:133-157) in one call with one synchronisation
int32_t gamd_forces_host(gamd_handle* h, const float* pos_host, const uint8_t* species_dev, const float* box, float* out_host,
                         int32_t denormalize, void* stream) {
    int r;
    if ((r = check_ready(h))) return r;
    if (!pos_host || !out_host || !box) return fail(-22, "null argument");
    DeviceGuard guard(h->dev);
    const size_t bytes = sizeof(float) * 3 * (size_t)h->n;
    if (!h->host_in) {
        InitStream init((hipStream_t)stream);
        if (hipHostMalloc((void**)&h->host_in, bytes) != hipSuccess) { h->host_in = nullptr; return fail(-12, "pinned allocation failed"); }
        if (hipHostMalloc((void**)&h->host_out, bytes) != hipSuccess) {
            (void)hipHostFree(h->host_in);
            h->host_in = h->host_out = nullptr;
            return fail(-12, "pinned allocation failed");
        }
        if (h->pos_in.ensure(bytes, false)) return fail(-12, "device allocation failed");
    }
    std::memcpy(h->host_in, pos_host, bytes);
    for (int attempt = 0; attempt < 4; ++attempt) {
        HIP_TRY(hipMemcpyAsync(h->pos_in.p, h->host_in, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
        if ((r = gamd_forces_async(h, h->pos_in.as<float>(), species_dev, box, nullptr, denormalize ? h->f_den.as<float>() : nullptr, stream)))
            return r;
        HIP_TRY(hipMemcpyAsync(h->host_out, denormalize ? h->f_den.p : h->f_norm.p, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
        r = gamd_sync_status(h, stream);                    // the one synchronisation; -34: regrown, replay
        if (r == 0) {
            std::memcpy(out_host, h->host_out, bytes);
            return attempt ? 1 : 0;
        }
        if (r != -34) return r;
    }
    return fail(-34, "neighbour buffers still overflow after regrowing");
}

int32_t gamd_forces_edges(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, const float* box,
                          const int32_t* centre_dev, const int32_t* neigh_dev, int64_t n_edges, float* out_norm_dev,
                          float* out_denorm_dev, void* stream) {
    int r;
    if ((r = check_ready(h))) return r;
    if (!pos_dev || !box || n_edges < 0 || (n_edges > 0 && (!centre_dev || !neigh_dev))) return fail(-22, "bad argument");
    if ((r = check_model_inputs(h, species_dev))) return r;
    if (n_edges > 0x7fff0000ll) return fail(-22, "edge list too long");
    DeviceGuard guard(h->dev);
    InitStream init((hipStream_t)stream);
    if ((r = set_box(h, box, (hipStream_t)stream))) return r;
    h->pending.active = false;
    int status = 0;
    // + one appended loop per atom, + at most 15 padding slots per box of a batch (neighbor.hip: d_box_align)
    const long long total = n_edges + (h->cfg.self_loop_mode ? h->n : 0) + (h->n_boxes > 1 ? 16ll * h->n_boxes : 0);
    if (total > h->e_cap) {                         // the count is known up front: grow before launching
        if ((r = alloc_edges(h, total + total / 8 + 1024))) return r;
        status = 1;
    }
    if (h->tmp_eid.ensure(sizeof(int) * ((size_t)std::max<long long>(total, 1) + 64), false))
        return fail(-12, "edge scratch allocation failed");
    const EdgeList el{centre_dev, neigh_dev, (long long)n_edges};
    ForwardCall c{pos_dev, species_dev, out_norm_dev, out_denorm_dev, (hipStream_t)stream};
    c.edges = &el;
    StageClock clock{h, c.st};
    if ((r = enqueue_forward(h, c, clock))) return r;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    h->sticky_host[STICKY_EDGE_OVERFLOW] = 0;
    if (h->counters_host[CNT_OVERFLOW]) {
        const int why = h->counters_host[CNT_OVERFLOW];
        h->counters_host[CNT_OVERFLOW] = 0;
        if ((r = clear_devflags(h))) return r;
        if (why == 2) return fail(-22, "edge list references an atom index outside [0, n_atoms)");
        return fail(-34, "edge buffers overflowed unexpectedly");
    }
    return status;
}

int32_t gamd_get_counts(gamd_handle* h, int64_t* n_edges, int64_t* n_pieces, int64_t* edge_capacity) {
    if (!h) return fail(-22, "null handle");
    if (n_edges) *n_edges = h->counters_host[CNT_E];
    if (n_pieces) *n_pieces = h->counters_host[CNT_PIECES];
    if (edge_capacity) *edge_capacity = h->e_cap;
    return 0;
}

int32_t gamd_get_skin_stats(gamd_handle* h, int64_t* n_rebuilds, int64_t* n_candidates, int64_t* candidate_capacity) {
    if (!h) return fail(-22, "null handle");
    if (n_rebuilds) *n_rebuilds = h->sticky_host[STICKY_REBUILDS];
    if (n_candidates) *n_candidates = h->sticky_host[STICKY_NCAND];
    if (candidate_capacity) *candidate_capacity = h->cand_cap;
    return 0;
}

int32_t gamd_debug_get(gamd_handle* h, int32_t what, void* host_out, size_t bytes) {
    if (!h || !host_out) return fail(-22, "null argument");
    DeviceGuard guard(h->dev);
    InitStream init(h->init_stream);
    HIP_TRY(hipDeviceSynchronize());
    const size_t n = (size_t)h->n;
    const size_t E = (size_t)std::min<long long>(h->counters_host[CNT_E], h->e_cap);
    const void* src = nullptr;
    size_t avail = 0;
    if (what == GAMD_DBG_PERM) { src = h->perm.p; avail = sizeof(int) * n; }
    else if (what == GAMD_DBG_ROWPTR) { src = h->row_ptr.p; avail = sizeof(int) * (n + 1); }
    else if (what == GAMD_DBG_COL) { src = h->col.p; avail = sizeof(int) * E; }
    else if (what == GAMD_DBG_EFRAG) {
        if (h->rt.ln_fold) return fail(-22, "EFRAG needs keep_stages=1 on this handle: the edge LayerNorm is folded into the conv layers and e is never formed");
        src = h->e_frag.p; avail = sizeof(float) * 4096 * (size_t)h->rt.EHT * ((E + 31) / 32);
    } else if (what == GAMD_DBG_FEAT) {
        if (!h->cfg.keep_stages) return fail(-22, "FEAT needs keep_stages=1");
        src = h->feat_dbg.p; avail = sizeof(float) * 48 * E;
    } else if (what >= GAMD_DBG_H0 && what <= GAMD_DBG_H0 + h->L) {
        if (!h->cfg.keep_stages) return fail(-22, "H_l needs keep_stages=1");
        src = h->hbuf.as<float>() + (size_t)(what - GAMD_DBG_H0) * n * (size_t)h->rt.H; avail = sizeof(float) * n * (size_t)h->rt.H;
    } else if (what == GAMD_DBG_PARTIAL) {
        src = h->partial.p; avail = sizeof(float) * (size_t)h->rt.H * (size_t)std::max(0, h->counters_host[CNT_PIECES]);
    } else if (what == GAMD_DBG_CYCLES) { src = h->tdbg.p; avail = sizeof(long long) * 16 * 8 * (size_t)h->n_cu;
    } else return fail(-22, "unknown debug tensor %d", what);
    if (bytes < avail) return fail(-22, "host buffer too small: %zu < %zu", bytes, avail);
    HIP_TRY(hipMemcpy(host_out, src, avail, hipMemcpyDeviceToHost));
    return 0;
}

int32_t gamd_md_run(gamd_handle* h, float* x_dev, float* v_dev, float* f_dev, const uint8_t* species_dev,
                    const float* box, const gamd_md_params* p, int64_t n_steps, void* stream) {
    int r;
    hipStream_t st = (hipStream_t)stream;
    RunScope scope;
    if ((r = begin_run(h, x_dev && v_dev && f_dev && box && p, n_steps, species_dev, box, p ? p->rigid_water : 0, st, scope))) return r;
    MdArgs m{};
    m.x = x_dev; m.v = v_dev; m.f = f_dev;
    if (!(p->mass_amu > 0.f)) return fail(-22, "mass_amu must be positive");
    m.inv_mass = 1.0f / p->mass_amu;
    m.inv_mass_h = p->mass_h_amu > 0.f ? 1.0f / p->mass_h_amu : 0.f;
    if ((r = fill_run_args(h, p, box, species_dev, st, &m))) return r;
    const double kB = 0.00831446261815324;                       // kJ/mol/K
    const double a = std::exp(-(double)p->gamma_per_ps * p->dt_ps);
    m.a = (float)a;
    m.b_len_kT = (float)(std::sqrt(1.0 - a * a) * (double)m.len * std::sqrt(kB * p->temperature_k));
    m.seed = p->seed;
    MdPending& pd = h->pending;
    pd.kind = 0; pd.m = m; pd.first_step = p->first_step;
    pd.mass = p->mass_amu; pd.mass_h = p->mass_h_amu > 0.f ? p->mass_h_amu : 0.f;
    return start_run(h, x_dev, f_dev, species_dev, box, n_steps, st);
}

int32_t gamd_md_force_source(gamd_handle* h, int32_t source) {
    if (!h) return fail(-22, "null handle");
    if (source != GAMD_FORCE_NETWORK && source != GAMD_FORCE_CLASSICAL && source != GAMD_FORCE_WATER_CLASSICAL)
        return fail(-22, "unknown force source %d (GAMD_FORCE_NETWORK = 0, GAMD_FORCE_CLASSICAL = 1, GAMD_FORCE_WATER_CLASSICAL = 2)", (int)source);
    if (h->pending.active) return fail(-22, "an MD run is still enqueued: call gamd_sync_status before gamd_md_force_source");
    if (source != GAMD_FORCE_NETWORK)
        if (int r = drive_check_source(h, source)) return r;
    h->force_source = source;
    return 0;
}

int32_t gamd_md_run_nhc(gamd_handle* h, float* x_dev, float* v_dev, float* f_dev, const uint8_t* species_dev,
                        const float* box, const gamd_nhc_params* p, double* chain_state_dev, int64_t n_steps, void* stream) {
    int r;
    hipStream_t st = (hipStream_t)stream;
    static const double YS1[] = {1.0};
    static const double YS3[] = {0.8289815435887510, -0.6579630871775020, 0.8289815435887510};
    static const double YS5[] = {0.2967324292201065, 0.2967324292201065, -0.1869297168804260, 0.2967324292201065,
                                 0.2967324292201065};                       // hack_integrator.py:183-187
    const double* ys = !p ? nullptr : p->num_yoshidasuzuki == 1 ? YS1 : p->num_yoshidasuzuki == 3 ? YS3 : p->num_yoshidasuzuki == 5 ? YS5 : nullptr;
    // the chain's own two refusals keep their places among the shared ones: behind the step count, behind the model's inputs
    const char* bad_chain = p && (p->chain_length < 1 || p->chain_length > 16) ? "chain_length must be in [1, 16]" : nullptr;
    const char* bad_ys = ys ? nullptr : "Invalid Yoshida-Suzuki value. Allowed values are: 1,3,5";
    RunScope scope;
    if ((r = begin_run(h, x_dev && v_dev && f_dev && box && p && chain_state_dev, n_steps, species_dev, box, p ? p->rigid_water : 0, st, scope,
                       bad_chain, bad_ys)))
        return r;
    NhcArgs a{};
    a.x = x_dev; a.v = v_dev; a.f = f_dev;
    if (!(p->mass_amu > 0.f)) return fail(-22, "mass_amu must be positive");
    a.mass = p->mass_amu; a.mass_h = p->mass_h_amu > 0.f ? p->mass_h_amu : 0.f;
    if ((r = fill_run_args(h, p, box, species_dev, st, &a))) return r;
    a.kT = 0.00831446261815324 * (double)p->temperature_k;
    a.freq = p->frequency_per_ps;
    a.ndf = p->ndf;
    a.M = p->chain_length; a.n_c = p->num_mts; a.n_ys = p->num_yoshidasuzuki;
    for (int i = 0; i < a.n_ys; ++i) a.w[i] = ys[i];
    a.state = chain_state_dev;
    a.n_blocks = std::min(256, (3 * h->n_per_box + 255) / 256);       // per box
    if (h->ke_partial.ensure(sizeof(double) * 256 * (size_t)h->n_boxes, true)) return fail(-12, "allocation failed");
    a.partial = h->ke_partial.as<double>();
    if (p->reset) {
        const size_t stride = 3 * (size_t)a.M + 2;
        std::vector<double> init(stride * (size_t)h->n_boxes, 0.0);
        for (int b = 0; b < h->n_boxes; ++b)
            for (int i = 0; i < a.M; ++i) init[stride * b + 2 * a.M + i] = -a.freq * a.freq;      // G_i = -frequency^2 (:255)
        HIP_TRY(hipMemcpyAsync(chain_state_dev, init.data(), sizeof(double) * init.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    MdPending& pd = h->pending;
    pd.kind = 1; pd.a = a; pd.first_step = 0;
    return start_run(h, x_dev, f_dev, species_dev, box, n_steps, st);
}

int32_t gamd_profile(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, const float* box,
                     float* out_norm_dev, void* stream, char* names, size_t names_bytes, float* ms, int32_t max_ms,
                     int32_t* n_out) {
    int r;
    if ((r = check_ready(h))) return r;
    if (!pos_dev || !box || !names || !ms || !n_out) return fail(-22, "null argument");
    if ((r = check_model_inputs(h, species_dev))) return r;
    DeviceGuard guard(h->dev);
    InitStream init((hipStream_t)stream);
    if ((r = set_box(h, box, (hipStream_t)stream))) return r;
    h->pending.active = false;
    hipStream_t st = (hipStream_t)stream;
    const int max_ev = 64;
    hipEvent_t evs[max_ev];
    for (int i = 0; i < max_ev; ++i) HIP_TRY(hipEventCreate(&evs[i]));
    const ForwardCall c{pos_dev, species_dev, out_norm_dev, nullptr, st};
    StageClock clock{h, st, evs};
    r = enqueue_forward(h, c, clock);
    if (r == 0) {
        HIP_TRY(hipStreamSynchronize(st));
        std::string all;
        int cnt = 0;
        for (int i = 1; i < clock.n_ev && cnt < max_ms; ++i, ++cnt) {
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, evs[i - 1], evs[i]));
            ms[cnt] = t;
            all += clock.labels[i];
            all += "\n";
        }
        *n_out = cnt;
        snprintf(names, names_bytes, "%s", all.c_str());
    }
    for (int i = 0; i < max_ev; ++i) (void)hipEventDestroy(evs[i]);
    return r;
}

int32_t gamd_timing_enable(gamd_handle* h, int32_t enable) {
    if (!h) return fail(-22, "null handle");
    DeviceGuard guard(h->dev);
    InitStream init(h->init_stream);
    h->timing = enable != 0;
    h->tev_used = 0;
    h->sev_used = 0;
    if (h->timing) {
        // a first pool of events HERE, not inside the region that is about to be timed (round-4 review: nothing but the
        // step's own launches belongs between the two synchronisation points); the pools still grow on demand
        while (h->tev.size() < 4096) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); h->tev.push_back(e); h->tev_kind.push_back(0); }
        while (h->sev.size() < 1024) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); h->sev.push_back(e); h->sev_closes.push_back(0); }
    }
    return 0;
}

int32_t gamd_timing_read_steps(gamd_handle* h, void* stream, float* step_ms, int64_t max_steps, int64_t* n_steps) {
    if (!h || !n_steps || (max_steps > 0 && !step_ms)) return fail(-22, "null argument");
    DeviceGuard guard(h->dev);
    InitStream init((hipStream_t)stream);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    // events: one in front of every step, one behind the last step of each enqueue_md_steps call.  The interval that starts
    // at such a closing event ends at the first event of the NEXT run: the host's gap between two gamd_md_run calls (or the
    // regrow of a run that froze on a neighbour-buffer overflow), not a step, and is skipped.  A frozen-and-resumed run
    // contributes its frozen steps (cheap: their kernels return at once) and the resumed ones.
    int64_t n = 0;
    for (size_t i = 0; i + 1 < h->sev_used; ++i) {
        if (h->sev_closes[i]) continue;
        if (n < max_steps) {
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, h->sev[i], h->sev[i + 1]));
            step_ms[n] = t;
        }
        ++n;
    }
    *n_steps = n;
    return 0;
}

int32_t gamd_timing_read(gamd_handle* h, void* stream, double* total_ms, int64_t* n_launches) {
    if (!h || !total_ms || !n_launches) return fail(-22, "null argument");
    double ms[3];
    int64_t cnt[3];
    int r = gamd_timing_read_stages(h, stream, ms, cnt);
    if (r) return r;
    *total_ms = ms[0];
    *n_launches = cnt[0];
    return 0;
}

int32_t gamd_timing_read_stages(gamd_handle* h, void* stream, double total_ms[3], int64_t n[3]) {
    if (!h || !total_ms || !n) return fail(-22, "null argument");
    DeviceGuard guard(h->dev);
    InitStream init((hipStream_t)stream);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (int k = 0; k < 3; ++k) { total_ms[k] = 0.0; n[k] = 0; }
    for (size_t i = 0; i + 1 < h->tev_used; i += 2) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, h->tev[i], h->tev[i + 1]));
        const int kind = h->tev_kind[i];
        const int slot = kind == 100 ? 1 : 0;
        total_ms[slot] += t;
        n[slot] += 1;
        // the node kernel between two conv layers of one force evaluation: stop of layer l -> start of layer l + 1
        if (kind != 100 && i + 3 < h->tev_used && h->tev_kind[i + 2] == kind + 1) {
            HIP_TRY(hipEventElapsedTime(&t, h->tev[i + 1], h->tev[i + 2]));
            total_ms[2] += t;
            n[2] += 1;
        }
    }
    return 0;
}

}  // extern "C"
