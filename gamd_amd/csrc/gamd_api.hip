// gamd_api.hip — the weight upload, the force evaluation, the MD driver and their extern "C" entry points of include/gamd_hip.h
// (the handle itself is in gamd_host.h, weight packing in gamd_weights_host.h; the run observers' entry points are in observe.hip).
#include "gamd_host.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>

static_assert(sizeof(gamd_config) == 96 && offsetof(gamd_config, n_boxes) == 88 && offsetof(gamd_config, edge_capacity) == 40,
              "gamd_config layout is part of the C ABI (gamd_amd/_lib.py mirrors it)");
static_assert(WH_FRAG_FLOATS == GAMD_WFRAG_FLOATS, "gamd_weights_host.h restates the size of a packed 128x128 weight");

namespace {

// batches never take the single-workgroup small-system path of neighbor.hip (k_step_small / k_filter_fill_small)
bool small_path(const gamd_handle* h) { return h->use_small; }

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
    r |= h->e_frag.ensure(sizeof(float) * 4096 * (size_t)h->EHT * (ec / GAMD_TILE + 1), false);
    if (h->ln_fold) r |= h->e_rstd.ensure(sizeof(float) * 64 * (ec / GAMD_TILE + 1), false);
    r |= h->partial.ensure(sizeof(float) * (size_t)h->H * (ec / GAMD_CHUNK + (size_t)h->n + 2), false);
    h->piece_cap = (long long)(ec / GAMD_CHUNK + (size_t)h->n + 2);
    if (h->update_edge) {                        // e_emb rows of one layer and the updated embedding tiles (H == Eh)
        r |= h->e_emb.ensure(sizeof(float) * (size_t)h->H * ec, false);
        r |= h->e_frag2.ensure(sizeof(float) * 4096 * (size_t)h->EHT * (ec / GAMD_TILE + 1), false);
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

// ---- the candidate radius of the Verlet-skin reuse, in fp32 ---------------------------------------------------------------
// Reuse rests on the triangle inequality: a pair that is an edge now (D1 <= rc) and whose atoms have each moved at most skin / 2
// since the build was at most rc + skin apart then (D0 <= D1 + 2 skin / 2), so it is in the candidate rows.  Every one of these
// four statements is decided by an fp32 predicate over wrapped coordinates, and each predicate sees the true minimum-image
// distance D only up to an ABSOLUTE error that scales with the box edge L, not with D.  With eps = 2^-24 (half an ulp, relative):
//   per component (gamd_min_image_wrapped on d = pc - pb, both in [0, L]):  d: eps L;  d + L/2: 1.5 eps L (|.| <= 1.5 L);
//     +/- L: eps L;  - L/2: 0.5 eps L   -> |r~ - r| <= 4 eps L   (a different image near +/- L/2 has the same |r| to that error)
//   vector:  | |r~| - D | <= sqrt(3) 4 eps L  < 7 eps L
//   squares and sums: three roundings per term, (1 + 3 eps) on d2, 1.5 eps D <= 1.3 eps L on the root (D <= sqrt(3) L / 2)
//   the threshold itself (rc2, skin_half2 rounded; the torch flavour's rounded sqrt):  <= eps D < 1 eps L
//   => each predicate decides "D~ < T" for some D~ with |D~ - D| <= E,  E = 10 eps L.
// Chain:  edge now => D1 <= rc + E;  not moved (twice) => each displacement <= skin / 2 + E;  so D0 <= rc + skin + 3 E, and the
// build's predicate sees D0~ <= rc + skin + 4 E.  The candidate radius must exceed that: rc + skin + 40 eps L, and 48 eps L once
// its own two roundings (rc_build, rc2_build) and a strict '<' are paid for.  L is the longest edge of any box of the handle
// (NbrArgs carries one radius for the whole batch).  At L = 30 / 150 / 1000 the margin is 8.6e-5 / 4.3e-4 / 2.9e-3: with
// rc + skin = 8.75 that is 1e-5 ... 3e-4 of the radius, 3e-5 ... 1e-3 of the candidates.  The exact filter and the move test are
// unchanged, so the edge set and the CSR order are what they were.  Without the margin a reuse step can miss an edge
// (tests/test_gpu_nbr_cutoff.py, profiles/nbr_cutoff_parity.md: 76-80 of 80 constructed pairs).
constexpr double GAMD_SKIN_MARGIN_EPS = 48.0 / 16777216.0;             // 48 x 2^-24, times the longest box edge
// The cell grid must hold the enlarged radius: a candidate pair is at most rc_build + E apart along every axis, and cell_coord
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

NbrArgs nbr_args(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev) {
    NbrArgs a{};
    a.n = h->n;
    a.flavour = h->cfg.nbr_flavour;
    for (int d = 0; d < 3; ++d) {
        a.box[d] = h->box[d];
        a.half[d] = 0.5f * h->box[d];
        a.nc[d] = h->nc[d];
    }
    a.rc = h->cfg.cutoff;
    a.rc2 = (float)((double)h->cfg.cutoff * (double)h->cfg.cutoff);   // graph_utils.py:59 cutoff ** 2
    a.ncell = h->ncell;
    a.bx = box_ref(h);
    a.box_shift = h->box_shift.as<int>();
    a.e_cap = h->e_cap;
    a.pos = pos_dev;
    a.species = species_dev;
    a.feat = h->feat_dev;
    a.self_loop = h->cfg.self_loop_mode == GAMD_SELF_LOOP_APPEND_ZERO_FEATURE ? 1 : 0;
    a.devflags = h->devflags.as<int>();
    a.pos_w = h->pos_w.as<float4>();
    a.pos_s = h->pos_s.as<float4>();
    a.cell_of = h->cell_of.as<int>();
    a.ncell_cap = h->ncell_cap;
    a.cell_cnt = h->counters.as<int>() + CNT_COUNT;
    a.cell_fill = h->counters.as<int>() + CNT_COUNT + h->ncell_cap;
    a.cell_start = h->cell_start.as<int>();
    a.perm = h->perm.as<int>();
    a.inv_perm = h->inv_perm.as<int>();
    a.deg = h->deg.as<int>();
    a.row_ptr = h->row_ptr.as<int>();
    a.na_excl = h->na_excl.as<int>();
    a.col = h->col.as<int>();
    a.erow = h->erow.as<int>();
    a.chunk_piece = h->chunk_piece.as<int>();
    a.chunk_mask = h->chunk_mask.as<unsigned>();
    a.counters = h->cur_counters ? h->cur_counters : h->counters.as<int>();
    a.sticky = h->sticky_dev;
    if (h->skin > 0.f) {
        a.skin_half2 = 0.25f * h->skin * h->skin;
        // rc + skin plus the rounding margin (GAMD_SKIN_MARGIN_EPS above): summed in double, rounded once
        a.rc_build = (float)((double)h->cfg.cutoff + (double)h->skin + GAMD_SKIN_MARGIN_EPS * (double)h->box_max);
        a.rc2_build = (float)((double)a.rc_build * (double)a.rc_build);
        a.cand_deg = h->cand_deg.as<int>();
        a.cand_ptr = h->cand_ptr.as<int>();
        a.cand_col = h->cand_col.as<int>();
        a.cand_cap = h->cand_cap;
        // fixed-width candidate rows (neighbor.hip): the width follows the capacity (alloc_candidates keeps cand_cap >= n, so
        // the width is at least 1: a buffer that is too small shows up as rows longer than the stride = the overflow -> regrow
        // protocol, not as a zero stride)
        a.use_small = small_path(h) ? 1 : 0;
        a.cand_stride = (int)std::max<long long>(1, std::min<long long>(h->cand_cap / h->n, 1 << 20));
    }
    return a;
}

struct EdgeList { const int* centre; const int* neigh; long long n; };

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

int enqueue_forward(gamd_handle* h, const float* pos_dev, const uint8_t* species_dev, float* out_norm_dev,
                    float* out_denorm_dev, hipStream_t st, hipEvent_t* evs, int* n_ev, std::vector<std::string>* labels,
                    const EdgeList* el = nullptr, const MdFuse* fuse = nullptr, bool copy_counters = true, bool l0_reuse = false,
                    bool drive = false) {
    auto mark = [&](const char* label) {
        if (evs) { (void)hipEventRecord(evs[*n_ev], st); ++*n_ev; labels->push_back(label); }
    };
    int r;
    mark("begin");
    // Verlet-skin reuse: ping-pong counter blocks instead of a memset node per call; n <= 1024: 4 neighbour launches per call
    // with the integrator halves folded in (neighbor.hip)
    const bool pingpong = !el && h->skin > 0.f;
    int* counters_next = nullptr;
    if (pingpong) {
        h->cnt_parity ^= 1;
        h->cur_counters = h->cnt2.as<int>() + h->cnt_parity * CNT_COUNT;
        counters_next = h->cnt2.as<int>() + (1 - h->cnt_parity) * CNT_COUNT;
    } else {
        h->cur_counters = h->counters.as<int>();
    }
    NbrArgs na = nbr_args(h, pos_dev, species_dev);
    na.counters_next = counters_next;
    if (el) {
        if ((r = launch_csr_from_edges(na, el->centre, el->neigh, el->n, h->tmp_eid.as<int>(), st)))
            return fail(-1, "edge-list CSR launch failed (%d)", r);
        h->cand_valid = false;                                    // atom order changed under the candidate list
    } else if (h->skin > 0.f) {
        na.ref_pos = h->ref_pos.as<float4>();
        na.force_rebuild = h->cand_valid ? 0 : 1;
        // rebuilds so far (host-mapped counter, lags the stream by what is enqueued) against calls so far: the one-workgroup
        // cell build costs ~70 us more per rebuild at 10^4 atoms and saves three gated launches (~14 us) on every other step
        ++h->skin_calls;
        na.cells_one_wg = (h->skin_calls < 32 || 6ll * h->sticky_host[STICKY_REBUILDS] < h->skin_calls) ? 1 : 0;
        if (fuse && !pingpong) return fail(-1, "internal: integrator halves can only be fused into the skin path");
        if ((r = launch_neighbor_skin(na, st, fuse))) return fail(-1, "neighbor (skin) launch failed (%d)", r);
        h->cand_valid = true;
    } else if ((r = launch_neighbor_build(na, st))) return fail(-1, "neighbor build launch failed (%d)", r);
    mark("neighbor_build");

    // classical force source (a step of an enqueued MD run, gamd_md_force_source): the neighbour stage above stays — the fused
    // integrator halves, the observers' edge list and pos_s, and the freeze / resume machinery hang on it — and the potential's
    // launches (two for Lennard-Jones, five for water) stand where encoder, conv layers and decoder would
    if (drive) {
        if ((r = drive_enqueue(h))) return r;
        if (copy_counters)
            HIP_TRY(hipMemcpyAsync(h->counters_host, h->cur_counters, sizeof(int) * CNT_COUNT, hipMemcpyDeviceToHost, st));
        return 0;
    }

    EncArgs ea{};
    ea.counters = h->cur_counters;
    ea.devflags = h->devflags.as<int>();
    ea.pos_s = h->pos_s.as<float4>();
    ea.col = h->col.as<int>();
    ea.erow = h->erow.as<int>();
    ea.bond_nbr = h->has_bonds ? h->bond_nbr.as<int>() : nullptr;
    ea.perm = h->perm.as<int>();
    ea.row_ptr = h->row_ptr.as<int>();
    ea.self_loop = na.self_loop;
    ea.zero_row = h->n;
    for (int d = 0; d < 3; ++d) { ea.box[d] = h->box[d]; ea.half[d] = 0.5f * h->box[d]; }
    ea.bx = box_ref(h);
    ea.length_mean = h->length_mean;
    ea.length_std = h->length_std;
    ea.gamma = (float)(1.0 / 0.025);             // RBFExpansion(high=1, gap=0.025): gamma = 1/gap (nn_module.py:240)
    ea.ln_inv_width = 1.0f / (float)h->Eh_true;
    ea.ln_n_pad = (float)(h->Eh - h->Eh_true);
    ea.n_feat = h->n_feat;
    ea.n_ksteps = (h->n_feat + 1) / 2;
    ea.centers = h->centers;
    ea.rbf = h->rbf;
    ea.w1p = h->enc_w1p; ea.w2p = h->enc_w2p; ea.w3p = h->enc_w3p;
    ea.b1 = h->enc_b1; ea.b2 = h->enc_b2; ea.b3 = h->enc_b3;
    ea.ln_g = h->enc_lng; ea.ln_b = h->enc_lnb;
    ea.e_format = !h->wide_enc ? 0 : h->cfg.edge_dtype == GAMD_EDGE_F16X3 ? 2 : h->cfg.edge_dtype == GAMD_EDGE_BF16 ? 1 : 0;
    ea.e_frag = h->e_frag.as<float>();
    ea.e_cap = h->e_cap;
    ea.sticky = h->sticky_dev;
    ea.feat_dbg = h->cfg.keep_stages ? h->feat_dbg.as<float>() : nullptr;
    ea.rstd_out = h->ln_fold ? h->e_rstd.as<float>() : nullptr;
    // fp32 path, few tiles (measured crossover ~500 tiles, half a tile per SIMD): the latency-oriented kernels, one tile
    // per 4-wave workgroup (conv_edge_small.hip, k_edge_encode_small).  They are bit-identical to the throughput kernels, so
    // the choice (from the last known edge count, or the density estimate before the first call) never shows in the results.
    int small_tiles = 0;
    if (h->cfg.edge_dtype == GAMD_EDGE_F32) {
        const long long e_est = el ? el->n + (na.self_loop ? h->n : 0)
                                   : (h->counters_host[CNT_E] > 0 ? (long long)h->counters_host[CNT_E] : (long long)((double)h->e_cap / 1.5));
        const long long tiles = (e_est + GAMD_TILE - 1) / GAMD_TILE;
        if (tiles <= h->small_tile_limit) small_tiles = (int)std::max<long long>(1, std::min<long long>(tiles + tiles / 8 + 1, 4096));
    }
    // Generic-width fp32 conv kernel on 16-edge work units (k_conv_edge_wide16, bit-identical to k_conv_edge_wide): opt-in through
    // GAMD_KSEL_FORCE_HALF_QUANTUM.  The idea — with t tiles per SIMD the launch takes ceil(2 t) / 2 tile quanta instead of ceil(t):
    // 1.5 instead of 2 at the DFT-water size — holds for the matrix time (61 against 82 us) but not for the launch: one wave per
    // SIMD pays the barrier, the 64 KiB weight copy and its vector work per 8 192-cycle phase instead of per 32 768-cycle phase
    // pair, ~2.7 us x 18 phases (110 us against 107, profiles/r06_experiments.md).  Not chosen automatically.
    const bool half_quantum = h->wide_conv && h->cfg.edge_dtype == GAMD_EDGE_F32 && (h->cfg.kernel_select & GAMD_KSEL_FORCE_HALF_QUANTUM) != 0;
    bool tev_full = false;
    auto tev_begin = [&](int kind) -> int {
        if (!h->timing) return 0;
        if (h->tev_used + 2 > h->tev.size()) {
            if (h->tev.size() >= 8 * gamd_handle::EVENT_POOL_CAP) { tev_full = true; return 0; }   // pool full: not timed any more
            for (int k = 0; k < 256; ++k) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); h->tev.push_back(e); h->tev_kind.push_back(0); }
        }
        h->tev_kind[h->tev_used] = kind;
        HIP_TRY(hipEventRecord(h->tev[h->tev_used], st));
        return 0;
    };
    auto tev_end = [&]() -> int {
        if (!h->timing || tev_full) return 0;
        HIP_TRY(hipEventRecord(h->tev[h->tev_used + 1], st));
        h->tev_used += 2;
        return 0;
    };
    if ((r = tev_begin(100))) return r;                         // kind 100: edge encoder
    r = h->DT > 1 ? launch_edge_encode_wide_d(ea, h->EHT, h->DT, h->n_cu, st)
        : h->wide_enc ? launch_edge_encode_wide(ea, h->EHT, h->n_cu, st)
        : h->cfg.edge_dtype == GAMD_EDGE_BF16 ? launch_edge_encode_bf16(ea, h->n_cu, st)
        : h->cfg.edge_dtype == GAMD_EDGE_F16X3 ? launch_edge_encode_f16x3(ea, h->n_cu, st)
        : small_tiles > 0 ? launch_edge_encode_small(ea, small_tiles, st) : launch_edge_encode(ea, h->n_cu, st);
    if (r) return fail(-1, "edge encode launch failed (%d)", r);
    if ((r = tev_end())) return r;
    mark("edge_encode");

    const size_t nh = (size_t)h->n * (size_t)h->H;
    auto node = [&](const NodeArgs& na_) {
        return h->DT > 1 ? launch_node_wide_d(na_, h->HT, h->DT, st) : h->wide_conv ? launch_node_wide(na_, h->HT, st) : launch_node(na_, st);
    };
    auto hptr = [&](int l) { return h->hbuf.as<float>() + (h->cfg.keep_stages ? (size_t)l * nh : (size_t)(l & 1) * nh); };

    NodeArgs no{};
#ifdef GAMD_PROFILING
    { static const bool node_time = getenv("GAMD_NODE_TIME") != nullptr; if (node_time) no.tdbg = h->tdbg.as<long long>(); }
#endif
    no.counters = h->cur_counters;
    no.devflags = h->devflags.as<int>();
    no.sticky = h->sticky_dev;
    no.n = h->n;
    no.pos_s = h->pos_s.as<float4>();
    no.node_emb = h->node_emb; no.enc_w = h->nenc_w; no.enc_b = h->nenc_b;
    no.row_ptr = h->row_ptr.as<int>(); no.na_excl = h->na_excl.as<int>(); no.deg = h->deg.as<int>();
    no.col = (h->l0_hoist && h->n_boxes > 1) ? h->col.as<int>() : nullptr;     // post(0) of the layer-0 form: box padding
    no.partial = h->partial.as<float>();
    no.piece_cap = h->piece_cap;
    no.P_in = h->P.as<float>();
    no.hn_perm = (!h->wide_conv && h->cfg.edge_dtype == GAMD_EDGE_F16X3) ? 1 : 0;
    no.tab16 = (!h->wide_conv && h->cfg.edge_dtype == GAMD_EDGE_BF16) ? 1 : 0;       // conv_edge_bf16.hip gathers fp16 rows
    no.hn_out = h->hn.as<float>(); no.S_out = h->S.as<float>(); no.D_out = h->D.as<float>(); no.P_out = h->P.as<float>();
    no.dec_w1p = h->dec_w1p; no.dec_b1 = h->dec_b1; no.dec_w2 = h->dec_w2; no.dec_b2 = h->dec_b2;
    no.ln_inv_width = 1.0f / (float)h->H_true;
    no.ln_n_pad = (float)(h->H - h->H_true);
    no.norm_bn = h->norm_bn;
    no.f16x3 = h->node_f16 ? 1 : 0;
    no.scale = (float)std::sqrt(h->scaler_var);
    no.shift = (float)h->scaler_mean;
    no.perm = h->perm.as<int>();
    no.forces_norm = out_norm_dev ? out_norm_dev : h->f_norm.as<float>();
    no.forces = out_denorm_dev;

    // layer 0 owns its tables in skin mode (see gamd_handle::l0_*); l0_reuse (steps of an enqueued MD run behind its first: same
    // species buffer, same weights): the launch returns at once unless this step rebuilt the candidate list
    const bool l0 = h->skin > 0.f && !el;
    float* const h0 = (l0 && !h->cfg.keep_stages) ? h->l0_h.as<float>() : hptr(0);
    no.mode = 0;
    no.pre = h->layers[0].node;
    no.h_out = h0;
    if (l0) { no.hn_out = h->l0_hn.as<float>(); no.S_out = h->l0_S.as<float>(); no.D_out = h->l0_D.as<float>(); no.P_out = h->l0_P.as<float>(); }
    no.l0_gate = (l0 && l0_reuse) ? 1 : 0;
    if ((r = node(no))) return fail(-1, "node(0) launch failed (%d)", r);
    no.l0_gate = 0;
    no.hn_out = h->hn.as<float>(); no.S_out = h->S.as<float>(); no.D_out = h->D.as<float>(); no.P_out = h->P.as<float>();
    mark("node_first");


    for (int l = 0; l < h->L; ++l) {
        ConvEdgeArgs ca{};
        ca.counters = h->cur_counters;
        ca.devflags = h->devflags.as<int>();
        ca.col = h->col.as<int>(); ca.erow = h->erow.as<int>();
        ca.chunk_piece = h->chunk_piece.as<int>(); ca.chunk_mask = h->chunk_mask.as<unsigned>();
        // update_edge_emb: layers after the first read the previous layer's LayerNorm(e_emb) (nn_module.py:145-146)
        ca.e_frag = (h->update_edge && l > 0) ? h->e_frag2.as<float>() : h->e_frag.as<float>();
        ca.emb_out = (h->update_edge && l + 1 < h->L) ? h->e_emb.as<float>() : nullptr;
        ca.hn = h->hn.as<float>(); ca.S = h->S.as<float>(); ca.D = h->D.as<float>();
        if (l0 && l == 0) { ca.hn = h->l0_hn.as<float>(); ca.S = h->l0_S.as<float>(); ca.D = h->l0_D.as<float>(); }
        const LayerDev& ld = h->layers[l];
        ca.w1p = ld.w1p; ca.w2p = ld.w2p; ca.w3p = ld.w3p; ca.w4p = ld.w4p; ca.w16p = ld.w16p;
        ca.b1 = ld.b1; ca.b3 = ld.b3; ca.b4 = ld.b4;
        // layer-0 form: three GEMMs per edge, phi_edge's part applied per atom by post(0) (timed as conv layer 0 all the same)
        const bool hoist = l == 0 && h->l0_hoist;
        if (hoist) { ca.w3p = ld.w3p_l0; ca.b3 = ld.b3_l0; }
        ca.e_rstd = h->ln_fold ? h->e_rstd.as<float>() : nullptr;
        ca.partial = h->partial.as<float>();
        ca.piece_cap = h->piece_cap;
        ca.sticky = h->sticky_dev;
        ca.e_cap = h->e_cap;
        ca.zero_row = h->n;
#ifdef GAMD_CHECKED
        // fault injection for tests/test_gpu_checked.py: the conv kernels are told that the node tables end at row 0, so the
        // first source index above it must be reported (GAMD_CHK_CONV_SRC) and clamped
        { static const bool inject = getenv("GAMD_CHK_INJECT") != nullptr; if (inject) ca.zero_row = 0; }
#endif
        ca.tdbg = h->tdbg.as<long long>();
        if ((r = tev_begin(l))) return r;                        // kind l: conv-layer edge kernel of layer l
        r = h->DT > 1 ? launch_conv_edge_wide_d(ca, h->EHT, h->HT, h->DT, h->n_cu, st)
            : h->wide_conv ? (h->cfg.edge_dtype == GAMD_EDGE_F16X3 ? launch_conv_edge_f16x3_wide(ca, h->EHT, h->HT, h->n_cu, st)
                            : h->cfg.edge_dtype == GAMD_EDGE_BF16 ? launch_conv_edge_bf16_wide(ca, h->EHT, h->HT, h->n_cu, st)
                            : (half_quantum && ca.w16p && !ca.emb_out) ? launch_conv_edge_wide16(ca, h->EHT, h->HT, h->n_cu, st)
                            : small_tiles > 0 ? launch_conv_edge_small_wide(ca, h->EHT, h->HT, small_tiles, st)
                                              : launch_conv_edge_wide(ca, h->EHT, h->HT, h->n_cu, st))
            : h->cfg.edge_dtype == GAMD_EDGE_BF16 ? launch_conv_edge_bf16(ca, h->n_cu, st)
            : h->cfg.edge_dtype == GAMD_EDGE_F16X3 ? launch_conv_edge_f16x3(ca, h->n_cu, st)
            : hoist ? (small_tiles > 0 ? launch_conv_edge_small_l0(ca, small_tiles, st) : launch_conv_edge_l0(ca, h->n_cu, st))
            : small_tiles > 0 ? launch_conv_edge_small(ca, small_tiles, st) : launch_conv_edge(ca, h->n_cu, st);
        if (r) return fail(-1, "conv edge launch failed (%d)", r);
        if ((r = tev_end())) return r;
        mark("conv_edge");
        if (ca.emb_out) {
            EdgeUpdateArgs ua{};
            ua.counters = h->cur_counters; ua.devflags = h->devflags.as<int>(); ua.e_cap = h->e_cap;
            ua.emb = ca.emb_out; ua.ln_g = ld.e_ln_g; ua.ln_b = ld.e_ln_b;
            ua.ln_inv_width = 1.0f / (float)h->Eh_true;
            ua.ln_n_pad = (float)(h->Eh - h->Eh_true);
            ua.e_frag_out = h->e_frag2.as<float>();
            if ((r = launch_edge_update(ua, h->HT, small_tiles > 0 ? std::max(1, small_tiles / 4) : 2 * h->n_cu, st)))
                return fail(-1, "edge update launch failed (%d)", r);
            mark("edge_update");
        }

        no.mode = (l == h->L - 1) ? 2 : 1;
        no.post = ld.node;
        if (l + 1 < h->L) no.pre = h->layers[l + 1].node;
        no.h_in = l == 0 ? h0 : hptr(l);
        no.P_in = (l0 && l == 0) ? h->l0_P.as<float>() : h->P.as<float>();
        no.h_out = hptr(l + 1);
        if ((r = node(no))) return fail(-1, "node launch failed (%d)", r);
        mark(no.mode == 2 ? "node_last_decode" : "node_mid");
    }
    // inside an enqueued MD run only the last step's counters are fetched (an overflow in any step reaches the host
    // through the mapped sticky flags): one copy node less per step
    if (copy_counters)
        HIP_TRY(hipMemcpyAsync(h->counters_host, h->cur_counters, sizeof(int) * CNT_COUNT, hipMemcpyDeviceToHost, st));
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

// steps [s_begin, n_steps) of the pending MD run; skip_first: the first half of step s_begin has already been done
int enqueue_md_steps(gamd_handle* h, long long s_begin, bool skip_first) {
    MdPending& p = h->pending;
    const bool drive = h->force_source != GAMD_FORCE_NETWORK;        // cannot change while the run is pending
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
            if ((r = enqueue_forward(h, p.x, p.species, nullptr, p.f, p.st, nullptr, nullptr, nullptr, nullptr, &fuse,
                                     s + 1 == p.n_steps, s > s_begin, drive)))
                return r;
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
        const bool first = !(skip_first && s == s_begin);
        const bool last = s + 1 == p.n_steps;
        if (p.kind == 0) {
            p.m.step = p.first_step + (unsigned long long)s;
            p.m.step_index = (int)s;
            if (first && (r = launch_baoab_first(p.m, p.st))) return fail(-1, "integrator launch failed (%d)", r);
            if ((r = enqueue_forward(h, p.x, p.species, nullptr, p.f, p.st, nullptr, nullptr, nullptr, nullptr, nullptr, last, s > s_begin, drive))) return r;
            if ((r = launch_baoab_second(p.m, p.st))) return fail(-1, "integrator launch failed (%d)", r);
        } else {
            p.a.step_index = (int)s;
            if (first && (r = launch_nhc_first(p.a, p.st))) return fail(-1, "integrator launch failed (%d)", r);
            if ((r = enqueue_forward(h, p.x, p.species, nullptr, p.f, p.st, nullptr, nullptr, nullptr, nullptr, nullptr, last, s > s_begin, drive))) return r;
            if ((r = launch_nhc_second(p.a, p.st))) return fail(-1, "integrator launch failed (%d)", r);
        }
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
    // Widths as build_model hands them to the model constructors (nn_module.py:561-601, :410-460, :266-320).  The kernels work
    // in 128-wide blocks: narrower (or in-between) widths are zero-padded by gamd_finalize_weights — padded features stay
    // exact zeros through every Linear / SiLU / GELU, and the two LayerNorms divide by the true width.
    const int H_true = cfg->encoding_size ? cfg->encoding_size : 128, Eh_true = cfg->edge_embedding_dim ? cfg->edge_embedding_dim : 128;
    const int D_true = cfg->hidden_dim ? cfg->hidden_dim : 128;
    if (H_true < 1 || H_true > 256 || Eh_true < 1 || Eh_true > 256)
        return fail(-22, "encoding_size and edge_embedding_dim must be in [1, 256] (got %d, %d)", H_true, Eh_true);
    if (D_true < 1 || D_true > 256) return fail(-22, "hidden_dim must be in [1, 256] (got %d)", D_true);
    const int Dp = D_true <= 128 ? 128 : 256;
    // hidden_dim above 128: two 128-blocks per D-wide operand, the fp32 kernels of wide_d.hip
    if (Dp > 128 && cfg->edge_dtype != GAMD_EDGE_F32)
        return fail(-22, "hidden_dim above 128 is built for edge_dtype f32 only (got hidden_dim %d)", D_true);
    const int H = H_true <= 128 ? 128 : 256, Eh = Eh_true <= 128 ? 128 : 256;
    const bool exact128 = H_true == 128 && Eh_true == 128 && D_true == 128;
    const bool generic = H != 128 || Eh != 128 || cfg->no_expand_edge;
    // reduced-precision edge MLPs (bf16, fp32-grade split-fp16) exist for every width and both feature sets: 128 / 128 / 128
    // expanded runs the specialised kernels, anything else wide.hip's encoder writing the operands + wide_lp.hip
    if (cfg->edge_dtype != GAMD_EDGE_F32 && H == 256 && (long long)cfg->n_atoms * n_boxes > (1ll << 22) - 2)
        return fail(-22, "bf16 / split-fp16 with encoding_size > 128: at most 2^22 - 2 atoms per handle (32-bit byte offsets into hn)");
    gamd_handle* h = new gamd_handle();
    h->obs = observers_new();
    h->cfg = *cfg;
    h->dev = cfg->device;
    if (hipStreamCreateWithFlags(&h->init_stream, hipStreamNonBlocking) != hipSuccess) {
        h->init_stream = nullptr;
        gamd_destroy(h);
        return fail(-12, "stream creation failed");
    }
    InitStream init(h->init_stream);
    h->n_boxes = n_boxes;
    h->n_per_box = cfg->n_atoms;
    h->n = cfg->n_atoms * n_boxes;
    h->L = cfg->n_layers;
    h->H = H; h->Eh = Eh; h->HT = H / 128; h->EHT = Eh / 128;
    h->H_true = H_true; h->Eh_true = Eh_true; h->D_true = D_true;
    h->Dp = Dp; h->DT = Dp / 128;
    h->skin = cfg->neighbor_skin;
    if (cfg->small_tile_limit != 0) h->small_tile_limit = cfg->small_tile_limit < 0 ? -1 : cfg->small_tile_limit;
    const bool forced = (cfg->kernel_select & GAMD_KSEL_FORCE_GENERIC_WIDTH) && cfg->edge_dtype == GAMD_EDGE_F32;
    // bf16 / split-fp16 outside 128 / 128 / 128 expanded: encoder, conv and node kernels all take the generic-width route
    const bool lp_generic = cfg->edge_dtype != GAMD_EDGE_F32 && (generic || !exact128);
    h->wide_enc = generic || forced || lp_generic || Dp > 128;
    h->wide_conv = H != 128 || Eh != 128 || forced || lp_generic || Dp > 128;
    // Folded edge LayerNorm (gamd_ln_fold_host.h): the fp32 128-wide kernels without appended self loops; not with keep_stages
    // (e is then a stage the getters hand out), not under GAMD_KSEL_NO_LN_FOLD, not for update_edge_emb models (which
    // gamd_finalize_weights moves to the generic-width kernels)
    h->ln_fold = cfg->edge_dtype == GAMD_EDGE_F32 && !h->wide_enc && !h->wide_conv && cfg->self_loop_mode == GAMD_SELF_LOOP_DGL07_NOOP &&
                 !cfg->keep_stages && !(cfg->kernel_select & GAMD_KSEL_NO_LN_FOLD);
    h->n_feat = (cfg->no_expand_edge ? 4 : 44) + (cfg->use_bond ? 1 : 0);
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
    const size_t nh = n * (size_t)H * sizeof(float), nd = n * (size_t)Dp * sizeof(float), zd = (size_t)Dp * sizeof(float);
    r |= h->hbuf.ensure(nh * (cfg->keep_stages ? (size_t)h->L + 1 : 2), true);
    // one extra, all-zero row (index n) behind the node tables the conv-layer edge kernel gathers from: the padding
    // slots of the last 32-edge tile point at it, so their messages are exact zeros without a per-element mask
    r |= h->hn.ensure(nh + (size_t)H * sizeof(float), true);
    r |= h->S.ensure(nd + zd, true);
    r |= h->D.ensure(nd + zd, true);
    r |= h->P.ensure(nd, true);
    if (cfg->neighbor_skin > 0.f) {
        r |= h->l0_hn.ensure(nh + (size_t)H * sizeof(float), true);
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
    if (r) { gamd_destroy(h); return fail(-12, "device allocation failed"); }
    {
        const int no_atom = -2;
        if (init_upload(h->perm.as<int>() + n, &no_atom, sizeof(int)) != hipSuccess) {
            gamd_destroy(h);
            return fail(-1, "device copy failed");
        }
    }
    if ((r = clear_devflags(h))) { gamd_destroy(h); return r; }
    if (hipHostMalloc((void**)&h->counters_host, sizeof(int) * CNT_COUNT) != hipSuccess) {
        gamd_destroy(h);
        return fail(-12, "pinned allocation failed");
    }
    memset(h->counters_host, 0, sizeof(int) * CNT_COUNT);
    if (hipHostMalloc((void**)&h->sticky_host, sizeof(int) * STICKY_COUNT, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void**)&h->sticky_dev, h->sticky_host, 0) != hipSuccess) {
        gamd_destroy(h);
        return fail(-12, "mapped host allocation failed");
    }
    memset(h->sticky_host, 0, sizeof(int) * STICKY_COUNT);
    if (h->skin > 0.f) {
        int rr = 0;
        rr |= h->ref_pos.ensure(sizeof(float4) * n, true);
        rr |= h->cand_deg.ensure(sizeof(int) * n, true);
        rr |= h->cand_ptr.ensure(sizeof(int) * (n + 1), true);
        if (rr) { gamd_destroy(h); return fail(-12, "device allocation failed"); }
    }
    {
        std::vector<float> all((size_t)n_boxes * 3);              // every box starts with the constructor's box
        for (int b = 0; b < n_boxes; ++b)
            for (int d = 0; d < 3; ++d) all[(size_t)3 * b + d] = cfg->box[d];
        if ((r = set_box(h, all.data()))) { gamd_destroy(h); return r; }
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
    if ((r = alloc_edges(h, ecap))) { gamd_destroy(h); return r; }
    if (hipStreamSynchronize(h->init_stream) != hipSuccess) { gamd_destroy(h); return fail(-1, "device synchronisation failed"); }
    *out = h;                                  // every initialising memset / copy has landed: any stream may use the handle
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
                      &h->cell_cnt, &h->cell_fill, &h->cell_start, &h->col, &h->erow, &h->chunk_piece,
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

// Transformation and packing are pack_weights (gamd_weights_host.h, host only); here: its flags onto the handle, the upload,
// and its offset tables turned into the device pointers of the same names.
int32_t gamd_finalize_weights(gamd_handle* h) {
    if (!h) return fail(-22, "null handle");
    DeviceGuard guard(h->dev);
    InitStream init(h->init_stream);
    WeightSpec spec;
    spec.kind = h->cfg.kind; spec.edge_dtype = h->cfg.edge_dtype; spec.no_expand_edge = h->cfg.no_expand_edge;
    spec.self_loop_mode = h->cfg.self_loop_mode; spec.kernel_select = h->cfg.kernel_select;
    spec.n_layers = h->L; spec.n_feat = h->n_feat;
    spec.H_true = h->H_true; spec.Eh_true = h->Eh_true; spec.D_true = h->D_true;
    spec.H = h->H; spec.Eh = h->Eh; spec.Dp = h->Dp;
    spec.wide_enc = h->wide_enc; spec.wide_conv = h->wide_conv; spec.ln_fold = h->ln_fold;
    const PackedWeights pw = pack_weights(spec, h->host_w);
    if (pw.err) return fail(pw.err, "%s", pw.msg);
    h->node_f16 = pw.node_f16;
    h->wide_enc = pw.wide_enc; h->wide_conv = pw.wide_conv; h->ln_fold = pw.ln_fold;
    if (pw.update_edge != h->update_edge) {                      // e_emb / e_frag2 come and go with it
        h->update_edge = pw.update_edge;
        if (alloc_edges(h, h->e_cap)) return -12;
    }
    h->norm_bn = pw.norm_bn ? 1 : 0;
    h->l0_hoist = pw.l0_hoist;
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
    return enqueue_forward(h, pos_dev, species_dev, out_norm_dev, out_denorm_dev, (hipStream_t)stream, nullptr, nullptr, nullptr);
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
    EdgeList el{centre_dev, neigh_dev, (long long)n_edges};
    if ((r = enqueue_forward(h, pos_dev, species_dev, out_norm_dev, out_denorm_dev, (hipStream_t)stream, nullptr, nullptr,
                             nullptr, &el)))
        return r;
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
        if (h->ln_fold) return fail(-22, "EFRAG needs keep_stages=1 on this handle: the edge LayerNorm is folded into the conv layers and e is never formed");
        src = h->e_frag.p; avail = sizeof(float) * 4096 * (size_t)h->EHT * ((E + 31) / 32);
    } else if (what == GAMD_DBG_FEAT) {
        if (!h->cfg.keep_stages) return fail(-22, "FEAT needs keep_stages=1");
        src = h->feat_dbg.p; avail = sizeof(float) * 48 * E;
    } else if (what >= GAMD_DBG_H0 && what <= GAMD_DBG_H0 + h->L) {
        if (!h->cfg.keep_stages) return fail(-22, "H_l needs keep_stages=1");
        src = h->hbuf.as<float>() + (size_t)(what - GAMD_DBG_H0) * n * (size_t)h->H; avail = sizeof(float) * n * (size_t)h->H;
    } else if (what == GAMD_DBG_PARTIAL) {
        src = h->partial.p; avail = sizeof(float) * (size_t)h->H * (size_t)std::max(0, h->counters_host[CNT_PIECES]);
    } else if (what == GAMD_DBG_CYCLES) { src = h->tdbg.p; avail = sizeof(long long) * 16 * 8 * (size_t)h->n_cu;
    } else return fail(-22, "unknown debug tensor %d", what);
    if (bytes < avail) return fail(-22, "host buffer too small: %zu < %zu", bytes, avail);
    HIP_TRY(hipMemcpy(host_out, src, avail, hipMemcpyDeviceToHost));
    return 0;
}

int32_t gamd_md_run(gamd_handle* h, float* x_dev, float* v_dev, float* f_dev, const uint8_t* species_dev,
                    const float* box, const gamd_md_params* p, int64_t n_steps, void* stream) {
    int r;
    if ((r = check_ready(h))) return r;
    if (!x_dev || !v_dev || !f_dev || !box || !p) return fail(-22, "null argument");
    if (n_steps < 0 || n_steps > 0x3fffffff) return fail(-22, "n_steps out of range");
    if ((r = check_model_inputs(h, species_dev))) return r;
    if ((r = observers_check_run(h, box, species_dev))) return r;
    if (h->force_source == GAMD_FORCE_WATER_CLASSICAL && !p->rigid_water)
        return fail(-22, "the water classical force source needs rigid_water: the potential has no bond or angle term (same-molecule "
                         "pairs are excluded), so only the constraints hold a molecule together");
    if (h->force_source != GAMD_FORCE_NETWORK && (r = drive_check_run(h, box, species_dev))) return r;
    DeviceGuard guard(h->dev);
    InitStream init((hipStream_t)stream);
    if ((r = set_box(h, box, (hipStream_t)stream))) return r;
    hipStream_t st = (hipStream_t)stream;
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
    if ((r = check_ready(h))) return r;
    if (!x_dev || !v_dev || !f_dev || !box || !p || !chain_state_dev) return fail(-22, "null argument");
    if (n_steps < 0 || n_steps > 0x3fffffff) return fail(-22, "n_steps out of range");
    if (p->chain_length < 1 || p->chain_length > 16) return fail(-22, "chain_length must be in [1, 16]");
    if ((r = check_model_inputs(h, species_dev))) return r;
    static const double YS1[] = {1.0};
    static const double YS3[] = {0.8289815435887510, -0.6579630871775020, 0.8289815435887510};
    static const double YS5[] = {0.2967324292201065, 0.2967324292201065, -0.1869297168804260, 0.2967324292201065,
                                 0.2967324292201065};                       // hack_integrator.py:183-187
    const double* ys = p->num_yoshidasuzuki == 1 ? YS1 : p->num_yoshidasuzuki == 3 ? YS3 : p->num_yoshidasuzuki == 5 ? YS5 : nullptr;
    if (!ys) return fail(-22, "Invalid Yoshida-Suzuki value. Allowed values are: 1,3,5");
    if ((r = observers_check_run(h, box, species_dev))) return r;
    if (h->force_source == GAMD_FORCE_WATER_CLASSICAL && !p->rigid_water)
        return fail(-22, "the water classical force source needs rigid_water: the potential has no bond or angle term (same-molecule "
                         "pairs are excluded), so only the constraints hold a molecule together");
    if (h->force_source != GAMD_FORCE_NETWORK && (r = drive_check_run(h, box, species_dev))) return r;
    DeviceGuard guard(h->dev);
    InitStream init((hipStream_t)stream);
    if ((r = set_box(h, box, (hipStream_t)stream))) return r;
    hipStream_t st = (hipStream_t)stream;
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
    int n_ev = 0;
    std::vector<std::string> labels;
    r = enqueue_forward(h, pos_dev, species_dev, out_norm_dev, nullptr, st, evs, &n_ev, &labels);
    if (r == 0) {
        HIP_TRY(hipStreamSynchronize(st));
        std::string all;
        int cnt = 0;
        for (int i = 1; i < n_ev && cnt < max_ms; ++i, ++cnt) {
            float t = 0.f;
            HIP_TRY(hipEventElapsedTime(&t, evs[i - 1], evs[i]));
            ms[cnt] = t;
            all += labels[i];
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
