// forward.hip — one force evaluation enqueued on a stream, as stages: the neighbour stage, then the network (edge encoder, node(0),
// per layer conv edge / edge update / node) or, in a step of an enqueued MD run under gamd_md_force_source, the classical potential.
// Which kernel each stage launches is the handle's route (gamd_route_host.h), looked up in the launcher tables below.
#include "gamd_host.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

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
        a.use_small = h->use_small ? 1 : 0;      // batches never take the single-workgroup small-system path of neighbor.hip
        a.cand_stride = (int)std::max<long long>(1, std::min<long long>(h->cand_cap / h->n, 1 << 20));
    }
    return a;
}

namespace {

// ---- the neighbour stage: the counter block of this call, then one of three paths ---------------------------------------------
int neighbour_stage(gamd_handle* h, const ForwardCall& c) {
    int r;
    // Verlet-skin reuse: ping-pong counter blocks instead of a memset node per call; n <= 1024: 4 neighbour launches per call
    // with the integrator halves folded in (neighbor.hip)
    const bool skin = !c.edges && h->skin > 0.f;
    int* counters_next = nullptr;
    if (skin) {
        h->cnt_parity ^= 1;
        h->cur_counters = h->cnt2.as<int>() + h->cnt_parity * CNT_COUNT;
        counters_next = h->cnt2.as<int>() + (1 - h->cnt_parity) * CNT_COUNT;
    } else {
        h->cur_counters = h->counters.as<int>();
    }
    NbrArgs na = nbr_args(h, c.pos, c.species);
    na.counters_next = counters_next;
    if (c.edges) {                                                // the CSR of a caller's edge list
        if ((r = launch_csr_from_edges(na, c.edges->centre, c.edges->neigh, c.edges->n, h->tmp_eid.as<int>(), c.st)))
            return fail(-1, "edge-list CSR launch failed (%d)", r);
        h->cand_valid = false;                                    // atom order changed under the candidate list
    } else if (skin) {                                            // check, gated candidate rebuild, exact filter
        na.ref_pos = h->ref_pos.as<float4>();
        na.force_rebuild = h->cand_valid ? 0 : 1;
        // rebuilds so far (host-mapped counter, lags the stream by what is enqueued) against calls so far: the one-workgroup
        // cell build costs ~70 us more per rebuild at 10^4 atoms and saves three gated launches (~14 us) on every other step
        ++h->skin_calls;
        na.cells_one_wg = (h->skin_calls < 32 || 6ll * h->sticky_host[STICKY_REBUILDS] < h->skin_calls) ? 1 : 0;
        if ((r = launch_neighbor_skin(na, c.st, c.fuse))) return fail(-1, "neighbor (skin) launch failed (%d)", r);
        h->cand_valid = true;
    } else if ((r = launch_neighbor_build(na, c.st))) {           // the exact build
        return fail(-1, "neighbor build launch failed (%d)", r);
    }
    return 0;
}

// ---- argument blocks: built per call (alloc_edges moves the buffers they point at) -------------------------------------------
EncArgs enc_args(const gamd_handle* h) {
    const Route& rt = h->rt;
    EncArgs ea{};
    ea.counters = h->cur_counters;
    ea.devflags = h->devflags.as<int>();
    ea.pos_s = h->pos_s.as<float4>();
    ea.col = h->col.as<int>();
    ea.erow = h->erow.as<int>();
    ea.bond_nbr = h->has_bonds ? h->bond_nbr.as<int>() : nullptr;
    ea.perm = h->perm.as<int>();
    ea.row_ptr = h->row_ptr.as<int>();
    ea.self_loop = h->cfg.self_loop_mode == GAMD_SELF_LOOP_APPEND_ZERO_FEATURE ? 1 : 0;
    ea.zero_row = h->n;
    for (int d = 0; d < 3; ++d) { ea.box[d] = h->box[d]; ea.half[d] = 0.5f * h->box[d]; }
    ea.bx = box_ref(h);
    ea.length_mean = h->length_mean;
    ea.length_std = h->length_std;
    ea.gamma = (float)(1.0 / 0.025);             // RBFExpansion(high=1, gap=0.025): gamma = 1/gap (nn_module.py:240)
    ea.ln_inv_width = 1.0f / (float)rt.Eh_true;
    ea.ln_n_pad = (float)(rt.Eh - rt.Eh_true);
    ea.n_feat = rt.n_feat;
    ea.n_ksteps = (rt.n_feat + 1) / 2;
    ea.centers = h->centers;
    ea.rbf = h->rbf;
    ea.w1p = h->enc_w1p; ea.w2p = h->enc_w2p; ea.w3p = h->enc_w3p;
    ea.b1 = h->enc_b1; ea.b2 = h->enc_b2; ea.b3 = h->enc_b3;
    ea.ln_g = h->enc_lng; ea.ln_b = h->enc_lnb;
    ea.e_format = rt.e_format;
    ea.e_frag = h->e_frag.as<float>();
    ea.e_cap = h->e_cap;
    ea.sticky = h->sticky_dev;
    ea.feat_dbg = h->cfg.keep_stages ? h->feat_dbg.as<float>() : nullptr;
    ea.rstd_out = rt.ln_fold ? h->e_rstd.as<float>() : nullptr;
    return ea;
}

// everything the node launches of one call share; mode, the layers' weights, h_in / h_out / P_in and layer 0's tables are set per launch
NodeArgs node_args(const gamd_handle* h, const ForwardCall& c) {
    const Route& rt = h->rt;
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
    no.col = (rt.l0_hoist && h->n_boxes > 1) ? h->col.as<int>() : nullptr;     // post(0) of the layer-0 form: box padding
    no.partial = h->partial.as<float>();
    no.piece_cap = h->piece_cap;
    no.P_in = h->P.as<float>();
    no.hn_perm = rt.hn_perm;
    no.tab16 = rt.tab16;
    no.hn_out = h->hn.as<float>(); no.S_out = h->S.as<float>(); no.D_out = h->D.as<float>(); no.P_out = h->P.as<float>();
    no.dec_w1p = h->dec_w1p; no.dec_b1 = h->dec_b1; no.dec_w2 = h->dec_w2; no.dec_b2 = h->dec_b2;
    no.ln_inv_width = 1.0f / (float)rt.H_true;
    no.ln_n_pad = (float)(rt.H - rt.H_true);
    no.norm_bn = h->norm_bn;
    no.f16x3 = rt.node_f16 ? 1 : 0;
    no.scale = (float)std::sqrt(h->scaler_var);
    no.shift = (float)h->scaler_mean;
    no.perm = h->perm.as<int>();
    no.forces_norm = c.out_norm ? c.out_norm : h->f_norm.as<float>();
    no.forces = c.out_denorm;
    return no;
}

// layer `layer`'s edge kernel; l0: layer 0 reads its own node tables (skin mode, see gamd_handle::l0_*)
ConvEdgeArgs conv_args(const gamd_handle* h, int layer, bool l0) {
    const Route& rt = h->rt;
    const LayerDev& ld = h->layers[layer];
    ConvEdgeArgs ca{};
    ca.counters = h->cur_counters;
    ca.devflags = h->devflags.as<int>();
    ca.col = h->col.as<int>(); ca.erow = h->erow.as<int>();
    ca.chunk_piece = h->chunk_piece.as<int>(); ca.chunk_mask = h->chunk_mask.as<unsigned>();
    // update_edge_emb: layers after the first read the previous layer's LayerNorm(e_emb) (nn_module.py:145-146)
    ca.e_frag = (rt.update_edge && layer > 0) ? h->e_frag2.as<float>() : h->e_frag.as<float>();
    ca.emb_out = (rt.update_edge && layer + 1 < h->L) ? h->e_emb.as<float>() : nullptr;
    ca.hn = h->hn.as<float>(); ca.S = h->S.as<float>(); ca.D = h->D.as<float>();
    if (l0 && layer == 0) { ca.hn = h->l0_hn.as<float>(); ca.S = h->l0_S.as<float>(); ca.D = h->l0_D.as<float>(); }
    ca.w1p = ld.w1p; ca.w2p = ld.w2p; ca.w3p = ld.w3p; ca.w4p = ld.w4p; ca.w16p = ld.w16p;
    ca.b1 = ld.b1; ca.b3 = ld.b3; ca.b4 = ld.b4;
    // layer-0 form: three GEMMs per edge, phi_edge's part applied per atom by post(0) (timed as conv layer 0 all the same)
    if (layer == 0 && rt.l0_hoist) { ca.w3p = ld.w3p_l0; ca.b3 = ld.b3_l0; }
    ca.e_rstd = rt.ln_fold ? h->e_rstd.as<float>() : nullptr;
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
    return ca;
}

EdgeUpdateArgs edge_update_args(const gamd_handle* h, int layer) {
    EdgeUpdateArgs ua{};
    ua.counters = h->cur_counters; ua.devflags = h->devflags.as<int>(); ua.e_cap = h->e_cap;
    ua.emb = h->e_emb.as<float>(); ua.ln_g = h->layers[layer].e_ln_g; ua.ln_b = h->layers[layer].e_ln_b;
    ua.ln_inv_width = 1.0f / (float)h->rt.Eh_true;
    ua.ln_n_pad = (float)(h->rt.Eh - h->rt.Eh_true);
    ua.e_frag_out = h->e_frag2.as<float>();
    return ua;
}

// ---- the route's enumerators to their launchers (the rows of gamd_route_host.h), one signature per stage -------------------
template <class Args> struct StageRow {
    using Launch = int (*)(const Args&, const Route&, int n_blocks, hipStream_t);
    Launch throughput, small;                  // small null: the family has one regime
};
#define ROUTE_ARGS_NB(fn) [](const auto& a, const Route&, int nb, hipStream_t st) { return fn(a, nb, st); }
#define ROUTE_ARGS_ENC_WIDE(fn) [](const auto& a, const Route& r, int nb, hipStream_t st) { return fn(a, r.EHT, nb, st); }
#define ROUTE_ARGS_ENC_WIDE_D(fn) [](const auto& a, const Route& r, int nb, hipStream_t st) { return fn(a, r.EHT, r.DT, nb, st); }
#define ROUTE_ARGS_CONV_WIDE(fn) [](const auto& a, const Route& r, int nb, hipStream_t st) { return fn(a, r.EHT, r.HT, nb, st); }
#define ROUTE_ARGS_CONV_WIDE_D(fn) [](const auto& a, const Route& r, int nb, hipStream_t st) { return fn(a, r.EHT, r.HT, r.DT, nb, st); }
#define ROUTE_ARGS_NODE(fn) [](const auto& a, const Route&, int, hipStream_t st) { return fn(a, st); }
#define ROUTE_ARGS_NODE_WIDE(fn) [](const auto& a, const Route& r, int, hipStream_t st) { return fn(a, r.HT, st); }
#define ROUTE_ARGS_NODE_WIDE_D(fn) [](const auto& a, const Route& r, int, hipStream_t st) { return fn(a, r.HT, r.DT, st); }
#define ROUTE_ROW1(e, args, fn, kernel) {ROUTE_ARGS_##args(launch_##fn), nullptr},
#define ROUTE_ROW2(e, args, fn, kernel, fn_small, kernel_small) {ROUTE_ARGS_##args(launch_##fn), ROUTE_ARGS_##args(launch_##fn_small)},
const StageRow<EncArgs> ENC_ROWS[ENC_KERNELS] = {GAMD_ENC_ROUTES(ROUTE_ROW1, ROUTE_ROW2)};
const StageRow<ConvEdgeArgs> CONV_ROWS[CONV_KERNELS] = {GAMD_CONV_ROUTES(ROUTE_ROW1, ROUTE_ROW2)};
const StageRow<NodeArgs> NODE_ROWS[NODE_KERNELS] = {GAMD_NODE_ROUTES(ROUTE_ROW1)};
#undef ROUTE_ROW1
#undef ROUTE_ROW2

// small_tiles > 0 and a small-tile kernel in the row: that many workgroups of it; else the throughput kernel on every CU
template <class Args> int launch_row(const StageRow<Args>& row, const Args& a, const gamd_handle* h, int small_tiles, hipStream_t st) {
    return small_tiles > 0 && row.small ? row.small(a, h->rt, small_tiles, st) : row.throughput(a, h->rt, h->n_cu, st);
}

// ---- the network: edge encoder, node(0), then per layer conv edge, (update_edge) edge update, node ---------------------------
int network_stage(gamd_handle* h, const ForwardCall& c, StageClock& clock) {
    const Route& rt = h->rt;
    int r;
    const long long e_est = c.edges ? c.edges->n + (h->cfg.self_loop_mode == GAMD_SELF_LOOP_APPEND_ZERO_FEATURE ? h->n : 0)
                            : h->counters_host[CNT_E] > 0 ? (long long)h->counters_host[CNT_E] : (long long)((double)h->e_cap / 1.5);
    const int small_tiles = route_small_tiles(rt, e_est, h->small_tile_limit);

    if ((r = clock.begin(100))) return r;
    if ((r = launch_row(ENC_ROWS[rt.enc], enc_args(h), h, small_tiles, c.st))) return fail(-1, "edge encode launch failed (%d)", r);
    if ((r = clock.end())) return r;
    clock.mark("edge_encode");

    const size_t nh = (size_t)h->n * (size_t)rt.H;
    auto hptr = [&](int l) { return h->hbuf.as<float>() + (h->cfg.keep_stages ? (size_t)l * nh : (size_t)(l & 1) * nh); };
    // layer 0 owns its tables in skin mode (see gamd_handle::l0_*); l0_reuse (steps of an enqueued MD run behind its first: same
    // species buffer, same weights): the launch returns at once unless this step rebuilt the candidate list
    const bool l0 = h->skin > 0.f && !c.edges;
    float* const h0 = (l0 && !h->cfg.keep_stages) ? h->l0_h.as<float>() : hptr(0);
    NodeArgs no = node_args(h, c);
    no.mode = 0;
    no.pre = h->layers[0].node;
    no.h_out = h0;
    if (l0) { no.hn_out = h->l0_hn.as<float>(); no.S_out = h->l0_S.as<float>(); no.D_out = h->l0_D.as<float>(); no.P_out = h->l0_P.as<float>(); }
    no.l0_gate = (l0 && c.l0_reuse) ? 1 : 0;
    if ((r = launch_row(NODE_ROWS[rt.node], no, h, 0, c.st))) return fail(-1, "node(0) launch failed (%d)", r);
    no.l0_gate = 0;
    no.hn_out = h->hn.as<float>(); no.S_out = h->S.as<float>(); no.D_out = h->D.as<float>(); no.P_out = h->P.as<float>();
    clock.mark("node_first");

    for (int l = 0; l < h->L; ++l) {
        const ConvEdgeArgs ca = conv_args(h, l, l0);
        if ((r = clock.begin(l))) return r;
        if ((r = launch_row(CONV_ROWS[route_conv(rt, l, h->L)], ca, h, small_tiles, c.st))) return fail(-1, "conv edge launch failed (%d)", r);
        if ((r = clock.end())) return r;
        clock.mark("conv_edge");
        if (ca.emb_out) {
            if ((r = launch_edge_update(edge_update_args(h, l), rt.HT, small_tiles > 0 ? std::max(1, small_tiles / 4) : 2 * h->n_cu, c.st)))
                return fail(-1, "edge update launch failed (%d)", r);
            clock.mark("edge_update");
        }
        no.mode = (l == h->L - 1) ? 2 : 1;
        no.post = h->layers[l].node;
        if (l + 1 < h->L) no.pre = h->layers[l + 1].node;
        no.h_in = l == 0 ? h0 : hptr(l);
        no.P_in = (l0 && l == 0) ? h->l0_P.as<float>() : h->P.as<float>();
        no.h_out = hptr(l + 1);
        if ((r = launch_row(NODE_ROWS[rt.node], no, h, 0, c.st))) return fail(-1, "node launch failed (%d)", r);
        clock.mark(no.mode == 2 ? "node_last_decode" : "node_mid");
    }
    return 0;
}

}  // namespace

// ---- timing: the marks of gamd_profile (one labelled event behind every stage) and the pairs of gamd_timing_* around the edge
//      kernels (kind 100: the encoder, kind l: the conv-layer edge kernel of layer l) -------------------------------------------
void StageClock::mark(const char* label) {
    if (!evs) return;
    (void)hipEventRecord(evs[n_ev++], st);
    labels.push_back(label);
}
int StageClock::begin(int kind) {
    if (!h->timing) return 0;
    if (h->tev_used + 2 > h->tev.size()) {
        if (h->tev.size() >= 8 * gamd_handle::EVENT_POOL_CAP) { full = true; return 0; }   // pool full: not timed any more
        for (int k = 0; k < 256; ++k) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); h->tev.push_back(e); h->tev_kind.push_back(0); }
    }
    h->tev_kind[h->tev_used] = kind;
    HIP_TRY(hipEventRecord(h->tev[h->tev_used], st));
    return 0;
}
int StageClock::end() {
    if (!h->timing || full) return 0;
    HIP_TRY(hipEventRecord(h->tev[h->tev_used + 1], st));
    h->tev_used += 2;
    return 0;
}

// classical: a step of an enqueued MD run under gamd_md_force_source.  The neighbour stage stays — the fused integrator halves,
// the observers' edge list and pos_s, and the freeze / resume machinery hang on it — and the potential's launches (two for
// Lennard-Jones, five for water) stand where encoder, conv layers and decoder would.
int enqueue_forward(gamd_handle* h, const ForwardCall& c, StageClock& clock, bool classical) {
    int r;
    clock.mark("begin");
    if ((r = neighbour_stage(h, c))) return r;
    clock.mark("neighbor_build");
    if ((r = classical ? drive_enqueue(h) : network_stage(h, c, clock))) return r;
    // inside an enqueued MD run only the last step's counters are fetched (an overflow in any step reaches the host
    // through the mapped sticky flags): one copy node less per step
    if (c.copy_counters)
        HIP_TRY(hipMemcpyAsync(h->counters_host, h->cur_counters, sizeof(int) * CNT_COUNT, hipMemcpyDeviceToHost, c.st));
    return 0;
}
