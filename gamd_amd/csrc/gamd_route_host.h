// gamd_route_host.h — which kernel family a configuration reaches, decided once: gamd_route() from gamd_config (and whether the
// state_dict carries update_edge_emb's per-layer edge_layer_norm) to the padded widths, the family flags and one enumerator per
// stage; route_small_tiles() for the per-call tile regime; and the table that names, per enumerator, the launcher and the kernel of
// both regimes.  gamd_create, pack_weights and the forward (forward.hip) read this one result.  Plain C++17 (no HIP header):
// tools/route_host_check.cpp builds it on its own under the host sanitizers, tests/test_route_host.py holds every case's route
// to tests/golden/forward_routes.json.
#pragma once
#include "../../include/gamd_hip.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>

#pragma GCC visibility push(hidden)

// ---- what the route depends on: gamd_config's fields of the same names, nothing else ------------------------------------------
struct RouteConfig {
    int kind = GAMD_KIND_LJ, edge_dtype = GAMD_EDGE_F32;
    int encoding_size = 0, edge_embedding_dim = 0, hidden_dim = 0;     // as given: 0 = 128
    int no_expand_edge = 0, use_bond = 0, self_loop_mode = 0, keep_stages = 0, kernel_select = 0;
};
template <class Cfg> inline RouteConfig route_config(const Cfg& c) {   // from a gamd_config
    RouteConfig r;
    r.kind = c.kind; r.edge_dtype = c.edge_dtype;
    r.encoding_size = c.encoding_size; r.edge_embedding_dim = c.edge_embedding_dim; r.hidden_dim = c.hidden_dim;
    r.no_expand_edge = c.no_expand_edge; r.use_bond = c.use_bond; r.self_loop_mode = c.self_loop_mode;
    r.keep_stages = c.keep_stages; r.kernel_select = c.kernel_select;
    return r;
}

// ---- the table: enumerator, argument list of the launchers (ROUTE_ARGS_* of forward.hip), launcher and kernel of the throughput
//      regime, launcher and kernel of the small-tile regime.  X1 rows have one regime.  Kernel names without template arguments ----
#define GAMD_ENC_ROUTES(X1, X2)                                                                                              \
    X2(ENC_F32, NB, edge_encode, k_edge_encode, edge_encode_small, k_edge_encode_small)                                      \
    X1(ENC_BF16, NB, edge_encode_bf16, k_edge_encode_bf16)                                                                   \
    X1(ENC_F16X3, NB, edge_encode_f16x3, k_edge_encode_f16x3)                                                                \
    X1(ENC_WIDE, ENC_WIDE, edge_encode_wide, k_edge_encode_wide)                                                             \
    X1(ENC_WIDE_D, ENC_WIDE_D, edge_encode_wide_d, k_edge_encode_wide_d)
#define GAMD_CONV_ROUTES(X1, X2)                                                                                             \
    X2(CONV_F32, NB, conv_edge, k_conv_edge, conv_edge_small, k_conv_edge_small)                                             \
    X2(CONV_F32_L0, NB, conv_edge_l0, k_conv_edge, conv_edge_small_l0, k_conv_edge_small)                                    \
    X1(CONV_BF16, NB, conv_edge_bf16, k_conv_edge_bf16)                                                                      \
    X1(CONV_F16X3, NB, conv_edge_f16x3, k_conv_edge_f16x3)                                                                   \
    X2(CONV_WIDE, CONV_WIDE, conv_edge_wide, k_conv_edge_wide, conv_edge_small_wide, k_conv_edge_small)                      \
    X1(CONV_WIDE16, CONV_WIDE, conv_edge_wide16, k_conv_edge_wide16)                                                         \
    X1(CONV_BF16_WIDE, CONV_WIDE, conv_edge_bf16_wide, k_conv_edge_bf16_wide)                                                \
    X1(CONV_F16X3_WIDE, CONV_WIDE, conv_edge_f16x3_wide, k_conv_edge_f16x3_wide)                                             \
    X1(CONV_WIDE_D, CONV_WIDE_D, conv_edge_wide_d, k_conv_edge_wide_d)
#define GAMD_NODE_ROUTES(X1)                                                                                                 \
    X1(NODE_128, NODE, node, k_node)                                                                                         \
    X1(NODE_WIDE, NODE_WIDE, node_wide, k_node_wide)                                                                         \
    X1(NODE_WIDE_D, NODE_WIDE_D, node_wide_d, k_node_wide_d)

#define GAMD_ROUTE_ENUM1(e, args, fn, kernel) e,
#define GAMD_ROUTE_ENUM2(e, args, fn, kernel, fn_small, kernel_small) e,
enum EncKernel { GAMD_ENC_ROUTES(GAMD_ROUTE_ENUM1, GAMD_ROUTE_ENUM2) ENC_KERNELS };
enum ConvKernel { GAMD_CONV_ROUTES(GAMD_ROUTE_ENUM1, GAMD_ROUTE_ENUM2) CONV_KERNELS };
enum NodeKernel { GAMD_NODE_ROUTES(GAMD_ROUTE_ENUM1) NODE_KERNELS };
#undef GAMD_ROUTE_ENUM1
#undef GAMD_ROUTE_ENUM2

struct RouteName { const char* route; const char* kernel; const char* kernel_small; };   // kernel_small null: one regime
#define GAMD_ROUTE_NAME1(e, args, fn, kernel) {#e, #kernel, nullptr},
#define GAMD_ROUTE_NAME2(e, args, fn, kernel, fn_small, kernel_small) {#e, #kernel, #kernel_small},
constexpr RouteName ENC_NAMES[ENC_KERNELS] = {GAMD_ENC_ROUTES(GAMD_ROUTE_NAME1, GAMD_ROUTE_NAME2)};
constexpr RouteName CONV_NAMES[CONV_KERNELS] = {GAMD_CONV_ROUTES(GAMD_ROUTE_NAME1, GAMD_ROUTE_NAME2)};
constexpr RouteName NODE_NAMES[NODE_KERNELS] = {GAMD_NODE_ROUTES(GAMD_ROUTE_NAME1)};
#undef GAMD_ROUTE_NAME1
#undef GAMD_ROUTE_NAME2
// the kernel a row launches with small_tiles tiles (route_small_tiles; 0: the throughput regime)
inline const char* route_kernel_name(const RouteName& n, int small_tiles) { return small_tiles > 0 && n.kernel_small ? n.kernel_small : n.kernel; }

struct Route {
    int err = 0;                               // 0, or the code gamd_create / gamd_finalize_weights returns with `msg` as the error text
    char msg[256] = "";
    bool f32 = true;                           // edge_dtype is GAMD_EDGE_F32
    int H_true = 128, Eh_true = 128, D_true = 128;     // encoding_size, edge_embedding_dim, hidden_dim as the state_dict has them
    int H = 128, Eh = 128, Dp = 128;           // padded to the kernels' 128-blocks
    int HT = 1, EHT = 1, DT = 1;               // ... and their block counts (DT = 2: wide_d.hip)
    int n_feat = 44;                           // edge features: 44 (RBF-expanded) or 4, + 1 with use_bond
    bool update_edge = false;                  // update_edge_emb=True: conv.<l>.edge_layer_norm keys in the state_dict
    bool wide_enc = false, wide_conv = false;  // generic-width kernels (wide.hip, wide_lp.hip, wide_d.hip)
    bool ln_fold = false;                      // edge LayerNorm folded into the encoder's norm and every layer's first matrix
    bool l0_hoist = false;                     // LJ, fp32, 128 wide: layer 0 in its three-GEMM form
    bool node_f16 = false;                     // the node kernel's GEMMs in split-fp16 (reduced-precision edge modes)
    bool wide16 = false;                       // GAMD_KSEL_FORCE_HALF_QUANTUM took effect: k_conv_edge_wide16 (conv == CONV_WIDE16)
    int e_format = 0;                          // EncArgs::e_format
    int hn_perm = 0, tab16 = 0;                // NodeArgs::hn_perm, NodeArgs::tab16
    EncKernel enc = ENC_F32;
    ConvKernel conv = CONV_F32;                // every layer but ...
    ConvKernel conv_l0 = CONV_F32;             // ... layer 0 (differs under l0_hoist) ...
    ConvKernel conv_emb = CONV_F32;            // ... and, update_edge, the layers that write e_emb for the next (all but the last):
                                               // k_conv_edge_wide16 has no such output, they stay on the 32-edge kernels
    NodeKernel node = NODE_128;
};
inline ConvKernel route_conv(const Route& r, int layer, int n_layers) {
    if (r.update_edge && layer + 1 < n_layers) return r.conv_emb;
    return layer == 0 ? r.conv_l0 : r.conv;
}

inline Route route_refuse(Route r, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(r.msg, sizeof(r.msg), fmt, ap);
    va_end(ap);
    r.err = code;
    return r;
}

// update_edge: the state_dict has "graph_conv.conv.0.edge_layer_norm.weight" (false until the weights are there: gamd_create)
inline Route gamd_route(const RouteConfig& c, bool update_edge) {
    Route r;
    const int dtype = c.edge_dtype;
    r.f32 = dtype == GAMD_EDGE_F32;
    // Widths as build_model hands them to the model constructors (nn_module.py:561-601, :410-460, :266-320).  The kernels work
    // in 128-wide blocks: narrower (or in-between) widths are zero-padded by pack_weights — padded features stay exact zeros
    // through every Linear / SiLU / GELU, and the two LayerNorms divide by the true width.
    r.H_true = c.encoding_size ? c.encoding_size : 128;
    r.Eh_true = c.edge_embedding_dim ? c.edge_embedding_dim : 128;
    r.D_true = c.hidden_dim ? c.hidden_dim : 128;
    if (r.H_true < 1 || r.H_true > 256 || r.Eh_true < 1 || r.Eh_true > 256)
        return route_refuse(r, -22, "encoding_size and edge_embedding_dim must be in [1, 256] (got %d, %d)", r.H_true, r.Eh_true);
    if (r.D_true < 1 || r.D_true > 256) return route_refuse(r, -22, "hidden_dim must be in [1, 256] (got %d)", r.D_true);
    r.H = r.H_true <= 128 ? 128 : 256; r.Eh = r.Eh_true <= 128 ? 128 : 256; r.Dp = r.D_true <= 128 ? 128 : 256;
    r.HT = r.H / 128; r.EHT = r.Eh / 128; r.DT = r.Dp / 128;
    // hidden_dim above 128: two 128-blocks per D-wide operand, the fp32 kernels of wide_d.hip
    if (r.DT > 1 && !r.f32) return route_refuse(r, -22, "hidden_dim above 128 is built for edge_dtype f32 only (got hidden_dim %d)", r.D_true);
    r.n_feat = (c.no_expand_edge ? 4 : 44) + (c.use_bond ? 1 : 0);
    // update_edge_emb=True checkpoints (WaterMDDynamicBoxNet(update_edge=True), nn_module.py:91-92): every conv layer owns an
    // edge_layer_norm; LayerNorm(in_edge_feats) is applied to e_emb of width in_node_feats (:141), so the two must agree.
    // Served by the generic-width kernels (wide.hip) for any width.
    r.update_edge = update_edge;
    if (update_edge) {
        if (r.H_true != r.Eh_true) return route_refuse(r, -22, "update_edge_emb needs encoding_size == edge_embedding_dim (got %d, %d)", r.H_true, r.Eh_true);
        if (!r.f32 || c.self_loop_mode) return route_refuse(r, -22, "update_edge_emb is built for the fp32 edge MLP without appended self loops");
    }
    const bool exact128 = r.H_true == 128 && r.Eh_true == 128 && r.D_true == 128;
    const bool generic = r.H != 128 || r.Eh != 128 || c.no_expand_edge;
    const bool forced = (c.kernel_select & GAMD_KSEL_FORCE_GENERIC_WIDTH) && r.f32;
    // reduced-precision edge MLPs (bf16, fp32-grade split-fp16) exist for every width and both feature sets: 128 / 128 / 128
    // expanded runs the specialised kernels, anything else wide.hip's encoder writing the operands + wide_lp.hip
    const bool lp_generic = !r.f32 && (generic || !exact128);
    r.wide_enc = generic || forced || lp_generic || r.DT > 1 || update_edge;
    r.wide_conv = r.H != 128 || r.Eh != 128 || forced || lp_generic || r.DT > 1 || update_edge;
    // Folded edge LayerNorm (gamd_ln_fold_host.h): the fp32 128-wide kernels without appended self loops; not with keep_stages
    // (e is then a stage the getters hand out), not under GAMD_KSEL_NO_LN_FOLD
    r.ln_fold = r.f32 && !r.wide_enc && !r.wide_conv && c.self_loop_mode == GAMD_SELF_LOOP_DGL07_NOOP && !c.keep_stages &&
                !(c.kernel_select & GAMD_KSEL_NO_LN_FOLD);
    // Layer-0 form (conv_edge.hip): every atom of an LJ model enters layer 0 with the same row node_emb (nn_module.py:681), so
    // hn0 = norm_layers[0](node_emb) is one row and phi_edge of the aggregated messages is M0 sum_j T3_j + d_i c0.  The fp32
    // 128-wide kernels only; not under GAMD_KSEL_NO_LAYER0_HOIST.
    r.l0_hoist = c.kind == GAMD_KIND_LJ && r.f32 && !r.wide_conv && !(c.kernel_select & GAMD_KSEL_NO_LAYER0_HOIST);
    // Reduced-precision edge modes: the node kernel's five GEMMs run in split-fp16 too (fp32-grade results at 3/16 of the fp32
    // matrix time, node.hip and wide.hip's k_node_wide)
    r.node_f16 = c.edge_dtype != GAMD_EDGE_F32;
    r.e_format = !r.wide_enc ? 0 : dtype == GAMD_EDGE_F16X3 ? 2 : dtype == GAMD_EDGE_BF16 ? 1 : 0;
    r.hn_perm = (!r.wide_conv && dtype == GAMD_EDGE_F16X3) ? 1 : 0;
    r.tab16 = (!r.wide_conv && dtype == GAMD_EDGE_BF16) ? 1 : 0;       // conv_edge_bf16.hip gathers fp16 rows
    // Generic-width fp32 conv kernel on 16-edge work units (k_conv_edge_wide16, bit-identical to k_conv_edge_wide): opt-in through
    // GAMD_KSEL_FORCE_HALF_QUANTUM.  The idea — with t tiles per SIMD the launch takes ceil(2 t) / 2 tile quanta instead of ceil(t):
    // 1.5 instead of 2 at the DFT-water size — holds for the matrix time (61 against 82 us) but not for the launch: one wave per
    // SIMD pays the barrier, the 64 KiB weight copy and its vector work per 8 192-cycle phase instead of per 32 768-cycle phase
    // pair, ~2.7 us x 18 phases (110 us against 107, profiles/r06_experiments.md).  Not chosen automatically.
    r.wide16 = r.wide_conv && r.f32 && r.DT == 1 && (c.kernel_select & GAMD_KSEL_FORCE_HALF_QUANTUM) != 0;

    r.enc = r.DT > 1 ? ENC_WIDE_D : r.wide_enc ? ENC_WIDE : dtype == GAMD_EDGE_BF16 ? ENC_BF16 : dtype == GAMD_EDGE_F16X3 ? ENC_F16X3 : ENC_F32;
    if (r.DT > 1) r.conv = r.conv_emb = CONV_WIDE_D;
    else if (r.wide_conv) {
        r.conv_emb = dtype == GAMD_EDGE_F16X3 ? CONV_F16X3_WIDE : dtype == GAMD_EDGE_BF16 ? CONV_BF16_WIDE : CONV_WIDE;
        r.conv = r.wide16 ? CONV_WIDE16 : r.conv_emb;
    } else r.conv = r.conv_emb = dtype == GAMD_EDGE_BF16 ? CONV_BF16 : dtype == GAMD_EDGE_F16X3 ? CONV_F16X3 : CONV_F32;
    r.conv_l0 = r.l0_hoist ? CONV_F32_L0 : r.conv;
    r.node = r.DT > 1 ? NODE_WIDE_D : r.wide_conv ? NODE_WIDE : NODE_128;
    return r;
}

// gamd_config.small_tile_limit as the handle keeps it: 0 the default, negative never
inline long long route_tile_limit(long long configured) { return configured == 0 ? 512 : configured < 0 ? -1 : configured; }

// fp32 path, few tiles (measured crossover ~500 tiles, half a tile per SIMD): the latency-oriented kernels, one tile per 4-wave
// workgroup (conv_edge_small.hip, k_edge_encode_small), launched with this many workgroups.  They are bit-identical to the
// throughput kernels, so the choice (e_est: the last known edge count, or the density estimate before the first call) never shows
// in the results.  0: the throughput kernels.
inline int route_small_tiles(const Route& r, long long e_est, long long small_tile_limit) {
    if (!r.f32) return 0;
    const long long tiles = (e_est + 31) / 32;                 // GAMD_TILE edges each
    if (tiles > small_tile_limit) return 0;
    return (int)std::max<long long>(1, std::min<long long>(tiles + tiles / 8 + 1, 4096));
}

#pragma GCC visibility pop
