// route_host_check.cpp — the kernel route (gamd_amd/csrc/gamd_route_host.h) without a device, as a stand-alone program for the
// host sanitizers (tests/test_route_host.py builds it with -fsanitize=address,undefined).
//   route_host_check <kind> <edge_dtype> <encoding_size> <edge_embedding_dim> <hidden_dim> <no_expand_edge> <use_bond>
//                    <self_loop_mode> <keep_stages> <kernel_select> <update_edge> <n_layers> <small_tile_limit> <edge estimate>
// (the ten fields of RouteConfig in declaration order, whether the state_dict carries update_edge_emb, the layer count,
// gamd_config.small_tile_limit and the edge estimate of the call).  Prints the route's flags, widths and enumerators, small_tiles,
// and the kernels of one force evaluation in launch order (encoder, node, then per layer conv edge, edge update where the layer
// writes e_emb, node) by their base names; a refusal prints "error <code> <text>" instead.
#include "../gamd_amd/csrc/gamd_route_host.h"

#include <cstdlib>

int main(int argc, char** argv) {
    if (argc != 15) {
        std::fprintf(stderr, "usage: route_host_check <10 RouteConfig fields> <update_edge> <n_layers> <small_tile_limit> <edge estimate>\n");
        return 2;
    }
    long long v[14];
    for (int i = 0; i < 14; ++i) v[i] = std::atoll(argv[i + 1]);
    RouteConfig c;
    c.kind = (int)v[0]; c.edge_dtype = (int)v[1]; c.encoding_size = (int)v[2]; c.edge_embedding_dim = (int)v[3]; c.hidden_dim = (int)v[4];
    c.no_expand_edge = (int)v[5]; c.use_bond = (int)v[6]; c.self_loop_mode = (int)v[7]; c.keep_stages = (int)v[8]; c.kernel_select = (int)v[9];
    const int n_layers = (int)v[11];
    const Route r = gamd_route(c, v[10] != 0);
    if (r.err) { std::printf("error %d %s\n", r.err, r.msg); return 0; }
    std::printf("flags update_edge=%d wide_enc=%d wide_conv=%d ln_fold=%d l0_hoist=%d node_f16=%d wide16=%d e_format=%d hn_perm=%d tab16=%d\n",
                (int)r.update_edge, (int)r.wide_enc, (int)r.wide_conv, (int)r.ln_fold, (int)r.l0_hoist, (int)r.node_f16, (int)r.wide16, r.e_format,
                r.hn_perm, r.tab16);
    std::printf("widths H=%d Eh=%d Dp=%d HT=%d EHT=%d DT=%d n_feat=%d\n", r.H, r.Eh, r.Dp, r.HT, r.EHT, r.DT, r.n_feat);
    std::printf("route enc=%s conv=%s conv_l0=%s conv_emb=%s node=%s\n", ENC_NAMES[r.enc].route, CONV_NAMES[r.conv].route,
                CONV_NAMES[r.conv_l0].route, CONV_NAMES[r.conv_emb].route, NODE_NAMES[r.node].route);
    const int small_tiles = route_small_tiles(r, v[13], route_tile_limit(v[12]));
    std::printf("small_tiles %d\n", small_tiles);
    std::printf("kernels %s %s", route_kernel_name(ENC_NAMES[r.enc], small_tiles), NODE_NAMES[r.node].kernel);
    for (int l = 0; l < n_layers; ++l) {
        std::printf(" %s", route_kernel_name(CONV_NAMES[route_conv(r, l, n_layers)], small_tiles));
        if (r.update_edge && l + 1 < n_layers) std::printf(" k_edge_update");
        std::printf(" %s", NODE_NAMES[r.node].kernel);
    }
    std::printf("\n");
    return 0;
}
