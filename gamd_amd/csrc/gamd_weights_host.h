// gamd_weights_host.h — everything gamd_finalize_weights does to the state_dict before the upload: the tensor look-up and
// zero padding, the host arithmetic the kernels' numerics rest on (eval BatchNorm fold, layer-0 form, centred last encoder
// Linear, log2 e / ln 2 rescaling, F2 row order, uniform RBF grid) and the fragment images of every kernel family, laid into one
// blob with its offset tables.  Plain C++17 (no HIP header): tools/weights_host_check.cpp builds it on its own under the host
// sanitizers, and tests/test_weights_host.py pins the blob of every family byte for byte (tests/golden/weight_blob_digests.json).
#pragma once
#include "../../include/gamd_hip.h"
#include "gamd_ln_fold_host.h"
#include "gamd_route_host.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <initializer_list>
#include <map>
#include <string>
#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
};

constexpr int WH_FRAG_FLOATS = 128 * 128;      // GAMD_WFRAG_FLOATS of gamd_common.h: one packed 128x128 weight = 64 KiB
constexpr int WH_ENC1_FLOATS = 4 * 6 * 64 * 4; // one 128-row image of the encoder's first Linear, K padded to 48

// ---- weight packing ---------------------------------------------------------------------------
// W [128 out][128 in] block of a row-major matrix with row stride ld -> fragment order of gamd_common.h
inline void pack128(const float* W, float* out, int ld = 128) {
    for (int tp = 0; tp < 4; ++tp)
        for (int t = 0; t < 4; ++t)
            for (int q = 0; q < 4; ++q)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j) {
                        const int n = 32 * tp + (lane & 31), k = 32 * t + 8 * q + 4 * (lane >> 5) + j;
                        out[((((tp * 4 + t) * 4 + q) * 64 + lane) * 4) + j] = W[(size_t)n * ld + k];
                    }
}
// W [128 out][128 in] -> operand order of node.hip's 16x16x4 chain: block (ob, blk) = 16 output features x 16 inputs,
// lane (i = lane & 15, g = lane >> 4) holds W[16 ob + i][16 blk + 4 g + 0..3]; a wave's quarter (ob = 2 w, 2 w + 1) is contiguous
inline void pack16(const float* W, float* out, int ld = 128) {
    for (int ob = 0; ob < 8; ++ob)
        for (int blk = 0; blk < 8; ++blk)
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 4; ++r)
                    out[(((ob * 8 + blk) * 64 + lane) * 4) + r] = W[(size_t)(16 * ob + (lane & 15)) * ld + 16 * blk + 4 * (lane >> 4) + r];
}
// encoder first layer W [128][n_feat]: MFMA step s covers features (2s, 2s+1); K padded to 48
inline void pack_enc1(const float* W, int n_feat, float* out) {
    for (int tp = 0; tp < 4; ++tp)
        for (int g = 0; g < 6; ++g)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    const int n = 32 * tp + (lane & 31), k = 2 * (4 * g + j) + (lane >> 5);
                    out[(((tp * 6 + g) * 64 + lane) * 4) + j] = k < n_feat ? W[n * n_feat + k] : 0.f;
                }
}

// ---- packing for the 16-edge generic-width conv kernel (wide16.hip) --------------------------------------------------------
// K position p = 4 m + g of the 32-edge kernels' accumulation order <-> input feature kfeat(m, g); image [ob 8][m4 8][lane 64][c 4]
// = W[row(ob, lane & 15)][kfeat(4 m4 + c, lane >> 4)].  chained = true (W1, W2, W3): packed output row 16 ob + 4 g' + r' is feature
// kfeat(4 ob + r', g'), so the C/D registers of one GEMM are the B operands of the next; chained = false (W4): packed column n of
// block ob is feature 64 (ob >> 2) + 4 n + (ob & 3) (a lane of the F2 output owns four consecutive features).
inline int kfeat16x(int m, int g) { return 32 * (m >> 3) + 8 * ((m >> 1) & 3) + 4 * (g & 1) + (g >> 1) + 2 * (m & 1); }
inline void pack16x(const float* W, float* out, int ld, bool chained) {
    for (int ob = 0; ob < 8; ++ob)
        for (int m4 = 0; m4 < 8; ++m4)
            for (int lane = 0; lane < 64; ++lane) {
                const int i = lane & 15, g = lane >> 4;
                const int row = chained ? kfeat16x(4 * ob + (i & 3), i >> 2) : 64 * (ob >> 2) + 4 * i + (ob & 3);
                for (int c = 0; c < 4; ++c)
                    out[(((size_t)ob * 8 + m4) * 64 + lane) * 4 + c] = W[(size_t)row * ld + kfeat16x(4 * m4 + c, g)];
            }
}

// ---- bf16 packing (config 5, layout of gamd_bf16.h) and split-fp16 packing (GAMD_EDGE_F16X3, layout of gamd_f16x3.h: [hi part |
//      lo part]) walk one order of 16-bit values: at(W[n][k]) for a 128 x 128 block, K padded to 48 for the encoder's first Linear
inline uint16_t f2bf(float x) {                // round to nearest even
    uint32_t u; memcpy(&u, &x, 4);
    if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)(u >> 16);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline void split_f16(float w, uint16_t* hi, uint16_t* lo) {
    const _Float16 h = (_Float16)w;                              // round to nearest even, subnormals kept
    const _Float16 l = (_Float16)(w - (float)h);
    memcpy(hi, &h, 2); memcpy(lo, &l, 2);
}
template <class Emit> inline void walk128_halves(const float* W, int ld, Emit emit) {       // [tp][t][u][lane][8]
    for (int tp = 0; tp < 4; ++tp)
        for (int t = 0; t < 4; ++t)
            for (int u = 0; u < 2; ++u)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int r = 8 * u + j, half = lane >> 5;
                        const int n = 32 * tp + (lane & 31), k = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half;
                        emit((size_t)((((tp * 4 + t) * 2 + u) * 64 + lane) * 8) + j, W[(size_t)n * ld + k]);
                    }
}
template <class Emit> inline void walk_enc1_halves(const float* W, int n_feat, Emit emit) {   // [tp][s][lane][8], K padded to 48
    for (int tp = 0; tp < 4; ++tp)
        for (int s = 0; s < 3; ++s)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int n = 32 * tp + (lane & 31), k = 16 * s + 8 * (lane >> 5) + j;
                    emit((size_t)(((tp * 3 + s) * 64 + lane) * 8) + j, k < n_feat ? W[n * n_feat + k] : 0.f);
                }
}
inline void pack128_bf16(const float* W, uint16_t* out, int ld = 128) { walk128_halves(W, ld, [&](size_t at, float w) { out[at] = f2bf(w); }); }
inline void pack_enc1_bf16(const float* W, int n_feat, uint16_t* out) { walk_enc1_halves(W, n_feat, [&](size_t at, float w) { out[at] = f2bf(w); }); }
// 2 x 16384 halves = 64 KiB; W: a 128 x 128 block, row stride ld
inline void pack128_f16x3(const float* W, uint16_t* out, int ld = 128) { walk128_halves(W, ld, [&](size_t at, float w) { split_f16(w, out + at, out + 16384 + at); }); }
inline void pack_enc1_f16x3(const float* W, int n_feat, uint16_t* out) { walk_enc1_halves(W, n_feat, [&](size_t at, float w) { split_f16(w, out + at, out + 6144 + at); }); }
// the node-side matrix as (hi | lo) fp16 fragments for node.hip's split-fp16 GEMMs on 16x16x32: fragment ((ob * 4 + m) * 2 + part),
// lane (o = lane & 15, g = lane >> 4), value j = W[16 ob + o][32 m + 16 (j >> 2) + 4 g + (j & 3)]  -- 64 KiB like the fp32 image
inline void pack16_f16x3(const float* W, uint16_t* out) {
    for (int ob = 0; ob < 8; ++ob)
        for (int m = 0; m < 4; ++m)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int k = 32 * m + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3);
                    const size_t hi = ((((size_t)(ob * 4 + m) * 2 + 0) * 64 + lane) * 8) + j, lo = ((((size_t)(ob * 4 + m) * 2 + 1) * 64 + lane) * 8) + j;
                    split_f16(W[(size_t)(16 * ob + (lane & 15)) * 128 + k], out + hi, out + lo);
                }
}

struct BlobBuilder {
    std::vector<float> host;
    size_t add(size_t n_floats) {
        const size_t off = host.size();
        host.resize(off + ((n_floats + 63) & ~(size_t)63), 0.f);
        return off;
    }
};

// a 128x128 block of a row-major matrix into one slot of the blob: the three edge-matrix formats (the bf16 image is half a slot)
using BlockPacker = void (*)(const float* W, float* out, int ld);
inline void block_f32(const float* W, float* out, int ld) { pack128(W, out, ld); }
inline void block_bf16(const float* W, float* out, int ld) { pack128_bf16(W, reinterpret_cast<uint16_t*>(out), ld); }
inline void block_f16x3(const float* W, float* out, int ld) { pack128_f16x3(W, reinterpret_cast<uint16_t*>(out), ld); }

// rows 32 q + s <- rows 4 s + q of a [128][128] matrix and its bias: the F2 output order of the last GEMM of the 128-wide
// fp32 / bf16 conv kernels (a lane holds four consecutive features of each edge)
inline void permute_f2(const HostTensor& w, const HostTensor& b, HostTensor& wo, HostTensor& bo) {
    wo = w;
    bo = b;
    for (int q = 0; q < 4; ++q)
        for (int s = 0; s < 32; ++s) {
            std::copy(w.data.begin() + (size_t)(4 * s + q) * 128, w.data.begin() + (size_t)(4 * s + q + 1) * 128,
                      wo.data.begin() + (size_t)(32 * q + s) * 128);
            bo.data[32 * q + s] = b.data[4 * s + q];
        }
}

// ---- what comes out: offsets into the blob, in floats, under the names of the pointers they become (LayerDev, NodeLayerW and
//      the handle's enc_* / dec_* / node_* members: gamd_finalize_weights walks these lists).  WOFF_NONE: a null pointer ---------
constexpr size_t WOFF_NONE = ~(size_t)0;
#define GAMD_W_LAYER_FIELDS(X) X(w1p) X(w2p) X(w3p) X(w4p) X(b1) X(b3) X(b4) X(w16p) X(e_ln_g) X(e_ln_b) X(w3p_l0) X(b3_l0)
#define GAMD_W_NODE_FIELDS(X) X(ln_g) X(ln_b) X(wsp) X(wdp) X(wpdp) X(bS) X(bP) X(wpep) X(c0) X(wphip) X(bphi)
#define GAMD_W_GLOBAL_FIELDS(X)                                                                                               \
    X(enc_w1p) X(enc_w2p) X(enc_w3p) X(enc_b1) X(enc_b2) X(enc_b3) X(enc_lng) X(enc_lnb) X(centers) X(node_emb) X(nenc_w) X(nenc_b) \
    X(dec_w1p) X(dec_b1) X(dec_w2) X(dec_b2)
#define GAMD_W_DECLARE(f) size_t f = WOFF_NONE;
struct NodeOff { GAMD_W_NODE_FIELDS(GAMD_W_DECLARE) };
struct LayerOff {
    GAMD_W_LAYER_FIELDS(GAMD_W_DECLARE)        // w16p: generic-width fp32 with hidden_dim <= 128 only; e_ln_*: update_edge only
    NodeOff node;                              // c0: layer 0 of an l0_hoist model only
    size_t m0 = WOFF_NONE;                     // l0_hoist, layer 0: M0, which post(0) reads in node.wpep's place
};
struct GlobalOff { GAMD_W_GLOBAL_FIELDS(GAMD_W_DECLARE) };
#undef GAMD_W_DECLARE

struct HostRbfGrid { int uniform = 0; float c0 = 0.f, delta = 0.f, A = 0.f, B = 0.f, C = 0.f; };   // RbfGrid of gamd_common.h

struct PackedWeights {
    int err = 0;                               // 0, or the code gamd_finalize_weights returns with `msg` as the error text
    char msg[512] = "";
    std::vector<float> blob;
    std::vector<LayerOff> layers;
    GlobalOff g;
    bool norm_bn = false;                      // graph_conv.norm_layers are BatchNorm1d (running statistics in the state_dict)
    float length_mean = 0.f, length_std = 1.f;
    HostRbfGrid rbf;                           // uniform = 1 when edge_expand.centers is a uniform grid
};

class WeightPacker {
public:
    WeightPacker(const RouteConfig& cfg, const Route& route, int n_layers, const std::map<std::string, HostTensor>& w)
        : s(cfg), rt(route), n_layers(n_layers), w(w), H(route.H), Eh(route.Eh), HT(route.HT), EHT(route.EHT), Ht(route.H_true),
          Et(route.Eh_true), Dt(route.D_true), Dp(route.Dp), DT(route.DT) {}

    PackedWeights run() { if (pack()) out.blob = std::move(bb.host); return std::move(out); }

private:
    bool pack() {
        if (rt.err) return refuse(rt.err, "%s", rt.msg);
        const bool lp128 = s.edge_dtype != GAMD_EDGE_F32 && !rt.wide_conv;   // 128 / 128 / 128 expanded: the specialised kernels
        bf16_edges = lp128 && s.edge_dtype == GAMD_EDGE_BF16;                 // (any other width / feature set: wide_lp.hip)
        f16x3_edges = lp128 && s.edge_dtype == GAMD_EDGE_F16X3;
        edge_fmt = s.edge_dtype == GAMD_EDGE_BF16 ? block_bf16 : s.edge_dtype == GAMD_EDGE_F16X3 ? block_f16x3 : block_f32;
        edge_slot = s.edge_dtype == GAMD_EDGE_BF16 ? WH_FRAG_FLOATS / 2 : WH_FRAG_FLOATS;
        // BatchNorm checkpoints carry running statistics next to norm_layers' weight and bias
        out.norm_bn = w.count("graph_conv.norm_layers.0.running_mean") != 0;
        if (rt.l0_hoist && !(emb0 = get("node_emb", {1, Ht}, {1, H}))) return false;
        // Folded edge LayerNorm: B = C W_e3, c = C b_e3 (the centred last encoder Linear, in double) for the layers' first matrices
        if (rt.ln_fold) {
            const HostTensor *w3 = get("edge_encoder.mlp_layer.4.weight", {Et, Dt}, {Eh, Dp}), *b3 = get("edge_encoder.mlp_layer.4.bias", {Et}, {Eh});
            fold_g = get("edge_layer_norm.weight", {Et}, {Eh});
            fold_b = get("edge_layer_norm.bias", {Et}, {Eh});
            if (out.err) return false;
            lnf_center(w3->data.data(), b3->data.data(), (int)Et, fold_B, fold_c);
        }
        out.layers.assign((size_t)n_layers, LayerOff{});
        for (int l = 0; l < n_layers; ++l)
            if (!pack_layer(l)) return false;
        return pack_encoder_decoder();
    }

    struct LayerTensors {
        const HostTensor *ea0w, *ea0b, *ea2w, *ea2b, *sw, *sb, *dw, *db, *t1w, *t1b, *t3w, *t3b, *pdw, *pdb, *pew, *peb, *phw, *phb, *ng, *nb;
    };

    const RouteConfig& s;
    const Route& rt;                           // the family flags and widths every branch below reads
    const int n_layers;
    const std::map<std::string, HostTensor>& w;
    const int64_t H, Eh, HT, EHT;              // padded widths the kernels work in
    const int64_t Ht, Et, Dt;                  // the state_dict's widths
    const int64_t Dp, DT;                      // hidden_dim padded to 128-blocks (DT = 2: wide_d.hip)
    PackedWeights out;
    BlobBuilder bb;
    std::deque<HostTensor> made;               // padded, folded, scaled and permuted tensors: alive until the blob is complete
    bool bf16_edges = false, f16x3_edges = false;
    BlockPacker edge_fmt = block_f32;
    size_t edge_slot = WH_FRAG_FLOATS;
    const HostTensor* emb0 = nullptr;
    std::vector<double> fold_B, fold_c;
    const HostTensor *fold_g = nullptr, *fold_b = nullptr;

    bool refuse(int code, const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(out.msg, sizeof(out.msg), fmt, ap);
        va_end(ap);
        out.err = code;
        return false;
    }
    const HostTensor* keep(HostTensor&& t) { made.push_back(std::move(t)); return &made.back(); }

    // A tensor that is missing or has another shape than the configuration's ends the packing with -2; the text says which of the
    // two it was.  Every look-up of a group runs before the group is judged, so the text names the group's last bad tensor.
    const HostTensor* find(const std::string& name, std::initializer_list<int64_t> shape) {
        auto it = w.find(name);
        if (it == w.end()) { refuse(-2, "missing weight '%s'", name.c_str()); return nullptr; }
        if (it->second.shape != std::vector<int64_t>(shape)) {
            auto dims = [](const std::vector<int64_t>& v) { std::string o; for (auto d : v) o += std::to_string(d) + ","; return o; };
            refuse(-2, "weight '%s' has shape (%s), expected (%s) for this configuration", name.c_str(), dims(it->second.shape).c_str(), dims(shape).c_str());
            return nullptr;
        }
        return &it->second;
    }
    // get(name, true shape, padded shape): the tensor as the reference stores it, zero-padded to the kernels' block widths.
    // Padded output rows / input columns are zeros, so padded features are exact zeros through every layer.
    const HostTensor* get(const std::string& nm, std::initializer_list<int64_t> shp, std::initializer_list<int64_t> pad) {
        const HostTensor* t = find(nm, shp);
        if (!t) return nullptr;
        const std::vector<int64_t> ps(pad);
        if (t->shape == ps) return t;
        HostTensor o;
        o.shape = ps;
        const int64_t r = ps.size() == 2 ? t->shape[0] : 1, c = ps.size() == 2 ? t->shape[1] : t->shape[0];
        const int64_t cp = ps.size() == 2 ? ps[1] : ps[0], rp = ps.size() == 2 ? ps[0] : 1;
        o.data.assign((size_t)(rp * cp), 0.f);
        for (int64_t i = 0; i < r; ++i) std::copy(t->data.begin() + i * c, t->data.begin() + (i + 1) * c, o.data.begin() + i * cp);
        return keep(std::move(o));
    }

    size_t put_vec(const HostTensor* t) { const size_t o = bb.add(t->data.size()); std::copy(t->data.begin(), t->data.end(), bb.host.begin() + o); return o; }
    // [128 OB][128 KB] matrix -> OB*KB packed 128x128 blocks in slots of `slot` floats, block (ob, kb) at index ob*KB + kb
    size_t put_blocks(const HostTensor* t, int64_t OB, int64_t KB, BlockPacker pack = block_f32, size_t slot = WH_FRAG_FLOATS) {
        const size_t o = bb.add((size_t)(OB * KB) * slot);
        for (int64_t ob = 0; ob < OB; ++ob)
            for (int64_t kb = 0; kb < KB; ++kb)
                pack(t->data.data() + (size_t)(128 * ob * 128 * KB + 128 * kb), bb.host.data() + o + (size_t)(ob * KB + kb) * slot, (int)(128 * KB));
        return o;
    }
    size_t put_edge(const HostTensor* t, int64_t OB = 1, int64_t KB = 1) { return put_blocks(t, OB, KB, edge_fmt, edge_slot); }
    // node-side matrices: the 128-wide node kernel (node.hip) runs on 16x16x4 MFMAs with its own operand order; the
    // generic-width node kernel of wide.hip keeps the 32x32x2 fragment blocks
    size_t put_node(const HostTensor* t, int64_t OB, int64_t KB) {
        if (rt.wide_conv) return put_blocks(t, OB, KB, rt.node_f16 ? block_f16x3 : block_f32);
        const size_t o = bb.add(WH_FRAG_FLOATS);
        if (rt.node_f16) pack16_f16x3(t->data.data(), reinterpret_cast<uint16_t*>(bb.host.data() + o));
        else pack16(t->data.data(), bb.host.data() + o);
        return o;
    }

    bool fetch_layer(int l, LayerTensors& t) {
        const std::string p = "graph_conv.conv." + std::to_string(l), n = "graph_conv.norm_layers." + std::to_string(l);
        // edge_affine = MLP(Eh, hidden_dim, hidden_layer=2): its inner width is MLP's default 128 (nn_module.py:25,95)
        t.ea0w = get(p + ".edge_affine.mlp_layer.0.weight", {128, Et}, {128, Eh}); t.ea0b = get(p + ".edge_affine.mlp_layer.0.bias", {128}, {128});
        t.ea2w = get(p + ".edge_affine.mlp_layer.2.weight", {Dt, 128}, {Dp, 128}); t.ea2b = get(p + ".edge_affine.mlp_layer.2.bias", {Dt}, {Dp});
        t.sw = get(p + ".src_affine.weight", {Dt, Ht}, {Dp, H}); t.sb = get(p + ".src_affine.bias", {Dt}, {Dp});
        t.dw = get(p + ".dst_affine.weight", {Dt, Ht}, {Dp, H}); t.db = get(p + ".dst_affine.bias", {Dt}, {Dp});
        t.t1w = get(p + ".theta_edge.mlp_layer.1.weight", {Dt, Dt}, {Dp, Dp}); t.t1b = get(p + ".theta_edge.mlp_layer.1.bias", {Dt}, {Dp});
        t.t3w = get(p + ".theta_edge.mlp_layer.3.weight", {Ht, Dt}, {H, Dp}); t.t3b = get(p + ".theta_edge.mlp_layer.3.bias", {Ht}, {H});
        t.pdw = get(p + ".phi_dst.weight", {Dt, Ht}, {Dp, H}); t.pdb = get(p + ".phi_dst.bias", {Dt}, {Dp});
        t.pew = get(p + ".phi_edge.weight", {Dt, Ht}, {Dp, H}); t.peb = get(p + ".phi_edge.bias", {Dt}, {Dp});
        t.phw = get(p + ".phi.mlp_layer.1.weight", {Ht, Dt}, {H, Dp}); t.phb = get(p + ".phi.mlp_layer.1.bias", {Ht}, {H});
        t.ng = get(n + ".weight", {Ht}, {H});
        t.nb = get(n + ".bias", {Ht}, {H});
        return !out.err;
    }

    // use_layer_norm=False (the constructors' default, nn_module.py:171-196,579): norm_layers are nn.BatchNorm1d; the
    // rollout runs the model in eval mode, where it is the per-feature affine map torch's CPU kernel evaluates as
    // x * alpha + beta with alpha = weight / sqrt(running_var + eps), beta = bias - running_mean * alpha (float).
    // Folded here into the ln_g / ln_b slots; padded features keep alpha = beta = 0.
    bool fold_batchnorm(int l, LayerTensors& t) {
        const std::string n = "graph_conv.norm_layers." + std::to_string(l);
        const HostTensor *rm = get(n + ".running_mean", {Ht}, {H}), *rv = get(n + ".running_var", {Ht}, {H});
        if (out.err) return false;
        const HostTensor *ng = t.ng, *nb = t.nb;
        HostTensor al, be;
        al.shape = be.shape = {H};
        al.data.assign((size_t)H, 0.f);
        be.data.assign((size_t)H, 0.f);
        for (int64_t i = 0; i < Ht; ++i) {
            const float invstd = 1.0f / std::sqrt(rv->data[i] + 1e-5f);
            al.data[i] = ng->data[i] * invstd;
            be.data[i] = nb->data[i] - rm->data[i] * al.data[i];
        }
        t.ng = keep(std::move(al));
        t.nb = keep(std::move(be));
        return true;
    }

    // bf16 edge MLP (conv_edge_bf16.hip): the pre-activations of the layer's three SiLUs are computed times log2 e, so that
    // SiLU(x) log2 e = x' / (1 + 2^-x') needs no multiply in front of its exponential: W1, b1 (first SiLU), the S / D tables
    // (second: W2 sees the first SiLU's output times log2 e and needs no factor itself), b3 (third) carry log2 e, W4 ln 2
    void scale_for_exp2(LayerTensors& t) {
        auto scaled = [&](const HostTensor* x, double f) {
            HostTensor o = *x;
            for (float& v : o.data) v = (float)((double)v * f);
            return keep(std::move(o));
        };
        const double LOG2E = 1.4426950408889634, LN2 = 0.6931471805599453;
        t.ea0w = scaled(t.ea0w, LOG2E); t.ea0b = scaled(t.ea0b, LOG2E); t.t1b = scaled(t.t1b, LOG2E); t.t3w = scaled(t.t3w, LN2);
        t.sw = scaled(t.sw, LOG2E); t.dw = scaled(t.dw, LOG2E);
        t.sb = scaled(t.sb, LOG2E); t.db = scaled(t.db, LOG2E); t.ea2b = scaled(t.ea2b, LOG2E);      // bS = (b_src + b_dst) + b_edge_affine.2
    }

    // hn0 as k_node mode 0 forms it (LayerNorm over the true width, or the folded eval BatchNorm), then
    // M0 = W_pe diag(hn0) W4 and c0 = W_pe (hn0 * b4), in double and rounded once; M0 takes phi_edge's place in post(0)
    void pack_layer0_form(const LayerTensors& t, LayerOff& o) {
        std::vector<double> hn0((size_t)H, 0.0);
        if (out.norm_bn) {
            for (int64_t i = 0; i < H; ++i) hn0[i] = (double)emb0->data[i] * t.ng->data[i] + t.nb->data[i];
        } else {
            double mean = 0.0, var = 0.0;
            for (int64_t i = 0; i < Ht; ++i) mean += emb0->data[i];
            mean /= (double)Ht;
            for (int64_t i = 0; i < Ht; ++i) var += ((double)emb0->data[i] - mean) * ((double)emb0->data[i] - mean);
            var /= (double)Ht;
            const double rstd = 1.0 / std::sqrt(var + 1e-5);
            for (int64_t i = 0; i < Ht; ++i) hn0[i] = ((double)emb0->data[i] - mean) * rstd * t.ng->data[i] + t.nb->data[i];
        }
        HostTensor m0, c0;
        m0.shape = {Dp, Dp};
        m0.data.assign((size_t)(Dp * Dp), 0.f);
        c0.shape = {Dp};
        c0.data.assign((size_t)Dp, 0.f);
        std::vector<double> row((size_t)Dp);
        for (int64_t r = 0; r < Dp; ++r) {
            std::fill(row.begin(), row.end(), 0.0);
            double cr = 0.0;
            for (int64_t i = 0; i < H; ++i) {
                const double a = (double)t.pew->data[(size_t)(r * H + i)] * hn0[i];
                if (a == 0.0) continue;
                for (int64_t k = 0; k < Dp; ++k) row[k] += a * t.t3w->data[(size_t)(i * Dp + k)];
                cr += a * t.t3b->data[i];
            }
            for (int64_t k = 0; k < Dp; ++k) m0.data[(size_t)(r * Dp + k)] = (float)row[k];
            c0.data[r] = (float)cr;
        }
        HostTensor w3f, b3f;
        permute_f2(*t.t1w, *t.t1b, w3f, b3f);
        o.w3p_l0 = put_blocks(&w3f, 1, 1);
        o.b3_l0 = put_vec(&b3f);
        o.m0 = put_node(&m0, 1, 1);
        o.node.c0 = put_vec(&c0);
    }

    // 128-wide fp32 and bf16 kernels (conv_edge.hip, conv_edge_small.hip, conv_edge_bf16.hip): output row 32 q + s of the
    // packed W4 is feature 4 s + q, so a lane of the last GEMM's F2 output holds four CONSECUTIVE features of each edge —
    // hn[src] is gathered and the pieces are stored 16 bytes at a time.  b4 is stored in the same order.
    const HostTensor* permute_w4(LayerTensors& t) {
        HostTensor w4, b4;
        permute_f2(*t.t3w, *t.t3b, w4, b4);
        t.t3b = keep(std::move(b4));
        return keep(std::move(w4));
    }

    // the four edge matrices of a layer in the format of its kernel family; may replace t.ea0b (ln_fold) and t.t3b (F2 order)
    void pack_edge_matrices(LayerTensors& t, LayerOff& o) {
        if (bf16_edges || f16x3_edges) {
            const HostTensor* w4 = bf16_edges ? permute_w4(t) : t.t3w;
            o.w1p = put_edge(t.ea0w); o.w2p = put_edge(t.ea2w); o.w3p = put_edge(t.t1w); o.w4p = put_edge(w4);
        } else if (s.edge_dtype != GAMD_EDGE_F32) {
            // wide_lp.hip: one contiguous run of bf16 (32 KiB) or [hi | lo] (64 KiB) images: W1[:, kb] (EHT) | W2 | W3 | W4[ob, :] (HT)
            o.w1p = put_edge(t.ea0w, 1, EHT);
            o.w2p = put_edge(t.ea2w);
            o.w3p = put_edge(t.t1w);
            o.w4p = put_edge(t.t3w, HT, 1);
        } else {
            // one contiguous run of blocks: W1[:, kb] (EHT) | W2 | W3 | W4[ob, :] (HT) -- the order the kernels stream them
            // (hidden_dim above 128, wide_d.hip: W1[:, kb] (EHT) | W2[db, :] (DT) | W3[ob][db] (DT x DT) | W4[ob][db] (HT x DT))
            if (rt.ln_fold) {
                // A_l = W1 diag(gamma) B and the extra K step's fragment (a_l, 0) take W1's place, b1'_l = b1 + W1 beta takes b1's
                std::vector<double> A, av, b1f;
                lnf_layer(t.ea0w->data.data(), t.ea0b->data.data(), fold_g->data.data(), fold_b->data.data(), fold_B, fold_c, A, av, b1f);
                const std::vector<float> Af = lnf_round(A), af = lnf_round(av);
                o.w1p = bb.add((size_t)LNF_A_FLOATS);
                lnf_pack_a(Af.data(), af.data(), bb.host.data() + o.w1p);
                HostTensor b1t;
                b1t.shape = {128};
                b1t.data = lnf_round(b1f);
                t.ea0b = keep(std::move(b1t));
            } else {
                o.w1p = put_blocks(t.ea0w, 1, EHT);
            }
            o.w2p = put_blocks(t.ea2w, DT, 1);
            o.w3p = put_blocks(t.t1w, DT, DT);
            if (DT > 1) {
                o.w4p = put_blocks(t.t3w, HT, DT);
            } else if (rt.wide_conv) {
                o.w4p = put_blocks(t.t3w, HT, 1);
                // the same run of blocks for the opt-in 16-edge kernel (wide16.hip): W1[:, kb] | W2 | W3 chained, W4[ob, :] not
                o.w16p = bb.add((size_t)(EHT + 2 + HT) * WH_FRAG_FLOATS);
                size_t at = o.w16p;
                for (int kb = 0; kb < (int)EHT; ++kb, at += WH_FRAG_FLOATS) pack16x(t.ea0w->data.data() + 128 * kb, bb.host.data() + at, 128 * (int)EHT, true);
                pack16x(t.ea2w->data.data(), bb.host.data() + at, 128, true); at += WH_FRAG_FLOATS;
                pack16x(t.t1w->data.data(), bb.host.data() + at, 128, true); at += WH_FRAG_FLOATS;
                for (int ob = 0; ob < (int)HT; ++ob, at += WH_FRAG_FLOATS) pack16x(t.t3w->data.data() + (size_t)128 * ob * 128, bb.host.data() + at, 128, false);
            } else {
                o.w4p = put_blocks(permute_w4(t), 1, 1);
            }
        }
    }

    bool pack_layer(int l) {
        LayerTensors t;
        if (!fetch_layer(l, t)) return false;
        if (out.norm_bn && !fold_batchnorm(l, t)) return false;
        if (bf16_edges) scale_for_exp2(t);
        LayerOff& o = out.layers[(size_t)l];
        if (l == 0 && rt.l0_hoist) pack_layer0_form(t, o);
        pack_edge_matrices(t, o);
        o.b1 = put_vec(t.ea0b); o.b3 = put_vec(t.t1b); o.b4 = put_vec(t.t3b);
        o.node.ln_g = put_vec(t.ng); o.node.ln_b = put_vec(t.nb);
        if (rt.update_edge) {
            const std::string p = "graph_conv.conv." + std::to_string(l);
            const HostTensor *eg = get(p + ".edge_layer_norm.weight", {Et}, {Eh}), *eb = get(p + ".edge_layer_norm.bias", {Et}, {Eh});
            if (out.err) return false;
            o.e_ln_g = put_vec(eg); o.e_ln_b = put_vec(eb);
        }
        o.node.wsp = put_node(t.sw, DT, HT); o.node.wdp = put_node(t.dw, DT, HT); o.node.wpdp = put_node(t.pdw, DT, HT);
        o.node.bS = bb.add((size_t)Dp);
        for (int i = 0; i < (int)Dp; ++i) bb.host[o.node.bS + i] = (t.sb->data[i] + t.db->data[i]) + t.ea2b->data[i];
        o.node.bP = bb.add((size_t)Dp);
        for (int i = 0; i < (int)Dp; ++i) bb.host[o.node.bP + i] = t.pdb->data[i] + t.peb->data[i];
        o.node.wpep = put_node(t.pew, DT, HT); o.node.wphip = put_node(t.phw, HT, DT); o.node.bphi = put_vec(t.phb);
        return true;
    }

    // fp32 path: the last encoder Linear is stored with its OUTPUT rows centred, W' = W - mean over rows, b' = b - mean(b)
    // (in double): y' = W' x + b' = y - mean(y) exactly in real arithmetic, so edge_layer_norm's mean subtraction
    // (nn_module.py:646) is done here once instead of per edge; the kernels only normalise the variance
    // (layernorm_chain_centered; wide.hip's generic LayerNorm sees a mean of ~0 and is unaffected).
    // (the mean is over the Et true output rows; zero-padded rows stay zero)
    void center_rows(const HostTensor& e4w, const HostTensor& e4b, HostTensor& wc, HostTensor& bc) const {
        for (int64_t k = 0; k < Dp; ++k) {
            double m = 0.0;
            for (int64_t o = 0; o < Et; ++o) m += (double)e4w.data[(size_t)(o * Dp + k)];
            m /= (double)Et;
            for (int64_t o = 0; o < Et; ++o) wc.data[(size_t)(o * Dp + k)] = (float)((double)e4w.data[(size_t)(o * Dp + k)] - m);
        }
        double mb = 0.0;
        for (int64_t o = 0; o < Et; ++o) mb += (double)e4b.data[(size_t)o];
        mb /= (double)Et;
        for (int64_t o = 0; o < Et; ++o) bc.data[(size_t)o] = (float)((double)e4b.data[(size_t)o] - mb);
    }

    // RBFExpansion builds linspace(low, high, n) (nn_module.py:237-239): uniform up to fp32 rounding.  Anything else
    // (hand-edited centres) keeps the exact per-centre form.
    static HostRbfGrid rbf_grid(const HostTensor& cen) {
        const double c0 = cen.data[0], delta = ((double)cen.data[39] - c0) / 39.0;
        bool uniform = delta > 0.0;
        for (int k = 0; k < 40 && uniform; ++k)
            uniform = std::fabs((double)cen.data[k] - (c0 + k * delta)) <= 2.5e-7 * std::max(1.0, std::fabs(c0 + k * delta));
        if (!uniform) return HostRbfGrid{};
        const double gexp = -(1.0 / 0.025) * 1.4426950408889634, s = 2.0 * delta;     // -gamma log2(e), chain step
        return HostRbfGrid{1, (float)c0, (float)delta, (float)(-2.0 * gexp * s), (float)(gexp * s * s), (float)std::exp2(2.0 * gexp * s * s)};
    }

    bool pack_encoder_decoder() {
        const int F = rt.n_feat;
        const bool expand = !s.no_expand_edge;
        GlobalOff& g = out.g;
        const HostTensor *e0w = get("edge_encoder.mlp_layer.0.weight", {Dt, (int64_t)F}, {Dp, (int64_t)F}), *e0b = get("edge_encoder.mlp_layer.0.bias", {Dt}, {Dp});
        const HostTensor *e2w = get("edge_encoder.mlp_layer.2.weight", {Dt, Dt}, {Dp, Dp}), *e2b = get("edge_encoder.mlp_layer.2.bias", {Dt}, {Dp});
        const HostTensor *e4w = get("edge_encoder.mlp_layer.4.weight", {Et, Dt}, {Eh, Dp}), *e4b = get("edge_encoder.mlp_layer.4.bias", {Et}, {Eh});
        const HostTensor *elg = get("edge_layer_norm.weight", {Et}, {Eh}), *elb = get("edge_layer_norm.bias", {Et}, {Eh});
        const HostTensor *cen = expand ? get("edge_expand.centers", {40}, {40}) : nullptr;
        const HostTensor *lm = get("length_mean", {1}, {1}), *ls = get("length_std", {1}, {1});
        const HostTensor *d0w = get("graph_decoder.mlp_layer.0.weight", {Dt, Ht}, {Dp, H}), *d0b = get("graph_decoder.mlp_layer.0.bias", {Dt}, {Dp});
        const HostTensor *d2w = get("graph_decoder.mlp_layer.2.weight", {3, Dt}, {3, Dp}), *d2b = get("graph_decoder.mlp_layer.2.bias", {3}, {3});
        if (out.err) return false;
        // (hidden_dim above 128: the DT 128-row images of the first Linear side by side in one 64 KiB slot, the streamed blocks of
        //  W2 and W3 right behind it — k_edge_encode_wide_d walks them as one run)
        g.enc_w1p = bb.add(DT > 1 ? (size_t)WH_FRAG_FLOATS : (size_t)WH_ENC1_FLOATS);
        float* e1 = bb.host.data() + g.enc_w1p;
        if (DT > 1) for (int64_t b = 0; b < DT; ++b) pack_enc1(e0w->data.data() + (size_t)(128 * b * F), F, e1 + (size_t)b * WH_ENC1_FLOATS);
        else if (bf16_edges) pack_enc1_bf16(e0w->data.data(), F, reinterpret_cast<uint16_t*>(e1));
        else if (f16x3_edges) pack_enc1_f16x3(e0w->data.data(), F, reinterpret_cast<uint16_t*>(e1));
        else pack_enc1(e0w->data.data(), F, e1);
        // generic-width encoder in the reduced-precision modes: its two 128-wide GEMMs run in split-fp16 (wide.hip, e_format != 0)
        const bool enc_wide_f16 = rt.wide_enc && s.edge_dtype != GAMD_EDGE_F32;
        const bool lp128 = bf16_edges || f16x3_edges;
        g.enc_w2p = lp128 ? put_edge(e2w) : enc_wide_f16 ? put_blocks(e2w, 1, 1, block_f16x3) : put_blocks(e2w, DT, DT);
        HostTensor e4w_c = *e4w, e4b_c = *e4b;
        if (!bf16_edges && !f16x3_edges) { center_rows(*e4w, *e4b, e4w_c, e4b_c); }
        if (rt.ln_fold) {
            // the encoder needs |B x2 + c| only: R of B = Q R (its six all-zero blocks left out) and Q^T c take W3's and b3's places
            std::vector<double> Rm, cq;
            lnf_qr(fold_B, fold_c, Rm, cq);
            e4b_c.data = lnf_round(cq);
            e4w_c.data = lnf_round(Rm);
            g.enc_w3p = bb.add((size_t)LNF_R_FLOATS);
            lnf_pack_r(e4w_c.data.data(), bb.host.data() + g.enc_w3p);
        } else {
            g.enc_w3p = lp128 ? put_edge(e4w) : enc_wide_f16 ? put_blocks(&e4w_c, EHT, 1, block_f16x3) : put_blocks(&e4w_c, EHT, DT);
        }
        g.enc_b1 = put_vec(e0b); g.enc_b2 = put_vec(e2b); g.enc_b3 = put_vec(&e4b_c); g.enc_lng = put_vec(elg); g.enc_lnb = put_vec(elb);
        g.centers = expand ? put_vec(cen) : bb.add(64);
        g.dec_w1p = put_node(d0w, DT, HT); g.dec_b1 = put_vec(d0b); g.dec_w2 = put_vec(d2w); g.dec_b2 = put_vec(d2b);
        if (s.kind == GAMD_KIND_LJ) {
            const HostTensor* emb = get("node_emb", {1, Ht}, {1, H});
            if (!emb) return false;
            g.node_emb = put_vec(emb);
        } else {
            const HostTensor *nw = get("node_encoder.weight", {Ht, 1}, {H, 1}), *nb = get("node_encoder.bias", {Ht}, {H});
            if (out.err) return false;
            g.nenc_w = put_vec(nw); g.nenc_b = put_vec(nb);
        }
        out.length_mean = lm->data[0];
        out.length_std = ls->data[0];
        if (expand) out.rbf = rbf_grid(*cen);
        return true;
    }
};

// route: gamd_route(cfg, route_update_edge(weights)); a refused route comes back as the packing's refusal
inline bool route_update_edge(const std::map<std::string, HostTensor>& weights) { return weights.count("graph_conv.conv.0.edge_layer_norm.weight") != 0; }
inline PackedWeights pack_weights(const RouteConfig& cfg, const Route& route, int n_layers, const std::map<std::string, HostTensor>& weights) {
    return WeightPacker(cfg, route, n_layers, weights).run();
}

#pragma GCC visibility pop
