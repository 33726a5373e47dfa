// weights_host_check.cpp — weight transformation and packing (gamd_amd/csrc/gamd_weights_host.h) without a device, as a
// stand-alone program for the host sanitizers (tests/test_weights_host.py builds it with -fsanitize=address,undefined).
//   weights_host_check pack  <case file> <blob file>   run pack_weights, write the blob, print the canonical table
//   weights_host_check arith <case file>               the same, then the host arithmetic of whatever this configuration
//                                                      forms against a naive restatement in double; "arith: ok" at the end
// Case file (little endian): 16 int32 — kind, edge_dtype, no_expand_edge, self_loop_mode, kernel_select, n_layers, n_feat, the
// three true and the three padded widths, and wide_enc, wide_conv, ln_fold as the writer expects gamd_create to decide them —,
// int32 tensor count, then per tensor int32 name length, the name, int32 ndim, int64 dims, float32 data.  The configuration is
// read back out of the first ten; the widths and flags the route (gamd_route_host.h) derives from it must then be the file's.
// Table: "blob <floats>", "flags ...", "scalars ..." (bit patterns), one "layer <l> name=offset ..." per layer and "global ...",
// offsets in floats as the device pointers see them (node.wpep of a hoisted layer 0 is M0), -1 for a null pointer; a refusal
// prints "error <code> <text>" instead.
#include "../gamd_amd/csrc/gamd_weights_host.h"

#include <cinttypes>

struct Case { RouteConfig cfg; int n_layers = 0; };
static bool read_case(const char* path, Case& c, std::map<std::string, HostTensor>& w) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    int32_t v[16], n = 0;
    bool ok = std::fread(v, 4, 16, f) == 16 && std::fread(&n, 4, 1, f) == 1;
    if (ok) {
        RouteConfig& s = c.cfg;
        s.kind = v[0]; s.edge_dtype = v[1]; s.no_expand_edge = v[2]; s.self_loop_mode = v[3]; s.kernel_select = v[4];
        c.n_layers = v[5]; s.use_bond = v[6] & 1;                  // n_feat: 44 or 4, + 1 with bonds
        s.encoding_size = v[7]; s.edge_embedding_dim = v[8]; s.hidden_dim = v[9];
        s.keep_stages = gamd_route(s, false).ln_fold && !v[15];   // the one thing a configuration can add to keep the fold off
        const Route r = gamd_route(s, false);
        const int derived[9] = {r.n_feat, r.H_true, r.Eh_true, r.D_true, r.H, r.Eh, r.Dp, (int)r.wide_enc, (int)r.wide_conv};
        ok = !r.err && std::equal(derived, derived + 9, v + 6) && (int)r.ln_fold == v[15];
        if (!ok) std::fprintf(stderr, "the case file's widths and flags are not what gamd_route derives from its configuration\n");
    }
    for (int32_t i = 0; ok && i < n; ++i) {
        int32_t len = 0, ndim = 0;
        ok = std::fread(&len, 4, 1, f) == 1 && len > 0 && len < 256;
        std::string name((size_t)(ok ? len : 0), ' ');
        ok = ok && std::fread(&name[0], 1, (size_t)len, f) == (size_t)len && std::fread(&ndim, 4, 1, f) == 1 && ndim >= 1 && ndim <= 2;
        HostTensor t;
        size_t cnt = 1;
        for (int d = 0; ok && d < ndim; ++d) {
            int64_t e = 0;
            ok = std::fread(&e, 8, 1, f) == 1 && e >= 0 && e <= 4096;
            t.shape.push_back(e);
            cnt *= (size_t)e;
        }
        if (ok) { t.data.resize(cnt); ok = std::fread(t.data.data(), 4, cnt, f) == cnt; }
        if (ok) w[name] = std::move(t);
    }
    std::fclose(f);
    return ok;
}

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static long long shown(size_t off) { return off == WOFF_NONE ? -1 : (long long)off; }

static void print_table(const Route& r, const PackedWeights& p) {
    std::printf("blob %zu\n", p.blob.size());
    std::printf("flags update_edge=%d norm_bn=%d l0_hoist=%d node_f16=%d wide_enc=%d wide_conv=%d ln_fold=%d\n", (int)r.update_edge,
                (int)p.norm_bn, (int)r.l0_hoist, (int)r.node_f16, (int)r.wide_enc, (int)r.wide_conv, (int)r.ln_fold);
    std::printf("scalars length_mean=%08x length_std=%08x rbf=%d,%08x,%08x,%08x,%08x,%08x\n", bits(p.length_mean), bits(p.length_std),
                p.rbf.uniform, bits(p.rbf.c0), bits(p.rbf.delta), bits(p.rbf.A), bits(p.rbf.B), bits(p.rbf.C));
    for (size_t l = 0; l < p.layers.size(); ++l) {
        LayerOff o = p.layers[l];
        if (o.m0 != WOFF_NONE) o.node.wpep = o.m0;
        std::printf("layer %zu", l);
#define SHOW(f) std::printf(" " #f "=%lld", shown(o.f));
        GAMD_W_LAYER_FIELDS(SHOW)
#undef SHOW
#define SHOW(f) std::printf(" " #f "=%lld", shown(o.node.f));
        GAMD_W_NODE_FIELDS(SHOW)
#undef SHOW
        std::printf("\n");
    }
    std::printf("global");
#define SHOW(f) std::printf(" " #f "=%lld", shown(p.g.f));
    GAMD_W_GLOBAL_FIELDS(SHOW)
#undef SHOW
    std::printf("\n");
}

// ---- the host arithmetic, restated naively --------------------------------------------------------------------------------
static int g_bad = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { std::printf("arith: FAILED %s\n", what); ++g_bad; }
}

// where element (n, k) of a 128x128 block lands in its pack128 / pack16 image: pack a matrix of indices and invert
template <class Pack> static std::vector<int> image_position(Pack pack) {
    std::vector<float> idx(128 * 128), img(128 * 128, -1.f);
    for (int i = 0; i < 128 * 128; ++i) idx[(size_t)i] = (float)i;
    pack(idx.data(), img.data(), 128);
    std::vector<int> pos(128 * 128, -1);
    for (int i = 0; i < 128 * 128; ++i) pos[(size_t)img[(size_t)i]] = i;
    return pos;
}
// the [128 OB][128 KB] matrix back out of its run of pack128 blocks
static std::vector<float> unpack_blocks(const float* img, int OB, int KB, const std::vector<int>& pos) {
    std::vector<float> m((size_t)OB * KB * 128 * 128);
    for (int ob = 0; ob < OB; ++ob)
        for (int kb = 0; kb < KB; ++kb)
            for (int n = 0; n < 128; ++n)
                for (int k = 0; k < 128; ++k)
                    m[(size_t)(128 * ob + n) * 128 * KB + 128 * kb + k] = img[(size_t)(ob * KB + kb) * WH_FRAG_FLOATS + pos[(size_t)n * 128 + k]];
    return m;
}
static bool zero_outside(const std::vector<float>& m, int rows, int cols, int rows_true, int cols_true) {
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c)
            if ((r >= rows_true || c >= cols_true) && bits(m[(size_t)r * cols + c]) != 0) return false;
    return true;
}

static void check_permute_f2() {
    HostTensor w, b, wo, bo;
    w.shape = {128, 128}; w.data.resize(128 * 128);
    b.shape = {128}; b.data.resize(128);
    for (int r = 0; r < 128; ++r) {
        b.data[(size_t)r] = (float)r;
        for (int k = 0; k < 128; ++k) w.data[(size_t)r * 128 + k] = (float)(1000 * r + k);
    }
    permute_f2(w, b, wo, bo);
    bool ok = true;
    std::vector<int> seen(128, 0);
    for (int q = 0; q < 4; ++q)
        for (int s = 0; s < 32; ++s) {
            ok = ok && bo.data[(size_t)(32 * q + s)] == (float)(4 * s + q);
            for (int k = 0; k < 128; ++k) ok = ok && wo.data[(size_t)(32 * q + s) * 128 + k] == (float)(1000 * (4 * s + q) + k);
            ++seen[(size_t)bo.data[(size_t)(32 * q + s)]];
        }
    for (int r = 0; r < 128; ++r) ok = ok && seen[(size_t)r] == 1;
    expect(ok, "permute_f2: row 32 q + s <- row 4 s + q, a permutation");
    std::printf("arith: permute_f2 is the permutation 32 q + s <- 4 s + q\n");
}

static int arith(const Case& s, const Route& r, const std::map<std::string, HostTensor>& w, const PackedWeights& p) {
    const int H = r.H, Ht = r.H_true, Eh = r.Eh, Et = r.Eh_true, Dp = r.Dp, Dt = r.D_true, HT = r.HT, EHT = r.EHT, DT = r.DT;
    const float* B = p.blob.data();
    const std::vector<int> pos128 = image_position([](const float* W, float* o, int ld) { pack128(W, o, ld); });
    const std::vector<int> pos16 = image_position([](const float* W, float* o, int ld) { pack16(W, o, ld); });
    check_permute_f2();
    auto T = [&](const std::string& n) -> const std::vector<float>& { return w.at(n).data; };

    // 1. eval-mode BatchNorm: alpha = weight / sqrt(running_var + eps), beta = bias - running_mean * alpha, in float
    if (p.norm_bn) {
        bool ok = true;
        for (int l = 0; l < s.n_layers; ++l) {
            const std::string n = "graph_conv.norm_layers." + std::to_string(l);
            const auto &g = T(n + ".weight"), &b = T(n + ".bias"), &rm = T(n + ".running_mean"), &rv = T(n + ".running_var");
            for (int i = 0; i < H; ++i) {
                float al = 0.f, be = 0.f;
                if (i < Ht) { al = g[(size_t)i] * (1.0f / std::sqrt(rv[(size_t)i] + 1e-5f)); be = b[(size_t)i] - rm[(size_t)i] * al; }
                ok = ok && bits(B[p.layers[(size_t)l].node.ln_g + (size_t)i]) == bits(al) && bits(B[p.layers[(size_t)l].node.ln_b + (size_t)i]) == bits(be);
            }
        }
        expect(ok, "BatchNorm alpha / beta bit-equal to the float formula");
        std::printf("arith: BatchNorm alpha / beta of %d layers bit-equal to the float formula\n", s.n_layers);
    }

    // 2. layer-0 form: M0 = W_pe diag(hn0) W4, c0 = W_pe (hn0 * b4) as a plain triple loop in double, rounded once
    if (r.l0_hoist) {
        const auto &emb = T("node_emb"), &pe = T("graph_conv.conv.0.phi_edge.weight"), &w4 = T("graph_conv.conv.0.theta_edge.mlp_layer.3.weight"),
                   &b4 = T("graph_conv.conv.0.theta_edge.mlp_layer.3.bias");
        std::vector<double> hn0((size_t)Ht);
        const float *g = B + p.layers[0].node.ln_g, *b = B + p.layers[0].node.ln_b;       // (BatchNorm: alpha, beta as checked above)
        if (p.norm_bn) {
            for (int i = 0; i < Ht; ++i) hn0[(size_t)i] = (double)emb[(size_t)i] * g[i] + b[i];
        } else {
            double mean = 0.0, var = 0.0;
            for (int i = 0; i < Ht; ++i) mean += emb[(size_t)i];
            mean /= Ht;
            for (int i = 0; i < Ht; ++i) var += (emb[(size_t)i] - mean) * (emb[(size_t)i] - mean);
            var /= Ht;
            for (int i = 0; i < Ht; ++i) hn0[(size_t)i] = (emb[(size_t)i] - mean) * (1.0 / std::sqrt(var + 1e-5)) * g[i] + b[i];
        }
        const float *m0 = B + p.layers[0].m0, *c0 = B + p.layers[0].node.c0;
        bool ok = true;
        for (int r = 0; r < 128; ++r) {
            double c = 0.0;
            for (int i = 0; i < Ht && r < Dt; ++i) c += ((double)pe[(size_t)r * Ht + i] * hn0[(size_t)i]) * b4[(size_t)i];
            ok = ok && bits(c0[r]) == bits(r < Dt ? (float)c : 0.f);
            for (int k = 0; k < 128; ++k) {
                double m = 0.0;
                for (int i = 0; i < Ht && r < Dt && k < Dt; ++i) m += ((double)pe[(size_t)r * Ht + i] * hn0[(size_t)i]) * w4[(size_t)i * Dt + k];
                ok = ok && m0[pos16[(size_t)r * 128 + k]] == (float)m;
            }
        }
        expect(ok, "M0 / c0 equal to the rounded triple loop in double");
        std::printf("arith: M0 and c0 equal the float rounding of a triple loop in double\n");
    }

    // 3. the centred last encoder Linear (fp32 kernels without the fold): columns of W' and b' sum to 0 over the true rows
    const bool fp32_blocks = r.f32 && !r.ln_fold;
    if (fp32_blocks) {
        const std::vector<float> w3 = unpack_blocks(B + p.g.enc_w3p, EHT, DT, pos128);
        const float* b3 = B + p.g.enc_b3;
        double big = 0.0, worst = 0.0, sb = 0.0, bigb = 0.0;
        for (int o = 0; o < Et; ++o) { sb += b3[o]; bigb = std::fmax(bigb, std::fabs((double)b3[o])); }
        for (int k = 0; k < Dp; ++k) {
            double sum = 0.0;
            for (int o = 0; o < Et; ++o) { sum += w3[(size_t)o * Dp + k]; big = std::fmax(big, std::fabs((double)w3[(size_t)o * Dp + k])); }
            worst = std::fmax(worst, std::fabs(sum));
        }
        auto ulp = [](double x) { return std::ldexp(1.0, std::ilogb(x) - 23); };      // of an fp32 value of that size
        expect(worst <= 128 * ulp(big) && std::fabs(sb) <= 128 * ulp(bigb), "centred W_e3 / b_e3 sum to 0 within 128 ulps of the largest entry");
        bool pad = zero_outside(w3, Eh, Dp, Et, Dt);
        for (int o = Et; o < Eh; ++o) pad = pad && bits(b3[o]) == 0;
        expect(pad, "centred W_e3 / b_e3: padded rows exactly zero");
        std::printf("arith: centred W_e3: worst column sum %.3e, bias sum %.3e (largest entries %.3e, %.3e); padded rows zero\n", worst, std::fabs(sb), big, bigb);
    }

    // 4. zero padding of every padded tensor, where all of them are fp32 block images: the generic-width fp32 kernels
    if (fp32_blocks && r.wide_conv) {
        bool ok = true;
        auto vec = [&](size_t off, int n, int n_true) { for (int i = n_true; i < n; ++i) ok = ok && bits(B[off + (size_t)i]) == 0; };
        auto mat = [&](size_t off, int OB, int KB, int rt, int ct) { ok = ok && zero_outside(unpack_blocks(B + off, OB, KB, pos128), 128 * OB, 128 * KB, rt, ct); };
        for (const LayerOff& o : p.layers) {
            mat(o.w1p, 1, EHT, 128, Et); mat(o.w2p, DT, 1, Dt, 128); mat(o.w3p, DT, DT, Dt, Dt); mat(o.w4p, HT, DT, Ht, Dt);
            vec(o.b3, Dp, Dt); vec(o.b4, H, Ht); vec(o.node.ln_g, H, Ht); vec(o.node.ln_b, H, Ht); vec(o.node.bS, Dp, Dt); vec(o.node.bP, Dp, Dt);
            vec(o.node.bphi, H, Ht);
            if (o.e_ln_g != WOFF_NONE) { vec(o.e_ln_g, Eh, Et); vec(o.e_ln_b, Eh, Et); }
            mat(o.node.wsp, DT, HT, Dt, Ht); mat(o.node.wdp, DT, HT, Dt, Ht); mat(o.node.wpdp, DT, HT, Dt, Ht); mat(o.node.wpep, DT, HT, Dt, Ht);
            mat(o.node.wphip, HT, DT, Ht, Dt);
        }
        mat(p.g.enc_w2p, DT, DT, Dt, Dt); mat(p.g.dec_w1p, DT, HT, Dt, Ht);
        vec(p.g.enc_b1, Dp, Dt); vec(p.g.enc_b2, Dp, Dt); vec(p.g.enc_lng, Eh, Et); vec(p.g.enc_lnb, Eh, Et); vec(p.g.dec_b1, Dp, Dt);
        for (int r = 0; r < 3; ++r) vec(p.g.dec_w2 + (size_t)r * Dp, Dp, Dt);
        if (p.g.node_emb != WOFF_NONE) vec(p.g.node_emb, H, Ht);
        if (p.g.nenc_w != WOFF_NONE) { vec(p.g.nenc_w, H, Ht); vec(p.g.nenc_b, H, Ht); }
        expect(ok, "padded rows and columns are exact zeros");
        std::printf("arith: padded rows and columns of every padded tensor are exact zeros (%d/%d/%d in %d/%d/%d)\n", Ht, Dt, Et, H, Dp, Eh);
    }
    if (g_bad) return 1;
    std::printf("arith: ok\n");
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (!((mode == "pack" && argc == 4) || (mode == "arith" && argc == 3))) {
        std::fprintf(stderr, "usage: weights_host_check pack <case file> <blob file> | arith <case file>\n");
        return 2;
    }
    Case c;
    std::map<std::string, HostTensor> w;
    if (!read_case(argv[2], c, w)) { std::fprintf(stderr, "cannot read case file %s\n", argv[2]); return 2; }
    const Route r = gamd_route(c.cfg, route_update_edge(w));
    const PackedWeights p = pack_weights(c.cfg, r, c.n_layers, w);
    if (p.err) { std::printf("error %d %s\n", p.err, p.msg); return 0; }
    print_table(r, p);
    if (mode == "arith") return arith(c, r, w, p);
    FILE* f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(p.blob.data(), sizeof(float), p.blob.size(), f) != p.blob.size()) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    std::fclose(f);
    return 0;
}
