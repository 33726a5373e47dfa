// ln_fold_host_check.cpp — the host arithmetic of the folded edge LayerNorm (gamd_amd/csrc/gamd_ln_fold_host.h) on seeded
// 128 x 128 weights, as a stand-alone program for the host sanitizers (tests/test_ln_fold_host.py builds it with
// -fsanitize=address,undefined).  Checks, all in double:
//   * the six blocks of R below the block diagonal are exactly zero;
//   * |R x + c_q| = |B x + c| to 1e-12, relative;
//   * the staged first-GEMM pre-activation W1 (gamma * y rstd + beta) + b1 and the folded one A (rstd x) + rstd a + b1' agree
//     to 1e-12 of the largest value;
//   * the packed images of R and of (A, a) round-trip, the left-out blocks as zeros.
// Prints one line per check and "ln_fold_host_check: ok".
#include "../gamd_amd/csrc/gamd_ln_fold_host.h"

#include <cstdint>
#include <cstdio>

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uniform() {                       // splitmix64 -> (-1, 1)
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

static int check(int width, int n_rows) {
    const int n = LNF_W;
    const double bound = 1.0 / std::sqrt((double)n);            // nn.Linear's initial scale
    std::vector<float> W3((size_t)n * n, 0.f), b3(n, 0.f), W1((size_t)n * n), b1(n), gamma(n, 0.f), beta(n, 0.f);
    for (int o = 0; o < width; ++o) {
        for (int k = 0; k < n; ++k) W3[(size_t)o * n + k] = (float)(bound * uniform());
        b3[o] = (float)(bound * uniform());
        gamma[o] = (float)(1.0 + 0.3 * uniform());
        beta[o] = (float)(0.2 * uniform());
    }
    for (auto& v : W1) v = (float)(bound * uniform());
    for (auto& v : b1) v = (float)(bound * uniform());

    std::vector<double> B, c, R, cq, A, a, b1f;
    lnf_center(W3.data(), b3.data(), width, B, c);
    lnf_qr(B, c, R, cq);
    lnf_layer(W1.data(), b1.data(), gamma.data(), beta.data(), B, c, A, a, b1f);

    // 1. the skipped blocks
    for (int tp = 1; tp < 4; ++tp)
        for (int i = 32 * tp; i < 32 * tp + 32; ++i)
            for (int k = 0; k < 32 * tp; ++k)
                if (R[(size_t)i * n + k] != 0.0) { std::printf("R[%d][%d] = %g below the block diagonal\n", i, k, R[(size_t)i * n + k]); return 1; }
    std::printf("width %d: skipped blocks of R are zero\n", width);

    // 2., 3. norms and pre-activations on random rows (GELU outputs: mostly positive, some slightly negative)
    double worst_norm = 0.0, worst_pre = 0.0, scale_pre = 0.0;
    std::vector<double> x(n), y(n), z(n), st(n), fo(n);
    for (int row = 0; row < n_rows; ++row) {
        for (int k = 0; k < n; ++k) { const double u = uniform(); x[k] = u > -0.6 ? 1.5 * (u + 0.6) : 0.17 * u; }
        double ny = 0.0, nz = 0.0;
        for (int i = 0; i < n; ++i) {
            double sy = c[i], sz = cq[i];
            for (int k = 0; k < n; ++k) { sy += B[(size_t)i * n + k] * x[k]; sz += R[(size_t)i * n + k] * x[k]; }
            y[i] = sy; z[i] = sz; ny += sy * sy; nz += sz * sz;
        }
        ny = std::sqrt(ny); nz = std::sqrt(nz);
        worst_norm = std::fmax(worst_norm, std::fabs(ny - nz) / ny);
        const double rstd = 1.0 / std::sqrt(ny * ny / (double)width + 1e-5);
        for (int r = 0; r < n; ++r) {
            double s = b1[r], f = b1f[r] + rstd * a[r];
            for (int i = 0; i < n; ++i) {
                s += (double)W1[(size_t)r * n + i] * ((double)gamma[i] * y[i] * rstd + (double)beta[i]);
                f += A[(size_t)r * n + i] * (rstd * x[i]);
            }
            st[r] = s; fo[r] = f;
            scale_pre = std::fmax(scale_pre, std::fabs(s));
            worst_pre = std::fmax(worst_pre, std::fabs(s - f));
        }
    }
    std::printf("width %d: |R x + cq| against |B x + c|: %.3e relative; folded against staged pre-activation: %.3e of max|value|\n",
                width, worst_norm, worst_pre / scale_pre);
    if (!(worst_norm <= 1e-12) || !(worst_pre <= 1e-12 * scale_pre)) { std::printf("above 1e-12\n"); return 1; }

    // 4. the images
    const std::vector<float> Rf = lnf_round(R), Af = lnf_round(A), af = lnf_round(a);
    std::vector<float> rimg(LNF_R_FLOATS, -1.f), aimg(LNF_A_FLOATS, -1.f), R2((size_t)n * n, -1.f), A2((size_t)n * n, -1.f), a2(n, -1.f);
    lnf_pack_r(Rf.data(), rimg.data());
    lnf_unpack_r(rimg.data(), R2.data());
    lnf_pack_a(Af.data(), af.data(), aimg.data());
    lnf_unpack_a(aimg.data(), A2.data(), a2.data());
    for (float v : rimg) if (v == -1.f) { std::printf("packed R has an unwritten element\n"); return 1; }
    for (float v : aimg) if (v == -1.f) { std::printf("packed A has an unwritten element\n"); return 1; }
    if (R2 != Rf || A2 != Af || a2 != af) { std::printf("a packed image does not round-trip\n"); return 1; }
    for (int tp = 0; tp < 4; ++tp)
        for (int lane = 32; lane < 64; ++lane)
            if (aimg[(size_t)n * n + tp * 64 + lane] != 0.f) { std::printf("extra K step: upper lanes not zero\n"); return 1; }
    // a lane's float4 of block (tp, t), group q is where the kernels read it
    for (int tp = 0; tp < 4; ++tp)
        for (int t = tp; t < 4; ++t)
            for (int q = 0; q < 4; ++q)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j)
                        if (rimg[(((size_t)lnf_r_block(tp, t) * 4 + q) * 64 + lane) * 4 + j] !=
                            Rf[(size_t)(32 * tp + (lane & 31)) * n + 32 * t + 8 * q + 4 * (lane >> 5) + j]) { std::printf("R image order\n"); return 1; }
    std::printf("width %d: packed images round-trip\n", width);
    return 0;
}

int main() {
    if (check(128, 4096)) return 1;
    if (check(96, 256)) return 1;           // a narrower edge embedding: zero-padded rows of W_e3, gamma, beta
    std::printf("ln_fold_host_check: ok\n");
    return 0;
}
