// gamd_ln_fold_host.h — host arithmetic of the folded edge LayerNorm: everything gamd_finalize_weights forms for
// it, in double, rounded once by the caller.  Plain C++ (no HIP header): tools/ln_fold_host_check.cpp builds it on its own
// under the host sanitizers.
//
// One edge: x2 = the encoder's second hidden activation, y = B x2 + c the centred output of its last Linear
// (B = C W_e3, c = C b_e3, C = I - 1 1^T / width), rstd = 1 / sqrt(|y|^2 / width + eps), e = gamma * y rstd + beta, and every
// conv layer starts with W1 e + b1.
//   * |y| is all the encoder needs of y: with B = Q R (Householder), |B x2 + c| = |R x2 + Q^T c|, and output block tp of the
//     upper-triangular R needs k >= 32 tp only (160 MFMAs per tile instead of 256).
//   * W1 e + b1 = A (rstd x2) + rstd a + b1',  A = W1 diag(gamma) B,  a = W1 (gamma * c),  b1' = b1 + W1 beta: the encoder
//     stores rstd x2 and rstd, the layer's first GEMM runs over A with one extra K step (rstd, 0) x (a, 0).
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

constexpr int LNF_W = 128;                         // block width of the 128-wide kernels
constexpr int LNF_R_BLOCKS = 10;                   // 32-row x 32-column blocks (tp, t >= tp) of R
constexpr int LNF_R_FLOATS = LNF_R_BLOCKS * 1024;  // packed R: 40 KiB
constexpr int LNF_A_FLOATS = LNF_W * LNF_W + 256;  // packed A + the fragment of the extra K step: 65 KiB

// B = C W, c = C b over the first `width` output rows (the true edge-embedding width; zero-padded rows stay zero).
// W: [128][128] row-major floats, b: [128]
inline void lnf_center(const float* W, const float* b, int width, std::vector<double>& B, std::vector<double>& c) {
    B.assign((size_t)LNF_W * LNF_W, 0.0);
    c.assign(LNF_W, 0.0);
    for (int k = 0; k < LNF_W; ++k) {
        double m = 0.0;
        for (int o = 0; o < width; ++o) m += (double)W[(size_t)o * LNF_W + k];
        m /= (double)width;
        for (int o = 0; o < width; ++o) B[(size_t)o * LNF_W + k] = (double)W[(size_t)o * LNF_W + k] - m;
    }
    double mb = 0.0;
    for (int o = 0; o < width; ++o) mb += (double)b[o];
    mb /= (double)width;
    for (int o = 0; o < width; ++o) c[o] = (double)b[o] - mb;
}

// Householder QR of B [128][128]: R (upper triangular, everything below the diagonal exactly zero) and cq = Q^T c.
// A column that is already zero below the diagonal (B has rank 127 at the most: its columns sum to zero) is left alone.
inline void lnf_qr(const std::vector<double>& B, const std::vector<double>& c, std::vector<double>& R, std::vector<double>& cq) {
    const int n = LNF_W;
    R = B;
    cq = c;
    std::vector<double> v(n);
    for (int j = 0; j < n; ++j) {
        double s = 0.0;
        for (int i = j; i < n; ++i) s += R[(size_t)i * n + j] * R[(size_t)i * n + j];
        const double nrm = std::sqrt(s);
        if (nrm > 0.0) {
            const double x0 = R[(size_t)j * n + j];
            const double alpha = x0 > 0.0 ? -nrm : nrm;
            double vv = 0.0;
            for (int i = j; i < n; ++i) { v[i] = R[(size_t)i * n + j]; if (i == j) v[i] -= alpha; vv += v[i] * v[i]; }
            if (vv > 0.0) {
                for (int k = j; k < n; ++k) {
                    double d = 0.0;
                    for (int i = j; i < n; ++i) d += v[i] * R[(size_t)i * n + k];
                    d *= 2.0 / vv;
                    for (int i = j; i < n; ++i) R[(size_t)i * n + k] -= d * v[i];
                }
                double d = 0.0;
                for (int i = j; i < n; ++i) d += v[i] * cq[i];
                d *= 2.0 / vv;
                for (int i = j; i < n; ++i) cq[i] -= d * v[i];
            }
        }
        for (int i = j + 1; i < n; ++i) R[(size_t)i * n + j] = 0.0;
    }
}

// One conv layer: A = W1 diag(gamma) B, a = W1 (gamma * c), b1f = b1 + W1 beta.  W1: [128][128] row-major floats.
inline void lnf_layer(const float* W1, const float* b1, const float* gamma, const float* beta, const std::vector<double>& B,
                      const std::vector<double>& c, std::vector<double>& A, std::vector<double>& a, std::vector<double>& b1f) {
    const int n = LNF_W;
    A.assign((size_t)n * n, 0.0);
    a.assign(n, 0.0);
    b1f.assign(n, 0.0);
    for (int r = 0; r < n; ++r) {
        double* row = A.data() + (size_t)r * n;
        double ar = 0.0, br = (double)b1[r];
        for (int i = 0; i < n; ++i) {
            const double w = (double)W1[(size_t)r * n + i];
            br += w * (double)beta[i];
            const double wg = w * (double)gamma[i];
            if (wg == 0.0) continue;
            ar += wg * c[i];
            const double* bi = B.data() + (size_t)i * n;
            for (int k = 0; k < n; ++k) row[k] += wg * bi[k];
        }
        a[r] = ar;
        b1f[r] = br;
    }
}

inline std::vector<float> lnf_round(const std::vector<double>& v) {
    std::vector<float> o(v.size());
    for (size_t i = 0; i < v.size(); ++i) o[i] = (float)v[i];
    return o;
}

// ---- fragment images (the order of gamd_common.h: lane (slot, half) of block (tp, t), group q holds
//      W[32 tp + slot][32 t + 8 q + 4 half + 0..3]) --------------------------------------------------------------------------
constexpr int lnf_r_block(int tp, int t) { return (tp == 0 ? 0 : tp == 1 ? 4 : tp == 2 ? 7 : 9) + (t - tp); }

template <bool UNPACK>
inline void lnf_block_copy(float* W, float* img, int tp, int t) {
    for (int q = 0; q < 4; ++q)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 4; ++j) {
                float& w = W[(size_t)(32 * tp + (lane & 31)) * LNF_W + 32 * t + 8 * q + 4 * (lane >> 5) + j];
                float& f = img[((size_t)q * 64 + lane) * 4 + j];
                if (UNPACK) w = f; else f = w;
            }
}

// R [128][128] -> the ten blocks with t >= tp, block (tp, t) at lnf_r_block(tp, t) * 1024 floats; the six blocks below the
// block diagonal (all zeros) are left out
inline void lnf_pack_r(const float* R, float* out) {
    for (int tp = 0; tp < 4; ++tp)
        for (int t = tp; t < 4; ++t) lnf_block_copy<false>(const_cast<float*>(R), out + (size_t)lnf_r_block(tp, t) * 1024, tp, t);
}
inline void lnf_unpack_r(const float* img, float* R) {
    for (int i = 0; i < LNF_W * LNF_W; ++i) R[i] = 0.f;
    for (int tp = 0; tp < 4; ++tp)
        for (int t = tp; t < 4; ++t) lnf_block_copy<true>(R, const_cast<float*>(img) + (size_t)lnf_r_block(tp, t) * 1024, tp, t);
}

// A [128][128], a [128] -> the 64 KiB image every 128 x 128 matrix has, then the extra K step's weight fragment: per output
// block tp 64 floats in lane order, lanes 0-31 a[32 tp + slot], lanes 32-63 zero
inline void lnf_pack_a(const float* A, const float* a, float* out) {
    for (int tp = 0; tp < 4; ++tp)
        for (int t = 0; t < 4; ++t) lnf_block_copy<false>(const_cast<float*>(A), out + (size_t)(tp * 4 + t) * 1024, tp, t);
    float* x = out + (size_t)LNF_W * LNF_W;
    for (int tp = 0; tp < 4; ++tp)
        for (int lane = 0; lane < 64; ++lane) x[tp * 64 + lane] = lane < 32 ? a[32 * tp + lane] : 0.f;
}
inline void lnf_unpack_a(const float* img, float* A, float* a) {
    for (int tp = 0; tp < 4; ++tp)
        for (int t = 0; t < 4; ++t) lnf_block_copy<true>(A, const_cast<float*>(img) + (size_t)(tp * 4 + t) * 1024, tp, t);
    const float* x = img + (size_t)LNF_W * LNF_W;
    for (int tp = 0; tp < 4; ++tp)
        for (int s = 0; s < 32; ++s) a[32 * tp + s] = x[tp * 64 + s];
}
