"""Operand-rounded stage functions for the reduced-precision edge kernels.

TEST INFRASTRUCTURE ONLY (the rules of gamd_oracle.py apply: tests/ may import it, the product package never does).

The bf16 edge kernels are fully specified arithmetic: MFMA operands rounded to bf16 (round to nearest even), fp32
accumulation, fp16 node tables in the 128-wide family, log2 e / ln 2 folded into the packed weights.  The functions
here restate one kernel each in plain PyTorch and round at the same points; everything else runs in the dtype of the
inputs (float64 weights and inputs give a float64 run, float32 an fp32 run).  A correct kernel then differs from the
float64 run only by fp32 accumulation noise, 1-ulp hardware transcendentals and the few elements where that noise flips
a rounding decision -- which is what tests/test_gpu_lp_stages.py measures, kernel by kernel, on device-produced inputs.

Every rounding point cites the kernel or packing line it restates (paths relative to gamd_amd/csrc).

variant "bf16_128"  edge_encode_bf16.hip, conv_edge_bf16.hip, k_node with NodeArgs::tab16 (128 / 128 / 128, RBF expanded)
variant "bf16_wide" wide.hip's k_edge_encode_wide (e_format 1), wide_lp.hip's k_conv_edge_bf16_wide, fp32 node tables
variant None        no rounding: gamd_oracle's own operations, in its own order

The fp32-grade families are restated the same way, so that their kernels are judged one by one as well:

variant "f32"        every fp32 kernel (edge_encode.hip, conv_edge.hip, conv_edge_small.hip, wide.hip, wide16.hip, wide_d.hip, node.hip):
                     the plain operations with the kernels' GELU fit and the host's fp32-folded eval BatchNorm
variant "f16x3_128"  edge_encode_f16x3.hip, conv_edge_f16x3.hip, k_node<true> (128 / 128 / 128, RBF expanded): operand-split GEMMs
variant "f16x3_wide" wide.hip's k_edge_encode_wide (e_format 2), wide_lp.hip's k_conv_edge_f16x3_wide, k_node_wide<HT, true>

Operand split (gamd_f16x3.h): an MFMA operand x is hi = fp16(x), lo = fp16(x - hi), round to nearest even, subnormals kept, the
residual formed in fp32 (gamd_split8, silu_split_pair, node.hip split16; host: split_f16 in gamd_weights_host.h); a product is
W_hi x_hi + (W_hi x_lo + W_lo x_hi), the lo x lo term is dropped.  Weights are split as the host packs them (no factors in these
families), activations where the kernel splits them.  The model has no overflow path: tests/test_lp_reference.py holds every
operand of every split case below 65504 (`operand_log`).

The encoders' GELU is the kernels' own fit (gelu_fit, coefficients copied from gamd_common.h), not the erf form: its relative
error for negative arguments is a hundred fp32 epsilons and lands in front of a bf16 rounding.  This costs independence: the
encoder check cannot see an error of the fit itself.  That the fit is the header's and within its stated distance of erf is
held by tests/test_lp_reference.py and tests/test_host_logic.py; Spec.gelu = "erf" gives the reference the exact form, to
measure what the fit costs.

A `Spec` may be passed wherever a variant name is accepted; its extra fields switch single rounding points the wrong way
(the mutations of tests/test_lp_reference.py) and are not part of any kernel's description.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Dict, Optional, Tuple, Union

import torch
import torch.nn.functional as F

import gamd_oracle as orc

Tensor = torch.Tensor

LOG2E = 1.4426950408889634      # gamd_weights_host.h, scale_for_exp2: `const double LOG2E = ..., LN2 = ...`
LN2 = 0.6931471805599453


@dataclass(frozen=True)
class Spec:
    family: str                          # "bf16_128" | "bf16_wide" | "f32" | "f16x3_128" | "f16x3_wide"
    # ---- the switches below describe WRONG kernels (mutation tests); the defaults are the kernels as written ----
    bf16_mode: str = "rne"               # "trunc": activations cut to bf16 instead of rounded (weights stay as the host packs them)
    fp16_tables: bool = True             # False: hn / S / D of the 128-wide family kept unrounded
    scale_then_round: bool = True        # False: weights rounded to bf16 BEFORE the log2 e / ln 2 factors
    drop_w4_kstep: Optional[Tuple[int, int, int]] = None   # (t, u, half): that K step of W4 (8 input features) contributes nothing
    drop_bond: bool = False              # feature column 44 (the bond flag) contributes nothing
    gelu: str = "fit"                    # "erf": the exact form in place of the kernels' fit (gelu_fit) -- what the fit costs
    folded_norm: bool = True             # False: F.batch_norm in place of the host's fp32-folded affine map (with gelu = "erf" the
                                         # "f32" family is then gamd_oracle itself)
    # ---- wrong fp32-grade kernels ----
    silu_err: Optional[Tuple[int, int, float]] = None      # (layer, k, rel): the k-th SiLU (0, 1, 2) of that conv layer's edge MLP is
                                                           # off by rel relative, systematic, sign following the argument
    flush_lo_subnormal: bool = False     # split model: lo halves that are fp16-subnormal become zero
    drop_wlo_kstep: Optional[Tuple[int, int, int, int]] = None   # (layer, g, t, u): W_lo x_hi of K step (t, u) -- 16 input features --
                                                                 # of the g-th GEMM (0 .. 3) of that conv layer's edge MLP is missing


VARIANTS = {k: Spec(k) for k in ("bf16_128", "bf16_wide", "f32", "f16x3_128", "f16x3_wide")}
FP32_GRADE = ("f32", "f16x3_128", "f16x3_wide")
Variant = Union[None, str, Spec]


def spec_of(variant: Variant) -> Optional[Spec]:
    if variant is None or isinstance(variant, Spec):
        return variant
    return VARIANTS[variant]


# --------------------------------------------------------------------------
# rounding
# --------------------------------------------------------------------------
def round_bf16(x: Tensor, mode: str = "rne") -> Tensor:
    """The value as the nearest bf16 (ties to even: v_cvt_pk_bf16_f32, gamd_bf16.h gamd_pk_bf16; host: f2bf in gamd_weights_host.h),
    in x's dtype.  The kernels round fp32 values, so a float64 input is taken to fp32 first."""
    x32 = x.to(torch.float32)
    if mode == "rne":
        y = x32.to(torch.bfloat16).to(torch.float32)
    elif mode == "trunc":
        y = (x32.contiguous().view(torch.int32) & -65536).view(torch.float32)
    else:
        raise ValueError(mode)
    return y.to(x.dtype)


def round_fp16(x: Tensor) -> Tensor:
    """fp32 -> fp16, ties to even, subnormals kept (node.hip cvt16x4)."""
    return x.to(torch.float32).to(torch.float16).to(x.dtype)


operand_log: Optional[list] = None      # a list: split_fp16 appends the largest magnitude of every operand it splits


def split_fp16(x: Tensor, sp: Optional[Spec] = None) -> Tuple[Tensor, Tensor]:
    """(hi, lo) of gamd_f16x3.h in x's dtype: hi = fp16(x), lo = fp16(x - hi).  The kernels split fp32 values (gamd_split8:
    `r = x - convertvector(h)` in fp32, exact there), so a float64 input is taken to fp32 first; both conversions round to
    nearest even and keep subnormals (v_cvt_pk_f16_f32 under the kernels' default mode; torch's CPU conversion does the same)."""
    x32 = x.to(torch.float32)
    if operand_log is not None and x32.numel():
        operand_log.append(float(x32.abs().max()))
    hi = x32.to(torch.float16).to(torch.float32)
    lo = (x32 - hi).to(torch.float16).to(torch.float32)
    if sp is not None and sp.flush_lo_subnormal:
        lo = torch.where(lo.abs() < 2.0 ** -14, torch.zeros_like(lo), lo)          # mutation
    return hi.to(x.dtype), lo.to(x.dtype)


def linear_x3(x: Tensor, w: Tensor, b: Optional[Tensor] = None, sp: Optional[Spec] = None, drop_wlo=None) -> Tensor:
    """x W^T (+ b) as gamd_f16x3_step / gemm128_f16x3_lazy / node.hip gemm16_half_f16 evaluate it: three MFMAs per K step in the
    order W_hi x_lo, W_lo x_hi, W_hi x_hi, accumulated in fp32 (here: in x's dtype); the bias is the accumulator's start and
    stays fp32.  `drop_wlo`: input features whose W_lo x_hi term is missing (mutation)."""
    xh, xl = split_fp16(x, sp)
    wh, wl = split_fp16(w, sp)
    if drop_wlo is not None:
        wl = wl.clone()
        wl[:, drop_wlo] = 0
    y = (F.linear(xl, wh) + F.linear(xh, wl)) + F.linear(xh, wh)
    return y if b is None else y + b


def bf16_bits(x) -> Tensor:
    """int32 bit patterns of bf16-representable values (the upper 16 bits of their fp32 form)."""
    x32 = torch.as_tensor(x).to(torch.float32).contiguous()
    return x32.view(torch.int32) >> 16


def kstep_features(t: int, u: int, half: int):
    """The 8 input features that lane half `half` feeds to K step (t, u) of a 128-wide bf16 GEMM (gamd_bf16.h:
    feat(t, r, half) = 32 t + (r & 3) + 8 (r >> 2) + 4 half, r = 8 u .. 8 u + 7)."""
    return [32 * t + (r & 3) + 8 * (r >> 2) + 4 * half for r in range(8 * u, 8 * u + 8)]


def _host_scaled(w: Tensor, f: float) -> Tensor:
    """gamd_finalize_weights' `scaled`: (float)((double)v * f) -- an fp32 value, whatever the working dtype."""
    return (w.double() * f).to(torch.float32)


def _packed(w: Tensor, factor: Optional[float], sp: Spec, dtype) -> Tensor:
    """A GEMM weight as the bf16 kernels hold it: the packing-time factor applied in double and rounded to fp32, THEN bf16
    (pack128_bf16 / pack_enc1_bf16 round what `scaled` left).  The result is exact in every working dtype."""
    w32 = w.to(torch.float32)
    if factor is None:
        return round_bf16(w32).to(dtype)
    if sp.scale_then_round:
        return round_bf16(_host_scaled(w32, factor)).to(dtype)
    return _host_scaled(round_bf16(w32), factor).to(dtype)          # mutation: rounded first, scaled after


# gamd_common.h GAMD_GELU_Q0 .. Q6 (tests/test_lp_reference.py holds the copy to the header)
GELU_Q = (-9.999880791e-01, -1.151242852e+00, -4.586574435e-01, -5.355345458e-02, 8.167289197e-03, -7.945232792e-04, 3.589583139e-05)


def gelu_fit(x: Tensor) -> Tensor:
    """GELU as every kernel evaluates it (gamd_common.h gamd_gelu_hw / gelu_pair): max(x, 0) - a 2^Q(a), a = min(|x|, 6), Q the
    degree-6 fit of log2 Phi(-a) with fp32 coefficients, Horner from Q6 down.  Against the exact erf form it is off by at most
    1.2e-7 ABSOLUTE (tests/test_host_logic.py) -- but Q(0) = -0.99998808, not -1, so for x < 0, where the tail is the whole
    result, by up to 8e-6 RELATIVE: a hundred fp32 epsilons, and in the bf16 encoder the result is rounded to bf16 at once.  The
    fit is therefore part of a bf16 kernel's specified arithmetic, like the 2^-x form of its SiLU, and the reference of a bf16
    variant evaluates it (in the working dtype); a reference with the erf form flips 20 times as many roundings of e as the
    kernel's own noise does (profiles/lp_stage_parity.md)."""
    a = x.abs().clamp(max=6.0)
    q = torch.full_like(a, float(torch.tensor(GELU_Q[6], dtype=torch.float32)))
    for c in GELU_Q[5::-1]:
        q = q * a + float(torch.tensor(c, dtype=torch.float32))
    return x.clamp(min=0.0) - a * torch.exp2(q)


def _silu_exp2(x: Tensor) -> Tensor:
    """conv_edge_bf16.hip silu_pack_bf16: the argument arrives times log2 e, y' = x' / (1 + 2^-x') = log2 e SiLU(x)."""
    return x / (1.0 + torch.exp2(-x))


def _silu(x: Tensor) -> Tensor:
    """gamd_bf16.h silu_pack_pair (wide_lp.hip): x * rcp(1 + exp2(-log2 e * x))."""
    return x / (1.0 + torch.exp2(-LOG2E * x))


# --------------------------------------------------------------------------
# stages
# --------------------------------------------------------------------------
def _enc(sd, i: int, kind: str) -> Tensor:
    return sd[f"edge_encoder.mlp_layer.{i}.{kind}"]


@torch.no_grad()
def encode_edges(sd: Dict[str, Tensor], feat: Tensor, variant: Variant = None) -> Tensor:
    """Edge features [E, 44 | 45 | 4 | 5] -> e [E, Eh] = edge_layer_norm(edge_encoder(feat)) (nn_module.py:646).

    GELU is the kernels' fit (gelu_fit) in both families.
    bf16_128 (edge_encode_bf16.hip): the features (K zero-padded to 48, which adds exact zeros) and the outputs of both GELUs
    are rounded to bf16 as MFMA operands; the three weight matrices are rounded to bf16 as stored (no factor; in THIS family
    the last Linear is not centred: gamd_finalize_weights centres it only `if (!bf16_edges && !f16x3_edges)`, and the kernel
    runs the full layernorm_chain); biases, GELU and LayerNorm are fp32; the normalised row is rounded to bf16
    (pack_chain_bf16).
    bf16_wide (wide.hip k_edge_encode_wide, LP): the first Linear runs on fp32 MFMA and the two 128-wide GEMMs in split-fp16
    (fp32-grade) on a last Linear whose rows the host centred -- in real arithmetic the plain encoder -- and only the
    normalised row is rounded to bf16 (e_format 1)."""
    sp = spec_of(variant)
    if sp is None:
        return orc.layer_norm(sd, "edge_layer_norm", orc.mlp(sd, "edge_encoder", feat, "gelu", 3))
    dt = feat.dtype
    if sp.drop_bond and feat.shape[1] in (45, 5):
        feat = feat.clone()
        feat[:, -1] = 0
    gelu = gelu_fit if sp.gelu == "fit" else F.gelu
    if sp.family in FP32_GRADE:
        return _encode_fp32_grade(sd, feat, sp, gelu)
    if sp.family == "bf16_wide":
        x = gelu(F.linear(feat, _enc(sd, 0, "weight"), _enc(sd, 0, "bias")))
        x = gelu(F.linear(x, _enc(sd, 2, "weight"), _enc(sd, 2, "bias")))
        y = F.linear(x, _enc(sd, 4, "weight"), _enc(sd, 4, "bias"))
        return round_bf16(orc.layer_norm(sd, "edge_layer_norm", y), sp.bf16_mode)
    r = lambda x: round_bf16(x, sp.bf16_mode)
    x = r(feat)
    x = r(gelu(F.linear(x, _packed(_enc(sd, 0, "weight"), None, sp, dt), _enc(sd, 0, "bias"))))
    x = r(gelu(F.linear(x, _packed(_enc(sd, 2, "weight"), None, sp, dt), _enc(sd, 2, "bias"))))
    y = F.linear(x, _packed(_enc(sd, 4, "weight"), None, sp, dt), _enc(sd, 4, "bias"))
    return r(orc.layer_norm(sd, "edge_layer_norm", y))


def _encode_fp32_grade(sd, feat: Tensor, sp: Spec, gelu) -> Tensor:
    """f32 (edge_encode.hip k_edge_encode / k_edge_encode_small, wide.hip k_edge_encode_wide with LP = false, wide_d.hip): the plain
      encoder with GELU as gamd_gelu_hw / gelu_pair.  (The host stores the last Linear with its output rows centred and the kernels
      normalise the variance only -- in real arithmetic the plain LayerNorm; gamd_finalize_weights, `if (!bf16_edges && !f16x3_edges)`.)
    f16x3_128 (edge_encode_f16x3.hip): the features are split per K step (`gamd_split8(fv, 0, fh, fl)`, K zero-padded to 48: exact
      zeros), both GELU outputs by gemm128_f16x3 (`gamd_split8(X[t], u, xh, xl)`); the three matrices by pack_enc1_f16x3 /
      pack128_f16x3, the last one NOT centred (full layernorm_chain in fp32); e is stored split (`gamd_split8(acc[t], u, eh, el)`)
      and read back as hi + lo.
    f16x3_wide (wide.hip k_edge_encode_wide, LP, e_format 2): the first Linear on the fp32 pipe (`mfma32(w[j], F[4 * g + j], ...)`:
      "the K = 48 first layer stays fp32"), the two 128-wide GEMMs split (`if (LP) gemm128_f16x3<false>`), the last one on rows
      the host centred in double and rounded to fp32 (e4w_c / e4b_c, put_blocks_f16x3(&e4w_c, ...)); the generic LayerNorm over
      the true width; e stored split (`if (LP && a.e_format == 2)`: gamd_split8(nv, u, eh, el))."""
    w, b = (lambda i: _enc(sd, i, "weight")), (lambda i: _enc(sd, i, "bias"))
    if sp.family == "f32":
        x = gelu(F.linear(feat, w(0), b(0)))
        x = gelu(F.linear(x, w(2), b(2)))
        return orc.layer_norm(sd, "edge_layer_norm", F.linear(x, w(4), b(4)))
    if sp.family == "f16x3_128":
        x = gelu(linear_x3(feat, w(0), b(0), sp))
        x = gelu(linear_x3(x, w(2), b(2), sp))
        y = linear_x3(x, w(4), b(4), sp)
    else:
        x = gelu(F.linear(feat, w(0), b(0)))
        x = gelu(linear_x3(x, w(2), b(2), sp))
        w4, b4 = w(4).double(), b(4).double()
        w4c = (w4 - w4.mean(dim=0, keepdim=True)).to(torch.float32).to(feat.dtype)
        b4c = (b4 - b4.mean()).to(torch.float32).to(feat.dtype)
        y = linear_x3(x, w4c, b4c, sp)
    hi, lo = split_fp16(orc.layer_norm(sd, "edge_layer_norm", y), sp)
    return hi + lo


def _node_norm(sd, layer: int, h: Tensor, sp: Optional[Spec]) -> Tensor:
    """hn as k_node's pre(l) forms it.  LayerNorm: fp32 row statistics (the plain operation).  Eval-mode BatchNorm: the host
    folds the running statistics into alpha = w / sqrt(var + eps), beta = b - mean * alpha IN FP32 (gamd_finalize_weights,
    `if (norm_bn)`) and the kernel evaluates (h - 0) * 1 * alpha + beta."""
    p = f"graph_conv.norm_layers.{layer}"
    if sp is None or not sp.folded_norm or p + ".running_mean" not in sd:
        return orc.node_norm(sd, p, h)
    f32 = lambda k: sd[p + k].to(torch.float32)
    invstd = 1.0 / torch.sqrt(f32(".running_var") + torch.tensor(1e-5, dtype=torch.float32))
    alpha = f32(".weight") * invstd
    beta = f32(".bias") - f32(".running_mean") * alpha
    return h * alpha.to(h.dtype) + beta.to(h.dtype)


def _silu_m(x: Tensor, sp: Spec, layer: int, k: int) -> Tensor:
    y = _silu(x)
    if sp.silu_err is not None and sp.silu_err[:2] == (layer, k):
        y = y * (1.0 + sp.silu_err[2] * torch.sign(x))                              # mutation
    return y


def _edge_mlp_fp32_grade(sd, layer: int, e: Tensor, tab_h: Tensor, src: Tensor, dst: Tensor, sp: Spec, gemms: int):
    """The edge MLP of the fp32-grade conv kernels up to its third (gemms = 3) or fourth GEMM: (hn, T4 or e_emb).
    Node tables (k_node / k_node_wide pre(l)): hn = norm(h) in fp32; S = src_affine(hn) + bS, D = dst_affine(hn) with
      bS = (b_src + b_dst) + b_edge_affine.2 (gamd_finalize_weights: `bb.host[o.bS + i] = (sb + db) + ea2b`, fp32 on the host; here
      in the working dtype, like everything that is not an operand rounding); fp32 tables
      in every one of these families.  f16x3: those GEMMs are split too (node.hip `GEMM16(true, a.pre.wsp, a.pre.wdp)` behind
      `SPLIT16()`, weights by pack16_f16x3; wide.hip wq_gemm_f16 on put_blocks_f16x3 images).
    Edge MLP: T1 = silu(W1 e + b1); T3 = silu((W2 T1 + D[dst]) + S[src]); T4 = silu(W3 T3 + b3); e_emb = W4 T4 + b4
      (conv_edge_f16x3.hip / wide_lp.hip phases 1 - 4: `(RC[tp][r0] + DQ[tp][q][j]) + SQ[tp][q][j]`; the accumulators start from
      the fp32 biases, bias_block).  f16x3: e arrives split (load_e_tile_s / load_e_block), every SiLU output is split where it is
      produced (silu_split_pair), the four matrices by pack128_f16x3 (put_edge_f16x3 / put_blocks_f16x3), no factors.
      SiLU = x * rcp(1 + exp2(-log2 e x)) (gamd_silu_hw, silu_split_pair).  Widths below a 128-block are zero-padded: exact zeros."""
    p = f"graph_conv.conv.{layer}"
    w = lambda k: sd[p + k]
    split = sp.family != "f32"

    def lin(x, wk, b=None, g=None):
        if not split:
            return F.linear(x, w(wk), b)
        drop = None
        if g is not None and sp.drop_wlo_kstep is not None and sp.drop_wlo_kstep[:2] == (layer, g):
            drop = kstep_features(sp.drop_wlo_kstep[2], sp.drop_wlo_kstep[3], 0) + kstep_features(sp.drop_wlo_kstep[2], sp.drop_wlo_kstep[3], 1)
        return linear_x3(x, w(wk), b, sp, drop)

    hn = _node_norm(sd, layer, tab_h, sp)
    bS = (w(".src_affine.bias") + w(".dst_affine.bias")) + w(".edge_affine.mlp_layer.2.bias")
    S = lin(hn, ".src_affine.weight", bS)
    D = lin(hn, ".dst_affine.weight")
    t1 = _silu_m(lin(e, ".edge_affine.mlp_layer.0.weight", w(".edge_affine.mlp_layer.0.bias"), 0), sp, layer, 0)
    t3 = _silu_m((lin(t1, ".edge_affine.mlp_layer.2.weight", None, 1) + D[dst]) + S[src], sp, layer, 1)
    t4 = _silu_m(lin(t3, ".theta_edge.mlp_layer.1.weight", w(".theta_edge.mlp_layer.1.bias"), 2), sp, layer, 2)
    if gemms == 3:
        return hn, t4
    return hn, lin(t4, ".theta_edge.mlp_layer.3.weight", w(".theta_edge.mlp_layer.3.bias"), 3)


@torch.no_grad()
def conv_edge_t3_sum(sd: Dict[str, Tensor], e: Tensor, h0: Tensor, src: Tensor, dst: Tensor, variant: Variant = "f32") -> Tensor:
    """Layer 0 in its hoisted form (conv_edge.hip `k_conv_edge<TIME, L0>`, conv_edge_small.hip's _l0; fp32, LJ, 128 / 128 / 128):
    the per-destination sum over the real edges of the third GEMM's activated output, SiLU(W3 T2 + b3) [N, D] -- what
    GamdForce.debug_partial holds when the hoisted layer is the last one.  h0 is the shared row repeated; S0 + D0 is phase 2's
    accumulator start."""
    sp = spec_of(variant)
    src, dst = src.long(), dst.long()
    _, t4 = _edge_mlp_fp32_grade(sd, 0, e, h0, src, dst, sp, 3)
    out = torch.zeros((h0.shape[0], t4.shape[1]), dtype=t4.dtype)
    out.index_add_(0, dst, t4)
    return out


@torch.no_grad()
def node_update_hoisted(sd: Dict[str, Tensor], t3_sum: Tensor, d: Tensor, h0: Tensor, variant: Variant = "f32") -> Tensor:
    """h_1 of the hoisted layer 0 from the per-atom sums of conv_edge_t3_sum and the in-degrees d [N] (node.hip post(0) with
    a.post.c0): phi_edge's part is M0 sum T3 + d_i c0 with M0 = W_pe diag(hn0) W4 and c0 = W_pe (hn0 * b4), formed on the host in
    double from the fp32 weights -- hn0 = norm_layers[0](node_emb) in double (LayerNorm) or the fp32-folded affine map (eval
    BatchNorm) -- and rounded to fp32 once (gamd_finalize_weights, `if (l == 0 && h->l0_hoist)`; `fmaf(n_real, c[o][r], mine[o][r])`)."""
    sp = spec_of(variant)
    p, dt = "graph_conv.conv.0", h0.dtype
    sd64 = cast_state_dict(sd, torch.float64)
    hn0 = _node_norm(sd64, 0, sd64["node_emb"].view(1, -1), sp).view(-1)
    wpe = sd64[p + ".phi_edge.weight"]
    m0 = ((wpe * hn0.view(1, -1)) @ sd64[p + ".theta_edge.mlp_layer.3.weight"]).to(torch.float32).to(dt)
    c0 = (wpe @ (hn0 * sd64[p + ".theta_edge.mlp_layer.3.bias"])).to(torch.float32).to(dt)
    hn = _node_norm(sd, 0, h0, sp)
    bP = sd[p + ".phi_dst.bias"] + sd[p + ".phi_edge.bias"]
    x = _silu((F.linear(hn, sd[p + ".phi_dst.weight"], bP) + F.linear(t3_sum, m0)) + d.to(dt).view(-1, 1) * c0.view(1, -1))
    return F.linear(x, sd[p + ".phi.mlp_layer.1.weight"], sd[p + ".phi.mlp_layer.1.bias"]) + h0


@torch.no_grad()
def conv_edge_agg(sd: Dict[str, Tensor], layer: int, e: Tensor, h_prev: Tensor, src: Tensor, dst: Tensor,
                  variant: Variant = None, tables_from: Optional[Tensor] = None) -> Tensor:
    """One conv layer's edge side (nn_module.py:135-142): e [E, Eh], the residual stream h_prev [N, H] entering the layer,
    edges src -> dst.  Returns the per-destination aggregate [N, H] = sum over incoming edges of hn[src] * e_emb: what the
    partial-sum pieces of the conv edge kernel add up to.

    bf16_128 (k_node pre(l) with tab16, conv_edge_bf16.hip):
      hn = norm(h_prev) in fp32, stored as fp16 (store16_h); S = src_affine(hn) + bS, D = dst_affine(hn) from the UNROUNDED
      hn on the split-fp16 (fp32-grade) node GEMMs, their weights and biases times log2 e (each factor applied in double and
      rounded to fp32; bS = (b_src' + b_dst') + b_edge_affine.2' in fp32), stored as fp16 (store16_tab).
      T1 = bf16(silu'(bf16(W1') e + b1'));  T3 = bf16(silu'((S16[src] + D16[dst]) + bf16(W2) T1))  [the accumulator starts
      from the fp32 sum S + D: add_h_h];  T4 = bf16(silu'(bf16(W3) T3 + b3'));  e_emb = bf16(W4') T4 + b4 with W4' = W4 ln 2
      (its row permutation is layout only);  message hn16[src] * e_emb and the segment sum in fp32 (fma_h_f_f).
      silu'(x') = x' / (1 + 2^-x').
    bf16_wide (k_node_wide, wide_lp.hip k_conv_edge_bf16_wide): fp32 tables hn, S = src_affine(hn) + bS, D = dst_affine(hn)
      with bS = (b_src + b_dst) + b_edge_affine.2; no factors; T3's argument is (W2 T1 + D[dst]) + S[src]; hn[src] is fp32
      (gamd_msg_acc); SiLU as x * rcp(1 + exp2(-log2 e x)).  Widths below a 128-block are zero-padded: exact zeros.
    f32, f16x3_128, f16x3_wide: _edge_mlp_fp32_grade; the message hn[src] * e_emb and the segment sum in fp32 (gamd_msg_acc).
    `tables_from` (mutation, these three families): the residual stream the node tables hn / S / D are formed from instead of
      h_prev -- a layer that reads the tables of an earlier one."""
    sp = spec_of(variant)
    p = f"graph_conv.conv.{layer}"
    src, dst = src.long(), dst.long()
    if sp is not None and sp.family in FP32_GRADE:
        hn, e_emb = _edge_mlp_fp32_grade(sd, layer, e, h_prev if tables_from is None else tables_from, src, dst, sp, 4)
        agg = torch.zeros_like(hn)
        agg.index_add_(0, dst, hn[src] * e_emb)
        return agg
    hn = _node_norm(sd, layer, h_prev, sp)
    if sp is None:
        edge_code = orc.mlp(sd, p + ".edge_affine", e, "silu", 2)
        src_code = orc.linear(sd, p + ".src_affine", hn[src])
        dst_code = orc.linear(sd, p + ".dst_affine", hn[dst])
        e_emb = orc.mlp(sd, p + ".theta_edge", edge_code + src_code + dst_code, "silu", 2, True)
        agg = torch.zeros_like(hn)
        agg.index_add_(0, dst, hn[src] * e_emb)
        return agg
    dt = h_prev.dtype
    r = lambda x: round_bf16(x, sp.bf16_mode)
    w = lambda k: sd[p + k]
    w4 = w(".theta_edge.mlp_layer.3.weight")
    if sp.drop_w4_kstep is not None:
        w4 = w4.clone()
        w4[:, kstep_features(*sp.drop_w4_kstep)] = 0
    if sp.family == "bf16_128":
        sc = lambda k: _host_scaled(w(k), LOG2E)
        bS = ((sc(".src_affine.bias") + sc(".dst_affine.bias")) + sc(".edge_affine.mlp_layer.2.bias")).to(dt)
        S = F.linear(hn, sc(".src_affine.weight").to(dt), bS)
        D = F.linear(hn, sc(".dst_affine.weight").to(dt))
        hn_t = hn
        if sp.fp16_tables:
            hn_t, S, D = round_fp16(hn), round_fp16(S), round_fp16(D)
        t1 = r(_silu_exp2(F.linear(e, _packed(w(".edge_affine.mlp_layer.0.weight"), LOG2E, sp, dt),
                                   sc(".edge_affine.mlp_layer.0.bias").to(dt))))
        t3 = r(_silu_exp2((S[src] + D[dst]) + F.linear(t1, _packed(w(".edge_affine.mlp_layer.2.weight"), None, sp, dt))))
        t4 = r(_silu_exp2(F.linear(t3, _packed(w(".theta_edge.mlp_layer.1.weight"), None, sp, dt),
                                   sc(".theta_edge.mlp_layer.1.bias").to(dt))))
        e_emb = F.linear(t4, _packed(w4, LN2, sp, dt), w(".theta_edge.mlp_layer.3.bias"))
    elif sp.family == "bf16_wide":
        f32 = lambda k: w(k).to(torch.float32)
        bS = ((f32(".src_affine.bias") + f32(".dst_affine.bias")) + f32(".edge_affine.mlp_layer.2.bias")).to(dt)
        S = F.linear(hn, w(".src_affine.weight"), bS)
        D = F.linear(hn, w(".dst_affine.weight"))
        hn_t = hn
        t1 = r(_silu(F.linear(e, _packed(w(".edge_affine.mlp_layer.0.weight"), None, sp, dt), w(".edge_affine.mlp_layer.0.bias"))))
        t3 = r(_silu((F.linear(t1, _packed(w(".edge_affine.mlp_layer.2.weight"), None, sp, dt)) + D[dst]) + S[src]))
        t4 = r(_silu(F.linear(t3, _packed(w(".theta_edge.mlp_layer.1.weight"), None, sp, dt), w(".theta_edge.mlp_layer.1.bias"))))
        e_emb = F.linear(t4, _packed(w4, None, sp, dt), w(".theta_edge.mlp_layer.3.bias"))
    else:
        raise ValueError(sp.family)
    agg = torch.zeros_like(hn)
    agg.index_add_(0, dst, hn_t[src] * e_emb)
    return agg


@torch.no_grad()
def node_update(sd: Dict[str, Tensor], layer: int, agg: Tensor, h_prev: Tensor, variant: Variant = None) -> Tensor:
    """h_next = phi(phi_dst(hn) + phi_edge(agg)) + h_prev (nn_module.py:147, :202).
    None and the bf16 variants: plain -- the node kernels run fp32 or split-fp16 GEMMs (fp32-grade) on the unrounded hn, and an
      eval-mode BatchNorm's fp32-folded affine map differs from F.batch_norm at fp32 rounding level, far below that stage's bar.
    f32: hn through the folded map (_node_norm); P = phi_dst(hn) + bP with bP = b_phi_dst + b_phi_edge
      (gamd_finalize_weights: `bb.host[o.bP + i] = pdb + peb`); SiLU as gamd_silu_hw.
    f16x3_128 / f16x3_wide (NodeArgs::f16x3 = node_f16): the three GEMMs split (node.hip: `SPLIT16()` behind every exchange16 --
      agg, SiLU(P + phi_edge(agg)), hn -- and `GEMM16(...)` on pack16_f16x3 weights; wide.hip k_node_wide<HT, true>: wq_gemm_f16)."""
    sp = spec_of(variant)
    p = f"graph_conv.conv.{layer}"
    if sp is None or sp.family not in FP32_GRADE:
        hn = orc.node_norm(sd, f"graph_conv.norm_layers.{layer}", h_prev)
        return orc.mlp(sd, p + ".phi", orc.linear(sd, p + ".phi_dst", hn) + orc.linear(sd, p + ".phi_edge", agg), "silu", 1, True) + h_prev
    lin = (lambda x, w, b=None: linear_x3(x, w, b, sp)) if sp.family != "f32" else F.linear
    hn = _node_norm(sd, layer, h_prev, sp)
    bP = sd[p + ".phi_dst.bias"] + sd[p + ".phi_edge.bias"]
    x = _silu(lin(hn, sd[p + ".phi_dst.weight"], bP) + lin(agg, sd[p + ".phi_edge.weight"]))
    return lin(x, sd[p + ".phi.mlp_layer.1.weight"], sd[p + ".phi.mlp_layer.1.bias"]) + h_prev


@torch.no_grad()
def decode(sd: Dict[str, Tensor], h: Tensor, variant: Variant = None) -> Tensor:
    """graph_decoder (nn_module.py:684): normalised forces [N, 3].
    None and the bf16 variants: plain, erf-GELU included (held to the fixed fp32 bar, where the fit's 1.2e-7 absolute does not show).
    f32 / f16x3: GELU as the node kernels evaluate it (node.hip mode 2: `gl[r] = gamd_gelu_hw(mine[o][r])`); f16x3: the first
      Linear split (`SPLIT16(); ... GEMM16(false, a.dec_w1p, nullptr)`, dec_w1p through put_node), the 3-row second one in fp32."""
    sp = spec_of(variant)
    if sp is None or sp.family not in FP32_GRADE:
        return orc.mlp(sd, "graph_decoder", h, "gelu", 2)
    gelu = gelu_fit if sp.gelu == "fit" else F.gelu
    w0, b0 = sd["graph_decoder.mlp_layer.0.weight"], sd["graph_decoder.mlp_layer.0.bias"]
    x = gelu(linear_x3(h, w0, b0, sp) if sp.family != "f32" else F.linear(h, w0, b0))
    return F.linear(x, sd["graph_decoder.mlp_layer.2.weight"], sd["graph_decoder.mlp_layer.2.bias"])


@torch.no_grad()
def initial_h(sd: Dict[str, Tensor], n: int, node_feat: Optional[Tensor] = None) -> Tensor:
    """h_0: node_emb repeated (nn_module.py:681) or node_encoder(feat) (:554)."""
    if node_feat is None:
        return sd["node_emb"].repeat((n, 1))
    return orc.linear(sd, "node_encoder", node_feat)


@torch.no_grad()
def forward_stages(sd: Dict[str, Tensor], feat: Tensor, h0: Tensor, src: Tensor, dst: Tensor, variant: Variant = None) -> dict:
    """The stages chained from edge features and h_0: {"e", "h": [h_0 .. h_L], "agg": [agg_0 .. agg_{L-1}], "out"}."""
    e = encode_edges(sd, feat, variant)
    h, aggs = [h0], []
    for l in range(orc.n_conv_layers(sd)):
        aggs.append(conv_edge_agg(sd, l, e, h[-1], src, dst, variant))
        h.append(node_update(sd, l, aggs[-1], h[-1], variant))
    return {"e": e, "h": h, "agg": aggs, "out": decode(sd, h[-1], variant)}


def cast_state_dict(sd: Dict[str, Tensor], dtype) -> Dict[str, Tensor]:
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def mutated(variant: Variant, **kw) -> Spec:
    return replace(spec_of(variant), **kw)
