"""The per-kernel float64 references (oracle/gamd_oracle_lp.py: operand-rounded for bf16, operand-split for split-fp16, plain with
the kernels' GELU fit and folded BatchNorm for fp32) checked against themselves and the oracle.  CPU only.

(a) without rounding it IS gamd_oracle, stage by stage; (b) with rounding it moves the forces by the size of error DESIGN
section 8 reports for the format; (c) the criteria of tests/test_gpu_lp_stages.py discriminate: a reference with ONE rounding
point reverted stands in for a subtly wrong kernel and must break at least one of them, every yardstick computed exactly as
the GPU test computes it (tests/lp_cases.py)."""
import numpy as np
import pytest
import torch

import gamd_oracle as orc
import gamd_oracle_lp as lp
import lp_cases as lc
from helpers import load_golden, rel_err

GOLDENS = ["lj258_seed0", "tip3p774_seed3", "dynbox384_dftcfg_seed5"]


def _oracle_run(name, dtype):
    """gamd_oracle on a committed golden in `dtype`: (sd, stages, out, src, dst, golden)."""
    g, cfg, sd = load_golden(name)
    sd = lp.cast_state_dict(sd, dtype)
    st = {}
    feat = torch.from_numpy(g["node_feat"]).to(dtype) if "node_feat" in g else None
    if cfg.kind == "dynbox":
        out = orc.forward_dynamic_box(sd, torch.from_numpy(g["pos"]).to(dtype), feat, g["box"], float(g["cutoff"]), stages=st)
        edge_idx = st["edge_idx"]
    else:
        box = float(g["box"])
        edge_idx = torch.from_numpy(g["edge_idx"]).long()
        out = orc.forward(sd, torch.from_numpy(np.mod(g["pos"], box)).float().to(dtype), edge_idx, box, feat=feat,
                          bond=g["bond"] if "bond" in g else None, stages=st)
    return sd, st, out, edge_idx[1].long(), edge_idx[0].long(), g


_runs = {}


def _run(name, dtype):
    if (name, dtype) not in _runs:
        _runs[(name, dtype)] = _oracle_run(name, dtype)
    return _runs[(name, dtype)]


@pytest.mark.parametrize("name", GOLDENS)
def test_without_rounding_the_stages_are_the_oracle(name):
    """variant=None against gamd_oracle.forward / forward_dynamic_box, stage by stage in float64 to 1e-12; the stages chained
    in float32 give the committed reference output at the suite's tolerance."""
    sd, st, out, src, dst, g = _run(name, torch.float64)
    assert rel_err(lp.encode_edges(sd, st["feat"], None).numpy(), st["e"].numpy()) < 1e-12
    for l in range(orc.n_conv_layers(sd)):
        agg = lp.conv_edge_agg(sd, l, st["e"], st["h"][l], src, dst, None)
        assert rel_err(lp.node_update(sd, l, agg, st["h"][l]).numpy(), st["h"][l + 1].numpy()) < 1e-12, f"layer {l}"
    assert rel_err(lp.decode(sd, st["h"][-1]).numpy(), out.numpy()) < 1e-12
    chain = lp.forward_stages(sd, st["feat"], st["h"][0], src, dst, None)
    assert rel_err(chain["out"].numpy(), out.numpy()) < 1e-12
    sd32, st32, out32, _, _, _ = _run(name, torch.float32)
    chain32 = lp.forward_stages(sd32, st32["feat"], st32["h"][0], src, dst, None)
    assert chain32["out"].dtype == torch.float32
    assert rel_err(chain32["out"].numpy(), g["out_norm"]) < lc.TOL


@pytest.mark.parametrize("variant", ["bf16_128", "bf16_wide"])
@pytest.mark.parametrize("name", GOLDENS)
def test_size_of_the_format_error(name, variant):
    """Each bf16 variant in float64 against no rounding in float64: the forces move by more than 1e-4 (the rounding really is
    applied) and by less than 1e-2 (the size DESIGN section 8 reports for the format)."""
    sd, st, out, src, dst, _ = _run(name, torch.float64)
    lo = lp.forward_stages(sd, st["feat"], st["h"][0], src, dst, variant)["out"]
    err = rel_err(lo.numpy(), out.numpy())
    print(f"format error {name} {variant}: {err:.3e}")
    assert 1e-4 < err < 1e-2, err


def test_rounding_helpers():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 3 * 2.0 ** -8)], dtype=torch.float64)
    # ties go to the even mantissa, anything above a tie goes up; truncation drops the low bits
    assert lp.round_bf16(x).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -6)]
    assert lp.round_bf16(x, "trunc").tolist() == [1.0, 1.0 + 2.0 ** -7, 1.0, -(1.0 + 2.0 ** -7)]
    assert lp.round_bf16(x).dtype == torch.float64 and lp.round_fp16(x.float()).dtype == torch.float32
    assert lp.round_fp16(torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11])).tolist() == [1.0, 1.0 + 2.0 ** -9]
    assert sorted(sum((lp.kstep_features(t, u, h) for t in range(4) for u in range(2) for h in range(2)), [])) == list(range(128))
    assert lp.kstep_features(1, 1, 0) == [48, 49, 50, 51, 56, 57, 58, 59]


def test_piece_map_from_the_csr():
    from helpers import pieces_of_csr
    # rows of 0, 3, 14, 0, 20 and 1 edges: pieces break at row starts and at multiples of 16
    piece, piece_row, n = pieces_of_csr(np.cumsum([0, 0, 3, 14, 0, 20, 1]))
    # row 1: slots 0-2 | row 2: 3-15, then 16 behind the chunk boundary | row 4: 17-31, 32-36 | row 5: 37
    assert n == 6 and piece_row.tolist() == [1, 2, 2, 4, 4, 5]
    assert piece.tolist() == [0] * 3 + [1] * 13 + [2] + [3] * 15 + [4] * 5 + [5]
    # a row that starts on a chunk boundary opens no piece of its own
    piece, piece_row, n = pieces_of_csr(np.array([0, 16, 40]))
    assert n == 3 and piece_row.tolist() == [0, 1, 1] and piece.tolist() == [0] * 16 + [1] * 16 + [2] * 8
    assert pieces_of_csr(np.zeros(5, dtype=np.int64))[2] == 0


# ---- the criteria discriminate ---------------------------------------------------------------------------------------
MUTATIONS = {
    "bf16_truncation": dict(bf16_mode="trunc"),                 # bf16 by truncation instead of round-to-nearest-even
    "no_fp16_tables": dict(fp16_tables=False),                  # S / D / hn not rounded to fp16
    "round_before_scaling": dict(scale_then_round=False),       # weights rounded before the log2 e / ln 2 factors
    "w4_kstep_dropped": dict(drop_w4_kstep=(3, 1, 1)),          # one K step of W4: features 116..119, 124..127 of one lane half
    "bond_feature_dropped": dict(drop_bond=True),               # column 44
}


def test_the_reference_carries_no_flip_in_its_median_row():
    """The yardsticks themselves: fp32 against float64 of the same reference stays at fp32 level in the aggregate's median row
    (so the median criterion has room), and every flip-driven yardstick x MARGIN sits below the smallest effect a mutation
    is required to show -- asserted per mutation below, recorded here."""
    for v in ("bf16_128", "bf16_wide"):
        y = lc.yardstick(v)
        print(f"yardstick {v}: " + ", ".join(f"{k} {y[k]:.3e}" for k in sorted(y)))
        assert y["agg_med"] < lc.TOL / 2
        assert all(lc.MARGIN * y[k] < 1e-2 for k in ("enc_bits", "agg_max", "e2e"))     # below the format's own error


# one LJ and one water case; the bond feature exists in the water case only
MUTATION_CASES = [(m, c) for m in sorted(MUTATIONS) for c in ("lj-3", "water-bond") if m != "bond_feature_dropped" or c == "water-bond"]


@pytest.mark.parametrize("mutation,case_id", MUTATION_CASES)
def test_a_reverted_rounding_point_breaks_a_criterion(mutation, case_id):
    """The mutated float64 reference plays the device: per stage on the unmutated reference's inputs, exactly as
    tests/test_gpu_lp_stages.py feeds a kernel the device's."""
    c = lc.BY_ID[case_id]
    spec = lp.mutated(c.variant, **MUTATIONS[mutation])
    stats = lc.compare_with_reference(case_id, lc.weights(case_id)[1], torch.float64, spec)
    yard = lc.yardstick(c.variant)
    bad = lc.criteria(stats, yard)
    print(f"{mutation} on {case_id}: breaks {bad}; " +
          ", ".join(f"{k} {stats[k]:.3e} (bar {lc.MARGIN * yard[k] if k in lc.FLIP_STATS else lc.TOL:.3e})" for k in sorted(stats)))
    assert bad, (mutation, stats, yard)


def test_lj_layer0_case_is_well_conditioned():
    """lj-1 judges layer 0 of an LJ model, where all atoms share one hn / S / D row: its weights must not put one of those
    values where an fp32-sized error flips its fp16 rounding (lp_cases.CASES).  30 seeded perturbations of h_0 of 4e-7
    relative (about 3 fp32 epsilons, the error of a row's LayerNorm in fp32) leave the median row at fp32 level."""
    assert lc.shared_row_conditioning("lj-1", 30, 4e-7) < 1e-6


@pytest.mark.parametrize("case_id", lc.BF16_IDS + ["ctl-f32"])        # the cases whose node kernel and decoder are held to the FIXED bar
def test_cases_leave_the_fp32_bar_its_headroom(case_id):
    """The node kernel and the decoder are held to 1e-5, per-row p99 included, a statistic that a model with a few nearly
    cancelling forces uses up on its own (weight seed 27 of the unexpanded case: 5.9e-6 between the reference in fp32 and in
    float64).  Every case's weights leave the fp32 reference below 2e-6 on all four statistics."""
    noise = lc.fp32_stage_noise(case_id)
    if not lc.BY_ID[case_id].dec_p99_held:          # the one case kept with such weights: its p99 is recorded, not asserted
        assert noise.pop("dec_p99") > 2e-6
    assert max(noise.values()) < 2e-6, noise


def test_gelu_fit_is_the_header_s():
    """gelu_fit's coefficients are gamd_common.h's, and the fit is within its stated 1.2e-7 of the erf form while off by
    ~8e-6 relative for negative arguments -- why a bf16 kernel's reference has to evaluate the fit."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gamd_amd", "csrc", "gamd_common.h")).read()
    q = [float(re.search(rf"#define GAMD_GELU_Q{i} (\S+)f", src).group(1)) for i in range(7)]
    assert tuple(q) == lp.GELU_Q
    x = torch.linspace(-8.0, 8.0, 160001, dtype=torch.float64)
    fit, erf = lp.gelu_fit(x), torch.nn.functional.gelu(x)
    assert float((fit - erf).abs().max()) < 1.2e-7
    neg = (x < -0.1) & (x > -3.0)
    rel = ((fit - erf).abs() / erf.abs())[neg]
    assert 2e-6 < float(rel.max()) < 2e-5


@pytest.mark.parametrize("case_id", ["lj-3", "wide-256"])
def test_the_erf_form_in_the_reference_would_fail_a_correct_encoder(case_id):
    """Spec.gelu = "erf": the float64 reference with the erf form against the one with the kernels' fit.  The fit alone flips more
    roundings of e than the encoder's bar allows, so a reference with the erf form would reject a correct kernel -- and with
    the fit in the reference the encoder check no longer sees an error of the fit itself (that is test_gelu_fit_is_the_header_s
    and tests/test_host_logic.py)."""
    c = lc.BY_ID[case_id]
    sd64 = lc.weights(case_id)[1]
    f = lc.cpu_inputs(case_id)["feat"].double()
    share, _ = lc.enc_stats(lp.encode_edges(sd64, f, lp.mutated(c.variant, gelu="erf")), lp.encode_edges(sd64, f, c.variant))
    print(f"erf against fit, {case_id}: share {share:.3e}, {share / lc.yardstick_of(case_id)['enc_bits']:.1f} x the case's yardstick")
    assert share > lc.MARGIN * lc.yardstick_of(case_id)["enc_bits"]


def test_the_unmutated_reference_breaks_none():
    for case_id in ("lj-3", "water-bond", "wide-256"):
        c = lc.BY_ID[case_id]
        stats = lc.compare_with_reference(case_id, lc.weights(case_id)[1], torch.float64, c.variant)
        assert lc.criteria(stats, lc.yardstick(c.variant)) == [] and max(stats.values()) == 0.0


def test_cases_reach_what_they_are_for():
    x = lc.cpu_inputs("sparse")
    deg = np.bincount(x["dst"].numpy(), minlength=128)
    assert (deg == 0).any() and 0 < deg.max() < 16                 # isolated atoms, rows shorter than a chunk
    x = lc.cpu_inputs("tiny")
    deg = np.bincount(x["dst"].numpy(), minlength=7)
    assert deg[6] == 0 and 0 < x["dst"].numel() < 32                # one partly filled tile, one isolated atom
    assert lc.cpu_inputs("water-bond")["feat"].shape[1] == 45 and lc.cpu_inputs("water-bond")["feat"][:, 44].sum() > 0
    assert lc.cpu_inputs("dynbox-noexp")["feat"].shape[1] == 4
    assert not (lc.cpu_inputs("dynbox-noexp")["src"] == lc.cpu_inputs("dynbox-noexp")["dst"]).any()
    # ---- the fp32-grade cases ----
    assert len(lc.GRADE_IDS) >= 28 and {"ctl-f32", "ctl-f16x3"} <= set(lc.GRADE_IDS)
    feats = {"water90": 44, "lj258": 44, "sparse128": 44, "tiny7": 44}
    for c in (lc.BY_ID[i] for i in lc.GRADE_IDS):
        x = lc.cpu_inputs(c.id)
        n, n_edges = x["h0"].shape[0], x["dst"].numel()
        assert n <= 270 and n_edges <= 10500, c.id
        deg = np.bincount(x["dst"].numpy(), minlength=n)
        want = 4 if c.cfg.n_rbf == 0 else feats[c.system] + (1 if c.cfg.use_bond else 0)
        assert x["feat"].shape[1] == want == c.cfg.edge_in, c.id
        if c.cfg.use_bond:
            assert x["feat"][:, 44].sum() > 0
        if c.system == "sparse128":
            assert (deg == 0).any() and 0 < deg.max() < 16, c.id             # isolated atoms, rows shorter than a chunk
        if c.system == "tiny7":
            assert deg[6] == 0 and 0 < n_edges < 32, c.id                    # one partly filled tile, one isolated atom
        else:
            assert n_edges % 32 != 0, c.id                                    # the last tile is partly filled everywhere
        # the side of the latency / throughput choice: the library's default limit is 512 tiles (gamd_host.h small_tile_limit)
        assert (n_edges + 31) // 32 <= 512, c.id
    by = lc.BY_ID
    for i in ("f32-wide-odd", "f16x3-wide-odd"):
        g = by[i].cfg
        assert all(w % 128 for w in (g.encoding_size, g.hidden_dim, g.edge_embedding_dim)) and by[i].generic_width
    g = by["f32-water-d256"].cfg
    assert g.hidden_dim > 128 and g.encoding_size % 128 and g.edge_embedding_dim % 128 and by["f32-water-d256"].family == "f32_wide_d"
    assert by["f32-lj-d192"].hidden_dim > 128 and not by["f32-lj-d192"].hoisted
    # the one-layer LJ case really is the hoisted configuration, and its forms around it are what their names say
    c = by["f32-lj-1"]
    assert c.hoisted and c.cfg.conv_layer == 1 and c.cfg.kind == "lj" and c.edge_dtype == "f32" and c.kernel_select == 0
    assert (c.cfg.encoding_size, c.cfg.hidden_dim, c.cfg.edge_embedding_dim, c.cfg.n_rbf) == (128, 128, 128, 40)
    assert by["f32-lj-3"].hoisted and by["f32-lj-3-tp"].hoisted and by["f32-bn5"].hoisted and not by["f32-lj-3-nohoist"].hoisted
    assert not by["f16x3-lj-3"].hoisted and not by["ctl-f32"].hoisted and not by["f32-generic-128"].hoisted
    assert by["f32-generic-128"].generic_width and not by["ctl-f32"].generic_width
    assert {by[i].family for i in lc.GRADE_IDS} == {"f32_128_latency", "f32_128_latency_l0", "f32_128_throughput", "f32_128_throughput_l0",
                                                     "f32_wide_latency", "f32_wide_throughput", "f32_wide16", "f32_wide_d", "f16x3_128",
                                                     "f16x3_wide"}
    # a row that starts on a chunk boundary exists where mutation 5 needs one
    for i in ("f32-lj-3", "f32-lj-1"):
        x = lc.cpu_inputs(i)
        assert lc.chunk_start_rows(x["dst"], x["h0"].shape[0]).sum() > 0


# ======================================================================================================================
# the fp32-grade families: "f32", "f16x3_128", "f16x3_wide"
# ======================================================================================================================
F32_PLAIN = lp.mutated("f32", gelu="erf", folded_norm=False)


def _csrc(name):
    import os
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gamd_amd", "csrc", name)).read()


@pytest.mark.parametrize("name", GOLDENS + ["lj258_bn_seed11"])
def test_f32_variant_is_the_oracle_but_for_the_fit_and_the_folded_norm(name):
    """"f32" with the erf form and F.batch_norm IS gamd_oracle, stage by stage in float64 to 1e-12.  With the kernels' fit and the
    folded norm each GELU output stays within the fit's stated 1.2e-7 absolute, the folded map within 1e-6 relative of
    F.batch_norm, and the forces within the variant's own fp32 yardstick (the two are fp32-grade restatements)."""
    sd, st, out, src, dst, _ = _run(name, torch.float64)
    assert rel_err(lp.encode_edges(sd, st["feat"], F32_PLAIN).numpy(), st["e"].numpy()) < 1e-12
    for l in range(orc.n_conv_layers(sd)):
        agg = lp.conv_edge_agg(sd, l, st["e"], st["h"][l], src, dst, F32_PLAIN)
        assert rel_err(agg.numpy(), lp.conv_edge_agg(sd, l, st["e"], st["h"][l], src, dst, None).numpy()) < 1e-12, f"layer {l}"
        assert rel_err(lp.node_update(sd, l, agg, st["h"][l], F32_PLAIN).numpy(), st["h"][l + 1].numpy()) < 1e-12, f"layer {l}"
    assert rel_err(lp.decode(sd, st["h"][-1], F32_PLAIN).numpy(), out.numpy()) < 1e-12
    assert rel_err(lp.forward_stages(sd, st["feat"], st["h"][0], src, dst, F32_PLAIN)["out"].numpy(), out.numpy()) < 1e-12
    # the fit: the first GELU of the encoder and the decoder's, on this golden's own pre-activations
    for pre in (torch.nn.functional.linear(st["feat"], sd["edge_encoder.mlp_layer.0.weight"], sd["edge_encoder.mlp_layer.0.bias"]),
                torch.nn.functional.linear(st["h"][-1], sd["graph_decoder.mlp_layer.0.weight"], sd["graph_decoder.mlp_layer.0.bias"])):
        assert float((lp.gelu_fit(pre) - torch.nn.functional.gelu(pre)).abs().max()) < 1.2e-7
    if "graph_conv.norm_layers.0.running_mean" in sd:
        folded = lp._node_norm(sd, 0, st["h"][0], lp.spec_of("f32"))
        assert 0 < rel_err(folded.numpy(), orc.node_norm(sd, "graph_conv.norm_layers.0", st["h"][0]).numpy()) < 1e-6
    err = rel_err(lp.forward_stages(sd, st["feat"], st["h"][0], src, dst, "f32")["out"].numpy(), out.numpy())
    print(f"f32 variant against the oracle, {name}: {err:.3e}")
    assert 0 < err < lc.yardstick("f32")["e2e"]


def test_the_restated_host_and_kernel_lines_are_the_sources():
    """The lines the fp32-grade variants restate, held to the sources like the GELU coefficients."""
    api, hdr, com = _csrc("gamd_weights_host.h"), _csrc("gamd_f16x3.h"), _csrc("gamd_common.h")
    # eval BatchNorm folded in fp32 (_node_norm)
    assert "const float invstd = 1.0f / std::sqrt(rv->data[i] + 1e-5f);" in api
    assert "al.data[i] = ng->data[i] * invstd;" in api and "be.data[i] = nb->data[i] - rm->data[i] * al.data[i];" in api
    # the split: hi = fp16(x), lo = fp16(x - hi) with the residual in fp32, on the host and in the kernels (split_fp16)
    assert "const gamd_f32x2_t r = x - __builtin_convertvector(h, gamd_f32x2_t);" in hdr
    assert "const gamd_f32x2_t rem = y - __builtin_convertvector(h, gamd_f32x2_t);" in hdr
    # three products, lo x lo dropped (linear_x3)
    step = hdr[hdr.index("void gamd_f16x3_step"):hdr.index("// acc (+)= W X^T")]
    assert step.count("mfma_f16(") == 6 and "mfma_f16(wl, xl" not in step and "mfma_f16(xl, wl" not in step
    # SiLU as x * rcp(1 + exp2(-log2 e x)) (_silu) and the unscaled, uncentred packing of the 128-wide split family
    assert "sk.nl2e = gamd_f32x2_t{-1.4426950408889634f, -1.4426950408889634f};" in _csrc("conv_edge_f16x3.hip")
    assert "const float e = __builtin_amdgcn_exp2f(x * -1.4426950408889634f);" in com and "return x * __builtin_amdgcn_rcpf(1.0f + e);" in com
    assert "if (!bf16_edges && !f16x3_edges) {" in api and "r.node_f16 = c.edge_dtype != GAMD_EDGE_F32;" in _csrc("gamd_route_host.h")
    assert "if (LP) gemm128_f16x3<false>((const f16x8*)w2, lane, X, acc);" in _csrc("wide.hip")        # GEMM 1 of the wide encoder stays fp32


def test_split_helpers():
    x = torch.tensor([1.0 + 2.0 ** -12 + 2.0 ** -20, 0.04, 3.0e-5, 1.0e-7, -70000.0 / 2], dtype=torch.float64)
    hi, lo = lp.split_fp16(x)
    assert hi.dtype == torch.float64 and hi[0] == 1.0 and lo[0] == 2.0 ** -12 + 2.0 ** -20
    # 0.04: lo is fp16-subnormal (quantum 2^-24), kept; flushed by the mutation
    assert 0 < abs(float(lo[1])) < 2.0 ** -14 and abs(float(hi[1] + lo[1]) - 0.04) <= 2.0 ** -25
    assert float(lp.split_fp16(x, lp.mutated("f16x3_128", flush_lo_subnormal=True))[1][1]) == 0.0
    assert float(hi[3]) == 2.0 ** -23 and float(lo[3]) == float(torch.tensor(1.0e-7 - 2.0 ** -23, dtype=torch.float32).to(torch.float16))
    w, v = torch.randn(5, 16, dtype=torch.float64), torch.randn(3, 16, dtype=torch.float64)
    wh, wl = lp.split_fp16(w)
    vh, vl = lp.split_fp16(v)
    full = torch.nn.functional.linear(vh + vl, wh + wl)
    assert torch.allclose(lp.linear_x3(v, w), full - torch.nn.functional.linear(vl, wl), rtol=0, atol=1e-15)     # lo x lo is what is missing


@pytest.mark.parametrize("variant", ["f16x3_128", "f16x3_wide"])
@pytest.mark.parametrize("name", GOLDENS)
def test_size_of_the_split_error(name, variant):
    """Each split-fp16 variant in float64 against no rounding in float64, per GEMM (on the golden's own operands, per-row error)
    and end to end: fp32 grade, below 1e-5 on the forces -- DESIGN section 8's claim for the format.  Per GEMM the bound is 2e-6
    of the row's largest output: gamd_f16x3.h gives 2^-22 = 2.4e-7 per operand and 7e-7 for operands below 0.125 (subnormal lo),
    two operands per product, and the dropped lo x lo term is 2^-22 again; measured 3e-7 .. 6e-7."""
    sd, st, out, src, dst, _ = _run(name, torch.float64)
    F = torch.nn.functional
    p = "graph_conv.conv.0"
    hn = orc.node_norm(sd, "graph_conv.norm_layers.0", st["h"][0])
    t1 = F.silu(F.linear(st["e"], sd[p + ".edge_affine.mlp_layer.0.weight"], sd[p + ".edge_affine.mlp_layer.0.bias"]))
    gemms = {"encoder 1": (st["feat"], "edge_encoder.mlp_layer.0.weight"), "conv W1": (st["e"], p + ".edge_affine.mlp_layer.0.weight"),
             "conv W2": (t1, p + ".edge_affine.mlp_layer.2.weight"), "node S": (hn, p + ".src_affine.weight"),
             "decoder 1": (st["h"][-1], "graph_decoder.mlp_layer.0.weight")}
    for tag, (xx, wk) in gemms.items():
        mx = lc.row_stats(lp.linear_x3(xx, sd[wk]).numpy(), F.linear(xx, sd[wk]).numpy())[1]
        print(f"split error {name} {variant} {tag}: max row {mx:.3e}")
        assert 0 < mx < 2e-6, (tag, mx)
    err = rel_err(lp.forward_stages(sd, st["feat"], st["h"][0], src, dst, variant)["out"].numpy(), out.numpy())
    print(f"split error {name} {variant} end to end: {err:.3e}")
    assert 1e-9 < err < 1e-5, err


@pytest.mark.parametrize("case_id", [c.id for c in lc.CASES if c.edge_dtype == "f16x3"])
def test_no_split_operand_reaches_the_fp16_range(case_id):
    """The model (like the kernels, gamd_f16x3.h "Range") has no overflow path: every operand stays far below 65504."""
    big = lc.max_split_operand(case_id)
    print(f"largest split operand, {case_id}: {big:.3g}")
    assert big < 65504.0


def test_every_grade_bar_is_stricter_than_the_fixed_one():
    """MARGIN x yardstick < TOL for every statistic of every fp32-grade variant (the two controls' old bar was TOL)."""
    for v in lp.FP32_GRADE:
        y = lc.yardstick(v)
        print(f"yardstick {v}: " + ", ".join(f"{k} {y[k]:.3e}" for k in lc.GRADE_STATS))
        assert set(y) == set(lc.GRADE_STATS)
        for k in lc.GRADE_STATS:
            assert 0 < lc.MARGIN * y[k] < lc.TOL, (v, k, y[k])


@pytest.mark.parametrize("case_id", ["f32-lj-3", "f32-lj-1", "ctl-f32", "f32-water-d256", "f16x3-lj-3", "ctl-f16x3", "f16x3-wide-256"])
def test_the_unmutated_grade_reference_breaks_none(case_id):
    c = lc.BY_ID[case_id]
    stats = lc.compare_with_reference(case_id, lc.weights(case_id)[1], torch.float64, c.variant)
    assert lc.criteria(stats, lc.yardstick(c.variant), fp32_grade=True) == []
    # identical but for layer 0 of a multi-layer hoisted case, where the run under test applies W4 per atom (M0, c0 rounded to
    # fp32 on the host) and the reference per edge: the same map in real arithmetic
    upd = max(stats.pop("upd_med"), stats.pop("upd_max"))
    assert max(stats.values()) == 0.0 and (0 < upd < 1e-7 if c.hoisted and c.cfg.conv_layer > 1 else upd == 0.0)
    own = lc.yardstick_of(case_id)                 # and the variant's own fp32 run passes, as it defines the yardstick
    assert lc.criteria(own, lc.yardstick(c.variant), fp32_grade=True) == []


def _last(case_id):
    return lc.BY_ID[case_id].cfg.conv_layer - 1


# (mutation, case) -> how the float64 reference is made wrong.  One LJ and one water case each; the hoisted form exists in LJ
# models only (mutation 5) and the stale table needs a middle layer (mutation 6: l = 1 of the 3-layer LJ case).
GRADE_MUTATIONS = [
    ("1_silu_4e-6", "f32-lj-3"), ("1_silu_4e-6", "ctl-f32"),
    ("2_erf_for_fit", "f32-lj-3"), ("2_erf_for_fit", "ctl-f32"),
    ("3_lo_subnormals_flushed", "f16x3-lj-3"), ("3_lo_subnormals_flushed", "ctl-f16x3"), ("3_lo_subnormals_flushed", "f16x3-wide-256"),
    ("4_wlo_xhi_kstep_dropped", "f16x3-lj-3"), ("4_wlo_xhi_kstep_dropped", "ctl-f16x3"), ("4_wlo_xhi_kstep_dropped", "f16x3-wide-256"),
    ("5_hoisted_d_off_by_one", "f32-lj-3"), ("5_hoisted_d_off_by_one", "f32-lj-1"),
    ("6_stale_node_tables", "f32-lj-3"),
]


@pytest.mark.parametrize("mutation,case_id", GRADE_MUTATIONS)
def test_a_subtly_wrong_fp32_grade_kernel_breaks_a_criterion(mutation, case_id):
    """The mutated float64 reference plays the device, per stage on the unmutated reference's inputs.  For mutations 1 and 2 the
    old fixed bar (every statistic < 1e-5) is evaluated next to the new one: it must NOT see the 4e-6 SiLU error."""
    c = lc.BY_ID[case_id]
    kw, spec = {}, c.variant
    if mutation.startswith("1"):
        spec = lp.mutated(c.variant, silu_err=(_last(case_id), 1, 4e-6))
    elif mutation.startswith("2"):
        spec = lp.mutated(c.variant, gelu="erf")
    elif mutation.startswith("3"):
        spec = lp.mutated(c.variant, flush_lo_subnormal=True)
    elif mutation.startswith("4"):
        spec = lp.mutated(c.variant, drop_wlo_kstep=(_last(case_id), 3, 3, 1))
    elif mutation.startswith("5"):
        kw = dict(d_off_by_one=True)
    else:
        kw = dict(stale_layer=1)
    stats = lc.compare_with_reference(case_id, lc.weights(case_id)[1], torch.float64, spec, **kw)
    yard = lc.yardstick(c.variant)
    bad = lc.criteria(stats, yard, fp32_grade=True)
    old = [k for k in lc.GRADE_STATS if not k.startswith("upd") and not k.endswith("_row") and not stats[k] < lc.TOL]
    print(f"{mutation} on {case_id}: breaks {bad}; the fixed 1e-5 on the old statistics: {old or 'nothing'}; " +
          ", ".join(f"{k} {stats[k]:.3e} (bar {lc.bar(k, yard, True):.3e})" for k in lc.GRADE_STATS))
    assert bad, (mutation, stats, yard)
    if mutation.startswith("1"):
        assert old == [], old                          # the point of the change
        assert 3e-6 < stats["agg_max"] < 1e-5          # the size measured in the issue: rows moved by 3e-6 .. 6e-6
    if mutation.startswith("2"):
        assert bad == ["enc_bias"] and old == []       # 1.2e-7 absolute with a sign: no maximum sees it, the mean over the edges does
    if mutation.startswith("6"):
        assert "upd_max" in bad or "upd_med" in bad    # only the per-layer check localises it
