"""The operand-rounded reference of the bf16 edge kernels (oracle/gamd_oracle_lp.py) checked against itself and the oracle.
CPU only.

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


@pytest.mark.parametrize("case_id", [c.id for c in lc.CASES if c.edge_dtype != "f16x3"])
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
