"""Each edge, encoder and node kernel judged alone against the float64 reference that restates its arithmetic
(oracle/gamd_oracle_lp.py): operand-rounded for bf16, operand-split for split-fp16, plain with the kernels' GELU fit for fp32.

Every stage is fed what the DEVICE produced in front of it (the existing debug getters of an engine built with
keep_stages=True), so the errors of one kernel do not reach the next:

  encoder      debug_feat -> reference e           against debug_e
  conv edge    debug_e bits, debug_h(L-1)          against the pieces of debug_partial, summed per destination in float64
               (a one-layer hoisted LJ model: the pieces hold sums of T3 and are compared with conv_edge_t3_sum)
  layer l<L-1  debug_e, debug_h(l)                 reference update h_{l+1} - h_l against debug_h(l+1) - debug_h(l), in float64
               (fp32-grade families: the only place a middle layer's edge kernel, and the hoisted layer 0 of a multi-layer
               model, is judged on its own inputs)
  node         those sums, debug_h(L-1)            against debug_h(L)
  decoder      debug_h(L)                          against the returned normalised forces
  end to end   the whole reference from positions  against the returned forces (printed next to the old figure against fp32)

Every edge-feature kernel family fills the FEAT getter (edge_encode*.hip, wide.hip, wide_d.hip all write feat_dbg), so no case
computes its features on the host for the per-stage checks; the end-to-end reference forms them in fp32 with
gamd_oracle.edge_features*, as the device does.

No bf16 bar is a fixed number: each flip-driven statistic is held to lp_cases.MARGIN x the same statistic of the reference in
fp32 against itself in float64 (lp_cases.yardstick, computed on the CPU, maximum over the cases of the variant); the
aggregate's median row, the node kernel and the decoder are held to the suite's fp32 bar.  In the fp32 and split-fp16 families
EVERY statistic (lp_cases.GRADE_STATS) is held to MARGIN x its yardstick, with the suite's 1e-5 as the outer bound only.
tests/test_lp_reference.py shows on the CPU that reverting any one rounding point, or any of six subtly wrong fp32-grade kernels,
breaks a criterion.  Every engine is one box in exact neighbour mode.  profiles/lp_stage_parity.md records the figures."""
import json

import numpy as np
import pytest
import torch

import gamd_oracle_lp as lp
import lp_cases as lc
from helpers import per_atom_err, pieces_of_csr, rel_err

pytestmark = pytest.mark.gpu

_measured = {}
_engine_failed = []          # an engine call that raised: no further case touches the device in this process


def _measure(case_id):
    """One forward of the case's engine and every statistic of it (cached: the five tests of a case share it)."""
    if case_id not in _measured:
        try:
            _measured[case_id] = _measure_once(case_id)
        except BaseException as exc:               # a case that fails is not run again by the other four tests of it
            _measured[case_id] = exc
    if isinstance(_measured[case_id], BaseException):
        raise _measured[case_id]
    return _measured[case_id]


def _measure_once(case_id):
    from gamd_amd.engine import GamdForce
    assert not _engine_failed, f"not run: the engine raised in case {_engine_failed[0]}"
    c = lc.BY_ID[case_id]
    sd32, sd64 = lc.weights(case_id)
    pos, box, species, bonds = lc.system(c.system)
    n, L, H = pos.shape[0], c.cfg.conv_layer, c.cfg.encoding_size
    bond = bonds if c.cfg.use_bond else None
    _engine_failed.append(case_id)
    # kernel_select and small_tile_limit select the family (lp_cases.Case.family); the library refuses bits it does not know
    eng = GamdForce(sd32, n, box, c.cutoff, bond=bond, nbr_flavour=c.flavour, keep_stages=True, cfg=c.cfg, edge_dtype=c.edge_dtype,
                    kernel_select=c.kernel_select, small_tile_limit=c.small_tile_limit)
    try:
        out = eng.forward(torch.from_numpy(pos), species=species).cpu().numpy()
        if c.fp32_grade:
            # the latency / throughput choice is made from the LAST known edge count: the second call is the one that is sure to
            # sit on the intended side, and the two kinds of kernel are bit-identical
            first, out = out, eng.forward(torch.from_numpy(pos), species=species).cpu().numpy()
            assert np.array_equal(first, out)
        n_edges, n_pieces, _ = eng.counts()
        perm = eng.debug_perm().astype(np.int64)
        row_ptr, col = eng.debug_csr()
        feat_dev, e_dev = eng.debug_feat(c.cfg.edge_in), eng.debug_e()
        pieces = eng.debug_partial()[:, :H].astype(np.float64)
        h_dev = [eng.debug_h(l) if (l > 0 or L > 1) else None for l in range(L + 1)] if c.fp32_grade else \
            [None] * (L - 1) + [eng.debug_h(L - 1) if L > 1 else None, eng.debug_h(L)]
        torch.cuda.synchronize()
        _engine_failed.pop()
    finally:
        eng.close()
    assert np.isfinite(out).all() and row_ptr[-1] == n_edges and (col < n).all()
    tiles = (n_edges + 31) // 32
    assert tiles <= 512                       # gamd_host.h small_tile_limit: the fp32 latency kernels unless small_tile_limit = -1
    deg = np.diff(row_ptr.astype(np.int64))
    dst = torch.from_numpy(perm[np.repeat(np.arange(n), deg)])                  # original atom ids, CSR order
    src = torch.from_numpy(perm[col.astype(np.int64)])
    node_in = lc.node_input(species) if c.cfg.kind != "lj" else None
    s = {"edges": int(n_edges), "pieces": int(n_pieces), "tiles": int(tiles)}
    var = c.variant if c.fp32_grade else None          # node kernel and decoder: restated for the fp32-grade families only

    # 1. encoder, from the device's features
    e_ref = lp.encode_edges(sd64, torch.from_numpy(feat_dev).double(), c.variant)
    s["enc_bits"], s["enc_max"] = lc.enc_stats(e_dev, e_ref)
    if c.fp32_grade:
        s["enc_bits"] = 0.0                                                     # fp32-grade e: no bf16 patterns to compare
        s["enc_bias"] = lc.enc_bias(e_dev, e_ref)
    e64 = torch.from_numpy(e_dev).double()

    # 2. the last conv layer's edge kernel, from the device's e bits and h_{L-1}
    piece, piece_row, count = pieces_of_csr(row_ptr)
    assert count == n_pieces, (count, n_pieces)
    agg_dev = np.zeros((n, H))
    np.add.at(agg_dev, perm[piece_row], pieces)
    # An atom without edges owns no piece, so the device has no aggregate row of it to read: that its sum is exactly zero is held
    # by the node check below, whose reference gives such an atom agg = 0 (the sparse and tiny cases have such atoms).
    h_prev = h_dev[L - 1]
    if h_prev is None:
        h_prev = lp.initial_h(sd64, n, None if node_in is None else node_in.double()).numpy()      # h_0, formed on the host
    h_prev = torch.from_numpy(np.asarray(h_prev, dtype=np.float64))
    hoisted_last = c.hoisted and L == 1                 # the pieces hold sums of T3 rows (GamdForce.debug_partial)
    if hoisted_last:
        agg_ref = lp.conv_edge_t3_sum(sd64, e64, h_prev, src, dst, c.variant).numpy()
    else:
        agg_ref = lp.conv_edge_agg(sd64, L - 1, e64, h_prev, src, dst, c.variant).numpy()
    s["agg_med"], s["agg_max"], s["agg_rows"] = lc.row_stats(agg_dev, agg_ref)
    assert not agg_ref[perm[deg == 0]].any()

    # 2b. every earlier layer, fp32-grade families: the update h_{l+1} - h_l in float64 on both sides
    if c.fp32_grade:
        s["upd"] = []
        for l in range(L - 1):
            h_l = torch.from_numpy(h_dev[l].astype(np.float64))
            upd_ref = lp.node_update(sd64, l, lp.conv_edge_agg(sd64, l, e64, h_l, src, dst, c.variant), h_l, c.variant) - h_l
            med, mx, _ = lc.row_stats(h_dev[l + 1].astype(np.float64) - h_dev[l].astype(np.float64), upd_ref.numpy())
            s["upd"].append([med, mx])
        s["upd_med"] = max([u[0] for u in s["upd"]], default=0.0)
        s["upd_max"] = max([u[1] for u in s["upd"]], default=0.0)

    # 3. node kernel, from the device's own sums; 4. decoder, from the device's h_L
    h_last = h_dev[L]
    if hoisted_last:
        d_in = torch.zeros(n, dtype=torch.int64)
        d_in[torch.from_numpy(perm)] = torch.from_numpy(deg)
        h_ref = lp.node_update_hoisted(sd64, torch.from_numpy(agg_dev), d_in, h_prev, c.variant).numpy()
    else:
        h_ref = lp.node_update(sd64, L - 1, torch.from_numpy(agg_dev), h_prev, var).numpy()
    s.update(lc.stage_stats("node", h_last, h_ref))
    out_ref = lp.decode(sd64, torch.from_numpy(h_last).double(), var).numpy()
    s.update(lc.stage_stats("dec", out, out_ref))
    # where the decoder's per-row error sits: the three worst atoms as (|f_i| / max |f|, |df_i| / |f_i|)
    fn, dn = np.linalg.norm(out_ref, axis=1), np.linalg.norm(out - out_ref, axis=1)
    worst = np.argsort(-(dn / np.maximum(fn, 1e-3 * fn.max())))[:3]
    s["dec_worst"] = [[float(fn[i] / fn.max()), float(dn[i] / fn[i])] for i in worst]

    # 5. end to end: the whole reference in float64 from the positions (features in fp32, as the device forms them)
    pos32 = torch.from_numpy(pos)
    feat32 = lc.features(sd32, pos32, src, dst, box, bond)
    h0 = lp.initial_h(sd32, n, node_in)
    s["e2e"] = rel_err(out, lp.forward_stages(sd64, feat32.double(), h0.double(), src, dst, c.variant)["out"].numpy())
    s["vs_fp32"] = rel_err(out, lp.forward_stages(sd32, feat32, h0, src, dst, None)["out"].numpy())   # the old statement

    yard = lc.yardstick(c.variant)
    keys = lc.GRADE_STATS if c.fp32_grade else lc.FLIP_STATS
    ratio = {k: (s[k] / yard[k] if yard[k] > 0 else None) for k in keys}
    rec = {"case": case_id, "variant": c.variant, "family": c.family, "device": s, "yardstick": yard, "ratio": ratio}
    print("LPSTAGE " + json.dumps(rec))
    for k in keys:
        r = f"{ratio[k]:.2f} x yardstick {yard[k]:.3e}" if ratio[k] is not None else "yardstick 0"
        print(f"  {case_id:13s} {k:9s} device {s[k]:.3e}  bar {lc.bar(k, yard, c.fp32_grade):.3e}  ({r})")
    print(f"  {case_id:13s} agg_med {s['agg_med']:.3e}  node {s['node_max']:.3e} / p99 {s['node_p99']:.3e}  decoder {s['dec_max']:.3e} / "
          f"p99 {s['dec_p99']:.3e}  against fp32 {s['vs_fp32']:.3e}")
    print(f"  {case_id:13s} decoder, worst atoms (|f|/max|f|, |df|/|f|): " + ", ".join(f"({a:.3f}, {b:.2e})" for a, b in s["dec_worst"]))
    return s, yard


def _held(case_id, s, yard, *keys):
    """Each of `keys` against its bar (lp_cases.bar: MARGIN x yardstick where the criteria derive it, TOL elsewhere)."""
    g = lc.BY_ID[case_id].fp32_grade
    bad = {k: (s[k], lc.bar(k, yard, g)) for k in keys if not (s[k] <= lc.bar(k, yard, g) and (s[k] < lc.TOL or not g))}
    assert not bad, (bad, s)


IDS = [c.id for c in lc.CASES]


@pytest.mark.parametrize("case_id", IDS)
def test_encoder_against_the_operand_rounded_reference(case_id):
    s, yard = _measure(case_id)
    if lc.BY_ID[case_id].fp32_grade:
        _held(case_id, s, yard, "enc_max", "enc_bias")           # max row error; per-feature signed mean over the edges
        return
    assert s["enc_bits"] <= lc.bar("enc_bits", yard, False), s   # share of elements whose bf16 bit patterns differ
    assert s["enc_max"] <= lc.bar("enc_max", yard, False), s     # max_i max_k |d| / max_k |e_ref[i]|


@pytest.mark.parametrize("case_id", IDS)
def test_last_conv_edge_kernel_against_the_operand_rounded_reference(case_id):
    s, yard = _measure(case_id)
    assert s["agg_rows"] > 0
    assert s["agg_med"] < lc.TOL, s                              # the median row carries no flipped rounding: anything systematic
    _held(case_id, s, yard, "agg_max", *(["agg_med"] if lc.BY_ID[case_id].fp32_grade else []))


@pytest.mark.parametrize("case_id", [i for i in lc.GRADE_IDS if lc.BY_ID[i].cfg.conv_layer > 1])
def test_earlier_layers_from_the_device_h(case_id):
    """Every layer below the last: the device's update h_{l+1} - h_l against the reference layer run on debug_e and debug_h(l)."""
    s, yard = _measure(case_id)
    assert len(s["upd"]) == lc.BY_ID[case_id].cfg.conv_layer - 1
    _held(case_id, s, yard, "upd_med", "upd_max")


@pytest.mark.parametrize("case_id", IDS)
def test_node_kernel_from_the_device_sums(case_id):
    s, yard = _measure(case_id)
    assert s["node_max"] < lc.TOL and s["node_p99"] < lc.P99_TOL, s
    if lc.BY_ID[case_id].fp32_grade:
        _held(case_id, s, yard, "node_max", "node_p99", "node_row")


@pytest.mark.parametrize("case_id", IDS)
def test_decoder_from_the_device_h(case_id):
    s, yard = _measure(case_id)
    assert s["dec_max"] < lc.TOL, s
    if lc.BY_ID[case_id].dec_p99_held:
        assert s["dec_p99"] < lc.P99_TOL, s
    if lc.BY_ID[case_id].fp32_grade:
        _held(case_id, s, yard, "dec_max", "dec_p99", "dec_row")


@pytest.mark.parametrize("case_id", IDS)
def test_end_to_end_against_the_operand_rounded_reference(case_id):
    s, yard = _measure(case_id)
    c = lc.BY_ID[case_id]
    _held(case_id, s, yard, "e2e")
    if not c.fp32_grade:
        assert s["vs_fp32"] > 1e-5, s                            # really the reduced-precision path (its budget against fp32, BF16_TOL, is
                                                                 # tests/test_gpu_parity.py's to hold)
    else:
        assert s["vs_fp32"] < lc.TOL, s                          # and the old statement of fp32 parity still holds
    assert lc.criteria(s, yard, c.dec_p99_held, c.fp32_grade) == []
