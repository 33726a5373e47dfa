"""Each reduced-precision edge kernel judged alone against the operand-rounded float64 reference (oracle/gamd_oracle_lp.py).

Every stage is fed what the DEVICE produced in front of it (the existing debug getters of an engine built with
keep_stages=True), so the errors of one kernel do not reach the next:

  encoder      debug_feat -> reference e           against debug_e
  conv edge    debug_e bits, debug_h(L-1)          against the pieces of debug_partial, summed per destination in float64
  node         those sums, debug_h(L-1)            against debug_h(L)
  decoder      debug_h(L)                          against the returned normalised forces
  end to end   the whole reference from positions  against the returned forces (printed next to the old figure against fp32)

Every edge-feature kernel family fills the FEAT getter (edge_encode*.hip, wide.hip, wide_d.hip all write feat_dbg), so no case
computes its features on the host for the per-stage checks; the end-to-end reference forms them in fp32 with
gamd_oracle.edge_features*, as the device does.

No bf16 bar is a fixed number: each flip-driven statistic is held to lp_cases.MARGIN x the same statistic of the reference in
fp32 against itself in float64 (lp_cases.yardstick, computed on the CPU, maximum over the cases of the variant); the
aggregate's median row, the node kernel and the decoder are held to the suite's fp32 bar; so is every statistic of the fp32 and
split-fp16 controls.  tests/test_lp_reference.py shows on the CPU that reverting any one rounding point breaks a criterion.
Every engine is one box in exact neighbour mode.  profiles/lp_stage_parity.md records the figures."""
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
    eng = GamdForce(sd32, n, box, c.cutoff, bond=bond, nbr_flavour=c.flavour, keep_stages=True, cfg=c.cfg, edge_dtype=c.edge_dtype)
    try:
        out = eng.forward(torch.from_numpy(pos), species=species).cpu().numpy()
        n_edges, n_pieces, _ = eng.counts()
        perm = eng.debug_perm().astype(np.int64)
        row_ptr, col = eng.debug_csr()
        feat_dev, e_dev = eng.debug_feat(c.cfg.edge_in), eng.debug_e()
        pieces = eng.debug_partial()[:, :H].astype(np.float64)
        h_prev = eng.debug_h(L - 1) if L > 1 else None
        h_last = eng.debug_h(L)
        torch.cuda.synchronize()
        _engine_failed.pop()
    finally:
        eng.close()
    assert np.isfinite(out).all() and row_ptr[-1] == n_edges and (col < n).all()
    deg = np.diff(row_ptr.astype(np.int64))
    dst = torch.from_numpy(perm[np.repeat(np.arange(n), deg)])                  # original atom ids, CSR order
    src = torch.from_numpy(perm[col.astype(np.int64)])
    node_in = lc.node_input(species) if c.cfg.kind != "lj" else None
    s = {"edges": int(n_edges), "pieces": int(n_pieces)}

    # 1. encoder, from the device's features
    e_ref = lp.encode_edges(sd64, torch.from_numpy(feat_dev).double(), c.variant)
    s["enc_bits"], s["enc_max"] = lc.enc_stats(e_dev, e_ref)
    if c.variant is None:
        s["enc_bits"] = 0.0                                                     # fp32-grade e: no bf16 patterns to compare

    # 2. the last conv layer's edge kernel, from the device's e bits and h_{L-1}
    piece, piece_row, count = pieces_of_csr(row_ptr)
    assert count == n_pieces, (count, n_pieces)
    agg_dev = np.zeros((n, H))
    np.add.at(agg_dev, perm[piece_row], pieces)
    # An atom without edges owns no piece, so the device has no aggregate row of it to read: that its sum is exactly zero is held
    # by the node check below, whose reference gives such an atom agg = 0 (the sparse and tiny cases have such atoms).
    if h_prev is None:
        h_prev = lp.initial_h(sd64, n, None if node_in is None else node_in.double()).numpy()      # h_0, formed on the host
    h_prev = torch.from_numpy(np.asarray(h_prev, dtype=np.float64))
    agg_ref = lp.conv_edge_agg(sd64, L - 1, torch.from_numpy(e_dev).double(), h_prev, src, dst, c.variant).numpy()
    s["agg_med"], s["agg_max"], s["agg_rows"] = lc.row_stats(agg_dev, agg_ref)
    assert not agg_ref[perm[deg == 0]].any()

    # 3. node kernel, from the device's own sums; 4. decoder, from the device's h_L
    h_ref = lp.node_update(sd64, L - 1, torch.from_numpy(agg_dev), h_prev).numpy()
    s["node_max"], s["node_p99"] = rel_err(h_last, h_ref), per_atom_err(h_last, h_ref)[1]
    out_ref = lp.decode(sd64, torch.from_numpy(h_last).double()).numpy()
    s["dec_max"], s["dec_p99"] = rel_err(out, out_ref), per_atom_err(out, out_ref)[1]
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

    yard = lc.yardstick(c.variant) if c.variant else None
    rec = {"case": case_id, "variant": c.variant or c.edge_dtype, "device": s, "yardstick": yard}
    print("LPSTAGE " + json.dumps(rec))
    for k in lc.FLIP_STATS:
        bar = lc.MARGIN * yard[k] if yard else lc.TOL
        ratio = f"{s[k] / yard[k]:.2f} x yardstick {yard[k]:.3e}" if yard and yard[k] > 0 else "control"
        print(f"  {case_id:13s} {k:9s} device {s[k]:.3e}  bar {bar:.3e}  ({ratio})")
    print(f"  {case_id:13s} agg_med {s['agg_med']:.3e}  node {s['node_max']:.3e} / p99 {s['node_p99']:.3e}  decoder {s['dec_max']:.3e} / "
          f"p99 {s['dec_p99']:.3e}  against fp32 {s['vs_fp32']:.3e}")
    print(f"  {case_id:13s} decoder, worst atoms (|f|/max|f|, |df|/|f|): " + ", ".join(f"({a:.3f}, {b:.2e})" for a, b in s["dec_worst"]))
    return s, yard


def _bar(k, yard):
    return lc.MARGIN * yard[k] if yard is not None and k in lc.FLIP_STATS else lc.TOL


IDS = [c.id for c in lc.CASES]


@pytest.mark.parametrize("case_id", IDS)
def test_encoder_against_the_operand_rounded_reference(case_id):
    s, yard = _measure(case_id)
    assert s["enc_bits"] <= _bar("enc_bits", yard), s            # share of elements whose bf16 bit patterns differ
    assert s["enc_max"] <= _bar("enc_max", yard), s              # max_i max_k |d| / max_k |e_ref[i]|


@pytest.mark.parametrize("case_id", IDS)
def test_last_conv_edge_kernel_against_the_operand_rounded_reference(case_id):
    s, yard = _measure(case_id)
    assert s["agg_rows"] > 0
    assert s["agg_med"] < lc.TOL, s                              # the median row carries no flipped rounding: anything systematic
    assert s["agg_max"] <= _bar("agg_max", yard), s


@pytest.mark.parametrize("case_id", IDS)
def test_node_kernel_from_the_device_sums(case_id):
    s, _ = _measure(case_id)
    assert s["node_max"] < lc.TOL and s["node_p99"] < lc.P99_TOL, s


@pytest.mark.parametrize("case_id", IDS)
def test_decoder_from_the_device_h(case_id):
    s, _ = _measure(case_id)
    assert s["dec_max"] < lc.TOL, s
    if lc.BY_ID[case_id].dec_p99_held:
        assert s["dec_p99"] < lc.P99_TOL, s


@pytest.mark.parametrize("case_id", IDS)
def test_end_to_end_against_the_operand_rounded_reference(case_id):
    s, yard = _measure(case_id)
    assert s["e2e"] <= _bar("e2e", yard), s
    if yard is not None:
        assert s["vs_fp32"] > 1e-5, s                            # really the reduced-precision path (its budget against fp32, BF16_TOL, is
                                                                 # tests/test_gpu_parity.py's to hold)
    assert lc.criteria(s, yard, lc.BY_ID[case_id].dec_p99_held) == []
