"""Cases, statistics and criteria shared by tests/test_lp_reference.py (CPU) and tests/test_gpu_lp_stages.py (GPU): each
edge, node and encoder kernel judged alone against the float64 reference of oracle/gamd_oracle_lp.py that restates its
arithmetic -- operand-rounded for the bf16 kernels, operand-split for the split-fp16 ones, plain for the fp32 ones.
update_edge models are out of scope of the per-stage checks: the e of their layers above the first never leaves the device
(no getter reads e_frag2); they keep their own tests (tests/test_gpu_round4.py, tests/test_gpu_parity.py).
Test infrastructure; not a test module."""
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional

import numpy as np
import torch

import gamd_oracle as orc
import gamd_oracle_lp as lp
from helpers import per_atom_err, rel_err
from gamd_amd import workloads
from gamd_amd.weights import ModelConfig, make_state_dict

TOL = 1e-5             # the suite's fp32 bar (tests/test_gpu_parity.py)
P99_TOL = 1e-5         # per-row p99 (helpers.per_atom_err), as __graft_entry__.smoke() holds it
MARGIN = 4.0           # device statistic <= MARGIN x the reference's own fp32-against-f64 statistic (see `criteria`)


@dataclass(frozen=True)
class Case:
    id: str
    cfg: ModelConfig
    seed: int
    length: tuple          # (length_mean, length_std) of the seeded weights
    system: str            # "lj258" | "water90" | "sparse128" | "tiny7"
    cutoff: float
    flavour: str = "jaxmd"
    edge_dtype: str = "bf16"
    variant: Optional[str] = "bf16_128"
    dec_p99_held: bool = True      # False: the decoder's per-row p99 is recorded, not asserted (see dynbox-noexp-s27)
    small_tile_limit: int = 0      # engine keyword: 0 the latency kernels (the default at these sizes), -1 the throughput kernels
    kernel_select: int = 0         # engine keyword: 1 generic width, 2 half quantum (k_conv_edge_wide16), 4 no layer-0 hoist

    @property
    def hidden_dim(self) -> int:
        return self.cfg.hidden_dim

    @property
    def fp32_grade(self) -> bool:
        return self.variant in lp.FP32_GRADE

    @property
    def generic_width(self) -> bool:
        """The library's wide_conv: any width but 128 / 128 / 128 with expanded RBFs, or forced."""
        g = self.cfg
        return bool(self.kernel_select & 1 and self.edge_dtype == "f32") or g.n_rbf == 0 or \
            (g.encoding_size, g.hidden_dim, g.edge_embedding_dim) != (128, 128, 128)

    @property
    def hoisted(self) -> bool:
        """Layer 0 runs in its hoisted form (the library's l0_hoist; GamdForce.debug_partial's docstring)."""
        return self.cfg.kind == "lj" and self.edge_dtype == "f32" and not self.generic_width and not self.kernel_select & 4

    @property
    def family(self) -> str:
        """The kernels the case is meant to reach (printed; what the library lets a test verify of it is asserted on the GPU)."""
        if self.edge_dtype != "f32":
            return self.edge_dtype + ("_wide" if self.generic_width else "_128")
        if self.cfg.hidden_dim > 128:
            return "f32_wide_d"
        tp = "throughput" if self.small_tile_limit < 0 else "latency"
        if self.generic_width:
            return "f32_wide16" if self.kernel_select & 2 else "f32_wide_" + tp
        return "f32_128_" + tp + ("_l0" if self.hoisted else "")


def _w(**kw):
    return ModelConfig(kind="water", conv_layer=2, **kw)


def _lj(layers, **kw):
    return ModelConfig(kind="lj", conv_layer=layers, **kw)


_W256 = dict(encoding_size=256, hidden_dim=128, edge_embedding_dim=256)
_WODD = dict(encoding_size=96, hidden_dim=64, edge_embedding_dim=160)

# The smallest shapes that still reach every code path of the bf16 kernels (one row per family and edge case):
CASES = [
    # layer 0 of an LJ model: every atom has the SAME hn / S / D row (h_0 = node_emb, formed on the host).  One fp16 rounding
    # of those 3 x 128 shared values that an fp32-sized error can flip shows in EVERY row of the aggregate, the median
    # included; about half of all weight seeds have such a value.  Seed 169 has none within reach of 3 fp32 epsilons
    # (test_lp_reference.py::test_lj_layer0_case_is_well_conditioned holds it to that), so the median criterion means here
    # what it means everywhere else.
    Case("lj-1", ModelConfig(kind="lj", conv_layer=1), 169, (5.0, 1.7), "lj258", 7.5),
    Case("lj-3", ModelConfig(kind="lj", conv_layer=3), 22, (5.0, 1.7), "lj258", 7.5),        # last layer fed by debug_h(2)
    Case("water-bond", _w(use_bond=True), 23, (2.9, 1.1), "water90", 4.2),                   # 45 features, K padded to 48, species tables
    Case("bn", ModelConfig(kind="lj", conv_layer=2, use_layer_norm=False), 24, (5.0, 1.7), "lj258", 7.5),   # the affine-norm hn
    Case("wide-256", _w(encoding_size=256, hidden_dim=128, edge_embedding_dim=256), 25, (2.9, 1.1), "water90", 4.2,
         variant="bf16_wide"),                                                               # wide_lp.hip, EHT = HT = 2
    Case("wide-odd", _w(encoding_size=96, hidden_dim=64, edge_embedding_dim=160), 26, (2.9, 1.1), "water90", 4.2,
         variant="bf16_wide"),                                                               # zero-padded blocks
    Case("dynbox-noexp", ModelConfig(kind="dynbox", conv_layer=2, encoding_size=256, hidden_dim=128, edge_embedding_dim=256, n_rbf=0),
         30, (2.9, 1.1), "water90", 4.2, flavour="torch", variant="bf16_wide"),              # 4 features, no self edges
    # The same model with weight seed 27, the one this case was first written with.  Its forces nearly cancel on a few atoms: the
    # decoder's per-row p99 is 5.9e-6 between the reference in fp32 and in float64 before any kernel is involved (the other
    # cases: below 2e-6) and 1.09e-5 on the device, on atoms that carry 4 - 5 % of the
    # largest force and are off by 5e-7 of it (profiles/lp_stage_parity.md, note 5).  Kept so that those weights stay judged: every statistic but that p99 is held as usual.
    Case("dynbox-noexp-s27", ModelConfig(kind="dynbox", conv_layer=2, encoding_size=256, hidden_dim=128, edge_embedding_dim=256, n_rbf=0),
         27, (2.9, 1.1), "water90", 4.2, flavour="torch", variant="bf16_wide", dec_p99_held=False),
    Case("sparse", _w(), 28, (2.0, 0.6), "sparse128", 3.0, flavour="torch"),                 # isolated atoms, rows shorter than a chunk
    Case("tiny", _w(), 28, (2.0, 0.6), "tiny7", 3.0, flavour="torch"),                       # one partly filled tile, padding slots
    # ---- the fp32-grade families: every statistic held to MARGIN x its yardstick (criteria) ----
    # fp32, 128 / 128 / 128, latency kernels (k_edge_encode_small, k_conv_edge_small, _small_l0)
    Case("ctl-f32", _w(), 29, (2.9, 1.1), "water90", 4.2, edge_dtype="f32", variant="f32"),
    Case("f32-water-bond", _w(use_bond=True), 23, (2.9, 1.1), "water90", 4.2, edge_dtype="f32", variant="f32"),            # 45 features
    Case("f32-lj-3", _lj(3), 22, (5.0, 1.7), "lj258", 7.5, edge_dtype="f32", variant="f32"),          # hoisted layer 0 through the layer chain
    Case("f32-lj-1", _lj(1), 169, (5.0, 1.7), "lj258", 7.5, edge_dtype="f32", variant="f32"),         # the hoisted layer is the last: sum T3 pieces
    Case("f32-bn", _lj(2, use_layer_norm=False), 24, (5.0, 1.7), "lj258", 7.5, edge_dtype="f32", variant="f32"),
    Case("f32-bn5", _lj(5, use_layer_norm=False), 31, (5.0, 1.7), "lj258", 7.5, edge_dtype="f32", variant="f32"),
    # fp32, 128 / 128 / 128, throughput kernels (k_edge_encode, k_conv_edge, _l0)
    Case("f32-water-tp", _w(), 29, (2.9, 1.1), "water90", 4.2, edge_dtype="f32", variant="f32", small_tile_limit=-1),
    Case("f32-lj-3-tp", _lj(3), 22, (5.0, 1.7), "lj258", 7.5, edge_dtype="f32", variant="f32", small_tile_limit=-1),
    Case("f32-tiny-tp", _w(), 28, (2.0, 0.6), "tiny7", 3.0, flavour="torch", edge_dtype="f32", variant="f32", small_tile_limit=-1),
    Case("f32-sparse-tp", _w(), 28, (2.0, 0.6), "sparse128", 3.0, flavour="torch", edge_dtype="f32", variant="f32", small_tile_limit=-1),
    # the general form of layer 0
    Case("f32-lj-3-nohoist", _lj(3), 22, (5.0, 1.7), "lj258", 7.5, edge_dtype="f32", variant="f32", kernel_select=4),
    # generic widths (wide.hip, wide16.hip)
    Case("f32-wide-256", _w(**_W256), 25, (2.9, 1.1), "water90", 4.2, edge_dtype="f32", variant="f32"),
    Case("f32-wide-256-tp", _w(**_W256), 25, (2.9, 1.1), "water90", 4.2, edge_dtype="f32", variant="f32", small_tile_limit=-1),
    Case("f32-wide-256-hq", _w(**_W256), 25, (2.9, 1.1), "water90", 4.2, edge_dtype="f32", variant="f32", kernel_select=2),
    Case("f32-wide-odd", _w(**_WODD), 26, (2.9, 1.1), "water90", 4.2, edge_dtype="f32", variant="f32"),              # zero-padded blocks
    Case("f32-dynbox-noexp", ModelConfig(kind="dynbox", conv_layer=2, n_rbf=0, **_W256), 30, (2.9, 1.1), "water90", 4.2, flavour="torch",
         edge_dtype="f32", variant="f32"),
    Case("f32-generic-128", _w(), 29, (2.9, 1.1), "water90", 4.2, edge_dtype="f32", variant="f32", kernel_select=1),
    # hidden_dim above 128 (wide_d.hip)
    Case("f32-lj-d192", _lj(2, hidden_dim=192), 32, (5.0, 1.7), "lj258", 7.5, edge_dtype="f32", variant="f32"),
    Case("f32-water-d256", _w(encoding_size=96, hidden_dim=256, edge_embedding_dim=200), 33, (2.9, 1.1), "water90", 4.2,
         edge_dtype="f32", variant="f32"),
    # split-fp16, 128 / 128 / 128 (k_edge_encode_f16x3, k_conv_edge_f16x3, k_node<true>)
    Case("ctl-f16x3", _w(), 29, (2.9, 1.1), "water90", 4.2, edge_dtype="f16x3", variant="f16x3_128"),
    Case("f16x3-water-bond", _w(use_bond=True), 23, (2.9, 1.1), "water90", 4.2, edge_dtype="f16x3", variant="f16x3_128"),
    Case("f16x3-lj-3", _lj(3), 22, (5.0, 1.7), "lj258", 7.5, edge_dtype="f16x3", variant="f16x3_128"),
    Case("f16x3-bn5", _lj(5, use_layer_norm=False), 31, (5.0, 1.7), "lj258", 7.5, edge_dtype="f16x3", variant="f16x3_128"),
    Case("f16x3-sparse", _w(), 28, (2.0, 0.6), "sparse128", 3.0, flavour="torch", edge_dtype="f16x3", variant="f16x3_128"),
    Case("f16x3-tiny", _w(), 28, (2.0, 0.6), "tiny7", 3.0, flavour="torch", edge_dtype="f16x3", variant="f16x3_128"),
    # split-fp16, generic widths (k_edge_encode_wide e_format 2, k_conv_edge_f16x3_wide, k_node_wide<HT, true>)
    Case("f16x3-wide-256", _w(**_W256), 25, (2.9, 1.1), "water90", 4.2, edge_dtype="f16x3", variant="f16x3_wide"),
    Case("f16x3-wide-odd", _w(**_WODD), 26, (2.9, 1.1), "water90", 4.2, edge_dtype="f16x3", variant="f16x3_wide"),
    Case("f16x3-dynbox-noexp", ModelConfig(kind="dynbox", conv_layer=2, n_rbf=0, **_W256), 30, (2.9, 1.1), "water90", 4.2, flavour="torch",
         edge_dtype="f16x3", variant="f16x3_wide"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
BF16_IDS = [c.id for c in CASES if not c.fp32_grade]
GRADE_IDS = [c.id for c in CASES if c.fp32_grade]


def system(name: str):
    """(pos f32 [N,3], box, species bool [N] or None, bonds or None)."""
    if name == "lj258":
        pos, box = workloads.lj_box(258, seed=77)
        return pos.astype(np.float32), box, None, None
    if name == "water90":
        pos, box, species, bonds = workloads.water_box(90, seed=78)
        return pos.astype(np.float32), box, species != 0, bonds
    rng = np.random.default_rng(79)
    if name == "sparse128":
        pos = rng.uniform(0.0, 16.0, (128, 3))
    elif name == "tiny7":
        pos = np.concatenate([4.0 + rng.uniform(0.0, 2.2, (6, 3)), np.array([[12.0, 12.0, 12.0]])])      # six neighbours and one isolated atom
    else:
        raise KeyError(name)
    return pos.astype(np.float32), 16.0, np.arange(pos.shape[0]) % 3 == 0, None


@lru_cache(maxsize=None)
def weights(case_id: str):
    c = BY_ID[case_id]
    sd = make_state_dict(c.cfg, c.seed, *c.length)
    return sd, lp.cast_state_dict(sd, torch.float64)


def features(sd32, pos32: torch.Tensor, src: torch.Tensor, dst: torch.Tensor, box, bonds) -> torch.Tensor:
    """The edge features in fp32 from fp32 positions, as the device forms them (centre = dst, neighbour = src)."""
    if "edge_expand.centers" in sd32:
        f = orc.edge_features(sd32, pos32, dst, src, box)
    else:
        d = orc._min_image(pos32[dst] - pos32[src], orc._box_tensor(box))
        f = orc.edge_features_from_dist(sd32, d, d.norm(dim=1))
    if bonds is not None:
        f = torch.cat((f, orc.bond_flags(dst, src, bonds).view(-1, 1).to(f.dtype)), dim=1)
    return f


def node_input(species):
    return None if species is None else torch.from_numpy(np.asarray(species, dtype=np.float32)).view(-1, 1)


# ---- statistics ------------------------------------------------------------------------------------------------------
def enc_stats(e, e_ref):
    """(share of elements whose bf16 bit patterns differ, max_i max_k |d| / max_k |e_ref[i]|)."""
    e, e_ref = torch.as_tensor(e).double(), torch.as_tensor(e_ref).double()
    if e.numel() == 0:
        return 0.0, 0.0
    share = float((lp.bf16_bits(e) != lp.bf16_bits(e_ref)).double().mean())
    row = (e - e_ref).abs().amax(dim=1) / e_ref.abs().amax(dim=1).clamp_min(1e-300)
    return share, float(row.max())


def enc_bias(e, e_ref) -> float:
    """max_k |mean_i d[i, k]| / mean_i max_k |e_ref[i]|: the signed error of each feature averaged over the edges.  Rounding noise
    averages out (fp32 against float64: 1e-8 at 10 000 edges, 5e-8 at 30); an error that has a sign does not -- the erf form of
    GELU against the kernels' fit, 1.2e-7 absolute per activation and invisible in the maximum row error, stands at 1e-6 here."""
    e, e_ref = torch.as_tensor(e).double(), torch.as_tensor(e_ref).double()
    if e.numel() == 0:
        return 0.0
    return float((e - e_ref).mean(dim=0).abs().max() / e_ref.abs().amax(dim=1).mean().clamp_min(1e-300))


def row_stats(a, ref):
    """Per-row error max_k |d| / max_k |ref[i]| over the rows with a non-zero reference: (median, max, rows counted)."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max(axis=1)
    keep = scale > 0
    if not keep.any():
        return 0.0, 0.0, 0
    r = np.abs(a - ref).max(axis=1)[keep] / scale[keep]
    return float(np.median(r)), float(r.max()), int(keep.sum())


FLIP_STATS = ("enc_bits", "enc_max", "agg_max", "e2e")      # driven by rare flipped rounding decisions: yardstick x MARGIN
# the fp32-grade families: EVERY statistic is held to MARGIN x its yardstick (and to TOL as an outer bound)
GRADE_STATS = ("enc_max", "enc_bias", "agg_med", "agg_max", "upd_med", "upd_max", "node_max", "node_p99", "node_row", "dec_max", "dec_p99",
               "dec_row", "e2e")


def stage_stats(prefix: str, a, ref) -> dict:
    """Node kernel / decoder: max-norm, per-row p99 and per-row maximum (helpers.per_atom_err: rows above 1e-3 of the largest)."""
    pa = per_atom_err(a, ref)
    return {prefix + "_max": rel_err(a, ref), prefix + "_p99": pa[1], prefix + "_row": pa[2]}


def bar(k: str, yard: Optional[dict], fp32_grade: bool) -> float:
    """The bar of statistic k: MARGIN x yardstick where the criteria derive it, the suite's TOL elsewhere and as the outer bound."""
    if fp32_grade:
        return min(MARGIN * yard[k], TOL)
    return MARGIN * yard[k] if yard is not None and k in FLIP_STATS else TOL


def criteria(stats: dict, yard: Optional[dict], dec_p99_held: bool = True, fp32_grade: bool = False) -> list:
    """Names of the criteria `stats` breaks.  `yard`: the variant's yardstick.

    fp32_grade (variants "f32", "f16x3_128", "f16x3_wide"): every statistic of GRADE_STATS is held to MARGIN x its yardstick and
    to TOL.  The argument below carries over with "flip" read as "fp32 rounding": the yardstick is what ONE fp32 evaluation of
    the stage costs against float64; a correct kernel adds its own accumulation order (the yardstick's size again) and 1-ulp
    v_exp_f32 / v_rcp_f32 in every SiLU.  The split-fp16 families get no allowance beyond that: their operand error is in the
    reference, not in the margin.  A statistic whose maximum is taken over a few hundred rows moves by about 2x between seeds.

    Why MARGIN x yardstick: the yardstick is the same statistic between the reference in fp32 and in float64 on the same inputs,
    i.e. the flips that ONE fp32-sized perturbation in front of every rounding causes.  A correct kernel perturbs the same
    roundings by its own fp32 accumulation in another order (the yardstick's size again) and by v_exp_f32 and v_rcp_f32 at
    1 ulp each in every SiLU: up to about three times the flip rate; and the maximum of a few thousand rare events moves by
    about 2x between seeds.  (The GELU fit is NOT among the device-only perturbations: its relative error is a hundred fp32
    epsilons, so the reference evaluates the fit itself, gamd_oracle_lp.gelu_fit.)  Measured: 0.0 - 2.1 x.
    The aggregate's MEDIAN row is held to the fp32 bar: that is what catches anything systematic."""
    bad = []
    if fp32_grade:
        return [k for k in GRADE_STATS if k in stats and not (stats[k] <= MARGIN * yard[k] and stats[k] < TOL)]
    if yard is None:
        for k in ("enc_max", "agg_med", "agg_max", "e2e"):
            if not stats[k] < TOL:
                bad.append(k)
    else:
        for k in FLIP_STATS:
            if not stats[k] <= MARGIN * yard[k]:
                bad.append(k)
        if not stats["agg_med"] < TOL:
            bad.append("agg_med")
    for k in ("node_max", "node_p99", "dec_max", "dec_p99"):
        if k == "dec_p99" and not dec_p99_held:
            continue
        if k in stats and not stats[k] < TOL:
            bad.append(k)
    return bad


# ---- the reference against itself (CPU) ------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def cpu_inputs(case_id: str):
    """fp32 positions, oracle edges, fp32 features and h_0 of a case: what every CPU run of the reference starts from."""
    c = BY_ID[case_id]
    sd32, sd64 = weights(case_id)
    pos, box, species, bonds = system(c.system)
    pos32 = torch.from_numpy(pos)
    edges = orc.neighbor_edges(pos32, box, c.cutoff, c.flavour)
    dst, src = edges[0], edges[1]
    bond = bonds if c.cfg.use_bond else None
    feat = features(sd32, pos32, src, dst, box, bond)
    h0 = lp.initial_h(sd32, pos.shape[0], node_input(species) if c.cfg.kind != "lj" else None)
    return dict(pos=pos32, box=box, species=species, bonds=bond, src=src, dst=dst, feat=feat, h0=h0)


@lru_cache(maxsize=None)
def reference_run(case_id: str):
    """The case's float64 reference chained from the fp32 features."""
    c = BY_ID[case_id]
    _, sd64 = weights(case_id)
    x = cpu_inputs(case_id)
    return lp.forward_stages(sd64, x["feat"].double(), x["h0"].double(), x["src"], x["dst"], c.variant)


@lru_cache(maxsize=None)
def yardstick_of(case_id: str) -> dict:
    """The reference in float32 against the reference in float64 on the same inputs (fp32-representable: the features, the
    reference's bf16 e, its h_{L-1} rounded to fp32), per stage."""
    return compare_with_reference(case_id, weights(case_id)[0], torch.float32, BY_ID[case_id].variant)


def in_degree(dst: torch.Tensor, n: int) -> torch.Tensor:
    return torch.bincount(dst.long(), minlength=n)


def chunk_start_rows(dst: torch.Tensor, n: int, chunk: int = 16) -> torch.Tensor:
    """bool [N]: non-empty rows whose first CSR slot sits on a chunk boundary (rows in atom order)."""
    deg = in_degree(dst, n)
    start = torch.cumsum(deg, 0) - deg
    return (deg > 0) & (start % chunk == 0)


def compare_with_reference(case_id: str, sd, dtype, variant, d_off_by_one: bool = False, stale_layer: Optional[int] = None) -> dict:
    """Statistics of the reference run with (`sd`, `dtype`, `variant`) against the case's float64 reference, every stage fed the
    float64 reference's inputs: the encoder the fp32 features, a conv layer the reference's e and (fp32-rounded) h_l, the node
    kernel the reference's aggregate, the decoder its h_L, the end-to-end chain the features and h_0.  This is the code path of
    tests/test_gpu_lp_stages.py with the run under test in the device's place: with the variant's own fp32 run it gives the
    yardstick, with a mutated float64 run it shows what the criteria catch.
    The fp32-grade variants get every statistic of GRADE_STATS; the two switches describe wrong kernels of theirs:
    d_off_by_one -- the hoisted layer 0 applies d_i c0 with d_i + 1 for rows that start on a chunk boundary;
    stale_layer  -- that layer's edge kernel reads the node tables of the layer before it."""
    c = BY_ID[case_id]
    _, sd64 = weights(case_id)
    x, ref = cpu_inputs(case_id), reference_run(case_id)
    L = c.cfg.conv_layer
    src, dst = x["src"], x["dst"]
    n = x["h0"].shape[0]
    e_in = ref["e"].float()                        # bf16-representable / what the device stores: exact in fp32
    h_in = ref["h"][L - 1].float()
    out = {}
    enc = enc_stats(lp.encode_edges(sd, x["feat"].to(dtype), variant), ref["e"])
    chain = lp.forward_stages(sd, x["feat"].to(dtype), x["h0"].to(dtype), src, dst, variant)
    if not c.fp32_grade:
        out["enc_bits"], out["enc_max"] = enc
        agg_ref = lp.conv_edge_agg(sd64, L - 1, e_in.double(), h_in.double(), src, dst, c.variant)
        agg = lp.conv_edge_agg(sd, L - 1, e_in.to(dtype), h_in.to(dtype), src, dst, variant)
        out["agg_med"], out["agg_max"], _ = row_stats(agg.numpy(), agg_ref.numpy())
        out["e2e"] = rel_err(chain["out"].numpy(), ref["out"].numpy())
        return out
    out["enc_max"] = enc[1]
    out["enc_bias"] = enc_bias(lp.encode_edges(sd, x["feat"].to(dtype), variant), ref["e"])
    d = in_degree(dst, n)
    d_dev = d + chunk_start_rows(dst, n).long() if d_off_by_one else d

    def layer(s, dt, l, h_l, var, device):
        """(aggregate or sum T3, h_{l+1}) of layer l from e_in and h_l; `device`: the side that may carry the switches."""
        h_l, e = h_l.to(dt), e_in.to(dt)
        if c.hoisted and l == 0 and (device or L == 1):
            t3 = lp.conv_edge_t3_sum(s, e, h_l, src, dst, var)
            return t3, lp.node_update_hoisted(s, t3, d_dev if device else d, h_l, var)
        stale = ref["h"][l - 1].float().to(dt) if device and stale_layer == l else None
        agg = lp.conv_edge_agg(s, l, e, h_l, src, dst, var, tables_from=stale)
        return agg, lp.node_update(s, l, agg, h_l, var)

    # the last conv layer's edge kernel (the one-layer hoisted case: the sums of T3 on both sides)
    agg_ref, _ = layer(sd64, torch.float64, L - 1, h_in, c.variant, False)
    agg, _ = layer(sd, dtype, L - 1, h_in, variant, True) if not (c.hoisted and L == 1) else \
        (lp.conv_edge_t3_sum(sd, e_in.to(dtype), h_in.to(dtype), src, dst, variant), None)
    out["agg_med"], out["agg_max"], _ = row_stats(agg.numpy(), agg_ref.numpy())
    # every earlier layer: the update h_{l+1} - h_l, formed in float64 on both sides
    out["upd_med"] = out["upd_max"] = 0.0
    for l in range(L - 1):
        h_l = ref["h"][l].float()
        upd_ref = layer(sd64, torch.float64, l, h_l, c.variant, False)[1] - h_l.double()
        upd = layer(sd, dtype, l, h_l, variant, True)[1].double() - h_l.double()
        med, mx, _ = row_stats(upd.numpy(), upd_ref.numpy())
        out["upd_med"], out["upd_max"] = max(out["upd_med"], med), max(out["upd_max"], mx)
    # node kernel of the last layer from the reference's (fp32-rounded) sums; decoder from its h_L
    a_in = agg_ref.float()
    if c.hoisted and L == 1:
        n_ref = lp.node_update_hoisted(sd64, a_in.double(), d, h_in.double(), c.variant)
        n_run = lp.node_update_hoisted(sd, a_in.to(dtype), d_dev, h_in.to(dtype), variant)
    else:
        n_ref = lp.node_update(sd64, L - 1, a_in.double(), h_in.double(), c.variant)
        n_run = lp.node_update(sd, L - 1, a_in.to(dtype), h_in.to(dtype), variant)
    out.update(stage_stats("node", n_run.numpy(), n_ref.numpy()))
    h_L = ref["h"][-1].float()
    out.update(stage_stats("dec", lp.decode(sd, h_L.to(dtype), variant).numpy(), lp.decode(sd64, h_L.double(), c.variant).numpy()))
    out["e2e"] = rel_err(chain["out"].numpy(), ref["out"].numpy())
    return out


def fp32_stage_noise(case_id: str) -> dict:
    """The node and decoder statistics of the reference in fp32 against itself in float64 on the reference's own (fp32-rounded)
    inputs: how much of the fp32 bar a case's weights use up before any kernel is involved."""
    c = BY_ID[case_id]
    sd32, sd64 = weights(case_id)
    ref = reference_run(case_id)
    L = c.cfg.conv_layer
    h, hp, ag = ref["h"][-1].float(), ref["h"][L - 1].float(), ref["agg"][-1].float()
    d32, d64 = lp.decode(sd32, h).numpy(), lp.decode(sd64, h.double()).numpy()
    n32, n64 = lp.node_update(sd32, L - 1, ag, hp).numpy(), lp.node_update(sd64, L - 1, ag.double(), hp.double()).numpy()
    return {"node_max": rel_err(n32, n64), "node_p99": per_atom_err(n32, n64)[1],
            "dec_max": rel_err(d32, d64), "dec_p99": per_atom_err(d32, d64)[1]}


def shared_row_conditioning(case_id: str, trials: int, amplitude: float) -> float:
    """LJ layer 0 (one conv layer): the largest median row error of the aggregate over `trials` fp32 runs of the reference
    whose shared h_0 row is perturbed by `amplitude` x N(0, 1) relative, against the float64 reference."""
    c = BY_ID[case_id]
    sd32, sd64 = weights(case_id)
    x, ref = cpu_inputs(case_id), reference_run(case_id)
    e = ref["e"].float()
    agg_ref = lp.conv_edge_agg(sd64, 0, e.double(), x["h0"].double(), x["src"], x["dst"], c.variant).numpy()
    g = torch.Generator().manual_seed(9)
    worst = 0.0
    for k in range(trials):
        h0 = x["h0"] * (1.0 + (amplitude if k else 0.0) * torch.randn(x["h0"].shape[1], generator=g))
        agg = lp.conv_edge_agg(sd32, 0, e, h0, x["src"], x["dst"], c.variant).numpy()
        worst = max(worst, row_stats(agg, agg_ref)[0])
    return worst


@lru_cache(maxsize=None)
def yardstick(variant: str) -> dict:
    """Per statistic, the maximum over this module's cases of the variant (a 7-atom case without a flip of its own is then not
    held to zero)."""
    ys = [yardstick_of(c.id) for c in CASES if c.variant == variant]
    return {k: max(y[k] for y in ys) for k in ys[0]}


def max_split_operand(case_id: str) -> float:
    """The largest magnitude of any operand the case's float64 reference run splits into fp16 halves."""
    c = BY_ID[case_id]
    _, sd64 = weights(case_id)
    x = cpu_inputs(case_id)
    lp.operand_log = []
    try:
        lp.forward_stages(sd64, x["feat"].double(), x["h0"].double(), x["src"], x["dst"], c.variant)
        return max(lp.operand_log)
    finally:
        lp.operand_log = None
