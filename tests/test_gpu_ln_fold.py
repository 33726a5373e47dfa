"""Folded edge LayerNorm of the fp32 128-wide kernels (gamd_ln_fold_host.h): the encoder keeps only the row norms of
its last Linear (through R of B = Q R) and stores rstd x2 and rstd, every conv layer's first GEMM runs over
A_l = W1_l diag(gamma) B with one extra K step.  Equal to the general form up to fp32 rounding; the general form stays
reachable through GAMD_KSEL_NO_LN_FOLD, which must change nothing where the fold does not apply.

Bars: 1e-5 against the reference goldens and the float64 oracle (the suite's), 3e-6 folded against general
(test_gpu_layer0_hoist.py's bar for a linear map moved past a sum).  Achieved values: profiles/ln_fold_numerics.txt."""
import numpy as np
import pytest
import torch

import gamd_oracle as orc
from helpers import load_golden, rel_err
from gamd_amd.engine import KSEL_FORCE_GENERIC_WIDTH, KSEL_NO_LAYER0_HOIST, KSEL_NO_LN_FOLD
from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
from gamd_amd import workloads

pytestmark = pytest.mark.gpu
TOL = 1e-5          # against the reference / the float64 oracle
FOLD_TOL = 3e-6     # folded against the general form


def _engine(*a, **kw):
    from gamd_amd.engine import GamdForce
    return GamdForce(*a, **kw)


def _pair(sd, n, box, rc, kernel_select=0, **kw):
    return (_engine(sd, n, box, rc, kernel_select=kernel_select, **kw),
            _engine(sd, n, box, rc, kernel_select=kernel_select | KSEL_NO_LN_FOLD, **kw))


def _report(tag, a, b):
    e = rel_err(a, b)
    print(f"[ln_fold] {tag}: max|df|/max|f| = {e:.3e}")
    return e


def _golden(name):
    g, cfg, sd = load_golden(name)
    box, rc, n = float(g["box"]), float(g["cutoff"]), g["pos"].shape[0]
    kw = dict(scaler=(g["scaler_mean"], g["scaler_var"]))
    if "bond" in g:
        kw["bond"] = g["bond"]
    species = (g["node_feat"].reshape(-1) != 0) if "node_feat" in g else None
    p = torch.from_numpy(np.mod(g["pos"], box).astype(np.float32))
    return g, sd, n, box, rc, kw, species, p


# (golden, kernel_select): both LJ variants -- layer-0 form on and off -- and water with the bond feature (K = 45)
GOLDEN_CASES = [("lj258_seed0", 0), ("lj258_seed0", KSEL_NO_LAYER0_HOIST), ("tip3p774_seed3", 0)]


@pytest.mark.parametrize("small_tile_limit", [0, -1])              # latency kernels and throughput kernels
@pytest.mark.parametrize("name,ksel", GOLDEN_CASES)
def test_goldens_folded_against_general_form_and_reference(name, ksel, small_tile_limit):
    g, sd, n, box, rc, kw, species, p = _golden(name)
    fold, plain = _pair(sd, n, box, rc, kernel_select=ksel, small_tile_limit=small_tile_limit, **kw)
    out, gen = fold.forward(p, species=species).cpu().numpy(), plain.forward(p, species=species).cpu().numpy()
    tag = f"{name} ksel={ksel} stl={small_tile_limit}"
    e_gen = _report(f"{tag} vs general", out, gen)
    e_ref = _report(f"{tag} vs reference", out, g["out_norm"])
    print(f"[ln_fold] {tag} general form vs reference: {rel_err(gen, g['out_norm']):.3e}")
    assert fold.counts()[0] == g["edge_idx"].shape[1]
    assert e_gen < FOLD_TOL and e_ref < TOL
    fold.close(); plain.close()


@pytest.mark.parametrize("name,ksel", GOLDEN_CASES)
def test_latency_and_throughput_kernels_are_bit_identical(name, ksel):
    g, sd, n, box, rc, kw, species, p = _golden(name)
    a = _engine(sd, n, box, rc, kernel_select=ksel, **kw)
    b = _engine(sd, n, box, rc, kernel_select=ksel, small_tile_limit=-1, **kw)
    assert np.array_equal(a.forward(p, species=species).cpu().numpy(), b.forward(p, species=species).cpu().numpy())
    a.close(); b.close()


@pytest.mark.parametrize("layers", [1, 4])
def test_one_and_four_layers_against_oracle(layers):
    g = load_golden("lj258_seed0")[0]
    box, rc = float(g["box"]), float(g["cutoff"])
    pos = np.mod(g["pos"], box).astype(np.float32)
    cfg = ModelConfig(kind="lj", conv_layer=layers)
    sd = make_state_dict(cfg, 3, 5.3, 1.6)
    fold, plain = _pair(sd, pos.shape[0], box, rc, cfg=cfg)
    p = torch.from_numpy(pos)
    out, gen = fold.forward(p).cpu().numpy(), plain.forward(p).cpu().numpy()
    e_gen = _report(f"L={layers} vs general", out, gen)
    ref = orc.forward(sd, p, torch.from_numpy(fold.debug_edges()).long(), box).numpy()
    e_ref = _report(f"L={layers} vs oracle", out, ref)
    assert e_gen < FOLD_TOL and e_ref < TOL
    fold.close(); plain.close()


def test_a_batch_of_two_boxes():
    """Box padding slots carry finite rstd x2 rows of their own and stay out of the sums: a batch is bit-identical to its
    boxes one by one."""
    g = load_golden("lj258_seed0")[0]
    n, box, rc = 258, float(g["box"]), float(g["cutoff"])
    base = np.mod(g["pos"], box)[:n]
    rng = np.random.default_rng(4)
    pos = [base, base + rng.normal(0, 0.3, base.shape)]
    sd = make_state_dict(ModelConfig(kind="lj"), 0, 5.3, 1.6)
    fold, plain = _pair(sd, n, box, rc, n_boxes=2, scaler=SHIPPED_SCALERS["lj"])
    x = torch.from_numpy(np.concatenate(pos)).float()
    out, gen = fold.forward(x).cpu().numpy(), plain.forward(x).cpu().numpy()
    assert int((fold.debug_csr()[1] == 2 * n).sum()) > 0               # padding slots present
    assert _report("batch of 2 vs general", out, gen) < FOLD_TOL
    single = _engine(sd, n, box, rc, scaler=SHIPPED_SCALERS["lj"])
    for b in range(2):
        assert np.array_equal(out[b * n:(b + 1) * n], single.forward(torch.from_numpy(pos[b]).float()).cpu().numpy()), b
    fold.close(); plain.close(); single.close()


def test_isolated_atom_ragged_last_tile_and_caller_edges():
    """A sparse box: atoms without edges, an edge count that is no multiple of 32 (the last tile's padding slots), through the
    built-in search and through the caller-edge entry point."""
    rng = np.random.default_rng(7)
    n, box, rc = 200, 30.0, 3.0
    pos = rng.uniform(0, box, (n, 3)).astype(np.float32)
    sd = make_state_dict(ModelConfig(kind="lj"), 2, 3.0, 1.0)
    fold, plain = _pair(sd, n, box, rc, nbr_flavour="torch")
    p = torch.from_numpy(pos)
    out, gen = fold.forward(p).cpu().numpy(), plain.forward(p).cpu().numpy()
    edges = fold.debug_edges()
    assert (np.bincount(edges[0], minlength=n) == 0).any() and fold.counts()[0] % 32 != 0
    assert _report("sparse box vs general", out, gen) < FOLD_TOL
    ref = orc.forward(sd, p, torch.from_numpy(edges).long(), box).numpy()
    assert _report("sparse box vs oracle", out, ref) < TOL
    ei = torch.from_numpy(edges[:, rng.permutation(edges.shape[1])]).long()
    oe, ge = fold.forward_edges(p, ei).cpu().numpy(), plain.forward_edges(p, ei).cpu().numpy()
    assert _report("caller edges vs general", oe, ge) < FOLD_TOL
    assert _report("caller edges vs oracle", oe, ref) < TOL
    fold.close(); plain.close()


def test_skin_reuse_across_a_rebuild():
    """Along a random walk that crosses a candidate-list rebuild, the folded form follows the general one step by step."""
    g, sd, n, box, rc, kw, species, p = _golden("lj258_seed0")
    fold, plain = _pair(sd, n, box, rc, neighbor_skin=rc / 6.0, **kw)
    exact = _engine(sd, n, box, rc, **kw)
    rng = np.random.default_rng(2)
    x = p.numpy().copy()
    worst = 0.0
    for step in range(10):
        xt = torch.from_numpy(np.mod(x, box).astype(np.float32))
        out, gen = fold.forward(xt).cpu().numpy(), plain.forward(xt).cpu().numpy()
        exact.forward(xt)
        assert fold.counts()[0] == plain.counts()[0] == exact.counts()[0], step     # the edges of the exact search
        worst = max(worst, rel_err(out, gen))
        x += rng.normal(0, 0.01 * rc, x.shape)       # a rebuild is due once an atom has moved rc / 12: every few steps
    print(f"[ln_fold] skin walk vs general: max|df|/max|f| = {worst:.3e}")
    assert fold.skin_stats()[0] >= 2 and fold.skin_stats()[0] < 10                # rebuilt on the way, reused in between
    assert worst < FOLD_TOL
    fold.close(); plain.close(); exact.close()


def test_a_20_step_md_run():
    g, sd, n, box, rc, kw, species, p = _golden("lj258_seed0")
    vel = workloads.maxwell_boltzmann(n, mass_amu=39.9, seed=9)
    res = []
    for eng in _pair(sd, n, box, rc, neighbor_skin=rc / 6.0, **kw):
        x, v = p.clone().cuda(), torch.from_numpy(vel).float().cuda()
        f = eng.forward(x, denormalize=True).clone()
        eng.md_run(x, v, f, 20, seed=3)
        torch.cuda.synchronize()
        res.append((x.cpu().numpy(), v.cpu().numpy(), f.cpu().numpy()))
        eng.close()
    errs = [_report(f"md_run 20 steps {nm}", a, b) for nm, a, b in zip("xvf", res[0], res[1])]
    assert max(errs) < FOLD_TOL


NOT_FOLDED = [("lj258_seed0", dict(edge_dtype="bf16")), ("lj258_seed0", dict(edge_dtype="f16x3")),
              ("lj258_seed0", dict(kernel_select=KSEL_FORCE_GENERIC_WIDTH)), ("lj258_w256_seed9", {}), ("lj258_d192_seed15", {}),
              ("lj258_selfloop_inplace_seed0", dict(self_loop_mode="append_zero_feature_loops")), ("lj258_seed0", dict(keep_stages=True)),
              ("tip3p774_seed3", dict(edge_dtype="bf16"))]


@pytest.mark.parametrize("name,extra", NOT_FOLDED, ids=[f"{n}-{'-'.join(map(str, e.values())) or 'as-is'}" for n, e in NOT_FOLDED])
def test_opt_out_bit_changes_nothing_where_the_fold_does_not_apply(name, extra):
    g, sd, n, box, rc, kw, species, p = _golden(name)
    cfg = load_golden(name)[1]
    extra = dict(extra)
    ksel = extra.pop("kernel_select", 0)
    a, b = _pair(sd, n, box, rc, kernel_select=ksel, cfg=cfg, **kw, **extra)
    assert np.array_equal(a.forward(p, species=species).cpu().numpy(), b.forward(p, species=species).cpu().numpy())
    a.close(); b.close()


def test_opt_out_bit_changes_nothing_with_update_edge():
    g, cfg, sd = load_golden("dynbox384_update_seed14")
    n, species = g["pos"].shape[0], g["node_feat"].reshape(-1) != 0
    a, b = _pair(sd, n, g["box"], float(g["cutoff"]), nbr_flavour="torch")
    p = torch.from_numpy(g["pos"])
    assert np.array_equal(a.forward(p, box=g["box"], species=species).cpu().numpy(), b.forward(p, box=g["box"], species=species).cpu().numpy())
    a.close(); b.close()


def test_the_e_getter_refuses_on_a_folded_handle_and_works_with_keep_stages():
    g, sd, n, box, rc, kw, species, p = _golden("lj258_seed0")
    fold = _engine(sd, n, box, rc, **kw)
    fold.forward(p)
    with pytest.raises(Exception, match="keep_stages"):
        fold.debug_e()
    fold.close()
    es = []
    for extra in (dict(keep_stages=True), dict(kernel_select=KSEL_NO_LN_FOLD)):
        eng = _engine(sd, n, box, rc, **kw, **extra)
        eng.forward(p)
        e = eng.debug_e()
        assert e.shape == (eng.counts()[0], 128) and np.isfinite(e).all()
        es.append(e)
        eng.close()
    assert np.array_equal(es[0], es[1])
