"""Layer-0 form of the LJ models (conv_edge.hip, node.hip post(0)): every atom enters layer 0 with the same row, so the last
edge Linear of layer 0 is applied per atom (M0 = W_pe diag(hn0) W4, c0 = W_pe (hn0 * b4)) and the edge kernel runs three
GEMMs per edge instead of four.  Equal to the general form up to fp32 rounding (a linear map moved past a sum); the general
form stays reachable through GAMD_KSEL_NO_LAYER0_HOIST, which must change nothing where the form does not apply."""
import numpy as np
import pytest
import torch

import gamd_oracle as orc
from helpers import load_golden, rel_err, per_atom_err
from gamd_amd.engine import KSEL_NO_LAYER0_HOIST
from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
from gamd_amd import workloads

pytestmark = pytest.mark.gpu
TOL = 1e-5          # against the reference / the float64 oracle (the suite's bar)
HOIST_TOL = 3e-6    # hoisted against the general form


def _engine(*a, **kw):
    from gamd_amd.engine import GamdForce
    return GamdForce(*a, **kw)


def _pair(sd, n, box, rc, **kw):
    return _engine(sd, n, box, rc, **kw), _engine(sd, n, box, rc, kernel_select=KSEL_NO_LAYER0_HOIST, **kw)


def _report(tag, a, b):
    e = rel_err(a, b)
    print(f"[layer0] {tag}: max|df|/max|f| = {e:.3e}")
    return e


LJ_GOLDENS = ["lj258_seed0", "lj258_pert_seed1", "lj258_bn_seed11", "lj258_selfloop_inplace_seed0", "lj64_h32"]


@pytest.mark.parametrize("small_tile_limit", [0, -1])              # latency kernel (default at 258 atoms) and throughput kernel
@pytest.mark.parametrize("name", LJ_GOLDENS)
def test_lj_goldens_hoisted_against_general_form_and_reference(name, small_tile_limit):
    g, cfg, sd = load_golden(name)
    box, rc, n = float(g["box"]), float(g["cutoff"]), g["pos"].shape[0]
    kw = dict(scaler=(g["scaler_mean"], g["scaler_var"]), small_tile_limit=small_tile_limit)
    if "selfloop" in name:
        kw["self_loop_mode"] = "append_zero_feature_loops"
    hoist, plain = _pair(sd, n, box, rc, **kw)
    p = torch.from_numpy(np.mod(g["pos"], box).astype(np.float32))
    out, ref = hoist.forward(p).cpu().numpy(), plain.forward(p).cpu().numpy()
    assert _report(f"{name} stl={small_tile_limit} vs general", out, ref) < HOIST_TOL
    e_ref = _report(f"{name} stl={small_tile_limit} vs reference", out, g["out_norm"])
    print(f"[layer0] {name} stl={small_tile_limit} general form vs reference: {rel_err(ref, g['out_norm']):.3e}")
    assert e_ref < TOL
    hoist.close(); plain.close()


def test_latency_and_throughput_kernels_are_bit_identical():
    g, cfg, sd = load_golden("lj258_seed0")
    box, rc, n = float(g["box"]), float(g["cutoff"]), g["pos"].shape[0]
    a = _engine(sd, n, box, rc)
    b = _engine(sd, n, box, rc, small_tile_limit=-1)
    p = torch.from_numpy(np.mod(g["pos"], box).astype(np.float32))
    assert np.array_equal(a.forward(p).cpu().numpy(), b.forward(p).cpu().numpy())
    a.close(); b.close()


@pytest.mark.parametrize("norm", ["layer", "batch"])
@pytest.mark.parametrize("layers", [1, 4])
def test_one_and_four_layers_against_oracle(layers, norm):
    """conv_layer=1 finishes layer 0 in the decoder launch (node.hip mode 2)."""
    g = load_golden("lj258_seed0")[0]
    box, rc = float(g["box"]), float(g["cutoff"])
    pos = np.mod(g["pos"], box).astype(np.float32)
    cfg = ModelConfig(kind="lj", conv_layer=layers, use_layer_norm=norm == "layer")
    sd = make_state_dict(cfg, 3, 5.3, 1.6)
    hoist, plain = _pair(sd, pos.shape[0], box, rc, cfg=cfg)
    p = torch.from_numpy(pos)
    out, gen = hoist.forward(p).cpu().numpy(), plain.forward(p).cpu().numpy()
    assert _report(f"L={layers} {norm} vs general", out, gen) < HOIST_TOL
    ref = orc.forward(sd, p, torch.from_numpy(hoist.debug_edges()).long(), box).numpy()
    assert _report(f"L={layers} {norm} vs oracle", out, ref) < TOL
    hoist.close(); plain.close()


@pytest.mark.parametrize("nb", [2, 5])
def test_batches_with_box_padding(nb):
    """The box padding slots (source n, <= 15 per box) must stay out of the sums and out of d_i: a batch stays
    bit-identical to its boxes one by one, and close to the general form."""
    g = load_golden("lj258_seed0")[0]
    n, box, rc = 258, float(g["box"]), float(g["cutoff"])
    base = np.mod(g["pos"], box)[:n]
    rng = np.random.default_rng(4)
    pos = [base + (rng.normal(0, 0.3, base.shape) if b else 0.0) for b in range(nb)]
    sd = make_state_dict(ModelConfig(kind="lj"), 0, 5.3, 1.6)
    hoist, plain = _pair(sd, n, box, rc, n_boxes=nb, scaler=SHIPPED_SCALERS["lj"])
    x = torch.from_numpy(np.concatenate(pos)).float()
    out, gen = hoist.forward(x).cpu().numpy(), plain.forward(x).cpu().numpy()
    row_ptr, col = hoist.debug_csr()
    assert int((col == nb * n).sum()) > 0                              # padding slots present
    assert _report(f"batch nb={nb} vs general", out, gen) < HOIST_TOL
    single = _engine(sd, n, box, rc, scaler=SHIPPED_SCALERS["lj"])
    for b in range(nb):
        assert np.array_equal(out[b * n:(b + 1) * n], single.forward(torch.from_numpy(pos[b]).float()).cpu().numpy()), b
    hoist.close(); plain.close(); single.close()


def test_isolated_atoms_and_caller_edges():
    """Atoms without edges get exactly phi(P) + h, through the built-in search and through the caller-edge entry point."""
    rng = np.random.default_rng(7)
    n, box, rc = 200, 30.0, 3.0
    pos = rng.uniform(0, box, (n, 3)).astype(np.float32)
    sd = make_state_dict(ModelConfig(kind="lj"), 2, 3.0, 1.0)
    hoist, plain = _pair(sd, n, box, rc, nbr_flavour="torch")
    p = torch.from_numpy(pos)
    out, gen = hoist.forward(p).cpu().numpy(), plain.forward(p).cpu().numpy()
    edges = hoist.debug_edges()
    assert (np.bincount(edges[0], minlength=n) == 0).any()
    assert _report("isolated atoms vs general", out, gen) < HOIST_TOL
    ref = orc.forward(sd, p, torch.from_numpy(edges).long(), box).numpy()
    assert _report("isolated atoms vs oracle", out, ref) < TOL
    ei = torch.from_numpy(edges[:, rng.permutation(edges.shape[1])]).long()
    oe, ge = hoist.forward_edges(p, ei).cpu().numpy(), plain.forward_edges(p, ei).cpu().numpy()
    assert _report("caller edges vs general", oe, ge) < HOIST_TOL
    assert rel_err(oe, ref) < TOL
    hoist.close(); plain.close()


def test_c2_full_size():
    """bench.py's default workload (10 000 atoms, cutoff 3 sigma): hoisted against the general form and the oracle."""
    pos, box = workloads.lj_box(10000)
    sd = make_state_dict(ModelConfig(kind="lj"), 0, 7.0, 2.2)
    hoist, plain = _pair(sd, 10000, box, 3.0 * workloads.LJ_SIGMA, scaler=SHIPPED_SCALERS["lj"])
    p = torch.from_numpy(pos).float()
    out, gen = hoist.forward(p).cpu().numpy(), plain.forward(p).cpu().numpy()
    assert _report("C2 vs general", out, gen) < HOIST_TOL
    ref = orc.forward(sd, p, torch.from_numpy(hoist.debug_edges()).long(), box).numpy()
    e_new, e_old = _report("C2 hoisted vs oracle", out, ref), _report("C2 general vs oracle", gen, ref)
    print(f"[layer0] C2 per-atom p99 vs oracle: hoisted {per_atom_err(out, ref)[1]:.3e}, general {per_atom_err(gen, ref)[1]:.3e}")
    assert e_new < TOL and e_old < TOL
    hoist.close(); plain.close()


@pytest.mark.parametrize("kind,edge_dtype", [("water", "f32"), ("lj", "bf16"), ("lj", "f16x3")])
def test_opt_out_bit_changes_nothing_where_the_form_does_not_apply(kind, edge_dtype):
    g, cfg, sd = load_golden("tip3p774_seed3" if kind == "water" else "lj258_seed0")
    box, rc, n = float(g["box"]), float(g["cutoff"]), g["pos"].shape[0]
    bond = g["bond"] if "bond" in g else None
    a, b = _pair(sd, n, box, rc, bond=bond, edge_dtype=edge_dtype)
    p = torch.from_numpy(np.mod(g["pos"], box).astype(np.float32))
    species = (g["node_feat"].reshape(-1) != 0) if "node_feat" in g else None
    assert np.array_equal(a.forward(p, species=species).cpu().numpy(), b.forward(p, species=species).cpu().numpy())
    a.close(); b.close()
