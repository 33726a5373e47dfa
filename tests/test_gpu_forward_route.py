"""The launch structure of one force evaluation (gamd_amd/csrc/forward.hip) per kernel family, with and without a Verlet skin:
the stage labels gamd_profile records come out in the order the stages are written in, the profiled evaluation returns the
forces of forward() bit for bit, and an enqueued MD run behind it still ends clean.  Which kernel each stage launches is held on
the CPU (tests/test_route_host.py); that every family computes the right forces, by tests/test_gpu_lp_stages.py."""
import numpy as np
import pytest
import torch

import lp_cases as lc
from gamd_amd.weights import make_state_dict
from test_weights_host import BY_ID as WEIGHT_CASES

pytestmark = pytest.mark.gpu

# (weights, system): 128-wide fp32 water and LJ (hoisted layer 0), update_edge_emb on the generic-width kernels, split-fp16 at
# 256 / 256, and one partly filled tile with the throughput kernels forced
CASES = [("ctl-f32", "water90"), ("f32-lj-3", "lj258"), ("update-edge", "water90"), ("f16x3-wide-256", "water90"), ("f32-tiny-tp", "tiny7")]
SYSTEM_CUTOFF = {"water90": 4.2, "lj258": 7.5, "tiny7": 3.0}


def _engine(weights, system, skin):
    from gamd_amd.engine import GamdForce
    w = WEIGHT_CASES[weights]
    c = lc.BY_ID.get(weights)
    pos, box, species, bonds = lc.system(system)
    eng = GamdForce(make_state_dict(w.cfg, w.seed, *w.length), pos.shape[0], box, SYSTEM_CUTOFF[system], bond=bonds if w.cfg.use_bond else None,
                    nbr_flavour=c.flavour if c else "jaxmd", cfg=w.cfg, edge_dtype=w.edge_dtype, kernel_select=w.kernel_select,
                    small_tile_limit=c.small_tile_limit if c else 0, neighbor_skin=skin, scaler=(0.25, 2.0))
    return eng, w.cfg, torch.from_numpy(pos).cuda(), species


def _expected_labels(cfg):
    labels = ["neighbor_build", "edge_encode", "node_first"]
    for l in range(cfg.conv_layer):
        last = l == cfg.conv_layer - 1
        labels.append("conv_edge")
        if cfg.update_edge and not last:
            labels.append("edge_update")
        labels.append("node_last_decode" if last else "node_mid")
    return labels


@pytest.mark.parametrize("skin", [0.0, 0.6], ids=["exact", "skin"])
@pytest.mark.parametrize("weights,system", CASES, ids=[c[0] for c in CASES])
def test_stage_order_forces_and_a_following_run(weights, system, skin):
    eng, cfg, pos, species = _engine(weights, system, skin)
    try:
        forces = eng.forward(pos, species=species)
        stages = eng.profile(pos, species=species)
        assert [name for name, _ in stages] == _expected_labels(cfg)
        assert all(ms >= 0.0 for _, ms in stages)
        profiled = eng._out.clone()                       # gamd_profile's out_norm_dev
        assert np.isfinite(profiled.cpu().numpy()).all() and profiled.abs().max() > 0
        assert torch.equal(profiled, forces)
        assert torch.equal(eng.forward(pos, species=species), forces)
        x, v, f = pos.clone(), torch.zeros_like(pos), eng.forward(pos, species=species, denormalize=True)
        eng.md_run(x, v, f, 4, species=species, sync=False)
        assert eng.sync_status() == 0
        assert np.isfinite(f.cpu().numpy()).all() and not torch.equal(x, pos)
    finally:
        eng.close()
