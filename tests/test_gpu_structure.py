"""The structure sampler on the device: the all-pairs g(r) histogram out to half the box and the partial S(k) sums taken
inside enqueued md_run / md_run_nhc calls, against a sampler-off run of the same trajectory cut into chunks and looked at
from the host after each chunk.

Conventions of the host references (systems and integrators: the _Case of tests/test_gpu_report.py)
* g(r): a float64 min-image histogram of all i != j pairs of the chunk's final positions, the box edges as the fp32 values the
  library holds.  The device takes the distance in fp32, so a pair whose x = r * bins / r_max lies within 1e-5 x of an integer
  k may fall on either side of bin edge k: |cum_dev[k] - cum_ref[k]| is bounded by the number of such pairs, and these pairs
  may be at most 1 % of all pairs or the case is ill-posed (the reporter test's convention, restated here for boxes with three
  different edges).
* S(k): rho_c(n) = sum_i exp(-2 pi i n.s_i) in float64 over the same fp32 positions, s = x / L, the phase reduced to
  [-1/2, 1/2] before the cosine (an exact subtraction).  |dev - host| <= 1e-12 * frames * N_a * N_b: the worst-case growth of a
  double sum over N unit terms is N eps = 1.7e-13 at N = 1500, relative to the N_a N_b a product can reach, so the bound leaves
  three orders of margin.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gamd_amd import workloads as wl
from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
from test_gpu_report import _Case, _class_of, _f32, _state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHK = os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")
CHUNKS = 6


def _edges(box):
    """the fp32 box edges the library holds, widened: [3] float64"""
    return np.broadcast_to(np.asarray(box, dtype=np.float32).astype(np.float64).reshape(-1), (3,)).copy()


# ---- host references -------------------------------------------------------------------------------------------------
def _pairs_host(x, box, r_max):
    """float64 min-image distances of all i != j pairs of ONE box with r < r_max: (i, j, r)."""
    xd, L = x.astype(np.float64), _edges(box)
    d = xd[:, None, :] - xd[None, :, :]
    d -= L * np.round(d / L)
    r = np.sqrt((d * d).sum(-1))
    np.fill_diagonal(r, np.inf)
    i, j = np.nonzero(r < r_max)
    return i, j, r[i, j]


class _RefHist:
    """cumulative reference histogram and the pairs fp32 may place on either side of each bin edge, summed over frames"""

    def __init__(self, n_boxes, n_pairs, bins, r_max):
        self.bins, self.r_max = bins, _f32(r_max)
        self.cum = np.zeros((n_boxes, n_pairs, bins + 1), dtype=np.int64)        # cum[k] = pairs with x < k
        self.near = np.zeros((n_boxes, n_pairs, bins + 1), dtype=np.int64)
        self.total = 0

    def add(self, b, x_box, box, species, exclude_same_molecule=False):
        i, j, r = _pairs_host(x_box, box, self.r_max * (1.0 + 2e-5))
        if exclude_same_molecule:
            keep = (i // 3) != (j // 3)
            i, j, r = i[keep], j[keep], r[keep]
        xs = r * self.bins / self.r_max
        cls = _class_of(species, i, j)
        k = np.rint(xs)
        near = np.abs(xs - k) <= 1e-5 * xs
        for c in range(self.cum.shape[1]):
            m = cls == c
            self.cum[b, c] += np.searchsorted(np.sort(xs[m]), np.arange(self.bins + 1), side="left")
            self.near[b, c] += np.bincount(k[m & near].astype(np.int64), minlength=self.bins + 2)[:self.bins + 1]
        self.total += int((xs < self.bins).sum())

    def check(self, counts, who="structure sampler"):
        """counts uint64 [B, P, bins] from the device"""
        dev = np.concatenate([np.zeros(counts.shape[:2] + (1,), np.int64), np.cumsum(counts.astype(np.int64), axis=2)], axis=2)
        excused = int(self.near.sum())
        print(f"g(r) {who}: {int(counts.sum())} device pairs, {self.total} reference pairs, {excused} within 1e-5 of a bin edge, "
              f"max |cum_dev - cum_ref| {int(np.abs(dev - self.cum).max())}")
        assert excused <= 0.01 * self.total, "ill-posed: more than 1 % of the pairs sit on a bin edge"
        assert (np.abs(dev - self.cum) <= self.near).all()


class _RefSk:
    """float64 sums of Re(rho_a conj(rho_b)) over frames, [B, P, K]"""

    def __init__(self, n_boxes, n_pairs, n2max):
        from gamd_amd.engine import structure_kvectors
        self.kv = structure_kvectors(n2max)
        self.sum = np.zeros((n_boxes, n_pairs, self.kv.shape[0]), dtype=np.float64)
        self.frames = 0
        self.n_cls = None

    def add(self, b, x_box, box, species):
        s = x_box.astype(np.float64) / _edges(box)[None, :]
        ph = self.kv.astype(np.float64) @ s.T                                  # [K, N]
        ph -= np.rint(ph)
        e = np.cos(2.0 * np.pi * ph) - 1j * np.sin(2.0 * np.pi * ph)
        if self.sum.shape[1] == 1:
            rho = e.sum(axis=1)
            self.sum[b, 0] += (rho * rho.conj()).real
            self.n_cls = (x_box.shape[0],)
        else:
            o = species != 0
            ro, rh = e[:, o].sum(axis=1), e[:, ~o].sum(axis=1)
            self.sum[b, 0] += (ro * ro.conj()).real
            self.sum[b, 1] += (ro * rh.conj()).real
            self.sum[b, 2] += (rh * rh.conj()).real
            self.n_cls = (int(o.sum()), int((~o).sum()))
        if b == 0:
            self.frames += 1

    def check(self, sk_sum):
        n = self.n_cls
        nn = np.array([n[0] * n[0]] if len(n) == 1 else [n[0] * n[0], n[0] * n[1], n[1] * n[1]], dtype=np.float64)
        bound = 1e-12 * self.frames * nn
        err = np.abs(sk_sum - self.sum).max(axis=(0, 2))
        print(f"S(k): {self.kv.shape[0]} k-vectors, {self.frames} frames, max |dev - host| per pair class {err}, "
              f"bound {bound}, ratio {np.max(err / bound):.3e}; largest sum {np.abs(self.sum).max():.6e}")
        assert sk_sum.shape == self.sum.shape and np.isfinite(sk_sum).all()
        assert (err <= bound).all()
        assert np.abs(self.sum).max() > 0


def _reference_chunks(case, bins, r_max, n2max, exclude=False, steps=None):
    """sampler-off run cut at `steps` (default: CHUNKS calls of K steps): final state, reference histogram, reference sums,
    the positions at every cut"""
    steps = [case.K * (c + 1) for c in range(CHUNKS)] if steps is None else steps
    eng, x, v, f = case.make()
    rh = _RefHist(case.nb, case.n_pairs, bins, r_max) if bins else None
    rs = _RefSk(case.nb, case.n_pairs, n2max) if n2max else None
    chain, done, frames = None, 0, []
    sp = case.species
    for g in steps:
        chain = case.run(eng, x, v, f, g - done, first_step=done, chain=chain)
        done = g
        xs, _, _ = _state(x, v, f)
        frames.append(xs)
        for b in range(case.nb):
            xb = xs[b * case.n:(b + 1) * case.n]
            if rh:
                rh.add(b, xb, case.box, sp, exclude)
            if rs:
                rs.add(b, xb, case.box, sp)
    out = _state(x, v, f)
    eng.close()
    return out, rh, rs, frames


def _sampled_run(case, bins, r_max, n2max, exclude=False, n_steps=None):
    eng, x, v, f = case.make()
    eng.structure_configure(case.K, rdf_bins=bins, rdf_rmax=r_max, exclude_same_molecule=exclude, sk_n2max=n2max)
    case.run(eng, x, v, f, CHUNKS * case.K if n_steps is None else n_steps)
    st = eng.structure_read()
    out = _state(x, v, f)
    eng.close()
    return out, st


def _check_against_chunks(case, bins, r_max, n2max, exclude=False):
    from gamd_amd.engine import structure_kvectors
    (xr, vr, fr), rh, rs, _ = _reference_chunks(case, bins, r_max, n2max, exclude)
    (x, v, f), st = _sampled_run(case, bins, r_max, n2max, exclude)
    # 1. the sampler does not perturb the run
    assert np.array_equal(x, xr) and np.array_equal(v, vr) and np.array_equal(f, fr)
    assert st.frames == CHUNKS
    # 2. the histogram
    assert st.rdf_counts.shape == (case.nb, case.n_pairs, bins)
    if bins:
        assert int(st.rdf_counts.sum()) > 0 and not (st.rdf_counts % np.uint64(2)).any()      # every pair adds 2
        rh.check(st.rdf_counts)
    # 3. the structure factors
    assert np.array_equal(st.kvectors, structure_kvectors(n2max))
    assert st.sk_sum.shape == (case.nb, case.n_pairs, st.kvectors.shape[0])
    if n2max:
        rs.check(st.sk_sum)
    return st, rh, rs


def _half(case):
    return float(np.float32(0.5) * np.asarray(case.box, dtype=np.float32).min())


# ---- 1: one full tile and a two-atom tail ----------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", ["baoab", "nhc"])
def test_lj258_out_to_half_the_box_with_structure_factors(integrator):
    """258 atoms = one full 256-atom tile plus a 2-atom tail (three tile pairs, two of them diagonal), r_max = L / 2."""
    case = _Case("lj", integrator)
    assert abs(_half(case) - 13.635) < 1e-5
    st, _, _ = _check_against_chunks(case, 128, _half(case), 16)
    assert st.kvectors.shape == (128, 3)
    # far more than the cutoff sphere holds: the reporter's range ends at 7.5 A
    r_mid, g = st.rdf(0, case.n)
    assert g.shape == (1, 128) and g[0][r_mid > 7.5].min() > 0 and abs(g[0][r_mid > 10.0].mean() - 1.0) < 0.1


# ---- 2: less than one tile, three classes, rigid molecules -----------------------------------------------------------
def test_water_three_classes_and_exclude_same_molecule_removes_exactly_the_intramolecular_pairs():
    """192 atoms.  r_max = 6.0 with 97 bins on purpose: the lattice start puts L / 4 on a bin edge of any even bin count at
    r_max = L / 2 (2.9 % of the pairs with 128 bins); with 6.0 / 97 it is 18 of 15 706."""
    case = _Case("water")
    assert 6.0 <= _half(case)
    st, _, _ = _check_against_chunks(case, 97, 6.0, 9)
    st_x, _, _ = _check_against_chunks(case, 97, 6.0, 9, exclude=True)
    diff = st.rdf_counts.astype(np.int64) - st_x.rdf_counts.astype(np.int64)
    assert (diff >= 0).all()
    assert [int(d) for d in diff[0].sum(axis=1)] == [0, 4 * case.n_mol * CHUNKS, 2 * case.n_mol * CHUNKS]
    assert np.array_equal(st.sk_sum, st_x.sk_sum)                           # the exclusion is the histogram's alone
    r_mid, g = st_x.rdf(0, (case.n_mol, 2 * case.n_mol))
    assert g.shape == (3, 97) and (g[1][r_mid < 1.2] == 0).all()
    k, s = st.sk(0, (case.n_mol, 2 * case.n_mol))
    assert s.shape == (3, 61) and k.shape == (61,) and (s[0] >= 0).all() and (s[2] >= 0).all()


# ---- 3: several tiles, skin mode -------------------------------------------------------------------------------------
def test_lj1500_in_skin_mode_covers_diagonal_and_off_diagonal_tile_pairs():
    """1500 atoms = 5 full tiles + a 220-atom tail: 21 tile pairs, 6 diagonal.  Verlet-skin reuse: the B of a sampled step is
    launched on its own in front of the sample."""
    case = _Case("lj1500", skin=1.25)
    st, _, _ = _check_against_chunks(case, 128, _half(case), 9)
    assert st.kvectors.shape == (61, 3)
    ks, ss = st.sk(0, case.n, shell_average=True)
    # |n|^2 = 7 is no sum of three squares: the shells up to 9 are 1 2 3 4 5 6 8 9
    n2 = np.array([1, 2, 3, 4, 5, 6, 8, 9], dtype=np.float64)
    assert ss.shape == (1, 8) and (ss >= 0).all()
    assert np.allclose(ks, 2.0 * np.pi * np.sqrt(n2) / float(np.float32(case.box)), rtol=1e-14)


# ---- 4: two boxes ----------------------------------------------------------------------------------------------------
def test_two_boxes_in_bohr_keep_their_own_counts_and_sums():
    case = _Case("lj", n_boxes=2, length_per_nm=wl.BOHR_PER_NM)
    st, _, _ = _check_against_chunks(case, 64, _half(case), 9)
    assert not np.array_equal(st.rdf_counts[0], st.rdf_counts[1])           # the boxes carry different velocities
    assert not np.array_equal(st.sk_sum[0], st.sk_sum[1])
    for b in range(2):
        assert 0 < int(st.rdf_counts[b].sum()) <= CHUNKS * case.n * (case.n - 1)


# ---- 5: three different edges ----------------------------------------------------------------------------------------
def test_orthorhombic_box_uses_the_shortest_edge_and_per_axis_k():
    case = _Case("lj")
    scale = np.array([1.0, 0.9, 1.15])
    L = case.box
    case.box = (np.float32(L) * scale.astype(np.float32)).astype(np.float32)
    case.pos = case.pos * scale[None, :]
    half = float(np.float32(0.5) * case.box.min())
    # the default r_max is half the shortest edge
    eng, x, v, f = case.make()
    eng.structure_configure(case.K, rdf_bins=100, sk_n2max=9)
    case.run(eng, x, v, f, CHUNKS * case.K)
    dflt = eng.structure_read()
    eng.close()
    assert dflt.r_max == half
    st, _, _ = _check_against_chunks(case, 100, half, 9)
    assert np.array_equal(dflt.rdf_counts, st.rdf_counts) and np.array_equal(dflt.sk_sum, st.sk_sum)
    k, _ = st.sk(0, case.n)
    e = case.box.astype(np.float64)
    assert np.allclose(k[:3], [2 * np.pi / e[2], 2 * np.pi / e[1], 2 * np.pi / e[0]], rtol=1e-14)
    with pytest.raises(ValueError, match="cubic"):
        st.sk(0, case.n, shell_average=True)


# ---- 6: the three samplers together ----------------------------------------------------------------------------------
def test_reporter_sampler_and_recorder_keep_their_own_step_lists():
    """intervals 4 (reporter), 6 (structure sampler), 3 (recorder) over 24 steps; r_max = 5.0 < cutoff, so the reporter's
    edge-list histogram and the all-pairs one are held to the same reference class and tolerance, each over its own steps
    (they share steps 12 and 24)."""
    case = _Case("lj")
    n_steps, bins, r_max = 24, 64, 5.0
    cuts = sorted(set(range(3, n_steps + 1, 3)) | set(range(4, n_steps + 1, 4)) | set(range(6, n_steps + 1, 6)))
    (xr, vr, fr), _, _, frames = _reference_chunks(case, 0, r_max, 0, steps=cuts)
    at = dict(zip(cuts, frames))
    eng, x, v, f = case.make()
    eng.report_configure(4, rdf_bins=bins, rdf_rmax=r_max)
    eng.structure_configure(6, rdf_bins=bins, rdf_rmax=r_max, sk_n2max=9)
    eng.traj_configure(3, max_frames=8, fields=("x",))
    case.run(eng, x, v, f, n_steps)
    rep, st, trj = eng.report_read(), eng.structure_read(), eng.traj_read()
    out = _state(x, v, f)
    eng.close()
    assert np.array_equal(out[0], xr) and np.array_equal(out[1], vr) and np.array_equal(out[2], fr)   # = all off
    assert np.array_equal(rep.steps, np.arange(4, 25, 4)) and rep.frames == 6
    assert st.frames == 4
    assert np.array_equal(trj.steps, np.arange(3, 25, 3))
    for q, g in enumerate(range(3, 25, 3)):
        assert np.array_equal(trj.x[q].reshape(-1, 3), at[g])
    ref_rep, ref_st, ref_sk = _RefHist(1, 1, bins, r_max), _RefHist(1, 1, bins, r_max), _RefSk(1, 1, 9)
    for g in range(4, 25, 4):
        ref_rep.add(0, at[g], case.box, None)
    for g in range(6, 25, 6):
        ref_st.add(0, at[g], case.box, None)
        ref_sk.add(0, at[g], case.box, None)
    ref_rep.check(rep.rdf_counts, "reporter")
    ref_st.check(st.rdf_counts)
    ref_sk.check(st.sk_sum)


# ---- 7: overflow inside the run --------------------------------------------------------------------------------------
def test_overflow_inside_the_run_gives_the_counts_and_sums_of_an_ample_buffer():
    from gamd_amd.engine import GamdForce
    nl, steps = 1500, 8
    sd = make_state_dict(ModelConfig(kind="lj", conv_layer=2), 2, 5.0, 1.7)
    pos, box = wl.lj_box(nl, seed=4)
    res = []
    for cap in (0, 4000):
        x = torch.from_numpy(pos).float().cuda()
        v = torch.from_numpy(wl.maxwell_boltzmann(nl, 300.0, seed=3)).float().cuda()
        big = GamdForce(sd, nl, box, 7.5, scaler=SHIPPED_SCALERS["lj"])
        f = big.forward(x, denormalize=True).clone()
        big.close()
        eng = GamdForce(sd, nl, box, 7.5, scaler=SHIPPED_SCALERS["lj"], edge_capacity=cap)
        eng.structure_configure(2, rdf_bins=64, sk_n2max=9)
        eng.md_run(x, v, f, steps, seed=11, sync=False)
        assert eng.sync_status() == (1 if cap else 0)
        res.append((eng.structure_read(), x.cpu().numpy()))
        eng.close()
    (a, xa), (b, xb) = res
    assert np.array_equal(xa, xb)
    assert a.frames == b.frames == 4
    assert np.array_equal(a.rdf_counts, b.rdf_counts) and int(a.rdf_counts.sum()) > 0
    assert np.array_equal(a.sk_sum.view(np.int64), b.sk_sum.view(np.int64)) and np.abs(a.sk_sum).max() > 0


# ---- 8: accumulation, reset, interval 0 ------------------------------------------------------------------------------
def test_accumulation_across_calls_reset_and_interval_zero():
    case = _Case("lj", K=3)
    n, half = 9, _half(case)
    eng, x, v, f = case.make()
    eng.structure_configure(case.K, rdf_bins=64, rdf_rmax=half, sk_n2max=9)
    case.run(eng, x, v, f, 2 * n)
    one = eng.structure_read()
    eng.close()
    eng, x, v, f = case.make()
    eng.structure_configure(case.K, rdf_bins=64, rdf_rmax=half, sk_n2max=9)
    case.run(eng, x, v, f, n - 1)                      # g runs across calls: 8 + 10 steps sample at 3, 6 | 9, 12, 15, 18
    case.run(eng, x, v, f, n + 1, first_step=n - 1)
    two = eng.structure_read()
    assert one.frames == two.frames == 6
    assert np.array_equal(two.rdf_counts, one.rdf_counts) and np.array_equal(two.sk_sum.view(np.int64), one.sk_sum.view(np.int64))
    eng.structure_reset()
    z = eng.structure_read()
    assert z.frames == 0 and int(z.rdf_counts.sum()) == 0 and not z.sk_sum.any() and z.kvectors.shape == (61, 3)
    # after the reset the count starts again: K more steps give one frame, the frame of the positions the run ends at
    case.run(eng, x, v, f, case.K, first_step=2 * n)
    again = eng.structure_read()
    assert again.frames == 1
    rh, rs = _RefHist(1, 1, 64, half), _RefSk(1, 1, 9)
    rh.add(0, x.cpu().numpy(), case.box, None)
    rs.add(0, x.cpu().numpy(), case.box, None)
    rh.check(again.rdf_counts)
    rs.check(again.sk_sum)
    # interval 0: off, what was sampled stays readable, further steps add nothing
    eng.structure_configure(0)
    case.run(eng, x, v, f, case.K, first_step=2 * n + case.K)
    off = eng.structure_read()
    assert off.frames == 1 and np.array_equal(off.rdf_counts, again.rdf_counts) and np.array_equal(off.sk_sum, again.sk_sum)
    eng.close()


# ---- 9: the same bits run after run ----------------------------------------------------------------------------------
def test_two_fresh_runs_give_identical_counts_and_sum_bits():
    case = _Case("lj")
    (_, a), (_, b) = (_sampled_run(case, 128, _half(case), 16) for _ in range(2))
    assert a.frames == b.frames == CHUNKS
    assert np.array_equal(a.rdf_counts, b.rdf_counts) and int(a.rdf_counts.sum()) > 0
    assert np.array_equal(a.sk_sum.view(np.int64), b.sk_sum.view(np.int64)) and np.abs(a.sk_sum).max() > 0


# ---- 10: rejections --------------------------------------------------------------------------------------------------
def test_rejections():
    from gamd_amd._lib import GamdError
    case = _Case("lj")
    eng, x, v, f = case.make()
    x0 = x.clone()
    eng.structure_configure(4, rdf_bins=64, rdf_rmax=_half(case) * 1.001)      # the box of a run is known at the run
    with pytest.raises(GamdError, match="rdf_rmax"):
        case.run(eng, x, v, f, 4)
    assert torch.equal(x, x0)                                                   # nothing was enqueued
    eng.structure_configure(4, rdf_bins=64, rdf_rmax=_half(case), sk_n2max=4)
    with pytest.raises(GamdError, match="rdf_rmax"):                            # a smaller box than the constructor's
        eng.md_run(x, v, f, 4, box=0.99 * case.box, **case.md)
    assert torch.equal(x, x0)
    with pytest.raises(GamdError, match="-22.*rdf_bins"):
        eng.structure_configure(4, rdf_bins=1025, rdf_rmax=5.0)
    with pytest.raises(GamdError, match="-22.*k-vectors"):
        eng.structure_configure(4, sk_n2max=155)                                # K = 4108
    with pytest.raises(GamdError, match="-22.*rdf_rmax"):
        eng.structure_configure(4, rdf_bins=64, rdf_rmax=0.0)
    # the configuration that was accepted last is still in force
    case.run(eng, x, v, f, 4, sync=False)
    with pytest.raises(GamdError, match="-22.*enqueued"):                       # a run is pending
        eng.structure_configure(4, rdf_bins=32, rdf_rmax=5.0)
    with pytest.raises(GamdError, match="-22.*enqueued"):
        eng.structure_reset()
    assert eng.sync_status() == 0
    st = eng.structure_read()
    assert st.frames == 1 and st.rdf_counts.shape == (1, 1, 64) and st.kvectors.shape == (16, 3)
    eng.close()


# ---- 11: checked build -----------------------------------------------------------------------------------------------
CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_structure as t
from gamd_amd import _lib
case = t._Case("water")
(x, v, f), st = t._sampled_run(case, 97, 6.0, 9, exclude=True)
print("RESULT", json.dumps(dict(version=_lib.load().gamd_version().decode(), frames=st.frames, counts=st.rdf_counts.tolist(),
                                sk=st.sk_sum.view(np.int64).tolist())))
"""


def test_checked_build_passes_every_range_check_with_the_same_counts_and_sums():
    """water with the perm lookups of exclude_same_molecule under libgamd_hip_chk.so in a child process: every perm value the
    sampler reads is range-checked there; a violation would come back as -35."""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    env = {k: v for k, v in os.environ.items() if k not in ("GAMD_LIB", "GAMD_CHK_INJECT")}
    env["GAMD_LIB"] = CHK
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert p.returncode == 0 and "RESULT" in p.stdout, (p.stdout[-800:], p.stderr[-1500:])
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got["version"].endswith("checked")
    _, st = _sampled_run(_Case("water"), 97, 6.0, 9, exclude=True)
    assert got["frames"] == st.frames == CHUNKS
    assert got["counts"] == st.rdf_counts.tolist() and int(st.rdf_counts.sum()) > 0
    assert got["sk"] == st.sk_sum.view(np.int64).tolist()
