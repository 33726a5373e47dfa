"""The run reporter on the device: kinetic-energy log and g(r) histogram taken inside enqueued md_run / md_run_nhc calls,
against a reporter-off run of the same trajectory cut into chunks and looked at from the host after each chunk.

Conventions of the host references
* masses and the length unit are the fp32 values of the parameter blocks widened to double (what the library uses);
* the g(r) reference is a float64 min-image histogram of all i != j pairs of the chunk's final positions (the box as the
  fp32 value the library holds).  The device computes the distance in fp32, so a pair whose x = r * bins / r_max lies
  within 1e-5 x of an integer k may fall on either side of bin edge k: |cum_dev[k] - cum_ref[k]| is bounded by the number
  of such pairs (about ten times the fp32 rounding of the distance chain), and these pairs may be at most 1 % of all pairs
  or the case is ill-posed.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gamd_oracle as orc
from helpers import load_golden
from gamd_amd import workloads as wl
from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHK = os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")
CHUNKS = 6


def _f32(x):
    return float(np.float32(x))


# ---- host references -------------------------------------------------------------------------------------------------
def _ke_host(v, mass, length_per_nm, n_boxes):
    """sum 1/2 m (v / len)^2 per box in float64; mass [N] float64 (fp32 values widened)."""
    vn = v.astype(np.float64) / (_f32(length_per_nm) if length_per_nm else 10.0)
    per_atom = mass * (vn * vn).sum(axis=1)
    return 0.5 * per_atom.reshape(n_boxes, -1).sum(axis=1)


def _pairs_host(x, box, r_max):
    """float64 min-image distances of all i != j pairs of ONE box with r < r_max: (i, j, r)."""
    xd = x.astype(np.float64)
    L = _f32(box)
    d = xd[:, None, :] - xd[None, :, :]
    d -= L * np.round(d / L)
    r = np.sqrt((d * d).sum(-1))
    np.fill_diagonal(r, np.inf)
    i, j = np.nonzero(r < r_max)
    return i, j, r[i, j]


def _class_of(species, i, j):
    if species is None:
        return np.zeros(i.shape[0], dtype=np.int64)
    so, do = species[i] != 0, species[j] != 0
    return np.where(so & do, 0, np.where(so | do, 1, 2))


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
            # cum[k] for k = 0 .. bins: pairs strictly below edge k
            self.cum[b, c] += np.searchsorted(np.sort(xs[m]), np.arange(self.bins + 1), side="left")
            self.near[b, c] += np.bincount(k[m & near].astype(np.int64), minlength=self.bins + 2)[:self.bins + 1]
        self.total += int((xs < self.bins).sum())

    def check(self, counts):
        """counts uint64 [B, P, bins] from the device"""
        dev = np.concatenate([np.zeros(counts.shape[:2] + (1,), np.int64), np.cumsum(counts.astype(np.int64), axis=2)], axis=2)
        excused = int(self.near.sum())
        print(f"g(r): {int(counts.sum())} device pairs, {self.total} reference pairs, {excused} within 1e-5 of a bin edge, "
              f"max |cum_dev - cum_ref| {int(np.abs(dev - self.cum).max())}")
        assert excused <= 0.01 * self.total, "ill-posed: more than 1 % of the pairs sit on a bin edge"
        assert (np.abs(dev - self.cum) <= self.near).all()


# ---- cases -----------------------------------------------------------------------------------------------------------
class _Case:
    """one seeded system + integrator; make() gives a fresh engine and state"""

    def __init__(self, kind, integrator="baoab", n_boxes=1, length_per_nm=0.0, edge_dtype="f32", skin=0.0, K=4,
                 edge_capacity=0):
        self.kind, self.integrator, self.nb, self.len, self.K = kind, integrator, n_boxes, length_per_nm, K
        self.edge_dtype, self.skin, self.edge_capacity = edge_dtype, skin, edge_capacity
        if kind in ("lj", "lj1500"):
            if kind == "lj":
                g, _, self.sd = load_golden("lj258_seed0")
                self.box, self.rc, self.n = float(g["box"]), float(g["cutoff"]), 258
                self.pos = np.mod(g["pos"], self.box)
            else:                                      # above 1024 atoms: the grid-wide neighbour kernels in skin mode
                self.sd = make_state_dict(ModelConfig(kind="lj", conv_layer=2), 2, 5.0, 1.7)
                self.n, self.rc = 1500, 7.5
                self.pos, self.box = wl.lj_box(self.n, seed=4)
            self.species = None
            self.mass = np.full(self.n * n_boxes, _f32(39.9), dtype=np.float64)
            self.v0 = np.concatenate([wl.maxwell_boltzmann(self.n, 100.0, seed=90 + b) for b in range(n_boxes)])
            self.md = dict(dt_ps=0.002, mass_amu=39.9, temperature_k=100.0, length_per_nm=length_per_nm)
            self.eng_kw = dict(scaler=SHIPPED_SCALERS["lj"])
            self.ndf = 3 * self.n
        else:
            _, _, self.sd = load_golden("tip3p774_seed3")
            n_mol = 64
            self.pos, self.box, self.species, bonds = wl.water_box(n_mol, seed=5, jitter=0.0, wrap=False)
            self.rc, self.n, self.n_mol = 4.2, 3 * n_mol, n_mol
            m = np.where(self.species == 1, _f32(wl.MASS_O), _f32(wl.MASS_H)).astype(np.float64)
            self.mass = np.tile(m, n_boxes)
            pairs, _ = orc.water_constraints(self.n, wl.TIP3P_R_OH, wl.TIP3P_R_HH)
            mm = np.where(self.species == 1, wl.MASS_O, wl.MASS_H).astype(np.float64).reshape(-1, 1)
            v0 = np.random.default_rng(6).normal(0, 1.0, (self.n, 3)) * 10.0 * np.sqrt(wl.KB * 300.0 / mm)
            self.v0 = orc.rattle_velocities(self.pos, v0, (1.0 / mm).reshape(-1), pairs)
            self.md = dict(dt_ps=0.0005, mass_amu=wl.MASS_O, mass_h_amu=wl.MASS_H, temperature_k=300.0, rigid_water=True,
                           r_oh=wl.TIP3P_R_OH, r_hh=wl.TIP3P_R_HH, species=self.species, remove_cm_motion=True)
            self.eng_kw = dict(bond=bonds, scaler=SHIPPED_SCALERS["tip3p"])
            self.ndf = 2 * self.n - 3
        self.n_pairs = 3 if kind == "water" else 1

    def make(self):
        from gamd_amd.engine import GamdForce
        eng = GamdForce(self.sd, self.n, self.box, self.rc, edge_dtype=self.edge_dtype, neighbor_skin=self.skin,
                        n_boxes=self.nb, edge_capacity=self.edge_capacity, **self.eng_kw)
        x = torch.from_numpy(np.tile(self.pos, (self.nb, 1))).float().cuda()
        v = torch.from_numpy(self.v0 if self.v0.shape[0] == self.n * self.nb else np.tile(self.v0, (self.nb, 1))).float().cuda()
        sp = None if self.species is None else np.tile(self.species, self.nb)
        f = eng.forward(x, species=sp, denormalize=True).clone()
        return eng, x, v, f

    def run(self, eng, x, v, f, n_steps, first_step=0, chain=None, sync=True):
        md = dict(self.md)
        if md.get("species") is not None:
            md["species"] = np.tile(self.species, self.nb)
        if self.integrator == "baoab":
            eng.md_run(x, v, f, n_steps, gamma_per_ps=25.0, seed=11, first_step=first_step, sync=sync, **md)
            return None
        return eng.md_run_nhc(x, v, f, n_steps, chain_state=chain, frequency_per_ps=25.0, sync=sync, **md)

    def report_kw(self):
        return dict(rigid_water=self.kind == "water")


def _state(x, v, f):
    return x.cpu().numpy().copy(), v.cpu().numpy().copy(), f.cpu().numpy().copy()


def _reference_chunks(case, bins, r_max, exclude=False):
    """reporter-off run in CHUNKS calls of K steps: final state, KE after each chunk, reference histogram, edge count"""
    eng, x, v, f = case.make()
    ref = _RefHist(case.nb, case.n_pairs, bins, r_max) if bins else None
    kes, chain, nonself = [], None, 0
    for c in range(CHUNKS):
        chain = case.run(eng, x, v, f, case.K, first_step=c * case.K, chain=chain)
        xs, vs, _ = _state(x, v, f)
        kes.append(_ke_host(vs, case.mass, case.len, case.nb))
        if ref:
            for b in range(case.nb):
                ref.add(b, xs[b * case.n:(b + 1) * case.n], case.box, case.species, exclude)
            e = eng.debug_edges()
            nonself += int((e[0] != e[1]).sum())
    out = _state(x, v, f)
    eng.close()
    return out, np.array(kes), ref, nonself


def _reported_run(case, bins, r_max, exclude=False, **kw):
    eng, x, v, f = case.make()
    eng.report_configure(case.K, rdf_bins=bins, rdf_rmax=r_max, exclude_same_molecule=exclude, **case.report_kw(), **kw)
    case.run(eng, x, v, f, CHUNKS * case.K)
    rep = eng.report_read()
    out = _state(x, v, f)
    eng.close()
    return out, rep


def _check_against_chunks(case, bins=100, r_max=None, strict_state=True):
    r_max = case.rc if r_max is None else r_max
    (xr, vr, fr), kes, ref, nonself = _reference_chunks(case, bins, r_max)
    (x, v, f), rep = _reported_run(case, bins, r_max)
    # 1. the reporter does not perturb the run
    assert np.array_equal(x, xr) and np.array_equal(v, vr) and np.array_equal(f, fr)
    # 2. the log
    assert rep.dropped == 0 and rep.frames == CHUNKS
    assert np.array_equal(rep.steps, case.K * np.arange(1, CHUNKS + 1))
    assert rep.ke.shape == (CHUNKS, case.nb)
    rel = np.abs(rep.ke - kes) / kes
    print(f"KE: max relative difference to the float64 host sum {rel.max():.3e}")
    assert rel.max() < 1e-10
    assert np.allclose(rep.temperature, 2.0 * rep.ke / (case.ndf * wl.KB), rtol=1e-14, atol=0)
    if case.nb > 1:
        assert not np.allclose(rep.ke[:, 0], rep.ke[:, 1], rtol=1e-6)         # the boxes carry different velocities
    # 3. the histogram
    assert rep.rdf_counts.shape == (case.nb, case.n_pairs, bins)
    if _f32(r_max) >= _f32(case.rc):
        assert int(rep.rdf_counts.sum()) == nonself                          # the edge set is exact
    ref.check(rep.rdf_counts)
    return rep


# ---- 1-3: exact rebuild every step -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,integrator", [("lj", "baoab"), ("water", "baoab"), ("lj", "nhc")])
def test_reporter_leaves_the_run_alone_and_logs_what_the_host_computes(kind, integrator):
    """BAOAB free atoms, BAOAB rigid water with remove_cm_motion (three pair classes), NHC: one reported call of 6 K steps
    against six unreported calls of K steps."""
    _check_against_chunks(_Case(kind, integrator), bins=100)


def test_two_boxes_in_bohr_keep_their_own_rows_and_histograms():
    _check_against_chunks(_Case("lj", "baoab", n_boxes=2, length_per_nm=wl.BOHR_PER_NM), bins=64)


def test_r_max_below_the_cutoff_and_above_it():
    from gamd_amd._lib import GamdError
    case = _Case("lj")
    _check_against_chunks(case, bins=64, r_max=5.0)
    eng, x, v, f = case.make()
    with pytest.raises(GamdError, match="rdf_rmax"):
        eng.report_configure(4, rdf_bins=64, rdf_rmax=case.rc * 1.01)
    eng.close()


def test_exclude_same_molecule_removes_exactly_the_intramolecular_pairs():
    case = _Case("water")
    _, rep = _reported_run(case, 100, case.rc)
    (x, v, f), rep_x = _reported_run(case, 100, case.rc, exclude=True)
    assert rep.frames == rep_x.frames == CHUNKS
    diff = rep.rdf_counts.astype(np.int64) - rep_x.rdf_counts.astype(np.int64)
    assert (diff >= 0).all() and int(diff.sum()) == 6 * case.n_mol * CHUNKS
    assert [int(d) for d in diff[0].sum(axis=1)] == [0, 4 * case.n_mol * CHUNKS, 2 * case.n_mol * CHUNKS]
    (_, _, _), _, ref, _ = _reference_chunks(case, 100, case.rc, exclude=True)
    ref.check(rep_x.rdf_counts)
    # normalised: no intramolecular peak left below 1.2 A in O-H
    r_mid, g = rep_x.rdf(0, (case.n_mol, 2 * case.n_mol))
    assert g.shape == (3, 100) and (g[1][r_mid < 1.2] == 0).all()


# ---- 4: skin mode ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lj", "water", "lj1500"])
def test_skin_mode_completes_the_second_half_before_the_sample(kind):
    """Verlet-skin reuse (the B of a step rides in the next step's first neighbour kernel; on sampled steps it is launched on
    its own): the same checks against a reporter-off run of the same mode in six chunks, x and v equality first."""
    case = _Case(kind, skin=0.7 if kind == "water" else 1.25)
    _check_against_chunks(case, bins=100)
    if kind == "water":                                 # NHC has no fused halves; it must not mind the skin either
        _check_against_chunks(_Case(kind, "nhc", skin=0.7), bins=100)


# ---- 5: overflow inside the run --------------------------------------------------------------------------------------
def test_overflow_inside_the_run_gives_the_log_and_counts_of_an_ample_buffer():
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
        eng.report_configure(2, rdf_bins=64)
        eng.md_run(x, v, f, steps, seed=11, sync=False)
        assert eng.sync_status() == (1 if cap else 0)
        res.append((eng.report_read(), x.cpu().numpy()))
        eng.close()
    (a, xa), (b, xb) = res
    assert np.array_equal(xa, xb)
    assert np.array_equal(a.steps, [2, 4, 6, 8]) and np.array_equal(a.steps, b.steps)
    assert np.array_equal(a.ke, b.ke) and np.array_equal(a.rdf_counts, b.rdf_counts)
    assert a.frames == b.frames == 4 and a.dropped == b.dropped == 0 and int(a.rdf_counts.sum()) > 0


@pytest.mark.parametrize("skin_frac", [0.0, 1.0 / 6.0])
def test_overflow_in_the_middle_of_a_run_counts_no_sample_twice(skin_frac):
    """A capacity that holds the first edge list but not what the contracting box needs later (the pattern of
    tests/test_gpu_batch.py, five boxes): samples in front of the freeze completed and must not be added again by the resumed run, the
    frozen step's sample and the later ones must not be lost.  Exact mode: log and counts of the ample run bit for bit.  Skin
    mode: the regrow forces a candidate rebuild the ample run does not have, which changes the summation order inside CSR
    rows, so the trajectories agree to fp32 rounding (1e-5 in x, 1e-4 in v: the existing test's bounds): KE to 2e-4, and
    only pairs within 1e-5 r of the cutoff sphere can enter or leave the histogram (well below 0.1 % of the pairs)."""
    from gamd_amd.engine import GamdForce
    g, _, _ = load_golden("lj258_seed0")
    nb, n, box, rc = 5, 258, float(g["box"]), float(g["cutoff"])
    sd = make_state_dict(ModelConfig(kind="lj"), 0, 5.3, 1.6)
    kw = dict(n_boxes=nb, scaler=SHIPPED_SCALERS["lj"], neighbor_skin=skin_frac * rc)
    base, rng = np.mod(g["pos"], box), np.random.default_rng(2)
    pos = np.concatenate([base + (rng.normal(0, 0.3, base.shape) if b else 0.0) for b in range(nb)])
    x0 = torch.from_numpy(pos).float().cuda()
    # velocities that pull every box's atoms towards its centre: the edge count grows step by step
    v0 = (-(torch.remainder(x0, box) - box / 2)).contiguous() * 1.5
    probe = GamdForce(sd, n, box, rc, **kw)
    probe.forward(x0)
    e_now = probe.counts()[0]
    probe.close()
    res = []
    for cap in (0, e_now + 40):
        eng = GamdForce(sd, n, box, rc, edge_capacity=cap, **kw)
        x, v = x0.clone(), v0.clone()
        f = eng.forward(x, denormalize=True).clone()
        assert eng.last_status == 0
        eng.report_configure(3, rdf_bins=64)
        eng.md_run(x, v, f, 30, temperature_k=0.0, gamma_per_ps=0.0, seed=1)
        assert eng.last_status == (1 if cap else 0), "the run was meant to outgrow its edge buffer"
        assert eng.counts()[0] > e_now + 40
        res.append(eng.report_read())
        eng.close()
    a, b = res
    assert np.array_equal(a.steps, 3 * np.arange(1, 11)) and np.array_equal(b.steps, a.steps)
    assert a.frames == b.frames == 10 and a.dropped == b.dropped == 0 and a.ke.shape == (10, nb)
    ta, tb = int(a.rdf_counts.sum()), int(b.rdf_counts.sum())
    print(f"skin {skin_frac:.3f}: pair totals {ta} / {tb}, max KE difference {np.abs(b.ke / a.ke - 1).max():.2e}")
    if skin_frac == 0.0:
        assert np.array_equal(a.ke, b.ke) and np.array_equal(a.rdf_counts, b.rdf_counts)
    else:
        assert np.abs(b.ke / a.ke - 1).max() < 2e-4 and abs(ta - tb) <= 1e-3 * ta


# ---- 6: accumulation, reset, a full log ------------------------------------------------------------------------------
def test_accumulation_across_calls_reset_and_a_full_log():
    case = _Case("lj", K=3)
    n = 9
    eng, x, v, f = case.make()
    eng.report_configure(case.K, rdf_bins=64)
    case.run(eng, x, v, f, 2 * n)
    one = eng.report_read()
    eng.close()
    eng, x, v, f = case.make()
    eng.report_configure(case.K, rdf_bins=64, max_samples=4)
    case.run(eng, x, v, f, n - 1)                      # g runs across calls: 8 + 10 steps sample at 3, 6 | 9, 12, 15, 18
    case.run(eng, x, v, f, n + 1, first_step=n - 1)
    two = eng.report_read()
    assert np.array_equal(one.steps, 3 * np.arange(1, 7)) and one.frames == 6 and one.dropped == 0
    assert two.dropped == 2 and two.frames == 6 and two.steps.shape == (4,)
    assert np.array_equal(two.steps, one.steps[:4]) and np.array_equal(two.ke, one.ke[:4])
    assert np.array_equal(two.rdf_counts, one.rdf_counts)           # the histogram keeps accumulating
    eng.report_reset()
    z = eng.report_read()
    assert z.steps.shape == (0,) and z.frames == 0 and z.dropped == 0 and int(z.rdf_counts.sum()) == 0
    # after the reset the count starts again: the same state run on gives the rows of a fresh reporter
    case.run(eng, x, v, f, case.K, first_step=2 * n)
    again = eng.report_read()
    assert np.array_equal(again.steps, [case.K]) and again.frames == 1
    assert abs(again.ke[0, 0] / _ke_host(v.cpu().numpy(), case.mass, case.len, 1)[0] - 1.0) < 1e-10
    # interval 0: off, what was recorded stays readable, further steps add nothing
    eng.report_configure(0)
    case.run(eng, x, v, f, case.K, first_step=2 * n + case.K)
    off = eng.report_read()
    assert np.array_equal(off.steps, again.steps) and np.array_equal(off.rdf_counts, again.rdf_counts)
    eng.close()


# ---- 7: checked build ------------------------------------------------------------------------------------------------
CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_report as t
from gamd_amd import _lib
case = t._Case(%r, skin=%r)
(x, v, f), rep = t._reported_run(case, 64, case.rc, exclude=case.kind == "water")
print("RESULT", json.dumps(dict(version=_lib.load().gamd_version().decode(), steps=rep.steps.tolist(), ke=rep.ke.tolist(),
                                counts=rep.rdf_counts.tolist(), frames=rep.frames, dropped=rep.dropped)))
"""


@pytest.mark.parametrize("kind,skin", [("water", 0.0), ("lj", 1.25)])
def test_checked_build_passes_every_range_check_with_the_same_counts(kind, skin):
    """KE + g(r) (water: with the perm lookups of exclude_same_molecule) under libgamd_hip_chk.so in a child process: every
    col / erow / perm / row_ptr value the reporter reads is range-checked there; a violation would come back as -35."""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), kind, skin)
    env = {k: v for k, v in os.environ.items() if k not in ("GAMD_LIB", "GAMD_CHK_INJECT")}
    env["GAMD_LIB"] = CHK
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert p.returncode == 0 and "RESULT" in p.stdout, (p.stdout[-800:], p.stderr[-1500:])
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got["version"].endswith("checked")
    case = _Case(kind, skin=skin)
    _, rep = _reported_run(case, 64, case.rc, exclude=kind == "water")
    assert got["steps"] == rep.steps.tolist() and got["frames"] == rep.frames == CHUNKS and got["dropped"] == 0
    assert got["counts"] == rep.rdf_counts.tolist() and int(rep.rdf_counts.sum()) > 0
    assert got["ke"] == rep.ke.tolist()


# ---- 8: reduced-precision edge dtypes --------------------------------------------------------------------------------
@pytest.mark.parametrize("edge_dtype", ["bf16", "f16x3"])
def test_reduced_precision_edge_dtypes_report_like_fp32(edge_dtype):
    """the reporter reads v, pos_s and the edge list only: the same checks against a reporter-off run of the same dtype"""
    _check_against_chunks(_Case("lj", edge_dtype=edge_dtype), bins=100)
