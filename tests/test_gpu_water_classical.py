"""The water classical observer on the device: O-O Lennard-Jones plus an Ewald sum in double for 3-site water, on given
positions (water_classical_forces) and inside enqueued md_run / md_run_nhc calls, against the float64 host reference of
tests/water_classical_ref.py on the frames of an observer-off run of the same trajectory cut into chunks.

Shapes: 774 atoms (258 molecules; three 256-atom row tiles plus a tail of 6; 256 is no multiple of 3, so molecules straddle tile
edges) and two boxes of 258 atoms (86 molecules, the last one split O | H,H across the tile edge) with different positions and
edges.

Tolerances (derived, not measured; DESIGN.md sections 4.9 and 4.10).  The device and the reference evaluate a term with the same
operations; they differ in the order of the sums, in erfc / erf / exp / sincospi (a few ulp each) and in S(k), which enters
the reciprocal force of every atom.  Each logged quantity and each force component lies within 1e-12 of the sum of the absolute
values of its terms: sum |u| for U_LJ and for U_real + U_excl, (4 pi C / V) sum_k A(k) (sum_j |q_j|)^2 for U_recip, |U_self| for
the one product U_self is, sum_j |F_ij| + (8 pi C / V) |q_i| sum_k A(k) |k| sum_j |q_j| for a force, and for each of the five
force-error sums the sum of its own absolute terms, recomputed on the host from the DEVICE's f_cl and the run's f.  Pair counts
are exact (every frame is asserted to hold no pair within 1e-12 r_cut of the cutoff) and the charge sum is exactly 0.
Nothing here claims parity with OpenMM or with a particle-mesh sum: the default parameters are unverified."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import classical_ref as cr
import gamd_oracle as orc
import water_classical_ref as wr
from gamd_amd import workloads as wl
from gamd_amd.weights import SHIPPED_SCALERS
from helpers import load_golden
from test_gpu_report import _Case, _state, _f32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHK = os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")
CHUNKS = 3
TOL = 1e-12
TOL_SPLIT = 1e-11                       # two splitting parameters against each other: the host test's bound
DELTA = 1e-8                            # ewald_tol of the cases checked against the host reference
WORST = {}                              # the largest observed fraction of each bound (printed; profiles/run_water_classical.md)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _note(name, value):
    WORST[name] = max(WORST.get(name, 0.0), float(value))
    return float(value)


class _Water(_Case):
    """test_gpu_report's water case (tip3p774_seed3 weights, whole rigid molecules, rattled velocities) at 258 molecules"""

    def __init__(self, integrator="baoab", skin=0.0, K=4, n_mol=258, edge_capacity=0):
        self.kind, self.integrator, self.nb, self.len, self.K = "water", integrator, 1, 0.0, K
        self.edge_dtype, self.skin, self.edge_capacity = "f32", skin, edge_capacity
        _, _, self.sd = load_golden("tip3p774_seed3")
        self.pos, self.box, self.species, bonds = wl.water_box(n_mol, seed=5, jitter=0.0, wrap=False)
        self.rc, self.n, self.n_mol = 4.2, 3 * n_mol, n_mol
        self.mass = np.where(self.species == 1, _f32(wl.MASS_O), _f32(wl.MASS_H)).astype(np.float64)
        pairs, _ = orc.water_constraints(self.n, wl.TIP3P_R_OH, wl.TIP3P_R_HH)
        mm = np.where(self.species == 1, wl.MASS_O, wl.MASS_H).astype(np.float64).reshape(-1, 1)
        v0 = np.random.default_rng(6).normal(0, 1.0, (self.n, 3)) * 10.0 * np.sqrt(wl.KB * 300.0 / mm)
        self.v0 = orc.rattle_velocities(self.pos, v0, (1.0 / mm).reshape(-1), pairs)
        self.md = dict(dt_ps=0.0005, mass_amu=wl.MASS_O, mass_h_amu=wl.MASS_H, temperature_k=300.0, rigid_water=True,
                       r_oh=wl.TIP3P_R_OH, r_hh=wl.TIP3P_R_HH, species=self.species, remove_cm_motion=True)
        self.eng_kw = dict(bond=bonds, scaler=SHIPPED_SCALERS["tip3p"])
        self.ndf, self.n_pairs = 2 * self.n - 3, 3


def _engine(n_mol, box, n_boxes=1):
    from gamd_amd.engine import GamdForce
    _, _, sd = load_golden("tip3p774_seed3")
    _, _, species, bonds = wl.water_box(n_mol, seed=5, jitter=0.0, wrap=False)
    return GamdForce(sd, 3 * n_mol, box, 4.2, bond=bonds, scaler=SHIPPED_SCALERS["tip3p"], n_boxes=n_boxes), species


def _check_box(tag, row, x_box, box, species, w, length_per_nm, fcl_dev, f_run=None):
    """one box of one frame: row [12] from the device, fcl_dev [n, 3] the device's forces"""
    ref = wr.evaluate(x_box, box, species, w, length_per_nm)
    fr = dict(lj=abs(row[0] - ref["u_lj"]) / (TOL * ref["abs_lj"]), coul=abs(row[1] - ref["u_coul"]) / (TOL * ref["abs_real"]),
              recip=abs(row[2] - ref["u_recip"]) / (TOL * ref["abs_recip"]), self=abs(row[3] - ref["u_self"]) / (TOL * abs(ref["u_self"])),
              force=(np.abs(fcl_dev - ref["forces"]) / (TOL * ref["abs_f"][:, None])).max())
    print(f"{tag}: pairs {row[4]:.0f} (ref {ref['pairs']:.0f}, {ref['near']} at the cutoff), K {ref['n_k']}, U_LJ {row[0]:.9e} U_coul {row[1]:.9e} "
          f"U_recip {row[2]:.9e} U_self {row[3]:.9e}, sum q {row[11]!r}; |dev - ref| / bound: " + ", ".join(f"{k} {v:.3e}" for k, v in fr.items()))
    for k, v in fr.items():
        _note(k, v)
    assert ref["near"] == 0, "ill-posed: a pair sits on the cutoff"
    assert ref["pairs"] > 0 and row[4] == ref["pairs"] and ref["abs_lj"] > 0
    assert row[11] == 0.0 and ref["sum_q"] == 0.0
    assert all(v <= 1.0 for v in fr.values()) and np.isfinite(fcl_dev).all()
    if f_run is not None:
        sums, ab = cr.force_error_sums(f_run, fcl_dev)
        ratio = np.abs(row[5:10] - sums[:5]) / (TOL * ab)
        print(f"{tag}: force-error sums {row[5:10]}, |dev - host| / bound {ratio}, left out of the cosine {row[10]:.0f}")
        _note("error sums", ratio.max())
        assert (ab > 0).all() and (ratio <= 1.0).all() and row[10] == sums[5]
    else:
        assert (row[5:11] == 0.0).all()
    return ref


def _rows(rd, q=0):
    return np.stack([getattr(rd, name)[q] for name in rd.COLUMNS], axis=-1)       # [B, 12]


# ---- 1: given positions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length_per_nm,kw", [
    (0.0, dict()),                                                        # Angstrom, the defaults: r_cut 9.5, no switch, no shift
    (0.0, dict(r_switch=8.0, shift=True)),
    (wl.BOHR_PER_NM, dict()),
    (wl.BOHR_PER_NM, dict(r_switch=8.0, shift=True)),
])
def test_forces_on_given_positions_774_atoms(length_per_nm, kw):
    unit = _f32(length_per_nm) / 10.0 if length_per_nm else 1.0
    pos, box, _, _ = wl.water_box(258, seed=5, jitter=0.02, wrap=False)
    x, box = (pos * unit).astype(np.float32), np.float32(box * unit)
    w = wr.Water(sigma_o=3.15075 * unit, r_cut=9.5 * unit, r_switch=kw.get("r_switch", 0.0) * unit, shift=kw.get("shift", False), ewald_tol=DELTA)
    assert 2 * w.r_cut <= box
    eng, species = _engine(258, float(box))
    eng.water_classical_configure(0, length_per_nm=length_per_nm, ewald_tol=DELTA,
                                  **{k: (v * unit if k == "r_switch" else v) for k, v in kw.items()})
    f, rd = eng.water_classical_forces(x, species, length_per_nm=length_per_nm)
    assert f.dtype == torch.float64 and tuple(f.shape) == (774, 3) and rd.energy.shape == (1, 1)
    ref = _check_box(f"774 atoms, len {length_per_nm}, {kw}", _rows(rd)[0], x, box, species, w, length_per_nm, f.cpu().numpy())
    assert abs(rd.energy[0, 0] - ref["energy"]) <= TOL * ref["abs_energy"]
    # the log is untouched by an evaluation outside a run
    log = eng.water_classical_read(forces=True)
    assert log.steps.shape == (0,) and np.array_equal(_bits(log.forces), _bits(f.cpu().numpy()))
    eng.close()


def _two_boxes(unit=1.0):
    pos, box, _, _ = wl.water_box(86, seed=5, jitter=0.02, wrap=False)
    scale = np.array([1.0, 1.03, 0.99])
    other, _, _, _ = wl.water_box(86, seed=7, jitter=0.02, wrap=False)
    x = np.concatenate([pos, other * scale[None, :]]) * unit
    boxes = (np.array([[box, box, box], box * scale]) * unit).astype(np.float32)
    return x.astype(np.float32), boxes


@pytest.mark.parametrize("length_per_nm,kw", [(0.0, dict()), (wl.BOHR_PER_NM, dict(r_switch=5.5, shift=True))])
def test_two_boxes_of_258_atoms_with_different_positions_and_edges(length_per_nm, kw):
    unit = _f32(length_per_nm) / 10.0 if length_per_nm else 1.0
    x, boxes = _two_boxes(unit)
    w = wr.Water(sigma_o=3.15075 * unit, r_cut=6.8 * unit, r_switch=kw.get("r_switch", 0.0) * unit, shift=kw.get("shift", False), ewald_tol=DELTA)
    assert 2 * w.r_cut <= boxes.min()
    eng, species = _engine(86, float(boxes[0, 0]), n_boxes=2)
    eng.water_classical_configure(0, **w.kwargs())
    f, rd = eng.water_classical_forces(x, species, box=boxes, length_per_nm=length_per_nm)
    fh, rows = f.cpu().numpy(), _rows(rd)
    for b in range(2):
        _check_box(f"box {b}, len {length_per_nm}", rows[b], x[b * 258:(b + 1) * 258], boxes[b], species, w, length_per_nm, fh[b * 258:(b + 1) * 258])
    assert rd.u_real[0, 0] != rd.u_real[0, 1] and rd.u_recip[0, 0] != rd.u_recip[0, 1]
    # the boxes are independent: box 1 alone (its own, shorter k-vector list is the part of the common one that carries weight)
    one, _ = _engine(86, boxes[1])
    one.water_classical_configure(0, **w.kwargs())
    f1, r1 = one.water_classical_forces(x[258:], species, box=boxes[1], length_per_nm=length_per_nm)
    for name in ("u_lj", "u_real", "u_self", "pairs", "sum_q"):
        assert _bits(getattr(r1, name))[0, 0] == _bits(getattr(rd, name))[0, 1], name
    ref = wr.evaluate(x[258:], boxes[1], species, w, length_per_nm)
    assert abs(r1.u_recip[0, 0] - rd.u_recip[0, 1]) <= TOL * ref["abs_recip"]
    assert (np.abs(f1.cpu().numpy() - fh[258:]) <= TOL * ref["abs_f"][:, None]).all()
    one.close()
    eng.close()


def test_two_splitting_parameters_agree_on_the_device():
    """the host test's pair (alpha, n2max) = (0.80, 400) and (0.92, 520) at L = 13.7, r_cut = 6.8: both leave less than 2e-14 of
    a term outside either sum, so the device's totals agree to 1e-11 of the sum of the absolute terms, and each agrees with the
    host reference to 1e-12 of them"""
    L = np.float32(13.7)
    pos, box, _, _ = wl.water_box(86, seed=5, jitter=0.02, wrap=False)
    x = (pos * (float(L) / box)).astype(np.float32)
    eng, species = _engine(86, float(L))
    res = []
    for alpha, n2max in ((0.80, 400), (0.92, 520)):
        w = wr.Water(r_cut=6.8, alpha=alpha, k_cut=2.0 * np.pi * np.sqrt(n2max) / float(L) * (1.0 + 1e-9))
        eng.water_classical_configure(0, **w.kwargs())
        f, rd = eng.water_classical_forces(x, species)
        fh = f.cpu().numpy()
        ref = _check_box(f"alpha {alpha}", _rows(rd)[0], x, L, species, w, 0.0, fh)
        assert ref["n_k"] == len(wr.kvectors(n2max)) and ref["tail"] == 0.0
        res.append((rd, fh, ref))
    (ra, fa, a), (rb, fb, b) = res
    d_e = abs(ra.energy[0, 0] - rb.energy[0, 0])
    ratio_f = (np.abs(fa - fb) / (TOL_SPLIT * np.maximum(a["abs_f"], b["abs_f"])[:, None])).max()
    print(f"E {ra.energy[0, 0]:.9f} / {rb.energy[0, 0]:.9f}: |dE| / bound {_note('split E', d_e / (TOL_SPLIT * max(a['abs_energy'], b['abs_energy']))):.3e}, "
          f"max |dF| / bound {_note('split F', ratio_f):.3e}")
    for name in ("u_real", "u_recip", "u_self"):
        assert abs(getattr(ra, name)[0, 0] - getattr(rb, name)[0, 0]) > 0.1 * abs(getattr(ra, name)[0, 0]), name
    assert d_e <= TOL_SPLIT * max(a["abs_energy"], b["abs_energy"]) and ratio_f <= 1.0
    eng.close()


# ---- 2: the same bits ------------------------------------------------------------------------------------------------
def test_periodic_images_and_a_second_call_give_the_same_bits():
    """Positions and box edges on a grid of 2^-10 A (edges 20.5, 19.25, 21.0): x + k L is exact in fp32, so d and L rint(d / L)
    stay on the grid in double (every image has the same minimum-image vectors bit for bit) and x - L floor(x / L) is the same
    double for every image (the same fractional coordinates, phases and S(k) bit for bit).  Atom-wise shifts: molecules are
    torn across images."""
    q = 2.0 ** -10
    pos, L, _, _ = wl.water_box(258, seed=5, jitter=0.02, wrap=False)
    box = np.array([20.5, 19.25, 21.0], dtype=np.float32)
    x = (np.rint(pos * (box.astype(np.float64) / L)[None, :] / q) * q).astype(np.float32)
    k = np.random.default_rng(3).integers(-2, 3, size=x.shape)
    xs = (x.astype(np.float64) + k * box.astype(np.float64)[None, :]).astype(np.float32)
    assert np.array_equal(xs.astype(np.float64), x.astype(np.float64) + k * box.astype(np.float64)[None, :]) and (k != 0).any()
    eng, species = _engine(258, box)
    eng.water_classical_configure(0, ewald_tol=DELTA)
    a = eng.water_classical_forces(x, species, box=box)
    b = eng.water_classical_forces(xs, species, box=box)
    c = eng.water_classical_forces(x, species, box=box)
    for other in (b, c):
        assert np.array_equal(_bits(a[0].cpu().numpy()), _bits(other[0].cpu().numpy()))
        assert np.array_equal(_bits(_rows(a[1])), _bits(_rows(other[1])))
    assert a[1].pairs[0, 0] > 0 and np.abs(a[0].cpu().numpy()).max() > 0 and a[1].u_recip[0, 0] > 0
    eng.close()


# ---- 3, 4: inside runs -----------------------------------------------------------------------------------------------
def _reference_frames(case, chunks):
    """observer-off run (a handle that was never configured) cut into `chunks` calls of K steps: final state, (x, f) at every
    cut, and afterwards the device's classical forces on every frame (gamd_water_eval: the sample's kernels on given positions)"""
    eng, x, v, f = case.make()
    chain, frames = None, []
    for c in range(chunks):
        chain = case.run(eng, x, v, f, case.K, first_step=c * case.K, chain=chain)
        xs, _, fs = _state(x, v, f)
        frames.append((xs, fs))
    out = _state(x, v, f)
    eng.water_classical_configure(0, ewald_tol=DELTA)
    fcl = [eng.water_classical_forces(xs, case.species, box=case.box)[0].cpu().numpy() for xs, _ in frames]
    eng.close()
    return out, frames, fcl


def _sampled_run(case, chunks, **kw):
    eng, x, v, f = case.make()
    eng.water_classical_configure(case.K, ewald_tol=DELTA, **kw)
    eng.report_configure(case.K, **case.report_kw())
    case.run(eng, x, v, f, chunks * case.K)
    rd, rep = eng.water_classical_read(forces=True), eng.report_read()
    out = _state(x, v, f)
    eng.close()
    return out, rd, rep


def _check_against_chunks(case, chunks=CHUNKS):
    (xr, vr, fr), frames, fcl = _reference_frames(case, chunks)
    (x, v, f), rd, rep = _sampled_run(case, chunks)
    # 1. the observer does not perturb the run (in skin mode: the B of a sampled step was complete in front of the sample)
    assert np.array_equal(x, xr) and np.array_equal(v, vr) and np.array_equal(f, fr)
    # 2. the rows
    assert rd.dropped == 0 and np.array_equal(rd.steps, case.K * np.arange(1, chunks + 1)) and np.array_equal(rd.steps, rep.steps)
    assert rd.energy.shape == (chunks, 1)
    w = wr.Water(ewald_tol=DELTA)
    for q, (xs, fs) in enumerate(frames):
        _check_box(f"water {case.integrator} skin {case.skin} frame {q}", _rows(rd, q)[0], xs, case.box, case.species, w, 0.0, fcl[q], fs)
    # 3. the last sample's forces are the ones the evaluation outside the run gives for that frame
    assert np.array_equal(_bits(rd.forces), _bits(fcl[-1]))
    fe = rd.force_errors(unit=0.0010364)
    assert all(fe[k].shape == (chunks, 1) and np.isfinite(fe[k]).all() for k in ("mae", "rmse", "cosine", "relative_mae"))
    assert (np.abs(fe["cosine"]) <= 1.0).all() and (fe["rmse"] >= fe["mae"]).all()
    return rd, rep


@pytest.mark.parametrize("integrator", ["baoab", "nhc"])
def test_water774_rows_are_the_reference_on_the_frames_of_an_observer_off_run(integrator, tmp_path):
    rd, rep = _check_against_chunks(_Water(integrator))
    rd.write_state_data(rep, tmp_path / "log.txt", 0.0005)
    assert len((tmp_path / "log.txt").read_text().splitlines()) == CHUNKS + 1


def test_skin_mode_completes_the_second_half_before_the_sample():
    """Verlet-skin reuse: the B of a step rides in the next step's first neighbour kernel; on sampled steps it is launched on its own."""
    _check_against_chunks(_Water(skin=0.7), chunks=2)


# ---- 5: overflow in the middle of a run ------------------------------------------------------------------------------
def test_overflow_in_the_middle_of_a_run_writes_every_row_once_with_the_bits_of_an_ample_buffer():
    """The scheme of tests/test_gpu_classical.py: flexible molecules contracting towards the centre of the box, a capacity that
    holds the first edge list but not a later one.  The samples in front of the freeze completed; the frozen step's sample and
    the later ones are enqueued again by the resumed run and write their own rows."""
    from gamd_amd.engine import GamdForce
    case = _Water()
    res = []
    x0 = torch.from_numpy(case.pos).float().cuda()
    v0 = (-(x0 - case.box / 2)).contiguous() * 6.0
    probe, x, v, f = case.make()
    e_now = probe.counts()[0]
    probe.close()
    md = dict(dt_ps=0.0005, mass_amu=wl.MASS_O, mass_h_amu=wl.MASS_H, temperature_k=0.0, gamma_per_ps=0.0, seed=1, species=case.species)
    for cap in (0, e_now + 60):
        eng = GamdForce(case.sd, case.n, case.box, case.rc, edge_capacity=cap, **case.eng_kw)
        x, v = x0.clone(), v0.clone()
        f = eng.forward(x, species=case.species, denormalize=True).clone()
        assert eng.last_status == 0
        eng.water_classical_configure(3, ewald_tol=DELTA)
        eng.md_run(x, v, f, 30, **md)
        assert eng.last_status == (1 if cap else 0), "the run was meant to outgrow its edge buffer"
        res.append((eng.water_classical_read(forces=True), x.cpu().numpy()))
        eng.close()
    (a, xa), (b, xb) = res
    assert np.array_equal(xa, xb)
    assert np.array_equal(a.steps, 3 * np.arange(1, 11)) and np.array_equal(b.steps, a.steps) and a.dropped == b.dropped == 0
    for name in a.COLUMNS:
        assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    assert np.array_equal(_bits(a.forces), _bits(b.forces))
    assert (a.pairs > 0).all() and np.isfinite(a.energy).all() and (a.sum_q == 0.0).all()


# ---- 6: accumulation, reset, a full log, interval 0 ------------------------------------------------------------------
def test_accumulation_across_calls_reset_a_full_log_and_interval_zero():
    case = _Water(K=3)
    n = 6
    eng, x, v, f = case.make()
    eng.water_classical_configure(case.K, ewald_tol=DELTA)
    case.run(eng, x, v, f, 2 * n)
    one = eng.water_classical_read()
    eng.close()
    eng, x, v, f = case.make()
    eng.water_classical_configure(case.K, max_samples=3, ewald_tol=DELTA)
    case.run(eng, x, v, f, n - 1)                      # g runs across calls: 5 + 7 steps sample at 3 | 6, 9, 12
    case.run(eng, x, v, f, n + 1, first_step=n - 1)
    two = eng.water_classical_read()
    assert np.array_equal(one.steps, 3 * np.arange(1, 5)) and one.dropped == 0
    assert two.dropped == 1 and np.array_equal(two.steps, one.steps[:3])
    for name in one.COLUMNS:
        assert np.array_equal(_bits(getattr(two, name)), _bits(getattr(one, name)[:3])), name
    eng.water_classical_reset()
    z = eng.water_classical_read()
    assert z.steps.shape == (0,) and z.dropped == 0 and z.energy.shape == (0, 1)
    # after the reset the count starts again: K more steps give one row, the row of the positions the run ends at
    case.run(eng, x, v, f, case.K, first_step=2 * n)
    again = eng.water_classical_read(forces=True)
    assert np.array_equal(again.steps, [case.K])
    _check_box("after reset", _rows(again)[0], x.cpu().numpy(), case.box, case.species, wr.Water(ewald_tol=DELTA), 0.0, again.forces, f.cpu().numpy())
    # interval 0: off, what was logged stays readable, further steps add nothing; the parameters it carries are taken
    eng.water_classical_configure(0, ewald_tol=DELTA, r_switch=8.0)
    case.run(eng, x, v, f, case.K, first_step=2 * n + case.K)
    off = eng.water_classical_read()
    assert np.array_equal(off.steps, again.steps) and np.array_equal(_bits(off.energy), _bits(again.energy))
    fo, ro = eng.water_classical_forces(x, case.species)
    _check_box("interval 0, switched", _rows(ro)[0], x.cpu().numpy(), case.box, case.species, wr.Water(ewald_tol=DELTA, r_switch=8.0), 0.0, fo.cpu().numpy())
    eng.close()


# ---- 7: refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    from gamd_amd._lib import GamdError
    from gamd_amd.engine import GamdForce
    lj = _Case("lj")
    eng, x, v, f = lj.make()
    with pytest.raises(GamdError, match="-22.*GAMD_KIND_LJ"):
        eng.water_classical_configure(4, r_cut=6.0)
    with pytest.raises(GamdError, match="-22.*GAMD_KIND_LJ"):
        eng.water_classical_forces(x, np.ones(lj.n, dtype=np.uint8))
    eng.close()
    case = _Water()
    odd = GamdForce(case.sd, case.n + 1, case.box, case.rc, **case.eng_kw)          # 775 atoms: not O,H,H triples
    with pytest.raises(GamdError, match="-22.*multiple of 3"):
        odd.water_classical_configure(4)
    odd.close()
    half = float(np.float32(0.5) * np.float32(case.box))
    eng, x, v, f = case.make()
    x0 = x.clone()
    with pytest.raises(GamdError, match="-22.*GAMD_KIND_WATER"):            # the Lennard-Jones observer still refuses water
        eng.classical_configure(4, r_cut=4.0, r_switch=3.0)
    with pytest.raises(GamdError, match="-22.*k_cut"):                      # more than 131 072 k-vectors in a 20 A box
        eng.water_classical_configure(4, k_cut=14.0)
    with pytest.raises(GamdError, match="-22.*k_cut"):                      # none
        eng.water_classical_configure(4, k_cut=0.1)
    for field in ("sigma_o", "r_cut", "alpha", "k_cut"):
        with pytest.raises(GamdError, match="-22.*" + field):
            eng.water_classical_configure(4, **{**dict(alpha=0.45, k_cut=3.9), field: 0.0})
    eng.water_classical_configure(4, r_cut=half * 1.001, ewald_tol=DELTA)   # the box of a run is known at the run
    with pytest.raises(GamdError, match="-22.*r_cut"):
        case.run(eng, x, v, f, 4)
    assert torch.equal(x, x0)                                               # nothing was enqueued
    with pytest.raises(GamdError, match="-22.*r_cut"):
        eng.water_classical_forces(x, case.species)
    eng.water_classical_configure(4, ewald_tol=DELTA)
    with pytest.raises(GamdError, match="-22.*r_cut"):                      # a smaller box than the constructor's
        eng.md_run(x, v, f, 4, box=0.9 * case.box, **case.md)
    with pytest.raises(GamdError, match="-22.*r_cut"):
        eng.water_classical_forces(x, case.species, box=0.9 * case.box)
    with pytest.raises(GamdError, match="-22.*k_cut"):                      # a box whose list would be too long: known at the call
        eng.water_classical_forces(x, case.species, box=40.0 * case.box)
    with pytest.raises(GamdError, match="-22.*species"):
        eng.md_run(x, v, f, 4, **{**case.md, "species": None, "rigid_water": False})
    with pytest.raises(GamdError, match="-22.*species"):
        eng.water_classical_forces(x, None)
    assert torch.equal(x, x0)
    with pytest.raises(GamdError, match="-22.*alpha"):
        eng.water_classical_configure(4, alpha=-1.0)
    # the configuration that was accepted last is still in force
    case.run(eng, x, v, f, 4, sync=False)
    with pytest.raises(GamdError, match="-22.*enqueued"):                   # a run is pending
        eng.water_classical_configure(4, r_switch=8.0)
    with pytest.raises(GamdError, match="-22.*enqueued"):
        eng.water_classical_reset()
    with pytest.raises(GamdError, match="-22.*enqueued"):
        eng.water_classical_forces(x0, case.species)
    assert eng.sync_status() == 0
    rd = eng.water_classical_read()
    assert np.array_equal(rd.steps, [4]) and rd.energy.shape == (1, 1)
    fcl = eng.water_classical_forces(x, case.species)[0].cpu().numpy()
    _check_box("after the refusals", _rows(rd)[0], x.cpu().numpy(), case.box, case.species, wr.Water(ewald_tol=DELTA), 0.0, fcl, f.cpu().numpy())
    eng.close()


# ---- 8: checked build ------------------------------------------------------------------------------------------------
CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_water_classical as t
from gamd_amd import _lib
(x, v, f), rd, rep = t._sampled_run(t._Water(skin=0.7), 2)
rows = np.stack([getattr(rd, name) for name in rd.COLUMNS], axis=-1)
print("RESULT", json.dumps(dict(version=_lib.load().gamd_version().decode(), steps=rd.steps.tolist(), dropped=rd.dropped,
                                rows=t._bits(rows).tolist(), forces=t._bits(rd.forces).tolist())))
"""


def test_checked_build_gives_the_same_rows_and_forces():
    """a sampled skin-mode run under libgamd_hip_chk.so in a child process: a failed device-side range check of any kernel of
    the run would come back as -35; the water kernels index with nothing they read from memory and give the same bits."""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    env = {k: v for k, v in os.environ.items() if k not in ("GAMD_LIB", "GAMD_CHK_INJECT")}
    env["GAMD_LIB"] = CHK
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert p.returncode == 0 and "RESULT" in p.stdout, (p.stdout[-800:], p.stderr[-1500:])
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got["version"].endswith("checked")
    _, rd, _ = _sampled_run(_Water(skin=0.7), 2)
    rows = np.stack([getattr(rd, name) for name in rd.COLUMNS], axis=-1)
    assert got["steps"] == rd.steps.tolist() == [4, 8] and got["dropped"] == 0
    assert got["rows"] == _bits(rows).tolist() and got["forces"] == _bits(rd.forces).tolist()
    assert (rd.pairs > 0).all()


def test_print_the_largest_observed_fractions_of_the_bounds():
    """(runs last in the file: the figures profiles/run_water_classical.md records)"""
    print("largest |dev - ref| / bound over the file: " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
