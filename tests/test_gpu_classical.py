"""The classical observer on the device: the switched, shifted Lennard-Jones potential evaluated in double on all pairs, on
given positions (classical_forces) and inside enqueued md_run / md_run_nhc calls, against the float64 host reference of
tests/classical_ref.py on the frames of an observer-off run of the same trajectory cut into chunks.

Tolerances (derived, not measured).  The device and the reference evaluate a pair term with the same operations in the same
order, about 20 roundings each; they differ in the order of the sums.  A sequential double sum over
N <= 1500 terms adds at most N eps = 1.7e-13 of the sum of the absolute terms (a tree adds less), so 1e-12 of the host-computed
sum of absolute terms leaves about five times that — the S(k) test's argument (tests/test_gpu_structure.py):
    |E - E_ref| <= 1e-12 sum_{i<j} |u|,   |W - W_ref| <= 1e-12 sum_{i<j} |r u'|,
    |f_cl - F_ref| <= 1e-12 sum_j |F_ij| per atom and component,
    each of the five force-error sums within 1e-12 of the sum of its own absolute terms, recomputed on the host from the
    DEVICE's f_cl (the same kernels on the frame, bit-equal to the sample's f_cl where that can be read) and the run's f.
Pair counts are exact: a pair's side of the cutoff is only open when |r - r_cut| <= 1e-12 r_cut, and every frame is asserted to
hold no such pair.  Nothing here claims parity with OpenMM: the default parameters are unverified (see classical_configure).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import classical_ref as cr
from gamd_amd import workloads as wl
from gamd_amd.weights import ModelConfig, make_state_dict, SHIPPED_SCALERS
from helpers import load_golden
from test_gpu_report import _Case, _state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHK = os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")
CHUNKS = 4
TOL = 1e-12


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _engine(n, box, n_boxes=1, cutoff=7.5):
    from gamd_amd.engine import GamdForce
    sd = make_state_dict(ModelConfig(kind="lj", conv_layer=2), 2, 5.0, 1.7)
    return GamdForce(sd, n, box, cutoff, scaler=SHIPPED_SCALERS["lj"], n_boxes=n_boxes)


def _check_box(tag, row, x_box, box, lj, length_per_nm, fcl_dev, f_run=None):
    """one box of one frame: row [9] from the device (E, W, pairs, five sums, excluded), fcl_dev [n, 3] the device's forces"""
    ref = cr.evaluate(x_box, box, lj, length_per_nm)
    e_err, w_err = abs(row[0] - ref["energy"]), abs(row[1] - ref["virial"])
    f_ratio = (np.abs(fcl_dev - ref["forces"]) / (TOL * ref["abs_f"][:, None])).max()
    print(f"{tag}: pairs {row[2]:.0f} (ref {ref['pairs']:.0f}, {ref['near']} at the cutoff), E {row[0]:.9e} |dE| / bound "
          f"{e_err / (TOL * ref['abs_u']):.3e}, W {row[1]:.9e} |dW| / bound {w_err / (TOL * ref['abs_ru']):.3e}, max |df| / bound {f_ratio:.3e}")
    assert ref["near"] == 0, "ill-posed: a pair sits on the cutoff"
    assert ref["pairs"] > 0 and row[2] == ref["pairs"]
    assert e_err <= TOL * ref["abs_u"] and w_err <= TOL * ref["abs_ru"]
    assert f_ratio <= 1.0 and np.isfinite(fcl_dev).all()
    if f_run is not None:
        sums, ab = cr.force_error_sums(f_run, fcl_dev)
        ratio = np.abs(row[3:8] - sums[:5]) / (TOL * ab)
        print(f"{tag}: force-error sums {row[3:8]}, |dev - host| / bound {ratio}, left out of the cosine {row[8]:.0f}")
        assert (ab > 0).all() and (ratio <= 1.0).all() and row[8] == sums[5]
    return ref


# ---- 1: given positions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,scale,kw", [
    (300, (1.0, 1.0, 1.0), dict()),                                       # one full tile plus 44
    (300, (1.0, 1.0, 1.0), dict(shift=False)),
    (300, (1.0, 1.0, 1.0), dict(r_switch=0.0)),
    (300, (1.0, 1.0, 1.0), dict(shift=False, r_switch=0.0)),
    (64, (1.0, 1.0, 1.0), dict(r_cut=8.5, r_switch=5.1)),                 # below one tile; box 17.1 A
    (1500, (1.0, 0.9, 1.15), dict()),                                     # six tiles, 32 slices of 47 atoms, three different edges
])
def test_classical_forces_on_given_positions(n, scale, kw):
    pos, L = wl.lj_box(n, seed=4)
    s = np.asarray(scale)
    x = (pos * s[None, :]).astype(np.float32)
    box = (np.float32(L) * s.astype(np.float32)).astype(np.float32)
    lj = cr.LJ(**kw)
    assert 2 * lj.r_cut <= box.min()
    eng = _engine(n, box, cutoff=5.0 if n == 64 else 7.5)
    eng.classical_configure(0, **lj.kwargs())
    f, e, w, c = eng.classical_forces(x, box=box)
    assert f.dtype == torch.float64 and tuple(f.shape) == (n, 3) and e.shape == w.shape == c.shape == (1,)
    _check_box(f"n={n} {kw}", np.array([e[0], w[0], c[0]]), x, box, lj, 0.0, f.cpu().numpy())
    # the log is untouched by an evaluation outside a run
    rd = eng.classical_read(forces=True)
    assert rd.steps.shape == (0,) and np.array_equal(_bits(rd.forces), _bits(f.cpu().numpy()))
    eng.close()


def test_two_boxes_with_different_positions_in_bohr():
    n = 300
    pos, L = wl.lj_box(n, seed=4)
    rng = np.random.default_rng(8)
    x = np.concatenate([pos, np.mod(pos + rng.normal(0, 0.4, pos.shape), L)]).astype(np.float32)
    boxes = np.array([[L, L, L], [L, 1.05 * L, 0.97 * L]], dtype=np.float32)
    lj = cr.LJ()
    eng = _engine(n, float(L), n_boxes=2)
    eng.classical_configure(0, **lj.kwargs())
    f, e, w, c = eng.classical_forces(x, box=boxes, length_per_nm=wl.BOHR_PER_NM)
    fh = f.cpu().numpy()
    for b in range(2):
        _check_box(f"box {b}", np.array([e[b], w[b], c[b]]), x[b * n:(b + 1) * n], boxes[b], lj, wl.BOHR_PER_NM, fh[b * n:(b + 1) * n])
    assert e[0] != e[1] and c[0] != c[1]
    # the boxes are independent: box 1 alone, in Angstrom, gives the same energy bits and forces that differ by the unit alone
    one = _engine(n, boxes[1])
    one.classical_configure(0, **lj.kwargs())
    f1, e1, w1, c1 = one.classical_forces(x[n:], box=boxes[1])
    assert _bits(e1)[0] == _bits(e)[1] and _bits(w1)[0] == _bits(w)[1] and c1[0] == c[1]
    assert np.allclose(f1.cpu().numpy() * (float(np.float32(wl.BOHR_PER_NM)) / 10.0), fh[n:], rtol=1e-15, atol=0)
    one.close()
    eng.close()


def test_whole_box_shifts_and_a_second_call_give_the_same_bits():
    """Positions and box edges on a grid of 2^-10 A (edges 28.5, 27.25, 30.0): x + k L is exact in fp32, d and L rint(d / L)
    stay on the grid in double, so every image of a configuration has the same minimum-image vectors bit for bit."""
    n, q = 300, 2.0 ** -10
    pos, L = wl.lj_box(n, seed=4)
    box = np.array([28.5, 27.25, 30.0], dtype=np.float32)
    x = (np.rint(pos * (box.astype(np.float64) / L)[None, :] / q) * q).astype(np.float32)
    k = np.random.default_rng(3).integers(-2, 3, size=(n, 3))
    xs = (x.astype(np.float64) + k * box.astype(np.float64)[None, :]).astype(np.float32)
    assert np.array_equal(xs.astype(np.float64), x.astype(np.float64) + k * box.astype(np.float64)[None, :]) and (k != 0).any()
    eng = _engine(n, box)
    eng.classical_configure(0)
    a = eng.classical_forces(x, box=box)
    b = eng.classical_forces(xs, box=box)
    c = eng.classical_forces(x, box=box)
    for other in (b, c):
        assert np.array_equal(_bits(a[0].cpu().numpy()), _bits(other[0].cpu().numpy()))
        for u, v in zip(a[1:], other[1:]):
            assert np.array_equal(_bits(u), _bits(v))
    assert a[3][0] > 0 and np.abs(a[0].cpu().numpy()).max() > 0
    eng.close()


# ---- 2, 3: inside runs -----------------------------------------------------------------------------------------------
def _reference_frames(case, chunks):
    """observer-off run cut into `chunks` calls of K steps: final state, (x, f) at every cut, and afterwards the device's
    classical forces on every frame (gamd_classical_eval: the sample's kernels on given positions)"""
    eng, x, v, f = case.make()
    chain, frames = None, []
    for c in range(chunks):
        chain = case.run(eng, x, v, f, case.K, first_step=c * case.K, chain=chain)
        xs, _, fs = _state(x, v, f)
        frames.append((xs, fs))
    out = _state(x, v, f)
    eng.classical_configure(0)
    fcl = [eng.classical_forces(xs, box=case.box, length_per_nm=case.len)[0].cpu().numpy() for xs, _ in frames]
    eng.close()
    return out, frames, fcl


def _sampled_run(case, chunks, **kw):
    eng, x, v, f = case.make()
    eng.classical_configure(case.K, **kw)
    eng.report_configure(case.K)
    case.run(eng, x, v, f, chunks * case.K)
    rd, rep = eng.classical_read(forces=True), eng.report_read()
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
    assert rd.energy.shape == (chunks, case.nb)
    lj, n = cr.LJ(), case.n
    for q, (xs, fs) in enumerate(frames):
        for b in range(case.nb):
            sl = slice(b * n, (b + 1) * n)
            row = np.array([getattr(rd, name)[q, b] for name in rd.COLUMNS])
            _check_box(f"{case.kind} {case.integrator} frame {q} box {b}", row, xs[sl], case.box, lj, case.len, fcl[q][sl], fs[sl])
    # 3. the last sample's forces are the ones the evaluation outside the run gives for that frame
    assert np.array_equal(_bits(rd.forces), _bits(fcl[-1]))
    if case.nb > 1:
        assert not np.array_equal(rd.energy[:, 0], rd.energy[:, 1])          # the boxes carry different velocities
    fe = rd.force_errors(unit=0.0010364)
    assert all(fe[k].shape == (chunks, case.nb) and np.isfinite(fe[k]).all() for k in ("mae", "rmse", "cosine", "relative_mae"))
    assert (np.abs(fe["cosine"]) <= 1.0).all() and (fe["rmse"] >= fe["mae"]).all()
    return rd, rep


@pytest.mark.parametrize("integrator", ["baoab", "nhc"])
def test_lj258_rows_are_the_reference_on_the_frames_of_an_observer_off_run(integrator):
    rd, rep = _check_against_chunks(_Case("lj", integrator))
    # total energy and pressure from the two observers' rows
    p = rd.pressure(rep.ke, float(np.float32(27.27)) ** 3 * 1e-3)
    assert p.shape == (CHUNKS, 1) and np.isfinite(p).all()


def test_two_boxes_in_bohr_keep_their_own_rows():
    _check_against_chunks(_Case("lj", n_boxes=2, length_per_nm=wl.BOHR_PER_NM), chunks=3)


@pytest.mark.parametrize("kind,chunks", [("lj", CHUNKS), ("lj1500", 2)])
def test_skin_mode_completes_the_second_half_before_the_sample(kind, chunks):
    """Verlet-skin reuse: the B of a step rides in the next step's first neighbour kernel; on sampled steps it is launched on its
    own.  258 atoms take the single-workgroup neighbour path, 1500 the grid-wide one (six row tiles, 32 slices)."""
    _check_against_chunks(_Case(kind, skin=1.25), chunks=chunks)


# ---- 4: overflow in the middle of a run ------------------------------------------------------------------------------
def test_overflow_in_the_middle_of_a_run_writes_every_row_once_with_the_bits_of_an_ample_buffer():
    """The scheme of test_overflow_in_the_middle_of_a_run_counts_no_sample_twice (tests/test_gpu_report.py), exact mode: five
    contracting boxes, a capacity that holds the first edge list but not a later one.  The samples in front of the freeze
    completed; the frozen step's sample and the later ones are enqueued again by the resumed run and write their own rows."""
    from gamd_amd.engine import GamdForce
    g, _, _ = load_golden("lj258_seed0")
    nb, n, box, rc = 5, 258, float(g["box"]), float(g["cutoff"])
    sd = make_state_dict(ModelConfig(kind="lj"), 0, 5.3, 1.6)
    kw = dict(n_boxes=nb, scaler=SHIPPED_SCALERS["lj"])
    base, rng = np.mod(g["pos"], box), np.random.default_rng(2)
    pos = np.concatenate([base + (rng.normal(0, 0.3, base.shape) if b else 0.0) for b in range(nb)])
    x0 = torch.from_numpy(pos).float().cuda()
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
        eng.classical_configure(3)
        eng.md_run(x, v, f, 30, temperature_k=0.0, gamma_per_ps=0.0, seed=1)
        assert eng.last_status == (1 if cap else 0), "the run was meant to outgrow its edge buffer"
        res.append((eng.classical_read(forces=True), x.cpu().numpy()))
        eng.close()
    (a, xa), (b, xb) = res
    assert np.array_equal(xa, xb)
    assert np.array_equal(a.steps, 3 * np.arange(1, 11)) and np.array_equal(b.steps, a.steps) and a.dropped == b.dropped == 0
    for name in a.COLUMNS:
        assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    assert np.array_equal(_bits(a.forces), _bits(b.forces))
    assert (a.pairs > 0).all() and np.isfinite(a.energy).all()


# ---- 5: accumulation, reset, a full log, interval 0 ------------------------------------------------------------------
def test_accumulation_across_calls_reset_a_full_log_and_interval_zero():
    case = _Case("lj", K=3)
    n = 9
    eng, x, v, f = case.make()
    eng.classical_configure(case.K)
    case.run(eng, x, v, f, 2 * n)
    one = eng.classical_read()
    eng.close()
    eng, x, v, f = case.make()
    eng.classical_configure(case.K, max_samples=4)
    case.run(eng, x, v, f, n - 1)                      # g runs across calls: 8 + 10 steps sample at 3, 6 | 9, 12, 15, 18
    case.run(eng, x, v, f, n + 1, first_step=n - 1)
    two = eng.classical_read()
    assert np.array_equal(one.steps, 3 * np.arange(1, 7)) and one.dropped == 0
    assert two.dropped == 2 and np.array_equal(two.steps, one.steps[:4])
    for name in one.COLUMNS:
        assert np.array_equal(_bits(getattr(two, name)), _bits(getattr(one, name)[:4])), name
    eng.classical_reset()
    z = eng.classical_read()
    assert z.steps.shape == (0,) and z.dropped == 0 and z.energy.shape == (0, 1)
    # after the reset the count starts again: K more steps give one row, the row of the positions the run ends at
    case.run(eng, x, v, f, case.K, first_step=2 * n)
    again = eng.classical_read(forces=True)
    assert np.array_equal(again.steps, [case.K])
    row = np.array([getattr(again, name)[0, 0] for name in again.COLUMNS])
    _check_box("after reset", row, x.cpu().numpy(), case.box, cr.LJ(), 0.0, again.forces, f.cpu().numpy())
    # interval 0: off, what was logged stays readable, further steps add nothing; the parameters it carries are taken
    eng.classical_configure(0, r_switch=0.0)
    case.run(eng, x, v, f, case.K, first_step=2 * n + case.K)
    off = eng.classical_read()
    assert np.array_equal(off.steps, again.steps) and np.array_equal(_bits(off.energy), _bits(again.energy))
    fo, eo, wo, co = eng.classical_forces(x)
    _check_box("interval 0, unswitched", np.array([eo[0], wo[0], co[0]]), x.cpu().numpy(), case.box, cr.LJ(r_switch=0.0), 0.0, fo.cpu().numpy())
    eng.close()


# ---- 6: refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    from gamd_amd._lib import GamdError
    water = _Case("water")
    eng, x, v, f = water.make()
    with pytest.raises(GamdError, match="-22.*GAMD_KIND_WATER"):
        eng.classical_configure(4, r_cut=4.0, r_switch=3.0)
    with pytest.raises(GamdError, match="-22.*GAMD_KIND_WATER"):
        eng.classical_forces(x)
    eng.close()
    case = _Case("lj")
    half = float(np.float32(0.5) * np.float32(case.box))
    eng, x, v, f = case.make()
    x0 = x.clone()
    eng.classical_configure(4, r_cut=half * 1.001)                          # the box of a run is known at the run
    with pytest.raises(GamdError, match="-22.*r_cut"):
        case.run(eng, x, v, f, 4)
    assert torch.equal(x, x0)                                               # nothing was enqueued
    with pytest.raises(GamdError, match="-22.*r_cut"):
        eng.classical_forces(x)
    eng.classical_configure(4)
    with pytest.raises(GamdError, match="-22.*r_cut"):                      # a smaller box than the constructor's
        eng.md_run(x, v, f, 4, box=0.74 * case.box, **case.md)
    with pytest.raises(GamdError, match="-22.*r_cut"):
        eng.classical_forces(x, box=0.74 * case.box)
    assert torch.equal(x, x0)
    with pytest.raises(GamdError, match="-22.*sigma"):
        eng.classical_configure(4, sigma=0.0)
    # the configuration that was accepted last is still in force
    case.run(eng, x, v, f, 4, sync=False)
    with pytest.raises(GamdError, match="-22.*enqueued"):                   # a run is pending
        eng.classical_configure(4, r_switch=0.0)
    with pytest.raises(GamdError, match="-22.*enqueued"):
        eng.classical_reset()
    with pytest.raises(GamdError, match="-22.*enqueued"):
        eng.classical_forces(x0)
    assert eng.sync_status() == 0
    rd = eng.classical_read()
    assert np.array_equal(rd.steps, [4]) and rd.energy.shape == (1, 1)
    row = np.array([getattr(rd, name)[0, 0] for name in rd.COLUMNS])
    fcl = eng.classical_forces(x)[0].cpu().numpy()
    _check_box("after the refusals", row, x.cpu().numpy(), case.box, cr.LJ(), 0.0, fcl, f.cpu().numpy())   # switched: the refused block was not taken
    eng.close()


# ---- 7: checked build ------------------------------------------------------------------------------------------------
CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_classical as t
from gamd_amd import _lib
case = t._Case("lj", skin=1.25)
(x, v, f), rd, rep = t._sampled_run(case, t.CHUNKS)
rows = np.stack([getattr(rd, name) for name in rd.COLUMNS], axis=-1)
print("RESULT", json.dumps(dict(version=_lib.load().gamd_version().decode(), steps=rd.steps.tolist(), dropped=rd.dropped,
                                rows=t._bits(rows).tolist(), forces=t._bits(rd.forces).tolist())))
"""


def test_checked_build_gives_the_same_rows_and_forces():
    """a sampled skin-mode run under libgamd_hip_chk.so in a child process: a failed device-side range check of any kernel of
    the run would come back as -35; the classical kernels index with nothing they read from memory and give the same bits."""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    env = {k: v for k, v in os.environ.items() if k not in ("GAMD_LIB", "GAMD_CHK_INJECT")}
    env["GAMD_LIB"] = CHK
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert p.returncode == 0 and "RESULT" in p.stdout, (p.stdout[-800:], p.stderr[-1500:])
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got["version"].endswith("checked")
    _, rd, _ = _sampled_run(_Case("lj", skin=1.25), CHUNKS)
    rows = np.stack([getattr(rd, name) for name in rd.COLUMNS], axis=-1)
    assert got["steps"] == rd.steps.tolist() == [4 * (q + 1) for q in range(CHUNKS)] and got["dropped"] == 0
    assert got["rows"] == _bits(rows).tolist() and got["forces"] == _bits(rd.forces).tolist()
    assert (rd.pairs > 0).all()
