"""The Lennard-Jones classical potential over a cell table (gamd_classical_cells) inside enqueued runs and in the minimiser.
Given positions, tables and bounds: tests/test_gpu_classical_cells.py.

What is asserted (cells on; every comparison is of bits unless a bar is named)
* Driven frames: every recorded frame of a classical-source run, and the final buffer, carry classical_forces(x)[0].float().
* The same trajectory from one call, two calls, a fresh handle, and with all observers armed; an armed observer's rows carry the
  bits classical_forces gives on the frame.
* Sampled frames of a NETWORK-driven run: every row of the armed observer against tests/classical_ref.py on the frame — E, W and
  the forces within the bounds of tests/test_gpu_classical_cells.py, the pair count exact, and the five force-error sums of the
  run's (network) forces against f_cl within 1e-12 of the sums of their absolute terms, with the left-out count, recomputed on
  the host from the device's f_cl (tests/test_gpu_classical.py's scheme for the all-pairs path); one and two boxes.
* A neighbour-buffer overflow in the middle of a driven, sampled run (the documented freeze / regrow path, the scheme of
  tests/test_gpu_classical_drive.py) gives the bits of an ample buffer.
* The checked library gives the same bits (a failed range check of a k_ljcell_* kernel would come back as -35).
* The minimiser: f is classical_forces(x)[0].float() at the returned x; the same bits from a second call, a fresh handle and
  check_every = 1, 64, 1000; the lj258_seed0 start reaches tolerance 10 in the iteration count of the float64 replay
  (tests/minimize_ref.py); after 64 iterations the positions lie within the bar tests/test_gpu_minimize.py applies to the
  all-pairs minimiser against that replay — 100 times the replay's own spread under three atom permutations, floor 1e-13 A,
  taken from that file's replay64 fixture and by its expression: the cell walk is one more summation order.

Runs are at 300 atoms (wl.lj_box(300, seed=4), cells per axis (5, 5, 5): every z window wraps or fills the axis); the overflow
scheme and the replay are the existing ones at 258."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import classical_ref as cr
import minimize_ref as mr
from gamd_amd import workloads as wl
from gamd_amd.weights import ModelConfig, make_state_dict
from test_gpu_report import _Case, _state
from test_gpu_classical_cells import _check_box
from test_gpu_classical_drive import _assert_frames_carry_the_classical_force, _i32, _i64, _seeded_engine, SKIN
from test_gpu_minimize import _assert_f_contract, _bits, _golden_start, _minimize, replay64, TOL  # noqa: F401 (replay64: a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHK = os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")


class _Lj300(_Case):
    """300 atoms of wl.lj_box(300, seed=4) with _Case's velocities and integrator settings.  _Case has no constructor for another
    size: this takes its "lj1500" branch (the seeded two-layer model, cutoff 7.5, md, eng_kw, species None) and sets again EVERY
    field that branch derives from the atom count or the positions — n, sd, pos, box, mass, v0, ndf.  A field _Case derives from
    them in future belongs here too; the assertions below fail if the list falls behind the ones make() and run() read."""

    def __init__(self, integrator="baoab", **kw):
        super().__init__("lj1500", integrator, **kw)
        self.n = 300
        self.sd = make_state_dict(ModelConfig(kind="lj", conv_layer=2), 2, 5.0, 1.7)
        self.pos, self.box = wl.lj_box(self.n, seed=4)
        self.mass = self.mass[:self.n * self.nb]
        self.v0 = np.concatenate([wl.maxwell_boltzmann(self.n, 100.0, seed=90 + b) for b in range(self.nb)])
        self.ndf = 3 * self.n
        assert 2 * cr.LJ().r_cut <= np.float32(self.box)
        assert self.pos.shape == (self.n, 3) and self.v0.shape == (self.n * self.nb, 3) and self.mass.shape == (self.n * self.nb,)
        assert self.species is None and self.rc == 7.5 and self.n_pairs == 1


def _make(case, cells=True):
    eng, x, v, f = case.make()
    eng.classical_configure(0, cells=cells)
    eng.md_force_source("classical")
    f = eng.classical_forces(x, length_per_nm=case.len)[0].float().contiguous()
    return eng, x, v, f


# ---- driven frames, chunks, observers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator,skin", [("baoab", SKIN), ("nhc", 0.0)])
def test_every_frame_of_a_driven_run_carries_the_classical_force_of_its_positions(integrator, skin):
    case = _Lj300(integrator, skin=skin)
    eng, x, v, f = _make(case)
    steps = 10
    eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
    case.run(eng, x, v, f, steps)
    assert eng.last_status == 0
    _assert_frames_carry_the_classical_force(eng, eng.traj_read(), x, f, steps)
    assert tuple(eng.classical_cells_table()[0]) == (5, 5, 5)
    eng.close()


def _driven(case, calls, observers=False):
    eng, x, v, f = _make(case)
    if observers:
        eng.report_configure(3, rdf_bins=32)
        eng.traj_configure(3, max_frames=8, fields=("x", "v", "f", "image"), n_lags=3)
        eng.structure_configure(3, rdf_bins=32, sk_n2max=4)
        eng.classical_configure(3, cells=True)
    chain = None
    for c, k in enumerate(calls):
        chain = case.run(eng, x, v, f, k, first_step=sum(calls[:c]), chain=chain)
        assert eng.last_status == 0
    out = _state(x, v, f)
    rows = None
    if observers:
        rd, tr = eng.classical_read(forces=True), eng.traj_read()
        rows = rd.steps
        for q, g in enumerate(rd.steps):                    # the rows are the eval call's on the frame
            fcl, e, w, c = eng.classical_forces(tr.x[q].reshape(-1, 3))
            assert tr.steps[q] == g and _i64(rd.energy[q])[0] == _i64(e)[0] and _i64(rd.virial[q])[0] == _i64(w)[0] and rd.pairs[q, 0] == c[0] > 0
        assert np.array_equal(_i64(rd.forces), _i64(eng.classical_forces(tr.x[len(rows) - 1].reshape(-1, 3))[0].cpu().numpy()))
    eng.close()
    return out, rows


@pytest.mark.parametrize("integrator,skin", [("baoab", 0.0), ("nhc", SKIN)])
def test_chunked_runs_fresh_handles_and_armed_observers_give_the_same_bits(integrator, skin):
    K = 6
    case = _Lj300(integrator, skin=skin, K=K)
    one, _ = _driven(case, [2 * K])
    two, _ = _driven(case, [K, K])
    again, _ = _driven(case, [2 * K])
    armed, rows = _driven(case, [2 * K], observers=True)
    assert np.array_equal(rows, 3 * np.arange(1, 5))
    for name, other in (("two calls", two), ("second handle", again), ("observers armed", armed)):
        for a, b in zip(one, other):
            assert np.array_equal(_i32(a), _i32(b)), name
    assert not np.array_equal(one[0], np.mod(case.pos, case.box).astype(np.float32))


# ---- sampled frames of a network-driven run: the whole row against the reference --------------------------------------
@pytest.mark.parametrize("integrator,skin,nb,unit", [("baoab", SKIN, 1, 0.0), ("nhc", 0.0, 2, wl.BOHR_PER_NM)])
def test_rows_of_a_network_driven_run_are_the_reference_on_the_frames_with_the_five_force_error_sums(integrator, skin, nb, unit):
    case = _Lj300(integrator, skin=skin, n_boxes=nb, length_per_nm=unit)
    eng, x, v, f = case.make()
    K, samples = case.K, 3
    eng.classical_configure(K, cells=True)
    eng.traj_configure(K, max_frames=samples, fields=("x", "f"))
    case.run(eng, x, v, f, samples * K)
    assert eng.last_status == 0 and eng.force_source == "network"
    rd, tr = eng.classical_read(forces=True), eng.traj_read()
    assert rd.dropped == 0 and np.array_equal(rd.steps, K * np.arange(1, samples + 1)) and np.array_equal(tr.steps, rd.steps)
    lj, n = cr.LJ(), case.n
    for q in range(samples):
        xs, fs = tr.x[q].reshape(-1, 3), tr.f[q].reshape(-1, 3)
        fcl = eng.classical_forces(xs, length_per_nm=unit)[0].cpu().numpy()     # the sample's kernels on the frame
        for b in range(nb):
            sl = slice(b * n, (b + 1) * n)
            row = np.array([getattr(rd, name)[q, b] for name in rd.COLUMNS])
            _check_box(f"cells {integrator} frame {q} box {b}", row, xs[sl], case.box, lj, unit, fcl[sl], fs[sl])
    assert np.array_equal(_i64(rd.forces), _i64(fcl))       # the last sample's f_cl is the eval call's on that frame
    assert np.array_equal(xs, x.cpu().numpy()) and np.array_equal(_i32(fs), _i32(f.cpu().numpy()))
    eng.close()


# ---- overflow in the middle of a run -----------------------------------------------------------------------------------
def test_overflow_in_the_middle_of_a_driven_sampled_run_gives_the_bits_of_an_ample_buffer():
    """test_overflow_in_the_middle_of_a_driven_run_gives_the_bits_of_an_ample_buffer (tests/test_gpu_classical_drive.py) with
    the cells on and the observer armed: five contracting boxes, a capacity that holds the first edge list but not a later
    one.  The run freezes on the device (every k_ljcell_* kernel returns while the flag is set), gamd_sync_status regrows the
    buffer and enqueues the rest, the frozen step's table is built again."""
    nb, n, rc, steps = 5, 258, 7.5, 30
    base, box = wl.lj_box(n)
    kw = dict(n_boxes=nb)
    rng = np.random.default_rng(2)
    pos = np.concatenate([base + (rng.normal(0, 0.3, base.shape) if b else 0.0) for b in range(nb)])
    x0 = torch.from_numpy(pos).float().cuda()
    v0 = (-(torch.remainder(x0, box) - box / 2)).contiguous() * 1.5
    probe = _seeded_engine(n, box, cutoff=rc, **kw)
    probe.forward(x0)
    e_now = probe.counts()[0]
    probe.close()
    res = []
    for cap in (0, e_now + 40):
        eng = _seeded_engine(n, box, cutoff=rc, edge_capacity=cap, **kw)
        x, v = x0.clone(), v0.clone()
        eng.forward(x)
        assert eng.last_status == 0
        eng.classical_configure(3, cells=True)
        eng.md_force_source("classical")
        f = eng.classical_forces(x)[0].float().contiguous()
        eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
        eng.md_run(x, v, f, steps, temperature_k=0.0, gamma_per_ps=0.0, seed=1, sync=False)
        status = eng.sync_status()
        assert status == (1 if cap else 0), "the run was meant to outgrow its edge buffer"
        res.append((_state(x, v, f), eng.traj_read(), eng.classical_read(forces=True)))
        eng.close()
    (sa, ta, ra), (sb, tb, rb) = res
    for a, b in zip(sa, sb):
        assert np.array_equal(_i32(a), _i32(b))
    assert ta.dropped == tb.dropped == 0 and np.array_equal(ta.steps, np.arange(1, steps + 1)) and np.array_equal(tb.steps, ta.steps)
    for name in ("x", "v", "f"):
        assert np.array_equal(_i32(getattr(ta, name)), _i32(getattr(tb, name))), name
    assert np.array_equal(ra.steps, 3 * np.arange(1, 11)) and np.array_equal(rb.steps, ra.steps) and ra.dropped == rb.dropped == 0
    for name in ra.COLUMNS:
        assert np.array_equal(_i64(getattr(ra, name)), _i64(getattr(rb, name))), name
    assert np.array_equal(_i64(ra.forces), _i64(rb.forces)) and (ra.pairs > 0).all()
    assert np.isfinite(sa[2]).all() and not np.array_equal(sa[0], x0.cpu().numpy())


# ---- the minimiser -------------------------------------------------------------------------------------------------------
def _cells_engine(n, box):
    eng = _seeded_engine(n, box)
    eng.classical_configure(0, cells=True)
    return eng


def test_minimiser_f_is_the_classical_force_and_every_call_gives_the_same_bits_at_300_atoms():
    x0, box = wl.lj_box(300, seed=4)
    x0 = np.random.default_rng(4).uniform(0.0, box, x0.shape).astype(np.float32)    # test_gpu_minimize.py's random starts
    eng = _cells_engine(300, box)
    first = _minimize(eng, x0, tolerance=1e-300, max_iter=150)
    assert first[0].iterations[0] > 64 and np.isfinite(first[2]).all()
    _assert_f_contract(eng, first[1], first[2])
    assert tuple(eng.classical_cells_table()[0]) == (5, 5, 5)
    ref = _bits(*first)
    assert _bits(*_minimize(eng, x0, tolerance=1e-300, max_iter=150)) == ref, "second call"
    eng.close()
    eng = _cells_engine(300, box)
    for every in (1, 64, 1000):
        assert _bits(*_minimize(eng, x0, tolerance=1e-300, max_iter=150, check_every=every)) == ref, f"check_every = {every}"
    eng.close()


def test_lj258_seed0_converges_in_the_iteration_count_of_the_float64_replay():
    x0, box = _golden_start()
    want = mr.minimize(x0, box, cr.LJ(), TOL)
    eng = _cells_engine(258, box)
    res, x, f, x64 = _minimize(eng, x0, tolerance=TOL)
    _assert_f_contract(eng, x, f)
    eng.close()
    print(f"lj258_seed0 with cells: {res!r}; the replay: {want['iterations']} iterations, rms {want['rms']:.6f}")
    assert res.status == 0 and res.state == ["converged"] and want["state"] == mr.CONVERGED
    assert res.iterations[0] == want["iterations"] and res.rms[0] <= TOL
    assert np.array_equal(x, mr.wrap_fp32(x64, box))


def test_positions_after_64_iterations_agree_with_the_float64_replay(replay64):
    x0, box = _golden_start()
    base = replay64[0][64]
    spread_x = max(np.abs(r[64]["x"] - base["x"]).max() for r in replay64[1:])
    bar_x = max(100.0 * spread_x, 1e-13)                    # tests/test_gpu_minimize.py's bar for the all-pairs minimiser
    eng = _cells_engine(258, box)
    res, x, f, x64 = _minimize(eng, x0, tolerance=1e-300, max_iter=64)
    _assert_f_contract(eng, x, f)
    eng.close()
    dx = np.abs(x64 - base["x"]).max()
    print(f"K = 64 with cells: |dx| max {dx:.3e} A (replay's spread {spread_x:.3e}, bar {bar_x:.3e})")
    assert res.status == 1 and res.state == ["max_iter"] and res.iterations[0] == 64 == base["iterations"]
    assert dx <= bar_x


# ---- checked build ---------------------------------------------------------------------------------------------------------
def _checked_case():
    case = _Lj300("baoab", skin=SKIN)
    eng, x, v, f = _make(case)
    steps = 8
    eng.classical_configure(4, cells=True)
    eng.traj_configure(1, max_frames=steps, fields=("x", "v", "f"))
    case.run(eng, x, v, f, steps, sync=False)
    status = eng.sync_status()
    tr, rd = eng.traj_read(), eng.classical_read(forces=True)
    out = _state(x, v, f)
    x0, box = _golden_start()
    eng.close()
    eng = _cells_engine(258, box)
    mn = _bits(*_minimize(eng, x0, tolerance=1e-300, max_iter=20))
    eng.close()
    rows = np.stack([getattr(rd, name) for name in rd.COLUMNS], axis=-1)
    return dict(status=status, steps=tr.steps.tolist(), frames=[_i32(a).tolist() for a in (tr.x, tr.v, tr.f)],
                final=[_i32(a).tolist() for a in out], rows=_i64(rows).tolist(), forces=_i64(rd.forces).tolist(), minimise=mn)


CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_classical_cells_runs as t
from gamd_amd import _lib
got = t._checked_case()
got["version"] = _lib.load().gamd_version().decode()
print("RESULT", json.dumps(got))
"""


def test_checked_build_gives_the_same_bits():
    """a driven, sampled skin-mode run and 20 iterations of the minimiser under libgamd_hip_chk.so in a child process: a failed
    device-side range check (an atom's cell, a cell's start, a slot, a table entry's atom index) would come back as -35"""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    env = {k: v for k, v in os.environ.items() if k not in ("GAMD_LIB", "GAMD_CHK_INJECT")}
    env["GAMD_LIB"] = CHK
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert p.returncode == 0 and "RESULT" in p.stdout, (p.stdout[-800:], p.stderr[-1500:])
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got.pop("version").endswith("checked") and got["status"] == 0
    want = _checked_case()
    assert want["steps"] == list(range(1, 9)) and sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k] or json.loads(json.dumps(want[k])) == got[k], k
