"""The run recorder on the device: trajectory frames, periodic-image counters and MSD / VACF sums taken inside enqueued
md_run / md_run_nhc calls.

Yardsticks
* frames: a recorder-off run of the same trajectory cut into chunks of `interval` steps and read from the host after each
  chunk; everything is compared bit for bit.
* image counters: float64 nearest-image differencing of consecutive interval-1 frames on the host.
* MSD / VACF: float64 sums over the recorded frames (x, image, v) with the formula of include/gamd_hip.h.  Each term is
  the same exactly representable difference on both sides, only the summation order differs: at most 1 548 atoms and 40
  origins give (n + Q) 2^-53 < 2e-13, the bound is 1e-12 of the sum of the terms' magnitudes.

Systems: the 258-atom LJ snapshot with the lj258_seed0 weights and 258 rigid TIP3P molecules (774 atoms) with the
tip3p774_seed3 weights.  The image tests use scaler (0, 1): forces of order 1 kJ/mol/nm, so the motion is close to ballistic
and the distances travelled follow from the initial speeds (what is counted does not depend on the forces).
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
XVF = ("x", "v", "f")
ALL = ("x", "v", "f", "image")


def _f32(x):
    return float(np.float32(x))


_WATER = {}


def _water_system():
    """258 whole, rigid TIP3P molecules and constraint-free thermal velocities (computed once)"""
    if not _WATER:
        n_mol = 258
        pos, box, species, bonds = wl.water_box(n_mol, seed=5, jitter=0.0, wrap=False)
        n = 3 * n_mol
        pairs, _ = orc.water_constraints(n, wl.TIP3P_R_OH, wl.TIP3P_R_HH)
        mm = np.where(species == 1, wl.MASS_O, wl.MASS_H).astype(np.float64).reshape(-1, 1)
        v0 = np.random.default_rng(6).normal(0, 1.0, (n, 3)) * 10.0 * np.sqrt(wl.KB * 300.0 / mm)
        _WATER.update(pos=pos, box=box, species=species, bonds=bonds, n=n, n_mol=n_mol,
                      v0=orc.rattle_velocities(pos, v0, (1.0 / mm).reshape(-1), pairs))
    return _WATER


class _Case:
    """one seeded system + integrator; make() gives a fresh engine and state"""

    def __init__(self, kind, integrator="baoab", n_boxes=1, edge_dtype="f32", skin=0.0, edge_capacity=0, boxes=None,
                 v0=None, scaler=None, md=None):
        self.kind, self.integrator, self.nb = kind, integrator, n_boxes
        self.edge_dtype, self.skin, self.edge_capacity = edge_dtype, skin, edge_capacity
        if kind == "lj":
            g, _, self.sd = load_golden("lj258_seed0")
            self.box, self.rc, self.n = float(g["box"]), float(g["cutoff"]), 258
            self.pos = np.mod(g["pos"], self.box)
            self.species = None
            self.mass = np.full(self.n * n_boxes, _f32(39.9), dtype=np.float64)
            self.v0 = np.concatenate([wl.maxwell_boltzmann(self.n, 100.0, seed=90 + b) for b in range(n_boxes)])
            self.md = dict(dt_ps=0.002, mass_amu=39.9, temperature_k=100.0)
            self.eng_kw = dict(scaler=SHIPPED_SCALERS["lj"])
        else:
            _, _, self.sd = load_golden("tip3p774_seed3")
            w = _water_system()
            self.pos, self.box, self.species, self.n, self.n_mol = w["pos"], w["box"], w["species"], w["n"], w["n_mol"]
            self.rc = 4.2
            m = np.where(self.species == 1, _f32(wl.MASS_O), _f32(wl.MASS_H)).astype(np.float64)
            self.mass = np.tile(m, n_boxes)
            self.v0 = w["v0"]
            self.md = dict(dt_ps=0.0005, mass_amu=wl.MASS_O, mass_h_amu=wl.MASS_H, temperature_k=300.0, rigid_water=True,
                           r_oh=wl.TIP3P_R_OH, r_hh=wl.TIP3P_R_HH, species=self.species, remove_cm_motion=True)
            self.eng_kw = dict(bond=w["bonds"], scaler=SHIPPED_SCALERS["tip3p"])
        if v0 is not None:
            self.v0 = v0
        if scaler is not None:
            self.eng_kw["scaler"] = scaler
        if md:
            self.md.update(md)
        # edge length per box (cubic): the run's box argument; fp32 values are what the library holds
        self.boxes = np.full(n_boxes, self.box) if boxes is None else np.asarray(boxes, dtype=np.float64)
        self.gamma = 25.0

    def make(self):
        from gamd_amd.engine import GamdForce
        eng = GamdForce(self.sd, self.n, self.box, self.rc, edge_dtype=self.edge_dtype, neighbor_skin=self.skin,
                        n_boxes=self.nb, edge_capacity=self.edge_capacity, **self.eng_kw)
        x = torch.from_numpy(np.tile(self.pos, (self.nb, 1))).float().cuda()
        v = torch.from_numpy(self.v0 if self.v0.shape[0] == self.n * self.nb else np.tile(self.v0, (self.nb, 1))).float().cuda()
        f = eng.forward(x, box=self._box_arg(), species=self._species(), denormalize=True).clone()
        return eng, x, v, f

    def _species(self):
        return None if self.species is None else np.tile(self.species, self.nb)

    def _box_arg(self):
        return self.boxes.reshape(self.nb, 1) if self.nb > 1 else float(self.boxes[0])

    def run(self, eng, x, v, f, n_steps, first_step=0, chain=None, sync=True, box=None):
        md = dict(self.md)
        if md.get("species") is not None:
            md["species"] = self._species()
        md["box"] = self._box_arg() if box is None else box
        if self.integrator == "baoab":
            eng.md_run(x, v, f, n_steps, gamma_per_ps=self.gamma, seed=11, first_step=first_step, sync=sync, **md)
            return None
        return eng.md_run_nhc(x, v, f, n_steps, chain_state=chain, frequency_per_ps=25.0, sync=sync, **md)


def _state(x, v, f):
    return x.cpu().numpy().copy(), v.cpu().numpy().copy(), f.cpu().numpy().copy()


def _chunked(case, interval, chunks):
    """recorder-off run in `chunks` calls of `interval` steps, the state read from the host after each"""
    eng, x, v, f = case.make()
    frames, chain = [], None
    for c in range(chunks):
        chain = case.run(eng, x, v, f, interval, first_step=c * interval, chain=chain)
        frames.append(_state(x, v, f))
    eng.close()
    return frames


def _recorded(case, interval, n_steps, calls=1, **cfg):
    """recorder-on run of n_steps in `calls` equal calls: (RunTrajectory, final state)"""
    eng, x, v, f = case.make()
    eng.traj_configure(interval, **cfg)
    chain = None
    for c in range(calls):
        chain = case.run(eng, x, v, f, n_steps // calls, first_step=c * (n_steps // calls), chain=chain)
    tr = eng.traj_read()
    out = _state(x, v, f)
    eng.close()
    return tr, out


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_frames_against_chunks(case, interval=10, chunks=6):
    ref = _chunked(case, interval, chunks)
    tr, fin = _recorded(case, interval, interval * chunks, max_frames=chunks, fields=XVF)
    assert tr.dropped == 0 and tr.n_samples == chunks and tr.image is None
    assert np.array_equal(tr.steps, interval * np.arange(1, chunks + 1))
    shape = (chunks, case.nb, case.n, 3)
    assert tr.x.shape == tr.v.shape == tr.f.shape == shape
    for c in range(chunks):
        for got, want in zip((tr.x[c], tr.v[c], tr.f[c]), ref[c]):
            assert _same_bits(got.reshape(-1, 3), want), f"frame {c}"
    for got, want in zip(fin, ref[-1]):
        assert _same_bits(got, want)
    assert np.isfinite(tr.x).all() and np.isfinite(tr.v).all() and np.isfinite(tr.f).all()
    assert not np.array_equal(tr.x[0], tr.x[-1])
    return ref


# ---- 1: frames are the trajectory ------------------------------------------------------------------------------------
@pytest.mark.parametrize("skin_on", [False, True])
@pytest.mark.parametrize("kind,integrator", [("lj", "baoab"), ("lj", "nhc"), ("water", "baoab")])
def test_frames_are_the_trajectory(kind, integrator, skin_on):
    """One enqueued run of 60 steps with the recorder (interval 10, x | v | f) against the recorder-off run in six chunks
    of 10 steps: every frame and the final state bit for bit; a recorder that was configured and switched off again
    (interval 0) leaves the final state alone as well."""
    skin = (0.7 if kind == "water" else 1.25) if skin_on else 0.0
    case = _Case(kind, integrator, skin=skin)
    ref = _check_frames_against_chunks(case)
    eng, x, v, f = case.make()
    eng.traj_configure(10, max_frames=6, fields=XVF, n_lags=4)
    eng.traj_configure(0)
    case.run(eng, x, v, f, 60)
    tr = eng.traj_read()
    assert tr.n_samples == 0 and tr.steps.shape == (0,)
    for got, want in zip(_state(x, v, f), ref[-1]):
        assert _same_bits(got, want)
    eng.close()


# ---- 2: image counters -----------------------------------------------------------------------------------------------
def _host_images(x, L):
    """x float32 [F, B, n, 3] consecutive frames, L float64 [B] -> int64 images [F, B, n, 3] (0 in the first frame) by
    float64 nearest-image differencing"""
    xd = x.astype(np.float64)
    Lb = L[None, :, None, None]
    k = np.rint((xd[1:] - xd[:-1]) / Lb)
    img = np.zeros(x.shape, dtype=np.int64)
    img[1:] = -np.cumsum(k, axis=0).astype(np.int64)
    return img


def _fast_lj(n_boxes=1, boxes=None):
    # speeds: N(0, 14 A/ps) per component (the thermal speed of argon at 9 400 K), dt 5 fs, 300 steps = 1.5 ps: a component
    # travels 21 A rms in a 27.27 A box, and at most 0.1 ps x 4.5 sigma = 6.3 A < L / 4 = 6.8 A between two interval-20 samples
    v0 = np.concatenate([wl.maxwell_boltzmann(258, 9400.0, seed=40 + b) for b in range(n_boxes)])
    c = _Case("lj", n_boxes=n_boxes, boxes=boxes, v0=v0, scaler=(0.0, 1.0), md=dict(dt_ps=0.005, temperature_k=100.0))
    c.gamma = 0.01
    return c


def _fast_water():
    # every molecule translates as a whole (the same velocity for O, H, H satisfies the constraints): N(0, 25 A/ps) per
    # component, dt 2 fs, 300 steps = 0.6 ps: 15 A rms in a 20 A box, at most 0.04 ps x 4.5 sigma = 4.5 A < L / 4 = 5 A
    vm = np.random.default_rng(8).normal(0.0, 25.0, (258, 3))
    c = _Case("water", v0=np.repeat(vm, 3, axis=0), scaler=(0.0, 1.0), md=dict(dt_ps=0.002))
    c.gamma = 0.01
    return c


@pytest.mark.parametrize("system", ["lj", "water", "lj_two_boxes"])
def test_image_counters_follow_every_face_crossing(system):
    """300 steps recorded at interval 1 and again at interval 20 (x | image).  The device's interval-1 images equal the
    host's unwrapping of the interval-1 frames; the interval-20 images equal the interval-1 images at the same steps
    (both count from their own first sample: the interval-1 images relative to step 20); no sample is ambiguous.  Not
    vacuous: a quarter of the atoms cross a face, some atom reaches |image| >= 2, and no component moves L / 4 between two
    interval-20 samples."""
    steps = 300
    case = {"lj": _fast_lj, "water": _fast_water, "lj_two_boxes": lambda: _fast_lj(2, [27.27, 31.5])}[system]()
    L = np.array([_f32(b) for b in case.boxes], dtype=np.float64)
    one, fin1 = _recorded(case, 1, steps, max_frames=steps, fields=("x", "image"))
    coarse, fin20 = _recorded(case, 20, steps, max_frames=steps // 20, fields=("x", "image"))
    assert one.x.shape == (steps, case.nb, case.n, 3) and coarse.x.shape == (steps // 20, case.nb, case.n, 3)
    assert np.isfinite(one.x).all()
    for a, b in zip(fin1, fin20):
        assert _same_bits(a, b)
    host = _host_images(one.x, L)
    u = one.x.astype(np.float64) + host * L[None, :, None, None]
    crossed = (host != 0).any(axis=(0, 3))                                   # [B, n]
    at20 = u[19::20]
    far = np.abs(at20[1:] - at20[:-1]).max(axis=(0, 2, 3)) / L
    print(f"{system}: {crossed.mean():.2f} of the atoms cross a face, max |image| {np.abs(host).max()}, largest component "
          f"displacement between interval-20 samples {far.max():.3f} L, ambiguous {one.ambiguous} / {coarse.ambiguous}")
    assert crossed.mean(axis=1).min() >= 0.25 and np.abs(host).max() >= 2 and far.max() < 0.25
    assert np.array_equal(one.image, host)
    assert np.array_equal(one.steps, np.arange(1, steps + 1)) and np.array_equal(coarse.steps, 20 * np.arange(1, steps // 20 + 1))
    assert _same_bits(coarse.x, one.x[19::20])
    assert np.array_equal(coarse.image, one.image[19::20] - one.image[19])
    assert one.ambiguous == 0 and coarse.ambiguous == 0
    # the unwrapped trajectory is continuous: no component jumps by more than L / 4 from one step to the next
    assert np.abs(np.diff(one.unwrapped(case.boxes.reshape(-1, 1)), axis=0)).max() < 0.25 * L.min()
    if system == "water":                                                    # molecules stay whole
        im = one.image.reshape(steps, case.n_mol, 3, 3)
        assert (im[:, :, 1:] == im[:, :, :1]).all()
        uu = one.unwrapped(case.box).reshape(steps, case.n_mol, 3, 3)
        d_oh = np.linalg.norm(uu[:, :, 1] - uu[:, :, 0], axis=-1)
        assert np.abs(d_oh - wl.TIP3P_R_OH).max() < 1e-3


# ---- 3: ambiguity is reported ----------------------------------------------------------------------------------------
def test_a_jump_of_0p4_box_edges_is_counted_as_ambiguous():
    case = _Case("lj")
    eng, x, v, f = case.make()
    eng.traj_configure(5, max_frames=4, fields=("x", "image"))
    case.run(eng, x, v, f, 10)
    assert eng.traj_read().ambiguous == 0
    x[:, 0] += 0.4 * case.box
    f.copy_(eng.forward(x, denormalize=True))
    case.run(eng, x, v, f, 10, first_step=10)
    tr = eng.traj_read()
    assert tr.n_samples == 4 and tr.ambiguous >= case.n
    eng.close()


# ---- 4: MSD / VACF against float64 -----------------------------------------------------------------------------------
def _host_sums(tr, L, mass, species, n_lags, subtract_com):
    """float64 sums from the recorded frames: msd, vacf and their error scales, each [B, classes, n_lags]"""
    x, img, v = tr.x.astype(np.float64), tr.image.astype(np.float64), tr.v.astype(np.float64)
    Q, B, n, _ = x.shape
    cls = np.zeros(n, dtype=np.int64) if species is None else np.where(species != 0, 0, 1)
    n_cls = int(cls.max()) + 1
    Lb = L[None, :, None, None]
    m = mass.reshape(B, n)
    com = ((x + img * Lb) * m[None, :, :, None]).sum(axis=2) / m.sum(axis=1)[None, :, None]      # [Q, B, 3]
    out = np.zeros((4, B, n_cls, n_lags))
    for q in range(Q):
        for j in range(min(q, n_lags - 1) + 1):
            o = q - j
            du = (x[q] - x[o]) + (img[q] - img[o]) * Lb[0]                                         # [B, n, 3]
            dc = com[q] - com[o]
            if subtract_com:
                du = du - dc[:, None, :]
            r2 = (du * du).sum(-1)
            vv = (v[q] * v[o]).sum(-1)
            mag_r = r2 + ((dc * dc).sum(-1)[:, None] if subtract_com else 0.0)
            mag_v = np.linalg.norm(v[q], axis=-1) * np.linalg.norm(v[o], axis=-1)
            for c in range(n_cls):
                k = cls == c
                out[0, :, c, j] += r2[:, k].sum(axis=1)
                out[1, :, c, j] += vv[:, k].sum(axis=1)
                out[2, :, c, j] += mag_r[:, k].sum(axis=1)
                out[3, :, c, j] += mag_v[:, k].sum(axis=1)
    return out


@pytest.mark.parametrize("system", ["lj", "water", "lj_two_boxes"])
def test_msd_and_vacf_match_float64_sums_over_the_recorded_frames(system):
    """interval 5, 16 lags, 200 steps (40 origins), with and without the centre-of-mass displacement; a second identical
    run gives the same bits."""
    case = {"lj": lambda: _Case("lj"), "water": lambda: _Case("water"),
            "lj_two_boxes": lambda: _Case("lj", n_boxes=2, boxes=[27.27, 30.0])}[system]()
    L = np.array([_f32(b) for b in case.boxes], dtype=np.float64)
    Q, n_lags = 40, 16
    kw = dict(max_frames=Q, fields=ALL, n_lags=n_lags)
    plain, _ = _recorded(case, 5, 200, **kw)
    again, _ = _recorded(case, 5, 200, **kw)
    com, _ = _recorded(case, 5, 200, subtract_com=True, **kw)
    n_cls = 2 if system == "water" else 1
    for tr in (plain, com):
        assert tr.n_samples == Q and tr.dropped == 0 and tr.ambiguous == 0 and np.isfinite(tr.x).all() and np.isfinite(tr.v).all()
        assert tr.msd_sum.shape == tr.vacf_sum.shape == (case.nb, n_cls, n_lags)
        assert np.array_equal(tr.class_atoms, [[258, 516]] if system == "water" else [[258]] * case.nb)
    assert np.array_equal(plain.msd_sum, again.msd_sum) and np.array_equal(plain.vacf_sum, again.vacf_sum)
    assert _same_bits(plain.x, com.x) and np.array_equal(plain.image, com.image) and np.array_equal(plain.vacf_sum, com.vacf_sum)
    for tr, sub in ((plain, False), (com, True)):
        msd, vacf, mag_r, mag_v = _host_sums(tr, L, case.mass, case.species, n_lags, sub)
        err_r, err_v = np.abs(tr.msd_sum - msd), np.abs(tr.vacf_sum - vacf)
        print(f"{system} subtract_com={sub}: max |dev - host| / bound scale: msd {np.max(err_r[..., 1:] / mag_r[..., 1:]):.2e}, "
              f"vacf {np.max(err_v / mag_v):.2e}")
        assert (msd[..., 1:] > 0).all() and (mag_v > 0).all()
        assert (err_r <= 1e-12 * (mag_r if sub else msd)).all()
        assert (err_v <= 1e-12 * mag_v).all()
        assert (tr.msd_sum[..., 0] == 0.0).all()                             # lag 0: the same operands on both sides of each difference
        v2 = (tr.v.astype(np.float64) ** 2).sum(-1)                          # [Q, B, n]
        cls = np.zeros(case.n, dtype=np.int64) if case.species is None else np.where(case.species != 0, 0, 1)
        for c in range(n_cls):
            s = v2[:, :, cls == c].sum(axis=(0, 2))
            assert (np.abs(tr.vacf_sum[:, c, 0] - s) <= 1e-12 * s).all()
    # the COM of a thermal box barely moves, but the subtraction is visible in the bits
    assert not np.array_equal(plain.msd_sum, com.msd_sum)
    assert plain.msd(0).shape == (n_cls, n_lags) and np.isfinite(plain.msd(0)).all() and (np.diff(plain.msd(0)[0, :4]) > 0).all()


# ---- 5: accumulation across calls, reset, a full frame buffer --------------------------------------------------------
def test_accumulation_across_calls_reset_and_a_full_frame_buffer():
    from gamd_amd._lib import GamdError
    case = _Case("lj")
    kw = dict(fields=ALL, n_lags=8, subtract_com=True)
    one, fin1 = _recorded(case, 6, 120, max_frames=20, **kw)             # samples at 6, 12, ..., 120: calls end between samples
    three, fin3 = _recorded(case, 6, 120, calls=3, max_frames=20, **kw)
    assert one.n_samples == three.n_samples == 20 and np.array_equal(one.steps, 6 * np.arange(1, 21))
    assert np.array_equal(one.steps, three.steps) and np.array_equal(one.image, three.image)
    for k in "xvf":
        assert _same_bits(getattr(one, k), getattr(three, k))
    assert np.array_equal(one.msd_sum, three.msd_sum) and np.array_equal(one.vacf_sum, three.vacf_sum)
    assert (one.msd_sum[..., 1:] > 0).all()
    # a full frame buffer keeps the first frames, counts the rest, and the sums go on
    eng, x, v, f = case.make()
    eng.traj_configure(6, max_frames=3, **kw)
    case.run(eng, x, v, f, 120)
    few = eng.traj_read()
    assert few.steps.tolist() == [6, 12, 18] and few.dropped == 17 and few.n_samples == 20 and few.x.shape[0] == 3
    assert _same_bits(few.x, one.x[:3]) and _same_bits(few.f, one.f[:3]) and np.array_equal(few.image, one.image[:3])
    assert np.array_equal(few.msd_sum, one.msd_sum) and np.array_equal(few.vacf_sum, one.vacf_sum)
    # another box while image counters are kept: refused until the recorder is reset
    with pytest.raises(GamdError, match="box differs"):
        case.run(eng, x, v, f, 6, first_step=120, box=case.box * 1.01)
    eng.sync_status()
    eng.traj_reset()
    z = eng.traj_read()
    assert z.steps.shape == (0,) and z.x.shape[0] == 0 and z.dropped == 0 and z.n_samples == 0 and z.ambiguous == 0
    assert z.msd_sum.size == 0 or not z.msd_sum.any()
    # after the reset the count starts again, from image 0
    case.run(eng, x, v, f, 12, first_step=120)
    again = eng.traj_read()
    assert again.steps.tolist() == [6, 12] and again.n_samples == 2 and not again.image[0].any()
    assert _same_bits(again.x[1].reshape(-1, 3), x.cpu().numpy())
    assert (again.msd_sum[..., 0] == 0).all() and (again.msd_sum[..., 1] > 0).all() and not again.msd_sum[..., 2:].any()
    # configuring while a run is pending is refused
    case.run(eng, x, v, f, 6, first_step=132, sync=False)
    with pytest.raises(GamdError, match="-22.*still enqueued"):
        eng.traj_configure(3)
    with pytest.raises(GamdError, match="-22.*still enqueued"):
        eng.traj_reset()
    assert eng.sync_status() == 0
    assert eng.traj_read().n_samples == 3
    eng.close()


# ---- 6: overflow in the middle of a run ------------------------------------------------------------------------------
@pytest.mark.parametrize("skin_frac", [0.0, 1.0 / 6.0])
def test_overflow_in_the_middle_of_a_run_records_no_sample_twice(skin_frac):
    """Five boxes whose atoms stream towards the box centre, so the edge count grows step by step (the pattern of the
    reporter's overflow test), with a capacity that holds the first edge lists but not the later ones: the run freezes, is
    resumed by sync_status, and frames, images and both sums must be those of the ample buffer, bit for bit.
    Skin mode: regrowing the buffers forces a candidate rebuild at the frozen step, and a rebuild renumbers the atoms and so
    changes the summation order of the forces.  The capacity is therefore chosen so that the run freezes at a step where the
    ample run rebuilds its candidates as well (found by stepping an ample engine once): both runs then rebuild from the
    same positions and stay on the same trajectory."""
    from gamd_amd.engine import GamdForce
    g, _, _ = load_golden("lj258_seed0")
    nb, n, box, rc, steps = 5, 258, float(g["box"]), float(g["cutoff"]), 30
    sd = make_state_dict(ModelConfig(kind="lj"), 0, 5.3, 1.6)
    kw = dict(n_boxes=nb, scaler=SHIPPED_SCALERS["lj"], neighbor_skin=skin_frac * rc)
    base, rng = np.mod(g["pos"], box), np.random.default_rng(2)
    pos = np.concatenate([base + (rng.normal(0, 0.3, base.shape) if b else 0.0) for b in range(nb)])
    x0 = torch.from_numpy(pos).float().cuda()
    v0 = (-(torch.remainder(x0, box) - box / 2)).contiguous() * 1.5
    md = dict(temperature_k=0.0, gamma_per_ps=0.0, seed=1)
    # edge counts (and candidate rebuilds) of the ample run, step by step
    probe = GamdForce(sd, n, box, rc, **kw)
    x, v = x0.clone(), v0.clone()
    f = probe.forward(x, denormalize=True).clone()
    counts, rebuilds = [probe.counts()[0]], [probe.skin_stats()[0]]
    for s in range(steps):
        probe.md_run(x, v, f, 1, first_step=s, **md)
        counts.append(probe.counts()[0])
        rebuilds.append(probe.skin_stats()[0])
    probe.close()
    counts, rebuilds = np.array(counts), np.array(rebuilds)
    peak = np.maximum.accumulate(counts)
    if skin_frac == 0.0:
        cap = int(counts[0]) + 40
    else:
        # step s (1-based) rebuilt in the ample run, and its edge list is the first that is longer than all before it by 2+
        hit = [s for s in range(2, steps + 1) if rebuilds[s] > rebuilds[s - 1] and counts[s] >= peak[s - 1] + 2]
        assert hit, f"no rebuild step with a growing edge list: counts {counts.tolist()}, rebuilds {rebuilds.tolist()}"
        cap = int(peak[hit[0] - 1] + counts[hit[0]]) // 2
    assert counts.max() > cap >= counts[0]
    res = []
    for c in (0, cap):
        eng = GamdForce(sd, n, box, rc, edge_capacity=c, **kw)
        x, v = x0.clone(), v0.clone()
        f = eng.forward(x, denormalize=True).clone()
        assert eng.last_status == 0
        eng.traj_configure(3, max_frames=10, fields=ALL, n_lags=4, subtract_com=True)
        eng.md_run(x, v, f, steps, sync=False, **md)
        assert eng.sync_status() == (1 if c else 0), "the run was meant to outgrow its edge buffer"
        res.append((eng.traj_read(), _state(x, v, f)))
        eng.close()
    (a, fa), (b, fb) = res
    assert np.array_equal(a.steps, 3 * np.arange(1, 11)) and np.array_equal(b.steps, a.steps)
    assert a.n_samples == b.n_samples == 10 and a.dropped == b.dropped == 0 and a.ambiguous == b.ambiguous == 0
    print(f"skin {skin_frac:.3f}: capacity {cap}, edge counts {counts[0]} .. {counts.max()}, max |x_a - x_b| "
          f"{np.abs(a.x - b.x).max():.2e}, max relative msd difference {np.abs(b.msd_sum[..., 1:] / a.msd_sum[..., 1:] - 1).max():.2e}")
    assert np.array_equal(a.image, b.image)
    for k in "xvf":
        assert _same_bits(getattr(a, k), getattr(b, k)), k
    for p, q in zip(fa, fb):
        assert _same_bits(p, q)
    assert np.array_equal(a.msd_sum, b.msd_sum) and np.array_equal(a.vacf_sum, b.vacf_sum)
    assert (a.msd_sum[..., 1:] > 0).all() and np.array_equal(a.class_atoms, [[258]] * nb)


# ---- 7: reporter and recorder together -------------------------------------------------------------------------------
def test_reporter_and_recorder_with_different_intervals_in_skin_mode():
    case = _Case("lj", skin=1.25)
    steps = 48

    def go(report, record):
        eng, x, v, f = case.make()
        if report:
            eng.report_configure(4, rdf_bins=64)
        if record:
            eng.traj_configure(6, max_frames=8, fields=XVF)
        case.run(eng, x, v, f, steps)
        out = (eng.report_read() if report else None, eng.traj_read() if record else None, _state(x, v, f))
        eng.close()
        return out
    rep_b, tr_b, fin_b = go(True, True)
    rep_r, _, fin_r = go(True, False)
    _, tr_t, fin_t = go(False, True)
    assert np.array_equal(rep_b.steps, 4 * np.arange(1, 13)) and np.array_equal(rep_b.steps, rep_r.steps)
    assert np.array_equal(rep_b.ke, rep_r.ke) and np.array_equal(rep_b.rdf_counts, rep_r.rdf_counts) and rep_b.frames == rep_r.frames == 12
    assert np.array_equal(tr_b.steps, 6 * np.arange(1, 9)) and np.array_equal(tr_b.steps, tr_t.steps)
    for k in "xvf":
        assert _same_bits(getattr(tr_b, k), getattr(tr_t, k))
    for p, q, r in zip(fin_b, fin_r, fin_t):
        assert _same_bits(p, q) and _same_bits(p, r)


# ---- 8: checked build ------------------------------------------------------------------------------------------------
def _digest(tr):
    import hashlib
    h = hashlib.sha256()
    for a in (tr.steps, tr.x, tr.v, tr.f, tr.image, tr.msd_sum, tr.vacf_sum, tr.class_atoms):
        h.update(np.ascontiguousarray(a).tobytes())
    return dict(sha=h.hexdigest(), n_samples=tr.n_samples, dropped=tr.dropped, ambiguous=tr.ambiguous,
                msd=tr.msd_sum.reshape(-1).tolist())


def _checked_case(kind, skin):
    """the frames of test 1 and the sums of test 4 in one run: interval 5, 60 steps, 8 lags"""
    tr, _ = _recorded(_Case(kind, skin=skin), 5, 60, max_frames=12, fields=ALL, n_lags=8, subtract_com=True)
    return tr


CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_traj as t
from gamd_amd import _lib
d = t._digest(t._checked_case(%r, %r))
d["version"] = _lib.load().gamd_version().decode()
print("RESULT", json.dumps(d))
"""


@pytest.mark.parametrize("kind,skin", [("water", 0.0), ("lj", 1.25)])
def test_checked_build_records_the_same_bits(kind, skin):
    """libgamd_hip_chk.so in a child process: status 0 from every call (a failed range check would come back as -35) and the
    frames, images and sums of the release build."""
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), kind, skin)
    env = {k: v for k, v in os.environ.items() if k not in ("GAMD_LIB", "GAMD_CHK_INJECT")}
    env["GAMD_LIB"] = CHK
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert p.returncode == 0 and "RESULT" in p.stdout, (p.stdout[-800:], p.stderr[-1500:])
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got.pop("version").endswith("checked")
    want = _digest(_checked_case(kind, skin))
    assert want["n_samples"] == 12 and want["dropped"] == 0 and any(want["msd"])
    assert got == want


# ---- 9: reduced-precision edge dtypes --------------------------------------------------------------------------------
@pytest.mark.parametrize("edge_dtype", ["bf16", "f16x3"])
def test_reduced_precision_edge_dtypes_record_their_own_trajectory(edge_dtype):
    """the recorder reads x, v, f only: frames bit-equal to the chunked run of the same dtype"""
    _check_frames_against_chunks(_Case("lj", edge_dtype=edge_dtype))
