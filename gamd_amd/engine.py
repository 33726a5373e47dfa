"""Host side of the MI355X force path: `GamdForce.forward(pos, box, species) -> forces`.

Mirrors what the reference's Python drivers call:
``ParticleNetLightning.predict_forces`` (LJ/train_network_lj.py:133-157,
water/train_network_tip3p.py:142-159) = neighbour search + model forward +
denormalise.  PyTorch is used for device memory and streams only; all compute
is in libgamd_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import GamdClassicalParams, GamdLbfgsParams, GamdMinimizeParams, GamdWaterParams, GamdWaterPmeParams, GamdReportParams, GamdStructParams, GamdTrajParams, GamdConfig, GamdMdParams, GamdNhcParams, TRAJ_FIELDS, check
from .weights import ModelConfig, infer_config, validate_state_dict

ArrayLike = Union[np.ndarray, torch.Tensor]

KIND = {"lj": 0, "water": 1, "dynbox": 1}
FLAVOUR = {"jaxmd": 0, "torch": 1}
# what `fluid_graph.add_self_loop()` with its result discarded does (nn_module.py:650-652)
SELF_LOOP = {"dgl07_noop": 0, "append_zero_feature_loops": 1}
KSEL_FORCE_GENERIC_WIDTH = 1
KSEL_NO_LAYER0_HOIST = 4        # LJ, fp32: layer 0 in its general four-GEMM form (include/gamd_hip.h)
KSEL_NO_LN_FOLD = 8             # fp32, 128-wide: e = LayerNorm(...) formed by the encoder, not folded into the conv layers


def _box3(box) -> np.ndarray:
    b = np.asarray(box, dtype=np.float64).reshape(-1)
    if b.size == 1:
        b = np.repeat(b, 3)
    if b.size != 3:
        raise ValueError("box must be a scalar or 3 values")
    return b.astype(np.float32)


def _boxes(box, n_boxes: int) -> np.ndarray:
    """scalar | [3] (ONE orthorhombic box, the same for every box) | [n_boxes, 1] or [n_boxes] cubic edge per box |
    [n_boxes, 3] -> float32 [n_boxes, 3].  A 1-D input of three numbers is always one box for all, also when n_boxes == 3:
    per-box cubic edges of a 3-box batch are spelled [3, 1] (or [3, 3])."""
    b = np.asarray(box, dtype=np.float64)
    if b.ndim == 0 or b.size == 1 or (b.ndim == 1 and b.size == 3):
        return np.tile(_box3(b), (n_boxes, 1))
    if b.ndim == 2 and b.shape == (n_boxes, 3):
        return b.astype(np.float32)
    if (b.ndim == 1 and b.size == n_boxes) or (b.ndim == 2 and b.shape == (n_boxes, 1)):
        return np.repeat(b.reshape(-1).astype(np.float32)[:, None], 3, axis=1)
    raise ValueError(f"box must be a scalar, 3 values, [{n_boxes}, 1] or [{n_boxes}, 3] ({n_boxes} boxes)")


def _rdf_from_counts(counts, frames: int, r_max: float, n_by_class, vol: float):
    """(r_mid [bins], g [P, bins]) from DIRECTED pair counts [P, bins]: g_ab(k) = c_ab[k] / (frames * m_ab * V_shell(k) / V)
    with m_aa = N_a^2 and m_ab = 2 N_a N_b.  Shared by the run reporter and the structure sampler."""
    c = np.asarray(counts).astype(np.float64)
    n_pairs, bins = c.shape
    if bins == 0 or frames == 0:
        raise ValueError("no histogram was recorded")
    nn = np.atleast_1d(np.asarray(n_by_class, dtype=np.float64))
    if n_pairs == 1:
        m = np.array([nn[0] ** 2])
    else:
        if nn.shape[0] != 2:
            raise ValueError("three pair classes need n_by_class = (N_O, N_H)")
        m = np.array([nn[0] ** 2, 2.0 * nn[0] * nn[1], nn[1] ** 2])
    edges = np.arange(bins + 1, dtype=np.float64) * (r_max / bins)
    shell = 4.0 / 3.0 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
    g = c / (frames * m[:, None] * shell[None, :] / vol)
    return 0.5 * (edges[1:] + edges[:-1]), g


def structure_kvectors(n2max: int) -> np.ndarray:
    """The structure sampler's wave-vector list as the library builds it: the integer triples n with 0 < |n|^2 <= n2max, one of
    each +-n (the one whose first non-zero component is positive), sorted by (|n|^2, n_x, n_y, n_z).  int32 [K, 3]."""
    n2max = int(n2max)
    if n2max <= 0:
        return np.zeros((0, 3), dtype=np.int32)
    m = int(np.floor(np.sqrt(n2max)))
    while (m + 1) * (m + 1) <= n2max:
        m += 1
    r = np.arange(-m, m + 1)
    n = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    n2 = (n * n).sum(axis=1)
    lead = np.where(n[:, 0] != 0, n[:, 0], np.where(n[:, 1] != 0, n[:, 1], n[:, 2]))
    keep = (n2 > 0) & (n2 <= n2max) & (lead > 0)
    n, n2 = n[keep], n2[keep]
    order = np.lexsort((n[:, 2], n[:, 1], n[:, 0], n2))
    return n[order].astype(np.int32)


class RunStructure:
    """What the structure sampler accumulated (GamdForce.structure_read).  Host-only: plain arrays in, plain arrays out.

    rdf_counts [n_boxes, P, bins] uint64: directed pair counts per distance bin out to ``r_max`` (every unordered pair adds
    2), P = 1 (LJ) or 3 (water: O-O, O-H, H-H); sk_sum [n_boxes, P, K] float64: sums over the frames of Re(rho_a conj(rho_b));
    kvectors [K, 3] int32: the integer triples n of k = 2 pi n / L; frames: samples taken; boxes [n_boxes, 3]: box edges."""

    def __init__(self, rdf_counts, sk_sum, kvectors, frames: int, r_max: float = 0.0, boxes=None):
        self.rdf_counts = np.asarray(rdf_counts, dtype=np.uint64)
        self.sk_sum = np.asarray(sk_sum, dtype=np.float64)
        self.kvectors = np.asarray(kvectors, dtype=np.int32).reshape(-1, 3)
        self.frames = int(frames)
        self.r_max = float(r_max)
        self.boxes = None if boxes is None else np.asarray(boxes, dtype=np.float64).reshape(-1, 3)

    def rdf(self, box: int, n_by_class, volume: Optional[float] = None):
        """(r_mid [bins], g [P, bins]) of box ``box``, normalised as RunReport.rdf: ``n_by_class`` is N for one pair class,
        (N_O, N_H) for three."""
        vol = float(volume) if volume is not None else float(np.prod(self.boxes[box]))
        return _rdf_from_counts(self.rdf_counts[box], self.frames, self.r_max, n_by_class, vol)

    def sk(self, box: int, n_by_class, shell_average: bool = False):
        """(|k| [K], S [P, K]) of box ``box``: S_ab(k) = sk_sum / (frames * sqrt(N_a N_b)) (Ashcroft-Langreth), |k| from the
        box edges.  ``shell_average``: one value per |n|^2, the mean over its vectors ([shells], [P, shells]); cubic boxes
        only (vectors of equal |n|^2 have different |k| otherwise)."""
        s = self.sk_sum[box]
        n_pairs, K = s.shape
        if K == 0 or self.frames == 0:
            raise ValueError("no structure factor was sampled")
        nn = np.atleast_1d(np.asarray(n_by_class, dtype=np.float64))
        if n_pairs == 1:
            m = np.array([nn[0]])
        else:
            if nn.shape[0] != 2:
                raise ValueError("three pair classes need n_by_class = (N_O, N_H)")
            m = np.array([nn[0], np.sqrt(nn[0] * nn[1]), nn[1]])
        edges = self.boxes[box]
        kk = 2.0 * np.pi * np.sqrt(((self.kvectors.astype(np.float64) / edges[None, :]) ** 2).sum(axis=1))
        val = s / (self.frames * m[:, None])
        if not shell_average:
            return kk, val
        if not (edges[0] == edges[1] == edges[2]):
            raise ValueError("shell_average needs a cubic box")
        n2 = (self.kvectors.astype(np.int64) ** 2).sum(axis=1)
        shells, inv, cnt = np.unique(n2, return_inverse=True, return_counts=True)
        out = np.zeros((n_pairs, shells.shape[0]), dtype=np.float64)
        for c in range(n_pairs):
            out[c] = np.bincount(inv, weights=val[c], minlength=shells.shape[0]) / cnt
        return 2.0 * np.pi * np.sqrt(shells.astype(np.float64)) / edges[0], out


class RunReport:
    """What the run reporter recorded (GamdForce.report_read).

    steps [S] int64: completed MD steps g at each sample; ke, temperature [S, n_boxes] float64 (kJ/mol, K);
    rdf_counts [n_boxes, P, bins] uint64: directed pair counts per distance bin, P = 1 (LJ) or 3 (water: O-O, O-H in both
    directions, H-H); frames: frames in the histogram; dropped: samples that found the log full.
    r_max / volumes: upper edge of the last bin and the box volumes, for ``rdf``."""

    def __init__(self, steps, ke, temperature, rdf_counts, frames: int, dropped: int, r_max: float = 0.0, volumes=None):
        self.steps = np.asarray(steps, dtype=np.int64)
        self.ke = np.atleast_2d(np.asarray(ke, dtype=np.float64))              # [S, n_boxes]
        self.temperature = np.atleast_2d(np.asarray(temperature, dtype=np.float64))
        self.rdf_counts = np.asarray(rdf_counts, dtype=np.uint64)
        self.frames, self.dropped = int(frames), int(dropped)
        self.r_max = float(r_max)
        self.volumes = None if volumes is None else np.asarray(volumes, dtype=np.float64).reshape(-1)

    def rdf(self, box: int, n_by_class, volume: Optional[float] = None):
        """(r_mid [bins], g [P, bins]) of box ``box``: g_ab(k) = c_ab[k] / (frames * m_ab * V_shell(k) / V) with
        m_aa = N_a^2 and m_ab = 2 N_a N_b for the directed counts.  ``n_by_class``: N for one pair class, (N_O, N_H) for
        three."""
        c = self.rdf_counts[box]
        if c.shape[1] == 0 or self.frames == 0:
            raise ValueError("no histogram was recorded")
        vol = float(volume) if volume is not None else float(self.volumes[box])
        return _rdf_from_counts(c, self.frames, self.r_max, n_by_class, vol)

    def write_state_data(self, path, dt_ps: float, separator: str = "\t", driver_step_convention: bool = False,
                         box: int = 0) -> None:
        """The log file OpenMM's StateDataReporter(step=True, time=True, kineticEnergy=True, temperature=True) writes.
        ``driver_step_convention``: Step and Time count the two ``simulation.step(1)`` calls per iteration of the
        reference drivers (Step = 2 g, Time = 2 g dt), as their own logs do; otherwise Step = g, Time = g dt."""
        k = 2 if driver_step_convention else 1
        head = ['"Step"', '"Time (ps)"', '"Kinetic Energy (kJ/mole)"', '"Temperature (K)"']
        with open(path, "w") as fh:
            fh.write("#" + separator.join(head) + "\n")
            for i, g in enumerate(self.steps):
                row = [str(k * int(g)), str(k * int(g) * float(dt_ps)), str(float(self.ke[i, box])),
                       str(float(self.temperature[i, box]))]
                fh.write(separator.join(row) + "\n")


class RunTrajectory:
    """What the run recorder kept (GamdForce.traj_read).  Host-only: plain arrays in, plain arrays out.

    steps [F] int64: completed MD steps g of each kept frame; x, v, f float32 and image int32 [F, B, n, 3] in the caller's
    atom order, or None when the field was not recorded; dropped: samples that found the frame buffer full; ambiguous:
    (atom, sample) pairs that moved more than a quarter of a box edge between two samples (the image counters assume less
    than half); n_samples: samples taken = time origins Q; class_atoms [B, classes]; msd_sum, vacf_sum [B, classes, n_lags]:
    the device's sums over origins and atoms; interval: MD steps between two samples (one lag)."""

    def __init__(self, steps=None, x=None, v=None, f=None, image=None, dropped: int = 0, ambiguous: int = 0,
                 n_samples: int = 0, class_atoms=None, msd_sum=None, vacf_sum=None, interval: int = 1):
        def arr(a, dt):
            return None if a is None else np.asarray(a, dtype=dt)
        self.steps = np.zeros(0, dtype=np.int64) if steps is None else np.asarray(steps, dtype=np.int64)
        self.x, self.v, self.f = arr(x, np.float32), arr(v, np.float32), arr(f, np.float32)
        self.image = arr(image, np.int32)
        self.dropped, self.ambiguous, self.n_samples = int(dropped), int(ambiguous), int(n_samples)
        self.class_atoms = None if class_atoms is None else np.atleast_2d(np.asarray(class_atoms, dtype=np.int64))
        self.msd_sum, self.vacf_sum = arr(msd_sum, np.float64), arr(vacf_sum, np.float64)
        self.interval = int(interval)

    @property
    def n_lags(self) -> int:
        return 0 if self.msd_sum is None else int(self.msd_sum.shape[-1])

    def unwrapped(self, box) -> np.ndarray:
        """float64 [F, B, n, 3] unwrapped positions x + image * L.  ``box``: scalar, [3], [B, 1] or [B, 3] edge lengths
        (used as their fp32 values, like the library)."""
        if self.x is None or self.image is None:
            raise ValueError("unwrapped needs the fields x and image")
        L = _boxes(box, self.x.shape[1]).astype(np.float64)
        return self.x.astype(np.float64) + self.image.astype(np.float64) * L[None, :, None, :]

    def _normalised(self, sums, box: int) -> np.ndarray:
        if sums is None or self.n_lags == 0:
            raise ValueError("no correlation functions were recorded (n_lags = 0)")
        origins = (self.n_samples - np.arange(self.n_lags)).astype(np.float64)             # Q - j
        den = np.where(origins > 0, origins, np.nan)[None, :] * self.class_atoms[box].astype(np.float64)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(den > 0, sums[box] / den, np.nan)

    def msd(self, box: int = 0) -> np.ndarray:
        """[classes, n_lags] mean-squared displacement of box ``box`` in (length unit)^2: msd_sum / ((Q - j) class_atoms);
        NaN where no origin has that lag yet."""
        return self._normalised(self.msd_sum, box)

    def vacf(self, box: int = 0) -> np.ndarray:
        """[classes, n_lags] <v(t) . v(0)> of box ``box`` in (length unit / ps)^2, normalised like ``msd``."""
        return self._normalised(self.vacf_sum, box)

    def lag_times(self, dt_ps: float) -> np.ndarray:
        return np.arange(self.n_lags, dtype=np.float64) * (self.interval * float(dt_ps))

    def diffusion_msd(self, box: int, cls: int, dt_ps: float, fit: Tuple[int, int], length_per_nm: float = 0.0) -> float:
        """Einstein relation: the unweighted least-squares slope (with an intercept) of MSD against time over the lags
        fit = (lo, hi), both included, divided by 6.  In (length unit)^2 / ps, or nm^2 / ps when ``length_per_nm`` is given."""
        lo, hi = int(fit[0]), int(fit[1])
        if not 0 <= lo < hi < self.n_lags:
            raise ValueError(f"fit = ({lo}, {hi}) must satisfy 0 <= lo < hi < n_lags = {self.n_lags}")
        t = self.lag_times(dt_ps)[lo:hi + 1]
        y = self.msd(box)[cls, lo:hi + 1]
        tc = t - t.mean()
        d = float((tc * (y - y.mean())).sum() / (tc * tc).sum()) / 6.0
        return d / float(length_per_nm) ** 2 if length_per_nm else d

    def diffusion_green_kubo(self, box: int, cls: int, dt_ps: float, upto: int, length_per_nm: float = 0.0) -> float:
        """Green-Kubo: the trapezoid integral of the VACF over the lags 0 .. upto (included), divided by 3."""
        upto = int(upto)
        if not 0 < upto < self.n_lags:
            raise ValueError(f"upto = {upto} must satisfy 0 < upto < n_lags = {self.n_lags}")
        c = self.vacf(box)[cls, :upto + 1]
        h = self.interval * float(dt_ps)
        d = float(h * (0.5 * c[0] + c[1:-1].sum() + 0.5 * c[-1])) / 3.0
        return d / float(length_per_nm) ** 2 if length_per_nm else d

    def write_dataset(self, dir, seed: int, prefix: str = "data_", length_per_nm: float = 0.0) -> list:
        """One ``{prefix}{seed}_{t}.npz`` per kept frame t of box 0, in the layout and units of the reference's data
        generators (dataset/generate_lj_data.py:100-106), which train_utils.LJDataNew / WaterDataNew open: ``pos`` in
        Angstrom, ``vel`` in m/s (Angstrom/ps x 100; when recorded), ``forces`` in kJ/mol/nm (when recorded); float32,
        caller order.  ``length_per_nm``: the run's length unit (0 or 10 = Angstrom, 18.8972613 = bohr).  Returns the paths."""
        if self.x is None:
            raise ValueError("write_dataset needs the field x")
        to_angstrom = np.float64(10.0) / np.float64(np.float32(length_per_nm)) if length_per_nm else np.float64(1.0)
        os.makedirs(dir, exist_ok=True)
        paths = []
        for t in range(self.x.shape[0]):
            out = {"pos": (self.x[t, 0].astype(np.float64) * to_angstrom).astype(np.float32)}
            if self.v is not None:
                out["vel"] = (self.v[t, 0].astype(np.float64) * (to_angstrom * 100.0)).astype(np.float32)
            if self.f is not None:
                out["forces"] = self.f[t, 0].astype(np.float32)
            paths.append(os.path.join(dir, f"{prefix}{seed}_{t}.npz"))
            np.savez(paths[-1], **out)
        return paths


KJ_PER_KCAL = 4.184
BAR_PER_KJ_MOL_NM3 = 16.6053906717          # 1 kJ/mol/nm^3 = 1e3 / (6.02214076e23 * 1e-27) Pa = 16.6053906717 bar


def lj_dispersion_correction(n_sites: int, volume_nm3: float, sigma: float, epsilon: float, r_cut: float,
                             r_switch: float = 0.0, order: int = 64) -> Tuple[float, float]:
    """(U_lrc, W_lrc) in kJ/mol: the long-range dispersion correction of ``n_sites`` Lennard-Jones sites at uniform density in
    ``volume_nm3`` for the switched 12-6 potential the observers evaluate, and its virial W_lrc = 3 U_lrc (U_lrc scales as
    1 / V, so -dU/dlnV^(1/3) = 3 U).  U_lrc = 2 pi n^2 / V * integral over r >= r_switch of [u_LJ(r) - u_used(r)] r^2 dr:
    beyond ``r_cut`` u_used = 0 and the integral is the closed form 4 eps (sigma^12 / (9 r_c^9) - sigma^6 / (3 r_c^3)); on the
    switch interval u_LJ - u_used = u_LJ (1 - S) with S(t) = 1 - t^3 (6 t^2 - 15 t + 10), t = (r - r_s) / (r_c - r_s), taken by
    Gauss-Legendre quadrature of ``order`` points (a smooth integrand: 64 points are exact to rounding).  ``sigma``,
    ``r_cut``, ``r_switch`` in nm, ``epsilon`` in kJ/mol; ``r_switch`` = 0 or >= r_cut: no switching.  Host only; it concerns
    energy and pressure, never forces.  Not defined for a shifted potential (the shift is a constant inside the cutoff, whose
    'correction' would grow with the volume): the ``pressure`` methods refuse that."""
    n, vol, sig, eps, rc, rs = float(n_sites), float(volume_nm3), float(sigma), float(epsilon), float(r_cut), float(r_switch)
    if not (vol > 0.0 and sig > 0.0 and rc > 0.0):
        raise ValueError("volume_nm3, sigma and r_cut must be positive")
    s6 = sig ** 6
    tail = 4.0 * eps * (s6 * s6 / (9.0 * rc ** 9) - s6 / (3.0 * rc ** 3))
    inner = 0.0
    if 0.0 < rs < rc:
        t, w = np.polynomial.legendre.leggauss(int(order))
        r = 0.5 * (rc - rs) * t + 0.5 * (rc + rs)
        u = (r - rs) / (rc - rs)
        one_minus_s = u ** 3 * ((6.0 * u - 15.0) * u + 10.0)
        s6r = s6 / r ** 6
        inner = 0.5 * (rc - rs) * float(np.sum(w * (4.0 * eps * (s6r * s6r - s6r)) * one_minus_s * r * r))
    u_lrc = 2.0 * np.pi * n * n / vol * (tail + inner)
    return float(u_lrc), float(3.0 * u_lrc)


def _dispersion_virial(lj, n_sites: int, vol: np.ndarray) -> np.ndarray:
    """[B] W_lrc of the potential ``lj`` (what classical_read / water_classical_read attach: sigma, epsilon, r_cut, r_switch in
    the engine's length unit, shift, length_per_nm) for the volumes ``vol`` [B] in nm^3"""
    if lj is None:
        raise ValueError("dispersion=True needs the potential's parameters: read the log through classical_read / water_classical_read")
    if lj["shift"]:
        raise ValueError("the long-range dispersion correction is not defined for a shifted potential (shift=True)")
    ln = float(lj["length_per_nm"]) or 10.0
    return np.array([lj_dispersion_correction(n_sites, v, lj["sigma"] / ln, lj["epsilon"], lj["r_cut"] / ln, lj["r_switch"] / ln)[1]
                     for v in vol], dtype=np.float64)


class RunClassical:
    """What the classical observer logged (GamdForce.classical_read).  Host-only: plain arrays in, plain arrays out.

    steps [S] int64: completed MD steps g at each sample; per sample and box, float64 [S, B]: energy (kJ/mol), virial
    W = sum_{i<j} d . F_ij (kJ/mol), pairs (pairs inside r_cut), and the force-error sums of the run's forces f against the
    classical forces f_cl (both kJ/mol/nm): sum_abs = sum_i sum_c |f - f_cl|, sum_sq = sum_i |f - f_cl|^2, sum_cos = sum_i
    cos(f_i, f_cl,i), sum_norm_cl = sum_i |f_cl,i|, sum_norm = sum_i |f_i|, excluded = atoms left out of sum_cos because one
    of the two forces is zero.  n_atoms: atoms per box; dropped: samples that found the log full; forces [B * n, 3] float64:
    the classical forces of the last sample, or None."""

    COLUMNS = ("energy", "virial", "pairs", "sum_abs", "sum_sq", "sum_cos", "sum_norm_cl", "sum_norm", "excluded")

    def __init__(self, steps, rows, n_atoms: int, dropped: int = 0, forces=None):
        self.steps = np.asarray(steps, dtype=np.int64)
        rows = np.asarray(rows, dtype=np.float64)
        if rows.ndim != 3 or rows.shape[0] != self.steps.shape[0] or rows.shape[2] != len(self.COLUMNS):
            raise ValueError(f"rows must be [{self.steps.shape[0]}, n_boxes, {len(self.COLUMNS)}], got {rows.shape}")
        for k, name in enumerate(self.COLUMNS):
            setattr(self, name, rows[:, :, k].copy())
        self.n_atoms, self.dropped = int(n_atoms), int(dropped)
        self.forces = None if forces is None else np.asarray(forces, dtype=np.float64)

    def force_errors(self, unit: float = 1.0) -> Dict[str, np.ndarray]:
        """The accuracy figures of LJ/test_script/lj.ipynb cell 3 per sample and box, [S, B] each, network force against
        classical force: ``mae`` = sum_abs / (3 N), ``rmse`` = sqrt(sum_sq / (3 N)), ``cosine`` = sum_cos / (N - excluded),
        ``relative_mae`` = mae / (sum_norm_cl / N).  ``unit`` multiplies mae and rmse (the notebook's 0.0010364 turns
        kJ/mol/nm into eV/Angstrom; the relative figure and the cosine do not depend on it)."""
        n = float(self.n_atoms)
        mae = self.sum_abs / (3.0 * n)
        with np.errstate(divide="ignore", invalid="ignore"):
            cos = np.where(n - self.excluded > 0, self.sum_cos / (n - self.excluded), np.nan)
            rel = np.where(self.sum_norm_cl > 0, mae / (self.sum_norm_cl / n), np.nan)
        return {"mae": float(unit) * mae, "rmse": float(unit) * np.sqrt(self.sum_sq / (3.0 * n)), "cosine": cos, "relative_mae": rel}

    lj = None          # the potential's parameters, attached by the engine's read calls (``dispersion`` needs them)

    def pressure(self, ke, volumes, dispersion: bool = False) -> np.ndarray:
        """[S, B] virial pressure in bar: (2 KE + W) / (3 V) with KE [S, B] in kJ/mol (RunReport.ke of the same samples),
        ``volumes`` scalar or [B] in nm^3; 1 kJ/mol/nm^3 = 16.6053906717 bar.  ``dispersion``: add W_lrc / (3 V), the
        long-range dispersion correction of ``lj_dispersion_correction`` for n_atoms sites (ValueError for a shifted
        potential); off by default, and then no long-range correction is applied."""
        ke = np.asarray(ke, dtype=np.float64).reshape(self.virial.shape)
        vol = np.broadcast_to(np.asarray(volumes, dtype=np.float64).reshape(-1), (self.virial.shape[1],))
        p = BAR_PER_KJ_MOL_NM3 * (2.0 * ke + self.virial) / (3.0 * vol[None, :])
        if dispersion:
            p = p + BAR_PER_KJ_MOL_NM3 * _dispersion_virial(self.lj, self.n_atoms, vol)[None, :] / (3.0 * vol[None, :])
        return p

    def write_state_data(self, report: "RunReport", path, dt_ps: float, separator: str = "\t",
                         driver_step_convention: bool = False, box: int = 0) -> None:
        """The log file OpenMM's StateDataReporter(step=True, time=True, potentialEnergy=True, kineticEnergy=True,
        totalEnergy=True, temperature=True) writes, in its column order, from a RunReport taken at the same interval (the
        two step columns must be equal).  ``driver_step_convention`` as in RunReport.write_state_data."""
        if not np.array_equal(np.asarray(report.steps, dtype=np.int64), self.steps):
            raise ValueError("the reporter's and the classical observer's step columns differ: configure both with one interval "
                             "and enough rows, and reset them together")
        k = 2 if driver_step_convention else 1
        head = ['"Step"', '"Time (ps)"', '"Potential Energy (kJ/mole)"', '"Kinetic Energy (kJ/mole)"', '"Total Energy (kJ/mole)"',
                '"Temperature (K)"']
        with open(path, "w") as fh:
            fh.write("#" + separator.join(head) + "\n")
            for i, g in enumerate(self.steps):
                pe, ke = float(self.energy[i, box]), float(report.ke[i, box])
                row = [str(k * int(g)), str(k * int(g) * float(dt_ps)), str(pe), str(ke), str(pe + ke), str(float(report.temperature[i, box]))]
                fh.write(separator.join(row) + "\n")


COULOMB_KJ_NM = 138.935456                   # 1 / (4 pi eps0) in kJ nm / (mol e^2), as OpenMM's ONE_4PI_EPS0 is remembered (UNVERIFIED)
# the 3-site defaults of water_classical_configure, and TIP4P-Ew as keyword arguments of it (lengths in Angstrom; the rigid
# geometry is TIP3P's, 0.9572 Angstrom and 104.52 degrees, so |OM| = 0.125 Angstrom).  Both sets are meant to be those of OpenMM's
# tip3p.xml / tip4pew.xml, but they were written down from memory and are UNVERIFIED: neither OpenMM nor openmmtools was
# available to compare against.
TIP3P = dict(q_h=0.417, sigma_o=3.15075, epsilon_o=0.635968, m_site=0.0)
TIP4PEW = dict(q_h=0.52422, sigma_o=3.16435, epsilon_o=0.680946, m_site=0.106676721)


PME_LENGTHS = (8, 16, 32, 64, 128)                          # the grid lengths gamd_water_pme takes


def pme_grid(alpha: float, box, tol: float, order: int = 6):
    """The smallest admissible grid (nx, ny, nz) for ``water_classical_configure(..., pme=...)``: per axis the smallest power of
    two in {8, ..., 128} with n >= 2 alpha L / (3 tol^(1/5)), OpenMM's rule for its PME grid (``alpha`` in the reciprocal of the
    length unit of ``box``, one edge or three).  The rule was derived for B-splines of order 5 and is used here as a STARTING
    POINT, not a guarantee: ``order`` 6 is usually more accurate than it promises and 4 less; profiles/run_water_pme.md has
    measured errors against the plain sum.  ``order`` is checked (4 or 6) and otherwise not used.  ValueError where an axis
    would need more than 128 points."""
    if int(order) not in (4, 6):
        raise ValueError(f"order = {order!r} is not 4 or 6 (odd orders are not offered)")
    if not (float(alpha) > 0.0 and 0.0 < float(tol) < 1.0):
        raise ValueError(f"alpha = {alpha!r} must be positive and tol = {tol!r} in (0, 1)")
    edges = np.broadcast_to(np.asarray(box, dtype=np.float64).reshape(-1), (3,))
    out = []
    for L in edges:
        need = 2.0 * float(alpha) * float(L) / (3.0 * float(tol) ** 0.2)
        fits = [n for n in PME_LENGTHS if n >= need]
        if not fits:
            raise ValueError(f"an edge of {L} needs {need:.1f} grid points at alpha = {alpha}, tol = {tol}: more than {PME_LENGTHS[-1]}")
        out.append(fits[0])
    return tuple(out)


class RunWaterClassical(RunClassical):
    """What the water classical observer logged (GamdForce.water_classical_read).  Host-only: plain arrays in, plain arrays
    out.

    steps [S] int64; per sample and box, float64 [S, B], all energies in kJ/mol: u_lj (O-O Lennard-Jones), u_real (real-space
    Ewald sum of the different-molecule pairs inside r_cut plus the same-molecule erf correction), u_recip, u_self, pairs
    (different-molecule pairs inside r_cut), the force-error sums and ``excluded`` of RunClassical, and sum_q, the sum of the
    charges in e: exactly 0.0 unless the species vector is not one O and two H per molecule.  ``energy`` is the sum of the four
    Coulomb terms plus u_lj, added as ((u_real + u_recip) + u_self) + u_lj.  The rows hold no virial: with rigid molecules
    the atomic virial is not the pressure.  ``force_errors`` and ``write_state_data`` are RunClassical's.

    With the virial log armed (``water_classical_configure(..., virial=True)``) ``virial_rows`` [S, B, 6] come with the rows,
    slot for slot: ``virial_terms`` = dict of w_lj, w_coul (the pair terms, real space and exclusion), w_recip, w_intra
    (sum over molecules of s_a . F_a about the centre of mass), each [S, B] in kJ/mol; ``ke_com`` [S, B] the kinetic energy
    of the molecules' centres of mass; ``virial`` [S, B] the molecular virial W_mol = w_lj + w_coul + w_recip - w_intra as the
    device added it.  Without them the three are None."""

    COLUMNS = ("u_lj", "u_real", "u_recip", "u_self", "pairs", "sum_abs", "sum_sq", "sum_cos", "sum_norm_cl", "sum_norm",
               "excluded", "sum_q")
    VIRIAL_COLUMNS = ("w_lj", "w_coul", "w_recip", "w_intra", "ke_com", "w_mol")

    def __init__(self, steps, rows, n_atoms: int, dropped: int = 0, forces=None, virial_rows=None):
        super().__init__(steps, rows, n_atoms, dropped, forces)
        self.energy = ((self.u_real + self.u_recip) + self.u_self) + self.u_lj
        self.set_virial_rows(virial_rows)

    def set_virial_rows(self, virial_rows) -> None:
        """Attach (or with None drop) the virial rows [S, B, 6] of the same samples."""
        self.virial = self.virial_terms = self.ke_com = None
        if virial_rows is not None:
            vr = np.asarray(virial_rows, dtype=np.float64)
            if vr.shape != self.u_lj.shape + (len(self.VIRIAL_COLUMNS),):
                raise ValueError(f"virial_rows must be {self.u_lj.shape + (len(self.VIRIAL_COLUMNS),)}, got {vr.shape}")
            self.virial_terms = {name: vr[:, :, k].copy() for k, name in enumerate(self.VIRIAL_COLUMNS[:4])}
            self.ke_com, self.virial = vr[:, :, 4].copy(), vr[:, :, 5].copy()

    def pressure(self, ke, volumes, dispersion: bool = False):
        """[S, B] pressure of the rigid molecules in bar: (2 KE_com + W_mol) / (3 V), ``volumes`` scalar or [B] in nm^3.
        ``ke`` None: the logged ``ke_com``; otherwise [S, B] centre-of-mass kinetic energies in kJ/mol (NOT RunReport.ke,
        which holds the rotations too).  ``dispersion``: add W_lrc / (3 V) for the n_atoms / 3 oxygens (ValueError for a
        shifted potential).  NotImplementedError without logged virial rows."""
        if self.virial is None:
            raise NotImplementedError("the water classical observer logged no virial rows (with rigid molecules the atomic virial is not "
                                      "the pressure): arm the molecular virial with water_classical_configure(..., virial=True)")
        ke = self.ke_com if ke is None else np.asarray(ke, dtype=np.float64).reshape(self.virial.shape)
        vol = np.broadcast_to(np.asarray(volumes, dtype=np.float64).reshape(-1), (self.virial.shape[1],))
        p = BAR_PER_KJ_MOL_NM3 * (2.0 * ke + self.virial) / (3.0 * vol[None, :])
        if dispersion:
            p = p + BAR_PER_KJ_MOL_NM3 * _dispersion_virial(self.lj, self.n_atoms // 3, vol)[None, :] / (3.0 * vol[None, :])
        return p


class MinimizeResult:
    """What ``GamdForce.minimize`` did.  ``status``: the call's return value (0 every box converged, 1 a box stopped at
    max_iter, 2 a box failed: not finite).  Per box, float64 [B] unless noted: ``state`` (list of "converged" | "max_iter" |
    "failed"), ``iterations`` (int64: position updates), ``energy_start`` / ``rms_start`` and ``energy`` / ``rms`` (kJ/mol,
    kJ/mol/nm: root mean square of the 3N force components, OpenMM's tolerance), ``fmax`` (largest |force component| at the
    end), ``dt`` (the final pseudo-time step).  ``x`` / ``f``: the tensors the call wrote; ``x64``: the unrounded, unwrapped
    double positions or None.  ``rows`` is the library's table [B, 8]."""

    def __init__(self, status: int, rows, x=None, f=None, x64=None):
        self.status = int(status)
        self.rows = np.asarray(rows, dtype=np.float64)
        self.state = [_lib.MINIMIZE_STATE[int(s)] for s in self.rows[:, 0]]
        self.iterations = self.rows[:, 1].astype(np.int64)
        self.energy_start, self.rms_start = self.rows[:, 2], self.rows[:, 3]
        self.energy, self.rms, self.fmax, self.dt = self.rows[:, 4], self.rows[:, 5], self.rows[:, 6], self.rows[:, 7]
        self.x, self.f, self.x64 = x, f, x64

    @property
    def converged(self) -> bool:
        return self.status == 0

    def __repr__(self):
        return f"MinimizeResult(state={self.state}, iterations={self.iterations.tolist()}, energy={self.energy.tolist()}, rms={self.rms.tolist()})"


class LbfgsResult:
    """What ``GamdForce.minimize_lbfgs`` did.  ``status``: the call's return value (0 every box converged, 1 a box stopped at
    max_iter, 2 a box failed: not finite, 3 a box stopped in the line search; the largest wins).  Per box, float64 [B] unless
    noted: ``state`` (list of "converged" | "max_iter" | "failed" | "line_search"), ``evaluations`` (int64: pair evaluations
    behind the start's), ``accepted`` (int64: steps taken), ``energy_start`` / ``rms_start`` and ``energy`` / ``rms`` (kJ/mol,
    kJ/mol/nm: root mean square of the 3N force components, OpenMM's tolerance), ``fmax`` (largest per-atom |F_i| at the end),
    ``skipped`` (int64: accepted steps whose pair the curvature test kept out of the history), ``resets`` (int64: line
    searches that failed and emptied the history).  ``x`` / ``f``: the tensors the call wrote; ``x64``: the unrounded,
    unwrapped double positions or None.  ``rows`` is the library's table [B, 10]."""

    def __init__(self, status: int, rows, x=None, f=None, x64=None):
        self.status = int(status)
        self.rows = np.asarray(rows, dtype=np.float64)
        self.state = [_lib.LBFGS_STATE[int(s)] for s in self.rows[:, 0]]
        self.evaluations = self.rows[:, 1].astype(np.int64)
        self.accepted = self.rows[:, 2].astype(np.int64)
        self.energy_start, self.rms_start = self.rows[:, 3], self.rows[:, 4]
        self.energy, self.rms, self.fmax = self.rows[:, 5], self.rows[:, 6], self.rows[:, 7]
        self.skipped, self.resets = self.rows[:, 8].astype(np.int64), self.rows[:, 9].astype(np.int64)
        self.x, self.f, self.x64 = x, f, x64

    @property
    def converged(self) -> bool:
        return self.status == 0

    def __repr__(self):
        return (f"LbfgsResult(state={self.state}, evaluations={self.evaluations.tolist()}, energy={self.energy.tolist()}, "
                f"rms={self.rms.tolist()})")


class GamdForce:
    """One GPU-resident force model for a fixed atom count.

    Parameters mirror build_model()/ParticleNetLightning.__init__ of the reference:
    ``state_dict`` (reference key names), ``box``/``cutoff`` (BOX_SIZE / CUTOFF_RADIUS
    module constants there), ``bond`` (create_water_bond) and the scaler (mean, var).

    ``n_boxes`` > 1: that many INDEPENDENT boxes of ``n_atoms`` atoms each share every launch (the reference's
    several-graphs-per-forward, nn_module.py:655-661,676-679; a replica ensemble on one GPU).  Positions / species /
    forces are then [n_boxes * n_atoms, ...] (or [n_boxes, n_atoms, ...]), box-major; ``box`` may differ per box
    ([n_boxes, 3]); ``bond`` names atoms of one box.  Results are bit-identical to the boxes evaluated one by one.
    """

    def __init__(self, state_dict: Dict[str, torch.Tensor], n_atoms: int, box, cutoff: float,
                 bond: Optional[np.ndarray] = None, scaler: Tuple[float, float] = (0.0, 1.0),
                 nbr_flavour: str = "jaxmd", device: int = 0, keep_stages: bool = False,
                 edge_capacity: int = 0, cfg: Optional[ModelConfig] = None, edge_dtype: str = "f32",
                 neighbor_skin: float = 0.0, self_loop_mode: str = "dgl07_noop", kernel_select: int = 0,
                 small_tile_limit: int = 0, n_boxes: int = 1):
        self._h = C.c_void_p()
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.GamdError("GamdForce needs a HIP device (torch.cuda.is_available() is False); "
                                 "there is no CPU fallback")
        cfg = cfg or infer_config(state_dict)
        # build_model's widths (nn_module.py:561-601): anything up to 256 / 256 / 256 — the library zero-pads to its 128-wide
        # blocks and normalises over the true widths (hidden_dim above 128: fp32 edge MLP only, the library says so)
        if (not 1 <= cfg.encoding_size <= 256 or not 1 <= cfg.edge_embedding_dim <= 256 or not 1 <= cfg.hidden_dim <= 256
                or cfg.n_rbf not in (0, 40)):
            raise ValueError("the gfx950 kernels cover encoding_size / edge_embedding_dim / hidden_dim up to 256 "
                             "and the RBF expansion on (40 centres) or off "
                             f"(got enc={cfg.encoding_size} hidden={cfg.hidden_dim} edge={cfg.edge_embedding_dim} "
                             f"n_rbf={cfg.n_rbf})")
        validate_state_dict(state_dict, cfg)
        self.cfg = cfg
        self.n = int(n_atoms)                          # atoms per box
        self.n_boxes = max(1, int(n_boxes))
        self.n_total = self.n * self.n_boxes
        self.device = torch.device("cuda", device)
        self.box = _box3(box)                          # constructor box (every box starts with it)
        self.cutoff = float(cutoff)
        c = GamdConfig()
        c.n_boxes = self.n_boxes
        c.n_atoms, c.kind, c.n_layers = self.n, KIND[cfg.kind], cfg.conv_layer
        c.use_bond, c.nbr_flavour, c.device = int(cfg.use_bond), FLAVOUR[nbr_flavour], device
        c.cutoff = self.cutoff
        for d in range(3):
            c.box[d] = float(self.box[d])
        c.edge_capacity, c.keep_stages = int(edge_capacity), int(keep_stages)
        c.edge_dtype = {"f32": 0, "bf16": 1, "f16x3": 2}[edge_dtype]
        c.encoding_size, c.edge_embedding_dim, c.hidden_dim = cfg.encoding_size, cfg.edge_embedding_dim, cfg.hidden_dim
        c.no_expand_edge = int(cfg.n_rbf == 0)
        c.neighbor_skin = float(neighbor_skin)      # > 0: Verlet-skin reuse (jax-md uses cutoff/6, graph_utils.py:24)
        if self_loop_mode not in SELF_LOOP:
            raise ValueError(f"self_loop_mode must be one of {sorted(SELF_LOOP)}")
        c.self_loop_mode = SELF_LOOP[self_loop_mode]
        c.kernel_select, c.small_tile_limit = int(kernel_select), int(small_tile_limit)
        self.edge_dtype = edge_dtype
        check(self._lib.gamd_create(C.byref(c), C.byref(self._h)), "gamd_create")
        self.keep_stages = keep_stages
        for name, t in state_dict.items():
            if name.endswith("num_batches_tracked"):      # BatchNorm's step counter: not used at inference
                continue
            a = np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32))
            shape = (C.c_int64 * a.ndim)(*a.shape)
            check(self._lib.gamd_load_weight(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim),
                  f"gamd_load_weight({name})")
        check(self._lib.gamd_finalize_weights(self._h), "gamd_finalize_weights")
        self.set_scaler(*scaler)
        if cfg.use_bond:
            if bond is None:
                raise ValueError("use_bond model needs the bond list")
            b = np.ascontiguousarray(np.asarray(bond, dtype=np.int32))
            check(self._lib.gamd_set_bonds(self._h, b.ctypes.data_as(C.c_void_p), b.shape[0]), "gamd_set_bonds")
        self._feat = None
        self._out = torch.empty((self.n_total, 3), dtype=torch.float32, device=self.device)
        self._out_den = torch.empty((self.n_total, 3), dtype=torch.float32, device=self.device)
        self.last_status = 0

    # -- lifetime -----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.gamd_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration -------------------------------------------------------------------------
    def set_scaler(self, mean, var):
        """load_training_stats (LJ/train_network_lj.py:119-123): mean/var of scaler.npz."""
        self.scaler_mean = np.asarray(mean, dtype=np.float64).reshape(-1)[:1]
        self.scaler_var = np.asarray(var, dtype=np.float64).reshape(-1)[:1]
        check(self._lib.gamd_set_scaler(self._h, float(self.scaler_mean[0]), float(self.scaler_var[0])),
              "gamd_set_scaler")

    # -- helpers ---------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev_pos(self, pos: ArrayLike) -> torch.Tensor:
        if isinstance(pos, np.ndarray):
            pos = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32))
        pos = pos.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(pos.shape) == (self.n_boxes, self.n, 3):
            pos = pos.view(self.n_total, 3)
        if tuple(pos.shape) != (self.n_total, 3):
            raise ValueError(f"pos must be [{self.n_total}, 3]" + (f" or [{self.n_boxes}, {self.n}, 3]" if self.n_boxes > 1 else "")
                             + f", got {tuple(pos.shape)}")
        return pos

    def _md_state(self, *ts):
        for t in ts:
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                    and tuple(t.shape) in ((self.n_total, 3), (self.n_boxes, self.n, 3))):
                raise ValueError(f"x, v, f must be contiguous float32 CUDA tensors of shape [{self.n_total}, 3]")

    def _dev_species(self, species) -> Optional[torch.Tensor]:
        """species / node feature [N] or [N,1] -> uint8 O=1/H=0 flags on the device (what the integrators pick masses
        by).  A floating-point input is ALSO handed to the library as the float node feature the reference feeds to
        node_encoder (nn_module.py:554): it need not be 0/1."""
        if species is None:
            self._set_features(None)
            return None
        if isinstance(species, np.ndarray):
            species = torch.from_numpy(species)
        # Host-side input (what the drivers pass): the device copy is kept by the engine and reused while the content stays the
        # same.  The library reads it from kernels that may still be in flight when an asynchronous md_run returns, so it must not
        # die with this call's locals; and a stable pointer lets the library skip its O,H,H layout check (a device -> host copy
        # and a stream synchronisation) on every call after the first.
        key = None
        if not species.is_cuda:
            c = species.detach().reshape(-1).contiguous()
            # (bytes through a uint8 view: dtypes numpy does not know, bfloat16, hash like any other)
            key = (str(c.dtype), c.numel(), hash(c.view(torch.uint8).numpy().tobytes()), torch.cuda.current_stream(self.device).cuda_stream)
            hit = getattr(self, "_species_cache", None)
            if hit is not None and hit[0] == key:
                self._set_features(hit[2])
                return hit[1]
        s = species.reshape(-1).to(device=self.device)
        if s.numel() == self.n and self.n_boxes > 1:
            s = s.repeat(self.n_boxes)                    # one box's species, the same for every box
        if s.numel() != self.n_total:
            raise ValueError("species must have one entry per atom")
        feat = s.to(torch.float32).contiguous() if s.dtype.is_floating_point and self.cfg.kind != "lj" else None
        self._set_features(feat)
        flags = (s != 0).to(torch.uint8).contiguous()
        # (a device tensor of the caller's is the caller's to keep alive; the flags derived from it are held until the next call)
        # The library skips its O,H,H layout check while the species POINTER is the one it validated last: new content must never
        # arrive at an address it has validated for other content.  The flags above were allocated while the previous buffer was
        # still alive, and the previous generation stays alive one change longer, so three consecutive generations are distinct.
        self._species_prev = getattr(self, "_species_cache", None)
        self._species_cache = (key, flags, feat)
        return flags

    def _set_features(self, feat: Optional[torch.Tensor]) -> None:
        if feat is None and self._feat is None:
            return
        self._feat = feat                             # keeps the device buffer alive while the library points at it
        check(self._lib.gamd_set_node_features(self._h, C.c_void_p(feat.data_ptr()) if feat is not None else None),
              "gamd_set_node_features")

    def _box_arg(self, box):
        b = _boxes(self.box if box is None else box, self.n_boxes)
        return (C.c_float * (3 * self.n_boxes))(*[float(x) for x in b.reshape(-1)])

    # -- the hot path ----------------------------------------------------------------------------
    def forward(self, pos: ArrayLike, box=None, species=None, denormalize: bool = False,
                inplace: bool = False) -> torch.Tensor:
        """pos [N,3] (any periodic image), box scalar/[3] (default: constructor box), species [N]
        (O=1/H=0, or the float node feature of the water models; ignored for LJ) -> network output [N,3] fp32 on
        the device, in the caller's atom order.  Normalised like ``pnet_model(...)`` unless ``denormalize`` (then
        fp32 out*sqrt(var)+mean).  Returns a FRESH tensor like the reference's ``pnet_model(...)``; ``inplace=True``
        returns the engine's persistent output buffer instead (overwritten by the next call: for MD loops)."""
        p = self._dev_pos(pos)
        s = self._dev_species(species)
        st = self._lib.gamd_forces(self._h, C.c_void_p(p.data_ptr()),
                                   C.c_void_p(s.data_ptr()) if s is not None else None,
                                   self._box_arg(box), C.c_void_p(self._out.data_ptr()),
                                   C.c_void_p(self._out_den.data_ptr()), self._stream())
        self.last_status = check(st, "gamd_forces")
        out = self._out_den if denormalize else self._out
        return out if inplace else out.clone()

    __call__ = forward

    def forward_host(self, pos: np.ndarray, box=None, species=None, denormalize: bool = False) -> np.ndarray:
        """The reference's host-array boundary (``predict_forces``: numpy positions in, numpy forces out,
        LJ/train_network_lj.py:133-157) through ``gamd_forces_host``: float64 -> float32 as ``torch.from_numpy(pos).float()``
        rounds, the library's pinned staging buffers both ways, copy in / kernels / copy out enqueued on the caller's stream
        and ONE synchronisation (the library replays the call if a neighbour buffer had to be regrown: ``last_status`` 1).
        Returns a float32 [N,3] array owned by the engine: valid until the next call."""
        pos = np.asarray(pos)
        if pos.shape == (self.n_boxes, self.n, 3):
            pos = pos.reshape(self.n_total, 3)
        if pos.shape != (self.n_total, 3):
            raise ValueError(f"pos must be [{self.n_total}, 3], got {tuple(pos.shape)}")
        p32 = np.ascontiguousarray(pos, dtype=np.float32)
        if getattr(self, "_host_out", None) is None:
            self._host_out = np.empty((self.n_total, 3), dtype=np.float32)
        s = self._dev_species(species)
        st = self._lib.gamd_forces_host(self._h, p32.ctypes.data_as(C.c_void_p), C.c_void_p(s.data_ptr()) if s is not None else None,
                                        self._box_arg(box), self._host_out.ctypes.data_as(C.c_void_p), 1 if denormalize else 0,
                                        self._stream())
        self.last_status = check(st, "gamd_forces_host")
        return self._host_out

    def forward_edges(self, pos: ArrayLike, edge_idx, box=None, species=None, denormalize: bool = False,
                      inplace: bool = False) -> torch.Tensor:
        """Model-level call of the reference, ``pnet_model([pos], [edge_idx])``: edge_idx [2,E] with row 0 =
        centre, row 1 = neighbour (LJ/train_network_lj.py:183-184); the built-in radius search is bypassed.
        Returns a fresh tensor unless ``inplace``."""
        p = self._dev_pos(pos)
        s = self._dev_species(species)
        if isinstance(edge_idx, np.ndarray):
            edge_idx = torch.from_numpy(edge_idx)
        e = edge_idx.to(device=self.device, dtype=torch.int32).contiguous()
        if e.dim() != 2 or e.shape[0] != 2:
            raise ValueError("edge_idx must be [2, E]")
        st = self._lib.gamd_forces_edges(self._h, C.c_void_p(p.data_ptr()),
                                         C.c_void_p(s.data_ptr()) if s is not None else None, self._box_arg(box),
                                         C.c_void_p(e[0].data_ptr()), C.c_void_p(e[1].data_ptr()), int(e.shape[1]),
                                         C.c_void_p(self._out.data_ptr()), C.c_void_p(self._out_den.data_ptr()),
                                         self._stream())
        self.last_status = check(st, "gamd_forces_edges")
        out = self._out_den if denormalize else self._out
        return out if inplace else out.clone()

    def build_neighbors(self, pos: ArrayLike, box=None, species=None) -> int:
        p = self._dev_pos(pos)
        s = self._dev_species(species)
        st = self._lib.gamd_build_neighbors(self._h, C.c_void_p(p.data_ptr()),
                                            C.c_void_p(s.data_ptr()) if s is not None else None,
                                            self._box_arg(box), self._stream())
        return check(st, "gamd_build_neighbors")

    def counts(self) -> Tuple[int, int, int]:
        e, p, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(self._lib.gamd_get_counts(self._h, C.byref(e), C.byref(p), C.byref(c)), "gamd_get_counts")
        return e.value, p.value, c.value

    def skin_stats(self) -> Tuple[int, int, int]:
        """(candidate-list rebuilds so far, candidates in the last rebuilt list, candidate capacity)."""
        r, c, cap = C.c_int64(), C.c_int64(), C.c_int64()
        check(self._lib.gamd_get_skin_stats(self._h, C.byref(r), C.byref(c), C.byref(cap)), "gamd_get_skin_stats")
        return r.value, c.value, cap.value

    # -- stage getters for parity tests ----------------------------------------------------------
    def _dbg(self, what: int, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        check(self._lib.gamd_debug_get(self._h, what, out.ctypes.data_as(C.c_void_p), out.nbytes), "gamd_debug_get")
        return out

    def debug_partial(self) -> np.ndarray:
        """[pieces, H] partial-sum pieces of the LAST conv layer (one row per run of edges with the same destination inside a
        16-edge chunk), CSR order; H padded to whole 128-blocks.  A piece holds the sum of its edges' messages hn[src] * e_emb
        -- always in the bf16 and split-fp16 modes, and in fp32 for every layer but one: layer 0 in its hoisted form (the
        library's l0_hoist: an LJ model, fp32 edge MLP, 128 / 128 / 128 widths, no update_edge_emb, not under
        KSEL_NO_LAYER0_HOIST), which is the LAST layer only in a one-layer model.  There the pieces hold sums of T3 rows, the
        third GEMM's activated output, and phi_edge's part is applied per atom by the node kernel (M0 sum T3 + d_i c0)."""
        return self._dbg(6, (self.counts()[1], 128 * ((self.cfg.encoding_size + 127) // 128)), np.float32)

    def debug_perm(self) -> np.ndarray:
        return self._dbg(0, (self.n_total,), np.int32)

    def debug_csr(self) -> Tuple[np.ndarray, np.ndarray]:
        e = self.counts()[0]
        return self._dbg(1, (self.n_total + 1,), np.int32), self._dbg(2, (e,), np.int32)

    def debug_edges(self) -> np.ndarray:
        """[2,E] (centre, neighbour) in ORIGINAL atom ids (box-major over all boxes), CSR order.  The padding slots that
        align the boxes of a batch (source index n_total) are not edges and are left out."""
        perm = self.debug_perm().astype(np.int64)
        row_ptr, col = self.debug_csr()
        dst = np.repeat(np.arange(self.n_total), np.diff(row_ptr))
        real = col < self.n_total
        return np.stack([perm[dst[real]], perm[col[real]]])

    def debug_edge_rows(self) -> np.ndarray:
        """CSR slots that hold real edges (bool [E]): the rows of debug_e / debug_feat that debug_edges lists."""
        return self.debug_csr()[1] < self.n_total

    def debug_e(self) -> np.ndarray:
        """e [E, edge_embedding_dim] de-fragmented to CSR edge order.  Needs keep_stages=True (or KSEL_NO_LN_FOLD) where the
        fp32 128-wide kernels fold the edge LayerNorm into the conv layers: e is then never formed and the library refuses."""
        e = self.counts()[0]
        nt = (e + 31) // 32
        nb = (self.cfg.edge_embedding_dim + 127) // 128               # widths below a 128-block are zero-padded on the device
        if self.edge_dtype in ("f16x3", "bf16"):
            # operand-form fragments: [tile][block][t][u][hi | lo][lane][8 halves] (split-fp16: the value is hi + lo) or
            # [tile][block][t][u][lane][8 bf16]; K step (t, u) value j of lane (slot, half) is feature
            # 128 block + 32 t + (r & 3) + 8 (r >> 2) + 4 half with r = 8 u + j
            raw = self._dbg(3, (nt, nb, 4096), np.float32)
            if self.edge_dtype == "f16x3":
                v = raw.view(np.float16).reshape(nt, nb, 4, 2, 2, 64, 8).astype(np.float32)
                val = v[:, :, :, :, 0] + v[:, :, :, :, 1]
            else:
                u16 = raw.reshape(-1).view(np.uint16)[:nt * nb * 4096].reshape(nt, nb, 4, 2, 64, 8)       # 8 KiB per (tile, block), dense
                val = (u16.astype(np.uint32) << 16).view(np.float32)
            lane = np.arange(64)
            slot, half = lane & 31, lane >> 5
            pi = 16 * ((slot >> 2) & 1) + (slot & 3) + 4 * (slot >> 3)
            rows = (np.arange(nt)[:, None] * 32 + pi[None, :])
            out = np.zeros((nt * 32, 128 * nb), dtype=np.float32)
            for blk in range(nb):
                for t in range(4):
                    for u in range(2):
                        for j in range(8):
                            r = 8 * u + j
                            feat = 128 * blk + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half
                            out[rows, feat[None, :]] = val[:, blk, t, u, :, j]
            return out[:e, :self.cfg.edge_embedding_dim]
        frag = self._dbg(3, (nt, nb, 4, 4, 64, 4), np.float32)
        lane = np.arange(64)
        slot, half = lane & 31, lane >> 5
        pi = 16 * ((slot >> 2) & 1) + (slot & 3) + 4 * (slot >> 3)
        out = np.zeros((nt * 32, 128 * nb), dtype=np.float32)
        rows = (np.arange(nt)[:, None] * 32 + pi[None, :])
        for b in range(nb):
            for t in range(4):
                for q in range(4):
                    for j in range(4):
                        feat = 128 * b + 32 * t + 8 * q + 4 * half + j           # per lane
                        out[rows, feat[None, :]] = frag[:, b, t, q, :, j]
        return out[:e, :self.cfg.edge_embedding_dim]

    def debug_feat(self, n_feat: int) -> np.ndarray:
        e = self.counts()[0]
        return self._dbg(4, (e, 48), np.float32)[:, :n_feat]

    def debug_h(self, layer: int) -> np.ndarray:
        """residual stream h_layer [N, encoding_size] in ORIGINAL atom order."""
        hp = 128 * ((self.cfg.encoding_size + 127) // 128)
        hs = self._dbg(16 + layer, (self.n_total, hp), np.float32)[:, :self.cfg.encoding_size]
        out = np.empty_like(hs)
        out[self.debug_perm()] = hs
        return out

    # -- on-device MD (split BAOAB of hack_integrator.py) ----------------------------------------
    def md_run(self, x: torch.Tensor, v: torch.Tensor, f: torch.Tensor, n_steps: int, dt_ps=0.002,
               mass_amu=39.9, temperature_k=100.0, gamma_per_ps=25.0, seed=0, first_step=0,
               box=None, species=None, sync: bool = True, mass_h_amu=0.0, length_per_nm=0.0,
               rigid_water: bool = False, r_oh=0.0, r_hh=0.0, remove_cm_motion: Optional[bool] = None) -> None:
        """Advance (x, v, f) in place by n_steps; f holds denormalised forces (kJ/mol/nm) at x.

        Water: ``mass_amu`` is the oxygen mass and ``mass_h_amu`` the mass of the species-0 atoms;
        ``rigid_water`` holds every O,H,H triple rigid at (r_oh, r_hh) like OpenMM's constrained water
        (positions must then be whole molecules; they are kept whole).  ``length_per_nm`` is the length
        unit of x/v/box (10 = Angstrom, the default; 18.8972613 = bohr for the DFT model).
        ``remove_cm_motion``: subtract the centre-of-mass velocity at the top of every step like the CMMotionRemover that
        hack_integrator.py:142 runs when the OpenMM System has one; default True with ``rigid_water`` (the water drivers'
        openmmtools WaterBox carries one), False otherwise (the LJ fluid does not).
        With the classical force source (``md_force_source("classical")``) ``f`` must hold the classical forces at ``x`` on
        entry: ``classical_forces(x)[0].float()``; with the water source (``md_force_source("water_classical")``, which
        needs ``rigid_water``) ``water_classical_forces(x, species)[0].float()``."""
        self._md_state(x, v, f)
        s = self._dev_species(species)
        if remove_cm_motion is None:
            remove_cm_motion = bool(rigid_water)
        p = GamdMdParams(dt_ps, mass_amu, temperature_k, gamma_per_ps, seed, first_step, mass_h_amu, length_per_nm,
                         int(rigid_water), r_oh, r_hh, int(bool(remove_cm_motion)))
        st = self._lib.gamd_md_run(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(v.data_ptr()),
                                   C.c_void_p(f.data_ptr()), C.c_void_p(s.data_ptr()) if s is not None else None,
                                   self._box_arg(box), C.byref(p), int(n_steps), self._stream())
        check(st, "gamd_md_run")
        if sync:
            self.last_status = check(self._lib.gamd_sync_status(self._h, self._stream()), "gamd_sync_status")

    def md_run_nhc(self, x: torch.Tensor, v: torch.Tensor, f: torch.Tensor, n_steps: int, chain_state: torch.Tensor = None,
                   dt_ps=0.002, mass_amu=39.9, temperature_k=100.0, frequency_per_ps=25.0, chain_length=10, num_mts=5,
                   num_yoshidasuzuki=5, ndf=None, box=None, species=None, sync: bool = True, mass_h_amu=0.0,
                   length_per_nm=0.0, rigid_water: bool = False, r_oh=0.0, r_hh=0.0,
                   remove_cm_motion: Optional[bool] = None) -> torch.Tensor:
        """Split Nose-Hoover-chain steps (hack_integrator.py:182-493).  Returns the chain state tensor
        (float64 [3*chain_length+2] on the device); pass it back in to continue a trajectory.
        Several boxes: one chain per box (state [n_boxes, 3*chain_length+2]), ``ndf`` is per box.
        ``ndf`` defaults to what hack_integrator.py:226-235 computes from the OpenMM System: 3 per particle, minus the
        constraints (three per rigid molecule), minus 3 when the System holds a CMMotionRemover.
        ``remove_cm_motion`` says whether it does: default True with ``rigid_water`` (the water drivers build an
        openmmtools WaterBox, whose System carries one), False otherwise (the LJ drivers' ndf is 3N).  When it does, the
        centre-of-mass velocity is also subtracted on the device where hack_integrator.py:271-272 does it: behind
        propagateNHC() of the first half (the chain sees the velocities as they are), in front of the kick.
        With the classical force source (``md_force_source("classical")``) ``f`` must hold the classical forces at ``x`` on
        entry: ``classical_forces(x)[0].float()``; with the water source (``md_force_source("water_classical")``, which
        needs ``rigid_water``) ``water_classical_forces(x, species)[0].float()``."""
        self._md_state(x, v, f)
        reset = chain_state is None
        if reset:
            shape = (3 * chain_length + 2,) if self.n_boxes == 1 else (self.n_boxes, 3 * chain_length + 2)
            chain_state = torch.zeros(shape, dtype=torch.float64, device=self.device)
        assert chain_state.dtype == torch.float64 and chain_state.is_contiguous() \
            and chain_state.numel() == self.n_boxes * (3 * chain_length + 2)
        s = self._dev_species(species)
        if remove_cm_motion is None:
            remove_cm_motion = bool(rigid_water)
        if ndf is None:
            ndf = (2 * self.n if rigid_water else 3 * self.n) - (3 if remove_cm_motion else 0)
        p = GamdNhcParams(dt_ps, mass_amu, temperature_k, frequency_per_ps, chain_length, num_mts, num_yoshidasuzuki,
                          int(reset), float(ndf),
                          mass_h_amu, length_per_nm, int(rigid_water), r_oh, r_hh, int(bool(remove_cm_motion)))
        st = self._lib.gamd_md_run_nhc(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(v.data_ptr()),
                                       C.c_void_p(f.data_ptr()), C.c_void_p(s.data_ptr()) if s is not None else None,
                                       self._box_arg(box), C.byref(p), C.c_void_p(chain_state.data_ptr()), int(n_steps),
                                       self._stream())
        check(st, "gamd_md_run_nhc")
        if sync:
            self.last_status = check(self._lib.gamd_sync_status(self._h, self._stream()), "gamd_sync_status")
        return chain_state

    # -- force source of md_run / md_run_nhc (the classical run next to the GNN run) ---------------------------------
    def md_force_source(self, source: str) -> None:
        """Where the forces of ``md_run`` / ``md_run_nhc`` come from: ``"network"`` (the default) or ``"classical"``, the
        Lennard-Jones potential of the last ``classical_configure`` (interval 0 will do), evaluated on all pairs in double
        on the device at every step and rounded to fp32 into ``f`` — bit for bit ``classical_forces(x)[0].float()``.  Sticky
        until set again; ``forward`` and the other force calls evaluate the network whatever the source.  Integrators,
        observers, skin mode, several boxes and the overflow resume work as in a network-driven run.  LJ models only;
        2 r_cut must not exceed a box edge.  Replaces the OpenMM run of the reference's data generator
        (dataset/generate_lj_data.py:74-107).  O(N^2) per step and box.

        ``"water_classical"`` (water models only) is the same under the water potential of the last
        ``water_classical_configure`` (interval 0 will do; 3-site, or 4-site with its ``m_site``): O-O Lennard-Jones plus a plain Ewald sum, bit for bit
        ``water_classical_forces(x, species)[0].float()``.  A run then needs ``rigid_water`` (the potential has no bond
        or angle term), ``species``, and 2 r_cut below every box edge.  Replaces the OpenMM run of
        dataset/generate_tip3p_data.py:76-103.  O(N^2 + N K) per step and box, K the k-vectors of the Ewald sum."""
        table = {**_lib.FORCE_SOURCE, **_lib.WATER_FORCE_SOURCE}
        if source not in table:
            raise ValueError(f"source must be one of {sorted(table)}")
        check(self._lib.gamd_md_force_source(self._h, table[source]), "gamd_md_force_source")
        self._force_source = source

    @property
    def force_source(self) -> str:
        """The force source of ``md_run`` / ``md_run_nhc`` as last set: ``"network"``, ``"classical"`` or
        ``"water_classical"``."""
        return getattr(self, "_force_source", "network")

    # -- run reporter (the drivers' StateDataReporter log and a g(r) histogram, taken inside enqueued runs) ----------
    def report_configure(self, interval: int, max_samples: int = 0, ndf: Optional[float] = None, rdf_bins: int = 0,
                         rdf_rmax: float = 0.0, exclude_same_molecule: bool = False, rigid_water: bool = False,
                         remove_cm_motion: Optional[bool] = None) -> None:
        """While configured, every ``interval``-th completed step of md_run / md_run_nhc (counted across calls) logs the
        kinetic energy per box on the device and, with ``rdf_bins`` > 0, adds the frame's pair distances below ``rdf_rmax``
        (default and at most: the cutoff) to a histogram; ``report_read`` fetches both.  ``interval`` = 0 switches it off.
        ``ndf`` (degrees of freedom per box, for the temperature) defaults as md_run_nhc's does: 3 per atom, 6 per rigid
        molecule (``rigid_water``), 3 fewer with ``remove_cm_motion`` (default: True with ``rigid_water``).
        Replaces ``simulation.reporters.append(StateDataReporter(file, 100, step=True, time=True, kineticEnergy=True,
        temperature=True))`` of the rollout drivers (LJ/test_script/test_langevin.py:79-83)."""
        if remove_cm_motion is None:
            remove_cm_motion = bool(rigid_water)
        if ndf is None:
            ndf = (2 * self.n if rigid_water else 3 * self.n) - (3 if remove_cm_motion else 0)
        p = GamdReportParams(int(interval), int(max_samples), float(ndf), int(rdf_bins), float(rdf_rmax),
                             int(bool(exclude_same_molecule)), 0)
        check(self._lib.gamd_report_configure(self._h, C.byref(p)), "gamd_report_configure")
        if interval:
            self._report_rmax = float(np.float32(rdf_rmax)) if rdf_rmax else float(np.float32(self.cutoff))

    def report_reset(self) -> None:
        """Step count, log and histogram back to zero; the configuration stays."""
        check(self._lib.gamd_report_reset(self._h), "gamd_report_reset")

    def report_read(self) -> "RunReport":
        """Synchronise and fetch what the reporter has recorded since it was configured or reset."""
        n_rows, frames, dropped = C.c_int64(), C.c_int64(), C.c_int64()
        dims = (C.c_int32 * 3)()
        rd = self._lib.gamd_report_read
        check(rd(self._h, self._stream(), None, None, None, 0, C.byref(n_rows), None, 0, C.byref(frames), C.byref(dropped), dims),
              "gamd_report_read")
        rows, (nb, npair, nbins) = n_rows.value, dims
        steps = np.zeros(rows, dtype=np.int64)
        ke = np.zeros((rows, nb), dtype=np.float64)
        temp = np.zeros((rows, nb), dtype=np.float64)
        counts = np.zeros((nb, npair, nbins), dtype=np.uint64)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        check(rd(self._h, self._stream(), vp(steps), vp(ke), vp(temp), rows, C.byref(n_rows), vp(counts), counts.size,
                 C.byref(frames), C.byref(dropped), dims), "gamd_report_read")
        return RunReport(steps, ke, temp, counts, frames.value, dropped.value, getattr(self, "_report_rmax", 0.0),
                         np.prod(_boxes(self.box, self.n_boxes).astype(np.float64), axis=1))

    # -- run recorder (trajectory frames, image counters, MSD / VACF, taken inside enqueued runs) ---------------------
    def traj_configure(self, interval: int, max_frames: int = 0, fields: Sequence[str] = ("x",), n_lags: int = 0,
                       subtract_com: bool = False) -> None:
        """While configured, every ``interval``-th completed step of md_run / md_run_nhc (counted across calls) keeps a
        frame of the ``fields`` (any of "x", "v", "f", "image") on the device, up to ``max_frames`` frames, and with
        ``n_lags`` > 0 adds to the mean-squared-displacement and velocity-autocorrelation sums for the lags
        0 .. n_lags - 1 (in units of ``interval``), every sample a time origin; ``traj_read`` fetches both.
        ``subtract_com``: displacements relative to the box's centre of mass.  ``interval`` = 0 switches it off.
        Replaces the ``getState`` / ``np.savez`` loop of the data generators (dataset/generate_lj_data.py:93-107)."""
        bits = 0
        for name in ((fields,) if isinstance(fields, str) else fields):
            if name not in TRAJ_FIELDS:
                raise ValueError(f"fields must be among {sorted(TRAJ_FIELDS)}, got {name!r}")
            bits |= TRAJ_FIELDS[name]
        p = GamdTrajParams(int(interval), int(max_frames), bits, int(n_lags), int(bool(subtract_com)), 0)
        check(self._lib.gamd_traj_configure(self._h, C.byref(p)), "gamd_traj_configure")
        if interval:
            self._traj_cfg = (int(interval), bits)

    def traj_reset(self) -> None:
        """Step count, frames, image counters, ring and sums back to zero; the configuration stays."""
        check(self._lib.gamd_traj_reset(self._h), "gamd_traj_reset")

    def traj_read(self) -> "RunTrajectory":
        """Synchronise and fetch what the recorder has kept since it was configured or reset."""
        interval, bits = getattr(self, "_traj_cfg", (1, 0))
        n_frames, dropped, n_samples, amb = C.c_int64(), C.c_int64(), C.c_int64(), C.c_uint64()
        dims = (C.c_int32 * 3)()
        st = self._stream()
        check(self._lib.gamd_traj_read_frames(self._h, st, 0, 0, None, None, None, None, None, C.byref(n_frames), C.byref(dropped)),
              "gamd_traj_read_frames")
        check(self._lib.gamd_traj_read_dynamics(self._h, st, None, None, 0, C.byref(n_samples), C.byref(amb), None, dims),
              "gamd_traj_read_dynamics")
        fr, (nb, ncls, nlags) = n_frames.value, dims
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        shape = (fr, self.n_boxes, self.n, 3)
        steps = np.zeros(fr, dtype=np.int64)
        x, v, f = (np.zeros(shape, dtype=np.float32) if bits & TRAJ_FIELDS[k] else None for k in ("x", "v", "f"))
        image = np.zeros(shape, dtype=np.int32) if bits & TRAJ_FIELDS["image"] else None
        check(self._lib.gamd_traj_read_frames(self._h, st, 0, fr, vp(steps), vp(x), vp(v), vp(f), vp(image), C.byref(n_frames),
                                              C.byref(dropped)), "gamd_traj_read_frames")
        msd = np.zeros((nb, ncls, nlags), dtype=np.float64)
        vacf = np.zeros((nb, ncls, nlags), dtype=np.float64)
        cls_atoms = np.zeros((nb, ncls), dtype=np.int64)
        check(self._lib.gamd_traj_read_dynamics(self._h, st, vp(msd), vp(vacf), msd.size, C.byref(n_samples), C.byref(amb),
                                                vp(cls_atoms), dims), "gamd_traj_read_dynamics")
        return RunTrajectory(steps, x, v, f, image, dropped.value, amb.value, n_samples.value, cls_atoms, msd, vacf, interval)

    # -- structure sampler (all-pairs g(r) out to half the box and S(k), taken inside enqueued runs) --------------------
    def structure_configure(self, interval: int, rdf_bins: int = 0, rdf_rmax: Optional[float] = None,
                            exclude_same_molecule: bool = False, sk_n2max: int = 0) -> None:
        """While configured, every ``interval``-th completed step of md_run / md_run_nhc (counted across calls, by a counter
        of its own) adds every pair distance of the frame below ``rdf_rmax`` to a histogram of ``rdf_bins`` bins (default
        ``rdf_rmax``: half the shortest edge of the engine's box, which is also the most a run accepts) and, with
        ``sk_n2max`` > 0, Re(rho_a conj(rho_b)) at every wave vector 2 pi n / L with 0 < |n|^2 <= ``sk_n2max``;
        ``structure_read`` fetches both.  O(N^2) pair distances per sample and box.  ``interval`` = 0 switches it off."""
        if rdf_rmax is None:
            rdf_rmax = float(np.float32(0.5) * self.box.min())
        p = GamdStructParams(int(interval), int(rdf_bins), float(rdf_rmax), int(bool(exclude_same_molecule)), int(sk_n2max))
        check(self._lib.gamd_struct_configure(self._h, C.byref(p)), "gamd_struct_configure")
        if interval:
            self._struct_rmax = float(np.float32(rdf_rmax))

    def structure_reset(self) -> None:
        """Step count, histogram and sums back to zero; the configuration stays."""
        check(self._lib.gamd_struct_reset(self._h), "gamd_struct_reset")

    def structure_read(self, box=None) -> "RunStructure":
        """Synchronise and fetch what the structure sampler has accumulated since it was configured or reset.  ``box``: the
        box edges the runs used when they differ from the constructor's (|k| and the g(r) volume are taken from them)."""
        frames = C.c_int64()
        dims = (C.c_int32 * 4)()
        rd = self._lib.gamd_struct_read
        check(rd(self._h, self._stream(), None, 0, None, 0, None, 0, C.byref(frames), dims), "gamd_struct_read")
        nb, npair, nbins, nk = dims
        counts = np.zeros((nb, npair, nbins), dtype=np.uint64)
        sk = np.zeros((nb, npair, nk), dtype=np.float64)
        kvec = np.zeros((nk, 3), dtype=np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        check(rd(self._h, self._stream(), vp(counts), counts.size, vp(sk), sk.size, vp(kvec), kvec.size, C.byref(frames), dims),
              "gamd_struct_read")
        boxes = _boxes(self.box if box is None else box, self.n_boxes).astype(np.float64)
        return RunStructure(counts, sk, kvec, frames.value, getattr(self, "_struct_rmax", 0.0), boxes)

    # -- classical observer (the LJ potential energy, virial and force error on sampled frames; classical force labels) ---
    def classical_configure(self, interval: int, max_samples: int = 0, sigma: float = 3.4, epsilon: float = 0.238 * KJ_PER_KCAL,
                            r_cut: Optional[float] = None, r_switch: Optional[float] = None, shift: bool = True,
                            cells: bool = False) -> None:
        """While configured, every ``interval``-th completed step of md_run / md_run_nhc (counted across calls, by a counter
        of its own) evaluates the switched, shifted Lennard-Jones potential on all pairs of every box in double on the
        device and logs the potential energy, the virial, the pair count and the error sums of the run's (network) forces
        against the classical forces; ``classical_read`` fetches the rows.  ``interval`` = 0 switches the observer off but
        still takes the parameters, which ``classical_forces`` uses.  LJ models only.

        ``sigma``, ``r_cut``, ``r_switch`` are in the engine's length unit, ``epsilon`` in kJ/mol.  ``r_cut`` defaults to
        3 sigma and ``r_switch`` to r_cut - sigma (0: no switching); ``shift`` subtracts u_LJ(r_cut).  The defaults (sigma =
        3.4 Angstrom, epsilon = 0.238 kcal/mol, cutoff 3 sigma, switch width 3.4 Angstrom, shifted) are meant to be those of
        openmmtools' ``LennardJonesFluid(shift=True)`` behind the reference's data generator, but they were written down from
        memory and are UNVERIFIED: neither OpenMM nor openmmtools was available to compare against, and no long-range
        dispersion correction is applied.  Check them against your OpenMM system before comparing energies.

        ``cells`` walks the pairs over a per-box cell table instead of all against all: per evaluation the atoms are ordered
        by (cell, atom index), cells of edge >= r_cut / 2, and every atom tests the atoms of the 5 x 5 x 5 cells around its
        own (every cell of an axis that has fewer than five).  The pairs and the pair count are exactly the all-pairs walk's;
        the energy, the virial and the forces differ from it in the order of the sums only, within 1e-12 of their sums of
        absolute terms.  The same bits come back run after run, a driven frame still carries
        ``classical_forces(x)[0].float()`` and so does ``minimize``'s ``f``; the same atoms given in OTHER periodic images may
        change cells at a face and with them the order of the sums (same bound, not the same bits).  The observer,
        ``classical_forces``, the ``"classical"`` force source and ``minimize`` follow it.  The table costs six launches per
        evaluation; where it pays: profiles/run_classical_cells.md.  Every call states it: the default False is the all-pairs
        walk, bit for bit what it was.  ``classical_cells_table`` reads the table of the last evaluation."""
        r_cut = 3.0 * float(sigma) if r_cut is None else float(r_cut)
        r_switch = r_cut - float(sigma) if r_switch is None else float(r_switch)
        p = GamdClassicalParams(int(interval), int(max_samples), float(sigma), float(epsilon), r_cut, r_switch, int(bool(shift)), 0)
        check(self._lib.gamd_classical_configure(self._h, C.byref(p)), "gamd_classical_configure")
        if cells or getattr(self, "_classical_cells", False):       # (a handle that never had cells makes the calls it made)
            check(self._lib.gamd_classical_cells(self._h, int(bool(cells))), "gamd_classical_cells")
            self._classical_cells = bool(cells)
        self._classical_set = True
        self._classical_lj = dict(sigma=float(sigma), epsilon=float(epsilon), r_cut=r_cut, r_switch=r_switch, shift=bool(shift),
                                  length_per_nm=0.0)

    def classical_cells_table(self, box: int = 0):
        """Diagnostic: the cell table of box ``box`` as the last sample, ``classical_forces`` call, driven step or ``minimize``
        call left it (``cells=True``): (nc, start, order) as ``water_cells_table`` returns them.  Synchronises."""
        return self._cells_table("gamd_classical_cells_read", box)

    def classical_reset(self) -> None:
        """Step count and rows back to zero; parameters and configuration stay."""
        check(self._lib.gamd_classical_reset(self._h), "gamd_classical_reset")

    def _potential_read(self, entry: str, width: int, cls, forces: bool):
        """The rows, steps, drop count and (``forces``) last forces of an observer with a potential, through its read call
        ``entry`` (row width ``width``), as a ``cls``."""
        n_rows, dropped = C.c_int64(), C.c_int64()
        rd = getattr(self._lib, entry)
        check(rd(self._h, self._stream(), None, None, 0, C.byref(n_rows), C.byref(dropped), None, 0), entry)
        rows = n_rows.value
        steps = np.zeros(rows, dtype=np.int64)
        data = np.zeros((rows, self.n_boxes, width), dtype=np.float64)
        fcl = np.full((self.n_total, 3), np.nan, dtype=np.float64) if forces else None
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        check(rd(self._h, self._stream(), vp(steps), vp(data), rows, C.byref(n_rows), C.byref(dropped), vp(fcl),
                 0 if fcl is None else fcl.size), entry)
        return cls(steps, data, self.n, dropped.value, fcl)

    def classical_read(self, forces: bool = False) -> "RunClassical":
        """Synchronise and fetch what the classical observer has logged since it was configured or reset; ``forces``: also
        the classical forces of the last sample."""
        rc = self._potential_read("gamd_classical_read", _lib.CLASSICAL_ROW, RunClassical, forces)
        rc.lj = getattr(self, "_classical_lj", None)
        return rc

    def classical_forces(self, pos: ArrayLike, box=None, length_per_nm: float = 0.0):
        """The classical potential of the last ``classical_configure`` (with the defaults and interval 0 when there was
        none) on given positions, outside any run: (forces float64 [N, 3] on the device in kJ/mol/nm, energy [B], virial
        [B], pairs [B] as float64 arrays).  ``pos`` [N, 3] in any periodic image, fp32 as the library reads it; ``box`` as
        in ``forward``; ``length_per_nm`` the length unit (0 or 10 = Angstrom).  Synchronises once."""
        if not getattr(self, "_classical_set", False):
            self.classical_configure(0)
        p = self._dev_pos(pos)
        out = torch.empty((self.n_total, 3), dtype=torch.float64, device=self.device)
        e, w, c = (np.zeros(self.n_boxes, dtype=np.float64) for _ in range(3))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        check(self._lib.gamd_classical_eval(self._h, C.c_void_p(p.data_ptr()), self._box_arg(box), float(length_per_nm),
                                            C.c_void_p(out.data_ptr()), vp(e), vp(w), vp(c), self._stream()), "gamd_classical_eval")
        return out, e, w, c

    # -- energy minimiser (the drivers' minimizeEnergy in front of the first step) -------------------------------------
    def minimize(self, x: torch.Tensor, f: Optional[torch.Tensor] = None, tolerance: float = 10.0, max_iter: int = 0, box=None,
                 length_per_nm: float = 0.0, return_x64: bool = False, check_every: int = 0, **fire) -> "MinimizeResult":
        """Relax the positions ``x`` (float32 CUDA tensor, changed in place) of every box under the classical potential of the
        last ``classical_configure`` (with the defaults and interval 0 when there was none) on the device, until the root
        mean square of the 3N force components of a box is at most ``tolerance`` (kJ/mol/nm; the meaning of OpenMM's
        ``minimizeEnergy(tolerance)``) or ``max_iter`` position updates are done (0 = 10 000).  The algorithm is FIRE in
        double, not OpenMM's L-BFGS: no parity with it is claimed.  ``fire``: any of dt_start, dt_max, n_min, f_inc, f_dec,
        alpha_start, f_alpha, max_step (0 or absent: the default, include/gamd_hip.h; the defaults are for Angstrom).

        On return ``x`` holds the result rounded to fp32 and wrapped into the box and ``f`` (allocated when None) the
        classical forces at exactly that ``x`` — ``classical_forces(x)[0].float()`` bit for bit, what a classical-source
        ``md_run`` / ``md_run_nhc`` needs on entry.  A box that was not finite at the start (two atoms at one point) keeps its
        ``x``; nothing is written to ``f`` for a box that failed.  ``return_x64``: also the unrounded, unwrapped double
        positions (``result.x64``).  LJ models only; 2 r_cut must not exceed a box edge.  Synchronises."""
        unknown = set(fire) - {"dt_start", "dt_max", "n_min", "f_inc", "f_dec", "alpha_start", "f_alpha", "max_step"}
        if unknown:
            raise TypeError(f"minimize() got unexpected FIRE constants {sorted(unknown)}")
        if not getattr(self, "_classical_set", False):
            self.classical_configure(0)
        if f is None:
            f = torch.zeros_like(x)
        self._md_state(x, f)
        x64 = torch.empty((self.n_total, 3), dtype=torch.float64, device=self.device) if return_x64 else None
        g = lambda k: float(fire.get(k, 0.0))
        p = GamdMinimizeParams(float(tolerance), int(max_iter), int(check_every), g("dt_start"), g("dt_max"), g("f_inc"), g("f_dec"),
                               g("alpha_start"), g("f_alpha"), g("max_step"), int(fire.get("n_min", 0)), 0)
        rows = np.zeros((self.n_boxes, _lib.MINIMIZE_ROW), dtype=np.float64)
        st = check(self._lib.gamd_minimize(self._h, C.c_void_p(x.data_ptr()), self._box_arg(box), float(length_per_nm),
                                           C.c_void_p(f.data_ptr()), C.c_void_p(x64.data_ptr()) if return_x64 else None,
                                           C.byref(p), rows.ctypes.data_as(C.c_void_p), self._stream()), "gamd_minimize")
        return MinimizeResult(st, rows, x, f, x64)

    def minimize_lbfgs(self, x: torch.Tensor, f: Optional[torch.Tensor] = None, tolerance: float = 10.0, max_iter: int = 0, box=None,
                       length_per_nm: float = 0.0, return_x64: bool = False, check_every: int = 0, m: int = 0, c1: float = 0.0,
                       curv: float = 0.0, max_ls: int = 0, max_step: float = 0.0) -> "LbfgsResult":
        """``minimize`` with L-BFGS in place of FIRE: the same task, arguments and results (``x`` changed in place, ``f`` the
        classical forces at exactly that ``x``, ``classical_forces(x)[0].float()`` bit for bit; a failed box keeps its ``x``
        and ``f``), for the tolerances at which FIRE's iteration count is what costs (the rollout drivers'
        ``minimizeEnergy(1e-6)``).  A history of ``m`` pairs (1 .. 8, 0 = 6) shapes the direction, a backtracking line search
        (sufficient decrease ``c1``, 0 = 1e-4; ``max_ls`` halvings, 0 = 20) sizes the step, no atom moves further than
        ``max_step`` (0 = 0.1, the engine's length unit) in one trial, a pair enters the history when s.y > ``curv`` |s||y|
        (0 = 1e-10), and ``max_iter`` (0 = 10 000) bounds the pair evaluations.  OpenMM's minimiser is L-BFGS too, but the line
        search and the stopping rule here are this library's own: no parity with OpenMM is claimed.  tests/lbfgs_ref.py is the
        recipe in float64.  LJ models only; 2 r_cut must not exceed a box edge.  Synchronises."""
        if not getattr(self, "_classical_set", False):
            self.classical_configure(0)
        if f is None:
            f = torch.zeros_like(x)
        self._md_state(x, f)
        x64 = torch.empty((self.n_total, 3), dtype=torch.float64, device=self.device) if return_x64 else None
        p = GamdLbfgsParams(float(tolerance), int(max_iter), int(check_every), float(max_step), float(c1), float(curv), int(m), int(max_ls), 0)
        rows = np.zeros((self.n_boxes, _lib.LBFGS_ROW), dtype=np.float64)
        st = check(self._lib.gamd_minimize_lbfgs(self._h, C.c_void_p(x.data_ptr()), self._box_arg(box), float(length_per_nm),
                                                 C.c_void_p(f.data_ptr()), C.c_void_p(x64.data_ptr()) if return_x64 else None,
                                                 C.byref(p), rows.ctypes.data_as(C.c_void_p), self._stream()), "gamd_minimize_lbfgs")
        return LbfgsResult(st, rows, x, f, x64)

    # -- water classical observer (3-site water: O-O Lennard-Jones plus an Ewald sum, on sampled frames; force labels) ------
    def water_classical_configure(self, interval: int, max_samples: int = 0, q_h: float = 0.417, sigma_o: Optional[float] = None,
                                  epsilon_o: float = 0.635968, r_cut: Optional[float] = None, r_switch: float = 0.0,
                                  shift: bool = False, ewald_tol: float = 1e-10, alpha: Optional[float] = None,
                                  k_cut: Optional[float] = None, coulomb_const: float = COULOMB_KJ_NM,
                                  length_per_nm: float = 0.0, m_site: float = 0.0, virial: bool = False, pme=None, pme_order: int = 6,
                                  cells: bool = False, minimize_configured: bool = False) -> None:
        """While configured, every ``interval``-th completed step of md_run / md_run_nhc (counted across calls, by a counter
        of its own) evaluates the classical potential of 3-site water in double on the device — O-O Lennard-Jones plus
        point charges q_H and q_O = -2 q_H by a plain Ewald sum (real space inside ``r_cut``, same-molecule exclusion,
        reciprocal space out to ``k_cut``, self term; no PME grid) — and logs its terms, the pair count, the charge sum and
        the error sums of the run's (network) forces against the classical forces; ``water_classical_read`` fetches the
        rows.  ``interval`` = 0 switches the observer off but still takes the parameters, which ``water_classical_forces``
        uses.  Water models only, atoms ordered O,H,H, runs with ``species``.  O(N^2) + O(N K) per sample and box.

        ``sigma_o``, ``r_cut``, ``r_switch`` are in the engine's length unit (``alpha``, ``k_cut`` in its reciprocal),
        ``epsilon_o`` in kJ/mol, ``q_h`` in e, ``coulomb_const`` in kJ nm / (mol e^2).  ``length_per_nm`` (0 or 10 =
        Angstrom) only scales the DEFAULTS of ``sigma_o`` (3.15075 Angstrom) and ``r_cut`` (9.5 Angstrom) into the engine's unit.
        Unless given, alpha = sqrt(-ln ewald_tol) / r_cut and k_cut = 2 alpha sqrt(-ln ewald_tol): both truncated tails
        are then about ``ewald_tol`` of a term.  ``r_switch`` and ``shift`` act on the Lennard-Jones term only (default:
        neither).  The defaults (q_H = 0.417 e, sigma_O = 3.15075 Angstrom, epsilon_O = 0.635968 kJ/mol, 138.935456 kJ nm /
        (mol e^2), cutoff 9.5 Angstrom) are meant to be those of OpenMM's ``tip3p.xml`` and of the drivers'
        ``WaterBox(cutoff=9.5 Angstrom)``, but they were written down from memory and are UNVERIFIED: neither OpenMM nor
        openmmtools was available to compare against.

        ``m_site`` = w > 0 puts the negative charge on the TIP4P virtual site M = O + w (d_1 + d_2) of every molecule (d_k
        the minimum-image vectors O -> H_k; OpenMM's ThreeParticleAverageSite with weights 1 - 2 w, w, w): the Coulomb terms
        are then taken on M, H, H, the Lennard-Jones term stays on O with a cutoff test of its own, and M's force goes back
        to the atoms with the same weights, the exact gradient with respect to O, H, H.  Handles, integrators and SETTLE
        still see three atoms.  The observer, ``water_classical_forces`` and the ``"water_classical"`` force source all
        follow it; ``water_minimize`` and ``water_minimize_lbfgs`` follow it with ``minimize_configured=True`` and refuse it
        otherwise.  Every call states the whole potential: the default 0 is 3-site water,
        bit for bit what it was.  ``water_classical_configure(0, **TIP4PEW)`` (module constant: q_H = 0.52422 e, sigma_O =
        3.16435 Angstrom, epsilon_O = 0.680946 kJ/mol, w = 0.106676721) is meant to be OpenMM's ``tip4pew.xml``; these values
        too were written down from memory and are UNVERIFIED.  ``sigma_o`` given explicitly is in the engine's length unit.

        ``virial`` arms the molecular virial log: every sample then also writes W_lj, W_coul, W_recip, W_intra, the
        centre-of-mass kinetic energy and W_mol per box (``RunWaterClassical.virial``, ``.virial_terms``, ``.ke_com``,
        ``.pressure``), by kernels of their own behind the observer's, which change nothing the observer, a force source or
        the trajectory computes.  Every call states it: the default switches the log off.

        ``pme`` = n or (nx, ny, nz) sums the reciprocal part by smooth particle-mesh Ewald (Essmann et al. 1995) of B-spline
        order ``pme_order`` (4 or 6) on a grid of that many points per box and axis, each one of 8, 16, 32, 64, 128
        (``pme_grid`` proposes one): O(N p^3 + G log G) per sample instead of O(N K), in double with an integer spread, so the
        bits repeat as the plain sum's do.  ``k_cut`` is then not read and the limit of 131 072 k-vectors does not apply;
        ``alpha``, ``r_cut`` and every other term are unchanged.  The observer, ``water_classical_forces`` and the
        ``"water_classical"`` force source follow it, with and without ``m_site``; ``virial=True`` and
        ``water_classical_virial`` refuse it, and so do the minimisers unless ``minimize_configured=True`` (without it:
        minimise under the plain sum, configure again with ``pme``, take ``f`` from ``water_classical_forces``).  Every call states it: the default None is the plain sum, bit for bit what it was.

        ``cells`` walks the real-space pairs over a per-box cell table instead of all against all: per sample the atoms are
        ordered by (cell, atom index), cells of edge >= r_cut / 2, and every atom tests the atoms of the 5 x 5 x 5 cells around
        its own (every cell of an axis that has fewer than five).  The pairs, the pair count and the charge sum are exactly the
        all-pairs walk's, U_recip and U_self its bits; U_LJ, U_real + U_excl and the forces differ from it in the order of
        the sums only, within 1e-12 of their sums of absolute terms.  The same bits come back run after run, and a driven
        frame still carries ``fp32(water_classical_forces(x))``; the same atoms given in OTHER periodic images may change
        cells at a face and with them the order of the sums (same bound, not the same bits).  The observer,
        ``water_classical_forces`` and the ``"water_classical"`` force source follow it, with and without ``m_site`` and
        ``pme``; the M-site form's O-O pass and the virial log's own walk stay all-pairs, and the minimisers refuse it unless
        ``minimize_configured=True`` (without it: minimise with ``cells=False``, configure again with ``cells=True``, take
        ``f`` from ``water_classical_forces``).
        The table costs six launches per evaluation: it pays above a few thousand atoms (profiles/run_water_cells.md).  Every
        call states it: the default False is the all-pairs walk, bit for bit what it was.  ``water_cells_table`` reads the
        table of the last evaluation.

        ``minimize_configured`` makes ``water_minimize`` and ``water_minimize_lbfgs`` minimise under the potential as this call
        states it — ``m_site``, ``pme`` (both orders, every grid) and ``cells`` in any combination, none of them included —
        instead of refusing the three.  With none of them set the minimisers' results are bit for bit what they are without
        it.  Every call states it: the default False is the minimisers as they were (3-site, plain sum, all pairs only).

        The plain sum is the limit OpenMM's PME approximates.  Not built: cells for the virial walk and the M-site form's O-O pass, a table kept across steps with a skin; the PME virial, odd orders,
        grids that are no power of two, real-to-complex transforms, the pressure tensor,
        a barostat; the long-range dispersion correction is ``lj_dispersion_correction`` on the host (``pressure(...,
        dispersion=True)``).  No parity with OpenMM is claimed.  Check the parameters against your OpenMM system before
        comparing energies."""
        unit = float(np.float32(length_per_nm)) / 10.0 if length_per_nm else 1.0     # the fp32 value the library holds
        sigma_o = 3.15075 * unit if sigma_o is None else float(sigma_o)
        r_cut = 9.5 * unit if r_cut is None else float(r_cut)
        if alpha is None or k_cut is None:
            if not 0.0 < float(ewald_tol) < 1.0:
                raise ValueError(f"ewald_tol = {ewald_tol} must lie in (0, 1)")
            root = float(np.sqrt(-np.log(float(ewald_tol))))
            alpha = root / r_cut if alpha is None else float(alpha)
            k_cut = 2.0 * alpha * root if k_cut is None else float(k_cut)
        p = GamdWaterParams(int(interval), int(max_samples), float(q_h), sigma_o, float(epsilon_o), r_cut, float(r_switch),
                            int(bool(shift)), 0, float(alpha), float(k_cut), float(coulomb_const))
        off = GamdWaterPmeParams(0, 0, 0, 0)
        if pme is None:
            grid = None
            if getattr(self, "_water_pme", None) is not None:       # the plain sum again, in front of its k-vector list
                check(self._lib.gamd_water_pme(self._h, C.byref(off)), "gamd_water_pme")
                self._water_pme = None
        else:
            grid = tuple(int(g) for g in ((pme,) * 3 if np.ndim(pme) == 0 else pme))
            if len(grid) != 3 or any(g not in PME_LENGTHS for g in grid):
                raise ValueError(f"pme = {pme!r}: one grid length or three, each one of {PME_LENGTHS}")
            if int(pme_order) not in (4, 6):
                raise ValueError(f"pme_order = {pme_order!r} is not 4 or 6 (odd orders are not offered)")
            if virial:
                raise ValueError("virial=True needs the plain sum: there is no PME virial (pme=None)")
            if getattr(self, "_water_pme", None) is None:
                # PME needs an accepted parameter block in front of it, and with PME on k_cut is not read: the block is first
                # taken with a k_cut whose list cannot be refused (1.01 pi / r_cut: every edge is at least 2 r_cut, so the
                # list holds the shortest vectors and little more), then again as the caller states it
                first = GamdWaterParams(0, 0, float(q_h), sigma_o, float(epsilon_o), r_cut, float(r_switch), int(bool(shift)), 0,
                                        float(alpha), min(float(k_cut), 1.01 * np.pi / r_cut), float(coulomb_const))
                check(self._lib.gamd_water_configure(self._h, C.byref(first)), "gamd_water_configure")
                check(self._lib.gamd_water_virial(self._h, 0), "gamd_water_virial")
            on = GamdWaterPmeParams(int(pme_order), *grid)
            check(self._lib.gamd_water_pme(self._h, C.byref(on)), "gamd_water_pme")
            self._water_pme = (int(pme_order), grid)
        check(self._lib.gamd_water_configure(self._h, C.byref(p)), "gamd_water_configure")
        check(self._lib.gamd_water_msite(self._h, float(m_site)), "gamd_water_msite")
        check(self._lib.gamd_water_virial(self._h, int(bool(virial))), "gamd_water_virial")
        if cells or getattr(self, "_water_cells", False):           # (a handle that never had cells makes the calls it made)
            check(self._lib.gamd_water_cells(self._h, int(bool(cells))), "gamd_water_cells")
            self._water_cells = bool(cells)
        if minimize_configured or getattr(self, "_water_min_configured", False):    # (likewise)
            check(self._lib.gamd_water_minimize_potential(self._h, int(bool(minimize_configured))), "gamd_water_minimize_potential")
            self._water_min_configured = bool(minimize_configured)
        self._water_set = True
        self._water_virial = bool(virial)
        self._water_lj = dict(sigma=sigma_o, epsilon=float(epsilon_o), r_cut=r_cut, r_switch=float(r_switch), shift=bool(shift),
                              length_per_nm=float(length_per_nm))

    def water_cells_table(self, box: int = 0):
        """Diagnostic: the cell table of box ``box`` as the last sample, ``water_classical_forces`` call or driven step left it
        (``cells=True``): (nc, start, order) — the cells per axis (3 ints), the first table slot of every cell with the atoms
        per box behind the last (cell = (cx nc[1] + cy) nc[2] + cz), and the atoms' indices inside the box in table order,
        that is by (cell, atom index).  Synchronises."""
        return self._cells_table("gamd_water_cells_read", box)

    def _cells_table(self, entry: str, box: int):
        """(nc, start, order) of box ``box`` through the read call ``entry`` of a potential's cell table."""
        rd = getattr(self._lib, entry)
        nc = (C.c_int32 * 3)()
        check(rd(self._h, self._stream(), int(box), nc, None, 0, None, 0), entry)
        start = np.zeros(nc[0] * nc[1] * nc[2] + 1, dtype=np.int32)
        order = np.zeros(self.n, dtype=np.int32)
        check(rd(self._h, self._stream(), int(box), nc, start.ctypes.data_as(C.c_void_p), start.size,
                 order.ctypes.data_as(C.c_void_p), order.size), entry)
        return np.array(list(nc), dtype=np.int64), start, order

    def water_classical_reset(self) -> None:
        """Step count and rows back to zero; parameters and configuration stay."""
        check(self._lib.gamd_water_reset(self._h), "gamd_water_reset")

    def water_classical_read(self, forces: bool = False) -> "RunWaterClassical":
        """Synchronise and fetch what the water classical observer has logged since it was configured or reset; ``forces``:
        also the classical forces of the last sample."""
        rc = self._potential_read("gamd_water_read", _lib.WATER_ROW, RunWaterClassical, forces)
        rc.lj = getattr(self, "_water_lj", None)
        if getattr(self, "_water_virial", False) and rc.steps.shape[0] > 0:
            vr = np.zeros((rc.steps.shape[0], self.n_boxes, _lib.WATER_VIRIAL_ROW), dtype=np.float64)
            n_rows = C.c_int64()
            check(self._lib.gamd_water_virial_read(self._h, self._stream(), vr.ctypes.data_as(C.c_void_p), vr.shape[0],
                                                   C.byref(n_rows)), "gamd_water_virial_read")
            rc.set_virial_rows(vr[:n_rows.value])
        return rc

    def _species_flags(self, species) -> Optional[torch.Tensor]:
        if species is None:
            return None
        s = torch.as_tensor(species).reshape(-1).to(device=self.device)
        if s.numel() == self.n and self.n_boxes > 1:
            s = s.repeat(self.n_boxes)
        if s.numel() != self.n_total:
            raise ValueError("species must have one entry per atom")
        return (s != 0).to(torch.uint8).contiguous()

    def water_classical_virial(self, pos: ArrayLike, species, vel: Optional[ArrayLike] = None, box=None, length_per_nm: float = 0.0,
                               mass_o_amu: float = 15.99943, mass_h_amu: float = 1.007947):
        """The molecular virial of the water classical potential of the last ``water_classical_configure`` on given positions
        (and velocities ``vel`` [N, 3] in length unit / ps, fp32 as the library reads them; None: KE_com = 0), outside any
        run and whether or not the log is armed: a RunWaterClassical of one row whose ``virial``, ``virial_terms`` and
        ``ke_com`` are filled, so ``.pressure(None, volumes)`` is the pressure of the frame.  Arguments as
        ``water_classical_forces``; the masses are those a run would be given as mass_amu / mass_h_amu.  Synchronises."""
        if not getattr(self, "_water_set", False):
            self.water_classical_configure(0, length_per_nm=length_per_nm)
        p = self._dev_pos(pos)
        flags = self._species_flags(species)
        v = None
        if vel is not None:
            v = torch.as_tensor(vel, dtype=torch.float32).to(device=self.device).reshape(-1, 3).contiguous()
            if v.shape[0] != self.n_total:
                raise ValueError("vel must have one row per atom")
        row = np.zeros((1, self.n_boxes, _lib.WATER_ROW), dtype=np.float64)
        vrow = np.zeros((1, self.n_boxes, _lib.WATER_VIRIAL_ROW), dtype=np.float64)
        check(self._lib.gamd_water_virial_eval(self._h, C.c_void_p(p.data_ptr()), C.c_void_p(flags.data_ptr()) if flags is not None else None,
                                               C.c_void_p(v.data_ptr()) if v is not None else None, self._box_arg(box),
                                               float(length_per_nm), float(mass_o_amu), float(mass_h_amu),
                                               vrow.ctypes.data_as(C.c_void_p), row.ctypes.data_as(C.c_void_p), self._stream()),
              "gamd_water_virial_eval")
        rc = RunWaterClassical([0], row, self.n, virial_rows=vrow)
        rc.lj = getattr(self, "_water_lj", None)
        return rc

    def water_classical_forces(self, pos: ArrayLike, species, box=None, length_per_nm: float = 0.0):
        """The water classical potential of the last ``water_classical_configure`` (with the defaults and interval 0 when
        there was none) on given positions, outside any run: (forces float64 [N, 3] on the device in kJ/mol/nm, a
        RunWaterClassical of one row with the terms per box; its force-error sums are 0).  ``pos`` [N, 3] in any periodic
        image, fp32 as the library reads it; ``species`` [N] (or one box's), O != 0; ``box`` as in ``forward``;
        ``length_per_nm`` the length unit (0 or 10 = Angstrom).  Synchronises once."""
        if not getattr(self, "_water_set", False):
            self.water_classical_configure(0, length_per_nm=length_per_nm)
        p = self._dev_pos(pos)
        flags = None
        if species is not None:
            s = torch.as_tensor(species).reshape(-1).to(device=self.device)
            if s.numel() == self.n and self.n_boxes > 1:
                s = s.repeat(self.n_boxes)
            if s.numel() != self.n_total:
                raise ValueError("species must have one entry per atom")
            flags = (s != 0).to(torch.uint8).contiguous()
        out = torch.empty((self.n_total, 3), dtype=torch.float64, device=self.device)
        row = np.zeros((1, self.n_boxes, _lib.WATER_ROW), dtype=np.float64)
        check(self._lib.gamd_water_eval(self._h, C.c_void_p(p.data_ptr()), C.c_void_p(flags.data_ptr()) if flags is not None else None,
                                        self._box_arg(box), float(length_per_nm), C.c_void_p(out.data_ptr()),
                                        row.ctypes.data_as(C.c_void_p), self._stream()), "gamd_water_eval")
        return out, RunWaterClassical([0], row, self.n)

    # -- water energy minimiser (the water drivers' minimizeEnergy in front of the first step) ---------------------------
    def water_minimize(self, x: torch.Tensor, species, f: Optional[torch.Tensor] = None, tolerance: float = 10.0, max_iter: int = 0,
                       box=None, length_per_nm: float = 0.0, r_oh: float = 0.0, r_hh: float = 0.0, return_x64: bool = False,
                       check_every: int = 0, **fire) -> "MinimizeResult":
        """Relax the rigid 3-site molecules ``x`` (float32 CUDA tensor, atoms ordered O,H,H, changed in place) of every box
        under the water classical potential of the last ``water_classical_configure`` (with the defaults and interval 0 when
        there was none) on the device, until the root mean square over 3N of the components of the force projected onto the
        constraint manifold is at most ``tolerance`` (kJ/mol/nm) or ``max_iter`` position updates are done (0 = 10 000).
        Rigid-molecule FIRE in double with SETTLE, unit weights in the constraint arithmetic; not OpenMM's L-BFGS: no
        parity with it is claimed.  ``r_oh``, ``r_hh``: the rigid geometry in the engine's length unit (0: TIP3P scaled by
        ``length_per_nm`` / 10); the input is put on it first.  ``fire`` as in ``minimize`` (the defaults are for Angstrom).

        On return ``x`` holds the result rounded to fp32 with molecules whole and every oxygen in [0, L), and ``f``
        (allocated when None) the classical forces at exactly that ``x`` — ``water_classical_forces(x, species)[0].float()``
        bit for bit, what a water-source ``md_run`` / ``md_run_nhc`` with ``rigid_water`` needs on entry.  A box that was
        not finite at the start keeps its ``x``; nothing is written to ``f`` for a box that failed.  ``return_x64``: also the
        unrounded, unwrapped, exactly rigid double positions (``result.x64``).  Water models only; 2 r_cut must not exceed a
        box edge.  Synchronises.

        Without ``water_classical_configure(..., minimize_configured=True)`` the minimiser is 3-site, plain sum, all pairs:
        with ``m_site`` != 0, ``pme`` or ``cells`` in force it raises (the library answers -22 and names the form and the
        switch) before anything is enqueued.  With it, the call minimises under the potential as configured, whatever
        combination of the three is set: the same arguments, states and rows; ``f`` is still
        ``water_classical_forces(x, species)[0].float()`` bit for bit, now under that configuration; ``tolerance`` bounds the
        rms of the projected force on the three real atoms, M's force having been spread onto them with the weights
        1 - 2 w, w, w; U in the result is the configured potential's.  With none of the three set the results are the
        switch-off results bit for bit."""
        unknown = set(fire) - {"dt_start", "dt_max", "n_min", "f_inc", "f_dec", "alpha_start", "f_alpha", "max_step"}
        if unknown:
            raise TypeError(f"water_minimize() got unexpected FIRE constants {sorted(unknown)}")
        if not getattr(self, "_water_set", False):
            self.water_classical_configure(0, length_per_nm=length_per_nm)
        if f is None:
            f = torch.zeros_like(x)
        self._md_state(x, f)
        flags = self._water_flags(species)
        unit = float(np.float32(length_per_nm)) / 10.0 if length_per_nm else 1.0     # the fp32 value the library holds
        from . import workloads as wl
        r_oh = float(r_oh) if r_oh else wl.TIP3P_R_OH * unit
        r_hh = float(r_hh) if r_hh else wl.TIP3P_R_HH * unit
        x64 = torch.empty((self.n_total, 3), dtype=torch.float64, device=self.device) if return_x64 else None
        g = lambda k: float(fire.get(k, 0.0))
        p = GamdMinimizeParams(float(tolerance), int(max_iter), int(check_every), g("dt_start"), g("dt_max"), g("f_inc"), g("f_dec"),
                               g("alpha_start"), g("f_alpha"), g("max_step"), int(fire.get("n_min", 0)), 0)
        rows = np.zeros((self.n_boxes, _lib.MINIMIZE_ROW), dtype=np.float64)
        st = check(self._lib.gamd_water_minimize(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(flags.data_ptr()) if flags is not None else None,
                                                 self._box_arg(box), float(length_per_nm), r_oh, r_hh, C.c_void_p(f.data_ptr()),
                                                 C.c_void_p(x64.data_ptr()) if return_x64 else None, C.byref(p),
                                                 rows.ctypes.data_as(C.c_void_p), self._stream()), "gamd_water_minimize")
        return MinimizeResult(st, rows, x, f, x64)

    def _water_flags(self, species):
        if species is None:
            return None
        s = torch.as_tensor(species).reshape(-1).to(device=self.device)
        if s.numel() == self.n and self.n_boxes > 1:
            s = s.repeat(self.n_boxes)
        if s.numel() != self.n_total:
            raise ValueError("species must have one entry per atom")
        return (s != 0).to(torch.uint8).contiguous()

    def water_minimize_lbfgs(self, x: torch.Tensor, species, f: Optional[torch.Tensor] = None, tolerance: float = 10.0, max_iter: int = 0,
                             box=None, length_per_nm: float = 0.0, r_oh: float = 0.0, r_hh: float = 0.0, return_x64: bool = False,
                             check_every: int = 0, m: int = 0, c1: float = 0.0, curv: float = 0.0, max_ls: int = 0,
                             max_step: float = 0.0) -> "LbfgsResult":
        """``water_minimize`` with L-BFGS in place of FIRE: the same task, arguments and results (``x`` changed in place:
        molecules whole, every oxygen in [0, L); ``f`` the classical forces at exactly that ``x``,
        ``water_classical_forces(x, species)[0].float()`` bit for bit; ``result.x64`` exactly rigid; a failed box keeps its
        ``x`` and ``f``), with the algorithm, constants and result of ``minimize_lbfgs``: a history of ``m`` pairs, a
        backtracking line search on sufficient decrease (``c1``, ``max_ls``), one clamp factor per molecule so that no atom's
        trial displacement exceeds ``max_step`` in front of SETTLE, ``max_iter`` evaluations at most.  The iterate stays on
        the manifold of rigid molecules: the force is projected onto the tangent space of the bond constraints (unit
        weights), SETTLE carries every trial back, and the history is used without vector transport.  ``rms`` and ``fmax``
        are of the projected force.  tests/water_lbfgs_ref.py is the recipe in float64; no parity with OpenMM is claimed.

        The DEFAULT Lennard-Jones term of ``water_classical_configure`` is cut at ``r_cut`` without a switch or a shift, so U
        jumps (about 0.03 kJ/mol at r_cut = 6.5 Angstrom) when an O-O pair crosses the cutoff, and the sufficient-decrease
        test cannot pass such a jump once the steps gain less than that: on the default potential the call stops as
        "line_search" somewhere below a tolerance of about 1.  For tolerances below about 1 configure the potential with
        ``r_switch`` > 0 or ``shift=True``.  Water models only.  Without
        ``water_classical_configure(..., minimize_configured=True)``: 3-site, plain Ewald sum, all pairs — with ``m_site``,
        ``pme`` or ``cells`` in force it raises (-22, naming the reason and the switch) before anything is enqueued.  With it:
        the potential as configured, under ``water_minimize``'s contract for that case (``f`` under the configuration in
        force, the projected force of the three real atoms after M's force has been spread); the trial positions go through
        the same route as the iterate's.  Synchronises."""
        if not getattr(self, "_water_set", False):
            self.water_classical_configure(0, length_per_nm=length_per_nm)
        if f is None:
            f = torch.zeros_like(x)
        self._md_state(x, f)
        flags = self._water_flags(species)
        unit = float(np.float32(length_per_nm)) / 10.0 if length_per_nm else 1.0     # the fp32 value the library holds
        from . import workloads as wl
        r_oh = float(r_oh) if r_oh else wl.TIP3P_R_OH * unit
        r_hh = float(r_hh) if r_hh else wl.TIP3P_R_HH * unit
        x64 = torch.empty((self.n_total, 3), dtype=torch.float64, device=self.device) if return_x64 else None
        p = GamdLbfgsParams(float(tolerance), int(max_iter), int(check_every), float(max_step), float(c1), float(curv), int(m), int(max_ls), 0)
        rows = np.zeros((self.n_boxes, _lib.LBFGS_ROW), dtype=np.float64)
        st = check(self._lib.gamd_water_minimize_lbfgs(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(flags.data_ptr()) if flags is not None else None,
                                                       self._box_arg(box), float(length_per_nm), r_oh, r_hh, C.c_void_p(f.data_ptr()),
                                                       C.c_void_p(x64.data_ptr()) if return_x64 else None, C.byref(p),
                                                       rows.ctypes.data_as(C.c_void_p), self._stream()), "gamd_water_minimize_lbfgs")
        return LbfgsResult(st, rows, x, f, x64)

    def sync_status(self) -> int:
        """0, or 1 when an enqueued MD run overflowed a neighbour buffer, froze on the device and was resumed."""
        return check(self._lib.gamd_sync_status(self._h, self._stream()), "gamd_sync_status")

    def nonfinite_seen(self) -> bool:
        """True if any force evaluation since the last call produced a non-finite component (clears the flag)."""
        flags = (C.c_int32 * 4)()
        check(self._lib.gamd_get_device_flags(self._h, flags), "gamd_get_device_flags")
        return bool(flags[0])

    def timing_enable(self, on: bool = True) -> None:
        check(self._lib.gamd_timing_enable(self._h, int(on)), "gamd_timing_enable")

    def timing_read(self) -> Tuple[float, int]:
        """(summed conv-edge kernel ms, launches) since timing_enable(True); synchronises."""
        tot, cnt = C.c_double(), C.c_int64()
        check(self._lib.gamd_timing_read(self._h, self._stream(), C.byref(tot), C.byref(cnt)), "gamd_timing_read")
        return tot.value, cnt.value

    def timing_read_stages(self):
        """{stage: (summed ms, count)} since timing_enable(True) for 'conv_edge', 'edge_encode' and 'node_mid' (the node
        kernel between two conv layers, kernel boundaries included); synchronises."""
        ms, cnt = (C.c_double * 3)(), (C.c_int64 * 3)()
        check(self._lib.gamd_timing_read_stages(self._h, self._stream(), ms, cnt), "gamd_timing_read_stages")
        return {k: (ms[i], cnt[i]) for i, k in enumerate(("conv_edge", "edge_encode", "node_mid"))}

    def timing_read_steps(self, max_steps: int = 1 << 16) -> np.ndarray:
        """Device milliseconds of every MD step enqueued by md_run / md_run_nhc since timing_enable(True) (one HIP event in
        front of each step's first kernel, one behind the last); synchronises."""
        buf = (C.c_float * max_steps)()
        n = C.c_int64()
        check(self._lib.gamd_timing_read_steps(self._h, self._stream(), buf, max_steps, C.byref(n)), "gamd_timing_read_steps")
        return np.ctypeslib.as_array(buf)[:min(n.value, max_steps)].astype(np.float64)

    def profile(self, pos: ArrayLike, box=None, species=None):
        """Event-timed single forward: list of (kernel label, ms)."""
        p = self._dev_pos(pos)
        s = self._dev_species(species)
        names = C.create_string_buffer(4096)
        ms = (C.c_float * 64)()
        n = C.c_int32()
        for _ in range(4):
            st = self._lib.gamd_profile(self._h, C.c_void_p(p.data_ptr()),
                                        C.c_void_p(s.data_ptr()) if s is not None else None, self._box_arg(box),
                                        C.c_void_p(self._out.data_ptr()), self._stream(), names, 4096, ms, 64, C.byref(n))
            check(st, "gamd_profile")
            st = self._lib.gamd_sync_status(self._h, self._stream())
            if st != -34:                          # -34: a neighbour buffer overflowed and was regrown -> replay
                check(st, "gamd_sync_status")
                break
        else:
            check(st, "gamd_sync_status")
        labels = names.value.decode().strip().split("\n")
        return list(zip(labels, [ms[i] for i in range(n.value)]))
