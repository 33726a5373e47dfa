"""Host side of the run recorder (no GPU): the binding table and parameter block of the four gamd_traj_* entry points, and
RunTrajectory's normalisation, unwrapping, diffusion coefficients and dataset files on synthetic arrays."""
import ctypes
import os

import numpy as np
import pytest

from gamd_amd import _lib
from gamd_amd._lib import GamdTrajParams
from gamd_amd.engine import RunTrajectory


def test_binding_table_has_the_recorder_entry_points():
    for name in ("gamd_traj_configure", "gamd_traj_reset", "gamd_traj_read_frames", "gamd_traj_read_dynamics"):
        assert name in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["gamd_traj_read_frames"][1]) == 11 and len(_lib.SYMBOLS["gamd_traj_read_dynamics"][1]) == 9
    assert _lib.TRAJ_FIELDS == {"x": 1, "v": 2, "f": 4, "image": 8}


def test_parameter_block_layout():
    assert ctypes.sizeof(GamdTrajParams) == 32
    assert [getattr(GamdTrajParams, k).offset for k in ("interval", "max_frames", "fields", "n_lags", "subtract_com", "reserved")] \
        == [0, 8, 16, 20, 24, 28]


def _synthetic(msd_of_t, vacf_of_t, n_lags=12, Q=40, class_atoms=(5, 10), interval=4, dt=0.002):
    """sums that normalise to the given functions of time for two classes (class 1: twice the values)"""
    t = np.arange(n_lags) * interval * dt
    norm = (Q - np.arange(n_lags))[None, :] * np.asarray(class_atoms, dtype=np.float64)[:, None]
    scale = np.array([1.0, 2.0])[:, None]
    msd = (scale * msd_of_t(t)[None, :] * norm)[None]
    vacf = (scale * vacf_of_t(t)[None, :] * norm)[None]
    return RunTrajectory(n_samples=Q, class_atoms=[class_atoms], msd_sum=msd, vacf_sum=vacf, interval=interval), t


def test_diffusion_from_an_exactly_linear_msd():
    D = 0.2371
    tr, t = _synthetic(lambda t: 6.0 * D * t + 0.03, lambda t: 0.0 * t)
    assert np.array_equal(tr.lag_times(0.002), t)
    assert tr.msd(0).shape == (2, 12)
    assert abs(tr.diffusion_msd(0, 0, 0.002, fit=(2, 11)) / D - 1.0) < 1e-12
    assert abs(tr.diffusion_msd(0, 1, 0.002, fit=(3, 9)) / (2.0 * D) - 1.0) < 1e-12
    # (length unit)^2 -> nm^2
    assert abs(tr.diffusion_msd(0, 0, 0.002, fit=(2, 11), length_per_nm=10.0) / (D / 100.0) - 1.0) < 1e-12
    with pytest.raises(ValueError):
        tr.diffusion_msd(0, 0, 0.002, fit=(5, 12))


def test_green_kubo_from_a_vacf_with_a_known_trapezoid():
    # linear VACF c(t) = c0 (1 - t / T): the trapezoid rule is exact, integral over [0, t_k] = c0 (t_k - t_k^2 / (2 T))
    c0, T = 7.5, 0.2
    tr, t = _synthetic(lambda t: 0.0 * t, lambda t: c0 * (1.0 - t / T))
    for upto in (1, 6, 11):
        exact = c0 * (t[upto] - t[upto] ** 2 / (2.0 * T)) / 3.0
        assert abs(tr.diffusion_green_kubo(0, 0, 0.002, upto) / exact - 1.0) < 1e-12
        assert abs(tr.diffusion_green_kubo(0, 1, 0.002, upto, length_per_nm=18.8972613) / (2.0 * exact / 18.8972613 ** 2) - 1.0) < 1e-12


def test_normalisation_is_nan_beyond_the_number_of_origins():
    Q, n_lags = 5, 8
    sums = np.ones((2, 1, n_lags))
    tr = RunTrajectory(n_samples=Q, class_atoms=[[4], [2]], msd_sum=sums, vacf_sum=3.0 * sums, interval=10)
    m, c = tr.msd(1), tr.vacf(0)
    assert m.shape == (1, n_lags) and np.isnan(m[0, Q:]).all() and np.isnan(c[0, Q:]).all()
    assert np.array_equal(m[0, :Q], 1.0 / ((Q - np.arange(Q)) * 2.0))
    assert np.array_equal(c[0, :Q], 3.0 / ((Q - np.arange(Q)) * 4.0))
    assert tr.n_lags == n_lags and np.array_equal(tr.lag_times(0.5), 5.0 * np.arange(n_lags))
    with pytest.raises(ValueError):
        RunTrajectory(n_samples=3).msd(0)


def test_unwrapped_on_hand_made_images():
    x = np.array([[[[0.5, 1.0, 9.5], [3.0, 3.0, 3.0]], [[0.25, 0.5, 0.75], [1.0, 2.0, 3.0]]]], dtype=np.float32)   # [1, 2, 2, 3]
    image = np.array([[[[1, 0, -2], [0, 0, 0]], [[0, 3, 0], [-1, -1, 1]]]], dtype=np.int32)
    tr = RunTrajectory(steps=[10], x=x, image=image)
    u = tr.unwrapped([[10.0], [4.0]])
    assert u.dtype == np.float64 and u.shape == (1, 2, 2, 3)
    assert np.array_equal(u[0, 0], [[10.5, 1.0, -10.5], [3.0, 3.0, 3.0]])
    assert np.array_equal(u[0, 1], [[0.25, 12.5, 0.75], [-3.0, -2.0, 7.0]])
    # an orthorhombic box for all; the fp32 value of the edge is what counts
    u = RunTrajectory(steps=[10], x=x[:, :1], image=image[:, :1]).unwrapped([10.0, 20.0, 0.1])
    assert np.array_equal(u[0, 0, 0], [10.5, 1.0, 9.5 - 2.0 * float(np.float32(0.1))])
    with pytest.raises(ValueError):
        RunTrajectory(steps=[10], x=x).unwrapped(10.0)


def test_write_dataset_round_trips(tmp_path):
    rng = np.random.default_rng(0)
    F, B, n = 3, 2, 7
    x = rng.uniform(0, 20, (F, B, n, 3)).astype(np.float32)
    v = rng.normal(0, 3, (F, B, n, 3)).astype(np.float32)
    f = rng.normal(0, 50, (F, B, n, 3)).astype(np.float32)
    tr = RunTrajectory(steps=[50, 100, 150], x=x, v=v, f=f)
    paths = tr.write_dataset(str(tmp_path / "lj_data"), seed=4)
    assert [os.path.basename(p) for p in paths] == ["data_4_0.npz", "data_4_1.npz", "data_4_2.npz"]
    for t, p in enumerate(paths):
        d = np.load(p)
        assert sorted(d.files) == ["forces", "pos", "vel"]
        assert all(d[k].dtype == np.float32 and d[k].shape == (n, 3) for k in d.files)
        assert np.array_equal(d["pos"], x[t, 0]) and np.array_equal(d["forces"], f[t, 0])
        assert np.array_equal(d["vel"], (v[t, 0].astype(np.float64) * 100.0).astype(np.float32))
    # bohr -> Angstrom; positions only; another prefix
    bohr = 18.8972613
    paths = RunTrajectory(steps=[5], x=x[:1]).write_dataset(str(tmp_path / "w"), seed=0, prefix="frame_", length_per_nm=bohr)
    assert [os.path.basename(p) for p in paths] == ["frame_0_0.npz"]
    d = np.load(paths[0])
    assert d.files == ["pos"]
    assert np.allclose(d["pos"], x[0, 0].astype(np.float64) * 10.0 / bohr, rtol=2e-7, atol=0)
    paths = RunTrajectory(steps=[5], x=x[:1], v=v[:1]).write_dataset(str(tmp_path / "w2"), seed=1, length_per_nm=bohr)
    assert np.allclose(np.load(paths[0])["vel"], v[0, 0].astype(np.float64) * 1000.0 / bohr, rtol=2e-7, atol=0)


def test_recorder_kernels_use_no_scratch():
    """the compiler reports neither spills nor a private segment for the six k_traj_* kernels, in the release and the
    checked library"""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    from kernel_resources import kernel_resources
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    for path in (_lib.LIB_PATH, os.path.join(root, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kernel_resources(path).items() if "k_traj_" in n}
        assert len(res) == 6, sorted(res)
        for n, v in res.items():
            assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0, (n, v)
