"""The water minimisers under the configured potential (gamd_water_minimize_potential, gamd_amd/csrc/water_relax.hip) as far as
they can be seen without a GPU.

* tests/water_relax_ref.py with every form off IS the existing replays: the same x, U, rms and counts, bit for bit, from
  water_minimize_ref.minimize and water_lbfgs_ref.minimize on the 86-molecule lattice start (8 iterations / evaluations).
* For each form (3-site plain, M-site, PME order 6, M-site + PME order 4 on the non-cubic grid; the cell table changes no value in
  float64) the PROJECTED force is the gradient on the rigid manifold: along random tangent directions d (per molecule a
  translation plus a rotation about the centroid, water_relax_ref.tangent) F_c . d equals the central difference
  -(U(x + h d) - U(x - h d)) / 2 h of the form's own energy at h = 1e-4 Angstrom.  Because d is tangent, F_c . d = F . d.
  The bars are the ones the reference modules state per COORDINATE for their forces against the same central differences —
  1.3e-8 of max |F| where the M-site or the plain 3-site reference forms the force (tests/test_water_msite_host.py's figure),
  9e-10 of max |F| for the 3-site PME reference — and a directional derivative is the combination sum_c d_c dU/dx_c of the
  coordinate ones, so its bar is that figure times max |F| times sum_c |d_c|.  The Lennard-Jones term is switched (a truncated
  one jumps when a pair crosses the cutoff inside +-h d); ewald_tol 1e-12.  The figures are printed.
* The entry is exported, bound, and refuses a null handle.
* The k_wrx_ kernels of the release and the checked library are exactly k_wrx_sites, k_wrx_lj, k_wrx_mols, k_wrx_lbmols, without
  scratch or a spilled register; the per-molecule passes within 128 vector registers (four waves per SIMD, k_wmin_mols' launch
  bounds), k_wrx_sites and k_wrx_lj within the 128 of k_w4_sites and k_w4_lj, which they restate
  (tests/test_water_msite_host.py)."""
import os
import sys

import numpy as np
import pytest

import water_classical_ref as wr
import water_lbfgs_ref as wlr
import water_minimize_ref as wm
import water_relax_ref as rr
from gamd_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

DELTA = 1e-8                                                    # ewald_tol of the water minimisers' tests
KERNELS = {"k_wrx_sites": 128, "k_wrx_lj": 128, "k_wrx_mols": 128, "k_wrx_lbmols": 128}   # the VGPR caps
NONCUBIC = np.array([13.875, 13.75, 14.0], dtype=np.float32)
FD_FORMS = [(rr.Form(), 1.3e-8), (rr.Form(w=rr.TIP4PEW_W), 1.3e-8), (rr.Form(pme=(16, 16, 16), order=6), 9e-10),
            (rr.Form(w=rr.TIP4PEW_W, pme=(16, 32, 8), order=4), 1.3e-8)]


@pytest.fixture(scope="module")
def lib():
    from gamd_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _start():
    pos, box, species, _ = wl.water_box(86, seed=5, jitter=0.0, wrap=False)
    return pos.astype(np.float32), np.float32(box), species


# ---- the replay ----------------------------------------------------------------------------------------------------------
def test_with_every_form_off_the_replays_are_the_existing_ones_exactly():
    x0, box, species = _start()
    w = wr.Water(r_cut=6.5, ewald_tol=DELTA)
    a, b = wm.minimize(x0, box, species, w, 1e-300, max_iter=8), rr.minimize(rr.Form(), x0, box, species, w, 1e-300, max_iter=8)
    assert a["state"] == b["state"] == wm.MAX_ITER and a["iterations"] == b["iterations"] == 8
    assert np.array_equal(a["x"], b["x"]) and all(a[k] == b[k] for k in ("u0", "rms0", "u", "rms", "fmax", "dt"))
    a, b = wlr.minimize(x0, box, species, w, 1e-300, max_iter=8), rr.minimize_lbfgs(rr.Form(), x0, box, species, w, 1e-300, max_iter=8)
    assert a["state"] == b["state"] == wlr.MAX_ITER and a["evaluations"] == b["evaluations"] == 8
    assert np.array_equal(a["x"], b["x"]) and all(a[k] == b[k] for k in ("u0", "rms0", "u", "rms", "fmax", "accepted", "skipped", "resets"))
    assert wm.wr is wr and wlr.wr is wr                         # the modules are as they were


def test_another_form_is_another_potential_and_the_replays_follow_it():
    x0, box, species = _start()
    w = wr.Water(r_cut=6.5, ewald_tol=DELTA)
    base = rr.minimize(rr.Form(), x0, box, species, w, 1e-300, max_iter=2)
    for form in (rr.Form(w=rr.TIP4PEW_W), rr.Form(pme=(16, 16, 16))):
        r = rr.minimize(form, x0, box, species, w, 1e-300, max_iter=2)
        l = rr.minimize_lbfgs(form, x0, box, species, w, 1e-300, max_iter=2)
        assert r["u0"] == l["u0"] == rr.evaluate(form, wm.settle(x0.astype(np.float64), x0.astype(np.float64), wm.TIP3P_R_OH, wm.TIP3P_R_HH),
                                                 box, species, w)["energy"]
        assert r["u0"] != base["u0"] and r["u"] < r["u0"] and l["u"] < l["u0"], form.name()


@pytest.mark.parametrize("form,bar", FD_FORMS, ids=[f.name() for f, _ in FD_FORMS])
def test_the_projected_force_is_the_gradient_of_the_forms_own_energy_on_the_rigid_manifold(form, bar):
    pos, box, species, _ = wl.water_box(86, seed=5, jitter=0.02, wrap=False)
    box = NONCUBIC if form.pme == (16, 32, 8) else np.float32(box)
    x = wm.settle(pos.astype(np.float64), pos.astype(np.float64), wm.TIP3P_R_OH, wm.TIP3P_R_HH)
    wat = wr.Water(r_cut=6.8, r_switch=5.8, ewald_tol=1e-12)
    Fc, rms, _ = rr.projected(form, x, box, species, wat)
    raw = rr.evaluate(form, x, box, species, wat)["forces"]
    fmax = np.abs(raw).max()
    h = 1e-4
    rng = np.random.default_rng(11)
    for k in range(3):
        d = rr.tangent(x, rng)
        d /= np.abs(d).max()
        lhs = float((Fc * d).sum()) / 10.0                      # kJ/mol/nm -> kJ/mol/Angstrom
        fd = -(rr.evaluate(form, x + h * d, box, species, wat)["energy"] - rr.evaluate(form, x - h * d, box, species, wat)["energy"]) / (2.0 * h)
        limit = bar * (fmax / 10.0) * np.abs(d).sum()
        print(f"{form.name()}, direction {k}: F_c.d = {lhs:.9e}, -dU/dh = {fd:.9e}, |difference| {abs(lhs - fd):.3e} (bar {limit:.3e}; "
              f"per coordinate {abs(lhs - fd) / ((fmax / 10.0) * np.abs(d).sum()):.2e} of max |F|); |F.d - F_c.d| {abs(float((raw * d).sum()) / 10.0 - lhs):.2e}")
        assert abs(lhs - fd) <= limit


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_the_entry_is_exported_bound_and_refuses_a_null_handle(lib):
    from gamd_amd import _lib
    from gamd_amd.engine import GamdForce
    import inspect
    assert hasattr(lib, "gamd_water_minimize_potential") and "gamd_water_minimize_potential" in _lib.SYMBOLS
    assert lib.gamd_water_minimize_potential(None, 1) == -22 and b"null handle" in lib.gamd_last_error()
    p = inspect.signature(GamdForce.water_classical_configure).parameters["minimize_configured"]
    assert p.default is False


# ---- kernels -------------------------------------------------------------------------------------------------------------
def test_wrx_kernels_are_the_documented_set_in_both_libraries_without_scratch_or_spills(lib):
    from gamd_amd import _lib
    if not os.path.exists(os.path.join(kr.LLVM_BIN, "llvm-readelf")):
        pytest.skip("ROCm LLVM tools not installed")
    for path in (_lib.LIB_PATH, os.path.join(ROOT, "gamd_amd", "libgamd_hip_chk.so")):
        res = {n: v for n, v in kr.kernel_resources(path).items() if "k_wrx_" in n}
        assert len(res) == len(KERNELS) and all(any(k + "(" in n for n in res) for k in KERNELS), sorted(res)
        for n, v in res.items():
            short = next(k for k in KERNELS if k + "(" in n)
            print(os.path.basename(path), short, "vgpr", v["vgpr_count"], "sgpr", v.get("sgpr_count"), "lds", v.get("group_segment_fixed_size", 0))
            assert v.get("private_segment_fixed_size", 0) == 0, (n, v)
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (n, v)
            assert v["vgpr_count"] + v.get("agpr_count", 0) <= KERNELS[short], (n, v)
