"""The device's Langevin noise (atom_noise of gamd_md_dev.h, inlined into k_baoab_first, k_baoab_first_rigid, k_step_small and
k_skin_check) against its numpy restatement, tests/md_noise_ref.py, number by number, and the O step's a and b = sqrt(1 - a^2)
held together for free atoms at T > 0.

The system is force-free: a random-weight model whose last decoder Linear is zero, no scaler, so f = 0 exactly (asserted after
every run) and the O step is all that acts.  With v = 0 on entry and gamma dt = 100 (a = e^-100) a run leaves
v = fl(bs xi(last step)), bs = b_len_kT sqrt(1/m); xi_dev = v / bs in float64, with bs formed in fp32 as the device forms it.

|xi_dev - xi_ref| <= 5e-6 absolute: |xi| < 6 (tests/test_md_noise_reference.py), u and t carry the same bits on both sides, so
what remains is fp32 logf / sqrtf at <= 2 ulp on r (2e-6), sinf / cosf at <= 2 ulp times r (1.4e-6), the products and the stored
v (1e-6).  Measured figures: profiles/md_noise_parity.md."""
import math

import numpy as np
import pytest
import torch

import md_noise_ref as nr
from helpers import rel_err
from gamd_amd import workloads as wl

pytestmark = pytest.mark.gpu

TOL = nr.DEVICE_TOL
RC = 7.5                                             # skin mode: a skin of RC / 6
T_K, M_AMU = 300.0, 39.9
FAST = dict(dt_ps=1e-6, gamma_per_ps=1e8)            # a = e^-100: nothing of the step before survives the O step


def free_state_dict():
    from gamd_amd.weights import ModelConfig, make_state_dict
    sd = make_state_dict(ModelConfig(), 0, 7.0, 2.2)
    sd["graph_decoder.mlp_layer.2.weight"].zero_()
    sd["graph_decoder.mlp_layer.2.bias"].zero_()
    return sd


@pytest.fixture(scope="module")
def engines():
    """(n per box, skin on, boxes, reduced density, cutoff) -> (engine, positions, box edge): each built once, closed at the end
    of the module."""
    from gamd_amd.engine import GamdForce
    sd, made = free_state_dict(), {}

    def get(n, skin, n_boxes=1, rho_star=0.5, rc=RC):
        key = (n, bool(skin), n_boxes, rho_star, rc)
        if key not in made:
            pos, box = wl.lj_box(n, rho_star=rho_star, seed=3)
            assert 2.0 * (rc + (rc / 6.0 if skin else 0.0)) < box
            eng = GamdForce(sd, n, box, rc, neighbor_skin=rc / 6.0 if skin else 0.0, n_boxes=n_boxes)
            made[key] = (eng, np.tile(pos, (n_boxes, 1)), box)
        return made[key]

    yield get
    for eng, _, _ in made.values():
        eng.close()


def species_of(n_total):
    """O, H, H, O, H, H, ... unconstrained: two masses, so bs differs from atom to atom."""
    return np.arange(n_total) % 3 == 0


def masses(n_total, species):
    return np.full(n_total, M_AMU) if species is None else np.where(species, wl.MASS_O, wl.MASS_H)


def mass_args(species):
    return dict(mass_amu=M_AMU) if species is None else dict(mass_amu=wl.MASS_O, mass_h_amu=wl.MASS_H, species=species)


def device_noise(eng, pos, n_steps, seed, first_step, species=None):
    """xi of step first_step + n_steps - 1, recovered from the velocities of a run that starts at rest."""
    x = torch.from_numpy(pos).float().cuda()
    v, f = torch.zeros_like(x), torch.zeros_like(x)
    eng.md_run(x, v, f, n_steps, temperature_k=T_K, seed=seed, first_step=first_step, **mass_args(species), **FAST)
    assert torch.count_nonzero(f).item() == 0                   # force-free, or nothing below means what it says
    v = v.cpu().double().numpy()
    assert np.isfinite(v).all()
    return v / nr.noise_scale_f32(masses(pos.shape[0], species), temperature_k=T_K, **FAST).reshape(-1, 1)


@pytest.mark.parametrize("case,n,skin,n_boxes,two_masses", nr.DEVICE_CASES, ids=[c[0] for c in nr.DEVICE_CASES])
def test_one_step_noise_is_the_restatement(engines, case, n, skin, n_boxes, two_masses):
    eng, pos, _ = engines(n, skin, n_boxes)
    species = species_of(n * n_boxes) if two_masses else None
    seed, step = nr.DEVICE_SEED, nr.DEVICE_STEP
    xi = device_noise(eng, pos, 1, seed, step, species)
    ref = nr.box_noise(seed, step, n, n_boxes)
    err = float(np.abs(xi - ref).max())
    print(f"noise parity {case}: max |xi_dev - xi_ref| {err:.3e} over {xi.size} numbers (largest |xi| {np.abs(ref).max():.2f})")
    assert xi.shape == ref.shape and err <= TOL
    if n_boxes > 1:                                               # the batch rule, said once more in the device's own terms
        one, pos1, _ = engines(n, skin, 1)
        for b in range(n_boxes):
            assert np.array_equal(xi[b * n:(b + 1) * n], device_noise(one, pos1, 1, seed + b, step)), b


@pytest.mark.parametrize("skin", [False, True], ids=["no_skin", "skin"])
def test_classical_force_source_draws_the_same_noise(skin):
    """The Lennard-Jones force source with epsilon = 0 is force-free too, and its steps go through the same launchers."""
    from gamd_amd.engine import GamdForce
    n, seed, step = 258, 11, 7
    pos, box = wl.lj_box(n, seed=3)
    eng = GamdForce(free_state_dict(), n, box, RC, neighbor_skin=RC / 6.0 if skin else 0.0)
    eng.classical_configure(0, epsilon=0.0)
    eng.md_force_source("classical")
    assert torch.count_nonzero(eng.classical_forces(pos)[0]).item() == 0
    err = float(np.abs(device_noise(eng, pos, 1, seed, step) - nr.box_noise(seed, step, n)).max())
    print(f"noise parity classical source ({'skin' if skin else 'no skin'}): max |xi_dev - xi_ref| {err:.3e}")
    assert err <= TOL
    eng.close()


@pytest.mark.parametrize("skin", [False, True], ids=["baoab_first", "step_small"])
@pytest.mark.parametrize("word", ["seed", "first_step"])
@pytest.mark.parametrize("value", nr.WORD_VALUES, ids=["5", "2^32+5", "2^63+5"])
def test_seed_and_step_enter_as_64_bit_words(engines, value, word, skin):
    """4 steps per run: the run's last step is first_step + 3, counted on the host in 64 bits and split into two counter words
    on the device; the seed is split into the two key words."""
    n, last = nr.WORD_N, nr.WORD_STEPS - 1
    eng, pos, _ = engines(n, skin)
    seed, first = nr.word_case(value, word)
    xi = device_noise(eng, pos, nr.WORD_STEPS, seed, first)
    err = float(np.abs(xi - nr.box_noise(seed, first + last, n)).max())
    print(f"noise parity {word} = {value} ({'skin' if skin else 'no skin'}), step first + 3: max |xi_dev - xi_ref| {err:.3e}")
    assert err <= TOL
    if value >> 32:                                               # ... and not what the low word alone would draw
        low_seed, low_first = nr.word_case(value & 0xffffffff, word)
        assert np.all(np.any(np.abs(xi - nr.box_noise(low_seed, low_first + last, n)) > 1e-3, axis=1))


@pytest.mark.parametrize("skin", [False, True], ids=["no_skin", "skin"])
@pytest.mark.parametrize("two_masses", [False, True], ids=["one_mass", "o_h_masses"])
def test_ou_recursion_of_free_atoms(engines, two_masses, skin):
    """a = exp(-gamma dt) = 0.951 and b = sqrt(1 - a^2) held together at T = 300 K: 40 force-free steps in chunks of 1, 7 and 32
    against the float64 recursion v <- a v + bs xi_ref(step), x <- x + (dt/2)(v_before + v_after); everything of the reference
    in float64 from the parameters, nothing taken from the device.

    The box is 15.7 A (rho* = 2.6; the model is force-free, the density means nothing), below 16 A on purpose: what the position
    check resolves is set by the rounding of the stored x, 80 additions of up to half an ulp each over the run, and ulp(x) is
    9.5e-7 A below 16 A against 1.9e-6 A in the 27 A box of rho* = 0.5, where that random walk alone reaches 1.6e-5 .. 2.0e-5 A over
    the 774 coordinates (measured) and leaves the 2e-5 A bound no room to see anything else."""
    n, seed, dt, gamma = 258, 23, 0.002, 25.0
    eng, pos, box = engines(n, skin, rho_star=2.6, rc=6.0)
    assert box < 16.0
    species = species_of(n) if two_masses else None
    a = math.exp(-gamma * dt)
    bs = (math.sqrt(1.0 - a * a) * 10.0 * np.sqrt(wl.KB * T_K / masses(n, species))).reshape(-1, 1)
    assert abs(a - 0.951) < 5e-4
    x0 = torch.from_numpy(pos).float()
    xr, vr = x0.double().numpy(), np.zeros((n, 3))
    x, v, done = x0.cuda(), torch.zeros(n, 3, device="cuda"), 0
    worst_v = worst_x = 0.0
    for chunk in (1, 7, 32):
        f = torch.zeros_like(x)
        eng.md_run(x, v, f, chunk, dt_ps=dt, gamma_per_ps=gamma, temperature_k=T_K, seed=seed, first_step=done, **mass_args(species))
        assert torch.count_nonzero(f).item() == 0
        for s in range(done, done + chunk):
            v_new = a * vr + bs * nr.box_noise(seed, s, n)
            xr = xr + 0.5 * dt * (vr + v_new)
            vr = v_new
        done += chunk
        ev = rel_err(v.cpu().numpy(), vr)
        d = x.cpu().double().numpy() - xr
        d -= box * np.round(d / box)
        ex = float(np.abs(d).max())
        print(f"OU recursion {'O/H masses' if two_masses else 'one mass'}, {'skin' if skin else 'no skin'}, after {done} steps: "
              f"v rel_err {ev:.3e}, max |dx| {ex:.3e} A")
        worst_v, worst_x = max(worst_v, ev), max(worst_x, ex)
        assert ev < 1e-5 and ex < 2e-5, (done, ev, ex)
    assert done == 40
    print(f"OU recursion {'O/H masses' if two_masses else 'one mass'}, {'skin' if skin else 'no skin'}: worst v rel_err {worst_v:.3e}, "
          f"worst |dx| {worst_x:.3e} A")
