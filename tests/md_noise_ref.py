"""The Langevin noise of the BAOAB step restated in numpy (gamd_amd/csrc/gamd_md_dev.h: philox_round, philox4x32_10, u01,
atom_noise, md_box_atom), for tests/test_md_noise_reference.py (CPU) and tests/test_gpu_md_noise.py (the device against it).

Philox4x32-10 (Salmon et al., SC'11; the Random123 known answers hold it) on uint64 arrays masked to 32 bits; u01 and the angle
t = fp32(2 pi) u in np.float32, bit for bit what the device forms (contraction is off in that header); the radius
r = sqrt(-2 ln u) and the sine / cosine in float64.  What is left between the device and this file is the error of fp32 logf /
sqrtf / sinf / cosf and of two products.

`mutant` names ONE deliberate deviation (MUTANTS): a subtly wrong generator that the criteria of the CPU tests must catch."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)          # the round's two multipliers
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)          # the key's two Weyl increments
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
TAG = 0x47414D44                                                # the fourth counter word
U64 = (1 << 64) - 1
TWO_PI_F32 = np.float32(6.28318530717958647692)

MUTANTS = (
    "nine_rounds",            # 9 Philox rounds
    "keys_not_bumped",        # the key stays what it was in every round
    "multipliers_swapped",    # M1 on word 0, M0 on word 2
    "step_hi_dropped",        # counter word 2 is 0: the step enters with its low 32 bits only
    "u01_low_bits",           # u01 takes x & 0xffffff, not x >> 8
    "u01_no_half",            # u01 without the + 0.5: u = 0 is drawn
    "z_with_r0",              # z = r0 cos t1: one radius for all three components
    "batch_global_index",     # a batch draws with the atom's index in the batch, not in its box
    "batch_one_seed",         # a batch draws every box with the seed of box 0
)


# What tests/test_gpu_md_noise.py draws on the device, kept here so that tests/test_md_noise_reference.py can show on the CPU that
# these draws tell a wrong generator from the right one at the device test's tolerance.
DEVICE_TOL = 5e-6
DEVICE_SEED, DEVICE_STEP = 11, 7
# (id, atoms per box, skin, boxes, two masses): one per kernel that inlines atom_noise; 1500 > 1024 and no multiple of 256
DEVICE_CASES = [
    ("baoab_first-258", 258, False, 1, False),
    ("baoab_first-1500", 1500, False, 1, False),
    ("step_small-258", 258, True, 1, False),
    ("skin_check-1500", 1500, True, 1, False),
    ("batch-3x258", 258, False, 3, False),
    ("batch-3x258-skin", 258, True, 3, False),
    ("masses-258", 258, False, 1, True),
    ("masses-258-skin", 258, True, 1, True),
    ("masses-1500-skin", 1500, True, 1, True),
]
WORD_VALUES = [5, 2 ** 32 + 5, 2 ** 63 + 5]                     # as the seed (first step 9) and as the first step (seed 13)
WORD_N, WORD_STEPS, WORD_OTHER_SEED, WORD_OTHER_STEP = 258, 4, 13, 9


def word_case(value, word):
    """(seed, first step) of one 64-bit-word case; the step compared is first step + WORD_STEPS - 1."""
    return (value, WORD_OTHER_STEP) if word == "seed" else (WORD_OTHER_SEED, value)


def device_draws():
    """(label, seed, step, atoms per box, boxes) of every draw the device test compares number by number."""
    out = [(c[0], DEVICE_SEED, DEVICE_STEP, c[1], c[3]) for c in DEVICE_CASES]
    for word in ("seed", "first_step"):
        for v in WORD_VALUES:
            seed, first = word_case(v, word)
            out.append((f"{word}={v}", seed, first + WORD_STEPS - 1, WORD_N, 1))
    return out


def _check(mutant):
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(f"unknown mutant {mutant!r}")


def _words(x):
    return np.asarray(x, dtype=np.uint64) & MASK


def philox4x32_10(counter, key, mutant=None):
    """counter: 4 words, key: 2 words (scalars or arrays that broadcast) -> list of 4 uint64 arrays holding 32-bit words."""
    _check(mutant)
    c = [w.copy() for w in np.broadcast_arrays(*[_words(w) for w in counter])]
    k0, k1 = _words(key[0]), _words(key[1])
    m0, m1 = (M1, M0) if mutant == "multipliers_swapped" else (M0, M1)
    for _ in range(9 if mutant == "nine_rounds" else 10):
        p0, p1 = m0 * c[0], m1 * c[2]                            # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & MASK, (p0 >> S32) ^ c[3] ^ k1, p0 & MASK]
        if mutant != "keys_not_bumped":
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def u01(x, mutant=None):
    """((float)(x >> 8) + 0.5f) * 2^-24 in np.float32: in (0, 1], and x >> 8 = 2^24 - 1 rounds to 1 exactly (r = 0, no NaN)."""
    _check(mutant)
    x = _words(x)
    top = (x & np.uint64(0xFFFFFF)) if mutant == "u01_low_bits" else (x >> np.uint64(8))
    f = top.astype(np.float32)                                   # exact: below 2^24
    if mutant != "u01_no_half":
        f = f + np.float32(0.5)
    return f * np.float32(2.0 ** -24)


def atom_noise(seed, step, i, mutant=None):
    """Three standard normals per atom index in `i` (any shape) at (seed, step): float64 [..., 3]."""
    _check(mutant)
    seed, step = int(seed) & U64, int(step) & U64
    i = np.asarray(i, dtype=np.uint64)
    hi = 0 if mutant == "step_hi_dropped" else step >> 32
    c = philox4x32_10((i, step & 0xFFFFFFFF, hi, TAG), (seed & 0xFFFFFFFF, seed >> 32), mutant)
    u = [u01(w, mutant) for w in c]
    t0, t1 = TWO_PI_F32 * u[1], TWO_PI_F32 * u[3]                # one fp32 product each
    assert t0.dtype == np.float32 and u[0].dtype == np.float32
    with np.errstate(divide="ignore"):
        r0 = np.sqrt(-2.0 * np.log(u[0].astype(np.float64)))
        r1 = np.sqrt(-2.0 * np.log(u[2].astype(np.float64)))
    t0, t1 = t0.astype(np.float64), t1.astype(np.float64)
    rz = r0 if mutant == "z_with_r0" else r1
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), rz * np.cos(t1)], axis=-1)


def box_noise(seed, step, n_per_box, n_boxes=1, mutant=None):
    """The batch rule (md_box_atom): atom i of box b draws what a single box with seed + b (mod 2^64) draws for its local
    index i - b n_per_box.  float64 [n_boxes * n_per_box, 3], box-major."""
    _check(mutant)
    out = []
    for b in range(n_boxes):
        first = b * n_per_box if mutant == "batch_global_index" else 0
        s = int(seed) if mutant == "batch_one_seed" else int(seed) + b
        out.append(atom_noise(s, step, np.arange(first, first + n_per_box), mutant))
    return np.concatenate(out)


def noise_scale_f32(mass_amu, dt_ps, gamma_per_ps, temperature_k, length_per_nm=10.0):
    """bs = b_len_kT sqrtf(1 / m), the factor of xi in the O step, with the device's roundings (gamd_md_run in gamd_api.hip,
    d_baoab_first_atom): the C ABI's float parameters, a = exp(-gamma dt) and b_len_kT = sqrt(1 - a^2) len sqrt(kB T) in double
    and rounded to fp32, then 1 / m, its square root and the product in fp32, each correctly rounded.  float64 [n].
    For turning a stored velocity back into xi; a reference of the O step itself forms bs in float64 from the parameters."""
    f32 = lambda x: float(np.float32(x))
    a = np.exp(-f32(gamma_per_ps) * f32(dt_ps))
    b_len_kt = np.float32(np.sqrt(1.0 - a * a) * f32(length_per_nm) * np.sqrt(0.00831446261815324 * f32(temperature_k)))
    bs = b_len_kt * np.sqrt(np.float32(1.0) / np.asarray(mass_amu, dtype=np.float32))
    assert bs.dtype == np.float32
    return bs.astype(np.float64)


def stream(seed, steps, n_atoms, mutant=None):
    """float64 [len(steps), n_atoms, 3]: the noise of a single box over several steps."""
    return np.stack([atom_noise(seed, s, np.arange(n_atoms), mutant) for s in steps])
