"""The numpy restatement of the Langevin noise (tests/md_noise_ref.py) checked against published known answers and against the
normal law, and the criteria shown to discriminate.  CPU only; tests/test_gpu_md_noise.py holds the device to this restatement.

(a) philox4x32_10 reproduces the Random123 known-answer vectors; (b) the stream of seed 11, steps 0..63, 4096 atoms
(N = 786 432 numbers, nothing random in the test) passes every distribution criterion; (c) the words that matter do matter;
(d) every mutant of md_noise_ref.MUTANTS -- a subtly wrong generator -- breaks at least one criterion."""
import math

import numpy as np
import pytest
import torch

import md_noise_ref as nr

SEED, STEPS, ATOMS = 11, range(64), 4096
Z_MAX, P_MIN = 5.0, 1e-3

# Random123 kat_vectors, philox4x32 with 10 rounds: counter, key -> output
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


# ---- statistics --------------------------------------------------------------------------------------------------------
def _corr(a, b):
    a, b = np.ravel(a), np.ravel(b)
    with np.errstate(invalid="ignore"):
        return float(np.corrcoef(a, b)[0, 1]) * math.sqrt(a.size)       # Pearson r of independent samples: standard error 1/sqrt(n)


def _kolmogorov_p(d, n):
    """P(D_n > d) by the limiting series; at n >= 2.6e5 the finite-n correction is far below what the criterion resolves."""
    lam = (math.sqrt(n) + 0.12 + 0.11 / math.sqrt(n)) * d
    if not lam > 0.2:
        return 1.0 if lam == lam else 0.0
    return float(min(1.0, max(0.0, 2.0 * sum((-1) ** (k - 1) * math.exp(-2.0 * k * k * lam * lam) for k in range(1, 101)))))


def _ks(sample, cdf):
    s = np.sort(np.ravel(sample))
    if not np.isfinite(s).all():
        return 0.0
    n = s.size
    f = cdf(s)
    d = max(float(np.max(np.arange(1, n + 1) / n - f)), float(np.max(f - np.arange(0, n) / n)))
    return _kolmogorov_p(d, n)


def _normal_cdf(x):
    return (0.5 * torch.special.erfc(-torch.from_numpy(x) / math.sqrt(2.0))).numpy()


def _exp2_cdf(x):
    return -np.expm1(-0.5 * x)


def distribution(xi, other):
    """xi, other: [steps, atoms, 3] streams of two seeds.  Returns (z-scores, KS p-values, all finite) by name; a z-score is the
    statistic over its standard error under the null hypothesis of independent standard normals."""
    n = xi.size
    flat = xi.ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        mean, var = flat.mean(), flat.var()
        std = (flat - mean) / math.sqrt(var) if var > 0 else flat * np.nan
        z = {"mean": mean * math.sqrt(n),
             "variance": (var - 1.0) / math.sqrt(2.0 / n),
             "skewness": (std ** 3).mean() / math.sqrt(6.0 / n),
             "excess kurtosis": ((std ** 4).mean() - 3.0) / math.sqrt(24.0 / n)}
        for a, b in ((0, 1), (0, 2), (1, 2)):
            z[f"corr {'xyz'[a]}{'xyz'[b]}"] = _corr(xi[..., a], xi[..., b])
        for a in (0, 1):
            z[f"corr {'xy'[a]}^2 z^2"] = _corr(xi[..., a] ** 2, xi[..., 2] ** 2)
        for d in range(3):
            z[f"step lag-1 {'xyz'[d]}"] = _corr(xi[:-1, :, d], xi[1:, :, d])
            z[f"atom lag-1 {'xyz'[d]}"] = _corr(xi[:, :-1, d], xi[:, 1:, d])
        z["corr with seed + 1"] = _corr(xi, other)
        p3 = math.erfc(3.0 / math.sqrt(2.0))
        z["|xi| > 3"] = (np.count_nonzero(np.abs(flat) > 3.0) / n - p3) / math.sqrt(p3 * (1.0 - p3) / n)
        p = {"KS all": _ks(flat, _normal_cdf)}
        for d in range(3):
            p[f"KS {'xyz'[d]}"] = _ks(xi[..., d], _normal_cdf)
        p["KS x^2 + y^2"] = _ks(xi[..., 0] ** 2 + xi[..., 1] ** 2, _exp2_cdf)
    return {k: float(v) for k, v in z.items()}, p, bool(np.isfinite(flat).all())


# ---- the criteria, each returning the names of what it finds broken -------------------------------------------------------
def crit_known_answers(m):
    bad = []
    for k, (c, key, want) in enumerate(KNOWN_ANSWERS):
        if tuple(int(w) for w in nr.philox4x32_10(c, key, m)) != want:
            bad.append(f"known answer {k}")
    # all three at once through the array path
    c = [np.array([v[0][w] for v in KNOWN_ANSWERS]) for w in range(4)]
    key = [np.array([v[1][w] for v in KNOWN_ANSWERS]) for w in range(2)]
    got = np.stack(nr.philox4x32_10(c, key, m), axis=-1)
    if got.tolist() != [list(v[2]) for v in KNOWN_ANSWERS]:
        bad.append("known answers, vectorised")
    return bad


def crit_u01(m):
    bad = []
    one, lo = nr.u01(0xffffffff, m), nr.u01(0, m)
    if not (one.dtype == np.float32 and float(one) == 1.0):
        bad.append("u01(0xffffffff) == 1")
    if float(lo) != 2.0 ** -25:
        bad.append("u01(0) == 2^-25")
    # the TOP 24 bits count: the low byte changes nothing, bit 8 is one step of 2^-24
    if not (float(nr.u01(0x000000ff, m)) == 2.0 ** -25 and float(nr.u01(0x000001ff, m)) == 1.5 * 2.0 ** -24
            and float(nr.u01(0x80000000, m)) == 0.5 and float(nr.u01(0xffffff00, m)) == 1.0):
        bad.append("u01 reads x >> 8")
    return bad


_streams = {}


def _stream(seed, m):
    if (seed, m) not in _streams:
        _streams[(seed, m)] = nr.stream(seed, STEPS, ATOMS, m)
    return _streams[(seed, m)]


def crit_distribution(m):
    z, p, finite = distribution(_stream(SEED, m), _stream(SEED + 1, m))
    bad = [k for k, v in z.items() if not abs(v) < Z_MAX] + [k for k, v in p.items() if not v > P_MIN]
    return bad + ([] if finite else ["finite"])


def crit_words(m):
    bad = []
    i = np.arange(ATOMS)
    differs = lambda a, b: bool(np.all(np.any(a != b, axis=-1)))
    if not differs(nr.atom_noise(SEED, 2 ** 32 + 5, i, m), nr.atom_noise(SEED, 5, i, m)):
        bad.append("step + 2^32 differs in every atom")
    if not differs(nr.atom_noise(SEED + 2 ** 32, 5, i, m), nr.atom_noise(SEED, 5, i, m)):
        bad.append("seed + 2^32 differs in every atom")
    n, nb = 258, 3
    batch = nr.box_noise(SEED, 5, n, nb, m)
    if batch.shape != (nb * n, 3) or not all(np.array_equal(batch[b * n:(b + 1) * n], nr.atom_noise(SEED + b, 5, np.arange(n), m))
                                             for b in range(nb)):
        bad.append("box b of a batch is a single box with seed + b")
    return bad


CRITERIA = (crit_known_answers, crit_u01, crit_distribution, crit_words)


def broken(m):
    return [name for c in CRITERIA for name in c(m)]


# ---- the tests ---------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    assert crit_known_answers(None) == []


def _philox_scalar(c, k):
    """Python integers only, after the Philox paper's round: an independent path for the uint64 array arithmetic."""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xffffffff, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xffffffff]
        k = [(k[0] + 0x9E3779B9) & 0xffffffff, (k[1] + 0xBB67AE85) & 0xffffffff]
    return c


def test_array_arithmetic_is_the_integer_arithmetic():
    rng = np.random.default_rng(0)
    w = rng.integers(0, 2 ** 32, (6, 200), dtype=np.uint64)
    w[:, 0], w[:, 1], w[:, 2], w[:, 3] = 0, 0xffffffff, 0x80000000, 1
    got = np.stack(nr.philox4x32_10(w[:4], w[4:]), axis=-1)
    for j in range(w.shape[1]):
        assert got[j].tolist() == _philox_scalar([int(x) for x in w[:4, j]], [int(x) for x in w[4:, j]]), j
    assert _philox_scalar(*KNOWN_ANSWERS[2][:2]) == list(KNOWN_ANSWERS[2][2])


def test_u01_edges_and_bits():
    assert crit_u01(None) == []
    # the largest draw: u = 1, r = 0 and the noise is exactly 0, not a NaN
    u = nr.u01(np.array([0xffffffff, 0xffffff00, 0xfffffe00]))
    assert u.dtype == np.float32 and u.tolist() == [1.0, 1.0, float(np.float32(16777214.5) * np.float32(2.0 ** -24))]
    assert np.sqrt(-2.0 * np.log(np.float64(u[0]))) == 0.0
    x = np.random.default_rng(1).integers(0, 2 ** 32, 100000, dtype=np.uint64)
    u = nr.u01(x)
    assert (u > 0).all() and (u <= 1).all() and (np.diff(nr.u01(np.sort(x))) >= 0).all()


def test_atom_noise_is_the_counter_layout_of_the_header():
    """Counter (i, step lo, step hi, tag), key (seed lo, seed hi); x and y share u[0], z takes u[2] and u[3]."""
    seed, step, i = 0x0123456789abcdef, 0xfedcba9876543210, 77
    c = _philox_scalar([i, step & 0xffffffff, step >> 32, 0x47414D44], [seed & 0xffffffff, seed >> 32])
    u = [np.float64(nr.u01(w)) for w in c]
    t = [np.float64(np.float32(6.28318530717958647692) * nr.u01(w)) for w in c]
    r0, r1 = math.sqrt(-2.0 * math.log(u[0])), math.sqrt(-2.0 * math.log(u[2]))
    want = [r0 * math.cos(t[1]), r0 * math.sin(t[1]), r1 * math.cos(t[3])]
    got = nr.atom_noise(seed, step, np.array([i]))[0]
    assert np.abs(got - want).max() < 1e-15
    assert nr.atom_noise(seed, step, np.arange(80)).shape == (80, 3)
    assert np.array_equal(nr.atom_noise(seed, step, np.arange(80))[77], got)
    # seed + b wraps at 2^64 like the device's unsigned sum
    assert np.array_equal(nr.box_noise(2 ** 64 - 1, 3, 10, 2)[10:], nr.atom_noise(0, 3, np.arange(10)))


def test_distribution_of_the_restatement():
    z, p, finite = distribution(_stream(SEED, None), _stream(SEED + 1, None))
    xi = _stream(SEED, None)
    assert xi.shape == (64, 4096, 3) and xi.size == 786432
    for k, v in z.items():
        print(f"z  {k:22s} {v:+.2f}")
    for k, v in p.items():
        print(f"p  {k:22s} {v:.3f}")
    far = int(np.count_nonzero(np.abs(xi) > 4.0))
    print(f"largest |z| {max(abs(v) for v in z.values()):.2f}; smallest p {min(p.values()):.3f}; beyond 4 sigma: {far} "
          f"(expected {xi.size * math.erfc(4.0 / math.sqrt(2.0)):.1f}); largest |xi| {np.abs(xi).max():.3f}")
    assert finite
    assert all(abs(v) < Z_MAX for v in z.values()), z
    assert all(v > P_MIN for v in p.values()), p
    assert len(z) == 4 + 3 + 2 + 6 + 1 + 1 and len(p) == 5
    assert np.abs(xi).max() < 6.0                                 # what the device test's tolerance assumes


def test_kolmogorov_p_value():
    """The p-value routine on known points of the Kolmogorov law, and on a sample that is uniform by construction."""
    n = 10 ** 6
    for lam, want in ((0.8276, 0.5), (1.2238, 0.1), (1.3581, 0.05), (1.9495, 0.001)):
        assert abs(_kolmogorov_p(lam / (math.sqrt(n) + 0.12 + 0.11 / math.sqrt(n)), n) - want) < 2e-3 * max(want, 0.01) + 2e-5
    grid = (np.arange(n) + 0.5) / n
    assert _ks(grid, lambda x: x) > 0.999 and _ks(grid ** 1.01, lambda x: x) < 1e-3
    assert abs(float(_normal_cdf(np.array([1.0]))[0]) - 0.8413447460685429) < 1e-15


def test_words_that_matter():
    assert crit_words(None) == []


def test_the_restatement_breaks_no_criterion():
    assert broken(None) == []


# what each mutant must at least break (a mutant that breaks nothing is a gap in the criteria, not in the mutant)
EXPECTED = {
    "nine_rounds": "known answer 0",
    "keys_not_bumped": "known answer 1",
    "multipliers_swapped": "known answer 2",
    "step_hi_dropped": "step + 2^32 differs in every atom",
    "u01_low_bits": "u01 reads x >> 8",
    "u01_no_half": "u01(0) == 2^-25",
    "z_with_r0": "corr x^2 z^2",
    "batch_global_index": "box b of a batch is a single box with seed + b",
    "batch_one_seed": "box b of a batch is a single box with seed + b",
}


@pytest.mark.parametrize("mutant", nr.MUTANTS)
def test_a_subtly_wrong_generator_breaks_a_criterion(mutant):
    bad = broken(mutant)
    print(f"{mutant}: breaks {bad}")
    assert bad, mutant
    assert EXPECTED[mutant] in bad, (mutant, bad)
    _streams.pop((SEED, mutant), None), _streams.pop((SEED + 1, mutant), None)


@pytest.mark.parametrize("mutant", nr.MUTANTS[:6])
def test_the_device_draws_tell_a_wrong_atom_noise_from_the_right_one(mutant):
    """The mutated restatement plays the device on the very draws tests/test_gpu_md_noise.py compares: at least one of them is
    off by more than twice that test's tolerance (the device's own error, below the tolerance, cannot cover it).  Not a matter
    of course for `u01_no_half`, which moves u by 3e-8: it shows in the radius only where u is below about 2e-3."""
    worst = {}
    for label, seed, step, n, n_boxes in nr.device_draws():
        with np.errstate(invalid="ignore"):
            d = np.abs(nr.box_noise(seed, step, n, n_boxes, mutant) - nr.box_noise(seed, step, n, n_boxes))
        worst[label] = float(np.where(np.isfinite(d), d, np.inf).max())
    seen = [k for k, v in worst.items() if v > 2.0 * nr.DEVICE_TOL]
    print(f"{mutant}: seen by {len(seen)} of {len(worst)} draws; largest difference {max(worst.values()):.3e}")
    assert seen, (mutant, worst)
    if mutant == "step_hi_dropped":
        assert sorted(seen) == sorted(f"first_step={v}" for v in nr.WORD_VALUES[1:])


def test_every_mutant_is_listed():
    assert set(EXPECTED) == set(nr.MUTANTS) and len(nr.MUTANTS) == 9
    with pytest.raises(ValueError):
        nr.atom_noise(0, 0, np.arange(2), "no_such_mutant")
