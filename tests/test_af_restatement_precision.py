"""The restatement of the reference's allele-frequency step (tests/af_restatement.py) against mpmath at 50 digits: the
transcendental pieces the device tests at large ploidy and on the log1mexp branches rely on -- log1mexp,
log10_one_minus_pow10, log10_sum_log10 over up to 1 024 values, and the log10 combination counts up to ploidy 1 023."""
import math

import numpy as np
import pytest

import af_restatement as R

ULP1 = 2.0 ** -52  # one ulp at 1.0


def _mp():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    return mpmath


def mp_log10_one_minus_pow10(mp, x):
    """log10(1 - 10^x) at mpmath's precision, each branch where it does not cancel."""
    b = mp.mpf(x) * mp.log(10)
    return (mp.log(-mp.expm1(b)) if b > -1 else mp.log1p(-mp.exp(b))) / mp.log(10)


def _pvp_gate(x):
    """log10_one_minus_pow10(x) rounds b = x * ln 10 (two roundings: relative 2^-52) before exp: where the log1p branch is
    taken the result is about -exp(b), so it carries a relative error of about |b| 2^-52 of the formula's own.  Gate: 1e-13
    plus four times that."""
    return 1e-13 + 4.0 * ULP1 * abs(x * R.LOG_10)


def test_log1mexp_against_mpmath():
    mp = _mp()
    t = R.LOG1MEXP_THRESHOLD
    worst = 0.0
    for a in [float(a) for a in -np.logspace(-17, math.log10(700.0), 1500)] + [t, math.nextafter(t, 0.0), math.nextafter(t, -1.0)]:
        want = mp.log1p(-mp.exp(a))
        worst = max(worst, float(abs((R.log1mexp(a) - want) / want)))
    assert worst <= 4 * ULP1, worst
    assert R.log1mexp(0.0) == -math.inf and math.isnan(R.log1mexp(1e-300))
    assert R.log1mexp(-800.0) == 0.0  # -exp(-800) underflows: 0 is the nearest double


def test_log10_one_minus_pow10_against_mpmath():
    mp = _mp()
    t = R.LOG1MEXP_THRESHOLD / R.LOG_10
    xs = [float(x) for x in -np.logspace(-16, math.log10(300.0), 2000)] + [t, math.nextafter(t, 0.0), math.nextafter(t, -1.0), -1e-300]
    worst = 0.0
    for x in xs:
        want = mp_log10_one_minus_pow10(mp, x)
        rel = float(abs((R.log10_one_minus_pow10(x) - want) / want))
        assert rel <= _pvp_gate(x), (x, rel)
        worst = max(worst, rel / _pvp_gate(x))
    assert worst > 0.0
    assert R.log10_one_minus_pow10(0.0) == -math.inf and math.isnan(R.log10_one_minus_pow10(1e-3))


def test_log10_sum_log10_against_mpmath():
    """Up to 1 024 values (one per genotype at ploidy 1 023), spread like log10 posteriors, with ties and -inf: within
    2^-52 (max(1, |sum|) + n) -- each term's exp10 and the sum's rounding, at most n of them."""
    mp = _mp()
    rng = np.random.default_rng(17)
    for n in (1, 2, 3, 7, 64, 65, 1024):
        for _ in range(120 if n < 1024 else 20):
            v = [float(x) for x in rng.normal(0.0, 1.0, n) * rng.choice([0.1, 3.0, 100.0, 300.0]) - rng.uniform(0.0, 300.0)]
            if n > 2 and rng.random() < 0.3:
                v[1] = v[0]
            if n > 3 and rng.random() < 0.3:
                v[2] = -math.inf
            got = R.log10_sum_log10(v)
            want = mp.log10(mp.fsum(mp.power(10, mp.mpf(x)) for x in v if x != -math.inf))
            assert float(abs(got - want)) <= ULP1 * (max(1.0, abs(float(want))) + n), (n, got, want)
    assert R.log10_sum_log10([-2.0] * 1024) == -2.0 + math.log10(1024.0)


@pytest.mark.parametrize("ploidy", [2, 21, 63, 64, 100, 255, 511, 1023])
def test_combination_counts_against_the_exact_multinomial(ploidy):
    """log10_combination_count is a difference of lgamma values (log10(1023!) ~ 2 640): within 4 ulp of log10(ploidy!) of
    log10 of the exact multinomial (measured: 2.5 ulp at most)."""
    mp = _mp()
    gate = 4.0 * math.ulp(R.log10_factorial(float(ploidy)))
    counts = [[ploidy]] + [[c, ploidy - c] for c in range(1, ploidy, max(1, ploidy // 97))]
    counts += [[ploidy // 3, ploidy // 3, ploidy - 2 * (ploidy // 3)]] if ploidy >= 3 else []
    for cs in counts:
        exact = math.factorial(ploidy)
        for c in cs:
            exact //= math.factorial(c)
        got = R.log10_combination_count(ploidy, cs)
        assert float(abs(got - mp.log10(exact))) <= gate, (ploidy, cs, got)
