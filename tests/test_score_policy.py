"""The figures of nnnoiseless_amd.score -- snr_db, si_sdr_db, segmental_snr_db -- against the formulas written out in NumPy on planted
sums, the zero-denominator cases included, and evaluate's plan.  Plain Python: no library, no device."""
import warnings

import numpy as np
import pytest

from nnnoiseless_amd import score


def test_snr_db():
    A, E = np.array([100.0, 1.0, 3.0, 7.5e9]), np.array([1.0, 100.0, 3.0, 2.5e3])
    assert np.array_equal(score.snr_db(A, E), 10.0 * np.log10(A / E))
    assert np.allclose(score.snr_db(A, E)[:3], [20.0, -20.0, 0.0], atol=1e-12)
    assert score.snr_db(100.0, 1.0) == 20.0 and score.snr_db(np.float32(100.0), 1).dtype == np.float64


def test_si_sdr_db():
    A, B, C = np.array([4.0, 9.0, 2.0e6]), np.array([9.0, 4.0, 3.0e6]), np.array([3.0, -5.0, 1.0e6])
    want = 10.0 * np.log10(C ** 2 / (A * B - C ** 2))
    assert np.array_equal(score.si_sdr_db(A, B, C), want)
    # y = 2 r + n with n orthogonal to r: the figure is |2 r|^2 / |n|^2 whatever the scale of y
    r, n = np.array([1.0, 2.0, -1.0, 0.0]), np.array([2.0, -1.0, 0.0, 5.0])
    assert r @ n == 0
    for g in (1.0, 0.25, 40.0):
        y = g * (2.0 * r + n)
        assert np.isclose(score.si_sdr_db(r @ r, y @ y, r @ y), 10.0 * np.log10(4.0 * (r @ r) / (n @ n)), atol=1e-9)


def test_zero_denominators_do_not_raise():
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # (nor warn)
        s = score.snr_db([5.0, 0.0, 0.0], [0.0, 5.0, 0.0])
        assert s[0] == np.inf and s[1] == -np.inf and np.isnan(s[2])
        q = score.si_sdr_db([4.0, 4.0, 0.0, 1.0], [9.0, 9.0, 5.0, 1.0], [6.0, 0.0, 0.0, 1.0 + 1e-9])
        assert q[0] == np.inf and q[1] == -np.inf and np.isnan(q[2]) and np.isnan(q[3])
        assert np.isnan(score.snr_db(np.nan, 1.0)) and np.isnan(score.si_sdr_db(np.nan, 1.0, 1.0))


def test_segmental_snr_db():
    # [frames, streams, 4]; stream 0: ratios 20 dB, 50 dB (above hi), -30 dB (below lo), one frame below `active`, one masked (zeros)
    fs = np.zeros((5, 3, 4))
    fs[:, 0, 0] = [480e4, 480e4, 480e2, 480 * 0.5, 0.0]
    fs[:, 0, 3] = [480e2, 480e-1, 480e5, 1.0, 0.0]
    # stream 1: an exact frame (E = 0 -> hi) and a 10 dB frame; stream 2: never active
    fs[:2, 1, 0], fs[:2, 1, 3] = [480e3, 480e3], [0.0, 480e2]
    fs[:, 2, 0], fs[:, 2, 3] = 100.0, 50.0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = score.segmental_snr_db(fs, active=1.0)
    assert np.isclose(got[0], (20.0 + 35.0 - 10.0) / 3.0) and np.isclose(got[1], (35.0 + 10.0) / 2.0) and np.isnan(got[2])
    # the formula written out, other clamps, a single stream's table
    lo, hi, active = -5.0, 25.0, 10.0
    A, E = fs[:, 0, 0], fs[:, 0, 3]
    on = A / 480.0 > active
    with np.errstate(all="ignore"):
        want = np.clip(10.0 * np.log10(A[on] / E[on]), lo, hi).mean()
    assert np.isclose(score.segmental_snr_db(fs[:, 0], lo, hi, active), want) and on.sum() == 3
    assert np.isclose(score.segmental_snr_db(fs[:, 0]), (20.0 + 35.0 - 10.0 + 10.0 * np.log10(240.0)) / 4.0)   # active = 0: every frame with A > 0


def test_evaluation_plan():
    """The same arguments give the same plan; every stream reads whole frames inside its arena; no clean signal is silenced."""
    rng = np.random.default_rng(0)
    sig = [rng.integers(-3000, 3000, n).astype(np.int16) for n in (4800, 7000, 481, 100)]
    noise = [rng.integers(-300, 300, n).astype(np.int16) for n in (9600, 500)]
    a = score.evaluation_plan(sig, noise, 70, 8, 3)
    b = score.evaluation_plan(sig, noise, 70, 8, 3)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    s, n, so, no, p = a
    assert so.shape == no.shape == (9, 8) and so.dtype == np.uint64 and p.shape == (8,)
    assert (so + 480 <= s.size).all() and (no + 480 <= n.size).all() and (p["signal_gain"] > 0).all()
    assert not np.array_equal(score.evaluation_plan(sig, noise, 70, 8, 4)[4], p)
    with pytest.raises(ValueError):
        score.evaluation_plan([], noise, 70, 8, 3)
