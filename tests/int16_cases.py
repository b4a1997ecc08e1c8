"""16-bit IF records (settings.dataType 'int16') derived from the int8 records of tests/helpers.py.

    embed(x8)  the same values as int16: every output must equal the int8 run's bit for bit;
    scale(x8)  256 x8, exact: every correlator sum is exactly 256 x the int8 run's (the sums are linear in the samples, and a power
               of two commutes with every rounding), every scale-free output is bit-equal;
    full(x8)   256 x8 + r with seeded r uniform in [-128, 127]: both bytes of every sample carry independent bits, and a dozen
               samples sit at -32768 and 32767.

An I/Q record is its interleaved (I, Q) values: the builders work value by value, so they serve real and I/Q records alike."""
import functools

import numpy as np

from helpers import track_case

N_EXTREMES = 12  # samples of full() set to the two ends of the int16 range


def settings16(s):
    return s.copy(dataType="int16")


def embed(x8):
    x8 = np.asarray(x8)
    assert x8.dtype == np.int8
    return x8.astype(np.int16)


def scale(x8):
    x8 = np.asarray(x8)
    assert x8.dtype == np.int8
    return (x8.astype(np.int32) * 256).astype(np.int16)  # |256 x8| <= 32768, and -128 * 256 = -32768 fits


def full(x8, seed=16):
    x8 = np.asarray(x8)
    assert x8.dtype == np.int8
    rng = np.random.default_rng(seed)
    r = rng.integers(-128, 128, x8.size, dtype=np.int32)
    r[r == 0] = 1  # no multiple of 256: the low byte of every sample is in use
    v = np.clip(x8.astype(np.int32) * 256 + r, -32768, 32767)
    where = rng.choice(x8.size, N_EXTREMES, replace=False)
    v[where[0::2]] = -32768
    v[where[1::2]] = 32767
    return v.astype(np.int16)


@functools.lru_cache(maxsize=None)
def case(signal, mode, n_epochs, iq=False):
    """track_case once per shape: (int8 settings, int16 settings, x8, channels); the record is read-only."""
    s, x8, chans = track_case(signal, mode, n_epochs, iq=iq)
    x8.setflags(write=False)
    return s, settings16(s), x8, chans


CORR_FIELDS = ("I_E", "I_P", "I_L", "Q_E", "Q_P", "Q_L", "Pilot_I_P", "Pilot_Q_P", "Pilot_I_E", "Pilot_I_L", "Pilot_Q_E", "Pilot_Q_L")


def assert_scaled_results(got, want, factor=256.0):
    """trackResults of a run on scale(x8) against the run on x8: the correlator fields exactly `factor` times, every other field
    (NCO frequencies and phases, positions, discriminators, C/N0, lock detector: all ratios) bit-equal."""
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        assert sorted(vars(g)) == sorted(vars(w))
        for f, wv in vars(w).items():
            gv = getattr(g, f)
            if isinstance(wv, np.ndarray):
                np.testing.assert_array_equal(gv, wv * factor if f in CORR_FIELDS else wv, err_msg=f"channel {c} {f}")
            else:
                assert gv == wv, (c, f, gv, wv)
