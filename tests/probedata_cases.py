"""Inputs, float64 restatements and tolerances for probe_data (csrc/bds_probedata.hip), shared by tests/test_probedata_cases.py
(CPU: the restatements against scipy / numpy, the bound, the rejected variants) and tests/test_probedata_gpu.py (the kernels).
Importable without the library.

The PSD tolerance.  Per segment the kernel computes X = FFT(w x) in fp32 (u = 2^-24) and P = |X|^2 / (fs sum w^2).  The issue states
the form: the transform errs by at most delta = gamma ||w x||_2 per bin, gamma = c 15 u, so

    |P^_k - P_k| <= (2 |X_k| delta + delta^2) / (fs sum w^2)          per segment, and the mean of that over the segments,

and leaves c to the butterflies actually used.  Every output bin is a sum of the 32768 terms w[n] x[n] W^{nk}, and each term
reaches it through a fixed chain of rounded operations (k_probe_segment; -ffp-contract=off, so none is fused):

    window      w rounded once to fp32, then the product w x (x an integer below 2^24: exact)                      2   u
    8-point     one complex multiply by the table twiddle exp(-2 pi i n k1 / 32768): sqrt(5) u for the product
                (Brent, Percival, Zimmermann 2007) + u for the table entry rounded from f64                         3.24 u
                the running sum over n1 = 0 .. 7: at most 7 additions                                                7   u
    4096-point  12 radix-2 stages, each a twiddle multiply (3.24 u) and one addition (u)                            50.8 u
    power       re^2 + im^2 in fp32: 2 u relative on |X|^2, which is u on |X| to first order                         1   u
                                                                                                             m  =   64.1 u

so |X^_k - X_k| <= ((1 + u)^m - 1) sum_n |w x|_n <= 1.0001 m u sqrt(32768) ||w x||_2 (Cauchy-Schwarz): worst case, every
rounding error aligned.  Hence c = 1.0001 (m / 15) sqrt(32768) = 1.0001 x 64.07 / 15 x 181.02 = 773.3 (C_BOUND below, computed from the list).
The f64 steps behind it (the sum over segments, the division) add at most 8 x 2^-53 relative, which the tolerance carries as a
separate term.  The bound is a worst case, so measured errors sit far inside it (they grow like sqrt(log N), not like sqrt(N) log N):
each test prints its worst ratio; profiles/probedata_errors.txt keeps the figures."""
import numpy as np

NFFT, NOVERLAP, HOP, NBINS = 32768, 2048, 30720, 257
U32 = 2.0 ** -24

ROUNDINGS = {"window": 2.0, "twiddle8": np.sqrt(5.0) + 1.0, "sum8": 7.0, "stages": 12 * (np.sqrt(5.0) + 1.0 + 1.0), "power": 1.0}
PATH_ROUNDINGS = sum(ROUNDINGS.values())                      # m = 64.07
C_BOUND = 1.0001 * PATH_ROUNDINGS / 15.0 * np.sqrt(NFFT)      # c = 773.3
GAMMA = C_BOUND * 15.0 * U32
F64_SLACK = 8 * 2.0 ** -53


def window():
    """hamming(32768) of MATLAB (symmetric): w[n] = 0.54 - 0.46 cos(2 pi n / 32767)."""
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(NFFT) / (NFFT - 1))


def n_segments(n):
    """K = fix((L - noverlap) / (nfft - noverlap)) of pwelch; 0 when no segment fits."""
    return 0 if n < NFFT else (n - NOVERLAP) // HOP


def segment_spectra(x, hop=HOP, window_roll=0):
    """FFT(w x_k) of every segment, float64 / complex128: [K, 32768].  (hop and window_roll exist for the rejected variants:
    segment i is weighted with the window rolled by i window_roll samples, as if the window were indexed from the record's start.)"""
    x = np.asarray(x)
    k = n_segments(x.size)
    w = window()
    return np.stack([np.fft.fft(np.roll(w, i * window_roll) * x[i * hop:i * hop + NFFT]) for i in range(k)])


def finish(power, fs, onesided, sum_w2=None):
    """mean |X|^2 over the segments -> density per Hz, one-sided (16385 bins, doubled except DC and Nyquist) or two-sided."""
    p = power / (fs * (np.sum(window() ** 2) if sum_w2 is None else sum_w2))
    if onesided:
        p = p[:NFFT // 2 + 1].copy()
        p[1:-1] *= 2.0
    return p


def welch_model(x, fs):
    """pwelch(x, 32768, 2048, 32768, fs) for real x, pwelch(..., 'twosided') for complex x."""
    x = np.asarray(x)
    s = segment_spectra(x.astype(np.complex128 if np.iscomplexobj(x) else np.float64))
    return finish(np.mean(np.abs(s) ** 2, axis=0), fs, not np.iscomplexobj(x))


def welch_bound(x, fs):
    """The per-bin tolerance derived in the module docstring, for the same x."""
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    xs = x.astype(np.complex128 if cplx else np.float64)
    k = n_segments(x.size)
    w = window()
    s = segment_spectra(xs)
    delta = GAMMA * np.array([np.linalg.norm(w * xs[i * HOP:i * HOP + NFFT]) for i in range(k)])
    b = np.mean(2.0 * np.abs(s) * delta[:, None] + delta[:, None] ** 2, axis=0)
    return finish(b, fs, not cplx) + F64_SLACK * welch_model(x, fs)


def hist_model(v):
    """hist(v, -128:128) for integer v: bin = clamp(v, -128, 128) + 128."""
    return np.bincount(np.clip(np.asarray(v, dtype=np.int64), -128, 128) + 128, minlength=NBINS).astype(np.int64)


def stats_model(v):
    v = np.asarray(v, dtype=np.int64)
    return dict(min=int(v.min()), max=int(v.max()), sum=int(v.sum()), sumsq=int(np.sum(v * v)))


# ---- the assertion functions both test files use --------------------------------------------------------------------------------
def psd_error_ratio(got, x, fs):
    """max over the bins of |got - model| / bound (0 / 0 counts as 0: where the bound is 0 the result must be exact)."""
    ref, bound = welch_model(x, fs), welch_bound(x, fs)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.isfinite(got))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r))


def assert_psd(got, x, fs, name):
    r = psd_error_ratio(got, x, fs)
    print(f"\nprobedata_errors: {name} worst |error| / bound = {r:.3e}")
    assert r <= 1.0, (name, r)
    return r


def assert_hist(got_i, got_q, stats, x, name):
    """Exact: the histograms, their total, and min / max / sum / sum of squares per component.  stats: dict with min_i ... sumsq_q."""
    x = np.asarray(x)
    comps = [("i", np.real(x), got_i)] + ([("q", np.imag(x), got_q)] if np.iscomplexobj(x) else [])
    for c, v, got in comps:
        v = np.asarray(v).astype(np.int64)
        want = hist_model(v)
        assert np.array_equal(np.asarray(got), want), (name, c, np.flatnonzero(np.asarray(got) != want)[:8])
        assert int(np.sum(got)) == v.size, (name, c)
        for k, val in stats_model(v).items():
            assert int(stats[f"{k}_{c}"]) == val, (name, c, k, stats[f"{k}_{c}"], val)


# ---- record formats ----------------------------------------------------------------------------------------------------------------
FORMATS = ["s8", "s8c", "packed", "s16", "s16c"]   # int8 real, int8 I/Q, packed 2+2-bit I/Q, int16 real, int16 I/Q
FORMAT_SETTINGS = {"s8": (1, "schar"), "s8c": (2, "schar"), "packed": (3, "schar"), "s16": (1, "int16"), "s16c": (2, "int16")}
BITS = {"s8": 8, "s8c": 16, "packed": 4, "s16": 16, "s16c": 32}


def is_complex(fmt):
    return fmt in ("s8c", "packed", "s16c")


def pack_nibbles(z):
    """complex samples with I, Q in {+-1, +-3} -> nibble codes (unpack_cplx.m:18-30: bit 0 / 1 sign of I / Q, bit 2 / 3 magnitude 3)."""
    i, q = np.real(z).astype(np.int64), np.imag(z).astype(np.int64)
    assert set(np.unique(np.abs(i))) <= {1, 3} and set(np.unique(np.abs(q))) <= {1, 3}
    return ((i < 0) * 1 + (q < 0) * 2 + (np.abs(i) == 3) * 4 + (np.abs(q) == 3) * 8).astype(np.uint8)


def encode(fmt, x, lead=0):
    """The record's bytes (uint8) of samples x in format fmt, with `lead` samples of filler in front (what a file's
    skipNumberOfBytes, counted in samples, or a device pointer offset skips).  Filler differs from every case's data."""
    x = np.asarray(x)
    if fmt == "packed":
        nib = np.concatenate([np.full(lead, 0b1101, dtype=np.uint8), pack_nibbles(x)])
        if nib.size % 2:
            nib = np.concatenate([nib, np.zeros(1, dtype=np.uint8)])
        return (nib[0::2] | (nib[1::2] << 4)).astype(np.uint8)
    dt = np.dtype("<i2") if fmt in ("s16", "s16c") else np.dtype(np.int8)
    if is_complex(fmt):
        v = np.empty(2 * x.size, dtype=dt)
        v[0::2], v[1::2] = np.real(x).astype(dt), np.imag(x).astype(dt)
        fill = np.tile(np.array([77, -55], dtype=dt), lead)
    else:
        v, fill = x.astype(dt), np.full(lead, 99, dtype=dt)
    return np.concatenate([fill, v]).view(np.uint8)


def quantise(fmt, x):
    """Integer-valued samples the format can hold, from float / complex x (rounded, clipped; packed: sign and |.| > 20 -> 3)."""
    x = np.asarray(x)
    if fmt == "packed":
        lv = lambda v: np.where(v < 0, -1, 1) * np.where(np.abs(v) > 20, 3, 1)
        return lv(np.real(x)) + 1j * lv(np.imag(x))
    lo, hi = (-32768, 32767) if fmt in ("s16", "s16c") else (-128, 127)
    r = lambda v: np.clip(np.rint(v), lo, hi)
    return r(np.real(x)) + 1j * r(np.imag(x)) if is_complex(fmt) else r(np.real(x))


L5 = NFFT + 4 * HOP + 17  # five segments and a ragged tail
LENGTHS = [32768, 63487, 63488, L5]


def noise(n, cplx, seed, sigma=20.0):
    rng = np.random.default_rng(seed)
    g = rng.normal(0.0, sigma, n)
    return g + 1j * rng.normal(0.0, sigma, n) if cplx else g


def tone_amplitude(sigma=20.0, db=60.0):
    """Amplitude of a real tone A cos(.) at a bin centre whose one-sided PSD peak, A^2 (sum w)^2 / (2 fs sum w^2), stands `db` above
    the noise density 2 sigma^2 / fs: A = sigma sqrt(4 10^(db/10) sum w^2 / (sum w)^2) = 258 for sigma 20, 60 dB."""
    w = window()
    return sigma * np.sqrt(4.0 * 10.0 ** (db / 10.0) * np.sum(w * w) / np.sum(w) ** 2)


def tone_plus_noise(n, cplx, k_bin, seed):
    """sigma = 20 noise plus a tone 60 dB above it in the PSD, at bin k_bin (may be fractional; negative for an I/Q record, where
    A e^{j.} of the same A stands 63 dB above).  A = 258 is more than an int8 holds: quantise() clips the int8 formats at
    -128 / 127 and the packed format keeps two bits -- the test compares kernel and model on the record as quantised."""
    t = np.arange(n)
    ph = 2.0 * np.pi * k_bin * t / NFFT
    return noise(n, cplx, seed) + tone_amplitude() * (np.exp(1j * ph) if cplx else np.cos(ph))


def stepped_power(n, cplx, seed):
    """Five segments whose power steps by 10 dB each (40 dB from first to last): exercises the accumulation over segments."""
    x = noise(n, cplx, seed, sigma=1.0)
    gain = 10.0 ** (np.minimum(np.arange(n) // HOP, 4) / 2.0)
    return x * gain
