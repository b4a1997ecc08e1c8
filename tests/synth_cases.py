"""NumPy float64 restatement of the device generator of synthetic IF records (bds_synth, csrc/bds_synth.hip and
csrc/bds_synth_math.h) for the tests: Philox4x32-10, the noise and symbol streams drawn from it, the record before quantisation
(synth.make_if's lines, satellite by satellite in list order), and the quantisers.

  noise of sample n      counter (n low, n high, 0, 0), key (seed low, seed high) -> w0..w3;
                         u1 = (((w0 2^32 + w1) >> 12) + 0.5) 2^-52 in (0, 1), u2 = ((w2 2^32 + w3) >> 11) 2^-53 in [0, 1);
                         r = sqrt(-2 log u1), g_I = r cos(2 pi u2), g_Q = r sin(2 pi u2)
  symbol                 counter (period + 1 as int64 two's complement: low, high; 1; 2 prn + component); +1 when bit 0 of w0 is set
  sample n               sum over satellites of make_if's z, then + sigma g, rint, clip to +-127
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of 32-bit words, key: two.  Returns the four output words as uint64 arrays < 2^32."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & MASK for c in counter)
    k0, k1 = (np.uint64(int(k) & 0xFFFFFFFF) for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # 32 x 32 -> 64 bits: no overflow
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & MASK, n2, p0 & MASK
        k0, k1 = np.uint64((int(k0) + W0) & 0xFFFFFFFF), np.uint64((int(k1) + W1) & 0xFFFFFFFF)
    return c0, c1, c2, c3


def _key(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return seed & 0xFFFFFFFF, seed >> 32


def noise_words(seed, n):
    """The four Philox words of samples n (global sample indices, int64 array)."""
    u = np.asarray(n, dtype=np.int64).astype(np.uint64)
    z = np.zeros_like(u)
    return philox4x32_10((u & MASK, u >> np.uint64(32), z, z), _key(seed))


def noise_uniforms(seed, n):
    w0, w1, w2, w3 = noise_words(seed, n)
    u1 = ((((w0 << np.uint64(32)) | w1) >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52
    u2 = (((w2 << np.uint64(32)) | w3) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return u1, u2


def noise_normals(seed, n):
    """(g_I, g_Q): two independent N(0, 1) values per sample."""
    u1, u2 = noise_uniforms(seed, n)
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)


def symbols(seed, period, prn, component):
    """+-1 (float64) of code periods `period` (int64 array, may be negative) of satellite prn, component 0 data / 1 secondary."""
    p = (np.asarray(period, dtype=np.int64) + 1).astype(np.uint64)  # two's complement
    w0 = philox4x32_10((p & MASK, p >> np.uint64(32), np.full_like(p, 1), np.full_like(p, prn * 2 + component)), _key(seed))[0]
    return np.where(w0 & np.uint64(1), 1.0, -1.0)


def clean_record(settings, sats, first, n_samples, seed=3550, sigma=20.0, iq=False, code_doppler=True, pilot61_secondary=False,
                 symbol_table=None, codegen=None, chunk=1 << 20):
    """The record before the noise, samples first .. first + n_samples: float64 (iq False) or complex128 (the analytic signal;
    a conjugated record is its conjugate).  synth.make_if lines 87-112 on global sample indices; symbol_table int8
    [n_sat, 2, n_sym] (index (period + 1) mod n_sym) replaces the generated symbols."""
    from bds_amd import synth

    codegen = codegen or synth.default_codegen()
    fs, fc, ncode = float(settings.samplingFreq), float(settings.codeFreqBasis), int(settings.codeLength)
    b1c = str(settings.signal).upper() == "B1C"
    sig = "B1C" if b1c else "B2A"
    prim = {s.prn: (np.asarray(codegen(sig, "data", s.prn), dtype=np.float64), np.asarray(codegen(sig, "pilot", s.prn), dtype=np.float64))
            for s in sats}
    out = np.zeros(n_samples, dtype=np.complex128 if iq else np.float64)
    for a in range(0, n_samples, chunk):
        b = min(n_samples, a + chunk)
        n = np.arange(first + a, first + b, dtype=np.float64)
        acc = np.zeros(b - a, dtype=out.dtype)
        for k, s in enumerate(sats):
            amp = sigma * np.sqrt(4.0 * 10 ** (s.cn0_dbhz / 10) / fs)
            fcode = fc * (1.0 + s.doppler / float(settings.carrFreqBasis)) if code_doppler else fc
            chips = (n - s.delay) * (fcode / fs)
            period = np.floor(chips / ncode)
            cph = chips - period * ncode
            ci = np.minimum(cph.astype(np.int64), ncode - 1)
            pint = period.astype(np.int64)
            if symbol_table is not None:
                tab = np.asarray(symbol_table)
                pidx = (pint + 1) % tab.shape[2]
                d_sym, p_sym = tab[k, 0][pidx].astype(np.float64), tab[k, 1][pidx].astype(np.float64)
            else:
                up, inv = np.unique(pint, return_inverse=True)
                d_sym, p_sym = symbols(seed, up, s.prn, 0)[inv], symbols(seed, up, s.prn, 1)[inv]
            cd, cp = prim[s.prn][0][ci], prim[s.prn][1][ci]
            th = 2 * np.pi * np.fmod((float(settings.IF) + s.doppler) * n / fs, 1.0) + s.phase
            if b1c:
                boc11 = 2.0 * (np.floor(cph * 2).astype(np.int64) & 1) - 1.0
                boc61 = np.where((np.floor(cph * 12).astype(np.int64) % 12) % 2 == 0, -1.0, 1.0)
                s_i = 0.5 * d_sym * cd * boc11 - np.sqrt(1 / 11) * cp * boc61 * (p_sym if pilot61_secondary else 1.0)
                s_q = np.sqrt(29 / 44) * cp * boc11 * p_sym
                base = s_i + 1j * s_q
            else:
                base = p_sym * cp - 1j * (d_sym * cd)
            z = amp * base * np.exp(1j * th)
            acc += z if iq else z.real
        out[a:b] = acc
    return out


def amp_sum(settings, sats, sigma=20.0):
    """Sum of the satellites' amplitudes: the scale of every bound on the clean record."""
    return float(sum(sigma * np.sqrt(4.0 * 10 ** (s.cn0_dbhz / 10) / float(settings.samplingFreq)) for s in sats))


def record_values(settings, sats, first, n_samples, seed=3550, sigma=20.0, iq_sign=0, **kw):
    """The float64 values the quantiser sees: v (real record) or (v_I, v_Q) flattened to interleaved pairs (iq_sign +1 / -1)."""
    z = clean_record(settings, sats, first, n_samples, seed=seed, sigma=sigma, iq=bool(iq_sign), **kw)
    g_i, g_q = noise_normals(seed, np.arange(first, first + n_samples, dtype=np.int64))
    if not iq_sign:
        return z + sigma * g_i
    v = np.empty(2 * n_samples)
    v[0::2] = z.real + sigma * g_i
    v[1::2] = (z.imag if iq_sign > 0 else -z.imag) + sigma * g_q
    return v


def quantise8(v):
    return np.clip(np.rint(v), -127, 127).astype(np.int8)


def near_boundary(v, margin=1e-9):
    """Where v is within `margin` of a value at which rint changes (k + 1/2; +-127.5, where the clip sets in, are among them)."""
    return np.abs(np.abs(v - np.floor(v)) - 0.5) <= margin


def make_if_symbols(settings, sats, n_samples, seed):
    """synth.make_if's own symbol draws as a table [n_sat, 2, n_periods]: default_rng(seed), per satellite data then pilot."""
    rng = np.random.default_rng(seed)
    n_periods = int(np.ceil(n_samples * float(settings.codeFreqBasis) / float(settings.samplingFreq) / int(settings.codeLength))) + 3
    tab = np.empty((len(sats), 2, n_periods), dtype=np.int8)
    for k in range(len(sats)):
        tab[k, 0] = rng.choice([-1.0, 1.0], n_periods)
        tab[k, 1] = rng.choice([-1.0, 1.0], n_periods)
    return tab
