"""Seeded synthetic int8 IF generator (bench / test input).

The reference ships no IF recording (README.md:91-148 lists downloads only), so
every workload here is synthetic.  The signal is written in the reference's own
code arrays and carrier conventions so that its loops lock with the documented
signs:

  B1C:  x = s_I cos(th) - s_Q sin(th),
        s_I = 1/2 D dataBOC11 - sqrt(1/11) pilotBOC61,  s_Q = sqrt(29/44) pilotBOC11 S
        (WB_tracking.m:375-380 then adds the BOC(6,1) and BOC(1,1) pilot parts
        constructively; NB_tracking.m:357 sees the pilot on Q)
  B2a:  x = D c_d sin(th) + S c_p cos(th)
        (tracking.m:309-314: data power lands in I_P = sum c imag(e^{+j th} x))

  th = 2 pi (IF + f_d) t + phi0; code rate scaled by (1 + f_d / carrFreqBasis);
  D / S = random +-1 per primary-code period; noise N(0, sigma); round + clip
  to int8.  Amplitude per satellite A = sigma sqrt(4 CN0 / fs).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class Sat:
    prn: int
    doppler: float  # Hz
    delay: float  # samples (0-based sample at which a primary-code period starts)
    phase: float  # rad
    cn0_dbhz: float = 45.0


def default_codegen():
    from . import native

    return native.gen_primary_code


def random_sats(rng, prns, spc, cn0_dbhz=45.0, max_doppler=4500.0):
    return [Sat(int(p), float(rng.uniform(-max_doppler, max_doppler)),
                float(rng.uniform(0, spc)), float(rng.uniform(0, 2 * np.pi)), cn0_dbhz)
            for p in prns]


def make_if(settings, sats, n_samples, seed=3550, sigma=20.0, codegen=None, chunk=1 << 22,
            out=None, iq_sign=0, clean=False, code_doppler=True, pilot61_secondary=False):
    """Return int8[n_samples] of real IF samples (fileType 1), or -- iq_sign = +1 / -1 --
    int8[2*n_samples] of interleaved I/Q pairs (fileType 2) holding the analytic signal
    a(t) e^{+j th} (iq_sign +1) or its conjugate (iq_sign -1).  The reference mixes with
    exp(+j th) in both acquisition.m files and B2a/tracking.m (:309) and with exp(-j th) in
    B1C/{NB,WB}_tracking.m (:320 / :341), so a complex record needs iq_sign -1 for the former
    and +1 for the latter to correlate.
    clean=True (real records only): the float64 sum of the satellites' signals, no noise, not quantised -- the caller adds
    its own noise realisations (bench.cfg4_record builds a long record from several of them).
    code_doppler=False: the code runs at the nominal rate whatever the carrier Doppler, so that a block of whole code
    periods repeats seamlessly (with the Doppler-scaled rate the code phase of such a record has a sawtooth of
    f_d / carrFreqBasis x chips per block -- 0.02 chip at 1.5 kHz, a quarter of the BOC(6,1) correlation peak's half width).
    pilot61_secondary=True: the BOC(6,1) part of the B1C pilot carries the secondary-code chip S like its BOC(1,1) part (as
    the two sub-carriers of one pilot code do on the air).  SURVEY.md section 8d's model -- the default here -- puts S on the
    BOC(1,1) part only; WB_tracking's QMBOC prompt -sqrt(4/33) p61 + sqrt(29/33) p11 then changes magnitude with S
    (measured: 0.8e11 vs 1.5e11 in |P|^2), which the moments-based C/N0 estimator reads as noise."""
    codegen = codegen or default_codegen()
    rng = np.random.default_rng(seed)
    fs = float(settings.samplingFreq)
    fc = float(settings.codeFreqBasis)
    ncode = int(settings.codeLength)
    b1c = str(settings.signal).upper() == "B1C"
    sig = "B1C" if b1c else "B2A"
    prim = {s.prn: (np.asarray(codegen(sig, "data", s.prn), dtype=np.float32),
                    np.asarray(codegen(sig, "pilot", s.prn), dtype=np.float32)) for s in sats}
    n_periods = int(np.ceil(n_samples * fc / fs / ncode)) + 3
    syms = {s.prn: (rng.choice([-1.0, 1.0], n_periods).astype(np.float32),
                    rng.choice([-1.0, 1.0], n_periods).astype(np.float32)) for s in sats}
    if clean:
        assert not iq_sign and out is None
        out = np.empty(n_samples, dtype=np.float64)
    elif out is None:
        out = np.empty(n_samples * (2 if iq_sign else 1), dtype=np.int8)
    for a in range(0, n_samples, chunk):
        b = min(n_samples, a + chunk)
        n = np.arange(a, b, dtype=np.float64)
        acc = rng.normal(0.0, sigma, b - a) if not clean else np.zeros(b - a)
        if iq_sign:
            acc = acc + 1j * rng.normal(0.0, sigma, b - a)
        for s in sats:
            amp = sigma * np.sqrt(4.0 * 10 ** (s.cn0_dbhz / 10) / fs)
            fcode = fc * (1.0 + s.doppler / float(settings.carrFreqBasis)) if code_doppler else fc
            chips = (n - s.delay) * (fcode / fs)  # code phase in chips (may be < 0)
            period = np.floor(chips / ncode)
            cph = chips - period * ncode
            ci = np.minimum(cph.astype(np.int64), ncode - 1)
            pidx = (period.astype(np.int64) + 1) % n_periods
            d_sym, p_sym = syms[s.prn][0][pidx], syms[s.prn][1][pidx]
            cd, cp = prim[s.prn][0][ci], prim[s.prn][1][ci]
            th = 2 * np.pi * np.fmod((float(settings.IF) + s.doppler) * n / fs, 1.0) + s.phase
            if b1c:
                sub2 = np.floor(cph * 2).astype(np.int64) & 1  # 0 -> -c, 1 -> +c
                boc11 = (2.0 * sub2 - 1.0)
                sub12 = np.floor(cph * 12).astype(np.int64) % 12  # ii-1 -> (-1)^ii
                boc61 = np.where(sub12 % 2 == 0, -1.0, 1.0)
                s_i = 0.5 * d_sym * cd * boc11 - np.sqrt(1 / 11) * cp * boc61 * (p_sym if pilot61_secondary else 1.0)
                s_q = np.sqrt(29 / 44) * cp * boc11 * p_sym
                base = s_i + 1j * s_q
            else:  # d sin(th) + p cos(th) = Re[(p - j d) e^{j th}]
                base = p_sym * cp - 1j * (d_sym * cd)
            z = amp * base * np.exp(1j * th)
            if iq_sign:
                acc += z if iq_sign > 0 else np.conj(z)
            else:
                acc += z.real
        if iq_sign:
            out[2 * a:2 * b:2] = np.clip(np.rint(acc.real), -127, 127).astype(np.int8)
            out[2 * a + 1:2 * b:2] = np.clip(np.rint(acc.imag), -127, 127).astype(np.int8)
        elif clean:
            out[a:b] = acc
        else:
            out[a:b] = np.clip(np.rint(acc), -127, 127).astype(np.int8)
    return out


def dme_pulses(settings, n_samples, pairs_per_s, peak, f_offset=0.0, seed=0, iq_sign=0):
    """DME / TACAN-like pulse interference for n_samples samples at settings.samplingFreq: float64[n_samples], or -- iq_sign
    = +1 / -1 -- complex128 (the analytic signal or its conjugate, as make_if's iq_sign).  Pulse pairs arrive as a Poisson process
    of pairs_per_s; a pair is two Gaussian pulses of 3.5 us width at half amplitude, 12 us apart, of amplitude `peak`, on a carrier at
    IF + f_offset with a random phase per pair.  NumPy only.  The caller adds it to a record's values and quantises again with
    clip(rint(.), -127, 127)."""
    rng = np.random.default_rng(seed)
    fs = float(settings.samplingFreq)
    span = n_samples / fs
    sig_t = 3.5e-6 / (2.0 * np.sqrt(2.0 * np.log(2.0)))  # half-amplitude width -> standard deviation
    reach = 5.0 * sig_t
    lo = -(12e-6 + reach)  # pairs that begin in front of the record still reach into it
    n_pairs = int(rng.poisson(pairs_per_s * (span - lo)))
    t0 = np.sort(rng.uniform(lo, span, n_pairs))
    phase = rng.uniform(0.0, 2.0 * np.pi, n_pairs)
    out = np.zeros(n_samples, dtype=np.complex128 if iq_sign else np.float64)
    f = float(settings.IF) + float(f_offset)
    for t, ph in zip(t0, phase):
        for tc in (t, t + 12e-6):
            a, b = max(int(np.floor((tc - reach) * fs)), 0), min(int(np.ceil((tc + reach) * fs)) + 1, n_samples)
            if b <= a:
                continue
            tt = np.arange(a, b, dtype=np.float64) / fs
            env = peak * np.exp(-0.5 * ((tt - tc) / sig_t) ** 2)
            th = 2.0 * np.pi * f * (tt - t) + ph
            if iq_sign:
                out[a:b] += env * np.exp((1j if iq_sign > 0 else -1j) * th)
            else:
                out[a:b] += env * np.cos(th)
    return out


def cw_tones(settings, n_samples, tones, first_sample=0, iq_sign=0):
    """Continuous narrow-band interferers for samples first_sample .. first_sample + n_samples - 1 at settings.samplingFreq:
    float64[n_samples], or -- iq_sign = +1 / -1 -- complex128 (the analytic signal or its conjugate, as make_if's iq_sign).
    tones: (f_offset from settings.IF [Hz], amplitude, phase [rad]) each; the sum of amplitude cos(2 pi (IF + f_offset) t + phase),
    t = n / fs.  NumPy only.  The caller adds it to a record's values and quantises again with clip(rint(.))."""
    n = int(n_samples)
    out = np.zeros(n, dtype=np.complex128 if iq_sign else np.float64)
    t = (np.arange(n, dtype=np.float64) + float(first_sample)) / float(settings.samplingFreq)
    for f_offset, amp, ph in tones:
        th = 2.0 * np.pi * (float(settings.IF) + float(f_offset)) * t + float(ph)
        if iq_sign:
            out += float(amp) * np.exp((1j if iq_sign > 0 else -1j) * th)
        else:
            out += float(amp) * np.cos(th)
    return out


def _device_format(iq_sign, clean, packed):
    if clean:
        if iq_sign or packed:
            raise ValueError("clean=True is the real float64 sum: neither iq_sign nor packed goes with it")
        return 0
    if packed:
        if not iq_sign:
            raise ValueError("a packed record is an I/Q record: give iq_sign = +1 or -1")
        return 3
    return 2 if iq_sign else 1


@dataclass
class Trajectory:
    """Code and carrier phase of every satellite of a record as piecewise cubics in the sample index (bds_synth_seg,
    include/bds_mi355x.h): segs [n_sat, n_seg] of native.SYNTH_SEG_DTYPE, segment j covering samples first + j 2^seg_log2 ..
    first + (j + 1) 2^seg_log2 - 1; prns, one per row.  trajectory() makes one from a receiver position and ephemerides; one made
    by hand (any coefficients with code[1] > 0) is as good to make_if_device."""
    segs: np.ndarray
    first: int
    seg_log2: int
    prns: np.ndarray

    def _at(self, n):
        n = np.asarray(n, dtype=np.int64)
        m = n - np.int64(self.first)
        j = m >> np.int64(self.seg_log2)
        if ((j < 0) | (j >= self.segs.shape[1])).any():
            raise ValueError("a sample outside the trajectory")
        return j, (m - (j << np.int64(self.seg_log2))).astype(np.float64)

    def code_phase(self, n, ncode=10230):
        """(code phase in [0, ncode) chips, code period) of samples n, [n_sat, ...]: the device's own operations, one rounding each."""
        j, u = self._at(n)
        g = self.segs[:, j]
        a = g["code"]
        c = ((a[..., 3] * u + a[..., 2]) * u + a[..., 1]) * u + a[..., 0]
        k = np.floor(c / float(ncode))
        return c - k * float(ncode), g["period0"] + k.astype(np.int64)

    def carrier_phase(self, n):
        """Carrier phase [cycles] of samples n, [n_sat, ...]: the polynomial's value (whole cycles of a segment's start left out)."""
        j, u = self._at(n)
        a = self.segs[:, j]["carr"]
        return ((a[..., 3] * u + a[..., 2]) * u + a[..., 1]) * u + a[..., 0]

    def carrier_rate(self, n):
        """d(carrier phase) / dn [cycles per sample] of samples n, [n_sat, ...]: carr[1] + 2 carr[2] u + 3 carr[3] u^2."""
        j, u = self._at(n)
        a = self.segs[:, j]["carr"]
        return (3.0 * a[..., 3] * u + 2.0 * a[..., 2]) * u + a[..., 1]


def trajectory(settings, ephs, rx, n_samples, tow, t0, first_sample=0, seg_log2=17):
    """The Trajectory of the record whose sample n is taken at system time tow + t0 + n / fs (the receiver clock offset is part
    of t0) by a receiver at rest at rx [m, Earth-fixed], from the satellites of ephs (eph dicts as navdecode / native.nav_fields
    give; one row each) -- bds_synth_trajectory, host only: the library's own satpos, the Earth's rotation during the travel time,
    no atmosphere.  It covers samples first_sample .. first_sample + n_samples and the up to 32 more a device call may evaluate."""
    from . import native

    ephs = list(ephs)
    n_seg = -(-(int(n_samples) + 32) >> int(seg_log2)) if 0 <= int(seg_log2) < 63 else 1
    segs = native.synth_trajectory(settings, ephs, rx, tow, t0, int(first_sample), max(n_seg, 1), int(seg_log2))
    return Trajectory(segs, int(first_sample), int(seg_log2), np.array([int(e["PRN"]) for e in ephs], dtype=np.int32))


def make_if_device(settings, sats, n_samples, seed=3550, sigma=20.0, first_sample=0, iq_sign=0, clean=False, packed=False,
                   threshold=None, code_doppler=True, pilot61_secondary=False, symbols=None, device=0, out=None, trajectory=None):
    """make_if's signal generated on the device (bds_synth): samples first_sample .. first_sample + n_samples of the record, as
    int8[n_samples] (real), int8[2 n_samples] (iq_sign = +1 / -1, as in make_if), float64[n_samples] (clean=True: no noise, not
    quantised) or uint8[n_samples / 2] (packed=True with an iq_sign: the 2+2-bit bytes of fileType 3 -- magnitude 3 where the
    int8 value exceeds `threshold`, default sigma).  Every sample is make_if's, in the same float64 operation order; the random
    stream is not: noise and symbols are counter-based (Philox4x32-10 keyed by `seed`, include/bds_mi355x.h), so sample n does not
    depend on where a call starts -- a record made in pieces equals the record made at once -- and a seed gives another record
    than make_if's.  symbols: int8 [n_sat, 2, n_sym] of +-1 (data, secondary per satellite entry; code period p reads index
    (p + 1) mod n_sym) instead of the generated ones.  out="torch": the record stays in HBM -- a torch tensor on the device
    (int8, uint8 for packed, float64 for clean; bds_synth_dev), ready for acquisition(), tracking() and TrackSession without a
    trip through host memory; the default is the NumPy array.  There is no CPU fallback.
    trajectory: a Trajectory with one row per entry of sats (bds_synth_traj): code and carrier phase of each satellite follow its
    segments -- Doppler, code Doppler and their rates with them -- in place of one constant Doppler and delay; of a Sat the prn,
    phase and cn0_dbhz are used, a non-zero doppler or delay is a ValueError, and code_doppler is ignored."""
    from .acquisition import get_context

    fmt = _device_format(iq_sign, clean, packed)
    sats = list(sats)
    if trajectory is not None:
        for k, t in enumerate(sats):
            if t.doppler != 0 or t.delay != 0:
                raise ValueError(f"satellite {k + 1}: doppler = {t.doppler}, delay = {t.delay}: with a trajectory, which sets both, they must be 0")
    return get_context(device).synth(settings, sats, first_sample, n_samples, fmt, seed=seed, sigma=sigma, iq_sign=iq_sign,
                                     threshold=threshold, code_doppler=code_doppler, pilot61_secondary=pilot61_secondary,
                                     symbols=symbols, out=out, trajectory=trajectory)


def write_if(path, settings, sats, n_samples, seed=3550, sigma=20.0, first_sample=0, iq_sign=0, clean=False, packed=False,
             threshold=None, code_doppler=True, pilot61_secondary=False, symbols=None, device=0, piece_samples=0):
    """The bytes of make_if_device(...) written to `path` (bds_synth_file): the record is generated piece by piece, the next
    piece on a second stream while the last one is copied out and written, so its length is bounded by the disk alone.  The file
    is byte-identical whatever piece_samples is (0: 64 MiB per piece)."""
    from .acquisition import get_context

    fmt = _device_format(iq_sign, clean, packed)
    get_context(device).synth_file(settings, list(sats), first_sample, n_samples, fmt, path, piece_samples=piece_samples, seed=seed,
                                   sigma=sigma, iq_sign=iq_sign, threshold=threshold, code_doppler=code_doppler,
                                   pilot61_secondary=pilot61_secondary, symbols=symbols)


# ---- navigation messages: the inverse of navdecode (plain NumPy; for tests and for users of make_if*) -------------------------
# Bit positions are the reference's own (B1C/include/ephemeris.m:66-230, B2a/include/ephemeris.m:60-310), 1-based and
# inclusive, in the 878-bit decodedNav of a B-CNAV1 frame and the 288-bit B-CNAV2 message; values are the raw integers
# (two's complement for negative ones).  Fields the reference reads from overlapping bits overlap here as well.
BCNAV1_FIELDS = {
    "PRN": (1, 6), "SOH": (7, 14), "WN": (15, 27), "HOW": (28, 35), "IODC": (36, 46), "IODE": (46, 53),
    "t_oe": (54, 64), "SatType": (65, 66), "deltaA": (67, 92), "ADot": (93, 117), "delta_n_0": (118, 134),
    "delta_n_0Dot": (135, 157), "M_0": (158, 190), "e": (191, 223), "omega": (224, 256),
    "omega_0": (257, 289), "i_0": (290, 322), "omegaDot": (323, 341), "i_0Dot": (342, 356), "C_is": (357, 372),
    "C_ic": (373, 388), "C_rs": (389, 412), "C_rc": (413, 436), "C_us": (437, 457), "C_uc": (458, 478),
    "t_oc": (479, 489), "a_0": (490, 514), "a_1": (515, 536), "a_2": (537, 547),
    "T_GDB2ap": (548, 559), "ISC_B1Cd": (560, 571), "T_GDB1Cp": (572, 583),
    "PageID": (615, 620), "HS": (621, 622), "DIF": (623, 623), "SIF": (624, 624), "AIF": (625, 625), "SISMAI": (626, 629),
    # page 1
    "alpha1": (657, 666), "alpha2": (667, 674), "alpha3": (675, 682), "alpha4": (683, 690), "alpha5": (691, 698),
    "alpha6": (699, 706), "alpha7": (707, 714), "alpha8": (715, 722), "alpha9": (723, 730),
    "A_0UTC": (731, 746), "A_1UTC": (747, 759), "A_2UTC": (760, 766), "delta_t_LS": (767, 774), "t_ot": (775, 790),
    "WN_ot": (791, 803), "WN_LSF": (804, 816), "DN": (817, 819), "delta_t_LSF": (820, 827),
    # page 3
    "GNSS_ID": (773, 775), "WN_0BGTO": (776, 788), "t_0BGTO": (789, 804), "A_0BGTO": (805, 820), "A_1BGTO": (821, 833),
    "A_2BGTO": (834, 840),
}
_B2_CLOCK = {"t_oc": (43, 53), "a_0": (54, 78), "a_1": (79, 100), "a_2": (101, 111), "IODC_MSB2": (112, 113),
             "IODC_LSB8": (114, 121)}
BCNAV2_HEAD = {"PRN": (1, 6), "MesType": (7, 12), "SOW": (13, 30)}
BCNAV2_FIELDS = {
    10: {"WN": (31, 43), "DIF": (44, 44), "SIF": (45, 45), "AIF": (46, 46), "t_oe": (62, 72), "SatType": (73, 74),
         "deltaA": (75, 100), "ADot": (101, 125), "delta_n_0": (126, 142), "delta_n_0Dot": (143, 165), "M_0": (166, 198),
         "e": (199, 231), "omega": (232, 264)},
    11: {"HS": (31, 32), "DIF": (33, 33), "SIF": (34, 34), "AIF": (36, 36), "omega_0": (43, 75), "i_0": (76, 108),
         "omegaDot": (109, 127), "i_0Dot": (128, 142), "C_is": (143, 158), "C_ic": (159, 174), "C_rs": (175, 198),
         "C_rc": (199, 222), "C_us": (223, 243), "C_uc": (244, 264)},
    30: dict(_B2_CLOCK, alpha1=(146, 155), alpha2=(156, 163), alpha3=(164, 171), alpha4=(172, 179), alpha5=(180, 187),
             alpha6=(188, 195), alpha7=(196, 203), alpha8=(204, 211), alpha9=(212, 219)),
    31: dict(_B2_CLOCK),
    32: dict(_B2_CLOCK),
    33: dict(_B2_CLOCK, WN_0BGTO=(115, 127), t_0BGTO=(128, 143), A_0BGTO=(144, 159), A_1BGTO=(160, 172), A_2BGTO=(173, 179)),
    34: {"t_oc": (65, 75), "a_0": (76, 100), "a_1": (101, 122), "a_2": (123, 133), "IODC_MSB2": (134, 135),
         "IODC_LSB8": (136, 143)},
}
BCNAV2_PREAMBLE = np.array([-1, -1, -1, 1, 1, 1, -1, 1, 1, -1, 1, 1, -1, -1, 1, -1, -1, -1, -1, 1, -1, 1, 1, 1], dtype=np.int8)
BCNAV2_SECOND = np.array([1, 1, 1, -1, 1], dtype=np.int8)
CRC24Q = 0x1864CFB  # x^24 + x^23 + x^18 + x^17 + x^14 + x^11 + x^10 + x^7 + x^6 + x^5 + x^4 + x^3 + x + 1


def _put(bits, first, last, value, name):
    w = last - first + 1
    v = int(value)
    if not -(1 << (w - 1)) <= v < (1 << w):
        raise ValueError(f"{name} = {value} does not fit {w} bits")
    v &= (1 << w) - 1
    bits[first - 1:last] = [(v >> (w - 1 - i)) & 1 for i in range(w)]


def crc24q(bits):
    """CRC-24Q of a 0 / 1 sequence, first bit first, zero initial state, no reflection -> 24 bits (uint8 0 / 1)."""
    r = 0
    for b in np.asarray(bits).astype(int).tolist() + [0] * 24:
        r = (r << 1) | b
        if r >> 24:
            r ^= CRC24Q
    return np.array([(r >> (23 - i)) & 1 for i in range(24)], dtype=np.uint8)


def bch_codeword(hyp, k, n, feedback):
    """The n code symbols (uint8 0 / 1) of the k-bit value `hyp` from the shift register of BCH21_6Decoding.m:65-89 /
    BCH51_8Decoding.m:63-87: the register starts as the value (most significant bit at the output end), the feedback is the
    XOR of the 1-based `feedback` positions."""
    reg = [(int(hyp) >> i) & 1 for i in range(k)]
    out = np.empty(n, dtype=np.uint8)
    for s in range(n):
        out[s] = reg[-1]
        f = 0
        for p in feedback:
            f ^= reg[p - 1]
        reg = [f] + reg[:-1]
    return out


def pack_bcnav1_fields(**fields):
    """878 bits (uint8 0 / 1) of a B-CNAV1 frame's decodedNav with the named raw integer fields of BCNAV1_FIELDS set (later
    names overwrite earlier ones where the reference's ranges overlap); the CRC positions are left to bcnav1_symbols."""
    bits = np.zeros(878, dtype=np.uint8)
    for name, value in fields.items():
        _put(bits, *BCNAV1_FIELDS[name], value, name)
    return bits


def pack_bcnav2_fields(MesType, **fields):
    """The 264 information bits (uint8 0 / 1) of a B-CNAV2 message of type `MesType` with the named raw integer fields set
    (PRN, SOW and the type's entries of BCNAV2_FIELDS; any other type carries PRN and SOW alone)."""
    bits = np.zeros(264, dtype=np.uint8)
    layout = dict(BCNAV2_HEAD, **BCNAV2_FIELDS.get(int(MesType), {}))
    _put(bits, *layout["MesType"], MesType, "MesType")
    for name, value in fields.items():
        _put(bits, *layout[name], value, name)
    return bits


def bcnav1_symbols(bits878, fill=None):
    """One B-CNAV1 frame as 1800 symbols (int8 +-1, +1 = bit 1, the sign BCNAV1decoding.m:105 reads): BCH(21,6) of bits 1..6,
    BCH(51,8) of bits 7..14, sub-frame 2 = bits 15..590 + CRC-24Q + 600 parity symbols, sub-frame 3 = bits 615..854 + CRC-24Q +
    264 parity symbols, interleaved as the 36 x 48 block of :146-154.  The LDPC parity halves are not computed (nothing reads
    them): they are `fill` (864 values 0 / 1: 600 for sub-frame 2, then 264) or zeros."""
    b = np.asarray(bits878, dtype=np.uint8).reshape(-1)
    if b.size != 878:
        raise ValueError("bcnav1_symbols: 878 bits")
    fill = np.zeros(864, dtype=np.uint8) if fill is None else np.asarray(fill, dtype=np.uint8).reshape(-1)
    if fill.size != 864:
        raise ValueError("bcnav1_symbols: fill has 600 + 264 values")
    val = lambda x: int("".join(map(str, x.tolist())), 2)  # noqa: E731
    s1 = np.concatenate([bch_codeword(val(b[:6]), 6, 21, (2, 4, 5, 6)), bch_codeword(val(b[6:14]), 8, 51, (1, 4, 5, 6, 7, 8))])
    f2 = np.concatenate([b[14:590], crc24q(b[14:590]), fill[:600]])
    f3 = np.concatenate([b[614:854], crc24q(b[614:854]), fill[600:]])
    rows3 = np.arange(2, 35, 3)  # 0-based rows of Frame3Colum = 3:3:35
    rows2 = np.setdiff1d(np.arange(36), rows3)
    block = np.empty((36, 48), dtype=np.uint8)
    block[rows2] = f2.reshape(25, 48)
    block[rows3] = f3.reshape(11, 48)
    bits = np.concatenate([s1, block.reshape(-1, order="F")])
    return (2 * bits.astype(np.int8) - 1).astype(np.int8)


def bcnav2_symbols(bits264):
    """One B-CNAV2 message as 3000 one-millisecond symbols (int8 +-1): the 24-symbol preamble, the 264 bits + CRC-24Q (bit 1 =
    symbol -1, BCNAV2decoding.m:136), 288 zero parity symbols (not computed, as above), each times the five-chip secondary
    code [1 1 1 -1 1] (:69)."""
    b = np.asarray(bits264, dtype=np.uint8).reshape(-1)
    if b.size != 264:
        raise ValueError("bcnav2_symbols: 264 bits")
    msg = np.concatenate([b, crc24q(b), np.zeros(288, dtype=np.uint8)])
    sym = np.concatenate([BCNAV2_PREAMBLE, (1 - 2 * msg.astype(np.int8)).astype(np.int8)])
    return np.kron(sym, BCNAV2_SECOND).astype(np.int8)
