"""The tone excisor's model and cases (shared by tests/test_notch_cases.py and tests/test_notch_gpu.py): the rule of
include/bds_mi355x.h "tone excision" restated in NumPy int64, once straight from the definition sample by sample and once
vectorised, the four record formats, and the builders of the records the device is held to."""
from types import SimpleNamespace

import numpy as np

import bds_amd
from bds_amd import native, synth

P = native.NOTCH_PHASE_BITS
L = 1 << native.NOTCH_LO_LOG2
M32 = (1 << 32) - 1

# name -> (fileType, dataType, NumPy dtype of the elements, components per sample)
FORMATS = {"s8": (1, "schar", np.int8, 1), "s8c": (2, "schar", np.int8, 2), "s16": (1, "int16", np.dtype("<i2"), 1), "s16c": (2, "int16", np.dtype("<i2"), 2)}


def settings_of(fmt, **kw):
    ft, dt, _, _ = FORMATS[fmt]
    return bds_amd.init_settings_b2a(fileType=ft, dataType=dt, **kw)


def sample_bytes(fmt):
    return np.dtype(FORMATS[fmt][2]).itemsize * FORMATS[fmt][3]


def lo_table():
    """(C, S) as int64[2^P], built as the header says: the first quadrant in float64, the rest by the symmetries of sine."""
    q = 1 << (P - 2)
    s = np.zeros(1 << P, dtype=np.int64)
    s[:q + 1] = np.rint(L * np.sin(2.0 * np.pi * np.arange(q + 1) / (1 << P))).astype(np.int64)
    s[q + 1:2 * q + 1] = s[q - 1::-1][:q]
    s[2 * q + 1:] = -s[1:2 * q]
    return s[(np.arange(1 << P) + q) % (1 << P)], s


def width(block_log2):
    """One notch width, fs / B, as a phase step."""
    return 1 << (32 - block_log2)


def floor_shift(v, k):
    return v >> k  # (Python ints and NumPy int64 both shift arithmetically)


def model_definition(rec, fmt, steps, block_log2, first_sample=0, apply=True):
    """Straight from the definition, sample by sample, in Python integers: (the notched record, report)."""
    _, _, dt, c = FORMATS[fmt]
    C, S = (t.tolist() for t in lo_table())
    x = np.asarray(rec).astype(np.int64).reshape(-1, c).tolist()
    n, B, K = len(x), 1 << block_log2, len(steps)
    lo_v, hi_v = int(np.iinfo(dt).min), int(np.iinfo(dt).max)

    def lo(k, j):
        phi = (steps[k] * ((first_sample + j) & M32)) & M32
        i = (((phi + (1 << (31 - P))) & M32) >> (32 - P)) % (1 << P)
        return C[i], S[i]

    nb = -(-n // B)
    est = np.zeros((nb, K, 2), dtype=np.int32)
    out = [list(v) for v in x]
    sat = 0
    for b in range(nb):
        a, e = b * B, min(n, b * B + B)
        r = e - a
        for k in range(K):
            sr = si = 0
            for j in range(a, e):
                cc, ss = lo(k, j)
                if c == 1:
                    sr += x[j][0] * cc
                    si -= x[j][0] * ss
                else:
                    sr += x[j][0] * cc + x[j][1] * ss
                    si += x[j][1] * cc - x[j][0] * ss
            est[b, k] = ((2 * 256 * sr + r * L) // (2 * r * L), (2 * 256 * si + r * L) // (2 * r * L))  # (// floors)
        if not apply:
            continue
        for j in range(a, e):
            er = ei = 0
            for k in range(K):
                cc, ss = lo(k, j)
                ar, ai = int(est[b, k, 0]), int(est[b, k, 1])
                er += ar * cc - ai * ss
                ei += ar * ss + ai * cc
            y = [x[j][0] - ((er + (1 << 20)) >> 21)] if c == 1 else [x[j][0] - ((er + (1 << 21)) >> 22), x[j][1] - ((ei + (1 << 21)) >> 22)]
            z = [min(max(v, lo_v), hi_v) for v in y]
            sat += z != y
            out[j] = z
    o = np.array(out, dtype=np.int64).reshape(-1)
    rep = {"n_samples": n, "n_blocks": nb, "n_saturated": sat if apply else 0, "sum_sq_in": sum(v * v for s in x for v in s) % (1 << 64),
           "sum_sq_out": int((o * o).sum()) % (1 << 64) if apply else 0, "est": est}
    return (o.astype(dt).reshape(np.asarray(rec).shape) if apply else None), rep


def model(rec, fmt, steps, block_log2, first_sample=0, apply=True):
    """The same vectorised in int64 (uint64 for the phases): (the notched record, report)."""
    _, _, dt, c = FORMATS[fmt]
    C, S = lo_table()
    x = np.asarray(rec).astype(np.int64).reshape(-1, c)
    n, B, K = x.shape[0], 1 << block_log2, len(steps)
    nb = -(-n // B)
    starts = np.arange(0, max(n, 1), B)[:nb]
    r = np.minimum(n - starts, B).astype(np.int64) if nb else np.zeros(0, np.int64)
    idx_n = (np.arange(n, dtype=np.uint64) + np.uint64(first_sample)) & np.uint64(M32)
    est = np.zeros((nb, K, 2), dtype=np.int64)
    er, ei = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    los = []
    for k, st in enumerate(steps):
        phi = (np.uint64(st) * idx_n) & np.uint64(M32)
        i = (((phi + np.uint64(1 << (31 - P))) & np.uint64(M32)) >> np.uint64(32 - P)).astype(np.int64)
        cc, ss = C[i], S[i]
        los.append((cc, ss))
        if c == 1:
            zr, zi = x[:, 0] * cc, -x[:, 0] * ss
        else:
            zr, zi = x[:, 0] * cc + x[:, 1] * ss, x[:, 1] * cc - x[:, 0] * ss
        if nb:
            sr, si = np.add.reduceat(zr, starts), np.add.reduceat(zi, starts)
            est[:, k, 0] = np.floor_divide(512 * sr + r * L, 2 * r * L)
            est[:, k, 1] = np.floor_divide(512 * si + r * L, 2 * r * L)
    rep = {"n_samples": n, "n_blocks": nb, "n_saturated": 0, "sum_sq_in": int((x * x).sum(dtype=np.uint64)), "sum_sq_out": 0, "est": est.astype(np.int32)}
    if not apply:
        return None, rep
    blk = np.arange(n) >> block_log2
    for k, (cc, ss) in enumerate(los):
        ar, ai = est[blk, k, 0], est[blk, k, 1]
        er += ar * cc - ai * ss
        ei += ar * ss + ai * cc
    if c == 1:
        y = (x[:, 0] - ((er + (1 << 20)) >> 21))[:, None]
    else:
        y = np.stack([x[:, 0] - ((er + (1 << 21)) >> 22), x[:, 1] - ((ei + (1 << 21)) >> 22)], axis=1)
    z = np.clip(y, np.iinfo(dt).min, np.iinfo(dt).max)
    rep["n_saturated"] = int((z != y).any(axis=1).sum())
    rep["sum_sq_out"] = int((z * z).sum(dtype=np.uint64))
    return z.astype(dt).reshape(np.asarray(rec).shape), rep


def pieces(rec, fmt, steps, block_log2, piece):
    """The record worked on `piece` samples at a time (a multiple of the block), each piece told its first sample: the joined
    record, the stacked estimates and the summed integers."""
    c = FORMATS[fmt][3]
    n = np.asarray(rec).size // c
    if piece % (1 << block_log2):
        raise ValueError("a cut off the block grid")
    out, est, tot = [], [], np.zeros(4, dtype=object)
    for a in range(0, n, piece):
        o, r = model(rec[a * c:min(n, a + piece) * c], fmt, steps, block_log2, first_sample=a)
        out.append(o), est.append(r["est"])
        tot += [r["n_blocks"], r["n_saturated"], r["sum_sq_in"], r["sum_sq_out"]]
    return np.concatenate(out), np.concatenate(est), tuple(int(v) for v in tot)


def noise(fmt, n, seed=0, sigma=None):
    """n samples of rounded Gaussian noise (sigma 6 for int8, 300 for int16 by default)."""
    _, _, dt, c = FORMATS[fmt]
    sigma = (6.0 if np.dtype(dt).itemsize == 1 else 300.0) if sigma is None else sigma
    v = np.random.default_rng(seed).normal(0.0, sigma, n * c)
    return np.clip(np.rint(v), np.iinfo(dt).min, np.iinfo(dt).max).astype(dt)


def with_tones(fmt, n, steps, amp=None, seed=0, sigma=None, first_sample=0):
    """noise() plus one carrier per step (amplitude amp, default 100 / 10000, phases 0.3 + k), re-quantised."""
    _, _, dt, c = FORMATS[fmt]
    amp = (100.0 if np.dtype(dt).itemsize == 1 else 10000.0) if amp is None else amp
    v = noise(fmt, n, seed, sigma).astype(np.float64).reshape(-1, c)
    j = np.arange(n, dtype=np.float64) + first_sample
    for k, st in enumerate(steps):
        th = 2.0 * np.pi * (st / 4294967296.0) * j + 0.3 + k
        v[:, 0] += amp * np.cos(th)
        if c == 2:
            v[:, 1] += amp * np.sin(th)
    return np.clip(np.rint(v), np.iinfo(dt).min, np.iinfo(dt).max).astype(dt).reshape(-1)


def steps_for(fmt, block_log2, n_tones):
    """n_tones admitted steps: the lowest and the highest first, for I/Q a negative frequency and one exactly on the spacing limit
    of the first; the rest spread over the band at no multiple of the block rate."""
    w = width(block_log2)
    if FORMATS[fmt][3] == 1:
        base = [2 * w, (1 << 31) - 2 * w]
        lo_s, hi_s = 2 * w, (1 << 31) - 2 * w
    else:
        base = [w // 3, (1 << 32) - 7 * w - w // 5, 4 * w + w // 3]  # next to DC, a negative frequency, exactly four widths from the first
        lo_s, hi_s = 0, (1 << 32) - 1
    k = 0
    while len(base) < n_tones:
        k += 1
        cand = (lo_s + (hi_s - lo_s) * k // 9 + 12345 * k) & M32
        if all(min((cand - b) & M32, (b - cand) & M32) >= 4 * w for b in base):
            base.append(cand)
    return base[:n_tones]


def cw_scenario():
    """The jammed B2a record of the issue: settings, the clean record, the jammed one, the line's frequency and the block.  The
    clean scene is tests/test_oracle_golden.py::test_acquisition_recovers_injected_satellite's at 44 dB-Hz (as the blanker's); the
    line stands 0.4 MHz above the IF, inside the B2a main lobe, at amplitude 60 against a noise sigma of 20 (J/N = +6.5 dB)."""
    s = bds_amd.init_settings_b2a(samplingFreq=25e6, IF=6.5e6, acqSatelliteList=[9, 14], acqSearchBand=2000, fineNoncoh=5)
    spc = int(np.floor(s.samplingFreq / (s.codeFreqBasis / s.codeLength) + 0.5))
    clean = synth.make_if(s, [synth.Sat(9, -1230.0, 12345.6, 2.0, 44.0)], 8 * spc, seed=2)
    f_line = s.IF + 0.4e6 + 317.0
    cw = synth.cw_tones(s, 8 * spc, [(0.4e6 + 317.0, 60.0, 1.0)])
    jammed = np.clip(np.rint(clean.astype(np.float64) + cw), -127, 127).astype(np.int8)
    return SimpleNamespace(settings=s, spc=spc, clean=clean, jammed=jammed, f_line=f_line, amp=60.0, block=1024)
