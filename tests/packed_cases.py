"""Packed 2+2-bit I/Q records (settings.fileType 3, the input of B2a/include/unpack_cplx.m:18-30) for the tests: the inverse of the
reference's look-up tables, and a quantiser that turns the synthetic I/Q records of tests/helpers.py into that alphabet.

Layout: complex sample n is nibble n & 1 of byte n >> 1, low nibble first; per nibble bit 0 = I negative, bit 1 = Q negative,
bit 2 = |I| is 3 (else 1), bit 3 = |Q| is 3 (else 1)."""
import numpy as np

SIGMA = 20.0  # per-component noise rms of synth.make_if: the signal is far below it, so this is the record's rms per component


def pack_iq(pairs) -> np.ndarray:
    """int8 pairs (I, Q, I, Q, ...) with every value in {+-1, +-3}, an even number of samples -> uint8 packed bytes."""
    p = np.asarray(pairs)
    if p.dtype != np.int8 or p.ndim != 1 or p.size % 4:
        raise ValueError("pack_iq takes a flat int8 array of I/Q pairs holding an even number of samples")
    if not np.isin(p, (-3, -1, 1, 3)).all():
        raise ValueError("pack_iq: values outside {-3, -1, 1, 3}")
    i, q = p[0::2].astype(np.int16), p[1::2].astype(np.int16)
    nib = ((i < 0) * 1 + (q < 0) * 2 + (np.abs(i) == 3) * 4 + (np.abs(q) == 3) * 8).astype(np.uint8)
    return (nib[0::2] | (nib[1::2] << 4)).astype(np.uint8)


def quantise(x_iq, threshold=SIGMA) -> np.ndarray:
    """int8 I/Q pairs of any amplitude -> pairs in {+-1, +-3}: the sign, and magnitude 3 above one threshold near the rms (a
    2-bit sign/magnitude converter; 0 counts as positive).  An odd sample at the end is dropped: a byte holds two."""
    x = np.asarray(x_iq, dtype=np.int8)
    x = x[: x.size // 4 * 4]
    mag = np.where(np.abs(x.astype(np.int16)) > threshold, 3, 1)
    return np.where(x < 0, -mag, mag).astype(np.int8)


def uses_every_nibble(packed) -> bool:
    """A quantised record exercises the whole alphabet: all 16 nibble values occur, in both halves of a byte."""
    b = np.asarray(packed, dtype=np.uint8)
    return np.unique(b & 15).size == 16 and np.unique(b >> 4).size == 16


def packed_record(x_iq):
    """(packed uint8 bytes, the int8 I/Q pairs they unpack to) of a synthetic fileType-2 record."""
    pairs = quantise(x_iq)
    packed = pack_iq(pairs)
    assert uses_every_nibble(packed)
    return packed, pairs
