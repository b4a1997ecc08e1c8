// Host arithmetic of bds_probe_data* (csrc/bds_probedata.hip): the record formats, pwelch's segment count, the cut of a window
// into pieces whose seams fall on segment starts, the window and twiddle tables, the argument checks and the last step from the
// f64 sums to the density.  Plain C++, no HIP: tests/host_models/probe_math_check.cpp runs it under the sanitizers.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bds_mi355x.h"

namespace bds {
namespace probe {

constexpr int kNfft = 32768;              // pwelch(data, 32768, 2048, 32768, fs): window = nfft   (B2a/include/probeData.m:128,131)
constexpr int kOverlap = 2048;
constexpr int kHop = kNfft - kOverlap;    // 30720: segment k starts at sample 30720 k
constexpr int kN1 = 8, kN2 = 4096;        // the transform's factorisation 32768 = 8 x 4096
constexpr int kBins = 257;                // hist(data, -128:128)                                  (probeData.m:146)
constexpr double kPi = 3.14159265358979323846264338327950288;

enum Format { kS8 = 0, kS8C = 1, kPacked = 2, kS16 = 3, kS16C = 4 };

// fileType / dataType -> format, by the rule of bds_track; < 0 = BDS_ERR_*, with the message in `why`
inline int format_of(const bds_settings &s, const char **why) {
    *why = "";
    if (s.dataType != 0 && s.dataType != 1) {
        *why = "settings.dataType must be 0 ('schar') or 1 ('int16')";
        return BDS_ERR_UNSUPPORTED;
    }
    if (s.fileType == 1) return s.dataType ? kS16 : kS8;
    if (s.fileType == 2) return s.dataType ? kS16C : kS8C;
    if (s.fileType == 3) {
        if (s.dataType == 0) return kPacked;
        *why = "settings.fileType 3 (packed 2+2-bit I/Q) goes with dataType 0 only";
        return BDS_ERR_ARG;
    }
    *why = "settings.fileType must be 1, 2 or 3";
    return BDS_ERR_ARG;
}
inline bool is_complex(int fmt) { return fmt == kS8C || fmt == kPacked || fmt == kS16C; }
inline int bits_per_sample(int fmt) { return fmt == kS8 ? 8 : fmt == kPacked ? 4 : fmt == kS16C ? 32 : 16; }
// bytes a record must be a whole multiple of (an odd byte count of an I/Q or 16-bit record is an error)
inline int byte_unit(int fmt) { return fmt == kS16C ? 4 : (fmt == kS8C || fmt == kS16) ? 2 : 1; }
// alignment the decoder needs of the record's first byte (the element size)
inline int elem_bytes(int fmt) { return (fmt == kS16 || fmt == kS16C) ? 2 : 1; }
inline int64_t samples_in_bytes(int fmt, uint64_t n_bytes) { return (int64_t)(n_bytes * 8 / (uint64_t)bits_per_sample(fmt)); }
// the bytes that hold samples [a, b) of a record whose sample 0 is the low end of byte 0
inline void byte_span(int fmt, int64_t a, int64_t b, int64_t *first, int64_t *end) {
    const int64_t bits = bits_per_sample(fmt);
    *first = a * bits / 8;
    *end = (b * bits + 7) / 8;
}

// K = fix((L - noverlap) / (nfft - noverlap)); 0 when not one segment fits
inline int64_t segments(int64_t n) { return n < kNfft ? 0 : (n - kOverlap) / kHop; }
inline int psd_bins(int fmt) { return is_complex(fmt) ? kNfft : kNfft / 2 + 1; }

// n_samples = 0 of bds_probe_data_file: what the signal's own probeData.m reads
//   B2a/include/probeData.m:76   fread(fid, [1, dataAdaptCoeff*5*samplesPerCode], ...)
//   B1C/include/probeData.m:76   fread(fid, [1, dataAdaptCoeff*10*samplesPerCode], ...)
inline int64_t reference_window(const bds_settings &s) {
    const double spc = std::floor(s.samplingFreq / (s.codeFreqBasis / s.codeLength) + 0.5);
    return (int64_t)spc * (s.signal == BDS_SIGNAL_B1C ? 10 : 5);
}

// Piece j of a window of n samples cut every seg_per_piece segments.  The seams fall on segment starts: a piece transforms
// segments [seg0, seg1), counts samples [hist0, hist1) into the histogram (the pieces' ranges tile [0, n): the last takes the
// tail no segment covers) and needs samples [load0, load1) on the device (its last segment runs 2048 samples into the next piece).
struct Piece {
    int64_t seg0, seg1, hist0, hist1, load0, load1;
};
inline int64_t piece_count(int64_t n, int64_t seg_per_piece) {
    const int64_t k = segments(n);
    return k <= 0 ? 0 : (k + seg_per_piece - 1) / seg_per_piece;
}
inline Piece piece(int64_t n, int64_t seg_per_piece, int64_t j) {
    const int64_t k = segments(n);
    Piece p;
    p.seg0 = j * seg_per_piece;
    p.seg1 = p.seg0 + seg_per_piece < k ? p.seg0 + seg_per_piece : k;
    const bool last = p.seg1 == k;
    p.hist0 = p.load0 = p.seg0 * kHop;
    p.hist1 = last ? n : p.seg1 * kHop;
    p.load1 = last ? n : (p.seg1 - 1) * kHop + kNfft;
    return p;
}
// segments per piece: the caller's limit, else as many as 256 MiB of the record hold
inline int64_t default_piece_segments(int fmt, int64_t limit) {
    if (limit > 0) return limit;
    const int64_t samples = ((int64_t)256 << 20) * 8 / bits_per_sample(fmt);
    return (samples - kOverlap) / kHop;
}

// symmetric Hamming window of 32768, w[n] = 0.54 - 0.46 cos(2 pi n / 32767), in f64 and rounded once to fp32; returns sum w^2 (f64 window)
inline double window(std::vector<float> &w32) {
    w32.resize(kNfft);
    double s2 = 0;
    for (int n = 0; n < kNfft; ++n) {
        const double w = 0.54 - 0.46 * std::cos(2.0 * kPi * (double)n / (double)(kNfft - 1));
        w32[n] = (float)w;
        s2 += w * w;
    }
    return s2;
}
// exp(-2 pi i m / len), m = 0 .. count - 1, as (re, im) fp32 pairs rounded once from f64
inline void twiddles(int len, int count, std::vector<float> &t) {
    t.resize((size_t)2 * count);
    for (int m = 0; m < count; ++m) {
        const double a = -2.0 * kPi * (double)m / (double)len;
        t[2 * m] = (float)std::cos(a);
        t[2 * m + 1] = (float)std::sin(a);
    }
}

// sums over the segments, in the kernel's [k1][k2] layout (bin k = k1 + 8 k2; nk2 entries per k1) -> density per Hz in natural order
inline void finish_psd(int fmt, const double *acc, int nk2, int64_t k_seg, double fs, double sum_w2, double *psd) {
    const int nb = psd_bins(fmt);
    const double scale = 1.0 / (fs * sum_w2);
    for (int k = 0; k < nb; ++k) {
        double v = acc[(size_t)(k & (kN1 - 1)) * nk2 + (k >> 3)] / (double)k_seg * scale;
        if (!is_complex(fmt) && k != 0 && k != kNfft / 2) v *= 2.0;
        psd[k] = v;
    }
}

// The argument checks every entry makes before any device work.  Returns BDS_OK or BDS_ERR_*, message in msg[len].
// n_bytes < 0: the caller counts in samples (n) already; else n is taken from the byte count, which must be whole samples
inline int check_args(const bds_settings *s, int fmt, int64_t n_bytes, int64_t n, int64_t n_time, const bds_probe_out *out, int64_t *n_samples,
                      char *msg, size_t len) {
    msg[0] = 0;
    if (!s || !out) return snprintf(msg, len, "settings or out is NULL"), BDS_ERR_ARG;
    if (n_bytes >= 0) {
        if (n_bytes % byte_unit(fmt))
            return snprintf(msg, len, "%lld bytes is not a whole number of samples (%d bytes each)", (long long)n_bytes, byte_unit(fmt)), BDS_ERR_ARG;
        n = samples_in_bytes(fmt, (uint64_t)n_bytes);
    }
    if (n < kNfft) return snprintf(msg, len, "%lld samples: pwelch needs at least one segment of %d", (long long)n, kNfft), BDS_ERR_ARG;
    if (!(s->samplingFreq > 0)) return snprintf(msg, len, "settings.samplingFreq must be positive"), BDS_ERR_ARG;
    if (!out->psd || out->cap < psd_bins(fmt)) return snprintf(msg, len, "out->psd holds %d bins, the record takes %d", out->psd ? out->cap : 0, psd_bins(fmt)), BDS_ERR_ARG;
    if (!out->hist_i || (is_complex(fmt) && !out->hist_q)) return snprintf(msg, len, "out->hist_i / hist_q is NULL"), BDS_ERR_ARG;
    if (n_time < 0 || n_time > n) return snprintf(msg, len, "n_time = %lld is outside the %lld samples", (long long)n_time, (long long)n), BDS_ERR_ARG;
    if (n_time && (!out->excerpt_re || (is_complex(fmt) && !out->excerpt_im))) return snprintf(msg, len, "out->excerpt_re / excerpt_im is NULL"), BDS_ERR_ARG;
    *n_samples = n;
    return BDS_OK;
}

}  // namespace probe
}  // namespace bds
