// What bds_blank* (csrc/bds_blank.hip) shares between the host and the device: the flag rule of the pulse blanker, the tile
// length, the argument checks every entry makes before any device call and the cut of a window into pieces with their context.
// Plain C++ on the host, __host__ __device__ under hipcc.  DESIGN.md section 2g describes the rule and the seams.
#pragma once

#include <cstdint>
#include <cstdio>

#include "bds_mi355x.h"
#include "bds_probe_math.h"
#include "bds_record_window.h"

#ifdef __HIPCC__
#define BDS_BLANK_HD __host__ __device__ __forceinline__
#else
#define BDS_BLANK_HD inline
#endif

namespace bds {
namespace blank {

using probe::kS16;
using probe::kS16C;
using probe::kS8;
using probe::kS8C;

constexpr int kTile = BDS_BLANK_TILE;        // samples per tile of the summary and apply kernels, every format
constexpr int kMaxWindow = BDS_BLANK_MAX_WINDOW;
constexpr int64_t kNoLast = -((int64_t)1 << 60), kNoNext = (int64_t)1 << 60;  // "no flagged sample before / after"

// ---- the rule ---------------------------------------------------------------------------------------------------------------------
// p = x^2 of a real sample, I^2 + Q^2 of a pair: at most 2 * 32768^2 = 2^31, exact in uint32
BDS_BLANK_HD uint32_t power(int re, int im) { return (uint32_t)(re * re) + (uint32_t)(im * im); }
BDS_BLANK_HD bool flagged(int re, int im, uint32_t threshold_sq) { return power(re, im) > threshold_sq; }
// sample n is blanked when a flagged m lies in n - post <= m <= n + pre... seen from n: last = the last flagged index <= n
// (kNoLast: none), next = the first flagged index >= n (kNoNext: none)
BDS_BLANK_HD bool blanked(int64_t n, int64_t last, int64_t next, int pre, int post) { return n - last <= post || next - n <= pre; }

// The rule on int8 records, several samples per 32-bit word (csrc/bds_blank.hip, flag_mask), with the same verdicts:
//   real   x^2 > threshold_sq  <=>  |x| > t, t = floor(sqrt(threshold_sq)); |x| <= 128, so t >= 128 flags nothing.  Per byte
//          |x| + (127 - t) reaches bit 7 exactly when |x| > t: add = 0x01010101 (127 - t), mask = 0x80808080 (0: t >= 128)
//   pairs  p = I^2 + Q^2 <= 2^15 fits 16 bits; for threshold_sq < 2^15 bit 15 of the 16-bit difference threshold_sq - p is set
//          exactly when p > threshold_sq (the difference lies in -2^15 .. 2^15 - 1); any16 = 0: threshold_sq >= 2^15 flags nothing
struct Fast8 {
    uint32_t add, mask, thr16, any16;
};
inline Fast8 fast8(uint32_t threshold_sq) {
    uint32_t t = 0;
    while (t < 128 && (t + 1) * (t + 1) <= threshold_sq) ++t;
    Fast8 f;
    f.add = t < 128 ? 0x01010101u * (127u - t) : 0u, f.mask = t < 128 ? 0x80808080u : 0u;
    f.any16 = threshold_sq < 32768u, f.thr16 = f.any16 ? threshold_sq : 0u;
    return f;
}

// ---- arguments --------------------------------------------------------------------------------------------------------------------
// fileType / dataType -> format; the packed 2+2-bit format has no amplitude to threshold
inline int format_of(const bds_settings *s, const char **why) {
    *why = "settings is NULL";
    if (!s) return BDS_ERR_ARG;
    const int fmt = probe::format_of(*s, why);
    if (fmt == probe::kPacked) {
        *why = "settings.fileType 3 (packed 2+2-bit I/Q) has no amplitude to threshold";
        return BDS_ERR_UNSUPPORTED;
    }
    return fmt;
}

// bins of the duty report for a window of n samples
inline int64_t duty_bins(int64_t n, int64_t duty_samples) { return duty_samples > 0 ? (n + duty_samples - 1) / duty_samples : 0; }

// The checks of bds_blank / bds_blank_dev / bds_blank_file on everything but the pointers' memory kind.  n_bytes < 0: the caller
// counts in samples (n) already.  BDS_OK with *n_samples = the samples of the buffer, or BDS_ERR_ARG with the message in msg.
inline int check_args(int fmt, int64_t n_bytes, int64_t n, const bds_blank_opts *o, const bds_blank_out *rep, int64_t *n_samples, char *msg, size_t len) {
    msg[0] = 0;
    if (!o || !rep) return snprintf(msg, len, "opts or report is NULL"), BDS_ERR_ARG;
    if (n_bytes >= 0) {
        if (n_bytes % probe::byte_unit(fmt))
            return snprintf(msg, len, "%lld bytes is not a whole number of samples (%d bytes each)", (long long)n_bytes, probe::byte_unit(fmt)), BDS_ERR_ARG;
        n = n_bytes / sample_bytes(fmt);
    }
    if (n < 0) return snprintf(msg, len, "%lld samples", (long long)n), BDS_ERR_ARG;
    if (o->pre < 0 || o->post < 0 || o->pre > kMaxWindow || o->post > kMaxWindow)
        return snprintf(msg, len, "pre = %d, post = %d: the hold-off window runs from 0 to %d samples each way", o->pre, o->post, kMaxWindow), BDS_ERR_ARG;
    if (o->lead < 0 || o->tail < 0 || o->lead > n || o->tail > n - o->lead)
        return snprintf(msg, len, "lead = %lld and tail = %lld do not fit the %lld samples", (long long)o->lead, (long long)o->tail, (long long)n), BDS_ERR_ARG;
    if (o->duty_samples < 0 || o->duty_samples > INT32_MAX)
        return snprintf(msg, len, "duty_samples = %lld is outside 0 .. 2^31 - 1", (long long)o->duty_samples), BDS_ERR_ARG;
    const int64_t bins = duty_bins(n - o->lead - o->tail, o->duty_samples);
    if (bins && (!rep->duty || rep->duty_cap < bins))
        return snprintf(msg, len, "report->duty holds %lld bins, the window takes %lld", (long long)(rep->duty ? rep->duty_cap : 0), (long long)bins), BDS_ERR_ARG;
    *n_samples = n;
    return BDS_OK;
}

// ---- pieces ------------------------------------------------------------------------------------------------------------------------
// A window [w0, w1) of a buffer of n samples, worked on `piece` samples at a time.  Piece j owns (writes and counts) [core0, core1)
// and is loaded with its context: post + 1 samples before (post for the bytes; the one more gives the blanked state of the sample in
// front of the piece, by which a run that crosses the seam is counted once, in the piece where it begins) and pre samples behind,
// as far as the buffer goes.
struct Piece {
    int64_t core0, core1, load0, load1;
};
inline int64_t piece_count(int64_t w0, int64_t w1, int64_t piece) { return w1 > w0 ? (w1 - w0 + piece - 1) / piece : 0; }
inline Piece piece_of(int64_t n, int64_t w0, int64_t w1, int64_t piece, int pre, int post, int64_t j) {
    Piece p;
    p.core0 = w0 + j * piece;
    p.core1 = p.core0 + piece < w1 ? p.core0 + piece : w1;
    p.load0 = p.core0 - post - 1 > 0 ? p.core0 - post - 1 : 0;
    p.load1 = p.core1 + pre < n ? p.core1 + pre : n;
    return p;
}
// samples per piece: the caller's, else 64 MiB of the record
inline int64_t default_piece(int fmt, int64_t piece_samples) { return piece_samples > 0 ? piece_samples : ((int64_t)64 << 20) / sample_bytes(fmt); }

}  // namespace blank
}  // namespace bds
