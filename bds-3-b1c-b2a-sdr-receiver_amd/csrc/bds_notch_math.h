// What bds_notch* (csrc/bds_notch.hip) shares between the host and the device: the rule of the tone excisor -- the phase of a
// sample, the index into the local-oscillator table, the block estimate and the subtraction, all in integers --, the table itself
// (host, f64, once), the argument checks every entry makes before any device call and the cut of a window into pieces.
// Plain C++ on the host, __host__ __device__ under hipcc: tests/host_models/notch_math_check.cpp runs it under the sanitizers.
// DESIGN.md section 2h describes the rule.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "bds_mi355x.h"
#include "bds_probe_math.h"
#include "bds_record_window.h"

#ifdef __HIPCC__
#define BDS_NOTCH_HD __host__ __device__ __forceinline__
#else
#define BDS_NOTCH_HD inline
#endif

namespace bds {
namespace notch {

using probe::kS16;
using probe::kS16C;
using probe::kS8;
using probe::kS8C;

constexpr int kP = BDS_NOTCH_PHASE_BITS;           // table of 2^P entries
constexpr int kTab = 1 << kP;
constexpr int kLoLog2 = BDS_NOTCH_LO_LOG2;         // L = 2^14: the table's amplitude
constexpr int kAmpFrac = BDS_NOTCH_AMP_FRAC;       // estimates in 1 / 256 LSB
constexpr int kMaxTones = BDS_NOTCH_MAX_TONES;
constexpr int64_t kRunBytes = BDS_NOTCH_RUN_BYTES;  // record bytes a workgroup of the two kernels takes: a run of whole blocks

// ---- the rule ---------------------------------------------------------------------------------------------------------------------
// phi(n) = step (n mod 2^32) mod 2^32; table index = ((phi + 2^(31 - P)) >> (32 - P)) mod 2^P (the uint32 sum wraps by itself)
BDS_NOTCH_HD uint32_t phase(uint32_t step, int64_t n) { return step * (uint32_t)(uint64_t)n; }
BDS_NOTCH_HD uint32_t lo_index(uint32_t phi) { return (uint32_t)(phi + (1u << (31 - kP))) >> (32 - kP); }
// floor(a / b), b > 0
BDS_NOTCH_HD int64_t floor_div(int64_t a, int64_t b) {
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
// a block's sum over r samples -> the tone's amplitude in 1 / 256 LSB: floor((2 256 S + r L) / (2 r L)); |S| <= 2^46, so the
// numerator stays below 2^56.  For r = 2^beta this is (S + 2^(beta + 5)) >> (beta + 6).
BDS_NOTCH_HD int32_t estimate(int64_t sum, int64_t r) {
    const int64_t rl = r * ((int64_t)1 << kLoLog2);
    return (int32_t)floor_div(sum * ((int64_t)2 << kAmpFrac) + rl, 2 * rl);
}
BDS_NOTCH_HD int32_t estimate_full(int64_t sum, int block_log2) { return (int32_t)((sum + ((int64_t)1 << (block_log2 + 5))) >> (block_log2 + 6)); }
// what is subtracted from a real sample (twice the real part: the projection of a real tone carries half its amplitude) and from
// each component of a pair; er, ei = sum over the tones of a x lo, at most 2^42
BDS_NOTCH_HD int32_t sub_real(int64_t er) { return (int32_t)((er + ((int64_t)1 << 20)) >> 21); }
BDS_NOTCH_HD int32_t sub_cplx(int64_t e) { return (int32_t)((e + ((int64_t)1 << 21)) >> 22); }

// ---- the table --------------------------------------------------------------------------------------------------------------------
// S[i] = rint(L sin(2 pi i / 2^P)) from the first quadrant j = 0 .. 2^(P - 2) and the exact symmetries of sine;
// C[i] = S[(i + 2^(P - 2)) mod 2^P].  cos_sin: C[0 .. 2^P), then S[0 .. 2^P).
inline void lo_table(int16_t *cos_sin) {
    int16_t *c = cos_sin, *s = cos_sin + kTab;
    constexpr int q = kTab / 4;
    for (int j = 0; j <= q; ++j) s[j] = (int16_t)std::nearbyint((double)(1 << kLoLog2) * std::sin(2.0 * probe::kPi * (double)j / (double)kTab));
    for (int i = q + 1; i <= 2 * q; ++i) s[i] = s[2 * q - i];
    for (int i = 2 * q + 1; i < kTab; ++i) s[i] = (int16_t)-s[i - 2 * q];
    for (int i = 0; i < kTab; ++i) c[i] = s[(i + q) & (kTab - 1)];
}

// ---- arguments --------------------------------------------------------------------------------------------------------------------
inline int format_of(const bds_settings *s, const char **why) {
    *why = "settings is NULL";
    if (!s) return BDS_ERR_ARG;
    const int fmt = probe::format_of(*s, why);
    if (fmt == probe::kPacked) {
        *why = "settings.fileType 3 (packed 2+2-bit I/Q) has no amplitude to subtract from";
        return BDS_ERR_UNSUPPORTED;
    }
    return fmt;
}

inline uint32_t circ_dist(uint32_t a, uint32_t b) {
    const uint32_t d = a - b, e = b - a;
    return d < e ? d : e;
}
inline int64_t block_count(int64_t n, int block_log2) { return (n + ((int64_t)1 << block_log2) - 1) >> block_log2; }

// The checks of bds_notch / bds_notch_dev / bds_notch_file on everything but the pointers.  n_bytes < 0: the caller counts in
// samples (n) already.  BDS_OK with *n_samples = the samples of the window, or BDS_ERR_ARG with the message in msg.
inline int check_args(int fmt, int64_t n_bytes, int64_t n, const bds_notch_opts *o, const bds_notch_out *rep, int64_t *n_samples, char *msg, size_t len) {
    msg[0] = 0;
    if (!o || !rep) return snprintf(msg, len, "opts or report is NULL"), BDS_ERR_ARG;
    if (n_bytes >= 0) {
        if (n_bytes % probe::byte_unit(fmt))
            return snprintf(msg, len, "%lld bytes is not a whole number of samples (%d bytes each)", (long long)n_bytes, probe::byte_unit(fmt)), BDS_ERR_ARG;
        n = n_bytes / sample_bytes(fmt);
    }
    if (n < 0) return snprintf(msg, len, "%lld samples", (long long)n), BDS_ERR_ARG;
    if (o->n_tones < 1 || o->n_tones > kMaxTones) return snprintf(msg, len, "n_tones = %d is outside 1 .. %d", o->n_tones, kMaxTones), BDS_ERR_ARG;
    if (o->block_log2 < BDS_NOTCH_MIN_LOG2 || o->block_log2 > BDS_NOTCH_MAX_LOG2)
        return snprintf(msg, len, "block_log2 = %d is outside %d .. %d", o->block_log2, BDS_NOTCH_MIN_LOG2, BDS_NOTCH_MAX_LOG2), BDS_ERR_ARG;
    const int64_t B = (int64_t)1 << o->block_log2;
    if (o->first_sample < 0 || o->first_sample % B)
        return snprintf(msg, len, "first_sample = %lld is not on the grid of the %lld-sample blocks", (long long)o->first_sample, (long long)B), BDS_ERR_ARG;
    const uint32_t width = 1u << (32 - o->block_log2);  // one notch width, fs / B, as a phase step
    if (!probe::is_complex(fmt))
        for (int k = 0; k < o->n_tones; ++k) {
            const uint32_t st = o->step[k];
            if (st == 0 || st >= 0x80000000u || st < 2 * width || 0x80000000u - st < 2 * width)
                return snprintf(msg, len, "step[%d] = %u: a tone of a real record lies at least two notch widths (%u) inside (0, 2^31), where it and its image can be told apart",
                                k, st, 2 * width), BDS_ERR_ARG;
        }
    for (int k = 0; k < o->n_tones; ++k)
        for (int j = 0; j < k; ++j)
            if (circ_dist(o->step[k], o->step[j]) < 4 * width)
                return snprintf(msg, len, "step[%d] = %u and step[%d] = %u are closer than four notch widths (%u)", j, o->step[j], k, o->step[k], 4 * width), BDS_ERR_ARG;
    const int64_t need = block_count(n, o->block_log2) * o->n_tones;
    if (rep->est && rep->est_cap < need)
        return snprintf(msg, len, "report->est holds %lld estimates, the window takes %lld", (long long)rep->est_cap, (long long)need), BDS_ERR_ARG;
    *n_samples = n;
    return BDS_OK;
}

// ---- pieces ------------------------------------------------------------------------------------------------------------------------
// Blocks are self-contained: a piece is a whole number of blocks and needs no context.  Samples per piece: the caller's rounded
// down to a block, else 64 MiB of the record (a multiple of every block).
inline int64_t piece_of(int fmt, int64_t piece_samples, int block_log2) {
    const int64_t p = piece_samples > 0 ? piece_samples : ((int64_t)64 << 20) / sample_bytes(fmt);
    return p >> block_log2 << block_log2;
}

}  // namespace notch
}  // namespace bds
