// bds_synth / bds_synth_file / bds_synth_noise: synthetic IF records made on the device (include/bds_mi355x.h, "synthetic IF
// records").  The signal is bds_amd/synth.py:make_if's, sample by sample in its own float64 operation order; the random stream is
// counter-based (bds_synth_math.h), so sample n depends on (seed, n, settings, satellites) alone and a record can be made in any
// pieces.  Built with -ffp-contract=off like the tracking correlator: the index arithmetic rounds as NumPy's does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "bds_internal.h"
#include "bds_synth_math.h"

namespace bds {
namespace synth {

constexpr int kCodeLen = 10230;
constexpr int kCodeWords = 320;  // a primary code as bits: 10230 bits = 1 279 bytes, held in 320 dwords
constexpr int kUnitBytes = 16;   // what one lane stores: one 16-byte store of consecutive samples

struct Sat {            // one satellite entry, everything the host can form once (same IEEE operations as synth.py:88-90,97)
    double delay;       // samples
    double ratio;       // fcode / fs
    double fcarr;       // IF + doppler
    double phase;
    double amp;         // sigma sqrt(4 10^(cn0 / 10) / fs)
    int64_t pmin;       // first code period of this call's symbol table
    int64_t sym_off;    // offset of its D row in the symbol table; the S row follows at + sym_len
    int32_t sym_len;    // periods in the table
    int32_t code_slot;  // which bit-packed (data, pilot) code pair
};

struct Params {
    const Sat *sats;
    const uint32_t *codes;  // [slot][data, pilot][kCodeWords], bit i = chip i is +1
    const int8_t *sym;      // +-1
    double fs, ncode, sigma, threshold, k61, k29;
    uint64_t seed;
    int32_t n_sat, b1c, conj, p61s;
};

// One satellite's term of one sample from its code phase cph in [0, ncode), code period and carrier angle on: make_if's z
// (synth.py:93-112) added to the sums.  Shared by the constant-Doppler path and the trajectory path.
template <bool IQ>
__device__ __forceinline__ void add_term(const Params &p, const Sat &s, double cph, int64_t period, double th, double &acc_i, double &acc_q) {
    const int ci = min((int)cph, kCodeLen - 1);
    int64_t pi = period - s.pmin;  // the table covers every period of the call; the clamp keeps a lane in bounds whatever happens
    pi = pi < 0 ? 0 : (pi >= s.sym_len ? s.sym_len - 1 : pi);
    const double d_sym = (double)p.sym[s.sym_off + pi], p_sym = (double)p.sym[s.sym_off + s.sym_len + pi];
    const uint32_t *code = p.codes + (size_t)s.code_slot * (2 * kCodeWords) + (ci >> 5);
    const double cd = ((code[0] >> (ci & 31)) & 1u) ? 1.0 : -1.0;
    const double cp = ((code[kCodeWords] >> (ci & 31)) & 1u) ? 1.0 : -1.0;
    double br, bi;
    if (p.b1c) {
        const double boc11 = ((int64_t)floor(cph * 2.0) & 1) ? 1.0 : -1.0;  // 0 -> -c, 1 -> +c
        const double boc61 = ((int64_t)floor(cph * 12.0) & 1) ? 1.0 : -1.0;  // sub-chip ii - 1 -> (-1)^ii (the parity of a (mod 12) is the parity of a)
        br = 0.5 * d_sym * cd * boc11 - p.k61 * cp * boc61 * (p.p61s ? p_sym : 1.0);
        bi = p.k29 * cp * boc11 * p_sym;
    } else {  // d sin(th) + p cos(th) = Re[(p - j d) e^{j th}]
        br = p_sym * cp;
        bi = -(d_sym * cd);
    }
    const double ar = s.amp * br, ai = s.amp * bi;
    double sn, cs;
    sincos_strict(th, sn, cs);
    acc_i += ar * cs - ai * sn;
    if (IQ) {
        const double im = ar * sn + ai * cs;
        acc_q += p.conj ? -im : im;
    }
}

// the record before the noise: sum over the satellites, in list order, of make_if's z (synth.py:87-112)
template <bool IQ>
__device__ __forceinline__ void clean_sum(const Params &p, int64_t n, double &acc_i, double &acc_q) {
    const double nd = (double)n;
    acc_i = 0.0;
    acc_q = 0.0;
    for (int k = 0; k < p.n_sat; ++k) {
        const Sat s = p.sats[k];
        const double chips = (nd - s.delay) * s.ratio;  // code phase in chips (may be < 0)
        const double period = floor(chips / p.ncode);
        const double cph = chips - period * p.ncode;
        double x = (s.fcarr * nd) / p.fs;
        x = x - trunc(x);  // fmod(x, 1), exactly
        const double th = 6.283185307179586 * x + s.phase;
        add_term<IQ>(p, s, cph, (int64_t)period, th, acc_i, acc_q);
    }
}

// The trajectory path: what the device needs of a bds_synth_traj (segments in device memory).
struct Traj {
    const bds_synth_seg *seg;  // [n_sat][n_seg]
    int64_t first, n_seg;
    int32_t seg_log2;
};

// The clean sums of G consecutive samples from n0 on, satellite by satellite: a satellite's 72-byte segment is loaded once for the
// group and again only where the group crosses a joint -- a segment has at least 1024 samples, so at most once.  Each sample's
// sum still takes the satellites in list order.
template <bool IQ, int G>
__device__ __forceinline__ void traj_sums(const Params &p, const Traj &t, int64_t n0, double (&acc_i)[G], double (&acc_q)[G]) {
#pragma unroll
    for (int i = 0; i < G; ++i) acc_i[i] = acc_q[i] = 0.0;
    const int64_t seg_len = (int64_t)1 << t.seg_log2;
    int64_t j0, u0;
    traj_index(n0, t.first, t.seg_log2, j0, u0);
    j0 = j0 < 0 ? 0 : (j0 >= t.n_seg ? t.n_seg - 1 : j0);  // the host has checked the span; the clamp keeps a lane in bounds whatever happens
    for (int k = 0; k < p.n_sat; ++k) {
        const Sat s = p.sats[k];
        const bds_synth_seg *sp = t.seg + (int64_t)k * t.n_seg + j0;
        bds_synth_seg g = *sp;
        int64_t u = u0;
#pragma unroll
        for (int i = 0; i < G; ++i) {
            if (u == seg_len) {  // the joint: the next segment from its first sample on
                if (j0 + 1 < t.n_seg) g = sp[1];
                u = 0;
            }
            double cph;
            int64_t period;
            traj_code(g.period0, g.code, (double)u, p.ncode, cph, period);
            add_term<IQ>(p, s, cph, period, traj_carrier(g.carr, (double)u, s.phase), acc_i[i], acc_q[i]);
            ++u;
        }
    }
}

__device__ __forceinline__ int quantise8(double v) {  // np.clip(np.rint(v), -127, 127).astype(int8)
    return (int)fmin(fmax(rint(v), -127.0), 127.0);
}

// FMT 0: float64 clean sum; 1: real int8; 2: interleaved I/Q int8; 3: packed 2+2-bit I/Q.  A lane makes the consecutive samples
// of one 16-byte unit (2 / 16 / 8 / 32 of them) and stores the unit whole; unit u starts at sample first + u * samples-per-unit.
// `out` holds n_units units (the host pads the device buffer to whole units and copies out what was asked for).
template <int FMT>
__global__ __launch_bounds__(256) void k_synth_if(Params p, int64_t first, int64_t n_units, uint4 *__restrict__ out) {
    constexpr int kPerDword = FMT == 1 ? 4 : FMT == 2 ? 2 : 8;  // samples per dword (FMT 0: a sample is two dwords)
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < n_units; u += (int64_t)gridDim.x * 256) {
        uint4 unit;
        if (FMT == 0) {
            double a, b, q;
            clean_sum<false>(p, first + 2 * u, a, q);
            clean_sum<false>(p, first + 2 * u + 1, b, q);
            unit.x = (uint32_t)__double2loint(a), unit.y = (uint32_t)__double2hiint(a);
            unit.z = (uint32_t)__double2loint(b), unit.w = (uint32_t)__double2hiint(b);
        } else {
            const int64_t n0 = first + u * (4 * kPerDword);
            uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
            for (int d = 0; d < 4; ++d) {
                uint32_t w = 0;
                for (int j = 0; j < kPerDword; ++j) {
                    const int64_t n = n0 + d * kPerDword + j;
                    double si, sq, gi, gq;
                    clean_sum<FMT != 1>(p, n, si, sq);
                    noise_normals(p.seed, n, gi, gq);
                    const int vi = quantise8(si + p.sigma * gi);
                    if (FMT == 1) {
                        w |= (uint32_t)(uint8_t)vi << (8 * j);
                    } else {
                        const int vq = quantise8(sq + p.sigma * gq);
                        if (FMT == 2)
                            w |= ((uint32_t)(uint8_t)vi | ((uint32_t)(uint8_t)vq << 8)) << (16 * j);
                        else  // bit 0 = I negative, bit 1 = Q negative, bit 2 = |I| is 3, bit 3 = |Q| is 3; 0 counts as positive
                            w |= ((vi < 0 ? 1u : 0u) | (vq < 0 ? 2u : 0u) | ((double)abs(vi) > p.threshold ? 4u : 0u) |
                                  ((double)abs(vq) > p.threshold ? 8u : 0u))
                                 << (4 * j);
                    }
                }
                w0 = d == 0 ? w : w0, w1 = d == 1 ? w : w1, w2 = d == 2 ? w : w2, w3 = d == 3 ? w : w3;
            }
            unit = make_uint4(w0, w1, w2, w3);
        }
        out[u] = unit;
    }
}

// k_synth_if's record on the trajectory path: the same units, formats and quantisers.  A lane makes its unit in groups of G = 4
// samples (format 0: its 2) whose clean sums are held in registers while traj_sums walks the satellites, and shifts each group's
// bits into the unit.  (Holding a whole unit's sums, 16 samples unrolled, takes all 256 VGPRs -- one wave per SIMD -- and 200 KB of
// code; with groups of 4 a segment is loaded once per four samples, the kernel takes 99 .. 107 VGPRs -- four waves per SIMD,
// k_synth_if has six -- and the loop body stays small.)
template <int FMT>
__global__ __launch_bounds__(256) void k_synth_traj(Params p, Traj t, int64_t first, int64_t n_units, uint4 *__restrict__ out) {
    constexpr int G = FMT == 0 ? 2 : 4;                                  // samples per group
    constexpr int kBits = FMT == 1 ? 8 : FMT == 2 ? 16 : 4;              // bits per sample in the unit (FMT 0: not used)
    constexpr int kGroups = FMT == 0 ? 1 : 128 / (G * kBits);            // 4 / 2 / 8
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < n_units; u += (int64_t)gridDim.x * 256) {
        uint4 unit;
        double si[G], sq[G];
        if (FMT == 0) {
            traj_sums<false, G>(p, t, first + 2 * u, si, sq);
            unit.x = (uint32_t)__double2loint(si[0]), unit.y = (uint32_t)__double2hiint(si[0]);
            unit.z = (uint32_t)__double2loint(si[1]), unit.w = (uint32_t)__double2hiint(si[1]);
        } else {
            const int64_t n0 = first + u * (G * kGroups);
            uint64_t lo = 0, hi = 0;  // the unit's 128 bits
#pragma unroll 1
            for (int g = 0; g < kGroups; ++g) {
                traj_sums<FMT != 1, G>(p, t, n0 + g * G, si, sq);
                uint64_t bits = 0;
#pragma unroll
                for (int i = 0; i < G; ++i) {
                    double gi, gq;
                    noise_normals(p.seed, n0 + g * G + i, gi, gq);
                    const int vi = quantise8(si[i] + p.sigma * gi);
                    uint64_t v;
                    if (FMT == 1) {
                        v = (uint64_t)(uint8_t)vi;
                    } else {
                        const int vq = quantise8(sq[i] + p.sigma * gq);
                        if (FMT == 2)
                            v = (uint64_t)(uint8_t)vi | ((uint64_t)(uint8_t)vq << 8);
                        else  // the nibble of k_synth_if
                            v = (vi < 0 ? 1u : 0u) | (vq < 0 ? 2u : 0u) | ((double)abs(vi) > p.threshold ? 4u : 0u) |
                                ((double)abs(vq) > p.threshold ? 8u : 0u);
                    }
                    bits |= v << (kBits * i);
                }
                const int pos = g * (G * kBits);
                if (pos < 64)
                    lo |= bits << pos;
                else
                    hi |= bits << (pos - 64);
            }
            unit = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
        }
        out[u] = unit;
    }
}

__global__ __launch_bounds__(256) void k_synth_noise(uint64_t seed, int64_t first, int64_t n, double *__restrict__ g_i, double *__restrict__ g_q) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double a, b;
        noise_normals(seed, first + i, a, b);
        if (g_i) g_i[i] = a;
        if (g_q) g_q[i] = b;
    }
}

static int samples_per_unit(int fmt) { return fmt == 0 ? 2 : fmt == 1 ? 16 : fmt == 2 ? 8 : 32; }
// bytes of n samples (format 3: n even)
static size_t bytes_of(int fmt, int64_t n) { return fmt == 0 ? (size_t)n * 8 : fmt == 1 ? (size_t)n : fmt == 2 ? (size_t)n * 2 : (size_t)n / 2; }
static int64_t units_of(int fmt, int64_t n) { return (n + samples_per_unit(fmt) - 1) / samples_per_unit(fmt); }

// what a call needs on the device besides its output buffers
struct Plan {
    Params p{};
    int fmt = 0;
    std::vector<Sat> sats;
    std::vector<uint32_t> codes;
    std::vector<int8_t> sym;
    void *d_sats = nullptr, *d_codes = nullptr, *d_sym = nullptr;
    bool traj = false;  // the trajectory path: t and the host segments it will be uploaded from
    Traj t{};
    const bds_synth_seg *h_seg = nullptr;
    void *d_seg = nullptr;
};

// Every argument check of bds_synth / bds_synth_file / bds_synth_traj, and the host side of the plan.  No device call in here.
// traj: NULL on the constant-Doppler path; `traj_path` says which one the caller is (a NULL traj on the trajectory path is an error).
static int make_plan(bds_ctx *ctx, const char *who, const bds_settings *s, int n_sat, const bds_synth_sat *sats, const bds_synth_opts *o,
                     int64_t first, int64_t n, Plan &pl, const struct bds_synth_traj *traj = nullptr, bool traj_path = false) {
    if (!s || !o) return fail(ctx, BDS_ERR_ARG, "%s: settings / opts is NULL", who);
    if (o->size != (int32_t)sizeof(bds_synth_opts))
        return fail(ctx, BDS_ERR_ARG, "%s: opts.size = %d, sizeof(bds_synth_opts) = %d", who, o->size, (int)sizeof(bds_synth_opts));
    if (o->format < 0 || o->format > 3) return fail(ctx, BDS_ERR_ARG, "%s: opts.format = %d (0 float64 clean, 1 int8, 2 I/Q int8, 3 packed I/Q)", who, o->format);
    if (s->signal != BDS_SIGNAL_B1C && s->signal != BDS_SIGNAL_B2A) return fail(ctx, BDS_ERR_ARG, "%s: settings.signal invalid", who);
    if (s->codeLength != kCodeLen) return fail(ctx, BDS_ERR_ARG, "%s: settings.codeLength = %d, the primary codes have %d chips", who, s->codeLength, kCodeLen);
    if (!(s->samplingFreq > 0) || !std::isfinite(s->samplingFreq) || !(s->codeFreqBasis > 0) || !std::isfinite(s->codeFreqBasis) || !std::isfinite(s->IF))
        return fail(ctx, BDS_ERR_ARG, "%s: settings.samplingFreq / codeFreqBasis / IF invalid", who);
    if (!traj_path && o->code_doppler && (!(s->carrFreqBasis != 0) || !std::isfinite(s->carrFreqBasis)))
        return fail(ctx, BDS_ERR_ARG, "%s: settings.carrFreqBasis invalid (code_doppler is on)", who);
    if (n_sat < 0 || n_sat > BDS_MAX_PRN || (n_sat && !sats)) return fail(ctx, BDS_ERR_ARG, "%s: n_sat = %d (0 .. %d satellites)", who, n_sat, BDS_MAX_PRN);
    if (!(o->sigma >= 0) || !std::isfinite(o->sigma) || !std::isfinite(o->threshold)) return fail(ctx, BDS_ERR_ARG, "%s: opts.sigma / threshold invalid", who);
    if (first < 0 || n < 0 || first > (1LL << 53) - n) return fail(ctx, BDS_ERR_ARG, "%s: samples %lld .. +%lld outside 0 .. 2^53", who, (long long)first, (long long)n);
    if (o->format == 3 && ((first | n) & 1))
        return fail(ctx, BDS_ERR_ARG, "%s: a packed record holds two samples per byte: first_sample = %lld and n_samples = %lld must be even", who, (long long)first, (long long)n);
    if (o->symbols && o->n_sym < 1) return fail(ctx, BDS_ERR_ARG, "%s: opts.n_sym = %lld with symbols given", who, (long long)o->n_sym);
    for (int k = 0; k < n_sat; ++k) {
        if (sats[k].prn < 1 || sats[k].prn > BDS_MAX_PRN) return fail(ctx, BDS_ERR_ARG, "%s: satellite %d: PRN %d out of range (1 .. %d)", who, k + 1, sats[k].prn, BDS_MAX_PRN);
        if (!std::isfinite(sats[k].doppler) || !std::isfinite(sats[k].delay) || !std::isfinite(sats[k].phase) || !std::isfinite(sats[k].cn0_dbhz) ||
            std::fabs(sats[k].phase) > 1e6)
            return fail(ctx, BDS_ERR_ARG, "%s: satellite %d: doppler / delay / phase / cn0_dbhz invalid", who, k + 1);
    }
    const double fs = s->samplingFreq, fc = s->codeFreqBasis, ncode = (double)kCodeLen;
    pl.fmt = o->format;
    int64_t last_eval = 0;  // trajectory path: the last sample the device evaluates
    if (traj_path) {
        if (!traj) return fail(ctx, BDS_ERR_ARG, "%s: traj is NULL", who);
        if (traj->size != (int32_t)sizeof(struct bds_synth_traj))
            return fail(ctx, BDS_ERR_ARG, "%s: traj.size = %d, sizeof(struct bds_synth_traj) = %d", who, traj->size, (int)sizeof(struct bds_synth_traj));
        if (traj->seg_log2 < 10 || traj->seg_log2 > 26) return fail(ctx, BDS_ERR_ARG, "%s: traj.seg_log2 = %d (10 .. 26)", who, traj->seg_log2);
        if (!traj->seg) return fail(ctx, BDS_ERR_ARG, "%s: traj.seg is NULL", who);
        if (traj->n_seg < 1 || traj->n_seg > (1LL << 26) || traj->first < -(1LL << 53) || traj->first > (1LL << 53))
            return fail(ctx, BDS_ERR_ARG, "%s: traj.n_seg = %lld, traj.first = %lld out of range", who, (long long)traj->n_seg, (long long)traj->first);
        for (int k = 0; k < n_sat; ++k)
            if (sats[k].doppler != 0 || sats[k].delay != 0)
                return fail(ctx, BDS_ERR_ARG, "%s: satellite %d: doppler = %g, delay = %g: both must be 0 with a trajectory, which sets them", who, k + 1,
                            sats[k].doppler, sats[k].delay);
        // every piece of the call makes its last 16-byte unit whole, and a piece is a multiple of 32 samples
        last_eval = first + units_of(o->format, n) * samples_per_unit(o->format) - 1;
        const int64_t t_end = traj->first + (traj->n_seg << traj->seg_log2);
        if (n > 0 && (first < traj->first || last_eval >= t_end))
            return fail(ctx, BDS_ERR_ARG, "%s: samples %lld .. %lld (the call's, made up to a whole 16-byte unit) are outside the trajectory's %lld .. %lld",
                        who, (long long)first, (long long)last_eval, (long long)traj->first, (long long)(t_end - 1));
        for (int64_t i = 0; i < (int64_t)n_sat * traj->n_seg; ++i) {
            const bds_synth_seg &g = traj->seg[i];
            bool fin = true;
            for (int c = 0; c < 4; ++c) fin = fin && std::isfinite(g.code[c]) && std::isfinite(g.carr[c]);
            if (!fin || std::llabs(g.period0) > (1LL << 53))
                return fail(ctx, BDS_ERR_ARG, "%s: satellite %lld, segment %lld: a coefficient is not finite (or period0 is beyond 2^53)", who,
                            (long long)(i / traj->n_seg + 1), (long long)(i % traj->n_seg));
            const double seg_len = (double)(1LL << traj->seg_log2);  // the code polynomial stays an exact-integer-sized number of chips
            if (std::fabs(g.code[0]) + (std::fabs(g.code[1]) + (std::fabs(g.code[2]) + std::fabs(g.code[3]) * seg_len) * seg_len) * seg_len > 4503599627370496.0)
                return fail(ctx, BDS_ERR_ARG, "%s: satellite %lld, segment %lld: the code polynomial exceeds 2^52 chips inside its segment", who,
                            (long long)(i / traj->n_seg + 1), (long long)(i % traj->n_seg));
            if (!(g.code[1] > 0))
                return fail(ctx, BDS_ERR_ARG, "%s: satellite %lld, segment %lld: code[1] = %g: the code rate must be positive", who,
                            (long long)(i / traj->n_seg + 1), (long long)(i % traj->n_seg), g.code[1]);
        }
        pl.traj = true;
        pl.t.first = traj->first, pl.t.n_seg = traj->n_seg, pl.t.seg_log2 = traj->seg_log2;
        pl.h_seg = traj->seg;
    }
    Params &p = pl.p;
    p.fs = fs, p.ncode = ncode, p.sigma = o->sigma, p.threshold = o->threshold > 0 ? o->threshold : o->sigma;
    p.k61 = std::sqrt(1.0 / 11.0), p.k29 = std::sqrt(29.0 / 44.0);
    p.seed = o->seed, p.n_sat = n_sat, p.b1c = s->signal == BDS_SIGNAL_B1C, p.conj = o->iq_sign < 0, p.p61s = o->pilot61_secondary != 0;
    // the samples the device evaluates: every piece of the call makes its last 16-byte unit whole (at most 31 samples more)
    const int64_t last = first + n + 32;
    int slot_of[BDS_MAX_PRN + 1];
    std::fill(slot_of, slot_of + BDS_MAX_PRN + 1, -1);
    int n_slots = 0;
    int64_t sym_total = 0;
    pl.sats.resize((size_t)n_sat);
    for (int k = 0; k < n_sat; ++k) {
        Sat &d = pl.sats[(size_t)k];
        const bds_synth_sat &a = sats[k];
        const double fcode = o->code_doppler && !traj_path ? fc * (1.0 + a.doppler / s->carrFreqBasis) : fc;
        d.delay = a.delay, d.ratio = fcode / fs, d.fcarr = s->IF + a.doppler, d.phase = a.phase;
        d.amp = o->sigma * std::sqrt(4.0 * std::pow(10.0, a.cn0_dbhz / 10.0) / fs);
        if (!(d.ratio > 0) || !std::isfinite(d.ratio) || !std::isfinite(d.amp))
            return fail(ctx, BDS_ERR_ARG, "%s: satellite %d: code rate / amplitude not finite and positive", who, k + 1);
        // the code period is monotone in n: the first and the last sample bound it (one period of margin either side)
        double p0 = std::floor(((double)first - d.delay) * d.ratio / ncode), p1 = std::floor(((double)last - d.delay) * d.ratio / ncode);
        if (traj_path && n > 0) {  // the same bound from the trajectory's own arithmetic at the first and the last sample evaluated
            const int64_t ends[2] = {first, last_eval};
            double pe[2];
            for (int e = 0; e < 2; ++e) {
                int64_t j, u, period;
                double cph;
                traj_index(ends[e], traj->first, traj->seg_log2, j, u);
                const bds_synth_seg &g = traj->seg[(int64_t)k * traj->n_seg + j];
                traj_code(g.period0, g.code, (double)u, ncode, cph, period);
                pe[e] = (double)period;
            }
            p0 = pe[0], p1 = pe[1];
        } else if (traj_path) {
            p0 = p1 = 0;
        }
        if (!(std::fabs(p0) < 4e18) || !(std::fabs(p1) < 4e18) || p1 - p0 > (double)(1 << 28) || p1 < p0)
            return fail(ctx, BDS_ERR_ARG, "%s: satellite %d: code periods %g .. %g: too many for one call", who, k + 1, p0, p1);
        d.pmin = (int64_t)p0 - 1;
        d.sym_len = (int32_t)((int64_t)p1 + 1 - d.pmin + 1);
        d.sym_off = sym_total;
        sym_total += 2 * (int64_t)d.sym_len;
        if (sym_total > (1LL << 30)) return fail(ctx, BDS_ERR_ARG, "%s: symbol table of more than 2^30 entries: make the record in shorter calls", who);
        if (slot_of[a.prn] < 0) slot_of[a.prn] = n_slots++;
        d.code_slot = slot_of[a.prn];
    }
    pl.sym.resize((size_t)sym_total);
    for (int k = 0; k < n_sat; ++k) {
        const Sat &d = pl.sats[(size_t)k];
        for (int c = 0; c < 2; ++c)
            for (int32_t i = 0; i < d.sym_len; ++i) {
                const int64_t period = d.pmin + i;
                int v;
                if (o->symbols) {  // (period + 1) mod n_sym, non-negative, as make_if's pidx
                    int64_t m = (period + 1) % o->n_sym;
                    if (m < 0) m += o->n_sym;
                    v = o->symbols[((size_t)k * 2 + (size_t)c) * (size_t)o->n_sym + (size_t)m];
                    if (v != 1 && v != -1) return fail(ctx, BDS_ERR_ARG, "%s: opts.symbols[%d][%d][%lld] = %d is not +-1", who, k, c, (long long)m, v);
                } else {
                    v = symbol(o->seed, period, sats[k].prn, c);
                }
                pl.sym[(size_t)d.sym_off + (size_t)c * (size_t)d.sym_len + (size_t)i] = (int8_t)v;
            }
    }
    pl.codes.assign((size_t)n_slots * 2 * kCodeWords, 0u);
    for (int prn = 1; prn <= BDS_MAX_PRN; ++prn) {
        if (slot_of[prn] < 0) continue;
        int8_t chips[kCodeLen];
        for (int c = 0; c < 2; ++c) {
            if (gen_primary(s->signal, c == 1, prn, chips) != kCodeLen) return fail(ctx, BDS_ERR_ARG, "%s: no primary code for PRN %d", who, prn);
            uint32_t *w = &pl.codes[((size_t)slot_of[prn] * 2 + (size_t)c) * kCodeWords];
            for (int i = 0; i < kCodeLen; ++i)
                if (chips[i] > 0) w[i >> 5] |= 1u << (i & 31);
        }
    }
    return BDS_OK;
}

static void plan_free(Plan &pl) {
    if (pl.d_sats) (void)hipFree(pl.d_sats);
    if (pl.d_codes) (void)hipFree(pl.d_codes);
    if (pl.d_sym) (void)hipFree(pl.d_sym);
    if (pl.d_seg) (void)hipFree(pl.d_seg);
    pl.d_sats = pl.d_codes = pl.d_sym = pl.d_seg = nullptr;
}

static int plan_upload(bds_ctx *ctx, Plan &pl) {
    auto up = [&](void *&d, const void *h, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(&d, std::max<size_t>(bytes, 16));
        if (e == hipSuccess && bytes) e = hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
        return e;
    };
    BDS_HIP(ctx, up(pl.d_sats, pl.sats.data(), pl.sats.size() * sizeof(Sat)));
    BDS_HIP(ctx, up(pl.d_codes, pl.codes.data(), pl.codes.size() * sizeof(uint32_t)));
    BDS_HIP(ctx, up(pl.d_sym, pl.sym.data(), pl.sym.size()));
    pl.p.sats = (const Sat *)pl.d_sats, pl.p.codes = (const uint32_t *)pl.d_codes, pl.p.sym = (const int8_t *)pl.d_sym;
    if (pl.traj) {
        BDS_HIP(ctx, up(pl.d_seg, pl.h_seg, (size_t)pl.p.n_sat * (size_t)pl.t.n_seg * sizeof(bds_synth_seg)));
        pl.t.seg = (const bds_synth_seg *)pl.d_seg;
    }
    return BDS_OK;
}

// n samples from `first` into d_out (whole units: units_of(fmt, n) * 16 bytes), on `stream`
static int launch(bds_ctx *ctx, const Plan &pl, hipStream_t stream, int64_t first, int64_t n, void *d_out) {
    const int64_t units = units_of(pl.fmt, n);
    if (units < 1) return BDS_OK;
    const unsigned grid = (unsigned)std::min<int64_t>((units + 255) / 256, (int64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256) * 8);
    uint4 *out = (uint4 *)d_out;
    if (pl.traj) {
        switch (pl.fmt) {
            case 0: hipLaunchKernelGGL(k_synth_traj<0>, dim3(grid), dim3(256), 0, stream, pl.p, pl.t, first, units, out); break;
            case 1: hipLaunchKernelGGL(k_synth_traj<1>, dim3(grid), dim3(256), 0, stream, pl.p, pl.t, first, units, out); break;
            case 2: hipLaunchKernelGGL(k_synth_traj<2>, dim3(grid), dim3(256), 0, stream, pl.p, pl.t, first, units, out); break;
            default: hipLaunchKernelGGL(k_synth_traj<3>, dim3(grid), dim3(256), 0, stream, pl.p, pl.t, first, units, out); break;
        }
        BDS_HIP(ctx, hipGetLastError());
        return BDS_OK;
    }
    switch (pl.fmt) {
        case 0: hipLaunchKernelGGL(k_synth_if<0>, dim3(grid), dim3(256), 0, stream, pl.p, first, units, out); break;
        case 1: hipLaunchKernelGGL(k_synth_if<1>, dim3(grid), dim3(256), 0, stream, pl.p, first, units, out); break;
        case 2: hipLaunchKernelGGL(k_synth_if<2>, dim3(grid), dim3(256), 0, stream, pl.p, first, units, out); break;
        default: hipLaunchKernelGGL(k_synth_if<3>, dim3(grid), dim3(256), 0, stream, pl.p, first, units, out); break;
    }
    BDS_HIP(ctx, hipGetLastError());
    return BDS_OK;
}

// samples per piece: a multiple of 32 (a whole unit in every format), at least 32
static int64_t piece_of(int fmt, int64_t piece_samples) {
    if (piece_samples <= 0) piece_samples = (int64_t)((64u << 20) / (fmt == 0 ? 8 : fmt == 2 ? 2 : 1));  // 64 MiB per piece (packed: 32 MiB)
    return piece_samples;
}

static void timing_of(bds_ctx *ctx, double total, double gen, double copy) {
    ctx->timing = bds_timing{};
    ctx->timing.total_ms = total, ctx->timing.forward_ms = gen, ctx->timing.search_ms = copy;
}

}  // namespace synth
}  // namespace bds

using namespace bds;
using namespace bds::synth;

// bds_synth and bds_synth_traj: the record into host memory
static int synth_host(bds_ctx *ctx, const char *who, const bds_settings *s, int n_sat, const bds_synth_sat *sats, const bds_synth_opts *opts,
                      const struct bds_synth_traj *traj, bool traj_path, int64_t first_sample, int64_t n_samples, void *out, size_t out_bytes) {
    Plan pl;
    if (int rc = make_plan(ctx, who, s, n_sat, sats, opts, first_sample, n_samples, pl, traj, traj_path)) return rc;
    const size_t need = bytes_of(pl.fmt, n_samples);
    if (out_bytes < need || (need && !out))
        return fail(ctx, BDS_ERR_ARG, "%s: out holds %zu bytes, %lld samples of format %d take %zu", who, out ? out_bytes : (size_t)0, (long long)n_samples, pl.fmt, need);
    if (!ctx) return fail(ctx, BDS_ERR_ARG, "%s: ctx is NULL", who);
    if (n_samples == 0) return BDS_OK;
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)ctx->stream;
    const int64_t piece = std::min<int64_t>(n_samples, (piece_of(pl.fmt, 0) * 4 + 31) / 32 * 32);  // up to 256 MiB of the record on the device at a time
    void *d_out = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    double t_gen = 0, t_copy = 0;
    int rc = plan_upload(ctx, pl);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMalloc(&d_out, (size_t)units_of(pl.fmt, piece) * kUnitBytes);
    for (int i = 0; i < 3 && !rc && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
    for (int64_t a = 0; a < n_samples && !rc && e == hipSuccess; a += piece) {
        const int64_t m = std::min(piece, n_samples - a);
        e = hipEventRecord(ev[0], st);
        if (e == hipSuccess) rc = launch(ctx, pl, st, first_sample + a, m, d_out);
        if (!rc && e == hipSuccess) e = hipEventRecord(ev[1], st);
        if (!rc && e == hipSuccess) e = hipMemcpyAsync((char *)out + bytes_of(pl.fmt, a), d_out, bytes_of(pl.fmt, m), hipMemcpyDeviceToHost, st);
        if (!rc && e == hipSuccess) e = hipEventRecord(ev[2], st);
        if (!rc && e == hipSuccess) e = hipStreamSynchronize(st);
        float g = 0, c = 0;
        if (!rc && e == hipSuccess) e = hipEventElapsedTime(&g, ev[0], ev[1]);
        if (!rc && e == hipSuccess) e = hipEventElapsedTime(&c, ev[1], ev[2]);
        t_gen += g, t_copy += c;
    }
    for (auto v : ev)
        if (v) (void)hipEventDestroy(v);
    if (d_out) (void)hipFree(d_out);
    plan_free(pl);
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? BDS_ERR_NOMEM : BDS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    timing_of(ctx, t_gen + t_copy, t_gen, t_copy);
    return BDS_OK;
}

extern "C" int bds_synth(bds_ctx *ctx, const bds_settings *s, int n_sat, const bds_synth_sat *sats, const bds_synth_opts *opts,
                         int64_t first_sample, int64_t n_samples, void *out, size_t out_bytes) {
    return synth_host(ctx, "bds_synth", s, n_sat, sats, opts, nullptr, false, first_sample, n_samples, out, out_bytes);
}

extern "C" int bds_synth_traj(bds_ctx *ctx, const bds_settings *s, int n_sat, const bds_synth_sat *sats, const bds_synth_opts *opts,
                              const struct bds_synth_traj *traj, int64_t first_sample, int64_t n_samples, void *out, size_t out_bytes) {
    return synth_host(ctx, "bds_synth_traj", s, n_sat, sats, opts, traj, true, first_sample, n_samples, out, out_bytes);
}

// The record into the caller's device memory.  The kernels store whole 16-byte units at 16-byte-aligned addresses, so they write in
// place only the whole units of a 16-byte-aligned d_out; everything else (the last, partial unit; all of a misaligned d_out) is
// generated into a buffer of the library's and copied device to device, byte-exact, so not one byte outside the record is written.
static int synth_device(bds_ctx *ctx, const char *who, const bds_settings *s, int n_sat, const bds_synth_sat *sats, const bds_synth_opts *opts,
                        const struct bds_synth_traj *traj, bool traj_path, int64_t first_sample, int64_t n_samples, void *d_out, size_t out_bytes) {
    Plan pl;
    if (int rc = make_plan(ctx, who, s, n_sat, sats, opts, first_sample, n_samples, pl, traj, traj_path)) return rc;
    const size_t need = bytes_of(pl.fmt, n_samples);
    if (out_bytes < need || (need && !d_out))
        return fail(ctx, BDS_ERR_ARG, "%s: d_out holds %zu bytes, %lld samples of format %d take %zu", who, d_out ? out_bytes : (size_t)0, (long long)n_samples, pl.fmt, need);
    if (!ctx) return fail(ctx, BDS_ERR_ARG, "%s: ctx is NULL", who);
    if (int rc = check_device_span(ctx, who, "d_out", d_out, out_bytes)) return rc;
    if (n_samples == 0) return BDS_OK;
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)ctx->stream;
    const int64_t spu = samples_per_unit(pl.fmt);
    const int64_t n_direct = ((uintptr_t)d_out % kUnitBytes) == 0 ? (int64_t)(need / kUnitBytes) * spu : 0;  // samples of the units written in place
    const int64_t n_staged = n_samples - n_direct;
    const int64_t piece = std::min<int64_t>(n_staged, (piece_of(pl.fmt, 0) + 31) / 32 * 32);  // up to 64 MiB of the record staged at a time
    void *d_stage = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    double t_gen = 0, t_copy = 0;
    int rc = plan_upload(ctx, pl);
    hipError_t e = hipSuccess;
    if (!rc && n_staged) e = hipMalloc(&d_stage, (size_t)units_of(pl.fmt, piece) * kUnitBytes);
    for (int i = 0; i < 3 && !rc && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
    if (!rc && e == hipSuccess && n_direct) {
        e = hipEventRecord(ev[0], st);
        if (e == hipSuccess) rc = launch(ctx, pl, st, first_sample, n_direct, d_out);
        if (!rc && e == hipSuccess) e = hipEventRecord(ev[1], st);
        if (!rc && e == hipSuccess) e = hipStreamSynchronize(st);
        float g = 0;
        if (!rc && e == hipSuccess) e = hipEventElapsedTime(&g, ev[0], ev[1]);
        t_gen += g;
    }
    for (int64_t a = n_direct; a < n_samples && !rc && e == hipSuccess; a += piece) {
        const int64_t m = std::min(piece, n_samples - a);
        e = hipEventRecord(ev[0], st);
        if (e == hipSuccess) rc = launch(ctx, pl, st, first_sample + a, m, d_stage);
        if (!rc && e == hipSuccess) e = hipEventRecord(ev[1], st);
        if (!rc && e == hipSuccess) e = hipMemcpyAsync((char *)d_out + bytes_of(pl.fmt, a), d_stage, bytes_of(pl.fmt, m), hipMemcpyDeviceToDevice, st);
        if (!rc && e == hipSuccess) e = hipEventRecord(ev[2], st);
        if (!rc && e == hipSuccess) e = hipStreamSynchronize(st);
        float g = 0, c = 0;
        if (!rc && e == hipSuccess) e = hipEventElapsedTime(&g, ev[0], ev[1]);
        if (!rc && e == hipSuccess) e = hipEventElapsedTime(&c, ev[1], ev[2]);
        t_gen += g, t_copy += c;
    }
    (void)hipStreamSynchronize(st);  // nothing of this call may still run when its buffers go
    for (auto v : ev)
        if (v) (void)hipEventDestroy(v);
    if (d_stage) (void)hipFree(d_stage);
    plan_free(pl);
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? BDS_ERR_NOMEM : BDS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    timing_of(ctx, t_gen + t_copy, t_gen, t_copy);
    return BDS_OK;
}

extern "C" int bds_synth_dev(bds_ctx *ctx, const bds_settings *s, int n_sat, const bds_synth_sat *sats, const bds_synth_opts *opts,
                             int64_t first_sample, int64_t n_samples, void *d_out, size_t out_bytes) {
    return synth_device(ctx, "bds_synth_dev", s, n_sat, sats, opts, nullptr, false, first_sample, n_samples, d_out, out_bytes);
}

extern "C" int bds_synth_traj_dev(bds_ctx *ctx, const bds_settings *s, int n_sat, const bds_synth_sat *sats, const bds_synth_opts *opts,
                                  const struct bds_synth_traj *traj, int64_t first_sample, int64_t n_samples, void *d_out, size_t out_bytes) {
    return synth_device(ctx, "bds_synth_traj_dev", s, n_sat, sats, opts, traj, true, first_sample, n_samples, d_out, out_bytes);
}

extern "C" int bds_synth_file(bds_ctx *ctx, const bds_settings *s, int n_sat, const bds_synth_sat *sats, const bds_synth_opts *opts,
                              int64_t first_sample, int64_t n_samples, const char *path, int64_t piece_samples) {
    Plan pl;
    if (int rc = make_plan(ctx, "bds_synth_file", s, n_sat, sats, opts, first_sample, n_samples, pl)) return rc;
    if (!path) return fail(ctx, BDS_ERR_ARG, "bds_synth_file: path is NULL");
    if (piece_samples < 0) return fail(ctx, BDS_ERR_ARG, "bds_synth_file: piece_samples = %lld", (long long)piece_samples);
    if (!ctx) return fail(ctx, BDS_ERR_ARG, "bds_synth_file: ctx is NULL");
    int64_t piece = piece_of(pl.fmt, piece_samples);
    if (pl.fmt == 3) piece += piece & 1;  // a byte holds two samples
    piece = std::min(piece, std::max<int64_t>(n_samples, 2));
    FILE *fo = fopen(path, "wb");
    if (!fo) return fail(ctx, BDS_ERR_IO, "Unable to write file %s", path);
    const int64_t n_pieces = (n_samples + piece - 1) / piece;
    const size_t buf_bytes = (size_t)units_of(pl.fmt, piece) * kUnitBytes;
    hipStream_t s_copy = (hipStream_t)ctx->stream, s_gen = (hipStream_t)ctx->stream2;
    void *d_buf[2] = {nullptr, nullptr}, *h_buf[2] = {nullptr, nullptr};
    hipEvent_t g0[3] = {}, g1[3] = {}, c0[2] = {}, c1[2] = {}, t0 = nullptr, t1 = nullptr;  // (g: per piece mod 3 -- piece k + 2 is launched before piece k's times are read)
    double t_gen = 0, t_copy = 0;
    float total = 0;
    int rc = BDS_OK;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess && n_pieces) {
        rc = plan_upload(ctx, pl);
        for (int i = 0; i < 2 && !rc && e == hipSuccess; ++i) {
            e = hipMalloc(&d_buf[i], buf_bytes);
            if (e == hipSuccess) e = hipHostMalloc(&h_buf[i], buf_bytes, hipHostMallocDefault);
            for (hipEvent_t *v : {&c0[i], &c1[i]})
                if (e == hipSuccess) e = hipEventCreate(v);
        }
        for (int i = 0; i < 3; ++i)
            for (hipEvent_t *v : {&g0[i], &g1[i]})
                if (e == hipSuccess) e = hipEventCreate(v);
        if (e == hipSuccess) e = hipEventCreate(&t0);
        if (e == hipSuccess) e = hipEventCreate(&t1);
    }
    auto span = [&](int64_t k) { return std::min(piece, n_samples - k * piece); };
    // piece k is generated on the second stream into device buffer k & 1 (after the copy that last read it), copied out on the first
    // stream into pinned buffer k & 1, and written by this thread while piece k + 1 is copied and piece k + 2 generated
    auto generate = [&](int64_t k) {
        const int b = (int)(k & 1);
        if (k >= 2) e = hipStreamWaitEvent(s_gen, c1[b], 0);
        if (e == hipSuccess) e = hipEventRecord(g0[k % 3], s_gen);
        if (e == hipSuccess) rc = launch(ctx, pl, s_gen, first_sample + k * piece, span(k), d_buf[b]);
        if (!rc && e == hipSuccess) e = hipEventRecord(g1[k % 3], s_gen);
    };
    auto finish = [&](int64_t k) {  // wait for the copy of piece k, write it
        const int b = (int)(k & 1);
        e = hipEventSynchronize(c1[b]);
        float g = 0, c = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&g, g0[k % 3], g1[k % 3]);
        if (e == hipSuccess) e = hipEventElapsedTime(&c, c0[b], c1[b]);
        t_gen += g, t_copy += c;
        const size_t nb = bytes_of(pl.fmt, span(k));
        if (e == hipSuccess && fwrite(h_buf[b], 1, nb, fo) != nb) rc = fail(ctx, BDS_ERR_IO, "short write on %s", path);
    };
    if (!rc && e == hipSuccess && n_pieces) {
        e = hipEventRecord(t0, s_gen);
        if (e == hipSuccess) generate(0);
        for (int64_t k = 0; k < n_pieces && !rc && e == hipSuccess; ++k) {
            const int b = (int)(k & 1);
            if (k + 1 < n_pieces) generate(k + 1);
            if (!rc && e == hipSuccess) e = hipStreamWaitEvent(s_copy, g1[k % 3], 0);
            if (!rc && e == hipSuccess) e = hipEventRecord(c0[b], s_copy);
            if (!rc && e == hipSuccess) e = hipMemcpyAsync(h_buf[b], d_buf[b], bytes_of(pl.fmt, span(k)), hipMemcpyDeviceToHost, s_copy);
            if (!rc && e == hipSuccess) e = hipEventRecord(c1[b], s_copy);
            if (!rc && e == hipSuccess && k >= 1) finish(k - 1);
        }
        if (!rc && e == hipSuccess) finish(n_pieces - 1);
        if (!rc && e == hipSuccess) e = hipEventRecord(t1, s_copy);
        if (!rc && e == hipSuccess) e = hipEventSynchronize(t1);
        if (!rc && e == hipSuccess) e = hipEventElapsedTime(&total, t0, t1);
    }
    // nothing of this call may still run when its buffers go
    (void)hipStreamSynchronize(s_gen);
    (void)hipStreamSynchronize(s_copy);
    for (int i = 0; i < 2; ++i) {
        if (d_buf[i]) (void)hipFree(d_buf[i]);
        if (h_buf[i]) (void)hipHostFree(h_buf[i]);
        for (hipEvent_t v : {c0[i], c1[i]})
            if (v) (void)hipEventDestroy(v);
    }
    for (int i = 0; i < 3; ++i)
        for (hipEvent_t v : {g0[i], g1[i]})
            if (v) (void)hipEventDestroy(v);
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
    plan_free(pl);
    if (fclose(fo) != 0 && !rc && e == hipSuccess) rc = fail(ctx, BDS_ERR_IO, "short write on %s", path);
    if (rc) return rc;
    if (e != hipSuccess) return fail(ctx, e == hipErrorOutOfMemory ? BDS_ERR_NOMEM : BDS_ERR_HIP, "bds_synth_file: %s", hipGetErrorString(e));
    timing_of(ctx, total, t_gen, t_copy);
    return BDS_OK;
}

extern "C" int bds_synth_noise(bds_ctx *ctx, uint64_t seed, int64_t first, int64_t n, double *g_i, double *g_q) {
    if (first < 0 || n < 0 || first > (1LL << 53) - n) return fail(ctx, BDS_ERR_ARG, "bds_synth_noise: samples %lld .. +%lld outside 0 .. 2^53", (long long)first, (long long)n);
    if (n > (1LL << 28)) return fail(ctx, BDS_ERR_ARG, "bds_synth_noise: n = %lld: at most 2^28 draws per call", (long long)n);
    if (!ctx) return fail(ctx, BDS_ERR_ARG, "bds_synth_noise: ctx is NULL");
    if (n == 0 || (!g_i && !g_q)) return BDS_OK;
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)ctx->stream;
    double *d = nullptr;
    hipError_t e = hipMalloc((void **)&d, (size_t)n * 2 * sizeof(double));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_synth_noise, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 2048)), dim3(256), 0, st, seed, first, n, d, d + n);
        e = hipGetLastError();
    }
    if (e == hipSuccess && g_i) e = hipMemcpyAsync(g_i, d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && g_q) e = hipMemcpyAsync(g_q, d + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (d) (void)hipFree(d);
    if (e != hipSuccess) return fail(ctx, BDS_ERR_HIP, "bds_synth_noise: %s", hipGetErrorString(e));
    return BDS_OK;
}
