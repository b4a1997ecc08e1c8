// Correlation function along a tracked channel: any set of tap offsets, many epochs, open loop.
//
// An item is one epoch of one channel, given as bds_track_correlate takes it (prn + state6); a call takes n_items items and one
// list of n_taps tap offsets tau (primary-code chips, the unit of dllCorrelatorSpacing) and returns, per item, component and tap,
// the raw sums (I, Q) of the carrier-wiped samples against the replica delayed by tau.  The replica index of tap tau is the
// reference's own (B2a/tracking.m:260-316, B1C/WB_tracking.m:289-324) with tau in the place of -+earlyLateSpc,
//     t = (rem + tau)[*2] : step[*2] : (((blk-1)*step + rem) + tau)[*2],   u = ceil(t),   u6 = ceil(6 t),
// read from the PERIODIC extension of the code (unit u reads c[((u - 1) mod U) + 1]), so a tap may lie many chips out.
//
// The run identity of the tracking correlator (bds_track.hip, correlate_runs),
//     sum_k x[k] c[idx(k)]  =  c[idx(last)] S(end)  -  sum over index steps u (c[u] - c[u-1]) S(k_u),
// pays the expensive part -- the f64 carrier per sample and the prefix sums S -- once per sample, however many taps are wanted:
//   k_corrfn         grid (chunks, items), one workgroup per chunk of kCfChunk samples of an item
//     phase 1  lane t wipes the carrier off kCfSeg consecutive samples (the trackers' default numerics: sin / cos of the
//              reference's own trigarg per sample) and the workgroup writes the f64 prefix sums S of the chunk to LDS
//     phase 2  wave w takes taps w, w + 4, ...: the index steps of the tap are spread over its lanes, each finds its k_u with
//              the exact search the trackers use, reads S(k_u) and adds its term in f64; the lanes are added up with the
//              fixed-order wave scan and lane 63 writes the chunk's partial sum of (item, component, tap)
//   k_corrfn_reduce  adds an item's chunks in ascending order
// The chunk is a constant and an item's chunks depend on the item alone, so a result depends on nothing but the item, the tap
// list and the settings -- not on the other items of the call, the batching, or where the record came from.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <vector>

#include "bds_internal.h"
#include "bds_record.h"
#include "bds_strict_math.h"
#include "bds_trk_replica.h"

namespace bds {

static constexpr int kCfThreads = 256, kCfWaves = kCfThreads / 64;
static constexpr int kCfSeg = 8;                       // samples per lane
static constexpr int kCfChunk = kCfThreads * kCfSeg;   // samples per workgroup: 2048, whatever the call holds
static constexpr int kCfMaxTaps = 128;
static constexpr double kCfMaxTau = 16.0;
// entries of the code tables a chunk can touch that are staged in LDS (what lies beyond -- low sampling rates -- is read from
// global memory with the same explicit wrap): (data, pilot) pairs at the look-up's resolution, BOC(6,1) twelfths
static constexpr int kCfCap1 = 2048, kCfCap6 = 12288;
static constexpr int kCfPre = kCfChunk + kCfChunk / kCfSeg + 1;  // prefix sums: position i at i + i / kCfSeg (bank spread)
static constexpr size_t kCfLds = (size_t)kCfPre * 16 + kCfWaves * 16 + kCfMaxTaps * 8 + (size_t)kCfCap1 * 2 + kCfCap6;
static constexpr size_t kCfResident = (size_t)256 << 20;  // resident limit when the context has none
static constexpr size_t kCfPartBytes = (size_t)64 << 20;  // partial sums of one launch (items per launch follow from it)
static constexpr size_t kCfStage = (size_t)64 << 20;      // pinned staging of a record read from a file, at the most

struct CfParams {
    int pilot, n_comp, n_taps, code_len, max_chunks;
    double fs, inv_fs;
    double tau_min, tau_max;
    long long base, win_end;  // samples of the record held in `data`: [base, win_end)
};

__device__ __forceinline__ int cf_wrap(int v, int n) {  // non-negative v mod n
    v %= n;
    return v < 0 ? v + n : v;
}
__device__ __forceinline__ int cf_pre(int i) { return i + i / kCfSeg; }

// sample n of the record as the trackers decode it
template <int FMT>
__device__ __forceinline__ void cf_sample(const int8_t *__restrict__ dwin, long long n, double &re, double &im) {
    im = 0.0;
    if constexpr (FMT == kFmtPacked) {  // nibble n & 1 of byte n >> 1
        const uint32_t v = iq_of_packed(((uint32_t)(uint8_t)dwin[n >> 1] >> (4 * (int)(n & 1))) & 15u);
        re = (double)(int)(int8_t)(v & 0xffu);
        im = (double)(int)(int8_t)((v >> 8) & 0xffu);
    } else if constexpr (FMT == kFmtReal16) {
        re = (double)(int)reinterpret_cast<const short *>(dwin)[n];
    } else if constexpr (FMT == kFmtIQ16) {
        const short2 v = reinterpret_cast<const short2 *>(dwin)[n];
        re = (double)(int)v.x, im = (double)(int)v.y;
    } else if constexpr (FMT == kFmtIQ) {
        const char2 v = reinterpret_cast<const char2 *>(dwin)[n];
        re = (double)(int)v.x, im = (double)(int)v.y;
    } else {
        re = (double)(int)dwin[n];
    }
}

// part: [item][max_chunks][n_comp][n_taps][2]
template <int MODE, int FMT>
__global__ __launch_bounds__(kCfThreads) void k_corrfn(const int8_t *__restrict__ data, const int8_t *__restrict__ prim, CfParams p,
                                                       const int *__restrict__ prn, const double *__restrict__ state6,
                                                       const double *__restrict__ taps, double *__restrict__ part) {
    constexpr double sc = MODE == BDS_TRACK_B2A ? 1.0 : 2.0;
    constexpr int UNITS = MODE == BDS_TRACK_B2A ? 1 : 2;
    constexpr bool CPLX = fmt_complex(FMT);
    extern __shared__ __attribute__((aligned(16))) unsigned char cf_lds[];
    double2 *s_pre = reinterpret_cast<double2 *>(cf_lds);                        // [kCfPre]
    double2 *s_wtot = s_pre + kCfPre;                                            // [kCfWaves]
    double *s_tau = reinterpret_cast<double *>(s_wtot + kCfWaves);               // [kCfMaxTaps]
    char2 *s_t1 = reinterpret_cast<char2 *>(s_tau + kCfMaxTaps);                 // [kCfCap1]
    int8_t *s_t6 = reinterpret_cast<int8_t *>(s_t1 + kCfCap1);                   // [kCfCap6]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int item = blockIdx.y;
    const double *s6 = state6 + (long)item * 6;
    const long long pos = (long long)s6[0];
    const long blk = (long)s6[1];
    const double rem = s6[2], step = s6[3] / p.fs, remCarr = s6[4], carrFreq = s6[5];
    const long k0l = (long)blockIdx.x * kCfChunk;
    if (k0l >= blk) return;  // (the reduction reads the item's own chunks only)
    const int V = p.n_comp * p.n_taps * 2;
    double *out = part + ((long)item * p.max_chunks + blockIdx.x) * V;
    if (pos < p.base || pos + blk > p.win_end) {  // the host never launches such an item; nothing is read for it
        for (int i = t; i < V; i += kCfThreads) out[i] = 0.0;
        return;
    }
    const int k0 = (int)k0l, k1 = (int)min(blk, k0l + kCfChunk);  // blksize < 2^31
    const int NU = UNITS * p.code_len, N6 = 12 * p.code_len;
    const bool wb6 = MODE == BDS_TRACK_WB && p.pilot;
    const char2 *__restrict__ g1 = reinterpret_cast<const char2 *>(prim + ((long)(prn[item] - 1) * 2 + 0) * kTabStride) + kTabPad;
    const int8_t *__restrict__ g6 = prim + ((long)(prn[item] - 1) * 2 + 1) * kTabStride + kTabPad;
    const double inc = step * sc, inv_inc = 1.0 / inc;
    const double last = (double)(blk - 1) * step + rem;  // (blksize-1)*codePhaseStep + remCodePhase, then + tau, then *2
    auto tap_colon = [&](double tau) { return colon_vec((rem + tau) * sc, step * sc, (last + tau) * sc); };

    // ---- the tap list and the slices of the code tables this chunk can touch, to LDS
    if (t < p.n_taps) s_tau[t] = taps[t];
    int lo1, n1, lo6 = 0, n6 = 0;
    {
        const ColonVec ca = tap_colon(p.tau_min), cb = tap_colon(p.tau_max);
        lo1 = (int)ceil(code_arg<0>(ca, k0)) - 2;  // (one unit below the first index for c[u-1], one for the ulps between taps)
        n1 = max(0, min(kCfCap1, (int)ceil(code_arg<0>(cb, k1 - 1)) + 2 - lo1));
        for (int i = t; i < n1; i += kCfThreads) s_t1[i] = g1[cf_wrap(lo1 + i - 1, NU)];
        if (wb6) {
            lo6 = (int)ceil(code_arg<1>(ca, k0)) - 2;
            n6 = max(0, min(kCfCap6, (int)ceil(code_arg<1>(cb, k1 - 1)) + 2 - lo6));
            for (int i = t; i < n6; i += kCfThreads) s_t6[i] = g6[cf_wrap(lo6 + i - 1, N6)];
        }
    }
    auto at1 = [&](int u) -> char2 {  // unit u of the periodic (data, pilot) code
        const unsigned d = (unsigned)(u - lo1);
        return d < (unsigned)n1 ? s_t1[d] : g1[cf_wrap(u - 1, NU)];
    };
    auto at6 = [&](int u) -> int {  // unit u of the periodic pilot BOC(6,1)
        const unsigned d = (unsigned)(u - lo6);
        return d < (unsigned)n6 ? (int)s_t6[d] : (int)g6[cf_wrap(u - 1, N6)];
    };

    // ---- phase 1: carrier wipe-off of this lane's samples, f64 prefix sums of the chunk
    {
        const int8_t *__restrict__ dwin = FMT == kFmtPacked ? data - (p.base >> 1) : data - p.base * fmt_bps(FMT);  // (packed: base even)
        const double w_ref = (carrFreq * 2.0) * 3.14159265358979323846;  // trigarg = (carrFreq*2*pi) .* (k ./ fs) + remCarrPhase
        const int kb = k0 + t * kCfSeg;
        const int n_here = max(0, min(kCfSeg, k1 - kb));
        double loc_i[kCfSeg], loc_q[kCfSeg];
        double run_i = 0.0, run_q = 0.0;
#pragma unroll
        for (int j = 0; j < kCfSeg; ++j) {
            loc_i[j] = run_i, loc_q[j] = run_q;
            if (j < n_here) {
                double rw, rw_q;
                cf_sample<FMT>(dwin, pos + kb + j, rw, rw_q);
                const double tt = div_by_fs((double)(kb + j), p.fs, p.inv_fs);
                const double trig = (w_ref * tt) + remCarr;
                double s2, c2;
                sincos_strict(trig, s2, c2);
                double ib, qb;
                if (MODE == BDS_TRACK_B2A) {  // exp(+j th): q = real, i = imag (tracking.m:309-314)
                    qb = CPLX ? fma(rw, c2, -(rw_q * s2)) : rw * c2;
                    ib = CPLX ? fma(rw, s2, rw_q * c2) : rw * s2;
                } else {  // exp(-j th): i = real, q = imag (NB_tracking.m:320-325)
                    ib = CPLX ? fma(rw, c2, rw_q * s2) : rw * c2;
                    qb = CPLX ? fma(rw_q, c2, -(rw * s2)) : -(rw * s2);
                }
                run_i += ib, run_q += qb;
            }
        }
        const double vi = wave_scan_incl(run_i), vq = wave_scan_incl(run_q);
        if (lane == 63) s_wtot[wave] = make_double2(vi, vq);
        __syncthreads();  // (also: s_tau, s_t1, s_t6 written)
        double bi = 0.0, bq = 0.0;
        for (int w = 0; w < wave; ++w) bi += s_wtot[w].x, bq += s_wtot[w].y;
        bi += vi - run_i, bq += vq - run_q;
#pragma unroll
        for (int j = 0; j < kCfSeg; ++j) s_pre[cf_pre(t * kCfSeg + j)] = make_double2(bi + loc_i[j], bq + loc_q[j]);
        if (t == kCfThreads - 1) s_pre[cf_pre(kCfChunk)] = make_double2(bi + run_i, bq + run_q);
        __syncthreads();
    }
    const double2 tot = s_pre[cf_pre(k1 - k0)];  // sum of the chunk's wiped samples

    // ---- phase 2: one wave per tap, one lane per index step
    for (int tap = wave; tap < p.n_taps; tap += kCfWaves) {
        const ColonVec cv = tap_colon(s_tau[tap]);
        {
            const int ua = (int)ceil(code_arg<0>(cv, k0)), ub = (int)ceil(code_arg<0>(cv, k1 - 1));
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            for (int r = lane; r < ub - ua; r += 64) {
                const int u = ua + 1 + r;
                const double thr = (double)(u - 1);
                int kk = (int)floor((thr - cv.a) * inv_inc) + 1;  // a prediction, confirmed with the exact expression
                kk = max(k0 + 1, min(kk, k1 - 1));
                if (!(!(code_arg<0>(cv, kk - 1) > thr) && code_arg<0>(cv, kk) > thr)) kk = first_sample_of<0>(cv, inv_inc, u, k0, k1 - 1);
                const double2 S = s_pre[cf_pre(kk - k0)];
                const char2 cn = at1(u), co = at1(u - 1);
                const double dd = (double)((int)cn.x - (int)co.x), dp = (double)((int)cn.y - (int)co.y);
                a0 = fma(-dd, S.x, a0), a1 = fma(-dd, S.y, a1);
                a2 = fma(-dp, S.x, a2), a3 = fma(-dp, S.y, a3);
            }
            if (lane == 0) {
                const char2 cl = at1(ub);
                a0 += (double)cl.x * tot.x, a1 += (double)cl.x * tot.y;
                a2 += (double)cl.y * tot.x, a3 += (double)cl.y * tot.y;
            }
            a0 = wave_scan_incl(a0), a1 = wave_scan_incl(a1);
            if (lane == 63) out[(0 * p.n_taps + tap) * 2] = a0, out[(0 * p.n_taps + tap) * 2 + 1] = a1;
            if (p.pilot) {  // (wave-uniform)
                a2 = wave_scan_incl(a2), a3 = wave_scan_incl(a3);
                if (lane == 63) out[(1 * p.n_taps + tap) * 2] = a2, out[(1 * p.n_taps + tap) * 2 + 1] = a3;
            }
        }
        if (wb6) {  // pilotBOC61(ceil(tcode*6)+1)  (WB_tracking.m:298,311,324); below 12.276 MS/s several steps share a sample
            const int ua = (int)ceil(code_arg<1>(cv, k0)), ub = (int)ceil(code_arg<1>(cv, k1 - 1));
            double a0 = 0.0, a1 = 0.0;
            for (int r = lane; r < ub - ua; r += 64) {
                const int u = ua + 1 + r;
                const double thr = (double)(u - 1);
                int kk = (int)floor((thr * (1.0 / 6.0) - cv.a) * inv_inc) + 1;
                kk = max(k0 + 1, min(kk, k1 - 1));
                if (!(!(code_arg<1>(cv, kk - 1) > thr) && code_arg<1>(cv, kk) > thr)) kk = first_sample_of<1>(cv, inv_inc, u, k0, k1 - 1);
                const double2 S = s_pre[cf_pre(kk - k0)];
                const double d6 = (double)(at6(u) - at6(u - 1));
                a0 = fma(-d6, S.x, a0), a1 = fma(-d6, S.y, a1);
            }
            if (lane == 0) {
                const double cl = (double)at6(ub);
                a0 += cl * tot.x, a1 += cl * tot.y;
            }
            a0 = wave_scan_incl(a0), a1 = wave_scan_incl(a1);
            if (lane == 63) out[(2 * p.n_taps + tap) * 2] = a0, out[(2 * p.n_taps + tap) * 2 + 1] = a1;
        }
    }
}

// out[item][v] = the item's chunks added in ascending order; grid (ceil(V / 256), items)
__global__ __launch_bounds__(256) void k_corrfn_reduce(const double *__restrict__ part, const double *__restrict__ state6, int max_chunks,
                                                       int V, double *__restrict__ out) {
    const int item = blockIdx.y, v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const long blk = (long)state6[(long)item * 6 + 1];
    const int n = (int)((blk + kCfChunk - 1) / kCfChunk);
    double acc = 0.0;
    for (int c = 0; c < n; ++c) acc += part[((long)item * max_chunks + c) * V + v];
    out[(long)item * V + v] = acc;
}

template <int MODE>
static void cf_launch_fmt(bds_ctx *ctx, int fmt, dim3 grid, hipStream_t stream, const int8_t *data, const int8_t *prim, const CfParams &p,
                          const int *prn, const double *s6, const double *taps, double *part) {
    auto fire = [&](auto kern) {
        if (ctx->lds_attr_done.insert((const void *)kern).second)
            (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCfLds);
        hipLaunchKernelGGL(kern, grid, dim3(kCfThreads), kCfLds, stream, data, prim, p, prn, s6, taps, part);
    };
    switch (fmt) {
    case kFmtReal: fire(k_corrfn<MODE, kFmtReal>); break;
    case kFmtIQ: fire(k_corrfn<MODE, kFmtIQ>); break;
    case kFmtPacked: fire(k_corrfn<MODE, kFmtPacked>); break;
    case kFmtReal16: fire(k_corrfn<MODE, kFmtReal16>); break;
    default: fire(k_corrfn<MODE, kFmtIQ16>); break;
    }
}

static bool cf_whole(double v) { return std::isfinite(v) && v == std::floor(v); }

// The three entries differ in where the record lies (bds_record.h).
static int corr_function_run(bds_ctx *ctx, const char *who, const bds_settings *s, const RecordSource &src, int n_items,
                             const int32_t *prn, const double *state6, int n_taps, const double *taps, double *out, int32_t *n_comp_out) {
    if (!s || !prn || !state6 || !taps || !out) return fail(ctx, BDS_ERR_ARG, "%s: NULL argument", who);
    if (n_items < 1) return fail(ctx, BDS_ERR_ARG, "%s: n_items = %d (at least one item)", who, n_items);
    if (n_taps < 1 || n_taps > kCfMaxTaps) return fail(ctx, BDS_ERR_ARG, "%s: n_taps = %d (1 .. %d)", who, n_taps, kCfMaxTaps);
    double tau_min = taps[0], tau_max = taps[0];
    for (int i = 0; i < n_taps; ++i) {
        if (!std::isfinite(taps[i]) || std::fabs(taps[i]) > kCfMaxTau)
            return fail(ctx, BDS_ERR_ARG, "%s: taps[%d] = %g (finite, at most %g chips either way)", who, i, taps[i], kCfMaxTau);
        tau_min = std::min(tau_min, taps[i]), tau_max = std::max(tau_max, taps[i]);
    }
    if (int rc = track_session_guard(ctx, who)) return rc;  // (the code tables are the open session's: another signal would replace them)
    const size_t n_bytes = src.size();
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    TrkOpenLoop o{};
    if (int rc = track_open_loop_setup(ctx, *s, n_bytes, o)) return rc;
    const int fmt = o.fmt;
    const int n_comp = 1 + (o.pilot ? 1 : 0) + (o.mode == BDS_TRACK_WB && o.pilot ? 1 : 0);
    const int V = n_comp * n_taps * 2;
    const double sc = o.mode == BDS_TRACK_B2A ? 1.0 : 2.0;
    // ---- every item, before anything is launched
    long max_blk = 0;
    for (int i = 0; i < n_items; ++i) {
        const double *q = state6 + (size_t)i * 6;
        if (prn[i] < 1 || prn[i] > BDS_MAX_PRN) return fail(ctx, BDS_ERR_ARG, "%s: prn[%d] = %d out of range", who, i, (int)prn[i]);
        if (!cf_whole(q[0]) || q[0] < 0 || q[0] >= 9.0e15) return fail(ctx, BDS_ERR_ARG, "%s: item %d: sample offset %g (a whole number >= 0)", who, i, q[0]);
        if (!cf_whole(q[1]) || q[1] < 1 || q[1] > 2.0e9) return fail(ctx, BDS_ERR_ARG, "%s: item %d: blksize %g (a whole number, 1 .. 2e9)", who, i, q[1]);
        if (!std::isfinite(q[2]) || !(q[3] > 0) || !std::isfinite(q[3]) || !std::isfinite(q[4]) || !std::isfinite(q[5]))
            return fail(ctx, BDS_ERR_ARG, "%s: item %d: remCodePhase, codeFreq (> 0), remCarrPhase and carrFreq must be finite", who, i);
        const long long pos = (long long)q[0];
        const long blk = (long)q[1];
        if (pos + blk > o.n_samples)
            return fail(ctx, BDS_ERR_ARG, "%s: item %d reaches past the end of the record (samples %lld .. %lld of %lld)", who, i, pos, pos + blk,
                        o.n_samples);
        const double rem = q[2], step = q[3] / o.fs;
        const double last = (double)(blk - 1) * step + rem;
        for (int j = 0; j < n_taps; ++j) {  // MATLAB would stop at tcode(blksize) otherwise
            const ColonVec cv = colon_vec((rem + taps[j]) * sc, step * sc, (last + taps[j]) * sc);
            if ((long)cv.n != blk - 1)
                return fail(ctx, BDS_ERR_ARG, "%s: item %d, tap %d (%g chips): the replica's colon vector has %ld elements for blksize %ld", who, i, j,
                            taps[j], (long)cv.n + 1, blk);
        }
        max_blk = std::max(max_blk, blk);
    }
    // ---- items by position, batches whose span of the record fits the resident limit
    std::vector<int> order(n_items);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return state6[(size_t)a * 6] < state6[(size_t)b * 6]; });
    const size_t limit = o.resident_limit ? o.resident_limit : kCfResident;
    const long long al = fmt_align(fmt);
    auto span_of = [&](long long first, long long end, size_t &off, size_t &bytes) {  // bytes of the record that hold [first, end)
        const long long b0 = first / al * al, e0 = std::min<long long>((end + 1) / 2 * 2, o.n_samples + (o.n_samples & 1));
        off = (size_t)fmt_bytes(fmt, b0);
        bytes = std::min((size_t)fmt_bytes(fmt, e0), n_bytes) - off;
        return b0;
    };
    struct Batch {
        int first, count;  // in `order`
        long long base, end;
        size_t off, bytes;
    };
    std::vector<Batch> batches;
    size_t max_bytes = 0;
    for (int i = 0; i < n_items;) {
        const double *q = state6 + (size_t)order[i] * 6;
        const long long first = (long long)q[0];
        long long end = first + (long)q[1];
        Batch b{i, 1, 0, end, 0, 0};
        b.base = span_of(first, end, b.off, b.bytes);
        if (b.bytes > limit)
            return fail(ctx, BDS_ERR_ARG, "%s: item %d alone needs %zu bytes of the record resident, the limit is %zu (bds_track_set_resident_limit)",
                        who, order[i], b.bytes, limit);
        int j = i + 1;
        for (; j < n_items; ++j) {
            const double *r = state6 + (size_t)order[j] * 6;
            const long long e2 = std::max(end, (long long)r[0] + (long)r[1]);
            size_t off2, bytes2;
            span_of(first, e2, off2, bytes2);
            if (bytes2 > limit) break;
            end = e2, b.bytes = bytes2;
        }
        b.count = j - i, b.end = end;
        max_bytes = std::max(max_bytes, b.bytes);
        batches.push_back(b);
        i = j;
    }
    const int max_chunks = (int)((max_blk + kCfChunk - 1) / kCfChunk);
    const size_t item_part = (size_t)max_chunks * V * sizeof(double);
    const int per_launch = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)n_items, 65535), kCfPartBytes / item_part));
    // ---- device buffers, released on every exit path
    int8_t *d_data = nullptr;
    int *d_prn = nullptr;
    double *d_s6 = nullptr, *d_taps = nullptr, *d_part = nullptr, *d_out = nullptr;
    DevScope scope;
    hipStream_t stream = (hipStream_t)ctx->stream;
    if (scope.alloc(&d_data, max_bytes + kDataSlack) != hipSuccess || scope.alloc(&d_prn, sizeof(int) * n_items) != hipSuccess ||
        scope.alloc(&d_s6, sizeof(double) * 6 * n_items) != hipSuccess || scope.alloc(&d_taps, sizeof(double) * n_taps) != hipSuccess ||
        scope.alloc(&d_part, item_part * per_launch) != hipSuccess || scope.alloc(&d_out, sizeof(double) * (size_t)n_items * V) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, BDS_ERR_NOMEM, "%s: device buffers (%zu bytes of the record, %zu of partial sums)", who, max_bytes, item_part * per_launch);
    }
    std::vector<int> h_prn(n_items);
    std::vector<double> h_s6((size_t)n_items * 6);
    for (int i = 0; i < n_items; ++i) {
        h_prn[i] = prn[order[i]];
        std::copy(state6 + (size_t)order[i] * 6, state6 + (size_t)order[i] * 6 + 6, h_s6.begin() + (size_t)i * 6);
    }
    auto mark = [&]() -> hipEvent_t {
        hipEvent_t e = nullptr;
        if (scope.event(&e) != hipSuccess) return nullptr;
        (void)hipEventRecord(e, stream);
        return e;
    };
    const hipEvent_t ev_begin = mark();
    BDS_HIP(ctx, hipMemcpyAsync(d_prn, h_prn.data(), sizeof(int) * n_items, hipMemcpyHostToDevice, stream));
    BDS_HIP(ctx, hipMemcpyAsync(d_s6, h_s6.data(), sizeof(double) * 6 * n_items, hipMemcpyHostToDevice, stream));
    BDS_HIP(ctx, hipMemcpyAsync(d_taps, taps, sizeof(double) * n_taps, hipMemcpyHostToDevice, stream));
    CfParams p{};
    p.pilot = o.pilot, p.n_comp = n_comp, p.n_taps = n_taps, p.code_len = o.code_len, p.max_chunks = max_chunks;
    p.fs = o.fs, p.inv_fs = o.inv_fs, p.tau_min = tau_min, p.tau_max = tau_max;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> kernel_spans;
    for (const Batch &b : batches) {
        if (int rc = src.load(b.off, b.bytes, d_data, stream)) return rc;
        p.base = b.base;
        p.win_end = b.base + fmt_samples(fmt, (long long)b.bytes);
        for (int i0 = 0; i0 < b.count; i0 += per_launch) {
            const int n = std::min(per_launch, b.count - i0), at = b.first + i0;
            const dim3 grid(max_chunks, n);
            const hipEvent_t e0 = mark();
            if (o.mode == BDS_TRACK_B2A)
                cf_launch_fmt<BDS_TRACK_B2A>(ctx, fmt, grid, stream, d_data, o.d_prim, p, d_prn + at, d_s6 + (size_t)at * 6, d_taps, d_part);
            else if (o.mode == BDS_TRACK_NB)
                cf_launch_fmt<BDS_TRACK_NB>(ctx, fmt, grid, stream, d_data, o.d_prim, p, d_prn + at, d_s6 + (size_t)at * 6, d_taps, d_part);
            else
                cf_launch_fmt<BDS_TRACK_WB>(ctx, fmt, grid, stream, d_data, o.d_prim, p, d_prn + at, d_s6 + (size_t)at * 6, d_taps, d_part);
            hipLaunchKernelGGL(k_corrfn_reduce, dim3((V + 255) / 256, n), dim3(256), 0, stream, (const double *)d_part,
                               (const double *)(d_s6 + (size_t)at * 6), max_chunks, V, d_out + (size_t)at * V);
            BDS_HIP(ctx, hipGetLastError());
            kernel_spans.emplace_back(e0, mark());
        }
    }
    std::vector<double> h_out((size_t)n_items * V);
    BDS_HIP(ctx, hipMemcpyAsync(h_out.data(), d_out, sizeof(double) * h_out.size(), hipMemcpyDeviceToHost, stream));
    const hipEvent_t ev_end = mark();
    BDS_HIP(ctx, hipStreamSynchronize(stream));
    for (int i = 0; i < n_items; ++i) std::copy(h_out.begin() + (size_t)i * V, h_out.begin() + (size_t)(i + 1) * V, out + (size_t)order[i] * V);
    if (n_comp_out) *n_comp_out = n_comp;
    // bds_get_timing: total_ms the call's stream time, search_ms its kernels alone, n_pairs its batches, n_comp
    ctx->timing = bds_timing{};
    float ms = 0.f;
    if (ev_begin && ev_end && hipEventElapsedTime(&ms, ev_begin, ev_end) == hipSuccess) ctx->timing.total_ms = ms;
    for (const auto &ks : kernel_spans)
        if (ks.first && ks.second && hipEventElapsedTime(&ms, ks.first, ks.second) == hipSuccess) ctx->timing.search_ms += ms;
    ctx->timing.n_pairs = (int64_t)batches.size();
    ctx->timing.n_comp = n_comp;
    return BDS_OK;
}

}  // namespace bds

using namespace bds;

extern "C" int bds_corr_function_mem(bds_ctx *ctx, const bds_settings *s, const int8_t *file_bytes, size_t n_bytes, int n_items,
                                     const int32_t *prn, const double *state6, int n_taps, const double *taps, double *out,
                                     int32_t *n_comp) {
    if (!ctx) return BDS_ERR_ARG;
    if (!file_bytes) return fail(ctx, BDS_ERR_ARG, "bds_corr_function_mem: file_bytes is NULL");
    RecordSource src;
    src.set_host(ctx, file_bytes, n_bytes);
    return corr_function_run(ctx, "bds_corr_function_mem", s, src, n_items, prn, state6, n_taps, taps, out, n_comp);
}

extern "C" int bds_corr_function_dev(bds_ctx *ctx, const bds_settings *s, const void *d_file_bytes, size_t n_bytes, int n_items,
                                     const int32_t *prn, const double *state6, int n_taps, const double *taps, double *out,
                                     int32_t *n_comp) {
    if (!ctx) return BDS_ERR_ARG;
    if (!d_file_bytes) return fail(ctx, BDS_ERR_ARG, "bds_corr_function_dev: d_file_bytes is NULL");
    if (int rc = check_device_span(ctx, "bds_corr_function_dev", "d_file_bytes", d_file_bytes, n_bytes)) return rc;
    RecordSource src;
    src.set_device(ctx, d_file_bytes, n_bytes);
    return corr_function_run(ctx, "bds_corr_function_dev", s, src, n_items, prn, state6, n_taps, taps, out, n_comp);
}

extern "C" int bds_corr_function(bds_ctx *ctx, const bds_settings *s, const char *path, int n_items, const int32_t *prn,
                                 const double *state6, int n_taps, const double *taps, double *out, int32_t *n_comp) {
    if (!ctx) return BDS_ERR_ARG;
    if (!path) return fail(ctx, BDS_ERR_ARG, "bds_corr_function: path is NULL");
    RecordSource src;
    if (int rc = src.open_file(ctx, path, kCfStage)) return rc;
    return corr_function_run(ctx, "bds_corr_function", s, src, n_items, prn, state6, n_taps, taps, out, n_comp);
}
