// Tracking: channel-batched correlate-and-dump + DLL/PLL loop update on the GPU.
//
// Replaces BDS-3_B2a/tracking.m:98-441, BDS-3_B1C/NB_tracking.m:107-448 and
// BDS-3_B1C/WB_tracking.m:114-488 (the per-channel, per-epoch MATLAB loops), plus the
// C/N0 + lock-detector post-pass of include/Calc_CNo_PLD.m.
//
// Structure: the window of the IF record the channels can touch lives in HBM (int8).  Every epoch is ONE launch:
//   k_trk_correlate  grid (workgroups, channels).  Head: every workgroup applies the loop update of the previous
//                    epoch to the channel state (apply_update: fixed-order sum of that epoch's partial sums, the
//                    discriminators and loop filters in f64 exactly in the reference's operation order; workgroup 0
//                    writes the result arrays and the new state; state and partial sums ping-pong between buffers).
//                    Body: the workgroup re-derives the epoch geometry (blksize, code / carrier NCO start values)
//                    from the f64 state and emits its 6/12/18 partial correlator sums -- correlate_runs (default:
//                    prefix sums of the carrier-wiped samples + an exact search of the code-index steps) or
//                    correlate_slice (per sample, BDS_TRK_PERSAMPLE)
//   k_trk_update     apply_update as its own launch: closes the last epoch (and every epoch with
//                    BDS_TRK_NOFUSE_UPDATE)
// The host enqueues all epochs back to back and never synchronises inside the loop: the
// sequential dependence (next blksize / phases depend on this epoch's discriminators) is
// carried entirely by device memory.
// A window that does not fit (or exceeds bds_track_set_resident_limit) is STREAMED: the same launches in batches of epochs
// over a span of the record that slides through two half-size buffers, the next piece loading while a batch runs (do_track).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <type_traits>

#include "bds_debug.h"
#include "bds_internal.h"
#include "bds_record.h"
#include "bds_strict_math.h"
#include "bds_trk_replica.h"

namespace bds {

// samples per correlate workgroup (TrkParams::chunk): 8192 for the 10-ms B1C epochs, 2048 for the
// 1-ms B2a epochs (measured on 12 channels at 99.375 MS/s, us per epoch: B1C WB 148 / 93 / 84 / 82 and
// B2a 23.3 / 20.2 / 21.7 / 29.7 at 1024 / 2048 / 4096 / 8192)
static constexpr int kTrkThreads = 256;
static constexpr int kNSums = 18;      // I_E,Q_E,I_P,Q_P,I_L,Q_L x {data, pilot BOC11 / B2a pilot, pilot BOC61}

struct ChanState {
    double codeFreq, remCodePhase, carrFreq, carrFreqBasis, remCarrPhase;
    double oldCodeNco, oldCodeError, d2CarrError, dCarrError;
    double codeFreqBasis;  // channel.codeFreq (tracking.m:389)
    long long pos;         // sample offset of the next read: ftell / dataAdaptCoeff (tracking.m:226)
    int prn;               // 0 = channel unused
    int active;            // 1 while the channel keeps tracking; 0 stopped at a short read (end of file);
                           // -2 its reads left the part of the record held in HBM (one window: the host reloads the whole
                           // file; streamed: the host repeats the batch from the state it started with)
    int completed;         // epochs finished
    int pad;
};

static constexpr int kUpdGroups = 14;    // groups of correlate workgroups in the fixed-order sum of the partial sums
static constexpr int kUpdThreads = 256;  // >= kUpdGroups * kNSums
static constexpr int kUpdScratch = (1 + kUpdGroups) * kNSums * 8 + 48 + (int)sizeof(ChanState);  // LDS bytes of apply_update

struct TrkParams {
    int mode;        // BDS_TRACK_*
    int pilot;       // pilot correlators on
    int cplx;        // sample format (kFmt*): fileType 2, the record is interleaved I/Q int8 pairs (tracking.m:132-136,242-246);
                     // fileType 3, two 2+2-bit I/Q samples per byte (unpack_cplx.m:18-30); dataType 1, int16 samples or pairs
    int chunk;       // samples per correlate workgroup
    int runs;        // 1: run-based correlator (correlate_runs), chunk = kTrkThreads * 8 or * 16
    int prec;        // numerics of the run-based correlator's carrier wipe-off and prefix sums (Tuning::trk_prec)
    int code_len;    // 10230
    int n_epochs;
    double fs, inv_fs;
    double spacing;  // dllCorrelatorSpacing (earlyLateSpc)
    double tau1, tau2, pdi, pf1, pf2, pf3, factor;
    long long n_bytes;  // samples in the record: file bytes / dataAdaptCoeff (packed: 2 per byte)
    long long base;     // first sample of the record held in HBM (only the window the channels can touch is loaded;
                        // streamed: the resident span, which moves between launches)
    long long win_end;  // one past the last sample held
};

// (the sample formats kFmt*, fmt_* and iq_of_packed: bds_trk_replica.h)

struct TrkOut {  // device arrays [n_ch][n_epochs]
    double *absoluteSample, *codeFreq, *carrFreq, *I_P, *I_E, *I_L, *Q_E, *Q_P, *Q_L;
    double *Pilot_I_P, *Pilot_Q_P, *Pilot_I_E, *Pilot_I_L, *Pilot_Q_E, *Pilot_Q_L;
    double *dllDiscr, *dllDiscrFilt, *pllDiscr, *pllDiscrFilt, *remCodePhase, *remCarrPhase;
};

// Padded-array look-up of the reference: [c(L) c(1..L) c(1)], 1-based index i in 1..L+2
// (B2a/tracking.m:158; B1C/WB_tracking.m:181,187,192).  The device keeps, per PRN, the three arrays
// the trackers index -- data code, pilot code, pilot BOC(6,1) -- expanded to their own resolution
//   B2a: chips;  B1C: BOC(1,1) half-chips [-c, +c] (generateDataBOC11.m:85-91);
//   BOC(6,1): twelfths (-1)^ii c, ii = 1..12 (generatePilotBOC61.m:89-96)
// with kTabPad wrapped entries on both sides, so a look-up is one clamped index and one byte load
// (deriving chip, sub-chip sign and wrap from the index cost ~11 instructions per look-up, nine
// look-ups per sample in wide-band mode).  (kTabPad, kTabStride: bds_trk_replica.h)
__device__ __forceinline__ float tab_at(const int8_t *__restrict__ tab, int n_units, int i1) {
    int j = i1 + (kTabPad - 2);  // unit index i1 - 2, shifted by the left padding
    BDS_DASSERT(j >= 0 && j <= n_units + 2 * kTabPad - 1);  // (the clamp below is a guard, never the intended look-up)
    j = max(0, min(j, n_units + 2 * kTabPad - 1));
    return (float)tab[j];
}
// data and pilot codes are read at the same index: slot 0 of a PRN holds them interleaved
__device__ __forceinline__ char2 tab2_at(const int8_t *__restrict__ tab, int n_units, int i1) {
    int j = i1 + (kTabPad - 2);
    BDS_DASSERT(j >= 0 && j <= n_units + 2 * kTabPad - 1);
    j = max(0, min(j, n_units + 2 * kTabPad - 1));
    return reinterpret_cast<const char2 *>(tab)[j];
}

// (the reference's replica index vectors -- ColonVec, colon_vec, colon_at --: bds_trk_replica.h)
// the three replica vectors of an epoch: E, P, L
template <int SCALE2>
__device__ __forceinline__ void epoch_colons(double rem, double step, double spacing, long blk, ColonVec cv[3]) {
    const double sc = SCALE2 ? 2.0 : 1.0;
    const double last = (double)(blk - 1) * step + rem;  // (blksize-1)*codePhaseStep + remCodePhase, then -+ earlyLateSpc, then *2
    cv[0] = colon_vec((rem - spacing) * sc, step * sc, (last - spacing) * sc);
    cv[1] = colon_vec(rem * sc, step * sc, last * sc);
    cv[2] = colon_vec((rem + spacing) * sc, step * sc, (last + spacing) * sc);
    BDS_DASSERT(cv[0].n == blk - 1 && cv[1].n == blk - 1 && cv[2].n == blk - 1);  // MATLAB would stop at tcode(blksize) otherwise
}

struct EpochGeom {
    long long pos;
    long blk;
    double step, rem, carrFreq, remCarr;
};

__device__ __forceinline__ EpochGeom epoch_geom(const ChanState &s, const TrkParams &p) {
    EpochGeom g;
    g.pos = s.pos;
    g.step = s.codeFreq / p.fs;                                               // tracking.m:230
    g.blk = (long)ceil(((double)p.code_len - s.remCodePhase) / g.step);       // :233
    g.rem = s.remCodePhase;
    g.carrFreq = s.carrFreq;
    g.remCarr = s.remCarrPhase;
    return g;
}

// One block of samples [k0, k1) of one channel: 18 partial sums (f64) to part[].
template <int MODE>
__device__ __forceinline__ void correlate_slice(const int8_t *__restrict__ data, const int8_t *__restrict__ prim_d,
                                                const int8_t *__restrict__ prim_p, const TrkParams &p,
                                                const EpochGeom &g, long k0_first, long k_stride, bool pilot, double *sums) {
    constexpr int UNITS = MODE == BDS_TRACK_B2A ? 1 : 2;
    const int NU = UNITS * p.code_len;
    ColonVec cv[3];  // tracking.m:260-286 / WB_tracking.m:289-317
    epoch_colons<(MODE != BDS_TRACK_B2A)>(g.rem, g.step, p.spacing, g.blk, cv);
    const double two_pi = 6.283185307179586476925286766559;
    const double cyc0 = g.remCarr / two_pi;
    float acc[kNSums];
#pragma unroll
    for (int i = 0; i < kNSums; ++i) acc[i] = 0.f;
    double wr, wi, cr = 1.0, ci = 0.0;
    {
        const double dcyc = g.carrFreq * ((double)blockDim.x * p.inv_fs);
        sincospi(2.0 * (dcyc - floor(dcyc)), &wi, &wr);
    }
    int it = 0;
    // data[] starts at sample p.base of the record (packed: p.base is even)
    const int8_t *__restrict__ dwin = p.cplx == kFmtPacked ? data - (p.base >> 1) : data - (p.base * fmt_bps(p.cplx));
    // chunk k0 .. k0+chunk of the block, then (only when blksize outgrew the grid the call was sized for:
    // a code rate more than 2 % below the slowest channel's initial one) every k_stride-th chunk after it
    for (long k0 = k0_first; k0 < g.blk; k0 += k_stride) {
    const long k1 = min(g.blk, k0 + p.chunk);
    for (int k = (int)k0 + (int)threadIdx.x; k < (int)k1; k += (int)blockDim.x) {  // blksize < 2^31
        float raw, raw_q = 0.f;
        BDS_DASSERT(g.pos + k >= p.base && g.pos + k < p.win_end);  // inside the window of the record held in HBM
        if (p.cplx == kFmtPacked) {  // nibble (pos + k) & 1 of byte (pos + k) >> 1
            const long long n = g.pos + k;
            const uint32_t v = iq_of_packed(((uint32_t)(uint8_t)dwin[n >> 1] >> (4 * (int)(n & 1))) & 15u);
            raw = (float)(int8_t)(v & 0xffu);
            raw_q = (float)(int8_t)(v >> 8);
        } else if (p.cplx == kFmtReal16) {  // fread(fid, blksize, 'int16')
            raw = (float)reinterpret_cast<const short *>(dwin)[g.pos + k];
        } else if (p.cplx == kFmtIQ16) {
            const short2 v = reinterpret_cast<const short2 *>(dwin)[g.pos + k];
            raw = (float)v.x;
            raw_q = (float)v.y;
        } else if (p.cplx) {  // rawSignal = data(1:2:end) + 1i*data(2:2:end)  (tracking.m:242-246)
            const char2 v = reinterpret_cast<const char2 *>(dwin)[g.pos + k];
            raw = (float)v.x;
            raw_q = (float)v.y;
        } else {
            raw = (float)dwin[g.pos + k];
        }
        const double kd = (double)k;
        const double te = colon_at(cv[0], k), tp = colon_at(cv[1], k), tl = colon_at(cv[2], k);
        const int ie = (int)ceil(te) + 1, il = (int)ceil(tl) + 1, ip = (int)ceil(tp) + 1;
        // carrier: trigarg = (carrFreq*2*pi)*(k/fs) + remCarrPhase  (tracking.m:303-304).  A thread's
        // samples are blockDim apart, so its carrier is an f64 phasor rotated by a constant angle; it is
        // re-evaluated exactly (phase reduced in f64, cycles) every 8th step.
        if ((it & 7) == 0) {
            const double cyc = g.carrFreq * (kd * p.inv_fs) + cyc0;
            sincospi(2.0 * (cyc - floor(cyc)), &ci, &cr);
        } else {
            const double nr = cr * wr - ci * wi;
            ci = cr * wi + ci * wr;
            cr = nr;
        }
        ++it;
        const float c2 = (float)cr, s2 = (float)ci;
        float ib, qb;
        if (MODE == BDS_TRACK_B2A) {  // exp(+j th): q = real, i = imag (tracking.m:309-314)
            qb = raw * c2 - raw_q * s2;
            ib = raw * s2 + raw_q * c2;
        } else {  // exp(-j th): i = real, q = imag (NB_tracking.m:320-325)
            ib = raw * c2 + raw_q * s2;
            qb = raw_q * c2 - raw * s2;
        }
        const char2 ve = tab2_at(prim_d, NU, ie), vp = tab2_at(prim_d, NU, ip), vl = tab2_at(prim_d, NU, il);
        const float ce = (float)ve.x, cp = (float)vp.x, cl = (float)vl.x;
        acc[0] = fmaf(ce, ib, acc[0]);
        acc[1] = fmaf(ce, qb, acc[1]);
        acc[2] = fmaf(cp, ib, acc[2]);
        acc[3] = fmaf(cp, qb, acc[3]);
        acc[4] = fmaf(cl, ib, acc[4]);
        acc[5] = fmaf(cl, qb, acc[5]);
        if (pilot) {
            const float pe = (float)ve.y, pp = (float)vp.y, pl = (float)vl.y;
            acc[6] = fmaf(pe, ib, acc[6]);
            acc[7] = fmaf(pe, qb, acc[7]);
            acc[8] = fmaf(pp, ib, acc[8]);
            acc[9] = fmaf(pp, qb, acc[9]);
            acc[10] = fmaf(pl, ib, acc[10]);
            acc[11] = fmaf(pl, qb, acc[11]);
            if (MODE == BDS_TRACK_WB) {  // pilotBOC61(ceil(tcode*6)+1)  (WB_tracking.m:298,311,324)
                const int8_t *p6 = prim_p;  // the PRN's BOC(6,1) array
                const float se = tab_at(p6, 12 * p.code_len, (int)ceil(te * 6) + 1);
                const float sp = tab_at(p6, 12 * p.code_len, (int)ceil(tp * 6) + 1);
                const float sl = tab_at(p6, 12 * p.code_len, (int)ceil(tl * 6) + 1);
                acc[12] = fmaf(se, ib, acc[12]);
                acc[13] = fmaf(se, qb, acc[13]);
                acc[14] = fmaf(sp, ib, acc[14]);
                acc[15] = fmaf(sp, qb, acc[15]);
                acc[16] = fmaf(sl, ib, acc[16]);
                acc[17] = fmaf(sl, qb, acc[17]);
            }
        }
    }
    }
    // wave reduction (f64 from here), then one LDS hop
    __shared__ double s_part[kTrkThreads / 64][kNSums];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < kNSums; ++i) {
        double v = (double)acc[i];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) s_part[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < kNSums) {
        double v = 0;
        for (int w = 0; w < kTrkThreads / 64; ++w) v += s_part[w][threadIdx.x];
        sums[threadIdx.x] = v;
    }
}


// ---- run-based correlator ---------------------------------------------------------------------
// The replica codes are piecewise constant: at 99.375 MS/s a BOC(1,1) half-chip lasts 48.6 samples,
// a BOC(6,1) twelfth 8.1, a B2a chip 9.7.  With S(k) = the running sum of the carrier-wiped samples,
//     sum_k x[k] c[idx(k)]  =  c[idx(last)] S(end)  -  sum over index steps u (c[u] - c[u-1]) S(k_u),
// k_u = the first sample whose index reaches u.  The per-sample index of the reference, ceil() of element k of its colon
// vector (ColonVec above; x 6 for BOC(6,1), WB_tracking.m:298), is monotone in k -- neighbouring elements are one step apart to
// a few ulp in both halves and across the junction --, so k_u is found
// from a division and confirmed with the reference's own expression on k_u - 1 and k_u: every sample gets
// exactly the index the per-sample evaluation gives it, at two exact evaluations per code unit instead
// of one per sample and replica.
//   phase 1  thread t wipes the carrier off SEG consecutive samples (per-thread f64 phasor x a table
//            of the SEG per-sample rotations), writes the exclusive fp32 prefix sums of its segment to
//            LDS; the segment totals are scanned in f64 over the workgroup (segment bases)
//   phase 2  the index steps of the six (E/P/L x {code, BOC(6,1)}) sequences are spread over the
//            threads; each finds its k_u, reads S(k_u) = base + local prefix and adds its term in f64
static constexpr int kCap1 = 256, kCap6 = 1280;  // code / BOC(6,1) table entries of a wave's pass staged in LDS
// (code_arg, first_sample_of -- the exact search of an index step's first sample --: bds_trk_replica.h)

// LDS of one wave of correlate_runs<., SEG>: prefix sums, segment bases, rotation table, code-table slices
// (prec: TrkParams::prec -- 0 fp32 carrier + fp32 local prefix sums, 1 f64 prefix sums, 2 f64 carrier too, 3 the
// reference's own trigarg per sample; f64 prefix entries are 16 bytes, the f64 rotation table as well)
__host__ __device__ constexpr size_t runs_wave_lds(int seg, int prec) {
    return (size_t)(64 * seg + 64) * (prec >= 1 ? 16 : 8) + 64 * 16 + (size_t)seg * (prec >= 2 ? 16 : 8) + (size_t)kCap1 * 2 + kCap6;
}
static inline size_t runs_lds_bytes(int seg, int prec) {
    return std::max<size_t>(runs_wave_lds(seg, prec) * (kTrkThreads / 64), sizeof(double) * (kTrkThreads / 64) * kNSums);
}
// (wave_sync, the 64-lane f64 add-scan wave_scan_incl and lane_f64: bds_trk_replica.h)

// The waves of a workgroup work independently (wave w on samples k0 + w 64 SEG .. of each chunk, its own LDS
// slice, no workgroup barrier before the final reduction): the kernel is bound by latency -- HBM reads,
// dependent f64 evaluations -- and independent waves hide it where barrier-separated phases cannot.
template <int MODE, int SEG, int FMT, int PREC>
__device__ __forceinline__ void correlate_runs(const int8_t *__restrict__ data, const int8_t *__restrict__ prim_d,
                                               const int8_t *__restrict__ prim_p, const TrkParams &p,
                                               const EpochGeom &g, long k0_first, long k_stride, bool pilot, double *sums) {
    constexpr int NT = kTrkThreads, NW = NT / 64, WCH = 64 * SEG;
    constexpr double scale = MODE == BDS_TRACK_B2A ? 1.0 : 2.0;
    constexpr int UNITS = MODE == BDS_TRACK_B2A ? 1 : 2;
    constexpr int NWD = SEG / 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char trk_lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // PT: type of a segment's local prefix sums; CT: type of the carrier replica and the wiped samples
    using PT = std::conditional_t<(PREC >= 1), double, float>;
    using PT2 = std::conditional_t<(PREC >= 1), double2, float2>;
    using CT = std::conditional_t<(PREC >= 2), double, float>;
    using CT2 = std::conditional_t<(PREC >= 2), double2, float2>;
    constexpr size_t kLoc = (size_t)(WCH + 64) * sizeof(PT2);
    unsigned char *wl = trk_lds + runs_wave_lds(SEG, PREC) * wave;
    PT2 *s_loc = reinterpret_cast<PT2 *>(wl);                                       // [WCH + 64]: position i at i + i / SEG
    double2 *s_base = reinterpret_cast<double2 *>(wl + kLoc);                       // [64] segment bases
    CT2 *s_w = reinterpret_cast<CT2 *>(wl + kLoc + 64 * 16);                        // [SEG]
    char2 *s_t1 = reinterpret_cast<char2 *>(wl + kLoc + 64 * 16 + (size_t)SEG * sizeof(CT2));  // [kCap1]
    int8_t *s_t6 = reinterpret_cast<int8_t *>(s_t1 + kCap1);                                    // [kCap6]
    const int NU = UNITS * p.code_len, n6 = 12 * p.code_len;
    const double inc = g.step * scale, inv_inc = 1.0 / inc;
    ColonVec cv3[3];  // E, P, L
    epoch_colons<(MODE != BDS_TRACK_B2A)>(g.rem, g.step, p.spacing, g.blk, cv3);
    const double two_pi = 6.283185307179586476925286766559;
    const double cyc0 = g.remCarr / two_pi;
    constexpr bool CPLX = fmt_complex(FMT);
    constexpr bool W16 = fmt_16bit(FMT);  // int16 samples: two per dword, an I/Q pair is one dword
    constexpr int coeff = FMT == kFmtPacked ? 2 : fmt_bps(FMT);  // bytes of a sample (packed: of the pair it decodes to)
    constexpr int nwd = NWD * coeff;  // dwords of a segment
    constexpr int nrd = FMT == kFmtPacked ? SEG / 8 : nwd;  // ... as the record holds it (packed: SEG / 2 bytes)
    // dwords fetched: one more than the segment's, for the funnel shift -- except int16 pairs, which start on a dword
    constexpr int nfd = FMT == kFmtIQ16 ? nrd : nrd + 1;
    const int8_t *__restrict__ dwin = FMT == kFmtPacked ? data - (p.base >> 1) : data - p.base * coeff;  // (packed: p.base is even)
    // address of the byte that holds sample pos + kb
    auto seg_addr = [&](long kb) {
        if constexpr (FMT == kFmtPacked)
            return (uintptr_t)(dwin + ((g.pos + kb) >> 1));
        else
            return (uintptr_t)(dwin + (g.pos + kb) * coeff);
    };
    double acc[kNSums];
#pragma unroll
    for (int i = 0; i < kNSums; ++i) acc[i] = 0.0;
    if ((PREC < 3 || PREC == 5) && lane < SEG) {  // rotation of sample j of a segment against its first sample
        const double cyc = g.carrFreq * ((double)lane * p.inv_fs);
        double sn, cs;
        sincospi(2.0 * (cyc - floor(cyc)), &sn, &cs);
        s_w[lane].x = (CT)cs, s_w[lane].y = (CT)sn;
    }
    // PREC 3: the carrier argument of every sample exactly as the reference forms it,
    //   trigarg = (carrFreq*2*pi) .* ((0:blksize) ./ fs) + remCarrPhase   (tracking.m:303-304; left to right, one rounding
    // per operation: the translation unit is built with -ffp-contract=off), then sin / cos of that f64 value
    const double w_ref = (g.carrFreq * 2.0) * 3.14159265358979323846;
    // the segment's bytes (I/Q pairs: 2 SEG bytes; packed: SEG / 2, from either nibble of the first), whole aligned dwords around it
    uint32_t raw[nrd + 1];
    auto fetch = [&](long kw) {
        const long kb = kw + (long)lane * SEG;
        if (kb < g.blk) {
            BDS_DASSERT(g.pos + kb >= p.base && g.pos + kb < p.win_end);  // first sample of the segment inside the window held in HBM
            const uintptr_t a = seg_addr(kb);
            const uint32_t *__restrict__ q = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
#pragma unroll
            for (int i = 0; i < nfd; ++i) raw[i] = q[i];
        }
    };
    const long kw_first = k0_first + (long)wave * WCH;
    if (kw_first < g.blk) fetch(kw_first);
    // carrier at this lane's first sample of the first pass (tracking.m:303-304); every further pass is k_stride
    // samples on: one f64 rotation instead of a sincospi per pass
    double bs, bc, rs = 0.0, rc = 1.0;
    {
        const double cyc = g.carrFreq * ((double)(kw_first + (long)lane * SEG) * p.inv_fs) + cyc0;
        sincospi(2.0 * (cyc - floor(cyc)), &bs, &bc);
        if (kw_first + k_stride < g.blk) {  // (wave-uniform) a second pass exists
            const double cyr = g.carrFreq * ((double)k_stride * p.inv_fs);
            sincospi(2.0 * (cyr - floor(cyr)), &rs, &rc);
        }
    }
    for (long kwl = kw_first; kwl < g.blk; kwl += k_stride) {
        const int k0 = (int)kwl, k1 = (int)min(g.blk, kwl + WCH);  // blksize < 2^31
        wave_sync();  // s_w written / the previous pass's phase 2 done with the LDS slice
        // ---- index ranges of this pass's E/P/L replicas and their slice of the code tables (phase 2 then reads LDS
        // instead of issuing dependent global loads; longer ranges -- low sampling rates -- stay in global memory)
        int ua1[3], ub1[3], ua6[3], ub6[3];
        {  // the twelve range ends are wave-uniform: lane 3 e + ph (+ 6 for BOC(6,1)) evaluates one, readlane spreads them
            const int ph = lane % 3, end = (lane / 3) & 1, r6 = (lane / 6) & 1;
            const ColonVec &cl = ph == 0 ? cv3[0] : ph == 1 ? cv3[1] : cv3[2];
            double v = colon_at(cl, end ? k1 - 1 : k0);  // as code_arg
            if (r6) v = v * 6;
            const int idx = (int)ceil(v);
#pragma unroll
            for (int ph2 = 0; ph2 < 3; ++ph2) {
                ua1[ph2] = __builtin_amdgcn_readlane(idx, ph2), ub1[ph2] = __builtin_amdgcn_readlane(idx, 3 + ph2);
                ua6[ph2] = __builtin_amdgcn_readlane(idx, 6 + ph2), ub6[ph2] = __builtin_amdgcn_readlane(idx, 9 + ph2);
            }
        }
        const int lo1 = min(ua1[0], min(ua1[1], ua1[2])), hi1 = max(ub1[0], max(ub1[1], ub1[2])) + 1;
        const int lo6 = min(ua6[0], min(ua6[1], ua6[2])), hi6 = max(ub6[0], max(ub6[1], ub6[2])) + 1;
        const bool use1 = hi1 - lo1 < kCap1, use6 = MODE == BDS_TRACK_WB && pilot && hi6 - lo6 < kCap6;
        if (use1)
            for (int i = lane; i <= hi1 - lo1; i += 64) s_t1[i] = tab2_at(prim_d, NU, lo1 + i);
        if (use6)
            for (int i = lane; i <= hi6 - lo6; i += 64) s_t6[i] = (int8_t)tab_at(prim_p, n6, lo6 + i);
        // ---- phase 1: wipe the carrier off this lane's SEG samples, exclusive prefix sums of the segment to LDS
        const int kb = k0 + lane * SEG;
        const int n_here = max(0, min(SEG, k1 - kb));
        PT run_i = 0, run_q = 0;
        if (n_here > 0) {
            uint32_t wr[nwd];
            if constexpr (FMT == kFmtPacked) {
                // funnel shift by the byte offset and the nibble, then every byte to the (I, Q, I, Q) dword of the I/Q record
                const uint32_t sh = 8u * (uint32_t)(seg_addr(kb) & 3) + 4u * (uint32_t)((g.pos + kb) & 1);
#pragma unroll
                for (int i = 0; i < nrd; ++i) {
                    const uint32_t w = __builtin_amdgcn_alignbit(raw[i + 1], raw[i], sh);
#pragma unroll
                    for (int b = 0; b < 4; ++b) wr[4 * i + b] = iq_of_packed((w >> (8 * b)) & 0xffu);
                }
            } else if constexpr (FMT == kFmtIQ16) {
                BDS_DASSERT((seg_addr(kb) & 3) == 0);  // (buffers are dword-aligned, a pair is 4 bytes)
#pragma unroll
                for (int i = 0; i < nwd; ++i) wr[i] = raw[i];
            } else {  // (int16 samples: byte offset 0 or 2)
                const uint32_t sh = (uint32_t)(seg_addr(kb) & 3);
#pragma unroll
                for (int i = 0; i < nwd; ++i) wr[i] = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], sh);
            }
            const CT bcf = (CT)bc, bsf = (CT)bs;
            const int lbase = lane * SEG + lane;
            double trig5 = 0.0, c5 = 1.0, s5 = 0.0;
            const double dlt5 = w_ref * p.inv_fs;
            if constexpr (PREC == 5) {  // the reference's trigarg of the segment's first sample and its phasor
                trig5 = (w_ref * div_by_fs((double)kb, p.fs, p.inv_fs)) + g.remCarr;
                sincos_strict(trig5, s5, c5);
            }
            // sample j of the segment, carrier-wiped: (ib, qb).  PREC < 3: the carrier is base x table entry with
            // explicit FMAs (the exact two-rounding rule of the build only matters for the code index), in fp32
            // (PREC 0, 1) or f64 (PREC 2); PREC 3: sin / cos of the reference's own trigarg(k)
            auto wiped = [&](int j, CT &ib, CT &qb) {
                CT rw, rw_q = 0;
                if constexpr (FMT == kFmtIQ16) {  // one dword: I in the low half, Q in the high half
                    const uint32_t w = wr[j];
                    rw = (CT)(int)(int16_t)w;
                    rw_q = (CT)(int)(int16_t)(w >> 16);
                } else if constexpr (W16) {
                    rw = (CT)(int)(int16_t)(wr[j >> 1] >> ((j & 1) * 16));
                } else if (CPLX) {  // rawSignal = data(1:2:end) + 1i*data(2:2:end)  (tracking.m:242-246)
                    const uint32_t w = wr[j >> 1];
                    rw = (CT)(int)(int8_t)(w >> ((j & 1) * 16));
                    rw_q = (CT)(int)(int8_t)(w >> ((j & 1) * 16 + 8));
                } else {
                    rw = (CT)(int)(int8_t)(wr[j >> 2] >> ((j & 3) * 8));
                }
                CT c2, s2;
                if constexpr (PREC == 3) {
                    const double tt = (double)(kb + j) / p.fs;
                    const double trig = (w_ref * tt) + g.remCarr;
                    sincos(trig, &s2, &c2);
                } else if constexpr (PREC == 5) {
                    // the same value from one library-free sin / cos per lane and pass: trigarg(k + j) = trigarg(k) + D_j with D_j
                    // EXACT (difference of two neighbouring f64 values), D_j = j dlt + eps_j with dlt = 2 pi carrFreq / fs and
                    // |eps_j| ~ 1e-10 rad the reference's own rounding noise, so
                    //   exp(i trigarg(k + j)) = exp(i trigarg(k)) x exp(i j dlt) x (1 + i eps_j)      (eps^2 / 2 < 1e-19)
                    // -- the segment's first phasor, the wave's rotation table, a first-order correction: 14 f64 operations per
                    // sample instead of 40
                    const double tt = div_by_fs((double)(kb + j), p.fs, p.inv_fs);
                    const double trig = (w_ref * tt) + g.remCarr;
                    const double eps = fma(-(double)j, dlt5, trig - trig5);
                    const CT2 w = s_w[j];
                    const double c1 = fma(c5, w.x, -(s5 * w.y)), s1 = fma(s5, w.x, c5 * w.y);
                    c2 = fma(-eps, s1, c1), s2 = fma(eps, c1, s1);
                } else if constexpr (PREC == 4) {
                    const double tt = div_by_fs((double)(kb + j), p.fs, p.inv_fs);
                    BDS_DASSERT(tt == (double)(kb + j) / p.fs);
                    BDS_DASSERT(tt == (double)(kb + j) / p.fs);
                    const double trig = (w_ref * tt) + g.remCarr;
                    sincos_strict(trig, s2, c2);
                } else {
                    const CT2 w = s_w[j];
                    c2 = fma(bcf, w.x, -(bsf * w.y)), s2 = fma(bsf, w.x, bcf * w.y);
                }
                if (MODE == BDS_TRACK_B2A) {  // exp(+j th): q = real, i = imag (tracking.m:309-314)
                    qb = CPLX ? fma(rw, c2, -(rw_q * s2)) : rw * c2;
                    ib = CPLX ? fma(rw, s2, rw_q * c2) : rw * s2;
                } else {  // exp(-j th): i = real, q = imag (NB_tracking.m:320-325)
                    ib = CPLX ? fma(rw, c2, rw_q * s2) : rw * c2;
                    qb = CPLX ? fma(rw_q, c2, -(rw * s2)) : -(rw * s2);
                }
            };
            if (n_here == SEG) {  // every segment but the last one of the block
#pragma unroll
                for (int j = 0; j < SEG; ++j) {
                    CT ib, qb;
                    wiped(j, ib, qb);
                    s_loc[lbase + j].x = run_i, s_loc[lbase + j].y = run_q;
                    run_i += (PT)ib, run_q += (PT)qb;
                }
            } else {
#pragma unroll
                for (int j = 0; j < SEG; ++j) {
                    CT ib, qb;
                    wiped(j, ib, qb);
                    s_loc[lbase + j].x = run_i, s_loc[lbase + j].y = run_q;
                    run_i += j < n_here ? (PT)ib : (PT)0, run_q += j < n_here ? (PT)qb : (PT)0;
                }
            }
        }
        if (kwl + k_stride < g.blk) {
            fetch(kwl + k_stride);  // next pass's bytes: in flight during the scan and phase 2
            const double nc = bc * rc - bs * rs;
            bs = bs * rc + bc * rs;
            bc = nc;
        }
        // exclusive f64 scan of the segment totals over the wave
        const double vi = wave_scan_incl((double)run_i), vq = wave_scan_incl((double)run_q);
        s_base[lane] = make_double2(vi - (double)run_i, vq - (double)run_q);
        const double ti = lane_f64(vi, 63), tq = lane_f64(vq, 63);  // pass totals
        wave_sync();
        // ---- phase 2
        auto prefix = [&](int kk) -> double2 {  // sum of the wiped samples k0 .. kk-1, kk in (k0, k1)
            const int pos = kk - k0, seg = pos / SEG;
            const double2 b = s_base[seg];
            const PT2 l = s_loc[pos + seg];
            return make_double2(b.x + (double)l.x, b.y + (double)l.y);
        };
        if (MODE != BDS_TRACK_B2A) {
            // B1C: ~21 half-chip steps per replica and pass -- one lane per (replica, step), the three replicas laid
            // end to end (63-66 items: one iteration as a rule), instead of three searches on a third of the lanes
            const int lo = lo1;
            auto at1 = [&](int i1) -> char2 {
                BDS_DASSERT(!use1 || (i1 - lo >= 0 && i1 - lo < kCap1));  // inside the table slice staged in LDS
                return use1 ? s_t1[i1 - lo] : tab2_at(prim_d, NU, i1);
            };
            const int n0 = ub1[0] - ua1[0], n1 = ub1[1] - ua1[1], n2 = ub1[2] - ua1[2];
            for (int r = lane; r < n0 + n1 + n2; r += 64) {
                const int ph = r < n0 ? 0 : r < n0 + n1 ? 1 : 2;
                const int u = (ph == 0 ? ua1[0] + r : ph == 1 ? ua1[1] + (r - n0) : ua1[2] + (r - n0 - n1)) + 1;
                const ColonVec &cl = ph == 0 ? cv3[0] : ph == 1 ? cv3[1] : cv3[2];
                const double thr = (double)(u - 1);
                int kk = (int)floor((thr - cl.a) * inv_inc) + 1;  // a prediction, confirmed with the exact expression
                kk = max(k0 + 1, min(kk, k1 - 1));
                if (!(!(code_arg<0>(cl, kk - 1) > thr) && code_arg<0>(cl, kk) > thr))
                    kk = first_sample_of<0>(cl, inv_inc, u, k0, k1 - 1);
                const double2 S = prefix(kk);
                const char2 cn = at1(u + 1), co = at1(u);
                const double dd = (double)((int)cn.x - (int)co.x), dp = (double)((int)cn.y - (int)co.y);
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const double d = ph == q ? dd : 0.0;
                    acc[2 * q] = fma(-d, S.x, acc[2 * q]);
                    acc[2 * q + 1] = fma(-d, S.y, acc[2 * q + 1]);
                    if (pilot) {
                        const double e = ph == q ? dp : 0.0;
                        acc[6 + 2 * q] = fma(-e, S.x, acc[6 + 2 * q]);
                        acc[7 + 2 * q] = fma(-e, S.y, acc[7 + 2 * q]);
                    }
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int ph = 0; ph < 3; ++ph) {
                    const char2 cl = at1(ub1[ph] + 1);
                    acc[2 * ph] += (double)cl.x * ti;
                    acc[2 * ph + 1] += (double)cl.x * tq;
                    if (pilot) {
                        acc[6 + 2 * ph] += (double)cl.y * ti;
                        acc[7 + 2 * ph] += (double)cl.y * tq;
                    }
                }
            }
        } else
        {  // code (and pilot code) at the look-up's own resolution: E, P, L steps of one rank together
            const int lo = lo1;
            auto at1 = [&](int i1) -> char2 {
                BDS_DASSERT(!use1 || (i1 - lo >= 0 && i1 - lo < kCap1));  // inside the table slice staged in LDS
                return use1 ? s_t1[i1 - lo] : tab2_at(prim_d, NU, i1);
            };
            const int nmax = max(ub1[0] - ua1[0], max(ub1[1] - ua1[1], ub1[2] - ua1[2]));
            for (int r = lane; r < nmax; r += 64) {
                int kk[3], uu[3];
                bool val[3], bad = false;
#pragma unroll
                for (int ph = 0; ph < 3; ++ph) {
                    uu[ph] = ua1[ph] + 1 + r;
                    val[ph] = uu[ph] <= ub1[ph];
                    const double thr = (double)(uu[ph] - 1);
                    int kc = (int)floor((thr - cv3[ph].a) * inv_inc) + 1;  // a prediction, confirmed with the exact expression
                    kc = max(k0 + 1, min(kc, k1 - 1));
                    const bool good = !(code_arg<0>(cv3[ph], kc - 1) > thr) && code_arg<0>(cv3[ph], kc) > thr;
                    bad |= val[ph] && !good;
                    kk[ph] = val[ph] ? kc : k0 + 1;
                }
                if (bad) {
#pragma unroll
                    for (int ph = 0; ph < 3; ++ph)
                        if (val[ph]) kk[ph] = first_sample_of<0>(cv3[ph], inv_inc, uu[ph], k0, k1 - 1);
                }
#pragma unroll
                for (int ph = 0; ph < 3; ++ph) {
                    const double2 S = prefix(kk[ph]);
                    const int u = val[ph] ? uu[ph] : ua1[ph];  // (u, u + 1) inside the staged range
                    const char2 cn = at1(u + 1), co = at1(u);
                    const double dd = val[ph] ? (double)((int)cn.x - (int)co.x) : 0.0;
                    acc[2 * ph] = fma(-dd, S.x, acc[2 * ph]);
                    acc[2 * ph + 1] = fma(-dd, S.y, acc[2 * ph + 1]);
                    if (pilot) {
                        const double dp = val[ph] ? (double)((int)cn.y - (int)co.y) : 0.0;
                        acc[6 + 2 * ph] = fma(-dp, S.x, acc[6 + 2 * ph]);
                        acc[7 + 2 * ph] = fma(-dp, S.y, acc[7 + 2 * ph]);
                    }
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int ph = 0; ph < 3; ++ph) {
                    const char2 cl = at1(ub1[ph] + 1);
                    acc[2 * ph] += (double)cl.x * ti;
                    acc[2 * ph + 1] += (double)cl.x * tq;
                    if (pilot) {
                        acc[6 + 2 * ph] += (double)cl.y * ti;
                        acc[7 + 2 * ph] += (double)cl.y * tq;
                    }
                }
            }
        }
        if (MODE == BDS_TRACK_WB && pilot) {  // pilotBOC61(ceil(tcode*6)+1)  (WB_tracking.m:298,311,324)
            const int lo = lo6;
            auto at6 = [&](int i1) -> float {
                BDS_DASSERT(!use6 || (i1 - lo >= 0 && i1 - lo < kCap6));
                return use6 ? (float)s_t6[i1 - lo] : tab_at(prim_p, n6, i1);
            };
            const int nmax = max(ub6[0] - ua6[0], max(ub6[1] - ua6[1], ub6[2] - ua6[2]));
            for (int r = lane; r < nmax; r += 64) {
                int kk[3], uu[3];
                bool val[3], bad = false;
#pragma unroll
                for (int ph = 0; ph < 3; ++ph) {
                    uu[ph] = ua6[ph] + 1 + r;
                    val[ph] = uu[ph] <= ub6[ph];
                    const double thr = (double)(uu[ph] - 1);
                    int kc = (int)floor((thr * (1.0 / 6.0) - cv3[ph].a) * inv_inc) + 1;
                    kc = max(k0 + 1, min(kc, k1 - 1));
                    const bool good = !(code_arg<1>(cv3[ph], kc - 1) > thr) && code_arg<1>(cv3[ph], kc) > thr;
                    bad |= val[ph] && !good;
                    kk[ph] = val[ph] ? kc : k0 + 1;
                }
                if (bad) {
#pragma unroll
                    for (int ph = 0; ph < 3; ++ph)
                        if (val[ph]) kk[ph] = first_sample_of<1>(cv3[ph], inv_inc, uu[ph], k0, k1 - 1);
                }
#pragma unroll
                for (int ph = 0; ph < 3; ++ph) {
                    const double2 S = prefix(kk[ph]);
                    const int u = val[ph] ? uu[ph] : ua6[ph];
                    const double d6 = val[ph] ? (double)(at6(u + 1) - at6(u)) : 0.0;
                    acc[12 + 2 * ph] = fma(-d6, S.x, acc[12 + 2 * ph]);
                    acc[13 + 2 * ph] = fma(-d6, S.y, acc[13 + 2 * ph]);
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int ph = 0; ph < 3; ++ph) {
                    const double cl = (double)at6(ub6[ph] + 1);
                    acc[12 + 2 * ph] += cl * ti;
                    acc[13 + 2 * ph] += cl * tq;
                }
            }
        }
    }
    // workgroup reduction
    __syncthreads();
    double(*s_part)[kNSums] = reinterpret_cast<double(*)[kNSums]>(trk_lds);
#pragma unroll
    for (int i = 0; i < kNSums; ++i) {
        if (i >= 12 && MODE != BDS_TRACK_WB) {  // no BOC(6,1) correlators outside wide-band mode
            if (lane == 63) s_part[wave][i] = 0.0;
            continue;
        }
        const double v = wave_scan_incl(acc[i]);
        if (lane == 63) s_part[wave][i] = v;
    }
    __syncthreads();
    if (t < kNSums) {
        double v = 0;
        for (int w = 0; w < NW; ++w) v += s_part[w][t];
        sums[t] = v;
    }
}

// grid (nblocks, n_ch); part: [n_ch][nblocks][18]
template <int MODE>
__device__ __forceinline__ void apply_update(const TrkParams &p, ChanState &s, const double *__restrict__ part, int ch,
                                             int nblocks, int epoch, const TrkOut &o, bool store, unsigned char *scratch);

// One kernel per (tracker, correlator variant, record type): a kernel holding all variants ran out of SGPRs
// (150 spilled in wide-band mode, each a lane write + read on the vector unit).
// With `part_prev` the kernel first applies the loop update of the previous epoch: every workgroup of a channel
// recomputes it from that epoch's partial sums (fixed summation order: the same bits everywhere), so no workgroup has to
// wait for another and an epoch is one launch instead of two (the update as its own kernel costs ~5 us, mostly the
// floor of a small dependent launch).  State and partial sums ping-pong between two buffers; workgroup 0 of the channel
// writes the results of the previous epoch and the state the current one starts from.
template <int MODE, int SEG, int FMT, int PREC>
__global__ __launch_bounds__(kTrkThreads, 1) void k_trk_correlate(const int8_t *__restrict__ data,
                                                              const int8_t *__restrict__ prim, TrkParams p,
                                                              const ChanState *__restrict__ st_in, ChanState *__restrict__ st_out,
                                                              const double *__restrict__ part_prev, double *__restrict__ part,
                                                              int nblocks, int epoch, const TrkOut *__restrict__ op) {
    const int ch = blockIdx.y;
    ChanState s = st_in[ch];
    // (the table of result arrays comes by pointer: 21 pointers by value cost this kernel 40 SGPRs it does not have)
    if (part_prev && s.active == 1) {
        if constexpr (SEG > 0) {  // the update's scratch sits in the dynamic region the correlator takes over afterwards
            extern __shared__ __attribute__((aligned(16))) unsigned char trk_lds[];
            apply_update<MODE>(p, s, part_prev, ch, nblocks, epoch - 1, *op, blockIdx.x == 0, trk_lds);
        } else {
            __shared__ __attribute__((aligned(16))) unsigned char scratch[kUpdScratch];
            apply_update<MODE>(p, s, part_prev, ch, nblocks, epoch - 1, *op, blockIdx.x == 0, scratch);
        }
    }
    if (st_out != st_in && blockIdx.x == 0 && threadIdx.x == 0) st_out[ch] = s;  // the state this epoch runs with
    double *out = part + ((long)ch * nblocks + blockIdx.x) * kNSums;
    if (s.active != 1) return;
    const EpochGeom g = epoch_geom(s, p);
    const long k0 = (long)blockIdx.x * p.chunk;
    // beyond the block; short read (the update kernel stops the channel); outside the loaded window (it flags it)
    if (k0 >= g.blk || g.pos + g.blk > p.n_bytes || g.pos < p.base || g.pos + g.blk > p.win_end) {
        if (threadIdx.x < kNSums) out[threadIdx.x] = 0.0;
        return;
    }
    const int8_t *pd = prim + ((long)(s.prn - 1) * 2 + 0) * kTabStride;  // (data, pilot) pairs
    const int8_t *pp = prim + ((long)(s.prn - 1) * 2 + 1) * kTabStride;  // pilot BOC(6,1)
    if constexpr (SEG > 0)  // run-based correlator, SEG samples per lane and pass
        correlate_runs<MODE, SEG, FMT, PREC>(data, pd, pp, p, g, k0, (long)nblocks * p.chunk, p.pilot != 0, out);
    else  // per-sample correlator (reads p.cplx itself)
        correlate_slice<MODE>(data, pd, pp, p, g, k0, (long)nblocks * p.chunk, p.pilot != 0, out);
}

// Open-loop variant: geometry supplied by the caller (bds_track_correlate).
template <int MODE, int SEG, int FMT, int PREC>
__global__ __launch_bounds__(kTrkThreads) void k_trk_correlate_open(const int8_t *__restrict__ data,
                                                                   const int8_t *__restrict__ prim, TrkParams p,
                                                                   const int *__restrict__ prn,
                                                                   const double *__restrict__ state6,
                                                                   double *__restrict__ part, int nblocks) {
    const int ch = blockIdx.y;
    const double *s6 = state6 + (long)ch * 6;
    EpochGeom g;
    g.pos = (long long)s6[0];
    g.blk = (long)s6[1];
    g.rem = s6[2];
    g.step = s6[3] / p.fs;
    g.remCarr = s6[4];
    g.carrFreq = s6[5];
    double *out = part + ((long)ch * nblocks + blockIdx.x) * kNSums;
    const long k0 = (long)blockIdx.x * p.chunk;
    if (k0 >= g.blk || g.pos + g.blk > p.n_bytes || g.pos < 0) {
        if (threadIdx.x < kNSums) out[threadIdx.x] = 0.0;
        return;
    }
    const int8_t *pd = prim + ((long)(prn[ch] - 1) * 2 + 0) * kTabStride;  // (data, pilot) pairs
    const int8_t *pp = prim + ((long)(prn[ch] - 1) * 2 + 1) * kTabStride;  // pilot BOC(6,1)
    if constexpr (SEG > 0)  // run-based correlator, SEG samples per lane and pass
        correlate_runs<MODE, SEG, FMT, PREC>(data, pd, pp, p, g, k0, (long)nblocks * p.chunk, p.pilot != 0, out);
    else  // per-sample correlator (reads p.cplx itself)
        correlate_slice<MODE>(data, pd, pp, p, g, k0, (long)nblocks * p.chunk, p.pilot != 0, out);
}

// launch k<MODE, SEG, FMT, PREC> for the run-time (mode, runs, cplx, prec) of p; the f64 prefix sums of PREC >= 1 need
// more dynamic LDS than the default limit of a kernel: raised once per kernel and context
#define BDS_TRK_LAUNCH(KERN, grid, lds, stream, ...)                                                        \
    do {                                                                                                    \
        auto fire = [&](auto kern) {                                                                        \
            if ((lds) > 48 * 1024 && ctx->lds_attr_done.insert((const void *)kern).second)                  \
                (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds)); \
            hipLaunchKernelGGL(kern, grid, dim3(kTrkThreads), lds, stream, __VA_ARGS__);                    \
        };                                                                                                  \
        auto go = [&](auto mode_c, auto prec_c) {                                                           \
            constexpr int M = decltype(mode_c)::value, PR = decltype(prec_c)::value;                        \
            /* 16-bit records: the default numerics only (fill_params refuses the rest) */                  \
            if (fmt_16bit(p.cplx) && p.runs) {                                                              \
                if (p.runs == 16 && p.cplx == kFmtReal16) fire(KERN<M, 16, kFmtReal16, 4>);                 \
                else if (p.runs == 16) fire(KERN<M, 16, kFmtIQ16, 4>);                                      \
                else if (p.cplx == kFmtReal16) fire(KERN<M, 8, kFmtReal16, 4>);                             \
                else fire(KERN<M, 8, kFmtIQ16, 4>);                                                         \
            } else if (p.runs == 16 && p.cplx == kFmtReal) fire(KERN<M, 16, kFmtReal, PR>);                 \
            else if (p.runs == 16 && p.cplx == kFmtIQ) fire(KERN<M, 16, kFmtIQ, PR>);                       \
            else if (p.runs == 16) fire(KERN<M, 16, kFmtPacked, PR>);                                       \
            else if (p.runs == 8 && p.cplx == kFmtReal) fire(KERN<M, 8, kFmtReal, PR>);                     \
            else if (p.runs == 8 && p.cplx == kFmtIQ) fire(KERN<M, 8, kFmtIQ, PR>);                         \
            else if (p.runs == 8) fire(KERN<M, 8, kFmtPacked, PR>);                                         \
            else fire(KERN<M, 0, kFmtReal, 0>);                                                             \
        };                                                                                                  \
        auto gp = [&](auto mode_c) {                                                                        \
            if (p.prec == 0) go(mode_c, std::integral_constant<int, 0>{});                                  \
            else if (p.prec == 1) go(mode_c, std::integral_constant<int, 1>{});                             \
            else if (p.prec == 2) go(mode_c, std::integral_constant<int, 2>{});                             \
            else if (p.prec == 3) go(mode_c, std::integral_constant<int, 3>{});                             \
            else if (p.prec == 4) go(mode_c, std::integral_constant<int, 4>{});                             \
            else go(mode_c, std::integral_constant<int, 5>{});                                              \
        };                                                                                                  \
        if (p.mode == BDS_TRACK_B2A) gp(std::integral_constant<int, BDS_TRACK_B2A>{});                      \
        else if (p.mode == BDS_TRACK_NB) gp(std::integral_constant<int, BDS_TRACK_NB>{});                   \
        else gp(std::integral_constant<int, BDS_TRACK_WB>{});                                               \
    } while (0)

__global__ void k_trk_reduce_open(const double *__restrict__ part, int nblocks, double *__restrict__ sums) {
    const int ch = blockIdx.x;
    if (threadIdx.x < kNSums) {
        double v = 0;
        for (int b = 0; b < nblocks; ++b) v += part[((long)ch * nblocks + b) * kNSums + threadIdx.x];
        sums[(long)ch * kNSums + threadIdx.x] = v;
    }
}

// one workgroup per channel: kUpdGroups x 18 threads add up the correlate workgroups' partial sums,
// thread 0 then runs the loop filters
// Loop update of one channel, run by a whole workgroup (>= kUpdGroups * 18 threads): `s` is the state the epoch was
// correlated with, `part` that epoch's partial sums; every thread returns with the next state in `s`.  The result
// arrays of the epoch are written only if `store` (one workgroup per channel).
template <int MODE>
__device__ __forceinline__ void apply_update(const TrkParams &p, ChanState &s, const double *__restrict__ part, int ch,
                                             int nblocks, int epoch, const TrkOut &o, bool store, unsigned char *scratch) {
    // kUpdScratch bytes of LDS (the caller's: at the head of a correlate launch the region the correlator uses afterwards)
    double *s_sum = reinterpret_cast<double *>(scratch);                                     // [18]
    double(*s_grp)[kNSums] = reinterpret_cast<double(*)[kNSums]>(scratch + kNSums * 8);      // [kUpdGroups][18]
    double *s_x = reinterpret_cast<double *>(scratch + (1 + kUpdGroups) * kNSums * 8);       // [6]
    ChanState &s_next = *reinterpret_cast<ChanState *>(scratch + (1 + kUpdGroups) * kNSums * 8 + 48);
    const EpochGeom g = epoch_geom(s, p);
    // fixed-order two-level sum over the correlate workgroups (bit-stable from run to run): group j
    // takes workgroups j, j+14, ...; the 14 group sums are then added in order.  (A single thread per
    // sum walking all ~243 workgroups of a 10-ms epoch cost 60 us of dependent loads per epoch.)
    if (threadIdx.x < kUpdGroups * kNSums) {
        const int grp = threadIdx.x / kNSums, i = threadIdx.x - grp * kNSums;
        const long nb = min((long)nblocks, (g.blk + p.chunk - 1) / p.chunk);
        double v = 0;
        for (long b = grp; b < nb; b += kUpdGroups) v += part[((long)ch * nblocks + b) * kNSums + i];
        s_grp[grp][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < kNSums) {
        double v = 0;
#pragma unroll
        for (int j = 0; j < kUpdGroups; ++j) v += s_grp[j][threadIdx.x];
        s_sum[threadIdx.x] = v;
    }
    __syncthreads();
    const double two_pi = 6.283185307179586476925286766559;
    const double pi = 3.14159265358979323846;
    const double L = (double)p.code_len;
    const double I_E = s_sum[0], Q_E = s_sum[1], I_P = s_sum[2], Q_P = s_sum[3], I_L = s_sum[4], Q_L = s_sum[5];
    double pI_E = s_sum[6], pQ_E = s_sum[7], pI_P = s_sum[8], pQ_P = s_sum[9], pI_L = s_sum[10], pQ_L = s_sum[11];
    double cI_E = 0, cQ_E = 0, cI_P = 0, cQ_P = 0, cI_L = 0, cQ_L = 0;
    if (MODE == BDS_TRACK_WB && p.pilot) {  // QMBOC composite, WB_tracking.m:375-380
        const double a = sqrt(4.0 / 33), b = sqrt(29.0 / 33);
        cI_E = -a * s_sum[12] + b * pQ_E;
        cQ_E = -a * s_sum[13] - b * pI_E;
        cI_P = -a * s_sum[14] + b * pQ_P;
        cQ_P = -a * s_sum[15] - b * pI_P;
        cI_L = -a * s_sum[16] + b * pQ_L;
        cQ_L = -a * s_sum[17] - b * pI_L;
    }
    // The update is a chain of dependent f64 operations (two atan, up to six sqrt, an fmod, divisions: ~3 us on one
    // thread, and at the head of a correlate launch every workgroup waits for it).  Its independent pieces run on four
    // waves of the workgroup (different SIMDs), one lane each, with exactly the expressions of the serial form; thread 0
    // then combines them in the reference's order.
    // s_x: data atan, pilot atan, data (E-L)/(E+L), pilot (E-L)/(E+L), next code phase, next carrier phase
    if ((threadIdx.x & 63) == 0 && threadIdx.x < 256) {
        const int w = threadIdx.x >> 6;
        if (w == 0) {
            s_x[0] = atan(Q_P / I_P) / two_pi;  // :337 (true division: I = 0 -> +-pi/2, 0/0 -> NaN, as MATLAB)
        } else if (w == 1) {
            double cq = 0.0;
            if (p.pilot) {
                if (MODE == BDS_TRACK_B2A) {
                    // QI = (pI + j pQ) * exp(-j pi/2); atan(imag/real)  (:345-348)
                    const double cr = cos(-pi / 2), sr = sin(-pi / 2);  // exp(-1i*pi/2) as MATLAB evaluates it
                    const double re = pI_P * cr - pQ_P * sr, im = pI_P * sr + pQ_P * cr;
                    cq = atan(im / re) / two_pi;
                } else if (MODE == BDS_TRACK_NB) {
                    cq = atan(-pI_P / pQ_P) / two_pi;  // NB:357
                } else {
                    cq = atan(cQ_P / cI_P) / two_pi;  // WB:392
                }
            }
            s_x[1] = cq;
        } else if (w == 2) {
            const double eE = sqrt(I_E * I_E + Q_E * Q_E), eL = sqrt(I_L * I_L + Q_L * Q_L);
            s_x[2] = (eE - eL) / (eE + eL);  // :366
            double pce = 0.0;
            if (p.pilot) {
                double pE, pL;
                if (MODE == BDS_TRACK_WB) {
                    pE = sqrt(cI_E * cI_E + cQ_E * cQ_E);
                    pL = sqrt(cI_L * cI_L + cQ_L * cQ_L);
                } else {
                    pE = sqrt(pI_E * pI_E + pQ_E * pQ_E);
                    pL = sqrt(pI_L * pI_L + pQ_L * pQ_L);
                }
                pce = (pE - pL) / (pE + pL);
            }
            s_x[3] = pce;
        } else {
            // remCodePhase = tcode(blksize) + codePhaseStep - codeLength  (:295; B1C: tcode/2, WB:327)
            if (MODE == BDS_TRACK_B2A) {
                const double tp_last = g.rem + (double)(g.blk - 1) * g.step;
                s_x[4] = (tp_last + g.step) - L;
            } else {
                const double tp_last = g.rem * 2.0 + (double)(g.blk - 1) * (g.step * 2.0);
                s_x[4] = tp_last / 2 + g.step - L;
            }
            // remCarrPhase = rem(trigarg(blksize+1), 2*pi)  (:303-305)
            const double t_end = (double)g.blk / p.fs;
            const double trig_end = ((s.carrFreq * 2.0 * pi) * t_end) + s.remCarrPhase;
            s_x[5] = fmod(trig_end, two_pi);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        [&] {
    const long e = (long)ch * p.n_epochs + epoch;
    if (g.pos + g.blk <= p.n_bytes && (g.pos < p.base || g.pos + g.blk > p.win_end)) {
        // inside the file but outside the part of it that is held: nothing of this epoch is valid; the host repeats the
        // call with the whole record in HBM (one window) or the batch with a wider margin (streamed)
        s.active = -2;
        return;
    }
    if (store) o.absoluteSample[e] = (double)s.pos;  // tracking.m:226 (assigned before the read)
    if (g.pos + g.blk > p.n_bytes) {
        // short read: message + return in the reference (tracking.m:250-254); partial results stay
        s.active = 0;
        return;
    }
    if (store) o.remCodePhase[e] = s.remCodePhase;  // :258
    if (store) o.remCarrPhase[e] = s.remCarrPhase;  // :300
    const double rem_next = s_x[4], carr_next = s_x[5];
    // ---- PLL discriminator ----------------------------------------------------------------------
    double carrError = s_x[0];
    if (p.pilot) {
        const double cq = s_x[1];
        if (MODE == BDS_TRACK_B2A)
            carrError = (carrError + cq) / 2;  // :352
        else if (MODE == BDS_TRACK_NB)
            carrError = (carrError * 11 + cq * 29) / 40;  // NB:360
        else
            carrError = (carrError * 1 + cq * 3) / 4;  // WB:395
    }
    s.d2CarrError = s.d2CarrError + carrError * p.pf3;                    // :356
    s.dCarrError = s.d2CarrError + carrError * p.pf2 + s.dCarrError;      // :357
    const double carrNco = s.dCarrError + carrError * p.pf1;              // :358
    if (store) o.carrFreq[e] = s.carrFreq;                                           // :361
    // ---- DLL discriminator ---------------------------------------------------------------------
    double codeError = s_x[2];  // :366
    if (MODE != BDS_TRACK_B2A) codeError = codeError * (1 - p.spacing);  // WB:409-410
    if (p.pilot) {
        const double pce = s_x[3];
        if (MODE == BDS_TRACK_B2A)
            codeError = (codeError + pce) / 2;  // :377
        else if (MODE == BDS_TRACK_NB)
            codeError = (codeError * 11 + pce * (1 - p.spacing) * 29) / 40;  // NB:381-384
        else
            codeError = codeError * p.factor + pce * (1 - p.spacing) * (1 - p.factor);  // WB:418
    }
    const double codeNco = s.oldCodeNco + (p.tau2 / p.tau1) * (codeError - s.oldCodeError) + codeError * (p.pdi / p.tau1);  // :381
    s.oldCodeNco = codeNco;
    s.oldCodeError = codeError;
    if (store) o.codeFreq[e] = s.codeFreq;  // :387
    if (store) o.dllDiscr[e] = codeError;
    if (store) o.dllDiscrFilt[e] = codeNco;
    if (store) o.pllDiscr[e] = carrError;
    if (store) o.pllDiscrFilt[e] = carrNco;
    if (store) o.I_E[e] = I_E;
    if (store) o.I_P[e] = I_P;
    if (store) o.I_L[e] = I_L;
    if (store) o.Q_E[e] = Q_E;
    if (store) o.Q_P[e] = Q_P;
    if (store) o.Q_L[e] = Q_L;
    if (p.pilot) {
        if (MODE == BDS_TRACK_WB) {
            if (store) o.Pilot_I_E[e] = cI_E;
            if (store) o.Pilot_Q_E[e] = cQ_E;
            if (store) o.Pilot_I_P[e] = cI_P;
            if (store) o.Pilot_Q_P[e] = cQ_P;
            if (store) o.Pilot_I_L[e] = cI_L;
            if (store) o.Pilot_Q_L[e] = cQ_L;
        } else {
            if (store) o.Pilot_I_P[e] = pI_P;
            if (store) o.Pilot_Q_P[e] = pQ_P;
        }
    }
    s.carrFreq = s.carrFreqBasis + carrNco;   // :363
    s.codeFreq = s.codeFreqBasis - codeNco;   // :389
    s.remCodePhase = rem_next;
    s.remCarrPhase = carr_next;
    s.pos += g.blk;
    s.completed = epoch + 1;
    // A code NCO that is not a positive finite number (an epoch of all-zero samples: atan(0/0), 0/0 in the DLL) has no next
    // block: MATLAB stops in fread.  The epoch's results stand as computed (NaN discriminators); the channel stops as at
    // a short read, so no later launch or host plan derives a block length from this state.
    if (!(isfinite(s.codeFreq) && isfinite(s.remCodePhase) && s.codeFreq > 0)) s.active = 0;
        }();
        s_next = s;
    }
    __syncthreads();
    s = s_next;
    __syncthreads();  // the scratch may be reused from here on
}

template <int MODE>
__global__ __launch_bounds__(kUpdThreads) void k_trk_update(TrkParams p, ChanState *__restrict__ st,
                                                   const double *__restrict__ part, int nblocks, int epoch,
                                                   TrkOut o) {
    const int ch = blockIdx.x;
    __shared__ __attribute__((aligned(16))) unsigned char scratch[kUpdScratch];
    ChanState s = st[ch];
    if (s.active != 1) return;
    apply_update<MODE>(p, s, part, ch, nblocks, epoch, o, true, scratch);
    if (threadIdx.x == 0) st[ch] = s;
}

// The two buffers the resident span of a streamed record slides through, `cap` bytes each (+ kDataSlack).  Owned by the context's
// TrackState (the one-shot call: kept from call to call while the size stays) or by a session.
struct SpanPair {
    int8_t *buf[2] = {nullptr, nullptr};
    size_t cap = 0;
    void release() {
        for (int8_t *&q : buf)
            if (q) (void)hipFree(q), q = nullptr;
        cap = 0;
    }
    int ensure(bds_ctx *ctx, size_t bytes) {
        if (cap == bytes && buf[0] && buf[1]) return BDS_OK;
        release();
        for (int8_t *&q : buf) {
            const hipError_t e = hipMalloc((void **)&q, bytes + kDataSlack);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                q = nullptr;
                return fail(ctx, BDS_ERR_NOMEM, "resident span of 2 x %zu bytes of the IF record does not fit in HBM: %s", bytes, hipGetErrorString(e));
            }
        }
        cap = bytes;
        return BDS_OK;
    }
};

struct TrackState {
    int8_t *d_data = nullptr;
    size_t data_cap = 0;
    size_t loaded_bytes = 0;  // bytes of the record the last call copied host-to-device (diagnostics)
    int8_t *d_prim = nullptr;
    int prim_signal = 0;
    SpanPair span;              // streamed mode
    size_t resident_limit = 0;  // bds_track_set_resident_limit (0: none)
    // bds_track_stream_info of the last call
    int pieces = 0;           // loads of a part of the record (1: one window)
    size_t resident_max = 0;  // most bytes of the record resident at a time
    int repeated = 0;         // batches run again after the window guard fired
    // the open tracking session of the context (at most one): it owns its channel states, launch geometry, span buffers and
    // C/N0 carry, and counts its pieces / repeated batches in the three fields above from bds_track_open* on
    bds_track_session *session = nullptr;
};

static void session_close(bds_track_session *h);

void track_state_free(TrackState *t) {
    if (!t) return;
    if (t->session) session_close(t->session);
    if (t->d_data) (void)hipFree(t->d_data);
    t->span.release();
    if (t->d_prim) (void)hipFree(t->d_prim);
    delete t;
}

static hipStream_t st(bds_ctx *ctx) { return (hipStream_t)ctx->stream; }

static int track_mode(const bds_settings &s) {
    if (s.signal == BDS_SIGNAL_B2A) return BDS_TRACK_B2A;
    return s.pilotTRKflag == 2 ? BDS_TRACK_WB : BDS_TRACK_NB;  // B1C/postProcessing.m:137-143
}

static int pilot_on(const bds_settings &s, int mode) {
    if (mode == BDS_TRACK_WB) return s.pilotTRKflag == 2;
    return s.pilotTRKflag == 1;  // tracking.m:70, NB_tracking.m:78
}

static int ensure_prim(bds_ctx *ctx, TrackState &t, int signal) {
    if (t.d_prim && t.prim_signal == signal) return BDS_OK;
    // per PRN two slots: (data, pilot) pairs at the code's own resolution, and the pilot BOC(6,1)
    // array; wrapped padding on both sides (tab_at / tab2_at)
    const size_t bytes = (size_t)BDS_MAX_PRN * 2 * kTabStride;
    if (!t.d_prim) BDS_HIP(ctx, hipMalloc((void **)&t.d_prim, bytes));
    std::vector<int8_t> tab(bytes, 0);
    int8_t prim[2][10230];
    for (int prn = 1; prn <= BDS_MAX_PRN; ++prn) {
        gen_primary(signal, false, prn, prim[0]);
        gen_primary(signal, true, prn, prim[1]);
        auto unit = [&](int comp, int units, long j) {  // value at padded position j of a `units`-per-chip array
            const long n = 10230L * units;
            long u = (j - kTabPad) % n;
            if (u < 0) u += n;
            const int8_t chip = prim[comp][u / units];
            const long sub = u % units;  // BOC(1,1): [-c, +c]; BOC(6,1): (-1)^ii c, ii = sub + 1
            return units == 1 ? chip : ((sub & 1) ? chip : (int8_t)-chip);
        };
        const int units = signal == BDS_SIGNAL_B1C ? 2 : 1;
        int8_t *dp = &tab[((size_t)(prn - 1) * 2 + 0) * kTabStride];
        for (long j = 0; j < 10230L * units + 2 * kTabPad; ++j) {
            dp[2 * j] = unit(0, units, j);
            dp[2 * j + 1] = unit(1, units, j);
        }
        if (signal == BDS_SIGNAL_B1C) {
            int8_t *b6 = &tab[((size_t)(prn - 1) * 2 + 1) * kTabStride];
            for (long j = 0; j < 10230L * 12 + 2 * kTabPad; ++j) b6[j] = unit(1, 12, j);
        }
    }
    BDS_HIP(ctx, hipMemcpy(t.d_prim, tab.data(), bytes, hipMemcpyHostToDevice));
    t.prim_signal = signal;
    return BDS_OK;
}

static int fill_params(bds_ctx *ctx, const bds_settings &s, TrkParams &p, int n_epochs, size_t n_bytes) {
    if (s.signal != BDS_SIGNAL_B1C && s.signal != BDS_SIGNAL_B2A) return fail(ctx, BDS_ERR_ARG, "settings.signal invalid");
    if (s.fileType != 1 && s.fileType != 2 && s.fileType != 3)
        return fail(ctx, BDS_ERR_ARG, "settings.fileType must be 1 (real), 2 (I/Q) or 3 (packed 2+2-bit I/Q)");
    if (s.dataType != 0 && s.dataType != 1)  // fread(fid, ..., settings.dataType), tracking.m:237-238
        return fail(ctx, BDS_ERR_UNSUPPORTED, "settings.dataType: only 'schar' (0: int8 samples) and 'int16' (1) are supported");
    if (s.dataType == 1 && s.fileType == 3)
        return fail(ctx, BDS_ERR_ARG, "settings.fileType 3 (packed 2+2-bit I/Q) has no 16-bit form: settings.dataType must be 'schar' (0)");
    if (s.codeLength != 10230 || !(s.samplingFreq > 0) || !(s.intTime > 0))
        return fail(ctx, BDS_ERR_ARG, "settings.codeLength/samplingFreq/intTime invalid");
    p.mode = track_mode(s);
    p.pilot = pilot_on(s, p.mode);
    p.code_len = s.codeLength;
    p.n_epochs = n_epochs;
    p.fs = s.samplingFreq;
    p.inv_fs = 1.0 / s.samplingFreq;
    p.spacing = s.dllCorrelatorSpacing;
    bds_calc_loop_coef(s.dllNoiseBandwidth, s.dllDampingRatio, 1.0, &p.tau1, &p.tau2);  // tracking.m:110-112
    bds_calc_loop_coef_carr(&s, &p.pf3, &p.pf2, &p.pf1);                                 // :116
    p.pdi = s.intTime;                                                                   // :107
    p.factor = p.mode == BDS_TRACK_WB ? bds_calc_weighing_factor(&s) : 0.0;              // WB_tracking.m:138
    p.cplx = s.fileType == 3 ? kFmtPacked : s.dataType == 1 ? (s.fileType == 2 ? kFmtIQ16 : kFmtReal16) : s.fileType == 2 ? kFmtIQ : kFmtReal;
    if (ctx->tune.trk_persample) {  // per-sample correlator (the round-1 kernel; A/B and cross-check)
        p.chunk = s.signal == BDS_SIGNAL_B2A ? 2048 : 8192;
        if (ctx->tune.trk_chunk > 0) p.chunk = std::max(256, ctx->tune.trk_chunk);
        p.runs = 0;
    } else {  // run-based correlator: 8 or 16 consecutive samples per thread
        p.runs = s.signal == BDS_SIGNAL_B2A ? 8 : 16;
        if (ctx->tune.trk_chunk == 2048) p.runs = 8;
        if (ctx->tune.trk_chunk == 4096) p.runs = 16;
        p.chunk = kTrkThreads * p.runs;
        p.prec = std::max(0, std::min(5, ctx->tune.trk_prec));
        if (ctx->tune.trk_seg == 8 || ctx->tune.trk_seg == 16) p.runs = ctx->tune.trk_seg, p.chunk = kTrkThreads * p.runs;
    }
    if (fmt_16bit(p.cplx)) {
        // the run-based correlator is built for 16-bit records in the default numerics only (the per-sample one decodes at run time)
        if (p.runs && p.prec != 4)
            return fail(ctx, BDS_ERR_UNSUPPORTED, "BDS_TRK_PREC=%d with settings.dataType 'int16': the tracking kernels for 16-bit records are "
                        "built for the default numerics (BDS_TRK_PREC=4) only", p.prec);
        if (n_bytes % (size_t)fmt_bps(p.cplx))
            return fail(ctx, BDS_ERR_ARG, "settings.dataType 'int16': the record's %zu bytes are not a whole number of %s", n_bytes,
                        p.cplx == kFmtIQ16 ? "I/Q int16 pairs (4 bytes each)" : "int16 samples (2 bytes each)");
    }
    // whole samples an fread can deliver
    p.n_bytes = fmt_samples(p.cplx, (long long)n_bytes);
    return BDS_OK;
}

template <class F>
static void for_each_field(bds_track_out *o, TrkOut *d, F f) {
    f(o->absoluteSample, d->absoluteSample, 0.0);
    f(o->codeFreq, d->codeFreq, INFINITY);
    f(o->carrFreq, d->carrFreq, INFINITY);
    f(o->I_P, d->I_P, 0.0);
    f(o->I_E, d->I_E, 0.0);
    f(o->I_L, d->I_L, 0.0);
    f(o->Q_E, d->Q_E, 0.0);
    f(o->Q_P, d->Q_P, 0.0);
    f(o->Q_L, d->Q_L, 0.0);
    f(o->Pilot_I_P, d->Pilot_I_P, 0.0);
    f(o->Pilot_Q_P, d->Pilot_Q_P, 0.0);
    f(o->Pilot_I_E, d->Pilot_I_E, 0.0);
    f(o->Pilot_I_L, d->Pilot_I_L, 0.0);
    f(o->Pilot_Q_E, d->Pilot_Q_E, 0.0);
    f(o->Pilot_Q_L, d->Pilot_Q_L, 0.0);
    f(o->dllDiscr, d->dllDiscr, INFINITY);
    f(o->dllDiscrFilt, d->dllDiscrFilt, INFINITY);
    f(o->pllDiscr, d->pllDiscr, INFINITY);
    f(o->pllDiscrFilt, d->pllDiscrFilt, INFINITY);
    f(o->remCodePhase, d->remCodePhase, INFINITY);
    f(o->remCarrPhase, d->remCarrPhase, INFINITY);
}

// include/Calc_CNo_PLD.m (B1C :45-114, B2a :38-100) over prompt values [k-M, k)
__device__ static void cno_pld_one(const double *I, const double *Q, int M, double T, double *lin, double *cno, double *pld) {
    double zm = 0;
    for (int i = 0; i < M; ++i) zm += I[i] * I[i] + Q[i] * Q[i];
    zm /= M;
    double zv = 0;
    for (int i = 0; i < M; ++i) {
        const double z = I[i] * I[i] + Q[i] * Q[i];
        zv += (z - zm) * (z - zm);
    }
    zv /= (M - 1);  // var(): N-1
    const double d = zm * zm - zv;
    if (d < 0) {
        // MATLAB's sqrt of a negative number is complex: Pav = j s, Nv = 0.5 (Zm - j s), and the abs() of B2a :58 / B1C :65 is
        // there for this case: |(1/T) j s / (Zm - j s)| = ((1/T) s) / |Zm - j s| -- finite, where a real sqrt gives NaN.
        // (Noise-only prompts take this branch in 37-47 % of their intervals.)
        const double s = sqrt(-d);
        *lin = ((1 / T) * s) / hypot(zm, s);
    } else {  // (a NaN d comes here and stays NaN)
        const double pav = sqrt(d);
        const double nv = 0.5 * (zm - pav);
        *lin = fabs((1 / T) * pav / (2 * nv));
    }
    *cno = 10 * log10(*lin);
    double sp = 0, sn = 0, sq = 0;
    for (int i = 0; i < M; ++i) {
        if (I[i] > 0) sp += I[i];
        if (I[i] < 0) sn += I[i];
        sq += Q[i];
    }
    const double a = (sp - sn) * (sp - sn);
    *pld = (a - sq * sq) / (a + sq * sq);
}

// C/N0 + phase-lock detector of every finished CNoInterval (tracking.m:411-434), on the device arrays the
// tracking loop just wrote: one workgroup per channel, one thread per interval, then the reference's
// two-point smoothing CNo = new/2 + previous/2 (:420-421; previous = 0 before the first interval).
// cno5: [5][n_ch][n_cno] = DataCNo, DataPLD, PilotCNo, PilotPLD, SigCNo; pm: 0 no pilot, 1 pilot with
// I/Q swapped (narrow-band, Calc_CNo_PLD.m:84-87), 2 pilot as is (wide-band).
__global__ __launch_bounds__(256) void k_trk_cno(TrkOut o, const ChanState *__restrict__ st, int n_epochs, int M,
                                                 int n_cno, int pm, double T, double *__restrict__ raw3,
                                                 double *__restrict__ cno5) {
    const int ch = blockIdx.x, n_ch = gridDim.x;
    const int done = st[ch].prn ? st[ch].completed : 0;
    const size_t plane = (size_t)n_ch * n_cno;
    double *r = raw3 + (size_t)ch * n_cno * 3;
    for (int q = threadIdx.x; q < n_cno; q += blockDim.x) {
        const size_t e = (size_t)ch * n_cno + q;
        for (int f = 0; f < 5; ++f) cno5[f * plane + e] = 0;
        r[q * 3 + 0] = r[q * 3 + 1] = r[q * 3 + 2] = 0;
        if ((q + 1) * M > done) continue;
        const size_t o0 = (size_t)ch * n_epochs + (size_t)q * M;
        double dlin, dcno, dpld, plin = 0, pcno = 0, ppld = 0;
        cno_pld_one(o.I_P + o0, o.Q_P + o0, M, T, &dlin, &dcno, &dpld);
        if (pm == 2)
            cno_pld_one(o.Pilot_I_P + o0, o.Pilot_Q_P + o0, M, T, &plin, &pcno, &ppld);
        else if (pm == 1)
            cno_pld_one(o.Pilot_Q_P + o0, o.Pilot_I_P + o0, M, T, &plin, &pcno, &ppld);
        r[q * 3 + 0] = dcno;
        r[q * 3 + 1] = pcno;
        r[q * 3 + 2] = 10 * log10(dlin + plin);
        cno5[1 * plane + e] = dpld;
        if (pm) cno5[3 * plane + e] = ppld;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < n_cno; q += blockDim.x) {
        if ((q + 1) * M > done) continue;
        const size_t e = (size_t)ch * n_cno + q;
        const double p0 = q ? r[(q - 1) * 3 + 0] : 0.0, p1 = q ? r[(q - 1) * 3 + 1] : 0.0, p2 = q ? r[(q - 1) * 3 + 2] : 0.0;
        cno5[0 * plane + e] = r[q * 3 + 0] * 0.5 + p0 * 0.5;
        if (pm) {
            cno5[2 * plane + e] = r[q * 3 + 1] * 0.5 + p1 * 0.5;
            cno5[4 * plane + e] = r[q * 3 + 2] * 0.5 + p2 * 0.5;
        }
    }
}

// The same post-pass for ONE bds_track_advance of a session.  The call's arrays hold the `done` epochs the channel ran in this
// call, and an interval may have begun in an earlier one, so the session keeps per channel
//   carry   [4][M] = I_P, Q_P, Pilot_I_P, Pilot_Q_P of the unfinished interval (n_carry < M epochs each)
//   prev3   the three raw values of the last finished interval, for the smoothing (0 before the first)
// Interval q of the call (q < nd = (n_carry + done) / M) covers entries [q M, (q + 1) M) of the carried prompts followed by this
// call's, in epoch order: the first is completed in the carry rows and evaluated there, the others lie whole in the call's
// arrays -- cno_pld_one sees the M values k_trk_cno gives it in the one-shot call, in the same order, and the smoothing is
// the same expression, so the values are the same bits.  What is left over becomes the new carry.
__global__ __launch_bounds__(256) void k_trk_cno_seg(TrkOut o, const ChanState *__restrict__ st, int n_epochs, int M, int n_cno,
                                                     int pm, double T, double *__restrict__ carry, int *__restrict__ n_carry,
                                                     double *__restrict__ prev3, double *__restrict__ raw3,
                                                     double *__restrict__ cno5) {
    const int ch = blockIdx.x, n_ch = gridDim.x;
    const int done = st[ch].prn ? st[ch].completed : 0;
    const int nc = n_carry[ch];
    const int nd = min((nc + done) / M, n_cno);  // (the host sized n_cno for every interval that can complete)
    const size_t plane = (size_t)n_ch * n_cno, row = (size_t)ch * n_epochs;
    double *cr = carry + (size_t)ch * 4 * M;
    const double *src[4] = {o.I_P + row, o.Q_P + row, o.Pilot_I_P + row, o.Pilot_Q_P + row};
    double *r = raw3 + (size_t)ch * n_cno * 3;
    double *p3 = prev3 + (size_t)ch * 3;
    for (int q = threadIdx.x; q < n_cno; q += blockDim.x)
        for (int f = 0; f < 5; ++f) cno5[f * plane + (size_t)ch * n_cno + q] = 0;
    const int fill = min(M - nc, nd > 0 ? M - nc : done);  // this call's epochs that belong to the carried interval
    for (int i = threadIdx.x; i < fill; i += blockDim.x)
        for (int f = 0; f < 4; ++f) cr[f * M + nc + i] = src[f][i];
    __syncthreads();
    for (int q = threadIdx.x; q < nd; q += blockDim.x) {
        const size_t e = (size_t)ch * n_cno + q;
        const int o0 = q * M - nc;  // (q > 0)
        const double *I = q ? src[0] + o0 : cr, *Q = q ? src[1] + o0 : cr + M;
        const double *PI = q ? src[2] + o0 : cr + 2 * M, *PQ = q ? src[3] + o0 : cr + 3 * M;
        double dlin, dcno, dpld, plin = 0, pcno = 0, ppld = 0;
        cno_pld_one(I, Q, M, T, &dlin, &dcno, &dpld);
        if (pm == 2)
            cno_pld_one(PI, PQ, M, T, &plin, &pcno, &ppld);
        else if (pm == 1)
            cno_pld_one(PQ, PI, M, T, &plin, &pcno, &ppld);
        r[q * 3 + 0] = dcno;
        r[q * 3 + 1] = pcno;
        r[q * 3 + 2] = 10 * log10(dlin + plin);
        cno5[1 * plane + e] = dpld;
        if (pm) cno5[3 * plane + e] = ppld;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < nd; q += blockDim.x) {
        const size_t e = (size_t)ch * n_cno + q;
        const double p0 = q ? r[(q - 1) * 3 + 0] : p3[0], p1 = q ? r[(q - 1) * 3 + 1] : p3[1], p2 = q ? r[(q - 1) * 3 + 2] : p3[2];
        cno5[0 * plane + e] = r[q * 3 + 0] * 0.5 + p0 * 0.5;
        if (pm) {
            cno5[2 * plane + e] = r[q * 3 + 1] * 0.5 + p1 * 0.5;
            cno5[4 * plane + e] = r[q * 3 + 2] * 0.5 + p2 * 0.5;
        }
    }
    __syncthreads();
    if (nd > 0) {
        const int left = nc + done - nd * M, o0 = nd * M - nc;
        for (int i = threadIdx.x; i < left && i < M; i += blockDim.x)
            for (int f = 0; f < 4; ++f) cr[f * M + i] = src[f][o0 + i];
        if (threadIdx.x == 0) {
            p3[0] = r[(nd - 1) * 3 + 0], p3[1] = r[(nd - 1) * 3 + 1], p3[2] = r[(nd - 1) * 3 + 2];
            n_carry[ch] = min(left, M - 1);
        }
    } else if (threadIdx.x == 0) {
        n_carry[ch] = min(nc + done, M - 1);
    }
}

// the result arrays of a call, one block of n_fields x n doubles, back to the reference's template values
// (tracking.m:48-82): Inf where bit f of inf_mask is set, else 0
__global__ void k_trk_fill_out(double *__restrict__ a, size_t n, int n_fields, uint32_t inf_mask) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * n_fields) return;
    a[i] = ((inf_mask >> (int)(i / n)) & 1u) ? INFINITY : 0.0;
}

// The 21 result arrays of a tracking call on the device: one block [21][n_ch][row] in the order of for_each_field, the table of
// its arrays for the kernels (by value: d; in device memory: d_out) and the fields whose template value is Inf.  A session keeps
// one for its lifetime, the one-shot call makes one per call.
struct TrkResults {
    static constexpr int kFields = sizeof(TrkOut) / sizeof(double *);
    double *d_fields = nullptr;
    size_t cap = 0;  // doubles at d_fields
    TrkOut d{};
    TrkOut *d_out = nullptr;
    int n_ch = 0, row = 0;  // the shape the table was made for
    uint32_t inf_mask = 0;
    std::vector<double> h;  // host copy of the block (fetch)

    TrkResults() = default;
    TrkResults(const TrkResults &) = delete;
    TrkResults &operator=(const TrkResults &) = delete;
    ~TrkResults() { release(); }
    void release() {
        if (d_fields) (void)hipFree(d_fields), d_fields = nullptr;
        if (d_out) (void)hipFree(d_out), d_out = nullptr;
        cap = 0, row = 0;
    }
    size_t n() const { return (size_t)n_ch * row; }
    // arrays of nc x r doubles at the template values, enqueued on the context's stream: the block grows when it has to, the
    // table is made again when the shape changes
    int prepare(bds_ctx *ctx, int nc, int r) {
        hipStream_t stream = (hipStream_t)ctx->stream;
        const size_t want = (size_t)nc * r * kFields;
        if (cap < want) {
            if (d_fields) (void)hipFree(d_fields), d_fields = nullptr, cap = 0;
            row = 0;
            const hipError_t e = hipMalloc((void **)&d_fields, sizeof(double) * want);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                d_fields = nullptr;
                return fail(ctx, BDS_ERR_NOMEM, "hipMalloc track output: %s", hipGetErrorString(e));
            }
            cap = want;
        }
        if (!d_out) BDS_HIP(ctx, hipMalloc((void **)&d_out, sizeof(TrkOut)));
        if (row != r || n_ch != nc) {
            n_ch = nc, row = r, inf_mask = 0;
            int f = 0;
            bds_track_out unused{};
            for_each_field(&unused, &d, [&](double *, double *&dev, double v0) {
                dev = d_fields + (size_t)f * n();
                if (v0 != 0.0) inf_mask |= 1u << f;
                ++f;
            });
            BDS_HIP(ctx, hipMemcpyAsync(d_out, &d, sizeof(TrkOut), hipMemcpyHostToDevice, stream));
            BDS_HIP(ctx, hipStreamSynchronize(stream));  // (d may not change while the copy reads it)
        }
        hipLaunchKernelGGL(k_trk_fill_out, dim3((unsigned)((want + 255) / 256)), dim3(256), 0, stream, d_fields, n(), kFields, inf_mask);
        return BDS_OK;
    }
    // the block to the host in one copy, then each array the caller supplied
    int fetch(bds_ctx *ctx, bds_track_out *out) {
        hipStream_t stream = (hipStream_t)ctx->stream;
        h.resize(n() * kFields);
        BDS_HIP(ctx, hipMemcpyAsync(h.data(), d_fields, sizeof(double) * h.size(), hipMemcpyDeviceToHost, stream));
        BDS_HIP(ctx, hipStreamSynchronize(stream));
        int f = 0;
        TrkOut unused{};
        for_each_field(out, &unused, [&](double *host, double *&, double) {
            if (host) memcpy(host, h.data() + (size_t)f * n(), sizeof(double) * n());
            ++f;
        });
        return BDS_OK;
    }
};

// The five C/N0 planes [5][n_ch][nq] at d_cno (k_trk_cno, k_trk_cno_seg; NULL: no interval was evaluated) into those of DataCNo,
// DataPLD, PilotCNo, PilotPLD, SigCNo the caller supplied (rows of out->n_cno): the first count(c) intervals of channel c, zero
// behind them and in the pilot planes of a channel tracked without pilot (pm == 0).
template <class F>
static int cno_scatter(bds_ctx *ctx, const double *d_cno, int n_ch, int nq, int pm, bds_track_out *out, F count) {
    hipStream_t stream = (hipStream_t)ctx->stream;
    std::vector<double> h((size_t)n_ch * nq * 5);
    if (d_cno) {
        BDS_HIP(ctx, hipMemcpyAsync(h.data(), d_cno, sizeof(double) * h.size(), hipMemcpyDeviceToHost, stream));
        BDS_HIP(ctx, hipStreamSynchronize(stream));
    }
    double *dst[5] = {out->DataCNo, out->DataPLD, out->PilotCNo, out->PilotPLD, out->SigCNo};
    const size_t plane = (size_t)n_ch * nq;
    for (int c = 0; c < n_ch; ++c) {
        const int nd = d_cno ? std::min(count(c), nq) : 0;
        for (int f = 0; f < 5; ++f) {
            if (!dst[f]) continue;
            for (int q = 0; q < out->n_cno; ++q)
                dst[f][(size_t)c * out->n_cno + q] = q < nd && (pm || f < 2) ? h[f * plane + (size_t)c * nq + q] : 0.0;
        }
    }
    return BDS_OK;
}

// Streamed tracking: the resident span of the record and the one being prepared (do_track plans the batches).
//   cur  the span the epochs of the current batch read, on the context's main stream
//   nxt  the span in preparation: its tail [pre_lo, pre_hi) is loaded by a host thread on the second stream while the batch
//        runs (start_load .. join); at the batch boundary move_to() copies what it shares with cur in front of that tail,
//        device-to-device on the main stream, and the two change places
// Who may touch a buffer when (the two streams are non-blocking: nothing orders them but what is written here):
//   * the loader's writes into nxt are complete before the main stream reads them: the thread synchronises its stream, and the
//     host joins it before move_to();
//   * after the exchange the OLD cur is nxt, and the main stream may still be reading it -- the carry copy just enqueued (the
//     kernels of earlier batches are done: the host synchronises the main stream at every batch end).  The next load writes
//     into that buffer, so move_to() records ev_carry behind the copy and the loader's stream waits for it before its first byte;
//   * loads that move_to() issues itself are on the main stream, behind the copy.
// Between start_load() and join() the loader may set the context's error message (the RecordSource reports its own failures):
// the main thread must not call fail() in that interval -- it keeps error codes in locals and reports them after join().
struct SpanStream {
    struct Span {  // samples [base, end) of the record at buf
        int8_t *buf = nullptr;
        long long base = 0, end = 0;
    } cur, nxt;
    bds_ctx *ctx;
    TrackState &t;
    const RecordSource &src;  // loaded from by one thread at a time: join() comes before every load of the main thread's
    hipStream_t main_stream, ld_stream;
    int fmt;            // sample format (kFmt*): span bounds are multiples of fmt_align(fmt) or even, so they fall on whole bytes
    long long span_n;   // samples a span buffer holds
    long long nb_of(long long n) const { return fmt_bytes(fmt, n); }  // bytes of n samples
    hipEvent_t ev_carry = nullptr;
    bool carry_pending = false;  // ev_carry is recorded behind a copy that reads nxt.buf
    // the prediction: the next span starts at sample pre_nb, its tail [pre_lo, pre_hi) goes behind what it shares with cur
    bool pre_valid = false;
    long long pre_nb = 0, pre_lo = 0, pre_hi = 0;
    std::thread th;
    int th_rc = BDS_OK;
    hipError_t th_err = hipSuccess;

    SpanStream(bds_ctx *c, TrackState &ts, const RecordSource &l, hipStream_t ms, hipStream_t ls, int fm, long long sn)
        : ctx(c), t(ts), src(l), main_stream(ms), ld_stream(ls), fmt(fm), span_n(sn) {}
    SpanStream(const SpanStream &) = delete;
    SpanStream &operator=(const SpanStream &) = delete;
    ~SpanStream() {
        if (th.joinable()) th.join();
        if (ev_carry) (void)hipEventDestroy(ev_carry);
    }
    // nxt becomes the span that starts at sample nb: what it shares with cur is carried device-to-device, the rest up to hi
    // is loaded here (main stream) unless the loader thread has put it there already; then the two change places
    int move_to(long long nb, long long hi, bool tail_loaded) {
        const bool carry = nb >= cur.base && nb < cur.end;
        if (carry) {
            if (!ev_carry) BDS_HIP(ctx, hipEventCreateWithFlags(&ev_carry, hipEventDisableTiming));
            BDS_HIP(ctx, hipMemcpyAsync(nxt.buf, cur.buf + nb_of(nb - cur.base), (size_t)nb_of(cur.end - nb), hipMemcpyDeviceToDevice, main_stream));
            BDS_HIP(ctx, hipEventRecord(ev_carry, main_stream));
            carry_pending = true;
        }
        const long long from = carry ? cur.end : nb;
        if (!tail_loaded && hi > from) {
            const size_t nbytes = (size_t)nb_of(hi - from);
            int r = src.load((size_t)nb_of(from), nbytes, nxt.buf + nb_of(from - nb), main_stream);
            if (r) return r;
            t.loaded_bytes += nbytes, t.pieces += 1;
        }
        nxt.base = nb, nxt.end = std::max(hi, from);
        t.resident_max = std::max(t.resident_max, (size_t)nb_of(cur.end - cur.base + nxt.end - nxt.base));
        std::swap(cur, nxt);
        pre_valid = false;
        return BDS_OK;
    }
    void predict(long long nb, long long hi) { pre_nb = nb, pre_lo = cur.end, pre_hi = hi, pre_valid = true; }
    // the predicted tail, on the loader's stream beside the batch just enqueued (nothing to do when a prediction kept over a
    // repeated batch is loaded already).  The bytes are counted when they are copied: a prediction that is discarded later
    // (the channels are not where it put them) is loaded, and counted, again by move_to().
    void start_load() {
        if (!pre_valid || th.joinable() || pre_lo >= pre_hi) return;
        int8_t *dst = nxt.buf + nb_of(pre_lo - pre_nb);
        const size_t off = (size_t)nb_of(pre_lo), nbytes = (size_t)nb_of(pre_hi - pre_lo);
        pre_lo = pre_hi;
        t.resident_max = std::max(t.resident_max, (size_t)nb_of(cur.end - cur.base) + nbytes);
        t.loaded_bytes += nbytes, t.pieces += 1;
        const bool wait_carry = carry_pending && ld_stream != main_stream;
        carry_pending = false;
        th_rc = BDS_OK, th_err = hipSuccess;
        th = std::thread([this, dst, off, nbytes, wait_carry] {
            th_err = hipSetDevice(ctx->device);
            if (th_err == hipSuccess && wait_carry) th_err = hipStreamWaitEvent(ld_stream, ev_carry, 0);  // nxt.buf is still being read
            if (th_err != hipSuccess) return;
            th_rc = src.load(off, nbytes, dst, ld_stream);
            if (th_rc == BDS_OK) th_err = hipStreamSynchronize(ld_stream);
        });
    }
    int join() {
        if (th.joinable()) th.join();
        if (th_rc) return th_rc;  // (the loader has set the message)
        if (th_err != hipSuccess) {
            const hipError_t e = th_err;
            th_err = hipSuccess;
            return fail(ctx, BDS_ERR_HIP, "loading the next piece of the IF record: %s", hipGetErrorString(e));
        }
        return BDS_OK;
    }
};

// ---- the three parts of a tracking call: set-up, "run one planned batch" (TrkRun::run_batch; run_streamed plans the batches of
// the resident-span path), finish.  bds_track / bds_track_mem / bds_track_dev run them in sequence (do_track); a tracking session
// (bds_track_open*) keeps what the first made and calls the second across bds_track_advance calls.  Both are built from the
// same pieces and keep only what really differs between them:
//   RecordSource (bds_record.h)  where the record lies -- a file, host memory, device memory -- behind one load()
//   TrkPlanner::span_samples     the span rule: samples a span buffer holds under a resident limit, or why the limit is too small
//   SpanPair                     the two span buffers (the context's, kept across one-shot calls; a session's)
//   TrkResults                   the 21 result arrays: one device block, prepare() before the epochs, fetch() after them
//   cno_scatter                  the five C/N0 planes to the caller's, with the caller's count of finished intervals
//   DevScope (bds_internal.h)    per-call device buffers and events, released on every exit path

// Set-up: parameters, code tables, the channel states the acquisition's table gives (tracking.m:170-188), the correlate grid.
// Nothing of it depends on the number of epochs, so a session gets the geometry of the one-shot call on the same channels.
struct TrkSetup {
    TrkParams p{};
    std::vector<ChanState> hs;
    int nblocks = 0;
    bool any_live = false;
};
static int track_setup(bds_ctx *ctx, TrackState &t, const bds_settings *s, int n_epochs, size_t n_bytes, int n_ch,
                       const bds_channel *channel, TrkSetup &u) {
    TrkParams &p = u.p;
    int rc = fill_params(ctx, *s, p, n_epochs, n_bytes);
    if (rc) return rc;
    if ((rc = ensure_prim(ctx, t, s->signal))) return rc;
    // channel state (tracking.m:170-188)
    std::vector<ChanState> &hs = u.hs;
    hs.assign((size_t)n_ch, ChanState{});
    double min_code_freq = 1e300;
    for (int c = 0; c < n_ch; ++c) {
        ChanState &cs = hs[c];
        memset(&cs, 0, sizeof(cs));
        cs.prn = channel[c].PRN;
        if (cs.prn == 0) continue;
        if (cs.prn < 1 || cs.prn > BDS_MAX_PRN) return fail(ctx, BDS_ERR_ARG, "channel(%d).PRN = %d out of range", c + 1, cs.prn);
        cs.active = 1;
        cs.codeFreq = cs.codeFreqBasis = channel[c].codeFreq;
        cs.carrFreq = cs.carrFreqBasis = channel[c].acquiredFreq;
        cs.pos = (long long)s->skipNumberOfBytes + (long long)channel[c].codePhase - 1;  // fseek, :151-153
        if (cs.pos < 0) return fail(ctx, BDS_ERR_ARG, "channel(%d): negative file offset", c + 1);
        if (!(cs.codeFreq > 0)) return fail(ctx, BDS_ERR_ARG, "channel(%d).codeFreq must be > 0", c + 1);
        min_code_freq = std::min(min_code_freq, cs.codeFreq);
        u.any_live = true;
    }
    // correlate grid: blksize stays near codeLength*fs/codeFreq; sized for code rates down to 2 % below the slowest
    // channel's (a longer block is walked by the same workgroups in further strides)
    long max_blk = (long)std::ceil((double)s->codeLength / ((min_code_freq < 1e299 ? min_code_freq : s->codeFreqBasis) * 0.98 / s->samplingFreq)) + 2;
    int nblocks = (int)((max_blk + p.chunk - 1) / p.chunk);
    if (p.runs && n_ch > 0) {
        // run-based correlator: every wave pays a fixed cost per launch (tables, first carrier, the 18-sum reduction), so
        // the grid is sized to fill the chip about once (3 workgroups per CU) and each wave walks several passes
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
        const int want = std::max(1, 3 * cus / n_ch);
        if (nblocks > want) {
            const int passes = (nblocks + want - 1) / want;
            nblocks = (nblocks + passes - 1) / passes;
        }
    }
    if (ctx->tune.trk_nblocks > 0) nblocks = ctx->tune.trk_nblocks;
    u.nblocks = nblocks;
    return BDS_OK;
}

// The planning rules of the resident-span path: how far the channels can get inside a span of the record.
static constexpr long long kNoEnd = 1LL << 36;  // "epochs still to run" of a call without a preset end (a session)
struct TrkPlanner {
    const bds_settings *s;
    const TrkParams &p;
    int n_ch;
    bool packed;
    // margin of a streamed batch's plan, in worst-case blocks kept behind the start of a channel's last planned epoch: 1 is
    // the window's own rule (n blocks at a code rate 2 % low fit); the guard of the update kernel catches a plan that was
    // too tight, and the batch is repeated with the margin doubled
    double margin;
    TrkPlanner(bds_ctx *ctx, const bds_settings *st, const TrkParams &pp, int nc)
        : s(st), p(pp), n_ch(nc), packed(pp.cplx == kFmtPacked), margin(ctx->tune.trk_stream_margin >= 0 ? ctx->tune.trk_stream_margin : 1.0) {}
    // bounds of a block while the channel's code rate stays within 2 % of f: hi is the rule the window is sized with
    long long blk_hi(double f) const { return (long long)((long)std::ceil((double)s->codeLength / (f * 0.98 / s->samplingFreq)) + 2); }
    long long blk_lo(double f) const { return std::max(1LL, (long long)std::floor((double)s->codeLength / (f * 1.02 / s->samplingFreq)) - 2); }
    // one past the last sample the `remaining` epochs still to run can touch
    long long need_end(const std::vector<ChanState> &v, long long remaining) const {
        long long e = 0;
        for (int c = 0; c < n_ch; ++c) {
            if (v[c].active != 1) continue;
            const long long B = blk_hi(v[c].codeFreq);
            e = std::max(e, v[c].pos + (remaining - 1) * B + (long long)std::ceil(std::max(1.0, margin) * (double)B));
        }
        if (packed) e = (e + 1) & ~1LL;  // (p.n_bytes is even)
        return std::min(e, p.n_bytes);
    }
    // epochs (n_max at the most) every live channel can take inside the span
    long long plan(const std::vector<ChanState> &v, const SpanStream::Span &sp, double m, long long n_max) const {
        long long n = n_max;
        for (int c = 0; c < n_ch; ++c) {
            if (v[c].active != 1) continue;
            if (v[c].pos < sp.base) return 0LL;
            if (sp.end >= p.n_bytes) continue;  // the span reaches the end of the file: a block past it is a short read
            const long long B = blk_hi(v[c].codeFreq), Blo = blk_lo(v[c].codeFreq);
            const long long per = m >= 1 ? B : Blo + (long long)(m * (double)(B - Blo));
            const long long room = sp.end - v[c].pos - std::max(1LL, (long long)std::ceil(m * (double)B));
            n = std::min(n, room < 0 ? 0LL : room / per + 1);
        }
        return n;
    }
    long long live_min_pos(const std::vector<ChanState> &v) const {
        long long m = p.n_bytes;
        for (int c = 0; c < n_ch; ++c)
            if (v[c].active == 1) m = std::min(m, v[c].pos);
        return m;
    }
    // samples a span buffer must hold at the least, from the aligned smallest position base0
    long long min_half(const std::vector<ChanState> &hs, long long base0, long long al) const {
        long long need = 0, hi_max = 0, lo_min = p.n_bytes + 1;
        for (int c = 0; c < n_ch; ++c) {
            if (hs[c].active != 1) continue;
            const long long B = blk_hi(hs[c].codeFreq);
            need = std::max(need, std::min(hs[c].pos + B, p.n_bytes) - base0);
            hi_max = std::max(hi_max, B), lo_min = std::min(lo_min, blk_lo(hs[c].codeFreq));
        }
        return (std::max(0LL, need) + std::max(0LL, hi_max - lo_min) + al + al - 1) & ~(al - 1);
    }
    // The span rule.  A span must hold, from the (16-sample aligned; packed: 32) smallest position base0, every channel's
    // position plus one block at a code rate 2 % low, plus what the start of the NEXT span -- predicted at a code rate 2 % high
    // while this one is in use -- can fall behind the channels in one epoch (min_half).  span_n: samples a span buffer holds
    // when the two together may take `limit` bytes.  A limit the library chose itself (own) is raised to what the channels
    // need; the caller's, when it is too small, is BDS_ERR_ARG.
    int span_samples(bds_ctx *ctx, const std::vector<ChanState> &hs, long long base0, size_t limit, bool own, long long &span_n,
                     long long &min_half_n) const {
        const long long al = fmt_align(p.cplx);
        min_half_n = min_half(hs, base0, al);
        const size_t min_limit = (size_t)fmt_bytes(p.cplx, 2 * min_half_n);
        if (own) limit = std::max(limit, min_limit);
        if (limit < min_limit)
            return fail(ctx, BDS_ERR_ARG, "resident limit of %zu bytes is too small for these channels: the spread of their positions plus "
                        "one block, in each of the two span buffers, needs at least %zu bytes%s", limit, min_limit,
                        packed ? " of the packed record" : "");
        span_n = fmt_samples(p.cplx, (long long)(limit / 2)) & ~(al - 1);
        return BDS_OK;
    }
};

// The device side of the epoch loop (buffers owned by the caller) and "run one planned batch".
struct TrkRun {
    bds_ctx *ctx;
    TrackState &t;
    TrkParams &p;      // base / win_end follow the span of the batch; n_epochs is the row length of the result arrays
    ChanState *d_st;   // [2][n_ch]: state and partial sums ping-pong between two halves (fuse) ...
    double *d_part;    // [2][part_n]
    size_t part_n;
    TrkOut d;          // device result arrays [n_ch][p.n_epochs]
    TrkOut *d_out;     // the same table in device memory
    int nblocks, n_ch;
    bool fuse;
    ChanState *st_final;  // where the state ends up

    void launch_update(ChanState *stp, const double *partp, int k) {
        switch (p.mode) {
            case BDS_TRACK_B2A:
                hipLaunchKernelGGL(k_trk_update<BDS_TRACK_B2A>, dim3(n_ch), dim3(kUpdThreads), 0, st(ctx), p, stp, partp, nblocks, k, d);
                break;
            case BDS_TRACK_NB:
                hipLaunchKernelGGL(k_trk_update<BDS_TRACK_NB>, dim3(n_ch), dim3(kUpdThreads), 0, st(ctx), p, stp, partp, nblocks, k, d);
                break;
            default:
                hipLaunchKernelGGL(k_trk_update<BDS_TRACK_WB>, dim3(n_ch), dim3(kUpdThreads), 0, st(ctx), p, stp, partp, nblocks, k, d);
                break;
        }
    }
    // epochs k0 .. k0 + n - 1 on span `sp`, from the state in half `slot` of d_st; the state ends up at st_final.  The last
    // epoch of a batch is closed by k_trk_update, the first one carries no update
    void run_batch(const SpanStream::Span &sp, int k0, int n, int slot) {
        p.base = sp.base, p.win_end = sp.end;
        const int8_t *data = sp.buf;
        const dim3 gc(nblocks, n_ch);
        for (int k = k0; k < k0 + n; ++k) {
            if (fuse) {
                const int curh = (slot + k - k0) & 1;
                ChanState *st_in = d_st + (size_t)curh * n_ch, *st_out = d_st + (size_t)(curh ^ 1) * n_ch;
                const double *part_prev = k > k0 ? d_part + (size_t)(curh ^ 1) * part_n : nullptr;
                double *part_cur = d_part + (size_t)curh * part_n;
                BDS_TRK_LAUNCH(k_trk_correlate, gc, (p.runs ? runs_lds_bytes(p.runs, p.prec) : 0), st(ctx), data, (const int8_t *)t.d_prim, p,
                               (const ChanState *)st_in, st_out, part_prev, part_cur, nblocks, k, (const TrkOut *)d_out);
                st_final = st_out;
                if (k == k0 + n - 1) launch_update(st_final, part_cur, k);  // the last epoch's update has no next launch to ride on
            } else {
                ChanState *stp = d_st + (size_t)slot * n_ch;
                BDS_TRK_LAUNCH(k_trk_correlate, gc, (p.runs ? runs_lds_bytes(p.runs, p.prec) : 0), st(ctx), data, (const int8_t *)t.d_prim, p,
                               (const ChanState *)stp, stp, (const double *)nullptr, d_part, nblocks, k, (const TrkOut *)d_out);
                launch_update(stp, d_part, k);
                st_final = stp;
            }
        }
    }
};

// Streamed: epochs k .. n_call - 1 of a call in batches on the resident span.  At a batch boundary the host reads the channel
// states back, moves on to the span whose tail the loader thread filled meanwhile (the overlap with the current span is carried
// device-to-device) and enqueues as many epochs as every live channel can take inside it.  `hs` is the state at epoch k on
// entry (in half `slot` of d_st) and the state reached on return; the loop also ends when no channel is live any more.
//   open_end  the run has no preset end (a session): the span is sized and the next one prefetched for the record, not the call
//   feed      the span holds what the caller has fed so far and only the caller extends it: the loop ends (no error) at the
//             first plan that gives no epoch
static int run_streamed(TrkRun &run, TrkPlanner &pl, SpanStream &ss, std::vector<ChanState> &hs, int n_call, bool open_end,
                        bool feed, int &slot, int &k) {
    bds_ctx *ctx = run.ctx;
    TrackState &t = run.t;
    const TrkParams &p = run.p;
    const int n_ch = run.n_ch;
    const long long al = fmt_align(ss.fmt), span_n = ss.span_n;
    double &margin = pl.margin;
    int rc;
    std::vector<ChanState> h0;
    while (k < n_call) {
        bool live = false;
        for (int c = 0; c < n_ch; ++c) live |= hs[c].active == 1;
        if (!live) break;
        const long long remaining = open_end ? kNoEnd : n_call - k;
        const long long minp = pl.live_min_pos(hs);
        if (ss.pre_valid && minp >= ss.pre_nb && (rc = ss.move_to(ss.pre_nb, ss.pre_hi, true))) return rc;
        long long n = pl.plan(hs, ss.cur, margin, open_end ? kNoEnd : n_call);
        if (n == 0 && feed) break;
        if (n == 0) {  // no prefetched span, or the channels are not where it was predicted: a span from their smallest position
            const long long nb = minp & ~(al - 1), hi = std::max(nb, std::min(nb + span_n, pl.need_end(hs, remaining)));
            ss.pre_valid = false;
            if (nb != ss.cur.base || hi > ss.cur.end) {
                if ((rc = ss.move_to(nb, hi, false))) return rc;
                n = pl.plan(hs, ss.cur, margin, open_end ? kNoEnd : n_call);
            }
            if (n == 0) {
                long long need = 0;
                for (int c = 0; c < n_ch; ++c)
                    if (hs[c].active == 1)
                        need = std::max(need, hs[c].pos - nb + (long long)std::ceil(std::max(1.0, margin) * (double)pl.blk_hi(hs[c].codeFreq)));
                return fail(ctx, BDS_ERR_ARG, "epoch %d: the resident span of %lld bytes (half the resident limit) cannot hold the channels' spread of positions "
                            "plus a block any more: it needs %lld bytes", k + 1, ss.nb_of(span_n), ss.nb_of((need + 2 * al - 1) & ~(al - 1)));
            }
        }
        // (a call without a preset end prefetches only when this batch uses the span up)
        const bool more = open_end ? n <= n_call - k : k + n < n_call;
        n = std::min<long long>(n, n_call - k);
        const long long want_end = pl.need_end(hs, remaining);
        if (!feed && !ss.pre_valid && more && ss.cur.end < want_end) {
            // the next span starts where the slowest channel is after the epochs a plan at the regular margin gives this
            // span, at the shortest blocks a code rate within 2 % allows: never past a channel, and still right when
            // this batch has to be repeated
            const long long n_safe = std::min(n, pl.plan(hs, ss.cur, std::max(margin, 1.0), open_end ? kNoEnd : n_call));
            long long nb = p.n_bytes;
            for (int c = 0; c < n_ch; ++c)
                if (hs[c].active == 1) nb = std::min(nb, hs[c].pos + n_safe * pl.blk_lo(hs[c].codeFreq));
            nb = std::max(ss.cur.base, nb & ~(al - 1));
            const long long hi = std::min(nb + span_n, want_end);
            if (nb <= ss.cur.end && hi > ss.cur.end) ss.predict(nb, hi);
        }
        h0 = hs;
        run.run_batch(ss.cur, k, (int)n, slot);
        // (from here to join() the loader may report an error of its own: codes are kept and reported after it)
        const hipError_t e_launch = hipGetLastError();
        if (e_launch == hipSuccess) ss.start_load();
        const hipError_t e_copy = e_launch == hipSuccess ? hipMemcpyAsync(hs.data(), run.st_final, sizeof(ChanState) * n_ch, hipMemcpyDeviceToHost, st(ctx)) : e_launch;
        const hipError_t e_sync = e_copy == hipSuccess ? hipStreamSynchronize(st(ctx)) : e_copy;
        if ((rc = ss.join())) return rc;
        BDS_HIP(ctx, e_sync);
        bool left = false;
        for (int c = 0; c < n_ch; ++c) left |= hs[c].active == -2;
        if (left) {
            // a block reached past the span (or a channel fell behind it): the batch runs again from the state it
            // started with -- the kernels are deterministic, what it rewrites is identical -- with a wider margin
            t.repeated += 1;
            margin = margin < 1 ? 1.0 : margin * 2;
            if (margin > 64) return fail(ctx, BDS_ERR_HIP, "bds_track: epoch %d: a channel keeps leaving the resident span of the record", k + 1);
            hs = h0;
            BDS_HIP(ctx, hipMemcpyAsync(run.d_st + (size_t)slot * n_ch, hs.data(), sizeof(ChanState) * n_ch, hipMemcpyHostToDevice, st(ctx)));
            BDS_HIP(ctx, hipStreamSynchronize(st(ctx)));
            continue;
        }
        slot = (int)((run.st_final - run.d_st) / n_ch);
        k += (int)n;
    }
    return BDS_OK;
}

// whole_file: load every byte (second attempt after a channel's reads left the window of the first)
static int do_track(bds_ctx *ctx, const bds_settings *s, const RecordSource &src, int n_ch, const bds_channel *channel,
                    bds_track_out *out, bool whole_file = false) {
    if (!ctx || !s || !channel || !out) return BDS_ERR_ARG;
    if (n_ch < 1 || out->n_ch != n_ch || out->n_epochs < 1) return fail(ctx, BDS_ERR_ARG, "bds_track: n_ch / n_epochs mismatch");
    if (!out->completed || !out->status || !out->absoluteSample || !out->I_P || !out->Q_P)
        return fail(ctx, BDS_ERR_ARG, "bds_track: required output arrays missing");
    if (int g = track_session_guard(ctx, "bds_track")) return g;
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->trk) ctx->trk = new TrackState();
    TrackState &t = *ctx->trk;
    const int n_epochs = out->n_epochs;
    for (int c = 0; c < n_ch; ++c) out->completed[c] = 0, out->status[c] = '-';
    TrkSetup u;
    int rc = track_setup(ctx, t, s, n_epochs, src.size(), n_ch, channel, u);
    if (rc) return rc;
    TrkParams &p = u.p;
    std::vector<ChanState> &hs = u.hs;
    const int nblocks = u.nblocks;
    // Only the part of the record the channels can touch goes to HBM: from the earliest start sample to the latest
    // start + n_epochs blocks at a code rate 2 % low (the reference streams blksize samples per epoch with fread,
    // tracking.m:237-240; a recording is usually far longer than msToProcess).  End-of-file is still judged against
    // the real file size (p.n_bytes).
    // That window is held whole (one window) when it fits and does not exceed the resident limit; otherwise the record is
    // STREAMED through a span of span_n samples that slides through two buffers (the epoch loop below).
    // Positions stay in samples; bytes appear only where memory is sized and the loader is called.  A packed record holds two
    // samples per byte: window and span bounds are kept even there (bases multiples of 32 samples = 16 bytes), so that every
    // range is whole bytes.
    const int fmt = p.cplx;
    const long long al = fmt_align(fmt);
    const bool packed = fmt == kFmtPacked;
    auto nb_of = [&](long long n) { return fmt_bytes(fmt, n); };
    const bool any_live = u.any_live;
    bool stream = false;
    using Span = SpanStream::Span;
    Span cur, nxt;  // one window: cur is the window; streamed: the two span buffers, handed to a SpanStream below
    long long span_n = 0;  // samples a span buffer holds
    TrkPlanner pl(ctx, s, p, n_ch);
    {
        long long first = p.n_bytes, last = 0;
        for (int c = 0; c < n_ch; ++c) {
            if (!hs[c].active) continue;
            const long blk_c = (long)pl.blk_hi(hs[c].codeFreq);
            first = std::min(first, hs[c].pos);
            last = std::max(last, hs[c].pos + (long long)n_epochs * blk_c);
        }
        if (whole_file || first > last) first = 0, last = p.n_bytes;
        first = std::max(0LL, std::min(first, p.n_bytes));
        last = std::max(first, std::min(last, p.n_bytes));
        if (packed) first &= ~(al - 1), last = std::min((last + 1) & ~1LL, p.n_bytes);
        p.base = first;
        p.win_end = last;
        const size_t wbytes = (size_t)nb_of(last - first);
        stream = any_live && t.resident_limit && wbytes > t.resident_limit;
        if (!stream && (t.data_cap < wbytes || !t.d_data || ctx->tune.trk_window_nomem)) {
            if (t.d_data) (void)hipFree(t.d_data), t.d_data = nullptr, t.data_cap = 0;
            hipError_t e = ctx->tune.trk_window_nomem ? hipErrorOutOfMemory : hipMalloc((void **)&t.d_data, wbytes + kDataSlack);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                if (!any_live)
                    return fail(ctx, BDS_ERR_NOMEM, "IF record window of %zu bytes does not fit in HBM: %s", wbytes, hipGetErrorString(e));
                stream = true;  // the record passes through HBM in pieces instead
            } else {
                t.data_cap = std::max<size_t>(wbytes, 1);
            }
        }
        if (!stream) {
            t.span.release();
            cur.buf = t.d_data, cur.base = first, cur.end = last;
        } else {
            if (t.d_data) (void)hipFree(t.d_data), t.d_data = nullptr, t.data_cap = 0;  // no stale window beside the span
            // the limit: the context's when it is what made the call stream, else (the window allocation failed) half of what is free
            size_t limit = t.resident_limit;
            const bool own = !limit || wbytes <= limit;
            if (own) {
                size_t fr = 0, tot = 0;
                (void)hipMemGetInfo(&fr, &tot);
                limit = std::min<size_t>(fr / 2, (size_t)1 << 30);
            }
            const long long base0 = pl.live_min_pos(hs) & ~(al - 1);
            long long min_half = 0;
            if ((rc = pl.span_samples(ctx, hs, base0, limit, own, span_n, min_half))) return rc;
            if ((rc = t.span.ensure(ctx, (size_t)nb_of(span_n)))) return rc;
            cur.buf = t.span.buf[0], nxt.buf = t.span.buf[1];
            cur.base = base0, cur.end = std::max(base0, std::min(base0 + span_n, pl.need_end(hs, n_epochs)));
        }
        // the window, or the first span
        const size_t nb0 = (size_t)nb_of(cur.end - cur.base);
        if (nb0 && (rc = src.load((size_t)nb_of(cur.base), nb0, cur.buf, st(ctx)))) return rc;
        t.loaded_bytes = nb0, t.pieces = 1, t.resident_max = nb0, t.repeated = 0;
    }
    DevScope scope;  // per-call device buffers and events, released on every exit path
    // state and partial sums ping-pong between two buffers when the loop update rides at the head of the next epoch's
    // correlate launch (default); with BDS_TRK_NOFUSE_UPDATE both halves are the same buffer and the update is its own launch
    const bool fuse = !ctx->tune.trk_nofuse_update;
    ChanState *d_st = nullptr;
    double *d_part = nullptr;
    const size_t part_n = (size_t)n_ch * nblocks * kNSums;
    BDS_HIP(ctx, scope.alloc(&d_st, sizeof(ChanState) * n_ch * 2));
    BDS_HIP(ctx, scope.alloc(&d_part, sizeof(double) * part_n * 2));
    BDS_HIP(ctx, hipMemcpyAsync(d_st, hs.data(), sizeof(ChanState) * n_ch, hipMemcpyHostToDevice, st(ctx)));
    // device result arrays, initialised like the reference template (tracking.m:48-82); arrays the variant does not create
    // still need a device target when the kernel writes them
    TrkResults res;
    if ((rc = res.prepare(ctx, n_ch, n_epochs))) return rc;
    hipEvent_t ev0, ev1;
    BDS_HIP(ctx, scope.event(&ev0));
    BDS_HIP(ctx, scope.event(&ev1));
    BDS_HIP(ctx, hipEventRecord(ev0, st(ctx)));
    TrkRun run{ctx, t, p, d_st, d_part, part_n, res.d, res.d_out, nblocks, n_ch, fuse, d_st};
    RoctxRange rg_epochs("trk.epoch_loop");
    if (!stream) {
        run.run_batch(cur, 0, n_epochs, 0);
    } else {
        SpanStream ss(ctx, t, src, st(ctx), ctx->stream2 ? (hipStream_t)ctx->stream2 : st(ctx), fmt, span_n);
        ss.cur = cur, ss.nxt = nxt;
        int slot = 0, k = 0;
        if ((rc = run_streamed(run, pl, ss, hs, n_epochs, false, false, slot, k))) return rc;
    }
    ChanState *st_final = run.st_final;
    BDS_HIP(ctx, hipGetLastError());
    BDS_HIP(ctx, hipEventRecord(ev1, st(ctx)));
    BDS_HIP(ctx, hipMemcpyAsync(hs.data(), st_final, sizeof(ChanState) * n_ch, hipMemcpyDeviceToHost, st(ctx)));
    BDS_HIP(ctx, hipStreamSynchronize(st(ctx)));
    float ms = 0;
    BDS_HIP(ctx, hipEventElapsedTime(&ms, ev0, ev1));
    memset(&ctx->timing, 0, sizeof(ctx->timing));
    ctx->timing.total_ms = ms;
    ctx->timing.n_pairs = n_epochs;
    for (int c = 0; c < n_ch; ++c)
        if (hs[c].active == -2) {  // a channel read past the loaded window (code rate > 2 % low): redo with the whole record
            if (whole_file || stream) return fail(ctx, BDS_ERR_HIP, "bds_track: channel %d left the loaded record", c + 1);
            res.release(), scope.release();  // the retry allocates its own result arrays: do not hold this attempt's beside them
            return do_track(ctx, s, src, n_ch, channel, out, true);
        }

    // The reference tracks channels one after another and returns at the first short read
    // (tracking.m:250-254): that channel keeps its partial results, later ones are never started.
    int first_abort = n_ch;
    for (int c = 0; c < n_ch; ++c)
        if (hs[c].prn != 0 && hs[c].completed < n_epochs) {
            first_abort = c;
            break;
        }
    if ((rc = res.fetch(ctx, out))) return rc;
    // epochs after the abort stay at the template value (device never wrote them), except absoluteSample of the aborted
    // epoch which the reference assigns before the read; the channels behind it go back to the template
    TrkOut unused{};
    for_each_field(out, &unused, [&](double *host, double *&, double v0) {
        if (!host) return;
        for (int c = first_abort + 1; c < n_ch; ++c)
            std::fill(host + (size_t)c * n_epochs, host + (size_t)(c + 1) * n_epochs, v0);
    });
    for (int c = 0; c < n_ch; ++c) {
        if (hs[c].prn == 0 || c > first_abort) {
            out->completed[c] = 0;
            continue;
        }
        out->completed[c] = hs[c].completed;
        if (hs[c].completed == n_epochs) out->status[c] = channel[c].status;  // :441
    }
    // C/N0 + lock detector (tracking.m:411-434): computed on the device from the arrays above
    const int M = s->CNoInterval;
    if (M > 1 && out->n_cno > 0 && out->DataCNo) {
        const int pm = p.pilot ? (p.mode == BDS_TRACK_WB ? 2 : 1) : 0;
        const int nq = out->n_cno;
        double *d_raw = nullptr, *d_cno = nullptr;
        BDS_HIP(ctx, scope.alloc(&d_raw, sizeof(double) * (size_t)n_ch * nq * 3));
        BDS_HIP(ctx, scope.alloc(&d_cno, sizeof(double) * (size_t)n_ch * nq * 5));
        BDS_HIP(ctx, hipMemcpyAsync(d_st, hs.data(), sizeof(ChanState) * n_ch, hipMemcpyHostToDevice, st(ctx)));
        hipLaunchKernelGGL(k_trk_cno, dim3(n_ch), dim3(256), 0, st(ctx), res.d, (const ChanState *)d_st, n_epochs, M, nq, pm,
                           s->intTime, d_raw, d_cno);
        // interval q counts when (q + 1) M <= completed
        return cno_scatter(ctx, d_cno, n_ch, nq, pm, out, [&](int c) { return out->completed[c] / M; });
    }
    return BDS_OK;
}

}  // namespace bds

// ---- tracking sessions (bds_track_open* .. bds_track_close) ---------------------------------------------------------------
// A session is the batch boundary of the resident-span path made public: between two bds_track_advance calls the host holds
// the ChanState of every channel, the first epoch of an advance carries no update and the last is closed by k_trk_update.
// Geometry (nblocks, chunk, SEG) is what track_setup gives the one-shot call on the same channels and settings -- the
// fixed-order sum of the partial sums depends on it --, so the concatenated arrays equal that call's bit for bit.
struct bds_track_session {
    bds_ctx *ctx = nullptr;
    bds_settings s{};
    int n_ch = 0;
    bds::TrkSetup u;        // parameters, host copy of the channel states (completed: epochs of the CURRENT advance), grid
    double margin = 1.0;    // of the batch plans; doubled for good when the window guard fires
    std::vector<long long> epochs_done;
    // the record
    bool feed = false, fed_last = false;
    bds::RecordSource src;  // (a fed session: none)
    std::unique_ptr<bds::SpanStream> ss;
    bds::SpanPair span;
    // the epoch loop's device buffers
    bds::ChanState *d_st = nullptr;
    double *d_part = nullptr;
    size_t part_n = 0;
    int slot = 0;
    bds::TrkResults res;  // the result arrays of an advance
    // C/N0 carry (k_trk_cno_seg)
    double *d_carry = nullptr, *d_prev3 = nullptr, *d_raw = nullptr, *d_cno = nullptr;
    int *d_ncarry = nullptr;
    int cno_cap = 0;
};

namespace bds {

static constexpr size_t kSessionResident = (size_t)256 << 20;  // resident limit of a session when the context has none
static constexpr size_t kSessionStage = (size_t)64 << 20;      // pinned staging of a session that reads a file, at the most
static constexpr long long kFeedOpen = 1LL << 60;             // "samples in the record" while a feed session has not seen `last`

static std::mutex g_sess_mu;
static std::set<const bds_track_session *> g_sessions;  // handles that are open: anything else is refused unread
static bds_track_session *live_session(bds_track_session *h) {
    std::lock_guard<std::mutex> lk(g_sess_mu);
    return h && g_sessions.count(h) ? h : nullptr;
}

int track_session_guard(bds_ctx *ctx, const char *who) {
    if (!ctx || !ctx->trk || !ctx->trk->session) return BDS_OK;
    const bds_track_session *h = ctx->trk->session;
    return fail(ctx, BDS_ERR_ARG, "%s: the context has an open tracking session (%d channels on %s): bds_track_close it first", who, h->n_ch,
                h->src.what());
}

static void session_close(bds_track_session *h) {
    {
        std::lock_guard<std::mutex> lk(g_sess_mu);
        g_sessions.erase(h);
    }
    bds_ctx *ctx = h->ctx;
    (void)hipSetDevice(ctx->device);
    h->ss.reset();  // joins the loader
    (void)hipStreamSynchronize(st(ctx));
    if (ctx->stream2) (void)hipStreamSynchronize((hipStream_t)ctx->stream2);
    h->span.release();
    for (void *q : {(void *)h->d_st, (void *)h->d_part, (void *)h->d_carry, (void *)h->d_prev3, (void *)h->d_raw, (void *)h->d_cno, (void *)h->d_ncarry})
        if (q) (void)hipFree(q);
    if (ctx->trk && ctx->trk->session == h) ctx->trk->session = nullptr;
    delete h;  // (the result block, the record's file and its staging buffer go with it)
}

// kind: 0 file at `path`, 1 `n_bytes` bytes at `mem`, 2 fed by the caller from sample `origin` on, 3 `n_bytes` bytes at `mem` in
// device memory (the caller has checked the span: check_device_span)
static bds_track_session *session_open(bds_ctx *ctx, const bds_settings *s, int kind, const char *path, const int8_t *mem,
                                       size_t n_bytes, long long origin, int n_ch, const bds_channel *channel) {
    const char *who = kind == 0 ? "bds_track_open" : kind == 1 ? "bds_track_open_mem" : kind == 2 ? "bds_track_open_feed" : "bds_track_open_dev";
    if (!ctx) return nullptr;
    if (!s || !channel || n_ch < 1 || (kind == 0 && !path) || ((kind == 1 || kind == 3) && !mem)) {
        fail(ctx, BDS_ERR_ARG, "%s: settings, channel table (n_ch >= 1) and the record are required", who);
        return nullptr;
    }
    if (track_session_guard(ctx, who)) return nullptr;
    if (hipSetDevice(ctx->device) != hipSuccess) {
        fail(ctx, BDS_ERR_HIP, "%s: hipSetDevice failed", who);
        return nullptr;
    }
    if (!ctx->trk) ctx->trk = new TrackState();
    TrackState &t = *ctx->trk;
    bds_track_session *h = new bds_track_session();
    h->ctx = ctx, h->s = *s, h->n_ch = n_ch, h->feed = kind == 2;
    h->epochs_done.assign((size_t)n_ch, 0);
    h->margin = ctx->tune.trk_stream_margin >= 0 ? ctx->tune.trk_stream_margin : 1.0;
    // (not registered yet: every failure below frees it here)
    auto body = [&]() -> int {
        int rc = BDS_OK;
        switch (kind) {
        case 0: rc = h->src.open_file(ctx, path, kSessionStage); break;
        case 1: h->src.set_host(ctx, mem, n_bytes); break;
        case 3: h->src.set_device(ctx, mem, n_bytes); break;
        default: h->src.set_none(ctx); break;
        }
        if (rc) return rc;
        if ((rc = track_setup(ctx, t, &h->s, 1, h->src.size(), n_ch, channel, h->u))) return rc;
        TrkParams &p = h->u.p;
        std::vector<ChanState> &hs = h->u.hs;
        const int fmt = p.cplx;
        const long long al = fmt_align(fmt);
        if (kind == 2) {
            if (origin < 0 || origin % 32) return fail(ctx, BDS_ERR_ARG, "%s: origin_sample = %lld must be a non-negative multiple of 32 samples", who, origin);
            for (int c = 0; c < n_ch; ++c)
                if (hs[c].active == 1 && hs[c].pos < origin)
                    return fail(ctx, BDS_ERR_ARG, "%s: channel(%d) starts at sample %lld of the record, before origin_sample = %lld", who, c + 1, hs[c].pos, origin);
            p.n_bytes = kFeedOpen;
        }
        // the resident span: sized like do_track's streamed path, from the context's resident limit or the session's default
        TrkPlanner pl(ctx, &h->s, p, n_ch);
        const long long base0 = kind == 2 ? origin : pl.live_min_pos(hs) & ~(al - 1);
        long long span_n = 0, min_half = 0;
        if ((rc = pl.span_samples(ctx, hs, base0, t.resident_limit ? t.resident_limit : kSessionResident, !t.resident_limit, span_n, min_half)))
            return rc;
        if (kind != 2)  // no more than the record from the first channel on
            span_n = std::min(span_n, std::max(min_half, (std::max(0LL, p.n_bytes - base0) + al - 1) & ~(al - 1)));
        if ((rc = h->span.ensure(ctx, (size_t)fmt_bytes(fmt, span_n)))) return rc;
        // (feed: the caller's thread is the loader -- one stream)
        h->ss.reset(new SpanStream(ctx, t, h->src, st(ctx), kind != 2 && ctx->stream2 ? (hipStream_t)ctx->stream2 : st(ctx), fmt, span_n));
        h->ss->cur.buf = h->span.buf[0], h->ss->cur.base = h->ss->cur.end = base0;  // (the first advance / feed fills it)
        h->ss->nxt.buf = h->span.buf[1];
        t.loaded_bytes = 0, t.pieces = 0, t.resident_max = 0, t.repeated = 0;
        // the epoch loop's buffers; the state starts in half 0
        h->part_n = (size_t)n_ch * h->u.nblocks * kNSums;
        BDS_HIP(ctx, hipMalloc((void **)&h->d_st, sizeof(ChanState) * n_ch * 2));
        BDS_HIP(ctx, hipMalloc((void **)&h->d_part, sizeof(double) * h->part_n * 2));
        const int M = h->s.CNoInterval;
        if (M > 1) {
            BDS_HIP(ctx, hipMalloc((void **)&h->d_carry, sizeof(double) * (size_t)n_ch * 4 * M));
            BDS_HIP(ctx, hipMalloc((void **)&h->d_prev3, sizeof(double) * (size_t)n_ch * 3));
            BDS_HIP(ctx, hipMalloc((void **)&h->d_ncarry, sizeof(int) * (size_t)n_ch));
            BDS_HIP(ctx, hipMemsetAsync(h->d_carry, 0, sizeof(double) * (size_t)n_ch * 4 * M, st(ctx)));
            BDS_HIP(ctx, hipMemsetAsync(h->d_prev3, 0, sizeof(double) * (size_t)n_ch * 3, st(ctx)));
            BDS_HIP(ctx, hipMemsetAsync(h->d_ncarry, 0, sizeof(int) * (size_t)n_ch, st(ctx)));
        }
        BDS_HIP(ctx, hipStreamSynchronize(st(ctx)));
        return BDS_OK;
    };
    if (body() != BDS_OK) {
        session_close(h);
        return nullptr;
    }
    t.session = h;
    std::lock_guard<std::mutex> lk(g_sess_mu);
    g_sessions.insert(h);
    return h;
}

}  // namespace bds

using namespace bds;

extern "C" bds_track_session *bds_track_open(bds_ctx *ctx, const bds_settings *s, const char *path, int n_ch, const bds_channel *channel) {
    return session_open(ctx, s, 0, path, nullptr, 0, 0, n_ch, channel);
}

extern "C" bds_track_session *bds_track_open_mem(bds_ctx *ctx, const bds_settings *s, const int8_t *file_bytes, size_t n_bytes, int n_ch,
                                                 const bds_channel *channel) {
    return session_open(ctx, s, 1, nullptr, file_bytes, n_bytes, 0, n_ch, channel);
}

extern "C" bds_track_session *bds_track_open_dev(bds_ctx *ctx, const bds_settings *s, const void *d_file_bytes, size_t n_bytes, int n_ch,
                                                 const bds_channel *channel) {
    if (!ctx) return nullptr;
    if (!d_file_bytes) {
        fail(ctx, BDS_ERR_ARG, "bds_track_open_dev: d_file_bytes is NULL");
        return nullptr;
    }
    if (check_device_span(ctx, "bds_track_open_dev", "d_file_bytes", d_file_bytes, n_bytes)) return nullptr;
    return session_open(ctx, s, 3, nullptr, (const int8_t *)d_file_bytes, n_bytes, 0, n_ch, channel);
}

extern "C" bds_track_session *bds_track_open_feed(bds_ctx *ctx, const bds_settings *s, long long origin_sample, int n_ch,
                                                  const bds_channel *channel) {
    return session_open(ctx, s, 2, nullptr, nullptr, 0, origin_sample, n_ch, channel);
}

extern "C" void bds_track_close(bds_track_session *sess) {
    if (bds_track_session *h = live_session(sess)) session_close(h);
}

// bds_track_feed (dev = false: `bytes` in host memory) and bds_track_feed_dev (dev = true: in device memory): one body, the copy's
// direction apart
static int track_feed(bds_track_session *sess, const int8_t *bytes, size_t n_bytes, int last, bool dev) {
    const char *who = dev ? "bds_track_feed_dev" : "bds_track_feed";
    bds_track_session *h = live_session(sess);
    if (!h) return BDS_ERR_ARG;
    bds_ctx *ctx = h->ctx;
    if (!h->feed) return fail(ctx, BDS_ERR_ARG, "%s: this session reads its record itself (it was not opened with bds_track_open_feed)", who);
    if (h->fed_last) return fail(ctx, BDS_ERR_ARG, "%s: the end of the record has been fed already", who);
    if (n_bytes && !bytes) return fail(ctx, BDS_ERR_ARG, "%s: %s missing (NULL with %zu bytes to go)", who, dev ? "d_bytes" : "bytes", n_bytes);
    TrkParams &p = h->u.p;
    if (p.cplx == kFmtIQ && (n_bytes & 1)) return fail(ctx, BDS_ERR_ARG, "%s: an I/Q record takes whole int8 pairs, %zu bytes is an odd count", who, n_bytes);
    // a 16-bit record: a call takes whole samples (or pairs) and leaves the rest of what it was offered to the caller; the END
    // of the record cannot lie inside one
    const size_t unit = fmt_16bit(p.cplx) ? (size_t)fmt_bps(p.cplx) : p.cplx == kFmtIQ ? 2 : 1;
    if (fmt_16bit(p.cplx) && last && n_bytes % unit)
        return fail(ctx, BDS_ERR_ARG, "%s: settings.dataType 'int16': the last %zu bytes of the record are not a whole number of %s", who, n_bytes,
                    p.cplx == kFmtIQ16 ? "I/Q int16 pairs (4 bytes each)" : "int16 samples (2 bytes each)");
    if (dev)
        if (int rc = check_device_span(ctx, who, "d_bytes", bytes, n_bytes)) return rc;
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    TrackState &t = *ctx->trk;
    SpanStream &ss = *h->ss;
    const long long al = fmt_align(ss.fmt);
    const size_t offered = std::min<size_t>(n_bytes, (size_t)1 << 30);  // (the count returned is an int)
    auto room = [&] { return (size_t)(ss.nb_of(ss.span_n) - ss.nb_of(ss.cur.end - ss.cur.base)); };
    if (room() < offered) {
        // release what lies behind the slowest live channel: the rest is carried to the other buffer, device to device
        long long nb = ss.cur.end;
        for (const ChanState &c : h->u.hs)
            if (c.active == 1) nb = std::min(nb, c.pos);
        nb &= ~(al - 1);
        if (nb > ss.cur.base) {
            int rc = ss.move_to(nb, ss.cur.end, true);
            if (rc) return rc;
        }
    }
    const size_t take = std::min(offered, room()) & ~(unit - 1);
    if (take) {
        BDS_HIP(ctx, hipMemcpyAsync(ss.cur.buf + ss.nb_of(ss.cur.end - ss.cur.base), bytes, take, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st(ctx)));
        BDS_HIP(ctx, hipStreamSynchronize(st(ctx)));  // the bytes are the caller's again on return
        ss.cur.end += fmt_samples(p.cplx, (long long)take);
        t.loaded_bytes += take, t.pieces += 1;
        t.resident_max = std::max(t.resident_max, (size_t)ss.nb_of(ss.cur.end - ss.cur.base));
    }
    if (last && take == n_bytes) h->fed_last = true, p.n_bytes = ss.cur.end;  // end of file is judged against the fed length from here on
    return (int)take;
}

extern "C" int bds_track_feed(bds_track_session *sess, const int8_t *bytes, size_t n_bytes, int last) {
    return track_feed(sess, bytes, n_bytes, last, false);
}

extern "C" int bds_track_feed_dev(bds_track_session *sess, const void *d_bytes, size_t n_bytes, int last) {
    return track_feed(sess, (const int8_t *)d_bytes, n_bytes, last, true);
}

extern "C" int bds_track_session_info(bds_track_session *sess, int32_t *epochs_done, long long *next_sample, long long *fed_end,
                                      long long *resident_bytes) {
    bds_track_session *h = live_session(sess);
    if (!h) return BDS_ERR_ARG;
    for (int c = 0; c < h->n_ch; ++c) {
        if (epochs_done) epochs_done[c] = (int32_t)h->epochs_done[c];
        if (next_sample) next_sample[c] = h->u.hs[c].prn ? h->u.hs[c].pos : 0;
    }
    if (fed_end) *fed_end = h->feed ? h->ss->cur.end : h->u.p.n_bytes;
    if (resident_bytes) *resident_bytes = h->ss->nb_of(h->ss->cur.end - h->ss->cur.base);
    return BDS_OK;
}

extern "C" int bds_track_advance(bds_track_session *sess, int max_epochs, bds_track_out *out, int32_t *n_cno_done) {
    bds_track_session *h = live_session(sess);
    if (!h) return BDS_ERR_ARG;
    bds_ctx *ctx = h->ctx;
    const int n_ch = h->n_ch;
    if (!out || max_epochs < 1 || out->n_ch != n_ch || out->n_epochs < max_epochs)
        return fail(ctx, BDS_ERR_ARG, "bds_track_advance: n_ch / n_epochs mismatch (out->n_epochs is the capacity: >= max_epochs)");
    if (!out->completed || !out->status || !out->absoluteSample || !out->I_P || !out->Q_P)
        return fail(ctx, BDS_ERR_ARG, "bds_track_advance: required output arrays missing");
    TrkParams &p = h->u.p;
    std::vector<ChanState> &hs = h->u.hs;
    // C/N0 intervals that can complete in this call: checked before anything runs
    const int M = h->s.CNoInterval;
    int need_cno = 0;
    if (M > 1)
        for (int c = 0; c < n_ch; ++c)
            if (hs[c].active == 1) need_cno = std::max(need_cno, (int)((h->epochs_done[c] + max_epochs) / M - h->epochs_done[c] / M));
    if (out->DataCNo && out->n_cno < need_cno)
        return fail(ctx, BDS_ERR_ARG, "bds_track_advance: out->n_cno = %d, but %d C/N0 intervals can complete in this call", out->n_cno, need_cno);
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    TrackState &t = *ctx->trk;
    // the call's result arrays, rows of out->n_epochs, at the reference's template values
    const int row = out->n_epochs;
    if (int rc = h->res.prepare(ctx, n_ch, row)) return rc;
    const int nq = std::max(need_cno, 1);
    if (M > 1 && h->cno_cap < nq) {
        if (h->d_raw) (void)hipFree(h->d_raw), h->d_raw = nullptr;
        if (h->d_cno) (void)hipFree(h->d_cno), h->d_cno = nullptr;
        h->cno_cap = 0;
        BDS_HIP(ctx, hipMalloc((void **)&h->d_raw, sizeof(double) * (size_t)n_ch * nq * 3));
        BDS_HIP(ctx, hipMalloc((void **)&h->d_cno, sizeof(double) * (size_t)n_ch * nq * 5));
        h->cno_cap = nq;
    }
    // the epochs: `completed` counts within the call, the result arrays are indexed by the call's own epoch number
    for (ChanState &c : hs) c.completed = 0;
    BDS_HIP(ctx, hipMemcpyAsync(h->d_st + (size_t)h->slot * n_ch, hs.data(), sizeof(ChanState) * n_ch, hipMemcpyHostToDevice, st(ctx)));
    p.n_epochs = row;
    TrkRun run{ctx, t, p, h->d_st, h->d_part, h->part_n, h->res.d, h->res.d_out, h->u.nblocks, n_ch, !ctx->tune.trk_nofuse_update,
               h->d_st + (size_t)h->slot * n_ch};
    TrkPlanner pl(ctx, &h->s, p, n_ch);
    pl.margin = h->margin;
    int k = 0, rc;
    {
        RoctxRange rg_epochs("trk.epoch_loop");
        rc = run_streamed(run, pl, *h->ss, hs, max_epochs, true, h->feed, h->slot, k);
    }
    h->margin = pl.margin;
    if (rc) return rc;
    BDS_HIP(ctx, hipGetLastError());
    const int pm = p.pilot ? (p.mode == BDS_TRACK_WB ? 2 : 1) : 0;
    const bool cno_ran = M > 1 && k > 0;
    if (cno_ran)
        hipLaunchKernelGGL(k_trk_cno_seg, dim3(n_ch), dim3(256), 0, st(ctx), h->res.d, (const ChanState *)(h->d_st + (size_t)h->slot * n_ch), row, M, nq,
                           pm, h->s.intTime, h->d_carry, h->d_ncarry, h->d_prev3, h->d_raw, h->d_cno);
    if ((rc = h->res.fetch(ctx, out))) return rc;
    // intervals a channel finished in this call: those its epochs of before and of this call complete together
    std::vector<int> nd((size_t)n_ch, 0);
    for (int c = 0; c < n_ch; ++c) {
        const int done = hs[c].prn ? hs[c].completed : 0;
        const long long e0 = h->epochs_done[c];
        if (M > 1) nd[c] = (int)((e0 + done) / M - e0 / M);
        out->completed[c] = done;
        out->status[c] = hs[c].prn && k > 0 && done == k ? 'T' : '-';
        if (n_cno_done) n_cno_done[c] = nd[c];
        h->epochs_done[c] = e0 + done;
    }
    if (out->DataCNo && (rc = cno_scatter(ctx, cno_ran ? h->d_cno : nullptr, n_ch, nq, pm, out, [&](int c) { return nd[c]; }))) return rc;
    return k;
}

extern "C" int bds_track_mem(bds_ctx *ctx, const bds_settings *s, const int8_t *file_bytes, size_t n_bytes, int n_ch,
                             const bds_channel *channel, bds_track_out *out) {
    if (!ctx || !file_bytes) return BDS_ERR_ARG;
    RecordSource src;
    src.set_host(ctx, file_bytes, n_bytes);
    return do_track(ctx, s, src, n_ch, channel, out);
}

extern "C" int bds_track_dev(bds_ctx *ctx, const bds_settings *s, const void *d_file_bytes, size_t n_bytes, int n_ch,
                             const bds_channel *channel, bds_track_out *out) {
    if (!ctx) return BDS_ERR_ARG;
    if (!d_file_bytes) return fail(ctx, BDS_ERR_ARG, "bds_track_dev: d_file_bytes is NULL");
    if (int rc = check_device_span(ctx, "bds_track_dev", "d_file_bytes", d_file_bytes, n_bytes)) return rc;
    RecordSource src;
    src.set_device(ctx, d_file_bytes, n_bytes);
    return do_track(ctx, s, src, n_ch, channel, out);
}

extern "C" int bds_track(bds_ctx *ctx, const bds_settings *s, const char *path, int n_ch, const bds_channel *channel,
                         bds_track_out *out) {
    if (!ctx || !path) return BDS_ERR_ARG;
    // the window of the record the channels can touch, staged through pinned memory in 256 MiB pieces
    RecordSource src;
    if (int rc = src.open_file(ctx, path, (size_t)256 << 20)) return rc;
    return do_track(ctx, s, src, n_ch, channel, out);
}

extern "C" long long bds_track_loaded_bytes(bds_ctx *ctx) {
    return (ctx && ctx->trk) ? (long long)ctx->trk->loaded_bytes : 0;
}

extern "C" int bds_track_set_resident_limit(bds_ctx *ctx, size_t bytes) {
    if (!ctx) return BDS_ERR_ARG;
    if (!ctx->trk) ctx->trk = new TrackState();
    ctx->trk->resident_limit = bytes;
    return BDS_OK;
}

extern "C" int bds_track_stream_info(bds_ctx *ctx, int32_t *pieces, long long *resident_max_bytes, int32_t *repeated_batches) {
    if (!ctx) return BDS_ERR_ARG;
    const TrackState *t = ctx->trk;
    if (pieces) *pieces = t ? t->pieces : 0;
    if (resident_max_bytes) *resident_max_bytes = t ? (long long)t->resident_max : 0;
    if (repeated_batches) *repeated_batches = t ? t->repeated : 0;
    return BDS_OK;
}

namespace bds {
// What bds_corrfn.hip takes over from the trackers for a record of n_bytes: mode, pilot, sample format and sample count as
// fill_params derives them (with its argument errors), the device's code tables, the resident limit of the context.
int track_open_loop_setup(bds_ctx *ctx, const bds_settings &s, size_t n_bytes, TrkOpenLoop &o) {
    if (!ctx->trk) ctx->trk = new TrackState();
    TrackState &t = *ctx->trk;
    TrkParams p{};
    if (int rc = fill_params(ctx, s, p, 1, n_bytes)) return rc;
    if (int rc = ensure_prim(ctx, t, s.signal)) return rc;
    o.mode = p.mode, o.pilot = p.pilot, o.fmt = p.cplx, o.code_len = p.code_len;
    o.fs = p.fs, o.inv_fs = p.inv_fs, o.n_samples = p.n_bytes;
    o.d_prim = t.d_prim;
    o.resident_limit = t.resident_limit;
    return BDS_OK;
}
}  // namespace bds

extern "C" int bds_track_correlate(bds_ctx *ctx, const bds_settings *s, const int8_t *file_bytes, size_t n_bytes,
                                   int n_ch, const int32_t *prn, const double *state6, double *sums18) {
    if (!ctx || !s || !file_bytes || !prn || !state6 || !sums18 || n_ch < 1) return BDS_ERR_ARG;
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->trk) ctx->trk = new TrackState();
    TrackState &t = *ctx->trk;
    TrkParams p{};
    int rc = fill_params(ctx, *s, p, 1, n_bytes);
    if (rc) return rc;
    p.base = 0, p.win_end = p.n_bytes;  // the whole block is resident (the bounds the debug build checks the loads against)
    if ((rc = ensure_prim(ctx, t, s->signal))) return rc;
    long max_blk = 0;
    for (int c = 0; c < n_ch; ++c) {
        if (prn[c] < 1 || prn[c] > BDS_MAX_PRN) return fail(ctx, BDS_ERR_ARG, "prn[%d] out of range", c);
        max_blk = std::max(max_blk, (long)state6[c * 6 + 1]);
    }
    const int nblocks = (int)std::max<long>(1, (max_blk + p.chunk - 1) / p.chunk);
    int8_t *d_data = nullptr;
    int *d_prn = nullptr;
    double *d_s6 = nullptr, *d_part = nullptr, *d_sums = nullptr;
    DevScope scope;
    BDS_HIP(ctx, scope.alloc(&d_data, n_bytes + kDataSlack));
    BDS_HIP(ctx, scope.alloc(&d_prn, sizeof(int) * n_ch));
    BDS_HIP(ctx, scope.alloc(&d_s6, sizeof(double) * 6 * n_ch));
    BDS_HIP(ctx, scope.alloc(&d_part, sizeof(double) * (size_t)n_ch * nblocks * kNSums));
    BDS_HIP(ctx, scope.alloc(&d_sums, sizeof(double) * (size_t)n_ch * kNSums));
    BDS_HIP(ctx, hipMemcpyAsync(d_data, file_bytes, n_bytes, hipMemcpyHostToDevice, st(ctx)));
    BDS_HIP(ctx, hipMemcpyAsync(d_prn, prn, sizeof(int) * n_ch, hipMemcpyHostToDevice, st(ctx)));
    BDS_HIP(ctx, hipMemcpyAsync(d_s6, state6, sizeof(double) * 6 * n_ch, hipMemcpyHostToDevice, st(ctx)));
    dim3 gc(nblocks, n_ch);
    // bds_get_timing after this call: search_ms = the two kernels alone (the upload and the download stand outside the events)
    hipEvent_t ev[2] = {nullptr, nullptr};
    BDS_HIP(ctx, scope.event(&ev[0]));
    BDS_HIP(ctx, scope.event(&ev[1]));
    BDS_HIP(ctx, hipEventRecord(ev[0], st(ctx)));
    BDS_TRK_LAUNCH(k_trk_correlate_open, gc, (p.runs ? runs_lds_bytes(p.runs, p.prec) : 0), st(ctx), (const int8_t *)d_data, (const int8_t *)t.d_prim, p,
                   (const int *)d_prn, (const double *)d_s6, d_part, nblocks);
    hipLaunchKernelGGL(k_trk_reduce_open, dim3(n_ch), dim3(64), 0, st(ctx), (const double *)d_part, nblocks, d_sums);
    BDS_HIP(ctx, hipGetLastError());
    BDS_HIP(ctx, hipEventRecord(ev[1], st(ctx)));
    BDS_HIP(ctx, hipMemcpyAsync(sums18, d_sums, sizeof(double) * (size_t)n_ch * kNSums, hipMemcpyDeviceToHost, st(ctx)));
    BDS_HIP(ctx, hipStreamSynchronize(st(ctx)));
    float ms = 0.f;
    BDS_HIP(ctx, hipEventElapsedTime(&ms, ev[0], ev[1]));
    ctx->timing = bds_timing{};
    ctx->timing.search_ms = ms;
    return BDS_OK;
}

// Test aid (bds_track_colon): element k[i] of the colon vector a[i] : d[i] : b[i] exactly as the correlators form it
__global__ void k_colon_eval(const double *__restrict__ a, const double *__restrict__ d, const double *__restrict__ b,
                             const int *__restrict__ k, int n, double *__restrict__ val, double *__restrict__ cend,
                             int *__restrict__ nint) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ColonVec v = colon_vec(a[i], d[i], b[i]);
    val[i] = colon_at(v, k[i]);
    cend[i] = v.c;
    nint[i] = v.n;
}

extern "C" int bds_track_colon(bds_ctx *ctx, int n, const double *a, const double *d, const double *b, const int32_t *k,
                               double *value, double *c_end, int32_t *n_intervals) {
    if (!ctx || !a || !d || !b || !k || !value || !c_end || !n_intervals || n < 1) return BDS_ERR_ARG;
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nd = sizeof(double) * (size_t)n, ni = sizeof(int) * (size_t)n;
    double *d_in = nullptr, *d_out = nullptr;  // a, d, b | value, c
    int *d_k = nullptr, *d_n = nullptr;
    DevScope scope;
    BDS_HIP(ctx, scope.alloc(&d_in, 3 * nd));
    BDS_HIP(ctx, scope.alloc(&d_out, 2 * nd));
    BDS_HIP(ctx, scope.alloc(&d_k, ni));
    BDS_HIP(ctx, scope.alloc(&d_n, ni));
    BDS_HIP(ctx, hipMemcpyAsync(d_in, a, nd, hipMemcpyHostToDevice, st(ctx)));
    BDS_HIP(ctx, hipMemcpyAsync(d_in + n, d, nd, hipMemcpyHostToDevice, st(ctx)));
    BDS_HIP(ctx, hipMemcpyAsync(d_in + 2 * (size_t)n, b, nd, hipMemcpyHostToDevice, st(ctx)));
    BDS_HIP(ctx, hipMemcpyAsync(d_k, k, ni, hipMemcpyHostToDevice, st(ctx)));
    hipLaunchKernelGGL(k_colon_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st(ctx), (const double *)d_in,
                       (const double *)(d_in + n), (const double *)(d_in + 2 * (size_t)n), (const int *)d_k, n, d_out, d_out + n, d_n);
    BDS_HIP(ctx, hipGetLastError());
    BDS_HIP(ctx, hipMemcpyAsync(value, d_out, nd, hipMemcpyDeviceToHost, st(ctx)));
    BDS_HIP(ctx, hipMemcpyAsync(c_end, d_out + n, nd, hipMemcpyDeviceToHost, st(ctx)));
    BDS_HIP(ctx, hipMemcpyAsync(n_intervals, d_n, ni, hipMemcpyDeviceToHost, st(ctx)));
    BDS_HIP(ctx, hipStreamSynchronize(st(ctx)));
    return BDS_OK;
}

// Test aid (bds_track_cno): k_trk_cno, or k_trk_cno_seg once per piece, on prompt arrays of the caller.  The host side only
// places the arrays and gathers the intervals of each piece, as do_track / bds_track_advance do.
extern "C" int bds_track_cno(bds_ctx *ctx, const bds_settings *s, int n_ch, int n_epochs, const double *prompts,
                             const int32_t *done, int n_pieces, const int32_t *pieces, int n_cno, double *cno5) {
    if (!ctx) return BDS_ERR_ARG;
    if (!s || !prompts || !done || !cno5 || n_ch < 1 || n_epochs < 1 || n_cno < 1 || n_pieces < 0 || (n_pieces > 0 && !pieces))
        return fail(ctx, BDS_ERR_ARG, "bds_track_cno: missing argument or empty shape");
    const int M = s->CNoInterval;
    if (M < 2 || !(s->intTime > 0)) return fail(ctx, BDS_ERR_ARG, "bds_track_cno: CNoInterval must be >= 2 and intTime > 0");
    if (s->signal != BDS_SIGNAL_B1C && s->signal != BDS_SIGNAL_B2A) return fail(ctx, BDS_ERR_ARG, "settings.signal invalid");
    for (int c = 0; c < n_ch; ++c)
        if (done[c] < 0 || done[c] > n_epochs) return fail(ctx, BDS_ERR_ARG, "bds_track_cno: done[%d] outside 0 .. n_epochs", c);
    long long total = 0;
    for (int i = 0; i < n_pieces; ++i) {
        if (pieces[i] < 1) return fail(ctx, BDS_ERR_ARG, "bds_track_cno: pieces[%d] must be >= 1", i);
        total += pieces[i];
    }
    if (n_pieces > 0 && total != n_epochs) return fail(ctx, BDS_ERR_ARG, "bds_track_cno: the pieces must add up to n_epochs");
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    const int mode = track_mode(*s);
    const int pm = pilot_on(*s, mode) ? (mode == BDS_TRACK_WB ? 2 : 1) : 0;
    const size_t ne = (size_t)n_ch * n_epochs;
    const int nq_max = std::max(n_cno, n_epochs / M + 2);  // intervals one launch can report
    DevScope scope;
    double *d_p = nullptr, *d_raw = nullptr, *d_cno = nullptr, *d_carry = nullptr, *d_prev3 = nullptr;
    int *d_ncarry = nullptr;
    ChanState *d_st = nullptr;
    BDS_HIP(ctx, scope.alloc(&d_p, sizeof(double) * 4 * ne));
    BDS_HIP(ctx, scope.alloc(&d_raw, sizeof(double) * (size_t)n_ch * nq_max * 3));
    BDS_HIP(ctx, scope.alloc(&d_cno, sizeof(double) * (size_t)n_ch * nq_max * 5));
    BDS_HIP(ctx, scope.alloc(&d_st, sizeof(ChanState) * n_ch));
    BDS_HIP(ctx, hipMemcpyAsync(d_p, prompts, sizeof(double) * 4 * ne, hipMemcpyHostToDevice, st(ctx)));
    std::vector<ChanState> hs(n_ch);
    for (int c = 0; c < n_ch; ++c) {
        hs[c] = ChanState{};
        hs[c].prn = 1;
    }
    const size_t out_plane = (size_t)n_ch * n_cno;
    if (n_pieces == 0) {  // the post-pass of bds_track
        for (int c = 0; c < n_ch; ++c) hs[c].completed = done[c];
        TrkOut d{};
        d.I_P = d_p, d.Q_P = d_p + ne, d.Pilot_I_P = d_p + 2 * ne, d.Pilot_Q_P = d_p + 3 * ne;
        BDS_HIP(ctx, hipMemcpyAsync(d_st, hs.data(), sizeof(ChanState) * n_ch, hipMemcpyHostToDevice, st(ctx)));
        hipLaunchKernelGGL(k_trk_cno, dim3(n_ch), dim3(256), 0, st(ctx), d, (const ChanState *)d_st, n_epochs, M, n_cno, pm, s->intTime,
                           d_raw, d_cno);
        BDS_HIP(ctx, hipGetLastError());
        BDS_HIP(ctx, hipMemcpyAsync(cno5, d_cno, sizeof(double) * 5 * out_plane, hipMemcpyDeviceToHost, st(ctx)));
        BDS_HIP(ctx, hipStreamSynchronize(st(ctx)));
        return BDS_OK;
    }
    // the post-pass of a session: one k_trk_cno_seg per piece, the carry buffers as bds_track_open* makes them
    BDS_HIP(ctx, scope.alloc(&d_carry, sizeof(double) * (size_t)n_ch * 4 * M));
    BDS_HIP(ctx, scope.alloc(&d_prev3, sizeof(double) * (size_t)n_ch * 3));
    BDS_HIP(ctx, scope.alloc(&d_ncarry, sizeof(int) * (size_t)n_ch));
    BDS_HIP(ctx, hipMemsetAsync(d_carry, 0, sizeof(double) * (size_t)n_ch * 4 * M, st(ctx)));
    BDS_HIP(ctx, hipMemsetAsync(d_prev3, 0, sizeof(double) * (size_t)n_ch * 3, st(ctx)));
    BDS_HIP(ctx, hipMemsetAsync(d_ncarry, 0, sizeof(int) * (size_t)n_ch, st(ctx)));
    std::fill(cno5, cno5 + 5 * out_plane, 0.0);
    std::vector<int> q_done(n_ch, 0);
    std::vector<double> h;
    int e0 = 0;
    for (int i = 0; i < n_pieces; ++i) {
        const int len = pieces[i];
        int nq = 1;  // (bds_track_advance: the most intervals a channel can complete in the call, at least one slot)
        for (int c = 0; c < n_ch; ++c) {
            const int before = std::min(done[c], e0);
            hs[c].completed = std::max(0, std::min(done[c] - e0, len));  // epochs the channel ran in this piece
            nq = std::max(nq, (before + len) / M - before / M);
        }
        // the piece's arrays are epochs [e0, e0 + len) of the caller's rows (row length n_epochs)
        TrkOut d{};
        d.I_P = d_p + e0, d.Q_P = d_p + ne + e0, d.Pilot_I_P = d_p + 2 * ne + e0, d.Pilot_Q_P = d_p + 3 * ne + e0;
        BDS_HIP(ctx, hipMemcpyAsync(d_st, hs.data(), sizeof(ChanState) * n_ch, hipMemcpyHostToDevice, st(ctx)));
        hipLaunchKernelGGL(k_trk_cno_seg, dim3(n_ch), dim3(256), 0, st(ctx), d, (const ChanState *)d_st, n_epochs, M, nq, pm, s->intTime,
                           d_carry, d_ncarry, d_prev3, d_raw, d_cno);
        BDS_HIP(ctx, hipGetLastError());
        h.resize((size_t)n_ch * nq * 5);
        BDS_HIP(ctx, hipMemcpyAsync(h.data(), d_cno, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st(ctx)));
        BDS_HIP(ctx, hipStreamSynchronize(st(ctx)));  // (hs and h are reused by the next piece)
        for (int c = 0; c < n_ch; ++c) {
            const int before = std::min(done[c], e0);
            const int nd = (before + hs[c].completed) / M - before / M;
            for (int q = 0; q < nd && q_done[c] + q < n_cno; ++q)
                for (int f = 0; f < 5; ++f)
                    cno5[f * out_plane + (size_t)c * n_cno + q_done[c] + q] = h[(size_t)f * n_ch * nq + (size_t)c * nq + q];
            q_done[c] += nd;
        }
        e0 += len;
    }
    return BDS_OK;
}

// Test aid (bds_track_update): k_trk_update for ONE epoch on the caller's channel states and correlator sums (nblocks = 1: the
// fixed-order sum of the partial sums returns the 18 values given), the record bounds set so the epoch lies inside the window.
extern "C" int bds_track_update(bds_ctx *ctx, const bds_settings *s, int n_ch, const double *state10, const double *sums18,
                                double *state10_out, int32_t *active, int32_t *completed, double *out21) {
    if (!ctx) return BDS_ERR_ARG;
    if (!s || !state10 || !sums18 || !state10_out || !active || !completed || !out21 || n_ch < 1)
        return fail(ctx, BDS_ERR_ARG, "bds_track_update: missing argument");
    TrkParams p{};
    int rc = fill_params(ctx, *s, p, 1, 0);
    if (rc) return rc;
    p.n_bytes = 1LL << 60, p.base = 0, p.win_end = p.n_bytes;  // no end of file, everything resident
    static_assert(offsetof(ChanState, pos) == 10 * sizeof(double), "the ten doubles of ChanState come first");
    std::vector<ChanState> hs(n_ch);
    for (int c = 0; c < n_ch; ++c) {
        hs[c] = ChanState{};
        memcpy(&hs[c], state10 + (size_t)c * 10, sizeof(double) * 10);
        // the state an epoch starts in gives a block length (epoch_geom); one that cannot was stopped by the update before it
        if (!(std::isfinite(hs[c].codeFreq) && hs[c].codeFreq > 0 && std::isfinite(hs[c].remCodePhase) && hs[c].remCodePhase < p.code_len))
            return fail(ctx, BDS_ERR_ARG, "bds_track_update: state of channel %d has no block length (codeFreq, remCodePhase)", c);
        hs[c].prn = 1, hs[c].active = 1;
    }
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    DevScope scope;
    ChanState *d_st = nullptr;
    double *d_part = nullptr;
    BDS_HIP(ctx, scope.alloc(&d_st, sizeof(ChanState) * n_ch));
    BDS_HIP(ctx, scope.alloc(&d_part, sizeof(double) * (size_t)n_ch * kNSums));
    TrkResults res;  // [21][n_ch] (one epoch), at the reference's template values
    if ((rc = res.prepare(ctx, n_ch, 1))) return rc;
    BDS_HIP(ctx, hipMemcpyAsync(d_st, hs.data(), sizeof(ChanState) * n_ch, hipMemcpyHostToDevice, st(ctx)));
    BDS_HIP(ctx, hipMemcpyAsync(d_part, sums18, sizeof(double) * (size_t)n_ch * kNSums, hipMemcpyHostToDevice, st(ctx)));
    if (!ctx->trk) ctx->trk = new TrackState();
    TrkRun run{ctx, *ctx->trk, p, d_st, d_part, (size_t)n_ch * kNSums, res.d, res.d_out, 1, n_ch, false, d_st};
    run.launch_update(d_st, d_part, 0);
    BDS_HIP(ctx, hipGetLastError());
    BDS_HIP(ctx, hipMemcpyAsync(hs.data(), d_st, sizeof(ChanState) * n_ch, hipMemcpyDeviceToHost, st(ctx)));
    BDS_HIP(ctx, hipMemcpyAsync(out21, res.d_fields, sizeof(double) * (size_t)n_ch * TrkResults::kFields, hipMemcpyDeviceToHost, st(ctx)));
    BDS_HIP(ctx, hipStreamSynchronize(st(ctx)));
    for (int c = 0; c < n_ch; ++c) {
        memcpy(state10_out + (size_t)c * 10, &hs[c], sizeof(double) * 10);
        active[c] = hs[c].active;
        completed[c] = hs[c].completed;
    }
    return BDS_OK;
}

BDS_DEBUG_TU_READER(bds_debug_failures_track)
