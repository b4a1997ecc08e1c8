// What the tracking correlators (bds_track.hip) and the correlation-function kernel (bds_corrfn.hip) share: the sample
// formats of the IF record and their decode, the geometry of the per-PRN code tables, the reference's replica index vectors
// (MATLAB colon vectors) with the exact search of an index step's first sample, and the wave-level f64 scan.
// Device code of translation units built with -ffp-contract=off (one rounding per operation, as written).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace bds {

static constexpr size_t kDataSlack = 256;  // bytes past the record a segment's aligned dword reads may touch

// Sample formats of the IF record.  Packed (the input of B2a/include/unpack_cplx.m:18-30): complex sample n is nibble n & 1 of
// byte n >> 1, low nibble first; per nibble bit 0 / 1 = I / Q negative, bit 2 / 3 = |I| / |Q| is 3 (else 1).
// 16-bit records (settings.dataType 1): little-endian int16 samples (fileType 1) or interleaved I, Q int16 pairs (fileType 2).
enum : int { kFmtReal = 0, kFmtIQ = 1, kFmtPacked = 2, kFmtReal16 = 3, kFmtIQ16 = 4 };
__host__ __device__ constexpr int fmt_align(int fmt) { return fmt == kFmtPacked ? 32 : 16; }  // samples: 16 bytes at least
// bytes of one sample of an unpacked format
__host__ __device__ constexpr int fmt_bps(int fmt) { return fmt == kFmtIQ16 ? 4 : fmt == kFmtIQ || fmt == kFmtReal16 ? 2 : 1; }
__host__ __device__ constexpr bool fmt_complex(int fmt) { return fmt == kFmtIQ || fmt == kFmtPacked || fmt == kFmtIQ16; }
__host__ __device__ constexpr bool fmt_16bit(int fmt) { return fmt == kFmtReal16 || fmt == kFmtIQ16; }
// bytes of n samples (packed: n even -- window and span bounds are kept even, the file itself holds whole bytes)
__host__ __device__ constexpr long long fmt_bytes(int fmt, long long n) { return fmt == kFmtPacked ? n / 2 : n * fmt_bps(fmt); }
// samples in n bytes (whole ones: a trailing part of a sample or pair does not count)
__host__ __device__ constexpr long long fmt_samples(int fmt, long long n) { return fmt == kFmtPacked ? n * 2 : n / fmt_bps(fmt); }
// one packed byte -> the int8 quadruple (I1, Q1, I2, Q2) unpack_cplx writes for it, without a branch: magnitudes 1 | 2 bit,
// then two's complement in every byte whose sign bit is set ((m ^ 0xff) + 1 never carries out of a byte for m = 1, 3)
__device__ __forceinline__ uint32_t iq_of_packed(uint32_t b) {
    const uint32_t sg = (b & 1u) | ((b & 2u) << 7) | ((b & 0x10u) << 12) | ((b & 0x20u) << 19);
    const uint32_t mg = 0x01010101u | ((b & 4u) >> 1) | ((b & 8u) << 6) | ((b & 0x40u) << 11) | ((b & 0x80u) << 18);
    return (mg ^ (sg * 0xffu)) + sg;
}

// Geometry of the per-PRN code tables (bds_track.hip, ensure_prim): two slots of kTabStride bytes per PRN -- slot 0 the (data,
// pilot) pairs at the look-up's own resolution, slot 1 the pilot BOC(6,1) --, each with kTabPad wrapped entries on both sides:
// entry kTabPad + (u - 1) holds unit u (1-based) of the code.
static constexpr int kTabPad = 32;
static constexpr long kTabStride = 122880;  // >= 12 * 10230 + 2 * kTabPad, multiple of 64

// The reference's replica index vectors are MATLAB colon vectors,
//     tcode = (rem -+ spc)[*2] : step[*2] : ((blksize-1)*step + rem -+ spc)[*2]     (tracking.m:260-286, NB_tracking.m:271-297,
//                                                                                      WB_tracking.m:289-317),
// and MATLAB does not build a:d:b as a + k d throughout (MathWorks' published colonop.m, Technical Solution 1-4FLI96): with
// n = round((b-a)/d) intervals (one less if a + n d overshoots b by more than tol = 2 eps max(|a|,|b|)) and the right end
// c = a + n d snapped to b within tol, elements 0 .. floor(n/2) are a + k d, the elements after them c - (n-k) d -- generated from
// the RIGHT end --, and the mid-point of an even n is (a+c)/2.  The second half differs from a + k d by 0-2 ulp of tcode, which
// moves ceil() for a sample that sits on a chip boundary to rounding (round 6; oracle/matlab.py m_colon is the checker's copy).
struct ColonVec {
    double a, d, c;
    int n, h;
    bool even;
};
// (also compiled for the host: bds_corrfn.hip counts a tap's elements there before it launches anything)
__host__ __device__ __forceinline__ ColonVec colon_vec(double a, double d, double b) {
    ColonVec v;
    const double tol = 2.0 * 2.220446049250313e-16 * fmax(fabs(a), fabs(b));
    long n = (long)floor((b - a) / d + 0.5);  // MATLAB round() of a non-negative quotient (the tcode vectors ascend)
    if (a + (double)n * d - b > tol) n -= 1;
    double c = a + (double)n * d;
    if (c - b > -tol) c = b;
    v.a = a, v.d = d, v.c = c, v.n = (int)n, v.h = (int)(n / 2), v.even = (n & 1) == 0;
    return v;
}
__device__ __forceinline__ double colon_at(const ColonVec &v, int k) {
    const double fwd = v.a + (double)k * v.d, bwd = v.c - (double)(v.n - k) * v.d;
    return k > v.h ? bwd : (v.even && k == v.h) ? (v.a + v.c) / 2 : fwd;
}

template <int R6>
__device__ __forceinline__ double code_arg(const ColonVec &v, int k) {
    double t = colon_at(v, k);  // element k of the reference's colon vector (-ffp-contract=off: one rounding per operation)
    if (R6) t = t * 6;
    return t;
}

// first k in (k_lo, k_hi] with ceil(arg(k)) >= u, given ceil(arg(k_lo)) < u <= ceil(arg(k_hi))
template <int R6>
__device__ __forceinline__ int first_sample_of(const ColonVec &v, double inv_inc, int u, int k_lo, int k_hi) {
    const double thr = (double)(u - 1);  // ceil(t) >= u  <=>  t > u - 1
    const double tgt = R6 ? thr * (1.0 / 6.0) : thr;  // a prediction only: confirmed below with the exact expression
    int kc = (int)floor((tgt - v.a) * inv_inc) + 1;
    kc = max(k_lo + 1, min(kc, k_hi));
    while (kc > k_lo + 1 && code_arg<R6>(v, kc - 1) > thr) --kc;
    while (kc < k_hi && !(code_arg<R6>(v, kc) > thr)) ++kc;
    return kc;
}

__device__ __forceinline__ void wave_sync() {  // LDS written by this wave is read by other lanes of this wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 64-lane inclusive f64 add-scan on the DPP network (row shifts inside the 16-lane rows, then the row
// broadcasts): 3 instructions per step instead of two LDS-pipe permutes; lane 63 ends up with the total
template <int CTRL, int ROW_MASK, bool BOUND>
__device__ __forceinline__ double dpp_f64(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, BOUND);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, BOUND);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_scan_incl(double v) {
    v += dpp_f64<0x111, 0xf, true>(v);   // row_shr:1
    v += dpp_f64<0x112, 0xf, true>(v);   // row_shr:2
    v += dpp_f64<0x114, 0xf, true>(v);   // row_shr:4
    v += dpp_f64<0x118, 0xf, true>(v);   // row_shr:8
    v += dpp_f64<0x142, 0xa, false>(v);  // row_bcast:15 into rows 1, 3
    v += dpp_f64<0x143, 0xc, false>(v);  // row_bcast:31 into rows 2, 3
    return v;
}
__device__ __forceinline__ double lane_f64(double v, int l) {  // broadcast of lane l (compile-time constant)
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

}  // namespace bds
