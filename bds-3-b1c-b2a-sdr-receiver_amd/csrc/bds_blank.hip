// Pulse blanking of an IF record on the device (include/bds_mi355x.h "pulse blanking"): every sample within
// [m - pre, m + post] of a flagged sample m (x^2 or I^2 + Q^2 above threshold_sq) is set to 0, on the record's own bytes.
//   k_blank_summary  per tile of kTile samples: first and last flagged index (or none) and the flagged count of the window
//   k_blank_scan_group, k_blank_scan   exclusive forward max-scan of "last flagged" and backward min-scan of "first flagged" over the
//                    tile summaries, in two levels (inside groups of 1024 tiles, then over the groups), and the sum of the flagged counts
//   k_blank_apply    a workgroup reads ONLY ITS OWN TILE'S raw samples (in place, a neighbour may already have zeroed its own) plus
//                    the scanned summaries; it redoes the scans of the flagged indices inside the tile -- per wave with
//                    shuffles, across the waves through LDS --, decides n - last <= post || next - n <= pre per sample, writes and counts
//   k_blank_sum      adds the tiles' blanked and run counts up
// A tile's bytes are its whole aligned 16-byte lines (16-byte loads and stores) and, where the record's address or its end leaves a
// line partly outside the tile, that line's own bytes one by one.  Lines are address-aligned, tiles sample-aligned: a sample that
// straddles two lines of a tile gets its upper bytes from the next line's thread through LDS, and no tile touches another's bytes.
// Integer arithmetic throughout; the only atomics are the int32 adds of the duty bins.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bds_blank_math.h"
#include "bds_internal.h"

namespace bds {
namespace blank {

constexpr int kNone = 1 << 30;  // tile-relative "no flagged sample behind" (in front: -1)

struct Args {
    const uint8_t *in;
    uint8_t *out;
    int64_t n, w0, w1;  // samples of the buffer; the window [lead, n - tail) that is written and counted
    uint32_t thr;
    Fast8 f8;
    int pre, post;
    int A;         // address of `in` modulo 16: line c holds the bytes [16 c - A, 16 c - A + 16) of the buffer
    int vec_out;   // `out` has the same address modulo 16: whole lines are stored as one 16-byte word
    int inplace;
    int64_t duty_samples, duty_origin;  // sample k of the window counts into bin (k - w0 + duty_origin) / duty_samples
    int32_t *duty;
    int64_t *first, *last;              // per tile, absolute indices (kNoNext / kNoLast: none)
    const int64_t *prev_last, *next_first;  // inside the tile's group of kGroup tiles ...
    const int64_t *g_prev, *g_next;         // ... and over the groups in front of it / behind it
    uint32_t *n_flag, *n_blank, *n_run;  // per tile
};

// ---- a tile's lines -------------------------------------------------------------------------------------------------------------------
// In "shifted" byte offsets (offset in the buffer + A) line c is [16 c, 16 c + 16) and sample k starts at A + k SB.
template <int SB>
struct Tile {
    int64_t lo, hi;      // samples
    int64_t s_lo, s_hi;  // shifted bytes
    int64_t c_lo, c_hi;  // lines (c_hi inclusive)
    int ph;              // position of the sample starts inside a line, modulo SB
    __device__ Tile(const Args &a, int64_t t) {
        lo = t * kTile;
        hi = lo + kTile < a.n ? lo + kTile : a.n;
        s_lo = a.A + lo * SB, s_hi = a.A + hi * SB;
        c_lo = s_lo >> 4, c_hi = (s_hi - 1) >> 4;
        ph = a.A & (SB - 1);
    }
    // the bytes of line c that are the tile's, as a 16-bit mask
    __device__ unsigned owned(int64_t c) const {
        const int64_t b = c << 4;
        const int f = s_lo > b ? (int)(s_lo - b) : 0, e = s_hi < b + 16 ? (int)(s_hi - b) : 16;
        return e > f ? ((0xffffu >> (16 - e)) & (0xffffu << f)) & 0xffffu : 0u;
    }
    // index of the sample that starts at position ph of line c (may lie outside the tile, below 0 in the record's first line)
    __device__ int64_t k_base(const Args &a, int64_t c) const { return ((c << 4) + ph - a.A) / SB; }
};
__device__ __forceinline__ unsigned bits_between(int64_t from, int64_t to, int n_slots) {  // slots i with from <= i < to, i < n_slots
    const int f = from > 0 ? (from < n_slots ? (int)from : n_slots) : 0, e = to > 0 ? (to < n_slots ? (int)to : n_slots) : 0;
    return e > f ? ((1u << e) - 1u) & ~((1u << f) - 1u) : 0u;
}

__device__ __forceinline__ uint4 load_line(const uint8_t *pb, int64_t c, unsigned own) {
    if (own == 0xffffu) return *reinterpret_cast<const uint4 *>(pb + (c << 4));
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < 16; ++b)
        if (own >> b & 1u) w[b >> 2] |= (uint32_t)pb[(c << 4) + b] << (8 * (b & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ void store_line(uint8_t *pb, int64_t c, unsigned own, bool vec, uint4 q) {
    if (own == 0xffffu && vec) {
        *reinterpret_cast<uint4 *>(pb + (c << 4)) = q;
        return;
    }
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int b = 0; b < 16; ++b)
        if (own >> b & 1u) pb[(c << 4) + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
}

// flagged samples among the 16 / SB that start in a line (bit i: the sample at byte ph + i SB); nx = the next line's first word.
// The general form takes every sample out of the line and applies flagged(); PH0: the samples start at the line's byte 0.
template <int SB, int E, bool PH0>
__device__ __forceinline__ unsigned flag_mask_general(const uint32_t (&w)[5], int ph, uint32_t thr) {
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < 16 / SB; ++i) {
        const int d = (i * SB) >> 2;
        uint32_t v;
        if (PH0) {
            v = w[d] >> (8 * ((i * SB) & 3));
        } else {
            const uint64_t two = ((uint64_t)w[d + 1] << 32) | w[d];
            v = (uint32_t)(two >> (8 * (((i * SB) & 3) + ph)));
        }
        int re, im = 0;
        if (E == 1) {
            re = (int8_t)(v & 0xffu);
            if (SB == 2) im = (int8_t)((v >> 8) & 0xffu);
        } else {
            re = (int16_t)(v & 0xffffu);
            if (SB == 4) im = (int16_t)(v >> 16);
        }
        m |= flagged(re, im, thr) ? 1u << i : 0u;
    }
    return m;
}
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
// The int8 records at their usual alignment, four (real) or two (pairs) samples per 32-bit word at a time; the same verdicts as
// flagged() (bds_blank_math.h: Fast8 says why), which the general form keeps for every other case.
template <int SB, int E>
__device__ __forceinline__ unsigned flag_mask(uint4 q, uint32_t nx, int ph, uint32_t thr, const Fast8 &f8) {
    const uint32_t w[5] = {q.x, q.y, q.z, q.w, nx};
    if (ph) return flag_mask_general<SB, E, false>(w, ph, thr);
    if (SB == 1) {
        unsigned m = 0;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint32_t x = w[d], s01 = (x >> 7) & 0x01010101u, sm = (s01 << 8) - s01;  // sm: 0xff in the bytes that are negative
            const uint32_t mag = (x ^ sm) + s01;                                           // |x| per byte, 0 .. 128: no carry between bytes
            const uint32_t g = ((mag + f8.add) & f8.mask) >> 7;                            // bit 0 / 8 / 16 / 24: |x| > t
            m |= ((g | (g >> 7) | (g >> 14) | (g >> 21)) & 15u) << (4 * d);
        }
        return m;
    }
    if (SB == 2 && E == 1) {
        if (!f8.any16) return 0u;
        unsigned m = 0;
        const unsigned short t16 = (unsigned short)f8.thr16;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            s16x2 v;
            __builtin_memcpy(&v, &w[d], 4);
            const s16x2 re = (s16x2)(v << 8) >> 8, im = v >> 8;                 // low byte I, high byte Q of each pair, sign-extended
            const u16x2 p = (u16x2)(re * re) + (u16x2)(im * im);               // at most 2 * 128^2 = 2^15
            const u16x2 dif = (u16x2){t16, t16} - p;                           // bit 15: p > threshold_sq (both below 2^15 + 1)
            uint32_t u;
            __builtin_memcpy(&u, &dif, 4);
            m |= (((u >> 15) & 1u) | ((u >> 30) & 2u)) << (2 * d);
        }
        return m;
    }
    return flag_mask_general<SB, E, true>(w, 0, thr);
}

// m | m << 1 | ... | m << p (p <= 16; uniform)
__device__ __forceinline__ unsigned smear_up(unsigned m, int p) {
    for (int span = 0; span < p;) {
        const int step = span + 1 < p - span ? span + 1 : p - span;
        m |= m << step, span += step;
    }
    return m;
}
__device__ __forceinline__ unsigned smear_down(unsigned m, int p) {
    for (int span = 0; span < p;) {
        const int step = span + 1 < p - span ? span + 1 : p - span;
        m |= m >> step, span += step;
    }
    return m;
}
template <int SB>
__device__ __forceinline__ unsigned slots_to_bytes(unsigned bits) {  // bit i -> bits i SB .. i SB + SB - 1
    if (SB == 1) return bits;
    unsigned x = bits;
    if (SB == 2) {
        x = (x | (x << 4)) & 0x0f0fu, x = (x | (x << 2)) & 0x3333u, x = (x | (x << 1)) & 0x5555u;
        return x * 3u;
    }
    x = (x | (x << 6)) & 0x0303u, x = (x | (x << 3)) & 0x1111u;
    return x * 15u;
}
__device__ __forceinline__ uint32_t byte_mask(unsigned nib) {  // 4 bits -> 4 bytes
    return ((nib & 1u) ? 0xffu : 0u) | ((nib & 2u) ? 0xff00u : 0u) | ((nib & 4u) ? 0xff0000u : 0u) | ((nib & 8u) ? 0xff000000u : 0u);
}

template <int SB>
constexpr int lines_per_thread() { return kTile * SB / 16 / 256 + 1; }  // (+ 1: a tile that starts inside a line ends inside one more)

// ---- summary ----------------------------------------------------------------------------------------------------------------------------
template <int SB, int E>
__global__ __launch_bounds__(256) void k_blank_summary(Args a) {
    constexpr int R = lines_per_thread<SB>(), NS = 16 / SB;
    __shared__ uint32_t sh_dw[R * 256 + 1];
    __shared__ int sh_f[4], sh_l[4];
    __shared__ unsigned sh_n[4];
    const int tid = threadIdx.x;
    const Tile<SB> T(a, blockIdx.x);
    const uint8_t *pb = a.in - a.A;
    uint4 q[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t c = T.c_lo + r * 256 + tid;
        q[r] = c <= T.c_hi ? load_line(pb, c, T.owned(c)) : make_uint4(0, 0, 0, 0);
        if (T.ph) sh_dw[r * 256 + tid] = q[r].x;
    }
    if (T.ph) {
        if (tid == 0) sh_dw[R * 256] = 0;
        __syncthreads();
    }
    int f = kNone, l = -1;
    unsigned cnt = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t c = T.c_lo + r * 256 + tid, kb = T.k_base(a, c);
        const unsigned m = flag_mask<SB, E>(q[r], T.ph ? sh_dw[r * 256 + tid + 1] : 0u, T.ph, a.thr, a.f8) & bits_between(T.lo - kb, T.hi - kb, NS);
        if (m) {
            const int rel = (int)(kb - T.lo);
            f = min(f, rel + __ffs((int)m) - 1), l = max(l, rel + 31 - __clz((int)m));
            cnt += __popc(m & bits_between(a.w0 - kb, a.w1 - kb, NS));
        }
    }
    for (int d = 32; d; d >>= 1) f = min(f, __shfl_xor(f, d)), l = max(l, __shfl_xor(l, d)), cnt += __shfl_xor(cnt, d);
    if ((tid & 63) == 0) sh_f[tid >> 6] = f, sh_l[tid >> 6] = l, sh_n[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) f = min(f, sh_f[w]), l = max(l, sh_l[w]), cnt += sh_n[w];
        a.first[blockIdx.x] = f < kNone ? T.lo + f : kNoNext;
        a.last[blockIdx.x] = l >= 0 ? T.lo + l : kNoLast;
        a.n_flag[blockIdx.x] = cnt;
    }
}

// ---- scan over the tiles ------------------------------------------------------------------------------------------------------------------
// Two levels.  k_blank_scan_group: a workgroup takes kGroup consecutive tiles, one per thread, and leaves per tile the exclusive
// maximum of last[] in front of it and minimum of first[] behind it INSIDE the group, and per group the three totals.
// k_blank_scan (one workgroup) does the same over the groups' totals.  The apply kernel joins the two levels.
constexpr int kGroup = 1024;
__global__ __launch_bounds__(kGroup) void k_blank_scan_group(const int64_t *__restrict__ first, const int64_t *__restrict__ last, const uint32_t *__restrict__ n_flag,
                                                             int64_t nt, int64_t *__restrict__ prev_last, int64_t *__restrict__ next_first,
                                                             int64_t *__restrict__ g_first, int64_t *__restrict__ g_last, uint32_t *__restrict__ g_flag) {
    __shared__ long long sh_mx[16], sh_mn[16];
    __shared__ unsigned sh_s[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t j = (int64_t)blockIdx.x * kGroup + tid;
    long long imx = j < nt ? (long long)last[j] : (long long)kNoLast, imn = j < nt ? (long long)first[j] : (long long)kNoNext;
    unsigned s = j < nt ? n_flag[j] : 0u;
    for (int d = 1; d < 64; d <<= 1) {
        const long long u = __shfl_up(imx, d), v = __shfl_down(imn, d);
        if (lane >= d) imx = max(imx, u);
        if (lane + d < 64) imn = min(imn, v);
    }
    for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 63) sh_mx[wv] = imx;
    if (lane == 0) sh_mn[wv] = imn, sh_s[wv] = s;
    long long emx = __shfl_up(imx, 1), emn = __shfl_down(imn, 1);
    if (lane == 0) emx = kNoLast;
    if (lane == 63) emn = kNoNext;
    __syncthreads();
    for (int w = 0; w < wv; ++w) emx = max(emx, sh_mx[w]);
    for (int w = wv + 1; w < 16; ++w) emn = min(emn, sh_mn[w]);
    if (j < nt) prev_last[j] = emx, next_first[j] = emn;
    if (tid == 0) {
        long long mx = kNoLast, mn = kNoNext;
        unsigned tot = 0;
        for (int w = 0; w < 16; ++w) mx = max(mx, sh_mx[w]), mn = min(mn, sh_mn[w]), tot += sh_s[w];
        g_last[blockIdx.x] = mx, g_first[blockIdx.x] = mn, g_flag[blockIdx.x] = tot;  // (at most 1024 x 16384 flagged samples: fits 32 bits)
    }
}
// prev_last[t] = max of last[u], u < t; next_first[t] = min of first[u], u > t; *n_flagged = sum of n_flag.  One workgroup of 1024.
__global__ __launch_bounds__(1024) void k_blank_scan(const int64_t *__restrict__ first, const int64_t *__restrict__ last, const uint32_t *__restrict__ n_flag,
                                                      int64_t nt, int64_t *__restrict__ prev_last, int64_t *__restrict__ next_first,
                                                      unsigned long long *__restrict__ n_flagged) {
    __shared__ long long sh_mx[16], sh_mn[16];
    __shared__ unsigned long long sh_s[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t chunk = (nt + 1023) / 1024, lo = std::min<int64_t>(nt, tid * chunk), hi = std::min<int64_t>(nt, lo + chunk);
    long long mx = kNoLast, mn = kNoNext;
    unsigned long long s = 0;
    for (int64_t j = lo; j < hi; ++j) mx = max(mx, (long long)last[j]), mn = min(mn, (long long)first[j]), s += n_flag[j];
    long long imx = mx, imn = mn;
    for (int d = 1; d < 64; d <<= 1) {
        const long long u = __shfl_up(imx, d), v = __shfl_down(imn, d);
        if (lane >= d) imx = max(imx, u);
        if (lane + d < 64) imn = min(imn, v);
    }
    for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 63) sh_mx[wv] = imx;
    if (lane == 0) sh_mn[wv] = imn, sh_s[wv] = s;
    long long emx = __shfl_up(imx, 1), emn = __shfl_down(imn, 1);
    if (lane == 0) emx = kNoLast;
    if (lane == 63) emn = kNoNext;
    __syncthreads();
    for (int w = 0; w < wv; ++w) emx = max(emx, sh_mx[w]);
    for (int w = wv + 1; w < 16; ++w) emn = min(emn, sh_mn[w]);
    for (int64_t j = lo; j < hi; ++j) prev_last[j] = emx, emx = max(emx, (long long)last[j]);
    for (int64_t j = hi - 1; j >= lo; --j) next_first[j] = emn, emn = min(emn, (long long)first[j]);
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) s += sh_s[w];
        *n_flagged = s;
    }
}

// the tiles' blanked and run counts added up: a workgroup per 4096 tiles, one 64-bit integer atomic add each (out zeroed before)
__global__ __launch_bounds__(1024) void k_blank_sum(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, int64_t nt,
                                                     unsigned long long *__restrict__ out_a, unsigned long long *__restrict__ out_b) {
    __shared__ unsigned long long sh[2][16];
    unsigned long long sa = 0, sb = 0;
    const int64_t base = (int64_t)blockIdx.x * 4096;
    for (int64_t j = base + threadIdx.x; j < nt && j < base + 4096; j += 1024) sa += a[j], sb += b[j];
    for (int d = 32; d; d >>= 1) sa += __shfl_xor(sa, d), sb += __shfl_xor(sb, d);
    if ((threadIdx.x & 63) == 0) sh[0][threadIdx.x >> 6] = sa, sh[1][threadIdx.x >> 6] = sb;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) sa += sh[0][w], sb += sh[1][w];
        if (sa) atomicAdd(out_a, sa);
        if (sb) atomicAdd(out_b, sb);
    }
}

// ---- apply ------------------------------------------------------------------------------------------------------------------------------
template <int SB, int E>
__global__ __launch_bounds__(256) void k_blank_apply(Args a) {
    constexpr int R = lines_per_thread<SB>(), NS = 16 / SB, NW = 4 * R;
    __shared__ uint32_t sh_dw[R * 256 + 1];
    __shared__ int sh_wl[NW], sh_wf[NW], sh_xl[NW], sh_xf[NW];
    __shared__ unsigned sh_cnt[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t t = blockIdx.x;
    const Tile<SB> T(a, t);
    const int64_t prev = max((long long)a.prev_last[t], (long long)a.g_prev[t / kGroup]), next = min((long long)a.next_first[t], (long long)a.g_next[t / kGroup]);
    const bool own_flags = a.first[t] != kNoNext;
    // nothing of the tile is blanked: no flagged sample in it, none in reach in front of it or behind it
    const bool untouched = !own_flags && T.lo - prev > a.post && next - (T.hi - 1) > a.pre;
    if (untouched && tid == 0) a.n_blank[t] = 0, a.n_run[t] = 0;
    if (untouched && a.inplace) return;
    const uint8_t *pb = a.in - a.A;
    uint8_t *ob = a.out - a.A;  // (with vec_out the same line grid; without, store_line goes byte by byte and any base serves)
    uint4 q[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t c = T.c_lo + r * 256 + tid;
        q[r] = c <= T.c_hi ? load_line(pb, c, T.owned(c)) : make_uint4(0, 0, 0, 0);
    }
    if (untouched) {  // out of place: a copy
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t c = T.c_lo + r * 256 + tid;
            if (c <= T.c_hi) store_line(ob, c, T.owned(c), a.vec_out, q[r]);
        }
        return;
    }
    if (T.ph) {
#pragma unroll
        for (int r = 0; r < R; ++r) sh_dw[r * 256 + tid] = q[r].x;
        if (tid == 0) sh_dw[R * 256] = 0;
        __syncthreads();
    }
    // flagged samples per line; per wave the inclusive forward max-scan of "last flagged" and backward min-scan of "first flagged",
    // tile-relative (-1 / kNone: none), shifted by one lane to the exclusive values
    unsigned m[R];
    int exl[R], exn[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t c = T.c_lo + r * 256 + tid, kb = T.k_base(a, c);
        m[r] = flag_mask<SB, E>(q[r], T.ph ? sh_dw[r * 256 + tid + 1] : 0u, T.ph, a.thr, a.f8) & bits_between(T.lo - kb, T.hi - kb, NS);
        const int rel = (int)(kb - T.lo);
        int il = m[r] ? rel + 31 - __clz((int)m[r]) : -1, inx = m[r] ? rel + __ffs((int)m[r]) - 1 : kNone;
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(il, d), v = __shfl_down(inx, d);
            if (lane >= d) il = max(il, u);
            if (lane + d < 64) inx = min(inx, v);
        }
        if (lane == 63) sh_wl[r * 4 + wv] = il;
        if (lane == 0) sh_wf[r * 4 + wv] = inx;
        exl[r] = __shfl_up(il, 1), exn[r] = __shfl_down(inx, 1);
        if (lane == 0) exl[r] = -1;
        if (lane == 63) exn[r] = kNone;
    }
    __syncthreads();
    if (tid < NW) {  // across the waves, in line order r * 4 + wave
        int l = -1, f = kNone;
        for (int j = 0; j < tid; ++j) l = max(l, sh_wl[j]);
        for (int j = tid + 1; j < NW; ++j) f = min(f, sh_wf[j]);
        sh_xl[tid] = l, sh_xf[tid] = f;
    }
    __syncthreads();
    // the tile's window bins, when they are one: a single add per tile
    const int64_t kk0 = T.lo > a.w0 ? T.lo : a.w0, kk1 = (T.hi < a.w1 ? T.hi : a.w1) - 1;
    int64_t bin0 = 0, bin1 = 0;
    uint32_t rem0 = 0;
    const bool duty = a.duty && kk1 >= kk0;
    if (duty) {
        const int64_t i0 = kk0 - a.w0 + a.duty_origin;
        bin0 = i0 / a.duty_samples, bin1 = (kk1 - a.w0 + a.duty_origin) / a.duty_samples;
        rem0 = (uint32_t)(i0 - bin0 * a.duty_samples);
    }
    unsigned n_blank = 0, n_run = 0;
    const int p_up = a.post < 16 ? a.post : 16, p_dn = a.pre < 16 ? a.pre : 16;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t c = T.c_lo + r * 256 + tid;
        if (c > T.c_hi) continue;
        const int64_t kb = T.k_base(a, c);
        const int el = max(exl[r], sh_xl[r * 4 + wv]), en = min(exn[r], sh_xf[r * 4 + wv]);
        const int64_t last = el >= 0 ? T.lo + el : prev, nxt = en < kNone ? T.lo + en : next;  // flagged in front of / behind this line
        const unsigned valid = bits_between(T.lo - kb, T.hi - kb, NS), win = bits_between(a.w0 - kb, a.w1 - kb, NS);
        // slot i is sample kb + i: in reach of `last` up to i = post - (kb - last), of `nxt` from i = (nxt - kb) - pre on
        const int64_t x = a.post - (kb - last), y = (nxt - kb) - a.pre;
        unsigned b = smear_up(m[r], p_up) | smear_down(m[r], p_dn);
        b |= x < 0 ? 0u : x >= 15 ? 0xffffu : (2u << (int)x) - 1u;
        b |= y > 15 ? 0u : y <= 0 ? 0xffffu : 0xffffu << (int)y;
        b &= valid;
        // the sample in front of the line's first own one: its state by the same rule, for the run count and for its upper bytes
        const int j0 = valid ? __ffs((int)valid) - 1 : 0;
        const int64_t kp = kb + j0 - 1, nown = m[r] ? kb + __ffs((int)m[r]) - 1 : nxt;
        const bool pb_state = kp >= 0 && blanked(kp, last, nown, a.pre, a.post);
        const unsigned starts = b & ~((b << 1) | ((pb_state ? 1u : 0u) << j0)) & win;
        const unsigned bw = b & win;
        n_blank += __popc(bw), n_run += __popc(starts);
        const unsigned own = T.owned(c);
        unsigned zb = (slots_to_bytes<SB>(bw) << T.ph) & 0xffffu;
        if (SB > 1 && T.ph && j0 == 0 && pb_state && kp >= a.w0 && kp < a.w1) zb |= (1u << T.ph) - 1u;
        zb &= own;
        const uint4 z = make_uint4(q[r].x & ~byte_mask(zb & 15u), q[r].y & ~byte_mask((zb >> 4) & 15u), q[r].z & ~byte_mask((zb >> 8) & 15u),
                                   q[r].w & ~byte_mask(zb >> 12));
        if (!a.inplace || z.x != q[r].x || z.y != q[r].y || z.z != q[r].z || z.w != q[r].w) store_line(ob, c, own, a.vec_out, z);
        if (duty && bin0 != bin1)  // bins narrower than the tile: every blanked sample on its own
            for (unsigned rest = bw; rest; rest &= rest - 1) {
                const uint32_t off = (uint32_t)(kb + (__ffs((int)rest) - 1) - kk0) + rem0;  // < kTile + duty_samples < 2^32
                atomicAdd(&a.duty[bin0 + off / (uint32_t)a.duty_samples], 1);
            }
    }
    for (int d = 32; d; d >>= 1) n_blank += __shfl_xor(n_blank, d), n_run += __shfl_xor(n_run, d);
    if (lane == 0) sh_cnt[0][wv] = n_blank, sh_cnt[1][wv] = n_run;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) n_blank += sh_cnt[0][w], n_run += sh_cnt[1][w];
        a.n_blank[t] = n_blank, a.n_run[t] = n_run;
        if (duty && bin0 == bin1 && n_blank) atomicAdd(&a.duty[bin0], (int)n_blank);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------
// per-call (per stream) scratch: the tile summaries, their scans, the per-tile counts and the three totals
struct Scratch {
    int64_t *first = nullptr, *last = nullptr, *prev = nullptr, *next = nullptr;
    int64_t *g_first = nullptr, *g_last = nullptr, *g_prev = nullptr, *g_next = nullptr;  // per group of kGroup tiles
    uint32_t *g_flag = nullptr;
    uint32_t *n_flag = nullptr, *n_blank = nullptr, *n_run = nullptr;
    unsigned long long *totals = nullptr;  // flagged, blanked, runs
    void *block = nullptr;
    hipError_t alloc(int64_t nt) {
        nt = std::max<int64_t>(nt, 1);
        const int64_t ng = (nt + kGroup - 1) / kGroup;
        const size_t bytes = (size_t)nt * (4 * 8 + 3 * 4) + (size_t)ng * (4 * 8 + 4) + 3 * 8 + 64;
        const hipError_t e = hipMalloc(&block, bytes);
        if (e != hipSuccess) return e;
        totals = static_cast<unsigned long long *>(block);
        first = reinterpret_cast<int64_t *>(totals + 4), last = first + nt, prev = last + nt, next = prev + nt;
        g_first = next + nt, g_last = g_first + ng, g_prev = g_last + ng, g_next = g_prev + ng;
        n_flag = reinterpret_cast<uint32_t *>(g_next + ng), n_blank = n_flag + nt, n_run = n_blank + nt, g_flag = n_run + nt;
        return hipSuccess;
    }
    ~Scratch() {
        if (block) (void)hipFree(block);
    }
};
inline int64_t tiles(int64_t n) { return (n + kTile - 1) / kTile; }

template <int SB, int E>
static void launch_t(hipStream_t st, const Args &a, int64_t nt, Scratch &sc) {
    const int64_t ng = (nt + kGroup - 1) / kGroup;
    hipLaunchKernelGGL((k_blank_summary<SB, E>), dim3((unsigned)nt), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_blank_scan_group, dim3((unsigned)ng), dim3(kGroup), 0, st, sc.first, sc.last, sc.n_flag, nt, sc.prev, sc.next, sc.g_first, sc.g_last, sc.g_flag);
    hipLaunchKernelGGL(k_blank_scan, dim3(1), dim3(1024), 0, st, sc.g_first, sc.g_last, sc.g_flag, ng, sc.g_prev, sc.g_next, sc.totals);
    hipLaunchKernelGGL((k_blank_apply<SB, E>), dim3((unsigned)nt), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_blank_sum, dim3((unsigned)((nt + 4095) / 4096)), dim3(1024), 0, st, a.n_blank, a.n_run, nt, sc.totals + 1, sc.totals + 2);
}

static void fill_report(bds_blank_out *rep, int64_t n_window, const bds_blank_opts &o, const unsigned long long tot[3]) {
    rep->n_samples = n_window, rep->n_flagged = (int64_t)tot[0], rep->n_blanked = (int64_t)tot[1], rep->n_runs = (int64_t)tot[2];
    rep->n_duty = duty_bins(n_window, o.duty_samples);
}

}  // namespace blank
}  // namespace bds

#include "bds_piece_pipe.h"  // what the entries share with the other conditioners: their checks, the layout switch, the piece loop

using namespace bds;
using namespace bds::blank;

// One buffer of n samples on the device: [lead, n - tail) is blanked from d_in into d_out (the context copied through when they
// differ), the three totals are left in sc.totals; asynchronous on `st`.  n = 0 launches nothing (the totals are zeroed).
static hipError_t run_device(hipStream_t st, int fmt, const uint8_t *d_in, uint8_t *d_out, int64_t n, int64_t lead, int64_t tail, const bds_blank_opts &o,
                             int32_t *d_duty, int64_t duty_origin, Scratch &sc) {
    const int64_t nt = tiles(n);
    hipError_t e0 = hipMemsetAsync(sc.totals, 0, 3 * 8, st);
    if (nt == 0 || e0 != hipSuccess) return e0;
    Args a{};
    a.in = d_in, a.out = d_out, a.n = n, a.w0 = lead, a.w1 = n - tail;
    a.thr = o.threshold_sq, a.f8 = fast8(o.threshold_sq), a.pre = o.pre, a.post = o.post;
    a.A = (int)(reinterpret_cast<uintptr_t>(d_in) & 15u);
    a.inplace = d_in == d_out;
    a.vec_out = (reinterpret_cast<uintptr_t>(d_out) & 15u) == (uintptr_t)a.A;
    a.duty_samples = d_duty ? o.duty_samples : 0, a.duty_origin = duty_origin, a.duty = o.duty_samples > 0 ? d_duty : nullptr;
    a.first = sc.first, a.last = sc.last, a.prev_last = sc.prev, a.next_first = sc.next, a.g_prev = sc.g_prev, a.g_next = sc.g_next;
    a.n_flag = sc.n_flag, a.n_blank = sc.n_blank, a.n_run = sc.n_run;
    with_sample_layout(fmt, [&](auto sb, auto el) { launch_t<decltype(sb)::value, decltype(el)::value>(st, a, nt, sc); });
    return hipGetLastError();
}

// bds_blank and bds_blank_file: the window [w0, w1) of a buffer of n samples in pieces (pipe::run, bds_piece_pipe.h).
// read(first_byte, n_bytes, dst) delivers bytes of the buffer into pinned memory, write(first_byte, n_bytes, src) takes the blanked
// bytes of a piece's own samples.  A piece is uploaded with its context and worked on in place; only its own samples come back.
template <class Read, class Write>
static int run_pieces(bds_ctx *ctx, const char *who, int fmt, int64_t n, const bds_blank_opts &o, int64_t piece_samples, bds_blank_out *rep, Read read, Write write) {
    const int SB = sample_bytes(fmt);
    const int64_t w0 = o.lead, w1 = n - o.tail, piece = default_piece(fmt, piece_samples), np = piece_count(w0, w1, piece);
    const int64_t bins = duty_bins(w1 - w0, o.duty_samples);
    const size_t cap = (size_t)(std::min(piece, std::max<int64_t>(w1 - w0, 1)) + o.pre + o.post + 1) * SB + 16;
    unsigned long long tot[3] = {0, 0, 0};
    Scratch sc[2];
    DevScope scope;
    int32_t *d_duty = nullptr;  // one for both streams
    auto piece_k = [&](int64_t k) { return piece_of(n, w0, w1, piece, o.pre, o.post, k); };
    const int rc = pipe::run(
        ctx, who, np, cap, 3 * 8,
        [&] {
            hipError_t e = sc[0].alloc(tiles((int64_t)(cap / SB)));
            if (e == hipSuccess) e = sc[1].alloc(tiles((int64_t)(cap / SB)));
            if (e != hipSuccess || !bins) return e;
            e = scope.alloc(&d_duty, (size_t)bins * 4);
            if (e == hipSuccess) e = hipMemsetAsync(d_duty, 0, (size_t)bins * 4, (hipStream_t)ctx->stream);
            return e == hipSuccess ? hipStreamSynchronize((hipStream_t)ctx->stream) : e;  // (the other stream adds to it as well)
        },
        [&](int64_t k) {
            const Piece pc = piece_k(k);
            return pipe::Span{pc.load0 * SB, (size_t)((pc.load1 - pc.load0) * SB)};
        },
        read,
        [&](int64_t k, pipe::Slot &s) {
            const Piece pc = piece_k(k);
            hipError_t e = run_device(s.stream, fmt, s.d_buf, s.d_buf, pc.load1 - pc.load0, pc.core0 - pc.load0, pc.load1 - pc.core1, o, d_duty, pc.core0 - w0, sc[k & 1]);
            const size_t core_off = (size_t)((pc.core0 - pc.load0) * SB);  // only the piece's own samples come back
            if (e == hipSuccess) e = hipMemcpyAsync(s.h_buf + core_off, s.d_buf + core_off, (size_t)((pc.core1 - pc.core0) * SB), hipMemcpyDeviceToHost, s.stream);
            if (e == hipSuccess) e = hipMemcpyAsync(s.h_res, sc[k & 1].totals, 3 * 8, hipMemcpyDeviceToHost, s.stream);
            return e;
        },
        [&](int64_t k, pipe::Slot &s) {
            const Piece pc = piece_k(k);
            for (int i = 0; i < 3; ++i) tot[i] += reinterpret_cast<const unsigned long long *>(s.h_res)[i];
            return write(pc.core0 * SB, (size_t)((pc.core1 - pc.core0) * SB), s.h_buf + (pc.core0 - pc.load0) * SB);
        });
    if (rc) return rc;
    if (bins && np) {
        const hipError_t e = hipMemcpy(rep->duty, d_duty, (size_t)bins * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(ctx, who, e);
    }
    if (!np)
        for (int64_t i = 0; i < bins; ++i) rep->duty[i] = 0;
    fill_report(rep, w1 - w0, o, tot);
    return BDS_OK;
}

static int check_piece(bds_ctx *ctx, const char *who, int64_t piece_samples, const bds_blank_opts &o) {
    if (piece_samples < 0) return fail(ctx, BDS_ERR_ARG, "%s: piece_samples = %lld", who, (long long)piece_samples);
    if (piece_samples > 0 && piece_samples < std::max(o.pre, o.post) + 1)
        return fail(ctx, BDS_ERR_ARG, "%s: a piece of %lld samples is too small for its context (pre = %d, post = %d)", who, (long long)piece_samples, o.pre, o.post);
    return BDS_OK;
}

extern "C" int bds_blank(bds_ctx *ctx, const bds_settings *s, const void *in, size_t n_bytes, void *out, const bds_blank_opts *opts, bds_blank_out *report) {
    const char *who = "bds_blank";
    int64_t n = 0;
    const int fmt = check_entry(ctx, who, format_of, check_args, s, (int64_t)n_bytes, 0, opts, report, &n);
    if (fmt < 0) return fmt;
    if (int rc = check_host_pair(ctx, who, in, out, n_bytes, true)) return rc;
    const uint8_t *src = static_cast<const uint8_t *>(in);
    uint8_t *dst = static_cast<uint8_t *>(out);
    const int SB = sample_bytes(fmt);
    if (src != dst) {  // the context goes through as it is
        std::memcpy(dst, src, (size_t)(opts->lead * SB));
        std::memcpy(dst + (n - opts->tail) * SB, src + (n - opts->tail) * SB, (size_t)(opts->tail * SB));
    }
    // In place the pieces still see raw context: piece k + 1 is read before piece k is written back, a piece's context in front
    // lies in the one piece before it (a piece is longer than post + 1 samples) and its context behind in pieces not yet written.
    return run_pieces(ctx, who, fmt, n, *opts, 0, report, pipe::from_memory(in), pipe::to_memory(out));
}

extern "C" int bds_blank_file(bds_ctx *ctx, const bds_settings *s, const char *path_in, const char *path_out, int64_t n_samples, int64_t piece_samples,
                              const bds_blank_opts *opts, bds_blank_out *report) {
    const char *who = "bds_blank_file";
    const char *why;
    const int fmt = format_of(s, &why);
    if (fmt < 0) return fail(ctx, fmt, "%s: %s", who, why);
    char msg[1024];
    if (int rc = RecordWindow::check_names(path_in, path_out, true, s->skipNumberOfBytes, msg, sizeof msg)) return fail(ctx, rc, "%s: %s", who, msg);
    if (!opts || !report) return fail(ctx, BDS_ERR_ARG, "%s: opts or report is NULL", who);
    if (int rc = check_piece(ctx, who, piece_samples, *opts)) return rc;
    RecordWindow w;
    if (int rc = w.open(path_in, fmt, s->skipNumberOfBytes, msg, sizeof msg)) return fail(ctx, rc, "%s", msg);
    const int64_t n = n_samples > 0 ? n_samples : w.have;
    int64_t n_chk = 0;
    if (int rc = w.select(n, msg, sizeof msg)) return fail(ctx, rc, "%s: %s", who, msg);
    if (int rc = check_args(fmt, -1, n, opts, report, &n_chk, msg, sizeof msg)) return fail(ctx, rc, "%s: %s", who, msg);
    if (!ctx) return fail(ctx, BDS_ERR_ARG, "%s: ctx is NULL", who);
    if (int rc = w.open_out(path_out, msg, sizeof msg)) return fail(ctx, rc, "%s", msg);
    auto told = [&](int rc) { return rc ? fail(ctx, rc, "%s: %s", who, msg) : rc; };
    const int SB = sample_bytes(fmt);
    // the bytes in front of the window and behind it, and the window's context samples, go through as they are
    int rc = told(w.copy_front(opts->lead * SB, msg, sizeof msg));
    if (!rc)
        rc = run_pieces(
            ctx, who, fmt, n, *opts, piece_samples, report, [&](int64_t o, size_t nb, uint8_t *to) { return told(w.read(o, nb, to, msg, sizeof msg)); },
            [&](int64_t o, size_t nb, const uint8_t *from) { return told(w.write(o, nb, from, msg, sizeof msg)); });
    if (!rc) rc = told(w.copy_back(opts->tail * SB, msg, sizeof msg));
    if (!rc) rc = told(w.close(msg, sizeof msg));
    return rc;
}

extern "C" int bds_blank_dev(bds_ctx *ctx, const bds_settings *s, const void *d_in, size_t n_bytes, void *d_out, const bds_blank_opts *opts,
                             bds_blank_out *report) {
    const char *who = "bds_blank_dev";
    int64_t n = 0;
    const int fmt = check_entry(ctx, who, format_of, check_args, s, (int64_t)n_bytes, 0, opts, report, &n);
    if (fmt < 0) return fmt;
    if (int rc = check_device_pair(ctx, who, fmt, d_in, d_out, n_bytes, true)) return rc;
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)ctx->stream;
    const int64_t n_window = n - opts->lead - opts->tail, bins = duty_bins(n_window, opts->duty_samples);
    Scratch sc;
    DevScope scope;
    int32_t *d_duty = nullptr;
    hipError_t e = sc.alloc(tiles(n));
    if (e == hipSuccess && bins) e = scope.alloc(&d_duty, (size_t)bins * 4);
    if (e != hipSuccess) return hip_fail(ctx, who, e);
    if (bins) BDS_HIP(ctx, hipMemsetAsync(d_duty, 0, (size_t)bins * 4, st));
    unsigned long long tot[3] = {0, 0, 0};
    e = run_device(st, fmt, static_cast<const uint8_t *>(d_in), static_cast<uint8_t *>(d_out), n, opts->lead, opts->tail, *opts, d_duty, 0, sc);
    if (e == hipSuccess) e = hipMemcpyAsync(tot, sc.totals, sizeof tot, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && bins) e = hipMemcpyAsync(report->duty, d_duty, (size_t)bins * 4, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);  // the caller's memory is the caller's again
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(ctx, BDS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    fill_report(report, n_window, *opts, tot);
    return BDS_OK;
}

