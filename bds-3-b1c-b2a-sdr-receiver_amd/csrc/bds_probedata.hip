// probeData on the device (B2a/include/probeData.m:63-168 and the B1C copy): the 257-bin histogram of hist(data, -128:128) with
// exact integer statistics, the Welch PSD of pwelch(data, 32768, 2048, 32768, fs) and the time-domain excerpt, of a record in
// any of the five formats, decoded from the record's own bytes.  DESIGN.md "probeData" describes the layout.
//   k_probe_hist     one pass over the bytes: 16-byte loads over the aligned body, the ragged head and tail byte by byte;
//                    per-workgroup LDS counters flushed with 64-bit integer atomics; min / max / sum / sum of squares likewise
//   k_probe_segment  workgroup (k1, segment): the k1-th output of the 8-point stage of 32768 = 8 x 4096 for every n2, one twiddle
//                    exp(-2 pi i n k1 / 32768) per input, then a 4096-point radix-2 transform in LDS; |X|^2 per bin in fp32
//   k_probe_accumulate  one thread per bin adds the batch's segments to the f64 sums in segment order
// No floating-point atomics; the sums over segments are a plain left-to-right f64 sum per bin, whatever the batches and pieces.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "bds_internal.h"
#include "bds_probe_math.h"

namespace bds {
namespace probe {

// ---- decoders -------------------------------------------------------------------------------------------------------------------
// sample s (counted from the low end of byte 0 of p) as integers; p is aligned to the element size
template <int F>
__device__ __forceinline__ void decode(const uint8_t *__restrict__ p, int64_t s, int &re, int &im) {
    if (F == kS8) {
        re = (int8_t)p[s], im = 0;
    } else if (F == kS8C) {
        re = (int8_t)p[2 * s], im = (int8_t)p[2 * s + 1];
    } else if (F == kPacked) {  // unpack_cplx.m:18-30: low nibble first; bit 0 / 1 sign of I / Q, bit 2 / 3 magnitude 3 (else 1)
        const unsigned v = (p[s >> 1] >> (4 * (int)(s & 1))) & 15u;
        re = ((v & 4) ? 3 : 1) * ((v & 1) ? -1 : 1);
        im = ((v & 8) ? 3 : 1) * ((v & 2) ? -1 : 1);
    } else if (F == kS16) {
        re = reinterpret_cast<const int16_t *>(p)[s], im = 0;
    } else {
        re = reinterpret_cast<const int16_t *>(p)[2 * s], im = reinterpret_cast<const int16_t *>(p)[2 * s + 1];
    }
}

// ---- histogram and statistics ---------------------------------------------------------------------------------------------------
struct Stat {
    long long mn[2], mx[2], sum[2], sq[2];
};
__device__ __forceinline__ void count(unsigned *sh, Stat &t, int c, int v) {
    const int b = (v < -128 ? -128 : v > 128 ? 128 : v) + 128;
    atomicAdd(&sh[c * kBins + b], 1u);
    t.mn[c] = v < t.mn[c] ? v : t.mn[c];
    t.mx[c] = v > t.mx[c] ? v : t.mx[c];
    t.sum[c] += v;
    t.sq[c] += (long long)v * v;
}
// the bytes [o, o + len) of the record (o counted from p; len a multiple of the element size), their values in `w` (little-endian)
template <int F>
__device__ __forceinline__ void count_bytes(unsigned *sh, Stat &t, int64_t o, int len, const uint32_t *w, int64_t s0, int64_t s1) {
    if (F == kS16 || F == kS16C) {
        for (int i = 0; i < len; i += 2) {
            const int v = (int16_t)((w[i >> 2] >> (8 * (i & 3))) & 0xffffu);
            count(sh, t, F == kS16C ? (int)(((o + i) >> 1) & 1) : 0, v);
        }
    } else {
        for (int i = 0; i < len; ++i) {
            const unsigned b = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
            if (F == kPacked) {
                for (int h = 0; h < 2; ++h) {
                    const int64_t s = 2 * (o + i) + h;
                    if (s < s0 || s >= s1) continue;
                    const unsigned v = (b >> (4 * h)) & 15u;
                    count(sh, t, 0, ((v & 4) ? 3 : 1) * ((v & 1) ? -1 : 1));
                    count(sh, t, 1, ((v & 8) ? 3 : 1) * ((v & 2) ? -1 : 1));
                }
            } else {
                count(sh, t, F == kS8C ? (int)((o + i) & 1) : 0, (int)(int8_t)b);
            }
        }
    }
}

// samples [s0, s1) of the record at p: bytes [b0, b1).  [a0, a1) is the part of it whose addresses are whole aligned 16-byte lines
// (a0 >= a1: none); work item c < n_lines is line c, item n_lines the head [b0, min(a0, b1)), item n_lines + 1 the tail.
template <int F>
__global__ __launch_bounds__(256) void k_probe_hist(const uint8_t *__restrict__ p, int64_t s0, int64_t s1, int64_t b0, int64_t b1, int64_t a0,
                                                    int64_t a1, unsigned long long *__restrict__ hist, long long *__restrict__ stats) {
    __shared__ unsigned sh[2 * kBins];
    for (int i = threadIdx.x; i < 2 * kBins; i += 256) sh[i] = 0;
    __syncthreads();
    Stat t;
    for (int c = 0; c < 2; ++c) t.mn[c] = INT64_MAX, t.mx[c] = INT64_MIN, t.sum[c] = 0, t.sq[c] = 0;
    const int64_t n_lines = a1 > a0 ? (a1 - a0) / 16 : 0;
    const int64_t head_end = a1 > a0 ? a0 : b1, tail_begin = a1 > a0 ? a1 : b1;
    constexpr int E = (F == kS16 || F == kS16C) ? 2 : 1;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n_lines + 2; c += (int64_t)gridDim.x * 256) {
        if (c < n_lines) {
            const uint4 q = *reinterpret_cast<const uint4 *>(p + a0 + 16 * c);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
            count_bytes<F>(sh, t, a0 + 16 * c, 16, w, s0, s1);
        } else {
            const int64_t lo = c == n_lines ? b0 : tail_begin, hi = c == n_lines ? head_end : b1;
            for (int64_t o = lo; o < hi; o += E) {  // fewer than 16 bytes each
                uint32_t w[1] = {p[o]};
                if (E == 2) w[0] |= (uint32_t)p[o + 1] << 8;
                count_bytes<F>(sh, t, o, E, w, s0, s1);
            }
        }
    }
    for (int c = 0; c < 2; ++c) {
        for (int d = 32; d; d >>= 1) {
            const long long mn = __shfl_xor(t.mn[c], d), mx = __shfl_xor(t.mx[c], d);
            t.mn[c] = mn < t.mn[c] ? mn : t.mn[c], t.mx[c] = mx > t.mx[c] ? mx : t.mx[c];
            t.sum[c] += __shfl_xor(t.sum[c], d), t.sq[c] += __shfl_xor(t.sq[c], d);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&stats[4 * c + 0], t.mn[c]);
            atomicMax(&stats[4 * c + 1], t.mx[c]);
            atomicAdd(reinterpret_cast<unsigned long long *>(&stats[4 * c + 2]), (unsigned long long)t.sum[c]);
            atomicAdd(reinterpret_cast<unsigned long long *>(&stats[4 * c + 3]), (unsigned long long)t.sq[c]);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * kBins; i += 256)
        if (sh[i]) atomicAdd(&hist[i], (unsigned long long)sh[i]);
}

// ---- one segment's periodogram ----------------------------------------------------------------------------------------------------
// X[k1 + 8 k2] = sum_{n2} [ sum_{n1} w[n] x[n] W^{n k1} ] W_4096^{n2 k2},  n = 4096 n1 + n2,  W = exp(-2 pi i / 32768)
// (W^{n k1} = W_8^{n1 k1} W^{n2 k1}: the 8-point stage and the inter-stage twiddle in one table look-up, index n k1 mod 32768).
// grid (8, segments of the batch); out[(segment * 8 + k1) * nk2 + k2] = |X|^2 for k2 < nk2 (2049 of a real record: bins 0 .. 16384)
template <int F>
__global__ __launch_bounds__(256) void k_probe_segment(const uint8_t *__restrict__ p, int64_t s_first, const float *__restrict__ win,
                                                       const float2 *__restrict__ tw_n, const float2 *__restrict__ tw_4k, int nk2,
                                                       float *__restrict__ out) {
    __shared__ float2 buf[kN2];
    constexpr bool C = F == kS8C || F == kPacked || F == kS16C;
    const int k1 = blockIdx.x, tid = threadIdx.x;
    const int64_t base = s_first + (int64_t)blockIdx.y * kHop;
    for (int j = 0; j < kN2 / 256; ++j) {
        const int n2 = tid + 256 * j;
        float ar = 0.f, ai = 0.f;
        for (int n1 = 0; n1 < kN1; ++n1) {
            const int n = kN2 * n1 + n2;
            int xr, xi;
            decode<F>(p, base + n, xr, xi);
            const float w = win[n];
            const float2 t = tw_n[(n * k1) & (kNfft - 1)];
            const float vr = w * (float)xr;
            if (C) {
                const float vi = w * (float)xi;
                ar += vr * t.x - vi * t.y;
                ai += vr * t.y + vi * t.x;
            } else {
                ar += vr * t.x;
                ai += vr * t.y;
            }
        }
        buf[__brev((unsigned)n2) >> 20] = make_float2(ar, ai);
    }
    __syncthreads();
    for (int s = 1; s <= 12; ++s) {
        const int half = 1 << (s - 1);
        for (int j = 0; j < kN2 / 2 / 256; ++j) {
            const int b = tid + 256 * j, pos = b & (half - 1);
            const int i0 = ((b >> (s - 1)) << s) + pos, i1 = i0 + half;
            const float2 t = tw_4k[pos << (12 - s)];
            const float2 u = buf[i0], v = buf[i1];
            const float mr = v.x * t.x - v.y * t.y, mi = v.x * t.y + v.y * t.x;
            buf[i0] = make_float2(u.x + mr, u.y + mi);
            buf[i1] = make_float2(u.x - mr, u.y - mi);
        }
        __syncthreads();
    }
    float *o = out + ((size_t)blockIdx.y * kN1 + k1) * nk2;
    for (int k2 = tid; k2 < nk2; k2 += 256) {
        const float2 z = buf[k2];
        o[k2] = z.x * z.x + z.y * z.y;
    }
}

// acc[i] += pow[b][i], b = 0 .. n_seg - 1 in this order: with the batches taken in order, the f64 sum of a bin is
// ((P_0 + P_1) + P_2) + ... over the record's segments, however they were batched
__global__ __launch_bounds__(256) void k_probe_accumulate(const float *__restrict__ pw, int n_seg, int per_seg, double *__restrict__ acc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= per_seg) return;
    double a = acc[i];
    for (int b = 0; b < n_seg; ++b) a += (double)pw[(size_t)b * per_seg + i];
    acc[i] = a;
}

template <int F>
__global__ __launch_bounds__(256) void k_probe_excerpt(const uint8_t *__restrict__ p, int64_t s_first, int64_t n, double *__restrict__ re,
                                                       double *__restrict__ im) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int xr, xi;
    decode<F>(p, s_first + i, xr, xi);
    re[i] = (double)xr;
    if (im) im[i] = (double)xi;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
constexpr int kBatch = 128;  // segments whose powers are held at a time (128 x 32768 fp32 = 16 MiB)

struct Run {
    bds_ctx *ctx = nullptr;
    hipStream_t st = nullptr;
    int fmt = 0, nk2 = 0;
    double sum_w2 = 0;
    float *d_win = nullptr, *d_pow = nullptr;
    float2 *d_twn = nullptr, *d_tw4 = nullptr;
    double *d_acc = nullptr, *d_ex = nullptr;
    unsigned long long *d_hist = nullptr;
    long long *d_stats = nullptr;
    ~Run() {
        for (void *q : {(void *)d_win, (void *)d_pow, (void *)d_twn, (void *)d_tw4, (void *)d_acc, (void *)d_ex, (void *)d_hist, (void *)d_stats})
            if (q) (void)hipFree(q);
    }
};

static int run_begin(Run &r, bds_ctx *ctx, int fmt, int64_t n_seg_max, int64_t n_time) {
    r.ctx = ctx, r.fmt = fmt, r.st = (hipStream_t)ctx->stream;
    r.nk2 = is_complex(fmt) ? kN2 : kN2 / 2 + 1;
    std::vector<float> w, tn, t4;
    r.sum_w2 = window(w);
    twiddles(kNfft, kNfft, tn);
    twiddles(kN2, kN2 / 2, t4);
    const size_t per_seg = (size_t)kN1 * r.nk2;
    BDS_HIP(ctx, hipMalloc(&r.d_win, w.size() * 4));
    BDS_HIP(ctx, hipMalloc(&r.d_twn, tn.size() * 4));
    BDS_HIP(ctx, hipMalloc(&r.d_tw4, t4.size() * 4));
    BDS_HIP(ctx, hipMalloc(&r.d_pow, (size_t)std::min<int64_t>(kBatch, n_seg_max) * per_seg * 4));
    BDS_HIP(ctx, hipMalloc(&r.d_acc, per_seg * 8));
    BDS_HIP(ctx, hipMalloc(&r.d_hist, 2 * kBins * 8));
    BDS_HIP(ctx, hipMalloc(&r.d_stats, 8 * 8));
    if (n_time) BDS_HIP(ctx, hipMalloc(&r.d_ex, (size_t)n_time * 16));
    BDS_HIP(ctx, hipMemcpyAsync(r.d_win, w.data(), w.size() * 4, hipMemcpyHostToDevice, r.st));
    BDS_HIP(ctx, hipMemcpyAsync(r.d_twn, tn.data(), tn.size() * 4, hipMemcpyHostToDevice, r.st));
    BDS_HIP(ctx, hipMemcpyAsync(r.d_tw4, t4.data(), t4.size() * 4, hipMemcpyHostToDevice, r.st));
    const long long init[8] = {INT64_MAX, INT64_MIN, 0, 0, INT64_MAX, INT64_MIN, 0, 0};
    BDS_HIP(ctx, hipMemcpyAsync(r.d_stats, init, sizeof init, hipMemcpyHostToDevice, r.st));
    BDS_HIP(ctx, hipMemsetAsync(r.d_acc, 0, per_seg * 8, r.st));
    BDS_HIP(ctx, hipMemsetAsync(r.d_hist, 0, 2 * kBins * 8, r.st));
    BDS_HIP(ctx, hipStreamSynchronize(r.st));  // (the tables and `init` are host locals)
    return BDS_OK;
}

// One span of the record on the device: p holds the record from the byte of sample `origin` on (sample origin + i is sample
// sub + i counted from the low end of p's byte 0; sub is 1 only for a packed record that starts at a high nibble).  Counts samples
// [hist0, hist1) and transforms segments [seg0, seg1) (record numbering); every byte read lies in the span's own samples.
template <int F>
static int run_span_t(Run &r, const uint8_t *p, int64_t origin, int sub, const Piece &pc) {
    bds_ctx *ctx = r.ctx;
    if (pc.hist1 > pc.hist0) {
        const int64_t s0 = pc.hist0 - origin + sub, s1 = pc.hist1 - origin + sub;
        int64_t b0, b1;
        byte_span(F, s0, s1, &b0, &b1);
        const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
        const int64_t a0 = (int64_t)(((addr + (uint64_t)b0 + 15) & ~(uintptr_t)15) - addr), a1 = (int64_t)(((addr + (uint64_t)b1) & ~(uintptr_t)15) - addr);
        const int64_t lines = a1 > a0 ? (a1 - a0) / 16 : 0;
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (lines + 2 + 256 * 8 - 1) / (256 * 8)));
        hipLaunchKernelGGL(k_probe_hist<F>, dim3(grid), dim3(256), 0, r.st, p, s0, s1, b0, b1, a0, a1, r.d_hist, r.d_stats);
        BDS_HIP(ctx, hipGetLastError());
    }
    const int per_seg = kN1 * r.nk2;
    for (int64_t g = pc.seg0; g < pc.seg1; g += kBatch) {
        const int nb = (int)std::min<int64_t>(kBatch, pc.seg1 - g);
        hipLaunchKernelGGL(k_probe_segment<F>, dim3(kN1, nb), dim3(256), 0, r.st, p, g * kHop - origin + sub, r.d_win, r.d_twn, r.d_tw4, r.nk2, r.d_pow);
        BDS_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_probe_accumulate, dim3((per_seg + 255) / 256), dim3(256), 0, r.st, r.d_pow, nb, per_seg, r.d_acc);
        BDS_HIP(ctx, hipGetLastError());
    }
    return BDS_OK;
}
static int run_span(Run &r, const uint8_t *p, int64_t origin, int sub, const Piece &pc) {
    switch (r.fmt) {
    case kS8: return run_span_t<kS8>(r, p, origin, sub, pc);
    case kS8C: return run_span_t<kS8C>(r, p, origin, sub, pc);
    case kPacked: return run_span_t<kPacked>(r, p, origin, sub, pc);
    case kS16: return run_span_t<kS16>(r, p, origin, sub, pc);
    default: return run_span_t<kS16C>(r, p, origin, sub, pc);
    }
}
static int run_excerpt(Run &r, const uint8_t *p, int sub, int64_t n_time) {
    if (!n_time) return BDS_OK;
    double *re = r.d_ex, *im = is_complex(r.fmt) ? r.d_ex + n_time : nullptr;
    const dim3 grid((unsigned)((n_time + 255) / 256));
    switch (r.fmt) {
    case kS8: hipLaunchKernelGGL(k_probe_excerpt<kS8>, grid, dim3(256), 0, r.st, p, (int64_t)sub, n_time, re, im); break;
    case kS8C: hipLaunchKernelGGL(k_probe_excerpt<kS8C>, grid, dim3(256), 0, r.st, p, (int64_t)sub, n_time, re, im); break;
    case kPacked: hipLaunchKernelGGL(k_probe_excerpt<kPacked>, grid, dim3(256), 0, r.st, p, (int64_t)sub, n_time, re, im); break;
    case kS16: hipLaunchKernelGGL(k_probe_excerpt<kS16>, grid, dim3(256), 0, r.st, p, (int64_t)sub, n_time, re, im); break;
    default: hipLaunchKernelGGL(k_probe_excerpt<kS16C>, grid, dim3(256), 0, r.st, p, (int64_t)sub, n_time, re, im); break;
    }
    BDS_HIP(r.ctx, hipGetLastError());
    return BDS_OK;
}

// download and the last host step; the first write to *out
static int run_end(Run &r, const bds_settings *s, int64_t n, int64_t n_time, bds_probe_out *out) {
    bds_ctx *ctx = r.ctx;
    const size_t per_seg = (size_t)kN1 * r.nk2;
    std::vector<double> acc(per_seg), ex((size_t)n_time * 2);
    unsigned long long hist[2 * kBins];
    long long stats[8];
    BDS_HIP(ctx, hipMemcpyAsync(acc.data(), r.d_acc, per_seg * 8, hipMemcpyDeviceToHost, r.st));
    BDS_HIP(ctx, hipMemcpyAsync(hist, r.d_hist, sizeof hist, hipMemcpyDeviceToHost, r.st));
    BDS_HIP(ctx, hipMemcpyAsync(stats, r.d_stats, sizeof stats, hipMemcpyDeviceToHost, r.st));
    if (n_time) BDS_HIP(ctx, hipMemcpyAsync(ex.data(), r.d_ex, (size_t)n_time * 16, hipMemcpyDeviceToHost, r.st));
    BDS_HIP(ctx, hipStreamSynchronize(r.st));
    const bool cplx = is_complex(r.fmt);
    for (int i = 0; i < kBins; ++i) {
        out->hist_i[i] = (int64_t)hist[i];
        if (out->hist_q) out->hist_q[i] = cplx ? (int64_t)hist[kBins + i] : 0;
    }
    out->min_i = stats[0], out->max_i = stats[1], out->sum_i = stats[2], out->sumsq_i = stats[3];
    out->min_q = cplx ? stats[4] : 0, out->max_q = cplx ? stats[5] : 0, out->sum_q = cplx ? stats[6] : 0, out->sumsq_q = cplx ? stats[7] : 0;
    out->n_segments = segments(n), out->n_samples = n, out->n_psd = psd_bins(r.fmt);
    finish_psd(r.fmt, acc.data(), r.nk2, segments(n), s->samplingFreq, r.sum_w2, out->psd);
    for (int64_t i = 0; i < n_time; ++i) {
        out->excerpt_re[i] = ex[i];
        if (cplx) out->excerpt_im[i] = ex[n_time + i];
    }
    return BDS_OK;
}

// What bds_probe_data and bds_probe_data_file share: the window is cut into pieces (bds_probe_math.h: piece) and every piece
// goes host to device and through run_span.  read(first_byte, n_bytes, dst) delivers bytes of the window, counted from the byte
// that holds the window's first sample.
template <class Read>
static int run_pieces(bds_ctx *ctx, const char *who, const bds_settings *s, int fmt, int sub, int64_t n, int64_t n_time, bds_probe_out *out, Read read) {
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t spp = default_piece_segments(fmt, ctx->probe_piece_segments), np = piece_count(n, spp);
    Run r;
    if (int rc = run_begin(r, ctx, fmt, std::min(spp, segments(n)), n_time)) return rc;
    size_t cap = 0;
    for (int64_t j = 0; j < np; ++j) {
        const Piece pc = piece(n, spp, j);
        int64_t b0, b1;
        byte_span(fmt, pc.load0 + sub, pc.load1 + sub, &b0, &b1);
        cap = std::max(cap, (size_t)(b1 - b0));
    }
    uint8_t *d_rec = nullptr;
    std::vector<uint8_t> host(cap);
    hipError_t e = hipMalloc(&d_rec, cap);
    if (e != hipSuccess) return hip_fail(ctx, who, e);
    int rc = BDS_OK;
    for (int64_t j = 0; j < np && !rc; ++j) {
        const Piece pc = piece(n, spp, j);
        int64_t b0, b1;
        byte_span(fmt, pc.load0 + sub, pc.load1 + sub, &b0, &b1);
        rc = read(b0, (size_t)(b1 - b0), host.data());
        if (!rc && (e = hipMemcpyAsync(d_rec, host.data(), (size_t)(b1 - b0), hipMemcpyHostToDevice, r.st)) != hipSuccess)
            rc = fail(ctx, BDS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
        // the piece's bytes start at byte b0 of the window: sample pc.load0 of the record is sample (pc.load0 + sub) - 8 b0 / bits of d_rec
        const int psub = fmt == kPacked ? (int)((pc.load0 + sub) & 1) : 0;
        if (!rc && j == 0) rc = run_excerpt(r, d_rec, psub, n_time);
        if (!rc) rc = run_span(r, d_rec, pc.load0, psub, pc);
        if (!rc && (e = hipStreamSynchronize(r.st)) != hipSuccess) rc = fail(ctx, BDS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));  // `host` is reused
    }
    (void)hipStreamSynchronize(r.st);
    (void)hipFree(d_rec);
    if (rc) return rc;
    return run_end(r, s, n, n_time, out);
}

static int settings_format(bds_ctx *ctx, const char *who, const bds_settings *s) {
    if (!ctx) return fail(ctx, BDS_ERR_ARG, "%s: ctx is NULL", who);
    if (!s) return fail(ctx, BDS_ERR_ARG, "%s: settings is NULL", who);
    const char *why;
    const int fmt = format_of(*s, &why);
    if (fmt < 0) return fail(ctx, fmt, "%s: %s", who, why);
    return fmt;
}

}  // namespace probe
}  // namespace bds

#include "bds_record_window.h"  // the file entry's window, as the conditioners take theirs

using namespace bds;
using namespace bds::probe;

extern "C" int bds_probe_set_piece_segments(bds_ctx *ctx, int64_t n_segments) {
    if (!ctx || n_segments < 0) return fail(ctx, BDS_ERR_ARG, "bds_probe_set_piece_segments: ctx is NULL or n_segments < 0");
    ctx->probe_piece_segments = n_segments;
    return BDS_OK;
}

extern "C" int bds_probe_data(bds_ctx *ctx, const bds_settings *s, const void *bytes, size_t n_bytes, int64_t n_time, bds_probe_out *out) {
    const int fmt = settings_format(ctx, "bds_probe_data", s);
    if (fmt < 0) return fmt;
    char msg[200];
    int64_t n = 0;
    if (int rc = check_args(s, fmt, (int64_t)n_bytes, 0, n_time, out, &n, msg, sizeof msg)) return fail(ctx, rc, "bds_probe_data: %s", msg);
    if (!bytes) return fail(ctx, BDS_ERR_ARG, "bds_probe_data: bytes is NULL");
    const uint8_t *src = static_cast<const uint8_t *>(bytes);
    return run_pieces(ctx, "bds_probe_data", s, fmt, 0, n, n_time, out, [&](int64_t b0, size_t nb, uint8_t *dst) {
        std::memcpy(dst, src + b0, nb);
        return (int)BDS_OK;
    });
}

extern "C" int bds_probe_data_file(bds_ctx *ctx, const bds_settings *s, const char *path, int64_t n_samples, int64_t n_time, bds_probe_out *out) {
    const char *who = "bds_probe_data_file";
    const int fmt = settings_format(ctx, who, s);
    if (fmt < 0) return fmt;
    if (!path) return fail(ctx, BDS_ERR_ARG, "%s: path is NULL", who);
    if (s->skipNumberOfBytes < 0 || n_samples < -1) return fail(ctx, BDS_ERR_ARG, "%s: skipNumberOfBytes < 0 or n_samples < -1", who);
    RecordWindow w;
    char msg[1024];
    if (int rc = w.open(path, fmt, s->skipNumberOfBytes, msg, sizeof msg)) return fail(ctx, rc, "%s", msg);  // probeData.m:173
    const int64_t n = n_samples == 0 ? reference_window(*s) : n_samples < 0 ? w.have : n_samples;
    int64_t n_chk = 0;
    if (int rc = w.select(n, msg, sizeof msg)) return fail(ctx, rc, "%s: %s", who, msg);  // probeData.m:81-84
    if (int rc = check_args(s, fmt, -1, n, n_time, out, &n_chk, msg, sizeof msg)) return fail(ctx, rc, "%s: %s", who, msg);
    return run_pieces(ctx, who, s, fmt, w.sub, n, n_time, out, [&](int64_t o, size_t nb, uint8_t *dst) {
        const int rc = w.read(o, nb, dst, msg, sizeof msg);
        return rc ? fail(ctx, rc, "%s: %s", who, msg) : rc;
    });
}

extern "C" int bds_probe_data_dev(bds_ctx *ctx, const bds_settings *s, const void *d_bytes, size_t n_bytes, int64_t n_time, bds_probe_out *out) {
    const char *who = "bds_probe_data_dev";
    const int fmt = settings_format(ctx, who, s);
    if (fmt < 0) return fmt;
    char msg[200];
    int64_t n = 0;
    if (int rc = check_args(s, fmt, (int64_t)n_bytes, 0, n_time, out, &n, msg, sizeof msg)) return fail(ctx, rc, "%s: %s", who, msg);
    if (reinterpret_cast<uintptr_t>(d_bytes) % (uintptr_t)elem_bytes(fmt))
        return fail(ctx, BDS_ERR_ARG, "%s: d_bytes is not aligned to the %d-byte samples of the record", who, elem_bytes(fmt));
    if (int rc = check_device_span(ctx, who, "d_bytes", d_bytes, n_bytes)) return rc;
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    Run r;
    if (int rc = run_begin(r, ctx, fmt, segments(n), n_time)) return rc;
    const uint8_t *p = static_cast<const uint8_t *>(d_bytes);
    Piece all = piece(n, segments(n), 0);  // the record is read where it lies: one span
    int rc = run_excerpt(r, p, 0, n_time);
    if (!rc) rc = run_span(r, p, 0, 0, all);
    hipError_t e = hipStreamSynchronize(r.st);  // the caller's memory is the caller's again
    if (!rc && e != hipSuccess) rc = fail(ctx, BDS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    if (rc) return rc;
    return run_end(r, s, n, n_time, out);
}
