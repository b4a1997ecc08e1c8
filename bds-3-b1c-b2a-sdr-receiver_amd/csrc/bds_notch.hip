// Tone excision of an IF record on the device (include/bds_mi355x.h "tone excision"): per block of
// B = 2^block_log2 samples and per tone the record's projection on the tone's local oscillator is estimated and subtracted, on the
// record's own bytes, in integers only.
//   k_notch_est    the int64 block sums of x lo* per tone, the division to ar, ai (1 / 256 LSB) and the sum of x^2 before
//   k_notch_apply  the same samples again: the LO recomputed, er / ei formed from the block's estimates, shifted, subtracted,
//                  saturated; the sum of y^2 and the count of saturated samples
// Both passes walk the record in 16-byte chunks of its OWN grid (chunk c = bytes [16 c, 16 c + 16) of the buffer, 16, 8, 8 or 4
// samples): blocks begin on chunks, so no chunk belongs to two blocks and none to two lanes.  A workgroup of 8 waves takes a run of
// whole blocks (BDS_NOTCH_RUN_BYTES of the record), a wave one block of the run at a time: its 64 lanes stride over the block's
// chunks, each with its chunk in registers and the tones looped over it (the record is read once whatever n_tones is); the block
// sums are reduced with shuffles inside the wave, so the kernels need no LDS but the table.  The apply pass reads only the chunk
// it writes and runs behind the finished estimates, which makes in place correct.  A buffer whose address is a multiple of 16
// moves as 16-byte words; at any other address, and in the record's last partial chunk, every byte moves on its own, and no byte
// outside the record is touched.  The LO table stands in LDS whole, (C, S) packed in 32 bits: 64 KiB, one lookup per sample and
// tone; two workgroups fit a CU.  The only atomics are the 64-bit integer adds of the three sums, one per wave: exact in any order.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bds_internal.h"
#include "bds_notch_math.h"

namespace bds {
namespace notch {

constexpr int kThreads = 512, kWaves = kThreads / 64;

struct Args {
    const uint8_t *in;
    uint8_t *out;
    int64_t n, first;      // samples of the buffer; absolute index of its sample 0 (a multiple of the block)
    int64_t n_blocks;
    int run;               // blocks per workgroup
    int n_tones, block_log2;
    int vec_in, vec_out;   // the address is a multiple of 16: whole chunks move as one 16-byte word
    uint32_t step[kMaxTones];
    const uint32_t *tab;   // [2^P]: C in the low half, S in the high half
    int32_t *est;          // [n_blocks][n_tones][2]
    unsigned long long *tot;  // sum_sq_in, sum_sq_out, n_saturated
};

// chunk c of a buffer of `total` bytes: the bytes behind the end read as 0 and are not written
__device__ __forceinline__ uint4 load_chunk(const uint8_t *p, int64_t c, int64_t total, bool vec) {
    const int64_t b = c << 4;
    if (vec && b + 16 <= total) return *reinterpret_cast<const uint4 *>(p + b);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (b + i < total) w[i >> 2] |= (uint32_t)p[b + i] << (8 * (i & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ void store_chunk(uint8_t *p, int64_t c, int64_t total, bool vec, uint4 q) {
    const int64_t b = c << 4;
    if (vec && b + 16 <= total) {
        *reinterpret_cast<uint4 *>(p + b) = q;
        return;
    }
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (b + i < total) p[b + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

// sample i of a chunk: SB bytes per sample, E bytes per element
template <int SB, int E>
__device__ __forceinline__ void sample_of(const uint32_t (&w)[4], int i, int &re, int &im) {
    im = 0;
    if (E == 1) {
        const uint32_t v = w[(i * SB) >> 2] >> (8 * ((i * SB) & 3));
        re = (int8_t)(v & 0xffu);
        if (SB == 2) im = (int8_t)((v >> 8) & 0xffu);
    } else {
        const uint32_t v = w[(i * SB) >> 2] >> (8 * ((i * SB) & 3));
        re = (int16_t)(v & 0xffffu);
        if (SB == 4) im = (int16_t)(v >> 16);
    }
}
__device__ __forceinline__ void lo_of(const uint32_t *tab, uint32_t phi, int &c, int &s) {
    const uint32_t v = tab[lo_index(phi)];
    c = (int16_t)(v & 0xffffu), s = (int16_t)(v >> 16);
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ void load_table(uint32_t *sh, const uint32_t *tab) {
    for (int i = threadIdx.x; i < kTab / 4; i += kThreads) reinterpret_cast<uint4 *>(sh)[i] = reinterpret_cast<const uint4 *>(tab)[i];
    __syncthreads();
}

// ---- estimate -------------------------------------------------------------------------------------------------------------------------
// Products per int32 partial sum: |x C| <= 2^21 (int8), 2^29 (int16); a pair's I C + Q S twice that.  A chunk of int8 samples
// stays below 2^25; of int16 real samples two fit an int32, of int16 pairs one.
template <int SB, int E>
__global__ __launch_bounds__(kThreads) void k_notch_est(Args a) {
    constexpr int NS = 16 / SB, G = E == 1 ? NS : (SB == 2 ? 2 : 1);
    constexpr bool CPLX = SB == 2 * E;
    __shared__ uint32_t sh_tab[kTab];
    load_table(sh_tab, a.tab);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t total = a.n * SB, B = (int64_t)1 << a.block_log2, cb = B * SB >> 4;
    const int64_t b0 = (int64_t)blockIdx.x * a.run, b1 = b0 + a.run < a.n_blocks ? b0 + a.run : a.n_blocks;
    unsigned long long sq = 0;
    for (int64_t b = b0 + wv; b < b1; b += kWaves) {
        long long sr[kMaxTones], si[kMaxTones];
#pragma unroll
        for (int k = 0; k < kMaxTones; ++k) sr[k] = 0, si[k] = 0;
        const int64_t c0 = b * cb;
        for (int64_t j = lane; j < cb; j += 64) {
            const int64_t c = c0 + j;
            if ((c << 4) >= total) break;
            const uint4 q = load_chunk(a.in, c, total, a.vec_in);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
            const int64_t n0 = a.first + c * NS;
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                int re, im;
                sample_of<SB, E>(w, i, re, im);
                sq += (unsigned long long)((uint32_t)(re * re) + (uint32_t)(im * im));
            }
#pragma unroll
            for (int k = 0; k < kMaxTones; ++k) {
                if (k >= a.n_tones) break;
                const uint32_t st = a.step[k];
                uint32_t phi = phase(st, n0);
#pragma unroll
                for (int g = 0; g < NS / G; ++g) {
                    int pr = 0, pi = 0;
#pragma unroll
                    for (int i = g * G; i < (g + 1) * G; ++i) {
                        int re, im, lc, ls;
                        sample_of<SB, E>(w, i, re, im);
                        lo_of(sh_tab, phi, lc, ls);
                        if (CPLX) pr += re * lc + im * ls, pi += im * lc - re * ls;
                        else pr += re * lc, pi -= re * ls;
                        phi += st;
                    }
                    sr[k] += pr, si[k] += pi;
                }
            }
        }
        const int64_t r = (b + 1) * B <= a.n ? B : a.n - b * B;
#pragma unroll
        for (int k = 0; k < kMaxTones; ++k) {
            if (k >= a.n_tones) break;
            long long vr = sr[k], vi = si[k];
            for (int d = 32; d; d >>= 1) vr += __shfl_xor(vr, d), vi += __shfl_xor(vi, d);
            if (lane == k) {
                int32_t *e = a.est + (b * a.n_tones + k) * 2;
                e[0] = r == B ? estimate_full(vr, a.block_log2) : estimate(vr, r);
                e[1] = r == B ? estimate_full(vi, a.block_log2) : estimate(vi, r);
            }
        }
    }
    sq = wave_sum(sq);
    if (lane == 0 && sq) atomicAdd(&a.tot[0], sq);
}

// ---- apply ----------------------------------------------------------------------------------------------------------------------------
template <int SB, int E>
__global__ __launch_bounds__(kThreads) void k_notch_apply(Args a) {
    constexpr int NS = 16 / SB;
    constexpr bool CPLX = SB == 2 * E;
    constexpr int LO = E == 1 ? -128 : -32768, HI = E == 1 ? 127 : 32767;
    __shared__ uint32_t sh_tab[kTab];
    load_table(sh_tab, a.tab);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t total = a.n * SB, B = (int64_t)1 << a.block_log2, cb = B * SB >> 4;
    const int64_t b0 = (int64_t)blockIdx.x * a.run, b1 = b0 + a.run < a.n_blocks ? b0 + a.run : a.n_blocks;
    unsigned long long sq = 0, sat = 0;
    for (int64_t b = b0 + wv; b < b1; b += kWaves) {
        int ar[kMaxTones], ai[kMaxTones];
#pragma unroll
        for (int k = 0; k < kMaxTones; ++k) {
            const bool on = k < a.n_tones;
            ar[k] = on ? a.est[(b * a.n_tones + k) * 2] : 0, ai[k] = on ? a.est[(b * a.n_tones + k) * 2 + 1] : 0;
        }
        const int64_t c0 = b * cb;
        for (int64_t j = lane; j < cb; j += 64) {
            const int64_t c = c0 + j;
            if ((c << 4) >= total) break;
            const uint4 q = load_chunk(a.in, c, total, a.vec_in);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
            const int64_t n0 = a.first + c * NS;
            long long er[NS], ei[CPLX ? NS : 1];
#pragma unroll
            for (int i = 0; i < NS; ++i) er[i] = 0;
#pragma unroll
            for (int i = 0; i < (CPLX ? NS : 1); ++i) ei[i] = 0;
#pragma unroll
            for (int k = 0; k < kMaxTones; ++k) {
                if (k >= a.n_tones) break;
                const uint32_t st = a.step[k];
                uint32_t phi = phase(st, n0);
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    int lc, ls;
                    lo_of(sh_tab, phi, lc, ls);
                    er[i] += (long long)ar[k] * lc - (long long)ai[k] * ls;
                    if (CPLX) ei[i] += (long long)ar[k] * ls + (long long)ai[k] * lc;
                    phi += st;
                }
            }
            const int64_t left = a.n - c * NS;  // samples of the chunk inside the record
            uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                int re, im;
                sample_of<SB, E>(w, i, re, im);
                int yr = re - (CPLX ? sub_cplx(er[i]) : sub_real(er[i])), yi = CPLX ? im - sub_cplx(ei[i]) : 0;
                const int zr = yr < LO ? LO : yr > HI ? HI : yr, zi = yi < LO ? LO : yi > HI ? HI : yi;
                if (i < left) {
                    sat += (zr != yr || zi != yi) ? 1u : 0u;
                    sq += (unsigned long long)((uint32_t)(zr * zr) + (uint32_t)(zi * zi));
                }
                uint32_t bits = E == 1 ? ((uint32_t)zr & 0xffu) : ((uint32_t)zr & 0xffffu);
                if (CPLX) bits |= (E == 1 ? ((uint32_t)zi & 0xffu) : ((uint32_t)zi & 0xffffu)) << (8 * E);
                o[(i * SB) >> 2] |= bits << (8 * ((i * SB) & 3));
            }
            store_chunk(a.out, c, total, a.vec_out, make_uint4(o[0], o[1], o[2], o[3]));
        }
    }
    sq = wave_sum(sq), sat = wave_sum(sat);
    if (lane == 0 && sq) atomicAdd(&a.tot[1], sq);
    if (lane == 0 && sat) atomicAdd(&a.tot[2], sat);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
template <int SB, int E>
static void launch_t(hipStream_t st, const Args &a, bool apply) {
    const unsigned nwg = (unsigned)((a.n_blocks + a.run - 1) / a.run);
    hipLaunchKernelGGL((k_notch_est<SB, E>), dim3(nwg), dim3(kThreads), 0, st, a);
    if (apply) hipLaunchKernelGGL((k_notch_apply<SB, E>), dim3(nwg), dim3(kThreads), 0, st, a);
}

static void fill_report(bds_notch_out *rep, int64_t n, const bds_notch_opts &o, const unsigned long long tot[3]) {
    rep->n_samples = n, rep->n_blocks = block_count(n, o.block_log2);
    rep->sum_sq_in = tot[0], rep->sum_sq_out = o.apply ? tot[1] : 0, rep->n_saturated = o.apply ? (int64_t)tot[2] : 0;
}

}  // namespace notch
}  // namespace bds

#include "bds_piece_pipe.h"  // what the entries share with the other conditioners: their checks, the layout switch, the piece loop

using namespace bds;
using namespace bds::notch;

// One buffer of n samples on the device, sample 0 of it the absolute sample `first`: estimates into d_est, the three sums into
// d_tot, the notched bytes into d_out when o.apply; asynchronous on `st`.  n = 0 launches nothing (the sums are zeroed).
static hipError_t run_device(hipStream_t st, int fmt, const uint8_t *d_in, uint8_t *d_out, int64_t n, int64_t first, const bds_notch_opts &o,
                             const uint32_t *d_tab, int32_t *d_est, unsigned long long *d_tot) {
    const hipError_t e0 = hipMemsetAsync(d_tot, 0, 3 * 8, st);
    if (n == 0 || e0 != hipSuccess) return e0;
    Args a{};
    a.in = d_in, a.out = d_out, a.n = n, a.first = first;
    a.n_blocks = block_count(n, o.block_log2);
    a.run = (int)std::max<int64_t>(1, kRunBytes / (((int64_t)1 << o.block_log2) * sample_bytes(fmt)));
    a.n_tones = o.n_tones, a.block_log2 = o.block_log2;
    a.vec_in = (reinterpret_cast<uintptr_t>(d_in) & 15u) == 0;
    a.vec_out = o.apply && (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0;
    for (int k = 0; k < kMaxTones; ++k) a.step[k] = k < o.n_tones ? o.step[k] : 0u;
    a.tab = d_tab, a.est = d_est, a.tot = d_tot;
    with_sample_layout(fmt, [&](auto sb, auto el) { launch_t<decltype(sb)::value, decltype(el)::value>(st, a, o.apply != 0); });
    return hipGetLastError();
}

// the table as the kernels keep it: C in the low half, S in the high half of a 32-bit word
static hipError_t upload_table(DevScope &scope, uint32_t **d_tab) {
    std::vector<int16_t> cs((size_t)2 * kTab);
    lo_table(cs.data());
    std::vector<uint32_t> packed(kTab);
    for (int i = 0; i < kTab; ++i) packed[i] = (uint32_t)(uint16_t)cs[i] | ((uint32_t)(uint16_t)cs[kTab + i] << 16);
    hipError_t e = scope.alloc(d_tab, (size_t)kTab * 4);
    if (e == hipSuccess) e = hipMemcpy(*d_tab, packed.data(), (size_t)kTab * 4, hipMemcpyHostToDevice);
    return e;
}

static int check_piece(bds_ctx *ctx, const char *who, int fmt, int64_t piece_samples, const bds_notch_opts &o) {
    if (piece_samples < 0) return fail(ctx, BDS_ERR_ARG, "%s: piece_samples = %lld", who, (long long)piece_samples);
    if (piece_samples > 0 && piece_of(fmt, piece_samples, o.block_log2) == 0)
        return fail(ctx, BDS_ERR_ARG, "%s: a piece of %lld samples is smaller than one block of %lld", who, (long long)piece_samples, (long long)1 << o.block_log2);
    return BDS_OK;
}

// bds_notch and bds_notch_file: a window of n samples in pieces of whole blocks (pipe::run, bds_piece_pipe.h).
// read(first_byte, n_bytes, dst) delivers bytes of the window into pinned memory, write(first_byte, n_bytes, src) takes a piece's
// notched bytes.  A slot's result block holds the three sums, then the piece's estimates.
template <class Read, class Write>
static int run_pieces(bds_ctx *ctx, const char *who, int fmt, int64_t n, const bds_notch_opts &o, int64_t piece_samples, bds_notch_out *rep, Read read, Write write) {
    const int SB = sample_bytes(fmt);
    const int64_t piece = piece_of(fmt, piece_samples, o.block_log2), np = n > 0 ? (n + piece - 1) / piece : 0;
    const int64_t per_block = (int64_t)o.n_tones * 2;
    const int64_t cap_samples = std::min(piece, std::max<int64_t>(n, 1));
    const size_t est_bytes = (size_t)(block_count(cap_samples, o.block_log2) * per_block) * 4;
    unsigned long long tot[3] = {0, 0, 0};
    DevScope scope;
    uint32_t *d_tab = nullptr;
    int32_t *d_est[2] = {nullptr, nullptr};
    unsigned long long *d_tot[2] = {nullptr, nullptr};
    auto samples_of = [&](int64_t k, int64_t *s0) { return *s0 = k * piece, std::min(n, *s0 + piece) - *s0; };
    auto est_bytes_of = [&](int64_t n_piece) { return (size_t)(block_count(n_piece, o.block_log2) * per_block) * 4; };
    const int rc = pipe::run(
        ctx, who, np, (size_t)cap_samples * SB + 16, 3 * 8 + est_bytes,
        [&] {
            hipError_t e = upload_table(scope, &d_tab);
            for (int i = 0; i < 2 && e == hipSuccess; ++i) {
                e = scope.alloc(&d_est[i], est_bytes);
                if (e == hipSuccess) e = scope.alloc(&d_tot[i], 3 * 8);
            }
            return e;
        },
        [&](int64_t k) {
            int64_t s0;
            const int64_t ns = samples_of(k, &s0);
            return pipe::Span{s0 * SB, (size_t)(ns * SB)};
        },
        read,
        [&](int64_t k, pipe::Slot &s) {
            int64_t s0;
            const int64_t ns = samples_of(k, &s0);
            const int b = (int)(k & 1);
            hipError_t e = run_device(s.stream, fmt, s.d_buf, s.d_buf, ns, o.first_sample + s0, o, d_tab, d_est[b], d_tot[b]);
            if (e == hipSuccess && o.apply) e = hipMemcpyAsync(s.h_buf, s.d_buf, (size_t)(ns * SB), hipMemcpyDeviceToHost, s.stream);
            if (e == hipSuccess && rep->est) e = hipMemcpyAsync(s.h_res + 3 * 8, d_est[b], est_bytes_of(ns), hipMemcpyDeviceToHost, s.stream);
            if (e == hipSuccess) e = hipMemcpyAsync(s.h_res, d_tot[b], 3 * 8, hipMemcpyDeviceToHost, s.stream);
            return e;
        },
        [&](int64_t k, pipe::Slot &s) {
            int64_t s0;
            const int64_t ns = samples_of(k, &s0);
            if (rep->est) std::memcpy(rep->est + (s0 >> o.block_log2) * per_block, s.h_res + 3 * 8, est_bytes_of(ns));
            for (int i = 0; i < 3; ++i) tot[i] += reinterpret_cast<const unsigned long long *>(s.h_res)[i];
            return o.apply ? write(s0 * SB, (size_t)(ns * SB), s.h_buf) : (int)BDS_OK;
        });
    if (rc) return rc;
    fill_report(rep, n, o, tot);
    return BDS_OK;
}

extern "C" int bds_notch_lo(int16_t *cos_sin) {
    if (!cos_sin) return fail(nullptr, BDS_ERR_ARG, "bds_notch_lo: cos_sin is NULL");
    lo_table(cos_sin);
    return BDS_OK;
}

extern "C" int bds_notch(bds_ctx *ctx, const bds_settings *s, const void *in, size_t n_bytes, void *out, const bds_notch_opts *opts, bds_notch_out *report) {
    const char *who = "bds_notch";
    int64_t n = 0;
    const int fmt = check_entry(ctx, who, format_of, check_args, s, (int64_t)n_bytes, 0, opts, report, &n);
    if (fmt < 0) return fmt;
    if (int rc = check_host_pair(ctx, who, in, out, n_bytes, opts->apply != 0)) return rc;
    return run_pieces(ctx, who, fmt, n, *opts, 0, report, pipe::from_memory(in), pipe::to_memory(out));
}

extern "C" int bds_notch_file(bds_ctx *ctx, const bds_settings *s, const char *path_in, const char *path_out, int64_t n_samples, int64_t piece_samples,
                              const bds_notch_opts *opts, bds_notch_out *report) {
    const char *who = "bds_notch_file";
    const char *why;
    const int fmt = format_of(s, &why);
    if (fmt < 0) return fail(ctx, fmt, "%s: %s", who, why);
    if (!opts || !report) return fail(ctx, BDS_ERR_ARG, "%s: opts or report is NULL", who);
    const bool writes = opts->apply != 0;
    char msg[1024];
    if (int rc = RecordWindow::check_names(path_in, path_out, writes, s->skipNumberOfBytes, msg, sizeof msg)) return fail(ctx, rc, "%s: %s", who, msg);
    RecordWindow w;
    if (int rc = w.open(path_in, fmt, s->skipNumberOfBytes, msg, sizeof msg)) return fail(ctx, rc, "%s", msg);
    const int64_t n = n_samples > 0 ? n_samples : w.have;
    int64_t n_chk = 0;
    if (int rc = w.select(n, msg, sizeof msg)) return fail(ctx, rc, "%s: %s", who, msg);
    if (int rc = check_args(fmt, -1, n, opts, report, &n_chk, msg, sizeof msg)) return fail(ctx, rc, "%s: %s", who, msg);
    if (int rc = check_piece(ctx, who, fmt, piece_samples, *opts)) return rc;
    if (!ctx) return fail(ctx, BDS_ERR_ARG, "%s: ctx is NULL", who);
    if (writes)
        if (int rc = w.open_out(path_out, msg, sizeof msg)) return fail(ctx, rc, "%s", msg);
    auto told = [&](int rc) { return rc ? fail(ctx, rc, "%s: %s", who, msg) : rc; };
    // the bytes in front of the window and behind it go through as they are
    int rc = writes ? told(w.copy_front(0, msg, sizeof msg)) : (int)BDS_OK;
    if (!rc)
        rc = run_pieces(
            ctx, who, fmt, n, *opts, piece_samples, report, [&](int64_t o, size_t nb, uint8_t *to) { return told(w.read(o, nb, to, msg, sizeof msg)); },
            [&](int64_t o, size_t nb, const uint8_t *from) { return told(w.write(o, nb, from, msg, sizeof msg)); });
    if (!rc && writes) rc = told(w.copy_back(0, msg, sizeof msg));
    if (!rc) rc = told(w.close(msg, sizeof msg));
    return rc;
}

extern "C" int bds_notch_dev(bds_ctx *ctx, const bds_settings *s, const void *d_in, size_t n_bytes, void *d_out, const bds_notch_opts *opts,
                             bds_notch_out *report) {
    const char *who = "bds_notch_dev";
    int64_t n = 0;
    const int fmt = check_entry(ctx, who, format_of, check_args, s, (int64_t)n_bytes, 0, opts, report, &n);
    if (fmt < 0) return fmt;
    if (int rc = check_device_pair(ctx, who, fmt, d_in, d_out, n_bytes, opts->apply != 0)) return rc;
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)ctx->stream;
    DevScope scope;
    uint32_t *d_tab = nullptr;
    int32_t *d_est = nullptr;
    unsigned long long *d_tot = nullptr;
    const size_t est_bytes = (size_t)(block_count(n, opts->block_log2) * opts->n_tones * 2) * 4;
    hipError_t e = upload_table(scope, &d_tab);
    if (e == hipSuccess) e = scope.alloc(&d_est, est_bytes);
    if (e == hipSuccess) e = scope.alloc(&d_tot, 3 * 8);
    if (e != hipSuccess) return hip_fail(ctx, who, e);
    unsigned long long tot[3] = {0, 0, 0};
    e = run_device(st, fmt, static_cast<const uint8_t *>(d_in), static_cast<uint8_t *>(d_out), n, opts->first_sample, *opts, d_tab, d_est, d_tot);
    if (e == hipSuccess) e = hipMemcpyAsync(tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && report->est && est_bytes) e = hipMemcpyAsync(report->est, d_est, est_bytes, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);  // the caller's memory is the caller's again
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(ctx, BDS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    fill_report(report, n, *opts, tot);
    return BDS_OK;
}

