// Frame-synchronisation correlators on the prompt outputs of tracking:
//   B1C  B1C/include/BCNAV1decoding.m:66-91   bits = sign(Pilot_I_P | Pilot_Q_P),
//        Secondary = generate2ndCode(PRN) (1800 chips), XcorrResult = xcorr(bits, Secondary),
//        second half, index = find(abs(.) >= 1799.5)
//   B2a  B2a/include/BCNAV2decoding.m:69-97   bits = sign(I_P), preamble_ms = kron(preamble_bits,
//        secondCode) (24 x 5 = 120 taps), index = find(abs(xcorr second half) > 115)
// The correlation is integer (+-1 against +-1), so the device result equals the reference's exactly.
// One thread per lag; the pattern sits in LDS, the thresholded bits are int8 in HBM.
// bds_nav_decode goes on from there (BCNAV1decoding.m:93-189, BCNAV2decoding.m:99-159): the candidates are listed on the device
// and every (channel, candidate) frame is decoded by one workgroup of one launch; fields and merging are host C++ (bds_nav.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "bds_internal.h"
#include "bds_nav.h"

namespace bds {

static constexpr int kMaxPattern = 1800;

// bits(bits > 0) = 1; bits(bits <= 0) = -1   (NaN > 0 is false -> -1, as in MATLAB)
__global__ __launch_bounds__(256) void k_sync_bits(const double *__restrict__ prompt, long n, int8_t *__restrict__ bits) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        bits[i] = prompt[i] > 0 ? 1 : -1;
}

// out[ch][lag] = sum_k bits[ch][lag + k] * pattern[ch][k],  lag = 0 .. M-1, M = max(n, m): the second
// half of xcorr(bits, pattern), which zero-pads the shorter input to the longer one's length.
__global__ __launch_bounds__(256) void k_sync_xcorr(const int8_t *__restrict__ bits, int n,
                                                    const int8_t *__restrict__ pattern, int m, int M,
                                                    int32_t *__restrict__ out) {
    __shared__ int8_t s_pat[kMaxPattern];
    const int ch = blockIdx.y;
    for (int i = threadIdx.x; i < m; i += blockDim.x) s_pat[i] = pattern[(long)ch * m + i];
    __syncthreads();
    const int8_t *b = bits + (long)ch * n;
    for (int lag = blockIdx.x * blockDim.x + threadIdx.x; lag < M; lag += gridDim.x * blockDim.x) {
        int acc = 0;
        const int kmax = lag < n ? min(m, n - lag) : 0;
        for (int k = 0; k < kmax; ++k) acc += (int)b[lag + k] * (int)s_pat[k];
        out[(long)ch * M + lag] = acc;
    }
}

// B2a/include/unpack_cplx.m:16-63: byte -> (I1, Q1, I2, Q2) int8; low nibble first; per nibble bit 0 / 1
// = sign of I / Q, bit 2 / 3 = magnitude 1 or 3 of I / Q.  One 32-bit store per input byte.
__device__ __forceinline__ uint32_t unpack_nibble(uint32_t v) {
    const int i = ((v & 4) ? 3 : 1) * ((v & 1) ? -1 : 1);
    const int q = ((v & 8) ? 3 : 1) * ((v & 2) ? -1 : 1);
    return (uint32_t)(uint8_t)(int8_t)i | ((uint32_t)(uint8_t)(int8_t)q << 8);
}
__global__ __launch_bounds__(256) void k_unpack_cplx(const uint8_t *__restrict__ in, size_t n, uint32_t *__restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t b = in[i];
        out[i] = unpack_nibble(b & 15u) | (unpack_nibble(b >> 4) << 16);
    }
}

// ---- navigation decoding (bds_nav_decode): the candidates stay on the device between the correlator and the decoders -----------
// index = find(abs(xcorr) > thr)' per channel, in ascending order: one workgroup per channel walks the M lags 256 at a time and
// numbers the hits with a ballot prefix.  idx has M slots per channel, so every hit has one.
// (thr = 1799 for B1C: the correlation is an integer, so abs(.) >= 1799.5 (BCNAV1decoding.m:91) is abs(.) > 1799; 115 for B2a, :97.)
__global__ __launch_bounds__(256) void k_nav_find(const int32_t *__restrict__ xc, int M, int thr, int32_t *__restrict__ idx,
                                                  int32_t *__restrict__ cnt) {
    __shared__ int s_wave[4];
    __shared__ int s_base;
    const int ch = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int start = 0; start < M; start += 256) {
        const int lag = start + tid;
        const bool hit = lag < M && abs(xc[(long)ch * M + lag]) > thr;
        const unsigned long long b = __ballot(hit);
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int off = s_base + __popcll(b & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) off += s_wave[w];
        if (hit) idx[(long)ch * M + off] = lag + 1;  // 1-based like find()
        __syncthreads();
        if (tid == 0) s_base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    if (tid == 0) cnt[ch] = s_base;
}

// Workgroup b of a decode launch -> (channel, candidate): first[c] = candidates of the channels before c, first[n_ch] = all.
__device__ __forceinline__ int nav_candidate(const int32_t *__restrict__ first, int n_ch, const int32_t *__restrict__ idx, int M,
                                             int *ch_out) {
    const int b = blockIdx.x;
    int ch = 0;
    while (ch + 1 < n_ch && b >= first[ch + 1]) ++ch;
    *ch_out = ch;
    return idx[(long)ch * M + (b - first[ch])] - 1;  // 0-based first prompt of the candidate
}

// (value, hypothesis) -> one int whose maximum is "largest value, lowest hypothesis on ties" (MATLAB's max); |value| <= 51
__device__ __forceinline__ int nav_key(int value, int hyp) { return ((value + 64) << 8) | (255 - hyp); }

// One B-CNAV1 frame per workgroup (BCNAV1decoding.m:100-173): bits, BCH(21,6) in either polarity, BCH(51,8) in the polarity kept,
// the 36 x 48 de-interleaver, the two CRC-24Q remainders, 878 bits packed.  The code-word correlation is n - 2 popcount(x ^ cw);
// the inverted frame's correlations are the negatives, so minimum and maximum of one pass serve both polarities.
__global__ __launch_bounds__(256) void k_nav_b1c(const double *__restrict__ data, int n, int n_ch, const int32_t *__restrict__ idx,
                                                 int M, const int32_t *__restrict__ first, const uint32_t *__restrict__ cw21,
                                                 const uint64_t *__restrict__ cw51, const uint32_t *__restrict__ crc,
                                                 NavRaw *__restrict__ out) {
    __shared__ uint8_t s_bit[1800], s_out[BDS_NAV_BITS_B1C + 2];
    __shared__ unsigned s_x21, s_crc[2];
    __shared__ unsigned long long s_x51;
    __shared__ int s_max1, s_min1, s_max2;
    const int tid = threadIdx.x;
    int ch;
    const int i0 = nav_candidate(first, n_ch, idx, M, &ch);
    NavRaw *o = out + blockIdx.x;
    if (tid < 112) o->bits[tid] = 0;
    if (i0 < 0 || (long)i0 + 1800 > n) {  // (a hit of all 1800 taps lies wholly inside the series; kept as the window's bound)
        if (tid == 0) o->status = 0, o->polarity = 0, o->bch1_max = 0, o->bch2_max = 0;
        return;
    }
    if (tid == 0) s_x21 = 0, s_x51 = 0, s_crc[0] = 0, s_crc[1] = 0, s_max1 = 0, s_min1 = 0, s_max2 = 0;
    __syncthreads();
    const double *p = data + (long)ch * n + i0;
    for (int s = tid; s < 1800; s += 256) {
        const bool bit = p[s] > 0;  // bits(bits > 0) = 1; bits(bits <= 0) = 0 (:105-106); NaN > 0 is false
        s_bit[s] = bit;
        if (bit && s < 21) atomicOr(&s_x21, 1u << (20 - s));
        if (bit && s >= 21 && s < 72) atomicOr(&s_x51, 1ull << (71 - s));
    }
    __syncthreads();
    if (tid < 64) {
        const int c = 21 - 2 * __popc(s_x21 ^ cw21[tid]);
        atomicMax(&s_max1, nav_key(c, tid));
        atomicMax(&s_min1, nav_key(-c, tid));
    }
    __syncthreads();
    int pol = 0, h1 = 0, m1 = (s_max1 >> 8) - 64;
    if (m1 >= 20) {  // maxValue >= threshold (BCH21_6Decoding.m:97)
        pol = 1, h1 = 255 - (s_max1 & 255);
    } else {  // bits = 1 - bits, and once more (:116-126)
        m1 = (s_min1 >> 8) - 64;
        if (m1 >= 20) pol = -1, h1 = 255 - (s_min1 & 255);
    }
    if (pol == 0) {
        if (tid == 0) o->status = 0, o->polarity = 0, o->bch1_max = m1, o->bch2_max = 0;
        return;
    }
    {
        const int c = pol * (51 - 2 * __popcll(s_x51 ^ cw51[tid]));
        atomicMax(&s_max2, nav_key(c, tid));
    }
    __syncthreads();
    const int m2 = (s_max2 >> 8) - 64, h2 = 255 - (s_max2 & 255);
    if (m2 < 50) {  // BCH51_8Decoding.m:95, then `continue` (:138-140)
        if (tid == 0) o->status = BDS_NAV_BCH1_OK, o->polarity = pol, o->bch1_max = m1, o->bch2_max = m2;
        return;
    }
    const unsigned inv = pol < 0;
    unsigned r2 = 0, r3 = 0;
    for (int k = tid; k < BDS_NAV_BITS_B1C; k += 256) {
        unsigned v;
        if (k < 6) {
            v = (h1 >> (5 - k)) & 1;  // decodedNav(1:6) = hypoBits(pos, :), most significant digit first
        } else if (k < 14) {
            v = (h2 >> (13 - k)) & 1;
        } else if (k < 614) {
            // temp_Bits = reshape(bits(73:end), [36, 48]) is column-major; sub-frame 2 = the 25 rows that are not 3, 6, .., 33,
            // row after row (:146-151); 0-based these are 0, 1, 3, 4, .., 33, 34 and 35
            const int q = k - 14, j = q / 48, c = q % 48, r = j < 24 ? (j >> 1) * 3 + (j & 1) : 35;
            v = s_bit[72 + c * 36 + r] ^ inv;
            if (v) r2 ^= crc[599 - q];
        } else {
            const int q = k - 614, j = q / 48, c = q % 48, r = 3 * j + 2;  // rows 3, 6, .. (:147,153-154)
            v = s_bit[72 + c * 36 + r] ^ inv;
            if (v) r3 ^= crc[263 - q];
        }
        s_out[k] = (uint8_t)v;
    }
    if (tid < 2) s_out[BDS_NAV_BITS_B1C + tid] = 0;
    atomicXor(&s_crc[0], r2);
    atomicXor(&s_crc[1], r3);
    __syncthreads();
    if (tid < (BDS_NAV_BITS_B1C + 7) / 8) {
        unsigned byte = 0;
        for (int j = 0; j < 8; ++j) byte = (byte << 1) | s_out[8 * tid + j];
        o->bits[tid] = (uint8_t)byte;
    }
    if (tid == 0) {
        o->status = BDS_NAV_BCH1_OK | BDS_NAV_BCH2_OK | (s_crc[0] == 0 ? BDS_NAV_CRC1_OK : 0) | (s_crc[1] == 0 ? BDS_NAV_CRC2_OK : 0);
        o->polarity = pol, o->bch1_max = m1, o->bch2_max = m2;
    }
}

// One B-CNAV2 message per workgroup (BCNAV2decoding.m:103-139) on the thresholded +-1 series of k_sync_bits.
__constant__ int8_t c_preamble[24] = {-1, -1, -1, 1, 1, 1, -1, 1, 1, -1, 1, 1, -1, -1, 1, -1, -1, -1, -1, 1, -1, 1, 1, 1};  // :74
__global__ __launch_bounds__(256) void k_nav_b2a(const int8_t *__restrict__ bits, int n, int n_ch, const int32_t *__restrict__ idx,
                                                 int M, const int32_t *__restrict__ first, const uint32_t *__restrict__ crc,
                                                 NavRaw *__restrict__ out) {
    __shared__ int8_t s_sym[600];
    __shared__ uint8_t s_out[BDS_NAV_BITS_B2A];
    __shared__ unsigned s_crc, s_differs;
    const int tid = threadIdx.x;
    int ch;
    const int i0 = nav_candidate(first, n_ch, idx, M, &ch);
    NavRaw *o = out + blockIdx.x;
    if (tid < 112) o->bits[tid] = 0;
    if (i0 < 0 || n - i0 < 3000) {  // length(bits) - index(i) + 1 >= 600*5 (:105), index = i0 + 1
        if (tid == 0) o->status = BDS_NAV_SHORT, o->polarity = 0, o->bch1_max = 0, o->bch2_max = 0;
        return;
    }
    if (tid == 0) s_crc = 0, s_differs = 0;
    const int8_t *b = bits + (long)ch * n + i0;
    for (int s = tid; s < 600; s += 256) {
        const int8_t *q = b + 5 * s;
        const int sum = q[0] + q[1] + q[2] - q[3] + q[4];  // secondCode = [1 1 1 -1 1] (:69,115); five odd terms: never 0
        s_sym[s] = sum > 0 ? 1 : -1;
    }
    __syncthreads();
    if (tid < 24 && s_sym[tid] != c_preamble[tid]) atomicOr(&s_differs, 1u);  // ~isequal(navBits(1:24), preamble_bits) (:122)
    __syncthreads();
    const int pol = s_differs ? -1 : 1;
    unsigned r = 0;
    for (int k = tid; k < BDS_NAV_BITS_B2A; k += 256) {
        const unsigned v = pol * s_sym[24 + k] < 0;  // navBits(25:end), NavDataLogic = decodedNavBits < 0.5 (:127-136)
        s_out[k] = (uint8_t)v;
        if (v) r ^= crc[287 - k];
    }
    atomicXor(&s_crc, r);
    __syncthreads();
    if (tid < BDS_NAV_BITS_B2A / 8) {
        unsigned byte = 0;
        for (int j = 0; j < 8; ++j) byte = (byte << 1) | s_out[8 * tid + j];
        o->bits[tid] = (uint8_t)byte;
    }
    if (tid == 0) o->status = s_crc == 0 ? BDS_NAV_CRC1_OK : 0, o->polarity = pol, o->bch1_max = 0, o->bch2_max = 0;
}

static hipStream_t st(bds_ctx *ctx) { return (hipStream_t)ctx->stream; }

// device to device on the context's stream: n_bytes packed bytes -> 4 n_bytes int8 (I, Q pairs); d_out is dword-aligned
int unpack_cplx_device(bds_ctx *ctx, const uint8_t *d_in, size_t n_bytes, int8_t *d_out) {
    if (!n_bytes) return BDS_OK;
    hipLaunchKernelGGL(k_unpack_cplx, dim3((unsigned)std::min<size_t>(8192, (n_bytes + 255) / 256)), dim3(256), 0, st(ctx), d_in, n_bytes,
                       reinterpret_cast<uint32_t *>(d_out));
    BDS_HIP(ctx, hipGetLastError());
    return BDS_OK;
}

}  // namespace bds

using namespace bds;

extern "C" int bds_sync_pattern(int signal, int prn, int8_t *out, int cap) {
    if (!out) return BDS_ERR_ARG;
    if (signal == BDS_SIGNAL_B1C) {
        if (cap < 1800) return BDS_ERR_ARG;
        return gen_secondary(prn, out);  // BCNAV1decoding.m:80
    }
    if (signal == BDS_SIGNAL_B2A) {
        if (cap < 120) return BDS_ERR_ARG;
        static const int8_t second[5] = {1, 1, 1, -1, 1};  // BCNAV2decoding.m:69
        static const int8_t preamble[24] = {-1, -1, -1, 1, 1, 1, -1, 1, 1, -1, 1, 1,
                                            -1, -1, 1, -1, -1, -1, -1, 1, -1, 1, 1, 1};  // :74
        for (int i = 0; i < 24; ++i)
            for (int j = 0; j < 5; ++j) out[i * 5 + j] = (int8_t)(preamble[i] * second[j]);  // kron, :78
        return 120;
    }
    return BDS_ERR_ARG;
}

extern "C" int bds_frame_sync(bds_ctx *ctx, int signal, int n_ch, const int32_t *prn, const double *prompt, int n,
                              int32_t *xcorr, int32_t *index, int32_t *n_index, int cap) {
    if (!ctx || !prn || !prompt || n_ch < 1 || n < 1) return BDS_ERR_ARG;
    if (signal != BDS_SIGNAL_B1C && signal != BDS_SIGNAL_B2A) return fail(ctx, BDS_ERR_ARG, "bds_frame_sync: signal invalid");
    const int m = signal == BDS_SIGNAL_B1C ? 1800 : 120;
    const int M = std::max(n, m);
    std::vector<int8_t> pat((size_t)n_ch * m);
    for (int c = 0; c < n_ch; ++c) {
        const int p = signal == BDS_SIGNAL_B1C ? prn[c] : 1;
        if (bds_sync_pattern(signal, p, &pat[(size_t)c * m], m) < 0)
            return fail(ctx, BDS_ERR_ARG, "bds_frame_sync: channel %d PRN %d out of range", c + 1, prn[c]);
    }
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    double *d_p = nullptr;
    int8_t *d_bits = nullptr, *d_pat = nullptr;
    int32_t *d_out = nullptr;
    const size_t np = (size_t)n_ch * n;
    auto release = [&]() {
        for (void *q : {(void *)d_p, (void *)d_bits, (void *)d_pat, (void *)d_out})
            if (q) (void)hipFree(q);
    };
    hipError_t e = hipMalloc((void **)&d_p, sizeof(double) * np);
    if (e == hipSuccess) e = hipMalloc((void **)&d_bits, np);
    if (e == hipSuccess) e = hipMalloc((void **)&d_pat, pat.size());
    if (e == hipSuccess) e = hipMalloc((void **)&d_out, sizeof(int32_t) * (size_t)n_ch * M);
    if (e != hipSuccess) {
        release();
        return fail(ctx, BDS_ERR_NOMEM, "bds_frame_sync: %s", hipGetErrorString(e));
    }
    (void)hipMemcpyAsync(d_p, prompt, sizeof(double) * np, hipMemcpyHostToDevice, st(ctx));
    (void)hipMemcpyAsync(d_pat, pat.data(), pat.size(), hipMemcpyHostToDevice, st(ctx));
    hipLaunchKernelGGL(k_sync_bits, dim3((unsigned)std::min<size_t>(1024, (np + 255) / 256)), dim3(256), 0, st(ctx),
                       (const double *)d_p, (long)np, d_bits);
    hipLaunchKernelGGL(k_sync_xcorr, dim3((unsigned)((M + 255) / 256), (unsigned)n_ch), dim3(256), 0, st(ctx),
                       (const int8_t *)d_bits, n, (const int8_t *)d_pat, m, M, d_out);
    std::vector<int32_t> h((size_t)n_ch * M);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d_out, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost, st(ctx));
    if (e == hipSuccess) e = hipStreamSynchronize(st(ctx));
    release();
    if (e != hipSuccess) return fail(ctx, BDS_ERR_HIP, "bds_frame_sync: %s", hipGetErrorString(e));
    if (xcorr) std::copy(h.begin(), h.end(), xcorr);
    int total = 0;
    for (int c = 0; c < n_ch; ++c) {
        int cnt = 0;
        for (int lag = 0; lag < M; ++lag) {
            const int v = std::abs(h[(size_t)c * M + lag]);
            // abs(XcorrResult) >= 1799.5 (BCNAV1decoding.m:91); abs(tlmXcorrResult) > 115 (BCNAV2decoding.m:97)
            const bool hit = signal == BDS_SIGNAL_B1C ? (double)v >= 1799.5 : v > 115;
            if (!hit) continue;
            if (index && cnt < cap) index[(size_t)c * cap + cnt] = lag + 1;  // 1-based like find()
            ++cnt;
        }
        if (n_index) n_index[c] = cnt;
        total += cnt;
    }
    return total;
}

extern "C" int bds_nav_decode(bds_ctx *ctx, const bds_settings *settings, int n_ch, const int32_t *prn, const double *sync_prompt,
                              const double *data_prompt, int n, bds_nav_frame *frames, int32_t *n_frames, int cap, bds_eph *eph,
                              double *firstSubFrame, double *TOW) {
    if (!ctx) return BDS_ERR_ARG;
    if (!settings || !prn || !sync_prompt || !eph || !firstSubFrame || !TOW)
        return fail(ctx, BDS_ERR_ARG, "bds_nav_decode: settings, prn, sync_prompt, eph, firstSubFrame and TOW are required");
    if (n_ch < 1 || n < 1 || cap < 0 || (cap > 0 && !frames))
        return fail(ctx, BDS_ERR_ARG, "bds_nav_decode: n_ch %d, n %d, cap %d%s", n_ch, n, cap, cap > 0 && !frames ? " without frames" : "");
    const int signal = settings->signal;
    if (signal != BDS_SIGNAL_B1C && signal != BDS_SIGNAL_B2A) return fail(ctx, BDS_ERR_ARG, "bds_nav_decode: settings.signal invalid");
    const bool b1c = signal == BDS_SIGNAL_B1C;
    if (!b1c && data_prompt && data_prompt != sync_prompt)
        return fail(ctx, BDS_ERR_ARG, "bds_nav_decode: B2a decodes the series it synchronises on; data_prompt must be NULL");
    if ((double)n_ch * (double)std::max(n, 1800) > 1e9) return fail(ctx, BDS_ERR_ARG, "bds_nav_decode: n_ch * n too large");
    for (int c = 0; c < n_ch; ++c)
        if (eph[c].size != sizeof(bds_eph))
            return fail(ctx, BDS_ERR_ARG, "bds_nav_decode: eph[%d].size is %u, not sizeof(bds_eph) = %zu", c, eph[c].size, sizeof(bds_eph));
    const int m = b1c ? 1800 : 120;
    const int M = std::max(n, m);
    std::vector<int8_t> pat((size_t)n_ch * m);
    for (int c = 0; c < n_ch; ++c)
        if (bds_sync_pattern(signal, b1c ? prn[c] : 1, &pat[(size_t)c * m], m) < 0)
            return fail(ctx, BDS_ERR_ARG, "bds_nav_decode: channel %d PRN %d out of range", c + 1, prn[c]);
    const NavTables &tab = nav_tables();
    const bool own_data = b1c && data_prompt && data_prompt != sync_prompt;

    BDS_HIP(ctx, hipSetDevice(ctx->device));
    DevScope dev;
    const size_t np = (size_t)n_ch * n;
    double *d_sync = nullptr, *d_data = nullptr;
    int8_t *d_bits = nullptr, *d_pat = nullptr;
    int32_t *d_xc = nullptr, *d_idx = nullptr, *d_cnt = nullptr, *d_first = nullptr;
    NavTables *d_tab = nullptr;
    NavRaw *d_out = nullptr;
    hipError_t e = dev.alloc(&d_sync, sizeof(double) * np);
    if (e == hipSuccess && own_data) e = dev.alloc(&d_data, sizeof(double) * np);
    if (e == hipSuccess) e = dev.alloc(&d_bits, np);
    if (e == hipSuccess) e = dev.alloc(&d_pat, pat.size());
    if (e == hipSuccess) e = dev.alloc(&d_xc, sizeof(int32_t) * (size_t)n_ch * M);
    if (e == hipSuccess) e = dev.alloc(&d_idx, sizeof(int32_t) * (size_t)n_ch * M);
    if (e == hipSuccess) e = dev.alloc(&d_cnt, sizeof(int32_t) * n_ch);
    if (e == hipSuccess) e = dev.alloc(&d_first, sizeof(int32_t) * (n_ch + 1));
    if (e == hipSuccess) e = dev.alloc(&d_tab, sizeof(NavTables));
    if (e != hipSuccess) return fail(ctx, BDS_ERR_NOMEM, "bds_nav_decode: %s", hipGetErrorString(e));
    // the prompts cross to the device once; bits, correlation and candidate lists stay there
    e = hipMemcpyAsync(d_sync, sync_prompt, sizeof(double) * np, hipMemcpyHostToDevice, st(ctx));
    if (e == hipSuccess && own_data) e = hipMemcpyAsync(d_data, data_prompt, sizeof(double) * np, hipMemcpyHostToDevice, st(ctx));
    if (e == hipSuccess) e = hipMemcpyAsync(d_pat, pat.data(), pat.size(), hipMemcpyHostToDevice, st(ctx));
    if (e == hipSuccess) e = hipMemcpyAsync(d_tab, &tab, sizeof(NavTables), hipMemcpyHostToDevice, st(ctx));
    if (e != hipSuccess) return fail(ctx, BDS_ERR_HIP, "bds_nav_decode: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_sync_bits, dim3((unsigned)std::min<size_t>(1024, (np + 255) / 256)), dim3(256), 0, st(ctx),
                       (const double *)d_sync, (long)np, d_bits);
    hipLaunchKernelGGL(k_sync_xcorr, dim3((unsigned)((M + 255) / 256), (unsigned)n_ch), dim3(256), 0, st(ctx),
                       (const int8_t *)d_bits, n, (const int8_t *)d_pat, m, M, d_xc);
    hipLaunchKernelGGL(k_nav_find, dim3((unsigned)n_ch), dim3(256), 0, st(ctx), (const int32_t *)d_xc, M, b1c ? 1799 : 115, d_idx, d_cnt);
    std::vector<int32_t> cnt(n_ch), first(n_ch + 1, 0);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int32_t) * n_ch, hipMemcpyDeviceToHost, st(ctx));
    if (e == hipSuccess) e = hipStreamSynchronize(st(ctx));
    if (e != hipSuccess) return fail(ctx, BDS_ERR_HIP, "bds_nav_decode: %s", hipGetErrorString(e));
    for (int c = 0; c < n_ch; ++c) {
        if (cnt[c] < 0 || cnt[c] > M) return fail(ctx, BDS_ERR_HIP, "bds_nav_decode: channel %d: candidate count %d", c + 1, cnt[c]);
        first[c + 1] = first[c] + cnt[c];
    }
    const int total = first[n_ch];
    std::vector<NavRaw> raw(total);
    std::vector<int32_t> index(total);
    if (total > 0) {
        e = dev.alloc(&d_out, sizeof(NavRaw) * (size_t)total);
        if (e != hipSuccess) return fail(ctx, BDS_ERR_NOMEM, "bds_nav_decode: %s", hipGetErrorString(e));
        e = hipMemcpyAsync(d_first, first.data(), sizeof(int32_t) * (n_ch + 1), hipMemcpyHostToDevice, st(ctx));
        if (e != hipSuccess) return fail(ctx, BDS_ERR_HIP, "bds_nav_decode: %s", hipGetErrorString(e));
        if (b1c)
            hipLaunchKernelGGL(k_nav_b1c, dim3((unsigned)total), dim3(256), 0, st(ctx), (const double *)(own_data ? d_data : d_sync), n,
                               n_ch, (const int32_t *)d_idx, M, (const int32_t *)d_first, (const uint32_t *)d_tab->cw21,
                               (const uint64_t *)d_tab->cw51, (const uint32_t *)d_tab->crc, d_out);
        else
            hipLaunchKernelGGL(k_nav_b2a, dim3((unsigned)total), dim3(256), 0, st(ctx), (const int8_t *)d_bits, n, n_ch,
                               (const int32_t *)d_idx, M, (const int32_t *)d_first, (const uint32_t *)d_tab->crc, d_out);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(raw.data(), d_out, sizeof(NavRaw) * (size_t)total, hipMemcpyDeviceToHost, st(ctx));
        for (int c = 0; c < n_ch && e == hipSuccess; ++c)
            if (cnt[c])
                e = hipMemcpyAsync(&index[first[c]], d_idx + (size_t)c * M, sizeof(int32_t) * cnt[c], hipMemcpyDeviceToHost, st(ctx));
        if (e == hipSuccess) e = hipStreamSynchronize(st(ctx));
        if (e != hipSuccess) return fail(ctx, BDS_ERR_HIP, "bds_nav_decode: %s", hipGetErrorString(e));
    }
    dev.release();

    // the decoding loops' bookkeeping (BCNAV1decoding.m:176-188, BCNAV2decoding.m:141-157), candidate after candidate
    int entered = 0;
    for (int c = 0; c < n_ch; ++c) {
        nav_eph_init(&eph[c]);
        firstSubFrame[c] = TOW[c] = INFINITY;
        for (int k = 0; k < cnt[c]; ++k) {
            NavRaw &r = raw[first[c] + k];
            const uint32_t need = b1c ? (BDS_NAV_CRC1_OK | BDS_NAV_CRC2_OK) : BDS_NAV_CRC1_OK;
            if (!(r.status & BDS_NAV_SHORT) && (r.status & need) == need) {
                if (nav_enter(signal, r.bits, &eph[c])) {
                    r.status |= BDS_NAV_ENTERED;
                    ++entered;
                    if (std::isinf(firstSubFrame[c])) {
                        firstSubFrame[c] = index[first[c] + k];
                        TOW[c] = b1c ? eph[c].TOW : eph[c].SOW;
                    }
                } else {
                    r.status |= BDS_NAV_PRN_RANGE;
                }
            }
            if (k < cap) {
                bds_nav_frame &f = frames[(size_t)c * cap + k];
                f.size = sizeof(bds_nav_frame);
                f.index = index[first[c] + k];
                f.status = r.status, f.polarity = r.polarity, f.bch1_max = r.bch1_max, f.bch2_max = r.bch2_max;
                std::memcpy(f.bits, r.bits, sizeof(f.bits));
            }
        }
        if (n_frames) n_frames[c] = cnt[c];
    }
    return entered;
}

extern "C" int bds_unpack_cplx(bds_ctx *ctx, const uint8_t *in, size_t n_bytes, int8_t *out) {
    if (!ctx || (!in && n_bytes) || (!out && n_bytes)) return BDS_ERR_ARG;
    if (n_bytes == 0) return BDS_OK;
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    uint8_t *d_in = nullptr;
    uint32_t *d_out = nullptr;
    hipError_t e = hipMalloc((void **)&d_in, n_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&d_out, 4 * n_bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(d_in, in, n_bytes, hipMemcpyHostToDevice, st(ctx));
    if (e == hipSuccess && unpack_cplx_device(ctx, d_in, n_bytes, reinterpret_cast<int8_t *>(d_out))) e = hipErrorLaunchFailure;
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, 4 * n_bytes, hipMemcpyDeviceToHost, st(ctx));
    if (e == hipSuccess) e = hipStreamSynchronize(st(ctx));
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (e != hipSuccess) return fail(ctx, BDS_ERR_HIP, "bds_unpack_cplx: %s", hipGetErrorString(e));
    return BDS_OK;
}

// unpack_cplx(filename_in, filename_out): 4e6-byte pieces in the reference (:11), 64 MiB here
extern "C" int bds_unpack_cplx_file(bds_ctx *ctx, const char *path_in, const char *path_out) {
    if (!ctx || !path_in || !path_out) return BDS_ERR_ARG;
    FILE *fi = fopen(path_in, "rb");
    if (!fi) return fail(ctx, BDS_ERR_IO, "Unable to read file %s", path_in);
    FILE *fo = fopen(path_out, "wb");
    if (!fo) {
        fclose(fi);
        return fail(ctx, BDS_ERR_IO, "Unable to write file %s", path_out);
    }
    const size_t piece = 64u << 20;
    std::vector<uint8_t> a(piece);
    std::vector<int8_t> b(4 * piece);
    int rc = BDS_OK;
    for (;;) {
        const size_t n = fread(a.data(), 1, piece, fi);
        if (n == 0) break;
        if ((rc = bds_unpack_cplx(ctx, a.data(), n, b.data()))) break;
        if (fwrite(b.data(), 1, 4 * n, fo) != 4 * n) {
            rc = fail(ctx, BDS_ERR_IO, "short write on %s", path_out);
            break;
        }
    }
    fclose(fi);
    fclose(fo);
    return rc;
}
