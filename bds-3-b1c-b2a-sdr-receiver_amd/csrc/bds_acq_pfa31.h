// N-point search pair for the B1C grid at N = 613 800 = 31 x 11 x 1800: 30.69 MS/s (30 samples per chip, the alternative rate of the
// reference's B1C/initSettings.m:57), acqCohT = 10 (tools/proto_pfa31.py is the NumPy model of the index maps, the layouts and the
// small transforms).  Opt-in: bds_acq_set_b1c_npoint.
//
// N = 8 x 9 x 25 x 11 x 31 with pairwise coprime factors: the search is a twiddle-free FIVE-dimensional (Good-Thomas) transform,
// spectrum index k <-> (k mod 31, k mod 11, k mod 8, k mod 9, k mod 25), lag t = sum t_d N / K_d mod N, Doppler bin b = the rotation of
// ONE signal spectrum by s = b * shift in every dimension.  The three dimensions 8, 9, 25 are the ROW (K3 = 1800 = one k3 = k mod 1800,
// lag part t3 = t8 225 + t9 200 + t25 72 mod 1800), so that the pair keeps the shape of its neighbours: rows over k3, then the
// columns (k1, k2) = (k mod 31, k mod 11).  There is no factor 53: nothing of the 53-point machinery is used, the kernels of the
// other three pairs are not touched.
//
//   row pass     k_pfa31_rows  wave = ONE row (k1, k2) x both components x a run of cells of one PRN.  The lanes read the rotated
//                              signal row and the code row in natural k3 order (coalesced: lane + 64 i), the spectrum product goes to
//                              the wave-private LDS region at its CRT position [k3 mod 8][k3 mod 9][k3 mod 25]; three in-place stages
//                              (25 points on pfa::pk_radix25: 72 units; 9 points = 3 x 3: 200 units; 8 points: 225 units) with
//                              wave-level fences only, no workgroup barrier; the lanes then gather the lags t3 = lane + 64 i, round to
//                              fp16 and store (component 0, component 1) as 8-byte pieces, 128 contiguous bytes per 16 lanes.
//                              A workgroup is 4 such waves (4 consecutive rows of the 341); the waves never meet.
//   column pass  k_pfa31_cols  wave = 4 lags t3 x all (t1, t2) x both components.  31 points over k1 on v_mfma_f32_16x16x32_f16: the 31
//                              complex inputs are 62 real K values = two 32-deep steps, the 62 real outputs four blocks of 16;
//                              coefficients hi + lo in fp16.  A operand rows = (lag ks of the wave's four, k2 slot 4 g + rr): three row
//                              groups = 12 slots for the 11 k2 (the twelfth repeats k2 = 10 and is dropped), so a lane's 12
//                              accumulators are all 11 k2 of ONE lag of one real output part: the 11-point transform is per lane
//                              (real_dft11), and the (re, im) lane pair forms |y[t2]|^2 and |y[11 - t2]|^2 as S +- X (k_pfa6_cols):
//                              even lane t2 = 0 .. 5, odd lane t2 = 10 .. 6.  Every block is computed once with hi + lo coefficients
//                              (no bound pass, nothing to prove), then w_d |y_d| + w_p |y_p| and the sieve protocol (bds_acq_sieve.h:
//                              the top-2 tail in its two halves around the relisting loop).
//
// Signal spectrum [31][11][2 x 1800] fp16 complex, every row stored twice (a rotated row is one contiguous read), natural k3 order.
// Code spectra [slot][component][31][11][1800] = conj sC / N.
// Inter-pass buffer of a cell: [tile of 16 lags t3 (113)][k1 31][k2 11][lag in the tile 16][component 2] fp16 complex: a column
// workgroup's item (4 waves x 4 lags, all 341 rows) is ONE contiguous 43.6 KB block.  1800 = 112 x 16 + 8: the last tile holds 8 lags
// (its waves 2 and 3 have none); the 8 pad lags are never written and never read.
#pragma once

#include "bds_acq_pfa32.h"

namespace bds {
namespace pfa31 {

using pfa::f4;
using pfa::h8;

constexpr int K1 = 31, K2 = 11, K3 = 1800;
constexpr int KA = 8, KB = 9, KC = 25;  // K3 = KA KB KC, position of (i8, i9, i25) in a row's LDS region: (i8 * 9 + i9) * 25 + i25
constexpr long NP = (long)K1 * K2 * K3;  // 613 800
constexpr int NB = 4;                    // output blocks of 16 (62 real outputs -> 64)
constexpr int NI = 2;                    // 32-deep MFMA steps (62 real inputs -> 64)
constexpr int kTileLags = 16, kTiles = (K3 + kTileLags - 1) / kTileLags;
constexpr int kWaveLags = 4;
constexpr size_t kCellElems = (size_t)kTiles * K1 * K2 * kTileLags * 2;  // 4-byte (fp16 complex) elements of a cell
__host__ __device__ constexpr size_t bw_piece(int k1, int k2, int t3) {  // element index of the 2-element piece of (k1, k2, t3) in its cell
    return (((size_t)(t3 / kTileLags) * K1 + k1) * K2 + k2) * (kTileLags * 2) + (size_t)(t3 % kTileLags) * 2;
}
constexpr int kRowsWaves = 4, kRowsThreads = 64 * kRowsWaves, kColsThreads = 256;
constexpr int kRowsWgs = (K1 * K2 + kRowsWaves - 1) / kRowsWaves;  // row workgroups per chunk of cells
constexpr int kPerLane = (K3 + 63) / 64;                          // 29 points of a row per lane (the last one: 8 lanes)
constexpr size_t kRowsLds = (size_t)kRowsWaves * K3 * sizeof(float2);
constexpr size_t kSpecElems = (size_t)K1 * K2 * 2 * K3;  // 4-byte elements of the signal spectrum (rows doubled)
constexpr int kCoefFrags = NB * NI * 2;                  // B fragments (16 bytes per lane): [nb][ins][hi / lo]
constexpr size_t kCoefBytes = (size_t)kCoefFrags * 64 * 16;
constexpr size_t kColsLds = kCoefBytes;
static_assert(kSpecElems * 4 < (1u << 24), "signal spectrum inside 2^24 bytes");

__host__ __device__ inline long lag_of(int t1, int t2, int t3) {
    return ((long)t1 * (NP / K1) + (long)t2 * (NP / K2) + (long)t3 * (NP / K3)) % NP;
}
// the same in 32 bits (the sum stays below 3 N)
__device__ __forceinline__ int lag_of32(int t1, int t2, int t3) {
    int l = t1 * (int)(NP / K1) + t2 * (int)(NP / K2) + t3 * (int)(NP / K3);
    l -= l >= (int)NP ? (int)NP : 0;
    l -= l >= (int)NP ? (int)NP : 0;
    return l;
}
// LDS position of spectrum index k3 (CRT) and of lag part t3 (Ruritanian: t8 = t3 mod 8, t9 = 5 t3 mod 9, t25 = 8 t3 mod 25, the
// inverses of 225 mod 8, 200 mod 9 and 72 mod 25)
__host__ __device__ constexpr int pos_of_k3(int k3) { return ((k3 % KA) * KB + k3 % KB) * KC + k3 % KC; }
__host__ __device__ constexpr int pos_of_t3(int t3) { return ((t3 % KA) * KB + (5 * t3) % KB) * KC + (8 * t3) % KC; }
// spectrum index k3 of the CRT coordinates
__host__ __device__ constexpr int k3_of(int i8, int i9, int i25) { return (225 * i8 + 1000 * i9 + 576 * i25) % K3; }

// ---- small inverse transforms of the row pass: out[t] = sum_j x[j] exp(+2 pi j j t / n), in place ---------------------------------
__device__ __forceinline__ v2f cmul(v2f a, v2f w) { return (v2f){a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }
__device__ __forceinline__ v2f mulj(v2f a) { return (v2f){-a.y, a.x}; }
__device__ __forceinline__ void dft3(v2f &a, v2f &b, v2f &c) {
    constexpr float h3 = 0.86602540378443865f;
    const v2f s = b + c, d = h3 * mulj(b - c);
    const v2f m = a - 0.5f * s;
    a = a + s, b = m + d, c = m - d;
}
// j = 3 j1 + j0, t = t0 + 3 t1: 3 points over j1, twiddle W9^(j0 t0), 3 points over j0
__device__ __forceinline__ void dft9(v2f (&x)[9]) {
    dft3(x[0], x[3], x[6]);  // j0 = 0: slot 3 t0 holds A[0][t0]
    dft3(x[1], x[4], x[7]);  // j0 = 1: slot 1 + 3 t0
    dft3(x[2], x[5], x[8]);  // j0 = 2: slot 2 + 3 t0
    x[4] = cmul(x[4], (v2f){0.766044443118978f, 0.6427876096865393f});    // W9^1
    x[7] = cmul(x[7], (v2f){0.17364817766693041f, 0.984807753012208f});   // W9^2
    x[5] = cmul(x[5], (v2f){0.17364817766693041f, 0.984807753012208f});   // W9^2
    x[8] = cmul(x[8], (v2f){-0.9396926207859083f, 0.3420201433256689f});  // W9^4
    // over j0 for each t0: slots 3 t0 + (0, 1, 2) -> t1 = 0, 1, 2, i.e. slot 3 t0 + t1 holds X[t0 + 3 t1]
    dft3(x[0], x[1], x[2]);
    dft3(x[3], x[4], x[5]);
    dft3(x[6], x[7], x[8]);
}
__host__ __device__ constexpr int slot9_index(int s) { return s / 3 + 3 * (s % 3); }  // output index held by slot s
__device__ __forceinline__ void dft4(v2f a0, v2f a1, v2f a2, v2f a3, v2f (&o)[4]) {
    const v2f s02 = a0 + a2, d02 = a0 - a2, s13 = a1 + a3, d13 = mulj(a1 - a3);
    o[0] = s02 + s13, o[2] = s02 - s13, o[1] = d02 + d13, o[3] = d02 - d13;
}
// X[t] = E[t mod 4] + W8^t O[t mod 4]: natural order in, natural order out
__device__ __forceinline__ void dft8(v2f (&x)[8]) {
    constexpr float r2 = 0.70710678118654752f;
    v2f e[4], o[4];
    dft4(x[0], x[2], x[4], x[6], e);
    dft4(x[1], x[3], x[5], x[7], o);
    o[1] = (v2f){r2 * (o[1].x - o[1].y), r2 * (o[1].x + o[1].y)};   // W8^1
    o[2] = mulj(o[2]);                                              // W8^2
    o[3] = (v2f){-r2 * (o[3].x + o[3].y), r2 * (o[3].x - o[3].y)};  // W8^3
#pragma unroll
    for (int t = 0; t < 4; ++t) x[t] = e[t] + o[t], x[t + 4] = e[t] - o[t];
}

// ---- row pass ----------------------------------------------------------------------------------------------------------------
// pfa::RowsArgs with Xs [31][11][2 x 1800], Cs [prn slot][component][31][11][1800], Bw [cell][kCellElems]
__device__ __forceinline__ void wave_sync_lds() {  // the wave's earlier LDS writes are ordered before its later LDS reads (one wave: in order)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(kRowsThreads, 2) void k_pfa31_rows(pfa::RowsArgs A) {
    extern __shared__ __align__(16) unsigned char pfa31_lds[];
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int rp = blockIdx.x % kRowsWgs, chunk = blockIdx.x / kRowsWgs;
    const int row = kRowsWaves * rp + wave;
    if (row >= K1 * K2) return;  // (wave-uniform; the kernel has no workgroup barrier)
    const int k1 = row / K2, k2 = row % K2;
    float2 *region = reinterpret_cast<float2 *>(pfa31_lds) + (size_t)wave * K3;  // wave-private
    const int c0 = chunk * A.gc, c1 = min(A.ncells, c0 + A.gc);
    if (c0 >= c1) return;
    const bool tail = lane < K3 - 64 * (kPerLane - 1);  // lanes of the last, partial point

    // code rows of this wave's PRN.  (They are read again for every cell, from the cache: held in registers, 58 of them, the kernel
    // needs 256 VGPRs and 588 bytes of scratch; like this 190 and none.)
    // (buffer loads: one 32-bit lane offset and a constant per point instead of a 64-bit address per point; what a lane past the row's
    //  end reads -- the next row, or zero past the buffer -- is not used)
    const __amdgpu_buffer_rsrc_t cs_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(A.Cs + A.cs[c0] + (size_t)row * K3), 0, (int)((NP + K3) * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t xs_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)A.Xs, 0, (int)(kSpecElems * 4), 0x00020000);
    // LDS positions of this lane's points: spectrum index k3 = lane + 64 i (low half) and lag t3 = lane + 64 i (high half)
    unsigned pos[kPerLane];
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
        const int e = min(lane + 64 * i, K3 - 1);
        pos[i] = (unsigned)pos_of_k3(e) | ((unsigned)pos_of_t3(e) << 16);
    }
    for (int cell = c0; cell < c1; ++cell) {
        const int s = A.bin[cell] * A.shift;
        const int k1s = ((k1 - s) % K1 + K1) % K1, k2s = ((k2 - s) % K2 + K2) % K2, o3 = (K3 - s % K3) % K3;
        const int xoff = ((k1s * K2 + k2s) * (2 * K3) + o3 + lane) * 4;  // < 2^24 bytes
        uint32_t outp[2][kPerLane];
        auto component = [&](auto comp, uint32_t (&out)[kPerLane]) {
            constexpr int c = decltype(comp)::value;
            // spectrum product X conj(C) (the conjugate is stored) to the CRT position of k3 = lane + 64 i
            // (the signal row is read once per component: the second read is served by the cache and the registers stay free)
            uint32_t xn[kPerLane], cvc[kPerLane];
#pragma unroll
            for (int i = 0; i < kPerLane; ++i) xn[i] = __builtin_amdgcn_raw_buffer_load_b32(xs_rsrc, xoff, 256 * i, 0);
#pragma unroll
            for (int i = 0; i < kPerLane; ++i) cvc[i] = __builtin_amdgcn_raw_buffer_load_b32(cs_rsrc, lane * 4, c * (int)NP * 4 + 256 * i, 0);
#pragma unroll
            for (int i = 0; i < kPerLane; ++i) {
                unsigned p = pos[i];
                asm volatile("" : "+v"(p));  // (keeps the unpacked positions out of registers of their own)
                const v2f x = __builtin_convertvector(__builtin_bit_cast(h2, xn[i]), v2f), w = __builtin_convertvector(__builtin_bit_cast(h2, cvc[i]), v2f);
                if (i < kPerLane - 1 || tail) region[p & 0xffffu] = to_f2(cmul(x, w));
            }
            wave_sync_lds();
            // 25 points over i25: 72 units (i8, i9), contiguous
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int u = lane + 64 * r;
                if (u < KA * KB) {
                    v2f x[25];
#pragma unroll
                    for (int q = 0; q < 25; ++q) x[q] = to_v2f(region[u * KC + q]);
                    pfa::pk_radix25(x);
#pragma unroll
                    for (int sl = 0; sl < 25; ++sl) region[u * KC + pfa::slot25_index(sl)] = to_f2(x[sl]);
                }
            }
            wave_sync_lds();
            // 9 points over i9: 200 units (i8, i25), stride 25
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int u = lane + 64 * r;
                if (u < KA * KC) {
                    float2 *p = region + (u / KC) * (KB * KC) + u % KC;
                    v2f x[9];
#pragma unroll
                    for (int q = 0; q < 9; ++q) x[q] = to_v2f(p[q * KC]);
                    dft9(x);
#pragma unroll
                    for (int sl = 0; sl < 9; ++sl) p[slot9_index(sl) * KC] = to_f2(x[sl]);
                }
            }
            wave_sync_lds();
            // 8 points over i8: 225 units (i9, i25), stride 225
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int u = lane + 64 * r;
                if (u < KB * KC) {
                    v2f x[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) x[q] = to_v2f(region[u + q * (KB * KC)]);
                    dft8(x);
#pragma unroll
                    for (int q = 0; q < 8; ++q) region[u + q * (KB * KC)] = to_f2(x[q]);
                }
            }
            wave_sync_lds();
            // the lags t3 = lane + 64 i, rounded to nearest even
#pragma unroll
            for (int i = 0; i < kPerLane; ++i) {
                unsigned p = pos[i];
                asm volatile("" : "+v"(p));
                out[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector(to_v2f(region[p >> 16]), h2));
            }
            wave_sync_lds();  // region free for the next component / cell
        };
        component(std::integral_constant<int, 0>{}, outp[0]);
        component(std::integral_constant<int, 1>{}, outp[1]);
        // lag t3 = lane + 64 i lies in tile (lane >> 4) + 4 i: one address per lane, a constant step per point
        constexpr size_t kTileElems = (size_t)K1 * K2 * kTileLags * 2;
        static_assert(kTileLags == 16, "64 lanes = 4 tiles");
        uint32_t *dst = A.Bw + (size_t)cell * kCellElems + bw_piece(k1, k2, 0) + (size_t)(lane >> 4) * kTileElems + (size_t)(lane & 15) * 2;
#pragma unroll
        for (int i = 0; i < kPerLane; ++i)
            if (i < kPerLane - 1 || tail) *reinterpret_cast<uint2 *>(dst + (size_t)i * (4 * kTileElems)) = make_uint2(outp[0][i], outp[1][i]);
    }
}

// ---- column pass -------------------------------------------------------------------------------------------------------------
// B operand of the 31-point stage in fragment order: frag[(nb * NI + ins) * 2 + part][lane] = 8 halves
//   coef[kappa = 32 ins + 8 (lane >> 4) + e][o = 16 nb + (lane & 15)],  kappa = 2 k1 + ri_in, o = 2 t1 + ri_out,
//   y_re = sum c x_re - s x_im, y_im = sum s x_re + c x_im, c + j s = exp(+2 pi j k1 t1 / 31); part 0 = fp16(coef), part 1 = fp16(coef - hi)
inline void make_coef_frags(uint16_t *out /* kCoefBytes / 2 halves */) {
    auto f2h = [](float f) { return __half_as_ushort(__float2half_rn(f)); };
    auto h2f = [](uint16_t h) { return __half2float(__ushort_as_half(h)); };
    for (int nb = 0; nb < NB; ++nb)
        for (int ins = 0; ins < NI; ++ins)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) {
                    const int kap = 32 * ins + 8 * (lane >> 4) + e, o = 16 * nb + (lane & 15);
                    const int k1 = kap >> 1, ri = kap & 1, t1 = o >> 1, ro = o & 1;
                    double v = 0.0;
                    if (k1 < K1 && t1 < K1) {
                        const double ang = 2.0 * M_PI * (double)((k1 * t1) % K1) / K1;
                        const double c = cos(ang), s = sin(ang);
                        v = ro == 0 ? (ri == 0 ? c : -s) : (ri == 0 ? s : c);
                    }
                    const uint16_t hi = f2h((float)v);
                    const uint16_t lo = f2h((float)(v - (double)h2f(hi)));
                    out[((((size_t)nb * NI + ins) * 2 + 0) * 64 + lane) * 8 + e] = hi;
                    out[((((size_t)nb * NI + ins) * 2 + 1) * 64 + lane) * 8 + e] = lo;
                }
}

// real 11-point transform F[t] = sum_k v[k] exp(+2 pi j k t / 11) of a real sequence: P = re F, Q = im F for t = 0 .. 5 (F[11 - t] = conj F[t])
__device__ __forceinline__ void real_dft11(const float (&v)[11], float (&P)[6], float (&Q)[6]) {
    constexpr float c[11] = {1.0f, 0.8412535328311812f, 0.41541501300188644f, -0.142314838273285f, -0.654860733945285f, -0.9594929736144974f,
                             -0.9594929736144975f, -0.6548607339452852f, -0.14231483827328523f, 0.41541501300188605f, 0.8412535328311812f};
    constexpr float s[11] = {0.0f, 0.5406408174555976f, 0.9096319953545183f, 0.9898214418809328f, 0.7557495743542583f, 0.28173255684142967f,
                             -0.2817325568414294f, -0.7557495743542582f, -0.9898214418809327f, -0.9096319953545186f, -0.5406408174555974f};
    float e[6], d[6];
#pragma unroll
    for (int k = 1; k < 6; ++k) e[k] = v[k] + v[11 - k], d[k] = v[k] - v[11 - k];
    P[0] = v[0] + ((e[1] + e[2]) + (e[3] + e[4])) + e[5], Q[0] = 0.f;
#pragma unroll
    for (int t = 1; t < 6; ++t) {
        float p = v[0], q = 0.f;
#pragma unroll
        for (int k = 1; k < 6; ++k) p = fmaf(e[k], c[(k * t) % 11], p), q = fmaf(d[k], s[(k * t) % 11], q);
        P[t] = p, Q[t] = q;
    }
}

// pfa::ColsArgs; stats[0] counts wave items, stats[1] the output blocks whose values were listed or compared; dbg is not used
__global__ __launch_bounds__(kColsThreads, 2) void k_pfa31_cols(pfa::ColsArgs A) {
    extern __shared__ __align__(16) unsigned char pfa31_lds[];
    uint4 *s_coef = reinterpret_cast<uint4 *>(pfa31_lds);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    for (int i = tid; i < kCoefFrags * 64; i += kColsThreads) s_coef[i] = A.coef[i];
    __syncthreads();
    const int ai = lane & 15, ks = lane >> 4;
    const bool odd = lane & 1;
    auto t2_of = [&](int i) { return odd ? K2 - i : i; };  // the output t2 behind slot i of this lane (the odd lane's slot 0 is no output)
    constexpr int kBlocks = kTiles;
    const int qch = A.qchunk > 0 ? A.qchunk : 1, nq = (kBlocks + qch - 1) / qch;
    // work list: qch adjacent tiles of one cell, then the same tiles of the NEXT cell (bds_acq_pfa.h)
    const unsigned ncl = (unsigned)A.ncells, uq = (unsigned)qch;
    unsigned b = blockIdx.x % uq, cl = (blockIdx.x / uq) % ncl, q = blockIdx.x / (uq * ncl);
    const unsigned gb = gridDim.x % uq, gcl = (gridDim.x / uq) % ncl, gq = gridDim.x / (uq * ncl);
    for (; q < (unsigned)nq; b += gb, cl += gcl + (b >= uq ? (b -= uq, 1u) : 0u), q += gq + (cl >= ncl ? (cl -= ncl, 1u) : 0u)) {
        const int blk = (int)(q * uq + b);
        const int t0 = kTileLags * blk + kWaveLags * wave;
        if (blk >= kBlocks || t0 >= K3) continue;
        const int cell = A.sieve.cell0 + cl;
        const uint32_t *base = A.Bw + (size_t)cl * kCellElems;
        // ---- A fragments: [component][row group][ins], k1 = 4 mg .. 4 mg + 3 with mg = 4 ins + ks, of row ai of the group:
        // lag t0 + (ai >> 2), k2 slot 4 g + (ai & 3) (slot 11 reads k2 = 10 again; its output is dropped)
        uint4 fa[2][3][NI];
        {
            const int t3 = min(t0 + (ai >> 2), K3 - 1);
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                const size_t off = bw_piece(0, min(4 * g + (ai & 3), K2 - 1), t3);
#pragma unroll
                for (int ins = 0; ins < NI; ++ins) {
                    const int mg = 4 * ins + ks;
                    // (row 31 reads row 30 again: its coefficients are zeros and the buffer holds finite values)
                    uint2 l[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) l[r] = *reinterpret_cast<const uint2 *>(base + (size_t)min(4 * mg + r, K1 - 1) * K2 * (kTileLags * 2) + off);
                    fa[0][g][ins] = make_uint4(l[0].x, l[1].x, l[2].x, l[3].x);
                    fa[1][g][ins] = make_uint4(l[0].y, l[1].y, l[2].y, l[3].y);
                }
            }
        }
        // |y|^2 of output block nb: m2[c][i] for the lane's (t1, lag t0 + ks): t2 = t2_of(i)
        auto block = [&](int nb, float (&m2)[2][6]) {
            uint4 fb[NI][2];
#pragma unroll
            for (int ins = 0; ins < NI; ++ins)
#pragma unroll
                for (int part = 0; part < 2; ++part) fb[ins][part] = s_coef[((nb * NI + ins) * 2 + part) * 64 + lane];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                f4 acc[3];
#pragma unroll
                for (int g = 0; g < 3; ++g) acc[g] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ins = 0; ins < NI; ++ins)
#pragma unroll
                    for (int part = 0; part < 2; ++part)
#pragma unroll
                        for (int g = 0; g < 3; ++g)
                            acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, fa[c][g][ins]), __builtin_bit_cast(h8, fb[ins][part]), acc[g], 0, 0, 0);
                // lane (ks, o = lane & 15): acc[g][rr] = row 4 ks + rr of group g = k2 slot 4 g + rr of lag t0 + ks, of the real (o even) /
                // imaginary (o odd) part of output 16 nb + o
                float v[11], P[6], Q[6];
#pragma unroll
                for (int k = 0; k < 11; ++k) v[k] = acc[k >> 2][k & 3];
                real_dft11(v, P, Q);
                // the lane pair holds A = DFT11(re z) = P_e + j Q_e and B = DFT11(im z) = P_o + j Q_o; y[t] = A[t] + j B[t],
                // y[11 - t] = conj A[t] + j conj B[t]: with x = Q P' - P Q' (' = the partner lane's) the even lane's S + 2 x is
                // |y[t]|^2, the odd lane's |y[11 - t]|^2 (bds_acq_pfa6.h); t = 0 is its own mirror (Q = 0)
                {
                    const float p0 = P[0] * P[0];
                    m2[c][0] = p0 + pfa32::row_partner(p0);
                }
#pragma unroll
                for (int t = 1; t < 6; ++t) {
                    const float sl = fmaf(Q[t], Q[t], P[t] * P[t]);
                    const float S = sl + pfa32::row_partner(sl);
                    float x = pfa32::row_partner(P[t]) * Q[t];
                    x = fmaf(-pfa32::row_partner(Q[t]), P[t], x);
                    m2[c][t] = fmaxf(fmaf(2.f, x, S), 0.f);  // (S + 2 x of a vanishing output may come out below zero)
                }
            }
        };
        const int t3o = t0 + ks;  // this lane's lag t3
        auto lag_at = [&](int nb, int k) { return lag_of32((16 * nb + (lane & 15)) >> 1, t2_of(k), t3o); };
        // which of the lane's six outputs of block nb it reports (bit i)
        auto mine_of = [&](int nb) {
            const int t1 = (16 * nb + (lane & 15)) >> 1;
            return t1 < K1 && t3o < K3 ? (odd ? 0x3eu : 0x3fu) : 0u;
        };
        // the cell's maximum so far and the PRN's running bound
        const SieveBounds bd = sieve_bounds(A.sieve, cell);
        const float wsum2 = A.w0 * A.w0 + A.w1 * A.w1;
        const float lim = sieve_limit(A.sieve, bd);
        if (A.stats && lane == 0) atomicAdd(A.stats, 1ull);
        // The skip test (bds_acq_sieve.h) per output block, on the exact squares: a block that passes it has nothing to report and skips
        // its square roots.
        SieveTop2 top;
        unsigned fmask = 0;
        for (int nb = 0; nb < NB; ++nb) {
            float m2[2][6];
            block(nb, m2);
            const unsigned mk = mine_of(nb);
            float bmax = 0.f;
#pragma unroll
            for (int k = 0; k < 6; ++k) bmax = fmaxf(bmax, (mk >> k) & 1 ? m2[0][k] + m2[1][k] : 0.f);
            if (!__builtin_amdgcn_ballot_w64(!sieve_below(bmax, wsum2, lim))) continue;  // (wave-uniform)
            fmask |= 1u << nb;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if ((mk >> k) & 1) top.offer(A.w0 * __builtin_amdgcn_sqrtf(m2[0][k]) + A.w1 * __builtin_amdgcn_sqrtf(m2[1][k]), lag_at(nb, k));
        }
        if (A.stats && lane == 0) atomicAdd(A.stats + 1, (unsigned long long)__builtin_popcount(fmask));
        // the top-2 tail in its two halves with the relisting loop here (bds_acq_pfa32.h)
        const SieveTop2Plan plan = sieve_top2_begin(A.sieve, bd, lane, cell, top);
        if (plan.exhaustive) {
            for (int nb = 0; nb < NB; ++nb) {
                if (!((fmask >> nb) & 1)) continue;
                float m2[2][6];
                block(nb, m2);
                const unsigned mk = mine_of(nb);
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    float a = -1.f;
                    if ((mk >> k) & 1) a = A.w0 * __builtin_amdgcn_sqrtf(m2[0][k]) + A.w1 * __builtin_amdgcn_sqrtf(m2[1][k]);
                    sieve_append(A.sieve, lane, a >= plan.thr, a, lag_at(nb, k), cell);
                }
            }
        }
        sieve_top2_end(A.sieve, bd, lane, cell, top, plan);
    }
}

// ---- forward transforms: the spectra of the signal (one per call) and of the codes (cached) ---------------------------------------
// X[k] = sum x[n] W_N^(-n k) with n = sum n_d N / K_d mod N over the five dimensions (31, 11, 8, 9, 25): a gather into the array
// [31][11][8][9][25], one dense stage of plain fp32 sums per dimension, and the stored form in natural k3 order.
template <class Loader>
__global__ __launch_bounds__(256) void k_pfa31_fwd_load(Loader ld, float2 *T /* [batch][NP] */) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int batch = blockIdx.y;
    if (e >= NP) return;
    const int n25 = (int)(e % KC), n9 = (int)(e / KC % KB), n8 = (int)(e / (KC * KB) % KA), n2 = (int)(e / K3 % K2), n1 = (int)(e / ((long)K3 * K2));
    const long n = ((long)n1 * (NP / K1) + (long)n2 * (NP / K2) + (long)n8 * (NP / KA) + (long)n9 * (NP / KB) + (long)n25 * (NP / KC)) % NP;
    T[(size_t)batch * NP + e] = ld(batch, n);
}

// out[outer][k][inner] = sum_n in[outer][n][inner] W_K^(-n k), inner = S elements
template <int K, int S>
__global__ __launch_bounds__(256) void k_pfa31_fwd_dim(const float2 *in, float2 *out) {
    __shared__ float2 w[K];
    if (threadIdx.x < K) {
        float sn, cs;
        sincospif(-2.0f * (float)threadIdx.x / (float)K, &sn, &cs);
        w[threadIdx.x] = make_float2(cs, sn);
    }
    __syncthreads();
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int batch = blockIdx.y;
    if (e >= NP / K) return;
    const size_t at = (size_t)batch * NP + (size_t)(e / S) * K * S + (size_t)(e % S);
    float2 x[K];
#pragma unroll
    for (int n = 0; n < K; ++n) x[n] = in[at + (size_t)n * S];
    for (int k = 0; k < K; ++k) {
        float ar = 0.f, ai = 0.f;
        int idx = 0;
#pragma unroll
        for (int n = 0; n < K; ++n) {
            const float2 ww = w[idx];
            ar = fmaf(x[n].x, ww.x, fmaf(-x[n].y, ww.y, ar));
            ai = fmaf(x[n].x, ww.y, fmaf(x[n].y, ww.x, ai));
            idx += k;
            idx -= idx >= K ? K : 0;
        }
        out[at + (size_t)k * S] = make_float2(ar, ai);
    }
}

// the stored form: value * scale (conjugated for the code spectra) as fp16 complex at its natural k3;
// doubled = 1: signal spectrum, rows [k1][k2][2 x 1800]; 0: code spectra [batch][k1][k2][1800], batches dst_batch_stride elements apart
__global__ __launch_bounds__(256) void k_pfa31_fwd_store(const float2 *U, uint32_t *dst, long dst_batch_stride, int conj_flag, float scale, int doubled) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int batch = blockIdx.y;
    if (e >= NP) return;
    const int i25 = (int)(e % KC), i9 = (int)(e / KC % KB), i8 = (int)(e / (KC * KB) % KA);
    const long row = e / K3;
    const int k3 = k3_of(i8, i9, i25);
    const float2 u = U[(size_t)batch * NP + e];
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const v2f val = (v2f){u.x * scale, (conj_flag ? -u.y : u.y) * scale};
    const uint32_t pk = __builtin_bit_cast(uint32_t, __builtin_convertvector(val, h2));
    uint32_t *d = dst + (size_t)batch * dst_batch_stride;
    if (doubled) {
        d[(size_t)row * (2 * K3) + k3] = pk;
        d[(size_t)row * (2 * K3) + K3 + k3] = pk;
    } else {
        d[(size_t)row * K3 + k3] = pk;
    }
}

// nb transforms (component of a PRN's codes; the signal: one): tmp holds 2 x nb x NP float2
template <class Loader>
inline void forward(hipStream_t st, Loader ld, int nb, float2 *tmp, uint32_t *dst, long dst_batch_stride, int conj_flag, float scale, int doubled) {
    float2 *T = tmp, *U = tmp + (size_t)nb * NP;
    auto grid = [&](long n) { return dim3((unsigned)((n + 255) / 256), nb); };
    hipLaunchKernelGGL(k_pfa31_fwd_load<Loader>, grid(NP), dim3(256), 0, st, ld, T);
    hipLaunchKernelGGL((k_pfa31_fwd_dim<K1, K2 * K3>), grid(NP / K1), dim3(256), 0, st, (const float2 *)T, U);
    hipLaunchKernelGGL((k_pfa31_fwd_dim<K2, K3>), grid(NP / K2), dim3(256), 0, st, (const float2 *)U, T);
    hipLaunchKernelGGL((k_pfa31_fwd_dim<KA, KB * KC>), grid(NP / KA), dim3(256), 0, st, (const float2 *)T, U);
    hipLaunchKernelGGL((k_pfa31_fwd_dim<KB, KC>), grid(NP / KB), dim3(256), 0, st, (const float2 *)U, T);
    hipLaunchKernelGGL((k_pfa31_fwd_dim<KC, 1>), grid(NP / KC), dim3(256), 0, st, (const float2 *)T, U);
    hipLaunchKernelGGL(k_pfa31_fwd_store, grid(NP), dim3(256), 0, st, (const float2 *)U, dst, dst_batch_stride, conj_flag, scale, doubled);
}

struct Plan {  // (bds_acq_pfa.h: the launches of a search pair)
    using RowsArgs = pfa::RowsArgs;
    using ColsArgs = pfa::ColsArgs;
    static constexpr long NP = pfa31::NP;
    static constexpr int K3 = pfa31::K3, kRows = K1 * K2, kRowsWgs = pfa31::kRowsWgs, kTiles = pfa31::kTiles;
    static constexpr size_t kCellElems = pfa31::kCellElems, kSpecElems = pfa31::kSpecElems, kCoefBytes = pfa31::kCoefBytes;
    static constexpr void (*make_coef_frags)(uint16_t *) = pfa31::make_coef_frags;  // the 31-point stage's own table
    static constexpr bool kChunkList = false, kMasked = false;
    template <class Loader>
    static void forward(hipStream_t st, Loader ld, int nb, float2 *tmp, uint32_t *dst, long dst_batch_stride, int conj_flag, float scale, int doubled) {
        pfa31::forward(st, ld, nb, tmp, dst, dst_batch_stride, conj_flag, scale, doubled);
    }
    template <class Lds>
    static void launch_rows(hipStream_t st, const RowsArgs &A, int chunks, Lds &&lds) {
        pfa::launch_rows_of(k_pfa31_rows, kRowsWgs, kRowsThreads, kRowsLds, st, A, chunks, lds);
    }
    template <class Lds>
    static void launch_cols(hipStream_t st, const ColsArgs &A, int qchunk, long grid, Lds &&lds) {
        pfa::launch_cols_of(k_pfa31_cols, kTiles, kColsThreads, kColsLds, st, A, qchunk, grid, lds);
    }
};

}  // namespace pfa31
}  // namespace bds
