// N-point search pair for the B2a grid at N = 198 750 = 53 x 6 x 625: 99.375 MS/s, two code periods (B2a/acquisition.m:134;
// tools/proto_pfa6.py is the NumPy model of the index maps, the layout and the 6-point epilogue).  Opt-in: bds_acq_set_b2a_npoint.
//
// The same twiddle-free 3-D (Good-Thomas) transform as bds_acq_pfa.h / bds_acq_pfa32.h, whose helpers this header uses: spectrum index
// k <-> (k1, k2, k3) = (k mod 53, k mod 6, k mod 625), lag t = (t1 N/53 + t2 N/6 + t3 N/625) mod N.  New here is the FRACTIONAL Doppler
// step: acqStep N / fs = p / q in lowest terms (cfg2: 400 Hz x 2 ms = 4/5), so with the 0-based bin b = q m + j
//   fft(carr_b x)[k] = fft(carr_j x)[k - p m]        (B2a/acquisition.m:187-211: frqBins(b) = IF - band + acqStep (b - 1))
// -- q signal spectra per call instead of one per bin, every cell the rotation of one of them by p m in each dimension.
//
//   row pass     k_pfa6_rows   the wave of k_pfa32_rows: the row pair (k1 = 2 mp, 2 mp + 1) of one k2 x both components x a run of cells of
//                              one PRN, 625 = 25 x 25 in packed fp32 with ONE wave-private LDS exchange, the pair meeting through
//                              v_permlane32_swap.  A workgroup is 3 such waves (k2 = 3 g .. 3 g + 2); the cell's spectrum j = b mod q
//                              and rotation p (b / q) come from its bin.
//   column pass  k_pfa6_cols   wave = 8 lags t3 x all (t1, t2) x both components: 48 A-operand rows = three MFMA row groups, the 96 fragment
//                              registers of k_pfa_cols (there 4 lags x 12 k2).  Row 4 ks + rr of group g is value i = 4 g + rr of the
//                              lane quarter ks: lag 2 ks + i / 6, k2 = i mod 6 -- a lane's 12 accumulators are all 6 k2 of TWO lags of one
//                              real output part, so the 6-point transform is per lane (pfa::real_dft6) and the (re, im) lane pair forms
//                              |y[t2]|^2 and |y[6 - t2]|^2 as S +- X, each output once: even lane t2 = 0, 1, 2, odd lane 3, 5, 4.
//                              Every block is computed once with hi + lo coefficients (no bound pass, no margin to prove), then
//                              w_d |y_d| + w_p |y_p| and the sieve protocol (bds_acq_sieve.h: the top-2 tail in its two halves).
//                              MASKED: per-cell lag ranges and an optional source-cell index (the second-peak pass on the main search's
//                              buffer, B2a/acquisition.m:224-249); only lags inside a range are reported.
//
// Signal spectra [q <= 5][53][6][2 x 625] fp16 complex, every row stored twice (a rotated row is one contiguous read); 5 x 1.59 MB is
// below the 2^24-byte offset range of the row kernel's buffer loads.  Code spectra [slot][2][53][6][625] = conj sC / N.
// Inter-pass buffer of a cell: [tile of 32 lags t3 (20)][mp 27][k2 6][lag in the tile 32][component 2][row of the pair 2] fp16 complex: a
// column workgroup's item (4 waves x 8 lags, all 162 (mp, k2)) is ONE contiguous 83 KB block, the block size of bds_acq_pfa.h.
// 625 = 19 x 32 + 17: the last tile holds 17 lags (its wave 2 has one live lag, its wave 3 none); the 15 pad lags are never written and
// never read (the column pass clamps the lag).
#pragma once

#include "bds_acq_pfa32.h"

namespace bds {
namespace pfa6 {

using pfa::f4;
using pfa::h8;

constexpr int K1 = 53, K2 = 6, K3 = 625;
constexpr long NP = (long)K1 * K2 * K3;  // 198 750
constexpr int MP = 27;                   // row pairs (54 rows: one zero row)
constexpr int NB = 7;                    // output blocks of 16 (106 real outputs -> 112)
constexpr int kMaxQ = 5;                 // signal spectra per call (the denominator of acqStep N / fs)
constexpr int kTileLags = 32, kTiles = (K3 + kTileLags - 1) / kTileLags;
constexpr int kWaveLags = 8;
constexpr size_t kCellElems = (size_t)kTiles * MP * K2 * kTileLags * 4;  // 4-byte (fp16 complex) elements of a cell
__host__ __device__ constexpr size_t bw_piece(int mp, int k2, int t3) {  // element index of the 4-element piece of (mp, k2, t3) in its cell
    return (((size_t)(t3 / kTileLags) * MP + mp) * K2 + k2) * (kTileLags * 4) + (size_t)(t3 % kTileLags) * 4;
}
constexpr int kRowsWaves = 3, kRowsThreads = 64 * kRowsWaves, kColsThreads = 256;
constexpr int kRowsWgs = MP * (K2 / kRowsWaves);                                   // row workgroups per chunk of cells
constexpr int kRowRegion = pfa32::kRowRegion;                                      // float2 elements of a row's LDS region (625 + pad)
constexpr size_t kRowsLds = (size_t)kRowsWaves * 2 * kRowRegion * sizeof(float2);  // 3 waves x 2 rows
constexpr size_t kSpecElems = (size_t)K1 * K2 * 2 * K3;                            // 4-byte elements of one signal spectrum (rows doubled)
constexpr size_t kCoefBytes = pfa::kCoefBytes;                                     // the same 53-point B fragments (pfa::make_coef_frags)
constexpr size_t kColsLds = kCoefBytes;
static_assert(pfa::K1 == K1 && pfa::NB == NB && pfa::MP == MP, "the 53-point stage shares its coefficient fragments with bds_acq_pfa.h");
static_assert(kMaxQ * kSpecElems * 4 < (1u << 24), "signal spectra inside the buffer-load offset range");

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

// ---- row pass ----------------------------------------------------------------------------------------------------------------
struct RowsArgs {
    const uint32_t *Xs;  // signal spectra of the bins 0 .. q - 1, CRT layout, every row doubled: [q][53][6][1250] fp16 complex
    const uint32_t *Cs;  // conjugated, scaled code spectra: [prn slot][component][53][6][625]
    uint32_t *Bw;        // inter-pass buffer [cell][kCellElems]
    const int *bin;      // per cell: Doppler bin b = q m + j -> spectrum j, rotation p m
    const long *cs;      // per cell: element offset of the PRN's spectra in Cs
    int ncells;          // cells of the launch
    int gc;              // cells a workgroup walks (all of one PRN)
    int p, q;            // acqStep N / fs = p / q in lowest terms, 1 <= q <= kMaxQ
};

__global__ __launch_bounds__(kRowsThreads, 2) void k_pfa6_rows(RowsArgs A) {
    extern __shared__ __align__(16) unsigned char pfa6_lds[];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, half = lane >> 5;  // (wave: a scalar)
    const int j = lane & 31;  // thread of the row: 25 of the 32 work
    const bool live = j < 25;
    const int jj = live ? j : 24;
    const int rp = blockIdx.x % kRowsWgs, chunk = blockIdx.x / kRowsWgs;
    const int mp = rp / (K2 / kRowsWaves), k2 = kRowsWaves * (rp % (K2 / kRowsWaves)) + wave;
    const int k1 = 2 * mp + half;
    const bool row_ok = k1 < K1;
    const int k1c = row_ok ? k1 : K1 - 1;
    float2 *region = reinterpret_cast<float2 *>(pfa6_lds) + (size_t)(2 * wave + half) * kRowRegion;  // wave-private
    const int c0 = chunk * A.gc, c1 = min(A.ncells, c0 + A.gc);
    if (c0 >= c1) return;

    // code rows of this wave's PRN (zero for the pad row: its outputs are zeros)
    uint32_t cv[2][25];
    {
        const uint32_t *crow = A.Cs + A.cs[c0] + ((size_t)k1c * K2 + k2) * K3;
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int q = 0; q < 25; ++q) cv[c][q] = row_ok ? crow[(size_t)c * NP + jj + 25 * q] : 0u;
    }
    // W625^(j p), p = 5 p0 + p1, as the product of two factors (bds_acq_pfa.h)
    v2f tw1a[5], tw1b[5];
#pragma unroll
    for (int p = 1; p < 5; ++p) tw1a[p] = pfa::unit((jj * p) % K3, K3), tw1b[p] = pfa::unit((jj * 5 * p) % K3, K3);
    const unsigned region_b = lds_offset(region);

    const __amdgpu_buffer_rsrc_t xs_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)A.Xs, 0, (int)(A.q * kSpecElems * 4), 0x00020000);
    int bin_cur = A.bin[c0];
    for (int cell = c0; cell < c1; ++cell) {
        const int m = bin_cur / A.q, spec = bin_cur - m * A.q, s = m * A.p;  // (scalars)
        const int k1s = ((k1c - s) % K1 + K1) % K1, k2s = ((k2 - s) % K2 + K2) % K2, o3 = (K3 - s % K3) % K3;
        const int xoff = (((spec * K1 + k1s) * K2 + k2s) * (2 * K3) + o3 + jj) * 4;  // < 2^24 bytes
        uint32_t xn[25];
#pragma unroll
        for (int q = 0; q < 25; ++q) xn[q] = __builtin_amdgcn_raw_buffer_load_b32(xs_rsrc, xoff, 100 * q, 0);
        int bin_next = A.bin[min(cell + 1, c1 - 1)];  // (the next cell's bin -- its spectrum index and rotation -- requested behind the loads)
        uint32_t outp[2][25];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            v2f x[25];
            pfa::dot25_summed(xn, cv[c], x);  // X conj(C), the first butterfly layer's sums formed on the addend (bds_acq_pfa.h)
            // stage 1: 25 points over q (k3 = j + 25 q) -> p, twiddle W625^(j p), a[j][p] at 25 j + p
            pfa::pk_radix25<true>(x);
            if (live) {
#pragma unroll
                for (int sl = 0; sl < 25; ++sl) {
                    const int p = pfa::slot25_index(sl);
                    v2f v = x[sl];
                    if (sl / 5) v = pk_cmul(v, tw1a[sl / 5]);
                    if (sl % 5) v = pk_cmul(v, tw1b[sl % 5]);
                    region[25 * j + p] = to_f2(v);
                }
            }
            // (one wave writes and reads the region: LDS operations of a wave complete in order, the wait stands in lds_read25)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // stage 2: lane t' = p: 25 points over j of a[j][p] -> t'': X[t' + 25 t'']
            pfa::lds_read25<25 * 8>(x, region_b + (unsigned)jj * 8u);
            pfa::pk_radix25(x);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int sl = 0; sl < 25; ++sl) {
                const int tq = pfa::slot25_index(sl);
                typedef _Float16 h2 __attribute__((ext_vector_type(2)));
                outp[c][tq] = __builtin_bit_cast(uint32_t, __builtin_convertvector(x[sl], h2));  // round to nearest even
            }
        }
        asm volatile("" : "+v"(bin_next));
        bin_cur = __builtin_amdgcn_readfirstlane(bin_next);
        typedef int v4i __attribute__((ext_vector_type(4)));
        const unsigned long long dst_base = (unsigned long long)(A.Bw + (size_t)cell * kCellElems + bw_piece(mp, k2, 0));
        const v4i dst_words = {(int)(unsigned)dst_base, (int)((unsigned)(dst_base >> 32) & 0xffffu), (int)(unsigned)((kCellElems - bw_piece(mp, k2, 0)) * 4), 0x00020000};
        // the two rows of the pair meet: after the swap half 0 holds (row 0, row 1) of t'' = e, half 1 of t'' = e + 1
#pragma unroll
        for (int e = 0; e < 25; e += 2) {
            uint32_t P[2], Q[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint32_t pe = outp[c][e], qo = e + 1 < 25 ? outp[c][e + 1 < 25 ? e + 1 : e] : 0u;
                const auto r = __builtin_amdgcn_permlane32_swap(pe, qo, false, false);
                P[c] = r[0], Q[c] = r[1];
            }
            const int tq = e + half;
            if (live && tq < 25) {  // lag t3 = j + 25 tq: tile t3 / 32, 16 bytes per lag in the tile
                typedef uint32_t u4 __attribute__((ext_vector_type(4)));
                const int t3s = j + 25 * tq;
                // (issued by hand so that the compiler's counted waits for the next cell's loads do not become vmcnt(0): bds_acq_pfa.h)
                asm volatile("buffer_store_dwordx4 %0, %1, %2, 0 offen\n s_nop 0" ::"v"((u4){P[0], Q[0], P[1], Q[1]}), "v"((int)(bw_piece(0, 0, t3s) * 4)), "s"(dst_words)
                             : "memory");
            }
        }
    }
}

// ---- column pass -------------------------------------------------------------------------------------------------------------
struct ColsArgs {
    const uint32_t *Bw;         // inter-pass buffer
    const uint4 *coef;          // pfa::make_coef_frags
    int ncells;                 // cells of the launch
    float w0, w1;               // magnitude weights (storage scales undone)
    SieveArgs sieve;            // where the pass reports (bds_acq_sieve.h)
    int qchunk;                 // tiles of a cell that follow each other in the work list
    unsigned long long *stats;  // optional (probe): [0] wave items, [1] output blocks whose values were listed or compared
    const int4 *rng;            // MASKED: per-cell searched lag ranges (lo1, hi1, lo2, hi2), inclusive, natural lag order
    const int *src;             // MASKED, optional: the rows of listed cell g lie at cell src[g] of Bw (else at cell g)
};

template <bool MASKED>
__global__ __launch_bounds__(kColsThreads, 2) void k_pfa6_cols(ColsArgs A) {
    extern __shared__ __align__(16) unsigned char pfa6_lds[];
    uint4 *s_coef = reinterpret_cast<uint4 *>(pfa6_lds);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    for (int i = tid; i < pfa::kCoefFrags * 64; i += kColsThreads) s_coef[i] = A.coef[i];
    __syncthreads();
    const int ai = lane & 15, ks = lane >> 4;
    const bool odd = lane & 1;
    auto t2_of = [&](int i) { return odd ? (i == 0 ? 3 : 6 - i) : i; };  // the output t2 behind slot i of this lane
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
        int lo1 = 0, hi1 = (int)NP - 1, lo2 = 1, hi2 = 0;
        size_t bcell = cl;
        if (MASKED) {
            const int4 r = A.rng[cl];
            lo1 = r.x, hi1 = r.y, lo2 = r.z, hi2 = r.w;
            if (A.src) bcell = (size_t)A.src[cl];
        }
        const uint32_t *base = A.Bw + bcell * kCellElems;
        // ---- A fragments: [component][row group][ins], k1 = 4 mg .. 4 mg + 3 with mg = 4 ins + ks, of row ai of the group: value
        // i = 4 g + (ai & 3) of the lane quarter ai >> 2 -> (lag 2 (ai >> 2) + i / 6, k2 = i mod 6)
        uint4 fa[2][3][4];
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const int i = 4 * g + (ai & 3);
            const int t3 = min(t0 + 2 * (ai >> 2) + i / 6, K3 - 1);
            const size_t off = bw_piece(0, i % 6, t3);
#pragma unroll
            for (int ins = 0; ins < 4; ++ins) {
                const int mg = 4 * ins + ks;
                // (rows past the 54th read row pair 26 again: their coefficients are zeros and the buffer holds finite values)
                const uint4 l0 = *reinterpret_cast<const uint4 *>(base + (size_t)min(2 * mg, MP - 1) * K2 * (kTileLags * 4) + off);
                const uint4 l1 = *reinterpret_cast<const uint4 *>(base + (size_t)min(2 * mg + 1, MP - 1) * K2 * (kTileLags * 4) + off);
                fa[0][g][ins] = make_uint4(l0.x, l0.y, l1.x, l1.y);
                fa[1][g][ins] = make_uint4(l0.z, l0.w, l1.z, l1.w);
            }
        }
        // |y|^2 of output block nb: m2[c][3 u + i] for the lane's (t1, lag t0 + 2 ks + u): t2 = t2_of(i)
        auto block = [&](int nb, float (&m2)[2][6]) {
            uint4 fb[4][2];
#pragma unroll
            for (int ins = 0; ins < 4; ++ins)
#pragma unroll
                for (int part = 0; part < 2; ++part) fb[ins][part] = s_coef[((nb * 4 + ins) * 2 + part) * 64 + lane];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                f4 acc[3];
#pragma unroll
                for (int g = 0; g < 3; ++g) acc[g] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ins = 0; ins < 4; ++ins)
#pragma unroll
                    for (int part = 0; part < 2; ++part)
#pragma unroll
                        for (int g = 0; g < 3; ++g)
                            acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, fa[c][g][ins]), __builtin_bit_cast(h8, fb[ins][part]), acc[g], 0, 0, 0);
                // lane (ks, o = lane & 15): acc[g][rr] = row 4 ks + rr of group g = value 4 g + rr: the 6 k2 of lag 2 ks, then of lag 2 ks + 1,
                // of the real (o even) / imaginary (o odd) part of output 16 nb + o
                auto partner = [](float a) { return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, a), 0xB1, 0xf, 0xf, true)); };
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    float v[6], P[4], Q[4];
#pragma unroll
                    for (int k = 0; k < 6; ++k) v[k] = acc[(6 * u + k) >> 2][(6 * u + k) & 3];
                    pfa::real_dft6(v[0], v[1], v[2], v[3], v[4], v[5], P, Q);
                    // the lane pair holds A = DFT6(re z) = P_e + j Q_e and B = DFT6(im z) = P_o + j Q_o; y[t] = A[t] + j B[t],
                    // y[6 - t] = conj A[t] + j conj B[t]: |y[t]|^2 = S + X, |y[6 - t]|^2 = S - X with S = P_e^2 + Q_e^2 + P_o^2 + Q_o^2,
                    // X = 2 (Q_e P_o - P_e Q_o).  With x = Q P' - P Q' (' = the partner lane's) the even lane's S + 2 x is |y[t]|^2, the odd
                    // lane's |y[6 - t]|^2 (bds_acq_pfa.h); t = 0 and 3 are their own mirrors (Q = 0).
                    {
                        const float p0 = P[0] * P[0], p3 = P[3] * P[3];
                        const float S0 = p0 + partner(p0), S3 = p3 + partner(p3);
                        m2[c][3 * u] = odd ? S3 : S0;
                    }
#pragma unroll
                    for (int t = 1; t < 3; ++t) {
                        const float sl = fmaf(Q[t], Q[t], P[t] * P[t]);
                        const float S = sl + partner(sl);
                        float x = partner(P[t]) * Q[t];
                        x = fmaf(-partner(Q[t]), P[t], x);
                        m2[c][3 * u + t] = fmaxf(fmaf(2.f, x, S), 0.f);  // (S + 2 x of a vanishing output may come out below zero)
                    }
                }
            }
        };
        const int t3o = t0 + 2 * ks;  // the first of this lane's two lags t3
        // which of the lane's six outputs of block nb it reports (bit 3 u + i), and their lags
        auto lag_at = [&](int nb, int k) { return lag_of32((16 * nb + (lane & 15)) >> 1, t2_of(k % 3), t3o + k / 3); };
        auto mine_of = [&](int nb) {
            const int t1 = (16 * nb + (lane & 15)) >> 1;
            unsigned mk = 0;
            if (t1 < K1) {
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    bool ok = t3o + k / 3 < K3;
                    if (MASKED) {
                        const int lag = lag_at(nb, k);
                        ok = ok && ((lag >= lo1 && lag <= hi1) || (lag >= lo2 && lag <= hi2));
                    }
                    mk |= ok ? 1u << k : 0u;
                }
            }
            return mk;
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
        // the top-2 tail in its two halves with the relisting loop here (bds_acq_pfa32.h: as a callback the loop cost registers there)
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

// ---- forward transforms: the spectra of the signal (q per call) and of the codes (cached), in the CRT layout -----------------------
// X[k1, k2, k3] = sum x[n] W_N^(-n k) with n = (n1 N/53 + n2 N/6 + n3 N/625) mod N: rows over n3 (625 = 25 x 25 on conjugates), then
// 53 points over n1 and 6 over n2 as plain fp32 sums -- the conventions of pfa32::forward.
// (the row and 53-point kernels are pfa32's, instantiated for K2 = 6)

// 6 points over n2, then the stored form: value * scale (conjugated for the code spectra) as fp16 complex;
// doubled = 1: signal spectra, rows [batch][k1][k2][2 x 625]; 0: code spectra [batch][k1][k2][625]; batches dst_batch_stride elements apart
__global__ __launch_bounds__(256) void k_pfa6_fwd_6(const float2 *U, uint32_t *dst, long dst_batch_stride, int conj_flag, float scale, int doubled) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;  // (k1, k3)
    const int batch = blockIdx.y;
    if (e >= (long)K1 * K3) return;
    const int k1 = (int)(e / K3), k3 = (int)(e % K3);
    const float2 *u = U + (size_t)batch * NP + (size_t)k1 * K2 * K3 + k3;
    float2 x[K2];
#pragma unroll
    for (int n2 = 0; n2 < K2; ++n2) x[n2] = u[(size_t)n2 * K3];
    constexpr float c[6] = {1.f, 0.5f, -0.5f, -1.f, -0.5f, 0.5f};
    constexpr float sn[6] = {0.f, 0.86602540378443865f, 0.86602540378443865f, 0.f, -0.86602540378443865f, -0.86602540378443865f};
    uint32_t *d = dst + (size_t)batch * dst_batch_stride;
#pragma unroll
    for (int k2 = 0; k2 < K2; ++k2) {
        float ar = 0.f, ai = 0.f;
#pragma unroll
        for (int n2 = 0; n2 < K2; ++n2) {  // W6^(-n2 k2) = (c, -sn)[(n2 k2) mod 6]
            const float wr = c[(n2 * k2) % 6], wi = -sn[(n2 * k2) % 6];
            ar = fmaf(x[n2].x, wr, fmaf(-x[n2].y, wi, ar));
            ai = fmaf(x[n2].x, wi, fmaf(x[n2].y, wr, ai));
        }
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const v2f val = (v2f){ar * scale, (conj_flag ? -ai : ai) * scale};
        const uint32_t pk = __builtin_bit_cast(uint32_t, __builtin_convertvector(val, h2));
        if (doubled) {
            d[((size_t)k1 * K2 + k2) * (2 * K3) + k3] = pk;
            d[((size_t)k1 * K2 + k2) * (2 * K3) + K3 + k3] = pk;
        } else {
            d[((size_t)k1 * K2 + k2) * K3 + k3] = pk;
        }
    }
}

// nb transforms (batch = Doppler bin of the signal, component of a PRN's codes): tmp holds 2 x nb x NP float2
template <class Loader>
inline void forward(hipStream_t st, Loader ld, int nb, float2 *tmp, uint32_t *dst, long dst_batch_stride, int conj_flag, float scale, int doubled) {
    float2 *T = tmp, *U = tmp + (size_t)nb * NP;
    hipLaunchKernelGGL((pfa32::k_pfa32_fwd_rows<K2, Loader>), dim3(K1 * K2, nb), dim3(32), 0, st, ld, T);
    hipLaunchKernelGGL(pfa32::k_pfa32_fwd_53<K2>, dim3((K2 * K3 + 255) / 256, nb), dim3(256), 0, st, (const float2 *)T, U);
    hipLaunchKernelGGL(k_pfa6_fwd_6, dim3((K1 * K3 + 255) / 256, nb), dim3(256), 0, st, (const float2 *)U, dst, dst_batch_stride, conj_flag, scale, doubled);
}

struct Plan {  // (bds_acq_pfa.h: the launches of a search pair)
    using RowsArgs = pfa6::RowsArgs;
    using ColsArgs = pfa6::ColsArgs;
    static constexpr long NP = pfa6::NP;
    static constexpr int K3 = pfa6::K3, kRows = K1 * K2, kRowsWgs = pfa6::kRowsWgs, kTiles = pfa6::kTiles;
    static constexpr size_t kCellElems = pfa6::kCellElems, kSpecElems = pfa6::kSpecElems, kCoefBytes = pfa6::kCoefBytes;
    static constexpr void (*make_coef_frags)(uint16_t *) = pfa::make_coef_frags;
    static constexpr bool kChunkList = false, kMasked = true;
    template <class Loader>
    static void forward(hipStream_t st, Loader ld, int nb, float2 *tmp, uint32_t *dst, long dst_batch_stride, int conj_flag, float scale, int doubled) {
        pfa6::forward(st, ld, nb, tmp, dst, dst_batch_stride, conj_flag, scale, doubled);
    }
    template <class Lds>
    static void launch_rows(hipStream_t st, const RowsArgs &A, int chunks, Lds &&lds) {
        pfa::launch_rows_of(k_pfa6_rows, kRowsWgs, kRowsThreads, kRowsLds, st, A, chunks, lds);
    }
    template <class Lds>  // the masked pass where the launch has lag ranges
    static void launch_cols(hipStream_t st, const ColsArgs &A, int qchunk, long grid, Lds &&lds) {
        if (!A.rng)
            pfa::launch_cols_of(k_pfa6_cols<false>, kTiles, kColsThreads, kColsLds, st, A, qchunk, grid, lds);
        else
            pfa::launch_cols_of(k_pfa6_cols<true>, kTiles, kColsThreads, kColsLds, st, A, qchunk, grid, lds);
    }
};

// ---- admission: acqStep N / fs = p / q exactly, in lowest terms ------------------------------------------------------------------
// step and fs are whole numbers of hertz in every admitted setting; the ratio is decided in 64-bit integers (one rounded double would
// take 410 Hz x 2 ms = 0.82 for whatever fraction lies nearest).  False when either is not a whole number or the product overflows.
inline bool step_ratio(double step, double fs, long n, long *p, long *q) {
    if (!(step >= 1.0 && step <= 1e9 && fs >= 1.0 && fs <= 1e12) || step != (double)(long)step || fs != (double)(long)fs || n < 1 || n > (1L << 30)) return false;
    long a = (long)step * n, b = (long)fs;  // a / b = acqStep N / fs
    long x = a, y = b;
    while (y) {
        const long t = x % y;
        x = y, y = t;
    }
    *p = a / x, *q = b / x;
    return true;
}

}  // namespace pfa6
}  // namespace bds
