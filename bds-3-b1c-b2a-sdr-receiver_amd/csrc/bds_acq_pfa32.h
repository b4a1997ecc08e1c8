// N-point search pair for the B1C grid at N = 1 060 000 = 53 x 32 x 625: 53 MS/s, the sampling rate of the reference's own
// B1C/initSettings.m (tools/proto_pfa32.py is the NumPy model of the index maps).
//
// The same twiddle-free 3-D (Good-Thomas) transform as bds_acq_pfa.h, whose helpers and argument structures this header uses:
// spectrum index k <-> (k1, k2, k3) = (k mod 53, k mod 32, k mod 625), lag t = (t1 N/53 + t2 N/32 + t3 N/625) mod N, Doppler bin b =
// the rotation of ONE signal spectrum by s = b * shift in each dimension.  The kernels of bds_acq_pfa.h are not touched: this pair
// stands beside them.
//
//   row pass     k_pfa32_rows  wave = the row pair (k1 = 2 mp, 2 mp + 1) of one k2 x both components x a run of cells of one PRN; a
//                              row lives in one 32-lane half, 25 live lanes x 25 points: spectrum product (v_dot2_f32_f16), inverse
//                              625-point transform over k3 as 25 x 25 in packed fp32 with ONE exchange through a wave-private LDS
//                              region (no workgroup barrier), lane t' ends with the lags t' + 25 t''; the two rows meet through
//                              v_permlane32_swap and leave as 16-byte pieces.  A workgroup is 4 such waves (4 consecutive k2).
//   column pass  k_pfa32_cols  wave = 2 lags t3 x all (t1, t2) x both components: 53 points over k1 on v_mfma_f32_16x16x32_f16 (data =
//                              A operand, rows = (lag, k2 mod 8), four row groups k2 = 8 m + ..; coefficients hi + lo in fp16), so that
//                              a lane holds 16 of the 32 k2 of one real output part: k2 = 8 m + 4 h + rr, h = bit 4 of the lane.  The
//                              32-point transform over k2 = 8 m + u -> t2 = ta + 4 tb: 4 points over m in the lane (the lane pair
//                              (re, im) splits the ta: even / odd), twiddle W32^(u ta), 4 -> 8 points over rr in the lane, and the last
//                              radix-2 level (h) across the two 16-lane rows by v_permlane16_swap: the rows split the tb.  A lane ends
//                              with 8 of the 32 outputs of its (t1, t3).  Then w_d |y_d| + w_p |y_p| and the sieve protocol
//                              (bds_acq_sieve.h: the top-2 tail of k_pfa_cols).  (fa[2][4][4] is 128 VGPRs; all 32 k2 per lane would
//                              be 256.)  Every output block is computed with hi + lo coefficients once: there is no hi-only bound pass
//                              and hence no margin to prove; the Cauchy-Schwarz test on the EXACT |y_d|^2 + |y_p|^2 only decides
//                              whether a block's square roots and list bookkeeping are needed.
//
// Inter-pass buffer of a cell: [tile of 8 lags t3 (79)][mp 27][k2 32][lag in the tile 8][component 2][row of the pair 2] fp16 complex:
// a column workgroup's item (4 waves x 2 lags, all 864 (mp, k2)) is ONE contiguous 108 KB block.  625 = 78 x 8 + 1: the last tile
// holds one lag; its seven pad lags are never written and never read (the column pass clamps the lag).
#pragma once

#include "bds_acq_pfa.h"

namespace bds {
namespace pfa32 {

using pfa::f4;
using pfa::h8;

constexpr int K1 = 53, K2 = 32, K3 = 625;
constexpr long NP = (long)K1 * K2 * K3;  // 1 060 000
constexpr int MP = 27;                   // row pairs (54 rows: one zero row)
constexpr int NB = 7;                    // output blocks of 16 (106 real outputs -> 112)
constexpr int kTileLags = 8, kTiles = (K3 + kTileLags - 1) / kTileLags;
constexpr size_t kCellElems = (size_t)kTiles * MP * K2 * kTileLags * 4;  // 4-byte (fp16 complex) elements of a cell
__host__ __device__ constexpr size_t bw_piece(int mp, int k2, int t3) {  // element index of the 4-element piece of (mp, k2, t3) in its cell
    return (((size_t)(t3 / kTileLags) * MP + mp) * K2 + k2) * (kTileLags * 4) + (size_t)(t3 % kTileLags) * 4;
}
constexpr int kRowsThreads = 256, kColsThreads = 256;
constexpr int kRowsWgs = MP * (K2 / 4);                              // row workgroups per chunk of cells: 4 waves = 4 k2 of one row pair
constexpr int kRowRegion = 640;                                      // float2 elements of a row's LDS region (625 + pad)
constexpr size_t kRowsLds = (size_t)4 * 2 * kRowRegion * sizeof(float2);  // 4 waves x 2 rows
constexpr size_t kSpecElems = (size_t)K1 * K2 * 2 * K3;              // 4-byte elements of the signal spectrum (rows doubled)
constexpr size_t kCoefBytes = pfa::kCoefBytes;                       // the same 53-point B fragments (pfa::make_coef_frags)
constexpr size_t kColsLds = kCoefBytes;
static_assert(pfa::K1 == K1 && pfa::NB == NB && pfa::MP == MP, "the 53-point stage shares its coefficient fragments with bds_acq_pfa.h");

__host__ __device__ inline long lag_of(int t1, int t2, int t3) {
    return ((long)t1 * (NP / K1) + (long)t2 * (NP / K2) + (long)t3 * (NP / K3)) % NP;
}

// ---- row pass ----------------------------------------------------------------------------------------------------------------
// pfa::RowsArgs with Xs [53][32][2 x 625], Cs [prn slot][component][53][32][625], Bw [cell][kCellElems]
__global__ __launch_bounds__(kRowsThreads, 2) void k_pfa32_rows(pfa::RowsArgs A) {
    extern __shared__ __align__(16) unsigned char pfa32_lds[];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, half = lane >> 5;  // (wave: a scalar)
    const int j = lane & 31;  // thread of the row: 25 of the 32 work
    const bool live = j < 25;
    const int jj = live ? j : 24;
    const int rp = blockIdx.x % kRowsWgs, chunk = blockIdx.x / kRowsWgs;
    const int mp = rp / (K2 / 4), k2 = 4 * (rp % (K2 / 4)) + wave;
    const int k1 = 2 * mp + half;
    const bool row_ok = k1 < K1;
    const int k1c = row_ok ? k1 : K1 - 1;
    float2 *region = reinterpret_cast<float2 *>(pfa32_lds) + (size_t)(2 * wave + half) * kRowRegion;  // wave-private
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

    const __amdgpu_buffer_rsrc_t xs_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)A.Xs, 0, K1 * K2 * 2 * K3 * 4, 0x00020000);
    int bin_cur = A.bin[c0];
    for (int cell = c0; cell < c1; ++cell) {
        const int s = bin_cur * A.shift;
        const int k1s = ((k1c - s) % K1 + K1) % K1, k2s = ((k2 - s) % K2 + K2) % K2, o3 = (K3 - s % K3) % K3;
        const int xoff = ((k1s * K2 + k2s) * (2 * K3) + o3 + jj) * 4;  // < 2^24 bytes
        uint32_t xn[25];
#pragma unroll
        for (int q = 0; q < 25; ++q) xn[q] = __builtin_amdgcn_raw_buffer_load_b32(xs_rsrc, xoff, 100 * q, 0);
        int bin_next = A.bin[min(cell + 1, c1 - 1)];
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
            if (live && tq < 25) {  // lag t3 = j + 25 tq
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
__device__ __forceinline__ float row_partner(float a) {  // the value of lane ^ 1
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, a), 0xB1, 0xf, 0xf, true));
}
// out[c] = sum_r a[r] exp(+2 pi j r c / 4)
__device__ __forceinline__ void dft4(v2f a0, v2f a1, v2f a2, v2f a3, v2f (&o)[4]) {
    const v2f s02 = a0 + a2, d02 = a0 - a2, s13 = a1 + a3, d13 = a1 - a3;
    o[0] = s02 + s13, o[2] = s02 - s13, o[1] = pk_addj(d02, d13), o[3] = pk_subj(d02, d13);
}

// pfa::ColsArgs; stats[0] counts wave items, stats[1] the output blocks whose values were listed or compared; dbg is not used
__global__ __launch_bounds__(kColsThreads, 2) void k_pfa32_cols(pfa::ColsArgs A) {
    extern __shared__ __align__(16) unsigned char pfa32_lds[];
    uint4 *s_coef = reinterpret_cast<uint4 *>(pfa32_lds);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    for (int i = tid; i < pfa::kCoefFrags * 64; i += kColsThreads) s_coef[i] = A.coef[i];
    __syncthreads();
    const int ai = lane & 15, ks = lane >> 4;
    const int ag = ai >> 3, ar = ai & 7;  // A operand: row ai = (lag ag of the item's two, k2 = 8 m + ar)
    const int h = ks & 1, e = lane & 1;   // accumulators: k2 = 8 m + 4 h + rr of the real (e = 0) / imaginary part of output (lane & 15) >> 1
    const int og = lane >> 5;             // ... of lag t0 + og
    const bool odd = e != 0;
    // W32^(u ta), u = 4 h + rr, ta = e + 2 tai
    v2f tw[4][2];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int tai = 0; tai < 2; ++tai) tw[rr][tai] = pfa::unit(((4 * h + rr) * (e + 2 * tai)) % 32, 32);
    auto t2_of = [&](int i) { return e + 2 * (i >> 2) + 16 * h + 4 * (i & 3); };  // the output t2 behind slot i = 4 tai + tbi of this lane
    constexpr int kBlocks = kTiles;
    const int qch = A.qchunk > 0 ? A.qchunk : 1, nq = (kBlocks + qch - 1) / qch;
    // work list: qch adjacent tiles of one cell, then the same tiles of the NEXT cell (bds_acq_pfa.h)
    const unsigned ncl = (unsigned)A.ncells, uq = (unsigned)qch;
    unsigned b = blockIdx.x % uq, cl = (blockIdx.x / uq) % ncl, q = blockIdx.x / (uq * ncl);
    const unsigned gb = gridDim.x % uq, gcl = (gridDim.x / uq) % ncl, gq = gridDim.x / (uq * ncl);
    for (; q < (unsigned)nq; b += gb, cl += gcl + (b >= uq ? (b -= uq, 1u) : 0u), q += gq + (cl >= ncl ? (cl -= ncl, 1u) : 0u)) {
        const int blk = (int)(q * uq + b);
        const int t0 = kTileLags * blk + 2 * wave;
        if (blk >= kBlocks || t0 >= K3) continue;
        const int cell = A.sieve.cell0 + cl;
        const int t3 = min(t0 + ag, K3 - 1);
        const uint32_t *base = A.Bw + (size_t)cl * kCellElems;
        // ---- A fragments: [component][m][ins], k1 = 4 mg .. 4 mg + 3 with mg = 4 ins + ks, of (k2 = 8 m + ar, t3)
        uint4 fa[2][4][4];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int ins = 0; ins < 4; ++ins) {
                const int mg = 4 * ins + ks;
                const size_t off = bw_piece(0, 8 * m + ar, t3);
                // (rows past the 54th read row pair 26 again: their coefficients are zeros and the buffer holds finite values)
                const uint4 l0 = *reinterpret_cast<const uint4 *>(base + (size_t)min(2 * mg, MP - 1) * K2 * (kTileLags * 4) + off);
                const uint4 l1 = *reinterpret_cast<const uint4 *>(base + (size_t)min(2 * mg + 1, MP - 1) * K2 * (kTileLags * 4) + off);
                fa[0][m][ins] = make_uint4(l0.x, l0.y, l1.x, l1.y);
                fa[1][m][ins] = make_uint4(l0.z, l0.w, l1.z, l1.w);
            }
        // |y|^2 of output block nb: m2[c][i = 4 tai + tbi] for the lane's (t1, t3): t2 = t2_of(i)
        auto block = [&](int nb, float (&m2)[2][8]) {
            uint4 fb[4][2];
#pragma unroll
            for (int ins = 0; ins < 4; ++ins)
#pragma unroll
                for (int part = 0; part < 2; ++part) fb[ins][part] = s_coef[((nb * 4 + ins) * 2 + part) * 64 + lane];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                f4 acc[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) acc[m] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ins = 0; ins < 4; ++ins)
#pragma unroll
                    for (int part = 0; part < 2; ++part)
#pragma unroll
                        for (int m = 0; m < 4; ++m)
                            acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, fa[c][m][ins]), __builtin_bit_cast(h8, fb[ins][part]), acc[m], 0, 0, 0);
                // lane (ks, o = lane & 15): acc[m][rr] = row 4 ks + rr <-> (t3 = t0 + og, k2 = 8 m + 4 h + rr) of output 16 nb + o; the lane
                // pair (o even: re z, o odd: im z) builds the complex z in both lanes
                v2f Zt[4][2];
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    v2f z[4];
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const float a = acc[m][rr], p = row_partner(a);
                        z[m] = odd ? (v2f){p, a} : (v2f){a, p};
                    }
                    // 4 points over m -> ta = e + 2 tai: even lane ta = 0, 2: (z0 + z2) +- (z1 + z3); odd lane ta = 1, 3: (z0 - z2) +- j (z1 - z3)
                    const v2f P = odd ? z[0] - z[2] : z[0] + z[2], Q = odd ? z[1] - z[3] : z[1] + z[3];
                    const v2f Qr = odd ? (v2f){-Q.y, Q.x} : Q;
                    Zt[rr][0] = pk_cmul(P + Qr, tw[rr][0]);
                    Zt[rr][1] = pk_cmul(P - Qr, tw[rr][1]);
                }
#pragma unroll
                for (int tai = 0; tai < 2; ++tai) {
                    // S[tb] = sum_rr Zt[rr] W8^(rr tb): tb = 2 c from Zt, tb = 2 c + 1 from Zt W8^rr
                    constexpr float r2 = 0.70710678118654752f;
                    v2f ev[4], od[4];
                    dft4(Zt[0][tai], Zt[1][tai], Zt[2][tai], Zt[3][tai], ev);
                    const v2f a1 = Zt[1][tai], a2 = Zt[2][tai], a3 = Zt[3][tai];
                    dft4(Zt[0][tai], (v2f){r2 * (a1.x - a1.y), r2 * (a1.x + a1.y)}, (v2f){-a2.y, a2.x}, (v2f){-r2 * (a3.x + a3.y), r2 * (a3.x - a3.y)}, od);
                    // tb = 0 .. 7: ev0 od0 ev1 od1 ev2 od2 ev3 od3.  Y[tb] = S_(h = 0)[tb] + (-1)^tb S_(h = 1)[tb]: the row h = 0 finishes
                    // tb = 0 .. 3, the row h = 1 tb = 4 .. 7 -- v_permlane16_swap: odd rows of the first <-> even rows of the second
                    const v2f lo[4] = {ev[0], od[0], ev[1], od[1]}, hi[4] = {ev[2], od[2], ev[3], od[3]};
#pragma unroll
                    for (int tbi = 0; tbi < 4; ++tbi) {
                        // (the components go through scalars of their own: __builtin_bit_cast of a vector ELEMENT reads element 0)
                        const float lx = lo[tbi].x, ly = lo[tbi].y, hx = hi[tbi].x, hy = hi[tbi].y;
                        const auto rx = __builtin_amdgcn_permlane16_swap(__float_as_uint(lx), __float_as_uint(hx), false, false);
                        const auto ry = __builtin_amdgcn_permlane16_swap(__float_as_uint(ly), __float_as_uint(hy), false, false);
                        const v2f s0 = (v2f){__uint_as_float(rx[0]), __uint_as_float(ry[0])};
                        const v2f s1 = (v2f){__uint_as_float(rx[1]), __uint_as_float(ry[1])};
                        const v2f y = (tbi & 1) ? s0 - s1 : s0 + s1;
                        m2[c][4 * tai + tbi] = fmaf(y.x, y.x, y.y * y.y);
                    }
                }
            }
        };
        const int t3o = t0 + og;  // the lag t3 of this lane's outputs
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
            float m2[2][8];
            block(nb, m2);
            const int t1 = (16 * nb + (lane & 15)) >> 1;
            const bool mine = t1 < K1 && t3o < K3;
            float bmax = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) bmax = fmaxf(bmax, m2[0][i] + m2[1][i]);
            if (!mine) bmax = 0.f;
            if (!__builtin_amdgcn_ballot_w64(!sieve_below(bmax, wsum2, lim))) continue;  // (wave-uniform)
            fmask |= 1u << nb;
            if (mine) {
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    top.offer(A.w0 * __builtin_amdgcn_sqrtf(m2[0][i]) + A.w1 * __builtin_amdgcn_sqrtf(m2[1][i]), (int)lag_of(t1, t2_of(i), t3o));
            }
        }
        if (A.stats && lane == 0) atomicAdd(A.stats + 1, (unsigned long long)__builtin_popcount(fmask));
        // The top-2 tail in its two halves, with the relisting loop here instead of sieve_top2_tail's callback: as a callback the loop is
        // optimised on its own before it is inlined, the compiler then keeps the item-invariant 64-bit parts of the eight lags of a lane
        // across the whole kernel, and at this kernel's register limit that is 256 VGPRs + 23 spilled instead of 254 and none
        // (profiles/r08_sieve_tail_resources.txt).
        const SieveTop2Plan plan = sieve_top2_begin(A.sieve, bd, lane, cell, top);
        if (plan.exhaustive) {
            for (int nb = 0; nb < NB; ++nb) {
                if (!((fmask >> nb) & 1)) continue;
                float m2[2][8];
                block(nb, m2);
                const int t1 = (16 * nb + (lane & 15)) >> 1;
                const bool mine = t1 < K1 && t3o < K3;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float a = -1.f;
                    if (mine) a = A.w0 * __builtin_amdgcn_sqrtf(m2[0][i]) + A.w1 * __builtin_amdgcn_sqrtf(m2[1][i]);
                    sieve_append(A.sieve, lane, a >= plan.thr, a, (int)lag_of(t1, t2_of(i), t3o), cell);
                }
            }
        }
        sieve_top2_end(A.sieve, bd, lane, cell, top, plan);
    }
}

// ---- forward transforms: the spectra of the signal (one per call) and of the codes (cached), in the CRT layout ---------------------
// X[k1, k2, k3] = sum x[n] W_N^(-n k) with n = (n1 N/53 + n2 N/32 + n3 N/625) mod N: rows over n3 (625 = 25 x 25 on conjugates), then
// 53 points over n1 and 32 over n2 as plain fp32 sums -- the conventions of pfa::forward.
// (both kernels are templates on K2: bds_acq_pfa6.h runs them for its 53 x 6 x 625)
template <int K2, class Loader>
__global__ __launch_bounds__(32) void k_pfa32_fwd_rows(Loader ld, float2 *T /* [batch][53 K2][625] */) {
    constexpr long NP = (long)K1 * K2 * K3;
    __shared__ float2 region[kRowRegion];
    const int row = blockIdx.x, batch = blockIdx.y, j = threadIdx.x;
    const bool live = j < 25;
    const int jj = live ? j : 24;
    const long base = ((long)(row / K2) * (NP / K1) + (long)(row % K2) * (NP / K2)) % NP;
    v2f x[25];
#pragma unroll
    for (int q = 0; q < 25; ++q) {
        const float2 v = ld(batch, (base + (long)(jj + 25 * q) * (NP / K3)) % NP);
        x[q] = (v2f){v.x, -v.y};  // forward transform = conj(inverse transform of the conjugate)
    }
    pfa::pk_radix25(x);
    if (live) {
#pragma unroll
        for (int sl = 0; sl < 25; ++sl) {
            const int p = pfa::slot25_index(sl);
            region[25 * j + p] = to_f2(p ? pk_cmul(x[sl], pfa::unit((jj * p) % K3, K3)) : x[sl]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 25; ++i) x[i] = to_v2f(region[25 * i + jj]);
    pfa::pk_radix25(x);
    if (live) {
        float2 *o = T + ((size_t)batch * K1 * K2 + row) * K3;
#pragma unroll
        for (int sl = 0; sl < 25; ++sl) o[j + 25 * pfa::slot25_index(sl)] = make_float2(x[sl].x, -x[sl].y);
    }
}

// U[batch][k1][n2][k3] = sum_n1 T[batch][n1][n2][k3] W53^(-n1 k1)
template <int K2>
__global__ __launch_bounds__(256) void k_pfa32_fwd_53(const float2 *T, float2 *U) {
    constexpr long NP = (long)K1 * K2 * K3;
    __shared__ float2 w[K1];
    if (threadIdx.x < K1) {
        float sn, cs;
        sincospif(-2.0f * (float)threadIdx.x / (float)K1, &sn, &cs);
        w[threadIdx.x] = make_float2(cs, sn);
    }
    __syncthreads();
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;  // (n2, k3)
    const int batch = blockIdx.y;
    if (e >= (long)K2 * K3) return;
    const float2 *t = T + (size_t)batch * NP + e;
    float2 *u = U + (size_t)batch * NP + e;
    float2 x[K1];
#pragma unroll
    for (int n1 = 0; n1 < K1; ++n1) x[n1] = t[(size_t)n1 * K2 * K3];
    for (int k1 = 0; k1 < K1; ++k1) {
        float ar = 0.f, ai = 0.f;
        int idx = 0;
#pragma unroll
        for (int n1 = 0; n1 < K1; ++n1) {
            const float2 ww = w[idx];
            ar = fmaf(x[n1].x, ww.x, fmaf(-x[n1].y, ww.y, ar));
            ai = fmaf(x[n1].x, ww.y, fmaf(x[n1].y, ww.x, ai));
            idx += k1;
            idx -= idx >= K1 ? K1 : 0;
        }
        u[(size_t)k1 * K2 * K3] = make_float2(ar, ai);
    }
}

// 32 points over n2, then the stored form: value * scale (conjugated for the code spectra) as fp16 complex;
// doubled = 1: signal spectrum, rows [k1][k2][2 x 625]; 0: code spectra [batch][k1][k2][625] from dst
__global__ __launch_bounds__(256) void k_pfa32_fwd_32(const float2 *U, uint32_t *dst, long dst_batch_stride, int conj_flag, float scale, int doubled) {
    __shared__ float2 w[K2];
    if (threadIdx.x < K2) {
        float sn, cs;
        sincospif(-2.0f * (float)threadIdx.x / (float)K2, &sn, &cs);
        w[threadIdx.x] = make_float2(cs, sn);
    }
    __syncthreads();
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;  // (k1, k3)
    const int batch = blockIdx.y;
    if (e >= (long)K1 * K3) return;
    const int k1 = (int)(e / K3), k3 = (int)(e % K3);
    const float2 *u = U + (size_t)batch * NP + (size_t)k1 * K2 * K3 + k3;
    float2 x[K2];
#pragma unroll
    for (int n2 = 0; n2 < K2; ++n2) x[n2] = u[(size_t)n2 * K3];
    uint32_t *d = dst + (size_t)batch * dst_batch_stride;
    for (int k2 = 0; k2 < K2; ++k2) {
        float ar = 0.f, ai = 0.f;
#pragma unroll
        for (int n2 = 0; n2 < K2; ++n2) {
            const float2 ww = w[(n2 * k2) & (K2 - 1)];
            ar = fmaf(x[n2].x, ww.x, fmaf(-x[n2].y, ww.y, ar));
            ai = fmaf(x[n2].x, ww.y, fmaf(x[n2].y, ww.x, ai));
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

// nb transforms: tmp holds 2 x nb x NP float2
template <class Loader>
inline void forward(hipStream_t st, Loader ld, int nb, float2 *tmp, uint32_t *dst, long dst_batch_stride, int conj_flag, float scale, int doubled) {
    float2 *T = tmp, *U = tmp + (size_t)nb * NP;
    hipLaunchKernelGGL((k_pfa32_fwd_rows<K2, Loader>), dim3(K1 * K2, nb), dim3(32), 0, st, ld, T);
    hipLaunchKernelGGL(k_pfa32_fwd_53<K2>, dim3((K2 * K3 + 255) / 256, nb), dim3(256), 0, st, (const float2 *)T, U);
    hipLaunchKernelGGL(k_pfa32_fwd_32, dim3((K1 * K3 + 255) / 256, nb), dim3(256), 0, st, (const float2 *)U, dst, dst_batch_stride, conj_flag, scale, doubled);
}

struct Plan {  // (bds_acq_pfa.h: the launches of a search pair)
    using RowsArgs = pfa::RowsArgs;
    using ColsArgs = pfa::ColsArgs;
    static constexpr long NP = pfa32::NP;
    static constexpr int K3 = pfa32::K3, kRows = K1 * K2, kRowsWgs = pfa32::kRowsWgs, kTiles = pfa32::kTiles;
    static constexpr size_t kCellElems = pfa32::kCellElems, kSpecElems = pfa32::kSpecElems, kCoefBytes = pfa32::kCoefBytes;
    static constexpr void (*make_coef_frags)(uint16_t *) = pfa::make_coef_frags;
    static constexpr bool kChunkList = false, kMasked = false;
    template <class Loader>
    static void forward(hipStream_t st, Loader ld, int nb, float2 *tmp, uint32_t *dst, long dst_batch_stride, int conj_flag, float scale, int doubled) {
        pfa32::forward(st, ld, nb, tmp, dst, dst_batch_stride, conj_flag, scale, doubled);
    }
    template <class Lds>
    static void launch_rows(hipStream_t st, const RowsArgs &A, int chunks, Lds &&lds) {
        pfa::launch_rows_of(k_pfa32_rows, kRowsWgs, kRowsThreads, kRowsLds, st, A, chunks, lds);
    }
    template <class Lds>
    static void launch_cols(hipStream_t st, const ColsArgs &A, int qchunk, long grid, Lds &&lds) {
        pfa::launch_cols_of(k_pfa32_cols, kTiles, kColsThreads, kColsLds, st, A, qchunk, grid, lds);
    }
};

}  // namespace pfa32
}  // namespace bds
