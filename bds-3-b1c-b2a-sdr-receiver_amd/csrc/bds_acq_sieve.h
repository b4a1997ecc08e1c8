// The sieve protocol: how a wave-level column pass of the search reports (gfx950).  Every such pass -- k_cols_wave_f
// (bds_acq_wcols.h), k_cols_small_f (bds_acq_scols.h), k_pfa_cols (bds_acq_pfa.h), k_pfa32_cols (bds_acq_pfa32.h) -- ends in one of
// the two tails below, so the refinement (bds_acq_refine.h, bds_acq_decide.h) does not know which kernel filled the sieve.
//
// The sieve (SieveArgs) is, per run:
//   cellmax[cell]       the cell's maximum so far as a packed word (value bits << 32) | ~lag, raised by a 64-bit atomic max: the larger
//                       value wins and, of equal values, the SMALLER lag (wc_pack) -- the first lag on ties, as MATLAB's max()
//   lb[cell / lb_div]   a running lower bound of the PRN's sieve maximum (the largest value any wave of the PRN has published)
//   extra[], count      ONE candidate list {value, lag, cell} behind one counter; entries past extra_cap are counted, not stored
//                       (the host sees count > extra_cap and re-runs)
//
// What a wave must report.  With Mw the exact maximum of the wave's searched outputs and lbv, cur the values of lb and of the cell's
// maximum the wave loaded (sieve_bounds):
//   * every output with value >= thr = max(Mw, lbv) * keep goes on the list;
//   * if Mw >= cur (the wave beats or TIES the cell's maximum so far) it publishes {Mw, the first lag at which Mw occurs} to cellmax
//     and raises lb to Mw.
// Mw and lbv are values that occur on the PRN's surface, hence <= its final maximum M, so every lag with value >= keep * M is on
// the list: the completeness argument of DESIGN.md section 1.5.
//
// When it may skip.  By Cauchy-Schwarz (w_d |y_d| + w_p |y_p|)^2 <= (w_d^2 + w_p^2)(|y_d|^2 + |y_p|^2).  If that bound, over ALL of
// the wave's outputs (or all outputs of one block of them), stays below min(cur, lbv * keep)^2, none of them beats the cell's
// maximum or reaches the list's threshold: no square root is taken and no lag is formed (sieve_limit / sieve_below).  The test is
// written so that unset or non-finite bounds never skip.
//
// Why stale bounds are safe.  lb and cellmax only grow.  A stale lbv or cur is a LOWER value: the skip test passes less often and
// thr is lower, i.e. a redundant visit or a redundant entry, never a lost candidate; the atomic max keeps the published maximum right
// whatever order the waves arrive in.  Hence relaxed loads, issued wherever the caller can hide their latency.
//
// The pieces (all __forceinline__, all taking kernel values by value or as callables: the callers sit at their register limits and
// the code below must melt into their cold regions): sieve_bounds, sieve_limit / sieve_below, sieve_reserve / sieve_put /
// sieve_append, sieve_publish, and the two tails sieve_staged_tail (values staged [k][lane] in LDS) and SieveTop2 / sieve_top2_tail
// (per-lane top two in registers, exhaustive relisting when that is not enough; k_pfa32_cols calls its halves sieve_top2_begin /
// sieve_top2_end around a relisting loop of its own, see there).
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "bds_debug.h"
#include "bds_lds.h"

namespace bds {

struct Extra {
    float v;
    int lag;   // 0-based
    int cell;  // cell index within the run (PRN index * D + bin, or the second-peak pass's PRN index)
};

struct SieveArgs {
    unsigned long long *cellmax;  // [run-wide cell]: (value bits << 32) | ~lag, by atomic max
    float *lb;                    // [(run-wide cell) / lb_div]: running lower bound of that PRN's sieve maximum
    int lb_div;
    Extra *extra;                 // candidate list
    int *extra_count;
    int extra_cap;
    int cell0;                    // run-wide index of cell 0 of this launch
    float keep;                   // 1 - tolerance of the sieve
};

__device__ __forceinline__ unsigned long long wc_pack(float v, int lag) {
    return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(~(unsigned)lag);
}

// maximum over the 64 lanes, wave-uniform result (DPP inside the 16-lane rows, then one read per row)
__device__ __forceinline__ float wave_max_f32(float v) {
    auto dpp = [](float x, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, 0xF, 0xF, true));
    };
    v = fmaxf(v, dpp(v, std::integral_constant<int, 0xB1>{}));   // quad_perm [1,0,3,2]
    v = fmaxf(v, dpp(v, std::integral_constant<int, 0x4E>{}));   // quad_perm [2,3,0,1]
    v = fmaxf(v, dpp(v, std::integral_constant<int, 0x141>{}));  // row_half_mirror
    v = fmaxf(v, dpp(v, std::integral_constant<int, 0x140>{}));  // row_mirror
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

// ---- bounds load ---------------------------------------------------------------------------------------------------------------
struct SieveBounds {
    float *lbp;    // the PRN's slot of lb
    float lbv;     // its value when loaded
    unsigned cur;  // value bits of the cell's maximum when loaded
};
// Two relaxed device-scope loads (L2 / fabric latency): the caller places this where that latency is covered.
// (the value half of the packed word alone: with the 64-bit load the compiler reuses the dead low register at once and waits for it)
__device__ __forceinline__ SieveBounds sieve_bounds(const SieveArgs &S, int cell) {
    SieveBounds b;
    b.lbp = S.lb + cell / S.lb_div;
    b.lbv = __hip_atomic_load(b.lbp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    b.cur = __hip_atomic_load(reinterpret_cast<const unsigned *>(S.cellmax + cell) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return b;
}

// ---- skip test -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sieve_limit(const SieveArgs &S, SieveBounds b) { return fminf(__uint_as_float(b.cur), b.lbv * S.keep); }
// true: outputs whose |y_d|^2 + |y_p|^2 are all <= sq2 (any margin the caller has to prove included) have nothing to report.
// (1e-5: rounding of the bound and of the squares, 40 x the fp32 unit; false while the bounds are unset or not finite)
__device__ __forceinline__ bool sieve_below(float sq2, float wsum2, float lim) { return sq2 * wsum2 * 1.00001f < lim * lim; }

// ---- list append ---------------------------------------------------------------------------------------------------------------
// n entries of the list for this wave: one device-scope atomic by lane 0, the wave-uniform index of the first
__device__ __forceinline__ int sieve_reserve(const SieveArgs &S, int lane, int n) {
    int base = 0;
    if (lane == 0) base = atomicAdd(S.extra_count, n);
    return __builtin_amdgcn_readfirstlane(base);
}
__device__ __forceinline__ void sieve_store(const SieveArgs &S, int base, unsigned long long mask, bool mine, float v, int lag, int cell) {
    if (mine) {
        const int idx = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        BDS_DASSERT(idx >= 0 && lag >= 0 && cell >= S.cell0);
        if ((unsigned)idx < (unsigned)S.extra_cap) {  // (unsigned: a counter run over 2^31 must not index backwards)
            Extra ex;
            ex.v = v, ex.lag = lag, ex.cell = cell;
            S.extra[idx] = ex;
        }
    }
}
// the lanes with `mine` store their entry from `base` on, in lane order; returns how many did (wave-uniform): for several puts
// behind ONE sieve_reserve of their counted total
__device__ __forceinline__ int sieve_put(const SieveArgs &S, int base, bool mine, float v, int lag, int cell) {
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(mine);
    sieve_store(S, base, mask, mine, v, lag, cell);
    return __builtin_popcountll(mask);
}
// one reservation per ballot: the lanes with `mine` append their entry
__device__ __forceinline__ void sieve_append(const SieveArgs &S, int lane, bool mine, float v, int lag, int cell) {
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(mine);
    if (mask) sieve_store(S, sieve_reserve(S, lane, __builtin_popcountll(mask)), mask, mine, v, lag, cell);  // (wave-uniform)
}

// ---- publish -------------------------------------------------------------------------------------------------------------------
// Mw: the wave's maximum (uniform); lag: this lane's first lag at which it holds Mw, 0x7fffffff if it does not
__device__ __forceinline__ void sieve_publish(const SieveArgs &S, SieveBounds b, int lane, int cell, float Mw, int lag) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lag = min(lag, __shfl_xor(lag, o));
    if (lane == 0) {
        atomicMax(S.cellmax + cell, wc_pack(Mw, lag));
        if (Mw > b.lbv) atomicMax(reinterpret_cast<unsigned *>(b.lbp), __float_as_uint(Mw));
    }
}

// ---- staged tail ---------------------------------------------------------------------------------------------------------------
// A lane's K exact values (outputs that are not searched hold -1; searched values are >= 0) go through the wave's own LDS region
// sm[k * 64], k < K (sm already offset by the lane), and a compact loop picks the maximum's first lag and every lag within the sieve
// tolerance of the bound.  mx: the lane's maximum of them; Mw = wave_max_f32(mx); lag_at(k): the lag of this lane's value k;
// stage(): writes the values to sm where the caller has not done so yet -- called only when the loop runs.  The wave's LDS
// traffic is ordered by lds_wave_sync().  One reservation per wave on the list's counter.
template <int K, class Stage, class LagAt>
__device__ __forceinline__ void sieve_staged_tail(const SieveArgs &S, SieveBounds b, int lane, int cell, float Mw, float mx, const float *sm,
                                                  Stage stage, LagAt lag_at) {
    if (!(Mw >= 0.f)) return;  // (wave-uniform) nothing of the wave's outputs is searched
    const float thr = fmaxf(Mw, b.lbv) * S.keep;
    const bool newmax = __float_as_uint(Mw) >= b.cur;  // this wave holds (a tie of) the cell's maximum so far
    if (!(newmax || __builtin_amdgcn_ballot_w64(mx >= thr) != 0)) return;
    // rare (wave-uniform)
    stage();
    lds_wave_sync();
    int best = 0x7fffffff, total = 0;
#pragma nounroll
    for (int k = 0; k < K; ++k) {
        const float a = sm[k * 64];
        total += __builtin_popcountll(__builtin_amdgcn_ballot_w64(a >= thr));
        if (newmax && a == Mw) best = min(best, lag_at(k));
    }
    if (total > 0) {
        int base = sieve_reserve(S, lane, total);
#pragma nounroll
        for (int k = 0; k < K; ++k) {
            const float a = sm[k * 64];
            base += sieve_put(S, base, a >= thr, a, lag_at(k), cell);
        }
    }
    if (newmax) sieve_publish(S, b, lane, cell, Mw, best);
}

// ---- top-2 tail ----------------------------------------------------------------------------------------------------------------
// A lane keeps the two largest of its values with their lags (first lag on ties, like max()).  Two qualifying values in one lane are
// the rare case of the rare case: then the flagged output blocks are listed exhaustively.
struct SieveTop2 {
    float top1 = -1.f, top2 = -1.f;
    int lag1 = 0x7fffffff, lag2 = 0x7fffffff;
    __device__ __forceinline__ void offer(float a, int lag) {
        if (a > top1 || (a == top1 && lag < lag1)) {
            top2 = top1, lag2 = lag1, top1 = a, lag1 = lag;
        } else if (a > top2 || (a == top2 && lag < lag2)) {
            top2 = a, lag2 = lag;
        }
    }
};
// What the wave does with what its lanes were offered.  sieve_top2_begin decides, and lists the common case (at most one qualifying
// value per lane: one reservation per wave on the list's counter) itself; when it returns `exhaustive` the caller recomputes the
// flagged output blocks (their values were never all in registers) and gives EVERY value a of EVERY lane, -1 for an output that is not
// the lane's to report, to sieve_append(S, lane, a >= thr, a, lag, cell) -- the same sequence of calls in every lane --; then
// sieve_top2_end publishes.
struct SieveTop2Plan {
    float Mw, thr;    // the wave's maximum, the list's threshold
    bool publish;     // this wave holds (a tie of) the cell's maximum so far
    bool exhaustive;  // two qualifying values in one lane
};
__device__ __forceinline__ SieveTop2Plan sieve_top2_begin(const SieveArgs &S, SieveBounds b, int lane, int cell, SieveTop2 t) {
    SieveTop2Plan p{wave_max_f32(t.top1), 0.f, false, false};
    if (p.Mw >= 0.f) {  // (wave-uniform, as everything below) something of the wave's outputs is searched
        p.thr = fmaxf(p.Mw, b.lbv) * S.keep;
        const bool newmax = __float_as_uint(p.Mw) >= b.cur;
        const unsigned long long hit1 = __builtin_amdgcn_ballot_w64(t.top1 >= p.thr), hit2 = __builtin_amdgcn_ballot_w64(t.top2 >= p.thr);
        if (newmax || hit1) {
            p.publish = newmax;
            if (!hit2)
                sieve_append(S, lane, t.top1 >= p.thr, t.top1, t.lag1, cell);
            else
                p.exhaustive = true;
        }
    }
    return p;
}
__device__ __forceinline__ void sieve_top2_end(const SieveArgs &S, SieveBounds b, int lane, int cell, SieveTop2 t, SieveTop2Plan p) {
    if (p.publish) sieve_publish(S, b, lane, cell, p.Mw, t.top1 == p.Mw ? t.lag1 : 0x7fffffff);
}
// The whole tail.  t: what the lane was offered from the output blocks in fmask (bit nb of NB).  relist(nb, emit) recomputes block nb
// and calls emit(value, lag) once per output slot, the same slots in every lane, value -1 for an output that is not the lane's to
// report.  exhaustive: optional counter of the waves that took that path (probes).
template <int NB, class Relist>
__device__ __forceinline__ void sieve_top2_tail(const SieveArgs &S, SieveBounds b, int lane, int cell, SieveTop2 t, unsigned fmask,
                                                unsigned long long *exhaustive, Relist relist) {
    const SieveTop2Plan p = sieve_top2_begin(S, b, lane, cell, t);
    if (p.exhaustive) {
        if (exhaustive && lane == 0) atomicAdd(exhaustive, 1ull);
        for (int nb = 0; nb < NB; ++nb) {
            if (!((fmask >> nb) & 1)) continue;
            relist(nb, [&](float a, int lag) { sieve_append(S, lane, a >= p.thr, a, lag, cell); });
        }
    }
    sieve_top2_end(S, b, lane, cell, t, p);
}

}  // namespace bds
