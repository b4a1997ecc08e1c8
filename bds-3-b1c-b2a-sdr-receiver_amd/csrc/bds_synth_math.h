// Counter-based arithmetic of the synthetic IF generator (bds_synth.hip): plain C++ that compiles for the device and for the
// host (tests/test_synth_cases.py builds this very header with g++ and holds it against the NumPy restatement of
// tests/synth_cases.py).  Built with -ffp-contract=off: every operation below rounds once, as written.
// Nothing here keeps state: sample n of a record depends on (seed, n) alone, a symbol on (seed, period, prn, component) alone,
// so a record can be made in any pieces, in any order, on any number of lanes.
#pragma once
#include <cmath>
#include <cstdint>

#include "bds_strict_math.h"

namespace bds {
namespace synth {

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of two
// 32 x 32 -> 64-bit products, the key bumped by the Weyl constants between rounds.
BDS_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// The two uniforms of sample n (the GLOBAL sample index of the record): counter (n low, n high, 0, 0), key = the seed's halves.
//   u1 = (((w0 2^32 + w1) >> 12) + 0.5) 2^-52  in (0, 1): 52 bits and a half -- exact in a double, never 0 (its log is finite)
//   u2 = ((w2 2^32 + w3) >> 11) 2^-53          in [0, 1)
BDS_HD void noise_uniforms(uint64_t seed, int64_t n, double &u1, double &u2) {
    uint32_t w[4];
    philox4x32_10((uint32_t)(uint64_t)n, (uint32_t)((uint64_t)n >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    u1 = ((double)((((uint64_t)w[0] << 32) | w[1]) >> 12) + 0.5) * 2.220446049250313e-16;  // 2^-52
    u2 = (double)((((uint64_t)w[2] << 32) | w[3]) >> 11) * 1.1102230246251565e-16;         // 2^-53
}

// Box-Muller on them: two independent N(0, 1) values per sample.  A real record uses g_i, an I/Q record both.
BDS_HD void noise_normals(uint64_t seed, int64_t n, double &g_i, double &g_q) {
    double u1, u2, sn, cs;
    noise_uniforms(seed, n, u1, u2);
    const double r = sqrt(-2.0 * log(u1));
    sincos_strict(6.283185307179586 * u2, sn, cs);
    g_i = r * cs;
    g_q = r * sn;
}

// Data (component 0) / secondary (component 1) symbol of primary-code period `period` (may be negative) of satellite `prn`:
// counter (period + 1 as a 64-bit two's complement: low, high; 1; 2 prn + component); +1 when bit 0 of the first word is set.
BDS_HD int symbol(uint64_t seed, int64_t period, int prn, int component) {
    const uint64_t p = (uint64_t)(period + 1);
    uint32_t w[4];
    philox4x32_10((uint32_t)p, (uint32_t)(p >> 32), 1u, (uint32_t)(prn * 2 + component), (uint32_t)seed, (uint32_t)(seed >> 32), w);
    return (w[0] & 1u) ? 1 : -1;
}

// ---- the trajectory path (bds_synth_traj; include/bds_mi355x.h, "driven by an orbit") -------------------------------------------
// Sample n of a trajectory that starts at sample `first` with segments of 2^seg_log2 samples: the segment index (a shift: no
// 64-bit division) and the offset inside the segment, an exact integer.
BDS_HD void traj_index(int64_t n, int64_t first, int seg_log2, int64_t &j, int64_t &u) {
    const int64_t m = n - first;
    j = m >> seg_log2;
    u = m - (j << seg_log2);
}

// ((a[3] u + a[2]) u + a[1]) u + a[0], six roundings
BDS_HD double traj_horner(const double a[4], double u) { return ((a[3] * u + a[2]) * u + a[1]) * u + a[0]; }

// Code phase in [0, ncode) chips and the code period of offset u in a segment.
BDS_HD void traj_code(int64_t period0, const double code[4], double u, double ncode, double &cph, int64_t &period) {
    const double c = traj_horner(code, u);
    const double k = floor(c / ncode);
    cph = c - k * ncode;
    period = period0 + (int64_t)k;
}

// Carrier angle [rad] of offset u in a segment: the whole cycles of the polynomial's value are dropped towards zero (fmod(x, 1)).
BDS_HD double traj_carrier(const double carr[4], double u, double phase) {
    const double x = traj_horner(carr, u);
    return 6.283185307179586 * (x - trunc(x)) + phase;
}

}  // namespace synth
}  // namespace bds
