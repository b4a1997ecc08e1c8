// bds_synth_trajectory: the segments of an orbit-driven synthetic IF record (include/bds_mi355x.h, "driven by an orbit"), host only.
// The physical model is the one postNavigation inverts -- the library's own satpos (bds_pvt_math.h), the rotation of e_r_corr.m by
// the travel time, no atmosphere -- so the generator and the solver share one orbit model.  Per satellite and node sample n the
// departure time rel (relative to tow, on the satellite's clock) solves
//     rel = a - delay(rel),   a = t0 + n / fs,   delay(rel) = |R3(OmegaE_dot travel) pos - rx| / c - clk
// by fixed-point iteration (it contracts by the range rate over c, ~3e-6 per step), and
//     code phase    = rel codeFreqBasis                       [chips since tow]
//     carrier phase = IF n / fs - carrFreqBasis (delay - t0)  [cycles]   (n / fs - rel = delay - t0 at the solution)
// A segment is the cubic through its nodes u = 0, rint(L / 3), rint(2 L / 3), L (L = 2^seg_log2).  The end node of a segment is the
// start node of the next, computed once, so neighbours meet at the joint.  Differences against the segment's first node are formed
// from the small quantities (u / fs and delay - delay0), in long double, so the seconds of the record do not cost digits; the cubic
// is found in s = u / L (Newton's divided differences) and its coefficients divided by L^k, which is exact: L is a power of two.
#include <cmath>
#include <vector>

#include "bds_internal.h"
#include "bds_pvt_math.h"

namespace {

constexpr double kC = 299792458.0;             // settings.c
constexpr double kOmegaEDot = 7.292115147e-5;  // e_r_corr.m:21
constexpr int kCodeLen = 10230;

// arrival minus satellite-clock time of departure, for a departure at tow + rel
double delay_of(const bds_eph &e, int b1c, const double rx[3], double tow, double rel) {
    double pos[3], clk;
    bds::pvt_satpos(e, b1c, tow + rel, pos, clk);
    const double d0 = pos[0] - rx[0], d1 = pos[1] - rx[1], d2 = pos[2] - rx[2];
    const double travel = std::sqrt(d0 * d0 + d1 * d1 + d2 * d2) / kC;
    const double w = kOmegaEDot * travel, cw = std::cos(w), sw = std::sin(w);
    const double r0 = cw * pos[0] + sw * pos[1] - rx[0], r1 = -sw * pos[0] + cw * pos[1] - rx[1];
    return std::sqrt(r0 * r0 + r1 * r1 + d2 * d2) / kC - clk;
}

// delay at the sample that arrives at tow + a
double solve_delay(const bds_eph &e, int b1c, const double rx[3], double tow, double a) {
    double d = 0.08;
    for (int it = 0; it < 6; ++it) {
        const double next = delay_of(e, b1c, rx, tow, a - d);
        const bool done = std::fabs(next - d) < 1e-16;
        d = next;
        if (done || !std::isfinite(d)) break;
    }
    return d;
}

bool eph_ready(const bds_eph &e, int b1c) {  // postNavigation's rule (bds_pvt_plan)
    if (b1c) return e.flag == 1;
    bool clock = false;
    for (int k = 0; k < 5; ++k) clock = clock || e.idValid[2 + k] == 30 + k;
    return e.idValid[0] == 10 && e.idValid[1] == 11 && clock;
}

// the cubic through (0, 0), (s1, z1), (s2, z2), (1, z3) as b1 s + b2 s^2 + b3 s^3
void cubic(long double s1, long double s2, long double z1, long double z2, long double z3, long double b[4]) {
    const long double d1 = z1 / s1, d12 = (z2 - z1) / (s2 - s1), d23 = (z3 - z2) / (1 - s2);
    const long double dd1 = (d12 - d1) / s2, dd2 = (d23 - d12) / (1 - s1);
    const long double ddd = dd2 - dd1;
    b[0] = 0;
    b[1] = d1 - dd1 * s1 + ddd * s1 * s2;
    b[2] = dd1 - ddd * (s1 + s2);
    b[3] = ddd;
}

}  // namespace

extern "C" int bds_synth_trajectory(const bds_settings *s, int n_sat, const bds_eph *eph, const double rx[3], double tow, double t0,
                                    int64_t first, int64_t n_seg, int seg_log2, bds_synth_seg *out) {
    using bds::fail;
    const char *who = "bds_synth_trajectory";
    if (!s || !eph || !rx || !out) return fail(nullptr, BDS_ERR_ARG, "%s: settings / eph / rx / out is NULL", who);
    if (seg_log2 < 10 || seg_log2 > 26) return fail(nullptr, BDS_ERR_ARG, "%s: seg_log2 = %d (10 .. 26)", who, seg_log2);
    if (n_sat < 1 || n_sat > BDS_MAX_PRN || n_seg < 1 || n_seg > (1LL << 26) || first < -(1LL << 53) || first > (1LL << 53))
        return fail(nullptr, BDS_ERR_ARG, "%s: n_sat = %d (1 .. %d), n_seg = %lld (1 .. 2^26), first = %lld out of range", who, n_sat, BDS_MAX_PRN,
                    (long long)n_seg, (long long)first);
    if (s->signal != BDS_SIGNAL_B1C && s->signal != BDS_SIGNAL_B2A) return fail(nullptr, BDS_ERR_ARG, "%s: settings.signal invalid", who);
    if (s->codeLength != kCodeLen) return fail(nullptr, BDS_ERR_ARG, "%s: settings.codeLength = %d, the primary codes have %d chips", who, s->codeLength, kCodeLen);
    if (!(s->codeFreqBasis > 0) || !std::isfinite(s->codeFreqBasis))
        return fail(nullptr, BDS_ERR_ARG, "%s: settings.codeFreqBasis = %g: the code rate must be positive", who, s->codeFreqBasis);
    if (!(s->samplingFreq > 0) || !std::isfinite(s->samplingFreq) || !std::isfinite(s->IF) || !std::isfinite(s->carrFreqBasis))
        return fail(nullptr, BDS_ERR_ARG, "%s: settings.samplingFreq / IF / carrFreqBasis invalid", who);
    const int b1c = s->signal == BDS_SIGNAL_B1C;
    for (int k = 0; k < n_sat; ++k) {
        if (eph[k].size != sizeof(bds_eph)) return fail(nullptr, BDS_ERR_ARG, "%s: eph[%d].size = %u, sizeof(bds_eph) = %d", who, k, eph[k].size, (int)sizeof(bds_eph));
        if (!eph_ready(eph[k], b1c)) return fail(nullptr, BDS_ERR_ARG, "%s: eph[%d] is not ready (no complete ephemeris has entered)", who, k);
        if (eph[k].SatType < 1 || eph[k].SatType > 3) return fail(nullptr, BDS_ERR_ARG, "%s: eph[%d]: unknown SatType %d", who, k, eph[k].SatType);
    }
    const long double fs = s->samplingFreq, fc = s->codeFreqBasis, fcarr = s->carrFreqBasis, f_if = s->IF, ncode = kCodeLen;
    const int64_t L = (int64_t)1 << seg_log2;
    const int64_t u1 = (int64_t)std::llrint((double)L / 3.0), u2 = (int64_t)std::llrint(2.0 * (double)L / 3.0);
    const long double s1 = (long double)u1 / (long double)L, s2 = (long double)u2 / (long double)L;
    std::vector<double> joint((size_t)n_seg + 1);
    for (int k = 0; k < n_sat; ++k) {
        auto at = [&](int64_t n) { return solve_delay(eph[k], b1c, rx, tow, (double)((long double)t0 + (long double)n / fs)); };
        for (int64_t j = 0; j <= n_seg; ++j) joint[(size_t)j] = at(first + j * L);
        for (int64_t j = 0; j < n_seg; ++j) {
            const int64_t n0 = first + j * L;
            const double d0 = joint[(size_t)j], d3 = joint[(size_t)j + 1], d1 = at(n0 + u1), d2 = at(n0 + u2);
            bds_synth_seg &g = out[(size_t)k * (size_t)n_seg + (size_t)j];
            // node 0: rel = a - delay; its chips and cycles with the whole periods and cycles taken out
            const long double a0 = (long double)t0 + (long double)n0 / fs;
            const long double chips0 = (a0 - (long double)d0) * fc;
            long double p0 = floorl(chips0 / ncode), c0 = chips0 - p0 * ncode;
            if ((double)c0 >= (double)ncode) p0 += 1, c0 -= ncode;  // (rounding to double may reach the period's end)
            const long double cyc0 = f_if * ((long double)n0 / fs) - fcarr * ((long double)d0 - (long double)t0);
            long double x0 = cyc0 - floorl(cyc0);
            if ((double)x0 >= 1.0) x0 = 0;
            // differences against node 0: rel - rel0 = u / fs - (d - d0);  cycles - cycles0 = IF u / fs - fcarr (d - d0)
            const int64_t un[3] = {u1, u2, L};
            const double dn[3] = {d1, d2, d3};
            long double zc[3], zx[3];
            for (int i = 0; i < 3; ++i) {
                const long double dt = (long double)un[i] / fs, dd = (long double)dn[i] - (long double)d0;
                zc[i] = (dt - dd) * fc;
                zx[i] = f_if * dt - fcarr * dd;
            }
            long double bc[4], bx[4];
            cubic(s1, s2, zc[0], zc[1], zc[2], bc);
            cubic(s1, s2, zx[0], zx[1], zx[2], bx);
            bc[0] = c0, bx[0] = x0;
            bool ok = std::isfinite((double)p0) && std::fabs((double)p0) < 9e15;
            g.period0 = ok ? (int64_t)p0 : 0;
            for (int c = 0; c < 4; ++c) {
                g.code[c] = (double)ldexpl(bc[c], -seg_log2 * c);
                g.carr[c] = (double)ldexpl(bx[c], -seg_log2 * c);
                ok = ok && std::isfinite(g.code[c]) && std::isfinite(g.carr[c]);
            }
            if (!ok) return fail(nullptr, BDS_ERR_ARG, "%s: satellite %d, segment %lld: the result is not finite (check rx, tow, t0 and the ephemeris)", who, k + 1, (long long)j);
            if (!(g.code[1] > 0)) return fail(nullptr, BDS_ERR_ARG, "%s: satellite %d, segment %lld: code rate %g chips per sample is not positive", who, k + 1, (long long)j, g.code[1]);
        }
    }
    return BDS_OK;
}
