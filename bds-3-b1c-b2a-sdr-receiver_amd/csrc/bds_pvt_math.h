// Measurement stage of postNavigation: the index search and transmit time of Common/calculatePseudoranges.m:72-98 and the
// satellite position and clock of include/satpos.m:47-153 (with include/check_t.m), for ONE (measurement epoch, channel).
// Plain C++ that compiles for the device (bds_pvt.hip, k_pvt_meas) and for the host (tools/pvt_solve_check.cpp builds its
// geometries with it).  Built with -ffp-contract=off: every operation rounds once, in the reference's order of evaluation.
#pragma once
#include <cmath>
#include <cstdint>

#include "bds_mi355x.h"
#include "bds_strict_math.h"

namespace bds {

// the constants of satpos.m:32-39
constexpr double PVT_BDS_PI = 3.1415926535898;
constexpr double PVT_OMEGA_E = 7.2921150e-5;
constexpr double PVT_MU = 3.986004418e14;
constexpr double PVT_F = -4.44280730904398e-10;
constexpr double PVT_A_REF_MEO = 27906100.0;
constexpr double PVT_A_REF_IGSO_GEO = 42162200.0;

// What one launch needs besides the series and the ephemerides.
struct PvtMeasArgs {
    double fs, code_length, code_freq_basis;  // settings.samplingFreq, .codeLength, .codeFreqBasis
    double sample_start, meas_step;           // currMeasSample(m) = sample_start + meas_step * (m - 1)  (postNavigation.m:172)
    int32_t n_ch, n, n_meas;
    int32_t b1c;  // 1: T_GDB1Cp is subtracted (B1C satpos.m:61,151); 0: B2a, whose ephemeris has no such field: the term is 0
};

// check_t.m:19-27
BDS_HD double pvt_check_t(double t) {
    const double half_week = 302400.0;
    if (t > half_week) return t - 2 * half_week;
    if (t < -half_week) return t + 2 * half_week;
    return t;
}

// sin / cos by the one routine both sides share; an argument it does not cover (not finite, or 2^27 and beyond) gives NaN
BDS_HD void pvt_sincos(double x, double &s, double &c) {
    if (fabs(x) < 134217728.0) {
        sincos_strict(x, s, c);
    } else {
        s = c = NAN;
    }
}

// calculatePseudoranges.m:76-82: the first entry of absoluteSample[0..n) strictly greater than `sample` (1-based; n when there is
// none, as the reference's loop variable ends), minus 1.  absoluteSample must increase strictly (bds_pvt_plan checks it).
BDS_HD int pvt_index(const double *abs_sample, int n, double sample) {
    int lo = 0, hi = n;  // upper bound: abs_sample[k] <= sample for k < lo, > sample for k >= hi
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (abs_sample[mid] > sample)
            hi = mid;
        else
            lo = mid + 1;
    }
    return (lo + 1 > n ? n : lo + 1) - 1;
}

// calculatePseudoranges.m:85-97 at the 1-based `index` (>= 1)
BDS_HD double pvt_transmit_time(const PvtMeasArgs &a, const double *abs_sample, const double *code_freq, const double *rem_code_phase,
                                int index, double sample, double sub_frame_start, double tow) {
    const double step = code_freq[index - 1] / a.fs;
    const double code_phase = rem_code_phase[index - 1] + step * (sample - abs_sample[index - 1]);
    return ((code_phase / a.code_length + (double)index) - sub_frame_start) * a.code_length / a.code_freq_basis + tow;
}

// satpos.m:54-151 for one satellite.  e.SatType is 1..3 (a ready channel: bds_pvt_plan).
BDS_HD void pvt_satpos(const bds_eph &e, int b1c, double transmit_time, double pos[3], double &clk) {
    const double two_pi = 2 * PVT_BDS_PI;
    const double tgd = b1c ? e.T_GDB1Cp : 0.0;
    const double dt = pvt_check_t(transmit_time - e.t_oc);                 // :54
    const double clk0 = (e.a_2 * dt + e.a_1) * dt + e.a_0 - tgd;          // :59-61
    const double time = transmit_time - clk0;                             // :63
    const double tk = pvt_check_t(time - e.t_oe);                         // :67
    const double A_ref = e.SatType == 3 ? PVT_A_REF_MEO : PVT_A_REF_IGSO_GEO;  // :69-73
    const double A0 = A_ref + e.deltaA;                                   // :76
    const double A = A0 + e.ADot * tk;                                    // :77
    const double n0 = sqrt(PVT_MU / (A0 * A0 * A0));                      // :80  (A0^3 = A0 * A0 * A0)
    const double delta_n = e.delta_n_0 + 0.5 * e.delta_n_0Dot * tk;       // :81
    const double n = n0 + delta_n;                                        // :84
    double M = e.M_0 + n * tk;                                            // :87
    M = fmod(M + two_pi, two_pi);                                         // :90
    double E = M, sE, cE;
    for (int ii = 0; ii < 10; ++ii) {                                     // :96-105
        const double E_old = E;
        pvt_sincos(E, sE, cE);
        E = M + e.e * sE;
        const double dE = fmod(E - E_old, two_pi);
        if (fabs(dE) < 1.e-12) break;
    }
    E = fmod(E + two_pi, two_pi);                                         // :108
    pvt_sincos(E, sE, cE);
    const double dtr = PVT_F * e.e * sqrt(A0) * sE;                       // :111
    const double nu = atan2(sqrt(1 - e.e * e.e) * sE, cE - e.e);          // :114
    double Phi = nu + e.omega;                                            // :117
    Phi = fmod(Phi, two_pi);                                              // :120 (keeps the sign of Phi)
    double s2, c2;
    pvt_sincos(2 * Phi, s2, c2);
    const double u = Phi + e.C_uc * c2 + e.C_us * s2;                     // :123-125
    const double r = A * (1 - e.e * cE) + e.C_rc * c2 + e.C_rs * s2;      // :127-129
    const double i = e.i_0 + e.i_0Dot * tk + e.C_ic * c2 + e.C_is * s2;   // :131-133
    double Omega = e.omega_0 + (e.omegaDot - PVT_OMEGA_E) * tk - PVT_OMEGA_E * e.t_oe;  // :136-137
    Omega = fmod(Omega + two_pi, two_pi);                                 // :139
    double su, cu, sO, cO, si, ci;
    pvt_sincos(u, su, cu);
    pvt_sincos(Omega, sO, cO);
    pvt_sincos(i, si, ci);
    const double xp = r * cu, yp = r * su;                                // :142-143
    pos[0] = xp * cO - yp * ci * sO;                                      // :144
    pos[1] = xp * sO + yp * ci * cO;                                      // :145
    pos[2] = yp * si;                                                     // :146
    clk = (e.a_2 * dt + e.a_1) * dt + e.a_0 - tgd + dtr;                  // :150-151
}

}  // namespace bds
