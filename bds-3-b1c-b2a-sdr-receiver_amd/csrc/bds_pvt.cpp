// Position fix, host half (bds_pvt_plan, bds_pvt_solve): the channel lists and measurement grid of postNavigation.m:69-122 and
// the sequential chain of postNavigation.m:146-298 with Common/calculatePseudoranges.m:100-110, Common/leastSquarePos.m,
// Common/e_r_corr.m, include/topocent.m, Common/togeod.m, Common/tropo.m and Common/cart2geo.m.  Plain C++, no GPU; the
// measurement stage the chain reads is bds_pvt.hip's.  Built with -ffp-contract=off: the reference's order of evaluation.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>
#include <vector>

#include "bds_mi355x.h"

namespace {

constexpr double kInf = std::numeric_limits<double>::infinity();
constexpr double kNaN = std::numeric_limits<double>::quiet_NaN();
constexpr double kPi = 3.14159265358979323846;  // MATLAB's pi

// e_r_corr.m:21-32
void e_r_corr(double traveltime, const double x[3], double out[3]) {
    const double Omegae_dot = 7.292115147e-5;
    const double omegatau = Omegae_dot * traveltime;
    const double c = std::cos(omegatau), s = std::sin(omegatau);
    out[0] = c * x[0] + s * x[1] + 0 * x[2];
    out[1] = -s * x[0] + c * x[1] + 0 * x[2];
    out[2] = 0 * x[0] + 0 * x[1] + 1 * x[2];
}

// togeod.m:32-111: (dphi, dlambda) in degrees, h
void togeod(double a, double finv, double X, double Y, double Z, double &dphi, double &dlambda, double &h) {
    h = 0;
    const double tolsq = 1.e-10;
    const int maxit = 10;
    const double rtd = 180 / kPi;
    const double esq = finv < 1.e-20 ? 0 : (2 - 1 / finv) / finv;
    const double oneesq = 1 - esq;
    const double P = std::sqrt(X * X + Y * Y);
    dlambda = P > 1.e-20 ? std::atan2(Y, X) * rtd : 0;
    if (dlambda < 0) dlambda = dlambda + 360;
    const double r = std::sqrt(P * P + Z * Z);
    double sinphi = r > 1.e-20 ? Z / r : 0;
    dphi = std::asin(sinphi);
    if (r < 1.e-20) {  // (:76-79: dphi stays in radians, here 0)
        h = 0;
        return;
    }
    h = r - a * (1 - sinphi * sinphi / finv);
    for (int i = 1; i <= maxit; ++i) {
        sinphi = std::sin(dphi);
        const double cosphi = std::cos(dphi);
        const double N_phi = a / std::sqrt(1 - esq * sinphi * sinphi);
        const double dP = P - (N_phi + h) * cosphi;
        const double dZ = Z - (N_phi * oneesq + h) * sinphi;
        h = h + (sinphi * dZ + cosphi * dP);
        dphi = dphi + (cosphi * dZ - sinphi * dP) / (N_phi + h);
        if (dP * dP + dZ * dZ < tolsq) break;
    }
    dphi = dphi * rtd;
}

// topocent.m:24-54: azimuth and elevation [deg] of dx seen from X
void topocent(const double X[3], const double dx[3], double &Az, double &El) {
    const double dtr = kPi / 180;
    double phi, lambda, h;
    togeod(6378137.0, 298.257222101, X[0], X[1], X[2], phi, lambda, h);
    const double cl = std::cos(lambda * dtr), sl = std::sin(lambda * dtr);
    const double cb = std::cos(phi * dtr), sb = std::sin(phi * dtr);
    // local_vector = F' * dx, F = [-sl -sb*cl cb*cl; cl -sb*sl cb*sl; 0 cb sb]
    const double E = -sl * dx[0] + cl * dx[1] + 0 * dx[2];
    const double N = -sb * cl * dx[0] + -sb * sl * dx[1] + cb * dx[2];
    const double U = cb * cl * dx[0] + cb * sl * dx[1] + sb * dx[2];
    const double hor_dis = std::sqrt(E * E + N * N);
    if (hor_dis < 1.e-20) {
        Az = 0;
        El = 90;
    } else {
        Az = std::atan2(E, N) / dtr;
        El = std::atan2(U, hor_dis) / dtr;
    }
    if (Az < 0) Az = Az + 360;
}

// tropo.m:34-97
double tropo(double sinel, double hsta, double p, double tkel, double hum, double hp, double htkel, double hhum) {
    const double a_e = 6378.137, b0 = 7.839257e-5, tlapse = -6.5;
    const double tkhum = tkel + tlapse * (hhum - htkel);
    const double atkel = 7.5 * (tkhum - 273.15) / (237.3 + tkhum - 273.15);
    const double e0 = 0.0611 * hum * std::pow(10.0, atkel);
    const double tksea = tkel - tlapse * htkel;
    const double em = -978.77 / (2.8704e6 * tlapse * 1.0e-5);
    const double tkelh = tksea + tlapse * hhum;
    const double e0sea = e0 * std::pow(tksea / tkelh, 4 * em);
    const double tkelp = tksea + tlapse * hp;
    const double psea = p * std::pow(tksea / tkelp, em);
    if (sinel < 0) sinel = 0;
    double trop = 0;
    double refsea = 77.624e-6 / tksea;
    double htop = 1.1385e-5 / refsea;
    refsea = refsea * psea;
    double ref = refsea * std::pow((htop - hsta) / htop, 4.0);
    for (int pass = 0; pass < 2; ++pass) {  // (:58-97: the loop body runs twice, dry then wet)
        double rtop = (a_e + htop) * (a_e + htop) - (a_e + hsta) * (a_e + hsta) * (1 - sinel * sinel);
        if (rtop < 0) rtop = 0;
        rtop = std::sqrt(rtop) - (a_e + hsta) * sinel;
        const double a = -sinel / (htop - hsta);
        const double b = -b0 * (1 - sinel * sinel) / (htop - hsta);
        double rn[8];
        for (int i = 1; i <= 8; ++i) rn[i - 1] = std::pow(rtop, (double)(i + 1));
        const double a2 = a * a, b2 = b * b;
        double alpha[8] = {2 * a, 2 * a2 + 4 * b / 3, a * (a2 + 3 * b), a2 * a2 / 5 + 2.4 * a2 * b + 1.2 * b2,
                           2 * a * b * (a2 + 3 * b) / 3, b2 * (6 * a2 + 4 * b) * 1.428571e-1, 0, 0};
        if (b2 > 1.0e-35) {
            alpha[6] = a * (b2 * b) / 2;
            alpha[7] = b2 * b2 / 9;
        }
        double dr = 0;
        for (int i = 0; i < 8; ++i) dr += alpha[i] * rn[i];
        dr = rtop + dr;
        trop = trop + dr * ref * 1000;
        if (pass == 1) break;
        refsea = (371900.0e-6 / tksea - 12.92e-6) / tksea;
        htop = 1.1385e-5 * (1255 / tksea + 0.05) / refsea;
        ref = refsea * e0sea * std::pow((htop - hsta) / htop, 4.0);
    }
    return trop;
}

// cart2geo.m:22-51 with i = 5
void cart2geo5(double X, double Y, double Z, double &phi, double &lambda, double &h) {
    const double a = 6378137, f = 1 / 298.257223563;
    lambda = std::atan2(Y, X);
    const double ex2 = (2 - f) * f / ((1 - f) * (1 - f));
    const double c = a * std::sqrt(1 + ex2);
    const double P = std::sqrt(X * X + Y * Y);
    phi = std::atan(Z / ((P * (1 - (2 - f))) * f));  // (:28, parenthesised as written there)
    h = 0.1;
    double oldh = 0;
    int iterations = 0;
    while (std::fabs(h - oldh) > 1.e-12) {
        oldh = h;
        const double N = c / std::sqrt(1 + ex2 * (std::cos(phi) * std::cos(phi)));
        phi = std::atan(Z / (P * (1 - (2 - f) * f * N / (N + h))));
        h = P / std::cos(phi) - N;
        if (++iterations > 100) break;
    }
    phi = phi * 180 / kPi;
    lambda = lambda * 180 / kPi;
}

// One-sided Jacobi SVD of the n x 4 matrix A (row-major): A = U diag(sigma) V', W = U diag(sigma).  A bounded number of sweeps,
// so an A with NaN / inf ends as well (its sigma are then NaN and the rank test fails).
struct Svd4 {
    std::vector<double> W;
    double V[4][4];
    double sigma[4];
};
void svd4(const std::vector<double> &A, int n, Svd4 &s) {
    s.W = A;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) s.V[i][j] = i == j;
    double *W = s.W.data();
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int i = 0; i < n; ++i) {
                    alpha += W[4 * i + p] * W[4 * i + p];
                    beta += W[4 * i + q] * W[4 * i + q];
                    gamma += W[4 * i + p] * W[4 * i + q];
                }
                if (!(std::fabs(gamma) > 1e-15 * std::sqrt(alpha * beta))) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1 + zeta * zeta));
                const double c = 1 / std::sqrt(1 + t * t), sn = c * t;
                for (int i = 0; i < n; ++i) {
                    const double wp = W[4 * i + p], wq = W[4 * i + q];
                    W[4 * i + p] = c * wp - sn * wq;
                    W[4 * i + q] = sn * wp + c * wq;
                }
                for (int i = 0; i < 4; ++i) {
                    const double vp = s.V[i][p], vq = s.V[i][q];
                    s.V[i][p] = c * vp - sn * vq;
                    s.V[i][q] = sn * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    for (int j = 0; j < 4; ++j) {
        double ss = 0;
        for (int i = 0; i < n; ++i) ss += W[4 * i + j] * W[4 * i + j];
        s.sigma[j] = std::sqrt(ss);
    }
}
// rank(A): singular values above max(size(A)) * eps(max(sigma))
int rank4(const Svd4 &s, int n) {
    double smax = 0;
    for (double v : s.sigma) {
        if (!(v == v)) return 0;
        if (v > smax) smax = v;
    }
    if (!std::isfinite(smax)) return 0;
    const double tol = (n > 4 ? n : 4) * (std::nextafter(smax, kInf) - smax);
    int r = 0;
    for (double v : s.sigma) r += v > tol;
    return r;
}

// leastSquarePos.m:33-121.  satpos: [ns][3], obs[ns] -> pos[4], el[ns], az[ns], dop[5].  Returns 0 on the rank exit (:90-95).
int least_square_pos(const double *satpos, const double *obs, int ns, const bds_pvt_params &set, double pos[4], double *el, double *az,
                     double dop[5]) {
    const double dtr = kPi / 180;
    pos[0] = pos[1] = pos[2] = pos[3] = 0;
    std::vector<double> A((size_t)ns * 4, 0.0), omc(ns, 0.0);
    for (int i = 0; i < ns; ++i) az[i] = el[i] = 0;
    Svd4 s;
    for (int iter = 1; iter <= 10; ++iter) {
        for (int i = 0; i < ns; ++i) {
            const double *X = satpos + 3 * i;
            double Rot_X[3], trop;
            if (iter == 1) {
                Rot_X[0] = X[0], Rot_X[1] = X[1], Rot_X[2] = X[2];
                trop = 2;
            } else {
                const double d0 = X[0] - pos[0], d1 = X[1] - pos[1], d2 = X[2] - pos[2];
                const double rho2 = d0 * d0 + d1 * d1 + d2 * d2;
                const double traveltime = std::sqrt(rho2) / set.c;
                e_r_corr(traveltime, X, Rot_X);
                const double dx[3] = {Rot_X[0] - pos[0], Rot_X[1] - pos[1], Rot_X[2] - pos[2]};
                topocent(pos, dx, az[i], el[i]);
                trop = set.useTropCorr == 1 ? tropo(std::sin(el[i] * dtr), 0.0, 1013.0, 293.0, 50.0, 0.0, 0.0, 0.0) : 0;
            }
            const double d[3] = {Rot_X[0] - pos[0], Rot_X[1] - pos[1], Rot_X[2] - pos[2]};
            const double nrm = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            omc[i] = obs[i] - nrm - pos[3] - trop;
            A[4 * i + 0] = -d[0] / nrm;
            A[4 * i + 1] = -d[1] / nrm;
            A[4 * i + 2] = -d[2] / nrm;
            A[4 * i + 3] = 1;
        }
        svd4(A, ns, s);
        if (rank4(s, ns) != 4) {
            pos[0] = pos[1] = pos[2] = pos[3] = 0;
            for (int k = 0; k < 5; ++k) dop[k] = kInf;
            return 0;
        }
        // x = A \ omc = V diag(1 / sigma^2) W' omc
        double x[4] = {0, 0, 0, 0};
        for (int j = 0; j < 4; ++j) {
            double dot = 0;
            for (int i = 0; i < ns; ++i) dot += s.W[4 * i + j] * omc[i];
            const double g = dot / (s.sigma[j] * s.sigma[j]);
            for (int k = 0; k < 4; ++k) x[k] += s.V[k][j] * g;
        }
        for (int k = 0; k < 4; ++k) pos[k] = pos[k] + x[k];
    }
    // Q = inv(A' * A) = V diag(1 / sigma^2) V', of the last A
    double Q[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 4; ++j) Q[k] += s.V[k][j] * s.V[k][j] / (s.sigma[j] * s.sigma[j]);
    dop[0] = std::sqrt(Q[0] + Q[1] + Q[2] + Q[3]);
    dop[1] = std::sqrt(Q[0] + Q[1] + Q[2]);
    dop[2] = std::sqrt(Q[0] + Q[1]);
    dop[3] = std::sqrt(Q[2]);
    dop[4] = std::sqrt(Q[3]);
    return 1;
}

bool settings_ok(const bds_settings *s) {
    return s && (s->signal == BDS_SIGNAL_B1C || s->signal == BDS_SIGNAL_B2A) && std::isfinite(s->samplingFreq) && s->samplingFreq > 0 &&
           std::isfinite(s->codeFreqBasis) && s->codeFreqBasis > 0 && s->codeLength > 0;
}
bool params_ok(const bds_pvt_params *p) {
    return p && p->size == sizeof(bds_pvt_params) && std::isfinite(p->c) && p->c != 0 && std::isfinite(p->navSolPeriod) &&
           std::isfinite(p->startOffset) && !std::isnan(p->elevationMask);
}

}  // namespace

extern "C" int bds_pvt_plan(const bds_settings *s, const bds_pvt_params *p, int n_ch, int n, const char *status,
                            const double *absoluteSample, const bds_eph *eph, const double *subFrameStart, const double *TOW,
                            int32_t *ready, double *sampleStart, double *sampleEnd, double *measSampleStep) {
    if (!settings_ok(s) || !params_ok(p) || n_ch < 1 || n < 1 || !status || !absoluteSample || !eph || !subFrameStart || !TOW || !ready ||
        !sampleStart || !sampleEnd || !measSampleStep)
        return BDS_ERR_ARG;
    for (int c = 0; c < n_ch; ++c)
        if (eph[c].size != sizeof(bds_eph)) return BDS_ERR_ARG;
    const double step = std::trunc(s->samplingFreq * p->navSolPeriod / 1000);  // :119
    *sampleStart = *sampleEnd = kNaN;
    *measSampleStep = step;
    int n_ready = 0;
    for (int c = 0; c < n_ch; ++c) {
        const bds_eph &e = eph[c];
        if (status[c] == '-') {  // :69
            ready[c] = BDS_PVT_IDLE;
            continue;
        }
        bool ok;
        if (s->signal == BDS_SIGNAL_B1C) {
            ok = e.flag == 1;  // :82
        } else {               // BDS-3_B2a/postNavigation.m:84-85
            bool clock = false;
            for (int k = 0; k < 5; ++k) clock = clock || e.idValid[2 + k] == 30 + k;
            ok = e.idValid[0] == 10 && e.idValid[1] == 11 && clock;
        }
        const double f = subFrameStart[c];
        if (!ok)
            ready[c] = BDS_PVT_NO_EPH;
        else if (e.SatType < 1 || e.SatType > 3)
            ready[c] = BDS_PVT_NO_SATTYPE;
        else if (!(f >= 1 && f <= n && f == std::trunc(f)) || !std::isfinite(TOW[c]))
            ready[c] = BDS_PVT_NO_FRAME;
        else
            ready[c] = BDS_PVT_READY, ++n_ready;
    }
    if (n_ready < 4) return 0;  // :92-98
    double start = 0, end = kInf;  // :103-104
    for (int c = 0; c < n_ch; ++c) {
        if (!(ready[c] & BDS_PVT_READY)) continue;
        const double *a = absoluteSample + (size_t)c * n;
        for (int k = 1; k < n; ++k)
            if (!(a[k] > a[k - 1])) return BDS_ERR_ARG;  // (a NaN fails too)
        if (!std::isfinite(a[0]) || !std::isfinite(a[n - 1])) return BDS_ERR_ARG;
        const double v = a[(int)subFrameStart[c] - 1];  // :107-108
        if (v > start) start = v;
        if (a[n - 1] < end) end = a[n - 1];  // :110
    }
    *sampleStart = start + 1;  // :115
    *sampleEnd = end - 1;      // :116
    if (!(step >= 1)) return BDS_ERR_ARG;
    const double n_meas = std::trunc((*sampleEnd - *sampleStart) / step);  // :122
    if (!(n_meas > 0)) return 0;
    if (n_meas > 2147483647.0 / 4) return BDS_ERR_ARG;
    return (int)n_meas;
}

extern "C" int bds_pvt_solve(const bds_settings *s, const bds_pvt_params *p, int n_ch, int n_meas, const int32_t *prn,
                             const int32_t *ready, double sampleStart, double measSampleStep, const double *transmitTime,
                             const double *satPos, const double *satClkCorr, bds_pvt_out *out) {
    if (!settings_ok(s) || !params_ok(p) || n_ch < 1 || n_meas < 0 || !prn || !ready || !transmitTime || !satPos || !satClkCorr || !out ||
        out->size != sizeof(bds_pvt_out) || out->cap < n_meas)
        return BDS_ERR_ARG;
    double *const per_ch[] = {out->PRN, out->el, out->az, out->transmitTime, out->satClkCorr, out->rawP, out->correctedP};
    double *const per_m[] = {out->DOP, out->X, out->Y, out->Z, out->dt, out->localTime, out->currMeasSample, out->latitude,
                             out->longitude, out->height};
    for (double *q : per_ch)
        if (!q) return BDS_ERR_ARG;
    for (double *q : per_m)
        if (!q) return BDS_ERR_ARG;
    const size_t cap = (size_t)out->cap;
    std::vector<double> satElev(n_ch, kInf), tt(n_ch), rawP(n_ch), sp((size_t)n_ch * 3), clk(n_ch), obs(n_ch), el(n_ch), az(n_ch);
    std::vector<int> active;
    active.reserve(n_ch);
    double localTime = kInf;  // :139
    for (int m = 0; m < n_meas; ++m) {
        // :151-152 (NaN >= mask is false: a channel once masked, or not active at the last fix, never returns)
        active.clear();
        for (int c = 0; c < n_ch; ++c)
            if ((ready[c] & BDS_PVT_READY) && satElev[c] >= p->elevationMask) active.push_back(c);
        for (int c = 0; c < n_ch; ++c) {
            const size_t o = (size_t)c * cap + m;
            out->PRN[o] = 0;
            out->el[o] = out->az[o] = out->transmitTime[o] = out->satClkCorr[o] = kNaN;  // :161-168
            out->correctedP[o] = 0;
            tt[c] = kInf;  // calculatePseudoranges.m:64
        }
        const double currMeasSample = sampleStart + measSampleStep * (double)m;  // :172
        const double *tt_m = transmitTime + (size_t)m * n_ch, *clk_m = satClkCorr + (size_t)m * n_ch;
        const double *sp_m = satPos + (size_t)m * n_ch * 3;
        for (int c : active) {
            out->PRN[(size_t)c * cap + m] = prn[c];  // :155-156
            tt[c] = tt_m[c];
        }
        if (localTime == kInf) {  // calculatePseudoranges.m:102-105; max() skips NaN
            double maxTime = kNaN;
            for (int c : active)
                if (!(tt[c] != tt[c]) && !(maxTime >= tt[c])) maxTime = tt[c];
            localTime = maxTime + p->startOffset / 1000;
        }
        for (int c = 0; c < n_ch; ++c) out->rawP[(size_t)c * cap + m] = rawP[c] = (localTime - tt[c]) * p->c;  // :110
        const int ns = (int)active.size();
        for (int i = 0; i < ns; ++i) {
            const int c = active[i];
            out->transmitTime[(size_t)c * cap + m] = tt[c];       // :182-183
            out->satClkCorr[(size_t)c * cap + m] = clk_m[c];      // :192
            clk[i] = clk_m[c];
            sp[3 * i] = sp_m[3 * c], sp[3 * i + 1] = sp_m[3 * c + 1], sp[3 * i + 2] = sp_m[3 * c + 2];
        }
        if (ns > 3) {  // :197
            for (int i = 0; i < ns; ++i) obs[i] = rawP[active[i]] + clk[i] * p->c;  // :201-202
            double pos[4], dop[5];
            least_square_pos(sp.data(), obs.data(), ns, *p, pos, el.data(), az.data(), dop);  // :205-208
            for (int i = 0; i < ns; ++i) {
                out->el[(size_t)active[i] * cap + m] = el[i];
                out->az[(size_t)active[i] * cap + m] = az[i];
            }
            for (int k = 0; k < 5; ++k) out->DOP[(size_t)k * cap + m] = dop[k];
            out->X[m] = pos[0], out->Y[m] = pos[1], out->Z[m] = pos[2];  // :212-214
            out->dt[m] = m == 0 ? 0 : pos[3];                            // :218-222
            localTime = localTime - pos[3] / p->c;                       // :225
            out->localTime[m] = localTime;
            out->currMeasSample[m] = currMeasSample;
            for (int c = 0; c < n_ch; ++c) satElev[c] = out->el[(size_t)c * cap + m];  // :232
            for (int i = 0; i < ns; ++i)                                               // :235-237
                out->correctedP[(size_t)active[i] * cap + m] = rawP[active[i]] + clk[i] * p->c - pos[3];
            cart2geo5(pos[0], pos[1], pos[2], out->latitude[m], out->longitude[m], out->height[m]);  // :242-248
        } else {  // :270-285; localTime and currMeasSample, which the reference does not assign here, are NaN
            out->X[m] = out->Y[m] = out->Z[m] = out->dt[m] = kNaN;
            for (int k = 0; k < 5; ++k) out->DOP[(size_t)k * cap + m] = 0;
            out->latitude[m] = out->longitude[m] = out->height[m] = kNaN;
            out->localTime[m] = out->currMeasSample[m] = kNaN;
        }
        localTime = localTime + measSampleStep / s->samplingFreq;  // :296
    }
    return n_meas;
}
