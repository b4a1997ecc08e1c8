// Stand-alone run of the position fix's host code (csrc/bds_pvt.cpp through bds_pvt_plan / bds_pvt_solve, and the shared
// arithmetic of csrc/bds_pvt_math.h) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU: random geometries with
// 4 .. 63 channels, all-masked epochs, rank-deficient geometries, NaN and inf in every input.  An ordinary executable; nothing is
// loaded into Python.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -Iinclude \
//       -Ibds-3-b1c-b2a-sdr-receiver_amd/csrc tools/pvt_solve_check.cpp bds-3-b1c-b2a-sdr-receiver_amd/csrc/bds_pvt.cpp \
//       -o /tmp/pvt_solve_check && /tmp/pvt_solve_check
//
// Exit status 0 and "pvt_solve_check: ok" = no report and every invariant held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "bds_mi355x.h"
#include "bds_pvt_math.h"

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static const double C = 299792458.0, OMEGAE_DOT = 7.292115147e-5;

// Output arrays of exactly the sizes the entry is told: a write past them is a report.
struct Out {
    std::vector<double> ch[7], dop, ep[9];
    bds_pvt_out o;
    Out(int n_ch, int cap) {
        for (auto &v : ch) v.assign((size_t)n_ch * cap, -7.0);
        dop.assign((size_t)5 * cap, -7.0);
        for (auto &v : ep) v.assign(cap, -7.0);
        o.size = sizeof o, o.cap = cap;
        o.PRN = ch[0].data(), o.el = ch[1].data(), o.az = ch[2].data(), o.transmitTime = ch[3].data(), o.satClkCorr = ch[4].data();
        o.rawP = ch[5].data(), o.correctedP = ch[6].data(), o.DOP = dop.data();
        o.X = ep[0].data(), o.Y = ep[1].data(), o.Z = ep[2].data(), o.dt = ep[3].data(), o.localTime = ep[4].data();
        o.currMeasSample = ep[5].data(), o.latitude = ep[6].data(), o.longitude = ep[7].data(), o.height = ep[8].data();
    }
};

static bds_settings settings(int signal) {
    bds_settings s;
    std::memset(&s, 0, sizeof s);
    s.signal = signal, s.samplingFreq = 53e6, s.codeFreqBasis = 1.023e6, s.codeLength = 10230;
    return s;
}
static bds_pvt_params params(int trop) {
    bds_pvt_params p;
    p.size = sizeof p, p.useTropCorr = trop, p.navSolPeriod = 200, p.elevationMask = 5, p.c = C, p.startOffset = 68.802;
    return p;
}

// A satellite at distance r from the Earth's centre, `el` radians above the horizon of rx at azimuth `az`.
static void place(const double rx[3], double az, double el, double r, double out[3]) {
    const double lat = std::atan2(rx[2], std::hypot(rx[0], rx[1])), lon = std::atan2(rx[1], rx[0]);
    const double e[3] = {-std::sin(lon), std::cos(lon), 0}, n[3] = {-std::sin(lat) * std::cos(lon), -std::sin(lat) * std::sin(lon), std::cos(lat)};
    const double u[3] = {std::cos(lat) * std::cos(lon), std::cos(lat) * std::sin(lon), std::sin(lat)};
    double d[3], b = 0, rr = 0;
    for (int k = 0; k < 3; ++k) {
        d[k] = std::cos(el) * (std::sin(az) * e[k] + std::cos(az) * n[k]) + std::sin(el) * u[k];
        b += rx[k] * d[k], rr += rx[k] * rx[k];
    }
    const double rho = -b + std::sqrt(b * b - rr + r * r);
    for (int k = 0; k < 3; ++k) out[k] = rx[k] + rho * d[k];
}
// The range the solver models: the satellite rotated by the travel time (e_r_corr.m), no troposphere.
static double model_range(const double x[3], const double rx[3]) {
    const double t = std::sqrt((x[0] - rx[0]) * (x[0] - rx[0]) + (x[1] - rx[1]) * (x[1] - rx[1]) + (x[2] - rx[2]) * (x[2] - rx[2])) / C;
    const double w = OMEGAE_DOT * t, r0 = std::cos(w) * x[0] + std::sin(w) * x[1] - rx[0], r1 = -std::sin(w) * x[0] + std::cos(w) * x[1] - rx[1];
    return std::sqrt(r0 * r0 + r1 * r1 + (x[2] - rx[2]) * (x[2] - rx[2]));
}

int main() {
    std::mt19937_64 rng(2025);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const bds_settings s = settings(BDS_SIGNAL_B1C);
    const double step = 10600000.0;

    // ---- random geometries, 4 .. 63 channels, a few epochs; some satellites below the mask; every second trial with tropo() --------
    for (int trial = 0; trial < 120; ++trial) {
        const int n_ch = trial < 60 ? 4 + trial : 4 + (int)(rng() % 60), n_meas = 1 + (int)(rng() % 4);
        const int trop = trial & 1;
        const bds_pvt_params p = params(trop);
        const double lat = (U(rng) - 0.5) * 2.8, lon = (U(rng) - 0.5) * 6.2, R = 6371000.0 + U(rng) * 3000;
        const double rx[3] = {R * std::cos(lat) * std::cos(lon), R * std::cos(lat) * std::sin(lon), R * std::sin(lat)};
        std::vector<int32_t> prn(n_ch), ready(n_ch, BDS_PVT_READY);
        std::vector<double> tt((size_t)n_meas * n_ch), sp((size_t)n_meas * n_ch * 3), clk((size_t)n_meas * n_ch, 0.0);
        int n_low = 0;
        std::vector<double> az(n_ch), el(n_ch);
        for (int c = 0; c < n_ch; ++c) {
            prn[c] = 1 + c;
            az[c] = 6.283 * (c + U(rng)) / n_ch;
            const bool low = c >= 5 && U(rng) < 0.2;  // the first five stay up: the fix keeps a fair geometry
            el[c] = low ? 0.02 + 0.04 * U(rng) : 0.2 + 1.2 * U(rng) * ((c % 3) ? 1.0 : 0.4);
            n_low += low;
            if (c % 7 == 6) ready[c] = BDS_PVT_IDLE;
        }
        for (int m = 0; m < n_meas; ++m)
            for (int c = 0; c < n_ch; ++c) {
                double *x = &sp[((size_t)m * n_ch + c) * 3];
                place(rx, az[c] + 1e-5 * m, el[c], c % 2 ? 27906100.0 : 42162200.0, x);
                tt[(size_t)m * n_ch + c] = 1000.0 + 0.2 * m - model_range(x, rx) / C;
            }
        Out out(n_ch, n_meas);
        EXPECT(bds_pvt_solve(&s, &p, n_ch, n_meas, prn.data(), ready.data(), 1e6, step, tt.data(), sp.data(), clk.data(), &out.o) == n_meas);
        for (int m = 0; m < n_meas; ++m) {
            int n_active = 0;
            for (int c = 0; c < n_ch; ++c) {
                const size_t o = (size_t)c * n_meas + m;
                const bool active = out.o.PRN[o] != 0;
                n_active += active;
                EXPECT(out.o.PRN[o] == 0 || out.o.PRN[o] == prn[c]);
                EXPECT(active || (std::isnan(out.o.el[o]) && out.o.rawP[o] == -inf && out.o.correctedP[o] == 0));
                EXPECT(!(ready[c] & BDS_PVT_IDLE) || !active);
                if (m > 0 && active) EXPECT(out.o.el[(size_t)c * n_meas + m - 1] >= 5);  // the mask works on the last fix's elevation
            }
            EXPECT(n_active >= 4);
            if (!trop) {  // the ranges were made without a troposphere: the fix is the truth
                const double d = std::sqrt((out.o.X[m] - rx[0]) * (out.o.X[m] - rx[0]) + (out.o.Y[m] - rx[1]) * (out.o.Y[m] - rx[1]) +
                                           (out.o.Z[m] - rx[2]) * (out.o.Z[m] - rx[2]));
                EXPECT(d < 1e-3 * out.o.DOP[m]);
            }
            EXPECT(out.o.DOP[m] > 0 && std::isfinite(out.o.DOP[m]) && out.o.DOP[m] >= out.o.DOP[(size_t)1 * n_meas + m]);
            EXPECT(out.o.currMeasSample[m] == 1e6 + step * m && (m > 0 || out.o.dt[m] == 0));
        }
    }

    // ---- all satellites below the mask after the first fix: NaN rows, zero DOP, nothing active -------------------------------------
    {
        const int n_ch = 6, n_meas = 4;
        const bds_pvt_params p = params(1);
        const double rx[3] = {-2148744.0, 4426641.0, 4044656.0};
        std::vector<int32_t> prn = {3, 5, 7, 9, 11, 13}, ready(n_ch, BDS_PVT_READY);
        std::vector<double> tt((size_t)n_meas * n_ch), sp((size_t)n_meas * n_ch * 3), clk((size_t)n_meas * n_ch, 1e-4);
        for (int m = 0; m < n_meas; ++m)
            for (int c = 0; c < n_ch; ++c) {
                place(rx, 1.0 * c, 0.01 + 0.01 * c, 27906100.0, &sp[((size_t)m * n_ch + c) * 3]);
                tt[(size_t)m * n_ch + c] = 5000.0 + 0.2 * m - model_range(&sp[((size_t)m * n_ch + c) * 3], rx) / C;
            }
        Out out(n_ch, n_meas);
        EXPECT(bds_pvt_solve(&s, &p, n_ch, n_meas, prn.data(), ready.data(), 1e6, step, tt.data(), sp.data(), clk.data(), &out.o) == n_meas);
        EXPECT(std::isfinite(out.o.X[0]));
        for (int m = 1; m < n_meas; ++m) {
            EXPECT(std::isnan(out.o.X[m]) && std::isnan(out.o.dt[m]) && std::isnan(out.o.height[m]) && out.o.DOP[m] == 0);
            for (int c = 0; c < n_ch; ++c) EXPECT(out.o.PRN[(size_t)c * n_meas + m] == 0 && out.o.rawP[(size_t)c * n_meas + m] == -inf);
        }
    }

    // ---- rank-deficient: the same satellite in every row; two equal rows of four; satellites on one line of sight -----------------
    for (int kind = 0; kind < 3; ++kind) {
        const int n_ch = kind == 1 ? 4 : 7, n_meas = 3;
        const bds_pvt_params p = params(kind == 2);
        const double rx[3] = {-2148744.0, 4426641.0, 4044656.0};
        std::vector<int32_t> prn(n_ch, 21), ready(n_ch, BDS_PVT_READY);
        std::vector<double> tt((size_t)n_meas * n_ch), sp((size_t)n_meas * n_ch * 3), clk((size_t)n_meas * n_ch, 0.0);
        for (int m = 0; m < n_meas; ++m)
            for (int c = 0; c < n_ch; ++c) {
                double *x = &sp[((size_t)m * n_ch + c) * 3];
                if (kind == 0) place(rx, 1.0, 0.7, 27906100.0, x);
                if (kind == 1) place(rx, 1.0 + (c == 3 ? 0 : c), 0.7, 27906100.0, x);
                if (kind == 2) place(rx, 1.0, 0.7, 2.0e7 + 3.0e6 * c, x);
                tt[(size_t)m * n_ch + c] = 5000.0 + 0.2 * m - model_range(x, rx) / C;
            }
        Out out(n_ch, n_meas);
        EXPECT(bds_pvt_solve(&s, &p, n_ch, n_meas, prn.data(), ready.data(), 1e6, step, tt.data(), sp.data(), clk.data(), &out.o) == n_meas);
        // leastSquarePos.m:90-95: pos = 0, dop = inf; cart2geo(0, 0, 0) = NaN, 0, NaN; el = 0 empties the list
        if (kind < 2) {
            EXPECT(out.o.X[0] == 0 && out.o.Y[0] == 0 && out.o.Z[0] == 0 && out.o.dt[0] == 0 && std::isinf(out.o.DOP[0]));
            EXPECT(std::isnan(out.o.latitude[0]) && out.o.longitude[0] == 0 && std::isnan(out.o.height[0]) && out.o.el[0] == 0);
            EXPECT(std::isnan(out.o.X[1]) && out.o.DOP[1] == 0 && out.o.PRN[1] == 0);
        } else {
            EXPECT(std::isinf(out.o.DOP[0]) || std::isfinite(out.o.X[0]));  // nearly collinear: either exit, no report
        }
    }

    // ---- NaN and inf in every input array, in turn and everywhere -----------------------------------------------------------------
    {
        const int n_ch = 8, n_meas = 3;
        const bds_pvt_params p = params(1);
        const double rx[3] = {-2148744.0, 4426641.0, 4044656.0};
        std::vector<int32_t> prn(n_ch, 30), ready(n_ch, BDS_PVT_READY);
        std::vector<double> tt0((size_t)n_meas * n_ch), sp0((size_t)n_meas * n_ch * 3), clk0((size_t)n_meas * n_ch, 1e-5);
        for (int m = 0; m < n_meas; ++m)
            for (int c = 0; c < n_ch; ++c) {
                place(rx, 0.8 * c, 0.3 + 0.1 * c, 27906100.0, &sp0[((size_t)m * n_ch + c) * 3]);
                tt0[(size_t)m * n_ch + c] = 5000.0 + 0.2 * m - model_range(&sp0[((size_t)m * n_ch + c) * 3], rx) / C;
            }
        const double bad[] = {nan, inf, -inf, 1e308, -1e308, 0.0};
        for (int trial = 0; trial < 400; ++trial) {
            std::vector<double> tt = tt0, sp = sp0, clk = clk0;
            std::vector<double> *arr[] = {&tt, &sp, &clk};
            const int hits = trial < 300 ? 1 + (int)(rng() % 3) : 40;
            for (int h = 0; h < hits; ++h) {
                std::vector<double> &a = *arr[rng() % 3];
                a[rng() % a.size()] = bad[rng() % 6];
            }
            Out out(n_ch, n_meas);
            EXPECT(bds_pvt_solve(&s, &p, n_ch, n_meas, prn.data(), ready.data(), 1e6, step, tt.data(), sp.data(), clk.data(), &out.o) == n_meas);
            for (int m = 0; m < n_meas; ++m) EXPECT(out.o.DOP[m] != -7.0 && out.o.X[m] != -7.0 && out.o.rawP[m] != -7.0);
        }
        std::vector<double> all_nan(sp0.size(), nan);
        Out out(n_ch, n_meas);
        EXPECT(bds_pvt_solve(&s, &p, n_ch, n_meas, prn.data(), ready.data(), nan, inf, all_nan.data(), all_nan.data(), all_nan.data(), &out.o) ==
               n_meas);
        EXPECT(out.o.X[0] == 0 && std::isinf(out.o.DOP[0]));  // the rank exit
        // refusals
        bds_pvt_params q = p;
        q.size = 0;
        EXPECT(bds_pvt_solve(&s, &q, n_ch, n_meas, prn.data(), ready.data(), 1e6, step, tt0.data(), sp0.data(), clk0.data(), &out.o) == BDS_ERR_ARG);
        q = p, q.c = nan;
        EXPECT(bds_pvt_solve(&s, &q, n_ch, n_meas, prn.data(), ready.data(), 1e6, step, tt0.data(), sp0.data(), clk0.data(), &out.o) == BDS_ERR_ARG);
        out.o.cap = n_meas - 1;
        EXPECT(bds_pvt_solve(&s, &p, n_ch, n_meas, prn.data(), ready.data(), 1e6, step, tt0.data(), sp0.data(), clk0.data(), &out.o) == BDS_ERR_ARG);
        out.o.cap = n_meas, out.o.az = nullptr;
        EXPECT(bds_pvt_solve(&s, &p, n_ch, n_meas, prn.data(), ready.data(), 1e6, step, tt0.data(), sp0.data(), clk0.data(), &out.o) == BDS_ERR_ARG);
        EXPECT(bds_pvt_solve(&s, &p, n_ch, n_meas, prn.data(), ready.data(), 1e6, step, tt0.data(), sp0.data(), clk0.data(), nullptr) == BDS_ERR_ARG);
    }

    // ---- bds_pvt_plan: random series and flags, NaN / inf in absoluteSample, subFrameStart and TOW --------------------------------
    for (int signal : {BDS_SIGNAL_B1C, BDS_SIGNAL_B2A})
        for (int trial = 0; trial < 300; ++trial) {
            const bds_settings ss = settings(signal);
            const bds_pvt_params p = params(1);
            const int n_ch = 1 + (int)(rng() % 12), n = 1 + (int)(rng() % 50);
            std::vector<char> status(n_ch);
            std::vector<bds_eph> eph(n_ch);
            std::vector<double> a((size_t)n_ch * n), sfs(n_ch), tow(n_ch), v(3);
            std::vector<int32_t> ready(n_ch, -1);
            for (int c = 0; c < n_ch; ++c) {
                status[c] = rng() % 5 ? 'T' : '-';
                std::memset(&eph[c], 0, sizeof(bds_eph));
                eph[c].size = sizeof(bds_eph), eph[c].flag = rng() % 6 != 0, eph[c].SatType = (int32_t)(rng() % 4);
                eph[c].idValid[0] = rng() % 6 ? 10 : 0, eph[c].idValid[1] = 11, eph[c].idValid[2 + rng() % 5] = 30 + (int32_t)(rng() % 5);
                const double odd[] = {nan, inf, -inf, 0.0, -3.0, 2.5, (double)n + 1, 1e300};
                sfs[c] = rng() % 5 ? 1.0 + (double)(rng() % n) : odd[rng() % 8];
                tow[c] = rng() % 9 ? 7218.0 : odd[rng() % 3];
                double t = 1000.0 * U(rng);
                for (int k = 0; k < n; ++k) a[(size_t)c * n + k] = (t += 1.0 + std::floor(530000.0 * U(rng)));
                if (rng() % 10 == 0) a[(size_t)c * n + rng() % n] = odd[rng() % 4];
            }
            const int rc = bds_pvt_plan(&ss, &p, n_ch, n, status.data(), a.data(), eph.data(), sfs.data(), tow.data(), ready.data(), &v[0], &v[1], &v[2]);
            EXPECT(rc >= 0 || rc == BDS_ERR_ARG);
            int n_ready = 0;
            for (int c = 0; c < n_ch; ++c) {
                EXPECT(ready[c] == 1 || ready[c] == 2 || ready[c] == 4 || ready[c] == 8 || ready[c] == 16);
                EXPECT((status[c] == '-') == (ready[c] == BDS_PVT_IDLE));
                n_ready += ready[c] == BDS_PVT_READY;
            }
            EXPECT(rc <= 0 || (n_ready >= 4 && v[1] - v[0] >= rc * v[2]));
            EXPECT(v[2] == 10600000.0);
        }

    // ---- the shared arithmetic on the host: the index search on every kind of sample, satpos on odd ephemerides --------------------
    {
        std::vector<double> a(37);
        for (size_t k = 0; k < a.size(); ++k) a[k] = 100.0 + 10.0 * (double)k;
        for (double x : {-inf, 0.0, 99.0, 100.0, 101.0, 110.0, 455.0, 459.0, 460.0, 461.0, 1e9, inf, nan}) {
            const int idx = bds::pvt_index(a.data(), (int)a.size(), x);
            int scan = 1;  // calculatePseudoranges.m:76-82 as written
            for (scan = 1; scan <= (int)a.size(); ++scan)
                if (a[scan - 1] > x) break;
            if (scan > (int)a.size()) scan = (int)a.size();
            EXPECT(idx == scan - 1 && idx >= 0 && idx <= (int)a.size() - 1);
        }
        const double only[1] = {5.0};
        EXPECT(bds::pvt_index(only, 1, 7.0) == 0 && bds::pvt_index(only, 1, 1.0) == 0);
        bds_eph e;
        for (int trial = 0; trial < 2000; ++trial) {
#define X(name) e.name = rng() % 7 == 0 ? (rng() % 2 ? nan : (rng() % 2 ? inf : -inf)) : (U(rng) - 0.5) * std::pow(10.0, (double)(rng() % 12) - 4);
            BDS_EPH_FIELDS(X)
#undef X
            e.SatType = 1 + (int32_t)(rng() % 3);
            double pos[3], clk;
            bds::pvt_satpos(e, trial & 1, rng() % 9 ? 604800.0 * U(rng) : nan, pos, clk);
            EXPECT(pos[0] == pos[0] || std::isnan(pos[0]));  // (it came back)
        }
    }
    std::printf(failures ? "pvt_solve_check: %d FAILED\n" : "pvt_solve_check: ok\n", failures);
    return failures ? 1 : 0;
}
