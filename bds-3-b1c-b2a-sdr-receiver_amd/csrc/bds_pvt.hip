// Position fix, device half: the measurement stage of postNavigation (bds_pvt_measure) and the whole step
// (bds_post_navigation = bds_pvt_plan -> bds_pvt_measure -> bds_pvt_solve; the other two are bds_pvt.cpp, host only).
//
// k_pvt_meas: one lane per (measurement epoch m, channel c), one launch per call.  Grid x covers the epochs, grid y the channels, so
// the channel is uniform in a workgroup: its ephemeris, subFrameStart, TOW and the base of its three series are scalar loads.  Each
// lane searches the channel's absoluteSample by bisection (log2 n dependent loads; the series stay in L2 between the lanes of a
// channel), forms the transmit time and runs satpos in f64.  The arithmetic is bds_pvt_math.h, shared with the host.
#include <hip/hip_runtime.h>

#include <cmath>

#include "bds_internal.h"
#include "bds_pvt_math.h"

using namespace bds;

namespace {
inline hipStream_t st(bds_ctx *c) { return (hipStream_t)c->stream; }

__global__ __launch_bounds__(256) void k_pvt_meas(PvtMeasArgs a, const int32_t *__restrict__ ready, const double *__restrict__ abs_sample,
                                                  const double *__restrict__ code_freq, const double *__restrict__ rem_code_phase,
                                                  const bds_eph *__restrict__ eph, const double *__restrict__ sub_frame_start,
                                                  const double *__restrict__ tow, double *__restrict__ transmit_time,
                                                  double *__restrict__ sat_pos, double *__restrict__ sat_clk) {
    const int c = (int)blockIdx.y;
    const int m = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= a.n_ch || m >= a.n_meas) return;
    double t = NAN, clk = NAN, pos[3] = {NAN, NAN, NAN};
    if (ready[c] & BDS_PVT_READY) {
        const size_t base = (size_t)c * (size_t)a.n;
        const double sample = a.sample_start + a.meas_step * (double)m;  // postNavigation.m:172
        const int index = pvt_index(abs_sample + base, a.n, sample);     // in [0, n - 1]; 0 = no interval starts before `sample`
        if (index >= 1) {
            t = pvt_transmit_time(a, abs_sample + base, code_freq + base, rem_code_phase + base, index, sample, sub_frame_start[c], tow[c]);
            pvt_satpos(eph[c], a.b1c, t, pos, clk);
        }
    }
    const size_t o = (size_t)m * (size_t)a.n_ch + (size_t)c;
    transmit_time[o] = t;
    sat_clk[o] = clk;
    sat_pos[3 * o] = pos[0];
    sat_pos[3 * o + 1] = pos[1];
    sat_pos[3 * o + 2] = pos[2];
}
}  // namespace

extern "C" int bds_pvt_measure(bds_ctx *ctx, const bds_settings *s, int n_ch, int n, const int32_t *ready, const double *absoluteSample,
                               const double *codeFreq, const double *remCodePhase, const bds_eph *eph, const double *subFrameStart,
                               const double *TOW, double sampleStart, double measSampleStep, int n_meas, double *transmitTime,
                               double *satPos, double *satClkCorr) {
    if (!ctx) return BDS_ERR_ARG;
    if (!s || !ready || !absoluteSample || !codeFreq || !remCodePhase || !eph || !subFrameStart || !TOW || !transmitTime || !satPos ||
        !satClkCorr)
        return fail(ctx, BDS_ERR_ARG, "bds_pvt_measure: every pointer is required");
    if (s->signal != BDS_SIGNAL_B1C && s->signal != BDS_SIGNAL_B2A) return fail(ctx, BDS_ERR_ARG, "bds_pvt_measure: settings.signal invalid");
    if (n_ch < 1 || n_ch > 65535 || n < 1 || n_meas < 0 || (double)n_ch * n > 2e8 || (double)n_ch * n_meas > 2e8)
        return fail(ctx, BDS_ERR_ARG, "bds_pvt_measure: n_ch %d (1 .. 65535), n %d, n_meas %d", n_ch, n, n_meas);
    if (!(s->samplingFreq > 0) || !(s->codeFreqBasis > 0) || s->codeLength < 1)
        return fail(ctx, BDS_ERR_ARG, "bds_pvt_measure: samplingFreq, codeFreqBasis and codeLength must be positive");
    for (int c = 0; c < n_ch; ++c) {
        if (eph[c].size != sizeof(bds_eph))
            return fail(ctx, BDS_ERR_ARG, "bds_pvt_measure: eph[%d].size is %u, not sizeof(bds_eph) = %zu", c, eph[c].size, sizeof(bds_eph));
        if ((ready[c] & BDS_PVT_READY) && (eph[c].SatType < 1 || eph[c].SatType > 3))
            return fail(ctx, BDS_ERR_ARG, "bds_pvt_measure: channel %d is marked ready with an empty SatType", c + 1);
    }
    if (n_meas == 0) return 0;
    PvtMeasArgs a;
    a.fs = s->samplingFreq, a.code_length = (double)s->codeLength, a.code_freq_basis = s->codeFreqBasis;
    a.sample_start = sampleStart, a.meas_step = measSampleStep;
    a.n_ch = n_ch, a.n = n, a.n_meas = n_meas, a.b1c = s->signal == BDS_SIGNAL_B1C;

    BDS_HIP(ctx, hipSetDevice(ctx->device));
    DevScope dev;
    const size_t ns = (size_t)n_ch * n, no = (size_t)n_ch * n_meas;
    double *d_abs = nullptr, *d_cf = nullptr, *d_rcp = nullptr, *d_sfs = nullptr, *d_tow = nullptr, *d_tt = nullptr, *d_sp = nullptr,
           *d_clk = nullptr;
    int32_t *d_ready = nullptr;
    bds_eph *d_eph = nullptr;
    hipError_t e = dev.alloc(&d_abs, sizeof(double) * ns);
    if (e == hipSuccess) e = dev.alloc(&d_cf, sizeof(double) * ns);
    if (e == hipSuccess) e = dev.alloc(&d_rcp, sizeof(double) * ns);
    if (e == hipSuccess) e = dev.alloc(&d_sfs, sizeof(double) * n_ch);
    if (e == hipSuccess) e = dev.alloc(&d_tow, sizeof(double) * n_ch);
    if (e == hipSuccess) e = dev.alloc(&d_ready, sizeof(int32_t) * n_ch);
    if (e == hipSuccess) e = dev.alloc(&d_eph, sizeof(bds_eph) * n_ch);
    if (e == hipSuccess) e = dev.alloc(&d_tt, sizeof(double) * no);
    if (e == hipSuccess) e = dev.alloc(&d_clk, sizeof(double) * no);
    if (e == hipSuccess) e = dev.alloc(&d_sp, sizeof(double) * no * 3);
    if (e != hipSuccess) return fail(ctx, BDS_ERR_NOMEM, "bds_pvt_measure: %s", hipGetErrorString(e));
    // the three series cross to the device once
    e = hipMemcpyAsync(d_abs, absoluteSample, sizeof(double) * ns, hipMemcpyHostToDevice, st(ctx));
    if (e == hipSuccess) e = hipMemcpyAsync(d_cf, codeFreq, sizeof(double) * ns, hipMemcpyHostToDevice, st(ctx));
    if (e == hipSuccess) e = hipMemcpyAsync(d_rcp, remCodePhase, sizeof(double) * ns, hipMemcpyHostToDevice, st(ctx));
    if (e == hipSuccess) e = hipMemcpyAsync(d_sfs, subFrameStart, sizeof(double) * n_ch, hipMemcpyHostToDevice, st(ctx));
    if (e == hipSuccess) e = hipMemcpyAsync(d_tow, TOW, sizeof(double) * n_ch, hipMemcpyHostToDevice, st(ctx));
    if (e == hipSuccess) e = hipMemcpyAsync(d_ready, ready, sizeof(int32_t) * n_ch, hipMemcpyHostToDevice, st(ctx));
    if (e == hipSuccess) e = hipMemcpyAsync(d_eph, eph, sizeof(bds_eph) * n_ch, hipMemcpyHostToDevice, st(ctx));
    if (e != hipSuccess) return fail(ctx, BDS_ERR_HIP, "bds_pvt_measure: %s", hipGetErrorString(e));
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // bds_get_timing: search_ms = the kernel alone
    if (dev.event(&ev0) != hipSuccess || dev.event(&ev1) != hipSuccess) ev0 = ev1 = nullptr;
    if (ev0) (void)hipEventRecord(ev0, st(ctx));
    hipLaunchKernelGGL(k_pvt_meas, dim3((unsigned)((n_meas + 255) / 256), (unsigned)n_ch), dim3(256), 0, st(ctx), a,
                       (const int32_t *)d_ready, (const double *)d_abs, (const double *)d_cf, (const double *)d_rcp, (const bds_eph *)d_eph,
                       (const double *)d_sfs, (const double *)d_tow, d_tt, d_sp, d_clk);
    e = hipGetLastError();
    if (ev1) (void)hipEventRecord(ev1, st(ctx));
    if (e == hipSuccess) e = hipMemcpyAsync(transmitTime, d_tt, sizeof(double) * no, hipMemcpyDeviceToHost, st(ctx));
    if (e == hipSuccess) e = hipMemcpyAsync(satClkCorr, d_clk, sizeof(double) * no, hipMemcpyDeviceToHost, st(ctx));
    if (e == hipSuccess) e = hipMemcpyAsync(satPos, d_sp, sizeof(double) * no * 3, hipMemcpyDeviceToHost, st(ctx));
    if (e == hipSuccess) e = hipStreamSynchronize(st(ctx));
    if (e != hipSuccess) return fail(ctx, BDS_ERR_HIP, "bds_pvt_measure: %s", hipGetErrorString(e));
    float ms = 0;
    ctx->timing = bds_timing{};
    if (ev0 && ev1 && hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) ctx->timing.search_ms = ms;
    return n_meas;
}

extern "C" int bds_post_navigation(bds_ctx *ctx, const bds_settings *s, const bds_pvt_params *p, int n_ch, int n, const char *status,
                                   const int32_t *prn, const double *absoluteSample, const double *codeFreq, const double *remCodePhase,
                                   const bds_eph *eph, const double *subFrameStart, const double *TOW, int32_t *ready, int32_t *n_meas,
                                   bds_pvt_out *out) {
    if (!ctx) return BDS_ERR_ARG;
    if (n_meas) *n_meas = 0;
    if (!prn || !codeFreq || !remCodePhase || !ready || !out || out->size != sizeof(bds_pvt_out) || out->cap < 0)
        return fail(ctx, BDS_ERR_ARG, "bds_post_navigation: prn, the three series, ready and out (with .size and .cap set) are required");
    double start = 0, end = 0, step = 0;
    const int nm = bds_pvt_plan(s, p, n_ch, n, status, absoluteSample, eph, subFrameStart, TOW, ready, &start, &end, &step);
    if (nm < 0)
        return fail(ctx, nm,
                    "bds_post_navigation: bds_pvt_plan refused its arguments (a pointer, a size field, the settings, or absoluteSample "
                    "not strictly increasing on a ready channel)");
    if (n_meas) *n_meas = nm;
    if (nm == 0) return 0;
    if (nm > out->cap) return fail(ctx, BDS_ERR_ARG, "bds_post_navigation: %d measurement epochs, out holds %d", nm, out->cap);
    std::vector<double> tt((size_t)nm * n_ch), clk((size_t)nm * n_ch), sp((size_t)nm * n_ch * 3);
    int rc = bds_pvt_measure(ctx, s, n_ch, n, ready, absoluteSample, codeFreq, remCodePhase, eph, subFrameStart, TOW, start, step, nm,
                             tt.data(), sp.data(), clk.data());
    if (rc < 0) return rc;
    rc = bds_pvt_solve(s, p, n_ch, nm, prn, ready, start, step, tt.data(), sp.data(), clk.data(), out);
    if (rc < 0) return fail(ctx, rc, "bds_post_navigation: bds_pvt_solve refused its arguments (an array of out is NULL)");
    return rc;
}
