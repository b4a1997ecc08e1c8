/*
 * bds_mex.c -- MEX gateway: MATLAB <-> libbds_mi355x.so (C ABI of include/bds_mi355x.h).
 *
 * Build (on a machine that has MATLAB; this image has none, so the file is kept
 * logic-free -- everything it calls is exercised through the same C ABI by the
 * repo's ctypes layer and tests):
 *
 *   mex -R2018a -I../include bds_mex.c -L../bds-3-b1c-b2a-sdr-receiver_amd -lbds_mi355x \
 *       LDFLAGS='$LDFLAGS -Wl,-rpath,/opt/rocm/lib'
 *
 * Usage from the drop-in wrappers in this directory:
 *   [carrFreq, codePhase, peakMetric, detected] = bds_mex('acquire', int8(longSignal), settings, signal, iq)
 *       iq (optional, default false): longSignal holds interleaved I/Q pairs (fileType 2);
 *       iq = 2: longSignal is a uint8 array of packed bytes, two 2+2-bit I/Q samples each (fileType 3, the input of
 *       B2a/include/unpack_cplx.m:18-30), as fread(fid, n/2, 'uint8=>uint8') returns them
 *   out = bds_mex('track', path, channel, settings, signal)        % struct of [nCh x nEpochs] arrays
 *   code = bds_mex('gen_code', signal, kind, prn)
 *   [XcorrResult, index] = bds_mex('frame_sync', signal, PRN, bits)   % one channel: second half of
 *       xcorr(sign(bits), pattern) and find(abs(.) >= 1799.5) (B1C) / find(abs(.) > 115) (B2a)
 *   out = bds_mex('nav_decode', signal, PRN, sync_bits, data_bits)   % one channel: the rest of BCNAV1decoding.m (:93-189) /
 *       BCNAV2decoding.m (:99-159).  sync_bits: the prompt series frame_sync takes; data_bits: I_P (B1C), [] for B2a.  struct with
 *       eph (one field per double of bds_eph, [] where the reference leaves []; SatType 0..3, flag, n_entered, idValid 1 x 8),
 *       firstSubFrame, TOW (inf where nothing decoded) and, per candidate (the first 64), the columns index, status, polarity.
 *       mex/B1C/include/BCNAV1decoding.m and mex/B2a/include/BCNAV2decoding.m shape eph like the reference's struct.
 *   out = bds_mex('probe_data', path, settings, signal[, n_samples])   % the numbers of include/probeData.m's figure (mex/probeData.m
 *       draws it): struct with hist_i, hist_q (1 x 257 counts over -128:128; hist_q empty for fileType 1), psd (column: one-sided
 *       16385 bins for fileType 1, else two-sided 32768 bins 0 .. fs), excerpt_re, excerpt_im (the samples of the time-domain
 *       plot), stats (min, max, sum, sum of squares of I, then of Q), n_segments, n_samples.  n_samples: 0 (default) = the
 *       window probeData.m reads, -1 = the whole file behind skipNumberOfBytes.
 *   out = bds_mex('blank_pulses', path_in, path_out, settings, signal, threshold, pre, post[, duty_samples[, piece_samples]])
 *       pulse blanking of a record file (mex/blankPulses.m; bds_blank_file): every sample within [m - pre, m + post] of a sample m of
 *       amplitude above `threshold` (x^2 or I^2 + Q^2 > floor(threshold^2)) is set to 0 in path_out; the bytes in front of
 *       settings.skipNumberOfBytes are copied.  struct with n_samples, n_flagged, n_blanked, n_runs, threshold_sq and duty (column:
 *       blanked samples per duty_samples, empty when duty_samples is 0 or absent).  Not for fileType 3.
 *   out = bds_mex('notch_tones', path_in, path_out, settings, signal, freqs, block_log2[, piece_samples])
 *       excision of narrow-band (CW) interference from a record file (mex/notchTones.m; bds_notch_file): per block of 2^block_log2
 *       samples the complex amplitude of every tone of freqs (Hz on probe_data's axis: 0 .. fs / 2 for fileType 1, signed baseband
 *       frequencies else; at most 8) is estimated and the tone subtracted in path_out; the bytes in front of
 *       settings.skipNumberOfBytes are copied.  struct with n_samples, n_blocks, n_saturated, sum_sq_in, sum_sq_out (doubles: exact
 *       below 2^53), steps (1 x n_tones, the uint32 phase steps applied) and est_re, est_im (n_blocks x n_tones, in LSB).  Not
 *       for fileType 3.
 *   out = bds_mex('corr_function', path, settings, prn, state6, taps)   % the correlation function of tracked epochs (mex/corrFunction.m
 *       builds prn and state6 from trackResults): prn 1 x n, state6 6 x n = {sample offset; blksize; remCodePhase; codeFreq;
 *       remCarrPhase; carrFreq} per item, taps in chips (at most 128, |tau| <= 16).  struct with I, Q ([numel(taps) * n_comp x n],
 *       tap fastest, then component: data, pilot, pilot BOC(6,1)) and n_comp.  The receiver is told from the settings (only
 *       B1C/initSettings.m defines acqCohT).
 *   out = bds_mex('post_navigation', settings, signal, status, PRN, absoluteSample, codeFreq, remCodePhase, eph, subFrameStart, TOW)
 *       postNavigation.m behind its decoding loop (mex/B1C/postNavigation.m and mex/B2a/postNavigation.m run that loop with
 *       'nav_decode').  status: char row, one per channel ('-' = idle); PRN, subFrameStart, TOW: double rows; absoluteSample,
 *       codeFreq, remCodePhase: n x nCh; eph: 1 x nCh struct array of 'nav_decode's eph structs (all fields [] on an idle channel).
 *       settings also needs navSolPeriod, elevationMask, useTropCorr, c and startOffset.  struct with n_meas (0: fewer than 4
 *       channels ready, or no measurement epoch fits), ready (1 x nCh, BDS_PVT_* flags), PRN, el, az, transmitTime, satClkCorr,
 *       rawP, correctedP (nCh x n_meas), DOP (5 x n_meas), X, Y, Z, dt, localTime, currMeasSample, latitude, longitude, height.
 * signal: 1 = B1C, 2 = B2a (the reference keeps one directory per receiver).
 * Acquisition runs on ONE GPU unless BDS_MEX_DEVICES=n (n > 1, or 0 = every visible GPU) opts into the multi-device
 * path of the library (bds_multi_create + RCCL all-reduce): that path has only ever run on one-GPU boxes (with the exchange
 * forced, and with two contexts aliased onto one device), so it is not the default of a MATLAB session.
 * No MATLAB exists in the build image: tests/test_mex_syntax.py compiles this file with -fsyntax-only against a header that
 * declares the MEX API, and tests/test_mex_mock.py builds it against a small stand-in for the MEX runtime
 * (tests/mex_stub/mex_mock.c) and runs every command and every error exit through ctypes.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bds_mi355x.h"
#include "mex.h"

/* The packed input of 'acquire' needs the uint8 part of the Matrix API.  MATLAB's mex defines MATLAB_MEX_FILE; a stand-in for
 * the MEX runtime that declares mxIsUint8 / mxGetUint8s says so with BDS_MEX_HAVE_UINT8 (tests/mex_stub_packed); one that
 * does not (tests/mex_stub) builds a gateway that refuses iq = 2. */
#if defined(MATLAB_MEX_FILE) || defined(BDS_MEX_HAVE_UINT8)
#define BDS_MEX_UINT8 1
#else
#define BDS_MEX_UINT8 0
#endif

/* One bds_multi for the MATLAB session: one GPU by default, BDS_MEX_DEVICES=n GPUs (0 = all visible).  Acquisition
 * goes through bds_acquire_multi (PRN shards + RCCL all-reduce inside the library); tracking, frame sync and the
 * converters run on device 0 of it (tracking needs no exchange: replicas only). */
static bds_multi *g_multi = NULL;

static void cleanup(void) {
    if (g_multi) bds_multi_destroy(g_multi);
    g_multi = NULL;
}

static bds_multi *multi(void) {
    if (!g_multi) {
        const char *e = getenv("BDS_MEX_DEVICES");
        g_multi = bds_multi_create(e ? atoi(e) : 1, NULL);
        if (!g_multi) mexErrMsgIdAndTxt("bds:create", "%s", bds_multi_last_error(NULL));
        mexAtExit(cleanup);
    }
    return g_multi;
}

static bds_ctx *ctx(void) { return bds_multi_ctx(multi(), 0); }

/* Every field of SURVEY.md Appendix D that the selected receiver's initSettings.m defines is REQUIRED: a settings
 * struct with a misspelt or missing field is an error naming the field, never a silent default. */
static const mxArray *need(const mxArray *s, const char *name) {
    const mxArray *f = mxGetField(s, 0, name);
    if (!f) mexErrMsgIdAndTxt("bds:settings", "settings.%s is missing", name);
    return f;
}
static double num(const mxArray *s, const char *name) {
    const mxArray *f = need(s, name);
    if (!(mxIsNumeric(f) || mxIsLogical(f)) || mxGetNumberOfElements(f) != 1)
        mexErrMsgIdAndTxt("bds:settings", "settings.%s must be a numeric scalar", name);
    return mxGetScalar(f);
}

static void pack_settings(const mxArray *s, int signal, bds_settings *o) {
    const mxArray *lst, *dt;
    char dts[32];
    size_t n, i;
    const double *p;
    if (!mxIsStruct(s)) mexErrMsgIdAndTxt("bds:settings", "settings must be a struct");
    if (signal != BDS_SIGNAL_B1C && signal != BDS_SIGNAL_B2A) mexErrMsgIdAndTxt("bds:settings", "signal must be 1 (B1C) or 2 (B2a)");
    memset(o, 0, sizeof(*o));
    o->signal = signal;
    /* both receivers (B1C/initSettings.m:48-151, B2a/initSettings.m:44-130) */
    o->fileType = (int)num(s, "fileType");
    o->samplingFreq = num(s, "samplingFreq");
    o->IF = num(s, "IF");
    o->codeFreqBasis = num(s, "codeFreqBasis");
    o->carrFreqBasis = num(s, "carrFreqBasis");
    o->codeLength = (int)num(s, "codeLength");
    o->numberOfChannels = (int)num(s, "numberOfChannels");
    o->skipNumberOfBytes = (int64_t)num(s, "skipNumberOfBytes");
    o->msToProcess = num(s, "msToProcess");
    o->acqSearchBand = num(s, "acqSearchBand");
    o->acqStep = num(s, "acqStep");
    o->acqThreshold = num(s, "acqThreshold");
    o->resamplingThreshold = num(s, "resamplingThreshold");
    o->resamplingflag = (int)num(s, "resamplingflag");
    o->pilotTRKflag = (int)num(s, "pilotTRKflag");
    o->intTime = num(s, "intTime");
    o->dllCorrelatorSpacing = num(s, "dllCorrelatorSpacing");
    o->dllDampingRatio = num(s, "dllDampingRatio");
    o->dllNoiseBandwidth = num(s, "dllNoiseBandwidth");
    o->pllNoiseBandwidth = num(s, "pllNoiseBandwidth");
    o->CNoInterval = (int)num(s, "CNoInterval");
    /* settings.dataType: the library reads int8 ('schar') records only (tracking.m:237-238) */
    dt = need(s, "dataType");
    if (!mxIsChar(dt) || mxGetString(dt, dts, sizeof(dts)) || strcmp(dts, "schar"))
        mexErrMsgIdAndTxt("bds:settings", "settings.dataType must be 'schar' (int8 samples)");
    o->dataType = 0;
    if (signal == BDS_SIGNAL_B1C) { /* B1C/initSettings.m:60,70,102 */
        o->acqCohT = num(s, "acqCohT");
        o->pilotACQflag = (int)num(s, "pilotACQflag");
        o->FEBW = num(s, "FEBW");
        o->fineNoncoh = 1;
    } else { /* B2a/initSettings.m:84 */
        o->fineNoncoh = (int)num(s, "fineNoncoh");
        o->acqCohT = 10;
        o->pilotACQflag = 1;
    }
    lst = need(s, "acqSatelliteList");
    if (!mxIsDouble(lst)) mexErrMsgIdAndTxt("bds:settings", "settings.acqSatelliteList must be a double row vector");
    n = mxGetNumberOfElements(lst);
    p = mxGetDoubles(lst);
    if (n > BDS_MAX_PRN) mexErrMsgIdAndTxt("bds:settings", "settings.acqSatelliteList longer than 63");
    o->n_acq = (int)n;
    for (i = 0; i < n; ++i) o->acqSatelliteList[i] = (int)p[i];
}

static void do_acquire(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    bds_settings s;
    int max_prn = 0, i, rc, iq;
    mxArray *det;
    const int8_t *samples;
    size_t n_samples;
    if (nrhs != 4 && nrhs != 5) mexErrMsgIdAndTxt("bds:args", "acquire: (int8 longSignal, settings, signal[, iq])");
    iq = nrhs == 5 ? (int)mxGetScalar(prhs[4]) : 0;
    if (iq == 2) { /* packed bytes: two samples each */
#if BDS_MEX_UINT8
        if (!mxIsUint8(prhs[1])) mexErrMsgIdAndTxt("bds:args", "acquire: iq = 2 takes a uint8 longSignal of packed bytes (fileType 3)");
        if (mxGetNumberOfElements(prhs[1]) == 0) mexErrMsgIdAndTxt("bds:args", "acquire: longSignal holds 0 packed bytes");
        samples = (const int8_t *)mxGetUint8s(prhs[1]);
        n_samples = mxGetNumberOfElements(prhs[1]) * 2;
#else
        mexErrMsgIdAndTxt("bds:args", "acquire: iq = 2 (packed uint8 longSignal) is not built into this gateway");
        return;
#endif
    } else {
        if (!mxIsInt8(prhs[1])) mexErrMsgIdAndTxt("bds:args", "acquire: (int8 longSignal, settings, signal[, iq])");
        iq = iq != 0;
        samples = (const int8_t *)mxGetInt8s(prhs[1]);
        n_samples = mxGetNumberOfElements(prhs[1]) / (iq ? 2 : 1);
    }
    pack_settings(prhs[2], (int)mxGetScalar(prhs[3]), &s);
    if ((iq == 2) != (s.fileType == 3))
        mexErrMsgIdAndTxt("bds:args", "acquire: iq = 2 (packed uint8 longSignal) and settings.fileType = 3 go together");
    for (i = 0; i < s.n_acq; ++i)
        if (s.acqSatelliteList[i] > max_prn) max_prn = s.acqSatelliteList[i];
    plhs[0] = mxCreateDoubleMatrix(1, max_prn, mxREAL);
    plhs[1] = mxCreateDoubleMatrix(1, max_prn, mxREAL);
    plhs[2] = mxCreateDoubleMatrix(1, max_prn, mxREAL);
    det = mxCreateNumericMatrix(1, max_prn, mxINT32_CLASS, mxREAL);
    {
        bds_acq_job job;
        memset(&job, 0, sizeof(job));
        job.settings = &s;
        job.samples = samples;
        job.n_samples = n_samples;
        job.is_complex = iq;
        job.max_prn = max_prn;
        job.carrFreq = mxGetDoubles(plhs[0]);
        job.codePhase = mxGetDoubles(plhs[1]);
        job.peakMetric = mxGetDoubles(plhs[2]);
        job.detected = (int32_t *)mxGetInt32s(det);
        rc = bds_acquire_multi(multi(), 1, &job); /* all GPUs of the session: PRN shards + one RCCL all-reduce */
    }
    if (rc) mexErrMsgIdAndTxt("bds:acquire", "%s", bds_multi_last_error(g_multi));
    if (nlhs > 3)
        plhs[3] = det;
    else
        mxDestroyArray(det);
}

static double *out_field(mxArray *st, const char *name, int rows, int cols) {
    mxArray *a = mxCreateDoubleMatrix(rows, cols, mxREAL); /* column-major: [epoch x channel] */
    mxAddField(st, name);
    mxSetField(st, 0, name, a);
    return mxGetDoubles(a);
}

static void do_track(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    bds_settings s;
    bds_track_out o;
    bds_channel *ch;
    char path[4096];
    int n_ch, n_ep, n_cno, c, rc, wb, pilot;
    mxArray *st, *comp, *stat;
    (void)nlhs;
    if (nrhs != 5) mexErrMsgIdAndTxt("bds:args", "track: (path, channel, settings, signal)");
    mxGetString(prhs[1], path, sizeof(path));
    pack_settings(prhs[3], (int)mxGetScalar(prhs[4]), &s);
    n_ch = (int)mxGetNumberOfElements(prhs[2]);
    ch = (bds_channel *)mxCalloc((size_t)n_ch, sizeof(bds_channel));
    for (c = 0; c < n_ch; ++c) {
        const mxArray *stc = mxGetField(prhs[2], c, "status");
        ch[c].PRN = (int)mxGetScalar(mxGetField(prhs[2], c, "PRN"));
        ch[c].acquiredFreq = mxGetScalar(mxGetField(prhs[2], c, "acquiredFreq"));
        ch[c].codePhase = mxGetScalar(mxGetField(prhs[2], c, "codePhase"));
        ch[c].codeFreq = mxGetScalar(mxGetField(prhs[2], c, "codeFreq"));
        ch[c].status = stc ? (int)mxGetChars(stc)[0] : '-';
    }
    /* epochs: msToProcess (B2a/tracking.m:100) or round(msToProcess/1000/intTime) (WB_tracking.m:56) */
    n_ep = s.signal == BDS_SIGNAL_B2A ? (int)s.msToProcess : (int)(s.msToProcess / 1000 / s.intTime + 0.5);
    n_cno = n_ep / s.CNoInterval;
    wb = s.signal == BDS_SIGNAL_B1C && s.pilotTRKflag == 2;
    pilot = wb || s.pilotTRKflag == 1;
    memset(&o, 0, sizeof(o));
    o.n_ch = n_ch;
    o.n_epochs = n_ep;
    o.n_cno = n_cno;
    st = mxCreateStructMatrix(1, 1, 0, NULL);
#define F(name) o.name = out_field(st, #name, n_ep, n_ch)
    F(absoluteSample); F(codeFreq); F(carrFreq); F(I_P); F(I_E); F(I_L); F(Q_E); F(Q_P); F(Q_L);
    if (pilot) { F(Pilot_I_P); F(Pilot_Q_P); }
    if (wb) { F(Pilot_I_E); F(Pilot_I_L); F(Pilot_Q_E); F(Pilot_Q_L); }
    F(dllDiscr); F(dllDiscrFilt); F(pllDiscr); F(pllDiscrFilt); F(remCodePhase); F(remCarrPhase);
#undef F
#define G(name) o.name = out_field(st, #name, n_cno, n_ch)
    G(DataCNo); G(DataPLD);
    if (pilot) { G(PilotCNo); G(PilotPLD); G(SigCNo); }
#undef G
    comp = mxCreateNumericMatrix(1, n_ch, mxINT32_CLASS, mxREAL);
    stat = mxCreateNumericMatrix(1, n_ch, mxINT32_CLASS, mxREAL);
    o.completed = (int32_t *)mxGetInt32s(comp);
    o.status = (int32_t *)mxGetInt32s(stat);
    mxAddField(st, "completed");
    mxSetField(st, 0, "completed", comp);
    mxAddField(st, "status");
    mxSetField(st, 0, "status", stat);
    /* the C arrays are channel-major [n_ch][n_epochs] == MATLAB column-major [n_epochs x n_ch] */
    rc = bds_track(ctx(), &s, path, n_ch, ch, &o);
    mxFree(ch);
    if (rc) mexErrMsgIdAndTxt("bds:track", "%s", bds_last_error(ctx()));
    plhs[0] = st;
}

static void do_gen_code(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    int8_t buf[122760];
    int n, i;
    double *p;
    (void)nlhs;
    if (nrhs != 4) mexErrMsgIdAndTxt("bds:args", "gen_code: (signal, kind, prn)");
    n = bds_gen_code((int)mxGetScalar(prhs[1]), (int)mxGetScalar(prhs[2]), (int)mxGetScalar(prhs[3]), buf, 122760);
    if (n < 0) mexErrMsgIdAndTxt("bds:gen_code", "bad signal/kind/prn");
    plhs[0] = mxCreateDoubleMatrix(1, n, mxREAL);
    p = mxGetDoubles(plhs[0]);
    for (i = 0; i < n; ++i) p[i] = buf[i];
}

/* BCNAV1decoding.m:75-91 / BCNAV2decoding.m:84-97 for one channel */
static void do_frame_sync(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    int signal, n, m, M, i, total;
    int32_t prn, cnt = 0, *xc, *idx;
    double *p;
    if (nrhs != 4 || !mxIsDouble(prhs[3])) mexErrMsgIdAndTxt("bds:args", "frame_sync: (signal, PRN, bits)");
    signal = (int)mxGetScalar(prhs[1]);
    prn = (int32_t)mxGetScalar(prhs[2]);
    n = (int)mxGetNumberOfElements(prhs[3]);
    m = signal == BDS_SIGNAL_B1C ? 1800 : 120;
    M = n > m ? n : m;
    xc = (int32_t *)mxCalloc((size_t)M, sizeof(int32_t));
    idx = (int32_t *)mxCalloc((size_t)M, sizeof(int32_t));
    total = bds_frame_sync(ctx(), signal, 1, &prn, mxGetDoubles(prhs[3]), n, xc, idx, &cnt, M);
    if (total < 0) mexErrMsgIdAndTxt("bds:frame_sync", "%s", bds_last_error(ctx()));
    plhs[0] = mxCreateDoubleMatrix(1, M, mxREAL);
    p = mxGetDoubles(plhs[0]);
    for (i = 0; i < M; ++i) p[i] = xc[i];
    if (nlhs > 1) {
        plhs[1] = mxCreateDoubleMatrix(cnt, 1, mxREAL); /* index = find(...)' is a column */
        p = mxGetDoubles(plhs[1]);
        for (i = 0; i < cnt; ++i) p[i] = idx[i];
    }
    mxFree(xc);
    mxFree(idx);
}

/* BCNAV1decoding.m:93-189 / BCNAV2decoding.m:99-159 for one channel: candidates, frame decoding, ephemeris, TOW */
static void eph_field(mxArray *st, const char *name, double v) {
    double *p = out_field(st, name, v != v ? 0 : 1, v != v ? 0 : 1); /* NaN = the reference's [] */
    if (v == v) p[0] = v;
}

static void do_nav_decode(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    enum { CAP = 64 };
    bds_settings s;
    bds_nav_frame *fr;
    bds_eph e;
    int32_t prn, cnt = 0;
    double first = 0, tow = 0, *pi, *ps, *pp;
    const double *data = NULL;
    int n, rc, i, shown;
    mxArray *res, *eph;
    (void)nlhs;
    if (nrhs != 5 || !mxIsDouble(prhs[3]) || !mxIsDouble(prhs[4])) mexErrMsgIdAndTxt("bds:args", "nav_decode: (signal, PRN, sync_bits, data_bits)");
    memset(&s, 0, sizeof(s));
    s.signal = (int)mxGetScalar(prhs[1]);
    prn = (int32_t)mxGetScalar(prhs[2]);
    n = (int)mxGetNumberOfElements(prhs[3]);
    if (mxGetNumberOfElements(prhs[4]) != 0) {
        if ((int)mxGetNumberOfElements(prhs[4]) != n) mexErrMsgIdAndTxt("bds:args", "nav_decode: sync_bits and data_bits differ in length");
        data = mxGetDoubles(prhs[4]);
    }
    memset(&e, 0, sizeof(e));
    e.size = sizeof(e);
    fr = (bds_nav_frame *)mxCalloc(CAP, sizeof(bds_nav_frame));
    rc = bds_nav_decode(ctx(), &s, 1, &prn, mxGetDoubles(prhs[3]), data, n, fr, &cnt, CAP, &e, &first, &tow);
    if (rc < 0) {
        mxFree(fr);
        mexErrMsgIdAndTxt("bds:nav_decode", "%s", bds_last_error(ctx()));
    }
    res = mxCreateStructMatrix(1, 1, 0, NULL);
    eph = mxCreateStructMatrix(1, 1, 0, NULL);
#define BDS_EPH_X(name) eph_field(eph, #name, e.name);
    BDS_EPH_FIELDS(BDS_EPH_X)
#undef BDS_EPH_X
    out_field(eph, "SatType", 1, 1)[0] = e.SatType;
    out_field(eph, "flag", 1, 1)[0] = e.flag;
    out_field(eph, "n_entered", 1, 1)[0] = e.n_entered;
    pi = out_field(eph, "idValid", 1, 8);
    for (i = 0; i < 8; ++i) pi[i] = e.idValid[i];
    mxAddField(res, "eph");
    mxSetField(res, 0, "eph", eph);
    out_field(res, "firstSubFrame", 1, 1)[0] = first;
    out_field(res, "TOW", 1, 1)[0] = tow;
    out_field(res, "n_frames", 1, 1)[0] = cnt;
    shown = cnt < CAP ? cnt : CAP;
    pi = out_field(res, "index", shown, 1);
    ps = out_field(res, "status", shown, 1);
    pp = out_field(res, "polarity", shown, 1);
    for (i = 0; i < shown; ++i) pi[i] = fr[i].index, ps[i] = fr[i].status, pp[i] = fr[i].polarity;
    mxFree(fr);
    plhs[0] = res;
}

/* include/probeData.m:63-168 of either receiver: everything the figure shows, computed on the device */
static void do_probe_data(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    bds_settings s;
    bds_probe_out o;
    char path[4096];
    int64_t hist[2][257], n_samples, n_time;
    double spc, *hi, *hq, *st, *ex_im;
    int cplx, rc, i, n_psd;
    mxArray *out;
    (void)nlhs;
    if (nrhs != 4 && nrhs != 5) mexErrMsgIdAndTxt("bds:args", "probe_data: (path, settings, signal[, n_samples])");
    if (mxGetString(prhs[1], path, sizeof(path))) mexErrMsgIdAndTxt("bds:args", "File name must be a string"); /* probeData.m:50 */
    pack_settings(prhs[2], (int)mxGetScalar(prhs[3]), &s);
    n_samples = nrhs == 5 ? (int64_t)mxGetScalar(prhs[4]) : 0;
    cplx = s.fileType != 1;
    spc = (double)(int64_t)(s.samplingFreq / (s.codeFreqBasis / s.codeLength) + 0.5); /* probeData.m:66-67 */
    /* B2a/include/probeData.m:96 round(spc / 500) of a real record, :106 round(spc / 2) of I/Q; B1C/include/probeData.m:96,106 spc / 2 */
    n_time = (int64_t)(spc / ((!cplx && s.signal == BDS_SIGNAL_B2A) ? 500 : 2) + 0.5);
    if (n_samples > 0 && n_time > n_samples) n_time = n_samples;
    n_psd = cplx ? 32768 : 16385;
    memset(&o, 0, sizeof(o));
    out = mxCreateStructMatrix(1, 1, 0, NULL);
    hi = out_field(out, "hist_i", 1, 257);
    hq = out_field(out, "hist_q", 1, cplx ? 257 : 0);
    o.psd = out_field(out, "psd", n_psd, 1);
    o.cap = n_psd;
    o.excerpt_re = out_field(out, "excerpt_re", 1, (int)n_time);
    ex_im = out_field(out, "excerpt_im", 1, cplx ? (int)n_time : 0);
    o.excerpt_im = cplx ? ex_im : NULL;
    st = out_field(out, "stats", 1, 8);
    o.hist_i = hist[0];
    o.hist_q = hist[1];
    rc = bds_probe_data_file(ctx(), &s, path, n_samples, n_time, &o);
    if (rc) {
        mxDestroyArray(out);
        mexErrMsgIdAndTxt("bds:probe_data", "%s", bds_last_error(ctx()));
    }
    for (i = 0; i < 257; ++i) {
        hi[i] = (double)hist[0][i];
        if (cplx) hq[i] = (double)hist[1][i];
    }
    st[0] = (double)o.min_i, st[1] = (double)o.max_i, st[2] = (double)o.sum_i, st[3] = (double)o.sumsq_i;
    st[4] = (double)o.min_q, st[5] = (double)o.max_q, st[6] = (double)o.sum_q, st[7] = (double)o.sumsq_q;
    out_field(out, "n_segments", 1, 1)[0] = (double)o.n_segments;
    out_field(out, "n_samples", 1, 1)[0] = (double)o.n_samples;
    plhs[0] = out;
}

/* Pulse blanking of a record file in front of acquisition and tracking (bds_blank_file): file in, file out, the report */
static void do_blank_pulses(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    bds_settings s;
    bds_blank_opts o;
    bds_blank_out r;
    char path_in[4096], path_out[4096];
    double thr, *pd;
    int64_t piece = 0, bins = 0, file_samples, i;
    int rc, sb;
    FILE *f;
    mxArray *rep;
    (void)nlhs;
    if (nrhs < 8 || nrhs > 10)
        mexErrMsgIdAndTxt("bds:args", "blank_pulses: (path_in, path_out, settings, signal, threshold, pre, post[, duty_samples[, piece_samples]])");
    if (mxGetString(prhs[1], path_in, sizeof(path_in)) || mxGetString(prhs[2], path_out, sizeof(path_out)))
        mexErrMsgIdAndTxt("bds:args", "File name must be a string");
    pack_settings(prhs[3], (int)mxGetScalar(prhs[4]), &s);
    thr = mxGetScalar(prhs[5]);
    if (!(thr >= 0)) mexErrMsgIdAndTxt("bds:args", "blank_pulses: threshold must be an amplitude >= 0");
    memset(&o, 0, sizeof(o));
    memset(&r, 0, sizeof(r));
    o.threshold_sq = thr * thr >= 4294967295.0 ? 4294967295u : (uint32_t)floor(thr * thr);
    o.pre = (int32_t)mxGetScalar(prhs[6]);
    o.post = (int32_t)mxGetScalar(prhs[7]);
    o.duty_samples = nrhs >= 9 ? (int64_t)mxGetScalar(prhs[8]) : 0;
    if (nrhs == 10) piece = (int64_t)mxGetScalar(prhs[9]);
    if (o.duty_samples > 0) { /* the bins of the window behind skipNumberOfBytes: the file's length tells how many */
        sb = (s.fileType == 2 ? 2 : 1) * (s.dataType == 1 ? 2 : 1);
        f = fopen(path_in, "rb");
        if (!f) mexErrMsgIdAndTxt("bds:blank_pulses", "Unable to read file %s", path_in);
        fseek(f, 0, SEEK_END);
        file_samples = (int64_t)ftell(f) / sb - s.skipNumberOfBytes;
        fclose(f);
        bins = file_samples > 0 ? (file_samples + o.duty_samples - 1) / o.duty_samples : 0;
        r.duty = (int32_t *)mxCalloc((size_t)(bins > 0 ? bins : 1), sizeof(int32_t));
        r.duty_cap = bins;
    }
    rc = bds_blank_file(ctx(), &s, path_in, path_out, -1, piece, &o, &r);
    if (rc) {
        if (r.duty) mxFree(r.duty);
        mexErrMsgIdAndTxt("bds:blank_pulses", "%s", bds_last_error(ctx()));
    }
    rep = mxCreateStructMatrix(1, 1, 0, NULL);
    out_field(rep, "n_samples", 1, 1)[0] = (double)r.n_samples;
    out_field(rep, "n_flagged", 1, 1)[0] = (double)r.n_flagged;
    out_field(rep, "n_blanked", 1, 1)[0] = (double)r.n_blanked;
    out_field(rep, "n_runs", 1, 1)[0] = (double)r.n_runs;
    out_field(rep, "threshold_sq", 1, 1)[0] = (double)o.threshold_sq;
    pd = out_field(rep, "duty", (int)r.n_duty, r.n_duty ? 1 : 0);
    for (i = 0; i < r.n_duty; ++i) pd[i] = (double)r.duty[i];
    if (r.duty) mxFree(r.duty);
    plhs[0] = rep;
}

/* Tone excision of a record file in front of acquisition and tracking (bds_notch_file): file in, file out, report and estimates */
static void do_notch_tones(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    bds_settings s;
    bds_notch_opts o;
    bds_notch_out r;
    char path_in[4096], path_out[4096];
    double *pf, *pr, *pi;
    int64_t piece = 0, file_samples, n_blocks, b;
    int rc, sb, k, n_tones;
    FILE *f;
    mxArray *nr;
    (void)nlhs;
    if (nrhs < 7 || nrhs > 8 || !mxIsDouble(prhs[5]))
        mexErrMsgIdAndTxt("bds:args", "notch_tones: (path_in, path_out, settings, signal, freqs, block_log2[, piece_samples])");
    if (mxGetString(prhs[1], path_in, sizeof(path_in)) || mxGetString(prhs[2], path_out, sizeof(path_out)))
        mexErrMsgIdAndTxt("bds:args", "File name must be a string");
    pack_settings(prhs[3], (int)mxGetScalar(prhs[4]), &s);
    n_tones = (int)mxGetNumberOfElements(prhs[5]);
    if (n_tones < 1 || n_tones > BDS_NOTCH_MAX_TONES) mexErrMsgIdAndTxt("bds:args", "notch_tones: freqs holds 1 to %d frequencies", BDS_NOTCH_MAX_TONES);
    memset(&o, 0, sizeof(o));
    memset(&r, 0, sizeof(r));
    pf = mxGetDoubles(prhs[5]);
    for (k = 0; k < n_tones; ++k) { /* floor(f / fs 2^32 + 0.5) mod 2^32 */
        double t = fmod(floor(pf[k] / s.samplingFreq * 4294967296.0 + 0.5), 4294967296.0);
        if (!(t == t)) mexErrMsgIdAndTxt("bds:args", "notch_tones: freqs(%d) is not a frequency", k + 1);
        if (t < 0) t += 4294967296.0;
        o.step[k] = (uint32_t)t;
    }
    o.n_tones = n_tones;
    o.block_log2 = (int32_t)mxGetScalar(prhs[6]);
    o.apply = 1;
    if (nrhs == 8) piece = (int64_t)mxGetScalar(prhs[7]);
    if (o.block_log2 < BDS_NOTCH_MIN_LOG2 || o.block_log2 > BDS_NOTCH_MAX_LOG2)
        mexErrMsgIdAndTxt("bds:args", "notch_tones: block_log2 runs from %d to %d", BDS_NOTCH_MIN_LOG2, BDS_NOTCH_MAX_LOG2);
    sb = (s.fileType == 2 ? 2 : 1) * (s.dataType == 1 ? 2 : 1); /* the estimates of the window behind skipNumberOfBytes */
    f = fopen(path_in, "rb");
    if (!f) mexErrMsgIdAndTxt("bds:notch_tones", "Unable to read file %s", path_in);
    fseek(f, 0, SEEK_END);
    file_samples = (int64_t)ftell(f) / sb - s.skipNumberOfBytes;
    fclose(f);
    n_blocks = file_samples > 0 ? (file_samples + ((int64_t)1 << o.block_log2) - 1) >> o.block_log2 : 0;
    r.est = (int32_t *)mxCalloc((size_t)(n_blocks > 0 ? n_blocks : 1) * n_tones * 2, sizeof(int32_t));
    r.est_cap = n_blocks * n_tones;
    rc = bds_notch_file(ctx(), &s, path_in, path_out, -1, piece, &o, &r);
    if (rc) {
        mxFree(r.est);
        mexErrMsgIdAndTxt("bds:notch_tones", "%s", bds_last_error(ctx()));
    }
    nr = mxCreateStructMatrix(1, 1, 0, NULL);
    out_field(nr, "n_samples", 1, 1)[0] = (double)r.n_samples;
    out_field(nr, "n_blocks", 1, 1)[0] = (double)r.n_blocks;
    out_field(nr, "n_saturated", 1, 1)[0] = (double)r.n_saturated;
    out_field(nr, "sum_sq_in", 1, 1)[0] = (double)r.sum_sq_in;
    out_field(nr, "sum_sq_out", 1, 1)[0] = (double)r.sum_sq_out;
    pf = out_field(nr, "steps", 1, n_tones);
    for (k = 0; k < n_tones; ++k) pf[k] = (double)o.step[k];
    pr = out_field(nr, "est_re", (int)r.n_blocks, n_tones);
    pi = out_field(nr, "est_im", (int)r.n_blocks, n_tones);
    for (b = 0; b < r.n_blocks; ++b)
        for (k = 0; k < n_tones; ++k) { /* column-major [n_blocks x n_tones] */
            pr[(size_t)k * r.n_blocks + b] = (double)r.est[(b * n_tones + k) * 2] / (double)(1 << BDS_NOTCH_AMP_FRAC);
            pi[(size_t)k * r.n_blocks + b] = (double)r.est[(b * n_tones + k) * 2 + 1] / (double)(1 << BDS_NOTCH_AMP_FRAC);
        }
    mxFree(r.est);
    plhs[0] = nr;
}

/* postNavigation.m:100-298 of either receiver behind the decoding loop: readiness, measurement grid, pseudoranges, satellite and
 * receiver positions (bds_post_navigation).  mex/B1C/postNavigation.m and mex/B2a/postNavigation.m decode the channels with
 * 'nav_decode' and hand its eph structs back in. */
static double eph_number(const mxArray *eph, size_t c, const char *name, double empty) {
    const mxArray *f = mxGetField(eph, c, name);
    if (!f || mxGetNumberOfElements(f) == 0) return empty; /* [] */
    if (!mxIsDouble(f)) mexErrMsgIdAndTxt("bds:args", "post_navigation: eph(%d).%s must be a double", (int)c + 1, name);
    return mxGetDoubles(f)[0];
}

static void do_post_navigation(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    static const char *per_ch[] = {"PRN", "el", "az", "transmitTime", "satClkCorr", "rawP", "correctedP"};
    static const char *per_m[] = {"X", "Y", "Z", "dt", "localTime", "currMeasSample", "latitude", "longitude", "height"};
    bds_settings s;
    bds_pvt_params p;
    bds_pvt_out o;
    bds_eph *eph;
    char *status;
    int32_t *prn, *ready, n_meas = 0;
    double *buf, *q, step;
    double **ch_slot[7], **m_slot[9];
    const double *pp, *lo, *hi;
    const mxArray *f;
    size_t n_ch, n, c, k, i, cap, per;
    int rc, signal, m;
    mxArray *res;
    (void)nlhs;
    if (nrhs != 11) mexErrMsgIdAndTxt("bds:args", "post_navigation: (settings, signal, status, PRN, absoluteSample, codeFreq, remCodePhase, eph, subFrameStart, TOW)");
    signal = (int)mxGetScalar(prhs[2]);
    pack_settings(prhs[1], signal, &s);
    memset(&p, 0, sizeof(p));
    p.size = sizeof(p);
    p.navSolPeriod = num(prhs[1], "navSolPeriod");
    p.elevationMask = num(prhs[1], "elevationMask");
    p.useTropCorr = (int32_t)num(prhs[1], "useTropCorr");
    p.c = num(prhs[1], "c");
    p.startOffset = num(prhs[1], "startOffset");
    n_ch = mxGetNumberOfElements(prhs[4]);
    if (n_ch < 1 || !mxIsChar(prhs[3]) || mxGetNumberOfElements(prhs[3]) != n_ch || !mxIsDouble(prhs[4]))
        mexErrMsgIdAndTxt("bds:args", "post_navigation: status is a char row and PRN a double row, one entry per channel");
    for (i = 5; i <= 7; ++i)
        if (!mxIsDouble(prhs[i]) || mxGetNumberOfElements(prhs[i]) == 0 || mxGetNumberOfElements(prhs[i]) % n_ch ||
            mxGetNumberOfElements(prhs[i]) != mxGetNumberOfElements(prhs[5]))
            mexErrMsgIdAndTxt("bds:args", "post_navigation: absoluteSample, codeFreq and remCodePhase are n x numel(PRN) doubles, one column per channel");
    n = mxGetNumberOfElements(prhs[5]) / n_ch;
    if (!mxIsStruct(prhs[8]) || mxGetNumberOfElements(prhs[8]) != n_ch || !mxIsDouble(prhs[9]) || mxGetNumberOfElements(prhs[9]) != n_ch ||
        !mxIsDouble(prhs[10]) || mxGetNumberOfElements(prhs[10]) != n_ch)
        mexErrMsgIdAndTxt("bds:args", "post_navigation: eph is a struct array, subFrameStart and TOW double rows, one entry per channel");
    status = (char *)mxCalloc(n_ch + 1, 1);
    prn = (int32_t *)mxCalloc(n_ch, sizeof(int32_t));
    ready = (int32_t *)mxCalloc(n_ch, sizeof(int32_t));
    eph = (bds_eph *)mxCalloc(n_ch, sizeof(bds_eph));
    pp = mxGetDoubles(prhs[4]);
    for (c = 0; c < n_ch; ++c) {
        status[c] = (char)mxGetChars(prhs[3])[c];
        prn[c] = (int32_t)pp[c];
        eph[c].size = sizeof(bds_eph);
#define BDS_EPH_X(name) eph[c].name = eph_number(prhs[8], c, #name, NAN);
        BDS_EPH_FIELDS(BDS_EPH_X)
#undef BDS_EPH_X
        eph[c].SatType = (int32_t)eph_number(prhs[8], c, "SatType", 0);
        eph[c].flag = (int32_t)eph_number(prhs[8], c, "flag", 0);
        eph[c].n_entered = (int32_t)eph_number(prhs[8], c, "n_entered", 0);
        f = mxGetField(prhs[8], c, "idValid");
        if (f && mxIsDouble(f))
            for (k = 0; k < 8 && k < mxGetNumberOfElements(f); ++k) eph[c].idValid[k] = (int32_t)mxGetDoubles(f)[k];
    }
    /* the capacity: what the plan can give at most, (last - first sample) / step + 1 */
    step = (double)(int64_t)(s.samplingFreq * p.navSolPeriod / 1000);
    lo = hi = mxGetDoubles(prhs[5]);
    for (i = 0, pp = lo; i < n * n_ch; ++i) {
        if (pp[i] < *lo) lo = pp + i;
        if (pp[i] > *hi) hi = pp + i;
    }
    cap = step >= 1 && *hi - *lo >= 0 && (*hi - *lo) / step < 1e8 ? (size_t)((*hi - *lo) / step) + 1 : 1;
    per = 7 * n_ch + 5 + 9;
    buf = (double *)mxCalloc(per * cap, sizeof(double));
    memset(&o, 0, sizeof(o));
    o.size = sizeof(o);
    o.cap = (int32_t)cap;
    ch_slot[0] = &o.PRN, ch_slot[1] = &o.el, ch_slot[2] = &o.az, ch_slot[3] = &o.transmitTime, ch_slot[4] = &o.satClkCorr;
    ch_slot[5] = &o.rawP, ch_slot[6] = &o.correctedP; /* in the order of per_ch / per_m */
    m_slot[0] = &o.X, m_slot[1] = &o.Y, m_slot[2] = &o.Z, m_slot[3] = &o.dt, m_slot[4] = &o.localTime, m_slot[5] = &o.currMeasSample;
    m_slot[6] = &o.latitude, m_slot[7] = &o.longitude, m_slot[8] = &o.height;
    for (i = 0, q = buf; i < 7; ++i, q += n_ch * cap) *ch_slot[i] = q;
    o.DOP = q, q += 5 * cap;
    for (i = 0; i < 9; ++i, q += cap) *m_slot[i] = q;
    /* an n x nCh matrix is, column-major, the C array [nCh][n] */
    rc = bds_post_navigation(ctx(), &s, &p, (int)n_ch, (int)n, status, prn, mxGetDoubles(prhs[5]), mxGetDoubles(prhs[6]), mxGetDoubles(prhs[7]),
                             eph, mxGetDoubles(prhs[9]), mxGetDoubles(prhs[10]), ready, &n_meas, &o);
    mxFree(status);
    mxFree(prn);
    mxFree(eph);
    if (rc < 0) {
        mxFree(ready);
        mxFree(buf);
        mexErrMsgIdAndTxt("bds:post_navigation", "%s", bds_last_error(ctx()));
    }
    res = mxCreateStructMatrix(1, 1, 0, NULL);
    out_field(res, "n_meas", 1, 1)[0] = rc;
    q = out_field(res, "ready", 1, (int)n_ch);
    for (c = 0; c < n_ch; ++c) q[c] = ready[c];
    for (i = 0; i < 7; ++i) { /* [nCh x n_meas], as navSolutions.<name>(channelNr, currMeasNr) */
        q = out_field(res, per_ch[i], (int)n_ch, rc);
        for (m = 0; m < rc; ++m)
            for (c = 0; c < n_ch; ++c) q[(size_t)m * n_ch + c] = (*ch_slot[i])[c * cap + (size_t)m];
    }
    q = out_field(res, "DOP", 5, rc);
    for (m = 0; m < rc; ++m)
        for (k = 0; k < 5; ++k) q[(size_t)m * 5 + k] = o.DOP[k * cap + (size_t)m];
    for (i = 0; i < 9; ++i) {
        q = out_field(res, per_m[i], 1, rc);
        for (m = 0; m < rc; ++m) q[m] = (*m_slot[i])[m];
    }
    mxFree(ready);
    mxFree(buf);
    plhs[0] = res;
}

/* bds_corr_function: the correlation function of tracked epochs at the caller's taps (mex/corrFunction.m builds the states) */
static void do_corr_function(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    bds_settings s;
    char path[4096];
    size_t n_items, n_taps, i, n;
    int32_t *prn, n_comp = 0;
    double *buf, *pi, *pq;
    const double *p;
    int rc, signal;
    mxArray *res, *a;
    (void)nlhs;
    if (nrhs != 6 || !mxIsDouble(prhs[3]) || !mxIsDouble(prhs[4]) || !mxIsDouble(prhs[5]))
        mexErrMsgIdAndTxt("bds:args", "corr_function: (path, settings, prn, state6, taps)");
    if (mxGetString(prhs[1], path, sizeof(path))) mexErrMsgIdAndTxt("bds:args", "File name must be a string");
    if (!mxIsStruct(prhs[2])) mexErrMsgIdAndTxt("bds:settings", "settings must be a struct");
    signal = mxGetField(prhs[2], 0, "acqCohT") ? BDS_SIGNAL_B1C : BDS_SIGNAL_B2A; /* only B1C/initSettings.m defines acqCohT */
    pack_settings(prhs[2], signal, &s);
    n_items = mxGetNumberOfElements(prhs[3]);
    n_taps = mxGetNumberOfElements(prhs[5]);
    if (n_items < 1 || mxGetNumberOfElements(prhs[4]) != 6 * n_items)
        mexErrMsgIdAndTxt("bds:args", "corr_function: state6 must be 6 x numel(prn), one column per item");
    if (n_taps < 1 || n_taps > 128) mexErrMsgIdAndTxt("bds:args", "corr_function: 1 .. 128 taps");
    prn = (int32_t *)mxCalloc(n_items, sizeof(int32_t));
    p = mxGetDoubles(prhs[3]);
    for (i = 0; i < n_items; ++i) prn[i] = (int32_t)p[i];
    buf = (double *)mxCalloc(n_items * 3 * n_taps * 2, sizeof(double)); /* [item][comp][tap][2], three components at most */
    /* a 6 x n matrix is, column-major, the C array [n][6] */
    rc = bds_corr_function(ctx(), &s, path, (int)n_items, prn, mxGetDoubles(prhs[4]), (int)n_taps, mxGetDoubles(prhs[5]), buf, &n_comp);
    mxFree(prn);
    if (rc) {
        mxFree(buf);
        mexErrMsgIdAndTxt("bds:corr_function", "%s", bds_last_error(ctx()));
    }
    /* I, Q: [n_taps * n_comp x n_items], tap fastest: reshape(I, n_taps, n_comp, []) in the wrapper */
    res = mxCreateStructMatrix(1, 1, 0, NULL);
    n = n_taps * (size_t)n_comp;
    pi = out_field(res, "I", (int)n, (int)n_items);
    pq = out_field(res, "Q", (int)n, (int)n_items);
    for (i = 0; i < n * n_items; ++i) pi[i] = buf[2 * i], pq[i] = buf[2 * i + 1];
    mxFree(buf);
    a = mxCreateDoubleMatrix(1, 1, mxREAL);
    mxGetDoubles(a)[0] = (double)n_comp;
    mxAddField(res, "n_comp");
    mxSetField(res, 0, "n_comp", a);
    plhs[0] = res;
}

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
    char cmd[32];
    if (nrhs < 1 || mxGetString(prhs[0], cmd, sizeof(cmd))) mexErrMsgIdAndTxt("bds:args", "first argument: command string");
    if (!strcmp(cmd, "acquire"))
        do_acquire(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "track"))
        do_track(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "gen_code"))
        do_gen_code(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "frame_sync"))
        do_frame_sync(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "nav_decode"))
        do_nav_decode(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "probe_data"))
        do_probe_data(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "blank_pulses"))
        do_blank_pulses(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "notch_tones"))
        do_notch_tones(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "corr_function"))
        do_corr_function(nlhs, plhs, nrhs, prhs);
    else if (!strcmp(cmd, "post_navigation"))
        do_post_navigation(nlhs, plhs, nrhs, prhs);
    else
        mexErrMsgIdAndTxt("bds:args", "unknown command %s", cmd);
}
