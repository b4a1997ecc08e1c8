// Weak-signal acquisition: non-coherent power sums of the coarse search over K code periods (included at the end of
// bds_acq.hip; include/bds_mi355x.h "weak-signal acquisition" has the rules, DESIGN.md 1.8 the derivation and the figures).
//
// Per block k (x[k spc : k spc + N]) the search is the reference's own: D signal spectra once, per PRN the spectrum product +
// inverse row pass (k_rows_inv, bds_acq_kernels.h), then the column pass below, which differs from k_cols_inv_max in what it does
// with a lag: it squares the combined magnitude and adds it into the PRN's D x N surface at the lag moved by the code drift of
// that Doppler bin.  fp32 arithmetic on fp32 storage throughout (no f64 re-evaluation stands behind this surface); the decision
// sums (population mean) and the fine-frequency sums are f64.
#pragma once

namespace bds {

// ---- column pass: inverse columns + |.| combine + square + add into the surface --------------------------------------------------
// grid (tiles, cells); cell g = bin b0 + g of the launch's PRN: Bw[g][comp][L] in, S[g][N] in / out.  Lag l = n1 L2 + col of the
// cell goes to (l + sh[g]) mod N, sh[g] in [0, N).  Every element of the cell's surface row is written by exactly one thread of
// one launch, and launches are ordered on the stream: a plain read-modify-write.  first != 0 (block 0) stores instead of adding,
// so a surface is never zeroed or read before it holds values.
// A tile is T = 2^logT adjacent columns: the T lanes that hold one n1 store T consecutive floats (deep_plan picks T = 16: 64 bytes).
// STORE = false is never instantiated by the library: the probe build of tools/build_deep_probe.sh times the pass without its surface
// traffic (tools/deep_timing.py --probe-lib).
template <int NCOMP, bool STORE = true>
__global__ __launch_bounds__(1024) void k_cols_deep(Plan1D p, int L2, int logT, int Spad, const float2 *__restrict__ Bw, long L, float w0,
                                                    float w1, long N, const int *__restrict__ sh, int first, float *__restrict__ S) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    const int T = 1 << logT;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int tile = (int)xcd_remap(blockIdx.x, gridDim.x);
    const int g = blockIdx.y;
    const int c0 = tile << logT;
    const int S1 = p.S;
    constexpr int MAXE = kPointsPerThread;
    float mag[MAXE];
#pragma unroll
    for (int comp = 0; comp < NCOMP; ++comp) {
        const float2 *src = Bw + ((long)g * NCOMP + comp) * L;
        for (int e = tid; e < (S1 << logT); e += nthr) {
            const int r = e >> logT, j = e & (T - 1);
            const int col = c0 + j;
            float2 v = make_float2(0.f, 0.f);
            if (col < L2) v = src[(long)r * L2 + col];
            lds[j * Spad + lds_phys(r)] = v;
        }
        __syncthreads();
        fft_lds<+1>(lds, p, Spad, T, tid, nthr);
        const float w = comp == 0 ? w0 : w1;
#pragma unroll
        for (int i = 0; i < MAXE; ++i) {
            const int e = tid + i * nthr;
            if (e < (S1 << logT)) {
                const int n1 = e >> logT, j = e & (T - 1);
                const float2 y = lds[j * Spad + lds_phys(n1)];
                const float a = w * sqrtf(y.x * y.x + y.y * y.y);
                mag[i] = comp == 0 ? a : mag[i] + a;
            }
        }
        __syncthreads();
    }
    const long shift = sh[g];
    float *row = S + (long)g * N;
#pragma unroll
    for (int i = 0; i < MAXE; ++i) {
        const int e = tid + i * nthr;
        if (e < (S1 << logT)) {
            const int n1 = e >> logT, j = e & (T - 1);
            const int col = c0 + j;
            const long lag = (long)n1 * L2 + col;
            if (col < L2 && lag < N) {
                long d = lag + shift;
                if (d >= N) d -= N;
                BDS_DASSERT(d >= 0 && d < N);
                const float v = mag[i] * mag[i];
                if constexpr (STORE)
                    row[d] = first ? v : row[d] + v;
                else if (v == -1.f)  // (never true: the arithmetic stays, the traffic goes)
                    row[d] = v;
            }
        }
    }
}

// ---- decision kernels ---------------------------------------------------------------------------------------------------------------
struct DeepPeak {  // of one (PRN, bin, slice): the maximum and the first lag that has it
    float v;
    int lag;
};
// grid (slices, D, PRNs of the group); surface of PRN index pi at S + pi * D * N
__global__ __launch_bounds__(256) void k_deep_peak(const float *__restrict__ S, long N, int D, DeepPeak *__restrict__ out) {
    const int nx = gridDim.x, x = blockIdx.x, b = blockIdx.y, pi = blockIdx.z;
    const long per = (N + nx - 1) / nx, lo = (long)x * per, hi = lo + per < N ? lo + per : N;
    const float *row = S + ((long)pi * D + b) * N;
    float bv = -1.f;
    int bl = -1;
    for (long l = lo + threadIdx.x; l < hi; l += 256) rec_better(bv, bl, row[l], (int)l);
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_down(bv, off, 64);
        const int ol = __shfl_down(bl, off, 64);
        rec_better(bv, bl, ov, ol);
    }
    __shared__ float s_v[4];
    __shared__ int s_l[4];
    if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = bv, s_l[threadIdx.x >> 6] = bl;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) rec_better(bv, bl, s_v[w], s_l[w]);
        out[((long)pi * D + b) * nx + x] = DeepPeak{bv, bl};
    }
}

struct DeepDec {       // per PRN, from the host: where its peak is and the B2a second-peak ranges (0-based, inclusive; empty: lo > hi)
    int l0, fbin;
    int lo1, hi1, lo2, hi2;
};
struct DeepStat {      // of one (PRN, bin, slice)
    double sum;        // of the population's values
    long long count;
    float pmax;        // the population's maximum (-1: none)
    float second;      // maximum over the second-peak ranges, row fbin only (-1: none)
};
// population: lags l with min(d, spc - d) >= s2c, d = (l - l0) mod spc -- the peak and its images one code period away are left out
__global__ __launch_bounds__(256) void k_deep_stats(const float *__restrict__ S, long N, int D, long spc, int s2c,
                                                    const DeepDec *__restrict__ dec, DeepStat *__restrict__ out) {
    const int nx = gridDim.x, x = blockIdx.x, b = blockIdx.y, pi = blockIdx.z;
    const long per = (N + nx - 1) / nx, lo = (long)x * per, hi = lo + per < N ? lo + per : N;
    const float *row = S + ((long)pi * D + b) * N;
    const DeepDec dc = dec[pi];
    double sum = 0;
    long long cnt = 0;
    float pm = -1.f, sec = -1.f;
    for (long l = lo + threadIdx.x; l < hi; l += 256) {
        const float v = row[l];
        long d = (l - dc.l0) % spc;
        if (d < 0) d += spc;
        const long dd = d < spc - d ? d : spc - d;
        if (dd >= s2c) sum += (double)v, ++cnt, pm = fmaxf(pm, v);
        if (b == dc.fbin && ((l >= dc.lo1 && l <= dc.hi1) || (l >= dc.lo2 && l <= dc.hi2))) sec = fmaxf(sec, v);
    }
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off, 64);
        cnt += __shfl_down(cnt, off, 64);
        pm = fmaxf(pm, __shfl_down(pm, off, 64));
        sec = fmaxf(sec, __shfl_down(sec, off, 64));
    }
    __shared__ double s_s[4];
    __shared__ long long s_c[4];
    __shared__ float s_p[4], s_2[4];
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        s_s[w] = sum, s_c[w] = cnt, s_p[w] = pm, s_2[w] = sec;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) sum += s_s[w], cnt += s_c[w], pm = fmaxf(pm, s_p[w]), sec = fmaxf(sec, s_2[w]);
        out[((long)pi * D + b) * nx + x] = DeepStat{sum, cnt, pm, sec};
    }
}

// B1C normaliser of block k (B1C/acquisition.m:150 on x[k spc : k spc + X]): exact integer sums of I, Q and I^2 + Q^2; grid K
__global__ __launch_bounds__(256) void k_deep_sigpow(SampleView sig, long spc, long X, long long *__restrict__ out /*[K][3]*/) {
    const long k = blockIdx.x;
    long long si = 0, sq = 0, ss = 0;
    for (long n = threadIdx.x; n < X; n += 256) {
        const double2 v = sig.load(k * spc + n);
        const long long a = (long long)v.x, c = (long long)v.y;
        si += a, sq += c, ss += a * a + c * c;
    }
    for (int off = 32; off > 0; off >>= 1) {
        si += __shfl_down(si, off, 64);
        sq += __shfl_down(sq, off, 64);
        ss += __shfl_down(ss, off, 64);
    }
    __shared__ long long s_a[4][3];
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        s_a[w][0] = si, s_a[w][1] = sq, s_a[w][2] = ss;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) si += s_a[w][0], sq += s_a[w][1], ss += s_a[w][2];
        out[k * 3] = si, out[k * 3 + 1] = sq, out[k * 3 + 2] = ss;
    }
}

// ---- fine frequency: f64 coherent sums over one code period of every block ----------------------------------------------------------
// grid (frequencies, K): out[(j K + k) NC + c] = sum_{n < spc} x[a_k + n] code_c(n) exp(+j 2 pi f_j n / fs), the phase from n = 0 of
// each block and reduced per sample in f64.  a_k may reach into the zero padding around the record (the view starts pad samples in).
// The sums are added in a fixed order: the same bits on every run.
template <int NC>
__global__ __launch_bounds__(256) void k_deep_fine(SampleView sig, long spc, const long *__restrict__ a_k, const double *__restrict__ freqs,
                                                   double inv_fs, const int8_t *__restrict__ code /*[NC][spc]*/, double2 *__restrict__ out) {
    const int j = blockIdx.x, k = blockIdx.y, K = gridDim.y;
    const double f = freqs[j];
    const long a0 = a_k[k];
    double sr[NC], si[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) sr[c] = si[c] = 0.0;
    for (long n = threadIdx.x; n < spc; n += 256) {
        const double2 x = sig.load(a0 + n);
        const double cyc = f * ((double)n * inv_fs);
        double sn, cs;
        sincospi(2.0 * (cyc - floor(cyc)), &sn, &cs);
        const double yr = x.x * cs - x.y * sn, yi = x.x * sn + x.y * cs;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const double cv = (double)code[(long)c * spc + n];
            sr[c] += yr * cv, si[c] += yi * cv;
        }
    }
    __shared__ double s_p[4][NC * 2];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double vr = corr_wave_sum(sr[c]), vi = corr_wave_sum(si[c]);
        if ((threadIdx.x & 63) == 0) s_p[threadIdx.x >> 6][c * 2] = vr, s_p[threadIdx.x >> 6][c * 2 + 1] = vi;
    }
    __syncthreads();
    if (threadIdx.x < NC) {
        const int c = threadIdx.x;
        double vr = s_p[0][c * 2], vi = s_p[0][c * 2 + 1];
        for (int w = 1; w < 4; ++w) vr += s_p[w][c * 2], vi += s_p[w][c * 2 + 1];
        out[((long)j * K + k) * NC + c] = make_double2(vr, vi);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct DeepPrn {
    double peak = 0, second = 0, mu = 0, sec = 0, sigpow2 = 0;  // S_peak, S_second (B2a), population mean and maximum, sum_k sigPower_k^2 (B1C)
    int fbin = 0;    // 0-based
    long l0 = 0;     // 0-based
    bool detected = false;
    std::vector<double> fine;  // F over the fine grid (detected PRNs)
};

struct DeepState {
    // key of the plan and the code tables
    int signal = 0, pilot = 0;
    double fs = 0, cfb = 0, cohT = 0;
    long spc = 0, X = 0, N = 0, n_ext = 0;
    int ncomp = 0;
    Plan2D plan;
    CodeTable tab{};
    int8_t *d_prim = nullptr;
    // work buffers (kept between calls; bds_acq_deep_release frees them)
    int8_t *d_rec = nullptr;   size_t rec_cap = 0;    // [pad | record | pad] bytes, the pads zero
    float2 *d_Cs = nullptr;    size_t cs_cap = 0;     // [P][ncomp][L] conj(code spectrum) / L
    float2 *d_Xs = nullptr;    size_t xs_cap = 0;     // [bins of a chunk][L]
    float2 *d_Bw = nullptr;    size_t bw_cap = 0;     // [bins of a chunk][ncomp][L]
    float *d_S = nullptr;      size_t s_cap = 0;      // [PRNs of a group][D][N]
    int *d_sh = nullptr;       size_t sh_cap = 0;     // [K][D] shifts in [0, N)
    char *d_dec = nullptr;     size_t dec_cap = 0;    // DeepPeak / DeepStat partials, DeepDec, sigPower sums, fine-search arguments
    int8_t *d_code = nullptr;  size_t code_cap = 0;   // [ncomp][spc] sampled code of the PRN whose fine search runs
    // the last call
    int D = 0, K = 0;
    bool kept = false;         // d_S holds the surfaces of every PRN of `prns`
    std::vector<int> prns;
    std::map<int, DeepPrn> last;
};

void deep_state_free(DeepState *d) {
    if (!d) return;
    plan_free(d->plan);
    for (void *p : {(void *)d->d_prim, (void *)d->d_rec, (void *)d->d_Cs, (void *)d->d_Xs, (void *)d->d_Bw, (void *)d->d_S, (void *)d->d_sh,
                    (void *)d->d_dec, (void *)d->d_code})
        if (p) (void)hipFree(p);
    delete d;
}

#ifdef BDS_DEEP_PROBE_NO_STORE  // tools/build_deep_probe.sh only: results are meaningless
constexpr bool kDeepStore = false;
#else
constexpr bool kDeepStore = true;
#endif
constexpr int kDeepSlices = 32;                 // slices of a surface row in the decision kernels
constexpr double kDeepDefaultGiB = 8.0;         // surface budget when the caller gives none
constexpr size_t kDeepChunkBytes = 1ull << 30;  // inter-pass buffer of one bin chunk

// The tile width of the deep column pass: 16 columns (64-byte store runs) where the LDS and the thread budget allow, else the widest below.
static int deep_plan(bds_ctx *ctx, DeepState &d) {
    Plan2D &pl = d.plan;
    int rc;
    if ((rc = plan_build(ctx, pl, d.n_ext, d.N, false))) return rc;
    int logT = 4;
    while (logT > 0 && ((1 << logT) > pl.L2 || threads_for(pl.p1, 1 << logT) > 1024 ||
                        sizeof(float2) * (size_t)(lds_span(pl.L1) + 4) * (size_t)(1 << logT) > kPlanLdsMax))
        --logT;
    pl.logT = logT;
    pl.Spad = lds_span(pl.L1) + 4;
    pl.ntiles = (pl.L2 + (1 << logT) - 1) >> logT;
    pl.nt_cols = threads_for(pl.p1, 1 << logT);
    pl.lds_cols = sizeof(float2) * (size_t)pl.Spad * (size_t)(1 << logT);
    if (pl.nt_cols > 1024 || pl.lds_cols > kPlanLdsMax || pl.lds_rows > kPlanLdsMax)
        return fail(ctx, BDS_ERR_UNSUPPORTED, "bds_acq_deep: transform %d x %d exceeds the per-workgroup budget", pl.L1, pl.L2);
    return BDS_OK;
}

static int deep_configure(bds_ctx *ctx, const bds_settings &s) {
    if (!ctx->deep) ctx->deep = new DeepState();
    DeepState &d = *ctx->deep;
    const long spc = samples_per_code(s);
    long X, N;
    int ncomp;
    if (s.signal == BDS_SIGNAL_B1C) {
        X = (long)m_round((double)spc / 10 * s.acqCohT);
        N = (long)m_round((double)spc / 10 * (10 + s.acqCohT));
        ncomp = s.pilotACQflag == 1 ? 2 : 1;
    } else {
        X = spc, N = 2 * spc, ncomp = 2;
    }
    if (X < 1 || X > spc || N <= X) return fail(ctx, BDS_ERR_ARG, "degenerate acquisition sizes (spc=%ld X=%ld N=%ld)", spc, X, N);
    if (N > 0x7fffffffL - 8192) return fail(ctx, BDS_ERR_UNSUPPORTED, "bds_acq_deep: block of %ld samples", N);
    const bool same = d.signal == s.signal && d.fs == s.samplingFreq && d.cfb == s.codeFreqBasis && d.cohT == s.acqCohT &&
                      d.pilot == s.pilotACQflag && d.plan.L > 0;
    if (same) return BDS_OK;
    d.plan.L = 0;
    d.kept = false, d.last.clear(), d.prns.clear();
    d.signal = s.signal, d.fs = s.samplingFreq, d.cfb = s.codeFreqBasis, d.cohT = s.acqCohT, d.pilot = s.pilotACQflag;
    d.spc = spc, d.X = X, d.N = N, d.n_ext = N + X - 1, d.ncomp = ncomp;
    if (int rc = deep_plan(ctx, d)) {
        d.plan.L = 0;
        return rc;
    }
    const size_t prim_bytes = (size_t)BDS_MAX_PRN * 2 * 10230;
    if (!d.d_prim) BDS_HIP(ctx, hipMalloc((void **)&d.d_prim, prim_bytes));
    std::vector<int8_t> prim(prim_bytes);
    for (int prn = 1; prn <= BDS_MAX_PRN; ++prn)
        for (int c = 0; c < 2; ++c) gen_primary(s.signal, c == 1, prn, &prim[((size_t)(prn - 1) * 2 + c) * 10230]);
    BDS_HIP(ctx, hipMemcpy(d.d_prim, prim.data(), prim.size(), hipMemcpyHostToDevice));
    d.tab.prim = d.d_prim;
    d.tab.ts = 1.0 / s.samplingFreq;
    d.tab.tc = s.signal == BDS_SIGNAL_B1C ? 1.0 / s.codeFreqBasis / 2 : 1.0 / s.codeFreqBasis;
    d.tab.spc = spc;
    d.tab.xlen = X;
    d.tab.code_len = 10230;
    d.tab.boc = s.signal == BDS_SIGNAL_B1C ? 1 : 0;
    return BDS_OK;
}

// forward transform of nb batches of loader ld on the run-time-plan kernels: dst[b * L] (fp32)
template <class Loader>
static int deep_forward(bds_ctx *ctx, DeepState &d, Loader ld, int nb, float2 *dst, int conj_flag, float scale) {
    const Plan2D &pl = d.plan;
    want_lds(ctx, k_cols_fwd<Loader>, kPlanLdsMax);
    want_lds(ctx, k_rows_fwd, kPlanLdsMax);
    hipLaunchKernelGGL(k_cols_fwd<Loader>, dim3(pl.ntiles, nb), dim3(pl.nt_cols), pl.lds_cols, st(ctx), pl.p1, pl.twl, pl.L2, pl.logT, pl.Spad, ld,
                       d.d_Bw, pl.L);
    hipLaunchKernelGGL(k_rows_fwd, dim3(pl.L1, nb), dim3(pl.nt_rows), pl.lds_rows, st(ctx), pl.p2, (const float2 *)d.d_Bw, pl.L, dst, pl.L,
                       conj_flag, scale);
    BDS_HIP(ctx, hipGetLastError());
    return BDS_OK;
}

// samples or d_samples (one of them NULL) -> the call; everything is checked before anything is launched or written
static int deep_run(bds_ctx *ctx, const bds_settings *s, const int8_t *samples, const void *d_samples, size_t n_samples, int is_complex,
                    const bds_deep_opts *o, int max_prn, double *carrFreq, double *codePhase, double *peakMetric, double *deepMetric,
                    int32_t *fbin, int32_t *detected) {
    if (!ctx) return BDS_ERR_ARG;
    if (!s || !o || (!samples && !d_samples) || !carrFreq || !codePhase || !peakMetric || !deepMetric || !fbin || !detected)
        return fail(ctx, BDS_ERR_ARG, "bds_acq_deep: NULL argument");
    int rc;
    if (s->dataType != 0) return fail(ctx, BDS_ERR_UNSUPPORTED, "bds_acq_deep takes int8 records: settings.dataType 'int16' is not built");
    if (is_complex == 2) return fail(ctx, BDS_ERR_UNSUPPORTED, "bds_acq_deep: packed 2+2-bit I/Q records are not built (unpack first)");
    if (is_complex != 0 && is_complex != 1) return fail(ctx, BDS_ERR_ARG, "bds_acq_deep: is_complex must be 0 (real) or 1 (I/Q int8 pairs)");
    if (s->resamplingflag == 1)
        return fail(ctx, BDS_ERR_UNSUPPORTED, "bds_acq_deep: the resampling pre-conditioner (settings.resamplingflag 1) is not built");
    if ((rc = check_settings(ctx, *s))) return rc;
    if (o->n_blocks < 1 || o->n_blocks > 4096) return fail(ctx, BDS_ERR_ARG, "bds_acq_deep: n_blocks = %d outside 1 .. 4096", (int)o->n_blocks);
    if (!(o->threshold > 1.0) || !std::isfinite(o->threshold))
        return fail(ctx, BDS_ERR_ARG, "bds_acq_deep: threshold = %g; the caller chooses one above 1 (there is no default)", o->threshold);
    if (!(s->carrFreqBasis > 0)) return fail(ctx, BDS_ERR_ARG, "settings.carrFreqBasis must be positive");
    int top = 0;
    for (int i = 0; i < s->n_acq; ++i) top = std::max(top, (int)s->acqSatelliteList[i]);
    if (max_prn < top) return fail(ctx, BDS_ERR_ARG, "bds_acq_deep: the result arrays hold %d PRNs, the list reaches %d", max_prn, top);
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = deep_configure(ctx, *s))) return rc;
    DeepState &d = *ctx->deep;
    const Plan2D &pl = d.plan;
    const int K = o->n_blocks, NC = d.ncomp;
    const long N = d.N, spc = d.spc, L = pl.L;
    if ((long)n_samples < N + (long)K * spc)
        return fail(ctx, BDS_ERR_ARG, "bds_acq_deep: the record has %zu samples, %d blocks need %ld (N + K samplesPerCode)", n_samples, K, N + (long)K * spc);
    const int D = (int)m_round(s->acqSearchBand * 2 / s->acqStep) + 1;
    const double f0 = s->IF - s->acqSearchBand, fstep = s->acqStep;
    std::vector<int> prns;
    for (int i = 0; i < s->n_acq; ++i)
        if (std::find(prns.begin(), prns.end(), (int)s->acqSatelliteList[i]) == prns.end()) prns.push_back((int)s->acqSatelliteList[i]);
    const int P = (int)prns.size();
    // code drift per bin and block in samples (the physical sign: a positive Doppler brings the code starts forward)
    std::vector<long> sh((size_t)K * D, 0);
    long maxsh = 0;
    if (o->compensate)
        for (int k = 0; k < K; ++k)
            for (int b = 0; b < D; ++b) {
                const double frq = f0 + fstep * (double)b;
                const long v = (long)std::nearbyint((double)((long)k * spc) * (frq - s->IF) / s->carrFreqBasis);
                sh[(size_t)k * D + b] = v;
                maxsh = std::max(maxsh, std::labs(v));
            }
    if (maxsh >= spc) return fail(ctx, BDS_ERR_ARG, "bds_acq_deep: the code drifts by %ld samples over %d blocks, more than a code period", maxsh, K);
    // surfaces: all PRNs resident when they fit the budget, else groups of PG
    const double budget = (o->surface_gib > 0 ? o->surface_gib : kDeepDefaultGiB) * 1073741824.0;
    const double per_prn = (double)D * (double)N * 4.0;
    int PG = (int)std::min<double>((double)P, std::floor(budget / per_prn));
    if (PG < 1) PG = 1;
    if (o->keep_surface && PG < P)
        return fail(ctx, BDS_ERR_ARG, "bds_acq_deep: keep_surface needs the surfaces of all %d PRNs resident (%.2f GiB), surface_gib allows %.2f", P,
                    per_prn * P / 1073741824.0, budget / 1073741824.0);
    const int bps = is_complex ? 2 : 1;
    const long pad = maxsh + 64;
    const long n_use = std::min<long>((long)n_samples, N + (long)K * spc + maxsh);
    if (d_samples && (rc = check_device_span(ctx, "bds_acq_deep_dev", "d_samples", d_samples, n_samples * (size_t)bps))) return rc;
    // ---- nothing was written up to here -------------------------------------------------------------------------------------------
    d.kept = false, d.last.clear(), d.prns.clear();
    const int Dc = (int)std::max<size_t>(1, std::min<size_t>((size_t)D, kDeepChunkBytes / (sizeof(float2) * (size_t)L * NC)));
    if ((rc = ensure(ctx, &d.d_rec, &d.rec_cap, (size_t)(n_use + 2 * pad) * bps))) return rc;
    if ((rc = ensure(ctx, &d.d_Cs, &d.cs_cap, (size_t)std::min(P, PG) * NC * L))) return rc;
    if ((rc = ensure(ctx, &d.d_Xs, &d.xs_cap, (size_t)Dc * L))) return rc;
    if ((rc = ensure(ctx, &d.d_Bw, &d.bw_cap, (size_t)std::max(Dc, 1) * NC * L))) return rc;
    if ((rc = ensure(ctx, &d.d_S, &d.s_cap, (size_t)PG * D * N))) return rc;
    if ((rc = ensure(ctx, &d.d_sh, &d.sh_cap, (size_t)K * D))) return rc;
    const int nfine = s->signal == BDS_SIGNAL_B1C ? 2 * (int)m_round(s->acqStep / 25) + 1 : (int)m_round(s->acqStep / 25) + 1;
    const size_t part_n = (size_t)PG * D * kDeepSlices;
    const size_t off_dec = part_n * sizeof(DeepStat), off_sp = off_dec + (size_t)PG * sizeof(DeepDec), off_ak = off_sp + (size_t)K * 3 * sizeof(long long),
                 off_fr = off_ak + (size_t)K * sizeof(long), off_fo = (off_fr + (size_t)nfine * sizeof(double) + 15) & ~(size_t)15,
                 dec_bytes = off_fo + (size_t)nfine * K * NC * sizeof(double2);
    static_assert(sizeof(DeepStat) >= sizeof(DeepPeak), "the partials share one buffer");
    if ((rc = ensure(ctx, &d.d_dec, &d.dec_cap, dec_bytes))) return rc;
    if ((rc = ensure(ctx, &d.d_code, &d.code_cap, (size_t)NC * spc))) return rc;
    hipStream_t q = st(ctx);
    // the record between two zero pads
    BDS_HIP(ctx, hipMemsetAsync(d.d_rec, 0, (size_t)(n_use + 2 * pad) * bps, q));
    BDS_HIP(ctx, hipMemcpyAsync(d.d_rec + pad * bps, samples ? (const void *)samples : d_samples, (size_t)n_use * bps,
                                samples ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, q));
    const int kind = is_complex ? kS8C : kS8;
    {
        std::vector<int> shm(sh.size());
        for (size_t i = 0; i < sh.size(); ++i) shm[i] = (int)(((sh[i] % N) + N) % N);
        BDS_HIP(ctx, hipMemcpyAsync(d.d_sh, shm.data(), sizeof(int) * shm.size(), hipMemcpyHostToDevice, q));
        BDS_HIP(ctx, hipStreamSynchronize(q));  // (shm and, for a host record, the caller's samples have been read)
    }
    float w0 = 1.f, w1 = 1.f;
    if (s->signal == BDS_SIGNAL_B1C && NC == 2) {
        w0 = (float)(std::sqrt(11.0) / std::sqrt(40.0));
        w1 = (float)(std::sqrt(29.0) / std::sqrt(40.0));
    }
    // B1C: sigPower_k^2 = var(x[k spc : k spc + X]) X from exact integer sums
    double sigpow2 = 0;
    if (s->signal == BDS_SIGNAL_B1C) {
        const SampleView v0{d.d_rec + pad * bps, kind, n_use + pad};
        long long *d_sp = (long long *)(d.d_dec + off_sp);
        hipLaunchKernelGGL(k_deep_sigpow, dim3(K), dim3(256), 0, q, v0, spc, d.X, d_sp);
        std::vector<long long> h((size_t)K * 3);
        BDS_HIP(ctx, hipMemcpyAsync(h.data(), d_sp, sizeof(long long) * h.size(), hipMemcpyDeviceToHost, q));
        BDS_HIP(ctx, hipStreamSynchronize(q));
        for (int k = 0; k < K; ++k) {
            const double n = (double)d.X, si = (double)h[(size_t)k * 3], sq = (double)h[(size_t)k * 3 + 1], ss = (double)h[(size_t)k * 3 + 2];
            sigpow2 += (ss - (si * si + sq * sq) / n) / (n - 1) * n;
        }
    }
    want_lds(ctx, k_rows_inv<1>, kPlanLdsMax);
    want_lds(ctx, k_rows_inv<2>, kPlanLdsMax);
    want_lds(ctx, k_cols_deep<1, kDeepStore>, kPlanLdsMax);
    want_lds(ctx, k_cols_deep<2, kDeepStore>, kPlanLdsMax);
    const int s2c = (int)std::ceil(s->samplingFreq / s->codeFreqBasis) * 2;
    std::map<int, DeepPrn> res;
    for (int p0 = 0; p0 < P; p0 += PG) {
        const int np = std::min(PG, P - p0);
        RoctxRange range("bds_acq_deep group");
        for (int pi = 0; pi < np; ++pi) {  // conj(fft([table zeros])) / L per component
            CodeLoader ld{d.tab, (prns[(size_t)(p0 + pi)] - 1) * 2};
            if ((rc = deep_forward(ctx, d, ld, NC, d.d_Cs + (size_t)pi * NC * L, 1, (float)(1.0 / (double)L)))) return rc;
        }
        for (int k = 0; k < K; ++k)
            for (int b0 = 0; b0 < D; b0 += Dc) {
                const int nb = std::min(Dc, D - b0);
                SignalLoader ld{SampleView{d.d_rec + (pad + (long)k * spc) * bps, kind, n_use + pad - (long)k * spc}, N, d.n_ext, f0, fstep,
                                1.0 / s->samplingFreq, b0};
                if ((rc = deep_forward(ctx, d, ld, nb, d.d_Xs, 0, 1.f))) return rc;
                for (int pi = 0; pi < np; ++pi) {
                    const float2 *cs = d.d_Cs + (size_t)pi * NC * L;
                    float *Sp = d.d_S + ((size_t)pi * D + b0) * N;
                    const int *shp = d.d_sh + (size_t)k * D + b0;
                    if (NC == 2) {
                        hipLaunchKernelGGL(k_rows_inv<2>, dim3(pl.L1, nb), dim3(pl.nt_rows), pl.lds_rows, q, pl.p2, pl.twl, (const float2 *)d.d_Xs, L, 0, cs, d.d_Bw);
                        hipLaunchKernelGGL((k_cols_deep<2, kDeepStore>), dim3(pl.ntiles, nb), dim3(pl.nt_cols), pl.lds_cols, q, pl.p1, pl.L2, pl.logT, pl.Spad,
                                           (const float2 *)d.d_Bw, L, w0, w1, N, shp, k == 0 ? 1 : 0, Sp);
                    } else {
                        hipLaunchKernelGGL(k_rows_inv<1>, dim3(pl.L1, nb), dim3(pl.nt_rows), pl.lds_rows, q, pl.p2, pl.twl, (const float2 *)d.d_Xs, L, 0, cs, d.d_Bw);
                        hipLaunchKernelGGL((k_cols_deep<1, kDeepStore>), dim3(pl.ntiles, nb), dim3(pl.nt_cols), pl.lds_cols, q, pl.p1, pl.L2, pl.logT, pl.Spad,
                                           (const float2 *)d.d_Bw, L, w0, w1, N, shp, k == 0 ? 1 : 0, Sp);
                    }
                }
                BDS_HIP(ctx, hipGetLastError());
            }
        // ---- decisions of the group: peak cell, then the statistics around it ----------------------------------------------------------
        const size_t npart = (size_t)np * D * kDeepSlices;
        std::vector<DeepPeak> hp(npart);
        hipLaunchKernelGGL(k_deep_peak, dim3(kDeepSlices, D, np), dim3(256), 0, q, (const float *)d.d_S, N, D, (DeepPeak *)d.d_dec);
        BDS_HIP(ctx, hipMemcpyAsync(hp.data(), d.d_dec, sizeof(DeepPeak) * npart, hipMemcpyDeviceToHost, q));
        BDS_HIP(ctx, hipStreamSynchronize(q));
        std::vector<DeepDec> hd((size_t)np);
        for (int pi = 0; pi < np; ++pi) {
            DeepPrn r;
            float best = -1.f;
            int bb = 0, l0 = -1;
            for (int b = 0; b < D; ++b)
                for (int x = 0; x < kDeepSlices; ++x) {
                    const DeepPeak &e = hp[((size_t)pi * D + b) * kDeepSlices + x];
                    if (e.lag < 0) continue;
                    if (e.v > best) best = e.v, bb = b, l0 = e.lag;  // first bin whose row maximum is largest ...
                    else if (e.v == best && e.lag < l0) l0 = e.lag;  // ... first lag whose column maximum is largest
                }
            r.peak = best, r.fbin = bb, r.l0 = l0, r.sigpow2 = sigpow2;
            const long cp = (long)l0 + 1;  // B2a/acquisition.m:224-246, 1-based
            const long e1 = cp - s2c, e2 = cp + s2c, e3 = cp - spc + s2c, e4 = cp + spc - s2c;
            DeepDec dc{l0, bb, 0, -1, 0, -1};
            if (s->signal == BDS_SIGNAL_B2A) {
                if (e1 >= 1) dc.lo1 = (int)(std::max<long>(1, e3) - 1), dc.hi1 = (int)(e1 - 1);
                if (e2 < N) dc.lo2 = (int)(e2 - 1), dc.hi2 = (int)(std::min<long>(e4, N) - 1);
            }
            hd[(size_t)pi] = dc;
            res[prns[(size_t)(p0 + pi)]] = r;
        }
        BDS_HIP(ctx, hipMemcpyAsync(d.d_dec + off_dec, hd.data(), sizeof(DeepDec) * hd.size(), hipMemcpyHostToDevice, q));
        hipLaunchKernelGGL(k_deep_stats, dim3(kDeepSlices, D, np), dim3(256), 0, q, (const float *)d.d_S, N, D, spc, s2c,
                           (const DeepDec *)(d.d_dec + off_dec), (DeepStat *)d.d_dec);
        std::vector<DeepStat> hs(npart);
        BDS_HIP(ctx, hipMemcpyAsync(hs.data(), d.d_dec, sizeof(DeepStat) * npart, hipMemcpyDeviceToHost, q));
        BDS_HIP(ctx, hipStreamSynchronize(q));
        for (int pi = 0; pi < np; ++pi) {
            DeepPrn &r = res[prns[(size_t)(p0 + pi)]];
            double sum = 0;
            long long cnt = 0;
            float pm = -1.f, sec = -1.f;
            for (size_t i = 0; i < (size_t)D * kDeepSlices; ++i) {  // in order: the same sum on every run
                const DeepStat &e = hs[(size_t)pi * D * kDeepSlices + i];
                sum += e.sum, cnt += e.count, pm = std::max(pm, e.pmax), sec = std::max(sec, e.second);
            }
            r.mu = cnt > 0 ? sum / (double)cnt : 0.0;
            r.sec = pm, r.second = sec;
            const double dm = (r.peak - r.mu) / (r.sec - r.mu);
            r.detected = cnt > 0 && dm > o->threshold;
            if (!r.detected) continue;
            // ---- fine frequency of a detected PRN, while its surface group is here -----------------------------------------------------
            const int prn = prns[(size_t)(p0 + pi)];
            CodeTable full = d.tab;
            full.xlen = spc;  // the whole one-period table
            for (int c = 0; c < NC; ++c)
                hipLaunchKernelGGL(k_make_code, dim3(256), dim3(256), 0, q, full, (prn - 1) * 2 + c, 0, spc, d.d_code + (size_t)c * spc);
            std::vector<long> ak((size_t)K);
            std::vector<double> fr((size_t)nfine);
            for (int k = 0; k < K; ++k) ak[(size_t)k] = pad + r.l0 + (long)k * spc - sh[(size_t)k * D + r.fbin];  // (from the front pad's first byte: never negative)
            const double fb = f0 + fstep * (double)r.fbin;
            for (int j = 0; j < nfine; ++j)
                fr[(size_t)j] = s->signal == BDS_SIGNAL_B1C ? fb - s->acqStep + 25.0 * j : fb - s->acqStep / 2 + 25.0 * j;
            BDS_HIP(ctx, hipMemcpyAsync(d.d_dec + off_ak, ak.data(), sizeof(long) * ak.size(), hipMemcpyHostToDevice, q));
            BDS_HIP(ctx, hipMemcpyAsync(d.d_dec + off_fr, fr.data(), sizeof(double) * fr.size(), hipMemcpyHostToDevice, q));
            const SampleView v0{d.d_rec, kind, n_use + 2 * pad};
            if (NC == 2)
                hipLaunchKernelGGL(k_deep_fine<2>, dim3(nfine, K), dim3(256), 0, q, v0, spc, (const long *)(d.d_dec + off_ak),
                                   (const double *)(d.d_dec + off_fr), 1.0 / s->samplingFreq, (const int8_t *)d.d_code, (double2 *)(d.d_dec + off_fo));
            else
                hipLaunchKernelGGL(k_deep_fine<1>, dim3(nfine, K), dim3(256), 0, q, v0, spc, (const long *)(d.d_dec + off_ak),
                                   (const double *)(d.d_dec + off_fr), 1.0 / s->samplingFreq, (const int8_t *)d.d_code, (double2 *)(d.d_dec + off_fo));
            BDS_HIP(ctx, hipGetLastError());
            std::vector<double2> fo((size_t)nfine * K * NC);
            BDS_HIP(ctx, hipMemcpyAsync(fo.data(), d.d_dec + off_fo, sizeof(double2) * fo.size(), hipMemcpyDeviceToHost, q));
            BDS_HIP(ctx, hipStreamSynchronize(q));
            const double wd = s->signal == BDS_SIGNAL_B2A ? 1.0 : NC == 2 ? 11.0 / 40.0 : 1.0, wp = s->signal == BDS_SIGNAL_B2A ? 1.0 : 29.0 / 40.0;
            r.fine.assign((size_t)nfine, 0.0);
            for (int j = 0; j < nfine; ++j)
                for (int k = 0; k < K; ++k) {
                    const double2 *v = &fo[((size_t)j * K + k) * NC];
                    const double m = wd * cabs2(v[0]) + (NC == 2 ? wp * cabs2(v[1]) : 0.0);
                    r.fine[(size_t)j] += m * m;
                }
        }
    }
    // ---- results ----------------------------------------------------------------------------------------------------------------------
    for (int i = 0; i < max_prn; ++i) carrFreq[i] = codePhase[i] = peakMetric[i] = deepMetric[i] = 0, fbin[i] = detected[i] = 0;
    for (auto &kv : res) {
        const DeepPrn &r = kv.second;
        const int i = kv.first - 1;
        peakMetric[i] = std::sqrt(r.peak / (s->signal == BDS_SIGNAL_B2A ? r.second : r.sigpow2));
        deepMetric[i] = (r.peak - r.mu) / (r.sec - r.mu);
        fbin[i] = r.fbin + 1;
        detected[i] = r.detected ? 1 : 0;
        if (!r.detected) continue;
        const int nf = (int)r.fine.size();
        int jm = 0;
        for (int j = 1; j < nf; ++j)
            if (r.fine[(size_t)j] > r.fine[(size_t)jm]) jm = j;
        const double fb = f0 + fstep * (double)r.fbin;
        double cf = s->signal == BDS_SIGNAL_B1C ? fb - s->acqStep + 25.0 * jm : fb - s->acqStep / 2 + 25.0 * jm;
        if (cf == 0) cf = 1;
        carrFreq[i] = cf;
        codePhase[i] = (double)(r.l0 + 1);
    }
    d.D = D, d.K = K, d.prns = prns, d.last = res;
    d.kept = o->keep_surface != 0;
    if (!d.kept && d.d_S) (void)hipFree(d.d_S), d.d_S = nullptr, d.s_cap = 0;  // the large one goes back at once
    return BDS_OK;
}

}  // namespace bds

extern "C" int bds_acq_deep(bds_ctx *ctx, const bds_settings *s, const int8_t *samples, size_t n_samples, int is_complex,
                            const bds_deep_opts *opts, int max_prn, double *carrFreq, double *codePhase, double *peakMetric,
                            double *deepMetric, int32_t *fbin, int32_t *detected) {
    if (ctx && !samples) return bds::fail(ctx, BDS_ERR_ARG, "bds_acq_deep: samples is NULL");
    return bds::deep_run(ctx, s, samples, nullptr, n_samples, is_complex, opts, max_prn, carrFreq, codePhase, peakMetric, deepMetric, fbin, detected);
}

extern "C" int bds_acq_deep_dev(bds_ctx *ctx, const bds_settings *s, const void *d_samples, size_t n_samples, int is_complex,
                                const bds_deep_opts *opts, int max_prn, double *carrFreq, double *codePhase, double *peakMetric,
                                double *deepMetric, int32_t *fbin, int32_t *detected) {
    if (ctx && !d_samples) return bds::fail(ctx, BDS_ERR_ARG, "bds_acq_deep_dev: d_samples is NULL");
    return bds::deep_run(ctx, s, nullptr, d_samples, n_samples, is_complex, opts, max_prn, carrFreq, codePhase, peakMetric, deepMetric, fbin, detected);
}

extern "C" int bds_acq_deep_row(bds_ctx *ctx, int prn, int bin, float *row, int64_t cap) {
    if (!ctx) return BDS_ERR_ARG;
    bds::DeepState *d = ctx->deep;
    if (!d || !d->kept || !d->d_S) return bds::fail(ctx, BDS_ERR_ARG, "bds_acq_deep_row: no surface is kept (bds_acq_deep with keep_surface first)");
    const auto it = std::find(d->prns.begin(), d->prns.end(), prn);
    if (it == d->prns.end() || bin < 1 || bin > d->D) return bds::fail(ctx, BDS_ERR_ARG, "bds_acq_deep_row: PRN %d, bin %d is not in the last call's grid", prn, bin);
    if (!row || cap < (int64_t)d->N) return bds::fail(ctx, BDS_ERR_ARG, "bds_acq_deep_row: row holds %lld values, a row has %ld", (long long)cap, d->N);
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pi = (size_t)(it - d->prns.begin());
    BDS_HIP(ctx, hipMemcpyAsync(row, d->d_S + (pi * (size_t)d->D + (size_t)(bin - 1)) * (size_t)d->N, sizeof(float) * (size_t)d->N, hipMemcpyDeviceToHost,
                                bds::st(ctx)));
    BDS_HIP(ctx, hipStreamSynchronize(bds::st(ctx)));
    return (int)d->N;
}

extern "C" int bds_acq_deep_fine(bds_ctx *ctx, int prn, double *F, int cap) {
    if (!ctx) return BDS_ERR_ARG;
    bds::DeepState *d = ctx->deep;
    if (!d) return bds::fail(ctx, BDS_ERR_ARG, "bds_acq_deep_fine: no call yet");
    const auto it = d->last.find(prn);
    if (it == d->last.end()) return bds::fail(ctx, BDS_ERR_ARG, "bds_acq_deep_fine: PRN %d was not searched by the last call", prn);
    const int n = (int)it->second.fine.size();
    if (n > cap || (n && !F)) return bds::fail(ctx, BDS_ERR_ARG, "bds_acq_deep_fine: F holds %d values, the grid has %d", cap, n);
    for (int j = 0; j < n; ++j) F[j] = it->second.fine[(size_t)j];
    return n;
}

extern "C" int bds_acq_deep_release(bds_ctx *ctx) {
    if (!ctx) return BDS_ERR_ARG;
    if (ctx->deep) {
        (void)hipSetDevice(ctx->device);
        if (ctx->stream) (void)hipStreamSynchronize((hipStream_t)ctx->stream);
        bds::deep_state_free(ctx->deep);
        ctx->deep = nullptr;
    }
    return BDS_OK;
}
