// Acquisition: host orchestration of the PRN x Doppler parallel code-phase search.
//
// Replaces BDS-3_B2a/acquisition.m:126-336 and BDS-3_B1C/acquisition.m:125-307 (and
// B1C/GPU_acquisition.m, which is the same algorithm on gpuArray built-ins).
//
// How the search is organised here (DESIGN.md has the full derivation):
//  * The reference's circular correlation of length N (2 code periods, code zero beyond
//    X samples) is evaluated as a linear correlation of the code with the periodic
//    extension of the wiped-off block, zero padded to a 5-smooth length
//    L >= N + X - 1 -- identical lag for lag, and L has no factor 53 (N = 2^2 3 5^5 53 at
//    99.375 MS/s).
//  * Forward transforms run once per Doppler bin (the reference redoes them per PRN),
//    code spectra once per PRN and are cached in the context.
//  * Per (PRN, bin) cell: one row-pass kernel (spectrum product + inverse rows) and one
//    column-pass kernel (inverse columns + |.| combine + max/argmax).  The D x N
//    results matrix is never materialised.
//  * fp32 is only a sieve: every cell within 2e-5 of a PRN's fp32 maximum (plus its
//    +-1 bin / +-1 lag neighbours) is re-evaluated in f64 by direct time-domain
//    correlation; peakSize, secondPeakSize, the fine-Doppler sums, sigPower and the
//    DC mean are all f64 / exact-integer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <functional>
#include <map>
#include <queue>
#include <set>
#include <tuple>

#include "bds_acq_sieve.h"
#include "bds_acq_scols.h"
#include "bds_acq_wcols.h"
#include "bds_acq_refine.h"
#include "bds_acq_wrows.h"
#include "bds_acq_pfa.h"
#include "bds_acq_pfa32.h"
#include "bds_acq_pfa6.h"
#include "bds_acq_pfa31.h"
#include "bds_internal.h"

namespace bds {

static const double kPi = 3.14159265358979323846;

#include "bds_acq_plan.h"  // Plan2D, choose_lengths, plan_build, the kernels' constant tables

// ---------------------------------------------------------------------------------------
// Events of a run, kept in the context across runs (a run records ~100 of them -- the timing triples of the sampled launch
// pairs -- and creating / destroying them was host time of every call): make() hands out the next one of its kind, rewind()
// starts over.
struct EventPool {
    std::vector<hipEvent_t> timed, untimed;
    size_t nt = 0, nu = 0;
    void rewind() { nt = nu = 0; }
    hipError_t make(hipEvent_t *e, unsigned flags = 0) {
        std::vector<hipEvent_t> &v = flags ? untimed : timed;
        size_t &n = flags ? nu : nt;
        if (n == v.size()) {
            hipEvent_t ne;
            const hipError_t rc_ = flags ? hipEventCreateWithFlags(&ne, flags) : hipEventCreate(&ne);
            if (rc_ != hipSuccess) return rc_;
            v.push_back(ne);
        }
        *e = v[n++];
        return hipSuccess;
    }
    ~EventPool() {
        for (hipEvent_t e : timed) (void)hipEventDestroy(e);
        for (hipEvent_t e : untimed) (void)hipEventDestroy(e);
    }
};

struct PrnResult {
    double peak = 0, denom = 0;
    int fbin = 0;  // 1-based
    long codePhase = 0;
    bool detected = false;
};

struct AcqState {
    // key of everything cached below
    int signal = 0, pilotACQ = 0, code_len = 0;
    double fs = 0, cfb = 0, cohT = 0;
    long spc = 0, X = 0, N = 0, n_ext = 0;
    int ncomp = 0;
    Plan2D plan;
    CodeTable tab{};   // xlen = X (coarse)
    // device buffers
    int8_t *d_sig = nullptr;        // int8 record as loaded (pairs when complex)
    size_t sig_cap = 0;
    uint8_t *d_packed = nullptr;    // packed bytes of a fileType-3 block, before they are unpacked into d_sig
    size_t packed_cap = 0;
    double *d_sig64 = nullptr;      // conditioned f64 block of the resampling branch (acquisition.m:56-124)
    size_t sig64_cap = 0;
    double *d_ffa = nullptr, *d_ffb = nullptr, *d_fir = nullptr;  // filtfilt work buffers, fir1 taps
    size_t ffa_cap = 0, ffb_cap = 0, fir_cap = 0;
    int skind = kS8;                // what the search reads: SampleKind
    bool w16 = false;               // the block was loaded as int16 samples (settings.dataType 1): d_sig holds its bytes, the search reads d_sig64
    long n_samples = 0;             // samples of the block the search sees (after resampling, if any)
    ResamplePlan rs;                // resampling branch of the loaded block
    // Host view of that block.  An int8 record is kept as the bytes it came in (interleaved I/Q for a complex one) with its
    // prefix sums at every 256th sample (round 5: the f64 copies and full-length prefix arrays of rounds 1-4 were 320 MB of host
    // writes per bds_acq_load at cfg3, 79 of the 291 ms of a cold call); the f64 block of the resampling branch keeps full arrays.
    std::vector<int8_t> h_s8;
    std::vector<double> h_cpre, h_cpre_q; // prefix sums of I (and Q) at samples 0, 256, 512, ... (exact integers below 2^53)
    std::vector<double> h_re, h_im;       // resampling branch only: the conditioned block
    std::vector<double> h_prefix;         // ... its prefix sums
    std::vector<double> h_prefix_q;       // ... of the imaginary part
    bool cplx = false;              // longSignal = I + 1i*Q (postProcessing.m:92-96)
    EventPool events;               // timing / ordering events of a run, re-used across runs
    double sample_re(long i) const { return skind >= kF64 ? h_re[(size_t)i] : (double)h_s8[(size_t)(cplx ? 2 * i : i)]; }
    double sample_im(long i) const { return !cplx ? 0.0 : skind >= kF64 ? h_im[(size_t)i] : (double)h_s8[(size_t)(2 * i + 1)]; }
    // sum of the first i samples (I part / Q part): for an int8 record the same integer, hence the same f64, in any order of adding
    double prefix(long i, int q = 0) const {
        if (skind >= kF64) return q ? h_prefix_q[(size_t)i] : h_prefix[(size_t)i];
        long acc = 0;
        const int8_t *b = h_s8.data();
        for (long m = (i >> 8) << 8; m < i; ++m) acc += cplx ? b[2 * m + q] : b[m];
        return (q ? h_cpre_q : h_cpre)[(size_t)(i >> 8)] + (double)acc;
    }
    SampleView sview() const { return SampleView{skind >= kF64 ? (const void *)d_sig64 : (const void *)d_sig, skind, n_samples}; }
    int8_t *d_prim = nullptr;       // [63][2][code_len]
    float2 *d_Cs = nullptr;         // [slots][ncomp][L]
    size_t cs_cap_slots = 0;
    std::map<int, int> cs_slot;     // PRN -> slot
    float2 *d_Xs = nullptr;
    size_t xs_cap = 0;  // elements
    float2 *d_Bw = nullptr;
    size_t bw_cap = 0;  // elements
    Rec *d_recs = nullptr;
    size_t recs_cap = 0;
    float *d_rowmax = nullptr;
    int *d_rowarg = nullptr;
    size_t rows_cap = 0;
    int8_t *d_codes = nullptr;       // sampled codes [slot*2 + mode][code_stride] for the f64 sums
    long code_stride = 0;
    std::vector<char> code_have;     // which (slot, mode) tables exist
    char *d_cells = nullptr;         // cell list of the batched second-peak launch
    size_t cells_cap = 0;
    double pair_gb = 0;              // bds_acq_set_pair_budget_gb (overrides the BDS_ACQ_PAIR_GB of the context's tuning)
    bool pair_gb_set = false;
    bool b2a_npoint = false;         // bds_acq_set_b2a_npoint: the N-point pair of bds_acq_pfa6.h may run (default off)
    bool b1c_npoint = false;         // bds_acq_set_b1c_npoint: the N-point pair of bds_acq_pfa31.h may run (default off)
    int pb_last = 0;                 // PRNs per launch pair the last run settled on, and what it was decided for: the next run with
    double pb_key[6] = {0};          // the same (P, D, L, element size, components, budget) takes it without asking the driver again
    char *d_mcells = nullptr;        // cell list of the main search of a small grid (all P x D cells in a few launch pairs) ...
    size_t mcells_cap = 0;
    std::vector<long> mcells_cs;     // ... and what it holds: uploaded again only when a run's list differs
    std::vector<int> mcells_bin;
    struct RowsChunks {              // chunk list of a launch pair of the N-point row pass (rows_chunk_plan), planned once per shape
        int nchunks = 0;
        int2 *d = nullptr;
    };
    std::map<std::tuple<int, int, int>, RowsChunks> rows_chunks;  // (PRNs of the pair, D, slots) -> its list on the device
    std::vector<long> ref_tabs_cs;   // what d_ref_tabs holds (refinement chain: code-spectrum offset and PRN of every searched PRN)
    std::vector<int> ref_tabs_prn;
    Extra *d_extra = nullptr;        // overflow list of the column pass (bds_acq_sieve.h)
    size_t extra_cap = 0;
    int *d_extra_count = nullptr;
    int n_extra_last = 0;            // entries of the last search (diagnostics)
    unsigned long long *d_cellmax = nullptr;  // wave-private column pass: packed {maximum, first lag} per cell ...
    size_t cellmax_cap = 0;
    float *d_lb = nullptr;                    // ... and the running lower bound of each PRN's sieve maximum
    size_t lb_cap = 0;
    std::map<int, std::vector<std::pair<int, long>>> last_cands;  // PRN -> (bin, lag) cells the last run refined in f64
    bool no_fast_search = false;     // this configuration fell back to the run-time-plan search kernels
    bool no_small = false;           // this configuration's 80 x 4096 plan fell back to fp32 storage: re-planned without it
    bool fell_back = false;          // a run of this configuration was redone with fp32 storage / on the run-time-plan kernels: the NEXT
                                     // block (bds_acq_load) starts on the default path again (round 6; until then the fallback stayed for
                                     // as long as the configuration did -- one pathological block made every later one ten times slower)
    CorrJob *d_jobs = nullptr;
    double2 *d_jobout = nullptr;
    size_t jobs_cap = 0;
    // device refinement chain (bds_acq_refine.h)
    char *d_ref_zero = nullptr;         // one block, zeroed per run: RefGlobal | RefPrn[P] | cellmax2[P] | lb2[P] | extra2_count
    size_t ref_zero_cap = 0;
    RefPrn *d_ref_prn = nullptr;        // (pointers into d_ref_zero)
    RefGlobal *d_ref_g = nullptr;
    RefCand *d_ref_cand = nullptr;      // [kRefCandCap] coarse candidates, then [kRefCandCap] of the second-peak pass
    size_t ref_cand_cap = 0;
    char *d_ref_tabs = nullptr;         // per run: PRN of index pi (int), code-spectrum offset of index pi (long)
    size_t ref_tabs_cap = 0;
    double *d_prefix_c = nullptr, *d_prefix_cq = nullptr;  // prefix sums of the block at every 256th sample (exact integers: int8 data)
    size_t prefix_c_cap = 0, prefix_cq_cap = 0;
    Extra *d_extra2 = nullptr;          // candidate list / per-PRN maxima / bounds of the B2a second-peak pass
    size_t extra2_cap = 0;
    int *d_extra2_count = nullptr;      // (these three: pointers into d_ref_zero)
    unsigned long long *d_cellmax2 = nullptr;
    float *d_lb2 = nullptr;
    int cands_on_device = 0;            // >0: last_cands of the last run still sits in d_ref_cand (fetched on demand)
    std::vector<int> cands_prns;
    // last run (diagnostics)
    int D = 0;
    std::vector<int> run_prns;
    std::vector<float> h_rowmax;
    std::vector<int> h_rowarg;
    std::map<int, PrnResult> last;
    // (PRN, bin) cells per launch pair; 0 = all Doppler bins of the PRN that fit the work-buffer budget.
    // Measured on the B1C plan (us/cell): 1 -> 41, 4 -> 25, 16 -> 21 without the row-pass cell loop;
    // with it 16 -> 17.5, 48 -> 16.5, 201 -> 15.9 (HISTORY.md 1.4)
    int group_env = 0;
    int group = 16;
    bool half = false;         // spectra + inter-pass buffer stored as fp16 complex (specialised plans only)
    double sum_abs_ext = 0;    // sum |x| over the periodically extended block: bound of |X[k]|
    double sum_sq_ext = 0;     // sum x^2 over it: X_rms^2 (Parseval)
    long sums_N = 0, sums_next = 0;  // sizes the two sums above were computed for
    float sX = 1.f, sC = 1.f, sB = 1.f;  // power-of-two storage scales
    // N-point plan (bds_acq_pfa.h: 1, bds_acq_pfa32.h: 2, bds_acq_pfa6.h: 3, bds_acq_pfa31.h: 4; 0: none): the cached code spectra are in its layout (CRT order), the search
    // runs its pair
    int cs_pfa = 0;
    std::map<void (*)(uint16_t *), uint4 *> pfa_coef;  // B fragments of the column passes' first stage: one table per Plan::make_coef_frags
    long sigpower_X = 0;       // X the cached B1C normaliser was computed for (0: none; reset by bds_acq_load)
    double sigpower = 0;       // sqrt(var(sig(1:X)) * X), B1C/acquisition.m:150
};

void acq_state_free(AcqState *a) {
    if (!a) return;
    plan_free(a->plan);
    for (void *p : {(void *)a->d_sig, (void *)a->d_packed, (void *)a->d_prim, (void *)a->d_Cs, (void *)a->d_Xs, (void *)a->d_Bw,
                    (void *)a->d_recs, (void *)a->d_rowmax, (void *)a->d_rowarg, (void *)a->d_jobs, (void *)a->d_codes,
                    (void *)a->d_jobout, (void *)a->d_sig64, (void *)a->d_ffa, (void *)a->d_ffb, (void *)a->d_fir, (void *)a->d_cells, (void *)a->d_mcells,
                    (void *)a->d_extra, (void *)a->d_extra_count, (void *)a->d_cellmax, (void *)a->d_lb, (void *)a->d_ref_zero,
                    (void *)a->d_ref_cand, (void *)a->d_ref_tabs, (void *)a->d_prefix_c, (void *)a->d_prefix_cq, (void *)a->d_extra2})
        if (p) (void)hipFree(p);
    for (auto &rc : a->rows_chunks)
        if (rc.second.d) (void)hipFree(rc.second.d);
    for (auto &cf : a->pfa_coef)
        if (cf.second) (void)hipFree(cf.second);
    delete a;
}

// After the tuning knobs changed: the plan, the storage mode and the kernels of the search (kernel_pick(), hence the element order of
// the cached spectra) all depend on them, so the next bds_acq_prepare re-derives everything.  The loaded IF block stays.
void acq_state_invalidate(AcqState *a) {
    if (a) a->plan.L = 0;
}

static int check_settings(bds_ctx *ctx, const bds_settings &s) {
    if (s.signal != BDS_SIGNAL_B1C && s.signal != BDS_SIGNAL_B2A)
        return fail(ctx, BDS_ERR_ARG, "settings.signal must be 1 (B1C) or 2 (B2a)");
    if (s.dataType != 0 && s.dataType != 1)
        return fail(ctx, BDS_ERR_UNSUPPORTED, "settings.dataType: only 'schar' (0: int8 samples) and 'int16' (1) are supported");
    if (!(s.samplingFreq > 0) || !(s.codeFreqBasis > 0) || s.codeLength != 10230)
        return fail(ctx, BDS_ERR_ARG, "settings.samplingFreq/codeFreqBasis must be positive and codeLength 10230");
    if (!(s.acqStep > 0) || !(s.acqSearchBand >= 0))
        return fail(ctx, BDS_ERR_ARG, "settings.acqStep must be > 0 and acqSearchBand >= 0");
    if (s.resamplingflag == 1 && s.samplingFreq > s.resamplingThreshold) {
        const ResamplePlan r = resample_plan(s);
        if (!(r.wp1 > 0 && r.wp2 < 1 && r.wp1 < r.wp2))
            return fail(ctx, BDS_ERR_ARG, "resampling band edges [%g %g] outside (0, 1): fir1 would fail (acquisition.m:66-68)", r.wp1, r.wp2);
    }
    if (s.n_acq < 1 || s.n_acq > BDS_MAX_PRN) return fail(ctx, BDS_ERR_ARG, "settings.acqSatelliteList is empty or too long");
    for (int i = 0; i < s.n_acq; ++i)
        if (s.acqSatelliteList[i] < 1 || s.acqSatelliteList[i] > BDS_MAX_PRN)
            return fail(ctx, BDS_ERR_ARG, "settings.acqSatelliteList[%d] = %d out of 1..63", i, s.acqSatelliteList[i]);
    if (s.signal == BDS_SIGNAL_B1C && !(s.acqCohT > 0 && s.acqCohT <= 10))
        return fail(ctx, BDS_ERR_ARG, "settings.acqCohT must be in (0, 10] ms");
    if (s.signal == BDS_SIGNAL_B2A && s.fineNoncoh < 1)
        return fail(ctx, BDS_ERR_ARG, "settings.fineNoncoh must be >= 1");
    return BDS_OK;
}

template <class T>
static int ensure(bds_ctx *ctx, T **p, size_t *cap, size_t need) {
    if (*cap >= need && *p) return BDS_OK;
    if (*p) (void)hipFree(*p), *p = nullptr, *cap = 0;
    hipError_t e = hipMalloc((void **)p, sizeof(T) * need);
    if (e != hipSuccess)
        return fail(ctx, BDS_ERR_NOMEM, "hipMalloc of %zu bytes failed: %s", sizeof(T) * need, hipGetErrorString(e));
    *cap = need;
    return BDS_OK;
}

// The inter-pass buffer also SHRINKS (round 6): a context that ran with a larger budget (serving mode: 150 GiB) and is
// then given a smaller one -- bds_acq_set_pair_budget_gb(ctx, 0), a lower BDS_ACQ_PAIR_GB -- returns the difference at its next
// search instead of holding it until bds_destroy.  Called where a run knows its final need (search()); the other ensure() sites
// only grow.  A quarter of slack (+256 MiB) is tolerated so that neighbouring settings do not reallocate back and forth.
template <class T>
static int ensure_fit(bds_ctx *ctx, T **p, size_t *cap, size_t need) {
    if (*p && *cap >= need && (double)*cap * sizeof(T) > 1.25 * (double)need * sizeof(T) + 268435456.0) {
        (void)hipFree(*p), *p = nullptr, *cap = 0;
    }
    return ensure(ctx, p, cap, need);
}

// (Re)derive sizes, plan and code tables when the settings that define them change.
static int acq_configure(bds_ctx *ctx, const bds_settings &s) {
    int rc = check_settings(ctx, s);
    if (rc) return rc;
    if (!ctx->acq) ctx->acq = new AcqState();
    AcqState &a = *ctx->acq;
    const long spc = samples_per_code(s);
    long X, N;
    int ncomp;
    if (s.signal == BDS_SIGNAL_B1C) {
        X = (long)m_round((double)spc / 10 * s.acqCohT);         // samplesXmsLen  B1C/acquisition.m:132
        N = (long)m_round((double)spc / 10 * (10 + s.acqCohT));  // len10PlusXms   :135
        ncomp = s.pilotACQflag == 1 ? 2 : 1;
    } else {
        X = spc;      // B2a/acquisition.m:179-180
        N = 2 * spc;  // len2ms :134
        ncomp = 2;
    }
    if (X < 1 || X > spc || N <= X) return fail(ctx, BDS_ERR_ARG, "degenerate acquisition sizes (spc=%ld X=%ld N=%ld)", spc, X, N);
    const bool same_key = a.signal == s.signal && a.fs == s.samplingFreq && a.cfb == s.codeFreqBasis &&
                          a.cohT == s.acqCohT && a.pilotACQ == s.pilotACQflag && a.code_len == s.codeLength;
    if (same_key && a.plan.L > 0) return BDS_OK;
    if (!same_key) a.no_small = false;  // (set by the fp32-storage fallback of an 80 x 4096 plan, which re-plans with plan.L = 0)
    a.no_fast_search = false;
    a.code_have.clear();  // sampled-code cache: same key
    a.cs_slot.clear();  // the spectra cache is keyed by everything above: drop it (slot size depends on L)
    if (a.d_Cs) (void)hipFree(a.d_Cs), a.d_Cs = nullptr;
    a.cs_cap_slots = 0;
    a.signal = s.signal;
    a.fs = s.samplingFreq;
    a.cfb = s.codeFreqBasis;
    a.cohT = s.acqCohT;
    a.pilotACQ = s.pilotACQflag;
    a.code_len = s.codeLength;
    a.spc = spc;
    a.X = X;
    a.N = N;
    a.n_ext = N + X - 1;
    a.ncomp = ncomp;
    // (the 80 x 4096 plan: two components, fp16 storage, wave-private row pass available; BDS_ACQ_SMALL=0 keeps 256 x 1280)
    const bool allow_small = ncomp == 2 && ctx->tune.fp16_storage != 0 && ctx->tune.small_plan != 0 && ctx->tune.wcols != 0 && !a.no_small;
    if ((rc = plan_build(ctx, a.plan, a.n_ext, N, allow_small))) return rc;
    a.group_env = ctx->tune.group;
    // default: fp32 search arithmetic on fp16-stored spectra (BDS_ACQ_FP16=0: fp32 storage)
    a.half = (a.plan.fast || a.plan.small) && ctx->tune.fp16_storage != 0;
    // code spectrum: |fft(code)| <= X; stored value conj(C)/L * sC, kept below 2^15
    a.sC = a.half ? (float)std::exp2(std::floor(std::log2(32768.0 * (double)a.plan.L / (double)a.X))) : 1.f;
    // primary codes of every PRN, both components
    const size_t prim_bytes = (size_t)BDS_MAX_PRN * 2 * 10230;
    if (!a.d_prim) BDS_HIP(ctx, hipMalloc((void **)&a.d_prim, prim_bytes));
    std::vector<int8_t> prim(prim_bytes);
    for (int prn = 1; prn <= BDS_MAX_PRN; ++prn)
        for (int c = 0; c < 2; ++c) gen_primary(s.signal, c == 1, prn, &prim[((size_t)(prn - 1) * 2 + c) * 10230]);
    BDS_HIP(ctx, hipMemcpy(a.d_prim, prim.data(), prim.size(), hipMemcpyHostToDevice));
    a.tab.prim = a.d_prim;
    a.tab.ts = 1.0 / s.samplingFreq;                                                     // makeDataTable.m:49
    a.tab.tc = s.signal == BDS_SIGNAL_B1C ? 1.0 / s.codeFreqBasis / 2 : 1.0 / s.codeFreqBasis;  // :50 / makeB2aDataTable.m:47
    a.tab.spc = spc;
    a.tab.xlen = X;
    a.tab.code_len = 10230;
    a.tab.boc = s.signal == BDS_SIGNAL_B1C ? 1 : 0;
    return BDS_OK;
}

static hipStream_t st(bds_ctx *ctx) { return (hipStream_t)ctx->stream; }

// raise a kernel's dynamic-LDS limit once per context (= per device)
template <class K>
static void want_lds(bds_ctx *ctx, K kern, size_t bytes) {
    if (ctx->lds_attr_done.insert((const void *)kern).second)
        (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// the run-time-plan kernels (bds_acq_kernels.h, k_rows_fwd_st) size their dynamic LDS from the plan: the limit they may be given,
// leaving room for their small static LDS
constexpr size_t kPlanLdsMax = 160 * 1024 - 4096;

// forward transform of `nb` batches produced by loader `ld` into dst[b*dst_stride]
// forward passes on the specialised stages (plans with pl.fast)
template <int S, class Loader>
static void launch_cols_fwd_t(bds_ctx *ctx, hipStream_t s_, const Plan2D &pl, Loader ld, int nb, float2 *Bw) {
    constexpr int T = 4;
    const size_t lds = sizeof(float2) * (T * tspan<S>() + lds_span(twiddle_entries<S>()));
    want_lds(ctx, k_cols_fwd_t<S, T, Loader>, lds);
    hipLaunchKernelGGL((k_cols_fwd_t<S, T, Loader>), dim3((pl.L2 + T - 1) / T, nb), dim3(cols_threads<S, T>()), lds, s_,
                       (const float2 *)pl.d_tw1, pl.twl, pl.L2, ld, Bw, pl.L);
}
template <int S, class ST>
static void launch_rows_fwd_t(bds_ctx *ctx, hipStream_t s_, const Plan2D &pl, int nb, const float2 *Bw, ST *dst, long dst_stride,
                              int conj_flag, float scale, int perm) {
    const size_t lds = sizeof(float2) * (tspan<S>() + lds_span(twiddle_entries<S>()));
    want_lds(ctx, k_rows_fwd_t<S, ST>, lds);
    hipLaunchKernelGGL((k_rows_fwd_t<S, ST>), dim3(pl.L1, nb), dim3(rows_threads<S>()), lds, s_, (const float2 *)pl.d_tw2, Bw,
                       pl.L, dst, dst_stride, conj_flag, scale, perm);
}
template <class ST>
static void launch_rows_fwd_any(bds_ctx *ctx, hipStream_t s_, const Plan2D &pl, int nb, const float2 *Bw, ST *dst, long dst_stride,
                                int conj_flag, float scale, int perm) {
    switch (pl.L2) {
        case 1280: launch_rows_fwd_t<1280, ST>(ctx, s_, pl, nb, Bw, dst, dst_stride, conj_flag, scale, 0); break;
        case 2048: launch_rows_fwd_t<2048, ST>(ctx, s_, pl, nb, Bw, dst, dst_stride, conj_flag, scale, 0); break;
        case 3072: launch_rows_fwd_t<3072, ST>(ctx, s_, pl, nb, Bw, dst, dst_stride, conj_flag, scale, 0); break;
        default: launch_rows_fwd_t<4096, ST>(ctx, s_, pl, nb, Bw, dst, dst_stride, conj_flag, scale, perm); break;
    }
}

// ---- which kernels a configuration's search runs on ----------------------------------------------------------------
// Decided HERE and nowhere else: kernel_pick() is the only reader of the tuning knobs that select kernels.  The forward transforms
// (element order of the spectra), AcqRun::setup (what the sieve's output looks like), the launcher of a pair (launch_pair) and the timing
// record (AcqRun::finish) read the fields.  The enumerators are the numbers bds_timing::rows_kernel / cols_kernel report.
enum RowsKernel { kRowsPlan = 0, kRowsInvF = 1, kRowsWaveF = 2, kRowsNPoint = 3 };  // run-time plan (k_rows_inv), k_rows_inv_f, k_rows_wave_f, an N-point plan's
enum ColsKernel { kColsPlan = 0, kColsTile = 1, kColsWave = 2, kColsSmall = 3, kColsNPoint = 4 };  // k_cols_inv_max, k_cols_inv_max_f, k_cols_wave_f, k_cols_small_f (80 x 4096), an N-point plan's
struct KernelPick {
    RowsKernel rows = kRowsPlan;
    ColsKernel cols = kColsPlan;
    bool permuted = false;  // the spectra are stored in the element order k_rows_wave_f reads (wrows_perm(), bds_acq_fast.h)
    bool ilv = false;       // an unmasked launch keeps both components of an element side by side in the inter-pass buffer (the 80 x 4096
                            // pair: every launch); launch_pair adds the per-launch part
    bool pk_rows = false, pk_cols = false;  // packed-fp32 butterflies (bds_fft_pk.h) in the row / column pass
    bool fast() const { return rows != kRowsPlan; }        // the fp32-arithmetic specialised kernels (or an N-point pair), not the run-time plan
    bool per_cell() const { return cols >= kColsWave; }    // the column pass reports packed per-cell maxima and running bounds, not per-tile records
};
// npoint = PfaPick::kind of the run (AcqState::cs_pfa; 0: the L-point pair).  Under an N-point pair ilv and pk_rows describe the L-point
// pair of the same plan, which is what kernel_flags has always reported there.  Every fallback of a run (fp32 storage, run-time-plan
// kernels) clears a.half / sets a.no_fast_search and re-runs bds_acq_prepare, which rebuilds the spectra for the new pick.
static KernelPick kernel_pick(const Tuning &tune, const AcqState &a, int npoint) {
    const Plan2D &pl = a.plan;
    KernelPick p;
    if (!(pl.fast || (pl.small && a.half) || npoint) || a.no_fast_search) return p;
    // wave-private 4096-point row pass (bds_acq_wrows.h): fp16 storage; the 80 x 4096 plan has no other
    const bool wave_rows = a.half && pl.L2 == 4096 && (tune.wrows != 0 || pl.small);
    p.rows = npoint ? kRowsNPoint : wave_rows ? kRowsWaveF : kRowsInvF;
    // wave-private column pass: the default, but the 256-point plans keep the tile kernel unless forced with BDS_ACQ_WCOLS=1 (a workgroup's
    // share of such a tile is 8 points per lane and the per-workgroup constants and barriers dominate: cfg2 2.18 vs 1.39 ms per launch)
    const bool wave_cols = tune.wcols != 0 && (pl.L1 != 256 || tune.wcols > 0);
    p.cols = npoint ? kColsNPoint : pl.small ? kColsSmall : wave_cols ? kColsWave : kColsTile;
    p.permuted = p.rows == kRowsWaveF;
    p.ilv = wave_rows && p.per_cell() && a.ncomp == 2 && ((pl.L1 == 768 && tune.ilv != 0) || pl.small);
    p.pk_rows = wave_rows && tune.pk != 0;
    p.pk_cols = p.ilv && p.cols == kColsWave && tune.pk != 0 && tune.pk != 2;  // (BDS_ACQ_PK=2: row pass only; only the interleaved variants have a packed form)
    return p;
}

// (half, ncomp) -> f(StoreTag<ST>{}, std::integral_constant<int, NC>{}): the one place that turns the storage mode and the component
// count into template arguments
template <class ST>
struct StoreTag {
    using type = ST;
};
template <class F>
static void with_storage(bool half, int ncomp, F &&f) {
    using C1 = std::integral_constant<int, 1>;
    using C2 = std::integral_constant<int, 2>;
    if (half)
        ncomp == 2 ? f(StoreTag<__half2>{}, C2{}) : f(StoreTag<__half2>{}, C1{});
    else
        ncomp == 2 ? f(StoreTag<float2>{}, C2{}) : f(StoreTag<float2>{}, C1{});
}

// perm: KernelPick::permuted of the configuration
template <class Loader>
static int forward(bds_ctx *ctx, AcqState &a, Loader ld, int nb, float2 *dst, long dst_stride, int conj_flag,
                   float scale, bool perm) {
    Plan2D &pl = a.plan;
    // rows of a specialised length, stored as the search reads them (dst counts in stored elements)
    const auto rows_typed = [&]() {
        with_storage(a.half, a.ncomp, [&](auto st_, auto) {
            using ST = typename decltype(st_)::type;
            launch_rows_fwd_any<ST>(ctx, st(ctx), pl, nb, (const float2 *)a.d_Bw, (ST *)dst, dst_stride, conj_flag, scale, perm ? 1 : 0);
        });
    };
    if (pl.fast && !ctx->tune.generic_fwd) {
        switch (pl.L1) {
            case 256: launch_cols_fwd_t<256>(ctx, st(ctx), pl, ld, nb, a.d_Bw); break;
            case 512: launch_cols_fwd_t<512>(ctx, st(ctx), pl, ld, nb, a.d_Bw); break;
            case 768: launch_cols_fwd_t<768>(ctx, st(ctx), pl, ld, nb, a.d_Bw); break;
            default: launch_cols_fwd_t<1024>(ctx, st(ctx), pl, ld, nb, a.d_Bw); break;
        }
        rows_typed();
        BDS_HIP(ctx, hipGetLastError());
        return BDS_OK;
    }
    dim3 g1(pl.ntiles, nb), g2(pl.L1, nb);
    want_lds(ctx, k_cols_fwd<Loader>, kPlanLdsMax);
    hipLaunchKernelGGL(k_cols_fwd<Loader>, g1, dim3(pl.nt_cols), pl.lds_cols, st(ctx), pl.p1, pl.twl, pl.L2,
                       pl.logT, pl.Spad, ld, a.d_Bw, pl.L);
    if (fast_rows(pl.L2) && !ctx->tune.generic && !ctx->tune.generic_fwd) {
        // rows of a specialised length under a run-time-plan column pass (the 80 x 4096 plan of cfg2): the compile-time row pass
        // (first stage from global memory, last stage to the typed store; 2 080 rows of cfg2 in ~25 us against 78 on the run-time engine)
        rows_typed();
    } else if (a.half) {  // dst counts in stored elements (fp16 complex)
        want_lds(ctx, k_rows_fwd_st<__half2>, kPlanLdsMax);
        hipLaunchKernelGGL(k_rows_fwd_st<__half2>, g2, dim3(pl.nt_rows), pl.lds_rows, st(ctx), pl.p2,
                           (const float2 *)a.d_Bw, pl.L, (__half2 *)dst, dst_stride, conj_flag, scale, perm ? 1 : 0);
    } else {
        want_lds(ctx, k_rows_fwd, kPlanLdsMax);
        hipLaunchKernelGGL(k_rows_fwd, g2, dim3(pl.nt_rows), pl.lds_rows, st(ctx), pl.p2, (const float2 *)a.d_Bw,
                           pl.L, dst, dst_stride, conj_flag, scale);
    }
    BDS_HIP(ctx, hipGetLastError());
    return BDS_OK;
}

// Cells one row workgroup walks when a multi-PRN launch pair is cut into UNIFORM chunks: all D bins of its PRN if the launch then still
// has >= 32 waves of row workgroups for the chip's 512 slots (their tail is what a short launch of long workgroups loses: 8 PRNs per
// pair in 201-bin workgroups 197.2-197.5 ms per cfg3 call = the lean mode's 197.0, in 67-bin chunks 192.0-192.3; 32 PRNs the same
// either way, profiles/r05_small_pairs*.txt), else the largest divisor of D that gives them, but no chunk below 32 cells.  A chunk stays
// inside one PRN's cells, hence a divisor.  list_gc = BDS_ACQ_LIST_GC of the hooks build (> 0: that divisor, -1: D).
static int rows_uniform_gc(int list_gc, int D, int np, long row_wgs) {
    int gc = D;
    if (list_gc > 0 && D % list_gc == 0) {
        gc = list_gc;
    } else if (list_gc == 0) {
        const long want_wgs = 32L * 512;
        for (int dv = 1; dv <= D; ++dv) {
            if (D % dv) continue;
            const int gc_ = D / dv;  // dv chunks per PRN and row
            if (gc_ < 32 && dv > 1) break;
            gc = gc_;
            if (row_wgs * np * dv >= want_wgs) break;
        }
    }
    return gc;
}

// ---- chunk list of the N-point row pass (bds_acq_pfa.h) ----------------------------------------------------------------------------------
// A launch of np PRNs x D cells runs kRowsWorkWgs working workgroups per chunk of cells, every one of them for (cells of the chunk + set-up) cell-times,
// on `slots` = 2 per CU resident workgroups: the pass ends when the last slot does.  With one chunk size for the whole launch the last round
// of workgroups runs on a nearly empty chip (13 PRNs in 67-cell chunks: 24.2 rounds cost 25).  The list therefore tapers: whole PRNs in
// equal chunks first, then one or a few PRNs in chunks that shrink geometrically, all in non-increasing order, so that what is still
// running when the slots start to drain is small.  No chunk straddles a PRN (a workgroup holds one PRN's code rows).
// The model: greedy assignment in block order onto the slots -- what the dispatcher does with workgroups of equal resources.
static constexpr int kRowsWorkWgs = pfa::kRowsWorkWgs;               // per chunk: the other pfa::kRowsWgs - 318 positions return at once
static constexpr int kRowsSetup8 = 3;                                 // set-up of a workgroup in eighths of a cell (measured 0.29 of a cell: profiles/r16_rows_chunks.txt)

// makespan in eighths of a cell-time of chunks of these sizes, in this order
static long rows_makespan8(const std::vector<int> &sizes, int slots) {
    std::priority_queue<long, std::vector<long>, std::greater<long>> free_at;
    for (int i = 0; i < slots; ++i) free_at.push(0);
    long end = 0;
    for (int sz : sizes) {
        const long d = 8L * sz + kRowsSetup8;
        for (int w = 0; w < kRowsWorkWgs; ++w) {
            const long t = free_at.top() + d;
            free_at.pop();
            free_at.push(t);
            end = std::max(end, t);
        }
    }
    return end;
}

// D cells in k chunks as equal as they come, larger first
static void rows_split_even(int D, int k, std::vector<int> &out) {
    for (int i = 0; i < k; ++i) out.push_back(D / k + (i < D % k ? 1 : 0));
}
// D cells in chunks of 1 / q of what is left, at most `cap` and at least `least` cells
static void rows_split_taper(int D, int cap, int q, int least, std::vector<int> &out) {
    for (int rem = D; rem > 0;) {
        const int c = std::min(rem, std::max(least, std::min(cap, (rem + q - 1) / q)));
        out.push_back(c);
        rem -= c;
    }
}

// the chunks (first cell, cells) of a launch of np PRNs x D cells for `slots` resident workgroups; `uniform_gc` = the chunk size the
// uniform rule would take (always a candidate: the list is never worse than it under the model)
static std::vector<int2> rows_chunk_plan(int np, int D, int slots, int uniform_gc) {
    std::vector<int2> best;
    if (np < 1 || D < 1 || slots < 1) return best;
    long best_t = -1;
    std::vector<int> ks;
    for (int k : {1, 2, 3, 4, 6, (D + std::max(1, uniform_gc) - 1) / std::max(1, uniform_gc)})
        if (k >= 1 && k <= D && std::find(ks.begin(), ks.end(), k) == ks.end()) ks.push_back(k);
    std::vector<std::vector<int>> per_prn((size_t)np);
    auto consider = [&]() {
        // all chunks of all PRNs, larger first; among equals the order of the cells
        std::vector<int2> list;
        for (int p = 0; p < np; ++p) {
            int c = p * D;
            for (int sz : per_prn[(size_t)p]) list.push_back(make_int2(c, sz)), c += sz;
        }
        std::stable_sort(list.begin(), list.end(), [](const int2 &a, const int2 &b) { return a.y > b.y; });
        std::vector<int> sizes;
        for (const int2 &ch : list) sizes.push_back(ch.y);
        const long t = rows_makespan8(sizes, slots);
        if (best_t < 0 || t < best_t || (t == best_t && list.size() < best.size())) best_t = t, best = list;
    };
    for (int k : ks) {
        const int cap = (D + k - 1) / k;
        for (int tapered = 0; tapered <= std::min(np, 3); ++tapered)
            for (int q : {2, 3, 4})
                for (int least : {1, 3}) {
                    if (!tapered && (q != 2 || least != 1)) continue;  // (nothing tapers: one candidate)
                    for (int p = 0; p < np; ++p) {
                        per_prn[(size_t)p].clear();
                        if (p < np - tapered)
                            rows_split_even(D, k, per_prn[(size_t)p]);
                        else
                            rows_split_taper(D, cap, q, least, per_prn[(size_t)p]);
                    }
                    consider();
                }
    }
    return best;
}

int rows_chunk_list(int np, int D, int slots, int *out, int cap) {
    const std::vector<int2> plan = rows_chunk_plan(np, D, slots, rows_uniform_gc(0, D, np, pfa::kRowsWgs));
    for (int i = 0; i < (int)plan.size() && i < cap; ++i) out[2 * i] = plan[(size_t)i].x, out[2 * i + 1] = plan[(size_t)i].y;
    return (int)plan.size();
}
int rows_place_list(int *out, int cap) {
    for (int l = 0; l < pfa::kRowsWgs && l < cap; ++l) out[2 * l] = pfa::rows_pos(l), out[2 * l + 1] = pfa::rows_place(pfa::rows_pos(l));
    return pfa::kRowsWgs;
}
int rows_lds_index_of(int e) { return e >= 0 && e < pfa::K3 ? pfa::rows_lds_index(e) : -1; }

// optional per-cell descriptors (device arrays) for a launch whose cells are not "one PRN, consecutive bins"
struct CellList {
    const int *bin = nullptr;    // Doppler bin of cell g
    const long *cs = nullptr;    // element offset of its code spectra from the Cs base
    const int4 *rng = nullptr;   // searched lag ranges (lo1, hi1, lo2, hi2)
    int gc = 1;                  // consecutive listed cells that share their code spectra (one row workgroup walks them)
    const int *src = nullptr;    // 80 x 4096 plan and bds_acq_pfa6.h only: the rows of listed cell g already lie at cell index src[g] of Bw -- no row pass
    const int2 *chunks = nullptr;  // bds_acq_pfa.h only: the row pass's chunks (first cell, cells) in place of uniform gc (rows_chunk_plan)
    int nchunks = 0;
};
// where a column pass reports: the sieve (bds_acq_sieve.h); the tile kernel writes per-tile records instead of cellmax / lb (both
// null then) and uses the list as its overflow list
struct SieveOut {
    Rec *recs = nullptr;
    SieveArgs sieve{nullptr, nullptr, 1, nullptr, nullptr, 0, 0, 1.f};
    hipEvent_t mid = nullptr;  // recorded between the two passes of a sampled launch pair (timing)
};

// ---- one launch pair of the L-point search: what it works on, and the launchers (dispatch on the compile-time lengths) --------------
struct PairArgs {
    const void *Xs = nullptr;  // signal spectra, one per Doppler bin
    const void *Cs = nullptr;  // code spectra: of the pair's PRN, or with a cell list the base cl.cs counts from
    void *Bw = nullptr;        // inter-pass buffer
    int G = 0, bin0 = 0;       // cells; without a cell list they are the bins bin0 .. bin0 + G - 1
    float out_scale = 1.f;     // of the row pass's stores
    float w0 = 1.f, w1 = 1.f;  // magnitude weights of the components
    int lo1 = 0, hi1 = -1, lo2 = 1, hi2 = 0;  // searched lag ranges (inclusive, empty when lo > hi); with cl.rng the list's
    SieveOut so;
    CellList cl;
    bool unmasked() const { return !cl.rng && lo1 == 0 && lo2 > hi2; }  // one lag range from 0
};

template <int S, int NC, class ST>
static void launch_rows_f(bds_ctx *ctx, hipStream_t sr, const Plan2D &pl, const KernelPick &pick, const PairArgs &pa, bool ilv) {
    const CellList &cl = pa.cl;
    const int G = pa.G;
    const size_t lds = sizeof(float2) * (tspan<S>() + f32_tw_span<S, false>());
    want_lds(ctx, k_rows_inv_f<S, NC, ST>, lds);
    // balanced chunks of at most tune.gchunk cells
    int nch = (G + ctx->tune.gchunk - 1) / ctx->tune.gchunk;
    int gc = (G + nch - 1) / nch;
    if (cl.bin) gc = cl.gc, nch = (G + cl.gc - 1) / cl.gc;  // a workgroup stays inside one PRN's cells
    const int nvb = pl.L1 * nch;  // L1 % 8 == 0 on every specialised plan: virtual workgroup vb sits on XCD vb % 8
    const RowsFArgs A{pl.d_tw2, pl.twl, pa.Xs, pl.L, pl.L1, G, pa.bin0, pa.Cs, pa.Bw, pa.out_scale, gc, nch, cl.bin, cl.cs, nvb, ctx->tune.clockprobe ? pl.d_clk : nullptr, ilv ? 1 : 0};
    const int grid = ctx->tune.rows_grid > 0 ? std::min(nvb, (ctx->tune.rows_grid + 7) / 8 * 8) : nvb;
    if constexpr (S == 4096 && std::is_same<ST, __half2>::value) {
        if (pick.rows == kRowsWaveF) {  // wave-private row pass (bds_acq_wrows.h): per-lane twiddle constants, 4 barriers per cell
            RowsFArgs B = A;
            B.tw = pl.d_wrtab;
            const bool pk = pick.pk_rows;
            auto go = [&](auto kern) {
                want_lds(ctx, kern, kWRowsLdsBytes);
                hipLaunchKernelGGL(kern, dim3(grid), dim3(256), kWRowsLdsBytes, sr, B);
            };
            if constexpr (NC == 2) {
                if (ilv) {
                    if (pk) go(k_rows_wave_f<NC, true, true>);
                    else go(k_rows_wave_f<NC, true, false>);
                    return;
                }
            }
            if (pk) go(k_rows_wave_f<NC, false, true>);
            else go(k_rows_wave_f<NC, false, false>);
            return;
        }
    }
    hipLaunchKernelGGL((k_rows_inv_f<S, NC, ST>), dim3(grid), dim3(rows_threads<S>()), lds, sr, A);
}
template <int S, int T, int NC, class ST>
static void launch_cols_ft(bds_ctx *ctx, hipStream_t sc, const Plan2D &pl, const PairArgs &pa) {
    const SieveOut &so = pa.so;
    const size_t lds = sizeof(float2) * (T * tspan<S>() + f32_tw_span<S, f32_tab_cols<S>()>());
    const ColsFArgs A{(const float2 *)(f32_tab_cols<S>() ? pl.d_ftab1 : pl.d_tw1), pl.L2, pa.Bw, pl.L, pa.w0, pa.w1, pa.lo1, pa.hi1, pa.lo2, pa.hi2, so.recs, pl.ntiles, pa.cl.rng,
                      so.sieve.extra, so.sieve.extra_count, so.sieve.extra_cap, so.sieve.cell0, so.sieve.keep};
    if (!pa.unmasked()) {
        want_lds(ctx, k_cols_inv_max_f<S, T, NC, true, ST>, lds);
        hipLaunchKernelGGL((k_cols_inv_max_f<S, T, NC, true, ST>), dim3(pl.ntiles, pa.G), dim3(cols_threads<S, T>()), lds, sc, A);
    } else {
        want_lds(ctx, k_cols_inv_max_f<S, T, NC, false, ST>, lds);
        hipLaunchKernelGGL((k_cols_inv_max_f<S, T, NC, false, ST>), dim3(pl.ntiles, pa.G), dim3(cols_threads<S, T>()), lds, sc, A);
    }
}
// wave-private column pass: one tile per workgroup, workgroups started by the hardware in list order (see the kernel's
// note on item order)
template <int S, int NC, bool MASKED, class ST, int NV, bool ILV = false, bool PK = false>
static void launch_cols_wm(bds_ctx *ctx, hipStream_t sc, const WColsArgs &A) {
    using W = WCols<S>;
    want_lds(ctx, k_cols_wave_f<S, NC, MASKED, ST, NV, ILV, PK>, W::kLdsBytes);
    WColsArgs B = A;
    const int quads = A.ntiles / 32;  // per XCD and cell
    const int want = ctx->tune.wcols_qchunk > 0 ? ctx->tune.wcols_qchunk : A.G >= 1000 ? 2 : 4;  // (see Tuning::wcols_qchunk: measured at 201 and at 6432 cells per launch)
    B.qchunk = std::max(1, std::min(want, quads));
    while (quads % B.qchunk) --B.qchunk;
    hipLaunchKernelGGL((k_cols_wave_f<S, NC, MASKED, ST, NV, ILV, PK>), dim3(A.n_items), dim3(W::NT), W::kLdsBytes, sc, B);
}
template <int S, int NC, class ST>
static void launch_cols_w(bds_ctx *ctx, hipStream_t sc, const Plan2D &pl, const KernelPick &pick, const PairArgs &pa, bool ilv) {
    const int ntiles = pl.L2 / WCols<S>::T;  // L2 % 256 == 0 on every specialised plan: ntiles % 32 == 0 (8 XCDs x quads)
    const WColsArgs A{(const float2 *)pl.d_wtab, pl.L2, ntiles, pa.G, pa.G * ntiles, pa.Bw, pl.L, pa.w0, pa.w1, pa.lo1, pa.hi1, pa.lo2, pa.hi2, pa.cl.rng, pa.so.sieve, 1,
                      ctx->tune.clockprobe ? pl.d_clk : nullptr};
    const bool six = pa.hi1 / pl.L2 < 6 * 8 * WCols<S>::R1;  // no searched lag beyond output row 48 R1: outputs v = 6, 7 of the last stage unused
    if constexpr (S == 768 && NC == 2 && std::is_same<ST, __half2>::value) {  // (the plan with 4096-point rows: cfg3)
        if (ilv) {  // k_rows_wave_f<2, true> laid the buffer out [cell][element][component]
            if (six) {
                if (pick.pk_cols) launch_cols_wm<S, NC, false, ST, 6, true, true>(ctx, sc, A);
                else launch_cols_wm<S, NC, false, ST, 6, true>(ctx, sc, A);
            } else {
                if (pick.pk_cols) launch_cols_wm<S, NC, false, ST, 8, true, true>(ctx, sc, A);
                else launch_cols_wm<S, NC, false, ST, 8, true>(ctx, sc, A);
            }
            return;
        }
    }
    if (!pa.unmasked())
        launch_cols_wm<S, NC, true, ST, 8>(ctx, sc, A);
    else if (six)
        launch_cols_wm<S, NC, false, ST, 6>(ctx, sc, A);
    else
        launch_cols_wm<S, NC, false, ST, 8>(ctx, sc, A);
}
// One group of cells: row pass, then column pass, on one stream, with the kernels of `pick`.  What only a launch knows is applied here:
//  * a launch that reports per-tile records (pa.so.sieve.cellmax null: the second-peak pass of the host refinement) takes the tile kernel
//    whatever the main search's column pass is -- the wave-private kernel's running bounds have nothing to run on there;
//  * components are interleaved (pick.ilv) only in an unmasked launch of the wave-private pair; the 80 x 4096 pair interleaves always.
template <int NC, class ST>
static void launch_pair(bds_ctx *ctx, hipStream_t st_, const Plan2D &pl, const KernelPick &pick, const PairArgs &pa) {
    const SieveOut &so = pa.so;
    const int G = pa.G;
    if (pick.rows == kRowsPlan) {  // run-time-plan kernels: fp32 storage, per-tile records, no lag mask beyond the two ranges
        want_lds(ctx, k_rows_inv<NC>, kPlanLdsMax);
        want_lds(ctx, k_cols_inv_max<NC>, kPlanLdsMax);
        hipLaunchKernelGGL(k_rows_inv<NC>, dim3(pl.L1, G), dim3(pl.nt_rows), pl.lds_rows, st_, pl.p2, pl.twl, (const float2 *)pa.Xs, pl.L, pa.bin0,
                           (const float2 *)pa.Cs, (float2 *)pa.Bw);
        hipLaunchKernelGGL(k_cols_inv_max<NC>, dim3(pl.ntiles, G), dim3(pl.nt_cols), pl.lds_cols, st_, pl.p1, pl.L2, pl.logT, pl.Spad,
                           (const float2 *)pa.Bw, pl.L, pa.w0, pa.w1, pa.lo1, pa.hi1, pa.lo2, pa.hi2, so.recs, pl.ntiles);
        return;
    }
    if constexpr (NC == 2 && std::is_same<ST, __half2>::value) {
        if (pick.cols == kColsSmall) {  // 80 x 4096: wave-private row pass (components interleaved) + one lane per column and component
            if (!pa.cl.src) launch_rows_f<4096, NC, ST>(ctx, st_, pl, pick, pa, true);
            if (so.mid) (void)hipEventRecord(so.mid, st_);
            const SColsArgs A{(const float2 *)pl.d_tw80, pl.L2, G, pa.Bw, pl.L, pa.w0, pa.w1, pa.lo1, pa.hi1, pa.lo2, pa.hi2, pa.cl.rng, so.sieve, pa.cl.src};
            want_lds(ctx, k_cols_small_f<NC>, kSColsLdsBytes);
            hipLaunchKernelGGL((k_cols_small_f<NC>), dim3((unsigned)(G * (pl.L2 / (kSColsNT / 2)))), dim3(kSColsNT), kSColsLdsBytes, st_, A);
            return;
        }
    }
    const bool wave = pick.cols == kColsWave && so.sieve.cellmax;
    // (the interleaved variants exist for the 768 x 4096 plan, two components, fp16 storage: what pick.ilv holds)
    const bool ilv = pick.ilv && wave && pa.unmasked();
    switch (pl.L2) {
        case 1280: launch_rows_f<1280, NC, ST>(ctx, st_, pl, pick, pa, false); break;
        case 2048: launch_rows_f<2048, NC, ST>(ctx, st_, pl, pick, pa, false); break;
        case 3072: launch_rows_f<3072, NC, ST>(ctx, st_, pl, pick, pa, false); break;
        default: launch_rows_f<4096, NC, ST>(ctx, st_, pl, pick, pa, ilv); break;
    }
    if (so.mid) (void)hipEventRecord(so.mid, st_);
    const auto cols = [&](auto s_) {
        constexpr int S = decltype(s_)::value;
        if (wave)
            launch_cols_w<S, NC, ST>(ctx, st_, pl, pick, pa, ilv);
        else if (pl.logT == 2)
            launch_cols_ft<S, 4, NC, ST>(ctx, st_, pl, pa);
        else
            launch_cols_ft<S, 8, NC, ST>(ctx, st_, pl, pa);
    };
    switch (pl.L1) {
        case 256: cols(std::integral_constant<int, 256>{}); break;
        case 512: cols(std::integral_constant<int, 512>{}); break;
        case 768: cols(std::integral_constant<int, 768>{}); break;
        default: cols(std::integral_constant<int, 1024>{}); break;
    }
}

// inter-pass work buffer in float2-sized elements per transform length: the `group` cells of one launch pair at the storage type of
// the search (fp16 complex: half an element) -- which is also what the forward pass of `group` bins needs at fp32.  (Rounds 1-5 kept two
// fp32-sized halves whatever the mode: 20 GB at cfg3 where 5 are used -- and every GiB a context frees is a GiB the driver clears before
// the next user gets it.)
static size_t bw_batches(const AcqState &a) {
    const int per_cell = a.half ? 1 : 2;                                  // float2-sized elements per cell and two components
    const int search = (a.group * a.ncomp * per_cell + 1) / 2;
    return (size_t)std::max(std::max(search, std::min(a.group, a.D > 0 ? a.D : a.group)), 8);
}

// cells per launch pair for a search over D bins: the whole Doppler row of a PRN when the two
// halves of the inter-pass buffer stay under 24 GiB (B1C cfg3: 201 cells, 20 GiB of the 288)
static void pick_group(AcqState &a, const bds_settings &s) {
    const int D = (int)m_round(s.acqSearchBand * 2 / s.acqStep) + 1;
    const double per_cell = 2.0 * a.ncomp * (double)a.plan.L * sizeof(float2);
    const int cap = (int)std::max(1.0, std::floor(24.0 * 1073741824.0 / per_cell));
    a.group = a.group_env ? a.group_env : std::min(cap, 256);
    a.group = std::max(1, std::min(a.group, D));
}

}  // namespace bds

using namespace bds;

// =======================================================================================
// The settings acquisition() works with after its resampling branch reassigned samplingFreq and IF
// (acquisition.m:103,119); everything downstream -- code tables, sizes, frequency bins -- uses these.
static const bds_settings *effective(const bds_settings *s, bds_settings *tmp) {
    const ResamplePlan r = resample_plan(*s);
    if (!r.on) return s;
    *tmp = *s;
    tmp->samplingFreq = r.new_fs;
    tmp->IF = r.new_if;
    tmp->resamplingflag = 0;
    return tmp;
}

// filtfilt(fir1(700, wp), 1, longSignal) + index decimation on the device (acquisition.m:56-112);
// leaves the conditioned block in a.d_sig64 and its host copy in h_re / h_im.
template <int NCH, class T>
static int condition_block(bds_ctx *ctx, AcqState &a, const ResamplePlan &r, long n_in, long *n_out) {
    constexpr int kTaps = 701, kFact = 3 * (kTaps - 1);  // filtfilt: nfact = 3*(nfilt-1)
    if (n_in <= kFact) return fail(ctx, BDS_ERR_ARG, "longSignal (%ld samples) is too short for filtfilt (needs > %d)", n_in, kFact);
    const std::vector<double> b = fir1_bandpass(kTaps, r.wp1, r.wp2);
    const long len = n_in + 2L * kFact;
    int rc;
    if ((rc = ensure(ctx, &a.d_fir, &a.fir_cap, (size_t)kTaps))) return rc;
    if ((rc = ensure(ctx, &a.d_ffa, &a.ffa_cap, (size_t)len * NCH))) return rc;
    if ((rc = ensure(ctx, &a.d_ffb, &a.ffb_cap, (size_t)len * NCH))) return rc;
    BDS_HIP(ctx, hipMemcpyAsync(a.d_fir, b.data(), sizeof(double) * kTaps, hipMemcpyHostToDevice, st(ctx)));
    const dim3 grid(2048), blk(256);
    hipLaunchKernelGGL((k_ff_extend<NCH, T>), grid, blk, 0, st(ctx), (const T *)a.d_sig, n_in, kFact, a.d_ffa);
    hipLaunchKernelGGL(k_ff_fir<NCH>, grid, blk, sizeof(double) * kTaps, st(ctx), (const double *)a.d_ffa, len,
                       (const double *)a.d_fir, kTaps, 0, a.d_ffb);
    hipLaunchKernelGGL(k_ff_fir<NCH>, grid, blk, sizeof(double) * kTaps, st(ctx), (const double *)a.d_ffb, len,
                       (const double *)a.d_fir, kTaps, 1, a.d_ffa);
    const long sig_len = (long)std::floor((double)(n_in - 1) / r.old_fs * r.new_fs);  // :107
    if (sig_len < 1) return fail(ctx, BDS_ERR_ARG, "resampled longSignal is empty");
    if ((rc = ensure(ctx, &a.d_sig64, &a.sig64_cap, (size_t)(sig_len + 4) * NCH))) return rc;  // (+4 samples: k_corr reads whole groups of four, bds_acq_corr.h)
    hipLaunchKernelGGL(k_ff_decimate<NCH>, grid, blk, 0, st(ctx), (const double *)a.d_ffa, kFact, sig_len, r.new_fs,
                       r.old_fs, a.d_sig64);
    BDS_HIP(ctx, hipGetLastError());
    std::vector<double> h((size_t)sig_len * NCH);
    BDS_HIP(ctx, hipMemcpyAsync(h.data(), a.d_sig64, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st(ctx)));
    BDS_HIP(ctx, hipStreamSynchronize(st(ctx)));
    a.h_re.resize((size_t)sig_len);
    a.h_im.assign(NCH == 2 ? (size_t)sig_len : 0, 0.0);
    for (long i = 0; i < sig_len; ++i) {
        a.h_re[(size_t)i] = h[(size_t)i * NCH];
        if (NCH == 2) a.h_im[(size_t)i] = h[(size_t)i * NCH + 1];
    }
    *n_out = sig_len;
    return BDS_OK;
}

// sum |x| and sum x^2 over the periodically extended block the search transforms (they set the fp16
// storage scales); keyed by the sizes they were computed for, so a run whose settings changed N re-derives them
static void ext_sums(AcqState &a) {
    a.sum_abs_ext = a.sum_sq_ext = 0;
    if (a.skind == kS8) {
        // (integers: the sequential f64 sums of rounds 1-4 were exact too, so these are the same values)
        long sa = 0, sq = 0;
        const int8_t *b = a.h_s8.data();
        for (long m = 0; m < a.N; ++m) sa += std::abs((int)b[m]), sq += (int)b[m] * (int)b[m];
        long sa2 = 0, sq2 = 0;
        for (long m = 0; m < a.n_ext - a.N; ++m) sa2 += std::abs((int)b[m]), sq2 += (int)b[m] * (int)b[m];
        a.sum_abs_ext = (double)(sa + sa2), a.sum_sq_ext = (double)(sq + sq2);
    } else {
        for (long i = 0; i < a.n_ext; ++i) {
            const long m = i < a.N ? i : i - a.N;
            const double v = a.cplx ? std::hypot(a.sample_re(m), a.sample_im(m)) : std::fabs(a.sample_re(m));
            a.sum_abs_ext += v;
            a.sum_sq_ext += v * v;
        }
    }
    a.sums_N = a.N;
    a.sums_next = a.n_ext;
}

// bds_acq_load and bds_acq_load_dev: the block is at `samples` in host memory, or (samples == NULL) at `d_samples` in device memory,
// which the caller has checked (check_device_span).  A device block is copied device to device where a host block is copied host to
// device, and then brought to the host once, as the packed path always was: everything from there on -- the block statistics, the
// resampling branch, what acq_run reads -- is the same lines on the same bytes for both sources.
// w16: the block holds int16 samples (settings.dataType 1; `samples` then points at int16 values).  They are widened to float64 on
// the device -- exactly: every int16 is a float64 -- and the search reads that block as it reads the resampling branch's.
static int acq_load_block(bds_ctx *ctx, const bds_settings *s_in, const int8_t *samples, const void *d_samples, size_t n_samples,
                          int is_complex, bool w16 = false) {
    if (int rc0 = check_settings(ctx, *s_in)) return rc0;  // (the resampling band edges are only visible here)
    if (w16 && is_complex == 2)
        return fail(ctx, BDS_ERR_ARG, "is_complex = 2 (packed 2+2-bit I/Q) has no 16-bit form: settings.dataType must be 'schar' (0)");
    bds_settings eff;
    const bds_settings *s = effective(s_in, &eff);
    // n_samples counts complex samples when is_complex: `samples` then holds 2*n_samples int8 (I,Q pairs), or, is_complex == 2,
    // ceil(n_samples / 2) packed bytes (fileType 3)
    if (is_complex < 0 || is_complex > 2) return fail(ctx, BDS_ERR_ARG, "is_complex must be 0 (real), 1 (I/Q int8 pairs) or 2 (packed 2+2-bit I/Q)");
    const bool cplx = is_complex != 0, packed = is_complex == 2;
    if (ctx->acq && ctx->acq->fell_back) {  // a new block: back to the default storage and kernels (acq_configure re-derives them)
        ctx->acq->fell_back = false;
        ctx->acq->no_small = false;
        ctx->acq->plan.L = 0;
    }
    int rc = acq_configure(ctx, *s);
    if (rc) return rc;
    AcqState &a = *ctx->acq;
    const ResamplePlan r = resample_plan(*s_in);
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nv = n_samples * (cplx ? 2 : 1);  // values of the block
    const size_t nb = w16 ? 2 * nv : nv;           // ... and its bytes as loaded
    const size_t npk = packed ? (n_samples + 1) / 2 : 0;  // packed bytes: each becomes four int8 (the last pair is unused when n_samples is odd)
    if ((rc = ensure(ctx, &a.d_sig, &a.sig_cap, std::max(nb, 4 * npk) + 16))) return rc;  // (+16: k_corr reads whole dwords, bds_acq_corr.h)
    std::vector<int8_t> h_unpacked;
    if (packed) {
        // The bytes go to the device as they are; the search, and the host's sums below, work on the int8 I/Q block unpacked there
        if ((rc = ensure(ctx, &a.d_packed, &a.packed_cap, npk))) return rc;
        if (samples)
            BDS_HIP(ctx, hipMemcpyAsync(a.d_packed, samples, npk, hipMemcpyHostToDevice, st(ctx)));
        else
            BDS_HIP(ctx, hipMemcpyAsync(a.d_packed, d_samples, npk, hipMemcpyDeviceToDevice, st(ctx)));
        if ((rc = unpack_cplx_device(ctx, a.d_packed, npk, a.d_sig))) return rc;
        h_unpacked.resize(nb);
        BDS_HIP(ctx, hipMemcpyAsync(h_unpacked.data(), a.d_sig, nb, hipMemcpyDeviceToHost, st(ctx)));
        BDS_HIP(ctx, hipStreamSynchronize(st(ctx)));
        samples = h_unpacked.data();
    } else if (samples) {
        BDS_HIP(ctx, hipMemcpyAsync(a.d_sig, samples, nb, hipMemcpyHostToDevice, st(ctx)));
    } else {
        BDS_HIP(ctx, hipMemcpyAsync(a.d_sig, d_samples, nb, hipMemcpyDeviceToDevice, st(ctx)));
        h_unpacked.resize(nb);
        BDS_HIP(ctx, hipMemcpyAsync(h_unpacked.data(), a.d_sig, nb, hipMemcpyDeviceToHost, st(ctx)));
        BDS_HIP(ctx, hipStreamSynchronize(st(ctx)));  // (the caller's memory has been read; the host sums below work on this copy)
        samples = h_unpacked.data();
    }
    a.cplx = cplx;
    a.rs = r;
    a.w16 = w16;
    long n_eff = (long)n_samples;
    if (r.on) {
        if (w16)
            rc = cplx ? condition_block<2, int16_t>(ctx, a, r, (long)n_samples, &n_eff) : condition_block<1, int16_t>(ctx, a, r, (long)n_samples, &n_eff);
        else
            rc = cplx ? condition_block<2, int8_t>(ctx, a, r, (long)n_samples, &n_eff) : condition_block<1, int8_t>(ctx, a, r, (long)n_samples, &n_eff);
        if (rc) return rc;
        a.skind = cplx ? kF64C : kF64;
    } else if (w16) {
        // the float64 view of the block, on the device for the search and on the host for the sums and the refinement jobs
        if ((rc = ensure(ctx, &a.d_sig64, &a.sig64_cap, nv + 8))) return rc;  // (+4 samples: k_corr reads whole groups of four, bds_acq_corr.h)
        hipLaunchKernelGGL(k_widen16, dim3(2048), dim3(256), 0, st(ctx), (const int16_t *)a.d_sig, (long)nv, a.d_sig64);
        BDS_HIP(ctx, hipGetLastError());
        const int16_t *h16 = reinterpret_cast<const int16_t *>(samples);
        a.h_re.resize(n_samples);
        a.h_im.assign(cplx ? n_samples : 0, 0.0);
        for (size_t i = 0; i < n_samples; ++i) {
            a.h_re[i] = (double)h16[cplx ? 2 * i : i];
            if (cplx) a.h_im[i] = (double)h16[2 * i + 1];
        }
        a.skind = cplx ? kF64C : kF64;
    } else {
        a.skind = cplx ? kS8C : kS8;
        a.h_s8.assign(samples, samples + nb);
        a.h_re.clear(), a.h_im.clear(), a.h_prefix.clear(), a.h_prefix_q.clear();
    }
    if (n_eff < a.N)
        return fail(ctx, BDS_ERR_ARG, "longSignal has %ld samples%s; acquisition needs at least %ld (acquisition.m:140)",
                    n_eff, r.on ? " after resampling" : "", a.N);
    a.n_samples = n_eff;
    a.sigpower_X = 0;
    if (a.skind >= kF64) {
        a.h_s8.clear(), a.h_cpre.clear(), a.h_cpre_q.clear();
        a.h_prefix.resize((size_t)n_eff + 1);
        a.h_prefix[0] = 0;
        a.h_prefix_q.clear();
        for (long i = 0; i < n_eff; ++i) a.h_prefix[(size_t)i + 1] = a.h_prefix[(size_t)i] + a.h_re[(size_t)i];
        if (cplx) {
            a.h_prefix_q.resize((size_t)n_eff + 1);
            a.h_prefix_q[0] = 0;
            for (long i = 0; i < n_eff; ++i) a.h_prefix_q[(size_t)i + 1] = a.h_prefix_q[(size_t)i] + a.h_im[(size_t)i];
        }
    } else {
        // prefix sums at every 256th sample: the host's DC means (AcqState::prefix) and the device refinement chain's (the DC of
        // the B1C fine-search block, bds_acq_refine.h) both add the few samples in between
        const size_t nc = (size_t)(n_eff >> 8) + 1;
        a.h_cpre.resize(nc);
        a.h_cpre_q.resize(cplx ? nc : 0);
        long tot = 0, tot_q = 0;
        const int8_t *b = a.h_s8.data();
        for (size_t c = 0; c < nc; ++c) {
            a.h_cpre[c] = (double)tot;
            if (cplx) a.h_cpre_q[c] = (double)tot_q;
            const long m0 = (long)c << 8, m1 = std::min(m0 + 256, n_eff);
            int s0 = 0, s1 = 0;
            if (cplx)
                for (long m = m0; m < m1; ++m) s0 += b[2 * m], s1 += b[2 * m + 1];
            else
                for (long m = m0; m < m1; ++m) s0 += b[m];
            tot += s0, tot_q += s1;
        }
        if ((rc = ensure(ctx, &a.d_prefix_c, &a.prefix_c_cap, nc))) return rc;
        BDS_HIP(ctx, hipMemcpyAsync(a.d_prefix_c, a.h_cpre.data(), sizeof(double) * nc, hipMemcpyHostToDevice, st(ctx)));
        if (cplx) {
            if ((rc = ensure(ctx, &a.d_prefix_cq, &a.prefix_cq_cap, nc))) return rc;
            BDS_HIP(ctx, hipMemcpyAsync(a.d_prefix_cq, a.h_cpre_q.data(), sizeof(double) * nc, hipMemcpyHostToDevice, st(ctx)));
        }
    }
    ext_sums(a);
    BDS_HIP(ctx, hipStreamSynchronize(st(ctx)));
    return BDS_OK;
}

// the typed entries take the sample type of settings.dataType only
static int check_entry_type(bds_ctx *ctx, const bds_settings &s, const char *who, bool w16) {
    if (!w16 && s.dataType != 0)
        return fail(ctx, BDS_ERR_UNSUPPORTED, "%s takes int8 samples: settings.dataType must be 'schar' (0); an 'int16' (1) block goes to %s16", who, who);
    if (w16 && s.dataType != 1)
        return fail(ctx, BDS_ERR_ARG, "%s16 takes int16 samples: settings.dataType must be 'int16' (1), not %d", who, (int)s.dataType);
    return BDS_OK;
}

extern "C" int bds_acq_load(bds_ctx *ctx, const bds_settings *s_in, const int8_t *samples, size_t n_samples,
                            int is_complex) {
    if (!ctx || !s_in || !samples) return BDS_ERR_ARG;
    if (int rc = check_entry_type(ctx, *s_in, "bds_acq_load", false)) return rc;
    return acq_load_block(ctx, s_in, samples, nullptr, n_samples, is_complex);
}

extern "C" int bds_acq_load16(bds_ctx *ctx, const bds_settings *s_in, const int16_t *samples, size_t n_samples, int is_complex) {
    if (!ctx || !s_in || !samples) return BDS_ERR_ARG;
    if (int rc = check_entry_type(ctx, *s_in, "bds_acq_load", true)) return rc;
    return acq_load_block(ctx, s_in, reinterpret_cast<const int8_t *>(samples), nullptr, n_samples, is_complex, true);
}

extern "C" int bds_acq_load_dev(bds_ctx *ctx, const bds_settings *s_in, const void *d_samples, size_t n_samples, int is_complex) {
    if (!ctx || !s_in) return BDS_ERR_ARG;
    if (is_complex < 0 || is_complex > 2) return fail(ctx, BDS_ERR_ARG, "is_complex must be 0 (real), 1 (I/Q int8 pairs) or 2 (packed 2+2-bit I/Q)");
    if (!d_samples) return fail(ctx, BDS_ERR_ARG, "bds_acq_load_dev: d_samples is NULL");
    if (n_samples > ((size_t)1 << 62)) return fail(ctx, BDS_ERR_ARG, "bds_acq_load_dev: n_samples = %zu", n_samples);
    const bool w16 = s_in->dataType == 1;  // (any other value but 0 is refused by the settings check)
    if (w16 && is_complex == 2)
        return fail(ctx, BDS_ERR_ARG, "is_complex = 2 (packed 2+2-bit I/Q) has no 16-bit form: settings.dataType must be 'schar' (0)");
    const size_t bytes = (is_complex == 2 ? (n_samples + 1) / 2 : is_complex == 1 ? 2 * n_samples : n_samples) * (w16 ? 2 : 1);
    if (int rc = check_device_span(ctx, "bds_acq_load_dev", "d_samples", d_samples, bytes)) return rc;
    return acq_load_block(ctx, s_in, nullptr, d_samples, n_samples, is_complex, w16);
}

// Does an N-point pair apply to a run with these settings, and which?  B1C with both components on N = 53 x 12 x 3125 samples
// (99.375 MS/s, acqCohT = 10: bds_acq_pfa.h) or N = 53 x 32 x 625 (53 MS/s, the reference's initSettings.m: bds_acq_pfa32.h), fp16
// storage, no resampling, and whole spectrum bins per Doppler step: acqStep N / fs an integer
// (B1C/acquisition.m:194-198: frqBins(b) = IF - band + acqStep (b - 1), so fft(carr_b x)[k] = fft(carr_1 x)[k - (b - 1) acqStep N / fs]).
// Everything else -- and every fallback of a run (fp32 storage, run-time-plan kernels) -- takes the L-point pair.
// LDS the device chain's fine-frequency pick (k_ref_fine_pick, bds_acq_refine.h) keeps its sums in: settings with thousands of fine
// frequencies (acqStep / 25 large) exceed kFinePickLdsMax and are refined through the host.  One formula for device_refine_ok(),
// refine_device() and pfa6_pick().
constexpr size_t kFinePickLdsMax = 60000;
static size_t fine_pick_lds(const bds_settings &s, int signal, int ncomp) {
    const bool b1c = signal == BDS_SIGNAL_B1C;
    const size_t nfine = b1c ? (size_t)m_round(s.acqStep / 25) * 2 + 1 : (size_t)m_round(s.acqStep / 25) + 1;  // B1C :267, B2a :265
    return sizeof(double) * ((size_t)(b1c ? ncomp : 2 * s.fineNoncoh) * nfine + nfine);
}
// ---- the N-point plans: each header's `Plan` describes and launches its pair (bds_acq_pfa.h) ------------------------------------------
// What the host asks of the selected plan at run time, as plain data
struct NPointInfo {
    int kind = 0;  // the number AcqState::cs_pfa keeps.  0: none, the L-point pair
    long np = 0;   // transform length N = K1 K2 K3
    int k3 = 0, rows = 0, rows_wgs = 0;             // row length, rows K1 K2, row workgroups per chunk of cells
    size_t cell_elems = 0, spec_elems = 0;          // 4-byte (fp16 complex) elements of a cell in the inter-pass buffer, of a signal spectrum
    void (*make_coef_frags)(uint16_t *) = nullptr;  // the column pass's coefficient table (AcqState::pfa_coef) ...
    size_t coef_bytes = 0;                          // ... and its size
    bool chunk_list = false;  // the row pass takes the tapered chunk list (rows_chunk_plan)
    bool masked = false;      // B2a: the second-peak pass is a masked column launch on the main search's cells, so all P x D cells of a run
                              // are ONE launch pair; the Doppler step is p / q spectrum bins and the run holds q signal spectra
};
// The one place that knows which number is which plan: f(Plan{}) of kind 1 .. 4
template <class F>
static void with_npoint(int kind, F &&f) {
    switch (kind) {
    case 1: f(pfa::Plan{}); break;    // B1C, N = 1 987 500 (the default)
    case 2: f(pfa32::Plan{}); break;  // B1C at 53 MS/s
    case 3: f(pfa6::Plan{}); break;   // B2a at 99.375 MS/s, opt-in
    case 4: f(pfa31::Plan{}); break;  // B1C at 30.69 MS/s, opt-in
    }
}
static NPointInfo npoint_info(int kind) {
    NPointInfo i;
    with_npoint(kind, [&](auto plan) {
        using P = decltype(plan);
        i = NPointInfo{kind, P::NP, P::K3, P::kRows, P::kRowsWgs, P::kCellElems, P::kSpecElems, P::make_coef_frags, P::kCoefBytes, P::kChunkList, P::kMasked};
    });
    return i;
}
struct PfaPick {
    int kind = 0;   // NPointInfo::kind
    int shift = 0;  // spectrum bins per Doppler step; a masked plan: p of acqStep N / fs = p / q in lowest terms
    int q = 1;      // a masked plan: signal spectra per call
};
// budget of the inter-pass buffer of one launch pair: the hooks build's BDS_ACQ_PBCAP_GB, else bds_acq_set_pair_budget_gb, else
// BDS_ACQ_PAIR_GB / its default.  GiB as given (< 0: "auto", 0: minimal), and in bytes for a small grid, where 0 counts as 8 GiB.
// "auto" is 60 % of the free device memory, which only AcqRun::setup asks the driver for: here it counts as the 8 GiB too.
static double pair_budget_gb(const bds_ctx *ctx, const AcqState &a) {
    const Tuning &tune = ctx->tune;
    return tune.pbcap_gb > 0 ? tune.pbcap_gb : a.pair_gb_set ? a.pair_gb : tune.pair_gb;
}
static double pair_budget_bytes(const bds_ctx *ctx, const AcqState &a) {
    const double pair_gb = pair_budget_gb(ctx, a);
    return (pair_gb > 0 ? pair_gb : 8.0) * 1073741824.0;
}
// bds_acq_pfa6.h (opt-in, bds_acq_set_b2a_npoint): B2a on N = 53 x 6 x 625 samples (99.375 MS/s), both components, fp16 storage on the 80 x 4096
// plan (whose refinement paths it shares), no resampling, acqStep N / fs = p / q exactly with q <= 5 (B2a/acquisition.m:187-211: bin
// b = q m + j is spectrum j rotated by p m), every rotation below N, all P x D cells in ONE launch pair within the pair budget (the
// second-peak pass reads the winning cells out of the main search's buffer), and the refinement as the device chain.
static PfaPick pfa6_pick(const bds_ctx *ctx, const AcqState &a, const bds_settings &s) {
    PfaPick pk;
    const Tuning &tune = ctx->tune;
    if (!a.b2a_npoint || !tune.pfa || !a.half || a.no_fast_search || a.signal != BDS_SIGNAL_B2A || a.ncomp != 2 || a.rs.on || a.N != pfa6::NP ||
        !a.plan.small || a.skind >= kF64)
        return pk;
    if (tune.neigh != 0 || tune.host_refine || tune.no_bwreuse || tune.nomulti || tune.pbcells > 0) return pk;  // (hooks build: those variants stay L-point)
    long p = 0, q = 0;
    if (!pfa6::step_ratio(s.acqStep, s.samplingFreq, a.N, &p, &q) || q > pfa6::kMaxQ || p < 1) return pk;
    const long D = (long)m_round(s.acqSearchBand * 2 / s.acqStep) + 1;
    if (p * ((D + q - 1) / q) >= a.N) return pk;
    if ((double)s.n_acq * (double)D * (double)pfa6::kCellElems * 4.0 > pair_budget_bytes(ctx, a)) return pk;
    if (fine_pick_lds(s, a.signal, a.ncomp) > kFinePickLdsMax) return pk;  // (device_refine_ok() would send the run to the host path)
    pk.kind = 3, pk.shift = (int)p, pk.q = (int)q;
    return pk;
}
static PfaPick pfa_pick(const bds_ctx *ctx, const AcqState &a, const bds_settings &s) {
    static const int admitted[] = {1, 2, 4};  // the B1C plans, each by its N
    PfaPick pk;
    if (a.signal == BDS_SIGNAL_B2A) return pfa6_pick(ctx, a, s);
    if (!ctx->tune.pfa || !a.half || a.no_fast_search || a.signal != BDS_SIGNAL_B1C || a.ncomp != 2 || a.rs.on || a.skind >= kF64) return pk;
    int kind = 0;
    for (const int k : admitted)
        if (a.N == npoint_info(k).np) kind = k;
    if (kind == 4 && !a.b1c_npoint) kind = 0;  // (opt-in: bds_acq_set_b1c_npoint)
    if (!kind) return pk;
    const double sh = s.acqStep * (double)a.N / s.samplingFreq;
    const long D = (long)m_round(s.acqSearchBand * 2 / s.acqStep) + 1;
    if (!(sh >= 1.0) || sh != std::floor(sh) || sh * (double)D >= (double)a.N) return pk;
    pk.kind = kind, pk.shift = (int)sh;
    return pk;
}

extern "C" int bds_acq_prepare(bds_ctx *ctx, const bds_settings *s_in) {
    if (!ctx || !s_in) return BDS_ERR_ARG;
    if (int rc0 = check_settings(ctx, *s_in)) return rc0;  // (the resampling band edges are only visible here)
    bds_settings eff;
    const bds_settings *s = effective(s_in, &eff);
    int rc = acq_configure(ctx, *s);
    if (rc) return rc;
    AcqState &a = *ctx->acq;
    BDS_HIP(ctx, hipSetDevice(ctx->device));
    Plan2D &pl = a.plan;
    pick_group(a, *s);
    if ((rc = ensure(ctx, &a.d_Bw, &a.bw_cap, bw_batches(a) * (size_t)pl.L))) return rc;
    {   // layout of the cached code spectra: the N-point plan's or the L-point plan's; a change drops the cache
        const NPointInfo want = npoint_info(pfa_pick(ctx, a, *s).kind);
        if (want.kind != a.cs_pfa) a.cs_slot.clear();
        a.cs_pfa = want.kind;
        if (a.half) a.sC = (float)std::exp2(std::floor(std::log2(32768.0 * (double)(want.kind ? a.N : pl.L) / (double)a.X)));
        if (want.kind) {  // its coefficient table (plans with the same first column stage share one)
            uint4 *&d_coef = a.pfa_coef[want.make_coef_frags];
            if (!d_coef) {
                std::vector<uint16_t> cf(want.coef_bytes / 2);
                want.make_coef_frags(cf.data());
                BDS_HIP(ctx, hipMalloc((void **)&d_coef, want.coef_bytes));
                BDS_HIP(ctx, hipMemcpy(d_coef, cf.data(), want.coef_bytes, hipMemcpyHostToDevice));
            }
        }
    }
    std::vector<int> todo;
    for (int i = 0; i < s->n_acq; ++i)
        if (!a.cs_slot.count(s->acqSatelliteList[i]) &&
            std::find(todo.begin(), todo.end(), s->acqSatelliteList[i]) == todo.end())
            todo.push_back(s->acqSatelliteList[i]);
    if (todo.empty()) return BDS_OK;
    RoctxRange rg("acq.prepare (code spectra)");
    const size_t need_slots = a.cs_slot.size() + todo.size();
    if (need_slots > a.cs_cap_slots) {
        // grow: spectra are cheap to rebuild, so drop the cache instead of copying
        for (auto &kv : a.cs_slot)
            if (std::find(todo.begin(), todo.end(), kv.first) == todo.end()) todo.push_back(kv.first);
        a.cs_slot.clear();
        if (a.d_Cs) (void)hipFree(a.d_Cs), a.d_Cs = nullptr;
        hipError_t e = hipMalloc((void **)&a.d_Cs, sizeof(float2) * need_slots * a.ncomp * (size_t)pl.L);
        if (e != hipSuccess) return fail(ctx, BDS_ERR_NOMEM, "code-spectrum cache (%zu PRNs) does not fit: %s", need_slots, hipGetErrorString(e));
        a.cs_cap_slots = need_slots;
    }
    // conj(fft([table zeros]))/L per PRN and component (B2a/acquisition.m:175-184, B1C/acquisition.m:174-187)
    const bool perm = kernel_pick(ctx->tune, a, a.cs_pfa).permuted;  // (the order the search of this configuration reads them in)
    for (int prn : todo) {
        const int slot = (int)a.cs_slot.size();
        CodeLoader ld{a.tab, (prn - 1) * 2};
        // components of one PRN are adjacent code slots: batch index = component
        // half storage: the same byte buffer holds 4-byte elements, so offsets count in those
        float2 *cs_dst = a.half ? (float2 *)((__half2 *)a.d_Cs + (size_t)slot * a.ncomp * pl.L)
                                : a.d_Cs + (size_t)slot * a.ncomp * pl.L;
        if (a.cs_pfa) {  // conj(fft(code)) / N in the CRT layout, [slot][component][53][K2][K3] (the slots keep the L-point stride)
            with_npoint(a.cs_pfa, [&](auto plan) {
                using P = decltype(plan);
                P::forward(st(ctx), ld, a.ncomp, a.d_Bw, (uint32_t *)cs_dst, P::NP, 1, (float)((double)a.sC / (double)a.N), 0);
            });
            BDS_HIP(ctx, hipGetLastError());
        } else if ((rc = forward(ctx, a, ld, a.ncomp, cs_dst, pl.L, 1, (float)((double)a.sC / (double)pl.L), perm)))
            return rc;
        a.cs_slot[prn] = slot;
    }
    BDS_HIP(ctx, hipStreamSynchronize(st(ctx)));
    return BDS_OK;
}

namespace bds {

struct Cell {
    int b;     // 0-based bin
    long lag;  // 0-based
    bool operator<(const Cell &o) const { return std::tie(b, lag) < std::tie(o.b, o.lag); }
};

// sampled code of (slot, mode) for the f64 sums: built once, cached in the context (a.d_codes allocated by the caller)
static void make_code_table(bds_ctx *ctx, AcqState &a, int slot, int mode) {
    const size_t t = (size_t)slot * 2 + mode;
    if (a.code_have[t]) return;
    CodeTable full = a.tab;
    full.xlen = a.spc;  // whole table; the coarse jobs read its first X samples
    const long len = mode ? a.code_stride : a.spc;
    hipLaunchKernelGGL(k_make_code, dim3(256), dim3(256), 0, st(ctx), full, slot, mode, len, a.d_codes + t * (size_t)a.code_stride);
    a.code_have[t] = 1;
}

static int ensure_code_cache(bds_ctx *ctx, AcqState &a, const bds_settings &s) {
    const long stride = a.signal == BDS_SIGNAL_B2A ? std::max<long>(a.spc, (long)s.fineNoncoh * a.spc) : a.spc;
    const size_t ntab = (size_t)BDS_MAX_PRN * 2 * 2;
    if (!a.d_codes || a.code_stride != stride || a.code_have.size() != ntab) {
        if (a.d_codes) (void)hipFree(a.d_codes), a.d_codes = nullptr;
        hipError_t e = hipMalloc((void **)&a.d_codes, ntab * (size_t)stride + 16);  // (+16: k_corr reads whole dwords)
        if (e != hipSuccess) return fail(ctx, BDS_ERR_NOMEM, "sampled-code cache: %s", hipGetErrorString(e));
        a.code_stride = stride;
        a.code_have.assign(ntab, 0);
    }
    return BDS_OK;
}

constexpr int kCorrSlices = 8;  // partial sums per job (k_corr_f64 grid.y)

static int ensure_job_buffers(bds_ctx *ctx, AcqState &a, size_t njobs) {
    if (a.jobs_cap >= njobs) return BDS_OK;
    int rc;
    if (a.d_jobs) (void)hipFree(a.d_jobs), a.d_jobs = nullptr;
    if (a.d_jobout) (void)hipFree(a.d_jobout), a.d_jobout = nullptr;
    size_t cap = std::max<size_t>(njobs, 1024), dummy = 0;
    if ((rc = ensure(ctx, &a.d_jobs, &dummy, cap))) return rc;
    dummy = 0;
    if ((rc = ensure(ctx, &a.d_jobout, &dummy, cap * kCorrSlices * kCorrFreqs))) return rc;
    a.jobs_cap = cap;
    return BDS_OK;
}

// multi: every job carries up to kCorrFreqs frequencies; out[j * kCorrFreqs + f]
// nc: jobs come in groups of nc that differ only in their code slot (the components of one candidate / segment) and are
// summed in one pass (bds_acq_corr.h)
static int run_jobs(bds_ctx *ctx, AcqState &a, const bds_settings &s, std::vector<CorrJob> &jobs,
                    std::vector<double2> &out, int nc, bool multi = false) {
    const int nper = multi ? kCorrFreqs : 1;
    out.resize(jobs.size() * nper);
    if (jobs.empty()) return BDS_OK;
    if (nc < 1 || nc > 2 || jobs.size() % (size_t)nc) return fail(ctx, BDS_ERR_ARG, "run_jobs: %zu jobs in groups of %d", jobs.size(), nc);
    int rc;
    // sampled codes the jobs refer to (built once per (slot, mode), cached in the context)
    if ((rc = ensure_code_cache(ctx, a, s))) return rc;
    for (const CorrJob &j : jobs) make_code_table(ctx, a, j.slot, j.mode);
    constexpr int kSlices = kCorrSlices;
    if ((rc = ensure_job_buffers(ctx, a, jobs.size()))) return rc;
    BDS_HIP(ctx, hipMemcpyAsync(a.d_jobs, jobs.data(), sizeof(CorrJob) * jobs.size(), hipMemcpyHostToDevice, st(ctx)));
    const dim3 grid((unsigned)(jobs.size() / (size_t)nc), kSlices);
    if (multi)
        launch_corr<kCorrFreqs>(st(ctx), grid, a.sview(), nc, a.N, (const int8_t *)a.d_codes, a.code_stride, 1.0 / a.fs, (const CorrJob *)a.d_jobs,
                                a.d_jobout, nullptr, 0);
    else
        launch_corr<1>(st(ctx), grid, a.sview(), nc, a.N, (const int8_t *)a.d_codes, a.code_stride, 1.0 / a.fs, (const CorrJob *)a.d_jobs,
                       a.d_jobout, nullptr, 0);
    BDS_HIP(ctx, hipGetLastError());
    std::vector<double2> part(jobs.size() * kSlices * nper);
    BDS_HIP(ctx, hipMemcpyAsync(part.data(), a.d_jobout, sizeof(double2) * part.size(), hipMemcpyDeviceToHost, st(ctx)));
    BDS_HIP(ctx, hipStreamSynchronize(st(ctx)));
    for (size_t j = 0; j < jobs.size(); ++j)
        for (int f = 0; f < (multi ? jobs[j].nf : 1); ++f) {
            double2 acc = make_double2(0.0, 0.0);  // slices in order, as a single-frequency job adds them
            for (int k = 0; k < kSlices; ++k) acc.x += part[(j * kSlices + k) * nper + f].x, acc.y += part[(j * kSlices + k) * nper + f].y;
            out[j * nper + f] = acc;
        }
    return BDS_OK;
}

static inline double cabs2(double2 v) { return std::hypot(v.x, v.y); }

// results(bin, lag) in f64 from the per-component coherent sums (B2a/acquisition.m:208-209,
// B1C/acquisition.m:212,218-219)
static inline double combine(const AcqState &a, const double2 *v) {
    if (a.signal == BDS_SIGNAL_B2A) return cabs2(v[0]) + cabs2(v[1]);
    if (a.ncomp == 1) return cabs2(v[0]);
    return (cabs2(v[0]) * std::sqrt(11.0) + cabs2(v[1]) * std::sqrt(29.0)) / std::sqrt(40.0);
}

}  // namespace bds

namespace bds {
namespace {

constexpr int kExtraCap = 1 << 22;  // entries of the sieve's candidate list (wave-private pass) / overflow list (tile pass)
constexpr int kSamples = 32;        // launch pairs of a run bracketed by timing events

// packed cell maximum -> (value, 0-based lag); nothing searched / nothing written: (-1, -1)
void unpack_cell(unsigned long long pk, float *v, int *lag) {
    if (pk == 0) {
        *v = -1.f, *lag = -1;
        return;
    }
    const uint32_t hi = (uint32_t)(pk >> 32);
    memcpy(v, &hi, sizeof(float));
    *lag = (int)~(uint32_t)(pk & 0xffffffffu);
}

// What a stage asks of bds_acq_run when the sieve cannot be trusted with the storage / kernels it ran on (never returned
// through the C ABI): redo the call with fp32 storage, or on the run-time-plan kernels (one record per tile, first-index ties)
//  * a non-finite row maximum (an fp16 value overflowed; Parseval bounds every fp16 value by sqrt(L) x its unit RMS < 2^11, so
//    int8 input cannot get here -- kept for non-finite f64 input, exercised by a test hook);
//  * the f64 peak disagrees with the sieve's maximum beyond kDelta / 2: the error model does not hold for this input;
//  * the candidate list ran over: at the fp16 tolerance (a nearly flat surface: an interferer 40 dB above the noise) fp32
//    storage first; with fp32 storage (massive exact ties, e.g. an all-zero block) the run-time-plan kernels.
constexpr int kRedoFp32 = -1000, kRedoPlain = -1001;

// One bds_acq_run attempt: inputs, the quantities its stages share, and the stages in call order.
struct AcqRun {
    bds_ctx *ctx;
    AcqState &a;
    const bds_settings *s;  // effective settings (after the resampling branch)
    std::vector<int> prns;
    double *carrFreq, *codePhase, *peakMetric;
    int32_t *detected;
    std::string why;  // reason of a kRedo* return

    int P = 0, D = 0, G = 0, ncomp = 0;
    double f0 = 0, kDelta = 0;
    float w0 = 1.f, w1 = 1.f;
    KernelPick pick;           // the kernels of this run (kernel_pick) ...
    bool fsearch = false, wcols = false;  // ... of which: pick.fast(), pick.per_cell()
    bool multiprn = false;
    int pfa = 0;               // > 0: an N-point pair runs; the value = spectrum bins per Doppler step
    NPointInfo np;             // which one, and its sizes and properties (kind 0: none)
    int pfa_q = 1;             // a masked plan: pfa = p, pfa_q = q of the Doppler step of p / q bins
    const uint4 *pfa_coef = nullptr;  // its coefficient table (bds_acq_prepare uploaded it)
    size_t cell_elems = 0;     // fp16-complex-sized elements of one cell in the inter-pass buffer (both components)
    bool dev_refined = false;  // the refinement ran as the device chain
    size_t elem = 8;  // bytes of one stored complex value
    int PB = 1;
    long n_pairs_total = 0, cells_per_pair = 0;
    SieveOut so{};
    // timing
    EventPool &evp;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    hipEvent_t sa[kSamples], sb[kSamples], sm[kSamples];
    int nsamp = 0;
    double samp_cells = 0;  // cells of the sampled multi-PRN pairs
    bool mids = false;  // the sampled pairs carry a mid event (fp32-arithmetic kernels)
    // the sieve's output and the decisions made on it
    int n_extra = 0;
    std::vector<Extra> h_extra;
    std::vector<float> thr_of, max_of;
    std::vector<std::vector<Cell>> cells;
    std::vector<PrnResult> res;

    AcqRun(bds_ctx *c, AcqState &st_, const bds_settings *s_) : ctx(c), a(st_), s(s_), evp(st_.events) { evp.rewind(); }
    hipStream_t stream() const { return st(ctx); }
    double bin_freq(int b) const { return f0 + s->acqStep * (double)b; }
    int redo(int code, const char *reason) {
        why = reason;
        return code;
    }

    int setup();        // sizes, work buffers, events, storage scales, the sieve's lists
    int forward_all();  // carrier wipe-off + forward transform of every Doppler bin
    void launch(PairArgs pa, Rec *recs, int cell0, hipEvent_t mid);  // one launch pair of the L-point search
    void launch_cells(int prn, int b0, int nb, Rec *recs, int lo1, int hi1, int lo2, int hi2, int cell0, hipEvent_t mid);
    void launch_list(int ncells, Rec *recs, const CellList &cl, int cell0, hipEvent_t mid);
    int search();          // all (PRN, bin) cells: row pass + column pass per group
    int collect();         // row maxima + list to the host; can the sieve be trusted?
    int refine();          // candidates -> f64 coherent sums -> peak, bin, code phase per PRN
    int metric_b1c_sigpower();
    int metric_b1c();      // GLRT normaliser
    int second_peak_b2a(); // second peak of the winning bin
    int fine_search();     // threshold + fine-Doppler search, results
    int finish();          // timing record
    // the same decisions as collect() .. fine_search() as one chain of launches with a single download (bds_acq_refine.h)
    size_t bw_cells() const;  // cells of this run's pair the inter-pass buffer holds
    bool device_refine_ok() const;
    int refine_device();
};

int AcqRun::setup() {
    Plan2D &pl = a.plan;
    const Tuning &tune = ctx->tune;
    int rc;
    D = (int)m_round(s->acqSearchBand * 2 / s->acqStep) + 1;  // numberOfFrqBins :150
    f0 = s->IF - s->acqSearchBand;                            // frqBins :190-191
    a.D = D;
    P = (int)prns.size();
    ncomp = a.ncomp;
    pick_group(a, *s);
    G = a.group;
    if (a.cs_pfa) {  // (bds_acq_prepare laid the code spectra out for it with these very settings)
        const PfaPick pk = pfa_pick(ctx, a, *s);
        if (a.cs_pfa == pk.kind) pfa = pk.shift, np = npoint_info(pk.kind), pfa_q = pk.q, pfa_coef = a.pfa_coef[np.make_coef_frags];
        // (a masked plan was admitted for the settings' PRN list: a run on a part of it has fewer cells, never more)
    }
    if (a.cs_pfa && !pfa) return fail(ctx, BDS_ERR_HIP, "internal: code spectra in the N-point layout for a run that cannot use them");
    if ((rc = ensure(ctx, &a.d_Bw, &a.bw_cap, bw_batches(a) * (size_t)pl.L))) return rc;
    // (N-point pair: ONE signal spectrum, every row stored twice -- 2 N fp16 complex = N float2-sized elements)
    if ((rc = ensure(ctx, &a.d_Xs, &a.xs_cap, pfa ? (size_t)pfa_q * (size_t)np.np : (size_t)D * pl.L))) return rc;

    BDS_HIP(ctx, evp.make(&ev0));
    BDS_HIP(ctx, evp.make(&ev1));
    BDS_HIP(ctx, evp.make(&ev2));
    BDS_HIP(ctx, evp.make(&ev3));
    for (int i = 0; i < kSamples; ++i) {
        BDS_HIP(ctx, evp.make(&sa[i]));
        BDS_HIP(ctx, evp.make(&sb[i]));
        BDS_HIP(ctx, evp.make(&sm[i]));
    }
    BDS_HIP(ctx, hipEventRecord(ev0, stream()));

    // ---- storage scales (fp16 mode): powers of two from exact sums of the block ----------
    a.sX = a.sB = 1.f;
    if (a.sums_N != a.N || a.sums_next != a.n_ext) ext_sums(a);  // settings of this run changed N after bds_acq_load
    if (a.half) {
        // |X[k]| <= sum|x|  -> keep the stored spectrum below 2^15
        a.sX = (float)std::exp2(std::floor(std::log2(32768.0 / std::max(1.0, a.sum_abs_ext))));
        // inter-pass values: rms = X_rms * C_rms / L * sqrt(L2) (Parseval); allow 64 x rms
        // (N-point pair: transform length N, rows of 3125 points; its row pass has no output scale -- sB rides on the stored signal
        //  spectrum, whose rms stays ~0.2 whatever the block: forward_all)
        const double b_rms = pfa ? std::sqrt(a.sum_sq_ext) * std::sqrt((double)a.X) / (double)a.N * std::sqrt((double)np.k3)
                                 : std::sqrt(a.sum_sq_ext) * std::sqrt((double)a.X) / (double)pl.L * std::sqrt((double)pl.L2);
        a.sB = (float)std::exp2(std::floor(std::log2(32768.0 / (64.0 * std::max(1e-30, b_rms) * a.sX * a.sC))));
    }

    // ---- the search's knobs and lists ------------------------------------------------------
    w0 = w1 = 1.f;
    if (a.signal == BDS_SIGNAL_B1C && ncomp == 2) {
        w0 = (float)(std::sqrt(11.0) / std::sqrt(40.0));
        w1 = (float)(std::sqrt(29.0) / std::sqrt(40.0));
    }
    {   // undo the storage scales in the final magnitude weights
        const float inv = 1.0f / (a.sX * a.sC * a.sB);
        w0 *= inv;
        w1 *= inv;
    }
    pick = kernel_pick(tune, a, np.kind);
    fsearch = pick.fast();  // fp32-arithmetic specialised kernels (default)
    // sieve tolerance: every lag within kDelta of a PRN's maximum is re-evaluated in f64.  fp32 storage (with the fp32 carrier / twiddle
    // rotations of the forward pass, round 4) errs by 5.3e-7 of the PRN maximum at worst against the f64 oracle (tools/sieve_error.py,
    // profiles/r05_sieve_error_small.txt: 19x inside its kDelta / 2 = 1e-5; checked at run time like the fp16 mode).  fp16 storage: three roundings lie between the exact value and the sieve's (signal spectrum, code spectrum,
    // inter-pass buffer; 2^-11 relative each).  On noise-like spectra they average out -- 2.5e-4 of the PRN maximum at worst
    // over 63 x 201 rows -- but a spectrum dominated by ONE line (a CW interferer) carries them coherently: 6.4e-4 / 7.9e-4
    // measured at J/N = +20 / +40 dB (tools/sieve_stress.py, profiles/r04_sieve_error.txt), bounded by 3 x 2^-11 = 1.46e-3.
    // kDelta / 2 = 2e-3 lies above that bound and 2.5x above the worst measured case (round 3 used 2e-3: 1.3x).
    kDelta = tune.kdelta > 0 ? tune.kdelta : a.half ? 4e-3 : 2e-5;
    {
        size_t cap = a.extra_cap;
        if ((rc = ensure(ctx, &a.d_extra, &cap, (size_t)kExtraCap))) return rc;
        a.extra_cap = cap;
        if (!a.d_extra_count) BDS_HIP(ctx, hipMalloc((void **)&a.d_extra_count, sizeof(int)));
        BDS_HIP(ctx, hipMemsetAsync(a.d_extra_count, 0, sizeof(int), stream()));
    }
    // wave-private column pass (default for the fp32-arithmetic search), the 80 x 4096 plan's, an N-point plan's: per-cell packed
    // maxima and per-PRN running bounds instead of per-tile records
    wcols = pick.per_cell();
    so = SieveOut{};
    so.sieve.extra = a.d_extra, so.sieve.extra_count = a.d_extra_count, so.sieve.extra_cap = kExtraCap, so.sieve.keep = (float)(1.0 - kDelta);
    if (wcols) {
        if ((rc = ensure(ctx, &a.d_cellmax, &a.cellmax_cap, (size_t)std::max(P, 1) * D))) return rc;
        if ((rc = ensure(ctx, &a.d_lb, &a.lb_cap, (size_t)std::max(P, 1)))) return rc;
        BDS_HIP(ctx, hipMemsetAsync(a.d_cellmax, 0, sizeof(unsigned long long) * (size_t)std::max(P, 1) * D, stream()));
        BDS_HIP(ctx, hipMemsetAsync(a.d_lb, 0, sizeof(float) * (size_t)std::max(P, 1), stream()));
        so.sieve.cellmax = a.d_cellmax;
        so.sieve.lb = a.d_lb;
        so.sieve.lb_div = D;
    } else {  // per-tile records + per-row reduction (tile kernel, run-time-plan kernels)
        if ((rc = ensure(ctx, &a.d_recs, &a.recs_cap, (size_t)std::max(P, 1) * D * pl.ntiles))) return rc;
        if (a.rows_cap < (size_t)P * D) {
            if (a.d_rowmax) (void)hipFree(a.d_rowmax), a.d_rowmax = nullptr;
            if (a.d_rowarg) (void)hipFree(a.d_rowarg), a.d_rowarg = nullptr;
            size_t d0 = 0, d1 = 0;
            if ((rc = ensure(ctx, &a.d_rowmax, &d0, (size_t)P * D))) return rc;
            if ((rc = ensure(ctx, &a.d_rowarg, &d1, (size_t)P * D))) return rc;
            a.rows_cap = (size_t)P * D;
        }
        so.recs = a.d_recs;
    }
    elem = a.half ? 4 : 8;
    cell_elems = pfa ? np.cell_elems : (size_t)ncomp * pl.L;  // stored complex values of one cell in the inter-pass buffer
    // One launch pair carries the whole Doppler rows of SEVERAL PRNs through a cell list: the grids fill the chip, a row workgroup
    // walks all the bins of one PRN (its code rows and twiddles set up once per D cells), the row workgroups of different PRNs
    // read the same spectrum rows at about the same time, and a call is a few long launches instead of many short ones.
    //   cfg2 (63 PRNs x 26 bins, round 3): 104 cells per pair 3.9 ms, 208 -> 3.6, 416 -> 3.2, 832 -> 3.1, all 1638 -> 3.0.
    //   cfg3 (63 PRNs x 201 bins, round 5, profiles/r05_multiprn_full*.txt, per call on one box): one PRN per pair 197.0 ms,
    //   8 PRNs 197.5, 11 PRNs 199.1 (202.3), 16 PRNs 192.8, 21 PRNs 191.8 (196.7), 32 PRNs 195.0 (202.3) -- 2.5 - 3.6 % for an
    //   inter-pass buffer of 106 - 162 GB, which is what 288 GB of HBM are for.
    // What that costs is memory, and time when it changes hands: a FRESH hipMalloc of 150 GiB takes 0.4 ms on these boxes, but freed
    // device memory is cleared by the driver at ~33 GB/s and an allocation that needs it waits -- 150 GiB allocated again after a free:
    // 4.5 - 4.8 s (tools/probe/alloc_probe.hip, profiles/r05_alloc_probe.txt).  A first call in a fresh process costs the same in both
    // modes (bench.py `cold`: 234 vs 266 ms); a process that builds and destroys contexts, or the next process on the device, pays for
    // the clearing.  So the budget is the deployment's to choose (BDS_ACQ_PAIR_GB / bds_acq_set_pair_budget_gb): the DEFAULT is
    // 40 GiB -- 8 PRNs per pair at cfg3, 2.5 % less time per call than one PRN per pair, a footprint a host can plan with (rounds
    // 1-5 allocated 20 GB whatever the mode) --, "auto" = 60 % of the device memory that is free (counting what this context already
    // holds: 32 + 31 PRNs, 150 GiB, another 2.5 %) is the SERVING mode of a process that keeps the device to itself, 0 the minimal
    // footprint (one PRN's row per pair, 5 GB at cfg3).  With the default budget a big grid is batched only when at least six PRNs
    // fit a pair (fewer gain nothing: 4 PRNs 197.8 against 196.7 ms); an explicit budget batches from two.
    // Small grids (D <= 104: cfg2's 63 x 26 cells are 4.3 GB) batch up to the budget too (8 GiB when the budget is 0).  The PRNs are dealt evenly over the
    // pairs; with room for less than two PRNs' cells a pair is one group of one PRN.
    // (BDS_ACQ_NOMULTI / BDS_ACQ_MULTI_ANY / BDS_ACQ_PBCELLS / BDS_ACQ_PBCAP_GB of the hooks build: off / on / cells per pair / budget.)
    const double pair_gb = pair_budget_gb(ctx, a);
    multiprn = fsearch && P > 1 && !tune.nomulti && (D <= 104 || tune.multi_any || pair_gb != 0);
    PB = 1;
    const double pb_key[6] = {(double)P, (double)D, (double)cell_elems, (double)elem, (double)ncomp, pair_gb + (tune.pbcells ? 1e6 * tune.pbcells : 0)};
    const bool pb_known = multiprn && a.pb_last > 0 && !memcmp(pb_key, a.pb_key, sizeof(pb_key));
    if (pb_known) {
        PB = a.pb_last;
        multiprn = PB >= 2;
    } else if (multiprn) {
        double budget = pair_budget_bytes(ctx, a);
        if (pair_gb < 0) {
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = (size_t)16 << 30;
            budget = 0.6 * ((double)fr + (double)a.bw_cap * sizeof(float2));
        }
        const long pb_cap = (long)(budget / ((double)cell_elems * (double)elem));  // cells
        const long pb_cells = tune.pbcells ? std::min<long>(tune.pbcells, pb_cap) : pb_cap;
        const long pb_max = std::min<long>(P, std::max<long>(D <= 104 ? 2 : 1, pb_cells / D));
        const bool explicit_budget = tune.pbcap_gb > 0 || a.pair_gb_set || tune.pair_gb_env || tune.pbcells > 0 || tune.multi_any;
        if (pb_max < (D <= 104 || explicit_budget ? 2 : 6)) {
            multiprn = false;
        } else {
            const long np_ = (P + pb_max - 1) / pb_max;
            PB = (int)((P + np_ - 1) / np_);
        }
    }
    if (!pb_known && !tune.nomulti && fsearch && P > 1) {
        memcpy(a.pb_key, pb_key, sizeof(pb_key));
        a.pb_last = multiprn ? PB : 1;
    }
    n_pairs_total = (long)P * ((D + G - 1) / G);
    cells_per_pair = G;
    if (multiprn) n_pairs_total = (P + PB - 1) / PB, cells_per_pair = (long)PB * D;
    if (pfa && !multiprn) multiprn = true, PB = 1, n_pairs_total = P, cells_per_pair = D;  // the N-point pair always runs on cell lists
    // (a masked plan was admitted because all cells fit one pair: the second-peak pass reads them there)
    if (np.masked) multiprn = true, PB = P, n_pairs_total = 1, cells_per_pair = (long)P * D;
    return BDS_OK;
}

int AcqRun::forward_all() {
    Plan2D &pl = a.plan;
    if (pfa) {  // ONE transform: the spectrum of bin 0; bin b is its rotation by b * pfa bins (bds_acq_pfa.h)
        SignalLoader ld{a.sview(), a.N, a.n_ext, f0, s->acqStep, 1.0 / a.fs, 0};
        // (a masked plan: q transforms, the bins 0 .. q - 1 -- the loader's batch index is the bin --, one spectrum apart)
        with_npoint(np.kind, [&](auto plan) {
            decltype(plan)::forward(stream(), ld, pfa_q, a.d_Bw, (uint32_t *)a.d_Xs, np.masked ? (long)np.spec_elems : 0, 0, a.sX * a.sB, 1);
        });
        BDS_HIP(ctx, hipGetLastError());
        BDS_HIP(ctx, hipEventRecord(ev1, stream()));
        return BDS_OK;
    }
    const int chunk = (int)bw_batches(a);
    for (int b0 = 0; b0 < D; b0 += chunk) {
        const int nb = std::min(chunk, D - b0);
        SignalLoader ld{a.sview(), a.N, a.n_ext, f0, s->acqStep, 1.0 / a.fs, b0};
        float2 *xs_dst = a.half ? (float2 *)((__half2 *)a.d_Xs + (size_t)b0 * pl.L) : a.d_Xs + (size_t)b0 * pl.L;
        if (int rc = forward(ctx, a, ld, nb, xs_dst, pl.L, 0, a.sX, pick.permuted)) return rc;
    }
    BDS_HIP(ctx, hipEventRecord(ev1, stream()));
    return BDS_OK;
}

// One launch pair of the L-point search on the main stream, with the kernels of `pick`: fills in what every pair of the run shares.
// recs = where a per-tile column pass reports, cell0 = run-wide index of the first cell (list bookkeeping), mid = timing event
// between the passes (or null)
void AcqRun::launch(PairArgs pa, Rec *recs, int cell0, hipEvent_t mid) {
    pa.Xs = a.d_Xs, pa.Bw = a.d_Bw, pa.out_scale = a.sB, pa.w0 = w0, pa.w1 = w1;
    pa.so = so;
    pa.so.recs = recs;
    pa.so.sieve.cell0 = cell0;
    pa.so.mid = mid;
    if (mid && fsearch) mids = true;
    with_storage(a.half, ncomp, [&](auto st_, auto nc) {
        launch_pair<decltype(nc)::value, typename decltype(st_)::type>(ctx, stream(), a.plan, pick, pa);
    });
}

// one group of cells of one PRN: consecutive bins b0 .. b0+nb-1, or one bin with lag ranges
void AcqRun::launch_cells(int prn, int b0, int nb, Rec *recs, int lo1, int hi1, int lo2, int hi2, int cell0, hipEvent_t mid) {
    PairArgs pa;
    pa.G = nb, pa.bin0 = b0;
    pa.Cs = (const char *)a.d_Cs + (size_t)a.cs_slot[prn] * ncomp * a.plan.L * elem;
    pa.lo1 = lo1, pa.hi1 = hi1, pa.lo2 = lo2, pa.hi2 = hi2;
    launch(pa, recs, cell0, mid);
}

// cells described by a list (whole rows of several PRNs, or one (PRN, winning bin) cell per PRN)
void AcqRun::launch_list(int ncells, Rec *recs, const CellList &cl, int cell0, hipEvent_t mid) {
    if (pfa) {  // the N-point pair: every lag of the N is searched, the cells come as a list.  With lag ranges (a masked plan): the masked column
                // pass alone on the cells cl.src names in the main search's buffer, or (no cl.src) behind a row pass of the listed cells
        const hipStream_t s_main = stream();
        SieveOut so1 = so;
        so1.sieve.cell0 = cell0;
        if (mid) mids = true;
        with_npoint(np.kind, [&](auto plan) {
            using P = decltype(plan);
            const auto lds = [&](auto kern, size_t bytes) { want_lds(ctx, kern, bytes); };
            const int gc = cl.rng ? 1 : std::max(1, cl.gc);
            if (!cl.src) {
                typename P::RowsArgs ra{(const uint32_t *)a.d_Xs, (const uint32_t *)a.d_Cs, (uint32_t *)a.d_Bw, cl.bin, cl.cs, ncells, gc, pfa};
                if constexpr (P::kMasked) ra.q = pfa_q;
                if constexpr (P::kChunkList) ra.chunks = cl.chunks, ra.nchunks = cl.nchunks;
                P::launch_rows(s_main, ra, cl.chunks ? cl.nchunks : (ncells + gc - 1) / gc, lds);
            }
            if (mid) (void)hipEventRecord(mid, s_main);
            typename P::ColsArgs ca{(const uint32_t *)a.d_Bw, pfa_coef, ncells, w0, w1, so1.sieve, 0, nullptr};
            if constexpr (P::kMasked)
                ca.rng = cl.rng, ca.src = cl.src;
            else
                ca.dbg_cell = ca.dbg_group = -1;
            const Tuning &tune = ctx->tune;  // (hooks build: tiles per run and workgroups as asked for, at most one workgroup per item)
            P::launch_cols(s_main, ca, tune.pfa_qchunk, std::min<long>(tune.pfa_cgrid, pfa::cols_items(P::kTiles, tune.pfa_qchunk, ncells)), lds);
        });
        return;
    }
    PairArgs pa;
    pa.G = ncells, pa.Cs = a.d_Cs, pa.cl = cl;
    pa.hi1 = (int)a.N - 1;                               // every lag ...
    if (cl.rng) pa.hi1 = -1, pa.lo2 = 0, pa.hi2 = -1;    // ... or the list's ranges
    launch(pa, recs, cell0, mid);
}

int AcqRun::search() {
    Plan2D &pl = a.plan;
    const hipStream_t s_main = stream();
    int rc;
    const long sample_every = std::max<long>(1, n_pairs_total / kSamples);
    long pair_idx = 0;
    if (!multiprn && (rc = ensure_fit(ctx, &a.d_Bw, &a.bw_cap, bw_batches(a) * (size_t)pl.L))) return rc;  // (gives a larger budget's buffer back)
    if (multiprn) {
        // float2-sized elements the PB*D cells of one launch pair occupy; if the device cannot give that much after all (another
        // process took it since setup() asked), halve the PRNs per pair
        for (int tries = 0;; ++tries) {
            const size_t need = ((size_t)PB * D * cell_elems * elem + 7) / 8;
            // (BDS_ACQ_TEST_PAIR_NOMEM of the hooks build: the first n allocations are taken to have failed)
            if (tries < ctx->tune.test_pair_nomem && PB > 2)
                rc = BDS_ERR_NOMEM;
            else if (!(rc = ensure_fit(ctx, &a.d_Bw, &a.bw_cap, std::max(need, bw_batches(a) * (size_t)pl.L))))
                break;
            if (PB <= 2) return rc;
            (void)hipGetLastError();  // (the failed hipMalloc is handled here: it must not surface at the end of the search)
            PB = (PB + 1) / 2;
            a.pb_last = PB;
            n_pairs_total = (P + PB - 1) / PB, cells_per_pair = (long)PB * D;
            if (ctx->tune.verbose) fprintf(stderr, "[bds] inter-pass buffer: allocation failed, %d PRNs per launch pair instead\n", PB);
        }
        const size_t nc_ = (size_t)P * D;
        std::vector<int> h_bin(nc_);
        std::vector<long> h_cs(nc_);
        for (int pi = 0; pi < P; ++pi)
            for (int b = 0; b < D; ++b) {
                h_bin[(size_t)pi * D + b] = b;
                h_cs[(size_t)pi * D + b] = (long)a.cs_slot[prns[pi]] * ncomp * pl.L;
            }
        const char *before = a.d_mcells;
        if ((rc = ensure(ctx, &a.d_mcells, &a.mcells_cap, (sizeof(long) + sizeof(int)) * nc_ + 64))) return rc;
        long *d_cs = (long *)a.d_mcells;
        int *d_bin = (int *)(d_cs + nc_);
        if (a.d_mcells != before || a.mcells_cs != h_cs || a.mcells_bin != h_bin) {  // (the same PRN list call after call: no upload)
            a.mcells_cs.clear(), a.mcells_bin.clear();
            BDS_HIP(ctx, hipMemcpyAsync(d_cs, h_cs.data(), sizeof(long) * nc_, hipMemcpyHostToDevice, s_main));
            BDS_HIP(ctx, hipMemcpyAsync(d_bin, h_bin.data(), sizeof(int) * nc_, hipMemcpyHostToDevice, s_main));
            BDS_HIP(ctx, hipStreamSynchronize(s_main));  // (pageable sources: the copies are done before the vectors go)
            a.mcells_cs = h_cs, a.mcells_bin = h_bin;
        }
        for (int pi0 = 0; pi0 < P; pi0 += PB, ++pair_idx) {
            const int np_ = std::min(PB, P - pi0);
            CellList cl;
            cl.bin = d_bin + (size_t)pi0 * D;
            cl.cs = d_cs + (size_t)pi0 * D;
            // Cells one row workgroup walks: uniform chunks (rows_uniform_gc), or for a plan whose row pass takes it (bds_acq_pfa.h) the
            // tapered list of rows_chunk_plan -- planned and uploaded when a shape is first seen, looked up on every later call.
            // BDS_ACQ_LIST_GC of the hooks build keeps the uniform chunks.
            cl.gc = rows_uniform_gc(ctx->tune.list_gc, D, np_, pfa ? np.rows_wgs : pl.L1);
            if (np.chunk_list && ctx->tune.list_gc == 0) {
                const int slots = 2 * (ctx->n_cu > 0 ? ctx->n_cu : 256);
                AcqState::RowsChunks &rc_ = a.rows_chunks[std::make_tuple(np_, D, slots)];
                if (!rc_.d) {
                    const std::vector<int2> plan = rows_chunk_plan(np_, D, slots, cl.gc);
                    int2 *d_plan = nullptr;
                    BDS_HIP(ctx, hipMalloc((void **)&d_plan, plan.size() * sizeof(int2)));
                    if (hipMemcpy(d_plan, plan.data(), plan.size() * sizeof(int2), hipMemcpyHostToDevice) != hipSuccess) {
                        (void)hipFree(d_plan);
                        BDS_HIP(ctx, hipErrorUnknown);
                    }
                    rc_.d = d_plan, rc_.nchunks = (int)plan.size();
                }
                cl.chunks = rc_.d, cl.nchunks = rc_.nchunks;
            }
            // (a call is a handful of pairs: all of them are timed, the last, shorter one included -- cell_pair_ms and
            //  cells_per_pair are then the means a kernel trace of the call shows)
            const bool sample = (np_ == PB || n_pairs_total <= kSamples) && (pair_idx % sample_every) == 0 && nsamp < kSamples;
            if (sample) BDS_HIP(ctx, hipEventRecord(sa[nsamp], s_main));
            launch_list(np_ * D, wcols ? nullptr : a.d_recs + (size_t)pi0 * D * pl.ntiles, cl, pi0 * D, sample ? sm[nsamp] : nullptr);
            if (sample) {
                BDS_HIP(ctx, hipEventRecord(sb[nsamp++], s_main));
                samp_cells += (double)np_ * D;
            }
        }
    } else {
        for (int pi = 0; pi < P; ++pi) {
            for (int b0 = 0; b0 < D; b0 += G, ++pair_idx) {
                const int nb = std::min(G, D - b0);
                const bool sample = nb == G && (pair_idx % sample_every) == 0 && nsamp < kSamples;
                if (sample) BDS_HIP(ctx, hipEventRecord(sa[nsamp], s_main));
                launch_cells(prns[pi], b0, nb, wcols ? nullptr : a.d_recs + ((size_t)pi * D + b0) * pl.ntiles, 0, (int)a.N - 1, 1, 0,
                             pi * D + b0, sample ? sm[nsamp] : nullptr);
                if (sample) BDS_HIP(ctx, hipEventRecord(sb[nsamp++], s_main));
            }
        }
    }
    BDS_HIP(ctx, hipGetLastError());
    if (!wcols)
        hipLaunchKernelGGL(k_reduce_rows, dim3((unsigned)(P * D)), dim3(256), 0, s_main, (const Rec *)a.d_recs,
                           pl.ntiles, pl.ntiles, a.d_rowmax, a.d_rowarg);
    BDS_HIP(ctx, hipEventRecord(ev2, s_main));
    return BDS_OK;
}

#include "bds_acq_decide.h"  // AcqRun::collect .. fine_search (host path), AcqRun::refine_device (device chain)

int AcqRun::finish() {
    Plan2D &pl = a.plan;
    const Tuning &tune = ctx->tune;
    BDS_HIP(ctx, hipEventRecord(ev3, stream()));
    BDS_HIP(ctx, hipEventSynchronize(ev3));
    for (int pi = 0; pi < P; ++pi) a.last[prns[pi]] = res[pi];

    bds_timing &t = ctx->timing;
    memset(&t, 0, sizeof(t));
    float ms = 0;
    BDS_HIP(ctx, hipEventElapsedTime(&ms, ev0, ev3));
    t.total_ms = ms;
    BDS_HIP(ctx, hipEventElapsedTime(&ms, ev0, ev1));
    t.forward_ms = ms;
    BDS_HIP(ctx, hipEventElapsedTime(&ms, ev1, ev2));
    t.search_ms = ms;
    BDS_HIP(ctx, hipEventElapsedTime(&ms, ev2, ev3));
    t.refine_ms = ms;
    double acc = 0, acc_r = 0, acc_c = 0;
    for (int i = 0; i < nsamp; ++i) {
        BDS_HIP(ctx, hipEventElapsedTime(&ms, sa[i], sb[i]));
        acc += ms;
        if (mids) {
            BDS_HIP(ctx, hipEventElapsedTime(&ms, sa[i], sm[i]));
            acc_r += ms;
            BDS_HIP(ctx, hipEventElapsedTime(&ms, sm[i], sb[i]));
            acc_c += ms;
        }
    }
    t.rows_ms = nsamp && mids ? acc_r / nsamp : 0;
    t.cols_ms = nsamp && mids ? acc_c / nsamp : 0;
    t.n_extra = a.n_extra_last;
    t.shader_clock_GHz = 0;
    if (tune.clockprobe && pl.d_clk) {  // sampled workgroups of the wave-private passes: shader-clock over reference-clock ticks
        unsigned long long h[4];
        int wall_khz = 0;
        BDS_HIP(ctx, hipMemcpy(h, pl.d_clk, sizeof(h), hipMemcpyDeviceToHost));
        BDS_HIP(ctx, hipMemset(pl.d_clk, 0, sizeof(h)));
        BDS_HIP(ctx, hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, ctx->device));
        if (h[1] + h[3]) t.shader_clock_GHz = (double)(h[0] + h[2]) / (double)(h[1] + h[3]) * wall_khz * 1e-6;
    }
    // (no pair was sampled: the average launch-pair duration is the search time over the pair count)
    t.cell_pair_ms = nsamp ? acc / nsamp : (n_pairs_total ? t.search_ms / (double)n_pairs_total : 0);
    t.cells_per_pair = samp_cells > 0 && nsamp ? samp_cells / nsamp : (double)cells_per_pair;
    t.n_pairs = n_pairs_total;
    t.fft_len = pfa ? np.np : pl.L;
    t.n_circ = a.N;
    t.n_bins = D;
    t.n_prn = P;
    t.n_comp = ncomp;
    t.half_storage = a.half ? 1 : 0;  // 0 fp32; 1 fp16 storage (fp32 arithmetic either way)
    t.plan_l1 = pfa ? np.rows : pl.L1;
    t.plan_l2 = pfa ? np.k3 : pl.L2;
    t.refine_path = dev_refined ? 1 : 0;
    // what ran: the pick, as the numbers of include/bds_mi355x.h (the enumerators are those numbers)
    t.rows_kernel = pick.rows;
    t.cols_kernel = pick.cols;
    t.kernel_flags = (pick.ilv ? 1 : 0) | (pick.pk_rows ? 2 : 0);
    return BDS_OK;
}

// one attempt of bds_acq_run with the storage / kernels the context is set to; kRedoFp32 / kRedoPlain: see above
int acq_run_once(bds_ctx *ctx, const bds_settings *s_in, const int32_t *prn_list, int n_prn, int max_prn, double *carrFreq,
                 double *codePhase, double *peakMetric, int32_t *detected, std::string *why) {
    if (int rc0 = check_settings(ctx, *s_in)) return rc0;  // (the resampling band edges are only visible here)
    bds_settings eff;
    const bds_settings *s = effective(s_in, &eff);
    int rc = acq_configure(ctx, *s);
    if (rc) return rc;
    AcqState &a = *ctx->acq;
    if (!a.d_sig || a.n_samples < a.N) return fail(ctx, BDS_ERR_ARG, "bds_acq_run: no IF block loaded (bds_acq_load)");
    if (a.rs.on != resample_plan(*s_in).on || (a.rs.on && a.rs.new_fs != s->samplingFreq))
        return fail(ctx, BDS_ERR_ARG, "bds_acq_run: the loaded block was conditioned for different resampling settings");
    if (a.w16 != (s_in->dataType == 1))
        return fail(ctx, BDS_ERR_ARG, "bds_acq_run: settings.dataType = %d, but the block was loaded as %s samples", (int)s_in->dataType, a.w16 ? "int16" : "int8");
    if ((rc = bds_acq_prepare(ctx, s))) return rc;
    AcqRun r(ctx, a, s);
    if (prn_list && n_prn > 0)
        r.prns.assign(prn_list, prn_list + n_prn);
    else
        r.prns.assign(s->acqSatelliteList, s->acqSatelliteList + s->n_acq);
    int list_max = 0;
    for (int i = 0; i < s->n_acq; ++i) list_max = std::max(list_max, (int)s->acqSatelliteList[i]);
    if (max_prn < list_max) return fail(ctx, BDS_ERR_ARG, "max_prn %d < max(acqSatelliteList) %d", max_prn, list_max);
    for (int p : r.prns)
        if (!a.cs_slot.count(p)) return fail(ctx, BDS_ERR_ARG, "PRN %d of the shard is not in settings.acqSatelliteList", p);
    for (int i = 0; i < max_prn; ++i) {
        carrFreq[i] = codePhase[i] = peakMetric[i] = 0.0;  // acquisition.m:161-165
        if (detected) detected[i] = 0;
    }
    r.carrFreq = carrFreq, r.codePhase = codePhase, r.peakMetric = peakMetric, r.detected = detected;
    RoctxRange whole("bds_acq_run");
    if ((rc = r.setup())) return rc;
    {
        RoctxRange rg("acq.forward");
        if ((rc = r.forward_all())) return rc;
    }
    {
        RoctxRange rg("acq.search");
        if ((rc = r.search())) return rc;
    }
    {
        RoctxRange rg("acq.refine");
        rc = r.device_refine_ok() ? r.refine_device() : kHostRefine;
        r.dev_refined = rc == BDS_OK;
        if (rc == kHostRefine) {  // host path: the lists travel to the host, jobs are built there (rounds 1-4)
            a.cands_on_device = 0;
            if (!(rc = r.collect()) && !(rc = r.refine()) && !(rc = a.signal == BDS_SIGNAL_B1C ? r.metric_b1c() : r.second_peak_b2a()))
                rc = r.fine_search();
        }
        if (!rc) rc = r.finish();
    }
    if (rc == kRedoFp32 || rc == kRedoPlain) *why = r.why;
    return rc;
}

}  // namespace
}  // namespace bds

/* Serving mode of the search (see AcqRun::setup): budget of the inter-pass buffer in GiB; 0 = the minimal footprint (one PRN per pair), < 0 = 60 % of the free device memory; unset: Tuning::pair_gb (40) */
extern "C" int bds_acq_set_pair_budget_gb(bds_ctx *ctx, double gib) {
    if (!ctx) return BDS_ERR_ARG;
    if (!(gib == gib)) return fail(ctx, BDS_ERR_ARG, "bds_acq_set_pair_budget_gb: not a number");
    if (!ctx->acq) ctx->acq = new AcqState();
    ctx->acq->pair_gb = gib;
    ctx->acq->pair_gb_set = true;
    return BDS_OK;
}

/* Opt-in N-point search for the B2a grid at 99.375 MS/s (bds_acq_pfa6.h; pfa6_pick has the conditions).  Takes effect at the next
   bds_acq_prepare / bds_acq_run: the cached configuration -- plan, storage mode, layout of the code spectra -- is re-derived. */
extern "C" int bds_acq_set_b2a_npoint(bds_ctx *ctx, int on) {
    if (!ctx) return BDS_ERR_ARG;
    if (!ctx->acq) ctx->acq = new AcqState();
    if (ctx->acq->b2a_npoint != (on != 0)) {
        ctx->acq->b2a_npoint = on != 0;
        acq_state_invalidate(ctx->acq);
    }
    return BDS_OK;
}

/* Opt-in N-point search for the B1C grid at 30.69 MS/s (bds_acq_pfa31.h; pfa_pick has the conditions).  Takes effect at the next
   bds_acq_prepare / bds_acq_run: the cached configuration -- plan, storage mode, layout of the code spectra -- is re-derived. */
extern "C" int bds_acq_set_b1c_npoint(bds_ctx *ctx, int on) {
    if (!ctx) return BDS_ERR_ARG;
    if (!ctx->acq) ctx->acq = new AcqState();
    if (ctx->acq->b1c_npoint != (on != 0)) {
        ctx->acq->b1c_npoint = on != 0;
        acq_state_invalidate(ctx->acq);
    }
    return BDS_OK;
}

extern "C" int bds_acq_run(bds_ctx *ctx, const bds_settings *s_in, const int32_t *prn_list, int n_prn, int max_prn,
                           double *carrFreq, double *codePhase, double *peakMetric, int32_t *detected) {
    if (!ctx || !s_in || !carrFreq || !codePhase || !peakMetric) return BDS_ERR_ARG;
    // at most three attempts: fp16 storage -> fp32 storage -> run-time-plan kernels
    for (int attempt = 0;; ++attempt) {
        std::string why;
        const int rc = acq_run_once(ctx, s_in, prn_list, n_prn, max_prn, carrFreq, codePhase, peakMetric, detected, &why);
        if (rc != kRedoFp32 && rc != kRedoPlain) return rc;
        if (attempt >= 2) return fail(ctx, BDS_ERR_UNSUPPORTED, "bds_acq_run: the search could not be completed (%s)", why.c_str());
        AcqState &a = *ctx->acq;
        a.fell_back = true;
        const bool plain_kernels = rc == kRedoPlain;
        if (ctx->tune.verbose) fprintf(stderr, "[bds] search re-run (%s): %s\n", plain_kernels ? "run-time-plan kernels" : "fp32 storage", why.c_str());
        if (a.plan.small) {
            // the 80 x 4096 plan has no fp32-storage kernels of its own: re-plan (256 x 1280 for cfg2) so that the re-run takes
            // the specialised fp32 pair instead of the run-time-plan kernels on 80 x 4096
            a.no_small = true;
            a.plan.L = 0;
            bds_settings eff;
            if (int rc2 = acq_configure(ctx, *effective(s_in, &eff))) return rc2;
        }
        a.half = false;
        a.no_fast_search = a.no_fast_search || plain_kernels;
        a.sC = 1.f;
        a.cs_slot.clear();
        // (the flags stay until the configuration changes: acq_configure keeps them for the same key)
        if (int rc2 = bds_acq_prepare(ctx, s_in)) return rc2;
    }
}

extern "C" int bds_resample_plan(const bds_settings *s, double *new_fs, double *new_if, double *wp) {
    if (!s) return BDS_ERR_ARG;
    const ResamplePlan r = resample_plan(*s);
    if (!r.on) return 0;
    if (new_fs) *new_fs = r.new_fs;
    if (new_if) *new_if = r.new_if;
    if (wp) wp[0] = r.wp1, wp[1] = r.wp2;
    return 1;
}

extern "C" int bds_fir1_bandpass(int n_taps, double wp1, double wp2, double *b) {
    if (n_taps < 3 || !b || !(wp1 > 0 && wp1 < wp2 && wp2 < 1)) return BDS_ERR_ARG;
    const std::vector<double> h = fir1_bandpass(n_taps, wp1, wp2);
    std::copy(h.begin(), h.end(), b);
    return BDS_OK;
}

extern "C" int bds_acquire(bds_ctx *ctx, const bds_settings *s, const int8_t *samples, size_t n_samples,
                           int is_complex, int max_prn, double *carrFreq, double *codePhase, double *peakMetric,
                           int32_t *detected) {
    int rc = bds_acq_load(ctx, s, samples, n_samples, is_complex);
    if (rc) return rc;
    if ((rc = bds_acq_prepare(ctx, s))) return rc;
    return bds_acq_run(ctx, s, nullptr, 0, max_prn, carrFreq, codePhase, peakMetric, detected);
}

extern "C" int bds_acquire16(bds_ctx *ctx, const bds_settings *s, const int16_t *samples, size_t n_samples,
                             int is_complex, int max_prn, double *carrFreq, double *codePhase, double *peakMetric,
                             int32_t *detected) {
    int rc = bds_acq_load16(ctx, s, samples, n_samples, is_complex);
    if (rc) return rc;
    if ((rc = bds_acq_prepare(ctx, s))) return rc;
    return bds_acq_run(ctx, s, nullptr, 0, max_prn, carrFreq, codePhase, peakMetric, detected);
}

extern "C" int bds_acq_grid(bds_ctx *ctx, float *row_max, int32_t *row_arg, int cap) {
    if (!ctx || !ctx->acq) return BDS_ERR_ARG;
    AcqState &a = *ctx->acq;
    const int n = (int)a.h_rowmax.size();
    if (cap < n) return fail(ctx, BDS_ERR_ARG, "bds_acq_grid: capacity %d < %d", cap, n);
    for (int i = 0; i < n; ++i) {
        if (row_max) row_max[i] = a.h_rowmax[i];
        if (row_arg) row_arg[i] = a.h_rowarg[i] + 1;  // 1-based like the reference
    }
    return n;
}

// Test aid (bds_acq_block): the host copy of the float64 block of the last load, as it is held.
extern "C" int bds_acq_block(bds_ctx *ctx, double *re, double *im, size_t cap, long long *n) {
    if (!ctx || !ctx->acq || !re || !n) return BDS_ERR_ARG;
    const AcqState &a = *ctx->acq;
    if (a.n_samples <= 0) return fail(ctx, BDS_ERR_ARG, "bds_acq_block: no block loaded (bds_acq_load first)");
    if (a.skind < kF64) return fail(ctx, BDS_ERR_ARG, "bds_acq_block: the loaded block is an int8 one, there is no float64 block");
    const size_t len = (size_t)a.n_samples;
    if (a.h_re.size() != len || (a.cplx && a.h_im.size() != len))
        return fail(ctx, BDS_ERR_ARG, "bds_acq_block: no block loaded (the last bds_acq_load failed)");
    if (a.cplx && !im) return fail(ctx, BDS_ERR_ARG, "bds_acq_block: the block is complex, im must not be NULL");
    if (cap < len) return fail(ctx, BDS_ERR_ARG, "bds_acq_block: capacity %zu < %zu samples", cap, len);
    std::copy(a.h_re.begin(), a.h_re.end(), re);
    if (a.cplx) std::copy(a.h_im.begin(), a.h_im.end(), im);
    *n = (long long)len;
    return a.cplx ? 1 : 0;
}

extern "C" int bds_acq_candidates(bds_ctx *ctx, int prn, int32_t *bin, int64_t *lag, int cap) {
    if (!ctx || !ctx->acq) return BDS_ERR_ARG;
    if (ctx->acq->cands_on_device > 0) {  // the device refinement chain keeps its candidates on the device: fetched when asked for
        bds::AcqState &a = *ctx->acq;
        std::vector<bds::RefCand> h((size_t)a.cands_on_device);
        (void)hipSetDevice(ctx->device);
        if (hipMemcpy(h.data(), a.d_ref_cand, sizeof(bds::RefCand) * h.size(), hipMemcpyDeviceToHost) != hipSuccess)
            return bds::fail(ctx, BDS_ERR_HIP, "bds_acq_candidates: download failed");
        a.last_cands.clear();
        for (const bds::RefCand &c : h)
            if (c.pi >= 0 && c.pi < (int)a.cands_prns.size()) a.last_cands[a.cands_prns[(size_t)c.pi]].push_back({c.b, (long)c.lag});
        for (auto &kv : a.last_cands) std::sort(kv.second.begin(), kv.second.end());
        a.cands_on_device = 0;
    }
    auto it = ctx->acq->last_cands.find(prn);
    if (it == ctx->acq->last_cands.end()) return 0;
    const int n = (int)it->second.size();
    for (int i = 0; i < n && i < cap; ++i) {
        if (bin) bin[i] = it->second[(size_t)i].first + 1;   // 1-based like the reference's indices
        if (lag) lag[i] = it->second[(size_t)i].second + 1;
    }
    return n;
}

extern "C" int bds_acq_coherent_sums(bds_ctx *ctx, const bds_settings *s_in, int prn, int64_t phase, const double *freqs, int nf, int mode,
                                     double *out, int cap) {
    using namespace bds;
    if (!ctx || !ctx->acq || !s_in || !freqs || !out || nf < 1 || nf > 4096 || mode < 0 || mode > 2 || prn < 1 || prn > BDS_MAX_PRN || cap < 0)
        return BDS_ERR_ARG;
    AcqState &a = *ctx->acq;
    bds_settings eff;
    const bds_settings *s = effective(s_in, &eff);
    if (a.n_samples <= 0 || a.spc <= 0) return fail(ctx, BDS_ERR_ARG, "bds_acq_coherent_sums: no block loaded (bds_acq_load / bds_acq_run first)");
    (void)hipSetDevice(ctx->device);
    const bool b1c = a.signal == BDS_SIGNAL_B1C;
    const int nc = b1c ? a.ncomp : 2;
    {  // (re, im) pairs the call writes: nothing is written when `out` cannot hold them (round 6: the entry had no capacity argument)
        const long need = mode == 0 ? (long)nf * a.ncomp : (long)(b1c ? 1 : s->fineNoncoh) * nc * nf;
        if (need > cap) return fail(ctx, BDS_ERR_ARG, "bds_acq_coherent_sums: out holds %d (re, im) pairs, the call writes %ld", cap, need);
    }
    std::vector<CorrJob> jobs;
    std::vector<double2> jout;
    int rc;
    if (mode == 0) {
        // the coarse cell (frequency, code phase): acquisition.m:194-209 -- circular, X samples, the sampled code table
        if (phase < 1 || phase > a.N) return BDS_ERR_ARG;
        for (int f = 0; f < nf; ++f)
            for (int c = 0; c < a.ncomp; ++c) {
                CorrJob j{};
                j.start = phase - 1, j.len = a.X, j.freq = freqs[f], j.slot = (prn - 1) * 2 + c, j.circ = 1, j.mode = 0;
                jobs.push_back(j);
            }
        if ((rc = run_jobs(ctx, a, *s, jobs, jout, a.ncomp))) return rc;
        for (size_t i = 0; i < jout.size(); ++i) out[2 * i] = jout[i].x, out[2 * i + 1] = jout[i].y;
        return (int)jout.size();
    }
    // the fine-search block starting at code phase `phase` (B2a/acquisition.m:287-316, B1C/acquisition.m:253-287)
    const int nseg = b1c ? 1 : s->fineNoncoh;
    const long blk = (long)nseg * a.spc;
    if (phase < 1 || phase - 1 + blk > a.n_samples) return BDS_ERR_ARG;
    double mean = 0, mean_q = 0;
    if (b1c) {
        mean = (a.prefix(phase - 1 + a.spc) - a.prefix(phase - 1)) / (double)a.spc;
        mean_q = a.cplx ? (a.prefix(phase - 1 + a.spc, 1) - a.prefix(phase - 1, 1)) / (double)a.spc : 0.0;
    }
    const bool multi = mode == 1;
    const int per = multi ? kCorrFreqs : 1, nchunk = (nf + per - 1) / per;
    for (int seg = 0; seg < nseg; ++seg)
        for (int ch = 0; ch < nchunk; ++ch)
            for (int c = 0; c < nc; ++c) {
                CorrJob j{};
                j.start = phase - 1 + (long)seg * a.spc, j.len = a.spc, j.code_k0 = b1c ? 0 : (long)seg * a.spc;
                j.mean = mean, j.mean_q = mean_q, j.slot = (prn - 1) * 2 + c, j.circ = 0, j.mode = b1c ? 0 : 1;
                j.nf = std::min(per, nf - ch * per);
                for (int f = 0; f < j.nf; ++f) j.fr[f] = freqs[ch * per + f];
                j.freq = j.fr[0];
                jobs.push_back(j);
            }
    if ((rc = run_jobs(ctx, a, *s, jobs, jout, nc, multi))) return rc;
    // out[((seg * nc + c) * nf + f) * 2 + {re, im}]
    for (int seg = 0; seg < nseg; ++seg)
        for (int c = 0; c < nc; ++c)
            for (int f = 0; f < nf; ++f) {
                const size_t j = ((size_t)seg * nchunk + f / per) * nc + c;
                const double2 v = jout[j * per + f % per];
                out[(((size_t)seg * nc + c) * nf + f) * 2] = v.x, out[(((size_t)seg * nc + c) * nf + f) * 2 + 1] = v.y;
            }
    return nseg * nc * nf;
}

extern "C" int bds_acq_peaks(bds_ctx *ctx, int max_prn, double *peak, double *denom, int32_t *fbin) {
    if (!ctx || !ctx->acq) return BDS_ERR_ARG;
    for (int i = 0; i < max_prn; ++i) {
        if (peak) peak[i] = 0;
        if (denom) denom[i] = 0;
        if (fbin) fbin[i] = 0;
    }
    for (auto &kv : ctx->acq->last) {
        if (kv.first > max_prn) continue;
        if (peak) peak[kv.first - 1] = kv.second.peak;
        if (denom) denom[kv.first - 1] = kv.second.denom;
        if (fbin) fbin[kv.first - 1] = kv.second.fbin;
    }
    return BDS_OK;
}

#include "bds_acq_deep.h"  // bds_acq_deep*: non-coherent power sums over K code periods on the run-time-plan kernels above

BDS_DEBUG_TU_READER(bds_debug_failures_acq)
