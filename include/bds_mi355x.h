/*
 * bds_mi355x.h -- C ABI of libbds_mi355x.so: MI355X (gfx950) acquisition and
 * tracking correlators for BDS-3 B1C / B2a.
 *
 * The reference (lyf8118/BDS-3-B1C-B2a-SDR-receiver) is pure MATLAB and has no
 * FFI layer of its own; the drop-in boundary is the MATLAB call surface used by
 * postProcessing.m.  Every entry point below names the reference interface it
 * replaces (paths relative to /root/reference/BDS3_B1C_B2a).  The MEX gateway
 * (mex/bds_mex.c) and the ctypes host layer (bds_amd/native.py) bind exactly
 * these symbols.  Plain pointers and sizes only; all buffers are caller-owned
 * host memory unless stated.
 *
 * Conventions: every function returning int returns 0 on success, <0 on error
 * (BDS_ERR_*); bds_last_error() gives the message.  Indices that the reference
 * reports 1-based (codePhase) stay 1-based; absoluteSample stays 0-based.
 */
#ifndef BDS_MI355X_H
#define BDS_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BDS_API __attribute__((visibility("default")))

#define BDS_MAX_PRN 63

enum { BDS_SIGNAL_B1C = 1, BDS_SIGNAL_B2A = 2 };
/* tracking variant: B2a/tracking.m | B1C/NB_tracking.m | B1C/WB_tracking.m */
enum { BDS_TRACK_B2A = 0, BDS_TRACK_NB = 1, BDS_TRACK_WB = 2 };
/* bds_gen_code kinds */
enum {
    BDS_CODE_DATA_PRIMARY = 0,  /* 10230 chips (+-1)                                        */
    BDS_CODE_PILOT_PRIMARY = 1, /* 10230 chips                                               */
    BDS_CODE_DATA_BOC11 = 2,    /* B1C only, 20460 half-chips   generateDataBOC11.m:85-91    */
    BDS_CODE_PILOT_BOC11 = 3,   /* B1C only, 20460              generatePilotBOC11.m:88-94   */
    BDS_CODE_PILOT_BOC61 = 4,   /* B1C only, 122760             generatePilotBOC61.m:89-96   */
    BDS_CODE_PILOT_SECONDARY = 5 /* B1C only, 1800 chips         generate2ndCode.m:59-84      */
};

enum {
    BDS_OK = 0,
    BDS_ERR_ARG = -1,         /* bad argument / settings field                    */
    BDS_ERR_HIP = -2,         /* HIP runtime error                                */
    BDS_ERR_UNSUPPORTED = -3, /* valid in the reference, not built yet            */
    BDS_ERR_IO = -4,          /* file open/read failure (fopen error, B2a/postProcessing.m:152-154) */
    BDS_ERR_NOMEM = -5
};

/*
 * Flat mirror of the `settings` struct fields the acquisition/tracking path
 * reads (B1C/initSettings.m:48-151, B2a/initSettings.m:44-130).
 * Field names are the MATLAB names.
 */
typedef struct bds_settings {
    int32_t signal; /* BDS_SIGNAL_*: which receiver directory the struct came from */
    int32_t fileType;              /* 1 = real, 2 = interleaved I/Q (int8, or int16 with dataType 1), 3 = packed 2+2-bit I/Q (below) */
    double samplingFreq;           /* [Hz] */
    double IF;                     /* [Hz] */
    double codeFreqBasis;          /* [Hz] */
    double carrFreqBasis;          /* [Hz] (B1C preRun Doppler aiding)               */
    int32_t codeLength;            /* [chips] 10230                                  */
    int32_t numberOfChannels;
    int64_t skipNumberOfBytes;
    double msToProcess;            /* [ms] */
    /* acquisition */
    double acqSearchBand;          /* [Hz] half width                                */
    double acqStep;                /* [Hz] */
    double acqThreshold;
    double acqCohT;                /* [ms] B1C only                                  */
    int32_t pilotACQflag;          /* B1C only                                       */
    int32_t fineNoncoh;            /* B2a only: code periods in the fine search      */
    double resamplingThreshold;
    int32_t resamplingflag;        /* 1: condition + resample when fs > threshold   */
    int32_t n_acq;                 /* length of acqSatelliteList                     */
    int32_t acqSatelliteList[BDS_MAX_PRN];
    /* tracking */
    int32_t pilotTRKflag;          /* B2a 0/1; B1C 0 / 1 (NB) / 2 (WB)               */
    double intTime;                /* [s] */
    double dllCorrelatorSpacing;   /* [chips] */
    double dllDampingRatio;
    double dllNoiseBandwidth;      /* [Hz] */
    double pllNoiseBandwidth;      /* [Hz] */
    int32_t CNoInterval;
    int32_t dataType;              /* settings.dataType of fread(fid, n, settings.dataType) (B2a/tracking.m:237-238):
                                      0 = 'schar' (int8 samples), 1 = 'int16' ('short': little-endian two's complement,
                                      full range; "16-bit records" below); with fileType 3 only 0 (else BDS_ERR_ARG);
                                      anything else is rejected with BDS_ERR_UNSUPPORTED                     */
    double FEBW;                   /* [Hz] B1C WB only (CalcWeighingFactor.m:46)     */
} bds_settings;

/* channel(1 x nCh) of preRun.m:46-56 */
typedef struct bds_channel {
    int32_t PRN;          /* 0 = unused */
    int32_t status;       /* '-' or 'T' */
    double acquiredFreq;  /* [Hz] */
    double codePhase;     /* 1-based sample */
    double codeFreq;      /* [Hz] */
} bds_channel;

/*
 * trackResults(1 x nCh) of B2a/tracking.m:48-96 / B1C/WB_tracking.m:53-112 as
 * structure-of-arrays: every pointer is caller-allocated double[n_ch * n_epochs]
 * (channel-major) except the C/N0 arrays, double[n_ch * n_cno], and
 * `completed`/`status`.  Pointers of fields the selected variant does not create
 *  may be NULL.  The library initialises the arrays the way
 * the reference template does (zeros / inf) before tracking.
 */
typedef struct bds_track_out {
    int32_t n_ch, n_epochs, n_cno, reserved0;
    double *absoluteSample, *codeFreq, *carrFreq;
    double *I_P, *I_E, *I_L, *Q_E, *Q_P, *Q_L;
    double *Pilot_I_P, *Pilot_Q_P;                         /* pilot tracking on     */
    double *Pilot_I_E, *Pilot_I_L, *Pilot_Q_E, *Pilot_Q_L; /* WB only               */
    double *dllDiscr, *dllDiscrFilt, *pllDiscr, *pllDiscrFilt;
    double *remCodePhase, *remCarrPhase;
    double *DataCNo, *DataPLD, *PilotCNo, *PilotPLD, *SigCNo; /* SigCNo = B1C_CNo | B2a_CNo */
    int32_t *completed; /* [n_ch] epochs finished per channel                        */
    int32_t *status;    /* [n_ch] '-' or 'T' (B2a/tracking.m:48,441)                 */
} bds_track_out;

/* per-stage device timing of the last bds_acq_run / bds_track call (hipEvent, ms) */
typedef struct bds_timing {
    double total_ms;        /* whole call, stream time                              */
    double forward_ms;      /* wipe-off + forward transforms, all bins              */
    double search_ms;       /* all (PRN, bin) cells: multiply + inverse + |.| max   */
    double refine_ms;       /* f64 re-evaluation of candidate cells + fine search   */
    double cell_pair_ms;    /* average duration of one (rows+cols) launch pair, sampled */
    double cells_per_pair;  /* (PRN, bin) cells one launch pair processes           */
    int64_t n_pairs;        /* launch pairs in the call                             */
    int64_t fft_len;        /* padded transform length L                            */
    int64_t n_circ;         /* N: the reference's circular correlation length       */
    int32_t n_bins, n_prn, n_comp;
    int32_t half_storage;   /* 0: fp32 search on fp32 storage; 1: fp32 arithmetic, spectra + inter-pass buffer
                               held as fp16 complex (default)                                           */
    double rows_ms;         /* average duration of the row-pass kernel of a sampled launch pair        */
    double cols_ms;         /* ... and of its column-pass kernel                                       */
    int64_t n_extra;        /* entries of the sieve's overflow list in the last search                 */
    double shader_clock_GHz; /* engine clock the search kernels ran at (sampled workgroups time themselves with the shader
                                clock against the reference clock); 0 unless BDS_ACQ_CLOCKPROBE=1              */
    int32_t plan_l1, plan_l2; /* two-pass factorisation of fft_len: column length x row length                          */
    int32_t rows_kernel;    /* row pass of the search: 0 run-time plan (k_rows_inv), 1 k_rows_inv_f, 2 k_rows_wave_f, 3 N-point pair: k_pfa_rows (fft_len 1 987 500 = 53 x 12 x 3125, B1C at 99.375 MS/s), k_pfa32_rows (fft_len 1 060 000 = 53 x 32 x 625, B1C at 53 MS/s), k_pfa6_rows (fft_len 198 750 = 53 x 6 x 625, B2a at 99.375 MS/s, bds_acq_set_b2a_npoint) or k_pfa31_rows (fft_len 613 800 = 31 x 11 x 1800, B1C at 30.69 MS/s, bds_acq_set_b1c_npoint) */
    int32_t cols_kernel;    /* column pass: 0 run-time plan (k_cols_inv_max), 1 tile kernel k_cols_inv_max_f, 2 k_cols_wave_f, 3 k_cols_small_f, 4 k_pfa_cols / k_pfa32_cols / k_pfa6_cols */
    int32_t kernel_flags;   /* bit 0: components interleaved in the inter-pass buffer; bit 1: packed-fp32 butterflies     */
    int32_t refine_path;     /* 1: candidates -> f64 sums -> peak / second peak / fine search as one device chain with a single download (csrc/bds_acq_refine.h); 0: through the host */
} bds_timing;

typedef struct bds_ctx bds_ctx;

/* ---- context ---------------------------------------------------------------- */
/* One context per GPU (one process per GPU under torch.distributed / RCCL). */
BDS_API bds_ctx *bds_create(int device_id);
BDS_API void bds_destroy(bds_ctx *ctx);
/* Environment knobs, read once at bds_create into the context.  The release library reads exactly these:
 *   BDS_ACQ_FP16=0       fp32 storage of the spectra and the inter-pass buffer as well (default: fp16 storage; every reported
 *                        value is decided in f64 either way)
 *   BDS_TRK_PREC=0..5    numerics of the tracking correlator: 4 (default) a sin / cos of the reference's own carrier argument
 *                        trigarg(k) per sample in f64 -- correlator sums 1e-13 of |P| from the float64 oracle, the loop state
 *                        bit-identical for hundreds of epochs, SURVEY.md 8d until a channel's first ceil() flip (cfg4 at full
 *                        rate: 11 of 12 channels over all 3 600 epochs); 5: the same argument by angle addition (one sin / cos
 *                        per 16 samples), 12 % faster, 4e-10 of |P| (6 of 12 channels); 0: fp32 carrier recurrence, ~1.5x
 *                        faster in wide-band mode, first flip after a few hundred epochs
 *   BDS_VERBOSE          progress / fallback messages on stderr
 *   BDS_ACQ_CLOCKPROBE=1 sampled workgroups time themselves with the shader clock (bds_timing.shader_clock_GHz)
 *   BDS_ACQ_PAIR_GB=n|auto budget of the search's inter-pass buffer in GiB: several PRNs' Doppler rows per launch pair (default 40;
 *                        "auto": 60 % of the free device memory, the serving mode; 0: minimal).  See bds_acq_set_pair_budget_gb.
 * (plus BDS_MEX_DEVICES in the MEX gateway and BDS_LIB_PATH in the ctypes host).  Kernel-selection, launch-shape and sieve
 * switches, the RCCL path override and the aliased-device hook exist only in libbds_mi355x_hooks.so (-DBDS_TEST_HOOKS,
 * built beside the release library by build.sh; tools/README.md lists them), which is what tests/ load.
 * bds_reload_tuning re-reads the knobs into an existing context and makes the next bds_acq_prepare re-derive the
 * acquisition configuration (plan, storage mode, cached code spectra).  Never needed by a host application. */
BDS_API int bds_reload_tuning(bds_ctx *ctx);
BDS_API const char *bds_last_error(const bds_ctx *ctx); /* ctx may be NULL: creation errors */
BDS_API int bds_device_name(const bds_ctx *ctx, char *buf, int buflen);
/* Binding self-check: returns 0 when the caller's struct sizes equal the library's. */
BDS_API int bds_abi_check(int sizeof_settings, int sizeof_channel, int sizeof_track_out, int sizeof_timing);
/* Which build this is: bit 0 = test hooks compiled in (libbds_mi355x_hooks.so), bit 1 = debug build (device-side bounds checks). */
BDS_API int bds_build_flags(void);

/* ---- ranging codes (host side, no GPU needed) -------------------------------- */
/* Replaces generateB2aDataCode.m / generateB2aPilotCode.m / generateDataBOC11.m /
 * generatePilotBOC11.m / generatePilotBOC61.m.  Writes +-1 into out[0..n); returns
 * the code length, or <0.  n must be >= the code length. */
BDS_API int bds_gen_code(int signal, int kind, int prn, int8_t *out, int n);

/* ---- acquisition -------------------------------------------------------------
 * acqResults = acquisition(longSignal, settings)
 *   B2a/acquisition.m:1, B1C/acquisition.m:1, B1C/GPU_acquisition.m:1
 * samples: int8 IF samples as fread(...,'schar') delivers them
 *   (B2a/postProcessing.m:89-90, B1C/postProcessing.m:94); n_samples real samples
 *   (or I/Q pairs when is_complex == 1, fileType 2).
 * Packed records: settings.fileType == 3 (tracking) and is_complex == 2 (acquisition) mean the input format of
 *   B2a/include/unpack_cplx.m:18-30 -- one byte holds two complex samples, 2-bit sign/magnitude I and Q each.  Complex sample n
 *   (0-based) is nibble n & 1 of byte n >> 1, low nibble first; within a nibble bit 0 = I negative, bit 1 = Q negative,
 *   bit 2 = |I| is 3 (else 1), bit 3 = |Q| is 3 (else 1).  `samples` then points at ceil(n_samples / 2) packed bytes (for an odd
 *   n_samples the last high nibble is ignored); in tracking everything that is counted in samples stays in samples (a channel
 *   starts at sample skipNumberOfBytes + codePhase - 1, which may be a high nibble), a file of B bytes holds 2 B samples, and
 *   end of file is judged in samples.  Every output equals, bit for bit, that of the same call with fileType 2 (is_complex 1)
 *   on the int8 pairs bds_unpack_cplx makes of the same bytes; bds_track_loaded_bytes / bds_track_stream_info count real bytes
 *   (a quarter of the fileType-2 record's), and so does the resident limit.
 * 16-bit records: settings.dataType == 1 means little-endian int16 samples (fileType 1) or interleaved I, Q int16 pairs
 *   (fileType 2).  Positions count SAMPLES, the rule of the packed format: skipNumberOfBytes, codePhase and absoluteSample are
 *   sample counts, a channel starts at sample skipNumberOfBytes + codePhase - 1, a file of B bytes holds B / 2 samples (B / 4
 *   pairs) and end of file is judged in samples.  (The reference's own fseek / ftell arithmetic counts bytes and says so --
 *   "Assumes sample type is schar (or 1 byte per sample)", B2a/tracking.m:151-153,226 -- so with a 2-byte type it would start
 *   every channel at half the intended offset; that is not reproduced.)  A sample enters the arithmetic as the same (double)
 *   value an int8 sample does: a 16-bit record whose values all fit int8 gives every output of the int8 record bit for bit.
 *   Tracking: bds_track, bds_track_mem, bds_track_open*, bds_track_feed*, the *_dev entries and bds_track_correlate take the
 *   record's bytes and need no other entry; a byte count that is not a whole number of samples (2 bytes; 4 for a pair) is
 *   BDS_ERR_ARG; bds_track_loaded_bytes / bds_track_stream_info and the resident limit count real bytes.  The kernels are built
 *   for the default numerics only: in the test-hooks build any BDS_TRK_PREC but 4 with dataType 1 is BDS_ERR_UNSUPPORTED.
 *   Acquisition: the entries typed int8_t (bds_acquire, bds_acq_load, bds_acquire_track, bds_acquire_multi) keep refusing
 *   dataType != 0 (BDS_ERR_UNSUPPORTED); bds_acquire16, bds_acq_load16 and bds_acquire_track16 take int16_t values and need
 *   dataType == 1 (else BDS_ERR_ARG); bds_acq_load_dev goes by settings.dataType.  is_complex == 2 with 16 bits is BDS_ERR_ARG.
 *   COST: a 16-bit block is widened on the device to the float64 block the resampling branch leaves (exact), so its search is
 *   the L-point pair and its refinement the host path (bds_timing.refine_path = 0): the N-point pairs and the device
 *   refinement chain read int8 blocks only.  resamplingflag = 1 works on a 16-bit block as on an int8 one.
 * carrFreq/codePhase/peakMetric: double[max_prn], max_prn >= max(acqSatelliteList);
 *   zero where not searched / not detected (B2a/acquisition.m:161-165).
 * detected (optional, may be NULL): int32[max_prn], 1 where the PRN passed the
 *   threshold -- lets the caller print the reference's "(19 20 . )" line
 *   (B2a/acquisition.m:167,259,360,366).
 */
BDS_API int bds_acquire(bds_ctx *ctx, const bds_settings *s, const int8_t *samples,
                        size_t n_samples, int is_complex, int max_prn, double *carrFreq,
                        double *codePhase, double *peakMetric, int32_t *detected);
/* ... on int16 samples (settings.dataType 1; n_samples samples, or I/Q pairs when is_complex == 1) */
BDS_API int bds_acquire16(bds_ctx *ctx, const bds_settings *s, const int16_t *samples,
                          size_t n_samples, int is_complex, int max_prn, double *carrFreq,
                          double *codePhase, double *peakMetric, int32_t *detected);

/* The same call split in three so that the timed region of a benchmark starts with
 * the IF block resident in HBM and the code spectra cached:
 *   bds_acq_load    H2D copy of the IF block
 *   bds_acq_prepare code spectra for settings.acqSatelliteList (cached in ctx)
 *   bds_acq_run     forward transforms, PRN x Doppler search, refinement, fine search
 * prn_list/n_prn select the PRN shard this rank searches (NULL/0 = acqSatelliteList);
 * outputs are zero for PRNs outside the shard so that an all-reduce(SUM) across
 * ranks reassembles acqResults bit-exactly (x + 0). */
BDS_API int bds_acq_load(bds_ctx *ctx, const bds_settings *s, const int8_t *samples,
                         size_t n_samples, int is_complex);
BDS_API int bds_acq_load16(bds_ctx *ctx, const bds_settings *s, const int16_t *samples,
                           size_t n_samples, int is_complex); /* int16 samples (settings.dataType 1) */
BDS_API int bds_acq_prepare(bds_ctx *ctx, const bds_settings *s);
BDS_API int bds_acq_run(bds_ctx *ctx, const bds_settings *s, const int32_t *prn_list, int n_prn,
                        int max_prn, double *carrFreq, double *codePhase, double *peakMetric,
                        int32_t *detected);
/* Budget of the search's inter-pass buffer: a launch pair (row pass + column pass) carries as many PRNs' Doppler rows as fit
 * `gib` GiB; a call is then a few long launches.  cfg3 (63 PRNs x 201 bins) on one box, round 6 (the N-point pair of
 * csrc/bds_acq_pfa.h: 3.3 GB per PRN; profiles/r06_pfa53_knobs_tiled.txt):
 *     0        one PRN per pair,  3.3 GB    144.6 ms per call     (the minimal footprint)
 *    20        5 - 6 PRNs per pair          132.8
 *    40        12 - 13 PRNs per pair        132.1 - 133.0         (the DEFAULT)
 *    80        21 PRNs per pair             132.8
 *   < 0       60 % of the device memory that is free: 32 + 31 PRNs, 100 GiB    132.2   (the SERVING mode; bench.py key `serving`)
 * B1C at 53 MS/s with the settings of the reference's B1C/initSettings.m (N = 1 060 000 = 53 x 32 x 625) runs on the N-point pair of
 * csrc/bds_acq_pfa32.h: 1.76 GB per PRN of 201 bins.
 * With the L-point pair of rounds 3-5 (5 GB per PRN; every configuration the two N-point pairs do not cover) more PRNs per pair also
 * shared the 2.5 GB of signal-spectrum rows in L2: 196.7 / 191.6 - 192.1 (8 PRNs) / 189.3 - 189.8 / 186.8 - 187.1 ms.
 * The price is the footprint, and time when it changes hands: a fresh allocation is free (a first call costs the same in every
 * mode), but the driver clears freed device memory at ~33 GB/s and whoever allocates next waits -- up to ~4.8 s after a 150-GiB
 * context is destroyed.  Results are the same bits in every mode.  Same switch as the environment knob BDS_ACQ_PAIR_GB (number
 * of GiB, or "auto"); takes effect at the next bds_acq_run -- in both directions: a context whose buffer is more than a quarter
 * (+256 MiB) larger than the new budget needs frees it and allocates the smaller one at that run (round 6; until then only
 * bds_destroy returned the memory). */
BDS_API int bds_acq_set_pair_budget_gb(bds_ctx *ctx, double gib);

/* Opt-in N-point search for B2a at 99.375 MS/s (csrc/bds_acq_pfa6.h), default 0 (off): the circular correlation over the reference's
 * own N = 2 code periods = 198 750 = 53 x 6 x 625 samples instead of the zero-padded 327 680.  B2a/acquisition.m:187-211 mixes the
 * block with one carrier per Doppler bin, frqBins(b) = IF - band + acqStep (b - 1); with acqStep N / fs = p / q in lowest terms the
 * spectrum of bin q m + j (0-based) is the spectrum of bin j rotated by p m, so a call transforms q signal blocks (5 at the default
 * 400 Hz step) instead of one per bin.  With the switch on a run takes this pair when ALL of these hold, and the L-point pair -- exactly
 * as with the switch off -- otherwise:
 *   - signal B2a (both components), N = 198 750 (samplingFreq 99.375e6), no resampling, int8 input;
 *   - fp16 storage on the 80 x 4096 plan (the defaults; BDS_ACQ_FP16=0 and every re-run of a call with fp32 storage stay L-point);
 *   - acqStep and samplingFreq whole numbers of hertz with acqStep N / fs = p / q, q <= 5, p >= 1 (400, 250, 500, 1000 Hz; not 410);
 *   - p ceil(bins / q) < N;
 *   - all (PRN of acqSatelliteList) x bin cells fit ONE launch pair within the pair budget (1.66 MB per cell: 2.7 GB for 63 x 26) --
 *     the second-peak pass (acquisition.m:224-249) reads the winning cells out of the main search's buffer;
 *   - the refinement runs as the device chain (bds_timing.refine_path 1).
 * bds_get_timing then reports rows_kernel 3, cols_kernel 4, fft_len 198750, plan_l1 x plan_l2 = 318 x 625.  acqResults are the same
 * numbers either way (they are decided in f64 on the candidates of the search).  Takes effect at the next bds_acq_prepare /
 * bds_acq_run and invalidates the cached configuration as bds_reload_tuning does. */
BDS_API int bds_acq_set_b2a_npoint(bds_ctx *ctx, int on);

/* Opt-in N-point search for B1C at sizes beyond the two that run by default (99.375 and 53 MS/s), default 0 (off).  One size so far:
 * 30.69 MS/s (30 samples per chip, the alternative rate of B1C/initSettings.m:57), N = 20 ms = 613 800 = 31 x 11 x 1800 samples
 * (csrc/bds_acq_pfa31.h): the circular correlation over N instead of the zero-padded L-point pair, all Doppler bins as rotations of ONE
 * signal spectrum.  With the switch on a run takes this pair when ALL of these hold, and the L-point pair -- exactly as with the switch
 * off -- otherwise:
 *   - signal B1C with both components (pilotACQflag 1), N = 613 800 (samplingFreq 30.69e6, acqCohT 10);
 *   - fp16 storage (the default; BDS_ACQ_FP16=0, BDS_ACQ_PFA=0 and every re-run of a call with fp32 storage or on the run-time-plan
 *     kernels stay L-point);
 *   - no resampling;
 *   - an int8 block, real or I/Q (packed 2+2-bit, int16 and resampled blocks stay L-point);
 *   - acqStep N / fs an integer >= 1 (50 Hz: 1, 100 Hz: 2; not 25 Hz) with that shift x bins < N.
 * bds_get_timing then reports rows_kernel 3, cols_kernel 4, fft_len 613800, plan_l1 x plan_l2 = 341 x 1800.  acqResults are the same
 * numbers either way (they are decided in f64 on the candidates of the search).  99.375 and 53 MS/s keep their own pairs whatever the
 * switch says.  Takes effect at the next bds_acq_prepare / bds_acq_run and invalidates the cached configuration as bds_reload_tuning
 * does. */
BDS_API int bds_acq_set_b1c_npoint(bds_ctx *ctx, int on);

/* Diagnostics of the last bds_acq_run: per searched PRN (in search order) and Doppler
 * bin, the maximum of results(bin,:) (fp32 search value) and its 1-based lag.
 * row_max/row_arg: [n_prn * n_bins].  Returns n_prn*n_bins or <0. */
BDS_API int bds_acq_grid(bds_ctx *ctx, float *row_max, int32_t *row_arg, int cap);
/* Diagnostics of the sieve: the (Doppler bin, code phase) cells of `prn` the last bds_acq_run re-evaluated in
 * f64 (1-based, like the reference's indices into results(bin, codePhase)).  Returns their number (may exceed
 * cap).  Tests use it to check that every cell within the sieve tolerance of the maximum was refined. */
BDS_API int bds_acq_candidates(bds_ctx *ctx, int prn, int32_t *bin, int64_t *lag, int cap);
/* Peak / second-peak (B2a) or peak / sigPower (B1C) of the last run, per PRN slot:
 * peak[max_prn], denom[max_prn], fbin[max_prn] (1-based frequency bin). */
BDS_API int bds_acq_peaks(bds_ctx *ctx, int max_prn, double *peak, double *denom, int32_t *fbin);
/* Check entry: the f64 coherent sums the decisions rest on, for caller-chosen cells of the block loaded by the last
 * bds_acq_load / bds_acq_run (csrc/bds_acq_corr.h), as interleaved (re, im) pairs.  Returns the number of pairs or < 0.
 *   mode 0  coarse cell (B2a/acquisition.m:194-209, B1C/acquisition.m:198-219): for each of freqs[0 .. nf) and each component,
 *           sum_n x[(phase-1+n) mod N] code_c(n) exp(+j 2 pi f t/fs), t = the wrapped sample index:  out[(f*ncomp + c)*2]
 *   mode 1  fine-search block starting at code phase `phase` (B2a :287-316: fineNoncoh segments, both components, long code;
 *           B1C :253-287: one code period, DC removed), every frequency of freqs[] in the multi-frequency pass:
 *           out[((seg*ncomp + c)*nf + f)*2]
 *   mode 2  the same sums, one frequency per pass (what mode 1 must agree with to rounding) */
BDS_API int bds_acq_coherent_sums(bds_ctx *ctx, const bds_settings *s, int prn, int64_t phase, const double *freqs, int nf, int mode,
                                  double *out, int cap); /* cap: (re, im) pairs `out` holds; BDS_ERR_ARG, nothing written, if the call needs more */
/* Test aid, never needed by a host application: the float64 block the search reads after the last bds_acq_load / bds_acq_load16 /
 * bds_acq_load_dev -- the output of the resampling branch (fir1 + filtfilt + index decimation, acquisition.m:56-112), or a 16-bit
 * block widened to float64 -- as the library holds it on the host, copied without any arithmetic.  re[cap], im[cap] (im may be NULL
 * for a real block); *n receives the number of samples.  Returns 0 for a real block, 1 for a complex one; BDS_ERR_ARG, nothing
 * written, when the loaded block is an int8 one (no resampling, dataType 'schar'), when nothing is loaded or when cap is smaller than the block.  The
 * tests hold every sample against a float64 restatement of filtfilt. */
BDS_API int bds_acq_block(bds_ctx *ctx, double *re, double *im, size_t cap, long long *n);
BDS_API int bds_get_timing(bds_ctx *ctx, bds_timing *t);

/* ---- multi-device acquisition -------------------------------------------
 * One host process drives N GPUs: what postProcessing.m's single acquisition() call (B1C/postProcessing.m:105-111,
 * B2a/postProcessing.m:100) becomes on a multi-GPU node.  The (signal, PRN) jobs are spread over the devices by cost
 * (bds_shard_jobs: longest-processing-time rule; bds_acq_job_cost: transform points x Doppler bins x components of
 * one PRN), every device searches its shard with the whole IF block, and one RCCL all-reduce(SUM) of
 * 3 x max_prn f64 per signal over xGMI leaves the complete acqResults everywhere (x + 0: bit-identical to one
 * device).  Several signals in one call = BASELINE.json configs[4] (B1C + B2a jointly).
 * Tracking needs no exchange: use bds_multi_ctx(m, i) with bds_track per device (replicas / channel shards). */
typedef struct bds_multi bds_multi;
typedef struct bds_acq_job {
    const bds_settings *settings; /* one receiver's settings (signal, acqSatelliteList, ...)          */
    const int8_t *samples;        /* its IF block (host), as for bds_acquire                           */
    size_t n_samples;
    int32_t is_complex;           /* 0 real, 1 I/Q int8 pairs, 2 packed 2+2-bit I/Q bytes              */
    int32_t max_prn;              /* >= max(acqSatelliteList), <= 63                                   */
    double *carrFreq, *codePhase, *peakMetric; /* out: double[max_prn] each                            */
    int32_t *detected;            /* out, optional: int32[max_prn]                                     */
} bds_acq_job;
/* n_devices <= 0: every visible device; device_ids NULL: 0 .. n_devices-1 */
BDS_API bds_multi *bds_multi_create(int n_devices, const int *device_ids);
BDS_API void bds_multi_destroy(bds_multi *m);
BDS_API const char *bds_multi_last_error(const bds_multi *m); /* m may be NULL: creation errors */
BDS_API int bds_multi_size(const bds_multi *m);
BDS_API bds_ctx *bds_multi_ctx(bds_multi *m, int i);
/* communicator size RCCL reported at the last all-reduce (0: none has run) */
BDS_API int bds_multi_rccl_ranks(const bds_multi *m);
BDS_API int bds_acquire_multi(bds_multi *m, int n_signals, const bds_acq_job *signals);
/* rank_of_job[j] in 0..world-1 for jobs of relative cost[j] (no GPU needed) */
BDS_API int bds_shard_jobs(int n_jobs, const double *cost, int world, int32_t *rank_of_job);
BDS_API double bds_acq_job_cost(const bds_settings *s);

/* ---- tracking -----------------------------------------------------------------
 * [trackResults, channel] = tracking(fid, channel, settings)
 *   B2a/tracking.m:1, B1C/NB_tracking.m:1, B1C/WB_tracking.m:1
 * The reference seeks absolutely from 'bof' (B2a/tracking.m:151-153), so the MATLAB
 * wrapper passes the file *path* (fopen(fid)) instead of the handle.
 * Returns 0 also when the file ends early: like B2a/tracking.m:250-254 the results
 * gathered so far are returned, `completed[ch]` says how far each channel got and
 * status stays '-' for the channel that hit EOF and all later ones.
 */
BDS_API int bds_track(bds_ctx *ctx, const bds_settings *s, const char *path, int n_ch,
                      const bds_channel *channel, bds_track_out *out);
/* Same, on an IF record already in host memory (n_bytes raw file bytes; fileType 3: packed bytes, 2 n_bytes samples). */
BDS_API int bds_track_mem(bds_ctx *ctx, const bds_settings *s, const int8_t *file_bytes,
                          size_t n_bytes, int n_ch, const bds_channel *channel,
                          bds_track_out *out);
/* Bytes of the IF record the last bds_track / bds_track_mem call copied host-to-device.  One window (the default when it
 * fits): only the window the channels can touch (earliest start sample .. latest start + msToProcess at a code rate 2 % low)
 * is loaded, so a recording far longer than msToProcess tracks fine.  Streamed (below): the total over all pieces, which is
 * about that window -- what consecutive pieces share moves device-to-device and is not loaded again.  (Bytes are counted when
 * they are copied.  A piece is loaded ahead to where the channels are predicted to be; should a channel's code rate leave the
 * +-2 % the prediction allows, that piece is discarded and its part of the record is loaded, and counted, a second time.)
 * End-of-file is always judged against the real file size. */
BDS_API long long bds_track_loaded_bytes(bds_ctx *ctx);
/* Streamed tracking.  A window that cannot be allocated, or that is larger than the resident limit, is not held whole: the
 * record passes through a resident span in HBM in successive pieces, the next piece loading (host thread, second stream)
 * while the epochs of the current one run, so a run may be as long as the file.  The kernels, the samples, the order of the
 * partial sums and the loop state are those of the one-window path: the results are the same bit for bit.
 * bds_track_set_resident_limit: at most `bytes` of the record are resident (two span buffers of half that each) in the
 *   bds_track / bds_track_mem / bds_acquire_track calls that follow on this context; 0 (the default) = no limit: one window
 *   when its allocation succeeds, streamed when it fails.  A limit at or above the window changes nothing.  A limit too
 *   small for the channels' spread of positions plus one block per span buffer makes the tracking call return BDS_ERR_ARG
 *   with the minimum in the message.
 * bds_track_stream_info: of the last tracking call, the pieces loaded (1 for a one-window run), the most bytes of the record
 *   that were resident at a time, and the batches of epochs that were run again because a block left the resident span (a
 *   code rate more than 2 % off: the batch restarts from the state it began with, so the results do not change).  Any
 *   pointer may be NULL. */
BDS_API int bds_track_set_resident_limit(bds_ctx *ctx, size_t bytes);
BDS_API int bds_track_stream_info(bds_ctx *ctx, int32_t *pieces, long long *resident_max_bytes, int32_t *repeated_batches);
/* ---- tracking sessions: advance in pieces, or on samples fed by the caller ---------------------------------------
 * bds_track / bds_track_mem / bds_acquire_track run msToProcess worth of epochs in one call and forget the loop state.  A
 * session keeps it: the channel states, the launch geometry, the resident span of the record and the C/N0 carry survive the
 * call, so a long record is tracked into arrays of any size, and a record that is still arriving is tracked as it comes.
 *   bds_track_open       the record is the file at `path`
 *   bds_track_open_mem   the record is n_bytes raw file bytes in host memory; the bytes stay the caller's until bds_track_close
 *   bds_track_open_feed  the record is what the caller feeds with bds_track_feed (below)
 * `channel` is the acquisition's channel table, as for bds_track.  A failing bds_track_open* returns NULL and leaves the
 * message in bds_last_error(ctx).
 *
 * bds_track_advance runs the next k <= max_epochs epochs of every live channel in lock-step and returns k (or < 0).
 *   out          an ordinary bds_track_out with n_epochs = max_epochs as capacity (the row length of its arrays); element
 *                [ch][i] is epoch epochs_done[ch] + i of the run; rows are at the reference's template values behind the
 *                epochs written
 *   completed[ch] the number of epochs this call wrote for the channel: k unless the channel stopped
 *   status[ch]   'T' when the channel ran all k epochs, else '-'
 *   C/N0 arrays  hold, in order, the CNoIntervals that completed during this call; their number per channel goes to
 *                n_cno_done[ch] ([n_ch], may be NULL) and equals floor((e0 + k) / M) - floor(e0 / M), e0 = the epochs done
 *                before the call, M = CNoInterval.  If out->n_cno is smaller than that number can get, the call returns
 *                BDS_ERR_ARG with the needed number in the message, before anything runs.
 * The contract: whatever the sizes of the pieces, the concatenation of the arrays of successive advances equals the arrays of
 * ONE bds_track / bds_track_mem call on the same record, settings and channels, with msToProcess set to the sum of the pieces
 * and no end of file in it -- every field, bit for bit, DataCNo / DataPLD / PilotCNo / PilotPLD / SigCNo with the reference's
 * two-point smoothing (whose "previous" value crosses call boundaries) included; for all three trackers, all three record
 * formats and every BDS_TRK_PREC.
 * Launch geometry is fixed at open: the correlate grid, the chunk and the samples per lane are exactly what the one-shot call
 * chooses for the same channels and settings, because the fixed-order sum of the partial sums depends on them.  A session
 * always runs on the resident-span path of streamed tracking (above), a batch of epochs per advance or several: the span is
 * bounded by bds_track_set_resident_limit as set when the session is opened, or by 256 MiB (and never more than the record)
 * when no limit is set; bds_track_stream_info / bds_track_loaded_bytes count over the session, from the open on.
 * msToProcess and end of file: settings.msToProcess is not read by a session: a session has no preset end.  The reference's
 * rule "the first channel that meets the end of file ends the call, later channels are never started" therefore has no
 * counterpart: a session cannot take back pieces it has already returned.  Each channel stops at its own short read.  It then
 * has active = 0, its completed stops growing, and its partial results stay valid.
 *
 * Feed sessions.  The record is what the caller feeds: sample origin_sample of the record is the first sample fed, and
 * origin_sample must be a multiple of 32 samples.  skipNumberOfBytes + codePhase - 1 stays a position in the record (and
 * absoluteSample counts from the record's sample 0); a start position before origin_sample is BDS_ERR_ARG.  Bytes are those of
 * the settings' fileType: an I/Q record takes whole pairs (an odd count is BDS_ERR_ARG), of a packed record every byte is two
 * samples.  Of a 16-bit record (settings.dataType 1) a call takes whole samples only -- 2 bytes, 4 for an I/Q pair: the count it
 * returns is a multiple of that, whatever was offered, and the caller offers the rest again with what follows; a `last` call
 * whose byte count is not a whole number of samples is BDS_ERR_ARG.
 *   bds_track_feed  appends to the resident span and returns how many bytes it took (>= 0) or < 0.  It takes fewer than
 *                offered when the span is full -- it never drops or overwrites samples a live channel still needs; what lies
 *                behind the slowest channel is released first, the rest carried device to device --: the caller then advances
 *                and feeds the rest.  last != 0 (with every byte taken) marks the end of the record: from then on end of file
 *                is judged against the fed length, exactly as a file's size is.
 *   bds_track_advance runs the most epochs, up to max_epochs, that every live channel can complete inside the data fed so
 *                far, by the planning rule of the streamed path (blocks at a code rate 2 % low, the window guard as the safety
 *                net).  It may return 0; that is not an error.
 * No loader thread runs in a feed session: the caller's thread is the loader.
 *
 * bds_track_session_info: per channel the epochs done and the sample the next epoch starts at, one past the last sample of the
 *   record known so far (feed: fed; otherwise the record's length in samples) and the bytes of the record resident now.  Any
 *   pointer may be NULL.
 * One open session per context: bds_track, bds_track_mem, bds_acquire_track and a second bds_track_open* on that context
 *   return BDS_ERR_ARG, naming the open session.  bds_acquire / bds_acq_* on the same context between two advances are
 *   allowed (re-acquisition during a run) and leave both results unchanged.  bds_destroy closes an open session.  Every call
 *   on a closed or NULL session returns BDS_ERR_ARG (bds_track_close: nothing) without touching memory. */
typedef struct bds_track_session bds_track_session;
BDS_API bds_track_session *bds_track_open(bds_ctx *ctx, const bds_settings *s, const char *path, int n_ch,
                                          const bds_channel *channel);
BDS_API bds_track_session *bds_track_open_mem(bds_ctx *ctx, const bds_settings *s, const int8_t *file_bytes, size_t n_bytes,
                                              int n_ch, const bds_channel *channel);
BDS_API bds_track_session *bds_track_open_feed(bds_ctx *ctx, const bds_settings *s, long long origin_sample, int n_ch,
                                               const bds_channel *channel);
BDS_API int bds_track_feed(bds_track_session *sess, const int8_t *bytes, size_t n_bytes, int last);
BDS_API int bds_track_advance(bds_track_session *sess, int max_epochs, bds_track_out *out, int32_t *n_cno_done);
BDS_API int bds_track_session_info(bds_track_session *sess, int32_t *epochs_done, long long *next_sample,
                                   long long *fed_end, long long *resident_bytes);
BDS_API void bds_track_close(bds_track_session *sess);
/* Open-loop check entry: one correlate-and-dump epoch per channel with the caller's
 * NCO state (no loop update).  state: per channel {sample offset (0-based), blksize,
 * remCodePhase, codeFreq, remCarrPhase, carrFreq}; sums: [n_ch][18] raw correlator
 * outputs in the order I_E,Q_E,I_P,Q_P,I_L,Q_L, pilot(6), pilot BOC61 (6). */
BDS_API int bds_track_correlate(bds_ctx *ctx, const bds_settings *s, const int8_t *file_bytes,
                                size_t n_bytes, int n_ch, const int32_t *prn,
                                const double *state6, double *sums18);
/* Test aid, never needed by a host application: element k[i] (0-based) of the MATLAB colon vector a[i] : d[i] : b[i]
 * (non-integer operands, d > 0) exactly as the tracking kernels form their replica index vectors tcode -- first half
 * a + k d, second half from the right-hand end point, mid-point of an even interval count -- evaluated on the device, one
 * thread per entry.  value[i]: the element; c_end[i]: the right-hand end point (a + n d, snapped to b within
 * 2 eps max(|a|,|b|)); n_intervals[i]: n (the vector has n + 1 elements).  The tests hold them bit for bit against the
 * oracle's restatement of MathWorks' colonop. */
BDS_API int bds_track_colon(bds_ctx *ctx, int n, const double *a, const double *d, const double *b, const int32_t *k,
                            double *value, double *c_end, int32_t *n_intervals);
/* Test aid, never needed by a host application: the C/N0 and lock-detector post-pass of tracking (include/Calc_CNo_PLD.m,
 * tracking.m:411-434) on prompt values of the caller.  prompts: double[4][n_ch][n_epochs] = I_P, Q_P, Pilot_I_P, Pilot_Q_P;
 * done[ch]: epochs the channel completed (0 .. n_epochs); settings give CNoInterval (>= 2), intTime and the pilot mode.
 * cno5: double[5][n_ch][n_cno] = DataCNo, DataPLD, PilotCNo, PilotPLD, SigCNo of the intervals that completed, 0 elsewhere.
 * n_pieces = 0 launches the kernel of bds_track once over the arrays; with a list of piece lengths (each >= 1, adding up to
 * n_epochs) the kernel of bds_track_advance runs once per piece over that piece's epochs, with a session's carry buffers, and
 * the intervals each piece completes are put end to end.  The aid does no arithmetic of its own. */
BDS_API int bds_track_cno(bds_ctx *ctx, const bds_settings *s, int n_ch, int n_epochs, const double *prompts,
                          const int32_t *done, int n_pieces, const int32_t *pieces, int n_cno, double *cno5);
/* Test aid, never needed by a host application: the loop update of ONE epoch (discriminators, loop filters, next NCO state:
 * tracking.m:295-389 and the B1C counterparts) by the tracking update kernel, on channel states and correlator sums of the
 * caller.  state10: per channel {codeFreq, remCodePhase, carrFreq, carrFreqBasis, remCarrPhase, oldCodeNco, oldCodeError,
 * d2CarrError, dCarrError, codeFreqBasis} (codeFreq > 0 and remCodePhase < codeLength, both finite: the state must give a
 * block length); sums18: [n_ch][18] in the order of bds_track_correlate.  The record has no end and is resident, so the epoch
 * is never a short read.  state10_out: the next state; active[ch]: 1, or 0 when the update stopped the channel; completed[ch];
 * out21: double[21][n_ch], the epoch's entries of the per-epoch arrays in the order of bds_track_out (absoluteSample ..
 * remCarrPhase), at the reference's template values where the tracker writes none. */
BDS_API int bds_track_update(bds_ctx *ctx, const bds_settings *s, int n_ch, const double *state10, const double *sums18,
                             double *state10_out, int32_t *active, int32_t *completed, double *out21);

/* ---- correlation function along a tracked channel -------------------------------
 * Open-loop replay of tracked epochs at ANY set of tap offsets: the shape of the correlation function (the BOC(1,1) side peaks,
 * the BOC(6,1) ripple, what a multipath ray does to the S-curve), where the trackers return the three sums at
 * -+dllCorrelatorSpacing only.  Beyond the reference: tau outside -+dllCorrelatorSpacing has no counterpart there.
 *
 * An item is one epoch of one channel, given as bds_track_correlate takes it: prn[i] and state6[i] = {sample offset (0-based),
 * blksize, remCodePhase, codeFreq, remCarrPhase, carrFreq} -- what bds_track returns for the epoch: absoluteSample, remCodePhase,
 * remCarrPhase, codeFreq and carrFreq of epoch e (the two rates are stored before the loop filters replace them,
 * WB_tracking.m:404-406,428-430, so entry e is what epoch e ran on), blksize = ceil((codeLength - remCodePhase) / (codeFreq / fs)).
 * taps: n_taps offsets tau in primary-code chips, the unit of dllCorrelatorSpacing.  Limits: 1 <= n_taps <= 128, every tau
 * finite and |tau| <= 16; anything else is BDS_ERR_ARG.
 *
 * Index rule (B2a/tracking.m:260-316, B1C/WB_tracking.m:289-324, with tau in the place of -+earlyLateSpc): the replica index
 * vector of tap tau is the MATLAB colon vector
 *     t = (rem + tau)*sc : step*sc : (((blk-1)*step + rem) + tau)*sc,       sc = 1 (B2a), 2 (B1C),  step = codeFreq / fs,
 * the code unit of sample k is u = ceil(t(k)), and u6 = ceil(6 t(k)) for the pilot BOC(6,1) in wide-band mode.  The replica is
 * the PERIODIC extension of the code: unit u reads c[((u - 1) mod U) + 1] (non-negative mod; U = 10230 chips for B2a, 20460
 * half-chips for BOC(1,1), 122760 twelfths for BOC(6,1)).  For tau in {-spacing, 0, +spacing} this is index for index what the
 * trackers read through the reference's padded table [c(L) c(1..L) c(1)].  A tap whose colon vector does not have blksize elements
 * (MATLAB itself would stop there) makes the call return BDS_ERR_ARG, naming the item and the tap, before anything is launched.
 * Carrier: the reference's argument (carrFreq*2*pi)*(k/fs) + remCarrPhase at the trackers' default numerics, with their I/Q
 * conventions -- B2a exp(+j th), i = imag, q = real; B1C exp(-j th), i = real, q = imag.
 *
 * Output: out[item][comp][tap][2] = (I, Q) raw sums, double; comp 0 data, comp 1 the pilot (B2a pilot / pilot BOC(1,1)) when the
 * pilot is on, comp 2 the pilot BOC(6,1) in wide-band mode only -- the order of sums18's components; *n_comp receives the count.
 * The QMBOC composite (WB_tracking.m:375-380) is formed by the caller from comps 1 and 2.
 *
 * Determinism: an item's result depends on the item, the tap list and the settings only -- bit for bit the same whichever other
 * items are in the call, however the call is batched, and whichever of the three entries supplies the record.
 *
 * Record: all five formats the trackers take (fileType 1 / 2 / 3, dataType 0 / 1).  Only the span the items touch is loaded: items
 * are sorted by position and run in batches whose span of the record fits the resident limit (bds_track_set_resident_limit when
 * set, else 256 MiB); results come back in the caller's order.  One item that does not fit the limit is BDS_ERR_ARG with the
 * needed bytes in the message; an item that reaches past the end of the record is BDS_ERR_ARG and names the item.  On any error
 * nothing is written to out.  Like the one-shot tracking calls, the entries are BDS_ERR_ARG, naming the session, while the context
 * has an open tracking session (they share its code tables).  bds_get_timing afterwards: total_ms the call's stream time, search_ms its kernels alone, n_pairs the
 * number of batches, n_comp.  (After bds_track_correlate, search_ms is that call's kernels alone.) */
BDS_API int bds_corr_function(bds_ctx *ctx, const bds_settings *s, const char *path, int n_items, const int32_t *prn,
                              const double *state6, int n_taps, const double *taps, double *out, int32_t *n_comp);
BDS_API int bds_corr_function_mem(bds_ctx *ctx, const bds_settings *s, const int8_t *file_bytes, size_t n_bytes, int n_items,
                                  const int32_t *prn, const double *state6, int n_taps, const double *taps, double *out,
                                  int32_t *n_comp);
/* the record in device memory, under the pointer rule of the *_dev entries ("records in device memory" below) */
#define BDS_CORR_DEV_API __attribute__((visibility("default")))
BDS_CORR_DEV_API int bds_corr_function_dev(bds_ctx *ctx, const bds_settings *s, const void *d_file_bytes, size_t n_bytes,
                                           int n_items, const int32_t *prn, const double *state6, int n_taps, const double *taps,
                                           double *out, int32_t *n_comp);

/* ---- helpers replacing small host functions on the path ------------------------ */
/* Common/calcLoopCoef.m:41-45 */
BDS_API void bds_calc_loop_coef(double lbw, double zeta, double k, double *tau1, double *tau2);
/* Common/calcLoopCoefCarr.m:41-56 */
BDS_API void bds_calc_loop_coef_carr(const bds_settings *s, double *pf3, double *pf2, double *pf1);
/* B1C/include/CalcWeighingFactor.m:43-81 */
BDS_API double bds_calc_weighing_factor(const bds_settings *s);
/* preRun.m:61-76 (B1C applies Doppler aiding to codeFreq, B2a does not) */
BDS_API int bds_pre_run(const bds_settings *s, int max_prn, const double *carrFreq,
                        const double *codePhase, const double *peakMetric, bds_channel *channel);
/* The same allocation as a device kernel (stable descending rank of peakMetric by counting, one wave): replaces the host
 * loop of include/preRun.m:61-76 (either receiver) when acquisition and tracking are chained inside the library; `channel` (host,
 * numberOfChannels entries) receives a copy.  Bit-identical to bds_pre_run; settings.numberOfChannels > 64 (more channels than
 * PRNs: the extra ones stay idle) is served by the host loop. */
BDS_API int bds_pre_run_device(bds_ctx *ctx, const bds_settings *s, int max_prn, const double *carrFreq,
                               const double *codePhase, const double *peakMetric, bds_channel *channel);
/* acquisition -> preRun -> tracking in ONE call (B2a/postProcessing.m:100-123, B1C/postProcessing.m:105-143 without the
 * MATLAB statements between them): bds_acquire on `samples`, bds_pre_run_device on its results, bds_track on the record
 * at `path` with the settings' own tracking variant.  acqResults (as bds_acquire) and the channel table
 * (numberOfChannels entries) are returned beside trackResults. */
BDS_API int bds_acquire_track(bds_ctx *ctx, const bds_settings *s, const int8_t *samples, size_t n_samples,
                              int is_complex, int max_prn, double *carrFreq, double *codePhase,
                              double *peakMetric, int32_t *detected, const char *path,
                              bds_channel *channel, bds_track_out *out);
/* ... with an int16 block and a 16-bit record at `path` (settings.dataType 1) */
BDS_API int bds_acquire_track16(bds_ctx *ctx, const bds_settings *s, const int16_t *samples, size_t n_samples,
                                int is_complex, int max_prn, double *carrFreq, double *codePhase,
                                double *peakMetric, int32_t *detected, const char *path,
                                bds_channel *channel, bds_track_out *out);
/* ---- frame synchronisation correlators (the first consumers of trackResults) -------------
 * B1C/include/BCNAV1decoding.m:66-91: bits = sign(Pilot_I_P) (wide-band tracking) or sign(Pilot_Q_P)
 *   (narrow-band), XcorrResult = second half of xcorr(bits, generate2ndCode(PRN)) (1800 chips),
 *   index = find(abs(XcorrResult) >= 1799.5).
 * B2a/include/BCNAV2decoding.m:69-97: bits = sign(I_P), pattern = kron(preamble_bits, secondCode)
 *   (120 taps), index = find(abs(.) > 115).
 * prompt: double[n_ch * n] prompt-correlator series, one row per channel; prn[n_ch].
 * xcorr (optional): int32[n_ch * M], M = max(n, pattern length): the correlation at lags 0..M-1.
 * index (optional): int32[n_ch * cap], 1-based like find(); n_index[n_ch] = number of hits per
 *   channel (may exceed cap).  Returns the total number of hits or <0.
 * bds_sync_pattern: the +-1 pattern itself (1800 or 120 values). */
BDS_API int bds_frame_sync(bds_ctx *ctx, int signal, int n_ch, const int32_t *prn, const double *prompt,
                           int n, int32_t *xcorr, int32_t *index, int32_t *n_index, int cap);
BDS_API int bds_sync_pattern(int signal, int prn, int8_t *out, int cap);

/* ---- navigation decoding: B-CNAV1 / B-CNAV2 frames, ephemeris, TOW ---------------------------------------
 * The rest of B1C/include/BCNAV1decoding.m (:93-189, with BCH21_6Decoding.m, BCH51_8Decoding.m and B1C/include/ephemeris.m)
 * and of B2a/include/BCNAV2decoding.m (:99-159, with B2a/include/ephemeris.m): every candidate frame start that
 * bds_frame_sync's correlator finds is decoded on the device (one workgroup per channel and candidate, one launch), the decoded
 * frames are merged on the host, in candidate order, into one ephemeris per channel.  As in the reference NO LDPC decoding is
 * done: the information halves of the LDPC blocks are taken as received and stand or fall with their CRC-24Q.
 *
 * One rule is this library's own.  In the reference a CRC-valid frame whose PRN field is outside 1..63 makes ephemeris() return
 * early, after which `TOW = eph.TOW` (B1C) finds an empty field.  Here such a frame is NOT ENTERED: it changes no field of the
 * ephemeris and does not set firstSubFrame / TOW (status BDS_NAV_PRN_RANGE). */
enum {
    BDS_NAV_SHORT = 1,      /* B2a: fewer than 3000 prompts from the candidate on (BCNAV2decoding.m:105); nothing else is set */
    BDS_NAV_BCH1_OK = 2,    /* B1C: BCH(21,6) of symbols 1..21 passed, as received or inverted */
    BDS_NAV_BCH2_OK = 4,    /* B1C: BCH(51,8) of symbols 22..72 passed in the polarity kept; bits[] is written */
    BDS_NAV_CRC1_OK = 8,    /* CRC-24Q of sub-frame 2's 600 bits (B1C) / of the message's 288 bits (B2a) */
    BDS_NAV_CRC2_OK = 16,   /* B1C: CRC-24Q of sub-frame 3's 264 bits */
    BDS_NAV_ENTERED = 32,   /* the frame entered the channel's ephemeris */
    BDS_NAV_PRN_RANGE = 64  /* all checks passed but the PRN field is outside 1..63: not entered (above) */
};
#define BDS_NAV_BITS_B1C 878 /* decodedNav: 6 + 8 + 600 + 264 (BCNAV1decoding.m:94,129,142,161,163) */
#define BDS_NAV_BITS_B2A 288 /* decodedNavBits (BCNAV2decoding.m:132) */
typedef struct bds_nav_frame {
    uint32_t size;     /* sizeof(bds_nav_frame), set by the library */
    int32_t index;     /* the candidate, 1-based as in the reference's `index` */
    uint32_t status;   /* BDS_NAV_* flags */
    int32_t polarity;  /* +1 as received, -1 inverted, 0 not determined (B1C: both BCH(21,6) attempts failed; B2a: short) */
    int32_t bch1_max;  /* B1C: maxValue of the last BCH(21,6) attempt made (the inverted one when the first failed) */
    int32_t bch2_max;  /* B1C: maxValue of BCH(51,8) in the polarity kept; 0 when not reached */
    uint8_t bits[112]; /* the decoded bits, first bit = most significant bit of bits[0]: 878 (B1C) or 288 (B2a), rest zero */
} bds_nav_frame;

/* One double per numeric field of B1C/include/eph_structure_init.m and B2a/include/eph_structure_init.m (the union of the two;
 * names as there).  NaN = the reference's []: not decoded, or not a field of this signal. */
#define BDS_EPH_FIELDS(X)                                                                                                   \
    X(PRN) X(SOH) X(SOW) X(WN) X(HOW) X(IODC) X(IODE) X(IODC_MSB2) X(IODC_LSB8)                                             \
    X(t_oe) X(deltaA) X(ADot) X(delta_n_0) X(delta_n_0Dot) X(M_0) X(e) X(omega)                                             \
    X(omega_0) X(i_0) X(omegaDot) X(i_0Dot) X(C_is) X(C_ic) X(C_rs) X(C_rc) X(C_us) X(C_uc)                                 \
    X(t_oc) X(a_0) X(a_1) X(a_2) X(T_GDB2ap) X(ISC_B1Cd) X(T_GDB1Cp)                                                        \
    X(PageID1) X(PageID3) X(HS) X(DIF) X(SIF) X(AIF) X(SISMAI)                                                              \
    X(alpha1) X(alpha2) X(alpha3) X(alpha4) X(alpha5) X(alpha6) X(alpha7) X(alpha8) X(alpha9)                               \
    X(A_0UTC) X(A_1UTC) X(A_2UTC) X(delta_t_LS) X(t_ot) X(WN_ot) X(WN_LSF) X(DN) X(delta_t_LSF)                             \
    X(GNSS_ID) X(WN_0BGTO) X(t_0BGTO) X(A_0BGTO) X(A_1BGTO) X(A_2BGTO) X(TOW)
typedef struct bds_eph {
    uint32_t size;       /* sizeof(bds_eph), set by the CALLER (of each array element); checked */
    int32_t flag;        /* 1 once a frame has entered (B1C: eph.flag), else 0 */
    int32_t SatType;     /* 0 = [] / code 0, 1 = 'GEO', 2 = 'IGSO', 3 = 'MEO' */
    int32_t n_entered;   /* frames / messages that entered */
    int32_t idValid[8];  /* B2a: 10, 11, 30..34 in slots 0..6 once seen, the last other message type in slot 7; B1C: zeros */
#define BDS_EPH_X(name) double name;
    BDS_EPH_FIELDS(BDS_EPH_X)
#undef BDS_EPH_X
} bds_eph;

/* BCNAV1decoding(trackResults, channelNr, settings) / BCNAV2decoding(I_P_InputBits) for n_ch channels in one call.
 *   settings:     only .signal is read; which series is the pilot's is the caller's choice by pilotTRKflag, as below.
 *   sync_prompt:  double[n_ch * n], what bds_frame_sync takes: Pilot_I_P / Pilot_Q_P by pilotTRKflag (B1C), I_P (B2a).
 *   data_prompt:  double[n_ch * n]: I_P (B1C).  NULL = sync_prompt itself; B2a decodes the series it synchronised on, so it must
 *                 be NULL (or the same pointer) there.
 *   frames (optional): bds_nav_frame[n_ch * cap], the first min(cap, n_frames[c]) candidates of channel c in candidate order;
 *                 n_frames[n_ch] (optional) = candidates per channel (may exceed cap; the ephemeris uses all of them).
 *   eph:          bds_eph[n_ch], each with .size set.  firstSubFrame, TOW: double[n_ch], +inf where nothing entered.
 * Returns the number of frames that entered, over all channels, or < 0.
 * bds_nav_fields (no GPU): the host half alone.  n_msg decoded messages of `stride` bytes each (bits as in bds_nav_frame,
 * at least 110 / 36 bytes) go, in order, through the field parser and the merging rules into *eph; returns how many entered. */
BDS_API int bds_nav_decode(bds_ctx *ctx, const bds_settings *settings, int n_ch, const int32_t *prn, const double *sync_prompt,
                           const double *data_prompt, int n, bds_nav_frame *frames, int32_t *n_frames, int cap, bds_eph *eph,
                           double *firstSubFrame, double *TOW);
BDS_API int bds_nav_fields(int signal, const uint8_t *bits, int n_msg, int stride, bds_eph *eph);

/* ---- position fix: postNavigation from trackResults to navSolutions -----------------------------------------
 * BDS-3_B1C/postNavigation.m:100-298 and BDS-3_B2a/postNavigation.m (the same text from "Set measurement-time point" on), with
 * Common/calculatePseudoranges.m:63-110, include/satpos.m, include/check_t.m, Common/leastSquarePos.m, Common/e_r_corr.m,
 * include/topocent.m, Common/togeod.m, Common/tropo.m and Common/cart2geo.m (ellipsoid 5).  Two stages:
 *   measure  on the device, one lane per (measurement epoch, channel), one launch: index search, transmit time, satpos.  None of
 *            it depends on an earlier epoch.
 *   solve    on the host, sequential over the epochs: localTime, the elevation mask, leastSquarePos, DOP, cart2geo.
 * This is a capability, not a throughput feature: the fix chain is a few microseconds per epoch of host arithmetic.
 *
 * Channels are the reference's channel numbers: n_ch = numberOfChannels rows, row c = channel c + 1, idle ones included.
 *
 * Rules that are this library's own:
 *   - B2a T_GDB1Cp.  BDS-3_B2a/include/satpos.m:62,152 reads eph.T_GDB1Cp, which the B2a eph_structure_init.m / ephemeris.m never
 *     create: the file cannot run as written.  For B2a the term is 0.
 *   - Empty SatType.  A ready channel whose eph.SatType is empty (0) would leave A_ref undefined (satpos.m:69-73); it is dropped
 *     from the ready list with BDS_PVT_NO_SATTYPE.
 *   - A channel that passes the readiness rule but has no finite subFrameStart in [1, n] or no finite TOW (the reference would index
 *     absoluteSample(inf)) is dropped with BDS_PVT_NO_FRAME.
 *   - absoluteSample order.  Over [1, n] absoluteSample must be strictly increasing on every ready channel (it is for any channel
 *     tracked to the end); otherwise BDS_ERR_ARG.  Only then does the binary search equal the reference's scan.
 *   - Duplicate PRNs.  Two channels with the same PRN are two rows, as in the reference (the fix is then rank deficient when they
 *     are two of four).
 *   - A matrix A with a NaN or inf entry, at which MATLAB's rank() stops with an error, takes the rank-failure exit. */
typedef struct bds_pvt_params {
    uint32_t size;        /* sizeof(bds_pvt_params), set by the caller; checked */
    int32_t useTropCorr;  /* settings.useTropCorr: 1 = tropo() in leastSquarePos.m:68-75, anything else = 0 m */
    double navSolPeriod;  /* [ms] settings.navSolPeriod (postNavigation.m:119) */
    double elevationMask; /* [deg] settings.elevationMask (:151) */
    double c;             /* [m/s] settings.c */
    double startOffset;   /* [ms] settings.startOffset (calculatePseudoranges.m:104) */
} bds_pvt_params;
enum {
    BDS_PVT_READY = 1,       /* on the ready list (readyChnList, postNavigation.m:135) */
    BDS_PVT_IDLE = 2,        /* status '-' (:69) */
    BDS_PVT_NO_EPH = 4,      /* readiness rule not met: B1C eph.flag == 1 (:82); B2a idValid(1) == 10 && idValid(2) == 11 &&
                                any(idValid(3:7) == 30:34) (BDS-3_B2a/postNavigation.m:84-85) */
    BDS_PVT_NO_SATTYPE = 8,  /* rule met, SatType empty: dropped (above) */
    BDS_PVT_NO_FRAME = 16    /* rule met, subFrameStart / TOW not usable: dropped (above) */
};
/* What the chain stores per epoch (postNavigation.m:155-293).  Every array is the caller's; cap = measurement epochs each holds.
 * Per channel and epoch, double[n_ch * cap], element [c * cap + m] (MATLAB's navSolutions.x(c + 1, m + 1)):
 *   PRN 0 where not active; el, az, transmitTime, satClkCorr NaN where not active; rawP -inf where not active (the reference
 *   computes (localTime - inf) * c); correctedP 0 where not active (MATLAB array growth).
 * DOP: double[5 * cap], element [k * cap + m] (GDOP, PDOP, HDOP, VDOP, TDOP).  The rest double[cap].
 * dt is forced to 0 at the first epoch (:218-222); localTime is still corrected with the solved value (:225). */
typedef struct bds_pvt_out {
    uint32_t size; /* sizeof(bds_pvt_out), set by the caller; checked */
    int32_t cap;
    double *PRN, *el, *az, *transmitTime, *satClkCorr, *rawP, *correctedP;
    double *DOP;
    double *X, *Y, *Z, *dt, *localTime, *currMeasSample, *latitude, *longitude, *height;
} bds_pvt_out;

/* bds_pvt_plan (no GPU): postNavigation.m:69-122 after the decoding.
 *   status: char[n_ch], trackResults.status ('-' = idle).  absoluteSample: double[n_ch * n].  eph: bds_eph[n_ch] (.size set),
 *   subFrameStart, TOW: double[n_ch], as bds_nav_decode leaves them (rows of idle channels are not read).
 *   ready: int32[n_ch], BDS_PVT_* flags.  sampleStart = max(absoluteSample(subFrameStart)) + 1 and sampleEnd =
 *   min(absoluteSample(end)) - 1 over the ready channels (:106-116), measSampleStep = fix(samplingFreq * navSolPeriod / 1000) (:119).
 * Returns n_meas = fix((sampleEnd - sampleStart) / measSampleStep) (:122), or 0 -- with the three numbers as far as they exist --
 * when fewer than 4 channels are ready (:92-98) or that number is <= 0 (the reference would leave navSolutions unassigned), or < 0.
 * bds_pvt_measure: the device stage.  ready as bds_pvt_plan left it; absoluteSample, codeFreq, remCodePhase: double[n_ch * n],
 *   uploaded once.  transmitTime, satClkCorr: double[n_meas * n_ch], element [m * n_ch + c]; satPos: double[n_meas * n_ch * 3], x y z
 *   per element.  A channel that is not ready gets NaN.  bds_get_timing afterwards: search_ms = the kernel alone (hipEvents).
 * bds_pvt_solve (no GPU): the chain of postNavigation.m:146-298 over those arrays.  prn: int32[n_ch].  Returns n_meas or < 0.
 * bds_post_navigation: plan, measure, solve.  *n_meas (optional) receives the planned number even when it exceeds out->cap, in which
 *   case the call returns BDS_ERR_ARG and writes nothing else.  Returns the number of epochs stored (0: no solution, above). */
BDS_API int bds_pvt_plan(const bds_settings *s, const bds_pvt_params *p, int n_ch, int n, const char *status,
                         const double *absoluteSample, const bds_eph *eph, const double *subFrameStart, const double *TOW,
                         int32_t *ready, double *sampleStart, double *sampleEnd, double *measSampleStep);
BDS_API int bds_pvt_measure(bds_ctx *ctx, const bds_settings *s, int n_ch, int n, const int32_t *ready, const double *absoluteSample,
                            const double *codeFreq, const double *remCodePhase, const bds_eph *eph, const double *subFrameStart,
                            const double *TOW, double sampleStart, double measSampleStep, int n_meas, double *transmitTime,
                            double *satPos, double *satClkCorr);
BDS_API int bds_pvt_solve(const bds_settings *s, const bds_pvt_params *p, int n_ch, int n_meas, const int32_t *prn,
                          const int32_t *ready, double sampleStart, double measSampleStep, const double *transmitTime,
                          const double *satPos, const double *satClkCorr, bds_pvt_out *out);
BDS_API int bds_post_navigation(bds_ctx *ctx, const bds_settings *s, const bds_pvt_params *p, int n_ch, int n, const char *status,
                                const int32_t *prn, const double *absoluteSample, const double *codeFreq, const double *remCodePhase,
                                const bds_eph *eph, const double *subFrameStart, const double *TOW, int32_t *ready, int32_t *n_meas,
                                bds_pvt_out *out);

/* B2a/include/unpack_cplx.m: converter of packed records (one byte = two complex samples, 2-bit
 * sign/magnitude I and Q each) into the int8 I/Q pairs of a fileType-2 record.
 * out: int8[4 * n_bytes] = I1, Q1, I2, Q2 per input byte.  The file variant mirrors
 * unpack_cplx(filename_in, filename_out). */
BDS_API int bds_unpack_cplx(bds_ctx *ctx, const uint8_t *in, size_t n_bytes, int8_t *out);
BDS_API int bds_unpack_cplx_file(bds_ctx *ctx, const char *path_in, const char *path_out);

/* The acquisition's resampling branch (B2a/acquisition.m:54-124, B1C/acquisition.m:54-123), taken
 * inside bds_acq_load when samplingFreq > resamplingThreshold && resamplingflag == 1.
 * bds_resample_plan: returns 1 and the sampling rate / IF acquisition() continues with (:103,:119)
 *   plus the fir1 band edges (:66) when the branch is taken, 0 (outputs untouched) otherwise.
 * bds_fir1_bandpass: b = fir1(n_taps-1, [wp1 wp2]) (Hamming window, unit gain at the band centre). */
BDS_API int bds_resample_plan(const bds_settings *s, double *new_fs, double *new_if, double *wp);
BDS_API int bds_fir1_bandpass(int n_taps, double wp1, double wp2, double *b);

/* ---- synthetic IF records, generated on the device ------------------------------------------------------
 * The reference ships no recording; bds_amd/synth.py:make_if (a NumPy loop) is the model the tests' inputs come from.  bds_synth
 * makes the same signal on the device, per sample and satellite in make_if's own float64 operation order (synth.py:87-119):
 *   chips = (n - delay) (fcode / fs), fcode = codeFreqBasis (1 + doppler / carrFreqBasis) (code_doppler 0: codeFreqBasis)
 *   period = floor(chips / codeLength), cph = chips - period codeLength, chip = min((int)cph, codeLength - 1)
 *   th = (2 pi) fmod(((IF + doppler) n) / fs, 1) + phase
 *   B1C: s_I = 1/2 D c_d boc11 - sqrt(1/11) c_p boc61 [S], s_Q = sqrt(29/44) c_p boc11 S;  B2a: s_I = S c_p, s_Q = -D c_d
 *   z = amp (s_I + j s_Q) e^{j th}, amp = sigma sqrt(4 10^(cn0 / 10) / fs), summed over the satellites in list order
 * n is the GLOBAL sample index of the record (first_sample + the index in `out`): a record made in pieces, in any order, is the
 * same bytes as the record made in one call.  What differs from make_if is the random stream, which is counter-based
 * (csrc/bds_synth_math.h: Philox4x32-10 keyed by the seed) instead of sequential:
 *   noise of sample n   counter (n low, n high, 0, 0) -> words w0..w3; u1 = (((w0 2^32 + w1) >> 12) + 0.5) 2^-52,
 *                       u2 = ((w2 2^32 + w3) >> 11) 2^-53; r = sqrt(-2 log u1), g_I = r cos(2 pi u2), g_Q = r sin(2 pi u2);
 *                       a real record adds sigma g_I, an I/Q record sigma (g_I + j g_Q)
 *   symbols             D (component 0) and S (component 1) of code period p of satellite prn: counter (p + 1 as int64: low, high;
 *                       1; 2 prn + component), +1 when bit 0 of w0 is set, else -1 -- or, when opts.symbols is given
 *                       (int8[n_sat][2][n_sym], +-1, [satellite][D, S][index]), element (p + 1) mod n_sym (non-negative)
 * Formats (opts.format), and what `out` holds for n_samples samples:
 *   0  double[n_samples]      the clean real sum: no noise, not quantised (make_if(clean=True))
 *   1  int8[n_samples]        real record (fileType 1): rint(sum + sigma g_I), clipped to +-127
 *   2  int8[2 n_samples]      interleaved I/Q (fileType 2): the analytic signal (iq_sign >= 0; make_if's iq_sign +1) or its conjugate (< 0)
 *   3  uint8[n_samples / 2]   packed 2+2-bit I/Q (fileType 3, the nibble layout above): of each int8 value of format 2 the sign (0 is
 *                             positive) and magnitude 3 where |value| > threshold, else 1; first_sample and n_samples must be even
 * Up to 63 satellites; n_sat = 0 is noise alone.  A PRN may repeat (multipath: the entries share code and symbols; with
 * opts.symbols every entry has its own rows).  opts.threshold <= 0 means sigma.  opts.size must be sizeof(bds_synth_opts).
 * All argument errors (BDS_ERR_ARG, message in bds_last_error -- of ctx, or of NULL when ctx is NULL) are raised before any
 * device call. */
typedef struct bds_synth_sat {
    int32_t prn, reserved0;
    double doppler;   /* [Hz] */
    double delay;     /* [samples] 0-based sample at which a primary-code period starts */
    double phase;     /* [rad] */
    double cn0_dbhz;
} bds_synth_sat;
typedef struct bds_synth_opts {
    int32_t size;     /* sizeof(bds_synth_opts), else BDS_ERR_ARG */
    int32_t format, iq_sign, code_doppler, pilot61_secondary, reserved0;
    uint64_t seed;
    double sigma, threshold;
    const int8_t *symbols; /* NULL: symbols from the counter-based stream */
    int64_t n_sym;
} bds_synth_opts;
BDS_API int bds_synth(bds_ctx *ctx, const bds_settings *s, int n_sat, const bds_synth_sat *sats, const bds_synth_opts *opts,
                      int64_t first_sample, int64_t n_samples, void *out, size_t out_bytes);
/* The same record written to `path` in pieces of piece_samples samples (0: 64 MiB of the record per piece, 32 MiB of a packed one):
 * piece k + 1 is generated on the context's second stream while piece k is copied out and written (two device buffers, two pinned
 * host buffers).  The file is byte-identical to the one-call result whatever piece_samples is (format 3: an odd piece_samples is
 * rounded up to even).  After either call bds_get_timing reports total_ms (stream time of the call), forward_ms (the generation
 * kernels, summed over the pieces) and search_ms (the pieces' device-to-host copies); every other field is 0. */
BDS_API int bds_synth_file(bds_ctx *ctx, const bds_settings *s, int n_sat, const bds_synth_sat *sats, const bds_synth_opts *opts,
                           int64_t first_sample, int64_t n_samples, const char *path, int64_t piece_samples);
/* Test aid: the raw N(0, 1) stream of samples first .. first + n - 1 as the device forms it (either pointer may be NULL). */
BDS_API int bds_synth_noise(bds_ctx *ctx, uint64_t seed, int64_t first, int64_t n, double *g_i, double *g_q);

/* ---- synthetic IF records driven by an orbit: a receiver position and ephemerides in, a record out -------------------------
 * bds_synth gives every satellite one constant Doppler and one constant delay.  On this path code and carrier phase of every
 * satellite follow a TRAJECTORY instead: piecewise cubics in the sample index, in segments of 2^seg_log2 samples (a power of two,
 * so the device finds a sample's segment with a shift and no 64-bit division).  Per sample n and satellite, every operation
 * rounding once (csrc/bds_synth_math.h: traj_index, traj_code, traj_carrier):
 *   j = (n - traj.first) >> seg_log2;  u = (double)(n - traj.first - (j << seg_log2))            seg = traj.seg[sat][j]
 *   c = ((code[3] u + code[2]) u + code[1]) u + code[0];  k = floor(c / codeLength);  cph = c - k codeLength;  period = period0 + (int64)k
 *   x = ((carr[3] u + carr[2]) u + carr[1]) u + carr[0];  th = (2 pi) (x - trunc(x)) + phase
 * and from cph, period and th on the sample is bds_synth's: chip index, BOC signs, symbols (element (period + 1) mod n_sym of
 * opts.symbols, or the counter-based stream), amplitude, pilot61_secondary, iq_sign, noise, the formats 0..3, threshold and the
 * timing report are those of bds_synth, and a record made in pieces, in any order, is the one-call record bit for bit: it depends
 * on (seed, n, trajectory) alone.  Carrier Doppler, code Doppler and their rates all follow from the one trajectory, so
 * opts.code_doppler is ignored, and of each bds_synth_sat entry prn, phase and cn0_dbhz are used: a non-zero doppler or delay is
 * BDS_ERR_ARG.
 * bds_synth_trajectory (host only, no GPU) fills the segments from the physical model that postNavigation inverts:
 *   sample n is taken at system time tow + t0 + n / fs (the receiver clock offset is part of t0);
 *   a signal that leaves satellite k at satellite-clock time tow + rel arrives at tow + rel + delay_k(rel),
 *   delay_k(rel) = |R3(OmegaE_dot travel) pos - rx| / c - clk, travel = |pos - rx| / c, (pos, clk) = satpos(eph_k, tow + rel)
 *   (the library's own satpos, csrc/bds_pvt_math.h; OmegaE_dot = 7.292115147e-5 rad/s of e_r_corr.m; c = 299 792 458 m/s; no
 *   ionosphere, no troposphere, a receiver at rest in the Earth-fixed frame);
 *   for a sample, rel solves rel = (t0 + n / fs) - delay_k(rel) (the iteration contracts by ~3e-6 per step), and then
 *   code phase = rel codeFreqBasis chips -- code period P is the one that leaves at tow + P codeLength / codeFreqBasis --
 *   carrier phase = IF n / fs - carrFreqBasis (n / fs - rel) cycles.
 * Each segment is the cubic through four of its points, both ends included (u = 0, rint(L / 3), rint(2 L / 3), L = 2^seg_log2), so
 * neighbours meet at the joint; the large parts stay out of the polynomials: period0 is an integer, code[0] lies in
 * [0, codeLength), carr[0] in [0, 1).  out: bds_synth_seg[n_sat][n_seg], segment j of satellite k at out[k * n_seg + j].
 * Argument errors (BDS_ERR_ARG, message in bds_last_error(NULL)): a NULL pointer, seg_log2 outside 10..26, n_sat / n_seg / first
 * out of range, an ephemeris that is not ready (postNavigation's rule) or has an unknown SatType, a non-finite result, a code rate
 * that is not positive.
 * bds_synth_traj / bds_synth_traj_dev check before any device call, besides what bds_synth checks: traj.size, traj.seg, seg_log2,
 * that every sample the device evaluates -- the call's samples and those that make its last 16-byte unit whole, up to 31 more --
 * lies inside first .. first + n_seg 2^seg_log2, that every coefficient is finite and code[1] > 0, and the symbol table's period
 * span (the code period is monotone in n: the first and the last sample bound it). */
typedef struct bds_synth_seg {   /* one satellite, one segment; u = n - (traj.first + j 2^seg_log2), an exact integer in a double */
    int64_t period0;             /* code period that code[] counts from */
    double code[4];              /* chips since the start of period0: ((code[3] u + code[2]) u + code[1]) u + code[0] */
    double carr[4];              /* carrier phase in cycles, same Horner form */
} bds_synth_seg;
/* (a struct tag without a typedef: the entry below carries the same name, as stat() and struct stat do, so the type is always
 * written `struct bds_synth_traj`) */
struct bds_synth_traj {
    int32_t size, seg_log2;      /* sizeof(struct bds_synth_traj); segments of 2^seg_log2 samples, 10 .. 26 */
    int64_t first, n_seg;        /* segment j covers samples first + j 2^seg_log2 .. first + (j + 1) 2^seg_log2 - 1 */
    const bds_synth_seg *seg;    /* [n_sat][n_seg] */
};
BDS_API int bds_synth_trajectory(const bds_settings *s, int n_sat, const bds_eph *eph, const double rx[3], double tow, double t0,
                                 int64_t first, int64_t n_seg, int seg_log2, bds_synth_seg *out);
BDS_API int bds_synth_traj(bds_ctx *ctx, const bds_settings *s, int n_sat, const bds_synth_sat *sats, const bds_synth_opts *opts,
                           const struct bds_synth_traj *traj, int64_t first_sample, int64_t n_samples, void *out, size_t out_bytes);

/* ---- records in device memory: generate, search and track without the host round trip -------------------------------
 * A record that is made on the card -- by bds_synth_dev, or by a front end of the caller's (filter, down-converter, channeliser)
 * -- is searched and tracked from where it lies.  Each entry below does what its host-memory counterpart does with the same
 * bytes, and every output is bit-identical to that counterpart's: acqResults and what bds_acq_grid / bds_acq_peaks /
 * bds_acq_candidates / bds_acq_coherent_sums / bds_get_timing report after them, every field of bds_track_out, the pieces of a
 * session with their C/N0 carry, bds_track_stream_info.  bds_track_loaded_bytes counts the bytes brought into the resident span
 * whatever their source, so the numbers of a device-sourced run are the host-sourced run's.
 *   bds_synth_dev       = bds_synth, the record written to d_out (out_bytes as for bds_synth: at least the n_samples samples of the
 *                         format).  A 16-byte-aligned d_out is written in place, the last partial 16 bytes apart; any other d_out
 *                         goes through a buffer of the library's and a device-to-device copy.  No byte outside the record is written.
 *                         bds_get_timing reports as after bds_synth; search_ms is the device-to-device copies (0: none was made).
 *   bds_acq_load_dev    = bds_acq_load.  The block is copied device to device and brought to the host once: the block statistics
 *                         (the sums that set the storage scales, the prefix sums of the DC means, the signal power of the B1C
 *                         decision) stay the host's exact sums, the same lines for both sources.  bds_acq_prepare / bds_acq_run,
 *                         the resampling branch and the fallbacks work after it exactly as after bds_acq_load.
 *   bds_track_dev       = bds_track_mem
 *   bds_track_open_dev  = bds_track_open_mem
 *   bds_track_feed_dev  = bds_track_feed
 *                         The one-window load, the pieces of the loader thread, the synchronous reload and the feed append are the
 *                         same copies, device to device, on the same streams in the same order.  The correlators never run on the
 *                         caller's buffer in place: their aligned reads assume the library's own allocations.
 * The pointer rule, checked before any device work: hipPointerGetAttributes must report ordinary device memory
 *   (hipMemoryTypeDevice: hipMalloc, or a framework's allocator on top of it) of the CONTEXT'S device, and hipMemGetAddressRange
 *   must show [p, p + bytes) inside one allocation.  A host pointer, pinned or registered host memory, managed memory, memory of
 *   another device, NULL with a non-zero size, or a range that runs past its allocation returns BDS_ERR_ARG with a message that
 *   names the argument and what was found; nothing is launched and nothing is copied.  Any byte alignment is accepted.
 * The ordering rule: the library works on its context's own non-blocking streams, which nothing orders against the caller's.
 *   The caller guarantees that all writes to the memory are complete when the call is made (synchronise the producing stream
 *   first).  bds_synth_dev, bds_acq_load_dev, bds_track_dev and bds_track_feed_dev return only after their reads and writes of
 *   caller memory are complete: the memory is the caller's again.  The record of bds_track_open_dev must stay valid and unmodified
 *   until bds_track_close, as for bds_track_open_mem: the loader thread reads it while epochs run.
 * The session rules carry over unchanged, with the same messages: one session per context, origin_sample a multiple of 32,
 *   whole I/Q pairs, `last`, partial takes when the span is full; bds_track_feed_dev on a session that was not opened with
 *   bds_track_open_feed, or on a closed one, returns BDS_ERR_ARG.  One feed session may take host and device bytes in turn. */
/* (these five entries are marked BDS_DEV_API, not BDS_API: the pointer they take for the record is a DEVICE pointer, which a host
 * language binding must not fill from its own arrays -- a binding generator that walks the BDS_API entries does not see them) */
#define BDS_DEV_API __attribute__((visibility("default")))
BDS_DEV_API int bds_synth_dev(bds_ctx *ctx, const bds_settings *s, int n_sat, const bds_synth_sat *sats, const bds_synth_opts *opts,
                          int64_t first_sample, int64_t n_samples, void *d_out, size_t out_bytes);
BDS_DEV_API int bds_acq_load_dev(bds_ctx *ctx, const bds_settings *s, const void *d_samples, size_t n_samples, int is_complex);
BDS_DEV_API int bds_track_dev(bds_ctx *ctx, const bds_settings *s, const void *d_file_bytes, size_t n_bytes, int n_ch,
                          const bds_channel *channel, bds_track_out *out);
BDS_DEV_API bds_track_session *bds_track_open_dev(bds_ctx *ctx, const bds_settings *s, const void *d_file_bytes, size_t n_bytes,
                                              int n_ch, const bds_channel *channel);
BDS_DEV_API int bds_track_feed_dev(bds_track_session *sess, const void *d_bytes, size_t n_bytes, int last);
/* bds_synth_traj, the record written to device memory: d_out and out_bytes under the pointer rule and the ordering rule above,
 * written as bds_synth_dev writes (any byte alignment, no byte outside the record); traj and traj->seg are HOST memory.  (Marked
 * BDS_SYNTH_DEV_API for the reason given above: its record pointer is a device pointer.) */
#define BDS_SYNTH_DEV_API __attribute__((visibility("default")))
BDS_SYNTH_DEV_API int bds_synth_traj_dev(bds_ctx *ctx, const bds_settings *s, int n_sat, const bds_synth_sat *sats,
                                         const bds_synth_opts *opts, const struct bds_synth_traj *traj, int64_t first_sample,
                                         int64_t n_samples, void *d_out, size_t out_bytes);

/* ---- probeData: histogram, Welch PSD and excerpt of an IF record ------------------------------------------------------------
 * probeData(settings) / probeData(fileName, settings)     B2a/include/probeData.m:1, B1C/include/probeData.m:1
 * The numbers behind the reference's figure 100, of a record in any format bds_track reads -- settings.fileType / dataType select
 * the decoder exactly as there: int8 real, int8 I/Q pairs, packed 2+2-bit I/Q (fileType 3), int16 real, int16 I/Q pairs -- decoded
 * on the device from the record's own bytes.
 *   histogram  hist(data, -128:128) (probeData.m:146; :155,:163 for I and Q): 257 bins, bin = clamp(v, -128, 128) + 128, so a
 *              16-bit value outside +-128 lands in an end bin as with hist.  int64 counts; they add up to n_samples.  A real
 *              record fills hist_i (hist_q, if given, is zeroed).  min / max / sum / sumsq per component are exact integers
 *              (sumsq needs n max(v^2) < 2^63).
 *   psd        pwelch(data, 32768, 2048, 32768, fs) (probeData.m:128; 'twosided' :131): symmetric Hamming window
 *              w[n] = 0.54 - 0.46 cos(2 pi n / 32767), segment k starts at sample 30720 k, n_segments = fix((n - 2048) / 30720),
 *              the tail is ignored, no detrending; |FFT(w x)|^2 / (fs sum w^2), averaged over the segments.  Real record: one-sided,
 *              n_psd = 16385 bins, all doubled except DC and Nyquist.  I/Q record: two-sided, n_psd = 32768 bins in natural order
 *              0 .. fs (the reordering of probeData.m:132-134 is the caller's).  Always the density per Hz of settings.samplingFreq
 *              (the fs / 1e6 of probeData.m:128 is an axis matter).  Transforms in fp32; the sum over segments is a left-to-right
 *              f64 sum per bin in segment order, independent of pieces and batches: every source gives the same bits.
 *   excerpt    the first n_time samples as double (probeData.m:96-97 plots round(samplesPerCode / 500) of a real record,
 *              :106-107,:114-115 round(samplesPerCode / 2) of I and Q; the B1C copy round(samplesPerCode / 2) of both).
 * bds_probe_out is caller-allocated: hist_i[257], hist_q[257] (may be NULL for a real record), psd[cap] with cap >= n_psd,
 *   excerpt_re[n_time] and, for an I/Q record, excerpt_im[n_time] (both may be NULL when n_time is 0).
 * bds_probe_data       the record is n_bytes raw file bytes in host memory (the whole array is the window)
 * bds_probe_data_file  the record is the file at `path` behind settings.skipNumberOfBytes (the fseek of probeData.m:63), counted
 *                      as bds_track counts it: in samples (bytes for an int8 real record; pairs for I/Q; a packed record may
 *                      start at a high nibble).  n_samples > 0: that many samples; 0: what the signal's own probeData.m reads --
 *                      5 samplesPerCode (B2a/include/probeData.m:76), 10 samplesPerCode (B1C/include/probeData.m:76); -1: to the
 *                      end of the file.
 * Both pass the window through device memory in pieces whose seams fall on segment starts (a piece carries whole segments and
 * the 2048 samples its last one shares with the next piece), by default as many segments as 256 MiB of the record hold.
 * bds_probe_set_piece_segments(ctx, n) sets the segments per piece for the calls that follow on the context (0: the default);
 * the results do not depend on it, bit for bit.
 * Errors: BDS_ERR_ARG with a message and nothing written to *out for fewer than 32768 samples (pwelch cannot form one segment),
 * a byte count that is not a whole number of samples (odd for an I/Q or 16-bit record), cap < n_psd, n_time outside the window,
 * and a file shorter than the window ("Could not read enough data", probeData.m:81-84); BDS_ERR_IO when the file cannot be opened. */
typedef struct bds_probe_out {
    int64_t *hist_i, *hist_q;
    int64_t min_i, max_i, sum_i, sumsq_i, min_q, max_q, sum_q, sumsq_q;
    double *psd;
    int32_t cap, n_psd;
    int64_t n_segments, n_samples;
    double *excerpt_re, *excerpt_im;
} bds_probe_out;
BDS_API int bds_probe_data(bds_ctx *ctx, const bds_settings *s, const void *bytes, size_t n_bytes, int64_t n_time, bds_probe_out *out);
BDS_API int bds_probe_data_file(bds_ctx *ctx, const bds_settings *s, const char *path, int64_t n_samples, int64_t n_time,
                                bds_probe_out *out);
BDS_API int bds_probe_set_piece_segments(bds_ctx *ctx, int64_t n_segments);
/* ... of a record in DEVICE memory (probeData.m:63-168 on bytes that never were in a file), read where it lies, without a copy:
 * the pointer rule and the ordering rule of the device-record entries above hold, and d_bytes must be aligned to the element size
 * (2 for a 16-bit record; any address for the int8 and packed formats -- the 16-byte loads of the histogram pass cover only the
 * whole aligned lines inside the record, the ragged ends go byte by byte).  Same bits as bds_probe_data on the same bytes.
 * The entry carries a device pointer; its marker has the meaning of the one above and a name of its own, because the five
 * device-record entries are a closed set. */
#define BDS_PROBE_DEV_API __attribute__((visibility("default")))
BDS_PROBE_DEV_API int bds_probe_data_dev(bds_ctx *ctx, const bds_settings *s, const void *d_bytes, size_t n_bytes, int64_t n_time,
                                         bds_probe_out *out);

/* ---- pulse blanking of an IF record (DME / TACAN mitigation in front of acquisition and tracking) ---------------------------
 * B2a lies at 1176.45 MHz inside the aeronautical band; pulse pairs of DME / TACAN beacons reach peak powers tens of dB above the
 * noise floor.  The blanker zeroes the samples around every strong one, on the record's own bytes: int8 real, int8 I/Q pairs,
 * int16 real, int16 I/Q pairs (settings.fileType 1 / 2, dataType 0 / 1 as for bds_track).  The packed 2+2-bit format
 * (fileType 3) has no amplitude to threshold: BDS_ERR_UNSUPPORTED.  A blanked record is an ordinary record of the same format.
 * The rule, in integers only (csrc/bds_blank_math.h):
 *   p[n]     = x^2 of a real sample, I^2 + Q^2 of a pair, as uint32 (at most 2 * 32768^2 = 2^31)
 *   flagged  p[n] > opts.threshold_sq
 *   blanked  there is a flagged m with m - pre <= n <= m + post: the hold-off window around each hit (the skirts of a Gaussian
 *            pulse and the zero crossings of its carrier lie under any threshold); pre and post from 0 to BDS_BLANK_MAX_WINDOW
 *   output   the record with every blanked sample set to 0 (both components of a pair), every other byte unchanged
 * Context: the first opts.lead and the last opts.tail samples of the buffer are read for flags only; they are neither changed
 *   nor counted, and out of place they are copied through.  A piece that carries post samples of the record in front of it and
 *   pre behind gives byte for byte, and in n_flagged and n_blanked count for count, what one call over the whole record gives.
 * Report (bds_blank_out; every value an exact integer, all of the buffer's samples outside lead / tail):
 *   n_samples, n_flagged, n_blanked
 *   n_runs   maximal runs of blanked samples (the pulse count): sample k begins a run when it is blanked and sample k - 1 is
 *            not; the first sample behind `lead` looks at the blanked state the rule gives the last context sample, so a run that
 *            crosses a seam is counted once, by the piece in which it begins.  That state needs one more flag than the bytes do:
 *            the pieces' counts add up to the whole record's when lead is post + 1 (or reaches the record's start); the
 *            library's own pieces (bds_blank, bds_blank_file) carry post + 1.
 *   duty[k]  (when opts.duty_samples > 0) the blanked samples among [k duty_samples, (k + 1) duty_samples), counted from the
 *            first sample behind `lead`; caller-allocated int32[duty_cap], n_duty = ceil(n_samples / duty_samples) bins are
 *            written; duty_samples at most 2^31 - 1.  (Pieces of a caller's own add their bins up at the offsets they know.)
 * bds_blank       n_bytes raw record bytes in host memory, through the device in pieces (bds_blank_file's, 64 MiB of the record
 *                 each); out == in is allowed, a partial overlap is not.
 * bds_blank_file  path_in -> path_out.  The window starts behind settings.skipNumberOfBytes, counted as bds_probe_data_file counts
 *                 it (in samples), and runs for n_samples samples (<= 0: to the end of the file); the bytes in front of it and behind
 *                 it are copied unchanged, so one settings struct reads both files.  Pieces of piece_samples samples (0: 64 MiB of
 *                 the record) are read from the INPUT file with their context and go through two device buffers and two pinned
 *                 host buffers on the context's two streams, piece k + 1 read and uploaded while piece k is worked on.  The result
 *                 does not depend on piece_samples, bit for bit.  piece_samples (when given) below max(pre, post) + 1: BDS_ERR_ARG.
 * bds_blank_dev   the record in DEVICE memory, read and written where it lies; d_out == d_in (in place) or a disjoint buffer.  The
 *                 pointer rule and the ordering rule of the device-record entries hold for both pointers; both must be aligned
 *                 to the element size (2 for a 16-bit record, any address for int8).  The aligned 16-byte lines inside the record
 *                 move as 16-byte loads and stores, the ragged ends byte by byte (a d_out whose address differs from d_in's
 *                 modulo 16 is written byte by byte throughout); no byte outside the record is written.  In place only the 16-byte
 *                 lines that change are written.  Its marker has a name of its own, as BDS_PROBE_DEV_API has.
 * Errors: BDS_ERR_ARG with a message BEFORE ANY DEVICE CALL (with ctx == NULL the message is bds_last_error(NULL)'s) for pre or
 * post negative or above BDS_BLANK_MAX_WINDOW, lead + tail above the buffer's samples, a byte count that is not a whole number of
 * samples (odd for pairs or 16-bit records), duty_cap below n_duty, duty_samples out of range, a partial overlap of in and out,
 * NULL pointers; BDS_ERR_IO when a file cannot be opened, read or written. */
#define BDS_BLANK_TILE 16384          /* samples per tile of the device pass (tests place their cases around it) */
#define BDS_BLANK_MAX_WINDOW 1048576
typedef struct bds_blank_opts {
    uint32_t threshold_sq;
    int32_t pre, post;
    int64_t lead, tail, duty_samples;
} bds_blank_opts;
typedef struct bds_blank_out {
    int64_t n_samples, n_flagged, n_blanked, n_runs;
    int32_t *duty;              /* NULL, or caller-allocated [duty_cap] */
    int64_t duty_cap, n_duty;
} bds_blank_out;
BDS_API int bds_blank(bds_ctx *ctx, const bds_settings *s, const void *in, size_t n_bytes, void *out, const bds_blank_opts *opts,
                      bds_blank_out *report);
BDS_API int bds_blank_file(bds_ctx *ctx, const bds_settings *s, const char *path_in, const char *path_out, int64_t n_samples,
                           int64_t piece_samples, const bds_blank_opts *opts, bds_blank_out *report);
#define BDS_BLANK_DEV_API __attribute__((visibility("default")))
BDS_BLANK_DEV_API int bds_blank_dev(bds_ctx *ctx, const bds_settings *s, const void *d_in, size_t n_bytes, void *d_out,
                                    const bds_blank_opts *opts, bds_blank_out *report);

/* ---- tone excision of an IF record (narrow-band / CW interference in front of acquisition and tracking) -----------------------
 * The blanker can do nothing against a continuous carrier: a CW line stands above any amplitude threshold all the time or never.
 * The excisor estimates each interfering carrier's complex amplitude block by block and subtracts it, on the record's own bytes:
 * int8 real, int8 I/Q pairs, int16 real, int16 I/Q pairs (settings.fileType 1 / 2, dataType 0 / 1).  The packed 2+2-bit format
 * (fileType 3) has no amplitude to subtract from: BDS_ERR_UNSUPPORTED.  A notched record is an ordinary record of the same format.
 * The rule, in integers only (csrc/bds_notch_math.h), so every source, every piece size and the NumPy model of the tests give the
 * same bytes and the same report:
 *   tones    opts.n_tones of them (1 .. BDS_NOTCH_MAX_TONES), each a uint32 phase step per sample in units of 2^-32 turn,
 *            step = floor(f / fs 2^32 + 0.5) mod 2^32 (a negative frequency of an I/Q record is the two's complement).  The phase
 *            of sample n is phi(n) = step (n mod 2^32) mod 2^32; n is the absolute index, opts.first_sample + position in the buffer.
 *   LO       i = ((phi + 2^(31 - P)) >> (32 - P)) mod 2^P, P = BDS_NOTCH_PHASE_BITS; lo(n) = (C[i], S[i]) with
 *            S[i] = rint(L sin(2 pi i / 2^P)), L = 2^BDS_NOTCH_LO_LOG2, C[i] = S[(i + 2^(P - 2)) mod 2^P].  The table is defined by
 *            its first quadrant (f64 on the host) and the exact symmetries of sine; bds_notch_lo hands it out.
 *   blocks   B = 2^opts.block_log2 samples (BDS_NOTCH_MIN_LOG2 .. BDS_NOTCH_MAX_LOG2) on the absolute grid: first_sample mod B == 0;
 *            a last block of r < B samples is allowed.  One notch is fs / B wide.
 *   estimate per block and tone: zr = x C, zi = -x S (real), zr = I C + Q S, zi = Q C - I S (pairs); Sr, Si their int64 sums over
 *            the block's r samples (at most 2^46); ar = floor((2 256 Sr + r L) / (2 r L)), ai alike: the tone's complex amplitude
 *            in 1 / 256 LSB (BDS_NOTCH_AMP_FRAC = 8), int32.  For r = B this is (S + 2^(beta + 5)) >> (beta + 6), beta = block_log2.
 *   subtract er = sum_k (ar_k C_k - ai_k S_k), ei = sum_k (ar_k S_k + ai_k C_k) in int64.  Real: y = x - ((er + 2^20) >> 21) (twice the
 *            real part: the projection of a real tone carries half its amplitude).  Pairs: yI = I - ((er + 2^21) >> 22),
 *            yQ = Q - ((ei + 2^21) >> 22).  Arithmetic shifts; y is saturated to the element's range.
 * The tones are projected independently: two tones D notch widths apart leak about 1 / (pi D) of their amplitude into each other's
 * estimate; a second call on the output removes the remainder.
 * Report (bds_notch_out; every value an exact integer):
 *   n_samples, n_blocks
 *   n_saturated   samples with any saturated component (each counted once)
 *   sum_sq_in, sum_sq_out   sums of x^2 (I^2 + Q^2) before and after, modulo 2^64; their ratio is the removed power
 *   est      (when the caller gives est / est_cap) int32 [n_blocks][n_tones][2]: ar, ai; est_cap counts (ar, ai) pairs
 * opts.apply = 0 estimates only: the output is not touched and may be NULL; sum_sq_out and n_saturated are 0.
 * bds_notch       n_bytes raw record bytes in host memory, through the device in pieces (64 MiB of the record each, whole
 *                 blocks); out == in is allowed, a partial overlap is not.
 * bds_notch_file  path_in -> path_out.  The window starts behind settings.skipNumberOfBytes (counted in samples as
 *                 bds_blank_file counts it), is sample opts.first_sample (0 for a record from its start) and runs for n_samples
 *                 samples (<= 0: to the end of the file); the bytes in front of it and behind it are copied unchanged.  Pieces of
 *                 piece_samples samples, rounded down to whole blocks (0: 64 MiB of the record; below one block: BDS_ERR_ARG), go
 *                 through two device buffers and two pinned host buffers on the context's two streams.  Blocks are
 *                 self-contained, so the pieces' bytes, estimates and sums are the one call's exactly.
 * bds_notch_dev   the record in DEVICE memory, read and written where it lies; d_out == d_in (in place) or a disjoint buffer; both
 *                 aligned to the element size.  Every estimate is finished before any byte is written, and the second pass reads
 *                 only the 16 bytes it writes.  A record whose address is a multiple of 16 moves as 16-byte loads and stores, its
 *                 ragged end byte by byte; any other address is read (written) byte by byte throughout.  No byte outside the
 *                 record is read or written.  A caller working in pieces of its own passes first_sample.
 * bds_notch_lo    the table, C[0 .. 2^P) then S[0 .. 2^P); needs no GPU and no context.
 * Errors: BDS_ERR_ARG with a message BEFORE ANY DEVICE CALL (with ctx == NULL the message is bds_last_error(NULL)'s) for n_tones or
 * block_log2 out of range, first_sample negative or off the block grid, two steps closer than 4 2^(32 - beta) in circular
 * distance, for a real record a step outside (0, 2^31) or closer than 2 2^(32 - beta) to 0 or to 2^31 (there the tone and its image
 * cannot be told apart), a byte count that is not whole samples, a partial overlap of in and out, est_cap below
 * n_blocks x n_tones, NULL pointers; BDS_ERR_IO when a file cannot be opened, read or written. */
#define BDS_NOTCH_MAX_TONES 8
#define BDS_NOTCH_MIN_LOG2 8
#define BDS_NOTCH_MAX_LOG2 16
#define BDS_NOTCH_PHASE_BITS 14
#define BDS_NOTCH_LO_LOG2 14
#define BDS_NOTCH_AMP_FRAC 8
#define BDS_NOTCH_RUN_BYTES 1048576   /* record bytes per workgroup of the device passes: a run of whole blocks (tests cross it) */
typedef struct bds_notch_opts {
    int32_t n_tones, block_log2;
    uint32_t step[BDS_NOTCH_MAX_TONES];
    int64_t first_sample;
    int32_t apply, reserved;    /* apply: 0 estimates only */
} bds_notch_opts;
typedef struct bds_notch_out {
    int64_t n_samples, n_blocks, n_saturated;
    uint64_t sum_sq_in, sum_sq_out;
    int32_t *est;               /* NULL, or caller-allocated [est_cap][2] */
    int64_t est_cap;
} bds_notch_out;
BDS_API int bds_notch(bds_ctx *ctx, const bds_settings *s, const void *in, size_t n_bytes, void *out, const bds_notch_opts *opts,
                      bds_notch_out *report);
BDS_API int bds_notch_file(bds_ctx *ctx, const bds_settings *s, const char *path_in, const char *path_out, int64_t n_samples,
                           int64_t piece_samples, const bds_notch_opts *opts, bds_notch_out *report);
BDS_API int bds_notch_lo(int16_t *cos_sin);
#define BDS_NOTCH_DEV_API __attribute__((visibility("default")))
BDS_NOTCH_DEV_API int bds_notch_dev(bds_ctx *ctx, const bds_settings *s, const void *d_in, size_t n_bytes, void *d_out,
                                    const bds_notch_opts *opts, bds_notch_out *report);

/* ---- weak-signal acquisition: non-coherent power sums of the coarse search over K code periods ------------------------------------
 * acquisition() integrates as long as the reference does: one code period (B2a) or acqCohT ms once (B1C).  bds_acq_deep adds the
 * squared search surfaces of K blocks one code period apart, which acquires satellites 5 - 10 dB below that; beside the
 * acqResults fields it reports deepMetric, the statistic its decision uses.  Nothing of bds_acquire / bds_acq_* changes.
 * The rules (0-based bins b and lags l in the formulas; fbin and codePhase are reported 1-based as in the reference):
 *   sizes    spc = samplesPerCode; N = the reference's block (2 spc for B2a, len10PlusXms for B1C); frq[b] = IF - acqSearchBand +
 *            acqStep b, D bins; s2c = ceil(fs / codeFreqBasis) 2.
 *   blocks   block k = x[k spc : k spc + N], k < K = opts.n_blocks.  m_k[b][l] is the reference's results(b, l) on that block with
 *            the carrier phase counted from the block's first sample: |y_d| + |y_p| (B2a), (sqrt(11) |y_d| + sqrt(29) |y_p|) /
 *            sqrt(40) (B1C, pilotACQflag 1), |y_d| (B1C, pilotACQflag 0).
 *   drift    sh(b, k) = rint(k spc (frq[b] - IF) / carrFreqBasis) samples (half to even), 0 with opts.compensate = 0: a positive
 *            Doppler runs the code fast, so its starts come earlier from block to block.  |sh| must stay below spc.
 *   surface  S[b][l] = sum_k m_k[b][(l - sh(b, k)) mod N]^2: power sums, fp32 arithmetic on fp32 storage, block 0 first.
 *   peak     fbin = the first bin whose row maximum is largest, l0 = the first lag whose column maximum is largest (the
 *            reference's max(max(results, [], 2)) and max(max(results))), S_peak that maximum.
 *   peakMetric   B2a: sqrt(S_peak / S_second), S_second the maximum of row fbin over the reference's codePhaseRange around l0
 *            (B2a/acquisition.m:224-249).  B1C: sqrt(S_peak / sum_k sigPower_k^2), sigPower_k = sqrt(var(x[k spc : k spc + X]) X)
 *            (B1C/acquisition.m:150 on block k).  With K = 1 both are the reference's peakMetric at the reference's cell.
 *   deepMetric   population: all bins x the lags with min(d, spc - d) >= s2c, d = (l - l0) mod spc (the peak and its images one code
 *            period away are left out); mu its mean (f64), S_sec its maximum; deepMetric = (S_peak - mu) / (S_sec - mu).
 *            detected = deepMetric > opts.threshold.  The caller chooses the threshold (> 1; README has noise-only figures).
 *   fine     for detected PRNs, on the reference's grid around frq[fbin]: -acqStep / 2 + 25 j, j = 0 .. round(acqStep / 25) (B2a),
 *            -acqStep + 25 j, j = 0 .. 2 round(acqStep / 25) (B1C).  F(f) = sum_k (w_d |sum_{n < spc} x[a_k + n] c_d(n)
 *            e^{+j 2 pi f n / fs}| + w_p |... c_p ...|)^2 in f64, a_k = l0 + k spc - sh(fbin, k), c the one-period sampling table
 *            of the coarse search, (w_d, w_p) = (1, 1) (B2a), (11 / 40, 29 / 40) (B1C), (1, 0) (B1C without pilot); a sample
 *            index outside the record counts as zero.  carrFreq = the first maximum of F (1 if that is 0 Hz).
 * Results (arrays of max_prn values, index PRN - 1; zero for PRNs that were not searched): peakMetric, deepMetric and fbin for every
 * searched PRN; detected; carrFreq and codePhase (= l0 + 1) where detected, else 0.  The results feed bds_pre_run unchanged.
 * Records: int8 real (is_complex 0) or int8 I/Q pairs (1) with at least N + K spc samples, else BDS_ERR_ARG (B1C's move-back
 * rule therefore never applies); packed records (is_complex 2), settings.dataType 'int16' and settings.resamplingflag 1 are
 * BDS_ERR_UNSUPPORTED.  opts.n_blocks < 1, opts.threshold <= 1 and NULL pointers are BDS_ERR_ARG.  A refused call writes nothing.
 * opts.surface_gib (<= 0: 8) bounds the surfaces (D N 4 bytes per PRN): when those of all searched PRNs do not fit, the PRNs are
 * processed in groups, with the same results bit for bit.  opts.keep_surface keeps the surfaces after the call for
 * bds_acq_deep_row and needs all of them resident (else BDS_ERR_ARG); without it the surface memory is freed before the call
 * returns.  Two calls on the same input give the same bits: every surface element has one writer per launch, no atomics.
 * bds_acq_deep_dev      the same on a record in device memory (the pointer rule of "records in device memory"); it is read, never written.
 * bds_acq_deep_row      row S[bin - 1][0 .. N) of `prn` from the last call (keep_surface); cap counts floats.  Returns N.
 * bds_acq_deep_fine     F over the fine grid of `prn` from the last call; returns the number of grid points, 0 if not detected.
 * bds_acq_deep_release  frees everything the deep search holds on the device (plan, buffers, kept surfaces). */
typedef struct bds_deep_opts {
    int32_t n_blocks;       /* K */
    int32_t compensate;     /* 1: align the blocks by sh(b, k); 0: sh = 0 */
    int32_t keep_surface;
    double threshold;       /* on deepMetric; > 1 */
    double surface_gib;     /* budget of the resident surfaces in GiB; <= 0: 8 */
} bds_deep_opts;
BDS_API int bds_acq_deep(bds_ctx *ctx, const bds_settings *s, const int8_t *samples, size_t n_samples, int is_complex,
                         const bds_deep_opts *opts, int max_prn, double *carrFreq, double *codePhase, double *peakMetric,
                         double *deepMetric, int32_t *fbin, int32_t *detected);
BDS_API int bds_acq_deep_row(bds_ctx *ctx, int prn, int bin, float *row, int64_t cap);
BDS_API int bds_acq_deep_fine(bds_ctx *ctx, int prn, double *F, int cap);
BDS_API int bds_acq_deep_release(bds_ctx *ctx);
#define BDS_DEEP_DEV_API __attribute__((visibility("default")))
BDS_DEEP_DEV_API int bds_acq_deep_dev(bds_ctx *ctx, const bds_settings *s, const void *d_samples, size_t n_samples, int is_complex,
                                      const bds_deep_opts *opts, int max_prn, double *carrFreq, double *codePhase, double *peakMetric,
                                      double *deepMetric, int32_t *fbin, int32_t *detected);

#ifdef __cplusplus
}
#endif
#endif /* BDS_MI355X_H */
