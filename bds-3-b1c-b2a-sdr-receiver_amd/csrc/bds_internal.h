// Internal declarations shared by the translation units of libbds_mi355x.so.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "bds_mi355x.h"

namespace bds {

// host code generation (bds_codes.cpp)
int gen_primary(int signal, bool pilot, int prn, int8_t *out /*10230*/);
int gen_secondary(int prn, int8_t *out /*1800*/);

// MATLAB round(): half away from zero
inline double m_round(double x) { return x >= 0 ? (double)(long long)(x + 0.5) : -(double)(long long)(-x + 0.5); }

// samplesPerCode = round(fs / (codeFreqBasis / codeLength))   (B2a/acquisition.m:130-131)
inline long samples_per_code(const bds_settings &s) {
    return (long)m_round(s.samplingFreq / (s.codeFreqBasis / s.codeLength));
}

// Tuning / test knobs, read from the environment ONCE at bds_create and kept per context (nothing on the
// product path calls getenv afterwards).  Defaults are the measured best; tools/README.md lists them.
struct Tuning {
    int force_l1 = 0, force_l2 = 0;  // BDS_ACQ_FORCE_L1L2=AxB: two-pass factorisation
    int logt = -1;                   // BDS_ACQ_LOGT: log2 of the column tile width
    bool generic = false;            // BDS_ACQ_GENERIC: run-time-radix search kernels
    bool generic_fwd = false;        // BDS_ACQ_GENERIC_FWD: run-time-radix forward transforms
    int group = 0;                   // BDS_ACQ_GROUP: (PRN, bin) cells per launch pair (0 = whole Doppler row)
    int fp16_storage = -1;           // BDS_ACQ_FP16: spectra / inter-pass buffer as fp16 complex (-1 = default on)
    int gchunk = 34;                 // BDS_ACQ_GCHUNK: cells one row-pass workgroup walks through
    bool multi_any = false, nomulti = false;  // BDS_ACQ_MULTI_ANY / BDS_ACQ_NOMULTI: multi-PRN launch pairs
    int pbcells = 0;                 // BDS_ACQ_PBCELLS
    double pbcap_gb = 0;             // BDS_ACQ_PBCAP_GB (hooks): budget of the inter-pass buffer of a multi-PRN launch pair, overrides pair_gb
    bool pair_gb_env = false;        // BDS_ACQ_PAIR_GB was given
    double pair_gb = 40;             // BDS_ACQ_PAIR_GB (release knob): budget of the inter-pass buffer in GiB -- a launch pair carries as many PRNs' Doppler
                                     // rows as fit (default 40: 8 PRNs at cfg3); 0 = minimal (one PRN's row per pair on big grids; small grids batch up
                                     // to 8 GiB), < 0 ("auto") = 60 % of the free device memory
    int rows_grid = 0;                  // BDS_ACQ_ROWS_GRID: workgroups of the (then persistent) row pass; 0 = one per item
    int list_gc = 0;                    // BDS_ACQ_LIST_GC: cells one row workgroup walks in a multi-PRN launch pair (a divisor of D; 0 = chosen by the launch's size -- an N-point plan with Plan::kChunkList then takes the tapered chunk list of rows_chunk_plan instead --, -1 = all D bins of its PRN)
    bool no_bwreuse = false;            // BDS_ACQ_NO_BWREUSE: the B2a second-peak pass runs its own row pass (A/B, tests)
    double kdelta = 0;                  // BDS_ACQ_KDELTA: test hook, sieve tolerance override (0 = per-mode default)
    bool no_selfcheck = false;          // BDS_ACQ_NO_SELFCHECK: timing experiments with invalid results (no re-run)
    bool test_force_fallback = false;   // BDS_ACQ_TEST_FORCE_FALLBACK: test hook, take the fp16 -> fp32 storage re-run
    int test_pair_nomem = 0;            // BDS_ACQ_TEST_PAIR_NOMEM: test hook, the first n allocations of a multi-PRN launch pair's inter-pass buffer are taken to have
                                        // failed (the search halves the PRNs per pair each time)
    int wcols = -1;                  // BDS_ACQ_WCOLS: wave-private column pass (bds_acq_wcols.h); -1 = default on, 0 = the round-2 tile kernel
    int clockprobe = 0;              // BDS_ACQ_CLOCKPROBE: sampled workgroups of the wave-private search kernels time themselves (bds_timing::shader_clock_GHz)
    int wrows = -1;                  // BDS_ACQ_WROWS: wave-private 4096-point row pass (bds_acq_wrows.h); -1 = default on, 0 = k_rows_inv_f
    int pfa = 1;                     // BDS_ACQ_PFA (hooks): the N-point search pairs where they apply (B1C, N = 53 x 12 x 3125: bds_acq_pfa.h, N = 53 x 32 x 625:
                                     // bds_acq_pfa32.h; fp16 storage, whole bins per acqStep); 0 = the L-point pair of rounds 3-5 everywhere
    int pfa_qchunk = 0;              // BDS_ACQ_PFA_QCHUNK (hooks): tiles of a cell (the plan's kTileLags lags each) that follow each other in the N-point column
                                     // passes' work list: the qchunk of Plan::launch_cols (0 = 1)
    int pfa_cgrid = 0;               // BDS_ACQ_PFA_CGRID (hooks): workgroups of the N-point column passes, at most one per work item: the grid of
                                     // Plan::launch_cols (0 = its default rule, bds_acq_pfa.h)
    int small_plan = 1;              // BDS_ACQ_SMALL: small two-component searches on the 80 x 4096 plan (bds_acq_scols.h); 0 = 256 x 1280 as in rounds 1-3
    bool host_refine = false;        // BDS_ACQ_HOSTREFINE: refinement through the host (lists downloaded, jobs built there: rounds 1-4) instead of the device chain
    int neigh = 0;                   // BDS_ACQ_NEIGH: also refine the +-n bin / lag neighbours of every candidate in f64 (rounds 1-3: 1)
    int pk = 1;                      // BDS_ACQ_PK: packed-fp32 butterflies in the wave-private search kernels (bds_fft_pk.h); 0 = one fp32 instruction per real operation
    int ilv = 1;                     // BDS_ACQ_ILV: the wave-private pair of the 768 x 4096 plan keeps both components of an element side by side in the inter-pass buffer (0 = separate planes)
    int wcols_qchunk = 0;            // BDS_ACQ_WCOLS_QCHUNK: adjacent 128-byte lines of a cell its work list keeps together (DRAM page locality; round 3, one PRN per launch:
                                     // 1: 1.84, 2: 1.70, 4: 1.70, 8: 1.75, 16: 1.83 ms per cfg3 launch); 0 = 4 for a launch of one PRN's cells, 2 for a multi-PRN launch (round 5, 32 PRNs
                                     // per pair, per call: 4: 189.0-190.1, 2: 187.9-188.3, 3: 187.9-188.5, 1: 188.5-188.6, 8: 191.4 ms; one PRN per pair: 4 and 2 the same, 1 +1 %)
    bool verbose = false;            // BDS_VERBOSE
    bool multi_force_rccl = false;      // BDS_MULTI_FORCE_RCCL: a single-device bds_multi still goes through RCCL (test hook)
    int trk_nblocks = 0;                // BDS_TRK_NBLOCKS: test hook, correlate workgroups per channel (0 = sized from the code rate)
    int trk_chunk = 0;               // BDS_TRK_CHUNK: samples per correlate workgroup (0 = per-mode default)
    bool trk_nofuse_update = false;  // BDS_TRK_NOFUSE_UPDATE: loop update as its own launch per epoch instead of at the head of the next correlate launch
    bool trk_persample = false;      // BDS_TRK_PERSAMPLE: per-sample tracking correlator instead of the run-based one
    int trk_prec = 4;                // BDS_TRK_PREC: carrier / prefix-sum numerics of the run-based correlator (bds_track.hip, TrkParams::prec; 4 = strict, the default: a sin / cos of the reference's trigarg per sample; 5 = the same argument by angle addition)
    int trk_seg = 0;                 // BDS_TRK_SEG: samples per lane and pass of the run-based correlator (8 / 16; 0 = per-signal default)
    double trk_stream_margin = -1;   // BDS_TRK_STREAM_MARGIN: test hook, margin of a streamed batch's plan in blocks (bds_track.hip, do_track; < 0 = the default, 1);
                                     // 0 plans every epoch that STARTS inside the resident span, so the window guard fires and the batch is repeated
    bool trk_window_nomem = false;   // BDS_TRK_WINDOW_NOMEM: test hook, the allocation of the one window is taken to have failed (the call streams)
};
Tuning tuning_from_env();

struct AcqState;    // bds_acq.hip
struct TrackState;  // bds_track.hip
struct DeepState;   // bds_acq_deep.h (bds_acq.hip)
void deep_state_free(DeepState *);
void acq_state_free(AcqState *);
void acq_state_invalidate(AcqState *);  // forget the configuration (plan, storage mode, cached spectra): re-derived by the next prepare
// The chunk list of the N-point row pass for a launch pair of np PRNs x D cells on `slots` resident workgroups (bds_acq.hip,
// rows_chunk_plan) as (first cell, cells) pairs: the number of chunks, of which the first min(n, cap) are written to out.
int rows_chunk_list(int np, int D, int slots, int *out, int cap);
// The placement and the LDS layout of the N-point row pass (bds_acq_pfa.h) as the kernel takes them: for each workgroup l of a chunk its
// position and 12 mp + k2 (-1: it returns at once) as pairs -- the number of workgroups per chunk, the first min(n, cap) written --, and
// the LDS index of element e of a row (-1 outside 0..3124).
int rows_place_list(int *out, int cap);
int rows_lds_index_of(int e);
void track_state_free(TrackState *);
// bds_track.hip, for bds_corrfn.hip: what an open-loop replay shares with the trackers
struct TrkOpenLoop {
    int mode, pilot, fmt, code_len;  // BDS_TRACK_*, pilot correlators on, kFmt* (bds_trk_replica.h), 10230
    double fs, inv_fs;
    long long n_samples;             // whole samples in the record
    const int8_t *d_prim;            // the per-PRN code tables on the device (bds_trk_replica.h: kTabPad, kTabStride)
    size_t resident_limit;           // bds_track_set_resident_limit (0: none)
};
int track_open_loop_setup(bds_ctx *ctx, const bds_settings &s, size_t n_bytes, TrkOpenLoop &o);
// BDS_OK, or BDS_ERR_ARG with a message naming the context's open tracking session: `who` (a one-shot tracking call, a
// second bds_track_open*) cannot run beside it
int track_session_guard(bds_ctx *ctx, const char *who);
// bds_sync.hip: packed 2+2-bit I/Q bytes (unpack_cplx.m:18-30) -> int8 (I, Q) pairs, device to device on the context's stream
int unpack_cplx_device(bds_ctx *ctx, const uint8_t *d_in, size_t n_bytes, int8_t *d_out);

}  // namespace bds

struct bds_ctx {
    int device = 0;
    void *stream = nullptr;   // hipStream_t: everything is ordered on this stream ...
    void *stream2 = nullptr;  // ... except what runs beside it: the loader of a streamed tracking span (bds_track.hip), the generator of bds_synth_file (bds_synth.hip)
    std::string err;
    std::string devname;
    bds::AcqState *acq = nullptr;
    bds::TrackState *trk = nullptr;
    bds::DeepState *deep = nullptr;  // weak-signal acquisition (bds_acq_deep*): plan, buffers, the last call's surfaces
    bds_timing timing{};
    bds::Tuning tune;
    std::set<const void *> lds_attr_done;  // kernels whose dynamic-LDS limit has been raised on this device
    int n_cu = 0;                          // compute units of the device
    long long probe_piece_segments = 0;    // bds_probe_set_piece_segments: segments per piece of bds_probe_data / _file (0 = 256 MiB of the record)
};

namespace bds {
int fail(bds_ctx *ctx, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));

// Stage markers for `rocprofv3 --marker-trace` (the reference's own stage timing is tic / toc around
// acquisition(), B1C/postProcessing.m:104,112): roctxRangePush / Pop around the forward pass, the search, the refinement and the
// tracking epoch loop.  The ROCTx library is resolved with dlopen at the first range (bds_api.hip) -- no link dependency; without it,
// or outside a profiler, a range costs one predictable branch.
void roctx_push(const char *name);
void roctx_pop();
struct RoctxRange {
    explicit RoctxRange(const char *name) { roctx_push(name); }
    ~RoctxRange() { roctx_pop(); }
    RoctxRange(const RoctxRange &) = delete;
    RoctxRange &operator=(const RoctxRange &) = delete;
};
}

namespace bds {
// The pointer rule of the *_dev entries (include/bds_mi355x.h, "records in device memory"): BDS_OK when [p, p + bytes) is ordinary
// device memory (hipMalloc) of the context's device and lies inside one allocation; otherwise BDS_ERR_ARG with a message that names
// `who`, the argument `arg` and what was found.  Two driver queries, no launch, no copy.  p == NULL with bytes == 0 passes.
int check_device_span(bds_ctx *ctx, const char *who, const char *arg, const void *p, size_t bytes);
}

#define BDS_HIP(ctx, expr)                                                                    \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return bds::fail((ctx), BDS_ERR_HIP, "%s failed: %s (%s:%d)", #expr,               \
                             hipGetErrorString(_e), __FILE__, __LINE__);                       \
    } while (0)

#ifdef __HIPCC__  // (bds_codes.cpp is plain C++ and sees no HIP runtime)
namespace bds {
// a failed HIP call of entry `who` as its return code: BDS_ERR_NOMEM for an allocation that did not fit, else BDS_ERR_HIP
inline int hip_fail(bds_ctx *ctx, const char *who, hipError_t e) {
    return fail(ctx, e == hipErrorOutOfMemory ? BDS_ERR_NOMEM : BDS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
}

// Device allocations, pinned host allocations and events of one call, released on every exit path (or earlier, by release()).
struct DevScope {
    std::vector<void *> mem, host;
    std::vector<hipEvent_t> ev;
    DevScope() = default;
    DevScope(const DevScope &) = delete;
    DevScope &operator=(const DevScope &) = delete;
    template <class T>
    hipError_t alloc(T **q, size_t bytes) {  // at least 8 bytes: an empty shape still gets a pointer a kernel may be handed
        *q = nullptr;
        const hipError_t e = hipMalloc((void **)q, bytes < 8 ? 8 : bytes);
        if (e == hipSuccess) mem.push_back(*q);
        return e;
    }
    template <class T>
    hipError_t pinned(T **q, size_t bytes) {  // page-locked host memory, at least 8 bytes as well
        *q = nullptr;
        const hipError_t e = hipHostMalloc((void **)q, bytes < 8 ? 8 : bytes, hipHostMallocDefault);
        if (e == hipSuccess) host.push_back(*q);
        return e;
    }
    hipError_t event(hipEvent_t *e) {
        const hipError_t r = hipEventCreate(e);
        if (r == hipSuccess) ev.push_back(*e);
        return r;
    }
    void release() {
        for (void *q : mem) (void)hipFree(q);
        for (void *q : host) (void)hipHostFree(q);
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        mem.clear();
        host.clear();
        ev.clear();
    }
    ~DevScope() { release(); }
};
}  // namespace bds
#endif
