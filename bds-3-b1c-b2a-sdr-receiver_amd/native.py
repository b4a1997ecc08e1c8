"""ctypes binding of ``libbds_mi355x.so`` (the C ABI declared in include/bds_mi355x.h).

This is the repo's counterpart of the MEX gateway (mex/bds_mex.c): the same
entry points, called from Python instead of MATLAB.  There is no CPU fallback --
if the library is missing or no GPU is visible the calls raise.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

BDS_MAX_PRN = 63
SIGNAL = {"B1C": 1, "B2A": 2}
TRACK_MODE = {"B2A": 0, "NB": 1, "WB": 2}
CODE_KIND = {"data": 0, "pilot": 1, "data_boc11": 2, "pilot_boc11": 3, "pilot_boc61": 4, "pilot_secondary": 5}
CODE_LEN = {0: 10230, 1: 10230, 2: 20460, 3: 20460, 4: 122760, 5: 1800}

# BDS_LIB_PATH: load another build of the library -- libbds_mi355x_hooks.so (the test-hooks build: tests/conftest.py),
# the debug or sanitizer build; default = the in-tree RELEASE build
_LIB_PATH = os.environ.get("BDS_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libbds_mi355x.so")


class BdsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libbds_mi355x error {code}: {msg}")
        self.code = code


class Settings(C.Structure):
    _fields_ = [
        ("signal", C.c_int32), ("fileType", C.c_int32),
        ("samplingFreq", C.c_double), ("IF", C.c_double), ("codeFreqBasis", C.c_double),
        ("carrFreqBasis", C.c_double),
        ("codeLength", C.c_int32), ("numberOfChannels", C.c_int32),
        ("skipNumberOfBytes", C.c_int64), ("msToProcess", C.c_double),
        ("acqSearchBand", C.c_double), ("acqStep", C.c_double), ("acqThreshold", C.c_double),
        ("acqCohT", C.c_double), ("pilotACQflag", C.c_int32), ("fineNoncoh", C.c_int32),
        ("resamplingThreshold", C.c_double), ("resamplingflag", C.c_int32), ("n_acq", C.c_int32),
        ("acqSatelliteList", C.c_int32 * BDS_MAX_PRN),
        ("pilotTRKflag", C.c_int32), ("intTime", C.c_double),
        ("dllCorrelatorSpacing", C.c_double), ("dllDampingRatio", C.c_double),
        ("dllNoiseBandwidth", C.c_double), ("pllNoiseBandwidth", C.c_double),
        ("CNoInterval", C.c_int32), ("dataType", C.c_int32), ("FEBW", C.c_double),
    ]


class Channel(C.Structure):
    _fields_ = [("PRN", C.c_int32), ("status", C.c_int32), ("acquiredFreq", C.c_double),
                ("codePhase", C.c_double), ("codeFreq", C.c_double)]


_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int32)

TRACK_FIELDS = ["absoluteSample", "codeFreq", "carrFreq", "I_P", "I_E", "I_L", "Q_E", "Q_P", "Q_L",
                "Pilot_I_P", "Pilot_Q_P", "Pilot_I_E", "Pilot_I_L", "Pilot_Q_E", "Pilot_Q_L",
                "dllDiscr", "dllDiscrFilt", "pllDiscr", "pllDiscrFilt", "remCodePhase", "remCarrPhase",
                "DataCNo", "DataPLD", "PilotCNo", "PilotPLD", "SigCNo"]


class TrackOut(C.Structure):
    _fields_ = ([("n_ch", C.c_int32), ("n_epochs", C.c_int32), ("n_cno", C.c_int32), ("reserved0", C.c_int32)]
                + [(f, _DP) for f in TRACK_FIELDS] + [("completed", _IP), ("status", _IP)])


class Timing(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("forward_ms", C.c_double), ("search_ms", C.c_double),
                ("refine_ms", C.c_double), ("cell_pair_ms", C.c_double), ("cells_per_pair", C.c_double),
                ("n_pairs", C.c_int64), ("fft_len", C.c_int64), ("n_circ", C.c_int64),
                ("n_bins", C.c_int32), ("n_prn", C.c_int32), ("n_comp", C.c_int32), ("half_storage", C.c_int32),
                ("rows_ms", C.c_double), ("cols_ms", C.c_double), ("n_extra", C.c_int64), ("shader_clock_GHz", C.c_double),
                ("plan_l1", C.c_int32), ("plan_l2", C.c_int32), ("rows_kernel", C.c_int32), ("cols_kernel", C.c_int32),
                ("kernel_flags", C.c_int32), ("refine_path", C.c_int32)]


class AcqJob(C.Structure):
    _fields_ = [("settings", C.POINTER(Settings)), ("samples", C.POINTER(C.c_int8)), ("n_samples", C.c_size_t),
                ("is_complex", C.c_int32), ("max_prn", C.c_int32), ("carrFreq", _DP), ("codePhase", _DP),
                ("peakMetric", _DP), ("detected", _IP)]


class SynthSat(C.Structure):
    _fields_ = [("prn", C.c_int32), ("reserved0", C.c_int32), ("doppler", C.c_double), ("delay", C.c_double),
                ("phase", C.c_double), ("cn0_dbhz", C.c_double)]


class SynthOpts(C.Structure):
    _fields_ = [("size", C.c_int32), ("format", C.c_int32), ("iq_sign", C.c_int32), ("code_doppler", C.c_int32),
                ("pilot61_secondary", C.c_int32), ("reserved0", C.c_int32), ("seed", C.c_uint64), ("sigma", C.c_double),
                ("threshold", C.c_double), ("symbols", C.POINTER(C.c_int8)), ("n_sym", C.c_int64)]


class SynthSeg(C.Structure):
    _fields_ = [("period0", C.c_int64), ("code", C.c_double * 4), ("carr", C.c_double * 4)]


class SynthTraj(C.Structure):
    _fields_ = [("size", C.c_int32), ("seg_log2", C.c_int32), ("first", C.c_int64), ("n_seg", C.c_int64), ("seg", C.POINTER(SynthSeg))]


# bds_synth_seg as a NumPy structured dtype (72 bytes, no padding): what synth.Trajectory holds
SYNTH_SEG_DTYPE = np.dtype([("period0", np.int64), ("code", np.float64, 4), ("carr", np.float64, 4)])


# the doubles of bds_eph, in the order of BDS_EPH_FIELDS (include/bds_mi355x.h)
EPH_FIELDS = ["PRN", "SOH", "SOW", "WN", "HOW", "IODC", "IODE", "IODC_MSB2", "IODC_LSB8",
              "t_oe", "deltaA", "ADot", "delta_n_0", "delta_n_0Dot", "M_0", "e", "omega",
              "omega_0", "i_0", "omegaDot", "i_0Dot", "C_is", "C_ic", "C_rs", "C_rc", "C_us", "C_uc",
              "t_oc", "a_0", "a_1", "a_2", "T_GDB2ap", "ISC_B1Cd", "T_GDB1Cp",
              "PageID1", "PageID3", "HS", "DIF", "SIF", "AIF", "SISMAI",
              "alpha1", "alpha2", "alpha3", "alpha4", "alpha5", "alpha6", "alpha7", "alpha8", "alpha9",
              "A_0UTC", "A_1UTC", "A_2UTC", "delta_t_LS", "t_ot", "WN_ot", "WN_LSF", "DN", "delta_t_LSF",
              "GNSS_ID", "WN_0BGTO", "t_0BGTO", "A_0BGTO", "A_1BGTO", "A_2BGTO", "TOW"]
NAV_SHORT, NAV_BCH1_OK, NAV_BCH2_OK, NAV_CRC1_OK, NAV_CRC2_OK, NAV_ENTERED, NAV_PRN_RANGE = 1, 2, 4, 8, 16, 32, 64
NAV_BITS = {1: 878, 2: 288}  # by SIGNAL value


class NavFrame(C.Structure):
    _fields_ = [("size", C.c_uint32), ("index", C.c_int32), ("status", C.c_uint32), ("polarity", C.c_int32),
                ("bch1_max", C.c_int32), ("bch2_max", C.c_int32), ("bits", C.c_uint8 * 112)]


class Eph(C.Structure):
    _fields_ = ([("size", C.c_uint32), ("flag", C.c_int32), ("SatType", C.c_int32), ("n_entered", C.c_int32),
                 ("idValid", C.c_int32 * 8)] + [(f, C.c_double) for f in EPH_FIELDS])


# bds_pvt_params / bds_pvt_out and the BDS_PVT_* flags of bds_pvt_plan's ready list (include/bds_mi355x.h)
PVT_READY, PVT_IDLE, PVT_NO_EPH, PVT_NO_SATTYPE, PVT_NO_FRAME = 1, 2, 4, 8, 16
PVT_SETTINGS = ["navSolPeriod", "elevationMask", "useTropCorr", "c", "startOffset"]
PVT_CHANNEL_FIELDS = ["PRN", "el", "az", "transmitTime", "satClkCorr", "rawP", "correctedP"]  # [n_ch, n_meas]
PVT_EPOCH_FIELDS = ["X", "Y", "Z", "dt", "localTime", "currMeasSample", "latitude", "longitude", "height"]  # [n_meas]; DOP is [5, n_meas]


class PvtParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("useTropCorr", C.c_int32), ("navSolPeriod", C.c_double), ("elevationMask", C.c_double),
                ("c", C.c_double), ("startOffset", C.c_double)]


class PvtOut(C.Structure):
    _fields_ = ([("size", C.c_uint32), ("cap", C.c_int32)]
                + [(f, C.POINTER(C.c_double)) for f in PVT_CHANNEL_FIELDS + ["DOP"] + PVT_EPOCH_FIELDS])


class ProbeOut(C.Structure):
    _fields_ = ([("hist_i", C.POINTER(C.c_int64)), ("hist_q", C.POINTER(C.c_int64))]
                + [(f"{k}_{c}", C.c_int64) for c in "iq" for k in ("min", "max", "sum", "sumsq")]
                + [("psd", C.POINTER(C.c_double)), ("cap", C.c_int32), ("n_psd", C.c_int32), ("n_segments", C.c_int64), ("n_samples", C.c_int64),
                   ("excerpt_re", C.POINTER(C.c_double)), ("excerpt_im", C.POINTER(C.c_double))])


class BlankOpts(C.Structure):
    _fields_ = [("threshold_sq", C.c_uint32), ("pre", C.c_int32), ("post", C.c_int32), ("lead", C.c_int64), ("tail", C.c_int64),
                ("duty_samples", C.c_int64)]


class BlankOut(C.Structure):
    _fields_ = [("n_samples", C.c_int64), ("n_flagged", C.c_int64), ("n_blanked", C.c_int64), ("n_runs", C.c_int64),
                ("duty", C.POINTER(C.c_int32)), ("duty_cap", C.c_int64), ("n_duty", C.c_int64)]


class DeepOpts(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("compensate", C.c_int32), ("keep_surface", C.c_int32), ("threshold", C.c_double),
                ("surface_gib", C.c_double)]


class NotchOpts(C.Structure):
    _fields_ = [("n_tones", C.c_int32), ("block_log2", C.c_int32), ("step", C.c_uint32 * 8), ("first_sample", C.c_int64),
                ("apply", C.c_int32), ("reserved", C.c_int32)]


class NotchOut(C.Structure):
    _fields_ = [("n_samples", C.c_int64), ("n_blocks", C.c_int64), ("n_saturated", C.c_int64), ("sum_sq_in", C.c_uint64),
                ("sum_sq_out", C.c_uint64), ("est", C.POINTER(C.c_int32)), ("est_cap", C.c_int64)]


NOTCH_MAX_TONES = 8          # BDS_NOTCH_MAX_TONES
NOTCH_MIN_LOG2 = 8           # BDS_NOTCH_MIN_LOG2
NOTCH_MAX_LOG2 = 16          # BDS_NOTCH_MAX_LOG2
NOTCH_PHASE_BITS = 14        # BDS_NOTCH_PHASE_BITS: the LO table holds 2^14 entries
NOTCH_LO_LOG2 = 14           # BDS_NOTCH_LO_LOG2: its amplitude L = 2^14
NOTCH_AMP_FRAC = 8           # BDS_NOTCH_AMP_FRAC: estimates in 1 / 256 LSB
NOTCH_RUN_BYTES = 1048576    # BDS_NOTCH_RUN_BYTES: record bytes per workgroup of the excisor's device passes

BLANK_TILE = 16384           # BDS_BLANK_TILE: samples per tile of the blanker's device pass
BLANK_MAX_WINDOW = 1048576   # BDS_BLANK_MAX_WINDOW: the largest pre / post

SYNTH_FORMATS = {0: (np.float64, 1, 1), 1: (np.int8, 1, 1), 2: (np.int8, 2, 1), 3: (np.uint8, 1, 2)}  # dtype, elements per `den` samples


# per-channel state of the update test aid (bds_track_update), in the order of its state10 rows
UPDATE_STATE = ["codeFreq", "remCodePhase", "carrFreq", "carrFreqBasis", "remCarrPhase", "oldCodeNco", "oldCodeError", "d2CarrError",
                "dCarrError", "codeFreqBasis"]

EXPORTS = [
    "bds_create", "bds_destroy", "bds_reload_tuning", "bds_last_error", "bds_device_name", "bds_abi_check", "bds_build_flags", "bds_gen_code", "bds_acquire",
    "bds_acq_load", "bds_acq_prepare", "bds_acq_run", "bds_acq_set_pair_budget_gb", "bds_acq_set_b2a_npoint", "bds_acq_set_b1c_npoint", "bds_resample_plan", "bds_fir1_bandpass", "bds_frame_sync", "bds_sync_pattern", "bds_unpack_cplx", "bds_unpack_cplx_file", "bds_acq_grid", "bds_acq_peaks", "bds_acq_candidates", "bds_acq_coherent_sums", "bds_acq_block", "bds_get_timing",
    "bds_acquire16", "bds_acq_load16", "bds_acquire_track16",
    "bds_acq_deep", "bds_acq_deep_row", "bds_acq_deep_fine", "bds_acq_deep_release",
    "bds_track", "bds_track_mem", "bds_track_loaded_bytes", "bds_track_set_resident_limit", "bds_track_stream_info", "bds_track_correlate", "bds_track_colon", "bds_track_cno", "bds_track_update",
    "bds_track_open", "bds_track_open_mem", "bds_track_open_feed", "bds_track_feed", "bds_track_advance", "bds_track_session_info", "bds_track_close",
    "bds_calc_loop_coef", "bds_calc_loop_coef_carr",
    "bds_calc_weighing_factor", "bds_pre_run", "bds_pre_run_device", "bds_acquire_track",
    "bds_multi_create", "bds_multi_destroy", "bds_multi_last_error", "bds_multi_size", "bds_multi_ctx",
    "bds_multi_rccl_ranks", "bds_acquire_multi", "bds_shard_jobs", "bds_acq_job_cost",
    "bds_synth", "bds_synth_file", "bds_synth_noise", "bds_synth_trajectory", "bds_synth_traj",
    "bds_probe_data", "bds_probe_data_file", "bds_probe_set_piece_segments",
    "bds_blank", "bds_blank_file",
    "bds_notch", "bds_notch_file", "bds_notch_lo",
    "bds_corr_function", "bds_corr_function_mem",
    "bds_nav_decode", "bds_nav_fields",
    "bds_pvt_plan", "bds_pvt_measure", "bds_pvt_solve", "bds_post_navigation",
]
# the entries marked BDS_DEV_API in the header: their record pointer is device memory (device_span below makes it)
DEVICE_EXPORTS = ["bds_synth_dev", "bds_acq_load_dev", "bds_track_dev", "bds_track_open_dev", "bds_track_feed_dev"]
# the entry marked BDS_SYNTH_DEV_API: a device pointer as well
SYNTH_DEVICE_EXPORTS = ["bds_synth_traj_dev"]
# the entry marked BDS_PROBE_DEV_API: a device pointer as well
PROBE_DEVICE_EXPORTS = ["bds_probe_data_dev"]
# the entry marked BDS_BLANK_DEV_API: device pointers as well (record in, record out)
BLANK_DEVICE_EXPORTS = ["bds_blank_dev"]
# the entry marked BDS_NOTCH_DEV_API: device pointers as well (record in, record out)
NOTCH_DEVICE_EXPORTS = ["bds_notch_dev"]
# the entry marked BDS_DEEP_DEV_API: a device pointer as well
DEEP_DEVICE_EXPORTS = ["bds_acq_deep_dev"]
# the entry marked BDS_CORR_DEV_API: a device pointer as well
CORR_DEVICE_EXPORTS = ["bds_corr_function_dev"]

_lib = None
HOOKS_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libbds_mi355x_hooks.so")


def has_test_hooks():
    """True when the loaded library is the test-hooks build (reads the tuning / test environment switches)."""
    return bool(lib().bds_build_flags() & 1)


def lib():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ImportError(f"{_LIB_PATH} is missing: run ./build.sh (or __graft_entry__.build()); "
                          "there is no CPU fallback")
    # Share ONE HIP runtime with PyTorch when both live in a process: torch bundles its own
    # libamdhip64.so.7; importing it first makes the loader reuse it for our DT_NEEDED entry.
    try:
        import torch  # noqa: F401
    except Exception:  # torch is plumbing only; the library also runs without it
        pass
    L = C.CDLL(_LIB_PATH)
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    i8p = C.POINTER(C.c_int8)
    SP = C.POINTER(Settings)
    L.bds_create.restype, L.bds_create.argtypes = vp, [i32]
    L.bds_destroy.restype, L.bds_destroy.argtypes = None, [vp]
    L.bds_reload_tuning.restype, L.bds_reload_tuning.argtypes = i32, [vp]
    L.bds_build_flags.restype, L.bds_build_flags.argtypes = i32, []
    L.bds_track_loaded_bytes.restype, L.bds_track_loaded_bytes.argtypes = C.c_longlong, [vp]
    L.bds_multi_create.restype, L.bds_multi_create.argtypes = vp, [i32, _IP]
    L.bds_multi_destroy.restype, L.bds_multi_destroy.argtypes = None, [vp]
    L.bds_multi_last_error.restype, L.bds_multi_last_error.argtypes = C.c_char_p, [vp]
    L.bds_multi_size.restype, L.bds_multi_size.argtypes = i32, [vp]
    L.bds_multi_ctx.restype, L.bds_multi_ctx.argtypes = vp, [vp, i32]
    L.bds_multi_rccl_ranks.restype, L.bds_multi_rccl_ranks.argtypes = i32, [vp]
    L.bds_acquire_multi.restype, L.bds_acquire_multi.argtypes = i32, [vp, i32, C.POINTER(AcqJob)]
    L.bds_shard_jobs.restype, L.bds_shard_jobs.argtypes = i32, [i32, _DP, i32, _IP]
    L.bds_acq_job_cost.restype, L.bds_acq_job_cost.argtypes = C.c_double, [SP]
    L.bds_last_error.restype, L.bds_last_error.argtypes = C.c_char_p, [vp]
    L.bds_device_name.restype, L.bds_device_name.argtypes = i32, [vp, C.c_char_p, i32]
    L.bds_gen_code.restype, L.bds_gen_code.argtypes = i32, [i32, i32, i32, i8p, i32]
    L.bds_acquire.restype = i32
    L.bds_acquire.argtypes = [vp, SP, i8p, sz, i32, i32, _DP, _DP, _DP, _IP]
    L.bds_acq_load.restype, L.bds_acq_load.argtypes = i32, [vp, SP, i8p, sz, i32]
    if hasattr(L, "bds_acquire16"):  # (a build of an older commit, loaded through BDS_LIB_PATH for an A/B run, takes int8 blocks only)
        i16p = C.POINTER(C.c_int16)
        L.bds_acquire16.restype, L.bds_acquire16.argtypes = i32, [vp, SP, i16p, sz, i32, i32, _DP, _DP, _DP, _IP]
        L.bds_acq_load16.restype, L.bds_acq_load16.argtypes = i32, [vp, SP, i16p, sz, i32]
        L.bds_acquire_track16.restype = i32
        L.bds_acquire_track16.argtypes = [vp, SP, i16p, sz, i32, i32, _DP, _DP, _DP, _IP, C.c_char_p, C.POINTER(Channel), C.POINTER(TrackOut)]
    L.bds_acq_prepare.restype, L.bds_acq_prepare.argtypes = i32, [vp, SP]
    L.bds_acq_run.restype = i32
    L.bds_acq_run.argtypes = [vp, SP, _IP, i32, i32, _DP, _DP, _DP, _IP]
    L.bds_acq_grid.restype, L.bds_acq_grid.argtypes = i32, [vp, C.POINTER(C.c_float), _IP, i32]
    L.bds_acq_candidates.restype, L.bds_acq_candidates.argtypes = i32, [vp, i32, _IP, C.POINTER(C.c_int64), i32]
    L.bds_acq_peaks.restype, L.bds_acq_peaks.argtypes = i32, [vp, i32, _DP, _DP, _IP]
    L.bds_acq_coherent_sums.restype = i32
    L.bds_acq_coherent_sums.argtypes = [vp, SP, i32, C.c_int64, _DP, i32, i32, _DP, i32]
    if hasattr(L, "bds_acq_block"):  # (a build of an older commit, loaded through BDS_LIB_PATH for an A/B run, has no block test aid)
        L.bds_acq_block.restype, L.bds_acq_block.argtypes = i32, [vp, _DP, _DP, sz, C.POINTER(C.c_longlong)]
    L.bds_get_timing.restype, L.bds_get_timing.argtypes = i32, [vp, C.POINTER(Timing)]
    L.bds_track.restype = i32
    L.bds_track.argtypes = [vp, SP, C.c_char_p, i32, C.POINTER(Channel), C.POINTER(TrackOut)]
    L.bds_track_mem.restype = i32
    L.bds_track_mem.argtypes = [vp, SP, i8p, sz, i32, C.POINTER(Channel), C.POINTER(TrackOut)]
    if hasattr(L, "bds_track_set_resident_limit"):  # (a build of an older commit, loaded through BDS_LIB_PATH for an A/B run, has no streamed mode)
        L.bds_track_set_resident_limit.restype, L.bds_track_set_resident_limit.argtypes = i32, [vp, sz]
        L.bds_track_stream_info.restype = i32
        L.bds_track_stream_info.argtypes = [vp, _IP, C.POINTER(C.c_longlong), _IP]
    if hasattr(L, "bds_track_open"):  # (as above: a build of an older commit has no tracking sessions)
        CP, OP, LLP = C.POINTER(Channel), C.POINTER(TrackOut), C.POINTER(C.c_longlong)
        L.bds_track_open.restype, L.bds_track_open.argtypes = vp, [vp, SP, C.c_char_p, i32, CP]
        L.bds_track_open_mem.restype, L.bds_track_open_mem.argtypes = vp, [vp, SP, i8p, sz, i32, CP]
        L.bds_track_open_feed.restype, L.bds_track_open_feed.argtypes = vp, [vp, SP, C.c_longlong, i32, CP]
        L.bds_track_feed.restype, L.bds_track_feed.argtypes = i32, [vp, i8p, sz, i32]
        L.bds_track_advance.restype, L.bds_track_advance.argtypes = i32, [vp, i32, OP, _IP]
        L.bds_track_session_info.restype, L.bds_track_session_info.argtypes = i32, [vp, _IP, LLP, LLP, LLP]
        L.bds_track_close.restype, L.bds_track_close.argtypes = None, [vp]
    L.bds_track_correlate.restype = i32
    L.bds_track_correlate.argtypes = [vp, SP, i8p, sz, i32, _IP, _DP, _DP]
    L.bds_track_colon.restype, L.bds_track_colon.argtypes = i32, [vp, i32, _DP, _DP, _DP, _IP, _DP, _DP, _IP]
    if hasattr(L, "bds_track_cno"):  # (as above: a build of an older commit has no scalar-stage test aids)
        L.bds_track_cno.restype, L.bds_track_cno.argtypes = i32, [vp, SP, i32, i32, _DP, _IP, i32, _IP, i32, _DP]
        L.bds_track_update.restype, L.bds_track_update.argtypes = i32, [vp, SP, i32, _DP, _DP, _DP, _IP, _IP, _DP]
    L.bds_calc_loop_coef.restype = None
    L.bds_calc_loop_coef.argtypes = [C.c_double, C.c_double, C.c_double, _DP, _DP]
    L.bds_calc_loop_coef_carr.restype, L.bds_calc_loop_coef_carr.argtypes = None, [SP, _DP, _DP, _DP]
    L.bds_calc_weighing_factor.restype, L.bds_calc_weighing_factor.argtypes = C.c_double, [SP]
    L.bds_pre_run.restype = i32
    L.bds_frame_sync.restype = i32
    L.bds_frame_sync.argtypes = [vp, i32, i32, _IP, _DP, i32, _IP, _IP, _IP, i32]
    L.bds_sync_pattern.restype, L.bds_sync_pattern.argtypes = i32, [i32, i32, C.POINTER(C.c_int8), i32]
    L.bds_nav_decode.restype = i32
    L.bds_nav_decode.argtypes = [vp, SP, i32, _IP, _DP, _DP, i32, C.POINTER(NavFrame), _IP, i32, C.POINTER(Eph), _DP, _DP]
    L.bds_nav_fields.restype, L.bds_nav_fields.argtypes = i32, [i32, C.POINTER(C.c_uint8), i32, i32, C.POINTER(Eph)]
    PP, EP, dbl = C.POINTER(PvtParams), C.POINTER(Eph), C.c_double
    L.bds_pvt_plan.restype, L.bds_pvt_plan.argtypes = i32, [SP, PP, i32, i32, C.c_char_p, _DP, EP, _DP, _DP, _IP, _DP, _DP, _DP]
    L.bds_pvt_measure.restype = i32
    L.bds_pvt_measure.argtypes = [vp, SP, i32, i32, _IP, _DP, _DP, _DP, EP, _DP, _DP, dbl, dbl, i32, _DP, _DP, _DP]
    L.bds_pvt_solve.restype = i32
    L.bds_pvt_solve.argtypes = [SP, PP, i32, i32, _IP, _IP, dbl, dbl, _DP, _DP, _DP, C.POINTER(PvtOut)]
    L.bds_post_navigation.restype = i32
    L.bds_post_navigation.argtypes = [vp, SP, PP, i32, i32, C.c_char_p, _IP, _DP, _DP, _DP, EP, _DP, _DP, _IP, _IP, C.POINTER(PvtOut)]
    L.bds_unpack_cplx.restype, L.bds_unpack_cplx.argtypes = i32, [vp, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_int8)]
    L.bds_unpack_cplx_file.restype, L.bds_unpack_cplx_file.argtypes = i32, [vp, C.c_char_p, C.c_char_p]
    L.bds_resample_plan.restype, L.bds_resample_plan.argtypes = i32, [SP, _DP, _DP, _DP]
    L.bds_fir1_bandpass.restype, L.bds_fir1_bandpass.argtypes = i32, [i32, C.c_double, C.c_double, _DP]
    L.bds_pre_run.argtypes = [SP, i32, _DP, _DP, _DP, C.POINTER(Channel)]
    L.bds_pre_run_device.restype, L.bds_pre_run_device.argtypes = i32, [vp, SP, i32, _DP, _DP, _DP, C.POINTER(Channel)]
    L.bds_acquire_track.restype = i32
    L.bds_acquire_track.argtypes = [vp, SP, i8p, sz, i32, i32, _DP, _DP, _DP, _IP, C.c_char_p, C.POINTER(Channel), C.POINTER(TrackOut)]
    if hasattr(L, "bds_synth"):  # (as above: a build of an older commit has no device generator)
        YP, OP, i64 = C.POINTER(SynthSat), C.POINTER(SynthOpts), C.c_int64
        L.bds_synth.restype, L.bds_synth.argtypes = i32, [vp, SP, i32, YP, OP, i64, i64, vp, sz]
        L.bds_synth_file.restype, L.bds_synth_file.argtypes = i32, [vp, SP, i32, YP, OP, i64, i64, C.c_char_p, i64]
        L.bds_synth_noise.restype, L.bds_synth_noise.argtypes = i32, [vp, C.c_uint64, i64, i64, _DP, _DP]
    if hasattr(L, "bds_synth_dev"):  # (as above: a build of an older commit takes no record in device memory)
        L.bds_synth_dev.restype, L.bds_synth_dev.argtypes = i32, [vp, SP, i32, YP, OP, i64, i64, vp, sz]
        L.bds_acq_load_dev.restype, L.bds_acq_load_dev.argtypes = i32, [vp, SP, vp, sz, i32]
        L.bds_track_dev.restype = i32
        L.bds_track_dev.argtypes = [vp, SP, vp, sz, i32, C.POINTER(Channel), C.POINTER(TrackOut)]
        L.bds_track_open_dev.restype, L.bds_track_open_dev.argtypes = vp, [vp, SP, vp, sz, i32, C.POINTER(Channel)]
        L.bds_track_feed_dev.restype, L.bds_track_feed_dev.argtypes = i32, [vp, vp, sz, i32]
    if hasattr(L, "bds_synth_traj"):  # (as above: a build of an older commit has no trajectory path)
        TP = C.POINTER(SynthTraj)
        L.bds_synth_trajectory.restype = i32
        L.bds_synth_trajectory.argtypes = [SP, i32, C.POINTER(Eph), _DP, C.c_double, C.c_double, i64, i64, i32, C.POINTER(SynthSeg)]
        L.bds_synth_traj.restype, L.bds_synth_traj.argtypes = i32, [vp, SP, i32, YP, OP, TP, i64, i64, vp, sz]
        L.bds_synth_traj_dev.restype, L.bds_synth_traj_dev.argtypes = i32, [vp, SP, i32, YP, OP, TP, i64, i64, vp, sz]
    if hasattr(L, "bds_probe_data"):  # (as above: a build of an older commit has no probeData)
        PP, i64 = C.POINTER(ProbeOut), C.c_int64
        L.bds_probe_data.restype, L.bds_probe_data.argtypes = i32, [vp, SP, vp, sz, i64, PP]
        L.bds_probe_data_file.restype, L.bds_probe_data_file.argtypes = i32, [vp, SP, C.c_char_p, i64, i64, PP]
        L.bds_probe_data_dev.restype, L.bds_probe_data_dev.argtypes = i32, [vp, SP, vp, sz, i64, PP]
        L.bds_probe_set_piece_segments.restype, L.bds_probe_set_piece_segments.argtypes = i32, [vp, i64]
    if hasattr(L, "bds_blank"):  # (as above: a build of an older commit has no pulse blanker)
        BO, BR, i64 = C.POINTER(BlankOpts), C.POINTER(BlankOut), C.c_int64
        L.bds_blank.restype, L.bds_blank.argtypes = i32, [vp, SP, vp, sz, vp, BO, BR]
        L.bds_blank_file.restype, L.bds_blank_file.argtypes = i32, [vp, SP, C.c_char_p, C.c_char_p, i64, i64, BO, BR]
        L.bds_blank_dev.restype, L.bds_blank_dev.argtypes = i32, [vp, SP, vp, sz, vp, BO, BR]
    if hasattr(L, "bds_notch"):  # (as above: a build of an older commit has no tone excisor)
        NO, NR, i64 = C.POINTER(NotchOpts), C.POINTER(NotchOut), C.c_int64
        L.bds_notch.restype, L.bds_notch.argtypes = i32, [vp, SP, vp, sz, vp, NO, NR]
        L.bds_notch_file.restype, L.bds_notch_file.argtypes = i32, [vp, SP, C.c_char_p, C.c_char_p, i64, i64, NO, NR]
        L.bds_notch_dev.restype, L.bds_notch_dev.argtypes = i32, [vp, SP, vp, sz, vp, NO, NR]
        L.bds_notch_lo.restype, L.bds_notch_lo.argtypes = i32, [C.POINTER(C.c_int16)]
    if hasattr(L, "bds_acq_deep"):  # (as above: a build of an older commit has no weak-signal acquisition)
        tail = [sz, i32, C.POINTER(DeepOpts), i32, _DP, _DP, _DP, _DP, _IP, _IP]
        L.bds_acq_deep.restype, L.bds_acq_deep.argtypes = i32, [vp, SP, i8p] + tail
        L.bds_acq_deep_dev.restype, L.bds_acq_deep_dev.argtypes = i32, [vp, SP, vp] + tail
        L.bds_acq_deep_row.restype, L.bds_acq_deep_row.argtypes = i32, [vp, i32, i32, C.POINTER(C.c_float), C.c_int64]
        L.bds_acq_deep_fine.restype, L.bds_acq_deep_fine.argtypes = i32, [vp, i32, _DP, i32]
        L.bds_acq_deep_release.restype, L.bds_acq_deep_release.argtypes = i32, [vp]
    if hasattr(L, "bds_corr_function"):  # (as above: a build of an older commit has no correlation function)
        tail = [i32, _IP, _DP, i32, _DP, _DP, _IP]  # n_items, prn, state6, n_taps, taps, out, n_comp
        L.bds_corr_function.restype, L.bds_corr_function.argtypes = i32, [vp, SP, C.c_char_p] + tail
        L.bds_corr_function_mem.restype, L.bds_corr_function_mem.argtypes = i32, [vp, SP, i8p, sz] + tail
        L.bds_corr_function_dev.restype, L.bds_corr_function_dev.argtypes = i32, [vp, SP, vp, sz] + tail
    L.bds_abi_check.restype, L.bds_abi_check.argtypes = i32, [i32, i32, i32, i32]
    if L.bds_abi_check(C.sizeof(Settings), C.sizeof(Channel), C.sizeof(TrackOut), C.sizeof(Timing)) != 0:
        raise ImportError("ctypes struct layout does not match libbds_mi355x.so (include/bds_mi355x.h changed?)")
    _lib = L
    return L


def debug_failures() -> int:
    """Failed device-side bounds checks since the last call; 0 on the product build (only the debug build, BDS_DEBUG=1
    ./build.sh, exports the counter) or when the library was never loaded."""
    if _lib is None or not hasattr(_lib, "bds_debug_failures"):
        return 0
    _lib.bds_debug_failures.restype = C.c_uint
    return int(_lib.bds_debug_failures())


def pack_settings(s) -> Settings:
    """MATLAB-style settings struct -> bds_settings.  Every field of SURVEY.md Appendix D that the selected
    receiver's initSettings.m defines is REQUIRED (a missing or misspelt field is an error naming it, never a silent
    default) -- the same rule as mex/bds_mex.c:pack_settings."""
    cs = Settings()
    sig = str(getattr(s, "signal", "")).upper()
    if sig not in SIGNAL:
        raise ValueError("settings.signal must be 'B1C' or 'B2A'")
    cs.signal = SIGNAL[sig]

    def need(name):
        if not hasattr(s, name):
            raise AttributeError(f"settings.{name} is missing")
        return getattr(s, name)

    # 'schar' / 'int8' -> 0, 'int16' / 'short' -> 1; every other type ('float32', ...) -> a value the library refuses
    # (BDS_ERR_UNSUPPORTED names the field), so that such a file is never read as int16
    cs.dataType = data_type_code(need("dataType"))
    cs.fileType = int(need("fileType"))
    cs.samplingFreq = float(need("samplingFreq"))
    cs.IF = float(need("IF"))
    cs.codeFreqBasis = float(need("codeFreqBasis"))
    cs.carrFreqBasis = float(need("carrFreqBasis"))
    cs.codeLength = int(need("codeLength"))
    cs.numberOfChannels = int(need("numberOfChannels"))
    cs.skipNumberOfBytes = int(need("skipNumberOfBytes"))
    cs.msToProcess = float(need("msToProcess"))
    cs.acqSearchBand = float(need("acqSearchBand"))
    cs.acqStep = float(need("acqStep"))
    cs.acqThreshold = float(need("acqThreshold"))
    cs.resamplingThreshold = float(need("resamplingThreshold"))
    cs.resamplingflag = int(need("resamplingflag"))
    if sig == "B1C":  # B1C/initSettings.m:60,70,102
        cs.acqCohT = float(need("acqCohT"))
        cs.pilotACQflag = int(need("pilotACQflag"))
        cs.FEBW = float(need("FEBW"))
        cs.fineNoncoh = 1
    else:  # B2a/initSettings.m:84
        cs.fineNoncoh = int(need("fineNoncoh"))
        cs.acqCohT = 10.0
        cs.pilotACQflag = 1
        cs.FEBW = 0.0
    sats = [int(p) for p in np.atleast_1d(need("acqSatelliteList"))]
    if len(sats) > BDS_MAX_PRN:
        raise ValueError("settings.acqSatelliteList longer than 63")
    cs.n_acq = len(sats)
    for i, p in enumerate(sats):
        cs.acqSatelliteList[i] = p
    cs.pilotTRKflag = int(need("pilotTRKflag"))
    cs.intTime = float(need("intTime"))
    cs.dllCorrelatorSpacing = float(need("dllCorrelatorSpacing"))
    cs.dllDampingRatio = float(need("dllDampingRatio"))
    cs.dllNoiseBandwidth = float(need("dllNoiseBandwidth"))
    cs.pllNoiseBandwidth = float(need("pllNoiseBandwidth"))
    cs.CNoInterval = int(need("CNoInterval"))
    return cs


DATA_TYPES = {"schar": 0, "int8": 0, "int16": 1, "short": 1}  # settings.dataType -> bds_settings.dataType
DATA_TYPE_REFUSED = 2  # what every other fread type maps to


def data_type_code(name) -> int:
    """bds_settings.dataType of a settings.dataType string."""
    return DATA_TYPES.get(str(name), DATA_TYPE_REFUSED)


def record_is_int16(settings, dtype_name, what="the record") -> bool:
    """The routing rule of every array that carries samples or raw record bytes: an int16 array goes with settings.dataType
    'int16' / 'short', an int8 array (uint8: raw bytes of a packed record) with 'schar' / 'int8'.  A disagreement raises BdsError
    naming dataType, before any copy or native call; arrays of other dtypes carry VALUES and are converted by the caller.
    Returns True when the settings say 16 bits.  dtype_name: NumPy's name of the array's dtype."""
    name = str(getattr(settings, "dataType", "schar"))
    code = data_type_code(name)
    if dtype_name == "int16" and code != 1:
        raise BdsError(-1, f"settings.dataType is {name!r} but {what} is an int16 array: int16 samples go with dataType 'int16'")
    if dtype_name in ("int8", "uint8") and code == 1:
        raise BdsError(-1, f"settings.dataType is {name!r} but {what} is an {dtype_name} array: a 16-bit record is passed as an int16 array "
                           "(little-endian samples; I, Q pairs for fileType 2)")
    return code == 1


def _i16(a, what="the record"):
    """Values as a contiguous little-endian int16 row (an int16 array as it is: no copy when contiguous)."""
    a = np.asarray(a)
    if a.dtype != np.dtype("<i2"):
        if a.dtype.kind not in "iuf":
            raise ValueError(f"{what} must hold int16 values, not {a.dtype}")
        r = np.rint(a)
        if not np.array_equal(r, a) or (r.size and (r.min() < -32768 or r.max() > 32767)):
            raise ValueError(f"{what} must hold int16 values (fread(..., 'int16'))")
        a = r.astype("<i2")
    return np.ascontiguousarray(a).reshape(-1)


def record_bytes(settings, data, what="the record"):
    """(int8 view of the record's raw bytes, 16-bit?) of a host array under the routing rule (record_is_int16)."""
    a = np.asarray(data)
    if record_is_int16(settings, a.dtype.name, what):
        return _i16(a, what).view(np.int8), True
    return _i8(a)[0].reshape(-1), False


def device_dtype_name(x) -> str:
    """NumPy's dtype name of a device array (a torch tensor, or an object with __cuda_array_interface__)."""
    if hasattr(x, "__cuda_array_interface__") and not (type(x).__module__.split(".")[0] == "torch"):
        return np.dtype(x.__cuda_array_interface__["typestr"]).name
    return str(x.dtype).split(".")[-1]


def device_record(settings, x, ctx_device, what="the record"):
    """device_span of a device array that carries a record or a block, under the routing rule: int16 with settings.dataType
    'int16', int8 / uint8 otherwise.  Returns (pointer, n_bytes, keepalive, 16-bit?)."""
    w16 = record_is_int16(settings, device_dtype_name(x), what)
    ptr, n_bytes, keep = device_span(x, ctx_device, dtypes=("int16",) if w16 else ("int8", "uint8"))
    return ptr, n_bytes, keep, w16


def _i8(a):
    a = np.asarray(a)
    if a.dtype == np.uint8:  # raw bytes (a packed fileType-3 record): the same bytes, not a conversion of values above 127
        a = np.ascontiguousarray(a).view(np.int8)
    a = np.ascontiguousarray(a, dtype=np.int8)
    return a, a.ctypes.data_as(C.POINTER(C.c_int8))


def is_device_array(x) -> bool:
    """True for what the *_dev entries take: a torch tensor on a GPU, or any object with __cuda_array_interface__.  Everything
    else -- NumPy arrays, CPU tensors, paths -- takes the host entries."""
    if type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr"):
        return bool(getattr(x, "is_cuda", False))
    return hasattr(x, "__cuda_array_interface__")


def _device_index(dev):
    """Device ordinal of a .device attribute (torch.device, an object with .id or .index, an int), or None when it tells none."""
    if dev is None or isinstance(dev, str):
        return None
    if isinstance(dev, (int, np.integer)):
        return int(dev)
    for name in ("index", "id"):
        v = getattr(dev, name, None)
        if isinstance(v, (int, np.integer)):
            return int(v)
    return None


def device_span(x, ctx_device, dtypes=("int8", "uint8")):
    """(pointer, n_bytes, keepalive) of a device array for the *_dev entries: a torch tensor on a GPU or an object with
    __cuda_array_interface__, contiguous, of one of `dtypes` (NumPy names), on the context's device `ctx_device`.  Anything
    else raises TypeError / ValueError before any native call.  The ordering rule of include/bds_mi355x.h is kept in here:
    torch's current stream on that device is synchronised before the span is returned, so that every write to the array
    enqueued there has completed when the library reads it on its own streams."""
    ctx_device = int(ctx_device)
    if type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr"):
        if not x.is_cuda:
            raise TypeError("a torch tensor in host memory is not a device array: pass it as a NumPy array (tensor.numpy()), or move it to the GPU")
        dev, dtype = x.device.index, str(x.dtype).split(".")[-1]
        contiguous = bool(x.is_contiguous())
        ptr, n_bytes = int(x.data_ptr()) if x.numel() else 0, int(x.numel()) * int(x.element_size())
    elif hasattr(x, "__cuda_array_interface__"):
        cai = x.__cuda_array_interface__
        dev, dtype = _device_index(getattr(x, "device", None)), np.dtype(cai["typestr"]).name
        shape, item = tuple(int(v) for v in cai["shape"]), np.dtype(cai["typestr"]).itemsize
        strides, want = cai.get("strides"), item
        contiguous = True
        if strides is not None:  # C order: the last axis steps by one element, every other by the extent of those behind it
            for n, st in zip(reversed(shape), reversed(tuple(strides))):
                contiguous &= n <= 1 or int(st) == want
                want *= n
        n_bytes = int(np.prod(shape, dtype=np.int64)) * item if shape else item
        ptr = int(cai["data"][0] or 0) if n_bytes else 0
    else:
        raise TypeError(f"{type(x).__name__} is not a device array (a torch tensor on a GPU, or an object with __cuda_array_interface__)")
    if dtype not in dtypes:
        raise TypeError(f"a device array of dtype {dtype}: the record takes {' / '.join(dtypes)}")
    if not contiguous:
        raise ValueError("the device array is not contiguous: the record is read as one run of bytes (.contiguous() makes a copy that is)")
    if dev is not None and dev != ctx_device:
        raise ValueError(f"the array is on device {dev}, the context runs on device {ctx_device}")
    _sync_current_stream(ctx_device)
    return ptr, n_bytes, x


def _sync_current_stream(device):
    """Wait for torch's current stream on `device` (nothing to wait for when torch is absent or has opened no GPU)."""
    try:
        import torch
    except Exception:
        return
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.current_stream(device).synchronize()


def check_feed_span(sess, n_bytes) -> None:
    """check_feed_bytes for bytes in device memory: the same argument errors, before any native call."""
    if not sess.get("feed"):
        raise ValueError("feed on a session that reads its record itself (it was opened on a file or an array, not with origin=)")
    if sess["fileType"] == 2 and n_bytes % 2 and not sess.get("w16"):
        raise ValueError(f"an I/Q record is fed in whole int8 pairs: {n_bytes} bytes is an odd count")


def synth_out_torch(fmt, n_samples, device):
    """synth_out as a torch tensor on GPU `device` (the generator's out="torch")."""
    import torch

    host = synth_out(fmt, 0)  # (the format check, and the dtype)
    n = synth_out_count(fmt, n_samples)
    return torch.empty(n, dtype=getattr(torch, host.dtype.name), device=f"cuda:{int(device)}")


def sample_format(is_complex) -> int:
    """is_complex of the C ABI: 0 real int8, 1 (True) interleaved I/Q int8 pairs, 2 packed 2+2-bit I/Q bytes (fileType 3)."""
    f = int(is_complex)
    if f not in (0, 1, 2):
        raise ValueError(f"is_complex must be 0 (real), 1 (I/Q int8 pairs) or 2 (packed 2+2-bit I/Q), not {is_complex!r}")
    return f


def n_samples_of(n_values: int, is_complex, n_samples=None) -> int:
    """Samples in an array of n_values int8 values (bytes, when packed) of the given format; n_samples, if given, is checked
    against what the array holds (a packed array of B bytes holds 2 B samples: an odd count ignores the last high nibble)."""
    f = sample_format(is_complex)
    if f == 1 and n_values % 2:
        raise ValueError(f"an I/Q record holds int8 pairs: {n_values} values is an odd count (packed bytes go with is_complex = 2)")
    have = n_values * 2 if f == 2 else n_values // 2 if f == 1 else n_values
    if n_samples is None:
        return have
    if not 0 <= int(n_samples) <= have:
        raise ValueError(f"n_samples = {n_samples} but the array holds {have} samples")
    return int(n_samples)


def check_feed_origin(origin) -> int:
    """origin_sample of a feed session: a non-negative multiple of 32 samples (checked before any native call)."""
    if int(origin) != origin or int(origin) < 0 or int(origin) % 32:
        raise ValueError(f"origin = {origin!r}: the first sample fed must be a non-negative multiple of 32 samples")
    return int(origin)


def check_feed_bytes(sess, data) -> np.ndarray:
    """The bytes of one track_feed call as a contiguous int8 array; argument errors raise before any native call."""
    if not sess.get("feed"):
        raise ValueError("feed on a session that reads its record itself (it was opened on a file or an array, not with origin=)")
    a = np.asarray(data)
    if sess.get("w16"):  # a 16-bit record: int16 samples, or raw bytes (uint8) in pieces of any size -- a call takes whole samples
        if a.dtype == np.uint8:
            return np.ascontiguousarray(a).reshape(-1).view(np.int8)
        if a.dtype == np.int8:
            raise BdsError(-1, "settings.dataType is 'int16' but the bytes fed are an int8 array: feed int16 samples, or raw bytes as uint8")
        return _i16(a, "the samples fed").view(np.int8)
    if a.dtype == np.int16:
        raise BdsError(-1, "settings.dataType is 'schar' but the samples fed are an int16 array: int16 samples go with dataType 'int16'")
    if a.dtype == np.uint8:
        a = a.view(np.int8)
    a = np.ascontiguousarray(a, dtype=np.int8).reshape(-1)
    if sess["fileType"] == 2 and a.size % 2:
        raise ValueError(f"an I/Q record is fed in whole int8 pairs: {a.size} bytes is an odd count")
    return a


def pack_synth(sats, fmt, seed=3550, sigma=20.0, iq_sign=0, threshold=None, code_doppler=True, pilot61_secondary=False,
               symbols=None):
    """(bds_synth_sat array, bds_synth_opts, what must stay alive) of one bds_synth / bds_synth_file call.  sats: objects with prn,
    doppler, delay, phase, cn0_dbhz (synth.Sat); symbols: None or int8-valued [n_sat, 2, n_sym] of +-1."""
    arr = (SynthSat * max(len(sats), 1))()
    for i, t in enumerate(sats):
        arr[i].prn, arr[i].doppler, arr[i].delay = int(t.prn), float(t.doppler), float(t.delay)
        arr[i].phase, arr[i].cn0_dbhz = float(t.phase), float(t.cn0_dbhz)
    o = SynthOpts()
    o.size, o.format, o.iq_sign = C.sizeof(SynthOpts), int(fmt), int(iq_sign)
    o.code_doppler, o.pilot61_secondary = int(bool(code_doppler)), int(bool(pilot61_secondary))
    o.seed, o.sigma, o.threshold = int(seed) & (2 ** 64 - 1), float(sigma), 0.0 if threshold is None else float(threshold)
    sym = None
    if symbols is not None:
        sym = np.ascontiguousarray(symbols, dtype=np.int8)
        if sym.ndim != 3 or sym.shape[:2] != (len(sats), 2) or sym.shape[2] < 1:
            raise ValueError(f"symbols must have shape [n_sat = {len(sats)}, 2, n_sym >= 1], not {sym.shape}")
        o.symbols, o.n_sym = sym.ctypes.data_as(C.POINTER(C.c_int8)), sym.shape[2]
    return arr, o, sym


def pack_traj(segs, first, seg_log2, n_sat):
    """(bds_synth_traj, the array it points into) from a structured array [n_sat, n_seg] of SYNTH_SEG_DTYPE."""
    a = np.ascontiguousarray(segs, dtype=SYNTH_SEG_DTYPE)
    if a.ndim != 2 or a.shape[0] != n_sat or a.shape[1] < 1:
        raise ValueError(f"the trajectory's segments must have shape [n_sat = {n_sat}, n_seg >= 1], not {a.shape}")
    t = SynthTraj()
    t.size, t.seg_log2, t.first, t.n_seg = C.sizeof(SynthTraj), int(seg_log2), int(first), a.shape[1]
    t.seg = a.ctypes.data_as(C.POINTER(SynthSeg))
    return t, a


def synth_trajectory(settings, ephs, rx, tow, t0, first, n_seg, seg_log2) -> np.ndarray:
    """bds_synth_trajectory (host only, no GPU): the segments [len(ephs), n_seg] (SYNTH_SEG_DTYPE) of the record whose sample n is
    taken at system time tow + t0 + n / fs by a receiver at rx [m, Earth-fixed]; ephs: eph dicts (eph_dict's layout)."""
    cs = pack_settings(settings)
    arr = eph_array(ephs)
    r = np.ascontiguousarray(rx, dtype=np.float64).reshape(-1)
    if r.size != 3:
        raise ValueError("rx must hold three coordinates")
    n_seg = int(n_seg)
    out = np.zeros((len(ephs), max(n_seg, 1)), dtype=SYNTH_SEG_DTYPE)
    rc = lib().bds_synth_trajectory(C.byref(cs), len(ephs), arr, r.ctypes.data_as(_DP), float(tow), float(t0), int(first), n_seg, int(seg_log2),
                                    out.ctypes.data_as(C.POINTER(SynthSeg)))
    if rc < 0:
        raise BdsError(rc, lib().bds_last_error(None).decode())
    return out


def blank_sample_bytes(settings) -> int:
    """Bytes per sample of a record the blanker takes (fileType 1 / 2, 8 or 16 bits); fileType 3 is the library's to refuse."""
    return (2 if int(settings.fileType) == 2 else 1) * (2 if data_type_code(getattr(settings, "dataType", "schar")) == 1 else 1)


def pack_blank(threshold_sq, pre, post, lead=0, tail=0, duty_samples=0):
    """(bds_blank_opts, bds_blank_out without a duty array, None) of one bds_blank* call."""
    o, rep = BlankOpts(), BlankOut()
    ts = int(threshold_sq)
    if not 0 <= ts <= 2 ** 32 - 1:
        raise ValueError(f"threshold_sq = {threshold_sq!r} is outside 0 .. 2^32 - 1")
    o.threshold_sq, o.pre, o.post, o.lead, o.tail, o.duty_samples = ts, int(pre), int(post), int(lead), int(tail), int(duty_samples)
    return o, rep, None


def blank_duty(rep, n, lead, tail, duty_samples):
    """The duty array of a window of n - lead - tail samples, hung into `rep` (None when no bins are asked for)."""
    ds = int(duty_samples)
    if ds <= 0:
        return None
    duty = np.zeros(max(-(-max(int(n) - int(lead) - int(tail), 0) // ds), 1), dtype=np.int32)
    rep.duty, rep.duty_cap = duty.ctypes.data_as(_IP), duty.size
    return duty


def pack_notch(steps, block_log2, first_sample=0, apply=True):
    """(bds_notch_opts, bds_notch_out without an est array) of one bds_notch* call; steps: uint32 phase steps per sample."""
    o, rep = NotchOpts(), NotchOut()
    steps = [int(v) for v in steps]
    if any(not 0 <= v <= 2 ** 32 - 1 for v in steps):
        raise ValueError(f"steps = {steps!r}: each is a uint32 phase step")
    o.n_tones, o.block_log2, o.first_sample, o.apply = len(steps), int(block_log2), int(first_sample), 1 if apply else 0
    for k, v in enumerate(steps[:NOTCH_MAX_TONES]):
        o.step[k] = v
    return o, rep


def notch_est(rep, n, block_log2, n_tones, want=True):
    """The int32 [n_blocks, n_tones, 2] estimates of a window of n samples, hung into `rep` (want=False: None, nothing hung)."""
    if not want:
        return None
    nb = -(-max(int(n), 0) // (1 << int(block_log2))) if 0 <= int(block_log2) < 32 else 0
    est = np.zeros((nb, max(int(n_tones), 0), 2), dtype=np.int32)
    if est.size:
        rep.est, rep.est_cap = est.ctypes.data_as(_IP), nb * int(n_tones)
    return est


def conditioner_out(source, out, file_message):
    """What blank_pulses / notch_tones hand Context.blank / .notch as `out`: the path for a path (file_message is raised when
    none is given), else `source` itself for "inplace", a new tensor for a tensor without one, and `out` as it is otherwise."""
    if isinstance(source, (str, bytes, os.PathLike)):
        if out is None or (isinstance(out, str) and out == "inplace"):
            raise ValueError(file_message)
        return out
    on_device = is_device_array(source)
    if isinstance(out, str) and out != "inplace":
        raise ValueError(f'out = {out!r}: None, "inplace" or {"a tensor" if on_device else "an array"}')
    if on_device and out is None:
        import torch

        return torch.empty_like(source)
    if isinstance(out, str) and not on_device:
        if not isinstance(source, np.ndarray) or not source.flags.c_contiguous or not source.flags.writeable:
            raise ValueError('out="inplace" takes a contiguous writeable NumPy array')
    return source if isinstance(out, str) else out


def conditioner_io(settings, source, out, writes, ctx_device, verb):
    """The record of one bds_blank* / bds_notch* call and where its output goes, for the three places a record can lie in:
    (kind, in, out, n_bytes, result, keepalive) with kind "file" (in / out: encoded paths, n_bytes None), "dev" or "host"
    (in / out: pointers).  out and result are None for a call that writes nothing; `verb` words the file refusal."""
    if isinstance(source, (str, bytes, os.PathLike)):
        if writes and not isinstance(out, (str, bytes, os.PathLike)):
            raise ValueError(f"{verb} a file writes a file: out must be a path")
        return "file", os.fsencode(source), os.fsencode(out) if writes else None, None, out if writes else None, ()
    if is_device_array(source):
        ptr, n_bytes, keep, _ = device_record(settings, source, ctx_device)
        if not writes:
            return "dev", ptr, None, n_bytes, None, (keep,)
        res = source if out is None else out
        optr, on_bytes, okeep, _ = device_record(settings, res, ctx_device, "the output record")
        if on_bytes != n_bytes:
            raise ValueError(f"the output record holds {on_bytes} bytes, the input {n_bytes}")
        return "dev", ptr, optr, n_bytes, res, (keep, okeep)
    a, w16 = record_bytes(settings, source)
    if not writes:
        return "host", a.ctypes.data_as(C.c_void_p), None, a.size, None, (a,)
    if out is None:
        res = np.empty(a.size // 2, dtype="<i2") if w16 else np.empty(a.size, dtype=np.asarray(source).dtype if np.asarray(source).dtype == np.uint8 else np.int8)
    else:
        res = out
        if not isinstance(res, np.ndarray) or not res.flags.c_contiguous or res.nbytes != a.size:
            raise ValueError(f"out must be a contiguous NumPy array of the record's {a.size} bytes")
    return "host", a.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p), a.size, res, (a, res)


def notch_lo() -> np.ndarray:
    """bds_notch_lo (no GPU): the excisor's local-oscillator table, int16 [2, 2^14]: cosines, then sines."""
    t = np.zeros((2, 1 << NOTCH_PHASE_BITS), dtype=np.int16)
    rc = lib().bds_notch_lo(t.ctypes.data_as(C.POINTER(C.c_int16)))
    if rc < 0:
        raise BdsError(rc, lib().bds_last_error(None).decode())
    return t


def synth_out(fmt, n_samples) -> np.ndarray:
    """The array n_samples samples of a format take (0: float64, 1: int8, 2: int8 pairs, 3: packed uint8, two samples a byte)."""
    if fmt not in SYNTH_FORMATS:
        raise ValueError(f"format must be 0 (float64 clean sum), 1 (int8), 2 (I/Q int8 pairs) or 3 (packed 2+2-bit I/Q), not {fmt!r}")
    return np.empty(synth_out_count(fmt, n_samples), dtype=SYNTH_FORMATS[fmt][0])


def synth_out_count(fmt, n_samples) -> int:
    """Elements of synth_out(fmt, n_samples)."""
    if fmt not in SYNTH_FORMATS:
        raise ValueError(f"format must be 0 (float64 clean sum), 1 (int8), 2 (I/Q int8 pairs) or 3 (packed 2+2-bit I/Q), not {fmt!r}")
    dtype, num, den = SYNTH_FORMATS[fmt]
    if int(n_samples) < 0 or int(n_samples) % den:
        raise ValueError(f"n_samples = {n_samples}: a packed record holds two samples per byte" if den > 1 else f"n_samples = {n_samples}")
    return int(n_samples) * num // den


def gen_code(signal: str, kind: str, prn: int) -> np.ndarray:
    """bds_gen_code -> int8 array of +-1 (host side; works without a GPU)."""
    k = CODE_KIND[kind]
    out = np.empty(CODE_LEN[k], dtype=np.int8)
    rc = lib().bds_gen_code(SIGNAL[signal.upper()], k, int(prn), out.ctypes.data_as(C.POINTER(C.c_int8)), out.size)
    if rc < 0:
        raise BdsError(rc, f"bds_gen_code({signal}, {kind}, {prn})")
    return out


def eph_dict(e: Eph) -> dict:
    """One bds_eph as a dict: flag, SatType (0..3), n_entered, idValid (int array) and a float per name of EPH_FIELDS (NaN = [])."""
    d = {"flag": int(e.flag), "SatType": int(e.SatType), "n_entered": int(e.n_entered), "idValid": np.array(e.idValid, dtype=np.int32)}
    d.update((f, float(getattr(e, f))) for f in EPH_FIELDS)
    return d


def eph_array(ephs):
    """bds_eph[len(ephs)] from eph dicts (eph_dict's layout; a missing name is NaN, a missing counter 0) or None (nothing decoded)."""
    arr = (Eph * max(1, len(ephs)))()
    for e, d in zip(arr, ephs):
        e.size = C.sizeof(Eph)
        d = d or {}
        e.flag, e.SatType, e.n_entered = int(d.get("flag", 0)), int(d.get("SatType", 0)), int(d.get("n_entered", 0))
        for k, v in enumerate(np.asarray(d.get("idValid", np.zeros(8)), dtype=np.int64)[:8]):
            e.idValid[k] = int(v)
        for f in EPH_FIELDS:
            setattr(e, f, float(d.get(f, math.nan)))
    return arr


def pack_pvt_params(s) -> PvtParams:
    """The settings postNavigation reads besides bds_settings -> bds_pvt_params; a missing one is an error naming it."""
    p = PvtParams()
    p.size = C.sizeof(PvtParams)
    for name in PVT_SETTINGS:
        if not hasattr(s, name):
            raise AttributeError(f"settings.{name} is missing")
        setattr(p, name, int(getattr(s, name)) if name == "useTropCorr" else float(getattr(s, name)))
    return p


def _status_bytes(status, n_ch):
    st = "".join(str(x)[:1] or "-" for x in status) if not isinstance(status, (str, bytes)) else status
    st = st.encode() if isinstance(st, str) else bytes(st)
    if len(st) != n_ch:
        raise ValueError(f"pvt: {n_ch} channels, {len(st)} status characters")
    return st


def _series(a, shape, what):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"pvt: {what} is {a.shape}, not {shape}")
    return a


def _pvt_out(n_ch, cap):
    """(bds_pvt_out over fresh arrays, the arrays by name)."""
    arrays = {f: np.zeros((n_ch, cap)) for f in PVT_CHANNEL_FIELDS}
    arrays["DOP"] = np.zeros((5, cap))
    arrays.update((f, np.zeros(cap)) for f in PVT_EPOCH_FIELDS)
    o = PvtOut()
    o.size, o.cap = C.sizeof(PvtOut), cap
    for f, a in arrays.items():
        setattr(o, f, a.ctypes.data_as(_DP))
    return o, arrays


def pvt_plan(settings, status, absolute_sample, ephs, sub_frame_start, tow) -> dict:
    """bds_pvt_plan (no GPU): status characters [n_ch], absoluteSample [n_ch, n], eph dicts, subFrameStart and TOW [n_ch] ->
    {"ready" (BDS_PVT_* flags per channel), "sampleStart", "sampleEnd", "measSampleStep", "n_meas"}."""
    cs, pp = pack_settings(settings), pack_pvt_params(settings)
    a = np.ascontiguousarray(absolute_sample, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("pvt_plan: absoluteSample is [n_ch, n]")
    n_ch, n = a.shape
    sfs, tw = _series(sub_frame_start, (n_ch,), "subFrameStart"), _series(tow, (n_ch,), "TOW")
    if len(ephs) != n_ch:
        raise ValueError(f"pvt_plan: {n_ch} channels, {len(ephs)} ephemerides")
    ready = np.zeros(n_ch, dtype=np.int32)
    v = np.zeros(3)
    rc = lib().bds_pvt_plan(C.byref(cs), C.byref(pp), n_ch, n, _status_bytes(status, n_ch), a.ctypes.data_as(_DP), eph_array(ephs),
                            sfs.ctypes.data_as(_DP), tw.ctypes.data_as(_DP), ready.ctypes.data_as(_IP),
                            v[0:].ctypes.data_as(_DP), v[1:].ctypes.data_as(_DP), v[2:].ctypes.data_as(_DP))
    if rc < 0:
        raise BdsError(rc, "bds_pvt_plan: an argument, the settings, or absoluteSample not strictly increasing on a ready channel")
    return {"ready": ready, "sampleStart": float(v[0]), "sampleEnd": float(v[1]), "measSampleStep": float(v[2]), "n_meas": rc}


def pvt_solve(settings, prns, ready, sample_start, meas_sample_step, transmit_time, sat_pos, sat_clk_corr) -> dict:
    """bds_pvt_solve (no GPU): the measure stage's arrays ([n_meas, n_ch], [n_meas, n_ch, 3], [n_meas, n_ch]) -> the arrays of
    navSolutions by name ([n_ch, n_meas], DOP [5, n_meas], [n_meas])."""
    cs, pp = pack_settings(settings), pack_pvt_params(settings)
    tt = np.ascontiguousarray(transmit_time, dtype=np.float64)
    if tt.ndim != 2:
        raise ValueError("pvt_solve: transmitTime is [n_meas, n_ch]")
    n_meas, n_ch = tt.shape
    sp, ck = _series(sat_pos, (n_meas, n_ch, 3), "satPos"), _series(sat_clk_corr, (n_meas, n_ch), "satClkCorr")
    prn, rd = np.ascontiguousarray(prns, dtype=np.int32), np.ascontiguousarray(ready, dtype=np.int32)
    if prn.shape != (n_ch,) or rd.shape != (n_ch,):
        raise ValueError(f"pvt_solve: {n_ch} channels, {prn.size} PRNs, {rd.size} ready flags")
    o, arrays = _pvt_out(n_ch, n_meas)
    rc = lib().bds_pvt_solve(C.byref(cs), C.byref(pp), n_ch, n_meas, prn.ctypes.data_as(_IP), rd.ctypes.data_as(_IP), float(sample_start),
                             float(meas_sample_step), tt.ctypes.data_as(_DP), sp.ctypes.data_as(_DP), ck.ctypes.data_as(_DP), C.byref(o))
    if rc < 0:
        raise BdsError(rc, "bds_pvt_solve")
    return arrays


def nav_frame_dict(f: NavFrame, signal) -> dict:
    """One bds_nav_frame as a dict; `bits` unpacked to uint8 0 / 1 (878 for B1C, 288 for B2a)."""
    sig = signal if isinstance(signal, int) else SIGNAL[str(signal).upper()]
    bits = np.unpackbits(np.frombuffer(bytes(f.bits), dtype=np.uint8))[:NAV_BITS[sig]]
    return {"index": int(f.index), "status": int(f.status), "polarity": int(f.polarity), "bch1_max": int(f.bch1_max),
            "bch2_max": int(f.bch2_max), "bits": bits}


def nav_fields(signal, messages) -> tuple:
    """bds_nav_fields (no GPU): decoded messages, uint8 0 / 1 of shape [n_msg, 878] (B1C) or [n_msg, 288] (B2a), through the
    field parser and the merging rules in order -> (eph dict, number of messages that entered)."""
    sig = SIGNAL[str(signal).upper()]
    m = np.atleast_2d(np.asarray(messages, dtype=np.uint8))
    if m.shape[1] != NAV_BITS[sig]:
        raise ValueError(f"nav_fields: {NAV_BITS[sig]} bits per message, got {m.shape[1]}")
    packed = np.ascontiguousarray(np.packbits(m, axis=1))
    e = Eph()
    e.size = C.sizeof(Eph)
    rc = lib().bds_nav_fields(sig, packed.ctypes.data_as(C.POINTER(C.c_uint8)), m.shape[0], packed.shape[1], C.byref(e))
    if rc < 0:
        raise BdsError(rc, "bds_nav_fields")
    return eph_dict(e), rc


def sync_pattern(signal: str, prn: int = 1) -> np.ndarray:
    """+-1 frame-sync pattern: B1C pilot secondary code of the PRN (1800) or the B2a preamble x NH (120)."""
    out = np.empty(1800, dtype=np.int8)
    rc = lib().bds_sync_pattern(SIGNAL[signal.upper()], int(prn), out.ctypes.data_as(C.POINTER(C.c_int8)), out.size)
    if rc < 0:
        raise BdsError(rc, f"bds_sync_pattern({signal}, {prn})")
    return out[:rc].copy()


def shard_jobs(costs, world: int) -> np.ndarray:
    """bds_shard_jobs: rank of every job (longest-processing-time rule); host side, works without a GPU."""
    c = np.ascontiguousarray(costs, dtype=np.float64)
    out = np.zeros(c.size, dtype=np.int32)
    rc = lib().bds_shard_jobs(int(c.size), c.ctypes.data_as(_DP), int(world), out.ctypes.data_as(_IP))
    if rc < 0:
        raise BdsError(rc, "bds_shard_jobs")
    return out


def acq_job_cost(settings) -> float:
    """bds_acq_job_cost: relative cost of searching one PRN with these settings."""
    cs = pack_settings(settings)
    return float(lib().bds_acq_job_cost(C.byref(cs)))


class MultiContext:
    """bds_multi: one host process driving several GPUs (device_ids None = every visible device)."""

    def __init__(self, device_ids=None):
        self._lib = lib()
        if device_ids is None:
            self._h = self._lib.bds_multi_create(0, None)
        else:
            ids = np.ascontiguousarray(device_ids, dtype=np.int32)
            self._h = self._lib.bds_multi_create(int(ids.size), ids.ctypes.data_as(_IP))
        if not self._h:
            raise BdsError(-2, self._lib.bds_multi_last_error(None).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bds_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self) -> int:
        return int(self._lib.bds_multi_size(self._h))

    def rccl_ranks(self) -> int:
        return int(self._lib.bds_multi_rccl_ranks(self._h))

    def acquire(self, jobs):
        """jobs: list of (settings, int8 samples, is_complex) -- one entry per signal (is_complex 2: uint8 packed bytes).
        Returns a list of (carrFreq, codePhase, peakMetric, detected), one per signal."""
        n = len(jobs)
        arr = (AcqJob * n)()
        keep, outs = [], []
        for i, (settings, samples, is_complex) in enumerate(jobs):
            cs = pack_settings(settings)
            record_is_int16(settings, np.asarray(samples).dtype.name, f"the block of signal {i}")  # (16-bit settings: refused by the library)
            a, p = _i8(samples)
            max_prn = max(int(q) for q in np.atleast_1d(settings.acqSatelliteList))
            carr, cph, pm = np.zeros(max_prn), np.zeros(max_prn), np.zeros(max_prn)
            det = np.zeros(max_prn, dtype=np.int32)
            arr[i].settings = C.pointer(cs)
            arr[i].samples = p
            arr[i].n_samples = n_samples_of(a.size, is_complex)
            arr[i].is_complex = sample_format(is_complex)
            arr[i].max_prn = max_prn
            arr[i].carrFreq, arr[i].codePhase, arr[i].peakMetric = (v.ctypes.data_as(_DP) for v in (carr, cph, pm))
            arr[i].detected = det.ctypes.data_as(_IP)
            keep.append((cs, a))
            outs.append((carr, cph, pm, det))
        rc = self._lib.bds_acquire_multi(self._h, n, arr)
        if rc < 0:
            raise BdsError(rc, self._lib.bds_multi_last_error(self._h).decode())
        return outs


def gen_primary_code(signal: str, kind: str, prn: int) -> np.ndarray:
    return gen_code(signal, kind, prn)


class Context:
    """One bds_ctx (one GPU)."""

    def __init__(self, device: int = 0):
        self._lib = lib()
        self.device = int(device)
        self._h = self._lib.bds_create(int(device))
        if not self._h:
            raise BdsError(-2, self._lib.bds_last_error(None).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bds_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc < 0:
            raise BdsError(rc, self._lib.bds_last_error(self._h).decode())
        return rc

    def reload_tuning(self):
        """Re-read the BDS_* environment knobs into this context (they are read once at creation)."""
        self._check(self._lib.bds_reload_tuning(self._h))

    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        self._check(self._lib.bds_device_name(self._h, buf, 256))
        return buf.value.decode()

    # -- acquisition -----------------------------------------------------------------
    def acq_load(self, settings, samples, is_complex=False, n_samples=None):
        """is_complex: 0 / False real int8, 1 / True I/Q int8 pairs, 2 packed 2+2-bit I/Q bytes (uint8, fileType 3).
        n_samples: use only the first n_samples of the array (default: all it holds).
        A device array (is_device_array: a torch tensor on the GPU, int8 / uint8) goes through bds_acq_load_dev, with the same
        checks and the same results."""
        if is_device_array(samples):
            return self.acq_load_dev(settings, samples, is_complex, n_samples)
        cs = pack_settings(settings)
        if record_is_int16(settings, np.asarray(samples).dtype.name, "the block"):  # int16 values: bds_acq_load16
            a = _i16(samples, "the block")
            n = n_samples_of(a.size, is_complex, n_samples)
            self._check(self._lib.bds_acq_load16(self._h, C.byref(cs), a.ctypes.data_as(C.POINTER(C.c_int16)), n, sample_format(is_complex)))
            return
        a, p = _i8(samples)
        n = n_samples_of(a.size, is_complex, n_samples)
        self._check(self._lib.bds_acq_load(self._h, C.byref(cs), p, n, sample_format(is_complex)))

    def acq_load_dev(self, settings, samples, is_complex=False, n_samples=None):
        """bds_acq_load_dev: acq_load of a block in device memory (int8, uint8 for packed bytes; int16 with settings.dataType 'int16')."""
        cs = pack_settings(settings)
        ptr, n_bytes, keep, w16 = device_record(settings, samples, self.device, "the block")
        n = n_samples_of(n_bytes // 2 if w16 else n_bytes, is_complex, n_samples)
        self._check(self._lib.bds_acq_load_dev(self._h, C.byref(cs), ptr, n, sample_format(is_complex)))

    def acq_block(self, cap):
        """Test aid (bds_acq_block): the float64 block the search reads after the last acq_load -- the resampling branch's output or a
        widened 16-bit block -- copied as the library holds it.  cap: samples the buffers hold (BdsError when the block is longer, is an
        int8 one, or nothing is loaded).  Returns a float64 array for a real block, a complex128 one for an I/Q block."""
        re, im = np.full(int(cap), np.nan), np.full(int(cap), np.nan)
        n = C.c_longlong(-1)
        cplx = self._check(self._lib.bds_acq_block(self._h, re.ctypes.data_as(_DP), im.ctypes.data_as(_DP), int(cap), C.byref(n)))
        return re[:n.value] + 1j * im[:n.value] if cplx else re[:n.value]

    def acq_prepare(self, settings):
        cs = pack_settings(settings)
        self._check(self._lib.bds_acq_prepare(self._h, C.byref(cs)))

    def acq_set_pair_budget(self, gib):
        """bds_acq_set_pair_budget_gb: serving mode of the search -- several PRNs' Doppler rows per launch pair, inter-pass buffer of
        `gib` GiB ("auto" / negative: 60 % of the free device memory; 0: the minimal footprint, one PRN per pair; the library default is 40).  Takes effect at the next acq_run, in both directions (a larger buffer is given back)."""
        g = -1.0 if (isinstance(gib, str) and gib.lower().startswith("a")) else float(gib)
        self._lib.bds_acq_set_pair_budget_gb.argtypes = [C.c_void_p, C.c_double]
        self._check(self._lib.bds_acq_set_pair_budget_gb(self._h, g))

    def acq_set_b2a_npoint(self, on):
        """bds_acq_set_b2a_npoint: opt-in N-point search (N = 198 750 = 53 x 6 x 625) for B2a at 99.375 MS/s; include/bds_mi355x.h lists when
        it applies -- everything else runs as with the switch off.  Takes effect at the next acq_prepare / acq_run."""
        self._lib.bds_acq_set_b2a_npoint.restype, self._lib.bds_acq_set_b2a_npoint.argtypes = C.c_int32, [C.c_void_p, C.c_int32]
        self._check(self._lib.bds_acq_set_b2a_npoint(self._h, 1 if on else 0))

    def acq_set_b1c_npoint(self, on):
        """bds_acq_set_b1c_npoint: opt-in N-point search (N = 613 800 = 31 x 11 x 1800) for B1C at 30.69 MS/s; include/bds_mi355x.h lists when
        it applies -- everything else runs as with the switch off.  Takes effect at the next acq_prepare / acq_run."""
        self._lib.bds_acq_set_b1c_npoint.restype, self._lib.bds_acq_set_b1c_npoint.argtypes = C.c_int32, [C.c_void_p, C.c_int32]
        self._check(self._lib.bds_acq_set_b1c_npoint(self._h, 1 if on else 0))

    def acq_run(self, settings, prn_list=None):
        cs = pack_settings(settings)
        max_prn = max(int(p) for p in np.atleast_1d(settings.acqSatelliteList))
        carr = np.zeros(max_prn)
        cph = np.zeros(max_prn)
        pm = np.zeros(max_prn)
        det = np.zeros(max_prn, dtype=np.int32)
        if prn_list is None:
            pl, npl = None, 0
        else:
            arr = np.ascontiguousarray(prn_list, dtype=np.int32)
            pl, npl = arr.ctypes.data_as(_IP), arr.size
        self._check(self._lib.bds_acq_run(self._h, C.byref(cs), pl, npl, max_prn,
                                          carr.ctypes.data_as(_DP), cph.ctypes.data_as(_DP),
                                          pm.ctypes.data_as(_DP), det.ctypes.data_as(_IP)))
        return carr, cph, pm, det

    # -- weak-signal acquisition (bds_acq_deep*) ----------------------------------------------------
    def acq_deep(self, settings, samples, is_complex, n_blocks, threshold, compensate=True, keep_surface=False, surface_gib=0.0, n_samples=None):
        """bds_acq_deep (a host array) / bds_acq_deep_dev (a device array): non-coherent power sums of the coarse search over n_blocks code
        periods.  The record's bytes go to the library as they are (int16 values as their bytes): what it does not take, it refuses.
        Returns (carrFreq, codePhase, peakMetric, deepMetric, fbin, detected), each 1 x max(acqSatelliteList)."""
        cs = pack_settings(settings)
        max_prn = max(int(p) for p in np.atleast_1d(settings.acqSatelliteList))
        carr, cph, pm, dm = (np.zeros(max_prn) for _ in range(4))
        fb, det = np.zeros(max_prn, dtype=np.int32), np.zeros(max_prn, dtype=np.int32)
        o = DeepOpts(int(n_blocks), 1 if compensate else 0, 1 if keep_surface else 0, float(threshold), float(surface_gib))
        out = [max_prn] + [a.ctypes.data_as(_DP) for a in (carr, cph, pm, dm)] + [fb.ctypes.data_as(_IP), det.ctypes.data_as(_IP)]
        if is_device_array(samples):
            ptr, n_bytes, keep, w16 = device_record(settings, samples, self.device, "the record")
            n = n_samples_of(n_bytes // 2 if w16 else n_bytes, is_complex, n_samples)
            rc = self._lib.bds_acq_deep_dev(self._h, C.byref(cs), ptr, n, sample_format(is_complex), C.byref(o), *out)
        else:
            a = np.asarray(samples)
            w16 = record_is_int16(settings, a.dtype.name, "the record")
            elems = a.size
            a, p = _i8(np.ascontiguousarray(a).view(np.int8) if w16 else a)
            n = n_samples_of(elems, is_complex, n_samples)
            rc = self._lib.bds_acq_deep(self._h, C.byref(cs), p, n, sample_format(is_complex), C.byref(o), *out)
        self._check(rc)
        return carr, cph, pm, dm, fb, det

    def acq_deep_row(self, prn, fbin, n):
        """bds_acq_deep_row: the accumulated surface row of (prn, 1-based bin) of the last acq_deep(keep_surface=True); n = its N lags."""
        row = np.empty(int(n), dtype=np.float32)
        got = self._check(self._lib.bds_acq_deep_row(self._h, int(prn), int(fbin), row.ctypes.data_as(C.POINTER(C.c_float)), row.size))
        return row[:got]

    def acq_deep_fine(self, prn, cap=4096):
        """bds_acq_deep_fine: F over the fine-frequency grid of a PRN of the last acq_deep (empty when it was not detected)."""
        f = np.empty(int(cap))
        return f[:self._check(self._lib.bds_acq_deep_fine(self._h, int(prn), f.ctypes.data_as(_DP), f.size))].copy()

    def acq_deep_release(self):
        """bds_acq_deep_release: give back everything the deep search holds on the device."""
        self._check(self._lib.bds_acq_deep_release(self._h))

    def acquire(self, settings, samples, is_complex=False, n_samples=None):
        cs = pack_settings(settings)
        w16 = record_is_int16(settings, np.asarray(samples).dtype.name, "the block")
        if w16:  # bds_acquire16
            a = _i16(samples, "the block")
            p = a.ctypes.data_as(C.POINTER(C.c_int16))
        else:
            a, p = _i8(samples)
        n = n_samples_of(a.size, is_complex, n_samples)
        entry = self._lib.bds_acquire16 if w16 else self._lib.bds_acquire
        max_prn = max(int(q) for q in np.atleast_1d(settings.acqSatelliteList))
        carr = np.zeros(max_prn)
        cph = np.zeros(max_prn)
        pm = np.zeros(max_prn)
        det = np.zeros(max_prn, dtype=np.int32)
        self._check(entry(self._h, C.byref(cs), p, n, sample_format(is_complex), max_prn,
                          carr.ctypes.data_as(_DP), cph.ctypes.data_as(_DP),
                          pm.ctypes.data_as(_DP), det.ctypes.data_as(_IP)))
        return carr, cph, pm, det

    # -- synthetic IF records (bds_synth*) -----------------------------------------------
    def synth(self, settings, sats, first_sample, n_samples, fmt, out=None, trajectory=None, **opts):
        """bds_synth: samples first_sample .. + n_samples of the record as float64 (fmt 0), int8 (1), int8 I/Q pairs (2) or packed
        uint8 (3); opts as pack_synth.  out="torch": the record stays in HBM -- a torch tensor on the context's device, made by
        bds_synth_dev; the default is the NumPy array.  trajectory (an object with segs, first, seg_log2: synth.Trajectory):
        bds_synth_traj / bds_synth_traj_dev, code and carrier phase from its segments."""
        if out == "torch":
            return self.synth_dev(settings, sats, first_sample, n_samples, fmt, synth_out_torch(fmt, n_samples, self.device),
                                  trajectory=trajectory, **opts)
        if out is not None:
            raise ValueError(f'out must be None (a NumPy array) or "torch" (a tensor on the device), not {out!r}')
        cs = pack_settings(settings)
        arr, o, keep = pack_synth(sats, fmt, **opts)
        out = synth_out(fmt, n_samples)
        if trajectory is None:
            self._check(self._lib.bds_synth(self._h, C.byref(cs), len(sats), arr, C.byref(o), int(first_sample), int(n_samples),
                                            out.ctypes.data_as(C.c_void_p), out.nbytes))
        else:
            t, keep_t = pack_traj(trajectory.segs, trajectory.first, trajectory.seg_log2, len(sats))
            self._check(self._lib.bds_synth_traj(self._h, C.byref(cs), len(sats), arr, C.byref(o), C.byref(t), int(first_sample),
                                                 int(n_samples), out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def synth_dev(self, settings, sats, first_sample, n_samples, fmt, out, trajectory=None, **opts):
        """bds_synth_dev: the same samples written into the device array `out` (float64 for fmt 0, else int8 / uint8; it may be a
        slice at any byte offset, and must hold at least the record); returns `out`.  trajectory: bds_synth_traj_dev."""
        cs = pack_settings(settings)
        arr, o, keep = pack_synth(sats, fmt, **opts)
        synth_out_count(fmt, n_samples)
        t = keep_t = None
        if trajectory is not None:
            t, keep_t = pack_traj(trajectory.segs, trajectory.first, trajectory.seg_log2, len(sats))
        ptr, n_bytes, _ = device_span(out, self.device, dtypes=("float64",) if fmt == 0 else ("int8", "uint8"))
        if t is None:
            self._check(self._lib.bds_synth_dev(self._h, C.byref(cs), len(sats), arr, C.byref(o), int(first_sample), int(n_samples), ptr, n_bytes))
        else:
            self._check(self._lib.bds_synth_traj_dev(self._h, C.byref(cs), len(sats), arr, C.byref(o), C.byref(t), int(first_sample),
                                                     int(n_samples), ptr, n_bytes))
        return out

    def synth_traj_dev(self, settings, sats, trajectory, first_sample, n_samples, fmt, out, **opts):
        """bds_synth_traj_dev: synth_dev with a trajectory."""
        return self.synth_dev(settings, sats, first_sample, n_samples, fmt, out, trajectory=trajectory, **opts)

    def synth_file(self, settings, sats, first_sample, n_samples, fmt, path, piece_samples=0, **opts):
        """bds_synth_file: the same record written to `path`, piece by piece."""
        cs = pack_settings(settings)
        arr, o, keep = pack_synth(sats, fmt, **opts)
        self._check(self._lib.bds_synth_file(self._h, C.byref(cs), len(sats), arr, C.byref(o), int(first_sample), int(n_samples),
                                             os.fsencode(path), int(piece_samples)))

    def synth_noise(self, seed, first, n):
        """bds_synth_noise (test aid): the N(0, 1) pairs (g_I, g_Q) of samples first .. first + n - 1."""
        gi, gq = np.empty(int(n)), np.empty(int(n))
        self._check(self._lib.bds_synth_noise(self._h, int(seed) & (2 ** 64 - 1), int(first), int(n), gi.ctypes.data_as(_DP),
                                              gq.ctypes.data_as(_DP)))
        return gi, gq

    # -- probeData (bds_probe_data*) --------------------------------------------------------
    def probe_set_piece_segments(self, n):
        """bds_probe_set_piece_segments: segments per piece of probe_data on host bytes or a file (0: the default)."""
        self._check(self._lib.bds_probe_set_piece_segments(self._h, int(n)))

    def probe_data(self, settings, source, n_time, n_samples=0):
        """bds_probe_data (host array of the record's bytes), bds_probe_data_file (a path; n_samples 0: the reference's window,
        -1: to the end of the file) or bds_probe_data_dev (a device array, read where it lies).  Returns a dict of arrays and
        integers: hist_i, hist_q, psd, excerpt_re, excerpt_im, the eight statistics, n_segments, n_samples."""
        cs = pack_settings(settings)
        cplx = int(settings.fileType) != 1
        n_time = int(n_time)
        hi, hq = np.zeros(257, dtype=np.int64), np.zeros(257, dtype=np.int64)
        psd = np.full(32768 if cplx else 16385, np.nan)
        ex = np.full((2, max(n_time, 1)), np.nan)
        o = ProbeOut()
        I64 = C.POINTER(C.c_int64)
        o.hist_i, o.hist_q, o.psd, o.cap = hi.ctypes.data_as(I64), hq.ctypes.data_as(I64), psd.ctypes.data_as(_DP), psd.size
        o.excerpt_re, o.excerpt_im = ex[0].ctypes.data_as(_DP), ex[1].ctypes.data_as(_DP)
        if isinstance(source, (str, bytes, os.PathLike)):
            rc = self._lib.bds_probe_data_file(self._h, C.byref(cs), os.fsencode(source), int(n_samples), n_time, C.byref(o))
        elif is_device_array(source):
            ptr, n_bytes, keep, _ = device_record(settings, source, self.device)
            rc = self._lib.bds_probe_data_dev(self._h, C.byref(cs), ptr, n_bytes, n_time, C.byref(o))
        else:
            a, _ = record_bytes(settings, source)
            rc = self._lib.bds_probe_data(self._h, C.byref(cs), a.ctypes.data_as(C.c_void_p), a.size, n_time, C.byref(o))
        self._check(rc)
        out = {k: int(getattr(o, k)) for k in ("n_segments", "n_samples", "min_i", "max_i", "sum_i", "sumsq_i", "min_q", "max_q", "sum_q", "sumsq_q")}
        out.update(hist_i=hi, hist_q=hq if cplx else None, psd=psd[:o.n_psd], excerpt_re=ex[0, :n_time], excerpt_im=ex[1, :n_time] if cplx else None)
        return out

    # -- pulse blanking (bds_blank*) ---------------------------------------------------------
    def blank(self, settings, source, threshold_sq, pre, post, out=None, lead=0, tail=0, duty_samples=0, n_samples=-1, piece_samples=0):
        """bds_blank (host array -> `out`, a host array of the same bytes, or None: a new one), bds_blank_file (path -> the path
        `out`) or bds_blank_dev (a device array -> `out`, a device array of the same size or the same array; None: in place).
        Returns (the record written, a dict of n_samples, n_flagged, n_blanked, n_runs and duty: int32 array or None)."""
        cs = pack_settings(settings)
        o, rep, duty = pack_blank(threshold_sq, pre, post, lead, tail, duty_samples)
        sb = blank_sample_bytes(settings)
        kind, src, dst, n_bytes, res, keep = conditioner_io(settings, source, out, True, self.device, "blanking")
        if kind == "file":
            if int(duty_samples) > 0:  # the window's length is the file's to tell
                n = int(n_samples) if int(n_samples) > 0 else os.path.getsize(source) // sb - int(settings.skipNumberOfBytes)
                duty = blank_duty(rep, n, lead, tail, duty_samples)
            rc = self._lib.bds_blank_file(self._h, C.byref(cs), src, dst, int(n_samples), int(piece_samples), C.byref(o), C.byref(rep))
        else:
            duty = blank_duty(rep, n_bytes // sb, lead, tail, duty_samples)
            rc = (self._lib.bds_blank_dev if kind == "dev" else self._lib.bds_blank)(self._h, C.byref(cs), src, n_bytes, dst, C.byref(o), C.byref(rep))
        self._check(rc)
        r = {k: int(getattr(rep, k)) for k in ("n_samples", "n_flagged", "n_blanked", "n_runs")}
        r["duty"] = None if duty is None else duty[:int(rep.n_duty)]
        return res, r

    # -- tone excision (bds_notch*) -----------------------------------------------------------
    def notch(self, settings, source, steps, block_log2, out=None, first_sample=0, apply=True, n_samples=-1, piece_samples=0, want_est=True):
        """bds_notch (host array -> `out`, a host array of the same bytes, or None: a new one), bds_notch_file (path -> the path
        `out`) or bds_notch_dev (a device array -> `out`, a device array of the same size or the same array; None: in place).
        apply=False estimates only: nothing is written and the record returned is None.  Returns (the record written, a dict of
        n_samples, n_blocks, n_saturated, sum_sq_in, sum_sq_out and est: int32 [n_blocks, n_tones, 2]; want_est=False leaves the
        estimates on the device and est None)."""
        cs = pack_settings(settings)
        o, rep = pack_notch(steps, block_log2, first_sample, apply)
        sb = blank_sample_bytes(settings)
        kind, src, dst, n_bytes, res, keep = conditioner_io(settings, source, out, bool(apply), self.device, "notching")
        if kind == "file":
            n = int(n_samples) if int(n_samples) > 0 else os.path.getsize(source) // sb - int(settings.skipNumberOfBytes)
            est = notch_est(rep, n, block_log2, len(steps), want_est)
            rc = self._lib.bds_notch_file(self._h, C.byref(cs), src, dst, int(n_samples), int(piece_samples), C.byref(o), C.byref(rep))
        else:
            est = notch_est(rep, n_bytes // sb, block_log2, len(steps), want_est)
            rc = (self._lib.bds_notch_dev if kind == "dev" else self._lib.bds_notch)(self._h, C.byref(cs), src, n_bytes, dst, C.byref(o), C.byref(rep))
        self._check(rc)
        r = {k: int(getattr(rep, k)) for k in ("n_samples", "n_blocks", "n_saturated", "sum_sq_in", "sum_sq_out")}
        r["est"] = None if est is None else est[:r["n_blocks"]]
        return res, r

    def frame_sync(self, signal, prns, prompt, cap=64):
        """bds_frame_sync: prompt [n_ch, n] -> (xcorr int32 [n_ch, M], [1-based index arrays])."""
        pr = np.ascontiguousarray(prompt, dtype=np.float64)
        n_ch, n = pr.shape
        sig = SIGNAL[str(signal).upper()]
        m = 1800 if sig == SIGNAL["B1C"] else 120
        M = max(n, m)
        prn = np.ascontiguousarray(prns, dtype=np.int32)
        xc = np.zeros((n_ch, M), dtype=np.int32)
        idx = np.zeros((n_ch, cap), dtype=np.int32)
        cnt = np.zeros(n_ch, dtype=np.int32)
        self._check(self._lib.bds_frame_sync(self._h, sig, n_ch, prn.ctypes.data_as(_IP), pr.ctypes.data_as(_DP), n,
                                             xc.ctypes.data_as(_IP), idx.ctypes.data_as(_IP), cnt.ctypes.data_as(_IP), cap))
        if np.any(cnt > cap):
            return self.frame_sync(signal, prns, prompt, cap=int(cnt.max()))
        return xc, [idx[c, :cnt[c]].copy() for c in range(n_ch)]

    def nav_decode(self, settings, prns, sync_prompt, data_prompt=None, cap=8):
        """bds_nav_decode: prompts [n_ch, n] -> per channel {"frames": [nav_frame_dict, ...] (the first `cap`), "n_frames",
        "eph": eph_dict, "firstSubFrame", "TOW"} (the last two +inf where nothing decoded)."""
        cs = pack_settings(settings)
        sp = np.ascontiguousarray(sync_prompt, dtype=np.float64)
        if sp.ndim != 2:
            raise ValueError("nav_decode: sync_prompt is [n_ch, n]")
        n_ch, n = sp.shape
        dp = None
        if data_prompt is not None:
            dp = np.ascontiguousarray(data_prompt, dtype=np.float64)
            if dp.shape != sp.shape:
                raise ValueError(f"nav_decode: data_prompt {dp.shape} and sync_prompt {sp.shape} differ in shape")
        prn = np.ascontiguousarray(prns, dtype=np.int32)
        if prn.shape != (n_ch,):
            raise ValueError(f"nav_decode: {n_ch} channels, {prn.size} PRNs")
        cap = int(cap)
        frames = (NavFrame * max(1, n_ch * cap))()
        eph = (Eph * n_ch)()
        for e in eph:
            e.size = C.sizeof(Eph)
        cnt = np.zeros(n_ch, dtype=np.int32)
        first = np.zeros(n_ch, dtype=np.float64)
        tow = np.zeros(n_ch, dtype=np.float64)
        self._check(self._lib.bds_nav_decode(self._h, C.byref(cs), n_ch, prn.ctypes.data_as(_IP), sp.ctypes.data_as(_DP),
                                             dp.ctypes.data_as(_DP) if dp is not None else None, n, frames, cnt.ctypes.data_as(_IP),
                                             cap, eph, first.ctypes.data_as(_DP), tow.ctypes.data_as(_DP)))
        return [{"frames": [nav_frame_dict(frames[c * cap + k], cs.signal) for k in range(min(cap, int(cnt[c])))],
                 "n_frames": int(cnt[c]), "eph": eph_dict(eph[c]), "firstSubFrame": float(first[c]), "TOW": float(tow[c])}
                for c in range(n_ch)]

    def pvt_measure(self, settings, ready, absolute_sample, code_freq, rem_code_phase, ephs, sub_frame_start, tow, sample_start,
                    meas_sample_step, n_meas):
        """bds_pvt_measure: the three series [n_ch, n] -> (transmitTime [n_meas, n_ch], satPos [n_meas, n_ch, 3], satClkCorr
        [n_meas, n_ch]); NaN on a channel that is not ready."""
        cs = pack_settings(settings)
        a = np.ascontiguousarray(absolute_sample, dtype=np.float64)
        if a.ndim != 2:
            raise ValueError("pvt_measure: absoluteSample is [n_ch, n]")
        n_ch, n = a.shape
        cf, rp = _series(code_freq, a.shape, "codeFreq"), _series(rem_code_phase, a.shape, "remCodePhase")
        sfs, tw = _series(sub_frame_start, (n_ch,), "subFrameStart"), _series(tow, (n_ch,), "TOW")
        rd = np.ascontiguousarray(ready, dtype=np.int32)
        if rd.shape != (n_ch,) or len(ephs) != n_ch:
            raise ValueError(f"pvt_measure: {n_ch} channels, {rd.size} ready flags, {len(ephs)} ephemerides")
        n_meas = int(n_meas)
        tt, sp, ck = np.zeros((n_meas, n_ch)), np.zeros((n_meas, n_ch, 3)), np.zeros((n_meas, n_ch))
        self._check(self._lib.bds_pvt_measure(self._h, C.byref(cs), n_ch, n, rd.ctypes.data_as(_IP), a.ctypes.data_as(_DP),
                                              cf.ctypes.data_as(_DP), rp.ctypes.data_as(_DP), eph_array(ephs), sfs.ctypes.data_as(_DP),
                                              tw.ctypes.data_as(_DP), float(sample_start), float(meas_sample_step), n_meas,
                                              tt.ctypes.data_as(_DP), sp.ctypes.data_as(_DP), ck.ctypes.data_as(_DP)))
        return tt, sp, ck

    def post_navigation(self, settings, status, prns, absolute_sample, code_freq, rem_code_phase, ephs, sub_frame_start, tow):
        """bds_post_navigation: plan, measure, solve -> (the arrays of navSolutions by name, or None when there is no solution;
        the ready flags per channel)."""
        cs, pp = pack_settings(settings), pack_pvt_params(settings)
        a = np.ascontiguousarray(absolute_sample, dtype=np.float64)
        if a.ndim != 2:
            raise ValueError("post_navigation: absoluteSample is [n_ch, n]")
        n_ch, n = a.shape
        cf, rp = _series(code_freq, a.shape, "codeFreq"), _series(rem_code_phase, a.shape, "remCodePhase")
        sfs, tw = _series(sub_frame_start, (n_ch,), "subFrameStart"), _series(tow, (n_ch,), "TOW")
        prn = np.ascontiguousarray(prns, dtype=np.int32)
        if prn.shape != (n_ch,) or len(ephs) != n_ch:
            raise ValueError(f"post_navigation: {n_ch} channels, {prn.size} PRNs, {len(ephs)} ephemerides")
        st, eph = _status_bytes(status, n_ch), eph_array(ephs)
        # the capacity: what the plan can give at most, (last - first sample) / step
        step = math.trunc(cs.samplingFreq * pp.navSolPeriod / 1000)
        cap = max(1, int((np.nanmax(a) - np.nanmin(a)) // step) + 1) if step >= 1 and np.isfinite(a).any() else 1
        o, arrays = _pvt_out(n_ch, cap)
        ready = np.zeros(n_ch, dtype=np.int32)
        n_meas = C.c_int32(0)
        rc = self._lib.bds_post_navigation(self._h, C.byref(cs), C.byref(pp), n_ch, n, st, prn.ctypes.data_as(_IP), a.ctypes.data_as(_DP),
                                           cf.ctypes.data_as(_DP), rp.ctypes.data_as(_DP), eph, sfs.ctypes.data_as(_DP),
                                           tw.ctypes.data_as(_DP), ready.ctypes.data_as(_IP), C.byref(n_meas), C.byref(o))
        self._check(rc)
        if rc == 0:
            return None, ready
        return {f: np.ascontiguousarray(v[..., :rc]) for f, v in arrays.items()}, ready

    def unpack_cplx(self, data):
        """bds_unpack_cplx: uint8[n] packed samples -> int8[4n] I/Q pairs (unpack_cplx.m)."""
        d = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        out = np.empty(4 * d.size, dtype=np.int8)
        self._check(self._lib.bds_unpack_cplx(self._h, d.ctypes.data_as(C.POINTER(C.c_uint8)), d.size,
                                              out.ctypes.data_as(C.POINTER(C.c_int8))))
        return out

    def unpack_cplx_file(self, filename_in, filename_out):
        self._check(self._lib.bds_unpack_cplx_file(self._h, os.fsencode(filename_in), os.fsencode(filename_out)))

    def acq_grid(self, n_prn, n_bins):
        rm = np.zeros(n_prn * n_bins, dtype=np.float32)
        ra = np.zeros(n_prn * n_bins, dtype=np.int32)
        self._check(self._lib.bds_acq_grid(self._h, rm.ctypes.data_as(C.POINTER(C.c_float)),
                                           ra.ctypes.data_as(_IP), rm.size))
        return rm.reshape(n_prn, n_bins), ra.reshape(n_prn, n_bins)

    def acq_candidates(self, prn):
        """(bin, codePhase) cells of `prn` the last run refined in f64, 1-based: int array [n, 2]."""
        n = self._check(self._lib.bds_acq_candidates(self._h, int(prn), None, None, 0))
        b = np.zeros(max(n, 1), dtype=np.int32)
        l = np.zeros(max(n, 1), dtype=np.int64)
        self._check(self._lib.bds_acq_candidates(self._h, int(prn), b.ctypes.data_as(_IP),
                                                 l.ctypes.data_as(C.POINTER(C.c_int64)), n))
        return np.stack([b[:n].astype(np.int64), l[:n]], axis=1)

    def acq_peaks(self, max_prn):
        pk = np.zeros(max_prn)
        dn = np.zeros(max_prn)
        fb = np.zeros(max_prn, dtype=np.int32)
        self._check(self._lib.bds_acq_peaks(self._h, max_prn, pk.ctypes.data_as(_DP), dn.ctypes.data_as(_DP),
                                            fb.ctypes.data_as(_IP)))
        return pk, dn, fb

    def acq_coherent_sums(self, settings, prn, phase, freqs, mode):
        """f64 coherent sums of caller-chosen cells (bds_acq_coherent_sums): complex array, mode 0 [nf, ncomp],
        modes 1 / 2 [segments * components, nf]."""
        cs = pack_settings(settings)
        fr = np.ascontiguousarray(freqs, dtype=np.float64)
        cap = max(int(getattr(settings, "fineNoncoh", 1) or 1), 1) * 2 * max(len(fr), 1)  # segments x components x frequencies
        out = np.zeros(2 * cap)
        n = self._check(self._lib.bds_acq_coherent_sums(self._h, C.byref(cs), int(prn), int(phase), fr.ctypes.data_as(_DP), len(fr),
                                                        int(mode), out.ctypes.data_as(_DP), cap))
        z = out[:2 * n:2] + 1j * out[1:2 * n:2]
        return z.reshape(len(fr), -1) if mode == 0 else z.reshape(-1, len(fr))  # modes 1 / 2: rows = (segment, component)

    def timing(self) -> dict:
        t = Timing()
        self._check(self._lib.bds_get_timing(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in Timing._fields_ if not f.startswith("reserved")}

    # -- tracking --------------------------------------------------------------------
    def track(self, settings, source, channels, n_epochs, n_cno, fields):
        """source: file path (str/bytes), int8 array of raw file bytes (uint8 for a packed fileType-3 record; an int16 array of
        samples with settings.dataType 'int16'), or those bytes as a device array (bds_track_dev).
        Returns dict field -> array [n_ch, n_epochs] (C/N0 fields [n_ch, n_cno])."""
        cs = pack_settings(settings)
        nch = len(channels)
        carr = (Channel * nch)()
        for i, ch in enumerate(channels):
            carr[i].PRN = int(ch.PRN)
            carr[i].status = ord(ch.status) if isinstance(ch.status, str) else int(ch.status)
            carr[i].acquiredFreq = float(ch.acquiredFreq)
            carr[i].codePhase = float(ch.codePhase)
            carr[i].codeFreq = float(ch.codeFreq)
        out = TrackOut()
        out.n_ch, out.n_epochs, out.n_cno = nch, n_epochs, n_cno
        arrays = {}
        for f in fields:
            n = n_cno if f in ("DataCNo", "DataPLD", "PilotCNo", "PilotPLD", "SigCNo") else n_epochs
            arrays[f] = np.zeros((nch, n))
            setattr(out, f, arrays[f].ctypes.data_as(_DP))
        completed = np.zeros(nch, dtype=np.int32)
        status = np.zeros(nch, dtype=np.int32)
        out.completed = completed.ctypes.data_as(_IP)
        out.status = status.ctypes.data_as(_IP)
        if isinstance(source, (str, bytes, os.PathLike)):
            path = os.fsencode(source)
            self._check(self._lib.bds_track(self._h, C.byref(cs), path, nch, carr, C.byref(out)))
        elif is_device_array(source):
            ptr, n_bytes, keep, _ = device_record(settings, source, self.device)
            self._check(self._lib.bds_track_dev(self._h, C.byref(cs), ptr, n_bytes, nch, carr, C.byref(out)))
        else:
            a, _ = record_bytes(settings, source)
            self._check(self._lib.bds_track_mem(self._h, C.byref(cs), a.ctypes.data_as(C.POINTER(C.c_int8)), a.size, nch, carr, C.byref(out)))
        arrays["completed"] = completed
        arrays["status"] = status
        return arrays

    @staticmethod
    def _channels(channels):
        carr = (Channel * len(channels))()
        for i, ch in enumerate(channels):
            carr[i].PRN = int(ch.PRN)
            carr[i].status = ord(ch.status) if isinstance(ch.status, str) else int(ch.status)
            carr[i].acquiredFreq = float(ch.acquiredFreq)
            carr[i].codePhase = float(ch.codePhase)
            carr[i].codeFreq = float(ch.codeFreq)
        return carr

    # -- tracking sessions (bds_track_open* .. bds_track_close): a session handle is the dict these return -------------
    def _session(self, h, settings, channels, keep=None):
        if not h:
            raise BdsError(-1, self._lib.bds_last_error(self._h).decode())
        return {"handle": h, "n_ch": len(channels), "fileType": int(settings.fileType), "keep": keep, "feed": False,
                "w16": data_type_code(getattr(settings, "dataType", "schar")) == 1}

    def track_open(self, settings, path_or_bytes, channel):
        """bds_track_open (a path) / bds_track_open_mem (int8 array of raw file bytes, uint8 for a packed fileType-3 record;
        the array is kept alive until track_close) / bds_track_open_dev (those bytes as a device array)."""
        if is_device_array(path_or_bytes):
            return self.track_open_dev(settings, path_or_bytes, channel)
        cs = pack_settings(settings)
        carr = self._channels(channel)
        if isinstance(path_or_bytes, (str, bytes, os.PathLike)):
            h = self._lib.bds_track_open(self._h, C.byref(cs), os.fsencode(path_or_bytes), len(channel), carr)
            return self._session(h, settings, channel)
        a, _ = record_bytes(settings, path_or_bytes)
        h = self._lib.bds_track_open_mem(self._h, C.byref(cs), a.ctypes.data_as(C.POINTER(C.c_int8)), a.size, len(channel), carr)
        return self._session(h, settings, channel, keep=a)

    def track_dev(self, settings, source, channels, n_epochs, n_cno, fields):
        """bds_track_dev: track() on the raw file bytes in device memory."""
        if not is_device_array(source):
            device_span(source, self.device)  # (anything but a device array raises here)
        return self.track(settings, source, channels, n_epochs, n_cno, fields)

    def track_open_dev(self, settings, source, channel):
        """bds_track_open_dev: the record is the device array `source` (raw file bytes); it is kept alive until track_close and
        must stay unmodified until then."""
        cs = pack_settings(settings)
        ptr, n_bytes, keep, _ = device_record(settings, source, self.device)
        h = self._lib.bds_track_open_dev(self._h, C.byref(cs), ptr, n_bytes, len(channel), self._channels(channel))
        return self._session(h, settings, channel, keep=keep)

    def track_feed_dev(self, sess, data, last=False) -> int:
        """bds_track_feed_dev: track_feed from a device array; the bytes are the caller's again on return."""
        name = device_dtype_name(data)
        if sess.get("w16") and name == "int8":
            raise BdsError(-1, "settings.dataType is 'int16' but the bytes fed are an int8 array: feed int16 samples, or raw bytes as uint8")
        if not sess.get("w16") and name == "int16":
            raise BdsError(-1, "settings.dataType is 'schar' but the samples fed are an int16 array: int16 samples go with dataType 'int16'")
        ptr, n_bytes, keep = device_span(data, self.device, dtypes=("int16", "uint8") if sess.get("w16") else ("int8", "uint8"))
        check_feed_span(sess, n_bytes)
        return self._check(self._lib.bds_track_feed_dev(sess["handle"], ptr, n_bytes, int(bool(last))))

    def track_open_feed(self, settings, origin, channel):
        """bds_track_open_feed: the record is what track_feed appends; sample `origin` (a multiple of 32) is the first one fed."""
        check_feed_origin(origin)
        cs = pack_settings(settings)
        h = self._lib.bds_track_open_feed(self._h, C.byref(cs), int(origin), len(channel), self._channels(channel))
        sess = self._session(h, settings, channel)
        sess["feed"] = True
        return sess

    def track_feed(self, sess, data, last=False) -> int:
        """bds_track_feed: bytes of the settings' fileType; returns how many were taken (fewer than offered: the span is full).
        A device array goes through bds_track_feed_dev."""
        if is_device_array(data):
            return self.track_feed_dev(sess, data, last)
        a = check_feed_bytes(sess, data)
        return self._check(self._lib.bds_track_feed(sess["handle"], a.ctypes.data_as(C.POINTER(C.c_int8)), a.size, int(bool(last))))

    def track_advance(self, sess, max_epochs, n_cno, fields):
        """bds_track_advance: (k, dict field -> array [n_ch, max_epochs] (C/N0 fields [n_ch, n_cno]) plus completed, status and
        n_cno_done [n_ch])."""
        out, arrays = self._track_out(sess["n_ch"], int(max_epochs), int(n_cno), fields)
        arrays["n_cno_done"] = np.zeros(sess["n_ch"], dtype=np.int32)
        k = self._check(self._lib.bds_track_advance(sess["handle"], int(max_epochs), C.byref(out), arrays["n_cno_done"].ctypes.data_as(_IP)))
        return k, arrays

    def track_session_info(self, sess) -> dict:
        """bds_track_session_info: epochs_done / next_sample per channel, fed_end (samples), resident_bytes."""
        done = np.zeros(sess["n_ch"], dtype=np.int32)
        nxt = np.zeros(sess["n_ch"], dtype=np.int64)
        fed, res = C.c_longlong(0), C.c_longlong(0)
        self._check(self._lib.bds_track_session_info(sess["handle"], done.ctypes.data_as(_IP), nxt.ctypes.data_as(C.POINTER(C.c_longlong)),
                                                     C.byref(fed), C.byref(res)))
        return {"epochs_done": done, "next_sample": nxt, "fed_end": int(fed.value), "resident_bytes": int(res.value)}

    def track_close(self, sess) -> None:
        """bds_track_close (a second close does nothing)."""
        if sess.get("handle"):
            self._lib.bds_track_close(sess["handle"])
        sess["keep"] = None

    def _track_out(self, nch, n_epochs, n_cno, fields):
        out = TrackOut()
        out.n_ch, out.n_epochs, out.n_cno = nch, n_epochs, n_cno
        arrays = {}
        for f in fields:
            n = n_cno if f in ("DataCNo", "DataPLD", "PilotCNo", "PilotPLD", "SigCNo") else n_epochs
            arrays[f] = np.zeros((nch, n))
            setattr(out, f, arrays[f].ctypes.data_as(_DP))
        arrays["completed"] = np.zeros(nch, dtype=np.int32)
        arrays["status"] = np.zeros(nch, dtype=np.int32)
        out.completed = arrays["completed"].ctypes.data_as(_IP)
        out.status = arrays["status"].ctypes.data_as(_IP)
        return out, arrays

    def pre_run_device(self, settings, carr_freq, code_phase, peak_metric):
        """bds_pre_run_device: preRun.m:61-76 as a device kernel; returns the ctypes channel array."""
        cs = pack_settings(settings)
        a = np.ascontiguousarray(carr_freq, dtype=np.float64)
        b = np.ascontiguousarray(code_phase, dtype=np.float64)
        c = np.ascontiguousarray(peak_metric, dtype=np.float64)
        ch = (Channel * int(settings.numberOfChannels))()
        self._check(self._lib.bds_pre_run_device(self._h, C.byref(cs), a.size, a.ctypes.data_as(_DP), b.ctypes.data_as(_DP),
                                                 c.ctypes.data_as(_DP), ch))
        return ch

    def acquire_track(self, settings, samples, is_complex, path, n_epochs, n_cno, fields):
        """bds_acquire_track: acquisition -> device preRun -> tracking of the record at `path` in one native call.
        Returns ((carrFreq, codePhase, peakMetric, detected), channel array, dict of trackResults arrays)."""
        cs = pack_settings(settings)
        w16 = record_is_int16(settings, np.asarray(samples).dtype.name, "the block")
        if w16:  # bds_acquire_track16
            a = _i16(samples, "the block")
            p = a.ctypes.data_as(C.POINTER(C.c_int16))
        else:
            a, p = _i8(samples)
        n = n_samples_of(a.size, is_complex)
        entry = self._lib.bds_acquire_track16 if w16 else self._lib.bds_acquire_track
        max_prn = max(int(q) for q in np.atleast_1d(settings.acqSatelliteList))
        carr, cph, pm = np.zeros(max_prn), np.zeros(max_prn), np.zeros(max_prn)
        det = np.zeros(max_prn, dtype=np.int32)
        nch = int(settings.numberOfChannels)
        ch = (Channel * nch)()
        out, arrays = self._track_out(nch, n_epochs, n_cno, fields)
        self._check(entry(self._h, C.byref(cs), p, n, sample_format(is_complex), max_prn, carr.ctypes.data_as(_DP),
                                                cph.ctypes.data_as(_DP), pm.ctypes.data_as(_DP), det.ctypes.data_as(_IP),
                                                os.fsencode(path), ch, C.byref(out)))
        return (carr, cph, pm, det), ch, arrays

    def track_loaded_bytes(self) -> int:
        """Bytes of the record the last track() call copied host-to-device: the window the channels can touch; for a streamed
        run the total over its pieces, which is about that window."""
        return int(self._lib.bds_track_loaded_bytes(self._h))

    def track_set_resident_limit(self, n_bytes: int) -> None:
        """bds_track_set_resident_limit: at most `n_bytes` of the IF record are resident in HBM in the tracking calls that
        follow on this context -- a larger window is streamed through in pieces, with identical results.  0 = no limit (the
        default: one window when it can be allocated, streamed when it cannot)."""
        self._check(self._lib.bds_track_set_resident_limit(self._h, int(n_bytes)))
        self._track_limit = int(n_bytes)

    def track_resident_limit(self) -> int:
        """The limit set with track_set_resident_limit (0: none)."""
        return getattr(self, "_track_limit", 0)

    def track_stream_info(self) -> dict:
        """bds_track_stream_info of the last tracking call: `pieces` loaded (1 for a one-window run), `resident_max_bytes` of
        the record in HBM at a time, `repeated_batches` run again because a block left the resident span."""
        pieces, rep, res = C.c_int32(0), C.c_int32(0), C.c_longlong(0)
        self._check(self._lib.bds_track_stream_info(self._h, C.byref(pieces), C.byref(res), C.byref(rep)))
        return {"pieces": int(pieces.value), "resident_max_bytes": int(res.value), "repeated_batches": int(rep.value)}

    def track_correlate(self, settings, file_bytes, prns, state6):
        cs = pack_settings(settings)
        a, _ = record_bytes(settings, file_bytes)
        p = a.ctypes.data_as(C.POINTER(C.c_int8))
        prn = np.ascontiguousarray(prns, dtype=np.int32)
        st = np.ascontiguousarray(state6, dtype=np.float64).reshape(prn.size, 6)
        sums = np.zeros((prn.size, 18))
        self._check(self._lib.bds_track_correlate(self._h, C.byref(cs), p, a.size, prn.size,
                                                  prn.ctypes.data_as(_IP), st.ctypes.data_as(_DP),
                                                  sums.ctypes.data_as(_DP)))
        return sums

    def corr_function(self, settings, source, prns, state6, taps):
        """bds_corr_function / _mem / _dev: the correlation function of the items (prns[i], state6[i]) -- one epoch of one channel
        each, as track_correlate takes them -- at the tap offsets `taps` (primary-code chips).  source: a path, the record's raw
        bytes as track() takes them, or those bytes as a device array.  Returns complex128 [n_items, n_comp, n_taps], I + jQ of the
        raw sums; comp 0 data, 1 the pilot (when on), 2 the pilot BOC(6,1) (wide-band mode)."""
        cs = pack_settings(settings)
        prn = np.ascontiguousarray(prns, dtype=np.int32).reshape(-1)
        st = np.ascontiguousarray(state6, dtype=np.float64).reshape(-1, 6)
        if st.shape[0] != prn.size:
            raise ValueError(f"corr_function: {prn.size} PRNs for {st.shape[0]} states")
        tp = np.ascontiguousarray(taps, dtype=np.float64).reshape(-1)
        out = np.zeros((max(prn.size, 1), 3, max(tp.size, 1), 2))  # room for three components; n_comp tells how many came back
        n_comp = C.c_int32(0)
        tail = (prn.size, prn.ctypes.data_as(_IP), st.ctypes.data_as(_DP), tp.size, tp.ctypes.data_as(_DP), out.ctypes.data_as(_DP),
                C.byref(n_comp))
        if isinstance(source, (str, bytes, os.PathLike)):
            self._check(self._lib.bds_corr_function(self._h, C.byref(cs), os.fsencode(source), *tail))
        elif is_device_array(source):
            ptr, n_bytes, keep, _ = device_record(settings, source, self.device)
            self._check(self._lib.bds_corr_function_dev(self._h, C.byref(cs), ptr, n_bytes, *tail))
        else:
            a, _ = record_bytes(settings, source)
            self._check(self._lib.bds_corr_function_mem(self._h, C.byref(cs), a.ctypes.data_as(C.POINTER(C.c_int8)), a.size, *tail))
        nc = int(n_comp.value)
        z = out.reshape(-1)[: prn.size * nc * tp.size * 2].reshape(prn.size, nc, tp.size, 2)
        return z[..., 0] + 1j * z[..., 1]

    def track_colon(self, a, d, b, k):
        """Test aid: element k[i] of the colon vector a[i]:d[i]:b[i] as the tracking kernels form it, evaluated on the device.
        Returns (value, c_end, n_intervals)."""
        k = np.ascontiguousarray(k, dtype=np.int32)
        a, d, b = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), k.shape)) for v in (a, d, b))
        val, c_end, n_int = np.empty(k.size), np.empty(k.size), np.empty(k.size, dtype=np.int32)
        self._check(self._lib.bds_track_colon(self._h, k.size, a.ctypes.data_as(_DP), d.ctypes.data_as(_DP), b.ctypes.data_as(_DP),
                                              k.ctypes.data_as(_IP), val.ctypes.data_as(_DP), c_end.ctypes.data_as(_DP),
                                              n_int.ctypes.data_as(_IP)))
        return val, c_end, n_int

    def track_cno(self, settings, prompts, done, n_cno, pieces=None):
        """Test aid: the C/N0 + lock-detector post-pass on the caller's prompts [4, n_ch, n_epochs] (I_P, Q_P, Pilot_I_P, Pilot_Q_P)
        with done[ch] completed epochs; pieces=None: the kernel of bds_track, once; a list of piece lengths: the kernel of
        bds_track_advance once per piece.  Returns cno5 [5, n_ch, n_cno] (DataCNo, DataPLD, PilotCNo, PilotPLD, SigCNo)."""
        cs = pack_settings(settings)
        pr = np.ascontiguousarray(prompts, dtype=np.float64)
        if pr.ndim != 3 or pr.shape[0] != 4:
            raise ValueError("prompts must be [4, n_ch, n_epochs]")
        _, n_ch, n_epochs = pr.shape
        dn = np.ascontiguousarray(done, dtype=np.int32)
        if dn.shape != (n_ch,):
            raise ValueError("done must be [n_ch]")
        pc = np.ascontiguousarray(pieces if pieces is not None else [], dtype=np.int32)
        out = np.zeros((5, n_ch, int(n_cno)))
        self._check(self._lib.bds_track_cno(self._h, C.byref(cs), n_ch, n_epochs, pr.ctypes.data_as(_DP), dn.ctypes.data_as(_IP),
                                            pc.size, pc.ctypes.data_as(_IP) if pc.size else None, int(n_cno), out.ctypes.data_as(_DP)))
        return out

    def track_update(self, settings, state10, sums18):
        """Test aid: the loop update of one epoch by the update kernel.  state10 [n_ch, 10] (UPDATE_STATE order), sums18 [n_ch, 18].
        Returns (next state [n_ch, 10], active [n_ch], completed [n_ch], dict per-epoch field -> [n_ch])."""
        cs = pack_settings(settings)
        st = np.ascontiguousarray(state10, dtype=np.float64)
        sm = np.ascontiguousarray(sums18, dtype=np.float64)
        if st.ndim != 2 or st.shape[1] != 10 or sm.shape != (st.shape[0], 18):
            raise ValueError("state10 must be [n_ch, 10] and sums18 [n_ch, 18]")
        n_ch = st.shape[0]
        new = np.zeros((n_ch, 10))
        active, completed = np.zeros(n_ch, dtype=np.int32), np.zeros(n_ch, dtype=np.int32)
        out = np.zeros((21, n_ch))
        self._check(self._lib.bds_track_update(self._h, C.byref(cs), n_ch, st.ctypes.data_as(_DP), sm.ctypes.data_as(_DP), new.ctypes.data_as(_DP),
                                               active.ctypes.data_as(_IP), completed.ctypes.data_as(_IP), out.ctypes.data_as(_DP)))
        return new, active, completed, {f: out[i] for i, f in enumerate(TRACK_FIELDS[:21])}


def calc_loop_coef(lbw, zeta, k):
    t1, t2 = C.c_double(), C.c_double()
    lib().bds_calc_loop_coef(lbw, zeta, k, C.byref(t1), C.byref(t2))
    return t1.value, t2.value


def calc_loop_coef_carr(settings):
    cs = pack_settings(settings)
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    lib().bds_calc_loop_coef_carr(C.byref(cs), C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def calc_weighing_factor(settings):
    cs = pack_settings(settings)
    return float(lib().bds_calc_weighing_factor(C.byref(cs)))


def resample_plan(settings):
    """(new_fs, new_if, (wp1, wp2)) of the acquisition's resampling branch, or None when it is not taken
    (acquisition.m:54-55,66,103,119)."""
    cs = pack_settings(settings)
    fs, fi, wp = C.c_double(), C.c_double(), (C.c_double * 2)()
    rc = lib().bds_resample_plan(C.byref(cs), C.byref(fs), C.byref(fi), wp)
    if rc < 0:
        raise BdsError(rc, "bds_resample_plan")
    return (fs.value, fi.value, (wp[0], wp[1])) if rc else None


def fir1_bandpass(n_taps, wp1, wp2):
    """b = fir1(n_taps - 1, [wp1 wp2])."""
    b = np.zeros(n_taps)
    rc = lib().bds_fir1_bandpass(int(n_taps), float(wp1), float(wp2), b.ctypes.data_as(_DP))
    if rc < 0:
        raise BdsError(rc, "bds_fir1_bandpass")
    return b


def pre_run(settings, carr_freq, code_phase, peak_metric):
    cs = pack_settings(settings)
    n = len(carr_freq)
    nch = int(settings.numberOfChannels)
    ch = (Channel * nch)()
    a = np.ascontiguousarray(carr_freq, dtype=np.float64)
    b = np.ascontiguousarray(code_phase, dtype=np.float64)
    c = np.ascontiguousarray(peak_metric, dtype=np.float64)
    rc = lib().bds_pre_run(C.byref(cs), n, a.ctypes.data_as(_DP), b.ctypes.data_as(_DP), c.ctypes.data_as(_DP), ch)
    if rc < 0:
        raise BdsError(rc, "bds_pre_run")
    return ch
