"""bds_amd -- MI355X-native acquisition / tracking correlators for BDS-3 B1C and B2a.

Host-side mirror of the reference's MATLAB call surface
(lyf8118/BDS-3-B1C-B2a-SDR-receiver):

    settings   = init_settings_b1c() / init_settings_b2a()      initSettings.m
    acqResults = acquisition(longSignal, settings)              acquisition.m / GPU_acquisition.m
    acqResults = acquisition_deep(longSignal, settings, K, thr) weak signals: power sums of the search over K code periods (extension)
    channel    = pre_run(acqResults, settings)                  include/preRun.m
    trackResults, channel = tracking(fid, channel, settings)    tracking.m / NB_tracking.m / WB_tracking.m
    TrackSession(source, channel, settings)                     the same run advanced in pieces, or fed by the caller
    probe_data(settings) / probe_data(fileName, settings)       include/probeData.m (the numbers; also arrays and device tensors)
    blank_pulses(source, settings, ...)                         pulse blanking of a record (DME / TACAN), file, array or device tensor
    notch_tones(source, settings, tones, ...)                   excision of CW / narrow-band interference, block by block, same sources
    frame_sync(trackResults, settings)                          include/BCNAV?decoding.m, the correlators
    nav_decode(trackResults, settings)                          include/BCNAV?decoding.m + ephemeris.m: eph, firstSubFrame, TOW
    navSolutions, eph = post_navigation(trackResults, settings) postNavigation.m: pseudoranges, satellite and receiver positions

All numeric work happens in ``libbds_mi355x.so`` (HIP kernels for gfx950) through
the C ABI of ``include/bds_mi355x.h``; there is no CPU fallback.
"""
from .settings import Settings, init_settings_b1c, init_settings_b2a  # noqa: F401
from .acquisition import acquisition, GPU_acquisition, acquisition_deep, AcqResults, get_context, release_context  # noqa: F401
from .tracking import tracking, NB_tracking, WB_tracking, pre_run, acquire_track, TrackResults, TrackSession  # noqa: F401
from .framesync import frame_sync, unpack_cplx  # noqa: F401
from .distributed import shard_prns, shard_joint, sharded_acquisition, sharded_acquisition_joint  # noqa: F401
from .probedata import probe_data, ProbeResult  # noqa: F401
from .blank import blank_pulses, blank_threshold, BlankReport  # noqa: F401
from .notch import notch_tones, notch_step, notch_detect, notch_refine, NotchReport  # noqa: F401
from .corrfn import corr_function, track_states  # noqa: F401
from .navdecode import nav_decode, BCNAV1decoding, BCNAV2decoding  # noqa: F401
from .pvt import post_navigation, postNavigation, pvt_plan, pvt_measure, pvt_solve  # noqa: F401
from . import native, synth  # noqa: F401
