"""Open-loop tracking states on which MATLAB's colon vector is NOT a + k d (shared by tests/test_track_colon_gpu.py, the CPU guards
of tests/test_matlab_colon.py and tools/colon_effect.py --states).

The reference's replica index vectors are colon vectors tcode = a : d : b (B2a/tracking.m:260-286, B1C/NB_tracking.m:271-297,
WB_tracking.m:289-317); MATLAB builds the second half of such a vector from the right-hand end (oracle/matlab.py m_colon).  On the
records of the rest of the suite the two forms give the same ceil() for every sample.  They part where many samples sit ON a code-unit
boundary: a sampling rate that is a multiple of the code rate's half-chip (30.69 / 61.38 / 92.07 / 102.3 MS/s), or a code rate that is
a short fraction of another rate (fs / 10 at 99.375 MS/s), with a code phase on that lattice -- remCodePhase = 0 and codeFreq =
codeFreqBasis, the state EVERY tracking run starts in, among them.

Every state is checked on the CPU (tests/test_matlab_colon.py): at least 100 samples whose index differs between the two forms in an
index the state's mode reads, and oracle sums that differ by at least 1e-3 of |P| between the two forms on the state's record.
"""
import ctypes
import functools
from collections import namedtuple

import numpy as np

import bds_amd
from bds_amd import synth
from oracle import cfast
from oracle import codes as ocodes

CODE_LEN = 10230
# blk: None = the block tracking itself would take, ceil((codeLength - rem) / step) (tracking.m:233); an int = that many samples.
# code_freq: None = the nominal code rate.  counted: False = an extra case with fewer than 100 differing samples (not part of the
# coverage, exempt from the two CPU conditions' thresholds but still required to differ).
State = namedtuple("State", "name signal mode fs IF iq spacing rem code_freq blk counted")


def _st(name, signal, mode, fs, IF, iq=False, rem=0.0, code_freq=None, blk=None, dblk=0, counted=True, spacing=None):
    spacing = spacing or spacing_of(signal, mode)
    s = State(name, signal, mode, float(fs), float(IF), bool(iq), spacing, float(rem), code_freq, blk, counted)
    if dblk:
        s = s._replace(blk=nominal_blk(s) + dblk)
    return s


def spacing_of(signal, mode):
    """dllCorrelatorSpacing of the states: the reference's defaults for B2a (0.5 chip) and for wide-band B1C (0.06), a quarter chip in
    narrow-band mode.  Wide-band mode cannot take more than 1 / 12 chip: the early / late BOC(6,1) indices ceil(tcode * 6) + 1 then
    leave the one padding element on either side of [p(end) p p(1)] (WB_tracking.m:192,298,324) and MATLAB itself stops with an
    index error (oracle.cfast.trk_epoch raises the same)."""
    return 0.5 if signal == "B2A" else (0.06 if mode == "WB" else 0.25)


def nominal_code_freq(signal):
    return 10.23e6 if signal == "B2A" else 1.023e6


def step_of(st):
    return (st.code_freq or nominal_code_freq(st.signal)) / st.fs  # codePhaseStep, tracking.m:230


def nominal_blk(st):
    return int(np.ceil((CODE_LEN - st.rem) / step_of(st)))  # tracking.m:233


def blk_of(st):
    return st.blk if st.blk is not None else nominal_blk(st)


# Launch shape of the correlators (csrc/bds_track.hip): the run-based kernel gives a lane SEG consecutive samples, a wave 64 SEG per
# pass, a workgroup chunk = 256 SEG (SEG 16 / chunk 4096 for B1C, 8 / 2048 for B2a; BDS_TRK_SEG switches either to the other).  The
# junction of the two halves of the colon vector is k = h, h + 1 with h = floor((blk - 1) / 2).  The block lengths below put it at the
# first (h = m U) and at the last (h = m U - 1: k = h + 1 opens the next unit) sample of a chunk (U = 4096: also a pass and a segment,
# for both SEG), of a pass only (U = 1024, not 4096) and of a segment only (U = 16, not 1024), with n = blk - 1 even (the mid-point
# element exists) and odd.  Most block lengths give NO differing sample (whether the two forms part depends on the right-hand end
# point, i.e. on blk): these are, per case, the longest block below the nominal one that does (a CPU scan over m).
_JUNCTION_BLK = {
    "b1c-wb-30.69": dict(chunk_first_even=303105, chunk_first_odd=286722, chunk_last_even=294911, chunk_last_odd=294912,
                         pass_first_even=305153, pass_first_odd=301058, pass_last_even=299007, pass_last_odd=305152,
                         seg_first_even=306881, seg_first_odd=306882, seg_last_even=306847, seg_last_odd=306848),
    "b2a-102.3": dict(chunk_first_even=98305, chunk_first_odd=90114, chunk_last_even=98303, chunk_last_odd=98304,
                      pass_first_even=100353, pass_first_odd=100354, pass_last_even=92159, pass_last_odd=94208,
                      seg_first_even=102273, seg_first_odd=102274, seg_last_even=102239, seg_last_odd=102240),
}
_JUNCTION_UNIT = dict(chunk=(4096, None), seg=(16, 1024))
_JUNCTION_UNIT["pass"] = (1024, 4096)


def junction_place(st):
    """(what, edge, parity) a junction state's name claims, and whether its block length delivers it"""
    what, edge, parity = st.name.split("-h-")[1].split("-")
    n = blk_of(st) - 1
    h = n // 2
    unit, excl = _JUNCTION_UNIT[what]
    at = h if edge == "first" else h + 1
    ok = at % unit == 0 and (excl is None or at % excl != 0) and (n % 2 == 0) == (parity == "even")
    return what, edge, parity, ok


def _junction(base, tag):
    return [base._replace(name=f"{tag}-h-{key.replace('_', '-')}", blk=blk) for key, blk in _JUNCTION_BLK[tag].items()]


_B1C_3069 = _st("b1c-wb-30.69-start", "B1C", "WB", 30.69e6, 7.5e6)
_B2A_1023 = _st("b2a-102.3-start", "B2A", "B2A", 102.3e6, 13.55e6)

STATES = [
    # ---- the natural start state (rem = 0, nominal code rate) at rates where every 30th / 60th / 10th sample sits on a boundary
    _B1C_3069,
    _st("b1c-nb-30.69-start", "B1C", "NB", 30.69e6, 7.5e6),  # NB reads the code rows only: the prompt replica differs
    _st("b1c-wb-30.69-start-iq", "B1C", "WB", 30.69e6, 7.5e6, iq=True),
    _st("b1c-wb-30.69-rem0.1", "B1C", "WB", 30.69e6, 7.5e6, rem=0.1),
    _st("b1c-wb-61.38-start", "B1C", "WB", 61.38e6, 14.58e6),  # code rows equal, BOC(6,1) rows differ
    _st("b1c-wb-61.38-blk-1", "B1C", "WB", 61.38e6, 14.58e6, dblk=-1),  # E, P and L code rows differ
    _st("b1c-nb-61.38-blk-1-iq", "B1C", "NB", 61.38e6, 14.58e6, iq=True, dblk=-1),
    # wide-band with the early / late replicas on the lattice too (a spacing of one sample step): all six index rows differ
    _st("b1c-wb-30.69-start-spc1/30", "B1C", "WB", 30.69e6, 7.5e6, spacing=1.0 / 30.0),
    _st("b1c-wb-61.38-blk-1-spc1/60-iq", "B1C", "WB", 61.38e6, 14.58e6, iq=True, dblk=-1, spacing=1.0 / 60.0),
    _st("b1c-wb-92.07-rem0.1", "B1C", "WB", 92.07e6, 14.58e6, rem=0.1),
    _B2A_1023,
    _st("b2a-102.3-start-iq", "B2A", "B2A", 102.3e6, 13.55e6, iq=True),
    _st("b2a-102.3-blk-1", "B2A", "B2A", 102.3e6, 13.55e6, dblk=-1),
    _st("b2a-102.3-rem0.3", "B2A", "B2A", 102.3e6, 13.55e6, rem=0.3),
    _st("b2a-61.38-rem1/3", "B2A", "B2A", 61.38e6, 13.55e6, rem=1.0 / 3.0),
    # ---- full rate of BASELINE.json (code-table slices staged in LDS): a code rate 2.9 % low makes step = 1 / 10
    _st("b2a-99.375-fs/10", "B2A", "B2A", 99.375e6, 13.55e6, code_freq=99.375e6 / 10),
    _st("b2a-99.375-fs/10-iq-blk-1", "B2A", "B2A", 99.375e6, 13.55e6, iq=True, code_freq=99.375e6 / 10, dblk=-1),
    # B1C at that rate: a seeded CPU search over 757 rational steps p / q (q <= 2000, within 3 % of nominal) x 4 code phases j step
    # (2 262 states) found 803 with >= 100 differing samples; three of them -- 0.9 % low, 1.2 % high, and 312 Hz (3e-4) above nominal
    _st("b1c-wb-99.375-fs/98", "B1C", "WB", 99.375e6, 14.58e6, code_freq=99.375e6 / 98),
    _st("b1c-nb-99.375-fs/98-iq", "B1C", "NB", 99.375e6, 14.58e6, iq=True, code_freq=99.375e6 / 98),
    _st("b1c-wb-99.375-fs/96-rem38/96", "B1C", "WB", 99.375e6, 14.58e6, code_freq=99.375e6 / 96, rem=38 * ((99.375e6 / 96) / 99.375e6)),
    _st("b1c-wb-99.375-9fs/874", "B1C", "WB", 99.375e6, 14.58e6, code_freq=99.375e6 * 9 / 874),
    # ---- a short block that ends inside a segment
    _B1C_3069._replace(name="b1c-wb-30.69-short", blk=100003),
    _B2A_1023._replace(name="b2a-102.3-short", blk=30012),
    # ---- an extra case below the 100-sample line
    _st("b2a-12.0-start", "B2A", "B2A", 12.0e6, 3.0e6, counted=False),
] + _junction(_B1C_3069, "b1c-wb-30.69") + _junction(_B2A_1023, "b2a-102.3")

# states of the same rates with a code phase off the lattice: 0 differing samples (the CPU guard asserts it).  The GPU module measures
# nothing on them; they document what the looser carrier modes' bounds were measured on (tests/test_track_colon_gpu.py docstring) and
# show that the guard's first condition tells the two kinds of state apart.
QUIET = [
    _st("b1c-wb-30.69-rem0.3", "B1C", "WB", 30.69e6, 7.5e6, rem=0.3),
    _st("b1c-nb-61.38-rem0.3-iq", "B1C", "NB", 61.38e6, 14.58e6, iq=True, rem=0.3),
    _st("b1c-wb-92.07-rem0.2345", "B1C", "WB", 92.07e6, 14.58e6, rem=0.2345),
    _st("b1c-wb-99.375-fs/98-rem0.3", "B1C", "WB", 99.375e6, 14.58e6, code_freq=99.375e6 / 98, rem=0.3),
    _st("b2a-102.3-rem0.2345", "B2A", "B2A", 102.3e6, 13.55e6, rem=0.2345),
    _st("b2a-61.38-rem0.2345-iq", "B2A", "B2A", 61.38e6, 13.55e6, iq=True, rem=0.2345),
    _st("b2a-99.375-fs/10-rem0.2345", "B2A", "B2A", 99.375e6, 13.55e6, code_freq=99.375e6 / 10, rem=0.2345),
    _st("b2a-12.0-rem0.2345", "B2A", "B2A", 12.0e6, 3.0e6, rem=0.2345),
]


def settings_of(st, n_ch=2):
    kw = dict(samplingFreq=st.fs, IF=st.IF, numberOfChannels=n_ch, fileType=2 if st.iq else 1, dllCorrelatorSpacing=st.spacing)
    if st.signal == "B2A":
        return bds_amd.init_settings_b2a(msToProcess=1, pilotTRKflag=1, **kw)
    return bds_amd.init_settings_b1c(msToProcess=10, pilotTRKflag=2 if st.mode == "WB" else 1, **kw)


def oracle_codegen(sig, kind, prn):
    """synth.make_if's code source from the oracle (the default one needs the built HIP library)"""
    if str(sig).upper() == "B1C":
        return ocodes.b1c_primary(int(prn), kind)
    return ocodes._b2a_code_cached(int(prn), kind, CODE_LEN)


Chan = namedtuple("Chan", "prn pos rem_carr")
_SATS = {"B1C": ((3, 1234, 1.0, 48.0), (12, 5003, 2.0, 46.0)), "B2A": ((9, 1234, 2.0, 50.0), (19, 5003, 0.4, 47.0))}


@functools.lru_cache(maxsize=8)
def _record(signal, fs, IF, iq, rem, code_freq, n):
    st = State("", signal, "", fs, IF, iq, 0.0, rem, code_freq, None, True)
    s = settings_of(st)
    fcode = code_freq or nominal_code_freq(signal)
    s_rec = s.copy(codeFreqBasis=fcode)  # the record's code runs at the state's rate, zero Doppler
    sats, chans = [], []
    for prn, pos, phase, cn0 in _SATS[signal]:
        # code phase = rem chips at sample pos; carrier phase of sample pos as remCarrPhase, so the prompt power sits where the loops expect it
        sats.append(synth.Sat(prn, 0.0, pos - rem * fs / fcode, phase, cn0))
        chans.append(Chan(prn, pos, float(np.fmod(2 * np.pi * np.fmod(IF * pos / fs, 1.0) + phase, 2 * np.pi))))
    x = synth.make_if(s_rec, sats, n, seed=1907, codegen=oracle_codegen, iq_sign=(0 if not iq else (-1 if signal == "B2A" else 1)))
    x.setflags(write=False)
    return x, tuple(chans)


def record_of(st):
    """(int8 record, channels): two satellites at 46-50 dB-Hz, zero Doppler, whose code phase at their start sample is the state's"""
    longest = max(blk_of(st), nominal_blk(st))
    n = 5003 + 4096 * (-(-longest // 4096)) + 4096  # one record per family: every block length of the table fits
    return _record(st.signal, st.fs, st.IF, st.iq, st.rem, st.code_freq, n)


def state6_of(st, chans):
    cf = st.code_freq or nominal_code_freq(st.signal)
    return [[c.pos, blk_of(st), st.rem, cf, c.rem_carr, st.IF] for c in chans]


def n_sums(st):
    return 18 if st.mode == "WB" else 12  # the sums the mode reports: data + pilot (+ pilot BOC(6,1))


def _trk_lib():
    cfast.build()
    L = cfast.lib()
    L.bds_oracle_trk_colon_diff.argtypes = [ctypes.c_long] + [ctypes.c_double] * 4 + [ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_double)]
    L.bds_oracle_trk_colon_diff.restype = ctypes.c_int
    L.bds_oracle_trk_set_plain_colon.argtypes = [ctypes.c_int]
    return L


def colon_counts(st):
    """samples whose index differs between the colon vector and a + k d: [E, P, L code, E, P, L BOC(6,1)] (C oracle)"""
    counts = (ctypes.c_long * 6)()
    mu = ctypes.c_double()
    rc = _trk_lib().bds_oracle_trk_colon_diff(blk_of(st), st.rem, step_of(st), st.spacing, 1.0 if st.signal == "B2A" else 2.0, counts, ctypes.byref(mu))
    assert rc == 0, rc
    return [int(c) for c in counts]


def counts_read(st):
    """the entries of colon_counts() the state's mode reads: code rows, and the BOC(6,1) rows in wide-band mode"""
    c = colon_counts(st)
    return c if st.mode == "WB" else c[:3]


@functools.lru_cache(maxsize=None)
def _codes_of(signal, mode, prn):
    s = settings_of(State("", signal, mode, 1.0, 0.0, False, 0.0, 0.0, None, None, True))
    ext = lambda c: np.ascontiguousarray(np.concatenate([[c[-1]], c, [c[0]]]), dtype=np.float64)  # noqa: E731  [c(end) c c(1)], tracking.m:158
    if signal == "B2A":
        return ext(ocodes.generate_b2a_data_code(prn, s)), ext(ocodes.generate_b2a_pilot_code(prn, s)), None
    p6 = ext(ocodes.generate_pilot_boc61(s, prn)) if mode == "WB" else None
    return ext(ocodes.generate_data_boc11(s, prn)), ext(ocodes.generate_pilot_boc11(s, prn)), p6


def oracle_sums(st, x, chans, plain=False):
    """[n_ch][18] correlator sums of the C oracle on the state (colon form; plain=True: a + k d throughout, the form a kernel that
    ignores MATLAB's colon semantics computes)"""
    L = _trk_lib()
    adapt = 2 if st.iq else 1
    blk = blk_of(st)
    b2a = st.signal == "B2A"
    out = []
    L.bds_oracle_trk_set_plain_colon(1 if plain else 0)
    try:
        for c in chans:
            d, p, p6 = _codes_of(st.signal, st.mode, c.prn)
            raw = x[adapt * c.pos: adapt * (c.pos + blk)]
            assert raw.size == adapt * blk
            sums, _, _ = cfast.trk_epoch(raw, blk, st.iq, st.rem, step_of(st), st.spacing, 1.0 if b2a else 2.0, c.rem_carr, st.IF, st.fs, b2a, d, p, p6)
            out.append(sums)
    finally:
        L.bds_oracle_trk_set_plain_colon(0)
    return np.array(out)
