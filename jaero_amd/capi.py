"""ctypes binding of libjaero_hip.so (the C ABI declared in include/jaero_hip.h).

The shared library is built in-tree by `__graft_entry__.build()` / `make -C jaero_amd/csrc`.  There is no CPU or
PyTorch fallback: importing this module without the library raises, and every call fails loudly when the HIP
extension cannot run (no device, wrong architecture).
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("JAERO_HIP_LIB") or os.path.join(HERE, "libjaero_hip.so")  # override: A/B builds of the same ABI

KIND_MSK, KIND_OQPSK, KIND_BURST_MSK, KIND_BURST_OQPSK = 0, 1, 2, 3
FLAG_EBNO, FLAG_STATUS_LOG, FLAG_CAPTURE_SYMBOLS, FLAG_TRACE = 1, 2, 4, 8
EV_SIGNAL, EV_EBNO, EV_FREQ, EV_PEAK, EV_TRIDENT = 0, 1, 2, 3, 4
PCM_CHANNEL_MAJOR, PCM_FRAME_MAJOR = 0, 1
W_RATE = 1  # jaero_ingest_push: sample rate differs from the bank (warning, data queued)
IQ_CS16, IQ_CU8, IQ_CS8, IQ_CF32 = 0, 1, 2, 3
ACT_PEAK, ACT_BLOCKS, ACT_BINS = 1, 2, 64  # jaero_activity_enable: what; bins of a channel's histogram
RATE_L, RATE_BINS = 4096, 2049  # jaero_rate: segment length, bins of a channel's row
GATE_MANUAL, GATE_AUTO, GATE_HIST, GATE_HBINS = 1, 2, 4, 321  # jaero_gate2_enable: mode; bins of a channel's histogram of E
AEROL_SUS, AEROL_PACKETS, AEROL_EVENTS, AEROL_VOICE, AEROL_MESSAGES = 0, 1, 2, 3, 4  # jaero_aerol_read_all: what
AEROL_OVF_SUS, AEROL_OVF_EVENTS, AEROL_OVF_VOICE, AEROL_OVF_MESSAGES = 1, 2, 4, 8  # a channel's overflow bits, one per output class
MSG_AES0, MSG_ACARS, MSG_TEXT, MSG_MORE, MSG_PARITY = 1, 2, 4, 8, 16  # jaero_aerol_msg.flags
BANK_SOFTBITS, BANK_STATUS_LOG, BANK_EVENTS, BANK_SYMBOLS = 0, 1, 2, 3  # jaero_read_all: what
E_OK, E_INVAL, E_NODEV, E_NOMEM, E_HIP, E_OVERFLOW, E_NOTSUP = 0, -1, -2, -3, -4, -5, -6

EXPORTS = [
    "jaero_create", "jaero_destroy", "jaero_set_settings", "jaero_set_flags", "jaero_set_dcd",
    "jaero_center_freq_changed", "jaero_write", "jaero_read_softbits", "jaero_read_softbits_all",
    "jaero_softbits_view", "jaero_discard_softbits", "jaero_read_status", "jaero_read_status_log",
    "jaero_read_symbols", "jaero_viterbi_decode_soft", "jaero_viterbi_continuous", "jaero_abi_version",
    "jaero_num_channels", "jaero_strerror", "jaero_last_error", "jaero_profile_enable", "jaero_profile_read", "jaero_profile_kernel", "jaero_debug_viterbi_layout", "jaero_debug_viterbi",
    "jaero_debug_sample_loop_layout", "jaero_debug_kernel_variant",
    "jaero_debug_coarse_poke", "jaero_debug_coarse_launch", "jaero_debug_coarse_peek",
    "jaero_debug_coarse_band", "jaero_debug_coarse_force_generic", "jaero_debug_coarse_band_class",
    "jaero_debug_loop_poke", "jaero_debug_loop_peek",
    "jaero_debug_schedule", "jaero_debug_schedule_lanes", "jaero_debug_prefilter", "jaero_debug_read_prefiltered", "jaero_read_events",
    "jaero_debug_burst_geom", "jaero_debug_burst_hilbert", "jaero_debug_burst_read_hist", "jaero_debug_burst_poke_cv", "jaero_debug_burst_trident",
    "jaero_debug_burst_front_geom", "jaero_debug_burst_front", "jaero_debug_burst_front_peek", "jaero_debug_burst_front_events", "jaero_debug_burst_front_poke", "jaero_debug_burst_poke_bt",
    "jaero_debug_ev_compact",
    "jaero_debug_burst_track_geom", "jaero_debug_burst_track", "jaero_debug_burst_track_peek", "jaero_debug_burst_track_fill", "jaero_debug_burst_track_read",
    "jaero_debug_burst_track_center_freq",
    "jaero_debug_pre8400_write", "jaero_debug_pre8400_poke", "jaero_debug_pre8400_peek", "jaero_debug_pre8400_restart", "jaero_debug_pre8400_read_ring",
    "jaero_aerol_create", "jaero_aerol_create_burst", "jaero_aerol_read_packets", "jaero_aerol_destroy", "jaero_aerol_write", "jaero_aerol_read_sus", "jaero_aerol_read_events",
    "jaero_aerol_tick_dcd", "jaero_aerol_profile_enable", "jaero_aerol_profile_read", "jaero_aerol_read_voice",
    "jaero_aerol_link_dcd", "jaero_aerol_read_all", "jaero_aerol_profile2_read", "jaero_aerol_debug_extra_bytes",
    "jaero_aerol_isu_enable", "jaero_aerol_read_msgs", "jaero_aerol_isu_stats", "jaero_aerol_rt_enable", "jaero_aerol_rt_stats",
    "jaero_read_all", "jaero_read_status_all", "jaero_profile2_read", "jaero_debug_read_all_bytes", "jaero_debug_softbit_counts",
    "jaero_ingest_create", "jaero_ingest_destroy", "jaero_ingest_push", "jaero_ingest_queued", "jaero_ingest_pump",
    "jaero_ingest_stats",
    "jaero_chan_create", "jaero_chan_destroy", "jaero_chan_write", "jaero_chan_pcm_view", "jaero_chan_read_pcm", "jaero_chan_retune",
    "jaero_chan_feed", "jaero_chan_profile_enable", "jaero_chan_profile_read", "jaero_chan2_create",
    "jaero_survey_enable", "jaero_survey_reset", "jaero_survey_read_psd", "jaero_survey_read_levels", "jaero_survey_profile_read",
    "jaero_chan2_retune_all",
    "jaero_activity_enable", "jaero_activity_reset", "jaero_activity_read_peak", "jaero_activity_read_blocks", "jaero_activity_profile_read",
    "jaero_chan3_create", "jaero_chan3_write", "jaero_chan3_feed", "jaero_chan3_read_staged", "jaero_chan3_profile_read",
    "jaero_split_create", "jaero_split_destroy", "jaero_split_write", "jaero_split_feed", "jaero_split_output", "jaero_split_info",
    "jaero_split_profile_enable", "jaero_split_profile_read",
    "jaero_rate_create", "jaero_rate_destroy", "jaero_rate_write", "jaero_rate_reset", "jaero_rate_read", "jaero_rate_profile_enable",
    "jaero_rate_profile_read",
    "jaero_gate_enable", "jaero_gate_set", "jaero_gate_read",
    "jaero_gate2_enable", "jaero_gate2_read", "jaero_gate2_read_hist",
    "jaero_lines_classify", "jaero_debug_rate_poke",
    "jaero_shard_range", "jaero_comm_get_unique_id", "jaero_comm_create", "jaero_comm_destroy", "jaero_fan_out_pcm", "jaero_gather_softbits",
]


class Settings(C.Structure):
    """struct jaero_settings == OqpskDemodulator::Settings / MskDemodulator::Settings."""

    _fields_ = [
        ("kind", C.c_int),
        ("coarsefreqest_fft_power", C.c_int),
        ("freq_center", C.c_double),
        ("lockingbw", C.c_double),
        ("fb", C.c_double),
        ("Fs", C.c_double),
        ("signalthreshold", C.c_double),
    ]


class Status(C.Structure):
    _fields_ = [
        ("mse", C.c_double),
        ("ebno", C.c_double),
        ("freq_est", C.c_double),
        ("freq_center", C.c_double),
        ("signal", C.c_int),
        ("n_estimates", C.c_int),
    ]


class CoarseState(C.Structure):
    """struct jaero_coarse_state: what jaero_debug_coarse_poke / _peek exchange besides a channel's ring and y."""

    _fields_ = [(n, C.c_int) for n in ("bb_ptr", "emptying", "flags", "countdown", "countdown2", "coarse_cnt", "nest", "log_cnt")] + [
        (n, C.c_double) for n in ("mse", "m2_freq", "mc_freq")]


class LoopState(C.Structure):
    """struct jaero_loop_state: what jaero_debug_loop_poke / _peek exchange."""

    _fields_ = [(n, C.c_double) for n in ("st_freq", "m2_freq", "lf_x1", "lf_x2", "lf_y1", "lf_y2")]


class Pre8400State(C.Structure):
    """struct jaero_pre8400_state: what jaero_debug_pre8400_poke / _peek exchange (n0, nprev, ring, cap: outputs of peek only)."""

    _fields_ = [("ptr", C.c_double), ("step", C.c_double), ("fsum", C.c_double), ("hold", C.c_longlong), ("n0", C.c_longlong),
                ("nprev", C.c_int), ("ring", C.c_int), ("cap", C.c_int)]


class BurstGeom(C.Structure):
    """struct jaero_burst_geom: what jaero_debug_burst_geom reports."""

    _fields_ = [(n, C.c_int) for n in ("kind", "nch", "nchp", "maxseg", "hist_len", "hil_lat", "cv_len", "D1", "tri_sz", "nb", "nt", "tri_grid")] + [
        ("nsamples", C.c_longlong)]


class TridentResult(C.Structure):
    """struct jaero_trident_result: one channel's result of jaero_debug_burst_trident."""

    _fields_ = [("ok", C.c_int), ("pad", C.c_int), ("freq", C.c_double), ("phase_deg", C.c_double), ("vol_gain", C.c_double), ("metric", C.c_double)]


class BurstFrontGeom(C.Structure):
    """struct jaero_burst_front_geom: what jaero_debug_burst_front_geom reports."""

    _fields_ = [(n, C.c_int) for n in ("PL", "bt_len", "bt_lag", "agc_len", "ma1_len", "mav1_len", "fa_len", "fa_lag", "ev_cap", "ngroups")] + [
        (n, C.c_double) for n in ("pd_thr", "bt_w", "fa_w")]


class BurstFrontState(C.Structure):
    """struct jaero_burst_front_state: the detector's scalars of one channel (jaero_debug_burst_front_peek)."""

    _fields_ = [(n, C.c_double) for n in ("agc_sum", "ma1_re", "ma1_im", "mav1_sum", "lastdy")] + [
        (n, C.c_int) for n in ("cntdown", "maxposcd", "tri_ptr", "ev_pos", "ev_cnt", "bt_hold")]


class BurstTrackGeom(C.Structure):
    """struct jaero_burst_track_geom: what jaero_debug_burst_track_geom reports."""

    _fields_ = [(n, C.c_int) for n in ("D2", "soft_cap", "sym_cap", "ev_cap", "msema_len", "win_ring", "agc2_len", "eb_len", "startstopstart", "firn", "ldsn",
                                       "ebno_tail")]


class BurstTrackState(C.Structure):
    """struct jaero_burst_track_state: the tracking chain's scalars of one channel (jaero_debug_burst_track_peek)."""

    INTS = ("startstop", "cntr", "yui", "insertpre", "nrx", "soft_cnt", "sym_cnt", "ev_cnt", "overflow", "msema_pos", "fir_pos", "eb_pos", "dly_pos", "d8_pos",
            "a1_pos", "gcnt")
    DBLS = ("mse", "lastmse", "m2_freq", "st_freq", "vol_gain", "eb_ebno", "rot_freq", "agc2_sum", "eb_esum", "eb_e2sum", "msema_sum", "mc_freq", "diff_last",
            "m2_ptr", "st_ptr", "stq_ptr")
    _fields_ = [(n, C.c_int) for n in INTS] + [(n, C.c_double) for n in DBLS]


class ViterbiProbe(C.Structure):
    """struct jaero_viterbi_probe: one launch of the Viterbi decoder as jaero_debug_viterbi takes it."""

    _fields_ = [("soft", C.c_void_p)] + [(n, C.c_int) for n in ("nblocks", "nsoft", "pitch", "tiled", "soft_misalign", "pad")] + [
        ("overlap", C.c_void_p), ("out", C.c_void_p)] + [
        (n, C.c_int) for n in ("out_rows", "out_stride", "out_start", "out_want", "packed", "layout", "update_overlap")] + [
        ("valid", C.c_void_p), ("lens", C.c_void_p)]


FRONT_RINGS = {"agc_ring": 0, "cvre": 1, "cvim": 2, "ma1re": 3, "ma1im": 4, "mav1": 5, "fa": 6, "bt": 7}  # JAERO_FRONT_RING_*
FRONT_CNTDOWN, FRONT_MAXPOSCD, FRONT_TRI_PTR, FRONT_BT_HOLD, FRONT_LASTDY = 0, 1, 2, 3, 4


class ChanChannel(C.Structure):
    """struct jaero_chan_channel: tuning word (centre = tune * Fs_in / 2^32, signed), audio word (offset = audio * out_rate / 2^32), gain."""

    _fields_ = [("tune", C.c_uint32), ("audio", C.c_uint32), ("gain", C.c_double)]


class Capture(C.Structure):
    """struct jaero_capture: format (IQ_*), capture rate in Hz, centre shift (cycles per input sample x 2^32), taps per phase K and the
    resampler prototype h[0 .. L K) (null when the capture already runs at out_rate x decim)."""

    _fields_ = [("format", C.c_int), ("fs_in", C.c_int), ("shift", C.c_uint32), ("taps_per_phase", C.c_int), ("rtaps", C.c_void_p)]


class ChanOutput(C.Structure):
    """struct jaero_chan_output: one output of a splitter -- its rate, its channels (tune words relative to fs_c, audio words to out_rate)
    and its prototype at fs_c."""

    _fields_ = [("out_rate", C.c_int), ("nchannels", C.c_int), ("ch", C.c_void_p), ("taps", C.c_void_p), ("ntaps", C.c_int)]


class Msg(C.Structure):
    """struct jaero_aerol_msg: one reassembled ISU (jaero_aerol_read_msgs); jaero_amd.acars.MSG_DTYPE is the same row for numpy."""

    _fields_ = [("frame", C.c_int32), ("k", C.c_int32), ("aesid", C.c_uint32), ("gesid", C.c_uint8), ("qno", C.c_uint8), ("refno", C.c_uint8),
                ("nooct", C.c_uint8), ("nbytes", C.c_uint16), ("flags", C.c_uint16), ("mode", C.c_uint8), ("tak", C.c_uint8),
                ("label", C.c_uint8 * 2), ("bi", C.c_uint8), ("pad", C.c_uint8 * 7), ("data", C.c_uint8 * 512)]


class JaeroError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libjaero_hip error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Load libjaero_hip.so; raises if the HIP extension has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C jaero_amd/csrc).  jaero_amd has no CPU fallback."
        )
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7.  Importing torch first makes the
    # dynamic linker resolve libjaero_hip.so's libamdhip64.so.7 dependency to that already-loaded copy, so tensors,
    # streams and this library share one runtime (loading /opt/rocm's copy first leaves torch without a device).
    try:
        import torch  # noqa: F401
    except ImportError:  # pragma: no cover - torch is part of the image
        pass
    L = C.CDLL(LIB_PATH)
    vp, ip, dp = C.c_void_p, C.c_int, C.c_double
    L.jaero_create.argtypes = [ip, ip, vp, ip, C.c_uint, ip, ip, C.POINTER(vp)]
    L.jaero_destroy.argtypes = [vp]
    L.jaero_destroy.restype = None
    L.jaero_set_settings.argtypes = [vp, ip, C.POINTER(Settings)]
    L.jaero_set_flags.argtypes = [vp, ip, ip, ip, ip]
    L.jaero_set_dcd.argtypes = [vp, ip, ip]
    L.jaero_center_freq_changed.argtypes = [vp, ip, dp]
    L.jaero_write.argtypes = [vp, vp, ip, ip, ip, vp]
    L.jaero_read_softbits.argtypes = [vp, ip, vp, ip, C.POINTER(ip)]
    L.jaero_read_softbits_all.argtypes = [vp, vp, ip, vp]
    L.jaero_softbits_view.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(ip)]
    L.jaero_discard_softbits.argtypes = [vp, vp]
    L.jaero_read_status.argtypes = [vp, ip, C.POINTER(Status)]
    L.jaero_read_status_log.argtypes = [vp, ip, vp, ip, C.POINTER(ip)]
    L.jaero_read_symbols.argtypes = [vp, ip, vp, ip, C.POINTER(ip)]
    L.jaero_read_events.argtypes = [vp, ip, vp, ip, C.POINTER(ip)]
    L.jaero_viterbi_decode_soft.argtypes = [ip, vp, ip, ip, vp, ip, vp]
    L.jaero_viterbi_continuous.argtypes = [ip, vp, ip, ip, ip, vp, vp, vp, ip, vp]
    L.jaero_abi_version.restype = ip
    L.jaero_num_channels.argtypes = [vp]
    L.jaero_strerror.argtypes = [ip]
    L.jaero_strerror.restype = C.c_char_p
    L.jaero_last_error.restype = C.c_char_p
    L.jaero_profile_enable.argtypes = [vp, ip]
    L.jaero_profile_read.argtypes = [vp, ip, C.POINTER(dp), C.POINTER(ip), ip]
    L.jaero_profile_kernel.argtypes = [vp, ip, C.c_char_p, ip]
    L.jaero_debug_viterbi_layout.argtypes = [ip]
    L.jaero_debug_viterbi.argtypes = [ip, C.POINTER(ViterbiProbe)]
    L.jaero_debug_sample_loop_layout.argtypes = [ip]
    L.jaero_debug_kernel_variant.argtypes = [vp, ip, C.c_char_p, ip]
    L.jaero_debug_coarse_poke.argtypes = [vp, ip, vp, vp, C.POINTER(CoarseState)]
    L.jaero_debug_coarse_launch.argtypes = [vp, vp, ip, ip]
    L.jaero_debug_coarse_peek.argtypes = [vp, ip, vp, vp, C.POINTER(CoarseState)]
    L.jaero_debug_loop_poke.argtypes = [vp, ip, C.POINTER(LoopState)]
    L.jaero_debug_loop_peek.argtypes = [vp, ip, C.POINTER(LoopState)]
    L.jaero_debug_coarse_band.argtypes = [vp, C.c_char_p, ip, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.jaero_debug_coarse_force_generic.argtypes = [vp, ip]
    L.jaero_debug_coarse_band_class.argtypes = [ip, dp, dp, dp]
    L.jaero_debug_schedule.argtypes = [ip, ip, ip, vp, ip, vp, ip, C.POINTER(ip)]
    L.jaero_debug_schedule_lanes.argtypes = [ip, ip, ip, vp, vp, ip, vp, ip, vp, ip, C.POINTER(ip)]
    L.jaero_debug_prefilter.argtypes = [ip, vp, ip, dp, dp, vp]
    L.jaero_debug_read_prefiltered.argtypes = [vp, ip, vp, ip]
    L.jaero_debug_pre8400_write.argtypes = [vp, vp, ip, ip, ip]
    L.jaero_debug_pre8400_poke.argtypes = [vp, ip, C.POINTER(Pre8400State)]
    L.jaero_debug_pre8400_peek.argtypes = [vp, ip, C.POINTER(Pre8400State)]
    L.jaero_debug_pre8400_restart.argtypes = [vp, ip]
    L.jaero_debug_pre8400_read_ring.argtypes = [vp, ip, C.c_longlong, ip, vp]
    L.jaero_debug_burst_geom.argtypes = [vp, C.POINTER(BurstGeom)]
    L.jaero_debug_burst_hilbert.argtypes = [vp, vp, ip, ip, vp]
    L.jaero_debug_burst_read_hist.argtypes = [vp, ip, C.c_longlong, ip, vp]
    L.jaero_debug_burst_poke_cv.argtypes = [vp, ip, C.c_longlong, ip, vp]
    L.jaero_debug_burst_trident.argtypes = [vp, vp, vp, ip, C.c_longlong, ip, vp, C.POINTER(ip)]
    L.jaero_debug_burst_front_geom.argtypes = [vp, C.POINTER(BurstFrontGeom)]
    L.jaero_debug_burst_front.argtypes = [vp, vp, ip, ip, vp, vp, vp, C.POINTER(ip)]
    L.jaero_debug_burst_front_peek.argtypes = [vp, ip, C.POINTER(BurstFrontState), ip, C.c_longlong, ip, vp]
    L.jaero_debug_burst_front_events.argtypes = [vp, ip, vp, ip, C.POINTER(ip)]
    L.jaero_debug_burst_front_poke.argtypes = [vp, ip, ip, dp]
    L.jaero_debug_burst_poke_bt.argtypes = [vp, ip, C.c_longlong, ip, vp]
    L.jaero_debug_ev_compact.argtypes = [ip, vp, ip, vp, C.POINTER(ip)]
    L.jaero_debug_burst_track_geom.argtypes = [vp, C.POINTER(BurstTrackGeom)]
    L.jaero_debug_burst_track.argtypes = [vp, ip, ip, vp, vp, vp, ip]
    L.jaero_debug_burst_track_peek.argtypes = [vp, ip, C.POINTER(BurstTrackState)]
    L.jaero_debug_burst_track_fill.argtypes = [vp, ip, dp]
    L.jaero_debug_burst_track_read.argtypes = [vp, ip, ip, vp, ip]
    L.jaero_debug_burst_track_center_freq.argtypes = [vp, ip, dp]
    L.jaero_aerol_create.argtypes = [ip, ip, ip, ip, ip, C.POINTER(vp)]
    L.jaero_aerol_create_burst.argtypes = [ip, ip, ip, ip, ip, C.POINTER(vp)]
    L.jaero_aerol_read_packets.argtypes = [vp, ip, vp, ip, C.POINTER(ip)]
    L.jaero_aerol_read_voice.argtypes = [vp, ip, vp, ip, C.POINTER(ip)]
    L.jaero_aerol_destroy.argtypes = [vp]
    L.jaero_aerol_destroy.restype = None
    L.jaero_aerol_write.argtypes = [vp, vp, vp, ip, ip, ip, vp]
    L.jaero_aerol_read_sus.argtypes = [vp, ip, vp, ip, C.POINTER(ip)]
    L.jaero_aerol_read_events.argtypes = [vp, ip, vp, ip, C.POINTER(ip)]
    L.jaero_aerol_tick_dcd.argtypes = [vp, vp]
    L.jaero_aerol_profile_enable.argtypes = [vp, ip]
    L.jaero_aerol_profile_read.argtypes = [vp, ip, C.POINTER(dp), C.POINTER(ip), ip]
    L.jaero_aerol_link_dcd.argtypes = [vp, vp]
    L.jaero_aerol_read_all.argtypes = [vp, ip, vp, ip, vp, C.POINTER(ip), C.POINTER(C.c_longlong), vp]
    L.jaero_aerol_profile2_read.argtypes = [vp, ip, C.POINTER(dp), C.POINTER(ip), ip]
    L.jaero_aerol_debug_extra_bytes.argtypes = [vp]
    L.jaero_aerol_debug_extra_bytes.restype = C.c_longlong
    L.jaero_aerol_isu_enable.argtypes = [vp, ip]
    L.jaero_aerol_read_msgs.argtypes = [vp, ip, vp, ip, C.POINTER(ip)]
    L.jaero_aerol_isu_stats.argtypes = [vp, vp]
    L.jaero_aerol_rt_enable.argtypes = [vp, ip]
    L.jaero_aerol_rt_stats.argtypes = [vp, vp]
    L.jaero_read_all.argtypes = [vp, ip, vp, ip, vp, C.POINTER(ip), C.POINTER(C.c_longlong), vp]
    L.jaero_read_status_all.argtypes = [vp, vp]
    L.jaero_profile2_read.argtypes = [vp, ip, C.POINTER(dp), C.POINTER(ip), ip]
    L.jaero_debug_read_all_bytes.argtypes = [vp]
    L.jaero_debug_read_all_bytes.restype = C.c_longlong
    L.jaero_debug_softbit_counts.argtypes = [vp, vp, vp]
    L.jaero_ingest_create.argtypes = [vp, ip, ip, C.POINTER(vp)]
    L.jaero_ingest_destroy.argtypes = [vp]
    L.jaero_ingest_destroy.restype = None
    L.jaero_ingest_push.argtypes = [vp, ip, vp, ip, C.c_uint]
    L.jaero_ingest_queued.argtypes = [vp, ip]
    L.jaero_ingest_pump.argtypes = [vp, ip, vp, C.POINTER(ip)]
    L.jaero_ingest_stats.argtypes = [vp, vp]
    L.jaero_chan_create.argtypes = [ip, ip, ip, vp, vp, ip, ip, C.POINTER(vp)]
    L.jaero_chan2_create.argtypes = [ip, ip, ip, ip, vp, vp, ip, ip, C.POINTER(vp)]
    L.jaero_chan_destroy.argtypes = [vp]
    L.jaero_chan_destroy.restype = None
    L.jaero_chan_write.argtypes = [vp, vp, ip, ip, vp, C.POINTER(ip)]
    L.jaero_chan_pcm_view.argtypes = [vp, C.POINTER(vp), C.POINTER(ip)]
    L.jaero_chan_read_pcm.argtypes = [vp, vp, ip, C.POINTER(ip)]
    L.jaero_chan_retune.argtypes = [vp, ip, C.POINTER(ChanChannel)]
    L.jaero_chan_feed.argtypes = [vp, vp, vp, ip, ip, vp, C.POINTER(ip)]
    L.jaero_chan_profile_enable.argtypes = [vp, ip]
    L.jaero_chan_profile_read.argtypes = [vp, ip, C.POINTER(dp), C.POINTER(ip), ip]
    L.jaero_survey_enable.argtypes = [vp, ip]
    L.jaero_survey_reset.argtypes = [vp]
    L.jaero_survey_read_psd.argtypes = [vp, vp, C.POINTER(C.c_longlong)]
    L.jaero_survey_read_levels.argtypes = [vp, vp, vp]
    L.jaero_survey_profile_read.argtypes = [vp, ip, C.POINTER(dp), C.POINTER(ip), ip]
    L.jaero_chan2_retune_all.argtypes = [vp, vp]
    L.jaero_activity_enable.argtypes = [vp, ip]
    L.jaero_activity_reset.argtypes = [vp]
    L.jaero_activity_read_peak.argtypes = [vp, vp, C.POINTER(C.c_longlong)]
    L.jaero_activity_read_blocks.argtypes = [vp, vp, vp, vp, vp, vp]
    L.jaero_activity_profile_read.argtypes = [vp, ip, C.POINTER(dp), C.POINTER(ip), ip]
    L.jaero_chan3_create.argtypes = [ip, C.POINTER(Capture), ip, ip, ip, vp, vp, ip, ip, C.POINTER(vp)]
    L.jaero_chan3_write.argtypes = [vp, vp, ip, ip, vp, C.POINTER(ip)]
    L.jaero_chan3_feed.argtypes = [vp, vp, vp, ip, ip, vp, C.POINTER(ip)]
    L.jaero_chan3_read_staged.argtypes = [vp, vp, ip, C.POINTER(ip), C.POINTER(C.c_longlong)]
    L.jaero_chan3_profile_read.argtypes = [vp, ip, C.POINTER(dp), C.POINTER(ip), ip]
    L.jaero_split_create.argtypes = [ip, C.POINTER(Capture), ip, ip, C.POINTER(ChanOutput), ip, C.POINTER(vp)]
    L.jaero_split_destroy.argtypes = [vp]
    L.jaero_split_destroy.restype = None
    L.jaero_split_write.argtypes = [vp, vp, ip, ip, vp, C.POINTER(ip)]
    L.jaero_split_feed.argtypes = [vp, C.POINTER(vp), vp, ip, ip, vp, C.POINTER(ip)]
    L.jaero_split_output.argtypes = [vp, ip, C.POINTER(vp)]
    L.jaero_split_info.argtypes = [vp, C.POINTER(ip), C.POINTER(ip), C.POINTER(ip)]
    L.jaero_split_profile_enable.argtypes = [vp, ip]
    L.jaero_split_profile_read.argtypes = [vp, ip, C.POINTER(dp), C.POINTER(ip), ip]
    L.jaero_rate_create.argtypes = [ip, ip, ip, C.POINTER(vp)]
    L.jaero_rate_destroy.argtypes = [vp]
    L.jaero_rate_destroy.restype = None
    L.jaero_rate_write.argtypes = [vp, vp, ip, ip, vp, C.POINTER(ip)]
    L.jaero_rate_reset.argtypes = [vp]
    L.jaero_rate_read.argtypes = [vp, vp, C.POINTER(C.c_longlong)]
    L.jaero_rate_profile_enable.argtypes = [vp, ip]
    L.jaero_rate_profile_read.argtypes = [vp, ip, C.POINTER(dp), C.POINTER(ip), ip]
    L.jaero_gate_enable.argtypes = [vp, ip]
    L.jaero_gate_set.argtypes = [vp, vp]
    L.jaero_gate_read.argtypes = [vp, vp, vp, C.POINTER(C.c_longlong)]
    L.jaero_gate2_enable.argtypes = [vp, ip]
    L.jaero_gate2_read.argtypes = [vp, vp, vp, C.POINTER(C.c_longlong)]
    L.jaero_gate2_read_hist.argtypes = [vp, vp, C.POINTER(C.c_longlong)]
    L.jaero_lines_classify.argtypes = [vp, ip, ip, vp, vp, vp, vp, C.POINTER(C.c_longlong), C.POINTER(dp)]
    L.jaero_debug_rate_poke.argtypes = [vp, vp, C.c_longlong]
    L.jaero_shard_range.argtypes =[ip, ip, ip, C.POINTER(ip), C.POINTER(ip)]
    L.jaero_comm_get_unique_id.argtypes = [vp]
    L.jaero_comm_create.argtypes = [ip, ip, ip, vp, C.POINTER(vp)]
    L.jaero_comm_destroy.argtypes = [vp]
    L.jaero_comm_destroy.restype = None
    L.jaero_fan_out_pcm.argtypes = [vp, ip, vp, ip, ip, vp, vp]
    L.jaero_gather_softbits.argtypes = [vp, ip, vp, vp, ip, ip, vp, vp, vp]
    for name in EXPORTS:
        getattr(L, name)  # raises AttributeError if a declared symbol is not exported
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != 0:
        L = lib()
        msg = L.jaero_last_error().decode() or L.jaero_strerror(rc).decode()
        raise JaeroError(rc, msg)
