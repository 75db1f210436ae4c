"""The device primitives of jaero_amd/csrc/jd_libm.h and jaero_device.h and how tests/test_gpu_device_math.py reaches them.

LAUNCHERS maps every extern "C" launcher of jaero_amd/libjaero_prims.so (jaero_amd/csrc/prims_check.hip) to the device function it runs;
NOT_LAUNCHED lists the jd_* / fb_* / bd_* functions of the two headers that have no launcher of their own, each with the reason.
tests/test_device_math_table.py checks both against the headers and the library; the GPU module runs every launcher.
"""
import ctypes as C
import os
import subprocess
from dataclasses import dataclass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jaero_amd", "csrc")
PRIMS_LIB = os.environ.get("JAERO_PRIMS_LIB") or os.path.join(ROOT, "jaero_amd", "libjaero_prims.so")  # override: a variant build of the same launchers
HEADERS = ("jd_libm.h", "jaero_device.h")

LAUNCHERS = {
    "jp_atan2": "jd_atan2",
    "jp_hypot": "jd_hypot",
    "jp_div": "jd_div",
    "jp_div_const": "jd_div_const",
    "jp_tanh": "jd_tanh",
    "jp_tanh_full": "jd_tanh_full",
    "jp_expm1": "jd_expm1",
    "jp_log10": "jd_log10",
    "jp_qround": "jd_qround",
    "jp_softbit": "jd_softbit",
    "jp_cisidx": "jd_cisidx",
    "jp_wt_next": "jd_wt_next",
    "jp_wt_setfreq": "jd_wt_setfreq",
    "jp_wt_inc_phase_deg": "jd_wt_inc_phase_deg",
    "jp_wt_advance_fraction": "jd_wt_advance_fraction",
    "jp_wt_passed": "jd_wt_passed",
    "jp_fb_wt_setfreq": "fb_wt_setfreq",
    "jp_fb_wt_next": "fb_wt_next",
    "jp_fb_fmod360": "fb_fmod360",
    "jp_bd_set_phase_deg": "bd_set_phase_deg",
    "jp_biquad": "jd_biquad",
    "jp_diff_soft": "jd_diff_soft",
    "jp_wt_next_symbol": "jd_wt_next_symbol",
}


@dataclass(frozen=True)
class FirRow:
    export: str
    func: str
    firn: int
    ldsn: int
    d: int
    fused: bool
    site: str  # the call site this instantiation stands for (file:line under jaero_amd/csrc)
    t0: int = 0  # block rows: the sum continues behind tap t0 - 1 from per-lane start sums ...
    bs: int = 0  # ... and reads the ring by blocks of bs slots (jd_fir_sum_blocks); 0: the ring walked or the 55-tap symmetric forms


# every matched-filter instantiation of jaero_device.h a kernel launches, plus the fused sum over the walked ring, which jd_fir_sum offers
FIR_ROWS = [
    FirRow("jp_fir_eval_40_24_8", "jd_fir_eval", 40, 24, 8, False, "k_msk.h:80"),  # MSK_LDSN_40: 1200 bps at 24 kHz, 600 bps at 12 kHz
    FirRow("jp_fir_eval_20_12_8", "jd_fir_eval", 20, 12, 8, False, "k_msk.h:80"),  # MSK_LDSN_20: 1200 bps at 12 kHz
    # jd_fir_sum<55, 36, 8, true, 0> over JdRingWalk: no kernel launches it (jd_fir_eval no longer fuses; the burst demodulator reads by blocks,
    # last row); the one combination of jd_fir_sum's two compile-time choices that has no call site, kept under its export's earlier name
    FirRow("jp_fir_eval_fused_55_36_8", "jd_fir_sum", 55, 36, 8, True, ""),
    FirRow("jp_fir_eval_sym_55_36_6", "jd_fir_eval_sym", 55, 36, 6, False, "k_oqpsk_fb.h:204"),  # FB_LDSN
    FirRow("jp_fir_eval_sym_static_55_36_6", "jd_fir_eval_sym_static", 55, 36, 6, False, "k_oqpsk_fb.h:266"),
    FirRow("jp_fir_eval_sym_static_but_last_55_36_6", "jd_fir_eval_sym_static_but_last", 55, 36, 6, False, "k_oqpsk_fb.h:236"),  # D = FB_SOLO_D
    # k_msk_fb's front half (TB > 0: all twelve instantiations), T0 = the back half's share of the tail, BS = mfb_bs<LDSN>()
    FirRow("jp_fir_sum_blocks_80_36_8_t32_b4", "jd_fir_sum_blocks", 80, 36, 8, False, "k_msk_fb.h:149", 32, 4),  # MFB_LDSN, MFB1_TB
    FirRow("jp_fir_sum_blocks_80_32_8_t18_b4", "jd_fir_sum_blocks", 80, 32, 8, False, "k_msk_fb.h:149", 18, 4),  # MFB4_LDSN, MFB4_TB
    FirRow("jp_fir_sum_blocks_160_72_8_t64_b4", "jd_fir_sum_blocks", 160, 72, 8, False, "k_msk_fb.h:149", 64, 4),  # MFB2_LDSN, MFB2_TB
    # k_burst_oqpsk_demod forms its block addresses itself and calls jd_fir_sum over JdRingBlocks<BD_LDSN, BD_BS, ..>: the same sums, from zero
    FirRow("jp_fir_sum_blocks_fused_55_36_8_t0_b6", "jd_fir_sum", 55, 36, 8, True, "k_burst_demod.h:199", 0, 6),  # BD_LDSN, BD_BS, BD_FUSED
]

NOT_LAUNCHED = {
    "jd_sload": "a scalar load through the constant address space, no arithmetic",
    "jd_with_hi": "replaces a high word; every use is inside jd_expm1 / jd_tanh, which are checked bit for bit",
    "jd_atan_lane_table": "built at entry of jp_atan2's kernel exactly as the sample kernels build it",
    "jd_atan2_t": "the template behind jd_atan2 (its only instantiation)",
    "jd_lds_barrier": "s_waitcnt lgkmcnt(0) + s_barrier, no arithmetic; every front / back pair and workgroup FFT the kernel tests run goes through it",
    "jd_vzero": "a v_mov of zero, no arithmetic; the tap offset of every jd_fir_sum_blocks row",
    "jd_fir_sym_tail": "the register-tail part of the three jd_fir_eval_sym* forms, checked through them",
    "jd_fir_eval_sym_static_t": "the template behind jd_fir_eval_sym_static and _but_last (its only instantiations)",
    "jd_fir_lds_part": "the ring part of jd_fir_eval_sym_static and _but_last, checked through them at every ring position",
}


@dataclass(frozen=True)
class DivConst:
    d: float
    what: str
    site: str  # file:line under jaero_amd/csrc where the divisor (or its reciprocal) is computed
    token: str  # text of that line


# every (d, rd = 1.0 / d) that reaches jd_div_const: k_oqpsk_fb (continuous OQPSK, 10 500 and 8400 bps, Fs = 48 000 only: jaero_hip.hip:380-384),
# k_burst_demod (burst OQPSK, 10 500 bps at 48 000 only) and bd_set_phase_deg (both burst kinds)
DIV_CONSTS = [
    DivConst(192000.0, "OQPSK agc_len = round(4 Fs), k_oqpsk_fb.h:122", "jaero_hip.hip:431", "g.agc_len = (int)round(4 * s.Fs)"),
    DivConst(96000.0, "OQPSK ebno_len = 2 Fs, k_oqpsk_fb.h:122", "jaero_hip.hip:426", "g.ebno_len = (int)(2 * s.Fs)"),
    DivConst(800.0, "OQPSK marg_len, k_oqpsk_fb.h:322", "jaero_hip.hip:432", "g.marg_len = 800"),
    DivConst(400.0, "OQPSK pm_len and msema_len, k_oqpsk_fb.h:322", "jaero_hip.hip:432", "g.pm_len = 400; g.msema_len = 400"),
    DivConst(48000.0, "samplerate = Fs (also k_burst_demod.h:131)", "k_oqpsk_fb.h:319", "r_samplerate = 1.0 / samplerate"),
    DivConst(360.0, "degrees (also k_burst_demod.h:131)", "k_oqpsk_fb.h:320", "r_360 = 1.0 / 360.0"),
    DivConst(360.0, "degrees in bd_set_phase_deg", "jaero_device.h:222", "jd_div_const(phase_deg, 360.0, 1.0 / 360.0)"),
    DivConst(19999.0, "JD_WTSIZE (also k_burst_demod.h:131)", "k_oqpsk_fb.h:320", "r_wtsize = 1.0 / wtsize_d"),
    DivConst(585.0, "burst OQPSK agc2_len = round(64 SPS), SPS = 2 Fs / fb, k_burst_demod.h:131", "burst_host.h:23",
             "g.agc2_len = (int)round((SPS * 64.0 / s.Fs) * s.Fs)"),
    DivConst(128.0, "burst OQPSK msema_len, k_burst_demod.h:132", "burst_host.h:36", "g.msema_len = 128"),
]


@dataclass(frozen=True)
class Biquad:
    what: str
    site: str  # file:line under jaero_amd/csrc of the line that sets b0 (the a's are on the line next to it)
    b: tuple  # b0, b1, b2
    a: tuple  # a1, a2


# the second-order sections fill_geometry gives the banks that jd_biquad serves: 10.5 kbps OQPSK (resonator, loop filter), MSK at 48 kHz
BIQUADS = [
    Biquad("OQPSK 10.5k resonator", "jaero_hip.hip:436", (0.00032714218939589035, 0.0, 0.00032714218939589035), (-0.39005299948210803, 0.99934571562120822)),
    Biquad("OQPSK loop filter", "jaero_hip.hip:444", (0.0010275610653672064, 0.0020551221307344128, 0.0010275610653672064),
           (-1.9207386815577139, 0.92509247310306331)),
    Biquad("MSK 1200 resonator", "jaero_hip.hip:460", (2.617308727964618e-04, 0.0, -2.617308727964618e-04), (-1.993312819378528, 0.999476538254407)),
    Biquad("MSK 600 resonator", "jaero_hip.hip:468", (1.308825621597620e-04, 0.0, -1.308825621597620e-04), (-1.998196509168551, 0.999738234875681)),
]
# the sample rates the oscillators divide by (jaero_hip.hip:380: continuous MSK also runs at 24 and 12 kHz)
SAMPLE_RATES = (48000.0, 24000.0, 12000.0)


def prims():
    """ctypes handle of libjaero_prims.so with the launchers' argument types (built by __graft_entry__.build / make -C jaero_amd/csrc)."""
    L = C.CDLL(PRIMS_LIB)
    P = C.c_void_p
    n, f, m = C.c_long, C.c_double, C.c_ulonglong
    sig = {
        "jp_atan2": [P, P, P, n, m],
        "jp_hypot": [P, P, P, n],
        "jp_div": [P, P, P, P, n],
        "jp_div_const": [P, P, P, n, f, f],
        "jp_wt_next": [P, P, n],
        "jp_fb_wt_next": [P, P, n],
        "jp_wt_setfreq": [P, P, P, n, f],
        "jp_fb_wt_setfreq": [P, P, P, n, f, f],
        "jp_wt_inc_phase_deg": [P, P, n],
        "jp_wt_advance_fraction": [P, P, n],
        "jp_wt_passed": [P, P, P, P, P, P, n],
        "jp_bd_set_phase_deg": [P, P, n],
        "jp_biquad": [P, P, P, n, C.c_int, f, f, f, f, f],
        "jp_diff_soft": [P, P, P, n],
        "jp_wt_next_symbol": [P, P, P, n],
    }
    for name in ("jp_tanh", "jp_tanh_full", "jp_expm1", "jp_log10", "jp_qround", "jp_softbit", "jp_cisidx", "jp_fb_fmod360"):
        sig[name] = [P, P, n]
    for r in FIR_ROWS:
        sig[r.export] = [P] * (9 if r.bs else 7)  # block rows: start_re, start_im in front of the outputs
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = C.c_int
    return L


REF_SRC = os.path.join(ROOT, "tests", "device_math_ref.c")


def build_ref(tmp_dir):
    """Compile tests/device_math_ref.c (the host libm and __float128 over arrays) into tmp_dir and load it."""
    so = os.path.join(str(tmp_dir), "libdevice_math_ref.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", REF_SRC, "-o", so, "-lm", "-lquadmath"])
    L = C.CDLL(so)
    for name in ("ref_hypot", "ref_atan2", "ref_atan2q"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    for name in ("ref_tanh", "ref_expm1"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    L.ref_libc_version.restype = C.c_char_p
    return L
