"""Host only: tests/device_prims.py lists every device primitive of jd_libm.h / jaero_device.h, libjaero_prims.so exports exactly its launchers,
the GPU module runs each of them, and its rows agree with the product's call sites.  Also: jd_atan2's table against mpmath, and the gcc-built
libm reference of the GPU module against the libm the process itself loads."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import device_prims as DP

HERE = os.path.dirname(os.path.abspath(__file__))
# a definition: `__device__ ... name(` or jd_libm.h's `JDA_FN ... name(` at the start of a line (templates put their head on the line before)
_DEF = re.compile(r"^(?:__device__|JDA_FN)\b[^(;]*?\b((?:jd|fb|bd)_[A-Za-z0-9_]+)\s*\(", re.M)


def read(name):
    with open(os.path.join(DP.CSRC, name)) as f:
        return f.read()


def defined_primitives():
    names = set()
    for h in DP.HEADERS:
        names |= set(_DEF.findall(read(h)))
    return names


def kernel_headers():
    """The headers that hold kernel text: every k_*.h and demod_stages.h, the stages several of them share."""
    return sorted(f for f in os.listdir(DP.CSRC) if (f.startswith("k_") and f.endswith(".h")) or f == "demod_stages.h")


def test_every_primitive_has_a_launcher_or_a_reason():
    have = defined_primitives()
    assert {"jd_atan2", "jd_hypot", "jd_div_const", "bd_set_phase_deg", "jd_fir_eval"} <= have, have
    launched = set(DP.LAUNCHERS.values()) | {r.func for r in DP.FIR_ROWS}
    assert not launched & set(DP.NOT_LAUNCHED), launched & set(DP.NOT_LAUNCHED)
    missing = sorted(have - launched - set(DP.NOT_LAUNCHED))
    stale = sorted((launched | set(DP.NOT_LAUNCHED)) - have)
    assert not missing, f"device primitives with neither a launcher nor a reason in tests/device_prims.py: {missing}"
    assert not stale, f"rows of tests/device_prims.py for functions the headers do not define: {stale}"


def test_helpers_live_beside_the_primitives_not_in_kernel_headers():
    """The test library includes no kernel header, so nothing it runs may be defined in one."""
    src = read("prims_check.hip")
    assert re.findall(r'#include\s+"([^"]+)"', src) == ["jaero_device.h"]
    assert "demod_stages.h" in kernel_headers()
    for k in kernel_headers():
        dup = set(_DEF.findall(read(k))) & defined_primitives()
        assert not dup, f"{k} defines {dup}"


def test_library_exports_exactly_the_launchers():
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("no nm on PATH")
    assert os.path.exists(DP.PRIMS_LIB), "libjaero_prims.so is not built (make -C jaero_amd/csrc)"
    out = subprocess.run([nm, "-D", "--defined-only", DP.PRIMS_LIB], check=True, capture_output=True, text=True).stdout
    exports = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("jp_")}
    want = set(DP.LAUNCHERS) | {r.export for r in DP.FIR_ROWS}
    assert exports == want, (sorted(exports - want), sorted(want - exports))


def test_gpu_module_runs_every_launcher():
    with open(os.path.join(HERE, "test_gpu_device_math.py")) as f:
        src = f.read()
    for name in DP.LAUNCHERS:
        assert f'"{name}"' in src, f"tests/test_gpu_device_math.py never calls {name}"
    assert "DP.FIR_ROWS" in src and "DP.DIV_CONSTS" in src and "DP.SAMPLE_RATES" in src


def test_fir_rows_match_their_call_sites():
    oq, hip = read("k_oqpsk_fb.h"), read("jaero_hip.hip")
    val = lambda src, name: int(re.search(rf"#define {name} (\d+)", src).group(1))  # noqa: E731
    fb_ldsn, solo_d = val(oq, "FB_LDSN"), val(oq, "FB_SOLO_D")
    msk40, msk20 = val(hip, "MSK_LDSN_40"), val(hip, "MSK_LDSN_20")
    # the block rows: k_msk_fb's front half calls jd_fir_sum_blocks<FIRN, LDSN, 8, false, TB, mfb_bs<LDSN>()> for the three msk_fb_rec<FIRN, LDSN,
    # PAIRS, TB> of jaero_hip.hip; k_burst_oqpsk_demod calls jd_fir_sum<55, BD_LDSN, 8, BD_FUSED, 0> over JdRingBlocks<BD_LDSN, BD_BS, ..>
    mfb, bd = read("k_msk_fb.h"), read("k_burst_demod.h")
    bs_max = val(mfb, "MFB_BS_MAX")
    assert "constexpr int mfb_bs() { return (LDSN % 8 == 0 && MFB_BS_MAX >= 8) ? 8 : (MFB_BS_MAX >= 4 ? 4 : 2); }" in mfb
    mfb_bs = lambda ldsn: 8 if (ldsn % 8 == 0 and bs_max >= 8) else (4 if bs_max >= 4 else 2)  # noqa: E731
    recs = re.findall(r"msk_fb_rec<(\d+), (\w+), \d+, (\w+)>", hip)
    assert sorted(recs) == sorted([("160", "MFB2_LDSN", "MFB2_TB"), ("80", "MFB4_LDSN", "MFB4_TB"), ("80", "MFB_LDSN", "MFB1_TB")]), recs
    blocks = {(int(firn), val(mfb, ldsn), 8, False, val(mfb, tb), mfb_bs(val(mfb, ldsn))) for firn, ldsn, tb in recs}
    bd_fused = re.search(r"#ifdef JD_BURST_EXACT\n#define BD_FUSED false\n.*?#else\n#define BD_FUSED true\n", bd, re.S) is not None
    blocks.add((55, val(bd, "BD_LDSN"), 8, bd_fused, 0, val(bd, "BD_BS")))
    assert {(r.firn, r.ldsn, r.d, r.fused, r.t0, r.bs) for r in DP.FIR_ROWS if r.bs} == blocks
    assert blocks == {(80, 36, 8, False, 32, 4), (80, 32, 8, False, 18, 4), (160, 72, 8, False, 64, 4), (55, 36, 8, True, 0, 6)}
    want = {
        "jp_fir_eval_40_24_8": (40, msk40, 8), "jp_fir_eval_20_12_8": (20, msk20, 8), "jp_fir_eval_fused_55_36_8": (55, fb_ldsn, 8),
        "jp_fir_eval_sym_55_36_6": (55, fb_ldsn, 6), "jp_fir_eval_sym_static_55_36_6": (55, fb_ldsn, 6),
        "jp_fir_eval_sym_static_but_last_55_36_6": (55, fb_ldsn, solo_d),
    }
    assert {r.export: (r.firn, r.ldsn, r.d) for r in DP.FIR_ROWS if not r.bs} == want
    # the only row without a call site is the fused sum over the walked ring; no row without blocks continues a sum
    assert [r.export for r in DP.FIR_ROWS if not r.site] == ["jp_fir_eval_fused_55_36_8"]
    assert [r.export for r in DP.FIR_ROWS if r.fused and not r.bs] == ["jp_fir_eval_fused_55_36_8"] and not any(r.t0 for r in DP.FIR_ROWS if not r.bs)
    prims = read("prims_check.hip")
    for r in DP.FIR_ROWS:
        if r.bs:
            assert f"JP_FIR_BLOCKS({r.export}, {r.firn}, {r.ldsn}, {r.d}, {'true' if r.fused else 'false'}, {r.t0}, {r.bs})" in prims, r
        else:
            assert f"JP_FIR({r.export}, " in prims and f", {r.firn}, {r.ldsn}, {r.d}, {'true' if r.fused else 'false'})" in prims, r
        if r.site:
            f, line = r.site.split(":")
            text = read(f).splitlines()[int(line) - 1]
            assert f"{r.func}<" in text, (r.site, text)
    assert "jd_fir_sum_blocks<FIRN, LDSN, 8, false, TB, mfb_bs<LDSN>()>(" in mfb and mfb.count("jd_fir_sum_blocks<") == 1
    assert "jd_fir_sum<FIRN, LDSN, 8, BD_FUSED, 0>(JdRingBlocks<LDSN, BD_BS, B, NB + 1>{" in bd and "constexpr int FIRN = 55, LDSN = BD_LDSN" in bd
    # the launcher of the block rows runs the dispatcher, and the dispatcher the same jd_fir_sum over JdRingBlocks
    assert "jd_fir_sum_blocks<FIRN, LDSN, D, FUSED, T0, BS>(" in prims
    assert "jd_fir_sum<FIRN, LDSN, D, FUSED, T0>(JdRingBlocks<LDSN, BS, B, NB + 1>{" in read("jaero_device.h")
    # the template arguments at the call sites: jd_fir_eval<FIRN, LDSN, 8> in k_msk.h (FIRN 40 / 20 from jaero_hip.hip), the 55-tap forms
    assert re.search(r"msk_samples_rec<40, MSK_LDSN_40>", hip) and re.search(r"msk_samples_rec<20, MSK_LDSN_20>", hip)
    assert "k_oqpsk_fb<55, FB_LDSN," in hip
    calls = re.findall(r"(jd_fir_eval[a-z_]*)<([^>]*)>\(", oq + read("k_msk.h"))
    assert sorted(calls) == sorted([("jd_fir_eval", "FIRN, LDSN, 8"), ("jd_fir_eval_sym", "FIRN, LDSN, 6"),
                                    ("jd_fir_eval_sym_static_but_last", "FIRN, LDSN, FB_SOLO_D"), ("jd_fir_eval_sym_static", "FIRN, LDSN, 6")])


def test_div_const_rows_cite_where_each_divisor_is_computed():
    for dc in DP.DIV_CONSTS:
        f, line = dc.site.split(":")
        text = read(f).splitlines()[int(line) - 1]
        assert dc.token in text, (dc.site, text)
    # the values those lines give for every supported (kind, fb, Fs): jd_div_const is only reached at Fs = 48 000 (OQPSK, burst OQPSK at 10 500 bps)
    Fs, fb = 48000.0, 10500.0
    sps = 2.0 * Fs / fb
    assert round(4 * Fs) == 192000 and int(2 * Fs) == 96000 and round((sps * 64.0 / Fs) * Fs) == 585
    assert sorted({dc.d for dc in DP.DIV_CONSTS}) == sorted({192000.0, 96000.0, 800.0, 400.0, 48000.0, 360.0, 19999.0, 585.0, 128.0})
    # every kernel header that calls jd_div_const is one whose divisors are listed
    users = [f for f in kernel_headers() if "jd_div_const(" in read(f)]
    assert users == ["k_burst_demod.h", "k_oqpsk_fb.h"], users


def _table():
    src = read("jd_atan2_tbl.h")
    arr = lambda name: [float.fromhex(v.strip().rstrip("f")) for v in re.search(rf"{name}\[65\] = \{{([^}}]*)\}}", src).group(1).split(",")]  # noqa: E731
    return arr("JD_ATAN_HI"), arr("JD_ATAN_LOF")


def test_atan_table_against_mpmath():
    mpmath = pytest.importorskip("mpmath")
    hi, lof = _table()
    assert len(hi) == 65 and len(lof) == 65
    mpmath.mp.prec = 300
    for i in range(65):
        a = mpmath.atan(mpmath.mpf(i) / 64)
        assert hi[i] == float(a), (i, hi[i].hex())  # the leading double is the correctly rounded atan(i/64)
        err = abs(mpmath.mpf(hi[i]) + mpmath.mpf(lof[i]) - a)
        assert err <= (a * mpmath.mpf(2) ** -75 if i else 0), (i, float(err))


def test_gcc_reference_agrees_with_the_process_libm(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    R = DP.build_ref(tmp_path)
    m = C.CDLL("libm.so.6")
    for fn in ("hypot", "atan2", "tanh", "expm1"):
        getattr(m, fn).restype = C.c_double
        getattr(m, fn).argtypes = [C.c_double] * (2 if fn in ("hypot", "atan2") else 1)
    rng = np.random.default_rng(5)
    n = 4000
    a = np.ascontiguousarray(np.concatenate([rng.standard_normal(n) * np.exp2(rng.uniform(-40, 40, n)), [0.0, -0.0, np.inf, -np.inf]]))
    b = np.ascontiguousarray(np.concatenate([rng.standard_normal(n) * np.exp2(rng.uniform(-40, 40, n)), [-0.0, 1.0, np.nan, 2.0]]))
    x = np.ascontiguousarray(np.concatenate([rng.uniform(-30, 30, n), [0.0, -0.0, 1e-300, 22.0]]))
    for name, ref, args in (("hypot", R.ref_hypot, (a, b)), ("atan2", R.ref_atan2, (a, b)), ("tanh", R.ref_tanh, (x,)), ("expm1", R.ref_expm1, (x,))):
        o = np.zeros(len(args[0]))
        ref(*[v.ctypes.data for v in args], o.ctypes.data, len(o))
        want = np.array([getattr(m, name)(*[float(v[i]) for v in args]) for i in range(len(o))])
        same = (o.view(np.int64) == want.view(np.int64)) | (np.isnan(o) & np.isnan(want))
        assert same.all(), (name, int((~same).sum()))
    # atan2q rounded once is the correctly rounded atan2 (mpmath at 200 bits on a sample)
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.prec = 200
    o = np.zeros(len(a))
    R.ref_atan2q(a.ctypes.data, b.ctypes.data, o.ctypes.data, len(a))
    for i in range(0, n, 8):
        assert o[i] == float(mpmath.atan2(mpmath.mpf(float(a[i])), mpmath.mpf(float(b[i])))), i
