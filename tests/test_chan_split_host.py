"""CPU: the splitter's C ABI without a device (exports, the refusals of jaero_split_create in their documented order, null handles, no CPU
fallback) and `plan_outputs`, the pure function between the rate meter and the banks."""
import ctypes as C

import numpy as np
import pytest

from jaero_amd import capi, channeliser as CH

SYMBOLS = ["jaero_split_create", "jaero_split_destroy", "jaero_split_write", "jaero_split_feed", "jaero_split_output", "jaero_split_info",
           "jaero_split_profile_enable", "jaero_split_profile_read"]
AUDIO = 715827883


def test_library_exports_the_eight_symbols():
    L = capi.lib()
    for name in SYMBOLS:
        assert name in capi.EXPORTS and hasattr(L, name), name
    assert C.sizeof(capi.ChanOutput) == 32  # 2 int, 2 pointers, int, padding
    assert L.jaero_abi_version() == 1


def _output(rate=48000, nch=2, gains=(1.0, 1.0), taps=None, ch_null=False, taps_null=False):
    arr = (capi.ChanChannel * max(nch, 1))(*[capi.ChanChannel(1000 * i, AUDIO, g) for i, g in zip(range(max(nch, 1)), gains)])
    t = np.ones(3) / 3 if taps is None else np.asarray(taps, dtype=np.float64)
    row = capi.ChanOutput(rate, nch, None if ch_null else C.cast(arr, C.c_void_p), None if taps_null else t.ctypes.data, t.size)
    return row, (arr, t)


def _create(L, fs_c=3072000, outs=({}, dict(rate=12000)), noutputs=None, outs_null=False, out_null=False, max_write_iq=8192, cap=None):
    """jaero_split_create of outputs described by keyword sets for `_output`; cap: None or keywords of a capi.Capture (rtaps "design": ones)."""
    rows, keep = zip(*[_output(**kw) for kw in outs]) if outs else ((), ())
    arr = (capi.ChanOutput * max(len(rows), 1))(*rows)
    cs = None
    if cap is not None:
        kw = dict(fmt=capi.IQ_CU8, fs_in=2400000, K=32, rtaps="design")
        kw.update(cap)
        rt = kw["rtaps"]
        if isinstance(rt, str):
            Lr = CH.resample_ratio(max(kw["fs_in"], 1), max(fs_c, 1))[0]
            rt = np.ones(min(Lr, 4096) * max(kw["K"], 1)) / max(kw["K"], 1)
        keep = keep + (rt,)
        cs = capi.Capture(kw["fmt"], kw["fs_in"], 0, kw["K"], None if rt is None else rt.ctypes.data)
    h = C.c_void_p()
    rc = L.jaero_split_create(0, None if cs is None else C.byref(cs), fs_c, len(rows) if noutputs is None else noutputs,
                              None if outs_null else arr, max_write_iq, None if out_null else C.byref(h))
    return rc, h


BAD_RT = np.ones(32 * 32)
BAD_RT[100] = np.nan
NINE = tuple({} for _ in range(9))

# each case: every earlier check passes (or is broken as well, to show the order), one thing is named
REFUSALS = [
    (dict(out_null=True, outs_null=True), b"out is null"),
    (dict(outs_null=True, noutputs=0), b"outs is null"),
    (dict(noutputs=0, fs_c=0), b"noutputs 0"), (dict(outs=NINE, fs_c=0), b"noutputs 9"), (dict(noutputs=-1), b"noutputs -1"),
    (dict(fs_c=0, outs=(dict(rate=5),)), b"fs_c 0"), (dict(fs_c=-3072000), b"fs_c -3072000"),
    # per output, in order: its rate, its D, then jaero_chan2_create's own checks
    (dict(outs=(dict(rate=44100, nch=0),)), b"output 0: out_rate 44100"),
    (dict(outs=({}, dict(rate=0, ch_null=True))), b"output 1: out_rate 0"),
    (dict(fs_c=1000000, outs=(dict(nch=0),)), b"output 0: fs_c 1000000 / out_rate 48000"),       # no exact D
    (dict(fs_c=384000, outs=(dict(nch=0),)), b"output 0: fs_c 384000 / out_rate 48000"),         # D = 8
    (dict(fs_c=768000, outs=({}, dict(rate=24000), dict(rate=12000), dict(rate=6000))), b"output 3: out_rate 6000"),
    (dict(fs_c=3072000, outs=({}, dict(rate=24000), dict(rate=12000)), max_write_iq=0), b"output 0: max_write_iq 0"),
    (dict(fs_c=6144000, outs=(dict(rate=12000),)), b"output 0: fs_c 6144000 / out_rate 12000"),  # D = 512
    (dict(outs=(dict(ch_null=True, nch=0),)), b"output 0: null"), (dict(outs=({}, dict(taps_null=True))), b"output 1: null"),
    (dict(outs=({}, dict(nch=0, taps=np.ones(8194)))), b"output 1: nchannels 0"),
    (dict(outs=(dict(taps=np.ones(8194)),), max_write_iq=0), b"output 0: ntaps 8194"),
    (dict(outs=({}, dict(gains=(1.0, 0.0))), max_write_iq=0), b"output 0: max_write_iq 0"),
    (dict(outs=({}, dict(gains=(1.0, 0.0), taps=[0.5, float("nan")]))), b"output 1: channel 1: gain 0"),
    (dict(outs=({}, dict(taps=[0.5, float("nan")])), cap=dict(fmt=9)), b"output 1: tap 1"),
    # an earlier output's fault is named before a later one's
    (dict(outs=(dict(gains=(1.0, -1.0)), dict(rate=7))), b"output 0: channel 1: gain -1"),
    # with a capture: jaero_chan3_create's checks with Fs_c = fs_c, behind every output's
    (dict(cap=dict(fmt=4, fs_in=0)), b"format 4"),
    (dict(cap=dict(fs_in=0, K=0)), b"fs_in 0"),
    (dict(cap=dict(fs_in=3072001, K=0)), b"L above 1024"),
    (dict(cap=dict(fs_in=3072000 * 8 + 3072, K=0)), b"beyond 8"),
    (dict(cap=dict(K=65)), b"taps_per_phase 65"), (dict(cap=dict(K=0, rtaps=None)), b"taps_per_phase 0"),
    (dict(cap=dict(rtaps=None)), b"rtaps"),
    (dict(cap=dict(rtaps=BAD_RT), max_write_iq=1 << 30), b"resampler tap 100"),
    (dict(cap=dict(fs_in=384000), max_write_iq=1 << 28), b"stages"),       # 8 / 1 x 2^28 staged samples
    (dict(cap=dict(fs_in=3072000, K=-3, rtaps=None), max_write_iq=(1 << 31) - 1), b"stages"),
]


@pytest.mark.parametrize("kw,word", REFUSALS)
def test_create_refusals_need_no_device_and_come_in_order(kw, word):
    """JAERO_EINVAL before a device is looked for, *out stays null, and the message names the function and the offending value."""
    L = capi.lib()
    rc, h = _create(L, **kw)
    msg = L.jaero_last_error()
    assert rc == capi.E_INVAL and not h.value, (rc, msg)
    assert msg.startswith(b"jaero_split_create:") and word in msg, msg


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


@pytest.mark.parametrize("kw", [
    dict(fs_c=3072000, outs=({},)),                                                   # D = 64
    dict(fs_c=3072000, outs=({}, dict(rate=24000), dict(rate=12000), dict(nch=1))),   # 64 / 128 / 256, two outputs share a D
    dict(fs_c=768000, outs=({}, dict(rate=24000), dict(rate=12000))),                 # 16 / 32 / 64
    dict(fs_c=3072000, cap={}),                                                       # cu8 at 2.4 MS/s
    dict(fs_c=3072000, cap=dict(fs_in=3072000, K=-3, rtaps=None)),                    # equal rates: K and rtaps are not looked at
    dict(outs=tuple({} for _ in range(8))),
])
def test_valid_arguments_get_as_far_as_the_device(kw):
    """Everything valid: the one thing left to fail is the device, and JAERO_ENODEV comes last (no CPU fallback)."""
    L = capi.lib()
    rc, h = _create(L, **kw)
    if _has_gpu():
        assert rc == capi.E_OK and h.value, L.jaero_last_error()
        L.jaero_split_destroy(h)
    else:
        assert rc == capi.E_NODEV and not h.value, (rc, L.jaero_last_error())


def test_null_handles_are_refused():
    L = capi.lib()
    n, ms, v = C.c_int(7), C.c_double(), C.c_void_p()
    buf = np.zeros(8, np.int16)
    banks = (C.c_void_p * 1)(None)
    L.jaero_split_destroy(None)  # nothing happens
    assert L.jaero_split_write(None, buf.ctypes.data, 2, 0, None, C.byref(n)) == capi.E_INVAL and b"jaero_split_write" in L.jaero_last_error()
    assert L.jaero_split_feed(None, banks, buf.ctypes.data, 2, 0, None, C.byref(n)) == capi.E_INVAL and b"jaero_split_feed" in L.jaero_last_error()
    assert L.jaero_split_output(None, 0, C.byref(v)) == capi.E_INVAL and b"jaero_split_output" in L.jaero_last_error()
    assert L.jaero_split_info(None, C.byref(n), C.byref(n), C.byref(n)) == capi.E_INVAL and b"jaero_split_info" in L.jaero_last_error()
    assert L.jaero_split_profile_enable(None, 1) == capi.E_INVAL and b"jaero_split_profile_enable" in L.jaero_last_error()
    assert L.jaero_split_profile_read(None, 0, C.byref(ms), C.byref(n), 0) == capi.E_INVAL and b"jaero_split_profile_read" in L.jaero_last_error()
    assert n.value == 7 and not v.value


def test_python_wrapper_has_no_cpu_fallback():
    outs = [(48000.0, [(0, 0, 1.0)], np.ones(1)), (12000.0, [(5, 0, 1.0)], None)]
    if _has_gpu():
        sp = CH.Splitter(3072000, outs)
        assert [(o.decim, o.nch, o.fs_out) for o in sp.outputs] == [(64, 1, 48000.0), (256, 1, 12000.0)]
        sp.close()
    else:
        with pytest.raises(capi.JaeroError) as e:
            CH.Splitter(3072000, outs)
        assert e.value.code == capi.E_NODEV
    with pytest.raises(capi.JaeroError) as e:
        CH.Splitter(1000000, [(48000.0, [(0, 0, 1.0)], np.ones(1))])
    assert e.value.code == capi.E_INVAL
    with pytest.raises(ValueError):
        CH.Splitter(1000000, [(48000.0, [(0, 0, 1.0)], None)])  # no D: no default taps either


# ---------------------------------------------------------------------------------------------- plan_outputs
def test_plan_outputs_groups_by_rate():
    fs_c = 3072000
    hz = [-1.2e6, 250000.0, -40000.5, 33.3, 900000.0, 123456.7, -700000.0, 5.0]
    rates = [600, 10500, 1200, 10500, 0, 600, 2400, 600]  # no 8400 carrier; 0 = no rate found, 2400 = a rate no bank runs
    p = CH.plan_outputs(hz, rates, fs_c)
    assert p.rates == [10500, 1200, 600]  # output order; no output for 8400
    assert [o[0] for o in p.outputs] == [48000.0, 24000.0, 12000.0] and all(o[2] is None for o in p.outputs)
    assert p.indices == [[1, 3], [2], [0, 5, 7]]
    assert p.left_out == [4, 6]
    for (fs_out, chans, _), idx in zip(p.outputs, p.indices):
        assert [c[0] for c in chans] == [CH.tune_word(hz[i], fs_c) for i in idx]
        assert all(c[1] == CH.tune_word(fs_out / 6, fs_out) and c[2] == 1.0 for c in chans)
        assert all(abs(CH.word_hz(c[0], fs_c) - hz[i]) <= fs_c / 2.0 ** 32 for c, i in zip(chans, idx))
    assert CH.tune_word(48000.0 / 6, 48000.0) == AUDIO


def test_plan_outputs_separates_the_two_48k_rates_and_takes_words():
    p = CH.plan_outputs([1000.0, 2000.0, 3000.0], [8400.0, 10500.0, 8400.0], 768000, audio_hz=1000.0, gain=2.5)
    assert p.rates == [10500, 8400] and p.indices == [[1], [0, 2]] and p.left_out == []
    assert [o[0] for o in p.outputs] == [48000.0, 48000.0]
    assert p.outputs[1][1] == [(CH.tune_word(1000.0, 768000.0), CH.tune_word(1000.0, 48000.0), 2.5),
                               (CH.tune_word(3000.0, 768000.0), CH.tune_word(1000.0, 48000.0), 2.5)]
    empty = CH.plan_outputs([], [], 3072000)
    assert empty.outputs == [] and empty.indices == [] and empty.left_out == []
    with pytest.raises(ValueError):
        CH.plan_outputs([1.0, 2.0], [600], 3072000)
