"""GPU (-m gpu): the channeliser's splitter (jaero_split_*, jaero_amd/csrc/split_host.h) against its definition: output g is, bit for bit and
in every reader, what a stand-alone handle of decim fs_c / fs_out_g with the output's channels and taps produces from the same writes.  The
stand-alone handle is the reference throughout (its own correctness is what tests/test_gpu_chan*.py establish), so no tolerance appears."""
import ctypes as C

import numpy as np
import pytest

import chan_oracle as CO
from chan_cases import AUDIO, CH

pytestmark = pytest.mark.gpu

HP = CO.HP
CAP_RUN = 256  # the staging kernel's run of outputs per workgroup


def random_channels(CHm, rng, n, fs_c):
    return [(CHm.tune_word(float(rng.uniform(-fs_c / 2, fs_c / 2)), float(fs_c)), AUDIO, 1.0) for _ in range(n)]


def four_outputs(CHm, fs_c, rng):
    """48 kHz x 9, 24 kHz x 5, 12 kHz x 33 (more than one workgroup of items at D = 256), and a second 48 kHz output with other taps."""
    outs = []
    for fs_out, nch, cutoff in ((48000.0, 9, None), (24000.0, 5, None), (12000.0, 33, None), (48000.0, 1, 20000.0)):
        taps = CHm.design_taps(int(fs_c // fs_out), cutoff_hz=cutoff, ntaps=2049, beta=10.0, fs_out=fs_out)
        outs.append((fs_out, random_channels(CHm, rng, nch, fs_c), taps))
    return outs


def make_pair(CHm, fs_c, outs, max_write_iq, capture=None):
    """(splitter, twins): the twins are the stand-alone handles of the definition."""
    sp = CHm.Splitter(fs_c, outs, capture=capture, max_write_iq=max_write_iq)
    twins = [CHm.Channeliser(int(fs_c // fs_out), chans, taps=taps, max_write_iq=max_write_iq, fs_out=fs_out, capture=capture)
             for fs_out, chans, taps in outs]
    for o, t in zip(sp.outputs, twins):
        assert (o.decim, o.nch, o.Mo, o.fs_out) == (t.decim, t.nch, t.Mo, t.fs_out)
    return sp, twins


def write_both(sp, twins, piece, where=""):
    """One write of the splitter and of every twin; nout and the PCM bytes must agree.  Returns the splitter's PCM per output."""
    nout = sp.write(piece)
    pcm = []
    for g, (o, t) in enumerate(zip(sp.outputs, twins)):
        assert t.write(piece) == nout[g] == o.last_nout, (where, g)
        got, ref = o.read_pcm(), t.read_pcm()
        assert got.shape == ref.shape == (o.nch, nout[g]), (where, g)
        assert got.tobytes() == ref.tobytes(), (where, g, "PCM differs from the stand-alone twin")
        assert o.pcm_view()[1] == nout[g]
        pcm.append(got)
    return pcm


def close_all(*hs):
    for h in hs:
        h.close()


# ---------------------------------------------------------------------------------------------- 1. twin identity, int16
@pytest.mark.parametrize("fs_c", [3072000, 768000])
def test_twin_identity_int16(CH, fs_c):
    import torch

    rng = np.random.default_rng(fs_c)
    mw = 4 * HP
    outs = four_outputs(CH, fs_c, rng)
    assert sorted({int(fs_c // o[0]) for o in outs}) == ([64, 128, 256] if fs_c == 3072000 else [16, 32, 64])
    sp, twins = make_pair(CH, fs_c, outs, mw)
    assert sp.nblk_max == 5
    sizes = [1, 8191, 8193, 3 * 8192 + 5, mw, 0, 8191 - 5, 2 * HP, 3]
    total = sum(sizes)
    iq = rng.integers(-32768, 32768, size=(total + HP, 2)).astype(np.int16)
    diq = torch.from_numpy(iq).cuda()
    pos, produced = 0, 0
    parts = [[] for _ in outs]
    for i, n in enumerate(sizes):
        on_device = (i + (fs_c == 768000)) % 2 == 1  # half of the writes from a device tensor, the other half in the other run
        piece = diq[pos:pos + n].contiguous() if on_device else iq[pos:pos + n]
        pcm = write_both(sp, twins, piece, f"write {i} of {n}")
        blocks = (pos + n) // HP - produced
        assert [p.shape[1] for p in pcm] == [blocks * o.Mo for o in sp.outputs]
        pos += n
        produced += blocks
        for g, p in enumerate(pcm):
            parts[g].append(p)
    for g, ps in enumerate(parts):
        rms = np.concatenate(ps, axis=1).astype(float).std(axis=1)
        print(f"fs_c {fs_c} output {g}: {len(rms)} channels, smallest RMS {rms.min():.0f} LSB")
        assert rms.min() > 100.0, g
    # an oversized write is refused and changes nothing: the next piece continues where the last accepted one ended
    from jaero_amd import capi
    with pytest.raises(capi.JaeroError) as e:
        sp.write(np.zeros((mw + 1, 2), np.int16))
    assert e.value.code == capi.E_INVAL and "jaero_split_write" in str(e.value)
    assert [o.last_nout for o in sp.outputs] == [0] * len(outs)  # what the last accepted write (3 samples) produced
    pcm = write_both(sp, twins, iq[pos:pos + HP], "behind the refusal")
    assert all(p.shape[1] == o.Mo for p, o in zip(pcm, sp.outputs))
    close_all(sp, *twins)


# ---------------------------------------------------------------------------------------------- 2. twin identity, capture handle
def ragged_capture_sizes(K, L, Mr, max_write_iq, total):
    """As tests/test_gpu_chan_capture.py cuts its captures: 0, 1, K - 2, K - 1, K, the inputs that stage one sample less than, exactly and
    one more than a workgroup's run (and two runs), max_write_iq, and odd sizes in between; the last pieces take what is left."""
    around = [(-(-k * Mr // L)) for k in (CAP_RUN - 1, CAP_RUN, CAP_RUN + 1, 2 * CAP_RUN - 1, 2 * CAP_RUN, 2 * CAP_RUN + 1)]
    sizes = [1, 0, max(K - 2, 0), max(K - 1, 0), K, 1, 1, 2] + around + [7777, 3, max_write_iq, 12345, 0, 5]
    assert sum(sizes) < total
    left = total - sum(sizes)
    while left > 0:
        sizes.append(min(left, max_write_iq - 1))
        left -= sizes[-1]
    return sizes


def capture_pair(CHm, rng, max_write_iq=40000):
    fs_c = 3072000
    cap = CHm.Capture(fs_in=2400000, fmt="cu8")
    outs = [(48000.0, random_channels(CHm, rng, 3, fs_c), CHm.design_taps(64, ntaps=2049, beta=10.0)),
            (12000.0, random_channels(CHm, rng, 7, fs_c), CHm.design_taps(256, ntaps=2049, beta=10.0, fs_out=12000.0))]
    return make_pair(CHm, fs_c, outs, max_write_iq, capture=cap)


def test_twin_identity_capture(CH):
    """cu8 at 2.4 MS/s into fs_c = 3.072 MS/s (32 / 25, K = 32): one staging launch and one forward transform feed both outputs; with the
    profile on, the splitter's staging launches are the writes that staged anything and the views never launch a front-end kernel."""
    rng = np.random.default_rng(24)
    sp, twins = capture_pair(CH, rng)
    L, Mr = CH.resample_ratio(2400000, 3072000)
    assert (L, Mr) == (32, 25) and sp.fmt == "cu8" and sp.outputs[1].fs_in == 2400000.0
    total = 100000
    raw = rng.integers(0, 256, size=(total, 2), dtype=np.uint8)
    sp.profile_enable(True)
    pos, staged_writes, block_writes, blocks = 0, 0, 0, 0
    parts = [[] for _ in twins]
    for i, n in enumerate(ragged_capture_sizes(32, L, Mr, 40000, total)):
        pcm = write_both(sp, twins, raw[pos:pos + n], f"write {i} of {n}")
        staged_writes += -(-(pos + n) * L // Mr) > -(-pos * L // Mr)
        pos += n
        done = -(-pos * L // Mr) // HP
        assert pcm[0].shape[1] == (done - blocks) * sp.outputs[0].Mo
        block_writes += done > blocks
        blocks = done
        for g, p in enumerate(pcm):
            parts[g].append(p)
    assert pos == total and blocks == 15
    for g, ps in enumerate(parts):
        assert np.concatenate(ps, axis=1).astype(float).std(axis=1).min() > 100.0, g
    assert sp.profile_read(1)[1] == staged_writes > 10
    assert sp.profile_read(0)[1] == block_writes > 3
    for o in sp.outputs:
        assert o.profile_read(0)[1] == 0 and o.capture_profile_read(0)[1] == 0 and o.capture_profile_read(1)[1] == 0
        assert o.profile_read(1)[1] == block_writes
    close_all(sp, *twins)


# ---------------------------------------------------------------------------------------------- 3. measurements on views
def measurements(c, spectra):
    """Every reader of the survey and the activity, as bytes (nan where a channel has no block: the same constant on both sides)."""
    e, n = c.read_level_sums()
    act = c.read_activity()
    got = {"level": e.tobytes(), "level_n": n.tolist(), "act_n": act.n.tolist(), "when": act.when.tolist(),
           "emax": act.emax.tobytes(), "emin": act.emin.tobytes(), "hist": act.hist.tobytes()}
    if spectra:
        s, ns = c.read_psd_sums()
        p, npk = c.read_peak_sums()
        got.update(psd=s.tobytes(), psd_n=ns, peak=p.tobytes(), peak_n=npk)
    return got


def test_measurements_on_views(CH):
    """Levels and block statistics on every view, spectrum and peak-hold spectrum on one, across retune and retune_all; and a rate meter
    that follows a view (RateMeter.write_from) reads what one that follows the twin reads."""
    from jaero_amd.ratemeter import RateMeter

    fs_c = 768000
    rng = np.random.default_rng(3)
    outs = [(48000.0, random_channels(CH, rng, 5, fs_c), CH.design_taps(16, ntaps=2049, beta=10.0)),
            (24000.0, random_channels(CH, rng, 3, fs_c), CH.design_taps(32, ntaps=2049, beta=10.0, fs_out=24000.0)),
            (12000.0, random_channels(CH, rng, 4, fs_c), CH.design_taps(64, ntaps=2049, beta=10.0, fs_out=12000.0))]
    sp, twins = make_pair(CH, fs_c, outs, 4 * HP)
    SPECTRA = 1  # the view that also keeps the spectrum and the peak-hold spectrum
    for g, (o, t) in enumerate(zip(sp.outputs, twins)):
        for c in (o, t):
            c.survey_enable(psd=g == SPECTRA, levels=True)
            c.activity_enable(peak=g == SPECTRA, blocks=True)
    sizes = [3 * HP + 17, HP - 17 + 5, 2 * HP + 100, 4 * HP, HP + 1]
    iq = rng.integers(-32768, 32768, size=(sum(sizes), 2)).astype(np.int16)
    pos = 0
    meter, tmeter = RateMeter(5, 48000.0), RateMeter(5, 48000.0)

    def compare(where):
        for g, (o, t) in enumerate(zip(sp.outputs, twins)):
            a, b = measurements(o, g == SPECTRA), measurements(t, g == SPECTRA)
            for k in a:
                assert a[k] == b[k], (where, g, k)

    for n in sizes[:3]:
        write_both(sp, twins, iq[pos:pos + n])
        assert meter.write_from(sp.outputs[0]) == tmeter.write_from(twins[0])
        pos += n
    before = pos // HP
    assert before == 6
    compare("three writes")
    assert measurements(sp.outputs[SPECTRA], True)["psd_n"] == before and sp.outputs[0].read_level_sums()[1].tolist() == [before] * 5
    # retune one channel of one view to another tune word; retune_all on another view: channels 0 and 2 move, 1 and 3 change gain only
    new = (CH.tune_word(-100000.3, float(fs_c)), CH.tune_word(1250.0, 48000.0), 0.25)
    assert new[0] != outs[0][1][2][0]
    moved = [list(c) for c in outs[2][1]]
    moved[0][0] = CH.tune_word(54321.0, float(fs_c))
    moved[2][0] = CH.tune_word(-222222.2, float(fs_c))
    moved[1][2], moved[3][2] = 0.5, 2.0
    sp.outputs[0].retune(2, *new); twins[0].retune(2, *new)
    sp.outputs[2].retune_all(moved); twins[2].retune_all(moved)
    for n in sizes[3:]:
        write_both(sp, twins, iq[pos:pos + n])
        assert meter.write_from(sp.outputs[0]) == tmeter.write_from(twins[0])
        pos += n
    after = pos // HP - before
    assert after == 5
    compare("behind the retunes")
    # only the retuned channels' counts restarted
    for reader in (lambda c: c.read_level_sums()[1].tolist(), lambda c: c.read_activity().n.tolist()):
        assert reader(sp.outputs[0]) == [before + after] * 2 + [after] + [before + after] * 2
        assert reader(sp.outputs[1]) == [before + after] * 3
        assert reader(sp.outputs[2]) == [after, before + after, after, before + after]
    assert sp.outputs[SPECTRA].read_psd_sums()[1] == sp.outputs[SPECTRA].read_peak_sums()[1] == before + after
    (R, nseg), (tR, tnseg) = meter.read(), tmeter.read()
    assert nseg == tnseg == (before + after) * sp.outputs[0].Mo // 4096 > 0 and R.tobytes() == tR.tobytes()
    close_all(sp, *twins, meter, tmeter)


# ---------------------------------------------------------------------------------------------- 4. one front end
def test_one_front_end(CH):
    """W writes that each complete a block: W forward transforms in all, none of them a view's, and W syntheses per view."""
    fs_c = 768000
    rng = np.random.default_rng(4)
    outs = [(48000.0, random_channels(CH, rng, 2, fs_c), None), (24000.0, random_channels(CH, rng, 3, fs_c), None),
            (12000.0, random_channels(CH, rng, 1, fs_c), None)]
    sp = CH.Splitter(fs_c, outs, max_write_iq=3 * HP)
    sp.profile_enable(True)
    sizes = [HP, HP + 5, 3 * HP, HP - 5, 2 * HP]
    iq = rng.integers(-32768, 32768, size=(sum(sizes), 2)).astype(np.int16)
    pos = 0
    for n in sizes:
        blocks = (pos + n) // HP - pos // HP
        assert blocks >= 1 and sp.write(iq[pos:pos + n]) == [blocks * o.Mo for o in sp.outputs]
        pos += n
    W = len(sizes)
    ms, launches = sp.profile_read(0)
    assert launches == W and ms > 0.0
    assert sp.profile_read(1)[1] == 0  # no capture: nothing is staged
    for o in sp.outputs:
        assert o.profile_read(0)[1] == 0
        assert o.profile_read(1)[1] == W
    assert sp.profile_read(0, reset=True)[1] == W and sp.profile_read(0)[1] == 0
    sp.close()


# ---------------------------------------------------------------------------------------------- 5. three banks from one capture
def three_class_capture(seconds=0.6):
    """fs_c = 3.072 MS/s: two 10.5 kbps OQPSK carriers, two 1200 bps and two 600 bps MSK carriers at distinct centres, each class generated
    at 0.1 / sqrt(3) of full scale (its own noise at Eb/N0 20 dB included) and summed: about 0.1 in all.  Returns (iq, classes); a class is
    (fb, fs_out, centres, LSB per unit amplitude, power of a unit carrier)."""
    from jaero_amd import signalgen as G

    fs_c = 3072000.0
    n = int(seconds * fs_c) // HP * HP
    rng = np.random.default_rng(5)
    plan = [(10500, 48000.0, [-400000.0, 250003.0]), (1200, 24000.0, [-1000000.7, 600000.0]), (600, 12000.0, [-50000.0, 1200000.3])]
    total = np.zeros((n, 2), np.int32)
    classes = []
    for fb, fs_out, centres in plan:
        bits = [rng.integers(0, 2, size=int(n / (fs_c / fb)) + 40, dtype=np.uint8) for _ in centres]
        kw = dict(fb=float(fb), ebno_db=20.0, rms=0.1 / np.sqrt(3.0), seed=fb, nsamples=n, return_info=True)
        iq, info = G.wideband_oqpsk(bits, centres, [1.0, 1.0], 64, **kw) if fb == 10500 else G.wideband_msk(bits, centres, [1.0, 1.0], fs_c, **kw)
        total += iq
        classes.append((fb, fs_out, centres, info["scale"], info["p_unit"]))
    assert np.abs(total).max() < 32768
    return total.astype(np.int16), classes


def test_three_banks_from_one_capture(CH):
    """Splitter.feed into an OQPSK bank at 48 kHz, an MSK 1200 bank at 24 kHz and an MSK 600 bank at 12 kHz against three stand-alone
    Channeliser.feed chains into three twin banks, cut the same way: every bank's soft bits and status are its twin's, and none is empty."""
    from jaero_amd import capi
    from jaero_amd import demodulator as B

    fs_c = 3072000
    iq, classes = three_class_capture()
    rms = np.sqrt(np.mean(iq.astype(float) ** 2) * 2) / 32768
    print(f"capture: {len(iq)} samples, RMS {rms:.3f} of full scale")
    assert 0.08 < rms < 0.12
    mw = 16 * HP
    outs, settings = [], []
    for fb, fs_out, centres, scale, p_unit in classes:
        audio_hz = {10500: 8000.0, 1200: 2000.0, 600: 1000.0}[fb]
        gain = 0.1 * 32768.0 / (scale * np.sqrt(p_unit / 2.0))  # the carrier's audio at 0.1 of full scale
        outs.append((fs_out, [(CH.tune_word(f, float(fs_c)), CH.tune_word(audio_hz, fs_out), gain) for f in centres], None))
        settings.append(B.OqpskSettings() if fb == 10500 else B.MskSettings(fb=float(fb), lockingbw=1.5 * fb, freq_center=audio_hz, Fs=fs_out))
    assert settings[0].Fs == 48000.0 and settings[0].fb == 10500.0
    sp, twins = make_pair(CH, fs_c, outs, mw)
    mk = lambda g: B.DemodulatorBank(settings[g], 2, max_write_samples=sp.nblk_max * sp.outputs[g].Mo, softbit_capacity=1 << 14)
    banks, tbanks = [mk(g) for g in range(3)], [mk(g) for g in range(3)]
    cuts, pos = [], 0
    for n in [5 * HP + 1, mw, 3 * HP - 1, 7, mw - 7] * 20:
        if pos >= len(iq):
            break
        cuts.append((pos, min(len(iq), pos + n)))
        pos = cuts[-1][1]
    for lo, hi in cuts:
        nout = sp.feed(banks, iq[lo:hi])
        assert nout == [(hi // HP - lo // HP) * o.Mo for o in sp.outputs]
        for g in range(3):
            assert twins[g].feed(tbanks[g], iq[lo:hi]) == nout[g]
    for g in range(3):
        assert sp.outputs[g].read_pcm().tobytes() == twins[g].read_pcm().tobytes()
        level = sp.outputs[g].read_pcm().astype(float).std(axis=1) / 32768
        print(f"output {g}: PCM RMS of the last write {level}")
        st, tst = banks[g].read_status_all(), tbanks[g].read_status_all()
        assert st.tobytes() == tst.tobytes(), g
        (rows, offs, taken), (trows, toffs, ttaken) = banks[g].read_all(capi.BANK_SOFTBITS), tbanks[g].read_all(capi.BANK_SOFTBITS)
        assert taken == ttaken == 2 and offs.tolist() == toffs.tolist() and rows.tobytes() == trows.tobytes(), g
        counts = np.diff(offs)
        print(f"bank {g} ({classes[g][0]} bps): soft bits per channel {counts.tolist()}, signal {st['signal'].tolist()}")
        assert (counts > 0).all(), (g, "a channel produced no soft bits")
    close_all(sp, *twins, *banks, *tbanks)


# ---------------------------------------------------------------------------------------------- 6. refusals that change nothing
def test_refusals_change_nothing(CH):
    from jaero_amd import capi
    from jaero_amd import demodulator as B

    fs_c = 768000
    rng = np.random.default_rng(6)
    mw = 2 * HP
    outs = [(48000.0, random_channels(CH, rng, 2, fs_c), CH.design_taps(16, ntaps=2049, beta=10.0)),
            (12000.0, random_channels(CH, rng, 3, fs_c), CH.design_taps(64, ntaps=2049, beta=10.0, fs_out=12000.0)),
            (48000.0, random_channels(CH, rng, 2, fs_c), CH.design_taps(16, cutoff_hz=20000.0, ntaps=2049, beta=10.0))]
    sp, twins = make_pair(CH, fs_c, outs, mw)
    L = sp.L
    iq = rng.integers(-32768, 32768, size=(12 * HP, 2)).astype(np.int16)
    pos = 0

    def good_write(n, where):
        nonlocal pos
        write_both(sp, twins, iq[pos:pos + n], where)
        pos += n

    good_write(HP + 11, "first")
    cap48, cap12 = sp.nblk_max * sp.outputs[0].Mo, sp.nblk_max * sp.outputs[1].Mo
    b48 = B.DemodulatorBank(B.OqpskSettings(), 2, max_write_samples=cap48, softbit_capacity=4096)
    b48b = B.DemodulatorBank(B.OqpskSettings(), 2, max_write_samples=cap48, softbit_capacity=4096)
    b12 = B.DemodulatorBank(B.MskSettings(fb=600.0, lockingbw=900.0, Fs=12000.0), 3, max_write_samples=cap12, softbit_capacity=4096)

    # on a view: the calls that consume input or own the handle
    v = sp.outputs[0]
    piece = iq[pos:pos + HP]
    n = C.c_int(-7)
    for fn, use in ((L.jaero_chan_write, b"jaero_split_write"), (L.jaero_chan3_write, b"jaero_split_write")):
        assert fn(v.h, piece.ctypes.data, HP, 0, None, C.byref(n)) == capi.E_INVAL
        assert use in L.jaero_last_error() and n.value == -7, L.jaero_last_error()
    for fn, use in ((L.jaero_chan_feed, b"jaero_split_feed"), (L.jaero_chan3_feed, b"jaero_split_feed")):
        assert fn(v.h, b48.h, piece.ctypes.data, HP, 0, None, C.byref(n)) == capi.E_INVAL
        assert use in L.jaero_last_error() and n.value == -7, L.jaero_last_error()
    first, buf = C.c_longlong(0), np.zeros((4, 2), np.float64)
    assert L.jaero_chan3_read_staged(v.h, buf.ctypes.data, 4, C.byref(n), C.byref(first)) == capi.E_INVAL
    L.jaero_chan_destroy(v.h)  # nothing happens: the view goes with its splitter
    again = C.c_void_p()
    assert L.jaero_split_output(sp.h, 0, C.byref(again)) == 0 and again.value == v.h.value  # the same pointer every time
    for call in (lambda: v.write(piece), lambda: v.feed(b48, piece), v.close):
        with pytest.raises(RuntimeError):
            call()
    good_write(HP, "behind the refusals on a view")

    # jaero_split_feed: every bank is checked against its output before anything advances
    def refused(banks, word):
        with pytest.raises(capi.JaeroError) as e:
            sp.feed(banks, iq[pos:pos + HP])
        assert e.value.code == capi.E_INVAL and "jaero_split_feed" in str(e.value) and word in str(e.value), str(e.value)

    other = B.DemodulatorBank(B.OqpskSettings(), 3, max_write_samples=cap48, softbit_capacity=4096)
    small = B.DemodulatorBank(B.OqpskSettings(), 2, max_write_samples=cap48 - 1, softbit_capacity=4096)
    for banks, word in (([other, b12, None], "channels"),          # the wrong channel count
                        ([b48, other, None], "Fs"),                # 3 channels as output 1 has, at 48 kHz for a 12 kHz output
                        ([None, b12, small], "max_write_samples"),
                        ([b48, b12, b48], "same bank")):
        refused(banks, word)
        good_write(HP - 1, f"behind the refusal of {word}")
    # a good feed; a None entry leaves that output produced and readable
    nout = sp.feed([b48, None, b48b], iq[pos:pos + mw])
    for g, t in enumerate(twins):
        assert t.write(iq[pos:pos + mw]) == nout[g] > 0
        assert sp.outputs[g].read_pcm().tobytes() == t.read_pcm().tobytes()
    b48.read_status(1), b48b.read_status(0)  # synchronise: the fed banks ran
    close_all(sp, *twins, b48, b48b, b12, other, small)
