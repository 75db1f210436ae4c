"""GPU (-m gpu): k_oqpsk_fb's queued output halves -- what a channel emits must not depend on where the launches of a stream begin and end.

The back half of the sample loop queues the output half of a symbol (averages, residual rotation, MSE, soft bits) per lane and runs the queue for
all lanes together at every FB_DEFER-th sample of a launch, and drains it at the end of a launch.  A stream cut into launches of 1, 7, 8, 9, 15,
17, 64 and 4096 samples puts batch points and the end-of-launch drain at every position relative to a lane's symbols; the outputs -- soft bits,
captured symbols, status log -- must be bit-identical to those of the same stream written whole.  96 channels (a full channel group and a ragged
one) carry 10.5 kbps / 8400 bps signals at distinct symbol-clock phases; four of them carry noise only and never lock, so lanes whose queue
stays idle sit next to locked ones.  Oracle parity of both ways of writing at the same sizes goes through test_gpu_parity.compare.
At 8400 bps the bit-identity does not hold with or without the queue (the prefilter in front of the loop works write by write; the commit
before this test existed differs between the two ways of writing as well), so there each way of writing is compared with the oracle.

Both banks first take the same PRE whole writes (the loops lock there, the coarse estimator's ring fills), then the section that is split."""
import functools

import numpy as np
import pytest

import kernel_variants as KV
from test_gpu_parity import compare
from test_gpu_variants import sample_loop_layout  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

NCH = 96  # channel groups of 64 and 32 lanes
NOISE = (5, 62, 64, 95)  # noise only: never lock
CHUNK = 4096
PRE = {10500.0: 5 * CHUNK, 8400.0: 10 * CHUNK}  # written whole to both banks: past the coarse estimator's 2^14-sample ring, the loops in lock
SPLIT = 6200  # the section written whole (4096 + 2104) or cut
SMALL = [7, 1, 64, 9, 8, 17, 15, 1, 8, 64, 15, 7, 17, 9]  # cycled around one 4096-sample launch
ORACLE_CHANNELS = (0, 5, 31, 63, 64, 77, 95)  # locked and noise-only lanes of both groups


def nsamp(fb):
    return PRE[fb] + SPLIT


def split_sizes():
    """The split section's launches: small ones in a fixed mixed order, the 4096-sample one after the first 40 of them."""
    out, s, k = [], 0, 0
    while s < SPLIT:
        m = CHUNK if k == 40 else SMALL[k % len(SMALL)]
        m = min(m, SPLIT - s)
        out.append(m)
        s += m
        k += 1
    assert {1, 7, 8, 9, 15, 17, 64, CHUNK} <= set(out)
    return out


def whole_sizes(fb):
    return [CHUNK] * (PRE[fb] // CHUNK) + [CHUNK, SPLIT - CHUNK]


def cut_sizes(fb):
    return [CHUNK] * (PRE[fb] // CHUNK) + split_sizes()


@functools.lru_cache(maxsize=None)
def signals(fb):
    """[NCH, N] int16: channel c's symbol clock starts c samples late (a symbol pair is 9.14 / 11.4 samples), carriers a few Hz apart."""
    from jaero_amd import signalgen as G

    rows, N = [], nsamp(fb)
    for c in range(NCH):
        seed = G.SEED_BASE + 9100 + c + (1000 if fb == 8400.0 else 0)
        if c in NOISE:
            rows.append(np.clip(np.random.default_rng(seed).normal(0.0, 2000.0, N), -32767, 32767).astype(np.int16))
        else:
            rows.append(G.oqpsk(N, fb=fb, fc=8000.0 + 3.0 * (c % 7 - 3), ebno_db=14.0, seed=seed, start_sample=c)[0])
    return np.stack(rows)


def settings(fb):
    from jaero_amd import demodulator as D
    from oracle import oracle as O

    return (D.OqpskSettings(freq_center=8000.0, lockingbw=fb, fb=fb, Fs=48000.0, coarsefreqest_fft_power=14, signalthreshold=0.65),
            O.oqpsk_settings(freq_center=8000.0, lockingbw=fb, fb=fb, Fs=48000.0, power=14, threshold=0.65))


def run_bank(fb, layout, set_layout, sizes):
    """Outputs of every channel for the stream written in launches of `sizes`: (kernel name, [(soft, symbols, log)] per channel)."""
    from jaero_amd import demodulator as D

    set_layout(layout)
    bank = D.DemodulatorBank([settings(fb)[0]] * NCH, ebno=False, status_log=True, capture_symbols=True, max_write_samples=CHUNK,
                             softbit_capacity=nsamp(fb))
    try:
        name = bank.kernel_variant(0)
        pcm, s = signals(fb), 0
        for m in sizes:
            bank.write(pcm[:, s:s + m])
            s += m
        assert s == nsamp(fb)
        return name, [(bank.read_softbits(c), bank.read_symbols(c), bank.read_status_log(c)) for c in range(NCH)]
    finally:
        bank.close()


@functools.lru_cache(maxsize=None)
def oracle_run(fb, cut, c):
    from oracle import oracle as O

    return O.run_demod(settings(fb)[1], signals(fb)[c], chunk=cut_sizes(fb) if cut else whole_sizes(fb), capture_symbols=True)


@pytest.mark.parametrize("family,layout", [("oqpsk_10500", 1), ("oqpsk_10500", 2), ("oqpsk_8400", 1), ("oqpsk_8400", 2)])
def test_outputs_do_not_depend_on_where_launches_end(oracle_mod, sample_loop_layout, family, layout):  # noqa: F811
    fb = KV.FAMILIES[family]["fb"]
    want = KV.find(family, False, True, layout).kernel0
    name_w, whole = run_bank(fb, layout, sample_loop_layout, whole_sizes(fb))
    name_c, cut = run_bank(fb, layout, sample_loop_layout, cut_sizes(fb))
    assert name_w == want and name_c == want, (name_w, name_c, want)
    nsoft = nsym = 0
    for c in range(NCH):
        (sw, yw, lw), (sc, yc, lc) = whole[c], cut[c]
        if family == "oqpsk_10500":
            assert np.array_equal(sw, sc), f"channel {c}: soft bits differ between whole and cut writes"
            assert yw.shape == yc.shape and np.array_equal(yw.view(np.int64), yc.view(np.int64)), f"channel {c}: captured symbols differ"
            assert lw.shape == lc.shape and np.array_equal(lw.view(np.int64), lc.view(np.int64)), f"channel {c}: status log differs"
        else:
            # 8400 bps: the prefilter in front of the loop works write by write (an FFT filter, re-mixed per write from a saved phase), so the
            # doubles depend on the write sizes with or without the queue; each way of writing is held to the oracle below
            assert yw.shape == yc.shape and lw.shape == lc.shape, f"channel {c}: symbol or estimate counts differ"
        if c not in NOISE:
            nsoft += len(sw)
            nsym += len(yw)
    # a symbol pair is 2 Fs / fb samples, and the locked channels emitted soft bits through most of the stream
    assert nsym > 0.98 * (NCH - len(NOISE)) * (nsamp(fb) * fb / 2 / 48000.0) and nsoft > (NCH - len(NOISE)) * 1000, (nsym, nsoft)
    # oracle parity of both ways of writing, locked and noise-only lanes (at 8400 bps this is the check, so it takes every fourth channel too)
    for c in sorted(set(ORACLE_CHANNELS) | (set(range(2, NCH, 4)) if family == "oqpsk_8400" else set())):
        for outs, is_cut in ((whole, False), (cut, True)):
            try:
                compare(*outs[c], oracle_run(fb, is_cut, c), check_ebno=False)
            except AssertionError as e:
                raise AssertionError(f"{family} layout {layout} channel {c} {'cut' if is_cut else 'whole'}: {e}") from e
