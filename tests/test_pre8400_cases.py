"""CPU: the host side of tests/test_gpu_pre8400.py holds together without a GPU -- the oracle's stand-alone prefilter object is the prefilter
of the oracle's demodulator (which tests/test_oracle_vs_ref.py pins to the unmodified reference), the oracle's own output passes the shared
checker on every case's input, and the checker fails on each of the errors it exists to catch."""
import numpy as np
import pytest

import pre8400_cases as PC


def run_model(O, pcm, sizes, fsums=None, restarts=()):
    """One channel through a Model in the given writes; fsums[k]: the sum found at write k; restarts: indices of writes in front of which the
    prefilter restarts"""
    m = PC.Model(O)
    s = 0
    for k, n in enumerate(sizes):
        if k in restarts:
            m.restart()
        m.write(pcm[s:s + n], None if fsums is None else fsums[k])
        s += n
    return m


def test_stand_alone_object_is_the_demodulators_prefilter(oracle_mod):
    """jo_pre8400_* fed the PCM and, write by write, the mixer2_freq_sum a run_demod of an 8400 bps signal reported: its output is the
    demodulator's cval_prefiltered bit for bit, its oscillator ends every write at the demodulator's frequency."""
    from jaero_amd import signalgen as G

    O = oracle_mod
    n = 61000
    pcm, _ = G.oqpsk(n, fb=8400.0, fc=7985.0, ebno_db=10.0, seed=G.SEED_BASE + 8421)
    sizes = PC.cycle_sizes([700, 3100, 4096, 50, 2048, 1, 513, 2047], n)
    ref = O.run_demod(O.oqpsk_settings(fb=8400.0, lockingbw=8400.0), pcm, chunk=sizes, capture_prefiltered=True)
    assert len(ref["prefiltered"]) == n >= 60000 and sum(ref["write_sizes"]) == n and len(set(ref["write_sizes"])) >= 8
    assert len(ref["soft"]) > 1000 and np.ptp(ref["pre_freq"]) > 0.0  # it locked, and the prefilter's oscillator moved with it
    p = O.Pre8400()
    out, s = [], 0
    for k, m in enumerate(ref["write_sizes"]):
        out.append(p.write(pcm[s:s + m])[1])
        p.end_of_write(ref["pre_freq_sum"][k], m)
        assert p.state[1] == ref["pre_freq"][k] * PC.WT / 48000.0
        s += m
    PC.check_bits(np.concatenate(out), ref["prefiltered"], "stand-alone object against the demodulator's capture")


@pytest.fixture(scope="module")
def streams(oracle_mod):
    """The kinds of input the GPU tests use, through the oracle: name -> (models of up to four channels, exact sums)"""
    O = oracle_mod
    out = {}
    # ragged writes over more than two ring lengths, three full-scale channels and one silent one (the zero channel of a four-channel group)
    sizes = PC.cycle_sizes(PC.FILTER_CYCLE, 36000)
    pcm = PC.fullscale_pcm(4, sum(sizes), 0x8400, zero_channel=2)
    out["ragged"] = [run_model(O, pcm[c], sizes) for c in range(4)]
    # the frequencies, previous write length never the current one
    sizes = [2047, 2048, 513, 4096, 700, 3100]
    pcm = PC.fullscale_pcm(4, sum(sizes), 0x8401)
    out["frequencies"] = [run_model(O, pcm[c], sizes, [0.0] + [PC.freq_sum(PC.FREQS[(c + k) % 5], c, k, sizes[k - 1]) for k in range(1, len(sizes))])
                          for c in range(4)]
    # restarts at moments that are no multiples of 2048, twice within 2048 samples
    sizes = [3000, 1111, 700, 3100, 4096, 2048, 2500]
    pcm = PC.fullscale_pcm(2, sum(sizes), 0x8402)
    out["restart"] = [run_model(O, pcm[0], sizes, restarts=(1, 5)), run_model(O, pcm[1], sizes, restarts=(2, 3))]
    # 7000 samples of digital silence in the middle of a full-scale channel
    sizes = PC.cycle_sizes([4096], 20000)
    pcm = PC.fullscale_pcm(1, sum(sizes), 0x8403)
    pcm[0, 5000:12000] = 0
    out["silence"] = [run_model(O, pcm[0], sizes)]
    pcm = PC.fullscale_pcm(1, sum(sizes), 0x8403)
    pcm[0, 4096:12288] = 0  # whole transform blocks, as tests/test_gpu_pre8400.py::test_exact_zeros_and_channel_isolation has it
    out["silence_aligned"] = [run_model(O, pcm[0], sizes)]
    return {k: (v, [PC.exact_prefilter(O, m) for m in v]) for k, v in out.items()}


def test_oracle_alone_meets_every_condition(oracle_mod, streams):
    """The oracle as candidate passes; its own error against the exact sum is round-off of a 4096-point fp64 transform pair (a mis-indexed exact
    sum, or one that forgot a restart, would show as an error of order one)."""
    for name, (models, exacts) in streams.items():
        worst = 0.0
        for c, (m, ex) in enumerate(zip(models, exacts)):
            o = m.all_out()
            if not o.any():
                assert not np.any(ex[0]) and not np.any(ex[1]) and not m.all_down().any()
                PC.check_zeros(o, o)
                continue
            e_c, e_o = PC.check_filtered(o, o, exact=ex, what=(name, c))
            # 12 butterfly stages there and back, each within 2^-53 relative: well inside 64 * 2^-52 of the peak
            assert 0.0 < e_o < 64 * PC.EPS, (name, c, e_o / PC.EPS)
            worst = max(worst, e_o)
            assert not o[:PC.L].any() and o[PC.L:PC.L + 8].all()
            for r in m.restarts:
                assert not o[r:r + PC.L].any() and (o[r + PC.L] != 0 or any(r < q <= r + PC.L for q in m.restarts))
        for c, m in enumerate(models):
            o = m.all_out()
            if o.any():
                PC.check_filtered(o, o, e_oracle_worst=worst, what=(name, c))
    # parts that are 0.0 beside a part that is not (pre8400_cases: no zeros of the filter) occur, and only in writes at 0 Hz
    half = 0
    for m in streams["frequencies"][0]:
        for k, o in enumerate(m.out):
            h = int(((o.real == 0) ^ (o.imag == 0)).sum())
            assert h == 0 or len(set(m.upidx[k])) == 1, (k, h)
            half += h
    assert half > 0
    sil = streams["silence"][0][0].all_out()
    assert not sil[10240:12288].any() and sil[10239] != 0 and sil[12288] != 0  # input blocks 3 and 4 (samples 6144 .. 10239) are all silence
    # Silence that does not cover whole blocks: at samples 9096 .. 10 239 and 12 288 .. 14 047 no tap reaches a non-zero sample -- the exact
    # output is 0 -- but a block that is not all silence contributes, and the oracle's output there is its transform's round-off, some of it
    # 0.0 by chance.  No other transform can be asked to repeat those, so the GPU test's silence covers whole blocks: every zero of the oracle
    # is then one of structure, and the outputs next to them are tap-sized, far above round-off.
    ex = streams["silence"][1][0]
    for a, b in ((9096, 10240), (12288, 14048)):
        assert not np.any(ex[0][a:b]) and not np.any(ex[1][a:b])
        assert sil[a:b].any() and np.abs(sil[a:b]).max() < 1e-15
    al = streams["silence_aligned"][0][0].all_out()
    z = np.flatnonzero(al[PC.L:] == 0) + PC.L
    assert z[0] == 8192 and z[-1] == 14335 and len(z) == 14336 - 8192
    assert np.abs(al[[8191, 14336]]).min() > 1e-12


def wrong_candidates(models):
    """name -> (channel, candidate) built from the oracle's output of the `ragged` stream"""
    o = [m.all_out() for m in models]
    out = {}
    a = o[0].copy()
    b = 3800 + 512  # the third write (4096 samples, stretches of 512) starts at sample 3800: the boundary between its first two stretches
    a[b - 1], a[b] = o[0][b], o[0][b - 1]
    out["a sample moved by one place at a stretch boundary"] = (0, a)
    a = o[0].copy()
    a[PC.L - 1] = complex(3e-17, -1e-17)
    out["the hold one sample short"] = (0, a)
    out["1e-9 of the LDS neighbour"] = (0, o[0] + 1e-9 * o[1])
    a = o[1].copy()
    a[3 * PC.L:4 * PC.L] *= 1.0 + 1e-10
    out["one block scaled by 1 + 1e-10"] = (1, a)
    a = o[2].copy()  # the silent channel
    a[12345] = complex(0.0, 1e-19)
    out["round-off in place of an exact zero"] = (2, a)
    return out


def test_checker_fails_on_each_wrong_candidate(oracle_mod, streams):
    models, exacts = streams["ragged"]
    worst = max(PC.err_vs_exact(m.all_out(), ex) for m, ex in zip(models, exacts) if m.all_out().any())
    cands = wrong_candidates(models)
    assert len(cands) == 5
    for name, (c, cand) in cands.items():
        o = models[c].all_out()
        assert not np.array_equal(cand.view(np.uint64), o.view(np.uint64)), name
        if o.any():
            with pytest.raises(AssertionError):
                PC.check_filtered(cand, o, exact=exacts[c], what=name)
        with pytest.raises(AssertionError):
            PC.check_filtered(cand, o, e_oracle_worst=worst, what=name)
    # the same displaced sample in the mix, and a pointer one ulp away
    d = models[0].all_down()
    bad = d.copy()
    bad[3800 + 512 - 1], bad[3800 + 512] = d[3800 + 512], d[3800 + 512 - 1]
    with pytest.raises(AssertionError):
        PC.check_bits(bad, d)
    with pytest.raises(AssertionError):
        PC.check_bits(np.array([np.nextafter(models[0].state[0], 0.0)]), np.array([models[0].state[0]]))
    PC.check_bits(d, d.copy())
    # the hold one sample short behind a restart
    (m0, _), (ex0, _) = streams["restart"]
    o = m0.all_out()
    r = m0.restarts[1]
    assert r % PC.L and (m0.restarts[0] % PC.L)
    a = o.copy()
    a[r + PC.L - 1] = complex(2e-17, 2e-17)
    with pytest.raises(AssertionError):
        PC.check_filtered(a, o, exact=ex0)
    a = o.copy()
    a[r + PC.L] = 0.0  # and one sample long: an output of order one missing
    with pytest.raises(AssertionError):
        PC.check_filtered(a, o, exact=ex0)


def test_case_generators():
    assert all(n < 512 for n in PC.SEQ_SMALL) and all(n >= 512 for n in PC.SEQ_LARGE)
    assert {n % 8 for n in PC.SEQ_LARGE} >= {0, 1, 7} and max(PC.SEQ_LARGE) == 4096
    pcm = PC.fullscale_pcm(5, 100, 1, zero_channel=4)
    assert pcm.min() == -32768 and pcm.max() == 32767 and not pcm[4].any() and pcm[:4].any(axis=1).all()
    sizes = PC.cycle_sizes(PC.FILTER_CYCLE, 36000)
    assert 36000 <= sum(sizes) <= PC.MAX_EXACT_SAMPLES and sum(sizes) > 2 * 16384
    for kind in PC.FREQS:
        f = PC.freq_sum(kind, 2, 3, 777) / 777
        assert (f == 0.0) if kind == "zero" else (f < 0) if kind == "negative" else 0 < f < 24000.0
    k = PC.freq_sum("integer_step", 2, 3, 777) / 777 * PC.WT / 48000.0
    assert abs(k - round(k)) < 1e-11 and round(k) == 3000 + 34 + 3
