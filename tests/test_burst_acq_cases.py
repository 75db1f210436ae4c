"""CPU: the host side of tests/test_gpu_burst_acq.py holds together without a GPU -- the oracle's stand-alone trident check is what its burst
demodulators run (the traced verdicts of the goldens' PCM, recomputed from the windows the demodulators saw), the oracle's own results and a
plain numpy restatement pass the shared checkers (tests/burst_acq_cases.py) on every case, the rejection caps hold, and the checkers fail on
each of the mistakes they exist to catch."""
from types import SimpleNamespace

import numpy as np
import pytest

import burst_acq_cases as BC
from conftest import load_golden

NDRAWS = BC.NDRAWS
NAMES = list(BC.CONFIGS)


@pytest.mark.parametrize("golden,kind,fb", [("burst_oqpsk_10k5_default", 3, 10500.0), ("burst_msk_1200_sample1_excerpt", 2, 1200.0)])
def test_stand_alone_trident_is_the_demodulators(oracle_mod, golden, kind, fb):
    """Every trident check of a traced run over a golden's PCM, recomputed by jo_trident from the window the demodulator ran it on (the
    tridentbuffer tap of the trace): the traced value is +-metric bit for bit, its sign is ok with the demodulator's state terms (burst MSK:
    dcd, cntr) applied, and an accepted check is followed by the frequency event the stand-alone result gives."""
    O = oracle_mod
    g = load_golden(golden)
    pcm = np.asarray(g["pcm"], dtype=np.int16)
    sett = O.burst_oqpsk_settings() if kind == 3 else O.burst_msk_settings(fb=fb)
    out = O.run_burst(sett, pcm, chunk=4096, trace=True)
    ev = out["events"]
    tri = ev[ev[:, 1] == 4]
    wins = out["trident_windows"]
    assert len(tri) == len(wins) >= 3 and wins.shape[1] == BC.CONFIGS["oqpsk" if kind == 3 else "msk1200"].tri_sz
    accepted = 0
    for row, w in zip(tri, wins):
        r, _, _ = O.trident(kind, 48000.0, fb, w)
        assert abs(row[2]) == r.metric, (golden, row)
        if row[2] > 0:
            accepted += 1
            assert r.ok == 1
            if kind == 3:  # mixer2.SetFreq(freq) and the Plottables emission at the same sample
                assert np.any((ev[:, 0] == row[0]) & (ev[:, 1] == 2) & (ev[:, 2] == r.freq)), (golden, row, r.freq)
        elif kind == 3:
            assert r.ok == 0  # burst OQPSK has no state terms
    assert accepted >= 1, "the golden holds at least one burst"


@pytest.mark.parametrize("name", NAMES)
def test_oracle_and_numpy_pass_the_trident_checker(oracle_mod, name):
    """The rejection cap (population asserts it), the oracle against its own bound, and numpy's transforms as a second right candidate"""
    cfg = BC.CONFIGS[name]
    cases, E, rejected = BC.population(oracle_mod, name, NDRAWS)
    assert rejected * 20 <= max(20, NDRAWS + rejected)
    worst = [0.0, 0.0, 0.0]
    for c in cases + BC.deliberate_cases(oracle_mod, name):
        BC.check_trident(c, c.oracle, E, "the oracle itself")
        errs = BC.check_trident(c, BC.numpy_trident(cfg, c.window), E, "numpy restatement")
        worst = [max(a, b or 0.0) for a, b in zip(worst, errs)]
    print(f"burst_acq {name}: numpy restatement's worst errors: metric {worst[0] / BC.EPS:.2f} eps, vol_gain {worst[1] / BC.EPS:.2f} eps, phase {worst[2] / BC.EPS:.2f} eps")


def test_deliberate_cases_are_what_they_claim(oracle_mod):
    """The properties the deliberate cases exist for, on the oracle's results"""
    O = oracle_mod
    for name in NAMES:
        cfg, by = BC.CONFIGS[name], {c.label: c for c in BC.deliberate_cases(O, name)}
        z = by["all-zero window"]
        assert (z.oracle.ok, z.oracle.freq, z.oracle.metric, z.oracle.phase_deg) == (0, 0.0, 0.0, by["zero base, live top"].oracle.phase_deg) and np.isinf(z.oracle.vol_gain)
        assert by["level 0.05: metric well below 500"].oracle.metric < 350.0 and by["level 0.05: metric well below 500"].oracle.ok == 0
        assert by["single sample at index 0"].adm.decided and by["single sample at index 0"].adm.margin == 0.0  # an exact tie: the first bin wins
        assert by["single sample at index 0"].adm.base == [0]
        assert not by["single sample at the base part's last index"].adm.decided  # 16384 bins equal up to rounding
        live = [c for c in BC.deliberate_cases(O, name) if "tones" in c.label or "bins above" in c.label]
        assert [c.oracle.ok for c in live] == [1, 0] and all(c.adm.accepted for c in live)
        if not cfg.oq:
            assert by["base peak below bin 50 + psb / 2"].adm.top[0] == 0
        if cfg.nb > 8192:
            assert by["single sample at index 8192 of the base part"].oracle.metric == 100.0


WRONG = [("oqpsk", "last_max", "all-zero window"), ("oqpsk", "shift1", None), ("msk1200", "shift1", None), ("msk600", "shift1", None),
         ("msk600", "nofold", None), ("msk600", "nofold", "single sample at index 8192 of the base part"),
         ("msk600", "sign_r1", "bin-centred carrier at bin 1365 = 4 * 341 + 1")]


@pytest.mark.parametrize("name,wrong,label", WRONG)
def test_wrong_trident_candidates_fail(oracle_mod, name, wrong, label):
    """last maximum instead of first, a window read one sample late, the MSK 600 fold dropped, the (-j)^r factor of one residue class negated:
    each must fail the checker (on the case named, or on the first draw)"""
    cfg = BC.CONFIGS[name]
    cases, E, _ = BC.population(oracle_mod, name, NDRAWS)
    c = cases[0] if label is None else {x.label: x for x in BC.deliberate_cases(oracle_mod, name)}[label]
    BC.check_trident(c, BC.numpy_trident(cfg, c.window), E)
    with pytest.raises(AssertionError):
        BC.check_trident(c, BC.numpy_trident(cfg, c.window, wrong), E)


def test_skipped_event_fails_the_list_checker(oracle_mod):
    cases, _, _ = BC.population(oracle_mod, "oqpsk", NDRAWS)
    expected = {ch: cases[ch % len(cases)].oracle for ch in (5, 0, 64, 63)}
    listed = [5, 0, 64, 63]
    BC.check_event_list(listed, [expected[ch] for ch in listed], 4, expected)
    sentinel = SimpleNamespace(ok=-1515870811, freq=-1.1, phase_deg=-1.1, vol_gain=-1.1, metric=-1.1)
    with pytest.raises(AssertionError):  # one event of the list skipped: its entry keeps the sentinel
        BC.check_event_list(listed, [expected[5], expected[0], sentinel, expected[63]], 3, expected)
    with pytest.raises(AssertionError):  # the results written, but one more entry of the bank touched
        BC.check_event_list(listed, [expected[ch] for ch in listed], 5, expected)
    with pytest.raises(AssertionError):  # two channels' results exchanged
        BC.check_event_list(listed, [expected[0], expected[5], expected[64], expected[63]], 4, expected)


@pytest.fixture(scope="module")
def hilbert_stream(oracle_mod):
    """Six channels (0 .. 3 live, 4 silent beside live 5 ... and a seventh, silent, whose partner is padding) through the oracle in the GPU
    tests' write sizes, with the exact sum of four of them"""
    O = oracle_mod
    sizes = BC.hilbert_sizes(4096, 19000)[:-1]
    n = sum(sizes)
    pcm = BC.fullscale_pcm(7, n, 0x41B, silent=(4, 6))
    orc = BC.oracle_hilbert(O, pcm, sizes)
    exact = {c: BC.exact_hilbert(O, pcm[c]) for c in (0, 1, 4, 5)}
    return pcm, orc, exact


def test_oracle_passes_the_hilbert_checker(hilbert_stream):
    pcm, orc, exact = hilbert_stream
    rows, _ = BC.check_hilbert(orc, orc, exact, "oracle")
    assert not orc[6].any() and not orc[4].any()  # the oracle filters channel by channel: its silent channels are zeros whoever sits beside them
    leak = orc.copy()
    leak[4, 7000:] = 2.0 ** -52 * orc[5, 7000:]  # the kernel's silent channel beside a live partner holds the partner's rounding: under the pair's bound
    BC.check_hilbert(leak, orc, exact, "a silent channel beside a live one")
    assert dict((r[0], r[1]) for r in rows)[6] == "both silent"


def test_wrong_hilbert_candidates_fail(hilbert_stream):
    """the pair's outputs swapped; one 2048-sample block taken from the block before"""
    pcm, orc, exact = hilbert_stream
    swapped = orc.copy()
    swapped[[0, 1]] = orc[[1, 0]]
    with pytest.raises(AssertionError):
        BC.check_hilbert(swapped, orc, exact, "swapped")
    swapped = orc.copy()
    swapped[[2, 3]] = orc[[3, 2]]  # a pair without an exact sum
    with pytest.raises(AssertionError):
        BC.check_hilbert(swapped, orc, exact, "swapped, oracle only")
    off = orc.copy()
    off[:, 8192:10240] = orc[:, 6144:8192]
    with pytest.raises(AssertionError):
        BC.check_hilbert(off, orc, exact, "block offset by 2048")
    leak = orc.copy()
    leak[6, 9000] = 1e-300
    with pytest.raises(AssertionError):
        BC.check_hilbert(leak, orc, exact, "a silent pair that is not zero")
