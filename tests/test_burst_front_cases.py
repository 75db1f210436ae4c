"""CPU: the case generator of tests/burst_front_cases.py against the oracle alone -- the geometry it restates, every poked peak-detector case's
triggers and winners, a numpy restatement of the detector passing and four deliberately wrong ones failing, the streaming draws' rejection cap and
decision clearances, jo_burst_front_write against the pinned jo_burst_write, and the k_ev_compact cases.  tests/test_gpu_burst_front.py runs the
same cases on the kernels."""
import numpy as np
import pytest

import burst_front_cases as FC


@pytest.mark.parametrize("name", list(FC.CONFIGS))
def test_geometry_matches_the_oracle(oracle_mod, name):
    cfg = FC.CONFIGS[name]
    g = FC.geometry(cfg)
    og = oracle_mod.BurstDemod(FC.oracle_settings(oracle_mod, cfg)).front_geom()
    assert (g.agc_len, g.ma1_len, g.mav1_len, g.PL, g.pd_thr, g.tri_sz) == (og["agc_len"], og["ma1_len"], og["mav1_len"], og["PL"], og["pd_thr"], og["tri_sz"])
    assert (g.bt_lag, g.fa_lag) == (int(np.ceil(og["bt_delay"])), int(np.ceil(og["fa_delay"])))


@pytest.mark.parametrize("name", list(FC.CONFIGS))
def test_peak_detector_cases(oracle_mod, name):
    """Every scenario: the oracle triggers where and with the winner each case was built for; the numpy restatement agrees with jo_peakdet_run on
    every segment; each wrong detector disagrees on at least one scenario.  The set covers a first maximum in every lane 0 .. 63 and in strides > 0."""
    scs = FC.scenarios(name)
    lanes, caught = set(), {w: [] for w in ("last_max", "lane_order", "stale", "ge_thr")}
    for sc in scs:
        exp = FC.expected(oracle_mod, sc)
        FC.check_coverage(sc, exp)
        lanes |= {mp % 64 for ph in exp for e in ph for t in e.trig.values() for _, mp in t if mp >= 64}
        key = lambda x: [[(e.ev_list, e.fires, {c: vars(s) for c, s in e.st.items()}) for e in ph] for ph in x]
        assert key(FC.expected(oracle_mod, sc, FC.numpy_peakdet(sc.g))) == key(exp), (name, sc.label, "the numpy restatement of the detector")
        for w in caught:
            if key(FC.expected(oracle_mod, sc, FC.numpy_peakdet(sc.g, w))) != key(exp):
                caught[w].append(sc.label)
    print(f"burst_front {name}: {len(scs)} scenarios; wrong detectors caught by: " + "; ".join(f"{w}: {len(v)}" for w, v in caught.items()))
    assert lanes == set(range(64)), sorted(set(range(64)) - lanes)
    assert all(caught.values()), caught


@pytest.mark.parametrize("name", list(FC.CONFIGS))
def test_streaming_draws(oracle_mod, name):
    """The rejection cap (inside population), the smallest clearance, at least one trigger per configuration, and no trigger whose winner is the entry
    written on the trigger sample or the one before it (module docstring of burst_front_cases: there is none to find)."""
    draws, E, rejected = FC.population(oracle_mod, name)
    assert len(draws) == FC.NDRAWS and all(sc.margin > FC.MARGIN for sc in draws)
    g = draws[0].g
    assert draws[0].n >= g.agc_len + 2 * g.ma1_len
    trig = np.concatenate([t for sc in draws for t in sc.trig.values()])
    assert len(trig) >= 1 and trig[:, 1].max() < 2 * g.PL - 1
    for sc in draws:
        for ch in sc.z:
            fires = np.flatnonzero(sc.rows[ch][:, sc.cols["fire"]])
            assert np.array_equal(fires, np.flatnonzero(sc.exact[ch][:, sc.cols["fire"]] != 0)), (name, ch, "the double and the exact run fire on different samples")
            assert np.array_equal(fires, sc.trig[ch][:, 0] + sc.trig[ch][:, 1]) or len(fires) < len(sc.trig[ch]), (name, ch)


@pytest.mark.parametrize("name", list(FC.CONFIGS))
def test_front_write_is_the_front_of_burst_write(oracle_mod, name):
    """jo_burst_front_write on oracle.hilbert_stream's output fires on the samples jo_burst_write logs its PEAK events on (trace), a live
    setSettings in mid-stream included: the stand-alone front end is the one tests/test_oracle_vs_ref.py pins."""
    O = oracle_mod
    cfg = FC.CONFIGS[name]
    g = FC.geometry(cfg)
    rng = np.random.default_rng(7)
    n = 3 * g.ma1_len + 30000
    t = np.arange(n)
    x = 300.0 * rng.standard_normal(n)
    s = 9000
    x[s:s + 2 * g.ma1_len] += 9000.0 * np.cos(2 * np.pi * 0.09 * t[s:s + 2 * g.ma1_len])
    pcm = np.rint(x).astype(np.int16)
    st = FC.oracle_settings(O, cfg)
    a, b = O.BurstDemod(st, trace=True), O.BurstDemod(st, trace=True)
    cut = s + g.ma1_len // 2
    a.write(pcm[:cut]); a.set_settings(st); a.write(pcm[cut:])  # setSettings restarts the Hilbert filter too
    r1 = b.front_write(O.hilbert_stream(pcm[:cut], chunk=cut)[0])
    b.set_settings(st)
    r2 = b.front_write(O.hilbert_stream(pcm[cut:], chunk=n - cut)[0])
    ev = a.take_events()
    peaks = ev[ev[:, 1] == 3][:, 0].astype(np.int64)
    fires = np.flatnonzero(np.concatenate([r1, r2])[:, 3])
    assert len(peaks) >= 1 and np.array_equal(peaks, fires), (name, peaks, fires)
    evb = b.take_events()
    assert np.array_equal(evb[evb[:, 1] == 3][:, 0].astype(np.int64), fires)


def test_ev_compact_cases():
    rng = np.random.default_rng(3)
    for ng in FC.EV_NGROUPS:
        for label, m in FC.ev_masks(ng, rng):
            assert m.dtype == np.uint64 and m.shape == (ng,)
            want = FC.ev_expected(m)
            assert len(want) == sum(bin(int(x)).count("1") for x in m) and np.all(np.diff(want) > 0), (ng, label)
            assert all((int(m[int(c) >> 6]) >> (int(c) & 63)) & 1 for c in want[:50])
