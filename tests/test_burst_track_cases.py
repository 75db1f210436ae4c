"""CPU: the cases of tests/burst_track_cases.py against the oracle alone -- the split of boqpsk_write / bmsk_write pinned by record and replay,
the zero-input cases independent of the segmentation, the coverage and decision robustness of the recorded streams, and the checkers on
deliberately wrong candidates.  tests/test_gpu_burst_track.py runs the same cases on the kernels."""
import numpy as np
import pytest

import burst_track_cases as TC

NAMES = list(TC.CONFIGS)
NDRAWS = 10


def equal_runs(a, b):
    return (np.array_equal(a.soft, b.soft) and np.array_equal(a.events, b.events) and np.array_equal(a.symbols, b.symbols) and
            all(np.array_equal(a.states[-1][k], b.states[-1][k]) for k in a.states[-1]))


@pytest.mark.parametrize("name", NAMES)
def test_track_write_replays_an_ordinary_run_bit_for_bit(oracle_mod, name):
    """val_to_demod of every sample and every trident result, recorded from jo_burst_write on a generated burst pair and fed through
    jo_burst_track_write on a fresh object in three segmentations: soft bits (pending tail included), events, symbols and every scalar of
    jo_burst_track_state equal to the ordinary run's, bit for bit."""
    O = oracle_mod
    S = TC.STREAMS[name]
    for k in (0, 2):
        val, ver, run = TC.recorded(O, name, k, TC.STREAM_SEEDS[name] + k)
        assert len(val) == S["total"] and sum(v[0] for _, v in ver) >= (2 if k == 0 else 1), (name, k, "the bursts must be accepted (at the low Eb/N0: one)", ver)
        keep = [[a for a, _ in ver]]
        for sizes, group in ((TC.ROTATION, 2), ((TC.MAXSEG,), 1), ((997, 3), 3)):
            c = TC.case(name, f"replay {sizes}", TC.plan_writes(len(val), sizes=sizes, group=group, keep_apart=keep), {0: ver}, vals={0: val}, capsym=True)
            e = TC.expected(O, c, 0)
            assert np.array_equal(e.soft, run.soft), (name, k, sizes, "soft")
            assert np.array_equal(e.events, run.events), (name, k, sizes, "events")
            assert np.array_equal(e.symbols, run.symbols) and len(run.symbols) > 100, (name, k, sizes, "symbols")
            last = e.states[-1]
            for f, v in run.state.items():
                assert np.array_equal(last[f], v), (name, k, sizes, f, last[f], v)
            assert e.cov == run.cov


@pytest.mark.parametrize("name", NAMES)
def test_zero_input_cases_do_not_depend_on_the_segmentation(oracle_mod, name):
    """Every Part A case on +0.0 input: the oracle's result under the case's writes equals its result with every segment a write of its own (squelch
    off: lastmse is the one thing a write boundary changes) and passes check_exact as its own candidate; soft bytes behind a burst OQPSK verdict
    are all 128.  The same cases on -0.0 input are printed where they differ: the places that depend on the sign of a zero."""
    O = oracle_mod
    signed = []
    for capsym in (False, True):
        for c in TC.zero_cases(O, name, capsym):
            geom = TC.capacities(c)
            for ch in c.watch:
                e = TC.expected(O, c, ch)
                if not c.sql:
                    c1 = TC.case(name, c.label, [[n] for w in c.writes for n in w], c.verdicts, capsym=c.capsym, trace=c.trace, softcap=c.softcap, watch=c.watch)
                    assert equal_runs(e, TC.expected(O, c1, ch)), (name, c.label, ch)
                if not c.overflow:
                    TC.check_exact(c, ch, e, TC.as_candidate(c, e, geom), geom)
                if c.cfg.oq:
                    assert set(np.unique(e.soft)) <= {-1, 128}, (name, c.label, ch, np.unique(e.soft))
                if ch not in c.verdicts:
                    assert len(e.soft) == 0 and len(e.events) == 1 and len(e.symbols) == 0 and e.states[-1]["startstop"] == -1 and e.states[-1]["cntr"] == 0
                if not capsym and not c.overflow:
                    m = TC.expected(O, c, ch, -np.zeros(c.total))
                    if not equal_runs(e, m):
                        signed.append((c.label, ch))
    print(f"burst_track {name}: cases whose result differs between +0.0 and -0.0 input: {signed if signed else 'none'}")


@pytest.mark.parametrize("name", NAMES)
def test_zero_input_cases_reach_what_they_are_about(oracle_mod, name):
    """The time-out, the EbNo emission, a wrap of win_ring / cv_len / the msema ring, a dropped squelch group and a kept one, both overflows."""
    O = oracle_mod
    cfg, g, lm = TC.CONFIGS[name], TC.geometry(TC.CONFIGS[name]), TC.landmarks(O, name)
    assert lm.marker < lm.ebno < lm.timeout and lm.ebno - lm.marker > g.ebno_tail
    b = TC.burst_cases(O, name, True)[1]
    assert b.total > g.cv_len + g.win_ring and b.trace
    e0 = TC.expected(O, b, 0)
    kinds = e0.events[:, 1].astype(int)
    assert (kinds == TC.EV_EBNO).sum() >= 2 and ((kinds == TC.EV_SIGNAL) & (e0.events[:, 2] == 0.0)).sum() >= 2 and e0.cov["timeout"] >= 2
    assert len(e0.symbols) > 3 * g.msema_len
    e2, e3 = TC.expected(O, b, 2), TC.expected(O, b, 3)
    assert len(e2.events) == 2 and e2.events[1, 1] == TC.EV_TRIDENT and e2.events[1, 2] < 0 and len(e2.soft) == 0
    assert (e3.events[:, 1] == TC.EV_TRIDENT).sum() == 2
    quiet = TC.expected(O, TC.burst_cases(O, name, True)[0], 2)
    assert len(quiet.events) == 1 and len(quiet.soft) == 0  # a rejecting verdict with trace off changes nothing at all
    if cfg.oq:
        sq = TC.squelch_cases(O, name, False)[0]
        for ch in (0, 1, 63, 64):
            e = TC.expected(O, sq, ch)
            assert e.cov["squelch_drop"] > 0 and len(e.soft) >= 32, (ch, e.cov, len(e.soft))
        assert len(TC.expected(O, sq, 0).soft) > 200  # the groups of the write whose lastmse was below the threshold


@pytest.mark.parametrize("name", NAMES)
def test_streams_cover_the_chain_and_their_decisions_are_robust(oracle_mod, name):
    """Part B's conditions: over the five recorded streams the loop clips, ct_ec reaches its clamp, a burst times out and (burst OQPSK) both yui
    corrections are taken and the squelch drops a group; of NDRAWS noise draws at most one in ten changes a decision of the oracle."""
    O = oracle_mod
    variants = [False, True] if TC.CONFIGS[name].oq else [False]
    for sql in variants:
        c = TC.stream_case(O, name, sql=sql)
        exp = {ch: TC.expected(O, c, ch) for ch in TC.OBS}
        cov = {k: sum(exp[ch].cov[k] for ch in TC.OBS) for k in O.BurstDemod.COVERAGE}
        print(f"burst_track {name} sql={int(sql)}: coverage {cov}")
        assert cov["clip"] > 0 and cov["clamp"] > 0 and cov["timeout"] > 0, cov
        if TC.CONFIGS[name].oq:
            assert cov["yui_even"] > 0 and cov["yui_odd"] > 0, cov
            assert (cov["squelch_drop"] > 0) == sql, cov
        for ch in TC.OBS:
            kinds = exp[ch].events[:, 1].astype(int)
            assert (kinds == TC.EV_SIGNAL).sum() >= 1 and (kinds == TC.EV_EBNO).sum() >= 1, (ch, exp[ch].events)
            assert len(exp[ch].soft) <= TC.capacities(c).soft_cap
        rejected, worst = 0, 0.0
        for draw in range(NDRAWS):
            res = [TC.noise_reference(O, c, ch, exp[ch], draw) for ch in TC.OBS]
            if any(why is not None for _, why in res):
                rejected += 1
                print(f"  draw {draw} rejected: {[why for _, why in res if why]}")
            else:
                worst = max(worst, max(en for en, _ in res))
                if draw == 0:
                    print(f"  draw 0: E_n per channel {[f'{en:.3e}' for en, _ in res]}")
        assert TC.noise_reference(O, c, TC.OBS[0], exp[TC.OBS[0]], 0)[1] is None  # the draw the GPU test uses
        assert rejected <= NDRAWS // 10, (name, rejected)
        print(f"  largest E_n of the accepted draws {worst:.3e} (the kernel's bound is min(SYM_TOL, E_n) per channel)")
        assert worst > 0.0, name


def test_checkers_refuse_wrong_candidates(oracle_mod):
    """check_exact on an oracle run that was tampered with: a soft byte, a store behind the count, an event's stamp, a count, a symbol."""
    O = oracle_mod
    c = TC.edge_cases("oqpsk", True)[4]
    geom, e = TC.capacities(c), TC.expected(O, TC.edge_cases("oqpsk", True)[4], 0)
    TC.check_exact(c, 0, e, TC.as_candidate(c, e, geom), geom)

    def tampered(f):
        g = TC.as_candidate(c, e, geom)
        f(g)
        with pytest.raises(AssertionError):
            TC.check_exact(c, 0, e, g, geom)

    tampered(lambda g: g.soft_row.__setitem__(5, 127))
    tampered(lambda g: g.soft_row.__setitem__(len(e.soft), 128))
    tampered(lambda g: g.events.__setitem__((1, 0), g.events[1, 0] + 1))
    tampered(lambda g: g.states[0].__setitem__("cntr", g.states[0]["cntr"] + 1))
    tampered(lambda g: g.sym_rows.__setitem__((3, 2), 1.0))
    tampered(lambda g: g.sym_rows.__setitem__((len(e.symbols), 0), 0.0))
    tampered(lambda g: g.states[-1].__setitem__("overflow", 1))
