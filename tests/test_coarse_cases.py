"""CPU: the host side of tests/test_gpu_coarse.py holds together without a GPU -- the matrix's bandwidths stay inside what the kernel's index
arithmetic covers, the exact cases give the bin they were built for in the oracle and in the fp64 restatement, the long-double restatement
follows the oracle, and the oracle alone stays unlocked on the never-locked streams."""
import numpy as np
import pytest

import coarse_cases as CC


@pytest.mark.parametrize("name", list(CC.CONFIGS))
def test_matrix_bandwidths_are_inside_the_kernels_index_checks(name):
    cfg = CC.CONFIGS[name]
    assert cfg.lbws[0] == cfg.lbw0
    for b in cfg.lbws:
        CC.check_index_ranges(cfg, b)
    sb = [cfg.startbin(b) for b in cfg.lbws]
    assert 1 in sb and any(a != b for a, b in zip(sb, sb[1:]))
    assert cfg.Fs / 2 in cfg.lbws and sum(not cfg.fold_inside(b) for b in cfg.lbws) >= 2
    if cfg.fb == 8400.0:
        k = [s >= 3583 for s in sb]  # C4_TABN - 1: the window is built per estimate from here
        assert any(a and not b for a, b in zip(k, k[1:])) and any(b and not a for a, b in zip(k, k[1:]))
        assert any(sb[i] == sb[i + 2] != sb[i + 1] for i in range(len(sb) - 2))  # the table is rebuilt, and rebuilt back
    with pytest.raises(AssertionError):
        CC.check_index_ranges(cfg, cfg.Fs / 2 + 1.0)


@pytest.mark.parametrize("name", list(CC.CONFIGS))
def test_exact_cases_agree_with_the_oracle(oracle_mod, name):
    cfg = CC.CONFIGS[name]
    zero = np.zeros(cfg.N, dtype=np.complex128)
    cases = CC.exact_cases(cfg)
    assert len({c[0] for c in cases}) == len(cases) >= 24
    for cname, lbw, y_in, built in cases:
        oc = oracle_mod.Coarse(cfg.power, lbw, cfg.fb, cfg.Fs)
        assert oc.process(zero) == 0.0
        oc.set_y(y_in)
        b = oc.peak_bin(oc.process(zero))
        assert np.array_equal(oc.get_y(), y_in * 0.9)
        assert b == CC.peak_bin(cfg, lbw, y_in * 0.9) and built in (None, b), (name, cname, b, built)


@pytest.mark.parametrize("name", ["oqpsk_10500", "oqpsk_8400", "msk_1200_12k"])
def test_restatement_follows_the_oracle(oracle_mod, name):
    """y of the oracle against the long-double restatement: 1e-12 where no bin sits at the clip, 1e-5 at 8400 bps (the window leaves |Z| near 1
    in thousands of bins); and the draws bind the peak bin (margin ratio > 1000)."""
    cfg = CC.CONFIGS[name]
    rng = np.random.default_rng(5)
    for lbw, signal in ((cfg.lbw0, True), (cfg.lbw0, False), (cfg.Fs / 2, True)):
        x = CC.draw(cfg, lbw, rng, signal)
        y_in = rng.uniform(0.0, 30.0, cfg.N)
        oc = oracle_mod.Coarse(cfg.power, lbw, cfg.fb, cfg.Fs)
        oc.process(np.zeros(cfg.N, dtype=np.complex128))
        oc.set_y(y_in)
        b = oc.peak_bin(oc.process(x))
        L, y_ld = CC.restate(cfg, lbw, x, y_in)
        assert float(np.max(np.abs(oc.get_y() - y_ld))) < (1e-5 if cfg.fb == 8400.0 else 1e-12)
        ok, ratio = CC.margin_ok(cfg, lbw, y_ld, oc.get_y())
        assert ok and b == CC.peak_bin(cfg, lbw, y_ld), (name, lbw, signal, ratio)


@pytest.mark.parametrize("kind", ["oqpsk", "msk"])
def test_the_oracle_stays_unlocked_on_the_never_locked_streams(oracle_mod, kind):
    O = oracle_mod
    sig = CC.stream_signals(kind)
    thr = CC.STREAM_THR[kind]
    ost = O.oqpsk_settings(threshold=thr) if kind == "oqpsk" else O.msk_settings(threshold=thr)
    for k in range(CC.STREAM_NSIG):
        rows = O.run_demod(ost, sig[k], chunk=4096)["status"]
        assert len(rows) >= 30 and int((rows[:, 5] == 0).sum()) >= CC.STREAM_MIN_UNLOCKED, (kind, k)
