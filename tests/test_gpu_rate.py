"""GPU (-m gpu): the rate meter (jaero_rate_*; k_rate_lines in jaero_amd/csrc/k_rate.h) against its definition (tests/rate_oracle.py), and
the blind chain it closes: capture -> channeliser -> rate lines -> classify_rates.

Tolerance against the oracle (tests/rate_cases.py assert_rule): per row |got - want| <= 1e-12 (want + mean_k want), the survey's bound;
the oracle itself lies within 4.2e-16 of a long-double DFT by the same rule (tests/test_rate_host.py), so the bound stands as it is.  Rows
of zeros and constant rows are compared with ==.  Cut and host / device independence are exact: np.array_equal on the float64."""
import numpy as np
import pytest

import rate_cases as RC
import rate_oracle as RO
from chan_cases import CH  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

L, BINS = RO.L, RO.BINS


@pytest.fixture(scope="module")
def RM():
    from jaero_amd import capi, ratemeter

    capi.lib()
    return ratemeter


def run(RM, pcm, cuts=None, device=False, max_write=None):
    """(R, nseg) of a fresh meter fed pcm [nch, n] in writes of `cuts` samples, from host memory or from a device tensor"""
    nch, n = pcm.shape
    cuts = cuts or [n]
    assert sum(cuts) == n
    m = RM.RateMeter(nch, 48000.0, max_write_samples=max_write or max(cuts))
    pos, done = 0, 0
    for k in cuts:
        part = np.ascontiguousarray(pcm[:, pos:pos + k])
        if device:
            import torch

            t = torch.from_numpy(part).cuda()
            done += m.write_device(t.data_ptr(), k)
            torch.cuda.synchronize()  # t is freed when it goes out of scope
        else:
            done += m.write(part)
        pos += k
        assert done == pos // L
    R, nseg = m.read()
    m.close()
    assert nseg == done
    return R, nseg


@pytest.mark.parametrize("nch", [1, 5, 67])
def test_rate_lines_equal_definition(RM, nch):
    """Three segments and a 100-sample tail of the nine case rows, cycled: one channel (half a workgroup), 5 and 67 (the last workgroup
    half empty)."""
    pcm = RC.case_rows(nch, RC.N_PARITY)
    o = RO.RateOracle(nch)
    o.write(pcm)
    R, nseg = run(RM, pcm)
    assert nseg == o.n == 3
    RC.assert_rule(R, o.R, f"nch={nch}")
    for c in RC.exact_rows(nch):
        assert (R[c] == 0.0).all()


def test_cuts_and_input_memory_change_nothing(RM):
    """The same rows in one write and cut as [1, 4095, 4097, 1, 8197, rest], from host memory and from a device tensor: four times the same bits."""
    pcm = RC.case_rows(11, RC.N_CUTS)
    o = RO.RateOracle(11)
    o.write(pcm)
    whole_h, n0 = run(RM, pcm)
    cut_h, n1 = run(RM, pcm, RC.CUTS)
    whole_d, n2 = run(RM, pcm, device=True)
    cut_d, n3 = run(RM, pcm, RC.CUTS, device=True)
    assert n0 == n1 == n2 == n3 == o.n == 5
    RC.assert_rule(whole_h, o.R, "one write, host")
    assert np.array_equal(whole_h, cut_h), "R depends on how the writes are cut"
    assert np.array_equal(whole_h, whole_d), "R depends on where the input lies"
    assert np.array_equal(whole_h, cut_d), "R depends on how device writes are cut"


def test_reset_keeps_the_segment_grid(RM):
    """A reset in the middle of a segment: R afterwards is the oracle's over the later segments of the SAME grid."""
    pcm = RC.case_rows(7, RC.N_PARITY)
    m = RM.RateMeter(7, 48000.0, max_write_samples=RC.N_PARITY)
    assert m.write(pcm[:, :L + 50]) == 1
    R1, n1 = m.read()
    m.reset()
    R0, n0 = m.read()
    assert n0 == 0 and not R0.any() and n1 == 1 and R1.any()
    assert m.write(pcm[:, L + 50:]) == 2
    R, n = m.read()
    m.close()
    o = RO.RateOracle(7)
    o.write(pcm[:, L:])
    assert n == o.n == 2
    RC.assert_rule(R, o.R, "after the reset")
    first = RO.RateOracle(7)
    first.write(pcm[:, :L])
    RC.assert_rule(R1, first.R, "before the reset")


def test_oversized_write_is_refused_and_consumes_nothing(RM):
    from jaero_amd import capi

    pcm = RC.case_rows(5, 2 * L + 30)
    a, b = RM.RateMeter(5, 48000.0, max_write_samples=L + 30), RM.RateMeter(5, 48000.0, max_write_samples=L + 30)
    for m in (a, b):
        assert m.write(pcm[:, :L]) == 1
    with pytest.raises(capi.JaeroError) as e:
        a.write(pcm[:, :L + 31])
    assert e.value.code == capi.E_INVAL and "max_write_samples" in str(e.value)
    for m in (a, b):
        assert m.write(pcm[:, L:]) == 1
    (Ra, na), (Rb, nb) = a.read(), b.read()
    a.close()
    b.close()
    assert na == nb == 2 and np.array_equal(Ra, Rb)
    o = RO.RateOracle(5)
    o.write(pcm)
    RC.assert_rule(Ra, o.R, "after the refusal")


def test_profile_counts_the_line_kernel(RM):
    pcm = RC.case_rows(3, L + 10)
    m = RM.RateMeter(3, 48000.0, max_write_samples=L + 10)
    m.profile_enable()
    m.write(pcm[:, :10])   # completes nothing: no launch
    m.write(pcm[:, 10:])   # one segment
    ms, launches = m.profile_read(reset=True)
    assert launches == 1 and ms > 0.0
    assert m.profile_read() == (0.0, 0)
    m.close()


def test_blind_chain_names_every_rate(CH, RM):
    """Capture -> Channeliser.write -> RateMeter.write_from (device to device) -> read -> classify_rates: R equals the oracle's on the
    channeliser's own int16 output, the four carriers get their rates and audio offsets, the empty channel gets none.  The margins are
    asserted on the CPU oracles alone in tests/test_rate_host.py."""
    iq, chans, _ = RC.chain()
    ch = CH.Channeliser(RC.CHAIN_DECIM, chans, max_write_iq=len(iq))
    m = RM.RateMeter(5, RC.CHAIN_FS_OUT, max_write_samples=RC.CHAIN_SEGS * L)
    assert ch.write(iq) == RC.CHAIN_SEGS * L
    assert m.write_from(ch) == RC.CHAIN_SEGS
    R, nseg = m.read()
    pcm = ch.read_pcm()
    o = RO.RateOracle(5)
    o.write(pcm)
    assert nseg == o.n == RC.CHAIN_SEGS
    RC.assert_rule(R, o.R, "chain")
    rate, audio, score = RM.classify_rates(R, m.fs)
    print("chain scores, dB:\n", np.round(score, 1), "\naudio:", audio)
    assert rate.tolist() == RC.CHAIN_RATES
    assert (np.abs(audio[:4] - np.array(RC.CHAIN_AUDIO)) <= RC.CHAIN_FS_OUT / L).all() and np.isnan(audio[4])
    m.close()
    ch.close()


def test_scale_one_launch(RM):
    """33 091 channels x (4096 + 7) samples made on the device, one launch (rows at odd addresses: every row's first and last 16-byte word
    is shared with its neighbours); 16 spread rows against the oracle."""
    import torch

    nch, n = 33091, L + 7
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    t = torch.randint(-32768, 32768, (nch, n), device="cuda", dtype=torch.int32, generator=g).to(torch.int16)
    m = RM.RateMeter(nch, 48000.0, max_write_samples=n)
    assert m.write_device(t.data_ptr(), n) == 1
    R, nseg = m.read()
    m.close()
    assert nseg == 1
    rows = np.unique(np.concatenate([np.linspace(0, nch - 1, 14).astype(int), [1, nch - 2]]))
    assert len(rows) == 16
    pcm = t[torch.from_numpy(rows).cuda()].cpu().numpy()
    o = RO.RateOracle(len(rows))
    o.write(pcm)
    RC.assert_rule(R[rows], o.R, "scale")
    assert (R > 0.0).any(axis=1).all()
