"""GPU (-m gpu): the rate lines read on the device (jaero_lines_classify; k_rate_classify in jaero_amd/csrc/k_rate_classify.h) against
their definition (tests/rate_lines_oracle.py) on the meter's own read(), and RateMeter.classify() against classify_rates(read()).

There is no tolerance anywhere in this file: the kernel only selects among the doubles of R (and halves one sum), so floor, score and
where are compared with np.array_equal, and so are the decisions (audio with equal_nan)."""
import ctypes as C

import numpy as np
import pytest

import rate_cases as RC
import rate_lines_cases as LC
import rate_lines_oracle as LO
import rate_oracle as RO
from chan_cases import CH  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

L, BINS = RO.L, RO.BINS
GPU_KMIN = (8, 7)


@pytest.fixture(scope="module")
def RM():
    from jaero_amd import capi, ratemeter

    capi.lib()
    return ratemeter


def check_meter(RM, m, where):
    """classify_lines against the oracle on m.read(), and classify() against classify_rates(m.read()), for every kmin, at m.fs"""
    R, nseg = m.read()
    d = RM.rate_distances(m.fs)
    for kmin in GPU_KMIN:
        floor, score, at, n = m.classify_lines(d, kmin)
        assert n == nseg and at.dtype == np.int32 and m.kernel_ms > 0.0
        LC.assert_lines_equal((floor, score, at), LO.lines(R, kmin, d), f"{where}, fs={m.fs}, kmin={kmin}")
        with np.errstate(all="ignore"):
            got = m.classify(kmin=kmin)
        LC.assert_decisions_equal(got, LC.classify_reference(R, m.fs, kmin), f"{where}, fs={m.fs}, kmin={kmin}")
    return R


@pytest.mark.parametrize("fs", LC.FS)
@pytest.mark.parametrize("nch", [1, 5, 67])
def test_case_rows(RM, nch, fs):
    """Three segments and a tail of the case rows, cycled: one channel (a quarter of a workgroup), 5 (the second workgroup holds one) and
    67 (the last holds three)."""
    m = RM.RateMeter(nch, fs, max_write_samples=RC.N_PARITY)
    assert m.write(RC.case_rows(nch, RC.N_PARITY)) == 3
    R = check_meter(RM, m, f"case rows, nch={nch}")
    m.close()
    assert R.any()


@pytest.mark.parametrize("fs", LC.FS)
@pytest.mark.parametrize("nch", [10, 67])
def test_made_rows(RM, nch, fs):
    """The ten rows no signal produces, poked into R: as they are, and cycled over 67 channels"""
    rows = LC.cycled(LC.made_rows(), nch)
    m = RM.RateMeter(nch, fs)
    m.poke(rows, 5)
    R = check_meter(RM, m, f"made rows, nch={nch}")
    assert np.array_equal(R, rows) and m.read()[1] == 5
    if fs == 48000.0:
        floor, score, at, _ = m.classify_lines(LC.D48, 8)
        assert at[1, 1] == 99 and at[8, 0] == LC.AT_KMIN and at[7, 0] == 1996 and (at[0] == 8).all() and floor[6] == 5e-324
    m.close()


def test_a_row_does_not_depend_on_its_neighbours(RM):
    """Row 66 of 67 (the third wavefront of the last workgroup) alone in a meter of one channel: the same bytes"""
    pcm = RC.case_rows(67, RC.N_PARITY)
    made = LC.cycled(LC.made_rows(), 67)
    big, one = RM.RateMeter(67, 48000.0, max_write_samples=RC.N_PARITY), RM.RateMeter(1, 48000.0, max_write_samples=RC.N_PARITY)
    big.write(pcm)
    one.write(pcm[66:67])
    for step in ("written", "poked"):
        if step == "poked":
            big.poke(made, 1)
            one.poke(made[66:67], 1)
        assert np.array_equal(big.read()[0][66:67], one.read()[0])
        for kmin in GPU_KMIN:
            fb, sb, wb, _ = big.classify_lines(LC.D48, kmin)
            fo, so, wo, _ = one.classify_lines(LC.D48, kmin)
            LC.assert_lines_equal((fb[66:67], sb[66:67], wb[66:67]), (fo, so, wo), f"{step}, kmin={kmin}")
    big.close()
    one.close()


def test_the_meter_is_left_as_it_was(RM):
    """read() before and after is equal, two calls give the same bytes, and a write behind the call goes on counting -- with the pending
    tail in place: R afterwards is the oracle's over all six segments."""
    pcm = RC.case_rows(5, 6 * L)
    m = RM.RateMeter(5, 48000.0, max_write_samples=3 * L + 100)
    assert m.write(pcm[:, :3 * L + 100]) == 3
    R0, n0 = m.read()
    a = m.classify_lines(LC.D48, 8)
    b = m.classify_lines(LC.D48, 8)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3] == 3
    R1, n1 = m.read()
    assert n0 == n1 == 3 and np.array_equal(R0, R1)
    assert m.write(pcm[:, 3 * L + 100:]) == 3
    R2, n2 = m.read()
    assert m.classify_lines(LC.D48, 8)[3] == n2 == 6
    m.close()
    o = RO.RateOracle(5)
    o.write(pcm)
    RC.assert_rule(R2, o.R, "after classify_lines")


def test_range_refusals_on_a_live_handle(RM):
    from jaero_amd import capi

    m = RM.RateMeter(3, 48000.0)
    m.poke(LC.made_rows()[:3], 1)
    floor, score, at = np.full(3, -7.0), np.full((3, 9), -7.0), np.full((3, 9), -7, dtype=np.int32)
    n, ms = C.c_longlong(-7), C.c_double(-7.0)

    def call(kmin, d):
        dd = np.array(d, dtype=np.int32)
        return m.lib.jaero_lines_classify(m.h, kmin, len(d), dd.ctypes.data if len(d) else np.zeros(1, np.int32).ctypes.data, floor.ctypes.data,
                                          score.ctypes.data, at.ctypes.data, C.byref(n), C.byref(ms))

    for kmin, d, word in ((8, [], b"nd 0"), (8, [51] * 9, b"nd 9"), (8, [51, 0], b"d[1] = 0"), (8, [-3], b"d[0] = -3"), (0, [51], b"kmin 0"),
                          (2048, [51], b"kmin 2048")):
        assert call(kmin, d) == capi.E_INVAL, (kmin, d)
        msg = m.lib.jaero_last_error()
        assert b"jaero_lines_classify" in msg and word in msg, msg
        assert (floor == -7.0).all() and (score == -7.0).all() and (at == -7).all() and n.value == -7 and ms.value == -7.0
    with pytest.raises(capi.JaeroError) as e:
        m.classify_lines([], 8)
    assert e.value.code == capi.E_INVAL
    assert call(2047, [1]) == 0 and at[0, 0] == 2047 and n.value == 1 and ms.value > 0.0  # the last kmin and the one a it leaves
    assert call(8, [2040, 2041, 1 << 30]) == 0 and at[0, :3].tolist() == [8, -1, -1]         # the last distance that fits
    assert m.lib.jaero_rate_profile_read(m.h, 1, None, None, 0) == capi.E_INVAL  # which != 0 stays refused: the launch has no timer slot
    m.close()


def test_gated_handle(RM):
    """One meter under the one-pass gates on the burst rows: classify() is classify_rates(read()), and names the bursts' rates"""
    import rate_auto_cases as AC
    import rate_gate_cases as GC

    pcm = AC.burst_rows("plain")
    m = RM.RateMeter(5, GC.BURST_FS, max_write_samples=GC.BURST_WRITE)
    m.gate_enable(auto=True)
    for pos in range(0, pcm.shape[1], GC.BURST_WRITE):
        m.write(np.ascontiguousarray(pcm[:, pos:pos + GC.BURST_WRITE]))
    R = check_meter(RM, m, "burst rows under AUTO")
    assert m.classify()[0].tolist() == AC.AUTO_RATES
    st = m.read_gate_auto()
    assert st[-1] == GC.BURST_NSEG and np.array_equal(m.read()[0], R)  # the gates' numbers are still there
    m.close()


def test_blind_chain_in_one_call(CH, RM):
    """Capture -> Channeliser.write -> RateMeter.write_from -> classify(): the rates, and exactly classify_rates(read())"""
    iq, chans, _ = RC.chain()
    ch = CH.Channeliser(RC.CHAIN_DECIM, chans, max_write_iq=len(iq))
    m = RM.RateMeter(5, RC.CHAIN_FS_OUT, max_write_samples=RC.CHAIN_SEGS * L)
    assert ch.write(iq) == RC.CHAIN_SEGS * L
    assert m.write_from(ch) == RC.CHAIN_SEGS
    rate, audio, score = m.classify()
    assert rate.tolist() == RC.CHAIN_RATES
    LC.assert_decisions_equal((rate, audio, score), RM.classify_rates(m.read()[0], m.fs), "chain")
    check_meter(RM, m, "chain")
    m.close()
    ch.close()


def test_scale(RM):
    """33 091 channels (the last workgroup holds three), one segment of the case rows cycled on the device, one write: 64 spread rows and
    the last 9 against the oracle on read()."""
    import torch

    nch, n = 33091, L + 7
    base = torch.from_numpy(np.array(RC.base_rows(n))).cuda()
    t = base[torch.arange(nch, device="cuda") % RC.NCASES].contiguous()
    m = RM.RateMeter(nch, 48000.0, max_write_samples=n)
    assert m.write_device(t.data_ptr(), n) == 1
    R, nseg = m.read()
    floor, score, at, n2 = m.classify_lines(LC.D48, 8)
    print(f"k_rate_classify over {nch} channels: {m.kernel_ms:.3f} ms")
    assert nseg == n2 == 1 and m.kernel_ms > 0.0
    m.close()
    rows = np.unique(np.concatenate([np.linspace(0, nch - 10, 64).astype(int), np.arange(nch - 9, nch)]))
    assert len(rows) == 73
    LC.assert_lines_equal((floor[rows], score[rows], at[rows]), LO.lines(R[rows], 8, LC.D48), "scale")
    assert floor.shape == (nch,) and score.shape == at.shape == (nch, 4)
