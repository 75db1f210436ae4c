"""CPU: what anchors tests/rt_isu_oracle.py, the definition the burst bank's reassembly is held to.
  * The case set itself (tests/rt_isu_cases.py): sizes, flags and counters of every case against values worked out by hand from
    JAERO/aerol.cpp:6-113, so that no comparison passes on nothing.
  * The unmodified reference (oracle/_ref, where it is built), over every case stream: the units it prints for its T packets are the ones
    the restatement feeds (at 600 / 1200 bps: the unit with a wrong CRC among them, the last unit sent not); " missing (or if unimplimented
    then TODO in C++)" behind a printed SSU -- the one thing it shows of ISUData -- is the restatement's missing SSU, position for position;
    and its " SU i of n. AES: .. GES: .." lines are the restatement's parsed R fields."""
import re

import numpy as np
import pytest

import isu_oracle as IO
import rt_isu_cases as RC
import rt_isu_oracle as RO
from jaero_amd import acars

MISSING = " missing (or if unimplimented then TODO in C++)"
A, B, C_, D = RC.A, RC.B, RC.C_, RC.D
RCH, SIG = RO.F_RCHAN, RO.F_RSIGNAL


def summary(msgs):
    return [(int(m["aesid"]), int(m["nbytes"]), int(m["flags"])) for m in msgs]


@pytest.mark.parametrize("fb", [10500, 1200, 600])
def test_every_case_does_what_it_is_there_for(oracle_mod, fb):
    E = lambda name: RC.expected(oracle_mod, name, fb)
    for name in RC.CASES:  # the search finds every packet a case sends whole, so the cases test the reassembly and not the search
        pk = E(name)[3]
        assert len(set(pk[:, 0].tolist())) == RC.good_packets(name, fb), name
    msgs, stats, missing, pk, ev, ch = E("r_sizes")
    # in order: the bytes sent; last first: sized 25 by the last unit; middle first: cut to 24 by the last; short last first: 24, never grown;
    # repeated first unit: cut to 15 by the second; SUTYPE 5 in the middle: 33
    assert summary(msgs) == [(A + k, n, RCH) for k, n in enumerate((1, 5, 11, 12, 22, 23, 33))] + [(B, 25, RCH), (B, 24, RCH), (B, 24, RCH), (C_, 15, RCH), (D, 33, RCH)]
    assert list(stats) == [0, 0, 0, 0, 28, 12, 12, 0]
    assert [(int(m["qno"]), int(m["refno"]), int(m["nooct"]), int(m["k"])) for m in msgs[:3]] == [(0, 0, 0, 0), (1, 1, 0, 0), (2, 2, 0, 0)]
    assert [int(m["frame"]) for m in msgs[:5]] == [0, 1, 2, 4, 6]  # the packet that completed it
    up = lambda t, n: bytes((t + i) & 255 for i in range(n))
    assert bytes(msgs[7]["data"][:25]) == up(0x40, 11) + up(0x50, 11) + up(0x60, 3)
    assert bytes(msgs[9]["data"][:24]) == up(0x40, 11) + up(0x50, 9) + bytes(2) + up(0x60, 2)  # bytes 20, 21: sized by the last unit, written by nobody
    assert bytes(msgs[10]["data"][:15]) == up(0x20, 11) + up(0x30, 4)                          # the repeated unit's second copy
    assert bytes(msgs[11]["data"][:33]) == up(0x40, 11) + up(0x50, 5) + bytes(6) + up(0x60, 11) and not msgs[11]["data"][33:].any()
    msgs, stats, missing, pk, ev, ch = E("r_keys")
    assert summary(msgs) == [(B, 29, RCH), (A, 28, RCH), (C_, 19, RCH), (D, 0, RCH | SIG), (D, 0, RCH | SIG), (D, 14, RCH)] + [(A, 0, RCH)] * 4 + [
        (0, 6, RCH | IO.F_AES0), (C_, 15, RCH)]
    assert list(stats) == [0, 0, 0, 0, 28, 17, 12, 2]  # 29 packets, one of them not user data
    assert bytes(msgs[2]["data"][:19]) == up(0x22, 11) + up(0x33, 8) and int(msgs[2]["refno"]) == 2  # REFNO 10 landed in REFNO 2's item
    # what never completes is still in the list or has aged out: SEQINDICATOR 0 / 7 grew to 9 bytes by the writes past its end
    grown = [it for it in ch.risu.items if it.AESID == B and it.QNO == 8]
    assert [bytes(it.userdata) for it in grown] == [up(0x03, 3) + up(0x02, 9)[3:]]
    msgs, stats, missing, pk, ev, ch = E("r_age")
    assert [(a, n) for a, n, f in summary(msgs) if n != 2] == [(A, 16), (0x400003, 12)] and list(stats) == [0, 0, 0, 0, 50, 48, 32, 0]
    # the twelve pending items filled the list to its eleven; each late unit then aged one out, and the second one's item left complete
    assert len(ch.risu.items) == 9 and sorted(it.count for it in ch.risu.items) == list(range(1, 10))
    msgs, stats, missing, pk, ev, ch = E("r_acars")
    AC, TX, MO, PA = IO.F_ACARS, IO.F_TEXT, IO.F_MORE, IO.F_PARITY
    assert summary(msgs) == [(A, 19, RCH | AC), (B, 29, RCH | AC | TX), (C_, 26, RCH | AC | TX | PA), (C_, 24, RCH | AC | TX | MO)]
    items = [acars.parse_msg(m) for m in msgs]
    assert all(it.downlink for it in items) and items[0].PLANEREG == b".A6-EDY" and items[1].message == "POS OK 12" and items[2].error and items[3].moretocome
    msgs, stats, missing, pk, ev, ch = E("t_basic")
    assert summary(msgs) == [(A, 23, 0), (B, 50, 0), (C_, 19, 0), (D, 34, AC | TX), (0, 10, IO.F_AES0)] and list(stats) == [5, 17, 0, 5, 0, 0, 0, 0]
    assert [int(m["frame"]) for m in msgs] == [0, 2, 4, 5, 6] and not missing
    assert acars.parse_msg(msgs[3], downlink=True).message == "T CHANNEL TEXT"
    msgs, stats, missing, pk, ev, ch = E("t_missing")
    assert summary(msgs) == [(B, 17, 0), (C_, 14, 0)] and list(stats) == [2, 14, 10, 2, 0, 0, 0, 0] and len(missing) == 10
    assert int((ev[:, 1] == 3).sum()) >= 1  # the refused packet's " Bad R/T Packet"
    msgs, stats, missing, pk, ev, ch = E("t_msk")
    assert summary(msgs) == [(D, 24, 0)] and list(stats) == [1, 3, 0, 1, 0, 0, 0, 0] and not missing  # the unit with the wrong CRC completed it; the last one sent was not looked at
    msgs, stats, missing, pk, ev, ch = E("mixed")
    assert summary(msgs) == [(A, 30, RCH), (A, 28, 0), (B, 0, RCH | SIG), (C_, 9, RCH)] and list(stats) == [1, 4, 0, 1, 5, 3, 3, 1]
    msgs, stats, missing, pk, ev, ch = E("noise")
    assert len(msgs) == 0 and not stats.any()


def test_the_generators_invert_the_definition():
    for n in (1, 11, 12, 22, 23, 33):
        u = bytes(range(100, 100 + n))
        ps = acars.r_isu_payloads(0x123456, 0x90, 5, 3, u)
        assert len(ps) == (n + 10) // 11 and all(len(p) == 17 and p[1] & 8 for p in ps)
        ch = RO.Channel(10500)
        for k, p in enumerate(ps):
            ch.packet(k, 1, p + bytes(3))
        (m,) = ch.take()
        assert bytes(m["data"][:n]) == u and int(m["nbytes"]) == n and (int(m["aesid"]), int(m["gesid"]), int(m["qno"]), int(m["refno"])) == (0x123456, 0x90, 5, 3)
    with pytest.raises(ValueError):
        acars.r_isu_payloads(1, 2, 3, 8, b"x")
    with pytest.raises(ValueError):
        acars.r_isu_payloads(1, 2, 3, 4, bytes(34))
    units = acars.isu_payloads(0x123456, 0x90, 1, 2, bytes(range(30)))
    pk = acars.t_packets(0xABCDEF, 0x90, units, 3)
    assert [len(us) for _, us in pk] == [3, 2] and pk[0][0] == bytes([0xAB, 0xCD, 0xEF, 0x90]) and sum((us for _, us in pk), []) == units
    assert [len(us) for _, us in acars.t_packets(1, 2, units[:1], 3)] == [2]
    pk = acars.t_packets(0xABCDEF, 0x90, units, 3, msk=True)
    assert [us[1] for _, us in pk] == [acars.FILL_IN] * 2 and [len(us) for _, us in pk] == [5, 4] and pk[0][1][0] == units[0] and pk[0][1][2:4] == units[1:3]


@pytest.fixture(scope="module")
def R(oracle_mod):
    if not oracle_mod.have_ref():
        pytest.skip("oracle/_ref/jaero_ref not available here")
    try:
        oracle_mod.run_ref_aerol_burst(10500, np.full(64, 128, np.int16))
    except Exception as e:
        pytest.skip(f"_ref cannot run here: {e}")
    return oracle_mod


@pytest.mark.parametrize("fb", [10500, 1200, 600])
def test_units_missing_ssus_and_r_fields_are_the_unmodified_references(R, fb):
    nmissing = nr = 0
    for name in RC.CASES:
        inv = (True, False) if name in ("t_missing", "r_keys") else (False, False)
        _, _, missing, pk, _, ch = RC.expected(R, name, fb, inv)
        _, _, txt = R.run_ref_aerol_burst(fb, RC.stream(name, fb, inv))
        lines = txt.split("\n")
        units = [m for m in (re.match(r"^((?: 0x[0-9A-F]{2}){10})( (?!0x).*|)$", ln) for ln in lines) if m]
        assert [bytes(int(x, 16) for x in m.group(1).split()) for m in units] == ch.t_units, (name, "the printed units are not the ones fed")
        # position among the fed units of every missing SSU: (packet, k) -> running index
        where, i = {}, 0
        for p in sorted(set(pk[:, 0].tolist())) if len(pk) else []:
            r = pk[pk[:, 0] == p]
            if int(r[0, 15]) == 2:
                for k in range(RO.number_of_sus(fb, bytes(int(v) for v in r[np.argsort(r[:, 1])][:, 2:14].reshape(-1))[: int(r[0, 14])])):
                    where[(int(p), k)] = i
                    i += 1
        assert [j for j, m in enumerate(units) if m.group(2).endswith(MISSING)] == [where[pkk] for pkk in missing], (name, fb)
        nmissing += len(missing)
        got = [(int(m.group(1)), int(m.group(2)), int(m.group(3), 16), int(m.group(4), 16))
               for m in (re.search(r" SU (\d+) of (\d+)\. AES: ([0-9A-F]{6}) GES: ([0-9A-F]{2})$", ln) for ln in lines) if m]
        assert got == ch.r_lines, (name, fb)
        nr += len(got)
    assert nmissing >= 10 and nr >= 100
