"""CPU: jaero_amd/acars.py -- the generators against the parser (through the definition's classification, tests/isu_oracle.py, which is what
the device writes into a row) and the defragmenter against ACARSDefragmenter's rules (JAERO/aerol.cpp:221-329)."""
import numpy as np
import pytest

import isu_oracle as IO
from jaero_amd import acars


def row_of(aesid, userdata, gesid=0x90, qno=1, refno=2):
    """The row the reassembly emits for a message sent as isu_payloads(...)."""
    isu = IO.ISUData()
    done = [it for it in (isu.update(p) for p in acars.isu_payloads(aesid, gesid, qno, refno, userdata)) if it is not None]
    assert len(done) == 1 and isu.stats[2] == 0
    return IO.msg_row(done[0], 5, 3)


def block(text, bi="A", more=False, reg=".A6-EDY", tak="\x15", label="H1", mode="2", aesid=0x8960FA):
    return acars.parse_msg(row_of(aesid, acars.acars_userdata(reg, mode, tak, label, bi, text, more)))


@pytest.mark.parametrize("n", [2, 3, 9, 10, 11, 18, 19, 250, 505, 506])
def test_isu_payloads_round_trip(n):
    u = bytes((7 * i + n) & 255 for i in range(n))
    pay = acars.isu_payloads(0x123456, 0x90, 3, 4, u)
    assert all(len(p) == 10 for p in pay) and pay[0][0] == 0x71 and pay[0][6] == len(pay) - 1 <= 63
    r = row_of(0x123456, u)
    assert int(r["nbytes"]) == n and bytes(r["data"][:n]) == u and not r["data"][n:].any()
    with pytest.raises(ValueError):
        acars.isu_payloads(0x123456, 0x90, 3, 4, bytes(507))


def test_generator_to_parser_round_trip():
    it = block("POSN 33.5S 151.2E\r\n/TS 120000 \x7f")
    assert it.valid and not it.nonacars and it.hastext and not it.moretocome and it.error is None
    assert (it.PLANEREG, chr(it.MODE), it.TAK, it.LABEL, chr(it.BI)) == (b".A6-EDY", "2", 0x15, b"H1", "A")
    assert it.message == "POSN 33.5S 151.2E\r\n/TS 120000 <DEL>"
    assert (it.aesid, it.gesid, it.qno, it.refno, it.frame, it.k) == (0x8960FA, 0x90, 1, 2, 5, 3)
    it = block(None)
    assert it.valid and not it.hastext and it.message == "" and len(it.userdata) == 19
    it = block("X" * 220, more=True)
    assert it.valid and it.moretocome and it.message == "X" * 220
    u = acars.acars_userdata(".A6-EDY", "2", "\x15", "H1", "A", "ODD")
    assert all(bin(b).count("1") & 1 for b in u[2:-3]) and u[:2] == b"\xff\xff" and u[-1] == 0x7F and u[15] == 0x02 and u[-4] == 0x83
    other = acars.parse_msg(row_of(0x8960FA, bytes(range(40, 60))))
    assert other.valid and other.nonacars and other.message == bytes(range(40, 60)).hex().upper()
    assert acars.parse_msg(row_of(0, u)).error == "Error: AESID == 0"


def test_parity_errors():
    u = bytearray(acars.acars_userdata(".A6-EDY", "2", "\x15", "H1", "A", "SOME TEXT"))
    for k, bad in ((4, True), (10, True), (16, True), (len(u) - 5, True), (3, False), (11, False), (len(u) - 4, False), (len(u) - 2, False)):
        v = bytearray(u)
        v[k] ^= 0x80
        it = acars.parse_msg(row_of(0x8960FA, bytes(v)))
        if k == len(u) - 4:
            continue  # (the ETX without its parity bit is not 0x97: still a block, no longer "more to come" either way)
        assert (not it.valid and "Parity error" in it.error) if bad else (it.valid and it.error is None), k
    v = bytearray(acars.acars_userdata(".A6-EDY", "2", "\x15", "H1", "A", None))
    v[16] ^= 0x80  # a header-only block: nothing behind byte 15 is text
    assert acars.parse_msg(row_of(0x8960FA, bytes(v))).valid


def test_three_blocks_become_one_message():
    d = acars.AcarsDefragmenter()
    assert d.push(block("FIRST ", "A", True)) is None
    assert d.push(block("other aircraft", "A", False, reg=".9V-SKM", aesid=0x76CD6D)).message == "other aircraft"
    assert d.push(block("SECOND ", "B", True)) is None
    out = d.push(block("THIRD", "C", False))
    assert out is not None and out.message == "FIRST SECOND THIRD" and chr(out.BI) == "C" and not out.moretocome and not d.frags
    z = acars.AcarsDefragmenter()
    assert z.push(block("1", "Z", True)) is None and z.push(block("2", "A", False)).message == "12"  # the block id wraps


def test_a_tak_mismatch_and_a_bi_gap_do_not_join():
    d = acars.AcarsDefragmenter()
    assert d.push(block("FIRST ", "A", True)) is None
    out = d.push(block("LAST", "B", False, tak="\x16"))
    assert out.message == "LAST" and len(d.frags) == 1
    out = d.push(block("LAST", "C", False))
    assert out.message == "LAST" and len(d.frags) == 1
    assert d.push(block("LAST", "B", False)).message == "FIRST LAST"


def test_a_fragment_ages_out_after_thirty():
    d = acars.AcarsDefragmenter()
    assert d.push(block("FIRST ", "A", True)) is None
    for i in range(30):
        assert d.push(block("noise", "A", False, reg=".9V-SKM")) is not None
    assert len(d.frags) == 1 and d.frags[0][1] == 30
    assert d.push(block("LAST", "B", False)).message == "LAST" and not d.frags  # the 31st push dropped it before looking
    e = acars.AcarsDefragmenter()
    assert e.push(block("FIRST ", "A", True)) is None
    for i in range(29):
        e.push(block("noise", "A", False, reg=".9V-SKM"))
    assert e.push(block("LAST", "B", False)).message == "FIRST LAST"
