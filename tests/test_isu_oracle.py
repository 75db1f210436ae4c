"""CPU: what anchors tests/isu_oracle.py, the definition the device code is held to.
  * An off-air recording: the CRC-clean signal units the unmodified reference printed for its own recording (tests/golden/
    recording_oqpsk_10k5.npz, `sus`) reassemble into ten ISUs with no SSU missing, five of them well-formed ACARS headers with odd parity on
    every registration byte.
  * The unmodified reference (oracle/_ref, where it is built): " missing (or if unimplimented then TODO in C++)" behind a printed SSU is the
    one thing it shows of ISUData; over the case streams that set of lines equals the oracle's missing SSUs, position for position.
  * The case set itself: every quirk produces what it is there for, so that neither comparison passes on nothing."""
import re

import numpy as np
import pytest

import isu_cases as IC
import isu_oracle as IO
from conftest import load_golden
from jaero_amd import acars

MISSING = " missing (or if unimplimented then TODO in C++)"
TEN, REGS = IC.RECORDING_MESSAGES, IC.RECORDING_REGS


def test_the_off_air_recording_gives_ten_messages():
    g = load_golden("recording_oqpsk_10k5")
    sus = g["sus"].astype(np.int32)  # what the reference printed: [unit index k, 10 payload bytes, crc ok]
    assert sus.shape[1] == 12 and int(sus[:, 11].sum()) == 468
    rows = np.zeros((len(sus), 16), np.int32)
    rows[:, 0] = np.concatenate([[0], np.cumsum(np.diff(sus[:, 0]) <= 0)])  # a frame ends where k stops rising
    rows[:, 1], rows[:, 2:12], rows[:, 14] = sus[:, 0], sus[:, 1:11], sus[:, 11]
    ch = IO.Channel()
    ch.units(rows)
    msgs = ch.take()
    assert [(int(m["aesid"]), int(m["gesid"]), int(m["qno"]), int(m["refno"]), int(m["nbytes"])) for m in msgs] == TEN
    assert ch.missing == [] and ch.stats[2] == 0 and ch.stats[3] == 10
    hdr = [m for m in msgs if m["nbytes"] == 19]
    assert [int(m["flags"]) for m in hdr] == [IO.F_ACARS] * 5  # the pattern, no text, ETX, every registration byte with odd parity
    assert [bytes(m["data"][4:11] & 0x7F) for m in hdr] == REGS
    assert all(int(m["flags"]) == 0 for m in msgs if m["nbytes"] != 19)
    # and the module users read rows with agrees, field by field
    assert acars.MSG_DTYPE == IO.MSG
    assert [acars.parse_msg(m).PLANEREG for m in hdr] == REGS and all(acars.parse_msg(m).valid for m in msgs)


def test_every_case_does_what_it_is_there_for(oracle_mod):
    fb = 1200
    done = 0
    for name in IC.NAMES:
        done += len(IC.expected(oracle_mod, name, fb)[0])
    assert done >= 20
    msgs, stats, missing, sus, ev = IC.expected(oracle_mod, "sizes", fb)
    assert [int(m["nbytes"]) for m in msgs] == [2 + 8 * (n - 1) + o for n in (1, 2, 30, 63) for o in (0, 1, 8)] and not missing
    assert len(set(int(m["frame"]) for m in msgs[-3:])) == 3 and int(msgs[-1]["frame"]) - int(msgs[-2]["frame"]) >= 10  # they span frames
    msgs, stats, missing, sus, ev = IC.expected(oracle_mod, "quirks", fb)
    assert list(stats) == [47, 20, 8, 8]
    # interleaved aircraft: the younger one completes; NOOCT 9: the good ISU behind it, and the NOOCT 9 item found after all; the restarted item: 2 + 8 + 4 bytes; ageing: ten
    # ISUs leave the item, eleven remove it; twelve aircraft: the last; the repeated last SSU: once; AESID 0
    assert [(int(m["aesid"]), int(m["nbytes"]), int(m["flags"])) for m in msgs] == [
        (IC.B, 15, 0), (IC.C_, 5, 0), (IC.D, 10, 0), (IC.D, 14, 0), (IC.A, 8, 0), (0x10000B, 4, 0), (IC.D, 17, 0), (0, 10, IO.F_AES0)]
    assert int(msgs[2]["nooct"]) == 9 and bytes(msgs[2]["data"][2:10]) == IC.ssu(0, 7, 7, 13)[2:]  # NOOCT 9, matched through a.NOOCT = 2
    assert bytes(msgs[3]["data"][2:10]) == IC.ssu(1, 5, 6, 6)[2:]  # the SSU behind the repeated ISU, not the one in front of it
    msgs, stats, missing, sus, ev = IC.expected(oracle_mod, "acars", fb)
    A, T, M, P = IO.F_ACARS, IO.F_TEXT, IO.F_MORE, IO.F_PARITY
    assert [int(m["flags"]) for m in msgs] == [A, A | T, A | T | M, A | T, A | T | P, A | T | P, A | T, 0, 0]
    assert (int(msgs[0]["mode"]), int(msgs[0]["tak"]), bytes(msgs[0]["label"]), int(msgs[0]["bi"])) == (ord("2"), 0x15, b"H1", ord("A"))
    assert not msgs[-1]["mode"] and not msgs[-1]["label"].any()
    # the tail: a unit fails its CRC inside the first long message, a short frame (the second kind-1 event: the first is the stream's
    # first unique word) resets the list under the second, and only the message behind both completes
    msgs, stats, missing, sus, ev = IC.expected(oracle_mod, "tail", fb)
    assert int((ev[:, 1] == 1).sum()) == 2 and [(int(m["aesid"]), int(m["nbytes"])) for m in msgs] == [(IC.C_, 20)]
    bad = sus[(sus[:, 2] & 0xC0) == 0xC0]
    assert (bad[:, 14] == 0).any()
    deaf = IO.Channel()
    deaf.short_frame = lambda: None
    IO.run_stream(oracle_mod, fb, IC.stream("tail", fb), deaf)
    # without the reset the SSU behind the long message would still have found the item opened in front of it
    assert len(deaf.missing) == len(missing) - 1 and [int(m["aesid"]) for m in deaf.take()] == [IC.B, IC.C_]


@pytest.fixture(scope="module")
def R(oracle_mod):
    if not oracle_mod.have_ref():
        pytest.skip("oracle/_ref/jaero_ref not available here")
    try:
        oracle_mod.run_ref_aerol(1200, np.zeros(24, np.int16), 12)
    except Exception as e:
        pytest.skip(f"_ref cannot run here: {e}")
    return oracle_mod


@pytest.mark.parametrize("fb", [1200, 10500])
def test_missing_ssus_are_the_unmodified_references(R, fb):
    nmissing = 0
    for name in IC.NAMES:
        for inv, lead in (((False, False), 0), ((True, False), 137)) if fb == 10500 else (((False, False), 0),):
            soft = IC.stream(name, fb, inv, lead)
            _, txt = R.run_ref_aerol(fb, soft, 32 if fb == 10500 else 12)
            lines = [m for m in (re.match(r"^(.)((?: 0x[0-9A-F]{2}){10})(.*)$", ln) for ln in txt.split("\n")) if m]
            _, _, missing, sus, _ = IC.expected(R, name, fb, inv, lead)
            assert [(ord(m.group(1)) - ord("0"), bytes(int(x, 16) for x in m.group(2).split())) for m in lines] == [
                (int(r[1]), bytes(r[2:12].astype(np.uint8))) for r in sus], (name, "the printed units are not the oracle's")
            ref = [i for i, m in enumerate(lines) if m.group(3).endswith(MISSING)]
            where = {(int(r[0]), int(r[1])): i for i, r in enumerate(sus)}
            assert ref == [where[fk] for fk in missing], (name, fb)
            nmissing += len(ref)
    assert nmissing >= 8 + 60
