"""The streams the ISU reassembly is tested on (tests/test_isu_oracle.py, tests/test_aerol_isu_emul.py, tests/test_gpu_aerol_isu.py): the smallest
sequences of signal units in which each rule of the definition (include/jaero_hip.h) can go wrong, packed into P-channel frames with
jaero_amd.aerol_frames and turned into soft bits.  A script is a list of 10-byte payloads; SCRIPTS names them, stream(name, fb) builds one."""
import functools

import numpy as np

from jaero_amd import acars
from jaero_amd import aerol_frames as AF

# what the off-air recording tests/golden/recording_oqpsk_10k5.npz reassembles into: (AESID, GESID, QNO, REFNO, bytes) in order, and the
# registrations of the five that are ACARS headers
RECORDING_MESSAGES = [(0x8960FA, 0x90, 7, 2, 19), (0x89618E, 0x90, 7, 5, 19), (0x34210A, 0x90, 0, 8, 36), (0x8960C8, 0x90, 2, 13, 15),
                      (0x89607F, 0x90, 3, 10, 10), (0x76CD6D, 0x90, 7, 14, 19), (0x34210A, 0x90, 0, 2, 56), (0x06A07D, 0x90, 7, 7, 19),
                      (0x706049, 0x90, 7, 4, 19), (0x89604A, 0x90, 2, 3, 10)]
RECORDING_REGS = [b".A6-EDY", b".A6-EEO", b".9V-SKM", b".A7-BBG", b".9K-GBA"]
FILL = bytes([0x01] + [0] * 9)
PER_FRAME = {600: 6, 1200: 6, 10500: 26}
A, B, C_, D = 0x8960FA, 0x34210A, 0x76CD6D, 0x06A07D
GES = 0x90


def isu(aes, qno, refno, seqno, nooct, u0=0x11, u1=0x22, ges=GES):
    return bytes([0x71, (aes >> 16) & 255, (aes >> 8) & 255, aes & 255, ges, (qno << 4) | refno, seqno & 63, (nooct << 4) | 0x05, u0, u1])


def ssu(seqno, qno, refno, tag=0):
    return bytes([0xC0 | (seqno & 63), (qno << 4) | refno] + [(tag + 16 * seqno + i) & 255 for i in range(8)])


def raw_message(aes, qno, refno, nssu, nooct, tag=0):
    """An ISU announcing nssu SSUs and NOOCT octets in the last one, and those SSUs (all eight bytes of the last one filled: the reassembly
    must take only NOOCT of them)."""
    return [isu(aes, qno, refno, nssu, nooct, u0=tag & 255, u1=nssu)] + [ssu(nssu - 1 - i, qno, refno, tag) for i in range(nssu)]


def acars_message(aes, qno, refno, reg, text, bi="A", more=False, tak="\x15", label="H1", mode="2", damage=None):
    u = bytearray(acars.acars_userdata(reg, mode, tak, label, bi, text, more))
    if damage is not None:
        u[damage] ^= 0x80  # one parity bit
    return acars.isu_payloads(aes, GES, qno, refno, bytes(u))


def _sizes():
    out, r = [], 0
    for nssu in (1, 2, 30, 63):  # the 63-SSU ones span frames at every rate (11 frames of 6 units, 3 of 26)
        for nooct in (0, 1, 8):
            out += raw_message(A + r, r % 16, (r * 3) % 16, nssu, nooct, tag=7 * r) + [FILL]
            r += 1
    return out


def _quirks():
    s = []
    # two aircraft interleaved with the same QNO / REFNO / SEQNO: the SSUs continue the LAST ISU's aircraft, the older one's are missing
    s += [isu(A, 3, 4, 2, 5), isu(B, 3, 4, 2, 5), ssu(1, 3, 4, 1), ssu(0, 3, 4, 1), ssu(1, 3, 4, 2), ssu(0, 3, 4, 2), FILL]
    # NOOCT = 9: appended, appended again as a duplicate, never matched; every SSU behind it is missing -- until the next good ISU
    s += [isu(C_, 1, 1, 1, 9), isu(C_, 1, 1, 1, 9), ssu(0, 1, 1, 3), ssu(0, 1, 1, 3)] + raw_message(C_, 1, 1, 1, 3, tag=4)
    # an item with NOOCT 9 found after all, through a later ISU of the same aircraft that left a.NOOCT = 2: the unit's eight bytes, no more
    s += [isu(D, 7, 7, 1, 9), isu(D, 7, 8, 1, 2), ssu(0, 7, 7, 13), FILL]
    # a repeated ISU restarts its item: the first SSU's eight bytes are gone
    s += [isu(D, 5, 6, 2, 4), ssu(1, 5, 6, 5), isu(D, 5, 6, 2, 4), ssu(1, 5, 6, 6), ssu(0, 5, 6, 6), FILL]
    # ageing: ten ISUs behind an item leave it in the list (count 10), an eleventh removes it.  The others are the same aircraft with other
    # REFNOs, so that `a` still names the aircraft when the SSU comes
    s += [isu(A, 9, 0, 1, 6)] + [isu(A, 9, 1 + i, 1, 6) for i in range(10)] + [ssu(0, 9, 0, 7)]
    s += [isu(B, 9, 0, 1, 6)] + [isu(B, 9, 1 + i, 1, 6) for i in range(11)] + [ssu(0, 9, 0, 8)]
    # twelve different aircraft in a row: the list never holds more than eleven
    s += [isu(0x100000 + i, 2, 2, 1, 2) for i in range(12)] + [ssu(0, 2, 2, 9)]
    # SEQNO 0 in the ISU: nothing can complete it
    s += [isu(C_, 4, 4, 0, 3), ssu(0, 4, 4, 10), ssu(63, 4, 4, 10)]
    # the last SSU repeated: missing
    s += raw_message(D, 6, 1, 2, 7, tag=11) + [ssu(0, 6, 1, 11)]
    # AESID 0
    s += raw_message(0, 1, 2, 1, 8, tag=12)
    # units that are neither: LSDUs, a broadcast, fill-in
    s += [bytes([0x74] + list(range(9))), bytes([0x76] + list(range(9))), bytes([0x0A] + [0xC1] * 9), FILL]
    return s


def _acars():
    s = []
    s += acars_message(A, 7, 2, ".A6-EDY", None)                                   # the 19-byte header-only block of the off-air recording
    s += acars_message(B, 0, 8, ".9V-SKM", "POSN 33.5S 151.2E\r\n/TS 120000")
    s += acars_message(B, 0, 9, ".9V-SKM", "X" * 220, bi="A", more=True)            # ETB
    s += acars_message(C_, 2, 3, ".A7-BBG", "DEL \x7f IN TEXT")
    s += acars_message(C_, 2, 4, ".A7-BBG", "PARITY IN REG", damage=6)
    s += acars_message(C_, 2, 5, ".A7-BBG", "PARITY IN TEXT", damage=20)
    s += acars_message(C_, 2, 6, ".A7-BBG", "BLOCK CHECK AND DEL ARE NOT CHECKED", damage=-2)
    s += acars.isu_payloads(D, GES, 1, 1, bytes([0xFF, 0xFF] + [0x31] * 13 + [0x83]))  # 16 bytes: one short of the pattern
    s += acars.isu_payloads(D, GES, 1, 2, bytes([0xFF, 0xFF] + [0x31] * 13 + [0x03, 1, 2, 3, 4]))  # byte 15 is neither 0x83 nor 0x02
    return s


def _tail():
    """Two long messages for the stream-level damage: a unit that fails its CRC in the first (31 units), a frame cut short under the second
    (64 units: at every rate its ISU is out of the decoder before the cut and SSUs follow behind it).  The units lost with the cut frame
    break the second message's chain whether or not the list is reset, so the reset shows elsewhere: a one-SSU item of the same aircraft is
    opened in front of the long message and its SSU comes behind it -- `a` still names the aircraft (it survives the reset), the item is
    gone, the SSU is missing; without the reset it would complete.  Then a fresh message (complete)."""
    return (raw_message(A, 8, 8, 30, 5, tag=40) + [FILL, isu(B, 8, 9, 1, 5)] + raw_message(B, 8, 10, 63, 5, tag=50) + [ssu(0, 8, 9, 51), FILL]
            + raw_message(C_, 8, 10, 3, 2, tag=60))


SCRIPTS = {"sizes": _sizes, "quirks": _quirks, "acars": _acars, "tail": _tail}


def frames_of(units, fb):
    n = PER_FRAME[fb]
    return [units[i:i + n] for i in range(0, len(units), n)]


def coded_positions(fb, frame, k, lo=24, hi=72):
    """Positions, in the channel-bit stream p_channel_bits returns, of the coded bits of information bits lo .. hi - 1 of unit k of `frame`."""
    g = AF.geometry(fb)
    ncols, blk = g["ncols"], 64 * g["ncols"]
    flen = g["uw"] + g["header"] + g["dummy"] + g["nbits"]
    pos = []
    for b in range(k * 96 + lo, k * 96 + hi):
        for c in (2 * b, 2 * b + 1):
            block, within = divmod(c, blk)
            j, i = divmod(within, 64)
            pos.append(frame * flen + g["uw"] + g["header"] + g["dummy"] + block * blk + ((i * 27) % 64) * ncols + j)
    return np.array(pos)


@functools.lru_cache(maxsize=None)
def stream(name: str, fb: int, inv=(False, False), lead: int = 0, sigma: float = 8.0):
    """Soft bits (int16) of one script at one rate.  "tail" carries the two stream-level cases: the coded bits of the middle of one SSU
    inverted (the unit fails its CRC), and 100 channel bits cut out of a frame in mid-message (the next unique word comes early: the
    short-frame notice, a kind-1 event)."""
    units = list(SCRIPTS[name]())
    n = PER_FRAME[fb]
    units = [FILL] * n + units  # a frame of fill-in units first: the decoder's delay line starts empty and it loses the stream's first frame
    frames = frames_of(units, fb) + [[FILL] * n] * 3  # the decoder hands a frame out one or two frames later
    bits, flen = AF.p_channel_bits(frames, fb, invert_i=inv[0], invert_q=inv[1])
    soft = AF.to_soft(bits, sigma=sigma, seed=len(units) + fb)
    if name == "tail":
        u_bad = n + 12                       # the 12th unit of the first long message: an SSU in its middle
        p = coded_positions(fb, u_bad // n, u_bad % n)
        soft[p] = 255 - soft[p]
        # the second message's ISU leaves the decoder delay_frames after the frame that carries it; the cut is in the frame after that
        f = (n + 33) // n + AF.geometry(fb)["delay_frames"] + 1
        at = f * flen + flen // 2
        soft = np.concatenate([soft[:at], soft[at + 100:]])
    if lead:
        rng = np.random.default_rng(lead)
        soft = np.concatenate([AF.to_soft(rng.integers(0, 2, lead, dtype=np.uint8), sigma=sigma, seed=lead), soft])
    return soft


NAMES = tuple(SCRIPTS)


def channel_plan(nch: int, fb: int):
    """(name, inv, lead) per channel: the four scripts in turn, arm inversions at 10 500 bps, a garbage prefix on every third channel."""
    plan = []
    for c in range(nch):
        inv = (bool(c & 4), bool(c & 8)) if fb == 10500 else (False, False)
        plan.append((NAMES[c % len(NAMES)], inv, 0 if c % 3 else 37 + 100 * (c % 5)))
    return plan


_EXPECTED = {}


def expected(O, name, fb, inv=(False, False), lead=0):
    """What the definition gives for one stream: (message rows, stats int64[4], [(frame, k)] of the missing SSUs, signal-unit rows, event
    rows), computed once per stream and shared (nobody changes it)."""
    import isu_oracle as IO

    key = (name, fb, inv, lead)
    if key not in _EXPECTED:
        chan, sus, ev = IO.run_stream(O, fb, stream(name, fb, inv, lead))
        _EXPECTED[key] = (chan.take(), chan.stats, list(chan.missing), sus, ev)
    return _EXPECTED[key]
