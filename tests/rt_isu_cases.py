"""The streams the burst bank's R / T reassembly is tested on (tests/test_rt_isu_oracle.py, tests/test_aerolb_isu_emul.py,
tests/test_gpu_aerol_rt.py): the smallest sequences of R and T packets in which each rule of the definition (include/jaero_hip.h) can go
wrong, turned into bursts with jaero_amd.aerol_frames.  A case is a list of entries ("R", 17 bytes, bad) | ("T", [10-byte units], bad) |
("Traw", (header, units as sent), bad); CASES names them, stream(name, fb) builds one.  `bad`: the fields sent with a wrong CRC (0 = the R
payload / the T header, k = the k-th unit sent, from 1)."""
import functools

import numpy as np

import isu_cases as IC
from jaero_amd import acars
from jaero_amd import aerol_frames as AF

A, B, C_, D, GES, FILL = IC.A, IC.B, IC.C_, IC.D, IC.GES, IC.FILL
T_AES = 0x4CA2D1  # the aircraft in the T packets' own header (the units name theirs)
GAP = {600: 4200, 1200: 4200, 10500: 8000}  # soft bits of noise behind a burst: past the frame countdown, and past the 95 columns a refused T packet collects


def r(seqind, sutype, aes, qno, refno, tag=0, ges=GES, flag=8):
    """One R packet payload; the data bytes count up from `tag`.  flag = 0: not user data."""
    return bytes([(seqind << 4) | sutype, (qno << 4) | flag | (refno & 7), (aes >> 16) & 255, (aes >> 8) & 255, aes & 255, ges] + [(tag + i) & 255 for i in range(11)])


def R(p, bad=()):
    return ("R", bytes(p), tuple(bad))


def T(units, bad=()):
    return ("T", [bytes(u) for u in units], tuple(bad))


def r_message(aes, qno, refno, n, ges=GES, tag=0):
    return [R(p) for p in acars.r_isu_payloads(aes, ges, qno, refno, bytes((tag + 3 * i) & 255 for i in range(n)))]


def _r_sizes(fb):
    s = []
    for k, n in enumerate((1, 5, 11, 12, 22, 23, 33)):  # one, two and three units, in order
        s += r_message(A + k, k, k % 8, n, tag=16 * k)
    # three units with the last first (sized 25 by the last, not grown by the first), with the middle first (sized 33, cut to 24 by the last),
    # and with a short last first, then the full first: shrink-then-no-grow
    s += [R(r(6, 3, B, 1, 1, 0x60)), R(r(4, 11, B, 1, 1, 0x40)), R(r(5, 11, B, 1, 1, 0x50))]
    s += [R(r(5, 11, B, 1, 2, 0x50)), R(r(4, 11, B, 1, 2, 0x40)), R(r(6, 2, B, 1, 2, 0x60))]
    s += [R(r(6, 2, B, 1, 3, 0x60)), R(r(4, 11, B, 1, 3, 0x40)), R(r(5, 9, B, 1, 3, 0x50))]
    # a repeated unit
    s += [R(r(2, 11, C_, 2, 1, 0x10)), R(r(2, 11, C_, 2, 1, 0x20)), R(r(3, 4, C_, 2, 1, 0x30))]
    # a middle unit with SUTYPE 5: bytes 16 .. 21 are written by nobody
    s += [R(r(4, 11, D, 3, 1, 0x40)), R(r(5, 5, D, 3, 1, 0x50)), R(r(6, 11, D, 3, 1, 0x60))]
    return s


def _r_keys(fb):
    s = []
    # two aircraft interleaved, same QNO / REFNO
    s += [R(r(4, 11, A, 3, 4, 1)), R(r(4, 11, B, 3, 4, 2)), R(r(5, 11, A, 3, 4, 3)), R(r(5, 11, B, 3, 4, 4)), R(r(6, 7, B, 3, 4, 5)), R(r(6, 6, A, 3, 4, 6))]
    # REFNO 2 and 10 are one key: the second message's first unit lands in the first one's item
    s += [R(r(2, 11, C_, 5, 2, 0x11)), R(r(2, 11, C_, 5, 10, 0x22)), R(r(3, 8, C_, 5, 10, 0x33)), R(r(3, 8, C_, 5, 2, 0x44))]
    # SUTYPE 15 beside a pending item of the same key: a fresh item, emitted at once; the pending one completes later
    s += [R(r(2, 11, D, 6, 1, 0x55)), R(r(1, 15, D, 6, 1, 0x66)), R(r(4, 15, D, 6, 1, 0x67)), R(r(3, 3, D, 6, 1, 0x77))]
    # SUTYPE 0 and 12 .. 14: a fresh item each time; with SEQINDICATOR 1 an empty message, with 2 an item of eleven zeros that never completes
    s += [R(r(1, t, A, 7, 1, t)) for t in (0, 12, 13, 14)] + [R(r(2, t, A, 7, 2, t)) for t in (0, 12)]
    # SEQINDICATOR 0 and 7: never complete; the data grows by the writes past its end
    s += [R(r(0, 5, B, 8, 1, 0x01)), R(r(7, 9, B, 8, 1, 0x02)), R(r(0, 3, B, 8, 1, 0x03))]
    # AESID 0
    s += [R(r(1, 6, 0, 1, 1, 0x70))]
    # mixed totals for one key: 4 then 3 completes as a two-unit message of 15 bytes; 2 then 6 never does (filledarray 5)
    s += [R(r(4, 11, C_, 9, 1, 0x80)), R(r(3, 4, C_, 9, 1, 0x90))]
    s += [R(r(2, 11, C_, 9, 2, 0xA0)), R(r(6, 3, C_, 9, 2, 0xB0))]
    # an R packet that is not user data (bit 3 of byte 1 clear), with the bytes of a complete one-unit message
    s += [R(r(1, 11, D, 10, 1, 0xC0, flag=0))]
    return s


def _r_age(fb):
    """Every update ages the list before it looks anything up -- the update that brings the late unit too."""
    s = []
    # pending, nine other user-data packets, the second unit: its own update makes the count 10, the item is still there
    s += [R(r(2, 11, A, 1, 1, 0x10))] + [R(r(1, 2, 0x200000 + i, 2, 2, i)) for i in range(9)] + [R(r(3, 5, A, 1, 1, 0x20))]
    # ten others: the late unit's own update makes the count 11 and removes the item, the unit opens a new one, which never completes
    s += [R(r(2, 11, B, 1, 1, 0x30))] + [R(r(1, 2, 0x300000 + i, 2, 2, i)) for i in range(10)] + [R(r(3, 5, B, 1, 1, 0x40))]
    # eleven others: gone before the late unit comes
    s += [R(r(2, 11, C_, 1, 1, 0x50))] + [R(r(1, 2, 0x500000 + i, 2, 2, i)) for i in range(11)] + [R(r(3, 5, C_, 1, 1, 0x60))]
    # twelve pending items of different aircraft in a row: the list never holds more than eleven, and only the oldest has left
    s += [R(r(2, 11, 0x400000 + i, 3, 3, i)) for i in range(12)] + [R(r(3, 1, 0x400000, 3, 3, 0x70)), R(r(3, 1, 0x400003, 3, 3, 0x71))]
    return s


def _r_acars(fb):
    s = []
    hdr = acars.acars_userdata(".A6-EDY", "2", "\x15", "H1", "A", None)  # 19 bytes: two R packets
    s += [R(p) for p in acars.r_isu_payloads(A, GES, 7, 2, hdr)]
    txt = acars.acars_userdata(".9V-SKM", "2", "\x15", "Q0", "B", "POS OK 12")  # 29 bytes: three
    s += [R(p) for p in acars.r_isu_payloads(B, GES, 0, 5, txt)]
    bad = bytearray(acars.acars_userdata(".A7-BBG", "2", "\x15", "H1", "C", "PARITY"))
    bad[18] ^= 0x80
    s += [R(p) for p in acars.r_isu_payloads(C_, GES, 2, 3, bytes(bad))]
    more = acars.acars_userdata(".A7-BBG", "2", "\x15", "H1", "D", "MORE", more=True)
    s += [R(p) for p in acars.r_isu_payloads(C_, GES, 2, 4, more)]
    return s


def _t_basic(fb):
    s = []
    s += [T(IC.raw_message(A, 1, 2, 3, 5, tag=7))]                       # an ISU and its SSUs in one packet
    m = IC.raw_message(B, 2, 3, 6, 8, tag=9)
    s += [T(m[:4]), T(m[4:])]                                            # a message spanning two bursts
    m = IC.raw_message(C_, 3, 4, 3, 1, tag=11)
    s += [T([FILL, m[0], FILL, m[1], m[2], FILL]), T([FILL, FILL, m[3]])]  # fill-in units between
    s += [T(IC.acars_message(D, 7, 2, ".A6-EDY", "T CHANNEL TEXT"))]
    s += [T(IC.raw_message(0, 1, 2, 1, 8, tag=12) + [FILL])]             # AESID 0
    return s


def _t_missing(fb):
    s = []
    m = IC.raw_message(A, 4, 5, 6, 3, tag=21)
    s += [T(m[:1] + [FILL, FILL], bad=(0,)), T(m[1:])]                   # the packet with the ISU is refused: all six SSUs are missing
    m = IC.raw_message(B, 5, 6, 2, 7, tag=23)
    s += [T(m + [m[-1], m[-1]])]                                         # the last SSU repeated twice: missing twice
    s += [T([IC.isu(C_, 6, 7, 2, 4), IC.ssu(1, 6, 8, 1), IC.ssu(1, 7, 7, 1), IC.ssu(1, 6, 7, 2), IC.ssu(0, 6, 7, 2)])]  # other REFNO, other QNO
    return s


def _t_msk(fb):
    """600 / 1200 bps: a unit sent with a wrong CRC is fed all the same, and the last unit sent is never looked at (here: an SSU that would
    be missing).  At 10 500 bps a unit with a wrong CRC refuses the packet, so the same units are sent clean there."""
    m = IC.raw_message(D, 8, 1, 3, 6, tag=31)
    if fb == 10500:
        return [T(m), T([FILL, FILL])]
    hdr = bytes([(T_AES >> 16) & 255, (T_AES >> 8) & 255, T_AES & 255, GES])
    late = IC.ssu(0, 8, 1, 99)
    return [("Traw", (hdr, [m[0], FILL, m[1], m[2], m[3], late]), (4,)),  # unit 3 (the fourth sent) with a wrong CRC
            ("Traw", (hdr, [FILL, FILL, FILL, FILL, late]), ())]


def _mixed(fb):
    t = IC.raw_message(A, 1, 1, 4, 2, tag=41)
    rr = r_message(A, 1, 1, 30, tag=43)  # the same aircraft, QNO and REFNO on the R channel: the two state machines do not meet
    return [T(t[:2]), rr[0], rr[1], T(t[2:4]), rr[2], T(t[4:] + [FILL]), R(r(1, 15, B, 2, 2))] + r_message(C_, 3, 3, 9, tag=45)


def _noise(fb):
    return []


CASES = {"r_sizes": _r_sizes, "r_keys": _r_keys, "r_age": _r_age, "r_acars": _r_acars, "t_basic": _t_basic, "t_missing": _t_missing, "t_msk": _t_msk,
         "mixed": _mixed, "noise": _noise}
NAMES = tuple(n for n in CASES if n != "noise")


def entries(name: str, fb: int):
    return CASES[name](fb)


def good_packets(name: str, fb: int) -> int:
    """Packets of a case the search accepts: all but those with a wrong header / payload CRC (and, at 10 500 bps, a wrong unit CRC)."""
    return sum(1 for _, _, bad in entries(name, fb) if not bad or (fb != 10500 and 0 not in bad))


def packet_bits(fb: int, kind: str, payload, bad):
    msk = fb != 10500
    if kind == "T":
        payload = acars.t_packets(T_AES, GES, payload, len(payload), msk=msk)[0]
    kind = "R" if kind == "R" else "T"
    return AF.rt_packet_bits_msk(kind, payload, bad_crc=bad) if msk else AF.rt_packet_bits(kind, payload, bad_crc=bad)


@functools.lru_cache(maxsize=None)
def stream(name: str, fb: int, inv=(False, False), sigma: float = 14.0, lead: int = 80):
    """Soft bits (int16) of one case at one rate, as a burst demodulator emits them: noise, then per burst the start-of-burst marker (-1),
    `lead` soft bits of noise, the unique word (on both arms at 10 500 bps), the packet, and GAP[fb] soft bits of noise
    (aerol_frames.rt_burst_stream / rt_burst_stream_msk, with the wrong CRCs a case asks for)."""
    seed = 1000 * (list(CASES).index(name) + 1) + fb % 1000 + 2 * int(inv[0]) + int(inv[1])
    rng = np.random.default_rng(seed)
    noise = lambda n: np.clip(np.round(128 + rng.normal(0, 40, n)), 0, 255).astype(np.int16)
    uw = np.array([(AF.UW >> (31 - k)) & 1 for k in range(32)], dtype=np.uint8)
    out = [noise(64)]
    if name == "noise":
        out.append(noise(9000))
    for kind, payload, bad in entries(name, fb):
        pb = packet_bits(fb, kind, payload, bad)
        if fb == 10500:
            bits = np.concatenate([np.repeat(uw, 2), pb])
            if inv[0]:
                bits[0::2] ^= 1
            if inv[1]:
                bits[1::2] ^= 1
        else:
            bits = np.concatenate([uw, pb]) ^ (1 if inv[0] else 0)
        out += [np.array([-1], dtype=np.int16), noise(lead + (lead & 1)), AF.to_soft(bits, sigma=sigma, seed=int(rng.integers(1 << 30))), noise(GAP[fb])]
    return np.concatenate(out)


def channel_plan(nch: int, fb: int, noise_every: int = 7):
    """(name, inv) per channel: the cases in turn, arm inversions, every `noise_every`-th channel noise only."""
    plan, k = [], 0
    for c in range(nch):
        if noise_every and c % noise_every == noise_every - 1:
            plan.append(("noise", (False, False)))
            continue
        inv = (bool(k & 8), bool(k & 16)) if fb == 10500 else (bool(k & 8), False)
        plan.append((NAMES[k % len(NAMES)], inv))
        k += 1
    return plan


_EXPECTED = {}


def expected(O, name, fb, inv=(False, False)):
    """What the definition gives for one stream: (message rows, stats int64[8], [(packet, k)] of the missing SSUs, packet rows, event rows,
    the Channel), computed once per stream and shared (nobody changes it)."""
    import rt_isu_oracle as RO

    key = (name, fb, inv)
    if key not in _EXPECTED:
        chan, pk, ev = RO.run_stream(O, fb, stream(name, fb, inv))
        _EXPECTED[key] = (chan.take(), chan.stats, list(chan.missing), pk, ev, chan)
    return _EXPECTED[key]
