"""ISU user data and ACARS blocks: the host side of the Aero-L bank's message log (AeroLBank.read_msgs, include/jaero_hip.h jaero_aerol_msg).

  * generators, the inverse of what the reference decodes: isu_payloads (an ISU 0x71 and its SSUs, JAERO/aerol.cpp:152-219) and
    acars_userdata (the byte pattern ParserISU::parse looks for, aerol.cpp:365-396)
  * r_isu_payloads (the one to three R packets RISUData::update puts back together, aerol.cpp:28-113) and t_packets (10-byte units as T packet
    payloads) for the burst bank's reassembly (AeroLBank.rt_enable)
  * parse_msg: a log row -> the ACARSItem fields ParserISU::parse fills in (aerol.cpp:340-480), text included
  * AcarsDefragmenter: ACARSDefragmenter (aerol.cpp:221-329) restated, one per channel

The plane database (dbtu->request) is not here."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

MSG_DTYPE = np.dtype([("frame", "<i4"), ("k", "<i4"), ("aesid", "<u4"), ("gesid", "u1"), ("qno", "u1"), ("refno", "u1"), ("nooct", "u1"),
                      ("nbytes", "<u2"), ("flags", "<u2"), ("mode", "u1"), ("tak", "u1"), ("label", "u1", (2,)), ("bi", "u1"),
                      ("pad", "u1", (7,)), ("data", "u1", (512,))])  # struct jaero_aerol_msg
MSG_AES0, MSG_ACARS, MSG_TEXT, MSG_MORE, MSG_PARITY = 1, 2, 4, 8, 16  # jaero_aerol_msg.flags
MSG_RCHAN, MSG_RSIGNAL = 32, 64  # burst banks: the row comes from an R packet (RISUData); it is an R signalling-information unit
SOH, STX, ETX, ETB, DEL = 0x01, 0x02, 0x03, 0x17, 0x7F
MAX_USERDATA = 506  # 2 bytes in the ISU, 8 in each of at most 62 SSUs, at most 8 in the last
MAX_R_USERDATA = 33  # three R packets of 11 bytes
FILL_IN = bytes([0x01] + [0] * 9)


def odd_parity(b: int) -> int:
    """b's low seven bits with bit 7 chosen so that the byte has an odd number of ones."""
    b &= 0x7F
    return b | (0 if bin(b).count("1") & 1 else 0x80)


def isu_payloads(aesid: int, gesid: int, qno: int, refno: int, userdata: bytes) -> List[bytes]:
    """The ISU followed by its SSUs, as 10-byte signal-unit payloads: two bytes ride in the ISU, eight in every SSU but the last, which holds
    NOOCT = 1 .. 8 (0 when userdata is just the ISU's two bytes: one empty SSU completes it).  ISU.SEQNO = the number of SSUs; SSU i carries
    SEQNO = (number of SSUs) - i, i = 1 ..; every SSU repeats QNO and REFNO."""
    u = bytes(userdata)
    if not 2 <= len(u) <= MAX_USERDATA:
        raise ValueError(f"user data of {len(u)} bytes: an ISU with SSUs carries 2 .. {MAX_USERDATA}")
    if not (0 <= aesid < 1 << 24 and 0 <= gesid < 256 and 0 <= qno < 16 and 0 <= refno < 16):
        raise ValueError("aesid / gesid / qno / refno out of range")
    rest = u[2:]
    nssu = max(1, (len(rest) + 7) // 8)
    nooct = len(rest) - 8 * (nssu - 1)
    out = [bytes([0x71, (aesid >> 16) & 255, (aesid >> 8) & 255, aesid & 255, gesid, (qno << 4) | refno, nssu, nooct << 4, u[0], u[1]])]
    for i in range(nssu):
        chunk = rest[8 * i:8 * i + 8]
        out.append(bytes([0xC0 | (nssu - 1 - i), (qno << 4) | refno]) + chunk + bytes(8 - len(chunk)))
    return out


def r_isu_payloads(aesid: int, gesid: int, qno: int, refno: int, userdata: bytes) -> List[bytes]:
    """The one to three 17-byte R packet payloads that carry `userdata` (1 .. 33 bytes): byte 0 = SEQINDICATOR << 4 | SUTYPE (1 of 1; 2, 3 of
    two; 4, 5, 6 of three; SUTYPE = the bytes this unit holds, 1 .. 11), byte 1 = QNO << 4 | 8 | REFNO (three bits: bit 3 marks user data),
    AESID, GESID, then eleven data bytes, zero padded."""
    u = bytes(userdata)
    if not 1 <= len(u) <= MAX_R_USERDATA:
        raise ValueError(f"user data of {len(u)} bytes: R packets carry 1 .. {MAX_R_USERDATA}")
    if not (0 <= aesid < 1 << 24 and 0 <= gesid < 256 and 0 <= qno < 16 and 0 <= refno < 8):
        raise ValueError("aesid / gesid / qno / refno out of range (an R packet has three bits of REFNO)")
    n = (len(u) + 10) // 11
    first = {1: 1, 2: 2, 3: 4}[n]
    out = []
    for i in range(n):
        chunk = u[11 * i:11 * i + 11]
        out.append(bytes([((first + i) << 4) | len(chunk), (qno << 4) | 8 | refno, (aesid >> 16) & 255, (aesid >> 8) & 255, aesid & 255, gesid])
                   + chunk + bytes(11 - len(chunk)))
    return out


def t_packets(aesid: int, gesid: int, units, per_packet: int, msk: bool = False):
    """T packet payloads (4-byte header, [10-byte units]) for aerol_frames.rt_packet_bits, `per_packet` of `units` in each.  A 10 500 bps packet
    has at least two units: fill-in units make up the number.  msk = True, for aerol_frames.rt_packet_bits_msk (600 / 1200 bps): the unit at
    index 1 is a fill-in unit whose first byte the generator overwrites with the count, another closes the packet (the reference never looks at
    the last unit sent), and at least four are sent."""
    if per_packet < 1 or any(len(x) != 10 for x in units):
        raise ValueError("per_packet >= 1 and 10-byte units")
    hdr = bytes([(aesid >> 16) & 255, (aesid >> 8) & 255, aesid & 255, gesid])
    out = []
    for s in range(0, len(units), per_packet):
        us = [bytes(x) for x in units[s:s + per_packet]]
        if msk:
            us = us[:1] + [FILL_IN] + us[1:]
            us += [FILL_IN] * max(1, 4 - len(us))
        else:
            us += [FILL_IN] * max(0, 2 - len(us))
        out.append((hdr, us))
    return out


def _bcs(data: bytes) -> int:
    crc = 0  # CRC-16 / KERMIT over the block; the reference never checks it
    for byte in data:
        crc ^= byte
        for _ in range(8):
            crc = (crc >> 1) ^ 0x8408 if crc & 1 else crc >> 1
    return crc


def acars_userdata(reg: str, mode: str, tak: str, label: str, bi: str, text: Optional[str], more: bool = False) -> bytes:
    """FF FF, SOH, mode, seven registration bytes, TAK, two label bytes, BI, then STX + text + ETX (ETB if `more`) or -- text None -- ETX
    alone, two block-check bytes, DEL.  Bytes 2 .. the ETX / ETB carry odd parity in bit 7 (the reference checks it on the registration and
    on the text); the block check and DEL do not."""
    if len(reg) != 7 or len(label) != 2 or len(mode) != 1 or len(tak) != 1 or len(bi) != 1:
        raise ValueError("reg has 7 characters, label 2, mode / tak / bi 1")
    body = [SOH, ord(mode)] + [ord(ch) for ch in reg] + [ord(tak), ord(label[0]), ord(label[1]), ord(bi)]
    if text is None:
        if more:
            raise ValueError("a block without text ends in ETX")
        body.append(ETX)
    else:
        body += [STX] + [ord(ch) for ch in text] + [ETB if more else ETX]
    if any(b > 0x7F for b in body):
        raise ValueError("seven-bit characters only")
    par = bytes(odd_parity(b) for b in body)
    c = _bcs(par[1:])
    u = b"\xff\xff" + par + bytes([c & 255, c >> 8, DEL])
    if len(u) > MAX_USERDATA:
        raise ValueError(f"{len(u)} bytes of user data: at most {MAX_USERDATA} fit an ISU")
    return u


@dataclass
class AcarsItem:
    """ACARSItem (JAERO/aerol.h:176-211) as ParserISU::parse leaves it; `error` is the text of its Errorsignal when it returns false."""
    aesid: int = 0
    gesid: int = 0
    qno: int = 0
    refno: int = 0
    frame: int = 0
    k: int = 0
    userdata: bytes = b""
    valid: bool = False
    nonacars: bool = False
    hastext: bool = False
    moretocome: bool = False
    downlink: bool = False
    MODE: int = 0
    TAK: int = 0
    LABEL: bytes = b""
    BI: int = 0
    PLANEREG: bytes = b""
    message: str = ""
    error: Optional[str] = None
    dblookupresult: list = field(default_factory=list)


def parse_msg(row, downlink: bool = False) -> AcarsItem:
    """One jaero_aerol_msg row (numpy record of MSG_DTYPE) -> what ParserISU::parse makes of it.  downlink: the row is a burst bank's (R and T
    channels are the aircraft's side; a row that says it comes from an R packet is one anyway).  The header fields and the three decisions
    (AESID 0, ACARS or not, parity) are the row's, made on the device; the text is formed here: seven bits per byte, 0x7F as "<DEL>", and
    for anything that is not ACARS the upper-case hex of the user data."""
    n, flags = int(row["nbytes"]), int(row["flags"])
    u = bytes(row["data"][:n].tobytes())
    it = AcarsItem(aesid=int(row["aesid"]), gesid=int(row["gesid"]), qno=int(row["qno"]), refno=int(row["refno"]), frame=int(row["frame"]),
                   k=int(row["k"]), userdata=u, downlink=bool(downlink or flags & MSG_RCHAN))
    if flags & MSG_AES0:
        it.error = "Error: AESID == 0"
        return it
    if not flags & MSG_ACARS:
        it.nonacars = it.valid = True
        it.message = u.hex().upper()
        return it
    it.MODE, it.TAK, it.BI = int(row["mode"]), int(row["tak"]), int(row["bi"])
    it.LABEL = bytes(int(v) for v in row["label"])
    it.hastext, it.moretocome = bool(flags & MSG_TEXT), bool(flags & MSG_MORE)
    if flags & MSG_PARITY:
        it.error = "ISU: AESID = %X GESID = %X QNO = %02X REFNO = %02X : Parity error" % (it.aesid, it.gesid, it.qno, it.refno)
        return it
    it.PLANEREG = bytes(b & 0x7F for b in u[4:11])
    if it.hastext:
        it.message = "".join("<DEL>" if (b & 0x7F) == 0x7F else chr(b & 0x7F) for b in u[16:n - 4])
    it.valid = True
    return it


class AcarsDefragmenter:
    """ACARSDefragmenter::defragment (JAERO/aerol.cpp:283-329) with findfragment (:221-282).  push(item) takes a valid ACARS item of
    parse_msg and returns the item to hand on -- the item itself when it is whole, the joined one (texts concatenated, the last block's BI)
    when it is the last block of a pending one -- or None while more is to come.  Every push ages the pending fragments; one older than 30
    pushes is dropped."""

    def __init__(self):
        self.frags = []  # [item, count]

    def _find(self, it: AcarsItem) -> int:
        for idx, (p, _) in enumerate(self.frags):
            if (it.PLANEREG == p.PLANEREG and it.LABEL == p.LABEL and it.MODE == p.MODE and it.aesid == p.aesid and it.gesid == p.gesid
                    and p.moretocome):
                if it.TAK != p.TAK:
                    continue
                if ((p.BI + 1 - ord("A")) % 26) + ord("A") == it.BI:
                    return idx
        return -1

    def push(self, it: AcarsItem) -> Optional[AcarsItem]:
        i = 0
        while i < len(self.frags):
            self.frags[i][1] += 1
            if self.frags[i][1] > 30:
                del self.frags[i]
                continue
            i += 1
        idx = self._find(it)
        if idx < 0:
            if not it.moretocome:
                return it
            self.frags.append([AcarsItem(**it.__dict__), 0])
            return None
        old = self.frags[idx]
        old[1] = 0
        old[0].BI = it.BI
        old[0].message += it.message
        old[0].moretocome = it.moretocome
        if it.moretocome:
            return None
        del self.frags[idx]
        return old[0]
