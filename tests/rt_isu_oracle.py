"""The definition of include/jaero_hip.h's "R / T user data of a burst bank" section, written out literally: RISUData::update
(JAERO/aerol.cpp:6-113) step by step with its quirks, ISUData::update (tests/isu_oracle.py) behind the units of a T packet
(aerol.cpp:1488-1516), the header part of ParserISU::parse and the jaero_aerol_msg row.  What the device code
(jaero_amd/csrc/k_aerolb_isu.h) is compared with, on the host (tests/test_aerolb_isu_emul.py) and on the GPU (tests/test_gpu_aerol_rt.py);
tests/test_rt_isu_oracle.py anchors it on the text the unmodified reference prints."""
import numpy as np

import isu_oracle as IO

MSG = IO.MSG
F_RCHAN, F_RSIGNAL = 32, 64
SEQ = {1: (1, 0), 2: (2, 0), 3: (2, 1), 4: (3, 0), 5: (3, 1), 6: (3, 2)}  # SEQINDICATOR -> (SUTotal, SUindex); anything else (0, 0)


class RItem:
    def __init__(self):
        self.AESID = self.GESID = self.QNO = self.REFNO = self.count = self.filled = 0
        self.NOOCT = 0
        self.userdata = bytearray()

    def copy(self):
        c = RItem()
        c.__dict__.update(self.__dict__)
        c.userdata = bytearray(self.userdata)
        return c


def r_fields(d: bytes):
    """(SUindex + 1, SUTotal, AESID, GESID) of an R user-data packet, as aerol.cpp:1401-1448 prints them."""
    total, index = SEQ.get(d[0] >> 4, (0, 0))
    return index + 1, total, (d[2] << 16) | (d[3] << 8) | d[4], d[5]


class RISUData:
    """One channel's R-channel reassembly.  update(d) returns (completed item (a copy), is a signalling unit) or None."""

    def __init__(self):
        self.items = []
        self.stats = [0, 0, 0, 0]  # user-data packets fed, items newly appended, completed messages, signalling-information units

    def update(self, d: bytes):
        assert len(d) == 17
        self.stats[0] += 1
        i = 0
        while i < len(self.items):  # deleteoldisuitems
            self.items[i].count += 1
            if self.items[i].count > 10:
                del self.items[i]
                continue
            i += 1
        a = RItem()  # anisuitem.clear()
        seqind, sutype = d[0] >> 4, d[0] & 15
        a.QNO, a.REFNO = d[1] >> 4, d[1] & 7
        a.AESID = (d[2] << 16) | (d[3] << 8) | d[4]
        a.GESID = d[5]
        idx = -1
        if 1 <= sutype <= 11:  # findisuitem
            for i, it in enumerate(self.items):
                if (a.GESID, a.AESID, a.QNO, a.REFNO) == (it.GESID, it.AESID, it.QNO, it.REFNO):
                    idx = i
                    break
        if idx < 0:
            self.items.append(a)
            idx = len(self.items) - 1
            self.stats[1] += 1
        assert len(self.items) <= 11
        it = self.items[idx]
        it.count = 0
        total, index = SEQ.get(seqind, (0, 0))
        nbytes = sutype if 1 <= sutype <= 11 else 0
        signal = sutype == 15
        thisnum = 11 * total - 11 + nbytes
        if thisnum > 0:
            if len(it.userdata) == 0:
                it.userdata = bytearray(thisnum)      # resize of an empty array: the new bytes are 0 here (corner 2)
            if thisnum < len(it.userdata):
                del it.userdata[thisnum:]             # a longer one is cut; a shorter one is not grown by this step
        if not signal:
            for i in range(nbytes):
                at = i + 11 * index
                if at >= len(it.userdata):
                    it.userdata += bytes(at + 1 - len(it.userdata))  # QByteRef::operator= -> expand (corner 1), new bytes 0 (corner 2)
                it.userdata[at] = d[6 + i]
            it.filled |= 1 << index
        else:
            it.userdata = bytearray()
        if signal or (it.filled, total) in ((7, 3), (3, 2), (1, 1)):
            out = it.copy()
            del self.items[idx]  # removed: ISUData keeps its item, RISUData does not
            self.stats[2] += 1
            if signal:
                self.stats[3] += 1
            return out, signal
        return None


def msg_row(item, frame: int, k: int, origin: int = 0) -> np.ndarray:
    r = np.zeros((), dtype=MSG)
    u = bytes(item.userdata)
    assert len(u) <= (33 if origin & F_RCHAN else 506)
    flags, mode, tak, l0, l1, bi = IO.classify(item.AESID, u)
    r["frame"], r["k"], r["aesid"] = frame, k, item.AESID
    r["gesid"], r["qno"], r["refno"], r["nooct"] = item.GESID, item.QNO, item.REFNO, item.NOOCT
    r["nbytes"], r["flags"], r["mode"], r["tak"], r["bi"] = len(u), flags | origin, mode, tak, bi
    r["label"] = (l0, l1)
    r["data"][:len(u)] = np.frombuffer(u, np.uint8)
    return r


def number_of_sus(fb: int, info: bytes) -> int:
    """numberofsus of an accepted T packet whose info field (after chop(1)) is `info`."""
    if fb == 10500:
        blockptr = 16 * (len(info) + 1)
        return 1 + int((blockptr - 320) / 192)  # C division: 0 for the two-column block (aerol.h:849)
    t = 2 + (info[6 + 12] & 63)               # the unit after the initial one announces it (aerol.h:709-729)
    if t >= 16:
        t = t // 2 + 1
    assert len(info) == 6 + 12 * (t + 1) + 1    # the block holds one unit more than are looked at
    return t


class Channel:
    """ISUData and RISUData behind a burst channel's accepted packets."""

    def __init__(self, fb: int, msg_capacity=None):
        self.fb = fb
        self.isu = IO.ISUData()
        self.risu = RISUData()
        self.msgs = []      # rows the log holds
        self.missing = []   # (packet, k) of every missing SSU
        self.t_units = []   # every unit fed to ISUData::update, in order
        self.r_lines = []   # r_fields of every R user-data packet, in order
        self.cap = msg_capacity
        self.overflowed = False

    def _emit(self, row):
        if self.cap is not None and len(self.msgs) >= self.cap:
            self.overflowed = True
        else:
            self.msgs.append(row)

    def packet(self, npk: int, ptype: int, info: bytes):
        if ptype == 1:
            d = bytes(info[:17])
            if not d[1] & 0x08:
                return
            self.r_lines.append(r_fields(d))
            res = self.risu.update(d)
            if res is not None:
                self._emit(msg_row(res[0], npk, 0, F_RCHAN | (F_RSIGNAL if res[1] else 0)))
            return
        for k in range(number_of_sus(self.fb, info)):
            d = bytes(info[6 + 12 * k: 6 + 12 * k + 10])
            self.t_units.append(d)
            it = self.isu.update(d)
            if self.isu.missing:
                self.missing.append((npk, k))
            if it is not None:
                self._emit(msg_row(it, npk, k))

    def rows(self, rows):
        """Packet rows [packet, chunk, 12 bytes, total bytes, type] as jaero_aerol_read_packets gives them, complete packets only."""
        for pk in sorted(set(rows[:, 0].tolist())) if len(rows) else []:
            r = rows[rows[:, 0] == pk]
            r = r[np.argsort(r[:, 1])]
            self.packet(int(pk), int(r[0, 15]), bytes(int(v) for v in r[:, 2:14].reshape(-1))[: int(r[0, 14])])

    def take(self):
        out = np.array(self.msgs, dtype=MSG) if self.msgs else np.zeros(0, dtype=MSG)
        self.msgs = []
        return out

    @property
    def stats(self):
        return np.array(self.isu.stats + self.risu.stats, dtype=np.int64)


def run_stream(O, fb: int, soft: np.ndarray, chan: Channel = None):
    """A soft-bit stream through the C oracle of the burst pipeline (oracle.run_aerol_burst) and a Channel behind its packets.
    Returns (Channel, packet rows, event rows)."""
    chan = chan or Channel(fb)
    o = O.run_aerol_burst(fb, soft)
    chan.rows(o["packets"])
    return chan, o["packets"], o["events"]
