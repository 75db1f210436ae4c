"""The definition of include/jaero_hip.h's "ISU user data and ACARS headers" section, written out literally: ISUData::update
(JAERO/aerol.cpp:117-219) with its quirks, the header part of ParserISU::parse (aerol.cpp:340-470) and the jaero_aerol_msg row.  What the
device code (jaero_amd/csrc/k_aerol_isu.h) is compared with, on the host (tests/test_aerol_isu_emul.py) and on the GPU
(tests/test_gpu_aerol_isu.py); tests/test_isu_oracle.py anchors it on the unmodified reference and on an off-air recording."""
import numpy as np

MSG = np.dtype([("frame", "<i4"), ("k", "<i4"), ("aesid", "<u4"), ("gesid", "u1"), ("qno", "u1"), ("refno", "u1"), ("nooct", "u1"),
                ("nbytes", "<u2"), ("flags", "<u2"), ("mode", "u1"), ("tak", "u1"), ("label", "u1", (2,)), ("bi", "u1"), ("pad", "u1", (7,)),
                ("data", "u1", (512,))])
assert MSG.itemsize == 544
F_AES0, F_ACARS, F_TEXT, F_MORE, F_PARITY = 1, 2, 4, 8, 16


class Item:
    def __init__(self):
        self.AESID = self.GESID = self.QNO = self.REFNO = self.SEQNO = self.NOOCT = self.count = 0
        self.userdata = bytearray()

    def copy(self):
        c = Item()
        c.__dict__.update(self.__dict__)
        c.userdata = bytearray(self.userdata)
        return c


def odd_parity(b: int) -> bool:
    return bin(b).count("1") & 1 == 1


def classify(aesid: int, u: bytes):
    """(flags, mode, tak, label0, label1, bi) of a completed item, as ParserISU::parse sees it."""
    n = len(u)
    if aesid == 0:
        return F_AES0, 0, 0, 0, 0, 0
    if not (n > 16 and u[0] == 0xFF and u[1] == 0xFF and u[15] in (0x83, 0x02)):
        return 0, 0, 0, 0, 0, 0
    flags = F_ACARS
    hastext = u[15] == 0x02
    if hastext:
        flags |= F_TEXT
    if u[n - 4] == 0x97:
        flags |= F_MORE
    bad = any(not odd_parity(u[k]) for k in range(4, 11))
    if hastext:
        bad = bad or any(not odd_parity(u[k]) for k in range(16, n - 4))
    if bad:
        flags |= F_PARITY
    return flags, u[3] & 0x7F, u[11] & 0x7F, u[12] & 0x7F, u[13] & 0x7F, u[14] & 0x7F


class ISUData:
    """One channel's reassembly.  update(d) returns the completed item (a copy) or None; .missing says whether the last unit was a missing SSU."""

    def __init__(self):
        self.items = []
        self.a = Item()
        self.missing = False
        self.stats = [0, 0, 0, 0]  # ISU updates, SSU updates, missing SSUs, completed messages

    def reset(self):
        self.items.clear()  # `a` stays

    def update(self, d: bytes):
        a = self.a
        self.missing = False
        if d[0] == 0x71:
            self.stats[0] += 1
            i = 0
            while i < len(self.items):  # deleteoldisuitems
                self.items[i].count += 1
                if self.items[i].count > 10:
                    del self.items[i]
                    continue
                i += 1
            a.AESID = (d[1] << 16) | (d[2] << 8) | d[3]
            a.GESID = d[4]
            a.QNO, a.REFNO = d[5] >> 4, d[5] & 15
            a.SEQNO = d[6] & 63
            a.NOOCT = d[7] >> 4
            a.count = 0
            a.userdata = bytearray(d[8:10])
            idx = -1
            if a.NOOCT <= 8:
                for i, it in enumerate(self.items):
                    if (a.AESID, a.GESID, a.QNO, a.REFNO) == (it.AESID, it.GESID, it.QNO, it.REFNO):
                        idx = i
                        break
            if idx < 0:
                self.items.append(a.copy())
            else:
                self.items[idx] = a.copy()
            assert len(self.items) <= 11
            return None
        if (d[0] & 0xC0) != 0xC0:
            return None
        self.stats[1] += 1
        a.SEQNO = d[0] & 63
        a.QNO, a.REFNO = d[1] >> 4, d[1] & 15
        idx = -1
        if a.NOOCT <= 8:
            for i, it in enumerate(self.items):
                if a.AESID == it.AESID and a.GESID == it.GESID and a.SEQNO + 1 == it.SEQNO and a.QNO == it.QNO and a.REFNO == it.REFNO:
                    idx = i
                    break
        if idx < 0:
            self.missing = True
            self.stats[2] += 1
            return None
        it = self.items[idx]
        it.SEQNO -= 1
        if it.SEQNO == 0:
            it.userdata += bytes(d[2:min(it.NOOCT, 8) + 2])  # (an item with NOOCT > 8 is reachable, see the header: the unit has eight bytes)
            self.stats[3] += 1
            return it.copy()
        it.userdata += bytes(d[2:10])
        return None


def msg_row(item: Item, frame: int, k: int) -> np.ndarray:
    r = np.zeros((), dtype=MSG)
    u = bytes(item.userdata)
    assert 2 <= len(u) <= 506
    flags, mode, tak, l0, l1, bi = classify(item.AESID, u)
    r["frame"], r["k"], r["aesid"] = frame, k, item.AESID
    r["gesid"], r["qno"], r["refno"], r["nooct"] = item.GESID, item.QNO, item.REFNO, item.NOOCT
    r["nbytes"], r["flags"], r["mode"], r["tak"], r["bi"] = len(u), flags, mode, tak, bi
    r["label"] = (l0, l1)
    r["data"][:len(u)] = np.frombuffer(u, np.uint8)
    return r


class Channel:
    """ISUData behind a channel's signal-unit rows [frame, k, 12 bytes, crc_ok, frameinfo] and its short-frame notices."""

    def __init__(self, msg_capacity=None):
        self.isu = ISUData()
        self.msgs = []       # rows the log holds
        self.missing = []    # (frame, k) of every missing SSU
        self.cap = msg_capacity
        self.overflowed = False

    def short_frame(self):
        self.isu.reset()

    def units(self, rows):
        for r in rows:
            if not r[14]:
                continue
            it = self.isu.update(bytes(int(v) for v in r[2:12]))
            if self.isu.missing:
                self.missing.append((int(r[0]), int(r[1])))
            if it is not None:
                if self.cap is not None and len(self.msgs) >= self.cap:
                    self.overflowed = True
                else:
                    self.msgs.append(msg_row(it, int(r[0]), int(r[1])))

    def take(self):
        out = np.array(self.msgs, dtype=MSG) if self.msgs else np.zeros(0, dtype=MSG)
        self.msgs = []
        return out

    @property
    def stats(self):
        return np.array(self.isu.stats, dtype=np.int64)


CHUNK = 64


def run_stream(O, fb: int, soft: np.ndarray, chan: Channel = None, aerol=None):
    """A soft-bit stream through the C oracle of the bit pipeline (oracle.AeroL) and a Channel behind it.  The pipeline is fed CHUNK soft bits at
    a time; within a chunk the signal units go first, then the short-frame notices: a frame's units come out at the bit that completes its
    last block, the notice at a unique word, and after a unique word the next frame end is more than a thousand bits away -- so when a chunk
    holds both, the units are the older ones (aerol.cpp:1583-1600 runs before :1995 when they fall on the same bit).
    Returns (Channel, signal-unit rows, event rows)."""
    chan = chan or Channel()
    a = aerol or O.AeroL(fb)
    sus, evs = [], []
    for s in range(0, len(soft), CHUNK):
        a.write(soft[s:s + CHUNK])
        r, e = a.take_sus(), a.take_events()
        if len(r):
            chan.units(r)
            sus.append(r)
        if len(e):
            for _ in range(int((e[:, 1] == 1).sum())):
                chan.short_frame()
            evs.append(e)
    cat = lambda xs, w, dt: np.concatenate(xs) if xs else np.zeros((0, w), dt)
    return chan, cat(sus, 16, np.int32), cat(evs, 3, np.int64)
