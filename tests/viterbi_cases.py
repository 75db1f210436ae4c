"""The launch modes of the Viterbi decoders (k_viterbi, k_viterbi_lanes, k_viterbi_lanes_x2): cases, and what each must leave in memory.

Shared by tests/test_viterbi_cases.py (CPU: the reference below against oracle.Codec and the golden, the coverage the case list claims) and
tests/test_gpu_viterbi_modes.py (GPU: every case through jaero_debug_viterbi, whole buffers compared).

THE CONTRACT (k_viterbi.h / k_viterbi_lanes.h; include/jaero_hip.h at jaero_debug_viterbi).  Row b of a launch decodes the stream
    overlap[b][:overlap[b][62]]  ++  soft[b][:len]  ++  pad x 128            len = lens[b] if lens else nsoft
of sets = (stream length) // 2 trellis steps (the last byte of an odd stream -- an odd overlap length -- is not used).  libcorrect emits sets - 6 decoded bits for it (the first six steps record no history).
Decoded bit k goes to position p = k - out_start of the row's output when 0 <= p < min(out_want, len // 2); everything else in the output
buffer -- positions outside that window, rows with valid == 0, rows at or beyond nblocks -- is not written.
    one byte per bit : out[b][p] = bit
    packed           : bit p & 31 of the little-endian 32-bit word p >> 5 of the row.  A word that receives at least one bit is written WHOLE,
                       its other bits 0 (pk_bits starts every word at 0, pk_store writes 32 bits); a word that receives none is not written.
With update_overlap the overlap row becomes the last 62 soft bytes of the row (zero-filled behind a row shorter than 62), byte 62 = 62,
byte 63 untouched (jconvolutionalcodec.cpp:197-198); rows with valid == 0 keep theirs.

expected() states this with oracle.Codec().decode_soft as the only decoder.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

VT_ORDER, VT_MINTB, VT_GROUP, VT_CAP, VT_RENORM = 7, 35, 105, 140, 128  # k_viterbi.h
POISON = 0xA5           # what the tests fill out with (a decoded bit is 0 or 1; a packed word 0xA5A5A5A5 is one in 2^32)
GAP = 0x3C              # bytes between nsoft and pitch, rows of a tiled buffer beyond nblocks
LAYOUTS = {"wave": 1, "lanes": 2, "x2": 3}  # jaero_viterbi_probe.layout


# ------------------------------------------------------------------------------------------------------------------ schedule model
@functools.lru_cache(maxsize=None)
def schedule(sets: int):
    """libcorrect's history buffer over a stream of `sets` steps, as both kernels restate it: six warm-up steps record nothing; every
    recorded step r = 1, 2, .. counts towards a renormalisation (every VT_RENORM) and towards a traceback (when VT_CAP slices are
    buffered: the oldest VT_GROUP bits come out, VT_MINTB slices stay); the flush after the last step emits the rest.  Steps
    sets - 6 .. sets - 1 are tail steps (only states that are multiples of skip = 2, 4, .. 64 are updated).
    Returns (tracebacks, renorms): tracebacks = tuples (rec, lo, hi, length, min_tb, skip) -- decoded bits [lo, hi) from `length` buffered
    slices at recorded step rec, skip = 1 outside the tail, min_tb = 0 for the flush; renorms = tuples (rec, skip, with_traceback)."""
    tbs, rens = [], []
    length = renorm = outpos = rec = 0
    for i in range(VT_ORDER - 1, sets):
        skip = 1 << (VT_ORDER - (sets - i)) if i >= sets - VT_ORDER + 1 else 1
        rec += 1
        renorm += 1
        length += 1
        ren, full = renorm == VT_RENORM, length == VT_CAP
        if ren:
            renorm = 0
            rens.append((rec, skip, full))
        if full:
            f = length - VT_MINTB
            tbs.append((rec, outpos, outpos + f, length, VT_MINTB, skip))
            outpos += f
            length -= f
    tbs.append((rec, outpos, outpos + length, length, 0, 64 if sets >= VT_ORDER else 1))
    return tuple(tbs), tuple(rens)


def nbits(sets: int) -> int:
    return max(sets - (VT_ORDER - 1), 0)


def traceback_windows(sets: int, out_start: int, want: int):
    """Per traceback that hands at least one bit into the window: (plo, phi, crossing) -- output positions [plo, phi) and whether one of
    the traceback's aligned four-iteration groups (k_viterbi_lanes: iterations j = 4g .. 4g + 3 from the newest slice, positions
    K0 - j with K0 = hi - 1 + min_tb - out_start) lies wholly inside the traceback and the window and yet in two 32-bit words."""
    res = []
    for rec, lo, hi, length, min_tb, skip in schedule(sets)[0]:
        plo, phi = max(lo - out_start, 0), min(hi - out_start, want)
        if plo >= phi:
            continue
        k0 = lo + length - 1 - out_start
        crossing = False
        for j in range(0, length, 4):
            klow = k0 - (j + 3)
            if j >= min_tb and j + 3 < length and klow >= 0 and klow + 3 < want and (klow >> 5) != ((klow + 3) >> 5):
                crossing = True
        res.append((plo, phi, crossing))
    return res


# ------------------------------------------------------------------------------------------------------------------ tiled layout
def tile_pack(rows: np.ndarray) -> np.ndarray:
    """[nblocks][nsoft] -> [wavefront][16-byte group][lane][16] (nsoft a multiple of 16; the rows of the last wavefront beyond nblocks are GAP)."""
    nb, ns = rows.shape
    assert ns % 16 == 0
    waves = (nb + 63) // 64
    full = np.full((waves * 64, ns), GAP, np.uint8)
    full[:nb] = rows
    return np.ascontiguousarray(full.reshape(waves, 64, ns // 16, 16).transpose(0, 2, 1, 3))


def tile_unpack(tiled: np.ndarray, nblocks: int) -> np.ndarray:
    waves, ng, lanes, sixteen = tiled.shape
    assert lanes == 64 and sixteen == 16
    return np.ascontiguousarray(tiled.transpose(0, 2, 1, 3).reshape(waves * 64, ng * 16)[:nblocks])


# ------------------------------------------------------------------------------------------------------------------ inputs
def encode(bits: np.ndarray) -> np.ndarray:
    """K = 7, rate 1/2, polynomials {109, 79}, newest bit in the register's bit 0: coded bits 2t, 2t + 1 (libcorrect's encoder; checked
    against oracle.encode_bits in tests/test_viterbi_cases.py)."""
    b = np.concatenate([np.zeros(6, np.uint8), bits.astype(np.uint8)])
    n = len(bits)
    d = lambda j: b[6 - j: 6 - j + n]
    c0 = d(0) ^ d(2) ^ d(3) ^ d(5) ^ d(6)   # 109 = 1101101b
    c1 = d(0) ^ d(1) ^ d(2) ^ d(3) ^ d(6)   # 79  = 1001111b
    return np.stack([c0, c1], 1).reshape(-1)


NROWS = 130


@functools.lru_cache(maxsize=None)
def rows(nsoft: int) -> np.ndarray:
    """NROWS rows of nsoft soft bytes, the same for every case of that length (so that cases share their oracle decodes): by row index
    mod 6 -- noisy codeword, uniform garbage (ties, uint16 wrap), coarse values (x // 64 * 64 + 31: exact ties), a noisier codeword, a
    codeword that ends in erasures, and a constant row (128, 0, 255 in turn)."""
    rng = np.random.default_rng(1000 + nsoft)
    out = np.zeros((NROWS, nsoft), np.uint8)
    for b in range(NROWS):
        kind = b % 6
        if kind in (0, 3, 4):
            coded = encode(rng.integers(0, 2, (nsoft + 1) // 2))[:nsoft]
            x = (coded.astype(float) * 2 - 1) + rng.normal(0, (0.3, 0, 0, 0.7, 0.5)[kind], nsoft)
            out[b] = np.clip(np.round(x * 64 + 128), 0, 255)
            if kind == 4:
                out[b, nsoft - nsoft // 5:] = 128
        elif kind == 1:
            out[b] = rng.integers(0, 256, nsoft)
        elif kind == 2:
            out[b] = rng.integers(0, 256, nsoft) // 64 * 64 + 31
        else:
            out[b] = (128, 0, 255)[(b // 6) % 3]
    out.setflags(write=False)
    return out


def overlaps(nblocks: int, lengths, seed: int) -> np.ndarray:
    """[nblocks][64]: 62 random bytes, byte 62 = lengths[b % len(lengths)], byte 63 = POISON (never read, never written)."""
    rng = np.random.default_rng(seed)
    ov = rng.integers(0, 256, (nblocks, 64)).astype(np.uint8)
    ov[:, 62] = [lengths[b % len(lengths)] for b in range(nblocks)]
    ov[:, 63] = POISON
    return ov


# ------------------------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    name: str
    group: str
    soft: np.ndarray                      # [nblocks][nsoft], the rows as the decoder is to see them (layout and pitch are applied by soft_buffer)
    pad: int = 0
    pitch: int = 0
    tiled: int = 0
    misalign: int = 0
    overlap: Optional[np.ndarray] = None  # [nblocks][64]
    update_overlap: int = 0
    out_start: int = 0
    out_want: int = 0                     # 0: nsoft // 2
    packed: int = 0
    valid: Optional[np.ndarray] = None
    lens: Optional[np.ndarray] = None
    layouts: tuple = field(default=())    # filled in: the layouts in which the mode exists

    def __post_init__(self):
        self.nblocks, self.nsoft = self.soft.shape
        if not self.out_want:
            self.out_want = self.nsoft // 2
        # rows of out: whole wavefronts, so that the rows a ragged last wavefront must not touch are there; stride: larger than the window
        # (and odd for bytes, so that rows start at every alignment)
        self.out_rows = (self.nblocks + 63) // 64 * 64
        self.out_stride = ((self.out_want + 31) // 32 * 4 + 8) if self.packed else self.out_want + 5 + (self.out_want & 1)
        minlen = int(self.lens.min()) if self.lens is not None else self.nsoft
        lanes_ok = (minlen + self.pad) // 2 >= 4 * VT_ORDER
        if self.tiled or self.packed:
            assert lanes_ok
            self.layouts = ("lanes", "x2")
        elif not self.layouts:
            self.layouts = ("wave", "lanes", "x2") if lanes_ok else ("wave",)

    def length(self, b: int) -> int:
        return int(self.lens[b]) if self.lens is not None else self.nsoft

    def ovl(self, b: int) -> int:
        return int(self.overlap[b, 62]) if self.overlap is not None else 0

    def stream(self, b: int) -> np.ndarray:
        head = self.overlap[b, : self.ovl(b)] if self.overlap is not None else np.zeros(0, np.uint8)
        return np.concatenate([head, self.soft[b, : self.length(b)], np.full(self.pad, 128, np.uint8)])

    def is_valid(self, b: int) -> bool:
        return self.valid is None or bool(self.valid[b])

    def window(self, b: int) -> int:
        return min(self.out_want, self.length(b) // 2)

    def soft_buffer(self) -> np.ndarray:
        """The bytes the launch reads: tiled, or row-major with `pitch` (the bytes between nsoft and pitch are GAP)."""
        if self.tiled:
            return tile_pack(self.soft)
        if self.pitch:
            buf = np.full((self.nblocks, self.pitch), GAP, np.uint8)
            buf[:, : self.nsoft] = self.soft
            return buf
        return np.ascontiguousarray(self.soft)

    def poisoned_out(self) -> np.ndarray:
        return np.full((self.out_rows, self.out_stride), POISON, np.uint8)

    def bits_compared(self) -> int:
        return sum(max(min(nbits(len(self.stream(b)) // 2) - self.out_start, self.window(b)), 0) for b in range(self.nblocks) if self.is_valid(b))


_CODEC = None
_DECODES = {}  # stream bytes -> decoded bits: cases of one length share rows, and the window cases share everything but the window


def decode_stream(O, stream: np.ndarray) -> np.ndarray:
    global _CODEC
    stream = stream[: len(stream) // 2 * 2]  # sets = total // 2: an odd last byte is never read (libcorrect itself refuses an odd length)
    key = stream.tobytes()
    if key not in _DECODES:
        if _CODEC is None:
            _CODEC = O.Codec(0)  # decode_soft keeps no state between calls
        _DECODES[key] = _CODEC.decode_soft(stream)[: nbits(len(stream) // 2)].copy()
    return _DECODES[key]


def oracle_decodes() -> int:
    return len(_DECODES)


def expected(O, c: Case, out_start_error: int = 0):
    """(out, overlap): every byte of the output buffer after the launch, from a POISON-filled one, and the overlap buffer (None when the
    case has none).  out_start_error is for the test that perturbs this reference."""
    out = c.poisoned_out()
    words = out.view("<u4") if c.packed else None
    for b in range(c.nblocks):
        if not c.is_valid(b):
            continue
        bits = decode_stream(O, c.stream(b))
        lo = c.out_start + out_start_error
        win = bits[lo: lo + c.window(b)]
        if c.packed:
            nw = (len(win) + 31) // 32
            padded = np.zeros(nw * 32, np.uint8)
            padded[: len(win)] = win
            words[b, :nw] = (padded.reshape(nw, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)
        else:
            out[b, : len(win)] = win
    ov = None
    if c.overlap is not None:
        ov = c.overlap.copy()
        if c.update_overlap:
            for b in range(c.nblocks):
                if c.is_valid(b):
                    tail = c.soft[b, max(c.nsoft - 62, 0): c.nsoft]   # the kernel takes the row's nsoft bytes, whatever lens says
                    ov[b, :62] = 0
                    ov[b, : len(tail)] = tail
                    ov[b, 62] = 62
    return out, ov


def _mk():
    cases = []
    add = cases.append
    R = rows
    # -- lengths: chunk edges at 128 bytes; sets just below / at / above the first traceback (140 recorded steps = 146 sets); the tail steps
    #    inside, at and behind a traceback or a renormalisation; block counts 1, 63, 64, 65, 130 (ragged last wavefront, several wavefronts)
    counts = {56: 3, 64: 65, 126: 63, 128: 64, 130: 1, 254: 5, 258: 65, 292: 3, 300: 130, 662: 5, 1210: 65}
    for ns, nb in counts.items():
        for pad in (0, 24):
            add(Case(f"len{ns}_pad{pad}_x{nb}", "lengths", R(ns)[:nb], pad=pad))
    # -- long: recorded step 8960 = 140 + 105 * 84 = 128 * 70 renormalises and traces back at once
    long_ns = 17952
    add(Case("long_wave_x3", "long", R(long_ns)[:3], pad=24, layouts=("wave",)))
    add(Case("long_lanes_x70", "long", R(long_ns)[:70], pad=24, layouts=("lanes", "x2")))
    # -- overlap: lengths 62, 0, 2, 31 (odd: every step of the block takes the byte-wise path) mixed in one wavefront = four passes; lane 0
    #    masked out in the second variant so that the first pending lane is not lane 0.  The continuation (call 2) is built by the tests.
    ovmix = (62, 0, 2, 31)
    for ns, nb in ((292, 65), (1210, 65)):
        add(Case(f"ovmix{ns}", "overlap", R(ns)[:nb], pad=24, overlap=overlaps(nb, ovmix, ns), update_overlap=1, out_start=25))
    v = np.ones(65, np.int32)
    v[0] = 0
    add(Case("ovmix292_lane0_off", "overlap", R(292)[:65], pad=24, overlap=overlaps(65, (31, 62, 0, 2), 7), update_overlap=1, out_start=25, valid=v))
    add(Case("ovmix662_nopad", "overlap", R(662)[:9], pad=0, overlap=overlaps(9, ovmix, 8), out_start=1))
    # -- window: out_start x out_want, bytes and packed, on one set of rows (300 soft bytes + 62 of overlap + 24 of padding: a traceback of 105
    #    bits and a flush of 82); and on 662 bytes (four tracebacks) for the windows that reach across them
    for ns, starts, wants in ((300, (0, 1, 25, 31, 32, 33), (1, 3, 4, 31, 32, 33, 150, 170)), (662, (1, 25, 33), (33, 331, 351))):
        for s in starts:
            for w in wants:
                for packed in (0, 1):
                    add(Case(f"win{ns}_s{s}_w{w}_{'pk' if packed else 'by'}", "window", R(ns)[:65], pad=24, overlap=overlaps(65, (62,), 300),
                             out_start=s, out_want=w, packed=packed))
    # -- pitch and alignment: rows that are no multiple of 16 in a pitch rounded up to 16 (the fast path reads the last group whole: GAP bytes
    #    come along and must not count), pitch == nsoft no multiple of 16 and a base that is not 16-byte aligned (byte-wise path for the whole block)
    for ns, pitch, mis in ((100, 112, 0), (116, 128, 0), (100, 0, 0), (130, 0, 0), (100, 112, 4), (128, 0, 4), (116, 144, 0), (116, 120, 0)):
        add(Case(f"pitch{ns}_in{pitch or ns}_mis{mis}", "pitch", R(ns)[:65], pad=24, pitch=pitch, misalign=mis, overlap=overlaps(65, (62, 0), 500 + ns),
                 update_overlap=1, out_start=25))
    # -- tiled input, with the overlap update reading the same layout
    for ns in (64, 128, 304, 1216):
        add(Case(f"tiled{ns}", "tiled", R(ns)[:65], pad=24, tiled=1, overlap=overlaps(65, (62, 0, 62), 600 + ns), update_overlap=1, out_start=25,
                 packed=int(ns == 304)))
    # -- lens: the R/T trial lengths per lane with holes; with padding and overlaps (pass = one (overlap, length) pair); 64 distinct lengths
    rng = np.random.default_rng(77)
    l3 = rng.choice([128, 320, 512], 130).astype(np.int32)
    holes = (rng.random(130) > 0.25).astype(np.int32)
    add(Case("lens_rt", "lens", R(512)[:130], lens=l3, valid=holes))
    add(Case("lens_rt_packed", "lens", R(512)[:130], lens=l3, valid=holes, packed=1))
    add(Case("lens_ov_pad", "lens", R(512)[:130], lens=l3, valid=holes, pad=24, overlap=overlaps(130, (62, 0, 2), 78), out_start=25, out_want=200))
    add(Case("lens_64_distinct", "lens", R(512)[:64], lens=(128 + 6 * rng.permutation(64)).astype(np.int32), out_want=300))
    # -- valid: none (early return), one lane, alternating lanes; output and overlap of a masked row untouched
    one = np.zeros(65, np.int32)
    one[37] = 1
    for nm, val in (("none", np.zeros(65, np.int32)), ("one", one), ("alternating", (np.arange(65) & 1).astype(np.int32))):
        add(Case(f"valid_{nm}", "valid", R(292)[:65], pad=24, overlap=overlaps(65, (62, 0), 900), update_overlap=1, out_start=25, valid=val))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


CASES = _mk()
GROUPS = sorted({c.group for c in CASES})


def by_group(group: str):
    return [c for c in CASES if c.group == group]


def case(name: str) -> Case:
    return next(c for c in CASES if c.name == name)


def continuation(c: Case, overlap_after: np.ndarray) -> Case:
    """The next call of the same streams: new rows (the second half of rows(nsoft)), the overlap the first call left."""
    return Case(c.name + "_call2", c.group, rows(c.nsoft)[NROWS - c.nblocks:], pad=c.pad, overlap=overlap_after.copy(), update_overlap=1,
                out_start=c.out_start, valid=c.valid)


# ------------------------------------------------------------------------------------------------------------------ coverage claims
def coverage():
    """What the case list reaches, from the schedule model alone (asserted by tests/test_viterbi_cases.py)."""
    cov = {"ren_and_tb": [], "tb_in_tail": set(), "ren_in_tail": set(), "straddled_word": [], "tb_within_word": [], "group_across_words": [],
           "sets_around_first_tb": set(), "passes": {}}
    for c in CASES:
        pairs = set()
        for b in range(c.nblocks):
            if not c.is_valid(b):
                continue
            pairs.add((c.ovl(b), c.length(b)))
        cov["passes"][c.name] = len({(c.ovl(b), c.length(b)) for b in range(min(c.nblocks, 64)) if c.is_valid(b)})  # of the first wavefront
        for ovl, ln in pairs:
            sets = (ovl + ln + c.pad) // 2
            tbs, rens = schedule(sets)
            cov["sets_around_first_tb"].add(sets - (VT_CAP + VT_ORDER - 1))
            if any(w for _, _, w in rens):
                cov["ren_and_tb"].append(c.name)
            cov["tb_in_tail"] |= {skip for _, _, _, _, min_tb, skip in tbs if min_tb and skip > 1}
            cov["ren_in_tail"] |= {skip for _, skip, _ in rens if skip > 1}
            if c.packed:
                wins = traceback_windows(sets, c.out_start, min(c.out_want, ln // 2))
                for (alo, ahi, _), (blo, bhi, _) in zip(wins, wins[1:]):
                    if ahi == blo and ahi % 32:
                        cov["straddled_word"].append(c.name)
                for plo, phi, crossing in wins:
                    if (plo >> 5) == ((phi - 1) >> 5):
                        cov["tb_within_word"].append(c.name)
                    if crossing:
                        cov["group_across_words"].append(c.name)
    return cov
