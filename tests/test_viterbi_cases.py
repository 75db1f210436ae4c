"""CPU: tests/viterbi_cases.py on its own -- the reference expected() against oracle.Codec and the golden of the real JConvolutionalCodec,
the tiled layout's packing, the schedule model, and the coverage the case list claims (tests/test_gpu_viterbi_modes.py runs the cases)."""
import numpy as np
import pytest

import viterbi_cases as V
from conftest import load_golden


def _one(soft, **kw):
    return V.Case("plain", "plain", np.ascontiguousarray(soft)[None, :], **kw)


def _continuous(O, blocks, pad, error=0):
    """Decode_Continuous restated with expected(): every call a one-row case with out_start = pad + 1, the overlap carried along."""
    ov = np.zeros((1, 64), np.uint8)
    res = []
    for blk in blocks:
        c = _one(blk, pad=pad, overlap=ov, update_overlap=1, out_start=pad + 1)
        out, ov = V.expected(O, c, out_start_error=error)
        row = out[0, : c.out_want]
        n = int((row != V.POISON).sum())
        assert (row[:n] != V.POISON).all() and (out[1:] == V.POISON).all() and (out[0, c.out_want:] == V.POISON).all()
        res.append(row[:n].copy())
    return res


def test_expected_reproduces_decode_soft(oracle_mod):
    O = oracle_mod
    for name in ("len64_pad0_x65", "len292_pad0_x3", "len1210_pad0_x65"):
        c = V.case(name)
        ns = c.nsoft
        out, ov = V.expected(O, c)
        assert ov is None and out.shape == (c.out_rows, c.out_stride) and c.out_stride > ns // 2
        for b in range(c.nblocks):
            ref = O.Codec().decode_soft(c.soft[b])
            assert len(ref) == ns // 2 and np.array_equal(out[b, : ns // 2 - 6], ref[: ns // 2 - 6])
            assert (out[b, ns // 2 - 6:] == V.POISON).all()  # libcorrect emits sets - 6 bits; the rest of the row is not the decoder's
        assert (out[c.nblocks:] == V.POISON).all()


def test_expected_reproduces_decode_continuous_and_notices_an_off_by_one(oracle_mod):
    O = oracle_mod
    for ns in (292, 662):
        blocks = [V.rows(ns)[b] for b in (1, 7, 2, 9)]  # garbage, garbage, coarse, a codeword
        codec = O.Codec(24)
        refs = [codec.decode_continuous(b) for b in blocks]
        mine = _continuous(O, blocks, 24)
        for k, (r, m) in enumerate(zip(refs, mine)):
            # a stream's first block: the reference returns sets - 25 bits, of which the decoder wrote sets - 6 - 25 (expected() has only those)
            assert len(r) == (ns // 2 if k else (ns + 24) // 2 - 25) and len(m) == len(r) - (0 if k else 6)
            assert np.array_equal(r[: len(m)], m), (ns, k)
        wrong = _continuous(O, blocks, 24, error=1)
        assert not any(np.array_equal(r[: len(m) - 1], m[: len(m) - 1]) for r, m in zip(refs, wrong))


def test_expected_reproduces_the_reference_golden(oracle_mod):
    """viterbi_cont: the real JConvolutionalCodec's Decode_Continuous over consecutive blocks, and its Decode_soft."""
    O = oracle_mod
    g = load_golden("viterbi_cont")
    soft, blen, out = g["soft"], int(g["blocklen"]), g["out_cont"]
    blocks = [soft[off: off + blen] for off in range(0, len(soft) - blen + 1, blen)]
    p = 0
    for k, mine in enumerate(_continuous(O, blocks, int(g["padding"]))):
        n = int(np.frombuffer(out[p: p + 4].tobytes(), "<u4")[0])
        ref = out[p + 4: p + 4 + n]
        p += 4 + n
        assert len(mine) == (n - 6 if k == 0 else n)  # the first block's last six bits come from bytes libcorrect never wrote
        assert np.array_equal(mine, ref[: len(mine)])
    blen2, out2 = int(g["blocklen_soft"]), g["out_soft"]
    p = 0
    for off in range(0, 3 * blen2, blen2):
        n = int(np.frombuffer(out2[p: p + 4].tobytes(), "<u4")[0])
        ref = out2[p + 4: p + 4 + n]
        p += 4 + n
        mine, _ = V.expected(O, _one(soft[off: off + blen2]))
        assert n == blen2 // 2 and np.array_equal(mine[0, : n - 6], ref[: n - 6]) and (mine[0, n - 6:] == V.POISON).all()


def test_packed_expected_is_the_byte_expected_packed(oracle_mod):
    """The packed reference against the byte reference of the same case: bit p & 31 of word p >> 5, a touched word's other bits 0, an
    untouched word poison."""
    O = oracle_mod
    for name in ("win300_s31_w33", "win300_s0_w1", "win662_s25_w351", "win300_s33_w170"):
        cb, cp = V.case(name + "_by"), V.case(name + "_pk")
        ob, _ = V.expected(O, cb)
        op, _ = V.expected(O, cp)
        words = op.view("<u4")
        for b in range(cb.nblocks):
            nbit = int((ob[b] != V.POISON).sum())
            assert nbit > 0 and (ob[b, :nbit] <= 1).all()
            for w in range(words.shape[1]):
                bits = ob[b, 32 * w: min(32 * w + 32, nbit)]
                if len(bits):
                    assert int(words[b, w]) == sum(int(v) << i for i, v in enumerate(bits))
                else:
                    assert int(words[b, w]) == 0xA5A5A5A5
        assert (op[cb.nblocks:] == V.POISON).all()


def test_tiled_layout_round_trip_and_addresses():
    rng = np.random.default_rng(3)
    for nb, ns in ((1, 16), (64, 64), (65, 304), (130, 128)):
        r = rng.integers(0, 256, (nb, ns)).astype(np.uint8)
        t = V.tile_pack(r)
        assert t.shape == ((nb + 63) // 64, ns // 16, 64, 16) and np.array_equal(V.tile_unpack(t, nb), r)
        flat = t.reshape(-1)
        for b, q in ((0, 0), (nb - 1, ns - 1), (nb // 2, 17 % ns), (nb - 1, 15)):
            # the address k_viterbi_overlap_update and k_viterbi_lanes form: [wavefront][16-byte group][lane][16]
            assert flat[(b >> 6) * 64 * ns + ((q >> 4) * 64 + (b & 63)) * 16 + (q & 15)] == r[b, q]
        assert (V.tile_unpack(t, t.shape[0] * 64)[nb:] == V.GAP).all()


def test_encoder_is_the_oracles(oracle_mod):
    msg = np.random.default_rng(0).integers(0, 256, 40, dtype=np.uint8)
    assert np.array_equal(oracle_mod.encode_bits(msg)[:640], V.encode(np.unpackbits(msg)))


def test_schedule_model():
    for sets in (28, 145, 146, 147, 151, 152, 374, 8990):
        tbs, rens = V.schedule(sets)
        assert tbs[0][1] == 0 and tbs[-1][2] == sets - 6 and all(a[2] == b[1] for a, b in zip(tbs, tbs[1:]))
        assert [t[0] for t in tbs[:-1]] == list(range(140, sets - 5, 105)) and all(t[2] - t[1] == 105 for t in tbs[:-1])
        assert [r[0] for r in rens] == list(range(128, sets - 5, 128))
        assert [r[0] for r in rens if r[2]] == [r for r in range(8960, sets - 5, 13440)]  # lcm(105, 128) = 13440; 8960 = 140 + 105 * 84
    assert V.schedule(146)[0][0][5] == 64 and V.schedule(150)[0][0][5] == 4 and V.schedule(152)[0][0][5] == 1


def test_case_list_reaches_what_it_claims():
    cov = V.coverage()
    assert {"long_wave_x3", "long_lanes_x70"} <= set(cov["ren_and_tb"])          # renormalise and trace back on one step, both layouts
    assert V.case("long_lanes_x70").nblocks == 70 and V.case("long_wave_x3").nblocks == 3
    assert {4, 64} <= cov["tb_in_tail"] and cov["ren_in_tail"]                    # a traceback / a renormalisation ON a tail step (search with skip)
    assert {-1, 0, 2} <= cov["sets_around_first_tb"]                              # sets just below, at and above the first traceback
    for key in ("straddled_word", "tb_within_word", "group_across_words"):         # the packed writer's three branches
        assert len(set(cov[key])) >= 3, key
    assert cov["passes"]["ovmix292"] == 4 and cov["passes"]["lens_64_distinct"] == 64 and cov["passes"]["lens_ov_pad"] >= 6
    c = V.case("ovmix292_lane0_off")
    assert not c.valid[0] and c.valid[1:].all() and {int(v) for v in c.overlap[:, 62]} == {0, 2, 31, 62}
    assert {c.nblocks for c in V.by_group("lengths")} == {1, 3, 5, 63, 64, 65, 130}
    assert {c.nsoft for c in V.by_group("lengths")} == {56, 64, 126, 128, 130, 254, 258, 292, 300, 662, 1210} and {c.pad for c in V.by_group("lengths")} == {0, 24}
    assert {c.nsoft for c in V.by_group("tiled")} == {64, 128, 304, 1216} and all(c.update_overlap for c in V.by_group("tiled"))
    wins = {(c.nsoft, c.out_start, c.out_want, c.packed) for c in V.by_group("window")}
    assert {(300, s, w, p) for s in (0, 1, 25, 31, 32, 33) for w in (1, 3, 4, 31, 32, 33, 150, 170) for p in (0, 1)} <= wins
    for c in V.CASES:  # every case leaves poison between and behind its rows
        assert c.out_stride > (c.out_want + 7) // 8 if c.packed else c.out_stride > c.out_want
        assert ("wave" in c.layouts) == (not c.tiled and not c.packed and c.name != "long_lanes_x70")
        assert set(c.layouts) - {"wave"} in ({"lanes", "x2"}, set())
    # rows whose fast path cannot run: an odd overlap, a misaligned base, a pitch that is no multiple of 16
    assert any(c.misalign for c in V.by_group("pitch")) and any((c.pitch or c.nsoft) % 16 for c in V.by_group("pitch"))
    assert any(c.pitch and c.pitch % 16 == 0 and c.nsoft % 16 for c in V.by_group("pitch"))


def test_whole_case_list_stays_cheap(oracle_mod):
    """Every case's expected buffers, the continuations included: a few thousand oracle decodes at most (cases of one length share rows,
    the window cases share all but the window), so that each GPU test stays at seconds."""
    O = oracle_mod
    for c in V.CASES:
        out, ov = V.expected(O, c)
        assert out.shape == (c.out_rows, c.out_stride) and (out[c.nblocks:] == V.POISON).all()
        if c.group == "overlap" and c.update_overlap:
            V.expected(O, V.continuation(c, ov))
    assert 500 < V.oracle_decodes() < 3000, V.oracle_decodes()
