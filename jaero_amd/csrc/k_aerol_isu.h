// k_aerol_isu.h -- what the reference does with a CRC-clean signal unit of a continuous P channel that carries user data: ISUData::update
// (JAERO/aerol.cpp:117-219, aerol.h:113-228: an ISU 0x71 and the SSUs behind it are put back together) and the header part of
// ParserISU::parse (aerol.cpp:340-470: is it an ACARS block, its mode / TAK / label / block id, text present, more to come, parity).  The
// definition, quirks included, is in include/jaero_hip.h; tests/isu_oracle.py restates it.  One lane per channel, all state in HBM:
//   chan   [nchp][ISU_CHAN_WORDS]  the scratch item `a`, the list's length, its order (slot numbers, oldest first) and the slots in use
//   items  [nchp][11][ISU_ITEM_BYTES]  per slot a 16-byte header and the user data collected so far (506 bytes at most, see isu_item)
//   log    [nchp][msg_cap] rows of jaero_aerol_msg, msg_cnt [nchp], stats [nchp][4]
// k_aerol_isu runs behind k_aerol_post / k_aerol_post_packed of a round, for the channels whose frame ended in that round (the test
// aerol_frame_end is called under) or whose short-frame mark is set.  The mark is written by aerol_event (kind 1, k_aerol.h) in k_aerol_bits; a
// lane's walk ends at the bit that completes a block, and the unique-word half of that bit runs in the next round, so a mark set in a round is
// older than the frame that ends in it: mark first, then the frame's units, is stream order (the jumping 10.5 kbps walk raises events only on
// its bit-by-bit stretches, through the same aerol_bit_b).  Integer only; plain stores.
#pragma once
#include "k_aerol.h"

#define ISU_MAX_ITEMS 11   // counts are distinct and an item goes once its count exceeds 10
#define ISU_MAX_BYTES 506  // 2 + 62 * 8 + 8
#define ISU_ITEM_BYTES 528 // 16 header + 512 data (the data 16-byte aligned: emitted 16 bytes per load)
#define ISU_CHAN_WORDS 8
#define ISU_ROW_BYTES 544
#define ISU_OVERFLOW_BIT 8 // of AI_OVERFLOW: 1 signal units, 2 events, (4 the C channel's voice,) 8 messages
enum { ISU_F_AES0 = 1, ISU_F_ACARS = 2, ISU_F_TEXT = 4, ISU_F_MORE = 8, ISU_F_PARITY = 16 };

struct isu_item // a slot's header
{
    uint32_t aesid;
    uint8_t gesid, qno, refno, seqno;
    uint8_t nooct, count;
    uint16_t len; // user-data bytes so far
    uint32_t pad;
};
struct isu_chan // a channel's header: the scratch item and the list
{
    uint32_t a_aesid;
    uint8_t a_gesid, a_qno, a_refno, a_seqno;
    uint8_t a_nooct, n, pad0, pad1;
    uint32_t used; // bit s: slot s holds an item of the list
    unsigned long long order; // the list, oldest first: slot number of entry i in bits 4 i .. 4 i + 3 (a byte array indexed by i would live in scratch)
    unsigned long long pad2;
};
__device__ __forceinline__ int isu_slot(const isu_chan &s, int i)
{
    const int sl = (int)((s.order >> (4 * i)) & 15ull);
    return sl < ISU_MAX_ITEMS ? sl : 0; // (never above: keeps the address inside the channel's memory whatever the state holds)
}
__device__ __forceinline__ void isu_set_slot(isu_chan &s, int i, int slot)
{
    s.order = (s.order & ~(15ull << (4 * i))) | ((unsigned long long)slot << (4 * i));
}
struct IPtrs
{
    uint32_t *chan;     // [nchp][ISU_CHAN_WORDS]
    uint8_t *items;     // [nchp][ISU_MAX_ITEMS][ISU_ITEM_BYTES]
    uint8_t *log;       // [nchp][msg_cap][ISU_ROW_BYTES]
    int *msg_cnt;       // [nchp]
    long long *stats;   // [nchp][4]: ISU updates, SSU updates, missing SSUs, completed messages
    int msg_cap;
};
static_assert(sizeof(isu_item) == 16 && sizeof(isu_chan) == 4 * ISU_CHAN_WORDS, "k_aerol_isu.h: state layout");

// 1 in bit 0 / 8 / 16 / 24 for every byte of w with ODD parity
__device__ __forceinline__ unsigned isu_odd_bytes(unsigned w)
{
    w ^= w >> 4; w ^= w >> 2; w ^= w >> 1;
    return w & 0x01010101u;
}
// 0xFF in every byte of a word whose index base + b lies in [lo, hi)
__device__ __forceinline__ unsigned isu_range_mask(int base, int lo, int hi)
{
    unsigned m = 0;
#pragma unroll
    for (int b = 0; b < 4; b++)
        if (base + b >= lo && base + b < hi) m |= 0xFFu << (8 * b);
    return m;
}

// A completed item goes to the channel's message log, classified as ParserISU::parse classifies it.  NSRC: the 16-byte groups u holds (a P or T
// channel item's 32; an R channel slot's 3, k_aerolb_isu.h: nothing is read behind them); origin: flag bits set whatever the classification says.
template <int NSRC = 32>
__device__ __forceinline__ void isu_emit(const IPtrs &q, int ch, const isu_item &it, const uint8_t *u, int frame, int kk, int &msg_cnt, int &overflow,
                                         unsigned origin = 0)
{
    if (msg_cnt >= q.msg_cap) { overflow |= ISU_OVERFLOW_BIT; return; }
    const int n = it.len;
    unsigned flags = 0, mode = 0, tak = 0, l0 = 0, l1 = 0, bi = 0;
    int t_lo = 0, t_hi = 0; // text bytes whose parity counts
    if (it.aesid == 0) flags = ISU_F_AES0;
    else if (n > 16 && u[0] == 0xFF && u[1] == 0xFF && (u[15] == 0x83 || u[15] == 0x02))
    {
        flags = ISU_F_ACARS;
        if (u[15] == 0x02) { flags |= ISU_F_TEXT; t_lo = 16; t_hi = n - 4; }
        if (u[n - 4] == 0x97) flags |= ISU_F_MORE;
        mode = u[3] & 0x7Fu; tak = u[11] & 0x7Fu; l0 = u[12] & 0x7Fu; l1 = u[13] & 0x7Fu; bi = u[14] & 0x7Fu;
    }
    uint4 *row = (uint4 *)(q.log + ((size_t)ch * q.msg_cap + msg_cnt) * ISU_ROW_BYTES);
    const uint4 *src = (const uint4 *)u;
    unsigned even = 0; // bytes with even parity among those that count
    for (int c = 0; c < 32; c++)
    {
        uint4 v = {0u, 0u, 0u, 0u};
        if (c < NSRC) v = src[c];
        unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            const int base = 16 * c + 4 * k;
            w[k] &= isu_range_mask(base, 0, n); // (a slot keeps what an earlier, longer item left behind its end)
            if (flags & ISU_F_ACARS) even |= (~isu_odd_bytes(w[k]) & 0x01010101u) & (isu_range_mask(base, 4, 11) | isu_range_mask(base, t_lo, t_hi));
        }
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        row[2 + c] = v;
    }
    if (even) flags |= ISU_F_PARITY;
    flags |= origin;
    uint4 h0, h1;
    h0.x = (unsigned)frame; h0.y = (unsigned)kk; h0.z = it.aesid;
    h0.w = (unsigned)it.gesid | ((unsigned)it.qno << 8) | ((unsigned)it.refno << 16) | ((unsigned)it.nooct << 24);
    h1.x = (unsigned)n | (flags << 16);
    h1.y = mode | (tak << 8) | (l0 << 16) | (l1 << 24);
    h1.z = bi; h1.w = 0;
    row[0] = h0; row[1] = h1;
    msg_cnt++;
}

// ISUData::update with the 10 payload bytes of one CRC-clean unit
__device__ __forceinline__ void isu_update(const IPtrs &q, int ch, isu_chan &s, const uint8_t *d, int frame, int kk, long long *st, int &msg_cnt, int &overflow)
{
    uint8_t *items = q.items + (size_t)ch * ISU_MAX_ITEMS * ISU_ITEM_BYTES;
    if (s.n > ISU_MAX_ITEMS) s.n = ISU_MAX_ITEMS; // (never: keeps every index below inside the channel's memory whatever the state holds)
    if (d[0] == 0x71)
    {
        st[0]++;
        // deleteoldisuitems: every count up by one, those above 10 leave, in list order
        int m = 0;
        for (int i = 0; i < s.n; i++)
        {
            const int slot = isu_slot(s, i);
            isu_item *it = (isu_item *)(items + slot * ISU_ITEM_BYTES);
            const int cnt = it->count + 1;
            if (cnt > 10) s.used &= ~(1u << slot);
            else { it->count = (uint8_t)cnt; isu_set_slot(s, m++, slot); }
        }
        s.n = (uint8_t)m;
        s.a_aesid = ((uint32_t)d[1] << 16) | ((uint32_t)d[2] << 8) | d[3];
        s.a_gesid = d[4]; s.a_qno = d[5] >> 4; s.a_refno = d[5] & 15; s.a_seqno = d[6] & 63; s.a_nooct = d[7] >> 4;
        int slot = -1;
        if (s.a_nooct <= 8)
            for (int i = 0; i < s.n && slot < 0; i++)
            {
                const int sl = isu_slot(s, i);
                const isu_item *it = (const isu_item *)(items + sl * ISU_ITEM_BYTES);
                if (it->aesid == s.a_aesid && it->gesid == s.a_gesid && it->qno == s.a_qno && it->refno == s.a_refno) slot = sl;
            }
        if (slot < 0)
        {
            if (s.n >= ISU_MAX_ITEMS) return; // (never, see above)
            for (int sl = 0; sl < ISU_MAX_ITEMS && slot < 0; sl++) if (!(s.used & (1u << sl))) slot = sl;
            if (slot < 0) return;
            s.used |= 1u << slot;
            isu_set_slot(s, s.n, slot);
            s.n++;
        }
        isu_item nw;
        nw.aesid = s.a_aesid; nw.gesid = s.a_gesid; nw.qno = s.a_qno; nw.refno = s.a_refno; nw.seqno = s.a_seqno; nw.nooct = s.a_nooct;
        nw.count = 0; nw.len = 2; nw.pad = 0;
        uint8_t *base = items + slot * ISU_ITEM_BYTES;
        *(isu_item *)base = nw;
        base[16] = d[8]; base[17] = d[9];
        return;
    }
    if ((d[0] & 0xC0) != 0xC0) return;
    st[1]++;
    s.a_seqno = d[0] & 63; s.a_qno = d[1] >> 4; s.a_refno = d[1] & 15;
    int slot = -1;
    if (s.a_nooct <= 8)
        for (int i = 0; i < s.n && slot < 0; i++)
        {
            const int sl = isu_slot(s, i);
            const isu_item *it = (const isu_item *)(items + sl * ISU_ITEM_BYTES);
            if (it->aesid == s.a_aesid && it->gesid == s.a_gesid && (int)s.a_seqno + 1 == (int)it->seqno && it->qno == s.a_qno && it->refno == s.a_refno) slot = sl;
        }
    if (slot < 0) { st[2]++; return; }
    uint8_t *base = items + slot * ISU_ITEM_BYTES;
    isu_item it = *(const isu_item *)base;
    it.seqno--;
    const int take = it.seqno == 0 ? it.nooct : 8; // the last SSU: d[2 .. nooct + 1]
    int len = it.len;
#pragma unroll
    for (int i = 0; i < 8; i++) if (i < take && len < ISU_MAX_BYTES) base[16 + len++] = d[2 + i];
    it.len = (uint16_t)len;
    *(isu_item *)base = it;
    if (it.seqno == 0)
    {
        st[3]++;
        isu_emit(q, ch, it, base + 16, frame, kk, msg_cnt, overflow);
    }
}

__global__ void k_aerol_isu(const AGeom g, const APtrs p, const IPtrs q)
{
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= g.nch) return;
    const int mark = p.isumark[ch];
    const bool frame_end = ALD(AI_HAS_BLOCK) && (ALD(AI_CNTR) - g.BitsInHeader) == (g.NumberOfBits - 1);
    if (!mark && !frame_end) return;
    isu_chan s;
    uint32_t *cw = q.chan + (size_t)ch * ISU_CHAN_WORDS;
    __builtin_memcpy(&s, cw, sizeof(s));
    if (mark) { s.n = 0; s.used = 0; p.isumark[ch] = 0; } // ISUData::reset: the list goes, `a` stays
    if (frame_end)
    {
        const uint8_t *info = p.info + (size_t)ch * g.info_cap;
        const int ninfo = ALD(AI_NINFO), frame = ALD(AI_NFRAMES) - 1; // (aerol_frame_end has counted this frame already)
        int msg_cnt = q.msg_cnt[ch], overflow = 0;
        long long st[4] = {0, 0, 0, 0};
        for (int kk = 0; kk < ninfo / 12; kk++)
        {
            const unsigned b0 = info[kk * 12];
            if (b0 != 0x71u && (b0 & 0xC0u) != 0xC0u) continue; // fill-in units and broadcasts pay for no CRC
            uint8_t su[12];
            __builtin_memcpy(su, info + kk * 12, 12);
            // (aerol_frame_end's all-zero exception cannot apply: the first byte is not 0)
            if (aerol_crc16(su, 10) != (((unsigned)su[11] << 8) | su[10])) continue;
            isu_update(q, ch, s, su, frame, kk, st, msg_cnt, overflow);
        }
        q.msg_cnt[ch] = msg_cnt;
        if (overflow) ALD(AI_OVERFLOW) = ALD(AI_OVERFLOW) | overflow;
        long long *gs = q.stats + (size_t)ch * 4;
#pragma unroll
        for (int k = 0; k < 4; k++) if (st[k]) gs[k] += st[k];
    }
    __builtin_memcpy(cw, &s, sizeof(s));
}

// jaero_aerol_isu_enable: an empty log has not overflowed
__global__ void k_aerol_isu_clear_overflow(const AGeom g, const APtrs p)
{
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= g.nch) return;
    const int ov = ALD(AI_OVERFLOW);
    if (ov & ISU_OVERFLOW_BIT) ALD(AI_OVERFLOW) = ov & ~ISU_OVERFLOW_BIT;
}
