// k_aerolb_isu.h -- what the reference does with an accepted packet of a burst (R / T channel) bank: RISUData::update for an R packet that carries
// user data (JAERO/aerol.cpp:6-113,1358,1395; aerol.h:135-146,231-243), ISUData::update for every signal unit of a T packet (aerol.cpp:1488-1516),
// and the header part of ParserISU::parse for what completes.  The definition, quirks included, is in include/jaero_hip.h; tests/rt_isu_oracle.py
// restates it.  One lane per channel, all state in HBM:
//   T path  the IPtrs state of k_aerol_isu.h (isu_update / isu_emit unchanged), the counters apart
//   R path  chan  [nchp][RISU_CHAN_WORDS]  the list's length, the slots in use and its order (slot numbers, oldest first, as isu_chan::order)
//           items [nchp][11][RISU_SLOT_BYTES]  per slot a 16-byte header and 48 bytes of user data (33 at most are ever used)
//   stats [nchp][8]; the message log and its counts are the IPtrs'
// k_aerolb_isu runs behind every k_aerolb_post of a round.  A lane has work only when that k_aerolb_post accepted a packet on it: the mark
// (APtrs::rtmark) then holds the packet's type, byte count and number, and the packet's descrambled bits still lie in p.vbits, one per byte -- the
// bit walk of the next round is the first to touch them again -- so a packet log without room loses no message.  Integer only; plain stores.
#pragma once
#include "k_aerol_burst.h"
#include "k_aerol_isu.h"

#define RISU_SLOT_BYTES 64 // 16 header + 48 data (the data 16-byte aligned: emitted 16 bytes per load, three loads, none behind the slot)
#define RISU_MAX_BYTES 33  // 11 * 2 + 11: the third unit of three, full
#define RISU_CHAN_WORDS 4
enum { ISU_F_RCHAN = 32, ISU_F_RSIGNAL = 64 }; // origin bits of a row's flags: from RISUData; a signalling-information unit (SUTYPE 15)
enum { RT_ST_T_ISU, RT_ST_T_SSU, RT_ST_T_MISSING, RT_ST_T_DONE, RT_ST_R_FED, RT_ST_R_NEW, RT_ST_R_DONE, RT_ST_R_SIGNAL, RT_NSTATS };

struct risu_item // a slot's header
{
    uint32_t aesid;
    uint8_t gesid, qno, refno, count;
    uint8_t len, filled, pad0, pad1; // user-data bytes (the QByteArray's size), filledarray
    uint32_t pad2;
};
struct risu_chan // a channel's header (the scratch item is cleared by every update: it needs no memory)
{
    uint32_t n, used;         // list length; bit s: slot s holds an item of the list
    unsigned long long order; // the list, oldest first: slot number of entry i in bits 4 i .. 4 i + 3
};
struct RPtrs
{
    uint32_t *chan;   // [nchp][RISU_CHAN_WORDS]
    uint8_t *items;   // [nchp][ISU_MAX_ITEMS][RISU_SLOT_BYTES]
    long long *stats; // [nchp][RT_NSTATS]
};
struct risu_counts { int fed, appended, done, signal; }; // what one update adds to RT_ST_R_*
static_assert(sizeof(risu_item) == 16 && sizeof(risu_chan) == 4 * RISU_CHAN_WORDS, "k_aerolb_isu.h: state layout");

__device__ __forceinline__ int risu_slot(const risu_chan &s, int i)
{
    const int sl = (int)((s.order >> (4 * i)) & 15ull);
    return sl < ISU_MAX_ITEMS ? sl : 0; // (never above: keeps the address inside the channel's memory whatever the state holds)
}
__device__ __forceinline__ void risu_set_slot(risu_chan &s, int i, int slot)
{
    s.order = (s.order & ~(15ull << (4 * i))) | ((unsigned long long)slot << (4 * i));
}

// RISUData::update with the 17 bytes of an R packet whose second byte has bit 3 set
__device__ __forceinline__ void risu_update(const IPtrs &q, const RPtrs &r, int ch, risu_chan &s, const uint8_t *d, int frame, risu_counts &st, int &msg_cnt,
                                            int &overflow)
{
    uint8_t *items = r.items + (size_t)ch * ISU_MAX_ITEMS * RISU_SLOT_BYTES;
    if (s.n > ISU_MAX_ITEMS) s.n = ISU_MAX_ITEMS; // (never: keeps every index below inside the channel's memory whatever the state holds)
    st.fed++;
    // deleteoldisuitems: every count up by one, those above 10 leave, in list order
    int m = 0;
    for (int i = 0; i < (int)s.n; i++)
    {
        const int slot = risu_slot(s, i);
        risu_item *it = (risu_item *)(items + slot * RISU_SLOT_BYTES);
        const int cnt = it->count + 1;
        if (cnt > 10) s.used &= ~(1u << slot);
        else { it->count = (uint8_t)cnt; risu_set_slot(s, m++, slot); }
    }
    s.n = (uint32_t)m;
    const int seqind = d[0] >> 4, sutype = d[0] & 15;
    const uint32_t aesid = ((uint32_t)d[2] << 16) | ((uint32_t)d[3] << 8) | d[4];
    const uint8_t gesid = d[5], qno = d[1] >> 4, refno = d[1] & 7;
    int slot = -1, idx = -1;
    if (sutype >= 1 && sutype <= 11)
        for (int i = 0; i < (int)s.n && slot < 0; i++)
        {
            const int sl = risu_slot(s, i);
            const risu_item *it = (const risu_item *)(items + sl * RISU_SLOT_BYTES);
            if (it->gesid == gesid && it->aesid == aesid && it->qno == qno && it->refno == refno) { slot = sl; idx = i; }
        }
    risu_item it;
    if (slot < 0)
    {
        if (s.n >= ISU_MAX_ITEMS) return; // (never: ten items at most survive the ageing)
        for (int sl = 0; sl < ISU_MAX_ITEMS && slot < 0; sl++) if (!(s.used & (1u << sl))) slot = sl;
        if (slot < 0) return;
        s.used |= 1u << slot;
        idx = (int)s.n;
        risu_set_slot(s, idx, slot);
        s.n++;
        st.appended++;
        it.aesid = aesid; it.gesid = gesid; it.qno = qno; it.refno = refno; it.len = 0; it.filled = 0; it.pad0 = it.pad1 = 0; it.pad2 = 0;
    }
    else it = *(const risu_item *)(items + slot * RISU_SLOT_BYTES);
    it.count = 0;
    uint8_t *base = items + slot * RISU_SLOT_BYTES;
    uint8_t *u = base + 16;
    // SEQINDICATOR 1 .. 6 -> (SUTotal, SUindex); anything else total 0, which never completes
    const int total = seqind == 1 ? 1 : (seqind == 2 || seqind == 3) ? 2 : (seqind >= 4 && seqind <= 6) ? 3 : 0;
    const int index = (seqind == 3 || seqind == 5) ? 1 : seqind == 6 ? 2 : 0;
    const int bytes = (sutype >= 1 && sutype <= 11) ? sutype : 0;
    const bool signal = sutype == 15;
    int len = it.len > RISU_MAX_BYTES ? RISU_MAX_BYTES : it.len; // (never above)
    const int thisnum = 11 * total - 11 + bytes;                // <= 33
    if (thisnum > 0)
    {
        if (len == 0) { for (int i = 0; i < thisnum; i++) u[i] = 0; len = thisnum; } // resize of an empty array: the new bytes are 0 here
        if (thisnum < len) len = thisnum;                                              // a longer one is cut, a shorter one stays
    }
    if (!signal)
    {
        const int end = 11 * index + bytes; // <= 33
        if (bytes > 0 && end > len) { for (int i = len; i < end; i++) u[i] = 0; len = end; } // a write past the end grows the array to reach
#pragma unroll
        for (int i = 0; i < 11; i++) if (i < bytes) u[11 * index + i] = d[6 + i];
        it.filled |= (uint8_t)(1u << index);
    }
    else len = 0;
    it.len = (uint8_t)len;
    const bool done = signal || (it.filled == 7 && total == 3) || (it.filled == 3 && total == 2) || (it.filled == 1 && total == 1);
    if (!done) { *(risu_item *)base = it; return; }
    // lastvalidisuitem = *pisuitem; isuitems.removeAt(idx)
    st.done++;
    st.signal += signal ? 1 : 0;
    isu_item e;
    e.aesid = it.aesid; e.gesid = it.gesid; e.qno = it.qno; e.refno = it.refno; e.seqno = 0; e.nooct = 0; e.count = 0; e.len = (uint16_t)len; e.pad = 0;
    isu_emit<RISU_SLOT_BYTES / 16 - 1>(q, ch, e, u, frame, 0, msg_cnt, overflow, ISU_F_RCHAN | (signal ? ISU_F_RSIGNAL : 0u));
    s.used &= ~(1u << slot);
    for (int i = idx; i + 1 < (int)s.n; i++) risu_set_slot(s, i, risu_slot(s, i + 1));
    s.n--;
}

__global__ __launch_bounds__(64) void k_aerolb_isu(const AGeom g, const APtrs p, const IPtrs q, const RPtrs r)
{
    const int ch = blockIdx.x * 64 + threadIdx.x;
    if (ch >= g.nch) return;
    const long long mark = p.rtmark[ch];
    if (!mark) return;
    p.rtmark[ch] = 0;
    const int type = (int)(mark & 3), ninfo = (int)((mark >> 2) & 0x3FFF), frame = (int)(mark >> 16);
    const unsigned long long *dec = (const unsigned long long *)(p.vbits + (size_t)ch * (RT_BLOCKSZ / 2)); // one bit per byte, the first bit of a byte its LSB
    int msg_cnt = q.msg_cnt[ch], overflow = 0;
    long long ts[4] = {0, 0, 0, 0}; // RT_ST_T_*: the four counters of k_aerol_isu, in its order
    risu_counts rs = {0, 0, 0, 0};
    if (type == 1)
    {
        uint8_t d[17];
#pragma unroll
        for (int j = 0; j < 17; j++) d[j] = (uint8_t)aerolb_pack8(dec[j]);
        if (!(d[1] & 0x08)) return; // (aerol.cpp:1358: any other R packet changes nothing)
        risu_chan s;
        uint32_t *cw = r.chan + (size_t)ch * RISU_CHAN_WORDS;
        __builtin_memcpy(&s, cw, sizeof(s));
        risu_update(q, r, ch, s, d, frame, rs, msg_cnt, overflow);
        __builtin_memcpy(cw, &s, sizeof(s));
    }
    else
    {
        // numberofsus: 1 + (blockptr - 320) / 192 at 10 500 bps (aerol.h:849), targetSUSize at 600 / 1200 bps (aerol.h:759), where the block holds one
        // unit more; from the byte count ninfo = blockptr / 16 - 1.  Never more than the 31 units 95 columns hold.
        int nsus = g.oqpsk ? (ninfo - 7) / 12 : (ninfo - 19) / 12;
        nsus = nsus < 0 ? 0 : nsus > 31 ? 31 : nsus;
        isu_chan s;
        uint32_t *cw = q.chan + (size_t)ch * ISU_CHAN_WORDS;
        __builtin_memcpy(&s, cw, sizeof(s));
        for (int kk = 0; kk < nsus; kk++)
        {
            uint8_t d[10];
#pragma unroll
            for (int j = 0; j < 10; j++) d[j] = (uint8_t)aerolb_pack8(dec[6 + 12 * kk + j]);
            isu_update(q, ch, s, d, frame, kk, ts, msg_cnt, overflow);
        }
        __builtin_memcpy(cw, &s, sizeof(s));
    }
    q.msg_cnt[ch] = msg_cnt;
    if (overflow) ALD(AI_OVERFLOW) = ALD(AI_OVERFLOW) | overflow;
    long long *gs = r.stats + (size_t)ch * RT_NSTATS;
#pragma unroll
    for (int k = 0; k < 4; k++) if (ts[k]) gs[RT_ST_T_ISU + k] += ts[k];
    if (rs.fed) gs[RT_ST_R_FED] += rs.fed;
    if (rs.appended) gs[RT_ST_R_NEW] += rs.appended;
    if (rs.done) gs[RT_ST_R_DONE] += rs.done;
    if (rs.signal) gs[RT_ST_R_SIGNAL] += rs.signal;
}
