// TEST INFRASTRUCTURE ONLY: the device code of the burst bank's R / T reassembly (jaero_amd/csrc/k_aerolb_isu.h: k_aerolb_isu with risu_update, and
// isu_update / isu_emit of k_aerol_isu.h behind it; the mark k_aerolb_post writes) compiled as plain host functions and driven thread by thread
// behind the emulated packet search of aerolb_emul.cpp, in the rounds of jaero_aerol_write (aerol_host.h) with the reassembly enabled.  Built by
// tests/test_aerolb_isu_emul.py with g++ -Itests/host_emul/stub; tests/host_emul/aerolb_isu_main.cpp drives it from a main of its own.
#include "aerolb_emul.cpp"

#include "../../jaero_amd/csrc/k_aerolb_isu.h"

struct EmulR
{
    EmulB *e;
    IPtrs q;
    RPtrs r;
};

// jaero_aerol_create_burst + jaero_aerol_rt_enable(msg_cap)
extern "C" EmulR *emulr_create(int nch, int fb, int su_cap, int msg_cap)
{
    EmulR *x = new EmulR();
    x->e = emulb_create(nch, fb, su_cap);
    EmulB *e = x->e;
    const AGeom &g = e->g;
    memset(&x->q, 0, sizeof(x->q));
    e->p.rtmark = zalloc<long long>(e, (size_t)g.nchp);
    x->q.chan = zalloc<uint32_t>(e, (size_t)g.nchp * ISU_CHAN_WORDS);
    x->q.items = zalloc<uint8_t>(e, (size_t)g.nchp * ISU_MAX_ITEMS * ISU_ITEM_BYTES);
    // the log is not zeroed by the bank (its rows are written whole): fill it with a pattern
    x->q.log = zalloc<uint8_t>(e, (size_t)g.nchp * msg_cap * ISU_ROW_BYTES);
    memset(x->q.log, 0xA5, (size_t)g.nchp * msg_cap * ISU_ROW_BYTES);
    x->q.msg_cnt = zalloc<int>(e, (size_t)g.nchp);
    x->q.msg_cap = msg_cap;
    x->r.chan = zalloc<uint32_t>(e, (size_t)g.nchp * RISU_CHAN_WORDS);
    // exactly the slots, behind no spare byte: a read or write past a channel's last slot is the sanitizer's to find (aerolb_isu_main.cpp)
    x->r.items = (uint8_t *)malloc((size_t)g.nchp * ISU_MAX_ITEMS * RISU_SLOT_BYTES);
    memset(x->r.items, 0, (size_t)g.nchp * ISU_MAX_ITEMS * RISU_SLOT_BYTES);
    e->mem.push_back(x->r.items);
    x->r.stats = zalloc<long long>(e, (size_t)g.nchp * RT_NSTATS);
    return x;
}
extern "C" void emulr_destroy(EmulR *x)
{
    if (!x) return;
    emulb_destroy(x->e);
    delete x;
}

// one jaero_aerol_write (emulb_write's rounds, k_aerolb_isu behind every k_aerolb_post)
extern "C" int emulr_write(EmulR *x, const int16_t *soft, const int *counts, int stride, int max_count)
{
    EmulB *e = x->e;
    const AGeom &g = e->g;
    const APtrs &p = e->p;
    const bool w = ((((size_t)soft) | ((size_t)stride * 2)) & 15) == 0;
    const int rounds = max_count / 192 + 4;
    std::vector<uint8_t> out(RT_BLOCKSZ / 2 + 64);
    for (int r = 0; r < rounds; r++)
    {
        if (w) each_thread(g.nchp, [&] { k_aerolb_bits<true>(g, p, soft, counts, stride); });
        else each_thread(g.nchp, [&] { k_aerolb_bits<false>(g, p, soft, counts, stride); });
        for (int ch = 0; ch < g.nch; ch++)
        {
            if (!ALD(AI_HAS_BLOCK)) continue;
            const int len = ALD(BI_TRIAL_LEN), cols = len / 64;
            const uint8_t *blk = p.rx + (size_t)ch * RT_BLOCKSZ;
            uint8_t *dst = p.deint + (size_t)ch * RT_BLOCKSZ;
            for (int lane = 0; lane < 64; lane++)
            {
                const int perm = (lane * 27) & 63;
                if (g.oqpsk)
                    for (int j = 0; j < cols; j++) dst[j * 64 + lane] = blk[perm * cols + j];
                else
                {
                    for (int j = 0; j < 5 && j < cols; j++) dst[j * 64 + lane] = blk[perm * 5 + j];
                    for (int proc = 5; proc + 3 <= cols; proc += 3)
                        for (int j = 0; j < 3; j++) dst[(proc + j) * 64 + lane] = blk[64 * proc + perm * 3 + j];
                }
            }
            const int nb = jo_decode_soft(e->codec, dst, len, out.data());
            uint8_t *vb = p.vbits + (size_t)ch * (RT_BLOCKSZ / 2);
            memcpy(vb, out.data(), (size_t)(nb < len / 2 ? nb : len / 2));
        }
        each_thread(g.nchp, [&] { k_aerolb_post(g, p); });
        each_thread(g.nchp, [&] { k_aerolb_isu(g, p, x->q, x->r); });
    }
    each_thread(g.nchp, [&] { k_aerol_end_write(g, p, counts); });
    return 0;
}

// which 0 / 1: as emulb_read; 2: message rows (ISU_ROW_BYTES each); returns the number of rows copied
extern "C" int emulr_read(EmulR *x, int ch, int which, void *rows, int cap)
{
    if (which < 2) return emulb_read(x->e, ch, which, rows, cap);
    const int n = std::min(x->q.msg_cnt[ch], cap);
    memcpy(rows, x->q.log + (size_t)ch * x->q.msg_cap * ISU_ROW_BYTES, (size_t)n * ISU_ROW_BYTES);
    return n;
}
extern "C" int emulr_overflow(EmulR *x, int ch) { return emulb_overflow(x->e, ch); }
extern "C" void emulr_stats(EmulR *x, int ch, long long *st8) { memcpy(st8, x->r.stats + (size_t)ch * RT_NSTATS, RT_NSTATS * sizeof(long long)); }
