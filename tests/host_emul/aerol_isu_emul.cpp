// TEST INFRASTRUCTURE ONLY: the device code of the ISU reassembly (jaero_amd/csrc/k_aerol_isu.h: k_aerol_isu with isu_update / isu_emit, and the
// short-frame mark aerol_event writes) compiled as plain host functions and driven thread by thread behind the emulated bit pipeline of
// aerolp_emul.cpp, in the rounds of jaero_aerol_write (aerol_host.h) with the reassembly enabled.  Built by tests/test_aerol_isu_emul.py with
// g++ -Itests/host_emul/stub.
#include "aerolp_emul.cpp"

#include "../../jaero_amd/csrc/k_aerol_isu.h"

struct EmulI
{
    EmulP *e;
    IPtrs q;
};

// jaero_aerol_create + jaero_aerol_isu_enable(msg_cap)
extern "C" EmulI *emuli_create(int nch, int fb, int su_cap, int msg_cap)
{
    EmulI *x = new EmulI();
    x->e = emulp_create(nch, fb, su_cap);
    EmulP *e = x->e;
    const AGeom &g = e->g;
    e->p.isumark = zalloc<int>(e, (size_t)g.nchp);
    x->q.chan = zalloc<uint32_t>(e, (size_t)g.nchp * ISU_CHAN_WORDS);
    x->q.items = zalloc<uint8_t>(e, (size_t)g.nchp * ISU_MAX_ITEMS * ISU_ITEM_BYTES);
    // the log is not zeroed by the bank (its rows are written whole): fill it with a pattern
    x->q.log = zalloc<uint8_t>(e, (size_t)g.nchp * msg_cap * ISU_ROW_BYTES);
    memset(x->q.log, 0xA5, (size_t)g.nchp * msg_cap * ISU_ROW_BYTES);
    x->q.msg_cnt = zalloc<int>(e, (size_t)g.nchp);
    x->q.stats = zalloc<long long>(e, (size_t)g.nchp * 4);
    x->q.msg_cap = msg_cap;
    return x;
}
extern "C" void emuli_destroy(EmulI *x)
{
    if (!x) return;
    emulp_destroy(x->e);
    delete x;
}

extern "C" int emuli_write(EmulI *x, const int16_t *soft, const int *counts, int stride, int max_count)
{
    EmulP *e = x->e;
    const AGeom &g = e->g;
    const APtrs &p = e->p;
    const int rounds = max_count / g.blocksz + 2;
    std::vector<uint8_t> out(g.blocksz / 2 + 64);
    for (int r = 0; r < rounds; r++)
    {
        each_thread(g.nchp, [&] { k_aerol_bits<false>(g, p, soft, counts, stride); });
        for (int ch = 0; ch < g.nch; ch++)
        {
            if (!ALD(AI_HAS_BLOCK)) continue;
            const uint8_t *blk = p.rx + (size_t)ch * g.blocksz;
            uint8_t *dst = p.deint + (size_t)ch * g.blocksz;
            for (int i = 0; i < 64; i++)
                for (int j = 0; j < g.N; j++) dst[j * 64 + i] = blk[((i * 27) & 63) * g.N + j];
            const int nb = jo_decode_continuous(e->codec[ch], dst, g.blocksz, out.data());
            memcpy(p.vbits + (size_t)ch * (g.blocksz / 2), out.data(), (size_t)(nb < g.blocksz / 2 ? nb : g.blocksz / 2));
        }
        each_thread(g.nchp, [&] { k_aerol_post(g, p); });
        each_thread(g.nchp, [&] { k_aerol_isu(g, p, x->q); });
    }
    each_thread(g.nchp, [&] { k_aerol_end_write(g, p, counts); });
    return 0;
}

// which 0 / 1: as emulp_read; 2: message rows (ISU_ROW_BYTES each); returns the number of rows copied
extern "C" int emuli_read(EmulI *x, int ch, int which, void *rows, int cap)
{
    if (which < 2) return emulp_read(x->e, ch, which, rows, cap);
    const int n = std::min(x->q.msg_cnt[ch], cap);
    memcpy(rows, x->q.log + (size_t)ch * x->q.msg_cap * ISU_ROW_BYTES, (size_t)n * ISU_ROW_BYTES);
    return n;
}
extern "C" int emuli_overflow(EmulI *x, int ch) { return emulp_overflow(x->e, ch); }
extern "C" void emuli_stats(EmulI *x, int ch, long long *st4) { memcpy(st4, x->q.stats + (size_t)ch * 4, 4 * sizeof(long long)); }
