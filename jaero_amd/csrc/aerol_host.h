// aerol_host.h -- C ABI of the Aero-L bit pipeline bank; included at the end of jaero_hip.hip.
#pragma once

#include <mutex>
#include "aerolc.h"
#include "k_aerol_isu.h"
#include "k_aerolb_isu.h"
#include "sweep_host.h"

struct jaero_aerol_ctx : DevHandle // (never poisoned, and ordered by its caller: a write moves last_stream without an event)
{
    AGeom g{}; // fb = 8400: nch, nchp and fb only
    APtrs p{};
    bool cchan = false; // fb = 8400: the C-channel pipeline (aerolc.h) on cg / cp
    CGeom cg{};
    CPtrs cp{};
    DevMem mem;
    int16_t *d_soft = nullptr; int *d_counts = nullptr; int stage_stride = 0;
    unsigned long long *d_vhist = nullptr; // k_viterbi_lanes history scratch (large banks only)
    // the three kernel classes of a write: 0 = the bit walk, 1 = k_viterbi + overlap update, 2 = the end of a block / frame; 3 = the sweep's kernels
    // (jaero_aerol_read_all), 4 = k_dcd_link, 5 = k_aerol_isu / k_aerolb_isu (jaero_aerol_profile2_read)
    KernelTimer timer{6};
    SweepBufs sweep;
    jaero_ctx *link = nullptr; // the demodulator bank whose dcd follows this bank's DataCarrierDetect emissions (jaero_aerol_link_dcd)
    int *d_dcdmark = nullptr;  // [nchp], allocated by the first link
    // ISU / SSU reassembly (jaero_aerol_isu_enable, k_aerol_isu.h): allocated by the first enable, launched while isu_on
    IPtrs isu{};
    int *d_isumark = nullptr;
    bool isu_on = false;
    long long isu_bytes = 0;
    // R / T user data of a burst bank (jaero_aerol_rt_enable, k_aerolb_isu.h): the T path's list and the message log are isu's, the rest is here
    RPtrs rt{};
    long long *d_rtmark = nullptr;
    bool rt_on = false;
    long long rt_bytes = 0;
};

extern "C" int jaero_aerol_profile_enable(jaero_aerol_ctx *c, int on)
{
    if (!c) return fail(JAERO_EINVAL, "null ctx");
    c->timer.on = on != 0;
    return 0;
}
extern "C" int jaero_aerol_profile_read(jaero_aerol_ctx *c, int which, double *total_ms, int *launches, int reset)
{
    if (!c || which < 0 || which > 2) return fail(JAERO_EINVAL, "jaero_aerol_profile_read: bad arguments");
    return c->timer.read(c->device, which, total_ms, launches, reset);
}

extern "C" int jaero_aerol_profile2_read(jaero_aerol_ctx *c, int which, double *total_ms, int *launches, int reset)
{
    if (!c || which < 0 || which > 5) return fail(JAERO_EINVAL, "jaero_aerol_profile2_read: bad arguments");
    return c->timer.read(c->device, which, total_ms, launches, reset);
}

// ------------------------------------------------------------------------------------------ the dcd link
// The linked Aero-L banks of the process (jaero_aerol_ctx::link names the other side): how a demodulator bank finds the Aero-L bank it feeds.
static std::mutex g_links_mu;
static std::vector<jaero_aerol_ctx *> g_links;
static jaero_aerol_ctx *link_of_bank(const jaero_ctx *b)
{
    std::lock_guard<std::mutex> lk(g_links_mu);
    for (jaero_aerol_ctx *a : g_links) if (a->link == b) return a;
    return nullptr;
}
static bool dcd_bank_linked(const jaero_ctx *b) { return link_of_bank(b) != nullptr; }
// Ends a link: one synchronisation, then the bank's host mirror learns the JF_DCD bits the device holds (a later rate change carries the
// mirror over, swap_in), and both sides forget each other.
static void aerol_unlink(jaero_aerol_ctx *c)
{
    jaero_ctx *b = c->link;
    if (!b) return;
    (void)c->quiesce();
    (void)b->quiesce(); // (on the same device: jaero_aerol_link_dcd)
    std::vector<int> f(b->o_nch);
    if (!b->poisoned && hipMemcpy(f.data(), b->o_flags, sizeof(int) * f.size(), hipMemcpyDeviceToHost) == hipSuccess)
        for (int ch = 0; ch < b->o_nch; ch++) b->m.flags[ch] = (b->m.flags[ch] & ~JF_DCD) | (f[ch] & JF_DCD);
    c->p.dcdmark = nullptr; c->cp.dcdmark = nullptr;
    std::lock_guard<std::mutex> lk(g_links_mu);
    for (size_t k = 0; k < g_links.size(); k++) if (g_links[k] == c) { g_links.erase(g_links.begin() + k); break; }
    c->link = nullptr;
}
static void dcd_unlink_bank(jaero_ctx *b)
{
    if (jaero_aerol_ctx *a = link_of_bank(b)) aerol_unlink(a);
}

extern "C" int jaero_aerol_link_dcd(jaero_aerol_ctx *c, jaero_ctx *b)
{
    const char *who = "jaero_aerol_link_dcd";
    if (!c) return fail(JAERO_EINVAL, "%s: null ctx", who);
    if (!b) { aerol_unlink(c); return 0; }
    if (b->device != c->device) return fail(JAERO_EINVAL, "%s: the bank is on device %d, the Aero-L bank on device %d", who, b->device, c->device);
    if (b->o_nch != c->g.nch) return fail(JAERO_EINVAL, "%s: the bank has %d channels, the Aero-L bank %d", who, b->o_nch, c->g.nch);
    if (b->burst != (c->g.burst != 0)) return fail(JAERO_EINVAL, "%s: a burst Aero-L bank goes with a burst demodulator bank, a continuous one with a continuous one", who);
    const double bank_fb = b->burst ? b->bg.fb : b->g.fb;
    if (bank_fb != (double)c->g.fb) return fail(JAERO_EINVAL, "%s: the bank runs at %g bps, the Aero-L bank at %d", who, bank_fb, c->g.fb);
    if (c->link == b) return 0; // the same pair again
    if (c->link || dcd_bank_linked(b)) return fail(JAERO_EINVAL, "%s: already linked (unlink first: bank = NULL)", who);
    if (b->burst && b->bg.kind == JAERO_KIND_BURST_OQPSK)
        return fail(JAERO_ENOTSUP, "%s: the reference connects DataCarrierDetect to no slot of the burst OQPSK demodulator (mainwindow.cpp:234-237)", who);
    if (b->burst) return fail(JAERO_ENOTSUP, "%s: burst MSK banks are not linked yet (only continuous banks are)", who);
    POISONCHK(b, who, POISON_LINKED_BANK);
    HIPCHK(hipSetDevice(c->device));
    int rc = 0;
    if (!c->d_dcdmark && (rc = dalloc(c->mem, &c->d_dcdmark, (size_t)c->g.nchp, false))) return rc;
    // emissions from before the link are not replayed: the marks start empty, behind whatever the Aero-L bank still has in flight on its stream,
    // and are empty before this call returns (a write on any stream, blocking or not, finds them so)
    HIPCHK(hipMemsetAsync(c->d_dcdmark, 0, sizeof(int) * (size_t)c->g.nchp, c->last_stream));
    QUIESCE(c);
    if (c->cchan) c->cp.dcdmark = c->d_dcdmark; else c->p.dcdmark = c->d_dcdmark;
    c->link = b;
    std::lock_guard<std::mutex> lk(g_links_mu);
    g_links.push_back(c);
    return 0;
}
// behind the last kernel of a jaero_aerol_write / jaero_aerol_tick_dcd of a linked handle, on its stream
static int aerol_link_apply(jaero_aerol_ctx *c, hipStream_t st)
{
    if (!c->link) return 0;
    const int pi = c->timer.begin(4, st);
    hipLaunchKernelGGL(k_dcd_link, dim3((c->g.nch + 255) / 256), dim3(256), 0, st, c->d_dcdmark, c->link->o_flags, c->g.nch, (int)JF_DCD);
    c->timer.end(pi, st);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" void jaero_aerol_destroy(jaero_aerol_ctx *c)
{
    if (!c) return;
    aerol_unlink(c);
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    delete c; // its device memory and timing events with it
}

// the C-channel state (aerolc.h) of a bank whose g.nch / g.nchp are set
static int aerolc_init(jaero_aerol_ctx *c, int su_capacity, const std::vector<uint8_t> &scr)
{
    CGeom &g = c->cg;
    CPtrs &p = c->cp;
    DevMem &m = c->mem;
    g.nch = c->g.nch; g.nchp = c->g.nchp;
    g.su_cap = su_capacity > 0 ? su_capacity : 3 * 64; // 64 frames between reads
    g.v_cap = (g.su_cap + 2) / 3;
    g.ev_cap = 256;
    int rc;
    DA(m, p.I, (size_t)CI_NFIELDS * g.nchp);
    DA(m, p.B, (size_t)4 * g.nchp);
    DA(m, p.dep, (size_t)g.nchp * CC_PITCH);
    DA(m, p.vbits, (size_t)g.nchp * (CC_NSOFT / 2));
    DA(m, p.overlap, (size_t)g.nchp * 64);
    DA(m, p.dl2, (size_t)CC_PREV_PITCH * g.nchp + 64);
    DA(m, p.sus, (size_t)g.nchp * g.su_cap * 16);
    DA(m, p.voice, (size_t)g.nchp * g.v_cap * 304);
    DA(m, p.events, (size_t)g.nchp * g.ev_cap * 3);
    if (viterbi_use_lanes(g.nch, CC_NSOFT, 24)) DA(m, c->d_vhist, viterbi_hist_bytes(g.nch) / sizeof(unsigned long long));
    uint8_t *d_scr = nullptr;
    DA(m, d_scr, 5000);
    unsigned long long *d_scrf = nullptr;
    DA(m, d_scrf, 50);
    p.scr = d_scr; p.scrf = d_scrf;
    HIPCHK(hipMemcpy(d_scr, scr.data(), 5000, hipMemcpyHostToDevice));
    std::vector<unsigned long long> scrf(50, 0ull);
    for (int y = 0; y < 25; y++)
        for (int i = 0; i < 108; i++) scrf[2 * y + i / 64] |= (unsigned long long)(scr[109 * y + 1 + i] & 1) << (i % 64);
    HIPCHK(hipMemcpy(d_scrf, scrf.data(), scrf.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    // the depunctured buffer: every 4th symbol an erasure, for good (the walk only writes the other three)
    std::vector<uint8_t> dep((size_t)g.nchp * CC_PITCH, 0);
    for (size_t k = 0; k < dep.size(); k++) if ((k % CC_PITCH) % 4 == 3) dep[k] = 128;
    HIPCHK(hipMemcpy(p.dep, dep.data(), dep.size(), hipMemcpyHostToDevice));
    std::vector<int> I((size_t)CI_NFIELDS * g.nchp, 0);
    for (int ch = 0; ch < g.nchp; ch++)
    {
        I[(size_t)CI_CNTR * g.nchp + ch] = 1000000000; // AeroL constructor (aerol.cpp:907)
        I[(size_t)CI_EV_CNT * g.nchp + ch] = 1;        // row 0 = [0, DCD, 0]: DataCarrierDetect(false) emitted by the constructor
    }
    HIPCHK(hipMemcpy(p.I, I.data(), I.size() * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

// aerol_create behind `new jaero_aerol_ctx`: what it allocated before a failure goes with jaero_aerol_destroy
static int aerol_init(jaero_aerol_ctx *c, int nchannels, int fb, int max_softbits_per_write, int su_capacity, int burst)
{
    int rc;
    DevMem &m = c->mem;
    AGeom &g = c->g;
    g.nch = nchannels; g.nchp = (nchannels + 63) / 64 * 64; g.fb = fb;
    c->stage_stride = max_softbits_per_write;
    DA(m, c->d_soft, (size_t)g.nch * max_softbits_per_write);
    DA(m, c->d_counts, g.nchp);
    const std::vector<uint8_t> scr = scrambler_bits();
    if (fb == 8400 && !burst) // C channel (aerolc.h)
    {
        c->cchan = true;
        if ((rc = aerolc_init(c, su_capacity, scr))) return rc;
        HIPCHK(hipDeviceSynchronize());
        return 0;
    }
    // AeroL::setSettings (JAERO/aerol.cpp:990-1072), burstmode = false
    switch (fb)
    {
    case 600: g.N = 6; g.dl2_sz = 576 - 6 + 1; g.NumberOfBits = 1152; g.BitsInHeader = 16; g.TotalNumberOfBits = 16 + 1152 + 32; g.oqpsk = 0; break;
    case 1200: g.N = 9; g.dl2_sz = 576 - 6 + 1; g.NumberOfBits = 1152; g.BitsInHeader = 16; g.TotalNumberOfBits = 16 + 1152 + 32; g.oqpsk = 0; break;
    default: g.N = 78; g.dl2_sz = 4992 - 6 + 1; g.NumberOfBits = 4992; g.BitsInHeader = 16 + 178; g.TotalNumberOfBits = 16 + 178 + 4992 + 64; g.oqpsk = 1; break;
    }
    g.blocksz = g.N * 64;
    g.burst = burst ? 1 : 0;
    if (burst)
    {
        // setSettings(fb, true) (aerol.cpp:996-1003,1062-1070): one second of bits as frame countdown; the block is the R/T packet
        // collector's (RTChannelDeleaveFECScram: up to 95 interleaver columns)
        g.TotalNumberOfBits = g.oqpsk ? fb : 3 * fb; // 1 s (10500 bps) / 3 s (600, 1200 bps) of bits
        g.blocksz = RT_BLOCKSZ;
    }
    g.idx_sat = (1000000000 - g.BitsInHeader) % g.blocksz;
    g.info_cap = g.NumberOfBits / 16 + 16;
    if (su_capacity <= 0) su_capacity = burst ? 256 : 32 * (g.NumberOfBits / 2 / 96) + 8; // 32 frames (burst: 256 packet rows) between reads
    g.su_cap = su_capacity; g.ev_cap = 256;
    DA(m, c->p.I, (size_t)AI_NFIELDS * g.nchp);
    DA(m, c->p.rx, (size_t)g.nchp * g.blocksz);
    DA(m, c->p.deint, (size_t)g.nchp * g.blocksz);
    DA(m, c->p.vbits, (size_t)g.nchp * (g.blocksz / 2));
    DA(m, c->p.overlap, (size_t)g.nchp * 64);
    DA(m, c->p.dl2, (size_t)g.nchp * g.dl2_sz);
    DA(m, c->p.info, (size_t)g.nchp * g.info_cap);
    DA(m, c->p.sus, (size_t)g.nchp * g.su_cap * 16);
    DA(m, c->p.events, (size_t)g.nchp * g.ev_cap * 3);
    uint8_t *d_scr = nullptr;
    DA(m, d_scr, 5000);
    unsigned *d_scrw = nullptr;
    DA(m, d_scrw, 5000 / 32 + 2);
    if (!burst && viterbi_use_lanes(g.nch, g.blocksz, 24))
    {
        // large bank: one block per lane in the Viterbi, tiled deinterleaver output, decoded bits and delay line packed 32 per word
        DA(m, c->d_vhist, viterbi_hist_bytes(g.nch) / sizeof(unsigned long long));
        g.packed = 1;
        // deinterleaver output: row-major.  The tiled layout ([wavefront][16-byte group][lane][16], k_viterbi_lanes reads 8 x 1 KiB per chunk)
        // was built when cold rows cost the decoder 0.85 ms; with its chunk prefetch it no longer gains anything and the tiled writes cost
        // 0.14 ms (3.51 vs 3.36 ms per step): not used (its switch left the library in round 3; the kernels keep the code path).
        g.tiled = 0;
        g.dl2_words = (g.dl2_sz + 31) / 32 + 1;
        DA(m, c->p.dl2w, (size_t)g.nchp * g.dl2_words);
    }
    // R/T packet search in a large bank: the trial decodes (each channel's own length) one block per lane as well, bits out one per byte
    if (burst && viterbi_use_lanes(g.nch, 128, 0)) DA(m, c->d_vhist, viterbi_hist_bytes(g.nch) / sizeof(unsigned long long));
    c->p.scr = d_scr;
    {
        HIPCHK(hipMemcpy(d_scr, scr.data(), 5000, hipMemcpyHostToDevice));
        std::vector<unsigned> scrw(5000 / 32 + 2, 0u);
        for (int k = 0; k < 5000; k++) scrw[k >> 5] |= (unsigned)scr[k] << (k & 31);
        HIPCHK(hipMemcpy(d_scrw, scrw.data(), scrw.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        c->p.scrw = d_scrw;
        // AeroL constructor state (aerol.cpp:904-977): cntr = 1000000000, blockcnt = -1, DataCarrierDetect(false) emitted
        std::vector<int> I((size_t)AI_NFIELDS * g.nchp, 0);
        std::vector<long long> ev((size_t)g.nchp * g.ev_cap * 3, 0);
        for (int ch = 0; ch < g.nchp; ch++)
        {
            I[(size_t)AI_CNTR * g.nchp + ch] = 1000000000;
            I[(size_t)AI_BLOCKCNT * g.nchp + ch] = -1;
            I[(size_t)AI_EV_CNT * g.nchp + ch] = 1; // row 0 = [0, DCD, 0]
        }
        if (burst)
            for (int ch = 0; ch < g.nchp; ch++)
            {
                I[(size_t)BI_RT_BLOCKPTR * g.nchp + ch] = 0;       // RTChannelDeleaveFECScram(): resetblockptr()
                I[(size_t)BI_RT_LAST * g.nchp + ch] = RT_NOTHING;
            }
        HIPCHK(hipMemcpy(c->p.I, I.data(), I.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->p.events, ev.data(), ev.size() * sizeof(long long), hipMemcpyHostToDevice));
    }
    HIPCHK(hipDeviceSynchronize());
    return 0;
}

static int aerol_create(int device, int nchannels, int fb, int max_softbits_per_write, int su_capacity, int burst, jaero_aerol_ctx **out)
{
    if (!out || nchannels <= 0 || max_softbits_per_write <= 0) return fail(JAERO_EINVAL, "jaero_aerol_create: bad arguments");
    *out = nullptr;
    if (fb != 600 && fb != 1200 && fb != 10500 && !(fb == 8400 && !burst))
        return fail(JAERO_ENOTSUP, "jaero_aerol_create: fb must be 600, 1200, 10500 or (continuous mode) 8400");
    int rc = open_device(device);
    if (rc) return rc;
    jaero_aerol_ctx *c = new jaero_aerol_ctx();
    c->device = device;
    rc = aerol_init(c, nchannels, fb, max_softbits_per_write, su_capacity, burst);
    if (rc) { jaero_aerol_destroy(c); return rc; }
    *out = c;
    return 0;
}

extern "C" int jaero_aerol_create(int device, int nchannels, int fb, int max_softbits_per_write, int su_capacity, jaero_aerol_ctx **out)
{
    return aerol_create(device, nchannels, fb, max_softbits_per_write, su_capacity, 0, out);
}
extern "C" int jaero_aerol_create_burst(int device, int nchannels, int fb, int max_softbits_per_write, int packet_row_capacity, jaero_aerol_ctx **out)
{
    return aerol_create(device, nchannels, fb, max_softbits_per_write, packet_row_capacity, 1, out);
}
// the C-channel pipeline's rounds of jaero_aerol_write
static int aerolc_write(jaero_aerol_ctx *c, const int16_t *dsoft, const int *dcounts, int stride, int max_count, hipStream_t st)
{
    const CGeom &g = c->cg;
    const CPtrs &p = c->cp;
    // a round finishes at most one frame per channel.  Frame ends are at least 4098 soft bits apart: the detector window reopens at
    // cntr > CC_FRAME - 112, so a (false or real) unique word can fire two bits after a completed frame and the next frame ends
    // CC_FRAME bits after that -- not CC_FRAME + 104 as in a clean stream.
    // A lane's round also ends when it meets a third jumpable stretch (k_aerolc_bits): it has then consumed at least one whole frame body
    // (CC_FRAME - 112 soft bits), so the bound below covers that too.
    const int rounds = max_count / (CC_FRAME - 112) + 2;
    const int *valid = p.I + (size_t)CI_HAS_BLOCK * g.nchp;
    const dim3 grid(g.nchp / 64), block(64);
    for (int r = 0; r < rounds; r++)
    {
        int pi = c->timer.begin(0, st);
        hipLaunchKernelGGL(k_aerolc_bits, grid, block, 0, st, g, p, dsoft, dcounts, stride);
        hipLaunchKernelGGL(k_aerolc_bulk, dim3((g.nch + 3) / 4), dim3(256), 0, st, g, p, dsoft, stride, -1, -1); // both stretches of a round, in order
        c->timer.end(pi, st);
        pi = c->timer.begin(1, st);
        // one block per wavefront for small banks, one per lane (k_viterbi_lanes) from 16 384 channels on, as the P-channel pipeline
        viterbi_launch(st, (const uint8_t *)p.dep, CC_NSOFT, (const uint8_t *)p.overlap, 24, p.vbits, CC_NSOFT / 2, 25, CC_NSOFT / 2, g.nch, valid,
                       c->d_vhist, 0, 0, 0, CC_PITCH);
        hipLaunchKernelGGL(k_viterbi_overlap_update, dim3(g.nch), dim3(64), 0, st, (const uint8_t *)p.dep, CC_NSOFT, p.overlap, g.nch, valid, 0, CC_PITCH);
        c->timer.end(pi, st);
        pi = c->timer.begin(2, st);
        hipLaunchKernelGGL(k_aerolc_post, grid, block, 0, st, g, p);
        c->timer.end(pi, st);
    }
    hipLaunchKernelGGL(k_aerolc_end_write, grid, block, 0, st, g, p, dcounts);
    HIPCHK(hipGetLastError());
    return 0;
}

// = processDemodulatedSoftBits for every channel: soft[ch * stride + k], k < counts[ch]
extern "C" int jaero_aerol_write(jaero_aerol_ctx *c, const int16_t *soft, const int *counts, int stride, int max_count, int is_device_ptr, void *stream)
{
    if (!c || !soft || !counts || stride <= 0 || max_count < 0 || max_count > stride) return fail(JAERO_EINVAL, "jaero_aerol_write: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (c->link && st != c->link->last_stream)
        return fail(JAERO_EINVAL, "jaero_aerol_write: a linked Aero-L bank writes on the stream of the bank's last jaero_write (nothing was consumed)");
    HIPCHK(hipSetDevice(c->device));
    c->last_stream = st;
    const AGeom &g = c->g;
    const int16_t *dsoft = soft;
    const int *dcounts = counts;
    if (!is_device_ptr)
    {
        if (stride > c->stage_stride) return fail(JAERO_EINVAL, "jaero_aerol_write: stride %d exceeds max_softbits_per_write %d", stride, c->stage_stride);
        for (int ch = 0; ch < g.nch; ch++) // a count above max_count would be cut short by the round budget, one above stride read past the row
            if (counts[ch] < 0 || counts[ch] > max_count) return fail(JAERO_EINVAL, "jaero_aerol_write: counts[%d] = %d outside [0, max_count = %d]", ch, counts[ch], max_count);
        HIPCHK(hipMemcpyAsync(c->d_soft, soft, sizeof(int16_t) * (size_t)g.nch * stride, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(c->d_counts, counts, sizeof(int) * g.nch, hipMemcpyHostToDevice, st));
        dsoft = c->d_soft; dcounts = c->d_counts;
    }
    if (max_count == 0) return 0;
    if (c->cchan)
    {
        const int rc = aerolc_write(c, dsoft, dcounts, stride, max_count, st);
        return rc ? rc : aerol_link_apply(c, st);
    }
    if (g.burst)
    {
        // R/T packet search: a round per trial length a channel can reach in this write (every 192 soft bits, plus 128 and 320)
        const int rounds = max_count / 192 + 4;
        const int *valid = c->p.I + (size_t)AI_HAS_BLOCK * g.nchp;
        const int *lens = c->p.I + (size_t)BI_TRIAL_LEN * g.nchp;
        const dim3 grid(g.nchp / 64), block(64);
        for (int r = 0; r < rounds; r++)
        {
            int pi = c->timer.begin(0, st);
            if (((((size_t)dsoft) | ((size_t)stride * 2)) & 15) == 0) hipLaunchKernelGGL(k_aerolb_bits<true>, grid, block, 0, st, g, c->p, dsoft, dcounts, stride);
            else hipLaunchKernelGGL(k_aerolb_bits<false>, grid, block, 0, st, g, c->p, dsoft, dcounts, stride);
            hipLaunchKernelGGL(k_aerolb_deint, dim3((g.nch + 3) / 4), dim3(256), 0, st, g, c->p);
            c->timer.end(pi, st);
            pi = c->timer.begin(1, st);
            // trial lengths are 128, 320, 512, .. (k_aerolb_bits): never below the lane layout's minimum of 4 * VT_ORDER steps
            viterbi_launch(st, (const uint8_t *)c->p.deint, RT_BLOCKSZ, (const uint8_t *)nullptr, 0, c->p.vbits, RT_BLOCKSZ / 2, 0, RT_BLOCKSZ / 2, g.nch, valid,
                           c->d_vhist, 0, 0, c->d_vhist != nullptr, 0, lens);
            c->timer.end(pi, st);
            pi = c->timer.begin(2, st);
            hipLaunchKernelGGL(k_aerolb_post, grid, block, 0, st, g, c->p);
            c->timer.end(pi, st);
            if (c->rt_on)
            {
                pi = c->timer.begin(5, st);
                hipLaunchKernelGGL(k_aerolb_isu, grid, block, 0, st, g, c->p, c->isu, c->rt);
                c->timer.end(pi, st);
            }
        }
        hipLaunchKernelGGL(k_aerol_end_write, grid, block, 0, st, g, c->p, dcounts);
        HIPCHK(hipGetLastError());
        return 0; // (a burst bank is never linked: jaero_aerol_link_dcd)
    }
    // every round finishes at most one interleaver block per channel (the reference completes a block -- Viterbi, descrambling,
    // CRC and its data-carrier-detect update -- before it looks at the next soft bit)
    const int rounds = max_count / g.blocksz + 2;
    const int *valid = c->p.I + (size_t)AI_HAS_BLOCK * g.nchp;
    const dim3 grid(g.nchp / 64), block(64);
    const bool bulk = g.oqpsk != 0; // 10.5 kbps: locked channels jump over the body of a frame (k_aerol_bits / k_aerol_bulk)
    if (bulk) hipLaunchKernelGGL(k_aerol_scan, dim3((g.nch + 3) / 4), dim3(256), 0, st, g, c->p, dsoft, dcounts, stride);
    for (int r = 0; r < rounds; r++)
    {
        int pi = c->timer.begin(0, st);
        if (bulk)
        {
            hipLaunchKernelGGL(k_aerol_bits<true>, grid, block, 0, st, g, c->p, dsoft, dcounts, stride);
            hipLaunchKernelGGL(k_aerol_bulk, dim3((g.nch + 3) / 4), dim3(256), 0, st, g, c->p, dsoft, stride);
        }
        else hipLaunchKernelGGL(k_aerol_bits<false>, grid, block, 0, st, g, c->p, dsoft, dcounts, stride);
        hipLaunchKernelGGL(k_aerol_deint, dim3((g.nch + 3) / 4), dim3(256), 0, st, g, c->p);
        c->timer.end(pi, st);
        pi = c->timer.begin(1, st);
        viterbi_launch(st, (const uint8_t *)c->p.deint, g.blocksz, (const uint8_t *)c->p.overlap, 24, c->p.vbits, g.blocksz / 2, 25, g.blocksz / 2,
                       g.nch, valid, c->d_vhist, g.tiled, g.packed /* bits out, 32 per word */, g.packed /* lane layout */);
        hipLaunchKernelGGL(k_viterbi_overlap_update, dim3(g.nch), dim3(64), 0, st, (const uint8_t *)c->p.deint, g.blocksz, c->p.overlap, g.nch, valid, g.tiled);
        c->timer.end(pi, st);
        pi = c->timer.begin(2, st);
        if (g.packed) hipLaunchKernelGGL(k_aerol_post_packed, grid, block, 0, st, g, c->p);
        else hipLaunchKernelGGL(k_aerol_post, grid, block, 0, st, g, c->p);
        c->timer.end(pi, st);
        if (c->isu_on)
        {
            pi = c->timer.begin(5, st);
            hipLaunchKernelGGL(k_aerol_isu, grid, block, 0, st, g, c->p, c->isu);
            c->timer.end(pi, st);
        }
    }
    hipLaunchKernelGGL(k_aerol_end_write, grid, block, 0, st, g, c->p, dcounts);
    HIPCHK(hipGetLastError());
    return aerol_link_apply(c, st);
}

// the readers of an Aero-L bank's per-channel outputs: drain channel ch of the rows whose count is column `cnt_field` of the bank's counters
// (the C channel's or the P / R/T banks'), then report `ovbit` of its overflow word
static int aerol_read(jaero_aerol_ctx *c, const char *who, int cnt_field, void *base, int cap, size_t rowbytes, int ch, void *rows, int caprows, int *nrows, int ovbit)
{
    int *I = c->cchan ? c->cp.I : c->p.I;
    const size_t nchp = c->g.nchp;
    const int rc = drain_rows(who, c->device, c->last_stream, c->g.nch, {base, I + cnt_field * nchp, cap, rowbytes}, ch, rows, caprows, nrows);
    return rc ? rc : report_overflow(I + (c->cchan ? CI_OVERFLOW : AI_OVERFLOW) * nchp + ch, ovbit, ch);
}
extern "C" int jaero_aerol_read_sus(jaero_aerol_ctx *c, int ch, int32_t *rows, int caprows, int *nrows)
{
    const char *who = "jaero_aerol_read_sus";
    if (!c) return fail(JAERO_EINVAL, "%s: null ctx", who);
    if (c->cchan) return aerol_read(c, who, CI_SU_CNT, c->cp.sus, c->cg.su_cap, 16 * sizeof(int32_t), ch, rows, caprows, nrows, 1);
    if (c->g.burst) return fail(JAERO_ENOTSUP, "jaero_aerol_read_sus: burst-mode bank (use jaero_aerol_read_packets)");
    return aerol_read(c, who, AI_SU_CNT, c->p.sus, c->g.su_cap, 16 * sizeof(int32_t), ch, rows, caprows, nrows, 1);
}
extern "C" int jaero_aerol_read_packets(jaero_aerol_ctx *c, int ch, int32_t *rows, int caprows, int *nrows)
{
    if (!c) return fail(JAERO_EINVAL, "jaero_aerol_read_packets: null ctx");
    if (!c->g.burst) return fail(JAERO_ENOTSUP, "jaero_aerol_read_packets: not a burst-mode bank (use jaero_aerol_read_sus)");
    return aerol_read(c, "jaero_aerol_read_packets", AI_SU_CNT, c->p.sus, c->g.su_cap, 16 * sizeof(int32_t), ch, rows, caprows, nrows, 1);
}
extern "C" int jaero_aerol_read_events(jaero_aerol_ctx *c, int ch, long long *rows, int caprows, int *nrows)
{
    const char *who = "jaero_aerol_read_events";
    if (!c) return fail(JAERO_EINVAL, "%s: null ctx", who);
    if (c->cchan) return aerol_read(c, who, CI_EV_CNT, c->cp.events, c->cg.ev_cap, 3 * sizeof(long long), ch, rows, caprows, nrows, 2);
    return aerol_read(c, who, AI_EV_CNT, c->p.events, c->g.ev_cap, 3 * sizeof(long long), ch, rows, caprows, nrows, 2);
}
extern "C" int jaero_aerol_read_voice(jaero_aerol_ctx *c, int ch, uint8_t *rows, int caprows, int *nrows)
{
    if (!c || !c->cchan) return fail(JAERO_EINVAL, "jaero_aerol_read_voice: not a C-channel (fb = 8400) bank");
    return aerol_read(c, "jaero_aerol_read_voice", CI_V_CNT, c->cp.voice, c->cg.v_cap, 304, ch, rows, caprows, nrows, 4);
}
// ------------------------------------------------------------------------------------------ ISU / SSU reassembly (k_aerol_isu.h)
static_assert(sizeof(jaero_aerol_msg) == ISU_ROW_BYTES && ISU_ROW_BYTES % 16 == 0, "a message row is what isu_emit writes and k_sweep_gather<16> moves");
// The message log of `msg_capacity` rows per channel, shared by both reassemblies (a bank has one of them): kept if it has that capacity, else
// allocated anew; `bytes` follows what is held.
static int aerol_msg_log(jaero_aerol_ctx *c, int msg_capacity, long long &bytes)
{
    const size_t nchp = c->g.nchp;
    if (c->isu.log && c->isu.msg_cap == msg_capacity) return 0;
    if (c->isu.log)
    {
        for (size_t k = 0; k < c->mem.ptrs.size(); k++) if (c->mem.ptrs[k] == (void *)c->isu.log) { c->mem.ptrs.erase(c->mem.ptrs.begin() + k); break; }
        hipFree(c->isu.log);
        bytes -= (long long)nchp * c->isu.msg_cap * ISU_ROW_BYTES;
        c->isu.log = nullptr; c->isu.msg_cap = 0;
    }
    if (const int rc = dalloc(c->mem, &c->isu.log, nchp * msg_capacity * ISU_ROW_BYTES, false)) return rc;
    c->isu.msg_cap = msg_capacity;
    bytes += (long long)nchp * msg_capacity * ISU_ROW_BYTES;
    return 0;
}
// Checks in the header's order, all before a device is touched.
extern "C" int jaero_aerol_isu_enable(jaero_aerol_ctx *c, int msg_capacity)
{
    const char *who = "jaero_aerol_isu_enable";
    if (!c) return fail(JAERO_EINVAL, "%s: null ctx", who);
    if (msg_capacity < 0) return fail(JAERO_EINVAL, "%s: msg_capacity < 0", who);
    if (c->g.burst) return fail(JAERO_ENOTSUP, "%s: burst-mode bank (the R / T channel reassembly, RISUData and the T packets' units, is jaero_aerol_rt_enable)", who);
    if (c->cchan) return fail(JAERO_ENOTSUP, "%s: fb = 8400 (AeroL::DecodeC never calls ISUData)", who);
    QUIESCE(c);
    if (msg_capacity == 0)
    {
        c->isu_on = false;
        c->p.isumark = nullptr; // the log, its counts and the counters stay where they are
        return 0;
    }
    const AGeom &g = c->g;
    int rc;
    if (!c->d_isumark)
    {
        DA(c->mem, c->d_isumark, g.nchp);
        DA(c->mem, c->isu.chan, (size_t)g.nchp * ISU_CHAN_WORDS);
        DA(c->mem, c->isu.items, (size_t)g.nchp * ISU_MAX_ITEMS * ISU_ITEM_BYTES);
        DA(c->mem, c->isu.msg_cnt, g.nchp);
        DA(c->mem, c->isu.stats, (size_t)g.nchp * 4);
        c->isu_bytes = (long long)g.nchp * (2 * sizeof(int) + 4 * ISU_CHAN_WORDS + ISU_MAX_ITEMS * ISU_ITEM_BYTES + 4 * sizeof(long long));
    }
    if ((rc = aerol_msg_log(c, msg_capacity, c->isu_bytes))) { c->isu_on = false; c->p.isumark = nullptr; return rc; }
    // an empty list, an empty log, counters at 0 and `a` zeroed; the messages' overflow bit cleared
    HIPCHK(hipMemset(c->d_isumark, 0, sizeof(int) * (size_t)g.nchp));
    HIPCHK(hipMemset(c->isu.chan, 0, sizeof(uint32_t) * (size_t)g.nchp * ISU_CHAN_WORDS));
    HIPCHK(hipMemset(c->isu.msg_cnt, 0, sizeof(int) * (size_t)g.nchp));
    HIPCHK(hipMemset(c->isu.stats, 0, sizeof(long long) * (size_t)g.nchp * 4));
    hipLaunchKernelGGL(k_aerol_isu_clear_overflow, dim3(g.nchp / 64), dim3(64), 0, c->last_stream, g, c->p);
    HIPCHK(hipGetLastError());
    QUIESCE(c);
    c->p.isumark = c->d_isumark;
    c->isu_on = true;
    return 0;
}
extern "C" int jaero_aerol_read_msgs(jaero_aerol_ctx *c, int ch, void *rows, int caprows, int *nrows)
{
    const char *who = "jaero_aerol_read_msgs";
    if (!c) return fail(JAERO_EINVAL, "%s: null ctx", who);
    const int rc = drain_rows(who, c->device, c->last_stream, c->g.nch, {c->isu.log, c->isu.msg_cnt, c->isu.msg_cap, ISU_ROW_BYTES}, ch, rows, caprows, nrows);
    return rc ? rc : report_overflow(c->p.I + (size_t)AI_OVERFLOW * c->g.nchp + ch, ISU_OVERFLOW_BIT, ch);
}
extern "C" int jaero_aerol_isu_stats(jaero_aerol_ctx *c, long long *stats)
{
    const char *who = "jaero_aerol_isu_stats";
    if (!c || !stats) return fail(JAERO_EINVAL, "%s: null ctx / stats", who);
    if (!c->isu.stats) return fail(JAERO_EINVAL, "%s: this bank never enabled the reassembly (jaero_aerol_isu_enable)", who);
    QUIESCE(c);
    HIPCHK(hipMemcpy(stats, c->isu.stats, sizeof(long long) * (size_t)c->g.nch * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------------------------------ R / T user data of a burst bank (k_aerolb_isu.h)
// an allocation of jaero_aerol_rt_enable: its size is counted where it is made (jaero_aerol_debug_extra_bytes)
template <class T>
static int rt_alloc(jaero_aerol_ctx *c, T *&ptr, size_t count)
{
    if (ptr) return 0; // the first enable's
    if (const int rc = dalloc(c->mem, &ptr, count)) return rc;
    c->rt_bytes += (long long)(count * sizeof(T));
    return 0;
}
// Checks in the header's order, all before a device is touched.
extern "C" int jaero_aerol_rt_enable(jaero_aerol_ctx *c, int msg_capacity)
{
    const char *who = "jaero_aerol_rt_enable";
    if (!c) return fail(JAERO_EINVAL, "%s: null ctx", who);
    if (msg_capacity < 0) return fail(JAERO_EINVAL, "%s: msg_capacity < 0", who);
    if (c->cchan || !c->g.burst) return fail(JAERO_ENOTSUP, "%s: not a burst-mode bank (a continuous P-channel bank has jaero_aerol_isu_enable)", who);
    QUIESCE(c);
    if (msg_capacity == 0)
    {
        c->rt_on = false;
        c->p.rtmark = nullptr; // the log, its counts and the counters stay where they are
        return 0;
    }
    const AGeom &g = c->g;
    const size_t nchp = g.nchp;
    int rc;
    if ((rc = rt_alloc(c, c->d_rtmark, nchp)) || (rc = rt_alloc(c, c->isu.chan, nchp * ISU_CHAN_WORDS)) ||
        (rc = rt_alloc(c, c->isu.items, nchp * ISU_MAX_ITEMS * ISU_ITEM_BYTES)) || (rc = rt_alloc(c, c->isu.msg_cnt, nchp)) ||
        (rc = rt_alloc(c, c->rt.chan, nchp * RISU_CHAN_WORDS)) || (rc = rt_alloc(c, c->rt.items, nchp * ISU_MAX_ITEMS * RISU_SLOT_BYTES)) ||
        (rc = rt_alloc(c, c->rt.stats, nchp * RT_NSTATS)))
        return rc;
    if ((rc = aerol_msg_log(c, msg_capacity, c->rt_bytes))) { c->rt_on = false; c->p.rtmark = nullptr; return rc; }
    // both lists empty, both scratch items zeroed, an empty log, counters at 0; the messages' overflow bit cleared
    HIPCHK(hipMemset(c->d_rtmark, 0, sizeof(long long) * nchp));
    HIPCHK(hipMemset(c->isu.chan, 0, sizeof(uint32_t) * nchp * ISU_CHAN_WORDS));
    HIPCHK(hipMemset(c->rt.chan, 0, sizeof(uint32_t) * nchp * RISU_CHAN_WORDS));
    HIPCHK(hipMemset(c->isu.msg_cnt, 0, sizeof(int) * nchp));
    HIPCHK(hipMemset(c->rt.stats, 0, sizeof(long long) * nchp * RT_NSTATS));
    hipLaunchKernelGGL(k_aerol_isu_clear_overflow, dim3(g.nchp / 64), dim3(64), 0, c->last_stream, g, c->p);
    HIPCHK(hipGetLastError());
    QUIESCE(c);
    c->p.rtmark = c->d_rtmark;
    c->rt_on = true;
    return 0;
}
extern "C" int jaero_aerol_rt_stats(jaero_aerol_ctx *c, long long *stats)
{
    const char *who = "jaero_aerol_rt_stats";
    if (!c || !stats) return fail(JAERO_EINVAL, "%s: null ctx / stats", who);
    if (!c->rt.stats) return fail(JAERO_EINVAL, "%s: this bank never enabled the reassembly (jaero_aerol_rt_enable)", who);
    QUIESCE(c);
    HIPCHK(hipMemcpy(stats, c->rt.stats, sizeof(long long) * (size_t)c->g.nch * RT_NSTATS, hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------------------------------ jaero_aerol_read_all
// test hook: bytes of device memory the link, the sweep and the reassembly have allocated for this bank so far (0 for a bank that used none)
extern "C" long long jaero_aerol_debug_extra_bytes(const jaero_aerol_ctx *c)
{
    if (!c) return -1;
    long long n = c->d_dcdmark ? (long long)sizeof(int) * c->g.nchp : 0;
    return n + c->sweep.bytes() + c->isu_bytes + c->rt_bytes;
}
extern "C" int jaero_aerol_read_all(jaero_aerol_ctx *c, int what, void *rows, int caprows, int *offsets, int *nchannels_taken, long long *rows_pending,
                                    unsigned char *overflowed)
{
    const char *who = "jaero_aerol_read_all";
    // (the message log is a class only of a bank that enabled the reassembly: with no such bank behind it, 4 is as unknown as it was before the class existed)
    if (what < JAERO_AEROL_SUS || what > JAERO_AEROL_MESSAGES || (what == JAERO_AEROL_MESSAGES && !(c && c->isu.log)))
        return fail(JAERO_EINVAL, "%s: what = %d is none of JAERO_AEROL_SUS / PACKETS / EVENTS / VOICE%s", who, what,
                    what == JAERO_AEROL_MESSAGES ? " (JAERO_AEROL_MESSAGES exists on a bank that has called jaero_aerol_isu_enable or jaero_aerol_rt_enable)" : " / MESSAGES");
    if (caprows < 0) return fail(JAERO_EINVAL, "%s: caprows < 0", who);
    if (!offsets || !nchannels_taken) return fail(JAERO_EINVAL, "%s: null offsets / nchannels_taken", who);
    if (!rows && caprows > 0) return fail(JAERO_EINVAL, "%s: null rows with caprows > 0", who);
    if (!c) return fail(JAERO_EINVAL, "%s: null ctx", who);
    const size_t nchp = c->g.nchp;
    int *I = c->cchan ? c->cp.I : c->p.I;
    int *ov = I + (size_t)(c->cchan ? CI_OVERFLOW : AI_OVERFLOW) * nchp;
    RowBuf b{};
    int ovbit = 0;
    switch (what)
    {
    case JAERO_AEROL_SUS:
        if (!c->cchan && c->g.burst) return fail(JAERO_ENOTSUP, "%s: burst-mode bank (use JAERO_AEROL_PACKETS)", who);
        b = c->cchan ? RowBuf{c->cp.sus, I + (size_t)CI_SU_CNT * nchp, c->cg.su_cap, 16 * sizeof(int32_t)} : RowBuf{c->p.sus, I + (size_t)AI_SU_CNT * nchp, c->g.su_cap, 16 * sizeof(int32_t)};
        ovbit = 1;
        break;
    case JAERO_AEROL_PACKETS:
        if (c->cchan || !c->g.burst) return fail(JAERO_ENOTSUP, "%s: not a burst-mode bank (use JAERO_AEROL_SUS)", who);
        b = RowBuf{c->p.sus, I + (size_t)AI_SU_CNT * nchp, c->g.su_cap, 16 * sizeof(int32_t)};
        ovbit = 1;
        break;
    case JAERO_AEROL_EVENTS:
        b = c->cchan ? RowBuf{c->cp.events, I + (size_t)CI_EV_CNT * nchp, c->cg.ev_cap, 3 * sizeof(long long)} : RowBuf{c->p.events, I + (size_t)AI_EV_CNT * nchp, c->g.ev_cap, 3 * sizeof(long long)};
        ovbit = 2;
        break;
    case JAERO_AEROL_MESSAGES: // (enabled at some time: checked with `what`)
        b = RowBuf{c->isu.log, c->isu.msg_cnt, c->isu.msg_cap, ISU_ROW_BYTES};
        ovbit = ISU_OVERFLOW_BIT;
        break;
    default:
        if (!c->cchan) return fail(JAERO_EINVAL, "%s: JAERO_AEROL_VOICE: not a C-channel (fb = 8400) bank", who);
        b = RowBuf{c->cp.voice, I + (size_t)CI_V_CNT * nchp, c->cg.v_cap, 304};
        ovbit = 4;
        break;
    }
    // one log of every channel in one call (sweep_host.h); the sweep's kernels are class 3 of the bank's timer
    return sweep_log({who, c->sweep, c->device, c->last_stream, c->mem, c->timer, 3, c->g.nch}, b, ov, ovbit, nullptr, rows, caprows, offsets, nchannels_taken,
                     rows_pending, overflowed);
}
#include "k_aerol_tick.h" // k_aerol_tick_dcd = AeroL::updateDCD (aerol.cpp:1109-1122)
extern "C" int jaero_aerol_tick_dcd(jaero_aerol_ctx *c, int *dcd_out_host)
{
    if (!c) return fail(JAERO_EINVAL, "null ctx");
    if (c->link && c->last_stream != c->link->last_stream)
        return fail(JAERO_EINVAL, "jaero_aerol_tick_dcd: the bank has written on another stream since this linked Aero-L bank's last write (nothing was ticked)");
    HIPCHK(hipSetDevice(c->device));
    int *dout = dcd_out_host ? c->d_counts : nullptr;
    if (c->cchan) hipLaunchKernelGGL(k_aerolc_tick_dcd, dim3(c->g.nchp / 64), dim3(64), 0, c->last_stream, c->cg, c->cp, dout);
    else hipLaunchKernelGGL(k_aerol_tick_dcd, dim3(c->g.nchp / 64), dim3(64), 0, c->last_stream, c->g, c->p, dout);
    { const int rc = aerol_link_apply(c, c->last_stream); if (rc) return rc; }
    if (dcd_out_host)
    {
        HIPCHK(hipMemcpyAsync(dcd_out_host, c->d_counts, sizeof(int) * c->g.nch, hipMemcpyDeviceToHost, c->last_stream));
        QUIESCE(c);
    }
    HIPCHK(hipGetLastError());
    return 0;
}
