// rate_host.h -- host side of the rate meter (k_rate.h; include/jaero_hip.h, "rate lines"; DESIGN 18, "Rate lines").
//
// One jaero_rate keeps, for nch rows of int16 PCM, the sums R [nch][2049] of the squared signal's windowed power spectrum over every
// completed 4096-sample segment.  State between writes: the pending partial segment ([nch][4096] int16, `fill` samples a row), the sums and
// the segment count.  A write that completes a segment launches k_rate_lines over (pending, write) and then stores the write's tail as the
// new pending segment; one that completes none appends to it.  Two pending buffers take turns, as the channeliser's history does: the
// tail is stored into the one the launch did not read.
//
// Gated rate lines (jaero_gate_*): the handle also keeps a gate per channel and four numbers per channel, and, once jaero_gate_enable has
// switched it over, a write launches k_rate_lines_gated in place of k_rate_lines.  Nothing else in a write differs; a handle that never
// enables the gate launches k_rate_lines alone, as before.
//
// One-pass gates (jaero_gate2_*): `mode` is 0, JAERO_GATE_MANUAL or JAERO_GATE_AUTO, with or without JAERO_GATE_HIST.  Mode 0 launches
// k_rate_lines and mode 1 k_rate_lines_gated, as before; every mode with AUTO or HIST launches k_rate_lines_auto, which also keeps e2 and
// start per channel (d_stats2), writes the gates under AUTO and counts the histogram (d_hist, allocated by the first mode with HIST).
//
// Rate lines, read on the device (jaero_lines_classify): k_rate_classify (k_rate_classify.h) reads R and leaves floor, score and where in
// three buffers of the handle that the first call allocates; the call changes nothing else of the handle.
#pragma once
#include "k_rate.h"
#include "k_rate_classify.h"

static_assert(RATE_L == JAERO_RATE_L && RATE_BINS == JAERO_RATE_BINS, "the kernel's segment and row are the ABI's");

struct jaero_rate : DevHandle
{
    int nch = 0, max_write = 0;
    DevMem mem;
    int16_t *d_pend[2] = {nullptr, nullptr}; // [nch][4096] each; d_pend[cur] holds `fill` samples a row
    int cur = 0, fill = 0;
    int16_t *d_in = nullptr;                 // [nch][max_write]: where a write from host memory is staged; allocated by the first one
    double2 *d_tw = nullptr;                 // [4096]: exp(-2 pi i k / 4096)
    double *d_R = nullptr;                   // [nch][2049]
    long long nseg = 0;
    int mode = 0;                            // jaero_gate2_enable: 0 k_rate_lines, JAERO_GATE_MANUAL k_rate_lines_gated, else k_rate_lines_auto
    unsigned long long *d_gate = nullptr;    // [nch]: the gates, 0 at create; every reset and switch keeps them
    unsigned long long *d_stats = nullptr;   // [nch][4]: emax, emin, njoin, ejoin over the segments since the last reset (gated only)
    unsigned long long *d_stats2 = nullptr;  // [nch][2]: e2, start (k_rate_lines_auto only)
    unsigned *d_hist = nullptr;              // [nch][321]: the histogram of E; allocated by the first enable with JAERO_GATE_HIST
    double *d_lfloor = nullptr;              // [nch], [nch][8], [nch][8]: jaero_lines_classify's results; allocated by the first call
    unsigned long long *d_lscore = nullptr;
    int *d_lwhere = nullptr;
    KernelTimer timer{1};                    // 0 k_rate_lines, k_rate_lines_gated or k_rate_lines_auto, whichever ran
};

extern "C" void jaero_rate_destroy(jaero_rate *r)
{
    if (!r) return;
    r->teardown();
    delete r;
}

// the four numbers with no segment yet: 0, 2^64 - 1, 0, 0; e2 and start: 0, 2^64 - 1; an empty histogram where there is one; and under
// AUTO every gate 0, the gate being a function of the numbers cleared here
static int rate_clear_stats(jaero_rate *r)
{
    std::vector<unsigned long long> st((size_t)r->nch * 4, 0ull);
    for (int c = 0; c < r->nch; c++) st[(size_t)c * 4 + 1] = ~0ull;
    HIPCHK(hipMemcpy(r->d_stats, st.data(), sizeof(unsigned long long) * st.size(), hipMemcpyHostToDevice));
    st.assign((size_t)r->nch * 2, 0ull);
    for (int c = 0; c < r->nch; c++) st[(size_t)c * 2 + 1] = ~0ull;
    HIPCHK(hipMemcpy(r->d_stats2, st.data(), sizeof(unsigned long long) * st.size(), hipMemcpyHostToDevice));
    if (r->d_hist) HIPCHK(hipMemset(r->d_hist, 0, sizeof(unsigned) * (size_t)r->nch * RATE_HBINS));
    if (r->mode & JAERO_GATE_AUTO) HIPCHK(hipMemset(r->d_gate, 0, sizeof(unsigned long long) * (size_t)r->nch));
    return 0;
}

static int rate_build(std::unique_ptr<jaero_rate> &r, int device, int nchannels, int max_write_samples)
{
    int rc = 0;
    r->device = device; r->nch = nchannels; r->max_write = max_write_samples;
    DA(r->mem, r->d_pend[0], (size_t)nchannels * RATE_L);
    DA(r->mem, r->d_pend[1], (size_t)nchannels * RATE_L);
    DA(r->mem, r->d_R, (size_t)nchannels * RATE_BINS);
    DA(r->mem, r->d_tw, RATE_L);
    std::vector<double2> tw(RATE_L); // rounded from long double, as the overlap-save filters' table is (fft4096_tables)
    for (int k = 0; k < RATE_L; k++)
    {
        const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)RATE_L;
        tw[k].x = (double)cosl(a); tw[k].y = (double)sinl(a);
    }
    HIPCHK(hipMemcpy(r->d_tw, tw.data(), sizeof(double2) * RATE_L, hipMemcpyHostToDevice));
    HIPCHK(hipFuncSetAttribute((const void *)k_rate_lines, hipFuncAttributeMaxDynamicSharedMemorySize, RATE_NC * RATE_L * (int)sizeof(double)));
    HIPCHK(hipFuncSetAttribute((const void *)k_rate_lines_gated, hipFuncAttributeMaxDynamicSharedMemorySize, RATE_NC * RATE_L * (int)sizeof(double)));
    HIPCHK(hipFuncSetAttribute((const void *)k_rate_lines_auto, hipFuncAttributeMaxDynamicSharedMemorySize, RATE_NC * RATE_L * (int)sizeof(double)));
    DA(r->mem, r->d_gate, nchannels);
    DA(r->mem, r->d_stats, (size_t)nchannels * 4);
    DA(r->mem, r->d_stats2, (size_t)nchannels * 2);
    return rate_clear_stats(r.get());
}

extern "C" int jaero_rate_create(int device, int nchannels, int max_write_samples, jaero_rate **out)
{
    if (!out) return fail(JAERO_EINVAL, "jaero_rate_create: out is null");
    *out = nullptr;
    if (nchannels < 1) return fail(JAERO_EINVAL, "jaero_rate_create: nchannels %d < 1", nchannels);
    if (max_write_samples < 1) return fail(JAERO_EINVAL, "jaero_rate_create: max_write_samples %d < 1", max_write_samples);
    { const int rc = open_device(device); if (rc) return rc; }
    std::unique_ptr<jaero_rate> r(new (std::nothrow) jaero_rate());
    if (!r) return fail(JAERO_ENOMEM, "jaero_rate_create: out of memory");
    const int rc = rate_build(r, device, nchannels, max_write_samples);
    if (rc) return rc;
    *out = r.release();
    return 0;
}

extern "C" int jaero_rate_write(jaero_rate *r, const int16_t *pcm, int nsamples, int is_device_ptr, void *stream, int *nseg_done)
{
    if (!r || !nseg_done || (nsamples > 0 && !pcm)) return fail(JAERO_EINVAL, "jaero_rate_write: null argument");
    if (nsamples < 0 || nsamples > r->max_write)
        return fail(JAERO_EINVAL, "jaero_rate_write: nsamples %d outside [0, max_write_samples = %d]", nsamples, r->max_write);
    POISONCHK(r, "jaero_rate_write", POISON_RATE);
    HIPCHK(hipSetDevice(r->device));
    hipStream_t st = (hipStream_t)stream;
    { const int rc = r->order_behind(st); if (rc) return rc; } // a write on another stream than the previous one waits for what was enqueued there
    *nseg_done = 0;
    if (nsamples == 0) return 0;
    const int n = nsamples, fill = r->fill;
    const int nseg = (int)(((long long)fill + n) / RATE_L), rest = (int)((long long)fill + n - (long long)nseg * RATE_L);
    const size_t row = sizeof(int16_t) * (size_t)n;
    const hipMemcpyKind kind = is_device_ptr ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (nseg == 0) // no segment completes: the write joins the pending one
    {
        PoisonGuard guard(*r);
        HIPCHK(hipMemcpy2DAsync(r->d_pend[r->cur] + fill, sizeof(int16_t) * RATE_L, pcm, row, row, (size_t)r->nch, kind, st));
        r->fill = fill + n;
        guard.commit();
        return 0;
    }
    const int16_t *src = pcm;
    if (!is_device_ptr)
    {
        if (!r->d_in) { const int rc = dalloc(r->mem, &r->d_in, (size_t)r->nch * r->max_write, false); if (rc) return rc; }
        HIPCHK(hipMemcpyAsync(r->d_in, pcm, row * (size_t)r->nch, hipMemcpyHostToDevice, st));
        src = r->d_in;
    }
    PoisonGuard guard(*r); // from here on the sums, the count and the pending segment advance together or not at all
    const int pi = r->timer.begin(0, st);
    if (r->mode & (JAERO_GATE_AUTO | JAERO_GATE_HIST))
    {
        hipLaunchKernelGGL(k_rate_lines_auto, dim3((unsigned)((r->nch + RATE_NC - 1) / RATE_NC)), dim3(RATE_THREADS), RATE_NC * RATE_L * sizeof(double), st,
                           (const int16_t *)r->d_pend[r->cur], fill, src, n, r->nch, nseg, (const double2 *)r->d_tw, r->d_R, r->d_gate, r->d_stats,
                           r->d_stats2, (r->mode & JAERO_GATE_HIST) ? r->d_hist : (unsigned *)nullptr, (r->mode & JAERO_GATE_AUTO) ? 1 : 0,
                           (unsigned long long)r->nseg);
        LAUNCHCHK("k_rate_lines_auto");
    }
    else if (r->mode == JAERO_GATE_MANUAL)
    {
        hipLaunchKernelGGL(k_rate_lines_gated, dim3((unsigned)((r->nch + RATE_NC - 1) / RATE_NC)), dim3(RATE_THREADS), RATE_NC * RATE_L * sizeof(double), st,
                           (const int16_t *)r->d_pend[r->cur], fill, src, n, r->nch, nseg, (const double2 *)r->d_tw, r->d_R,
                           (const unsigned long long *)r->d_gate, r->d_stats);
        LAUNCHCHK("k_rate_lines_gated");
    }
    else
    {
        hipLaunchKernelGGL(k_rate_lines, dim3((unsigned)((r->nch + RATE_NC - 1) / RATE_NC)), dim3(RATE_THREADS), RATE_NC * RATE_L * sizeof(double), st,
                           (const int16_t *)r->d_pend[r->cur], fill, src, n, r->nch, nseg, (const double2 *)r->d_tw, r->d_R);
        LAUNCHCHK("k_rate_lines");
    }
    r->timer.end(pi, st);
    // the tail behind the last completed segment lies wholly in this write (fill < 4096 <= 4096 nseg)
    if (rest > 0)
        HIPCHK(hipMemcpy2DAsync(r->d_pend[r->cur ^ 1], sizeof(int16_t) * RATE_L, src + (n - rest), row, sizeof(int16_t) * (size_t)rest,
                                (size_t)r->nch, hipMemcpyDeviceToDevice, st));
    r->cur ^= 1;
    r->fill = rest;
    r->nseg += nseg;
    HIPCHK(hipGetLastError());
    *nseg_done = nseg;
    guard.commit();
    return 0;
}

extern "C" int jaero_rate_reset(jaero_rate *r)
{
    if (!r) return fail(JAERO_EINVAL, "jaero_rate_reset: null handle");
    POISONCHK(r, "jaero_rate_reset", POISON_RATE);
    QUIESCE(r);
    HIPCHK(hipMemset(r->d_R, 0, sizeof(double) * (size_t)r->nch * RATE_BINS));
    r->nseg = 0; // the pending segment stays: the segment grid is absolute
    return r->mode ? rate_clear_stats(r) : 0; // off, the numbers are the empty ones already; the gates stay but under AUTO
}

// ---- gated rate lines (include/jaero_hip.h, "gated rate lines")
static int rate_set_mode(jaero_rate *r, int mode)
{
    QUIESCE(r);
    if ((mode & JAERO_GATE_HIST) && !r->d_hist)
    {
        const int rc = dalloc(r->mem, &r->d_hist, (size_t)r->nch * RATE_HBINS);
        if (rc) return rc;
    }
    HIPCHK(hipMemset(r->d_R, 0, sizeof(double) * (size_t)r->nch * RATE_BINS));
    r->nseg = 0; // as a reset: the pending segment stays, and so do the gates unless the new mode has AUTO
    r->mode = mode;
    return rate_clear_stats(r);
}

extern "C" int jaero_gate_enable(jaero_rate *r, int on)
{
    if (!r) return fail(JAERO_EINVAL, "jaero_gate_enable: null handle");
    POISONCHK(r, "jaero_gate_enable", POISON_RATE);
    return rate_set_mode(r, on ? JAERO_GATE_MANUAL : 0);
}

extern "C" int jaero_gate_set(jaero_rate *r, const unsigned long long *gate)
{
    if (!r || !gate) return fail(JAERO_EINVAL, "jaero_gate_set: null argument");
    POISONCHK(r, "jaero_gate_set", POISON_RATE);
    if (!r->mode) return fail(JAERO_EINVAL, "jaero_gate_set: the gate is off (jaero_gate_enable)");
    if (r->mode & JAERO_GATE_AUTO) return fail(JAERO_EINVAL, "jaero_gate_set: under JAERO_GATE_AUTO the device chooses the gates");
    QUIESCE(r); // the launches enqueued so far read the old gates
    HIPCHK(hipMemcpy(r->d_gate, gate, sizeof(unsigned long long) * (size_t)r->nch, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int jaero_gate_read(jaero_rate *r, unsigned long long *stats, unsigned long long *gate, long long *nseg)
{
    if (!r || !stats || !nseg) return fail(JAERO_EINVAL, "jaero_gate_read: null argument");
    POISONCHK(r, "jaero_gate_read", POISON_RATE);
    if (!r->mode) return fail(JAERO_EINVAL, "jaero_gate_read: the gate is off (jaero_gate_enable)");
    QUIESCE(r);
    HIPCHK(hipMemcpy(stats, r->d_stats, sizeof(unsigned long long) * (size_t)r->nch * 4, hipMemcpyDeviceToHost));
    if (gate) HIPCHK(hipMemcpy(gate, r->d_gate, sizeof(unsigned long long) * (size_t)r->nch, hipMemcpyDeviceToHost));
    *nseg = r->nseg;
    return 0;
}

// ---- one-pass gates (include/jaero_hip.h, "one-pass gates")
static_assert(RATE_HBINS == JAERO_GATE_HBINS, "the kernel's histogram row is the ABI's");

extern "C" int jaero_gate2_enable(jaero_rate *r, int mode)
{
    if (!r) return fail(JAERO_EINVAL, "jaero_gate2_enable: null handle");
    const int who = mode & ~JAERO_GATE_HIST; // HIST only together with MANUAL or AUTO, and never both of those
    if (mode != 0 && who != JAERO_GATE_MANUAL && who != JAERO_GATE_AUTO)
        return fail(JAERO_EINVAL, "jaero_gate2_enable: mode %d is none of 0, 1, 2, 1|4, 2|4", mode);
    POISONCHK(r, "jaero_gate2_enable", POISON_RATE);
    return rate_set_mode(r, mode);
}

extern "C" int jaero_gate2_read(jaero_rate *r, unsigned long long *stats, unsigned long long *gate, long long *nseg)
{
    if (!r || !stats || !nseg) return fail(JAERO_EINVAL, "jaero_gate2_read: null argument");
    POISONCHK(r, "jaero_gate2_read", POISON_RATE);
    if (!(r->mode & JAERO_GATE_AUTO)) return fail(JAERO_EINVAL, "jaero_gate2_read: the mode has no JAERO_GATE_AUTO (jaero_gate2_enable)");
    QUIESCE(r);
    const size_t w = sizeof(unsigned long long);
    HIPCHK(hipMemcpy2D(stats, 6 * w, r->d_stats, 4 * w, 4 * w, (size_t)r->nch, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy2D(stats + 4, 6 * w, r->d_stats2, 2 * w, 2 * w, (size_t)r->nch, hipMemcpyDeviceToHost));
    if (gate) HIPCHK(hipMemcpy(gate, r->d_gate, w * (size_t)r->nch, hipMemcpyDeviceToHost));
    *nseg = r->nseg;
    return 0;
}

extern "C" int jaero_gate2_read_hist(jaero_rate *r, unsigned *hist, long long *nseg)
{
    if (!r || !hist || !nseg) return fail(JAERO_EINVAL, "jaero_gate2_read_hist: null argument");
    POISONCHK(r, "jaero_gate2_read_hist", POISON_RATE);
    if (!(r->mode & JAERO_GATE_HIST)) return fail(JAERO_EINVAL, "jaero_gate2_read_hist: the mode has no JAERO_GATE_HIST (jaero_gate2_enable)");
    QUIESCE(r);
    HIPCHK(hipMemcpy(hist, r->d_hist, sizeof(unsigned) * (size_t)r->nch * RATE_HBINS, hipMemcpyDeviceToHost));
    *nseg = r->nseg;
    return 0;
}

extern "C" int jaero_rate_read(jaero_rate *r, double *sums, long long *nseg)
{
    if (!r || !sums || !nseg) return fail(JAERO_EINVAL, "jaero_rate_read: null argument");
    POISONCHK(r, "jaero_rate_read", POISON_RATE);
    QUIESCE(r);
    HIPCHK(hipMemcpy(sums, r->d_R, sizeof(double) * (size_t)r->nch * RATE_BINS, hipMemcpyDeviceToHost));
    *nseg = r->nseg;
    return 0;
}

extern "C" int jaero_rate_profile_enable(jaero_rate *r, int on)
{
    if (!r) return fail(JAERO_EINVAL, "jaero_rate_profile_enable: null handle");
    r->timer.on = on != 0;
    return 0;
}

extern "C" int jaero_rate_profile_read(jaero_rate *r, int which, double *total_ms, int *launches, int reset)
{
    if (!r || which != 0) return fail(JAERO_EINVAL, "jaero_rate_profile_read: bad arguments");
    return r->timer.read(r->device, which, total_ms, launches, reset);
}

// ---- rate lines, read on the device (include/jaero_hip.h, "rate lines, read on the device")
extern "C" int jaero_lines_classify(jaero_rate *r, int kmin, int nd, const int *d, double *floor, double *score, int *where, long long *nseg,
                                    double *kernel_ms)
{
    if (!r) return fail(JAERO_EINVAL, "jaero_lines_classify: null handle");
    if (!d) return fail(JAERO_EINVAL, "jaero_lines_classify: d is null");
    if (!floor) return fail(JAERO_EINVAL, "jaero_lines_classify: floor is null");
    if (!score) return fail(JAERO_EINVAL, "jaero_lines_classify: score is null");
    if (!where) return fail(JAERO_EINVAL, "jaero_lines_classify: where is null");
    if (!nseg) return fail(JAERO_EINVAL, "jaero_lines_classify: nseg is null");
    if (nd < 1 || nd > RCL_MAXD) return fail(JAERO_EINVAL, "jaero_lines_classify: nd %d outside 1 .. %d", nd, RCL_MAXD);
    rcl_dist dd = {};
    for (int i = 0; i < nd; i++)
    {
        if (d[i] < 1) return fail(JAERO_EINVAL, "jaero_lines_classify: d[%d] = %d < 1", i, d[i]);
        dd.d[i] = d[i];
    }
    if (kmin < 1 || kmin > RATE_BINS - 2) return fail(JAERO_EINVAL, "jaero_lines_classify: kmin %d outside 1 .. %d", kmin, RATE_BINS - 2);
    POISONCHK(r, "jaero_lines_classify", POISON_RATE);
    QUIESCE(r);
    if (!r->d_lwhere)
    {
        int rc = 0;
        if (!r->d_lfloor) DA(r->mem, r->d_lfloor, r->nch);
        if (!r->d_lscore) DA(r->mem, r->d_lscore, (size_t)r->nch * RCL_MAXD);
        DA(r->mem, r->d_lwhere, (size_t)r->nch * RCL_MAXD);
    }
    hipStream_t st = r->last_stream;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (kernel_ms)
    {
        HIPCHK(hipEventCreate(&ev[0]));
        const hipError_t e = hipEventCreate(&ev[1]);
        if (e != hipSuccess) { (void)hipEventDestroy(ev[0]); HIPCHK(e); }
        (void)hipEventRecord(ev[0], st);
    }
    hipLaunchKernelGGL(k_rate_classify, dim3((unsigned)((r->nch + RCL_NC - 1) / RCL_NC)), dim3(RCL_THREADS), 0, st,
                       (const unsigned long long *)r->d_R, r->nch, kmin, nd, dd, r->d_lfloor, r->d_lscore, r->d_lwhere);
    hipError_t e = hipGetLastError();
    if (kernel_ms) (void)hipEventRecord(ev[1], st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    float ms = 0.0f;
    if (kernel_ms)
    {
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
        (void)hipEventDestroy(ev[0]);
        (void)hipEventDestroy(ev[1]);
    }
    if (e != hipSuccess) return fail(JAERO_EHIP, "jaero_lines_classify: k_rate_classify failed: %s", hipGetErrorString(e));
    HIPCHK(hipMemcpy(floor, r->d_lfloor, sizeof(double) * (size_t)r->nch, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(score, r->d_lscore, sizeof(double) * (size_t)r->nch * nd, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(where, r->d_lwhere, sizeof(int) * (size_t)r->nch * nd, hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = (double)ms;
    *nseg = r->nseg;
    return 0;
}

extern "C" int jaero_debug_rate_poke(jaero_rate *r, const double *sums, long long nseg)
{
    if (!r || !sums) return fail(JAERO_EINVAL, "jaero_debug_rate_poke: null argument");
    if (nseg < 0) return fail(JAERO_EINVAL, "jaero_debug_rate_poke: nseg %lld < 0", nseg);
    POISONCHK(r, "jaero_debug_rate_poke", POISON_RATE);
    QUIESCE(r);
    HIPCHK(hipMemcpy(r->d_R, sums, sizeof(double) * (size_t)r->nch * RATE_BINS, hipMemcpyHostToDevice));
    r->nseg = nseg;
    return 0;
}
