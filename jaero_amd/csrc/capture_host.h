// capture_host.h -- host side of the channeliser's capture front end (k_chan_capture.h; jaero_chan3_*, DESIGN 18 "Capture front end").
//
// A capture's front end is a ChanFront whose input history is fp64 (ChanCapture::d_z, used exactly as d_in is: previous hop, then what waits;
// the tail of one buffer becomes the head of the other behind every write that completed a block) and is filled by k_capture_stage from
// the raw samples.  The raw history is the last K - 1 pairs in the raw format (two buffers as well: a write shorter than K - 1 would
// otherwise copy onto itself).  The counts T (capture samples taken) and m (staged samples made) live here, as 64-bit integers; every
// quotient and remainder the kernel needs is formed from them here.  Behind the staging everything is the channeliser's own: synthesis,
// survey, retune, pcm_view, feed.
#pragma once

static long long cap_gcd(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }
static long long cap_ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// What jaero_chan3_create checks of the capture against Fs_c, in its documented order, before jaero_chan2_create's own checks (who: the
// create the messages name).  rates: Fs_c is a rate at all (>= 1); where it is not, the later checks say so.  Leaves L / Mr and `resample`.
static int capture_check(const char *who, const jaero_capture *cap, bool rates, long long fs_c, long long *Lo, long long *Mro, bool *resample)
{
    if (!cap) return fail(JAERO_EINVAL, "%s: cap is null", who);
    if (cap->format != JAERO_IQ_CS16 && cap->format != JAERO_IQ_CU8 && cap->format != JAERO_IQ_CS8 && cap->format != JAERO_IQ_CF32)
        return fail(JAERO_EINVAL, "%s: format %d is not one of JAERO_IQ_*", who, cap->format);
    if (cap->fs_in < 1) return fail(JAERO_EINVAL, "%s: fs_in %d < 1", who, cap->fs_in);
    long long L = 1, Mr = 1;
    if (rates)
    {
        const long long g = cap_gcd(fs_c, cap->fs_in);
        L = fs_c / g; Mr = cap->fs_in / g;
        if (L > 1024) return fail(JAERO_EINVAL, "%s: fs_in %d to Fs_c %lld is %lld / %lld in lowest terms; L above 1024", who, cap->fs_in, fs_c, L, Mr);
        if ((long long)cap->fs_in > 8 * fs_c || fs_c > 8ll * cap->fs_in)
            return fail(JAERO_EINVAL, "%s: the ratio of fs_in %d and Fs_c %lld is beyond 8", who, cap->fs_in, fs_c);
    }
    *resample = L != 1 || Mr != 1;
    if (*resample)
    {
        if (cap->taps_per_phase < 1 || cap->taps_per_phase > CAP_MAXK)
            return fail(JAERO_EINVAL, "%s: taps_per_phase %d outside [1, %d]", who, cap->taps_per_phase, CAP_MAXK);
        if (!cap->rtaps) return fail(JAERO_EINVAL, "%s: rtaps is null and the rates differ", who);
        for (long long i = 0; i < L * cap->taps_per_phase; i++)
            if (!__builtin_isfinite(cap->rtaps[i])) return fail(JAERO_EINVAL, "%s: resampler tap %lld is not finite", who, i);
    }
    *Lo = L; *Mro = Mr;
    return 0;
}

// and behind them: the most staged samples a write can make (max_write_iq >= 1 by now), which the history must hold below 2^31
static int capture_check_staged(const char *who, int max_write_iq, long long L, long long Mr, long long *smax)
{
    *smax = cap_ceil_div((long long)max_write_iq * L, Mr);
    if (*smax + 1 + 2 * CHAN_HP > 0x7fffffffll)
        return fail(JAERO_EINVAL, "%s: max_write_iq %d stages %lld samples a write; the history holds fewer than 2^31", who, max_write_iq, *smax);
    return 0;
}

// The capture's half of a front end, behind chan_build_front: the raw and the fp64 histories and the resampler's phases.
static int capture_build(ChanFront *c, const jaero_capture *cap, long long L, long long Mr, bool resample, int max_write_iq, long long smax)
{
    int rc = 0;
    c->cap.reset(new (std::nothrow) ChanCapture());
    if (!c->cap) return fail(JAERO_ENOMEM, "jaero_chan3_create: out of memory");
    ChanCapture &k = *c->cap;
    k.format = cap->format; k.fs_in = cap->fs_in; k.shift = cap->shift; k.resample = resample;
    k.L = (int)L; k.Mr = (int)Mr; k.K = resample ? cap->taps_per_phase : 1;
    k.bps = cap->format == JAERO_IQ_CS16 ? 4 : cap->format == JAERO_IQ_CF32 ? 8 : 2;
    const size_t nraw = (size_t)(k.K - 1) + (size_t)max_write_iq;
    DA(c->mem, k.d_raw[0], nraw * k.bps);
    DA(c->mem, k.d_raw[1], nraw * k.bps);
    const size_t nz = 2 * (size_t)CHAN_HP + (size_t)smax + 1;
    DA(c->mem, k.d_z[0], nz);
    DA(c->mem, k.d_z[1], nz);
    if (resample)
    {
        std::vector<double> hp((size_t)k.L * k.K);
        for (int phi = 0; phi < k.L; phi++)
            for (int j = 0; j < k.K; j++) hp[(size_t)phi * k.K + j] = cap->rtaps[phi + (size_t)j * k.L];
        DA(c->mem, k.d_hp, hp.size());
        HIPCHK(hipMemcpy(k.d_hp, hp.data(), sizeof(double) * hp.size(), hipMemcpyHostToDevice));
    }
    HIPCHK(hipFuncSetAttribute((const void *)k_capture_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, C6_XCH * (int)sizeof(double)));
    return 0;
}

extern "C" int jaero_chan3_create(int device, const jaero_capture *cap, int decim, int out_rate, int nchannels, const jaero_chan_channel *ch,
                                  const double *taps, int ntaps, int max_write_iq, jaero_chan **out)
{
    if (!out) return fail(JAERO_EINVAL, "jaero_chan3_create: out is null");
    *out = nullptr;
    // the rate checks need Fs_c = out_rate x decim; where that is no rate at all, jaero_chan2_create's own checks below say so
    long long L = 1, Mr = 1, smax = 0;
    bool resample = false;
    { const int rc = capture_check("jaero_chan3_create", cap, out_rate >= 1 && decim >= 1, (long long)out_rate * decim, &L, &Mr, &resample); if (rc) return rc; }
    { const int rc = chan_check_create("jaero_chan2_create", decim, out_rate, nchannels, ch, taps, ntaps, max_write_iq); if (rc) return rc; }
    { const int rc = capture_check_staged("jaero_chan3_create", max_write_iq, L, Mr, &smax); if (rc) return rc; }
    { const int rc = open_device(device); if (rc) return rc; }

    std::unique_ptr<jaero_chan> c(new (std::nothrow) jaero_chan());
    if (!c) return fail(JAERO_ENOMEM, "jaero_chan3_create: out of memory");
    int rc = chan_build(c, device, decim, out_rate, nchannels, ch, taps, ntaps, max_write_iq, smax);
    if (rc) return rc;
    if ((rc = capture_build(c->own.get(), cap, L, Mr, resample, max_write_iq, smax))) return rc;
    *out = c.release();
    return 0;
}

template <int FMT, bool MIX>
static void capture_launch_fmt(const ChanCapture &k, const void *raw, long long nraw0, int nraw, long long q0, int r0, double2 *out, int nout, hipStream_t st)
{
    if (k.resample)
        hipLaunchKernelGGL((k_capture_stage<FMT, MIX, true>), dim3((unsigned)((nout + CAP_RUN - 1) / CAP_RUN)), dim3(CAP_THREADS), 0, st, raw, nraw0,
                           nraw, k.shift, (const double *)k.d_hp, k.L, k.Mr, k.K, q0, r0, out, nout);
    else
        hipLaunchKernelGGL((k_capture_stage<FMT, MIX, false>), dim3((unsigned)((nout + CAP_THREADS - 1) / CAP_THREADS)), dim3(CAP_THREADS), 0, st, raw,
                           nraw0, nraw, k.shift, (const double *)nullptr, 1, 1, 1, q0, r0, out, nout);
}

static void capture_launch(const ChanCapture &k, const void *raw, long long nraw0, int nraw, long long q0, int r0, double2 *out, int nout, hipStream_t st)
{
    auto go = [&](auto fmt) {
        constexpr int F = decltype(fmt)::value;
        if (k.shift) capture_launch_fmt<F, true>(k, raw, nraw0, nraw, q0, r0, out, nout, st);
        else capture_launch_fmt<F, false>(k, raw, nraw0, nraw, q0, r0, out, nout, st);
    };
    if (k.format == JAERO_IQ_CS16) go(std::integral_constant<int, JAERO_IQ_CS16>());
    else if (k.format == JAERO_IQ_CU8) go(std::integral_constant<int, JAERO_IQ_CU8>());
    else if (k.format == JAERO_IQ_CS8) go(std::integral_constant<int, JAERO_IQ_CS8>());
    else go(std::integral_constant<int, JAERO_IQ_CF32>());
}

// chan_write for a capture's front end: the raw copy, the staging kernel, then the channeliser's own kernels over the fp64 history
static int capture_write(ChanFront *c, const void *iq, int niq, int is_device_ptr, void *stream, int *nout, const char *who)
{
    hipStream_t st = (hipStream_t)stream;
    { const int rc = chan_write_enter(c, iq, niq, st, nout, who); if (rc) return rc; }
    ChanCapture &k = *c->cap;
    if (niq == 0) return 0;
    // every count of this write, before the first copy or launch
    const int hist = k.K - 1;
    const long long T1 = k.T + niq;
    const long long m1 = cap_ceil_div(T1 * k.L, k.Mr);          // z[m] exists once n_m <= T1 - 1
    const int nst = (int)(m1 - k.m);                            // <= ceil(niq L / Mr) <= smax
    const long long q0 = (k.m * k.Mr) / k.L;                    // n of the first staged sample: >= T, so the kernel reads [T - (K - 1), T1)
    const int r0 = (int)((k.m * k.Mr) % k.L);
    const int total = c->pending + nst;
    const int nblk = total / CHAN_HP;
    if (nst < 0 || nblk > c->nblk_max || (nst > 0 && (q0 < k.T || q0 + ((long long)r0 + (long long)(nst - 1) * k.Mr) / k.L > T1 - 1)))
        return fail(JAERO_EHIP, "%s: the staging counts do not add up (T %lld, m %lld, niq %d)", who, k.T, k.m, niq);

    char *raw = k.d_raw[k.rcur];
    HIPCHK(hipMemcpyAsync(raw + (size_t)hist * k.bps, iq, (size_t)k.bps * (size_t)niq, is_device_ptr ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    PoisonGuard guard(*c); // from here on the histories, the counts and the device buffers advance together or not at all
    double2 *z = k.d_z[c->cur];
    double2 *dst = z + CHAN_HP + c->pending;
    if (nst > 0)
    {
        const int pi = c->timer.begin(4, st);
        capture_launch(k, raw, k.T - hist, hist + niq, q0, r0, dst, nst, st);
        LAUNCHCHK("k_capture_stage");
        c->timer.end(pi, st);
    }
    if (hist > 0) // the last K - 1 raw pairs become the other buffer's head
    {
        HIPCHK(hipMemcpyAsync(k.d_raw[k.rcur ^ 1], raw + (size_t)niq * k.bps, (size_t)hist * k.bps, hipMemcpyDeviceToDevice, st));
        k.rcur ^= 1;
    }
    k.last_ptr = dst; k.last_n = nst; k.last_first = k.m;
    k.T = T1; k.m = m1;
    c->pending = total;
    if (nblk > 0)
    {
        const int pi = c->timer.begin(5, st);
        hipLaunchKernelGGL(k_capture_fwd, dim3(nblk), dim3(C2_THREADS), C6_XCH * sizeof(double), st, (const double2 *)z, c->d_spec, (const double2 *)c->d_tw);
        LAUNCHCHK("k_capture_fwd");
        c->timer.end(pi, st);
        { const int rc = chan_after_fwd(c, nblk, total, z, k.d_z[c->cur ^ 1], sizeof(double2), st); if (rc) return rc; }
    }
    return chan_write_leave(c, nblk, nout, guard);
}

extern "C" int jaero_chan3_write(jaero_chan *c, const void *iq, int niq, int is_device_ptr, void *stream, int *nout)
{
    if (!c || !nout || niq < 0 || (niq > 0 && !iq)) return fail(JAERO_EINVAL, "jaero_chan3_write: bad arguments");
    CHANVIEWCHK(c, "jaero_chan3_write", "jaero_split_write");
    if (!c->own->cap) return jaero_chan_write(c, (const int16_t *)iq, niq, is_device_ptr, stream, nout);
    return capture_write(c->own.get(), iq, niq, is_device_ptr, stream, nout, "jaero_chan3_write");
}

extern "C" int jaero_chan3_feed(jaero_chan *c, jaero_ctx *bank, const void *iq, int niq, int is_device_ptr, void *stream, int *nout)
{
    if (!c || !bank || !nout) return fail(JAERO_EINVAL, "jaero_chan3_feed: null argument");
    CHANVIEWCHK(c, "jaero_chan3_feed", "jaero_split_feed");
    if (!c->own->cap) return jaero_chan_feed(c, bank, (const int16_t *)iq, niq, is_device_ptr, stream, nout);
    const int rc0 = chan_feed_check(c, bank, "jaero_chan3_feed");
    if (rc0) return rc0;
    const int rc = capture_write(c->own.get(), iq, niq, is_device_ptr, stream, nout, "jaero_chan3_feed");
    if (rc || *nout <= 0) return rc;
    return jaero_write(bank, c->d_pcm, *nout, JAERO_PCM_CHANNEL_MAJOR, 1, stream);
}

// What the last write staged, on the host: npairs (re, im) pairs, the first of which is z[first_index].  A reader: nothing advances.
extern "C" int jaero_chan3_read_staged(jaero_chan *c, double *reim, int cap_pairs, int *npairs, long long *first_index)
{
    if (!c || !npairs || !first_index || cap_pairs < 0 || (cap_pairs > 0 && !reim)) return fail(JAERO_EINVAL, "jaero_chan3_read_staged: bad arguments");
    CHANVIEWCHK(c, "jaero_chan3_read_staged", "a stand-alone handle (a splitter has no jaero_chan3_read_staged)");
    if (!c->own->cap) return fail(JAERO_EINVAL, "jaero_chan3_read_staged: the handle has no capture front end (jaero_chan3_create)");
    POISONCHK(c->front, "jaero_chan3_read_staged", POISON_CHAN);
    const ChanCapture &k = *c->own->cap;
    if (cap_pairs < k.last_n) return fail(JAERO_EINVAL, "jaero_chan3_read_staged: cap_pairs %d is below the last write's %d staged samples", cap_pairs, k.last_n);
    QUIESCE(c->front);
    *npairs = k.last_n;
    *first_index = k.last_first;
    if (k.last_n > 0) HIPCHK(hipMemcpy(reim, k.last_ptr, sizeof(double2) * (size_t)k.last_n, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int jaero_chan3_profile_read(jaero_chan *c, int which, double *total_ms, int *launches, int reset)
{
    if (!c || which < 0 || which > 1) return fail(JAERO_EINVAL, "jaero_chan3_profile_read: bad arguments");
    return chan_timer_read(c, 4 + which, total_ms, launches, reset);
}
