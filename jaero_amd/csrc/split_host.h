// split_host.h -- host side of the channeliser's splitter (jaero_split_*, DESIGN 18 "Splitter"): one front end, any number of outputs.
//
// A jaero_split owns one ChanFront (built by chan_build_front, and capture_build with a capture) and one view per output: a jaero_chan built
// by chan_build_out that owns no front end and reads the splitter's d_spec.  A write is the front end's own write (chan_write / capture_write),
// which runs every output's kernels behind the forward transform (chan_after_fwd), each with the (nch, nblk, p0) the view's stand-alone twin
// would launch with.  No kernel is new and none is launched with other arguments than a stand-alone handle's: that is what makes a view's
// output its twin's bit for bit.  Everything is enqueued on the one stream of the write, so the next write's forward transform, which
// overwrites d_spec, runs behind every view's launches.
#pragma once

struct jaero_split
{
    int fs_c = 0;
    ChanFront front;
    std::vector<std::unique_ptr<jaero_chan>> views;
};

extern "C" void jaero_split_destroy(jaero_split *s)
{
    if (!s) return;
    s->front.teardown();
    delete s;
}

extern "C" int jaero_split_create(int device, const jaero_capture *cap, int fs_c, int noutputs, const jaero_chan_output *outs, int max_write_iq,
                                  jaero_split **out)
{
    if (!out) return fail(JAERO_EINVAL, "jaero_split_create: out is null");
    *out = nullptr;
    if (!outs) return fail(JAERO_EINVAL, "jaero_split_create: outs is null");
    if (noutputs < 1 || noutputs > 8) return fail(JAERO_EINVAL, "jaero_split_create: noutputs %d outside [1, 8]", noutputs);
    if (fs_c < 1) return fail(JAERO_EINVAL, "jaero_split_create: fs_c %d < 1", fs_c);
    for (int g = 0; g < noutputs; g++)
    {
        const jaero_chan_output &o = outs[g];
        if (o.out_rate != 48000 && o.out_rate != 24000 && o.out_rate != 12000)
            return fail(JAERO_EINVAL, "jaero_split_create: output %d: out_rate %d is not 48000, 24000 or 12000", g, o.out_rate);
        const int D = fs_c / o.out_rate;
        if (fs_c % o.out_rate != 0 || (D != 16 && D != 32 && D != 64 && D != 128 && D != 256))
            return fail(JAERO_EINVAL, "jaero_split_create: output %d: fs_c %d / out_rate %d is not exactly 16, 32, 64, 128 or 256", g, fs_c, o.out_rate);
        char who[48];
        snprintf(who, sizeof who, "jaero_split_create: output %d", g);
        const int rc = chan_check_create(who, D, o.out_rate, o.nchannels, o.ch, o.taps, o.ntaps, max_write_iq);
        if (rc) return rc;
    }
    long long L = 1, Mr = 1, smax = 0;
    bool resample = false;
    if (cap)
    {
        { const int rc = capture_check("jaero_split_create", cap, true, fs_c, &L, &Mr, &resample); if (rc) return rc; }
        { const int rc = capture_check_staged("jaero_split_create", max_write_iq, L, Mr, &smax); if (rc) return rc; }
    }
    { const int rc = open_device(device); if (rc) return rc; }

    // (a failure below frees what was built: the views and the front end go with s)
    std::unique_ptr<jaero_split> s(new (std::nothrow) jaero_split());
    if (!s) return fail(JAERO_ENOMEM, "jaero_split_create: out of memory");
    s->fs_c = fs_c;
    ChanFront *f = &s->front;
    int rc = chan_build_front(f, device, max_write_iq, smax);
    if (rc) return rc;
    if (cap && (rc = capture_build(f, cap, L, Mr, resample, max_write_iq, smax))) return rc;
    for (int g = 0; g < noutputs; g++)
    {
        const jaero_chan_output &o = outs[g];
        s->views.emplace_back(new (std::nothrow) jaero_chan());
        if (!s->views.back()) return fail(JAERO_ENOMEM, "jaero_split_create: out of memory");
        if ((rc = chan_build_out(s->views.back().get(), f, fs_c / o.out_rate, o.out_rate, o.nchannels, o.ch, o.taps, o.ntaps))) return rc;
    }
    *out = s.release();
    return 0;
}

// the write both entry points share; nout: one entry per output.  Refused: nothing advanced; failed part-way: the front end is poisoned, and
// with it every view
static int split_write(jaero_split *s, const void *iq, int niq, int is_device_ptr, void *stream, int *nout, const char *who)
{
    if (niq < 0 || (niq > 0 && !iq)) return fail(JAERO_EINVAL, "%s: bad arguments", who);
    ChanFront *f = &s->front;
    POISONCHK(f, who, POISON_SPLIT);
    return f->cap ? capture_write(f, iq, niq, is_device_ptr, stream, nout, who) : chan_write(f, (const int16_t *)iq, niq, is_device_ptr, stream, nout, who);
}

extern "C" int jaero_split_write(jaero_split *s, const void *iq, int niq, int is_device_ptr, void *stream, int *nout)
{
    if (!s || !nout) return fail(JAERO_EINVAL, "jaero_split_write: null argument");
    return split_write(s, iq, niq, is_device_ptr, stream, nout, "jaero_split_write");
}

extern "C" int jaero_split_feed(jaero_split *s, jaero_ctx *const *banks, const void *iq, int niq, int is_device_ptr, void *stream, int *nout)
{
    if (!s || !banks || !nout) return fail(JAERO_EINVAL, "jaero_split_feed: null argument");
    const int n = (int)s->views.size();
    for (int g = 0; g < n; g++)
    {
        if (!banks[g]) continue;
        { const int rc = chan_feed_check(s->views[g].get(), banks[g], "jaero_split_feed"); if (rc) return rc; }
        for (int h = 0; h < g; h++)
            if (banks[h] == banks[g]) return fail(JAERO_EINVAL, "jaero_split_feed: outputs %d and %d name the same bank", h, g);
    }
    int rc = split_write(s, iq, niq, is_device_ptr, stream, nout, "jaero_split_feed");
    if (rc) return rc;
    for (int g = 0; g < n; g++)
    {
        if (!banks[g] || nout[g] <= 0) continue;
        if ((rc = jaero_write(banks[g], s->views[g]->d_pcm, nout[g], JAERO_PCM_CHANNEL_MAJOR, 1, stream)))
        {
            s->front.poisoned = true; // the banks behind this one are not fed: they are no longer at one point of the capture
            return rc;
        }
    }
    return 0;
}

extern "C" int jaero_split_output(jaero_split *s, int output, jaero_chan **view)
{
    if (!s || !view) return fail(JAERO_EINVAL, "jaero_split_output: null argument");
    if (output < 0 || output >= (int)s->views.size())
        return fail(JAERO_EINVAL, "jaero_split_output: output %d outside [0, %d)", output, (int)s->views.size());
    *view = s->views[output].get();
    return 0;
}

extern "C" int jaero_split_info(const jaero_split *s, int *noutputs, int *fs_c, int *nblk_max)
{
    if (!s) return fail(JAERO_EINVAL, "jaero_split_info: null handle");
    if (noutputs) *noutputs = (int)s->views.size();
    if (fs_c) *fs_c = s->fs_c;
    if (nblk_max) *nblk_max = s->front.nblk_max;
    return 0;
}

extern "C" int jaero_split_profile_enable(jaero_split *s, int on)
{
    if (!s) return fail(JAERO_EINVAL, "jaero_split_profile_enable: null handle");
    s->front.timer.on = on != 0;
    for (auto &v : s->views) v->timer.on = on != 0;
    return 0;
}

// which 0: the forward transform, k_chan_fwd or k_capture_fwd as the front end has it; 1: k_capture_stage (never launched without a capture)
extern "C" int jaero_split_profile_read(jaero_split *s, int which, double *total_ms, int *launches, int reset)
{
    if (!s || which < 0 || which > 1) return fail(JAERO_EINVAL, "jaero_split_profile_read: bad arguments");
    ChanFront &f = s->front;
    return f.timer.read(f.device, which == 1 ? 4 : f.cap ? 5 : 0, total_ms, launches, reset);
}
