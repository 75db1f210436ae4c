// burst_host.h -- host side of the burst banks (included by jaero_hip.hip after jaero_ctx, fail and host_common.h are defined).
// Geometry = what BurstOqpskDemodulator::setSettings / BurstMskDemodulator::setSettings compute
// (JAERO/burstoqpskdemodulator.cpp:202-277, JAERO/burstmskdemodulator.cpp:150-325); initial scalar state = their constructors.
// The bank's device buffers belong to c->mem, burst_write's launches are timed by c->timer (jaero_profile_read's classes 0 - 4: demodulator,
// k_trident, history push, k_hilbert_fft, k_burst_front with k_ev_compact), and a bit-rate change (burst_rebank) ends in swap_in, as the
// continuous bank's does.
#pragma once

static int host_qround(double d) { return d >= 0.0 ? (int)(d + 0.5) : (int)(d - (double)((int)(d - 1)) + 0.5) + (int)(d - 1); }

static void burst_fill_geometry(BGeom &g, const jaero_settings &s, int nch, unsigned flags, int max_write)
{
    memset(&g, 0, sizeof g);
    g.kind = s.kind; g.nch = nch; g.nchp = (nch + 63) / 64 * 64; g.ngroups = g.nchp / 64;
    g.Fs = s.Fs; g.fb = s.fb; g.flags = flags;
    g.hil_ntaps = 2048;
    g.hil_lat = 4 * 2048 - 2048 + 1; // JFastFir: nfft - K + 1 with the inferred default nfft = 4 * 2^ceil(log2 K)
    g.agc_len = (int)round(1 * s.Fs);
    if (s.kind == JAERO_KIND_BURST_OQPSK)
    {
        const double SPS = 2.0 * s.Fs / s.fb;
        g.SPS = SPS;
        g.agc2_len = (int)round((SPS * 64.0 / s.Fs) * s.Fs);
        g.bt_lag = (int)ceil(1.0 * SPS); g.bt_w = delay_weight(1.0 * SPS);
        g.ma1_len = (int)round((double)host_qround(128.0 * SPS));
        g.mav1_len = (int)(SPS * 128);
        g.fa_lag = (int)ceil(SPS * 128); g.fa_w = delay_weight(SPS * 128); g.fa_len = g.fa_lag + 1;
        g.D1 = (int)(SPS * 128.0 * 2.5 - 190);
        g.tri_sz = host_qround((256.0 + 16.0 + 16.0) * SPS);
        g.D2 = g.tri_sz;
        g.PL = (int)(SPS * 128.0 / 2.0); g.pd_thr = 0.2;
        g.nb = host_qround(128.0 * SPS); g.nt = g.nb;
        g.a1_lag = (int)ceil(SPS / 2.0); g.a1_w = delay_weight(SPS / 2.0);
        g.ee = 0.4;
        g.eb_len = (int)(SPS * (256.0));
        g.msema_len = 128;
        g.startstopstart = (int)(SPS * (1050));
        g.w4 = delay_weight(SPS / 4.0); g.w8 = delay_weight(SPS / 8.0);
        g.res_b0 = 0.0048847995518126464; g.res_b1 = 0; g.res_b2 = -0.0048847995518126464;
        g.res_a1 = -0.3882746897971619; g.res_a2 = 0.99023040089637471;
        g.stref_freq = s.fb;
        g.stq_step = (s.fb / 4.0) * ((double)JD_WTSIZE) / ((float)(double)(int)s.Fs);
        g.fir_n = 55;
        g.maxseg = 2048; // <= tri_sz: at most one trident event per channel per segment
    }
    else
    {
        const double SPS = (int)(s.Fs / s.fb);
        g.SPS = SPS;
        g.agc2_len = (int)round((SPS * 128.0 / s.Fs) * s.Fs);
        g.eb_len = (int)(0.15 * s.Fs);
        g.msema_len = 75;
        g.bt_lag = (int)ceil(1.0 * SPS); g.bt_w = delay_weight(1.0 * SPS);
        if (s.fb >= 1200)
        {
            g.ma1_len = (int)round((double)host_qround(126.0 * SPS));
            g.mav1_len = (int)(SPS * 126);
            g.fa_lag = (int)ceil(SPS * 126); g.fa_w = delay_weight(SPS * 126);
            g.PL = (int)(SPS * 126.0 / 2.0); g.pd_thr = 0.1;
            g.tri_sz = host_qround((200.0) * SPS);
            g.D1 = (int)(((int)289 * SPS) + 20);
            g.D2 = (int)(host_qround(72 + 120.0) * SPS);
            g.startstopstart = (int)(SPS * (500));
            g.endRotation = (int)((120 + 37) * SPS);
            g.res_a1 = -1.993312819378528; g.res_a2 = 0.999476538254407;
            g.res_b0 = 2.617308727964618e-04; g.res_b1 = 0; g.res_b2 = -2.617308727964618e-04;
            g.ee = 0.025;
            g.startProcessing = 120;
            g.nb = host_qround(126 * SPS); g.nt = host_qround(74 * SPS);
        }
        else
        {
            g.mav1_len = (int)(SPS * 150);
            g.fa_lag = (int)ceil(SPS * 150); g.fa_w = delay_weight(SPS * 150);
            g.ma1_len = (int)round((double)host_qround(150.0 * SPS));
            g.PL = (int)(SPS * 150.0 / 2.0); g.pd_thr = 0.2;
            g.tri_sz = host_qround((224) * SPS);
            g.D1 = (int)(((int)397 * SPS) + 20);
            g.D2 = host_qround((72 + 150.0) * SPS);
            g.startstopstart = (int)(SPS * (500));
            g.res_a1 = -1.991228154418550; g.res_a2 = 0.997385427096603;
            g.res_b0 = 0.001307286451699; g.res_b1 = 0; g.res_b2 = -0.001307286451699;
            g.ee = 0.015;
            g.startProcessing = 150;
            g.endRotation = (int)((g.startProcessing + 56) * SPS);
            g.nb = host_qround(150 * SPS); g.nt = host_qround(74 * SPS);
        }
        g.fa_len = g.fa_lag + 1;
        g.a1_lag = (int)(SPS / 2); g.a1_w = 0.0;
        g.d8_len = (int)(SPS / 2) + 1; g.dly_len = (int)SPS + 1;
        g.d8_ring = (g.d8_len + 7) / 8 * 8; g.dly_ring = (g.dly_len + 7) / 8 * 8;
        if ((int)SPS == 40) g.d8_ring = g.d8_len; // 1200 bps: delayt8's ring lives in LDS during a launch (k_burst_msk_fb.h), its HBM copy is exactly d8_len entries
        g.stref_freq = s.fb / 2.0;
        g.stq_step = (s.fb / 2.0) * ((double)JD_WTSIZE) / ((float)(double)(int)s.Fs);
        g.fir_n = 2 * (int)SPS;
        g.maxseg = 4096; // <= tri_sz (8000 / 17920)
    }
    if (g.maxseg > max_write) g.maxseg = (max_write + 15) / 16 * 16;
    g.bt_len = 2 * g.PL + 1;
    g.win_ring = g.agc2_len > g.eb_len ? g.agc2_len : g.eb_len;
    g.cv_len = g.D1 + (g.D2 > g.tri_sz ? g.D2 : g.tri_sz) + g.maxseg + 64;
    // whole cells of four samples (k_hilbert); k_hilbert_fft's first block starts up to 2047 samples before the segment and looks
    // hil_lat + 2048 samples further back
    g.hist_len = (g.hil_lat + 2 * g.hil_ntaps + max_write + 64 + 3) & ~3;
}

template <int FIRN, int LDSN>
static KernelRec<BurstDemodFn> burst_msk_rec(const BGeom &g, bool cs)
{
    return {cs ? k_burst_msk_fb<true, FIRN, LDSN> : k_burst_msk_fb<false, FIRN, LDSN>, g.ngroups, 128, bmsk_fb_lds_bytes<FIRN, LDSN>(g.d8_len), 0, "k_burst_msk_fb",
            instantiation("k_burst_msk_fb", cs, FIRN, LDSN)};
}

// jaero_create of a burst bank, behind `new jaero_ctx`: what it allocated before a failure goes with jaero_destroy
static int burst_create(jaero_ctx *c, const std::vector<jaero_settings> &sets, const hipDeviceProp_t &prop, int softbit_capacity)
{
    const jaero_settings &s0 = sets[0];
    const int nch = (int)sets.size();
    int rc = 0;
    c->burst = true;
    burst_fill_geometry(c->bg, s0, nch, c->flags, c->max_write);
    BGeom &g = c->bg;
    BPtrs &p = c->bp;
    if (softbit_capacity <= 0) softbit_capacity = (int)ceil(2.0 * c->max_write * g.fb / g.Fs) + 128;
    g.soft_cap = (softbit_capacity + 7) & ~7; // 16-byte aligned rows: the burst-mode Aero-L bank reads them in place eight entries per load (k_aerolb_bits<true>)
    g.sym_cap = (c->flags & JAERO_FLAG_CAPTURE_SYMBOLS) ? g.soft_cap / 2 + 8 : 0;
    g.ev_cap = (c->flags & JAERO_FLAG_TRACE) ? 4096 : 256;
    const int nchp = g.nchp, ng = g.ngroups;
    const bool oq = g.kind == JAERO_KIND_BURST_OQPSK;
    DevMem &m = c->mem;
    DA(m, p.S, (size_t)BS_NFIELDS * nchp);
    DA(m, p.I, (size_t)BI_NFIELDS * nchp);
    DA(m, p.pcmhist, (size_t)g.hist_len * nchp);
    DA(m, p.him, (size_t)ng * g.maxseg * 64);
    DA(m, p.agc_ring, (size_t)ng * g.agc_len * 64);
    DA(m, p.cvre, (size_t)ng * g.cv_len * 64); DA(m, p.cvim, (size_t)ng * g.cv_len * 64);
    DA(m, p.ma1re, (size_t)ng * g.ma1_len * 64); DA(m, p.ma1im, (size_t)ng * g.ma1_len * 64);
    DA(m, p.mav1, (size_t)ng * g.mav1_len * 64);
    DA(m, p.fa, (size_t)ng * g.fa_len * 64);
    DA(m, p.bt, (size_t)ng * g.bt_len * 64);
    DA(m, p.ev_list, nchp); DA(m, p.ev_count, 4); DA(m, p.ev_mask, ng);
    DA(m, p.tri, nchp);
    DA(m, p.eb_e, (size_t)nchp * g.win_ring);
    DA(m, p.firsave, (size_t)nchp * 2 * g.fir_n);
    if (!oq) { DA(m, p.dly, (size_t)nchp * g.dly_ring); DA(m, p.dly8, (size_t)nchp * g.d8_ring); DA(m, p.a1, (size_t)nchp * g.d8_len); }
    DA(m, p.msema, (size_t)nchp * g.msema_len);
    DA(m, p.soft, (size_t)nchp * g.soft_cap);
    if (g.sym_cap) DA(m, p.sym, (size_t)nchp * g.sym_cap * 3);
    DA(m, p.evlog, (size_t)nchp * g.ev_cap * 3);
    DA(m, c->d_pcm_raw, (size_t)c->max_write * nch);
    DA(m, c->d_status, nchp);
    if (!oq && ((g.agc2_len | g.eb_len) & 7))
        return fail(JAERO_ENOTSUP, "burst MSK at fb %g / Fs %g: the AGC2 / EbNo windows (%d, %d entries) are not whole cells of eight", g.fb, g.Fs, g.agc2_len, g.eb_len);
    if (oq && ((int)floor((0.25 * g.fb) / (g.Fs / (double)TRI_N) + 0.5)) % 4 != 0)
        return fail(JAERO_ENOTSUP, "burst OQPSK at fb %g / Fs %g: k_trident searches one residue class of bins at a time and needs round(fb / 4 / hzperbin) to be a multiple of 4", g.fb, g.Fs);
    double2 *d_cis = nullptr, *d_tw = nullptr, *d_tw15 = nullptr;
    double *d_taps = nullptr, *d_hil = nullptr;
    DA(m, d_cis, JD_WTSIZE); DA(m, d_tw, TRI_H); DA(m, d_tw15, TRI_H); DA(m, d_taps, 2 * g.fir_n); DA(m, d_hil, g.hil_ntaps / 4);
    p.cis = d_cis; p.tw14 = d_tw; p.tw15 = d_tw15; p.taps2 = d_taps; p.hil_taps = d_hil;
    {
        HIPCHK(hipMemcpy(d_cis, cis_table().data(), sizeof(double2) * JD_WTSIZE, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_tw, twiddles(8192, 8192).data(), sizeof(double2) * 8192, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_tw15, twiddles(TRI_N, TRI_H).data(), sizeof(double2) * TRI_H, hipMemcpyHostToDevice));
        const std::vector<double> taps = oq ? rrc_design(1.0, 55, g.Fs, g.fb / 2.0) : half_sine_taps((int)g.SPS);
        HIPCHK(hipMemcpy(d_taps, doubled_taps(taps).data(), sizeof(double) * 2 * g.fir_n, hipMemcpyHostToDevice));
        // QJHilbertFilter::setSize (JAERO/DSP.cpp:760-787): imaginary part of the odd taps
        const int N = g.hil_ntaps;
        std::vector<double> hil(N / 4);
        for (int j = 0; j < N / 4; j++)
        {
            const int i = 2 * j + 1;
            hil[j] = (2.0 / ((double)N)) / (tan(M_PI * (((double)i) / ((double)N) - 0.5)));
        }
        HIPCHK(hipMemcpy(d_hil, hil.data(), sizeof(double) * hil.size(), hipMemcpyHostToDevice));
        // the same taps at their positions k = 1, 3, ... 2047 for the overlap-save form (k_hilbert_fft)
        std::vector<double> gk(N, 0.0);
        for (int k = 1; k < N; k += 2) gk[k] = (2.0 / ((double)N)) / (tan(M_PI * (((double)k) / ((double)N) - 0.5)));
        double2 *dH = nullptr, *dtw = nullptr;
        if ((rc = fft4096_tables(m, gk, &dH, &dtw, (const void *)k_hilbert_fft))) return rc;
        p.hilH = dH; p.tw12 = dtw;
        if (g.hil_ntaps != 2048) return fail(JAERO_ENOTSUP, "the overlap-save Hilbert kernel is built for QJHilbertFilter's 2048 taps");
    }
    // scalar state
    {
        std::vector<double> S((size_t)BS_NFIELDS * nchp, 0.0);
        std::vector<int> I((size_t)BI_NFIELDS * nchp, 0);
        std::vector<double> ev((size_t)nchp * g.ev_cap * 3, 0.0);
        c->settings.resize(nchp);
        for (int ch = 0; ch < nchp; ch++)
        {
            const jaero_settings &s = sets[ch < nch ? ch : 0];
            c->settings[ch] = s;
            auto SS = [&](int f) -> double & { return S[(size_t)f * nchp + ch]; };
            auto II = [&](int f) -> int & { return I[(size_t)f * nchp + ch]; };
            double fc = s.freq_center;
            if (fc > ((s.Fs / 2.0) - (s.lockingbw / 2.0))) fc = ((s.Fs / 2.0) - (s.lockingbw / 2.0));
            if (fc < 0) fc = 0;
            SS(BS_M2_FREQ) = fc; SS(BS_M2_STEP) = fc * ((double)JD_WTSIZE) / ((float)(double)(int)s.Fs); SS(BS_MC_FREQ) = fc;
            SS(BS_ST_FREQ) = g.stref_freq; SS(BS_ST_STEP) = g.stref_freq * ((double)JD_WTSIZE) / ((float)(double)(int)s.Fs);
            SS(BS_VOL_GAIN) = 1; SS(BS_STR_RE) = 1; SS(BS_SAV_RE) = 1; SS(BS_ROT_RE) = 1;
            SS(BS_MSE) = oq ? 100.0 : 10.0; SS(BS_LASTMSE) = SS(BS_MSE);
            SS(BS_THRESH) = s.signalthreshold; SS(BS_LOCKINGBW) = s.lockingbw; SS(BS_DIFF_LAST) = -1.0;
            II(BI_CNTDOWN) = 2 * g.PL; II(BI_MAXPOSCD) = -1; II(BI_TRI_PTR) = 0; II(BI_EV_POS) = -1;
            II(BI_STARTSTOP) = -1;
            // emit Plottables(...) at the end of setSettings
            ev[((size_t)ch * g.ev_cap) * 3 + 0] = 0; ev[((size_t)ch * g.ev_cap) * 3 + 1] = BEV_FREQ; ev[((size_t)ch * g.ev_cap) * 3 + 2] = fc;
            II(BI_EV_CNT) = 1;
        }
        HIPCHK(hipMemcpy(p.S, S.data(), S.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p.I, I.data(), I.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p.evlog, ev.data(), ev.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    c->o_nch = nch; c->o_nchp = nchp; c->o_soft_cap = g.soft_cap; c->o_sym_cap = g.sym_cap;
    c->o_soft = p.soft; c->o_sym = p.sym;
    c->o_soft_cnt = p.I + (size_t)BI_SOFT_CNT * nchp; c->o_sym_cnt = p.I + (size_t)BI_SYM_CNT * nchp;
    c->o_overflow = p.I + (size_t)BI_OVERFLOW * nchp; c->o_flags = p.I + (size_t)BI_FLAGS * nchp;
    c->o_nrx = p.I + (size_t)BI_NRX * nchp;
    c->m.nch = nch; c->m.nchp = nchp;
    c->m.flags.assign(nchp, 0);
    // the tracking kernel: burst OQPSK keeps BD_LDSN of its 55 history slots and the taps in LDS (k_burst_demod.h); burst MSK runs front / back
    // wavefront pairs (k_burst_msk_fb.h) with 48 of 80 (1200 bps) or 128 of 160 (600 bps) history slots, the mailboxes and the write-combining cells in LDS
    const bool cs = (c->flags & JAERO_FLAG_CAPTURE_SYMBOLS) != 0;
    if (oq) c->bdemod = {cs ? k_burst_oqpsk_demod<true> : k_burst_oqpsk_demod<false>, ng, 64, bd_lds_bytes(), 0, "k_burst_oqpsk_demod", instantiation("k_burst_oqpsk_demod", cs)};
    else if (g.fir_n == 80) c->bdemod = burst_msk_rec<80, BMSK_FB_LDSN_80>(g, cs);
    else { assert(g.fir_n == 160); c->bdemod = burst_msk_rec<160, BMSK_FB_LDSN_160>(g, cs); } // validate_settings: 600 or 1200 bps at 48 kHz
    // k_trident: two 256-thread workgroups per CU, wg_fft13_e32's exchange buffer in LDS (one residue class of trident differences shares it)
    const int tri_grid = 2 * (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256);
    c->trident = {oq ? k_trident<true> : k_trident<false>, tri_grid < nchp ? tri_grid : nchp, TRI_THREADS, TRI_XCH * (int)sizeof(double), 0, "k_trident",
                  instantiation("k_trident", oq)};
    HIPCHK(set_lds_attribute(c->bdemod));
    HIPCHK(set_lds_attribute(c->trident));
    HIPCHK(hipDeviceSynchronize());
    return 0;
}

// The launch lines of a write's transform kernels, shared by burst_write and the test hooks jaero_debug_burst_* (below): the history push of
// one write, k_hilbert_fft and k_burst_front of one segment, k_ev_compact and the bank's trident kernel with `grid` workgroups (burst_write:
// c->trident.grid).
static int burst_launch_hist_push(jaero_ctx *c, const int16_t *dsrc, int nsamples, int layout, int slot0, hipStream_t st)
{
    const BGeom &g = c->bg;
    const BPtrs &p = c->bp;
    const int nch = g.nch, nchp = g.nchp;
    if (layout == JAERO_PCM_FRAME_MAJOR)
        hipLaunchKernelGGL(k_hist_push_frames, dim3((nchp + 255) / 256, nsamples), dim3(256), 0, st, dsrc, nch, nch, p.pcmhist, nchp, g.hist_len, slot0, nsamples);
    else
        hipLaunchKernelGGL(k_hist_push_chmajor, dim3(nchp / 64, (nsamples + 63) / 64), dim3(256), 0, st, dsrc, nch, nsamples, p.pcmhist, nchp, g.hist_len, slot0);
    LAUNCHCHK("the burst history push");
    return 0;
}
static int burst_launch_hilbert(jaero_ctx *c, int n, long long n0, hipStream_t st)
{
    const BGeom &g = c->bg;
    const BPtrs &p = c->bp;
    hipLaunchKernelGGL(k_hilbert_fft, dim3(g.nchp / 8, (int)(((n0 + n - 1) >> 11) - (n0 >> 11) + 1)), dim3(PF_THREADS), 4 * 2 * PRE_L * (int)sizeof(double), st, g, p, n, n0);
    LAUNCHCHK("k_hilbert_fft");
    return 0;
}
// k_burst_front of one segment: the HOLD instantiation while a lane may still hold (see burst_write), and the count of what is left of that
static int burst_launch_front(jaero_ctx *c, int n, long long n0, hipStream_t st)
{
    const BGeom &g = c->bg;
    const BPtrs &p = c->bp;
    // bt_hold_left is an UPPER BOUND of every lane's BI_BT_HOLD (the per-lane, per-sample counter the kernel obeys): each setSettings sets
    // both to bt_lag at the same moment, the lane's falls by one per sample, this one by n per segment of n samples -- so while any lane
    // still holds, the HOLD instantiation runs (for all lanes: those whose counter is 0 compute what <false> computes).  A write that
    // poisons the bank leaves the counter alone: a poisoned bank accepts nothing but jaero_destroy.
    if (c->bt_hold_left > 0)
    {
        hipLaunchKernelGGL(k_burst_front<true>, dim3(g.ngroups), dim3(64), 0, st, g, p, n, n0);
        c->bt_hold_left -= n;
    }
    else hipLaunchKernelGGL(k_burst_front<false>, dim3(g.ngroups), dim3(64), 0, st, g, p, n, n0);
    LAUNCHCHK("k_burst_front");
    return 0;
}
static int burst_launch_ev_compact_on(const unsigned long long *mask, int ngroups, int *ev_list, int *ev_count, hipStream_t st)
{
    hipLaunchKernelGGL(k_ev_compact, dim3(1), dim3(1024), 0, st, mask, ngroups, ev_list, ev_count);
    LAUNCHCHK("k_ev_compact");
    return 0;
}
static int burst_launch_ev_compact(jaero_ctx *c, hipStream_t st)
{
    return burst_launch_ev_compact_on((const unsigned long long *)c->bp.ev_mask, c->bg.ngroups, c->bp.ev_list, c->bp.ev_count, st);
}
static int burst_launch_trident(jaero_ctx *c, int grid, long long n0, hipStream_t st)
{
    const KernelRec<TridentFn> &tri = c->trident;
    hipLaunchKernelGGL(tri.fn, dim3(grid), dim3(tri.block), tri.lds, st, c->bg, c->bp, n0);
    LAUNCHCHK("k_trident");
    return 0;
}
// BurstMskDemodulator::CenterFreqChangedSlot for one channel or all (channel < 0), stamped with the first sample of the write that follows
// (jaero_center_freq_changed and jaero_debug_burst_track_center_freq)
static int burst_launch_center_freq(jaero_ctx *c, int channel, double hz)
{
    const int lo = channel < 0 ? 0 : channel, n = channel < 0 ? c->o_nch : 1;
    hipLaunchKernelGGL(k_burst_msk_center_freq, dim3((n + 63) / 64), dim3(64), 0, c->last_stream, c->bg, c->bp, lo, n, hz, (long long)c->nsamples_total);
    HIPCHK(hipGetLastError());
    return 0;
}
// the bank's tracking kernel on one segment (burst_write and jaero_debug_burst_track)
static int burst_launch_demod(jaero_ctx *c, int n, long long n0, int first_of_write, hipStream_t st)
{
    const KernelRec<BurstDemodFn> &dm = c->bdemod;
    hipLaunchKernelGGL(dm.fn, dim3(dm.grid), dim3(dm.block), dm.lds, st, c->bg, c->bp, n, n0, first_of_write);
    LAUNCHCHK("the burst demodulator");
    return 0;
}

static int burst_write(jaero_ctx *c, const int16_t *pcm, int nsamples, int layout, int is_device_ptr, hipStream_t st)
{
    const BGeom &g = c->bg;
    const int nch = g.nch;
    int rc = 0;
    const int16_t *dsrc = pcm;
    if (!is_device_ptr)
    {
        HIPCHK(hipMemcpyAsync(c->d_pcm_raw, pcm, sizeof(int16_t) * (size_t)nch * nsamples, hipMemcpyHostToDevice, st));
        dsrc = c->d_pcm_raw;
    }
    // new samples -> PCM history ring (the Hilbert FIR only ever reads the ring)
    {
        const int pi = c->timer.begin(2, st);
        const int slot0 = (int)(c->nsamples_total % g.hist_len);
        if ((rc = burst_launch_hist_push(c, dsrc, nsamples, layout, slot0, st))) return rc;
        c->timer.end(pi, st);
    }
    int first = 1;
    PoisonGuard guard(*c); // the history push above is idempotent (same slots if the write is repeated); from here on state advances
    for (int pos = 0; pos < nsamples;)
    {
        const int n = (nsamples - pos) < g.maxseg ? (nsamples - pos) : g.maxseg;
        const long long n0 = c->nsamples_total;
        int pi = c->timer.begin(3, st);
        if ((rc = burst_launch_hilbert(c, n, n0, st))) return rc;
        c->timer.end(pi, st);
        pi = c->timer.begin(4, st);
        if ((rc = burst_launch_front(c, n, n0, st))) return rc;
        if ((rc = burst_launch_ev_compact(c, st))) return rc;
        c->timer.end(pi, st);
        pi = c->timer.begin(1, st);
        if ((rc = burst_launch_trident(c, c->trident.grid, n0, st))) return rc;
        c->timer.end(pi, st);
        pi = c->timer.begin(0, st);
        if ((rc = burst_launch_demod(c, n, n0, first, st))) return rc;
        c->timer.end(pi, st);
        first = 0;
        c->nsamples_total += n;
        pos += n;
    }
    HIPCHK(hipGetLastError());
    guard.commit();
    return 0;
}

// jaero_set_settings with another bit rate on a burst MSK bank (BurstMskDemodulator::setSettings with another fb on the live object,
// burstmskdemodulator.cpp:150-325): a sibling bank for the new rate takes the old one's place behind the handle; the scalar state comes
// across as whole columns, k_burst_carry moves the DelayThings' contents in storage order and applies what setSettings re-creates, msema and
// the outputs not read yet are copied.  Control plane: allocates and synchronises.
static int burst_rebank(jaero_ctx *c, const jaero_settings *s)
{
    LINKCHK(c);
    if (c->poisoned) return fail(JAERO_EHIP, "jaero_set_settings: a launch inside an earlier jaero_write failed; this bank's state cannot be carried over");
    const BGeom og = c->bg;
    QUIESCE(c);
    jaero_ctx *n = nullptr;
    int rc = jaero_create(c->device, og.nch, s, 0, c->flags, c->max_write, c->soft_cap_req, &n);
    if (rc) return rc;
    BankPtr nb(n, jaero_destroy); // goes again on every early return
    const BGeom &ng = n->bg;
    const int nchp = og.nchp;
    {
        // outputs not read yet: soft bits (RxDataBits' pending tail included), captured symbols, event rows
        std::vector<int> cnt(2 * (size_t)nchp);
        static_assert(BI_SYM_CNT == BI_SOFT_CNT + 1, "output counters are consecutive columns");
        HIPCHK(hipMemcpy(cnt.data(), c->bp.I + (size_t)BI_SOFT_CNT * nchp, sizeof(int) * cnt.size(), hipMemcpyDeviceToHost));
        int mx[2] = {0, 0};
        for (int k = 0; k < 2; k++) for (int ch = 0; ch < og.nch; ch++) mx[k] = cnt[(size_t)k * nchp + ch] > mx[k] ? cnt[(size_t)k * nchp + ch] : mx[k];
        if (mx[0] > ng.soft_cap || mx[1] > ng.sym_cap)
            return fail(JAERO_EINVAL, "jaero_set_settings: unread outputs (%d soft bits, %d symbols) exceed the new bank's buffers; read them first", mx[0], mx[1]);
        if ((rc = carry_rows(n->bp.soft, ng.soft_cap, c->bp.soft, og.soft_cap, sizeof(int16_t), mx[0], nchp)) ||
            (rc = carry_rows(n->bp.sym, ng.sym_cap, c->bp.sym, og.sym_cap, 3 * sizeof(double), mx[1], nchp)) ||
            (rc = carry(n->bp.evlog, c->bp.evlog, sizeof(double) * (size_t)nchp * og.ev_cap * 3)))
            return rc;
    }
    if ((rc = carry(n->bp.S, c->bp.S, sizeof(double) * (size_t)BS_NFIELDS * nchp)) || (rc = carry(n->bp.I, c->bp.I, sizeof(int) * (size_t)BI_NFIELDS * nchp)) ||
        (rc = carry(n->bp.msema, c->bp.msema, sizeof(double) * (size_t)nchp * og.msema_len))) // msema is made once, in the constructor
        return rc;
    BSetVals v;
    v.freq_center = s->freq_center; v.lockingbw = s->lockingbw; v.signalthreshold = s->signalthreshold;
    hipLaunchKernelGGL(k_burst_carry, dim3(nchp / 64), dim3(64), 0, 0, og, c->bp, ng, n->bp, v, (long long)c->nsamples_total);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(0) != hipSuccess) return fail(JAERO_EHIP, "jaero_set_settings: carry-over failed");
    n->nsamples_total = c->nsamples_total;
    n->bt_hold_left = ng.bt_lag;
    swap_in(c, std::move(nb));
    for (int &f : c->m.flags) f &= ~JF_DCD; // dcd = false at the end of BurstMskDemodulator::setSettings
    return 0;
}

// jaero_set_settings on live channels [lo, hi) of a burst bank: what BurstOqpskDemodulator::setSettings / BurstMskDemodulator::setSettings do to an
// object that has been running (k_burst_settings.h), on the bank's stream like every other call.  A bank's bit rate and sample rate are fixed
// (ring lengths, kernel instantiations): another fb / Fs is another bank.
static int burst_set_settings(jaero_ctx *c, int channel, const jaero_settings *s)
{
    const BGeom &g = c->bg;
    if (s->kind != g.kind) return fail(JAERO_EINVAL, "jaero_set_settings: the kind of a bank is fixed (another demodulator class in the reference); create a new bank");
    if (s->fb != g.fb || s->Fs != g.Fs)
    {
        if (g.kind != JAERO_KIND_BURST_MSK || s->Fs != g.Fs)
            return fail(JAERO_ENOTSUP, "jaero_set_settings on a burst bank: only burst MSK changes its bit rate (600 / 1200 bps at %g Hz); asked for fb %g / Fs %g", g.Fs, s->fb, s->Fs);
        if (channel >= 0 && g.nch > 1)
            return fail(JAERO_EINVAL, "jaero_set_settings: fb is shared by the channels of a bank; change it for the whole bank (channel = -1)");
        return burst_rebank(c, s);
    }
    HIPCHK(hipSetDevice(c->device));
    const int lo = channel < 0 ? 0 : channel, hi = channel < 0 ? g.nch : channel + 1;
    BSetVals v;
    v.freq_center = s->freq_center; v.lockingbw = s->lockingbw; v.signalthreshold = s->signalthreshold;
    hipLaunchKernelGGL(k_burst_apply_settings, dim3((hi - lo + 63) / 64, 65), dim3(64), 0, c->last_stream, g, c->bp, lo, hi, v, (long long)c->nsamples_total);
    HIPCHK(hipGetLastError());
    for (int ch = lo; ch < hi; ch++)
    {
        c->settings[ch] = *s;
        if (g.kind == JAERO_KIND_BURST_MSK) c->m.flags[ch] &= ~JF_DCD; // dcd = false at the end of BurstMskDemodulator::setSettings
    }
    c->bt_hold_left = g.bt_lag;
    return 0;
}

// ------------------------------------------------------------------------------------------ test hooks: the burst banks' transform kernels alone
// (tests/test_gpu_burst_acq.py), through burst_launch_hist_push / _hilbert / _ev_compact / _trident as burst_write calls them.  hilbert, poke_cv
// and trident leave the bank's state where no write would: poisoned, as after a write that failed part-way.
static int burst_hook_enter(jaero_ctx *c, const char *who, int channel, bool poison)
{
    if (!c) return fail(JAERO_EINVAL, "%s: null ctx", who);
    if (!c->burst) return fail(JAERO_EINVAL, "%s: not a burst bank", who);
    if (channel < 0 || channel >= c->bg.nch) return fail(JAERO_EINVAL, "%s: channel %d outside [0, %d)", who, channel, c->bg.nch);
    QUIESCE(c);
    if (poison) c->poisoned = true;
    return 0;
}
extern "C" int jaero_debug_burst_geom(jaero_ctx *c, jaero_burst_geom *out)
{
    if (!out) return fail(JAERO_EINVAL, "jaero_debug_burst_geom: null output");
    int rc = burst_hook_enter(c, "jaero_debug_burst_geom", 0, false);
    if (rc) return rc;
    const BGeom &g = c->bg;
    out->kind = g.kind; out->nch = g.nch; out->nchp = g.nchp; out->maxseg = g.maxseg; out->hist_len = g.hist_len; out->hil_lat = g.hil_lat;
    out->cv_len = g.cv_len; out->D1 = g.D1; out->tri_sz = g.tri_sz; out->nb = g.nb; out->nt = g.nt; out->tri_grid = c->trident.grid;
    out->nsamples = c->nsamples_total;
    return 0;
}
extern "C" int jaero_debug_burst_hilbert(jaero_ctx *c, const int16_t *pcm, int layout, int nsamples, double *out_im)
{
    if (c && c->burst && (!pcm || !out_im || nsamples <= 0 || nsamples > c->max_write))
        return fail(JAERO_EINVAL, "jaero_debug_burst_hilbert: nsamples %d (1 .. max_write_samples %d of host PCM, and an output)", nsamples, c->max_write);
    if (layout != JAERO_PCM_CHANNEL_MAJOR && layout != JAERO_PCM_FRAME_MAJOR) return fail(JAERO_EINVAL, "jaero_debug_burst_hilbert: bad layout");
    int rc = burst_hook_enter(c, "jaero_debug_burst_hilbert", 0, true);
    if (rc) return rc;
    const BGeom &g = c->bg;
    hipStream_t st = c->last_stream;
    HIPCHK(hipMemcpyAsync(c->d_pcm_raw, pcm, sizeof(int16_t) * (size_t)g.nch * nsamples, hipMemcpyHostToDevice, st));
    if ((rc = burst_launch_hist_push(c, c->d_pcm_raw, nsamples, layout, (int)(c->nsamples_total % g.hist_len), st))) return rc;
    std::vector<double> him((size_t)g.ngroups * g.maxseg * 64);
    for (int pos = 0; pos < nsamples;)
    {
        const int n = (nsamples - pos) < g.maxseg ? (nsamples - pos) : g.maxseg; // burst_write's segments
        if ((rc = burst_launch_hilbert(c, n, c->nsamples_total, st))) return rc;
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(him.data(), c->bp.him, sizeof(double) * him.size(), hipMemcpyDeviceToHost));
        for (int ch = 0; ch < g.nch; ch++)
            for (int i = 0; i < n; i++) out_im[(size_t)ch * nsamples + pos + i] = him[((size_t)(ch >> 6) * g.maxseg + i) * 64 + (ch & 63)];
        c->nsamples_total += n;
        pos += n;
    }
    return 0;
}
extern "C" int jaero_debug_burst_read_hist(jaero_ctx *c, int ch, long long first, int n, int16_t *out)
{
    if (!out) return fail(JAERO_EINVAL, "jaero_debug_burst_read_hist: null output");
    int rc = burst_hook_enter(c, "jaero_debug_burst_read_hist", ch, false);
    if (rc) return rc;
    const BGeom &g = c->bg;
    const long long H = g.hist_len, oldest = c->nsamples_total > H ? c->nsamples_total - H : 0;
    if (n <= 0 || first < oldest || first > c->nsamples_total - n)
        return fail(JAERO_EINVAL, "jaero_debug_burst_read_hist: samples [%lld, %lld + %d) are not all among the last %lld of the %lld written", first, first, n, H, (long long)c->nsamples_total);
    // the channel's cells of four samples (hb_idx, k_burst_front.h), one row of the ring each
    std::vector<int16_t> ring((size_t)H);
    HIPCHK(hipMemcpy2D(ring.data(), sizeof(int16_t) * 4, c->bp.pcmhist + (size_t)ch * 4, sizeof(int16_t) * 4 * (size_t)g.nchp, sizeof(int16_t) * 4, (size_t)(H / 4), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) out[i] = ring[(size_t)((first + i) % H)];
    return 0;
}
// a channel's column of a [group][slot][lane] ring, by absolute sample index (sample a lives at slot a mod len, mathematical modulo)
static int burst_ring_column(double *ring, int len, int ch, long long first, int n, double *host, bool to_device)
{
    const long long R = len;
    const int slot = (int)(((first % R) + R) % R), n1 = n < len - slot ? n : len - slot;
    double *col = ring + (size_t)(ch >> 6) * len * 64 + (ch & 63);
    if (to_device)
    {
        HIPCHK(hipMemcpy2D(col + (size_t)slot * 64, sizeof(double) * 64, host, sizeof(double), sizeof(double), (size_t)n1, hipMemcpyHostToDevice));
        if (n > n1) HIPCHK(hipMemcpy2D(col, sizeof(double) * 64, host + n1, sizeof(double), sizeof(double), (size_t)(n - n1), hipMemcpyHostToDevice));
    }
    else
    {
        HIPCHK(hipMemcpy2D(host, sizeof(double), col + (size_t)slot * 64, sizeof(double) * 64, sizeof(double), (size_t)n1, hipMemcpyDeviceToHost));
        if (n > n1) HIPCHK(hipMemcpy2D(host + n1, sizeof(double), col, sizeof(double) * 64, sizeof(double), (size_t)(n - n1), hipMemcpyDeviceToHost));
    }
    return 0;
}
extern "C" int jaero_debug_burst_poke_cv(jaero_ctx *c, int ch, long long first, int n, const double *re)
{
    if (!re) return fail(JAERO_EINVAL, "jaero_debug_burst_poke_cv: null input");
    if (c && c->burst && (n <= 0 || n > c->bg.cv_len || first < -(1LL << 40) || first > (1LL << 40)))
        return fail(JAERO_EINVAL, "jaero_debug_burst_poke_cv: n %d (1 .. cv_len %d samples from an index within +- 2^40)", n, c->bg.cv_len);
    int rc = burst_hook_enter(c, "jaero_debug_burst_poke_cv", ch, true);
    if (rc) return rc;
    return burst_ring_column(c->bp.cvre, c->bg.cv_len, ch, first, n, const_cast<double *>(re), true); // sample a lives at a mod cv_len (k_burst_front: s_cv = n0 % cv_len)
}
static_assert(sizeof(jaero_trident_result) == sizeof(TriResult) && offsetof(jaero_trident_result, metric) == offsetof(TriResult, metric), "jaero_trident_result is TriResult");
extern "C" int jaero_debug_burst_trident(jaero_ctx *c, const int *channels, const int *ev_pos, int nlist, long long n0, int grid, jaero_trident_result *results, int *nchanged)
{
    int rc = burst_hook_enter(c, "jaero_debug_burst_trident", 0, false);
    if (rc) return rc;
    const BGeom &g = c->bg;
    const int nch = g.nch, nchp = g.nchp;
    if (nlist < 0 || nlist > nch || (nlist > 0 && (!channels || !ev_pos || !results)))
        return fail(JAERO_EINVAL, "jaero_debug_burst_trident: nlist %d (0 .. %d channels with their event positions and room for their results)", nlist, nch);
    if (n0 < 0 || n0 > (1LL << 40)) return fail(JAERO_EINVAL, "jaero_debug_burst_trident: n0 %lld outside [0, 2^40]", n0);
    if (grid < 0 || grid > c->trident.grid) return fail(JAERO_EINVAL, "jaero_debug_burst_trident: grid %d (0 = as jaero_write, else 1 .. %d)", grid, c->trident.grid);
    std::vector<int> evp((size_t)nchp, -1);
    std::vector<unsigned long long> mask((size_t)g.ngroups, 0ULL);
    for (int k = 0; k < nlist; k++)
    {
        const int ch = channels[k];
        if (ch < 0 || ch >= nch || evp[(size_t)ch] >= 0)
            return fail(JAERO_EINVAL, "jaero_debug_burst_trident: entry %d (channel %d) is outside [0, %d) or listed twice", k, ch, nch);
        if (ev_pos[k] < 0 || ev_pos[k] >= g.maxseg) return fail(JAERO_EINVAL, "jaero_debug_burst_trident: entry %d: event position %d outside [0, %d)", k, ev_pos[k], g.maxseg);
        evp[(size_t)ch] = ev_pos[k];
        mask[(size_t)(ch >> 6)] |= 1ULL << (ch & 63);
    }
    hipStream_t st = c->last_stream;
    c->poisoned = true;
    const int sentinel = 0xA5;
    HIPCHK(hipMemset(c->bp.tri, sentinel, sizeof(TriResult) * (size_t)nchp));
    HIPCHK(hipMemcpy(c->bp.I + (size_t)BI_EV_POS * nchp, evp.data(), sizeof(int) * (size_t)nchp, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->bp.ev_mask, mask.data(), sizeof(unsigned long long) * mask.size(), hipMemcpyHostToDevice));
    if ((rc = burst_launch_ev_compact(c, st))) return rc;
    if ((rc = burst_launch_trident(c, grid ? grid : c->trident.grid, n0, st))) return rc;
    HIPCHK(hipStreamSynchronize(st));
    std::vector<TriResult> tri((size_t)nchp);
    HIPCHK(hipMemcpy(tri.data(), c->bp.tri, sizeof(TriResult) * (size_t)nchp, hipMemcpyDeviceToHost));
    TriResult untouched;
    memset(&untouched, sentinel, sizeof untouched);
    int changed = 0;
    for (int ch = 0; ch < nchp; ch++) changed += memcmp(&tri[(size_t)ch], &untouched, sizeof untouched) != 0;
    for (int k = 0; k < nlist; k++) memcpy(&results[k], &tri[(size_t)channels[k]], sizeof(TriResult));
    if (nchanged) *nchanged = changed;
    return 0;
}

// ------------------------------------------------------------------------------------------ test hooks: k_burst_front and k_ev_compact alone
// (tests/test_gpu_burst_front.py), through burst_launch_hist_push / _hilbert / _front / _ev_compact as burst_write calls them.  front, front_poke
// and poke_bt poison the bank; front_geom, front_peek and front_events only read.  Peek and the pokes reach the padding lanes of the last wavefront too.
static int burst_front_enter(jaero_ctx *c, const char *who, int channel, bool poison)
{
    if (c && c->burst && (channel < 0 || channel >= c->bg.nchp)) return fail(JAERO_EINVAL, "%s: channel %d outside [0, %d) (padding lanes included)", who, channel, c->bg.nchp);
    return burst_hook_enter(c, who, 0, poison);
}
extern "C" int jaero_debug_burst_front_geom(jaero_ctx *c, jaero_burst_front_geom *out)
{
    if (!out) return fail(JAERO_EINVAL, "jaero_debug_burst_front_geom: null output");
    int rc = burst_hook_enter(c, "jaero_debug_burst_front_geom", 0, false);
    if (rc) return rc;
    const BGeom &g = c->bg;
    out->PL = g.PL; out->bt_len = g.bt_len; out->bt_lag = g.bt_lag; out->agc_len = g.agc_len; out->ma1_len = g.ma1_len; out->mav1_len = g.mav1_len;
    out->fa_len = g.fa_len; out->fa_lag = g.fa_lag; out->ev_cap = g.ev_cap; out->ngroups = g.ngroups;
    out->pd_thr = g.pd_thr; out->bt_w = g.bt_w; out->fa_w = g.fa_w;
    return 0;
}
extern "C" int jaero_debug_burst_front(jaero_ctx *c, const int16_t *pcm, int layout, int n, const double *im, int *ev_pos, int *ev_list, int *ev_count)
{
    if (c && c->burst && (!pcm || !ev_pos || !ev_list || !ev_count || n <= 0 || n > c->bg.maxseg || n > c->max_write))
        return fail(JAERO_EINVAL, "jaero_debug_burst_front: n %d (one segment: 1 .. min(maxseg %d, max_write_samples %d) samples of host PCM, and the three outputs)", n, c->bg.maxseg, c->max_write);
    if (layout != JAERO_PCM_CHANNEL_MAJOR && layout != JAERO_PCM_FRAME_MAJOR) return fail(JAERO_EINVAL, "jaero_debug_burst_front: bad layout");
    int rc = burst_hook_enter(c, "jaero_debug_burst_front", 0, true);
    if (rc) return rc;
    const BGeom &g = c->bg;
    const int nch = g.nch, nchp = g.nchp;
    hipStream_t st = c->last_stream;
    const long long n0 = c->nsamples_total;
    HIPCHK(hipMemcpyAsync(c->d_pcm_raw, pcm, sizeof(int16_t) * (size_t)nch * n, hipMemcpyHostToDevice, st));
    if ((rc = burst_launch_hist_push(c, c->d_pcm_raw, n, layout, (int)(n0 % g.hist_len), st))) return rc;
    if (im)
    {
        // k_hilbert_fft's output layout: sample i of channel ch at ((ch >> 6) * maxseg + i) * 64 + (ch & 63)
        std::vector<double> him((size_t)g.ngroups * g.maxseg * 64, 0.0);
        for (int ch = 0; ch < nch; ch++)
            for (int i = 0; i < n; i++) him[((size_t)(ch >> 6) * g.maxseg + i) * 64 + (ch & 63)] = im[(size_t)ch * n + i];
        HIPCHK(hipMemcpyAsync(c->bp.him, him.data(), sizeof(double) * him.size(), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st)); // him leaves scope
    }
    else if ((rc = burst_launch_hilbert(c, n, n0, st))) return rc;
    if ((rc = burst_launch_front(c, n, n0, st))) return rc;
    if ((rc = burst_launch_ev_compact(c, st))) return rc;
    HIPCHK(hipStreamSynchronize(st));
    c->nsamples_total += n;
    int count = 0;
    HIPCHK(hipMemcpy(ev_pos, c->bp.I + (size_t)BI_EV_POS * nchp, sizeof(int) * (size_t)nch, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&count, c->bp.ev_count, sizeof(int), hipMemcpyDeviceToHost));
    *ev_count = count;
    if (count < 0 || count > nch) return fail(JAERO_EHIP, "jaero_debug_burst_front: k_ev_compact counted %d events among %d channels", count, nch);
    if (count) HIPCHK(hipMemcpy(ev_list, c->bp.ev_list, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int jaero_debug_burst_front_peek(jaero_ctx *c, int ch, jaero_burst_front_state *out, int ring, long long first, int n, double *ring_out)
{
    if (ring > JAERO_FRONT_RING_BT || (ring >= 0 && (!ring_out || n <= 0))) return fail(JAERO_EINVAL, "jaero_debug_burst_front_peek: ring %d, n %d (a ring 0 .. 7 with n >= 1 and an output, or ring < 0)", ring, n);
    int rc = burst_front_enter(c, "jaero_debug_burst_front_peek", ch, false);
    if (rc) return rc;
    const BGeom &g = c->bg;
    const BPtrs &p = c->bp;
    const int nchp = g.nchp;
    if (ring >= 0)
    {
        double *const rings[8] = {p.agc_ring, p.cvre, p.cvim, p.ma1re, p.ma1im, p.mav1, p.fa, p.bt};
        const int lens[8] = {g.agc_len, g.cv_len, g.cv_len, g.ma1_len, g.ma1_len, g.mav1_len, g.fa_len, g.bt_len};
        const long long total = c->nsamples_total;
        if (n > lens[ring] || first < total - lens[ring] || first > total - n)
            return fail(JAERO_EINVAL, "jaero_debug_burst_front_peek: samples [%lld, %lld + %d) are not all among the last %d before sample %lld", first, first, n, lens[ring], total);
        if ((rc = burst_ring_column(rings[ring], lens[ring], ch, first, n, ring_out, false))) return rc;
    }
    if (out)
    {
        const std::pair<int, double *> d[] = {{BS_AGC_SUM, &out->agc_sum}, {BS_MA1_RE, &out->ma1_re}, {BS_MA1_IM, &out->ma1_im}, {BS_MAV1_SUM, &out->mav1_sum},
                                              {BS_LASTDY, &out->lastdy}};
        const std::pair<int, int *> q[] = {{BI_CNTDOWN, &out->cntdown}, {BI_MAXPOSCD, &out->maxposcd}, {BI_TRI_PTR, &out->tri_ptr}, {BI_EV_POS, &out->ev_pos},
                                           {BI_EV_CNT, &out->ev_cnt}, {BI_BT_HOLD, &out->bt_hold}};
        if ((rc = peek_fields(p.S, nchp, ch, d)) || (rc = peek_fields(p.I, nchp, ch, q))) return rc;
    }
    return 0;
}
extern "C" int jaero_debug_burst_front_events(jaero_ctx *c, int ch, double *rows, int caprows, int *nrows)
{
    if (!rows || !nrows || caprows < 0) return fail(JAERO_EINVAL, "jaero_debug_burst_front_events: null output or negative capacity");
    int rc = burst_front_enter(c, "jaero_debug_burst_front_events", ch, false);
    if (rc) return rc;
    const BGeom &g = c->bg;
    int cnt = 0;
    HIPCHK(hipMemcpy(&cnt, c->bp.I + (size_t)BI_EV_CNT * g.nchp + ch, sizeof(int), hipMemcpyDeviceToHost));
    if (cnt < 0 || cnt > g.ev_cap) return fail(JAERO_EHIP, "jaero_debug_burst_front_events: channel %d counts %d rows in a log of %d", ch, cnt, g.ev_cap);
    *nrows = cnt;
    const int take = cnt < caprows ? cnt : caprows;
    if (take) HIPCHK(hipMemcpy(rows, c->bp.evlog + (size_t)ch * g.ev_cap * 3, sizeof(double) * 3 * (size_t)take, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int jaero_debug_burst_front_poke(jaero_ctx *c, int ch, int field, double value)
{
    if (c && c->burst)
    {
        const BGeom &g = c->bg;
        const double lo[5] = {0, -1, 0, 0, 0}, hi[5] = {2.0 * g.PL, 2.0 * g.PL, g.tri_sz + 1.0, (double)g.bt_lag, 0};
        const bool ok = field == JAERO_FRONT_LASTDY ? std::isfinite(value)
                                                    : field >= 0 && field < JAERO_FRONT_LASTDY && value >= lo[field] && value <= hi[field] && value == (double)(int)value;
        if (!ok) return fail(JAERO_EINVAL, "jaero_debug_burst_front_poke: field %d cannot take the value %g", field, value);
    }
    int rc = burst_front_enter(c, "jaero_debug_burst_front_poke", ch, true);
    if (rc) return rc;
    const int nchp = c->bg.nchp;
    if (field == JAERO_FRONT_LASTDY)
    {
        HIPCHK(hipMemcpy(c->bp.S + (size_t)BS_LASTDY * nchp + ch, &value, sizeof(double), hipMemcpyHostToDevice));
        return 0;
    }
    const int fld[4] = {BI_CNTDOWN, BI_MAXPOSCD, BI_TRI_PTR, BI_BT_HOLD};
    const int v = (int)value;
    HIPCHK(hipMemcpy(c->bp.I + (size_t)fld[field] * nchp + ch, &v, sizeof(int), hipMemcpyHostToDevice));
    if (field == JAERO_FRONT_BT_HOLD && c->bt_hold_left < v) c->bt_hold_left = v; // the launch line's upper bound of every lane's counter
    return 0;
}
extern "C" int jaero_debug_burst_poke_bt(jaero_ctx *c, int ch, long long first, int n, const double *values)
{
    if (!values) return fail(JAERO_EINVAL, "jaero_debug_burst_poke_bt: null input");
    if (c && c->burst && (n <= 0 || n > c->bg.bt_len || first < -(1LL << 40) || first > (1LL << 40)))
        return fail(JAERO_EINVAL, "jaero_debug_burst_poke_bt: n %d (1 .. bt_len %d samples from an index within +- 2^40)", n, c->bg.bt_len);
    int rc = burst_front_enter(c, "jaero_debug_burst_poke_bt", ch, true);
    if (rc) return rc;
    return burst_ring_column(c->bp.bt, c->bg.bt_len, ch, first, n, const_cast<double *>(values), true);
}
extern "C" int jaero_debug_ev_compact(int device, const unsigned long long *masks, int ngroups, int *list_out, int *count_out)
{
    if (!masks || !list_out || !count_out || ngroups < 1 || ngroups > 65536)
        return fail(JAERO_EINVAL, "jaero_debug_ev_compact: ngroups %d (1 .. 65536 masks, a list of 64 entries for each and a count)", ngroups);
    int rc = open_device(device);
    if (rc) return rc;
    DevMem m;
    unsigned long long *d_mask = nullptr;
    int *d_list = nullptr, *d_count = nullptr;
    DA(m, d_mask, ngroups); DA(m, d_list, (size_t)ngroups * 64); DA(m, d_count, 4);
    HIPCHK(hipMemcpy(d_mask, masks, sizeof(unsigned long long) * (size_t)ngroups, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_list, 0xA5, sizeof(int) * (size_t)ngroups * 64));
    HIPCHK(hipMemset(d_count, 0xA5, sizeof(int)));
    if ((rc = burst_launch_ev_compact_on(d_mask, ngroups, d_list, d_count, 0))) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(list_out, d_list, sizeof(int) * (size_t)ngroups * 64, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(count_out, d_count, sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

// ------------------------------------------------------------------------------------------ test hooks: the tracking kernel alone
// (tests/test_gpu_burst_track.py), through burst_launch_demod as burst_write calls it.  track and track_fill poison the bank; track_geom,
// track_peek and track_read only read.  Peek and read reach the padding lanes of the last wavefront too; track's list does not.
extern "C" int jaero_debug_burst_track_geom(jaero_ctx *c, jaero_burst_track_geom *out)
{
    if (!out) return fail(JAERO_EINVAL, "jaero_debug_burst_track_geom: null output");
    int rc = burst_hook_enter(c, "jaero_debug_burst_track_geom", 0, false);
    if (rc) return rc;
    const BGeom &g = c->bg;
    out->D2 = g.D2; out->soft_cap = g.soft_cap; out->sym_cap = g.sym_cap; out->ev_cap = g.ev_cap; out->msema_len = g.msema_len; out->win_ring = g.win_ring;
    out->agc2_len = g.agc2_len; out->eb_len = g.eb_len; out->startstopstart = g.startstopstart;
    // the instantiation burst_create chose (c->bdemod)
    if (g.kind == JAERO_KIND_BURST_OQPSK) { out->firn = 55; out->ldsn = BD_LDSN; }
    else { out->firn = g.fir_n; out->ldsn = g.fir_n == 80 ? BMSK_FB_LDSN_80 : BMSK_FB_LDSN_160; }
    out->ebno_tail = JD_EBNO_TAIL;
    return 0;
}
extern "C" int jaero_debug_burst_track(jaero_ctx *c, int n, int first_of_write, const int *channels, const int *ev_pos, const jaero_trident_result *verdicts, int nlist)
{
    if (c && c->burst && (n <= 0 || n > c->bg.maxseg || n > c->max_write))
        return fail(JAERO_EINVAL, "jaero_debug_burst_track: n %d (one segment: 1 .. min(maxseg %d, max_write_samples %d) samples)", n, c->bg.maxseg, c->max_write);
    if (first_of_write != 0 && first_of_write != 1) return fail(JAERO_EINVAL, "jaero_debug_burst_track: first_of_write %d (0 or 1)", first_of_write);
    int rc = burst_hook_enter(c, "jaero_debug_burst_track", 0, false);
    if (rc) return rc;
    const BGeom &g = c->bg;
    const int nch = g.nch, nchp = g.nchp;
    if (nlist < 0 || nlist > nch || (nlist > 0 && (!channels || !ev_pos || !verdicts)))
        return fail(JAERO_EINVAL, "jaero_debug_burst_track: nlist %d (0 .. %d channels with their event positions and verdicts)", nlist, nch);
    std::vector<int> evp((size_t)nchp, -1);
    for (int k = 0; k < nlist; k++)
    {
        const int ch = channels[k];
        if (ch < 0 || ch >= nch || evp[(size_t)ch] >= 0)
            return fail(JAERO_EINVAL, "jaero_debug_burst_track: entry %d (channel %d) is outside [0, %d) or listed twice", k, ch, nch);
        if (ev_pos[k] < 0 || ev_pos[k] >= n) return fail(JAERO_EINVAL, "jaero_debug_burst_track: entry %d: event position %d outside [0, %d)", k, ev_pos[k], n);
        evp[(size_t)ch] = ev_pos[k];
    }
    hipStream_t st = c->last_stream;
    c->poisoned = true;
    HIPCHK(hipMemcpy(c->bp.I + (size_t)BI_EV_POS * nchp, evp.data(), sizeof(int) * (size_t)nchp, hipMemcpyHostToDevice));
    for (int k = 0; k < nlist; k++) HIPCHK(hipMemcpy(c->bp.tri + channels[k], &verdicts[k], sizeof(TriResult), hipMemcpyHostToDevice));
    if ((rc = burst_launch_demod(c, n, c->nsamples_total, first_of_write, st))) return rc;
    HIPCHK(hipStreamSynchronize(st));
    c->nsamples_total += n;
    return 0;
}
extern "C" int jaero_debug_burst_track_peek(jaero_ctx *c, int ch, jaero_burst_track_state *out)
{
    if (!out) return fail(JAERO_EINVAL, "jaero_debug_burst_track_peek: null output");
    int rc = burst_front_enter(c, "jaero_debug_burst_track_peek", ch, false);
    if (rc) return rc;
    const BPtrs &p = c->bp;
    const int nchp = c->bg.nchp;
    memset(out, 0, sizeof *out);
    const std::pair<int, int *> q[] = {{BI_STARTSTOP, &out->startstop}, {BI_CNTR, &out->cntr}, {BI_YUI, &out->yui}, {BI_INSERTPRE, &out->insertpre},
                                       {BI_NRX, &out->nrx}, {BI_SOFT_CNT, &out->soft_cnt}, {BI_SYM_CNT, &out->sym_cnt}, {BI_EV_CNT, &out->ev_cnt},
                                       {BI_OVERFLOW, &out->overflow}, {BI_MSEMA_POS, &out->msema_pos}, {BI_FIR_POS, &out->fir_pos}, {BI_EB_POS, &out->eb_pos},
                                       {BI_DLY_POS, &out->dly_pos}, {BI_D8_POS, &out->d8_pos}, {BI_A1_POS, &out->a1_pos}, {BI_GCNT, &out->gcnt}};
    const std::pair<int, double *> d[] = {{BS_MSE, &out->mse}, {BS_LASTMSE, &out->lastmse}, {BS_M2_FREQ, &out->m2_freq}, {BS_ST_FREQ, &out->st_freq},
                                          {BS_VOL_GAIN, &out->vol_gain}, {BS_EB_EBNO, &out->eb_ebno}, {BS_ROT_FREQ, &out->rot_freq}, {BS_AGC2_SUM, &out->agc2_sum},
                                          {BS_EB_ESUM, &out->eb_esum}, {BS_EB_E2SUM, &out->eb_e2sum}, {BS_MSEMA_SUM, &out->msema_sum}, {BS_MC_FREQ, &out->mc_freq},
                                          {BS_DIFF_LAST, &out->diff_last}, {BS_M2_PTR, &out->m2_ptr}, {BS_ST_PTR, &out->st_ptr}, {BS_STQ_PTR, &out->stq_ptr}};
    if ((rc = peek_fields(p.I, nchp, ch, q))) return rc;
    return peek_fields(p.S, nchp, ch, d);
}
extern "C" int jaero_debug_burst_track_fill(jaero_ctx *c, int soft_value, double sym_value)
{
    if (soft_value < -32768 || soft_value > 32767) return fail(JAERO_EINVAL, "jaero_debug_burst_track_fill: soft value %d is no int16", soft_value);
    int rc = burst_hook_enter(c, "jaero_debug_burst_track_fill", 0, true);
    if (rc) return rc;
    const BGeom &g = c->bg;
    std::vector<int16_t> soft((size_t)g.nchp * g.soft_cap, (int16_t)soft_value);
    HIPCHK(hipMemcpy(c->bp.soft, soft.data(), sizeof(int16_t) * soft.size(), hipMemcpyHostToDevice));
    if (g.sym_cap)
    {
        std::vector<double> sym((size_t)g.nchp * g.sym_cap * 3, sym_value);
        HIPCHK(hipMemcpy(c->bp.sym, sym.data(), sizeof(double) * sym.size(), hipMemcpyHostToDevice));
    }
    return 0;
}
extern "C" int jaero_debug_burst_track_read(jaero_ctx *c, int ch, int what, void *rows, int caprows)
{
    if (!rows || (what != 0 && what != 1)) return fail(JAERO_EINVAL, "jaero_debug_burst_track_read: null output or what %d (0 soft row, 1 symbol rows)", what);
    int rc = burst_front_enter(c, "jaero_debug_burst_track_read", ch, false);
    if (rc) return rc;
    const BGeom &g = c->bg;
    const int need = what == 0 ? g.soft_cap : g.sym_cap;
    if (caprows < need) return fail(JAERO_EINVAL, "jaero_debug_burst_track_read: room for %d rows, the channel's whole log has %d", caprows, need);
    if (what == 0) HIPCHK(hipMemcpy(rows, c->bp.soft + (size_t)ch * g.soft_cap, sizeof(int16_t) * (size_t)g.soft_cap, hipMemcpyDeviceToHost));
    else if (g.sym_cap) HIPCHK(hipMemcpy(rows, c->bp.sym + (size_t)ch * g.sym_cap * 3, sizeof(double) * 3 * (size_t)g.sym_cap, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int jaero_debug_burst_track_center_freq(jaero_ctx *c, int ch, double hz)
{
    if (!std::isfinite(hz)) return fail(JAERO_EINVAL, "jaero_debug_burst_track_center_freq: the frequency is not finite");
    int rc = burst_hook_enter(c, "jaero_debug_burst_track_center_freq", ch, false);
    if (rc) return rc;
    if (c->bg.kind != JAERO_KIND_BURST_MSK) return fail(JAERO_EINVAL, "jaero_debug_burst_track_center_freq: not a burst MSK bank (burst OQPSK's slot is empty)");
    c->poisoned = true;
    if ((rc = burst_launch_center_freq(c, ch, hz))) return rc;
    QUIESCE(c);
    return 0;
}
