// k_burst_demod.h -- consumer side of the burst demodulators: the tracking chains, one channel per lane.
//   k_burst_oqpsk_demod : JAERO/burstoqpskdemodulator.cpp:488-515 (trident result applied), :517-733
//   (burst MSK: k_burst_msk_fb.h)
// Input is val_to_demod = real(cv[n - D1 - D2]) from the ring k_burst_front filled; the trident verdict for the event sample of
// this segment (if any) was computed by k_trident between the two launches.
#pragma once
#include "burst_device.h"
#include "jaero_device.h"
#include "demod_stages.h"
#include "k_burst_front.h"

__device__ __forceinline__ void bd_event(const BGeom &g, const BPtrs &p, int ch, int &ev_cnt, int &overflow, long long sample, int kind, double value)
{
    if (ev_cnt < g.ev_cap)
    {
        double *e = p.evlog + ((size_t)ch * g.ev_cap + ev_cnt) * 3;
        e[0] = (double)sample; e[1] = (double)kind; e[2] = value;
        ev_cnt++;
    }
    else overflow |= 4;
}
// BurstMskDemodulator::CenterFreqChangedSlot (JAERO/burstmskdemodulator.cpp:327-342; wired to the spectrum display, mainwindow.cpp:415)
// for channels [ch_lo, ch_lo + n): the same lines k_burst_msk_demod runs when a trident verdict retunes it, plus the slot's Plottables
// emission, stamped with the first sample of the write that follows.
__global__ void k_burst_msk_center_freq(const BGeom g, const BPtrs p, int ch_lo, int n, double freq_center, long long sample)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x, nchp = g.nchp;
    if (k >= n) return;
    const int ch = ch_lo + k;
    double m2_freq = BLDF(BS_M2_FREQ), m2_step = BLDF(BS_M2_STEP);
    const double lockingbw = BLDF(BS_LOCKINGBW);
    const bool afc = BLDI(BI_FLAGS) & JF_AFC;
    int ev_cnt = BLDI(BI_EV_CNT), overflow = BLDI(BI_OVERFLOW);
    double fc = freq_center;
    if (fc < (0.75 * g.fb)) fc = 0.75 * g.fb;
    if (fc > (g.Fs / 2.0 - 0.75 * g.fb)) fc = g.Fs / 2.0 - 0.75 * g.fb;
    double mc_freq = fc; if (mc_freq < 0) mc_freq = 0; // WaveTable::SetFreq
    if (afc) jd_wt_setfreq(m2_freq, m2_step, mc_freq, g.Fs);
    if ((m2_freq - mc_freq) > (lockingbw / 2.0)) jd_wt_setfreq(m2_freq, m2_step, mc_freq + (lockingbw / 2.0), g.Fs);
    if ((m2_freq - mc_freq) < (-lockingbw / 2.0)) jd_wt_setfreq(m2_freq, m2_step, mc_freq - (lockingbw / 2.0), g.Fs);
    bd_event(g, p, ch, ev_cnt, overflow, sample, BEV_FREQ, m2_freq);
    BLDF(BS_MC_FREQ) = mc_freq; BLDF(BS_M2_FREQ) = m2_freq; BLDF(BS_M2_STEP) = m2_step;
    BLDI(BI_EV_CNT) = ev_cnt; BLDI(BI_OVERFLOW) = overflow;
}
__device__ __forceinline__ void bd_cmul(double &ar, double &ai, double br, double bi)
{
    const double r = ar * br - ai * bi, i = ar * bi + ai * br;
    ar = r; ai = i;
}

// Arithmetic policy of this kernel: fused matched filter + the device library's hypot / atan2.  The A/B build
// (make -C jaero_amd/csrc ab_burst -> gpurun_tmp/libjaero_hip_burstexact.so, -DJD_BURST_EXACT) takes the continuous kernels' arithmetic instead --
// filter op for op, glibc's hypot, correctly rounded atan2 -- so that scripts/burst_recording_ab.py can count on the reference's own off-air
// recording what the choice moves (round 6: profiles/r6_burst_recording_ab.json).
#define BD_LDSN 36 // filter history slots in LDS (39 until round 6): six blocks of six for the filter's ring reads (JdRingBlocks)
#define BD_BS 6
static_assert(BD_LDSN % BD_BS == 0 && BD_BS <= 6, "ring blocks: k_burst_oqpsk_demod's switch has six cases");
#ifdef JD_BURST_EXACT
#define BD_FUSED false
#define BD_HYPOT(x, y) jd_hypot(x, y)
#define BD_ATAN2(y, x) jd_atan2(y, x, bd_atl)
#else
#define BD_FUSED true
#define BD_HYPOT(x, y) hypot(x, y)
#define BD_ATAN2(y, x) atan2(y, x)
#endif
// dynamic LDS of k_burst_oqpsk_demod: the two rings [BD_LDSN][64] and the 55 taps (64 slots): 37 376 B, four wavefronts per CU
constexpr int bd_lds_bytes() { return (2 * BD_LDSN * 64 + 64) * (int)sizeof(double); }
template <bool CAPSYM>
__global__ __launch_bounds__(64) void k_burst_oqpsk_demod(const BGeom g, const BPtrs p, int n, long long n0, int first_of_write)
{
    // matched-filter history as in k_oqpsk_fb.h: the LDSN newest entries of each arm in LDS ([slot][lane]), the FIRN-LDSN oldest in a
    // VGPR shift register, plus this wavefront's copy of the taps (jd_fir_sum) -> 36.5 KiB of LDS per wavefront (bd_lds_bytes), four per CU
    constexpr int FIRN = 55, LDSN = BD_LDSN, TAILN = FIRN - LDSN;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *lre = lds, *lim = lds + LDSN * 64, *ltap = lds + 2 * LDSN * 64;
    double tre[TAILN], tim[TAILN];
    const int lane = threadIdx.x, grp = blockIdx.x, ch = grp * 64 + lane, nchp = g.nchp;
    const double2 *__restrict__ cis = p.cis;
    const double *__restrict__ taps = p.taps2; // this bank's own taps, read once into LDS
    const double SPS = g.SPS, samplerate = g.Fs;
#ifdef JD_BURST_EXACT
    const JdAtanLane bd_atl = jd_atan_lane_table(lane);
#endif

    double m2_ptr = BLDF(BS_M2_PTR), m2_step = BLDF(BS_M2_STEP), m2_freq = BLDF(BS_M2_FREQ);
    double st_ptr = BLDF(BS_ST_PTR), st_step = BLDF(BS_ST_STEP), st_freq = BLDF(BS_ST_FREQ), st_last = BLDF(BS_ST_LAST);
    double stq_ptr = BLDF(BS_STQ_PTR), vol_gain = BLDF(BS_VOL_GAIN);
    double str_re = BLDF(BS_STR_RE), str_im = BLDF(BS_STR_IM), sav_re = BLDF(BS_SAV_RE), sav_im = BLDF(BS_SAV_IM);
    double rot_re = BLDF(BS_ROT_RE), rot_im = BLDF(BS_ROT_IM), rot_freq = BLDF(BS_ROT_FREQ);
    // cis(rot_freq), formed where rot_freq changes (verdict, symbol instants) instead of in every sample: the same function of the same
    // argument, off the per-sample chain (the instant block runs in nearly every sample anyway, and there this sincos overlaps the other one)
    double rfs, rfc;
    sincos(rot_freq, &rfs, &rfc);
    double a1_1 = BLDF(BS_A1_1), a1_2 = BLDF(BS_A1_2), a1_3 = BLDF(BS_A1_3), a1_4 = BLDF(BS_A1_4), a1_5 = BLDF(BS_A1_5);
    double agc2_sum = BLDF(BS_AGC2_SUM), eb_esum = BLDF(BS_EB_ESUM), eb_e2sum = BLDF(BS_EB_E2SUM), eb_ebno = BLDF(BS_EB_EBNO);
    double d1 = BLDF(BS_D1), d41_1 = BLDF(BS_D41_1), d41_2 = BLDF(BS_D41_2), d41_3 = BLDF(BS_D41_3);
    double d42_1 = BLDF(BS_D42_1), d42_2 = BLDF(BS_D42_2), d42_3 = BLDF(BS_D42_3), d8_1 = BLDF(BS_D8_1), d8_2 = BLDF(BS_D8_2);
    double res_x1 = BLDF(BS_RES_X1), res_x2 = BLDF(BS_RES_X2), res_y1 = BLDF(BS_RES_Y1), res_y2 = BLDF(BS_RES_Y2);
    double sig2l_re = BLDF(BS_SIG2L_RE), sig2l_im = BLDF(BS_SIG2L_IM), ptd_re = BLDF(BS_PTD_RE), ptd_im = BLDF(BS_PTD_IM);
    double ptd_th = jd_tanh(ptd_re); // kept beside ptd_re inside a launch; formed again here rather than stored
    double msema_sum = BLDF(BS_MSEMA_SUM), mse = BLDF(BS_MSE), lastmse = BLDF(BS_LASTMSE);
    const double thresh = BLDF(BS_THRESH);
    if (first_of_write) lastmse = mse; // double lastmse=mse at the top of writeDataSlot (:318)

    int startstop = BLDI(BI_STARTSTOP), cntr = BLDI(BI_CNTR), yui = BLDI(BI_YUI), insertpre = BLDI(BI_INSERTPRE);
    int msema_pos = BLDI(BI_MSEMA_POS), nrx = BLDI(BI_NRX);
    int soft_cnt = BLDI(BI_SOFT_CNT), sym_cnt = BLDI(BI_SYM_CNT), ev_cnt = BLDI(BI_EV_CNT), overflow = BLDI(BI_OVERFLOW);
    const int flags = BLDI(BI_FLAGS);
    const int ev_pos = BLDI(BI_EV_POS);
    const bool trace = (g.flags & 8u) != 0;

    const double *__restrict__ cvre = p.cvre + (size_t)grp * g.cv_len * 64 + lane;
    // ONE ring of |sig2|: ebnomeasure->Update(sig2abs) and agc2->Update(sig2abs) (:570,:576) are fed the same value in the same samples and both
    // start from empty windows at the same moments (constructor, setSettings), so AGC2's moving-average buffer is the newest agc2_len
    // entries of E's, and E2's entries are E's squared (MovingAverage::Update stores fabs(sig), DSP.cpp:408-416: fabs(x)^2 == fabs(x x))
    double *ebe_ring = p.eb_e + (size_t)grp * g.win_ring * 64 + lane;
    double *msema_ring = p.msema + (size_t)ch * g.msema_len;
    int16_t *__restrict__ soft = p.soft + (size_t)ch * g.soft_cap;

    stg_hist_load<FIRN, LDSN, TAILN>(p.firsave + (size_t)grp * 2 * FIRN * 64 + lane, lre, lim, lane, tre, tim);
    if (lane < FIRN) ltap[lane] = taps[lane];
    const int tapz = jd_vzero(); // tap reads become `register + immediate offset` (JdRingBlocks)
    int fir_slot = (int)(n0 % LDSN), s_eb = (int)(n0 % g.win_ring);
    int s_agc2 = s_eb - g.agc2_len; if (s_agc2 < 0) s_agc2 += g.win_ring; // the entry written agc2_len samples ago (slot s_eb itself holds the one written win_ring ago)
    int s_e = s_eb - g.eb_len; if (s_e < 0) s_e += g.win_ring;             // the entry written eb_len samples ago
    int s_val = (int)((n0 - g.D1 - g.D2 + 8LL * g.cv_len) % g.cv_len);
    const double w4 = g.w4, w4c = 1.0 - g.w4, w8 = g.w8, w8c = 1.0 - g.w8, a1w = g.a1_w, a1wc = 1.0 - g.a1_w;
    const double agc2_len_d = (double)g.agc2_len, eb_len_d = (double)g.eb_len;
    // divisions by these constants: reciprocal + two fma corrections (jd_div_const, bit-identical to the quotient)
    const double r_agc2_len = 1.0 / agc2_len_d, r_samplerate = 1.0 / samplerate, r_360 = 1.0 / 360.0, wtsize_d = (double)JD_WTSIZE, r_wtsize = 1.0 / wtsize_d;
    const double msema_len_d = (double)g.msema_len, r_msema_len = 1.0 / msema_len_d;

    // ring entries of sample i+1 are requested at the top of iteration i (all slots are wave-uniform and data independent)
    double nx_val = cvre[(size_t)s_val * 64], nx_agc2 = ebe_ring[(size_t)s_agc2 * 64];
    double nx_e = ebe_ring[(size_t)s_e * 64];
    for (int i = 0; i < n; i++)
    {
        const long long sample = n0 + i;
        const double val = nx_val, agc2_old = nx_agc2, e_old = nx_e, e2_old = nx_e * nx_e;
        if (i + 1 < n)
        {
            int sv = s_val + 1; if (sv >= g.cv_len) sv = 0;
            int sa = s_agc2 + 1; if (sa >= g.win_ring) sa = 0;
            int se = s_e + 1; if (se >= g.win_ring) se = 0;
            nx_val = cvre[(size_t)sv * 64]; nx_agc2 = ebe_ring[(size_t)sa * 64];
            nx_e = ebe_ring[(size_t)se * 64];
        }
        // ---- trident verdict for this sample (:488-515) ----
        if (i == ev_pos)
        {
            const TriResult tr = p.tri[ch];
            if (trace) bd_event(g, p, ch, ev_cnt, overflow, sample, BEV_TRIDENT, tr.ok ? tr.metric : -tr.metric);
            if (tr.ok)
            {
                jd_wt_setfreq(m2_freq, m2_step, tr.freq, samplerate);
                bd_set_phase_deg(m2_ptr, tr.phase_deg);
                bd_event(g, p, ch, ev_cnt, overflow, sample, BEV_FREQ, m2_freq);
                vol_gain = tr.vol_gain;
                jd_wt_setfreq(st_freq, st_step, g.stref_freq, samplerate);
                bd_set_phase_deg(st_ptr, 0);
                res_x1 = res_x2 = res_y1 = res_y2 = 0;
                startstop = g.startstopstart;
                cntr = 0;
                rot_re = 1; rot_im = 0;
                insertpre = 1;
                rot_freq = 0; rfs = 0.0; rfc = 1.0; // = sincos(0)
                sav_re = 1; sav_im = 0;
                bd_event(g, p, ch, ev_cnt, overflow, sample, BEV_SIGNAL, 1.0);
                mse = 0;
                for (int k = 0; k < g.msema_len; k++) msema_ring[k] = 0;
                msema_pos = 0; msema_sum = 0;
            }
        }
        // ---- mix + rrc (:517-521) ----
        const double2 c2 = cis[jd_cisidx(m2_ptr)];
        // the symbol oscillator's table entry, needed by the timing loop far below: requested here, under the matched filter (valid unless the
        // preamble block moves st_ptr in between; asked for where it is used it was an L2 round trip on every sample's chain)
        const double st_ptr_top = st_ptr;
        const double2 so_pre = cis[jd_cisidx(st_ptr)];
        const double xin = (vol_gain * val);
        const double cre = c2.x * xin, cim = c2.y * xin;
        double sre = 0, sim = 0;
        {
            // output from x[n-FIRN .. n-1] (FIR::FIRUpdateAndProcess excludes the sample being pushed): taps[i] <-> x[n-FIRN+i]
            // The block addresses and the switch of jd_fir_sum_blocks stay written out here, with one wrap-around subtraction and six plain
            // cases: through the shared dispatcher both instantiations of this kernel compile to longer listings (and, with one
            // subtraction there, 80 instead of 64 B of scratch): profiles/fir_refactor_isa.md.
            constexpr int NB = LDSN / BD_BS;
            int blk[NB + 1];
            const int ab = fir_slot / BD_BS; // wave-uniform
#pragma unroll
            for (int m = 0; m <= NB; m++)
            {
                int t = ab + m;
                if (t >= NB) t -= NB;
                blk[m] = t * BD_BS * 64 + lane;
            }
#define BD_V(B) case B: jd_fir_sum<FIRN, LDSN, 8, BD_FUSED, 0>(JdRingBlocks<LDSN, BD_BS, B, NB + 1>{lre, blk}, ltap, tapz, tre, tim, 0.0, 0.0, sre, sim); break;
            switch (fir_slot % BD_BS) { BD_V(0) BD_V(1) BD_V(2) BD_V(3) BD_V(4) BD_V(5) default: break; }
#undef BD_V
            // push x[n]: the oldest LDS entry moves into the register tail
#pragma unroll
            for (int j = TAILN - 1; j > 0; j--) { tre[j] = tre[j - 1]; tim[j] = tim[j - 1]; }
            tre[0] = lre[fir_slot * 64 + lane]; tim[0] = lim[fir_slot * 64 + lane];
            lre[fir_slot * 64 + lane] = cre; lim[fir_slot * 64 + lane] = cim;
            fir_slot++; if (fir_slot >= LDSN) fir_slot = 0;
        }
        // ---- sample counting and signal time-out (:523-544) ----
        if (startstop > 0)
        {
            startstop--;
            if (cntr < 1000000) cntr++;
            if (mse < 0.75) startstop = g.startstopstart;
        }
        if (startstop == 0) { startstop--; bd_event(g, p, ch, ev_cnt, overflow, sample, BEV_SIGNAL, 0.0); }
        if ((cntr > ((256 - 10) * SPS)) && insertpre)
        {
            if (soft_cnt < g.soft_cap) { soft[soft_cnt++] = (int16_t)-1; nrx++; } else overflow |= 1;
            insertpre = 0;
        }
        // ---- symbol tone in the preamble (:547-566) ----
        if ((cntr > SPS * (128 + 10)) && (cntr < ((256 - 10) * SPS)))
        {
            const double progress = (((double)cntr) - (SPS * (128 + 10))) / (((256 - 10) * SPS) - (SPS * (128 + 10)));
            double t_re = sre, t_im = sim;
            bd_cmul(t_re, t_im, str_re, str_im);
            bd_cmul(t_re, t_im, 0.0, 1.0);
            const double er = jd_tanh(t_im) * (t_re);
            double sn, cs;
            sincos(er * 0.01, &sn, &cs);
            bd_cmul(str_re, str_im, cs, sn);
            sav_re = sav_re * 0.95 + 0.05 * str_re; sav_im = sav_im * 0.95 + 0.05 * str_im;
            // a1.update(symboltone_pt.real()): Delay<double>(SPS/2): older = x[k-5], newer = x[k-4]
            const double a1out = a1w * a1_4 + a1wc * a1_5;
            a1_5 = a1_4; a1_4 = a1_3; a1_3 = a1_2; a1_2 = a1_1; a1_1 = t_re;
            t_im = a1out;
            const double2 cq = cis[jd_cisidx(stq_ptr)];
            const double e_re = cq.x * t_re - cq.y * (-t_im), e_im = cq.x * (-t_im) + cq.y * t_re;
            double st_err = BD_ATAN2(e_im, e_re);
            st_err *= 1.5 * (1.0 - progress * progress);
            jd_wt_advance_fraction(stq_ptr, -(1.0 / (2.0 * M_PI)) * st_err * 0.1);
            bd_set_phase_deg(st_ptr, jd_div_const(360.0 * stq_ptr, wtsize_d, r_wtsize) * 4.0 + (360.0 * g.ee));
        }
        // ---- carrier phase correction, EbNo, AGC, clip (:570-590) ----
        bd_cmul(sre, sim, sav_re, sav_im);
        bd_cmul(rot_re, rot_im, rfc, rfs);
        bd_cmul(sre, sim, rot_re, rot_im);
        const double sig2abs = BD_HYPOT(sre, sim);
        {
            const double sq = sig2abs * sig2abs;
            double *ep = ebe_ring + (size_t)s_eb * 64;
            eb_e2sum = eb_e2sum - e2_old; eb_e2sum = eb_e2sum + fabs(sq);
            eb_esum = eb_esum - e_old; eb_esum = eb_esum + fabs(sig2abs); *ep = fabs(sig2abs); // the one store: AGC2 below pushes the same value
            s_eb++; if (s_eb >= g.win_ring) s_eb = 0;
            s_e++; if (s_e >= g.win_ring) s_e = 0;
            // The meter's value is observable at the end of a launch (status) and once per burst, at cntr == 384 symbols (:581); its
            // IIR forgets a term after k samples as 0.8^k, so the divide/log10 runs only in the JD_EBNO_TAIL samples before either.
            const double to_emit = ((128.0 + 128.0 + 128.0) * SPS) - (double)cntr;
            if (i >= n - JD_EBNO_TAIL || (to_emit > -1.0 && to_emit < (double)JD_EBNO_TAIL))
                eb_ebno = stg_ebno_oqpsk(eb_ebno, eb_e2sum / eb_len_d, eb_esum / eb_len_d, g.Fs, g.fb);
        }
        if (fabs(cntr - ((128.0 + 128.0 + 128.0) * SPS)) < 0.5) bd_event(g, p, ch, ev_cnt, overflow, sample, BEV_EBNO, eb_ebno);
        {
            agc2_sum = agc2_sum - agc2_old; agc2_sum = agc2_sum + fabs(sig2abs);
            s_agc2++; if (s_agc2 >= g.win_ring) s_agc2 = 0;
            double gain = 1.414213562 / fmax(jd_div_const(agc2_sum, agc2_len_d, r_agc2_len), 0.000001);
            gain = fmax(gain, 0.000001);
            sre *= gain; sim *= gain;
        }
        const double abval = BD_HYPOT(sre, sim);
        if (abval > 2.84) { const double k = (2.84 / abval); sre = k * sre; sim = k * sim; }

        // ---- symbol timer (:592-612) ----
        double st_eta = stg_oqpsk_t4_pair(abval, d1, d41_1, d41_2, d41_3, d42_1, d42_2, d42_3, w4, w4c);
        {
            const double y = jd_biquad(st_eta, res_x1, res_x2, res_y1, res_y2, g.res_b0, g.res_b1, g.res_b2, g.res_a1, g.res_a2);
            if (cntr > SPS * (128 + 128)) st_eta = y;
        }
        const double d8out = w8 * d8_1 + w8c * d8_2; d8_2 = d8_1; d8_1 = st_eta;
        {
            double2 so = so_pre;
            if (st_ptr != st_ptr_top) so = cis[jd_cisidx(st_ptr)];
            const double m_re = st_eta, m_im = -d8out;
            const double o_re = so.x * m_re - so.y * m_im, o_im = so.x * m_im + so.y * m_re;
            const double st_angle_error = BD_ATAN2(o_im, o_re);
            if (cntr > SPS * (128 + 64))
            {
                fb_wt_setfreq(st_freq, st_step, (-st_angle_error * 0.00000001) + st_freq, samplerate, r_samplerate);
                jd_wt_advance_fraction(st_ptr, jd_div_const(-st_angle_error * 0.01, 360.0, r_360));
            }
            if (st_freq < (g.stref_freq - 0.1)) fb_wt_setfreq(st_freq, st_step, (g.stref_freq - 0.1), samplerate, r_samplerate);
            if (st_freq > (g.stref_freq + 0.1)) fb_wt_setfreq(st_freq, st_step, (g.stref_freq + 0.1), samplerate, r_samplerate);
        }
        // ---- sample times (:615-724) ----
        double frac;
        if (jd_wt_passed(st_last, st_ptr, st_step, g.ee, frac))
        {
            const double pt_last = frac, pt_this = 1.0 - pt_last;
            const double pt_re = pt_this * sre + pt_last * sig2l_re, pt_im = pt_this * sim + pt_last * sig2l_im;
            const double twospeed = -4.0 * (jd_div_const(fb_fmod360(jd_div_const(360.0 * stq_ptr, wtsize_d, r_wtsize) * 2.0 + (360.0 * g.ee * 0.5)), 360.0, r_360) - (0.34046 + 0.4111 * g.ee));
            const bool even = !(twospeed < 0);
            yui++; yui %= 2;
            if (cntr < ((128 + 128) * SPS))
            {
                if ((even && yui == 1) || (!even && yui == 0)) { yui++; yui %= 2; }
            }
            // one tanh per instant for both kinds of instant (k_oqpsk_fb.h, round 4): the earlier instant keeps tanh(ptd_re) beside ptd_re
            const double th = jd_tanh(yui ? pt_im : pt_re);
            if (!yui) { ptd_re = pt_re; ptd_im = pt_im; ptd_th = th; }
            else
            {
                const double q_re = pt_re, q_im = ptd_im;
                const double ct_xt = th * pt_re;
                const double ct_xt_d = ptd_th * ptd_im;
                double ct_ec = ct_xt_d - ct_xt;
                if (ct_ec > M_PI) ct_ec = M_PI;
                if (ct_ec < -M_PI) ct_ec = -M_PI;
                if (ct_ec > M_PI_2) ct_ec = M_PI_2;
                if (ct_ec < -M_PI_2) ct_ec = -M_PI_2;
                if (cntr > ((128 + 10) * SPS))
                {
                    double sn, cs;
                    sincos(ct_ec * 0.1, &sn, &cs);
                    bd_cmul(rot_re, rot_im, cs, sn);
                    rot_freq = rot_freq + ct_ec * 0.0001;
                    sincos(rot_freq, &rfs, &rfc);
                    const double tda = (fabs(q_re) - 1.0), tdb = (fabs(q_im) - 1.0);
                    const double e = (tda * tda) + (tdb * tdb);
                    double *mp = msema_ring + msema_pos;
                    msema_sum = msema_sum - *mp; msema_sum = msema_sum + fabs(e); *mp = fabs(e);
                    msema_pos++; if (msema_pos >= g.msema_len) msema_pos = 0;
                    mse = jd_div_const(msema_sum, msema_len_d, r_msema_len);
                }
                if (startstop > 0)
                {
                    if (CAPSYM)
                    {
                        if (sym_cnt < g.sym_cap) { double *sp = p.sym + ((size_t)ch * g.sym_cap + sym_cnt) * 3; sp[0] = q_re; sp[1] = q_im; sp[2] = mse; sym_cnt++; }
                        else overflow |= 2;
                    }
                    const int b0 = jd_softbit(0.75 * q_im * 127.0 + 128.0);
                    const int b1 = jd_softbit(0.75 * q_re * 127.0 + 128.0);
                    if (soft_cnt + 2 <= g.soft_cap) { soft[soft_cnt] = (int16_t)b0; soft[soft_cnt + 1] = (int16_t)b1; soft_cnt += 2; nrx += 2; }
                    else overflow |= 1;
                    if (nrx >= 32)
                    {
                        // emit unless squelched (:708-715); a squelched group is dropped
                        if (!(!(flags & JF_SQL) || mse < thresh || lastmse < thresh)) soft_cnt -= nrx;
                        nrx = 0;
                    }
                }
            }
        }
        sig2l_re = sre; sig2l_im = sim;
        // ---- advance the oscillators (:727-730) ----
        jd_wt_next(m2_ptr, m2_step);
        jd_wt_next_symbol(st_ptr, st_step, st_last);
        stq_ptr += g.stq_step;
        while (((int)stq_ptr) >= JD_WTSIZE) stq_ptr -= JD_WTSIZE;
        s_val++; if (s_val >= g.cv_len) s_val = 0;
    }

    BLDF(BS_M2_PTR) = m2_ptr; BLDF(BS_M2_STEP) = m2_step; BLDF(BS_M2_FREQ) = m2_freq;
    BLDF(BS_ST_PTR) = st_ptr; BLDF(BS_ST_STEP) = st_step; BLDF(BS_ST_FREQ) = st_freq; BLDF(BS_ST_LAST) = st_last;
    BLDF(BS_STQ_PTR) = stq_ptr; BLDF(BS_VOL_GAIN) = vol_gain;
    BLDF(BS_STR_RE) = str_re; BLDF(BS_STR_IM) = str_im; BLDF(BS_SAV_RE) = sav_re; BLDF(BS_SAV_IM) = sav_im;
    BLDF(BS_ROT_RE) = rot_re; BLDF(BS_ROT_IM) = rot_im; BLDF(BS_ROT_FREQ) = rot_freq;
    BLDF(BS_A1_1) = a1_1; BLDF(BS_A1_2) = a1_2; BLDF(BS_A1_3) = a1_3; BLDF(BS_A1_4) = a1_4; BLDF(BS_A1_5) = a1_5;
    BLDF(BS_AGC2_SUM) = agc2_sum; BLDF(BS_EB_ESUM) = eb_esum; BLDF(BS_EB_E2SUM) = eb_e2sum; BLDF(BS_EB_EBNO) = eb_ebno;
    BLDF(BS_D1) = d1; BLDF(BS_D41_1) = d41_1; BLDF(BS_D41_2) = d41_2; BLDF(BS_D41_3) = d41_3;
    BLDF(BS_D42_1) = d42_1; BLDF(BS_D42_2) = d42_2; BLDF(BS_D42_3) = d42_3; BLDF(BS_D8_1) = d8_1; BLDF(BS_D8_2) = d8_2;
    BLDF(BS_RES_X1) = res_x1; BLDF(BS_RES_X2) = res_x2; BLDF(BS_RES_Y1) = res_y1; BLDF(BS_RES_Y2) = res_y2;
    BLDF(BS_SIG2L_RE) = sig2l_re; BLDF(BS_SIG2L_IM) = sig2l_im; BLDF(BS_PTD_RE) = ptd_re; BLDF(BS_PTD_IM) = ptd_im;
    BLDF(BS_MSEMA_SUM) = msema_sum; BLDF(BS_MSE) = mse; BLDF(BS_LASTMSE) = lastmse;
    BLDI(BI_STARTSTOP) = startstop; BLDI(BI_CNTR) = cntr; BLDI(BI_YUI) = yui; BLDI(BI_INSERTPRE) = insertpre;
    BLDI(BI_MSEMA_POS) = msema_pos; BLDI(BI_NRX) = nrx;
    BLDI(BI_SOFT_CNT) = soft_cnt; BLDI(BI_SYM_CNT) = sym_cnt; BLDI(BI_EV_CNT) = ev_cnt; BLDI(BI_OVERFLOW) = overflow;
    stg_hist_save<FIRN, LDSN, TAILN>(p.firsave + (size_t)grp * 2 * FIRN * 64 + lane, lre, lim, lane, tre, tim);
}

// ------------------------------------------------------------------------------------------------ burst MSK
// k_burst_msk_fb.h (round 3): the tracking chain as a front / back wavefront pair.  The single-wavefront kernel k_burst_msk_demod lived here
// (rounds 1-2: 78 -> 43 ms per 4096-sample launch of 65 536 channels; what it taught is in that header and in DESIGN 10).
