// k_msk.h -- sample-loop kernel for the continuous 600/1200 bps MSK demodulator.
//
// Re-implements MskDemodulator::writeData's per-sample loop (JAERO/mskdemodulator.cpp:319-485) for 64 channels per
// wavefront, one channel per lane: coarse ring fill, NCO mix, half-sine matched filter (2*SPS taps),
// MSKEbNoMeasure (optional), AGC + clip, SPS-sample delayed arm, |pt_msk| -> resonator -> quadrature delay -> symbol
// PLL weighted by 1-|tanh(err)|, and at symbol instants the decision-directed carrier loop, residual rotation, MSE,
// soft differential decode (DiffDecode::UpdateSoft) and soft-bit demap.
//
// Runs the 40- and 20-tap filters (MSK at 24 and 12 kHz); 80 and 160 taps run on the front / back pairs of k_msk_fb.h.
// Layout of the matched-filter history: the newest LDSN inputs in an LDS ring, the older FIRN - LDSN in registers as a shift
// register, and this wavefront's copy of the taps in LDS behind the ring (msk_samples_lds_bytes).  The filter output of a sample does not contain that
// sample (the reference evaluates, then inserts), so it is evaluated one iteration ahead, and everything a sample reads
// from HBM (PCM, the rows leaving the AGC / EbNo windows, the two delay lines) is requested one iteration ahead too:
// written in reference order, every one of those reads was waited for on the spot, ~8 memory round trips per sample.
#pragma once
#include "jaero_device.h"
#include "demod_stages.h"

// dynamic LDS of k_msk_samples<FIRN, LDSN, ...>: the two rings [LDSN][64] and the taps
template <int FIRN, int LDSN>
constexpr int msk_samples_lds_bytes() { return (2 * LDSN * 64 + FIRN) * (int)sizeof(double); }

template <int FIRN, int LDSN, bool EBNO, bool CAPSYM>
__global__ __launch_bounds__(64) void k_msk_samples(const JGeom g, const JPtrs p, const int16_t *__restrict__ pcm, int pcm_stride,
                                                    int n, int skip_a_first, int only_a_last, int fir_slot0, int dly_slot0,
                                                    int d8_slot0)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *lre = lds;             // [LDSN][64]
    double *lim = lds + LDSN * 64; // [LDSN][64]
    constexpr int TAILN = FIRN - LDSN;
    constexpr int TAILA = TAILN > 0 ? TAILN : 1;
    double tre[TAILA], tim[TAILA]; // tre[j] = x_re[n-LDSN-j] once x[n] has been pushed

    const int lane = threadIdx.x;
    const int grp = blockIdx.x;
    const int ch = grp * 64 + lane;
    const int nchp = g.nchp;
    const bool live = ch < g.nch;
    const double2 *__restrict__ cis = p.cis;
    const double *__restrict__ taps = p.taps2; // this bank's own taps, read once into LDS

    double m2_ptr = LDF(S_M2_PTR), m2_step = LDF(S_M2_STEP), m2_freq = LDF(S_M2_FREQ);
    double mc_ptr = LDF(S_MC_PTR), mc_step = LDF(S_MC_STEP);
    double st_ptr = LDF(S_ST_PTR), st_step = LDF(S_ST_STEP), st_last = LDF(S_ST_LAST);
    double agc_sum = LDF(S_AGC_SUM);
    double eb_esum = LDF(S_EB_ESUM), eb_e2sum = LDF(S_EB_E2SUM), eb_ebno = LDF(S_EB_EBNO);
    double res_x1 = LDF(S_RES_X1), res_x2 = LDF(S_RES_X2), res_y1 = LDF(S_RES_Y1), res_y2 = LDF(S_RES_Y2);
    double marg_sum = LDF(S_MARG_SUM), msema_sum = LDF(S_MSEMA_SUM), mse = LDF(S_MSE);
    double diff_last = LDF(S_DIFF_LAST);

    int agc_pos = LDI(I_AGC_POS), bb_ptr = LDI(I_BB_PTR), coarse_cnt = LDI(I_COARSE_CNT);
    int marg_pos = LDI(I_MARG_POS), dt_pos = LDI(I_DT_POS), msema_pos = LDI(I_MSEMA_POS);
    const int flags = LDI(I_FLAGS);
    const bool dcd = flags & JF_DCD;
    int soft_cnt = LDI(I_SOFT_CNT), sym_cnt = LDI(I_SYM_CNT), overflow = LDI(I_OVERFLOW);

    const JdAtanLane atl = jd_atan_lane_table(lane); // jd_atan2's table, one entry per lane (every lane of the wavefront runs the sample loop)
    const double samplerate = g.Fs;
    const int nfft_mask = g.nfft - 1;
    double2 *__restrict__ bbring = p.bbring + (size_t)ch * g.nfft;
    // ONE ring of |sig2| values: the AGC's buffer, the EbNo meter's E buffer and, squared, its E2 buffer (k_msk_fb.h)
    double *__restrict__ win = p.win + (size_t)grp * g.win_len * 64 + lane;
    auto wslot = [&](int pos, int lag) { const int q = pos - lag; return q < 0 ? q + g.win_len : q; };
    double *__restrict__ marg_ring = p.marg + (size_t)ch * g.marg_len;
    double2 *__restrict__ dt_ring = p.dt + (size_t)ch * g.dt_len;
    double *__restrict__ msema_ring = p.msema + (size_t)ch * g.msema_len;
    int16_t *__restrict__ soft = p.soft + (size_t)ch * g.soft_cap;
    const int dly_len = g.sps + 1, d8_len = g.sps2 + 1;
    double2 *__restrict__ dly_ring = p.dly + (size_t)grp * dly_len * 64 + lane;
    double *__restrict__ d8_ring = p.dly8 + (size_t)grp * d8_len * 64 + lane;

    stg_hist_load<FIRN, LDSN, TAILN>(p.firsave + (size_t)grp * 2 * FIRN * 64 + lane, lre, lim, lane, tre, tim);
    int fir_slot = fir_slot0, dly_slot = dly_slot0, d8_slot = d8_slot0; // wave-uniform ring phases
    const double agc_len_d = (double)g.agc_len, eb_len_d = (double)g.ebno_len;

    // filter output for the current sample from the history x[n-FIRN .. n-1]: taps[i] <-> x[n-FIRN+i], oldest first (jd_fir_eval)
    double *ltap = lds + 2 * LDSN * 64; // [FIRN] this wavefront's copy of the taps
    for (int k = lane; k < FIRN; k += 64) ltap[k] = taps[k];
    auto fir_eval = [&](double &ore, double &oim) { jd_fir_eval<FIRN, LDSN, 8>(lre, lim, ltap, tre, tim, fir_slot, lane, ore, oim); };
    double ycur_re, ycur_im;
    fir_eval(ycur_re, ycur_im);

    // inputs of sample i+1 are requested at the top of iteration i (see the file header)
    auto ring_next = [](int pos, int len) { pos++; return pos >= len ? 0 : pos; };
    short nx_pcm = (live && n > 0) ? pcm[ch] : (short)0;
    double nx_agc = win[(size_t)wslot(agc_pos, g.agc_len) * 64];
    double nx_e = 0, nx_e2 = 0;
    if (EBNO) { nx_e = win[(size_t)wslot(agc_pos, g.ebno_len) * 64]; nx_e2 = nx_e * nx_e; }
    double2 nx_cc = cis[jd_cisidx(mc_ptr)];
    double2 nx_ptd = dly_ring[(size_t)ring_next(dly_slot, dly_len) * 64]; // slot read after this sample's write to dly_slot
    double nx_d8 = d8_ring[(size_t)ring_next(d8_slot, d8_len) * 64];

    for (int i = 0; i < n; i++)
    {
        const short s = nx_pcm;
        const double dval = ((double)s) / 32768.0;
        const double agc_old = nx_agc, e_old = nx_e, e2_old = nx_e2, d8out = nx_d8;
        const double2 ptd = nx_ptd;
        // this iteration's table look-ups and next iteration's streams, all independent of the chain below
        const double2 c2 = cis[jd_cisidx(m2_ptr)];
        const double2 c_st = cis[jd_cisidx(st_ptr)];
        if (i + 1 < n)
        {
            nx_pcm = live ? pcm[(size_t)(i + 1) * pcm_stride + ch] : (short)0;
            const int wn = ring_next(agc_pos, g.win_len);
            nx_agc = win[(size_t)wslot(wn, g.agc_len) * 64];
            if (EBNO) { nx_e = win[(size_t)wslot(wn, g.ebno_len) * 64]; nx_e2 = nx_e * nx_e; }
            nx_ptd = dly_ring[(size_t)ring_next(ring_next(dly_slot, dly_len), dly_len) * 64]; // dly_len, d8_len >= 3
            nx_d8 = d8_ring[(size_t)ring_next(ring_next(d8_slot, d8_len), d8_len) * 64];
        }

        // coarse-frequency ring fill (mskdemodulator.cpp:350-355)
        const double2 cc = nx_cc; // table entry of mixer_center for this sample, requested one iteration ago
        {
            double mcn = mc_ptr, mcs = mc_step;
            jd_wt_next(mcn, mcs); // nothing but WTnextFrame moves mixer_center inside a launch
            nx_cc = cis[jd_cisidx(mcn)];
        }
        if (!(i == 0 && skip_a_first))
        {
            const bool fill = (coarse_cnt >= g.Fs_int) || !(flags & JF_CPUREDUCE);
            if (fill)
            {
                bbring[bb_ptr] = make_double2(cc.x * dval, cc.y * dval);
                bb_ptr = (bb_ptr + 1) & nfft_mask;
            }
        }
        if (i == n - 1 && only_a_last) break;
        coarse_cnt++; // :368

        // mix + matched filter (:369-370): this sample's output was evaluated one iteration ago; x[n] is pushed at the end
        double sre = ycur_re, sim = ycur_im;
        // MSKEbNoMeasure::Update, AGC + clip (:375-382)
        stg_msk_meter_agc_clip<EBNO>(sre, sim, agc_old, e_old, e2_old, i >= n - JD_EBNO_TAIL /* wave-uniform */, eb_len_d, agc_len_d, eb_esum, eb_e2sum,
                                     eb_ebno, agc_sum, win, agc_pos, g.win_len);
        // the SPS-sample delayed arm and symbol timing (:384-405); ptd and d8out were requested one iteration ago
        double q_re, q_im; // pt_msk
        stg_msk_timing(g, sre, sim, ptd, d8out, c_st, dcd, atl, dly_ring, dly_slot, dly_len, d8_ring, d8_slot, d8_len, res_x1, res_x2, res_y1, res_y2,
                       st_ptr, q_re, q_im);

        double frac;
        if (jd_wt_passed(st_last, st_ptr, st_step, g.ee, frac))
        {
            // entries leaving the three symbol-rate windows (per-channel arrays in HBM), requested together ahead of their use
            const double marg_old = marg_ring[marg_pos];
            int dn = dt_pos + 1; if (dn >= g.dt_len) dn = 0;
            const double2 dt_old = dt_ring[dn]; // dt_len = SPS/2 + 1 > 1
            const double ms_old = msema_ring[msema_pos];
            const double ct_ec = stg_msk_carrier(g, sre, sim, ptd, dcd, samplerate, m2_ptr, m2_freq, m2_step);
            stg_msk_output_half<CAPSYM>(g, p, ch, ct_ec, q_re, q_im, marg_old, dt_old, ms_old, marg_ring, dt_ring, msema_ring, soft, marg_sum, marg_pos,
                                        dt_pos, msema_sum, msema_pos, mse, diff_last, soft_cnt, sym_cnt, overflow);
        }

        // push x[n] (mixed with the carrier phase this sample started with) and evaluate the filter for n+1
        {
            const double cre = c2.x * dval, cim = c2.y * dval;
#pragma unroll
            for (int j = TAILN - 1; j > 0; j--) { tre[j] = tre[j - 1]; tim[j] = tim[j - 1]; }
            if (TAILN > 0)
            {
                tre[0] = lre[fir_slot * 64 + lane];
                tim[0] = lim[fir_slot * 64 + lane];
            }
            lre[fir_slot * 64 + lane] = cre;
            lim[fir_slot * 64 + lane] = cim;
            fir_slot++;
            if (fir_slot >= LDSN) fir_slot = 0;
            fir_eval(ycur_re, ycur_im);
        }

        jd_wt_next(m2_ptr, m2_step);
        jd_wt_next(mc_ptr, mc_step);
        jd_wt_next_symbol(st_ptr, st_step, st_last);
    }

    LDF(S_M2_PTR) = m2_ptr; LDF(S_M2_STEP) = m2_step; LDF(S_M2_FREQ) = m2_freq;
    LDF(S_MC_PTR) = mc_ptr; LDF(S_MC_STEP) = mc_step;
    LDF(S_ST_PTR) = st_ptr; LDF(S_ST_STEP) = st_step; LDF(S_ST_LAST) = st_last;
    LDF(S_AGC_SUM) = agc_sum;
    LDF(S_EB_ESUM) = eb_esum; LDF(S_EB_E2SUM) = eb_e2sum; LDF(S_EB_EBNO) = eb_ebno;
    LDF(S_RES_X1) = res_x1; LDF(S_RES_X2) = res_x2; LDF(S_RES_Y1) = res_y1; LDF(S_RES_Y2) = res_y2;
    LDF(S_MARG_SUM) = marg_sum; LDF(S_MSEMA_SUM) = msema_sum; LDF(S_MSE) = mse;
    LDF(S_DIFF_LAST) = diff_last;
    LDI(I_AGC_POS) = agc_pos; LDI(I_BB_PTR) = bb_ptr; LDI(I_COARSE_CNT) = coarse_cnt;
    LDI(I_MARG_POS) = marg_pos; LDI(I_DT_POS) = dt_pos; LDI(I_MSEMA_POS) = msema_pos;
    LDI(I_SOFT_CNT) = soft_cnt; LDI(I_SYM_CNT) = sym_cnt; LDI(I_OVERFLOW) = overflow;
    stg_hist_save<FIRN, LDSN, TAILN>(p.firsave + (size_t)grp * 2 * FIRN * 64 + lane, lre, lim, lane, tre, tim);
}
