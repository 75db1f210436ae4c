// demod_stages.h -- the demodulator stages more than one sample-loop kernel runs, written once.
//
// jaero_device.h holds the pure primitives (jd_*: a value in, a value out).  Here are the stages that carry a demodulator's state by
// reference (stg_*): each is the reference's text for that stage -- the same fp64 operations in the same order as the kernel bodies they
// were lifted from -- and nothing else.  The SCHEDULE stays in the kernels: what is requested ahead and when, which wavefront of a pair
// runs which stage, the mailboxes, the barriers, the deferred output queue, the state load / store lists.  A stage therefore takes the
// window and ring entries it consumes as arguments (its caller decides when they are loaded) and stores only what the reference's
// stage itself writes.  Stages whose operation sequence differs between kernels (OQPSK's AGC with jd_div_const and jd_hypot against
// MSK's `/` and sqrt, the burst kernels' hypot / atan2 policy) are NOT here: a stage that branches on its caller is worse than two copies.
#pragma once
#include "jaero_device.h"

// ---- matched-filter history: firsave <-> the LDS ring and the register tail ---------------------------------------------------------
// A group's saved history is [2][FIRN] entries STRIDE doubles apart (64: [entry][lane] rows, fs already offset by the lane; 1: the burst
// MSK kernel's per-channel layout): entries [0, LDSN) are the LDS ring's slots, [LDSN, LDSN + TAILN) the register tail, the second arm
// FIRN entries on.  TAILN may be less than FIRN - LDSN (k_msk_fb: the oldest entries are the back half's, which saves its own).
// TAILN is given, not taken from the arrays: their extent TAILA is only deduced and may be larger (a kernel without a register tail
// still declares one element, TAILN = 0).
template <int FIRN, int LDSN, int TAILN, int STRIDE = 64, int TAILA>
__device__ __forceinline__ void stg_hist_load(const double *fs, double *lre, double *lim, int lane, double (&tre)[TAILA], double (&tim)[TAILA])
{
    for (int k = 0; k < LDSN; k++)
    {
        lre[k * 64 + lane] = fs[(size_t)k * STRIDE];
        lim[k * 64 + lane] = fs[(size_t)(FIRN + k) * STRIDE];
    }
#pragma unroll
    for (int j = 0; j < TAILN; j++)
    {
        tre[j] = fs[(size_t)(LDSN + j) * STRIDE];
        tim[j] = fs[(size_t)(FIRN + LDSN + j) * STRIDE];
    }
}
template <int FIRN, int LDSN, int TAILN, int STRIDE = 64, int TAILA>
__device__ __forceinline__ void stg_hist_save(double *fs, const double *lre, const double *lim, int lane, const double (&tre)[TAILA],
                                              const double (&tim)[TAILA])
{
    for (int k = 0; k < LDSN; k++)
    {
        fs[(size_t)k * STRIDE] = lre[k * 64 + lane];
        fs[(size_t)(FIRN + k) * STRIDE] = lim[k * 64 + lane];
    }
#pragma unroll
    for (int j = 0; j < TAILN; j++)
    {
        fs[(size_t)(LDSN + j) * STRIDE] = tre[j];
        fs[(size_t)(FIRN + LDSN + j) * STRIDE] = tim[j];
    }
}

// ---- coarse ring fill, four entries at a time -----------------------------------------------------------------------------------------
// A 16-byte store into the per-channel ring is a quarter of a 64-byte sector; issued one per sample (3.5 us apart) every one of them cost
// the L2 a sector fill from HBM plus a sector write (measured: 23 GB written and 15 GB of extra reads per 4096-sample launch for 4.3 GB
// of ring entries).  The last three entries wait in registers and go out with the fourth, back to back, as one complete sector; what is
// left at the end of the launch (at most three) goes out singly (flush).
// k_oqpsk_fb calls this; k_msk_fb keeps the same text written out (as the struct it cost that kernel a spilled entry in its loop).
struct StgSectorQueue
{
    double2 q1, q2, q3; // entries waiting: the ring positions just below bb_ptr, q1 the newest
    int n;              // how many of them
    int bb_ptr;         // the ring's write position (I_BB_PTR)
    __device__ __forceinline__ explicit StgSectorQueue(int bb_ptr0) : q1(make_double2(0.0, 0.0)), q2(q1), q3(q1), n(0), bb_ptr(bb_ptr0) {}
    __device__ __forceinline__ void flush(double2 *__restrict__ bbring)
    {
        double2 *dst = bbring + bb_ptr;
        if (n >= 3) dst[-3] = q3;
        if (n >= 2) dst[-2] = q2;
        if (n >= 1) dst[-1] = q1;
        n = 0;
    }
    __device__ __forceinline__ void fill(double2 *__restrict__ bbring, int nfft_mask, const double2 v)
    {
        if ((bb_ptr & 3) == 3)
        {
            flush(bbring);
            bbring[bb_ptr] = v;
        }
        else
        {
            q3 = q2; q2 = q1; q1 = v;
            n++;
        }
        bb_ptr = (bb_ptr + 1) & nfft_mask;
    }
};

// ---- the EbNo meters' formulas --------------------------------------------------------------------------------------------------------
// e2val, mean = the two window sums ALREADY divided by the window length: the continuous OQPSK kernel divides with jd_div_const, the
// others with `/`, and that choice is the caller's.  Return the meter's new value.
// OQPSKEbNoMeasure::Update (JAERO/DSP.cpp:729-744)
__device__ __forceinline__ double stg_ebno_oqpsk(double eb_ebno, double e2val, double mean, double Fs, double fb)
{
    const double meansq = mean * mean;
    double var = e2val - (mean * mean);
    var -= (0.024709 * meansq);
    double mvr = (((Fs * meansq / (2.0 * fb * var))) * 0.13743);
    if (mvr < 0.000000001) mvr = 0.000000001;
    double tebno = 10.0 * log10(mvr);
    if (isnan(tebno)) tebno = 50;
    if (tebno > 50.0) tebno = 50;
    if (tebno < 0.0) tebno = 0;
    return eb_ebno * 0.8 + 0.2 * tebno;
}
// MSKEbNoMeasure::Update (JAERO/DSP.cpp:493-505)
__device__ __forceinline__ double stg_ebno_msk(double eb_ebno, double e2val, double mean)
{
    const double var = e2val - (mean * mean);
    const double alpha = sqrt(2.0) / mean;
    double tebno = 10.0 * (log10(2.0) - log10(((var * alpha * alpha) - 0.0085))) - 5.0;
    if (isnan(tebno)) tebno = 50;
    if (tebno > 50.0) tebno = 50;
    return eb_ebno * 0.8 + 0.2 * tebno;
}

// ---- OQPSK symbol timing: the T/4 - T/4 delay chain (oqpskdemodulator.cpp:473-484, burstoqpskdemodulator.cpp:592-612) ----------------
// |sig2|^2 differentiated, through the two T/4 delays (Delay<double>::update: fractional delay, w4c = 1 - w4): the timing error that
// enters the resonator
__device__ __forceinline__ double stg_oqpsk_t4_pair(double abval, double &d1, double &d41_1, double &d41_2, double &d41_3, double &d42_1,
                                                         double &d42_2, double &d42_3, double w4, double w4c)
{
    const double ab2 = abval * abval;
    const double st_diff = d1 - ab2; d1 = ab2;
    const double st_d1out = w4 * d41_2 + w4c * d41_3; d41_3 = d41_2; d41_2 = d41_1; d41_1 = st_diff;
    const double st_d2out = w4 * d42_2 + w4c * d42_3; d42_3 = d42_2; d42_2 = d42_1; d42_1 = st_d1out;
    return (st_d2out - st_diff) * st_d1out;
}
// (The T/8 delay behind the resonator -- `d8out = w8 * d8_1 + w8c * d8_2; d8_2 = d8_1; d8_1 = st_eta` -- stays written out in both kernels:
// the burst kernel gates the resonator's output in front of it, and as a third call there it cost that kernel 16 bytes of scratch per lane.)

// ---- the continuous MSK chain (MskDemodulator::writeData's per-sample loop, JAERO/mskdemodulator.cpp:319-485) ------------------------
// for k_msk_samples (one wavefront) and k_msk_fb (front / back pairs)

// MSKEbNoMeasure::Update's two window sums (DSP.cpp:493-505; its formula only when eval_ebno: see JD_EBNO_TAIL), AGC + clip (:378-382).
// (sre, sim) = the matched filter's output on entry, the AGC'd and clipped sample on return.  agc_old / e_old / e2_old = the entries
// leaving the windows (E2's buffer holds the squares of E's); win = this lane's column of the one ring that serves all three
// (JPtrs::win), written at agc_pos.
template <bool EBNO>
__device__ __forceinline__ void stg_msk_meter_agc_clip(double &sre, double &sim, double agc_old, double e_old, double e2_old, bool eval_ebno,
                                                       double eb_len_d, double agc_len_d, double &eb_esum, double &eb_e2sum, double &eb_ebno,
                                                       double &agc_sum, double *__restrict__ win, int &agc_pos, int win_len)
{
    const double dabval = sqrt(sre * sre + sim * sim);
    if (EBNO)
    {
        const double sq = dabval * dabval;
        eb_e2sum = eb_e2sum - e2_old; eb_e2sum = eb_e2sum + fabs(sq);
        eb_esum = eb_esum - e_old; eb_esum = eb_esum + fabs(dabval);
        if (eval_ebno) eb_ebno = stg_ebno_msk(eb_ebno, eb_e2sum / eb_len_d, eb_esum / eb_len_d);
    }
    {
        double *ap = win + (size_t)agc_pos * 64;
        agc_sum = agc_sum - agc_old;
        agc_sum = agc_sum + fabs(dabval);
        *ap = fabs(dabval); // the one store: the EbNo meter above pushed the same value
        agc_pos++; if (agc_pos >= win_len) agc_pos = 0;
    }
    double gain = jd_div(1.414213562, fmax(agc_sum / agc_len_d, 0.000001));
    gain = fmax(gain, 0.000001);
    sre *= gain; sim *= gain;
    const double abval = sqrt(sre * sre + sim * sim);
    if (abval > 2.84) { const double k = jd_div(2.84, abval); sre = k * sre; sim = k * sim; }
}

// The SPS-sample delayed arm and symbol timing (:384-405): (sre, sim) goes into delayedsmpl's ring (SPS + 1 slots, ptd = the entry at the
// slot behind the write), pt_msk = (sre, ptd.y) comes back in (q_re, q_im); |pt_msk| -> resonator -> Delay<double>(SPS/2) (an integer
// delay, weighting 0: d8out = the entry at the slot behind the write) -> phase detector against the symbol oscillator's table value
// c_st -> nudge of st_ptr weighted by 1 - |tanh(error)|.
__device__ __forceinline__ void stg_msk_timing(const JGeom &g, double sre, double sim, const double2 ptd, double d8out, const double2 c_st,
                                               bool dcd, const JdAtanLane &atl, double2 *__restrict__ dly_ring, int &dly_slot, int dly_len,
                                               double *__restrict__ d8_ring, int &d8_slot, int d8_len, double &res_x1, double &res_x2,
                                               double &res_y1, double &res_y2, double &st_ptr, double &q_re, double &q_im)
{
    dly_ring[(size_t)dly_slot * 64] = make_double2(sre, sim);
    dly_slot++; if (dly_slot >= dly_len) dly_slot = 0;
    q_re = sre; q_im = ptd.y;
    const double st_eta = jd_biquad(jd_hypot(q_re, q_im), res_x1, res_x2, res_y1, res_y2, g.res_b0, g.res_b1, g.res_b2, g.res_a1, g.res_a2);
    d8_ring[(size_t)d8_slot * 64] = st_eta;
    d8_slot++; if (d8_slot >= d8_len) d8_slot = 0;
    const double m_re = st_eta, m_im = -d8out;
    const double o_re = c_st.x * m_re - c_st.y * m_im;
    const double o_im = c_st.x * m_im + c_st.y * m_re;
    const double st_angle_error = jd_atan2(o_im, o_re, atl);
    const double weighting = fabs(jd_tanh(st_angle_error));
    if (!dcd) jd_wt_advance_fraction(st_ptr, -(1.0 - weighting) * st_angle_error * (0.05 / 360.0));
    else jd_wt_advance_fraction(st_ptr, -(1.0 - weighting) * st_angle_error * (0.003 / 360.0));
}

// The carrier step at a symbol instant (:411-426): the half of the symbol that feeds back.  Returns the clamped error ct_ec.
__device__ __forceinline__ double stg_msk_carrier(const JGeom &g, double sre, double sim, const double2 ptd, bool dcd, double samplerate,
                                                  double &m2_ptr, double &m2_freq, double &m2_step)
{
    const double ct_xt = jd_tanh(sim) * sre;
    const double ct_xt_d = jd_tanh(ptd.x) * ptd.y;
    double ct_ec = ct_xt_d - ct_xt;
    if (ct_ec > M_PI) ct_ec = M_PI;
    if (ct_ec < -M_PI) ct_ec = -M_PI;
    if (ct_ec > M_PI_2) ct_ec = M_PI_2;
    if (ct_ec < -M_PI_2) ct_ec = -M_PI_2;
    double carrier_aggression = 12.0 * g.correctionfactor;
    if (dcd) carrier_aggression = 8.0 * g.correctionfactor;
    jd_wt_inc_phase_deg(m2_ptr, carrier_aggression * 1.0 * ct_ec);
    jd_wt_setfreq(m2_freq, m2_step, (carrier_aggression * 0.01 * ct_ec) + m2_freq, samplerate);
    return ct_ec;
}

// The output half of a symbol (:428-469): marg, dt, rotation by the averaged error, MSE, symbol capture, soft differential decode, soft
// bits.  Nothing of it feeds back into the loops.  marg_old / dt_old / ms_old = the entries leaving the three symbol-rate windows
// (marg_ring[marg_pos], dt_ring[dt_pos + 1], msema_ring[msema_pos]): the caller loads them when it suits its schedule.
// k_msk_samples calls this; k_msk_fb keeps the same text written out in its queued output half (as the call it cost the 160-tap kernel a spill).
template <bool CAPSYM>
__device__ __forceinline__ void stg_msk_output_half(const JGeom &g, const JPtrs &p, int ch, double ct_ec, double q_re, double q_im, double marg_old,
                                                    const double2 dt_old, double ms_old, double *__restrict__ marg_ring,
                                                    double2 *__restrict__ dt_ring, double *__restrict__ msema_ring, int16_t *__restrict__ soft,
                                                    double &marg_sum, int &marg_pos, int &dt_pos, double &msema_sum, int &msema_pos, double &mse,
                                                    double &diff_last, int &soft_cnt, int &sym_cnt, int &overflow)
{
    {
        const double v = ct_ec / 2.0;
        double *mp = marg_ring + marg_pos;
        marg_sum = marg_sum - marg_old; marg_sum = marg_sum + v; *mp = v;
        marg_pos++; if (marg_pos >= g.marg_len) marg_pos = 0;
    }
    const double marg_val = marg_sum / ((double)g.marg_len);
    {
        dt_ring[dt_pos] = make_double2(q_re, q_im);
        dt_pos++; if (dt_pos >= g.dt_len) dt_pos = 0;
        q_re = dt_old.x; q_im = dt_old.y;
    }
    {
        const double cr = cos(marg_val), sr = sin(marg_val);
        const double nr = q_re * cr - q_im * sr;
        const double ni = q_re * sr + q_im * cr;
        q_re = nr; q_im = ni;
    }
    {
        const double tda = (fabs(q_re * 0.75) - 1.0), tdb = (fabs(q_im * 0.75) - 1.0);
        const double e = (tda * tda) + (tdb * tdb);
        double *ep = msema_ring + msema_pos;
        msema_sum = msema_sum - ms_old; msema_sum = msema_sum + fabs(e); *ep = fabs(e);
        msema_pos++; if (msema_pos >= g.msema_len) msema_pos = 0;
        mse = msema_sum / ((double)g.msema_len);
    }
    if (CAPSYM)
    {
        if (sym_cnt < g.sym_cap)
        {
            double *sp = p.sym + ((size_t)ch * g.sym_cap + sym_cnt) * 3;
            sp[0] = q_re; sp[1] = q_im; sp[2] = mse;
            sym_cnt++;
        }
        else overflow |= 2;
    }
    // soft differential decode + demap (:450-469, DSP.cpp:531-563)
    const int b0 = jd_softbit((jd_diff_soft(q_im, diff_last)) * 127.0 + 128.0);
    const int b1 = jd_softbit((-jd_diff_soft(q_re, diff_last)) * 127.0 + 128.0);
    if (soft_cnt + 2 <= g.soft_cap)
    {
        soft[soft_cnt] = (int16_t)b0;
        soft[soft_cnt + 1] = (int16_t)b1;
        soft_cnt += 2;
    }
    else overflow |= 1;
}
