/* ORACLE -- TEST INFRASTRUCTURE ONLY.  CPU restatement of the reference's demodulator hot path.
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use it; the product path
 * (jaero_amd/, libjaero_hip.so) must never include, link or call anything in oracle/.  See jaero_oracle.c. */
#ifndef JAERO_ORACLE_H
#define JAERO_ORACLE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { JO_KIND_MSK = 0, JO_KIND_OQPSK = 1, JO_KIND_BURST_MSK = 2, JO_KIND_BURST_OQPSK = 3 };

typedef struct
{
    int kind;                    /* JO_KIND_* */
    int coarsefreqest_fft_power; /* Settings::coarsefreqest_fft_power */
    double freq_center;          /* Hz */
    double lockingbw;            /* Hz */
    double fb;                   /* bps */
    double Fs;                   /* Hz */
    double signalthreshold;
} jo_settings;

typedef struct jo_demod jo_demod;

/* = constructor + setSettings(settings) + start() of OqpskDemodulator / MskDemodulator */
jo_demod *jo_demod_create(const jo_settings *s);
void jo_demod_destroy(jo_demod *d);
/* = setSettings on a live object (JAERO/oqpskdemodulator.cpp:175-289, JAERO/mskdemodulator.cpp:135-263) */
void jo_demod_set_settings(jo_demod *d, const jo_settings *s);
/* = setAFC / setSQL / setCPUReduce */
void jo_demod_set_flags(jo_demod *d, int afc, int sql, int cpu_reduce);
/* = DCDstatSlot */
void jo_demod_set_dcd(jo_demod *d, int dcd);
/* = CenterFreqChangedSlot */
void jo_demod_center_freq_changed(jo_demod *d, double freq_center);
/* = writeData(const char*, len) with len = 2*nsamples */
long jo_demod_write(jo_demod *d, const int16_t *pcm, long nsamples);
/* tests only: the same write with the samples given as doubles on the int16 scale, which need not be whole numbers */
long jo_demod_write_f64(jo_demod *d, const double *x, long nsamples);

/* captured outputs (drained by the calls below) */
/* soft bits exactly as passed to processDemodulatedSoftBits, concatenated */
long jo_demod_take_soft(jo_demod *d, int16_t *dst, long cap);
/* one row of 6 doubles per FreqOffsetEstimateSlot: [n, freq_est(mixer2), freq_center(mixer_center), mse, ebno, signal] */
long jo_demod_take_status(jo_demod *d, double *dst, long caprows);
/* soft symbols: (re,im) of pt_qpsk / pt_msk after the residual rotation, one per symbol pair,
 * plus the mse value after that symbol: rows of 3 doubles.  Enabled by jo_demod_capture_symbols(d,1). */
void jo_demod_capture_symbols(jo_demod *d, int on);
long jo_demod_take_symbols(jo_demod *d, double *dst, long caprows);
/* pending soft bits not yet emitted (RxDataBits.size()) */
int jo_demod_pending_soft(jo_demod *d);
/* current values */
double jo_demod_get_mse(jo_demod *d);
double jo_demod_get_freq_est(jo_demod *d);
double jo_demod_get_freq_center(jo_demod *d);
double jo_demod_get_ebno(jo_demod *d); /* the EbNo meter's value (EbNoMeasurmentSignal), updated between estimates too */
/* cval_prefiltered of every 8400 bps write (JAERO/oqpskdemodulator.cpp:343-381), concatenated over writes: rows of (re, im) */
void jo_demod_capture_prefiltered(jo_demod *d, int on);
long jo_demod_take_prefiltered(jo_demod *d, double *dst, long caprows);
/* mixer_fir_pre's frequency and the mixer2_freq_sum of the last write, which it was set from (JAERO/oqpskdemodulator.cpp:607-608) */
double jo_demod_get_pre_freq(jo_demod *d);
double jo_demod_get_pre_freq_sum(jo_demod *d);

/* Branch counters of the continuous demodulators, per object: times taken in oqpsk_write / msk_write, the two slot functions and the meters.
 * jo_demod_coverage fills JO_DEMOD_NCOV longs in this order (oracle.py: Demod.COVERAGE). */
enum
{
    JO_COV_CLIP,          /* |sig2| > 2.84 */
    JO_COV_EC_PI,         /* ct_ec clamped at +-pi */
    JO_COV_LF_PI2_POS,    /* carrier loop: clamped at +pi/2 (10.5 kbps: behind the loop filter; MSK: the raw error) */
    JO_COV_LF_PI2_NEG,    /* ... at -pi/2 */
    JO_COV_ST_LOW,        /* OQPSK: st_osc held at st_osc_ref - 0.1 Hz */
    JO_COV_ST_HIGH,       /* ... at st_osc_ref + 0.1 Hz */
    JO_COV_SYM_GATED,     /* OQPSK: a symbol not output because mse >= signalthreshold */
    JO_COV_SOFT_255,      /* a soft byte saturated at 255 */
    JO_COV_SOFT_0,        /* ... at 0 */
    JO_COV_MU_FLOOR,      /* OQPSK: MSEcalc's mean floored at 1e-6 */
    JO_COV_OQ_MVR_FLOOR,  /* OQPSK meter: mvr floored at 1e-9 */
    JO_COV_OQ_TEBNO_HI,   /* ... tebno > 50 */
    JO_COV_OQ_TEBNO_LO,   /* ... tebno < 0 */
    JO_COV_OQ_NAN,        /* ... tebno NaN */
    JO_COV_MSK_NAN,       /* MSK meter: tebno NaN */
    JO_COV_MSK_TEBNO_HI,  /* ... tebno > 50 */
    JO_COV_M2_COUNTDOWN2, /* OQPSK slot: mixer2 set when countdown2 ran out */
    JO_COV_M2_RULE,       /* slot: mixer2 set by the unlocked rule (OQPSK: more than 3 Hz off; MSK: any difference) */
    JO_COV_AFC_RECENTRE,  /* slot: mixer_center moved to mixer2 */
    JO_COV_AFC_CLAMP_LO,  /* ... and held at lockingbw / 2 */
    JO_COV_AFC_CLAMP_HI,  /* ... at Fs / 2 - lockingbw / 2 */
    JO_DEMOD_NCOV
};
void jo_demod_coverage(jo_demod *d, long *out);
/* tebno of the EbNo meter's last update as computed, in front of its NaN / 50 / 0 lines: how far a taken line was from not being taken */
double jo_demod_get_tebno_raw(jo_demod *d);
/* st_osc's and mixer2's frequency, and the carrier loop filter's last two inputs and outputs, newest first (x1, y1) */
typedef struct { double st_freq, m2_freq, lf_x1, lf_x2, lf_y1, lf_y2; } jo_loop_state;
void jo_demod_loop_state(jo_demod *d, int set, jo_loop_state *s);

/* stand-alone pieces for unit tests */
/* RootRaisedCosine::design (JAERO/DSP.h:316-338); returns number of points written */
int jo_rrc_design(double alpha, int firsize, double samplerate, double symbol_freq, double *points);
/* CISWT table (JAERO/DSP.cpp:11-30): 19999 (re,im) pairs */
void jo_cis_table(double *dst_re_im);
/* FFTWrapper<double>::transform semantics on top of the same radix-2 FFT as oracle/ref/shim/jfft.h */
void jo_fft(double *re_im, int n, int inverse);
/* CoarseFreqEstimate stand-alone: create/setSettings, process one nfft buffer, returns emitted estimate */
typedef struct jo_coarse jo_coarse;
jo_coarse *jo_coarse_create(int power, double lockingbw, double fb, double Fs);
void jo_coarse_destroy(jo_coarse *c);
void jo_coarse_bigchange(jo_coarse *c);
double jo_coarse_process(jo_coarse *c, const double *re_im);
void jo_coarse_get_y(jo_coarse *c, double *y);
void jo_coarse_set_y(jo_coarse *c, const double *y);

/* The 8400 bps prefilter of OqpskDemodulator::writeData on its own (JAERO/oqpskdemodulator.cpp:343-381): mixer_fir_pre as the constructor
 * leaves it (8000 Hz, phase 0, :110-115) and fir_pre with setSettings' kernel (RRC 0.6, 2049 taps, nfft 4096 at fb / 2, :278-283).
 *   write         n int16 samples; down_re_im (optional) receives the down-mixed samples that went into the filter, out_re_im cval_prefiltered
 *   end_of_write  mixer_fir_pre.SetFreq(mixer2_freq_sum / n) (:607-608)
 *   restart       fir_pre.SetKernel as setSettings calls it (:278-283)
 *   get_state     mixer_fir_pre's WTptr and WTstep */
typedef struct jo_pre8400 jo_pre8400;
jo_pre8400 *jo_pre8400_create(void);
void jo_pre8400_destroy(jo_pre8400 *p);
void jo_pre8400_write(jo_pre8400 *p, const int16_t *pcm, long n, double *down_re_im, double *out_re_im);
void jo_pre8400_end_of_write(jo_pre8400 *p, double mixer2_freq_sum, long n);
void jo_pre8400_restart(jo_pre8400 *p);
void jo_pre8400_get_state(const jo_pre8400 *p, double *wtptr, double *wtstep);

/* ---- burst demodulators (jaero_oracle_burst.c): BurstOqpskDemodulator / BurstMskDemodulator ---- */
typedef struct jo_burst jo_burst;
/* = constructor + setAFC/SQL/CPUReduce defaults + setSettings + start(); kind = JO_KIND_BURST_* */
jo_burst *jo_burst_create(const jo_settings *s);
void jo_burst_destroy(jo_burst *d);
/* BurstOqpskDemodulator::setSettings / BurstMskDemodulator::setSettings on the live object (burstoqpskdemodulator.cpp:202-277,
 * burstmskdemodulator.cpp:150-325) */
void jo_burst_set_settings(jo_burst *d, const jo_settings *s);
void jo_burst_set_flags(jo_burst *d, int afc, int sql, int cpu_reduce);
void jo_burst_set_dcd(jo_burst *d, int dcd); /* BurstMskDemodulator::DCDstatSlot */
/* = writeData (mono) */
long jo_burst_write(jo_burst *d, const int16_t *pcm, long nsamples);
/* CenterFreqChangedSlot(freq_center): acts on burst MSK (burstmskdemodulator.cpp:327-342), empty for burst OQPSK (burstoqpskdemodulator.cpp:284-289) */
void jo_burst_center_freq_changed(jo_burst *d, double freq_center);
/* soft bits as passed to processDemodulatedSoftBits, concatenated; -1 = start-of-burst marker */
long jo_burst_take_soft(jo_burst *d, int16_t *dst, long cap);
/* rows of 3 doubles [absolute sample index, kind, value]; kind 0 SignalStatus(value), 1 EbNoMeasurmentSignal(value),
 * 2 Plottables(freq_est=value); with jo_burst_trace(d,1) also 3 = peak detector fired, 4 = trident check ran
 * (value = +metric accepted / -metric rejected) */
long jo_burst_take_events(jo_burst *d, double *dst, long caprows);
void jo_burst_trace(jo_burst *d, int on);
/* with trace on: the window (tridentbuffer, *row_len doubles) of every trident check so far, one row per kind-4 event, in their order; a bank
 * whose settings change its bit rate between checks must be drained before the change (rows are cut at the current length) */
long jo_burst_take_trident_windows(jo_burst *d, double *dst, long caprows, int *row_len);
/* rows [re, im, mse] of pt_qpsk (burst OQPSK, while startstop>0) / pt_msk (burst MSK, every symbol instant) */
void jo_burst_capture_symbols(jo_burst *d, int on);
long jo_burst_take_symbols(jo_burst *d, double *dst, long caprows);
int jo_burst_pending_soft(jo_burst *d);
double jo_burst_get_mse(jo_burst *d);
double jo_burst_get_freq_est(jo_burst *d);
/* QJHilbertFilter pieces (JAERO/DSP.cpp:754-794) */
/* The signal-only part of the trident checks (burstoqpskdemodulator.cpp:412-481, burstmskdemodulator.cpp:444-520) on a window of tri_sz samples,
 * what tridentbuffer holds when the check runs: the functions the demodulators above call.  ok leaves out burst MSK's dcd and cntr terms.
 * base_abs / top_abs (16384 doubles each, or NULL): |base| and |top| of the bins the searches run over.  Returns 0, or -1 for bad arguments. */
typedef struct jo_trident_result
{
    int ok, pad;
    double freq, phase_deg, vol_gain, metric; /* metric: maxval (burst OQPSK) / minval (burst MSK), the traced value */
} jo_trident_result;
int jo_trident(int kind, double Fs, double fb, const double *window, int tri_sz, jo_trident_result *result, double *base_abs, double *top_abs);
/* The front end alone (jaero_oracle_burst.c states the columns and the measured decisions): burst_front_end and the fire / tridentbuffer_ptr lines on
 * supplied analytic samples, on an ordinary jo_burst; its scalars and lengths; the same recurrence from a fresh object in long double; and
 * PeakDetector::update on given state. */
int jo_burst_front_cols(void);
long jo_burst_front_write(jo_burst *d, const double *re_im, long n, double *rows, int hold);
void jo_burst_front_state(jo_burst *d, double *out8);
void jo_burst_front_geom(jo_burst *d, double *out8);
long jo_burst_front_exact(jo_burst *geom, const double *re_im, long n, long double *rows, long hold_at, int hold, double *info, long *trig, long trigcap);
int jo_peakdet_run(int length, double threshold, const double *history, int cntdown, double lastdy, int maxposcntdown, const double *values, long n,
                   int *fire, int *maxpos, double *state_out);
/* The tracking chain alone (jaero_oracle_burst.c): the per-sample bodies the writers run behind the front end on supplied val_to_demod, a
 * supplied verdict applied in front of sample ev_at (-1: none); the recorder that takes both from an ordinary jo_burst_write; the scalars. */
void jo_burst_record(jo_burst *d, int on);
void jo_burst_coverage(jo_burst *d, long *out6); /* clip, ct_ec clamp, squelch drop, yui correction even / odd, time-out: times taken */
long jo_burst_take_recorded_val(jo_burst *d, double *dst, long cap);
long jo_burst_take_recorded_verdicts(jo_burst *d, double *dst, long caprows); /* rows of 6 doubles: sample, then a jo_trident_result */
long jo_burst_track_write(jo_burst *d, const double *val, long n, const jo_trident_result *verdict, long ev_at);
void jo_burst_track_state(jo_burst *d, long *ints8_96, double *dbl14);
int jo_hilbert_kernel(int N, double *re_im);
typedef struct jo_hilbert jo_hilbert;
jo_hilbert *jo_hilbert_create(int N);
void jo_hilbert_destroy(jo_hilbert *h);
int jo_hilbert_latency(jo_hilbert *h);
void jo_hilbert_update(jo_hilbert *h, const int16_t *pcm, long n, double *out_re_im);

#ifdef __cplusplus
}
#endif
void jo_fastfir_run(const double *in, long n, double alpha, int K, int nfft, double Fs, double fsym, double *out);
#endif
