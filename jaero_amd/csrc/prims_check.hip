// prims_check.hip -- libjaero_prims.so: the device primitives of jd_libm.h and jaero_device.h behind extern "C" launchers, for
// tests/test_gpu_device_math.py, which compares each with an independent host reference.  Test infrastructure, not the product: it
// includes no kernel header and is compiled with the product's flags (the Makefile's $(FLAGS)), so the functions run here are the
// sample kernels' own code, rounded as there.
//
// Every launcher takes host arrays and a count, runs the primitive elementwise (element i in thread i, 256 threads per block, so a count
// that is not a multiple of 64 leaves the last wavefront ragged), copies the outputs back and returns the first hipError_t as int.
// "io" arrays are copied in and out: elements a launch does not write keep what the caller put there.
#include "jaero_device.h"

#include <vector>

namespace
{
// device copies of a launcher's arrays; sync() copies the io / out arrays back
class Bufs
{
  public:
    ~Bufs()
    {
        for (auto &b : bufs_) (void)hipFree(b.dev);
    }
    template <class T> T *in(const T *h, long n) { return (T *)add((void *)h, n * sizeof(T), false); }
    template <class T> T *io(T *h, long n) { return (T *)add((void *)h, n * sizeof(T), true); }
    bool ok() const { return err_ == hipSuccess; }
    int sync()
    {
        if (err_ != hipSuccess) return (int)err_;
        err_ = hipGetLastError();
        if (err_ == hipSuccess) err_ = hipDeviceSynchronize();
        for (auto &b : bufs_)
            if (err_ == hipSuccess && b.back) err_ = hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost);
        return (int)err_;
    }

  private:
    struct B { void *host, *dev; size_t bytes; bool back; };
    void *add(void *h, size_t bytes, bool back)
    {
        void *d = nullptr;
        if (err_ == hipSuccess) err_ = hipMalloc(&d, bytes ? bytes : 8);
        if (err_ == hipSuccess) bufs_.push_back({h, d, bytes, back});
        if (err_ == hipSuccess && bytes) err_ = hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
        return d;
    }
    std::vector<B> bufs_;
    hipError_t err_ = hipSuccess;
};
constexpr int TPB = 256;
inline unsigned nblocks(long n) { return (unsigned)((n + TPB - 1) / TPB); }
} // namespace

#define JP_IDX const long i = (long)blockIdx.x * TPB + threadIdx.x

// ---- jd_libm.h --------------------------------------------------------------------------------------------------------------------
// jd_atan2 with the lane table built at kernel entry by every lane, as the sample kernels build it; the call itself runs only on the lanes
// of `mask` (and i < n): with part of the wavefront switched off, jda_fetch must take its table-in-memory path
__global__ void __launch_bounds__(TPB) k_jp_atan2(const double *y, const double *x, double *o, long n, unsigned long long mask)
{
    const int lane = threadIdx.x & 63;
    const JdAtanLane T = jd_atan_lane_table(lane);
    JP_IDX;
    if (i < n && (mask >> lane & 1)) o[i] = jd_atan2(y[i], x[i], T);
}
__global__ void __launch_bounds__(TPB) k_jp_hypot(const double *x, const double *y, double *o, long n)
{
    JP_IDX;
    if (i < n) o[i] = jd_hypot(x[i], y[i]);
}
// jd_div and the compiler's IEEE division of the same operands in the same kernel
__global__ void __launch_bounds__(TPB) k_jp_div(const double *a, const double *b, double *o, double *o_ieee, long n)
{
    JP_IDX;
    if (i < n) { o[i] = jd_div(a[i], b[i]); o_ieee[i] = a[i] / b[i]; }
}

// ---- jaero_device.h ---------------------------------------------------------------------------------------------------------------
// d and rd are wave-uniform kernel arguments, as the constants are in the sample kernels
__global__ void __launch_bounds__(TPB) k_jp_div_const(const double *x, double *o, double *o_ieee, long n, double d, double rd)
{
    JP_IDX;
    if (i < n) { o[i] = jd_div_const(x[i], d, rd); o_ieee[i] = x[i] / d; }
}
__global__ void __launch_bounds__(TPB) k_jp_tanh(const double *x, double *o, long n)
{
    JP_IDX;
    if (i < n) o[i] = jd_tanh(x[i]);
}
__global__ void __launch_bounds__(TPB) k_jp_tanh_full(const double *x, double *o, long n)
{
    JP_IDX;
    if (i < n) o[i] = jd_tanh_full(x[i]);
}
__global__ void __launch_bounds__(TPB) k_jp_expm1(const double *x, double *o, long n)
{
    JP_IDX;
    if (i < n) o[i] = jd_expm1(x[i]);
}
__global__ void __launch_bounds__(TPB) k_jp_log10(const double *x, double *o, long n)
{
    JP_IDX;
    if (i < n) o[i] = jd_log10(x[i]);
}
// c6_log10_half beside the product it replaces in the estimate kernels' epilogue (tests/test_gpu_log10_half.py wants the same bits)
__global__ void __launch_bounds__(TPB) k_jc_log10_half(const double *x, double *o_half, double *o_product, long n)
{
    JP_IDX;
    if (i < n) { o_half[i] = c6_log10_half(x[i]); o_product[i] = 0.5 * jd_log10(x[i]); }
}
__global__ void __launch_bounds__(TPB) k_jp_qround(const double *x, int *o, long n)
{
    JP_IDX;
    if (i < n) o[i] = jd_qround(x[i]);
}
__global__ void __launch_bounds__(TPB) k_jp_softbit(const double *x, int *o, long n)
{
    JP_IDX;
    if (i < n) o[i] = jd_softbit(x[i]);
}
__global__ void __launch_bounds__(TPB) k_jp_cisidx(const double *x, int *o, long n)
{
    JP_IDX;
    if (i < n) o[i] = jd_cisidx(x[i]);
}
__global__ void __launch_bounds__(TPB) k_jp_wt_next(double *ptr, double *step, long n)
{
    JP_IDX;
    if (i < n) { double p = ptr[i], s = step[i]; jd_wt_next(p, s); ptr[i] = p; step[i] = s; }
}
__global__ void __launch_bounds__(TPB) k_jp_wt_setfreq(const double *f, double *freq, double *step, long n, double samplerate)
{
    JP_IDX;
    if (i < n) { double fr, st; jd_wt_setfreq(fr, st, f[i], samplerate); freq[i] = fr; step[i] = st; }
}
__global__ void __launch_bounds__(TPB) k_jp_wt_inc_phase_deg(double *ptr, const double *phase_deg, long n)
{
    JP_IDX;
    if (i < n) { double p = ptr[i]; jd_wt_inc_phase_deg(p, phase_deg[i]); ptr[i] = p; }
}
__global__ void __launch_bounds__(TPB) k_jp_wt_advance_fraction(double *ptr, const double *f, long n)
{
    JP_IDX;
    if (i < n) { double p = ptr[i]; jd_wt_advance_fraction(p, f[i]); ptr[i] = p; }
}
__global__ void __launch_bounds__(TPB) k_jp_wt_passed(const double *last_ptr, const double *ptr, const double *step, const double *fraction_of_wave,
                                                      double *frac, int *passed, long n)
{
    JP_IDX;
    if (i < n) { double fr = frac[i]; passed[i] = jd_wt_passed(last_ptr[i], ptr[i], step[i], fraction_of_wave[i], fr) ? 1 : 0; frac[i] = fr; }
}
__global__ void __launch_bounds__(TPB) k_jp_fb_wt_setfreq(const double *f, double *freq, double *step, long n, double samplerate, double r_samplerate)
{
    JP_IDX;
    if (i < n) { double fr, st; fb_wt_setfreq(fr, st, f[i], samplerate, r_samplerate); freq[i] = fr; step[i] = st; }
}
__global__ void __launch_bounds__(TPB) k_jp_fb_wt_next(double *ptr, double *step, long n)
{
    JP_IDX;
    if (i < n) { double p = ptr[i], s = step[i]; fb_wt_next(p, s); ptr[i] = p; step[i] = s; }
}
__global__ void __launch_bounds__(TPB) k_jp_fb_fmod360(const double *x, double *o, long n)
{
    JP_IDX;
    if (i < n) o[i] = fb_fmod360(x[i]);
}
// `steps` consecutive updates per lane: x and y are [steps][n], st is [4][n] = x1, x2, y1, y2 (in and out); the coefficients are wave-uniform
// kernel arguments, as JGeom's are in the sample kernels
__global__ void __launch_bounds__(TPB) k_jp_biquad(const double *x, double *st, double *y, long n, int steps, double b0, double b1, double b2,
                                                   double a1, double a2)
{
    JP_IDX;
    if (i >= n) return;
    double x1 = st[i], x2 = st[n + i], y1 = st[2 * n + i], y2 = st[3 * n + i];
    for (int k = 0; k < steps; k++) y[(long)k * n + i] = jd_biquad(x[(long)k * n + i], x1, x2, y1, y2, b0, b1, b2, a1, a2);
    st[i] = x1; st[n + i] = x2; st[2 * n + i] = y1; st[3 * n + i] = y2;
}
__global__ void __launch_bounds__(TPB) k_jp_diff_soft(const double *soft_in, double *diff_last, double *o, long n)
{
    JP_IDX;
    if (i < n) { double d = diff_last[i]; o[i] = jd_diff_soft(soft_in[i], d); diff_last[i] = d; }
}
__global__ void __launch_bounds__(TPB) k_jp_wt_next_symbol(double *ptr, double *step, double *last_ptr, long n)
{
    JP_IDX;
    if (i < n) { double p = ptr[i], s = step[i], l = last_ptr[i]; jd_wt_next_symbol(p, s, l); ptr[i] = p; step[i] = s; last_ptr[i] = l; }
}
__global__ void __launch_bounds__(TPB) k_jp_bd_set_phase_deg(const double *phase_deg, double *ptr, long n)
{
    JP_IDX;
    if (i < n) { double p = ptr[i]; bd_set_phase_deg(p, phase_deg[i]); ptr[i] = p; }
}

// ---- the matched-filter evaluators ------------------------------------------------------------------------------------------------
// One wavefront per block, block b evaluating with the ring at position fir_slot = b (b = 0 .. LDSN-1): the same register tail
// (tail[j][lane] = x[n-LDSN-1-j]), the same LDS ring ([slot][lane]) and taps in every block.  out[b][lane].
// FORM 0: jd_fir_eval (taps from LDS, the ring walked; FUSED: jd_fir_sum over the walked ring with one fma per tap, which jd_fir_eval does not offer), 1: jd_fir_eval_sym, 2: jd_fir_eval_sym_static, 3: jd_fir_eval_sym_static_but_last (JTaps28: the first
// 28 of 55 bitwise symmetric taps; form 3 reads no ring slot fir_slot and sums taps 0..53).
template <int FORM, int FIRN, int LDSN, int D, bool FUSED>
__global__ void __launch_bounds__(64) k_jp_fir(const double *taps, const double *tail_re, const double *tail_im, const double *ring_re,
                                               const double *ring_im, JTaps28 tp, double *out_re, double *out_im)
{
    constexpr int TAILN = FIRN - LDSN, TAILA = TAILN > 0 ? TAILN : 1;
    __shared__ double lre[LDSN * 64], lim[LDSN * 64], ltap[FIRN];
    const int lane = threadIdx.x, fir_slot = blockIdx.x;
    for (int s = 0; s < LDSN; s++) { lre[s * 64 + lane] = ring_re[s * 64 + lane]; lim[s * 64 + lane] = ring_im[s * 64 + lane]; }
    for (int k = lane; k < FIRN; k += 64) ltap[k] = taps[k];
    double tre[TAILA], tim[TAILA];
#pragma unroll
    for (int j = 0; j < TAILA; j++) { tre[j] = TAILN > 0 ? tail_re[j * 64 + lane] : 0.0; tim[j] = TAILN > 0 ? tail_im[j * 64 + lane] : 0.0; }
    __syncthreads();
    double ore = 0, oim = 0;
    if constexpr (FORM == 0 && FUSED) jd_fir_sum<FIRN, LDSN, D, true, 0>(JdRingWalk<LDSN>{lre, lim, fir_slot, lane}, ltap, 0, tre, tim, 0.0, 0.0, ore, oim);
    else if constexpr (FORM == 0) jd_fir_eval<FIRN, LDSN, D>(lre, lim, ltap, tre, tim, fir_slot, lane, ore, oim);
    else if constexpr (FORM == 1) jd_fir_eval_sym<FIRN, LDSN, D>(lre, lim, tp, tre, tim, fir_slot, lane, ore, oim);
    else if constexpr (FORM == 2) jd_fir_eval_sym_static<FIRN, LDSN, D>(lre, lim, tp, tre, tim, fir_slot, lane, ore, oim);
    else jd_fir_eval_sym_static_but_last<FIRN, LDSN, D>(lre, lim, tp, tre, tim, fir_slot, lane, ore, oim);
    out_re[fir_slot * 64 + lane] = ore;
    out_im[fir_slot * 64 + lane] = oim;
}
template <int FORM, int FIRN, int LDSN, int D, bool FUSED>
static int run_fir(const double *taps, const double *tail_re, const double *tail_im, const double *ring_re, const double *ring_im, double *out_re,
                   double *out_im)
{
    constexpr int TAILA = FIRN - LDSN > 0 ? FIRN - LDSN : 1;
    JTaps28 tp;
    for (int k = 0; k < 28; k++) tp.t[k] = k < FIRN ? taps[k] : 0.0;
    Bufs b;
    const double *dt = b.in(taps, FIRN), *dtr = b.in(tail_re, TAILA * 64), *dti = b.in(tail_im, TAILA * 64);
    const double *drr = b.in(ring_re, LDSN * 64), *dri = b.in(ring_im, LDSN * 64);
    double *dor = b.io(out_re, LDSN * 64), *doi = b.io(out_im, LDSN * 64);
    if (b.ok()) k_jp_fir<FORM, FIRN, LDSN, D, FUSED><<<LDSN, 64>>>(dt, dtr, dti, drr, dri, tp, dor, doi);
    return b.sync();
}
// jd_fir_sum_blocks: the sum over taps T0 .. FIRN-1 continued from start[lane], ring reads by blocks of BS slots.  The same blocks, tail
// (FIRN-T0-LDSN entries) and ring as above; the im ring lies directly behind the re ring, as the block form reads it, and the LDS is taken
// dynamically (160 / 72: 73 728 B of rings plus the taps, above the static limit).
template <int FIRN, int LDSN, int D, bool FUSED, int T0, int BS>
__global__ void __launch_bounds__(64) k_jp_fir_blocks(const double *taps, const double *tail_re, const double *tail_im, const double *ring_re,
                                                      const double *ring_im, const double *start_re, const double *start_im, double *out_re, double *out_im)
{
    constexpr int TAILN = FIRN - T0 - LDSN, TAILA = TAILN > 0 ? TAILN : 1;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *lre = lds, *lim = lds + LDSN * 64, *ltap = lds + 2 * LDSN * 64;
    const int lane = threadIdx.x, fir_slot = blockIdx.x;
    for (int s = 0; s < LDSN; s++) { lre[s * 64 + lane] = ring_re[s * 64 + lane]; lim[s * 64 + lane] = ring_im[s * 64 + lane]; }
    for (int k = lane; k < FIRN; k += 64) ltap[k] = taps[k];
    double tre[TAILA], tim[TAILA];
#pragma unroll
    for (int j = 0; j < TAILA; j++) { tre[j] = TAILN > 0 ? tail_re[j * 64 + lane] : 0.0; tim[j] = TAILN > 0 ? tail_im[j * 64 + lane] : 0.0; }
    __syncthreads();
    double ore = 0, oim = 0;
    jd_fir_sum_blocks<FIRN, LDSN, D, FUSED, T0, BS>(lre, ltap, jd_vzero(), tre, tim, fir_slot, lane, start_re[lane], start_im[lane], ore, oim);
    out_re[fir_slot * 64 + lane] = ore;
    out_im[fir_slot * 64 + lane] = oim;
}
template <int FIRN, int LDSN, int D, bool FUSED, int T0, int BS>
static int run_fir_blocks(const double *taps, const double *tail_re, const double *tail_im, const double *ring_re, const double *ring_im,
                          const double *start_re, const double *start_im, double *out_re, double *out_im)
{
    constexpr int TAILA = FIRN - T0 - LDSN > 0 ? FIRN - T0 - LDSN : 1, LDS_BYTES = (2 * LDSN * 64 + FIRN) * (int)sizeof(double);
    const auto kernel = k_jp_fir_blocks<FIRN, LDSN, D, FUSED, T0, BS>;
    const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    Bufs b;
    const double *dt = b.in(taps, FIRN), *dtr = b.in(tail_re, TAILA * 64), *dti = b.in(tail_im, TAILA * 64);
    const double *drr = b.in(ring_re, LDSN * 64), *dri = b.in(ring_im, LDSN * 64), *dsr = b.in(start_re, 64), *dsi = b.in(start_im, 64);
    double *dor = b.io(out_re, LDSN * 64), *doi = b.io(out_im, LDSN * 64);
    if (b.ok()) kernel<<<LDSN, 64, LDS_BYTES>>>(dt, dtr, dti, drr, dri, dsr, dsi, dor, doi);
    return b.sync();
}

// ---- exports ----------------------------------------------------------------------------------------------------------------------
extern "C" {
int jp_atan2(const double *y, const double *x, double *o, long n, unsigned long long mask)
{
    Bufs b;
    const double *dy = b.in(y, n), *dx = b.in(x, n);
    double *d = b.io(o, n);
    if (b.ok() && n > 0) k_jp_atan2<<<nblocks(n), TPB>>>(dy, dx, d, n, mask);
    return b.sync();
}
#define JP_2IN_1OUT(NAME, T)                                                                                                                         \
    int NAME(const double *a, const double *c, T *o, long n)                                                                                         \
    {                                                                                                                                                \
        Bufs b;                                                                                                                                      \
        const double *da = b.in(a, n), *dc = b.in(c, n);                                                                                             \
        T *d = b.io(o, n);                                                                                                                           \
        if (b.ok() && n > 0) k_##NAME<<<nblocks(n), TPB>>>(da, dc, d, n);                                                                            \
        return b.sync();                                                                                                                             \
    }
#define JP_1IN_1OUT(NAME, T)                                                                                                                         \
    int NAME(const double *a, T *o, long n)                                                                                                          \
    {                                                                                                                                                \
        Bufs b;                                                                                                                                      \
        const double *da = b.in(a, n);                                                                                                               \
        T *d = b.io(o, n);                                                                                                                           \
        if (b.ok() && n > 0) k_##NAME<<<nblocks(n), TPB>>>(da, d, n);                                                                                \
        return b.sync();                                                                                                                             \
    }
JP_2IN_1OUT(jp_hypot, double)
JP_1IN_1OUT(jp_tanh, double)
JP_1IN_1OUT(jp_tanh_full, double)
JP_1IN_1OUT(jp_expm1, double)
JP_1IN_1OUT(jp_log10, double)
JP_1IN_1OUT(jp_qround, int)
JP_1IN_1OUT(jp_softbit, int)
JP_1IN_1OUT(jp_cisidx, int)
JP_1IN_1OUT(jp_fb_fmod360, double)
int jc_log10_half(const double *x, double *o_half, double *o_product, long n)
{
    Bufs b;
    const double *dx = b.in(x, n);
    double *dh = b.io(o_half, n), *dp = b.io(o_product, n);
    if (b.ok() && n > 0) k_jc_log10_half<<<nblocks(n), TPB>>>(dx, dh, dp, n);
    return b.sync();
}
int jp_div(const double *a, const double *bb, double *o, double *o_ieee, long n)
{
    Bufs b;
    const double *da = b.in(a, n), *db = b.in(bb, n);
    double *d = b.io(o, n), *di = b.io(o_ieee, n);
    if (b.ok() && n > 0) k_jp_div<<<nblocks(n), TPB>>>(da, db, d, di, n);
    return b.sync();
}
int jp_div_const(const double *x, double *o, double *o_ieee, long n, double dd, double rd)
{
    Bufs b;
    const double *dx = b.in(x, n);
    double *d = b.io(o, n), *di = b.io(o_ieee, n);
    if (b.ok() && n > 0) k_jp_div_const<<<nblocks(n), TPB>>>(dx, d, di, n, dd, rd);
    return b.sync();
}
int jp_wt_next(double *ptr, double *step, long n)
{
    Bufs b;
    double *dp = b.io(ptr, n), *ds = b.io(step, n);
    if (b.ok() && n > 0) k_jp_wt_next<<<nblocks(n), TPB>>>(dp, ds, n);
    return b.sync();
}
int jp_fb_wt_next(double *ptr, double *step, long n)
{
    Bufs b;
    double *dp = b.io(ptr, n), *ds = b.io(step, n);
    if (b.ok() && n > 0) k_jp_fb_wt_next<<<nblocks(n), TPB>>>(dp, ds, n);
    return b.sync();
}
int jp_wt_setfreq(const double *f, double *freq, double *step, long n, double samplerate)
{
    Bufs b;
    const double *df = b.in(f, n);
    double *dfr = b.io(freq, n), *ds = b.io(step, n);
    if (b.ok() && n > 0) k_jp_wt_setfreq<<<nblocks(n), TPB>>>(df, dfr, ds, n, samplerate);
    return b.sync();
}
int jp_fb_wt_setfreq(const double *f, double *freq, double *step, long n, double samplerate, double r_samplerate)
{
    Bufs b;
    const double *df = b.in(f, n);
    double *dfr = b.io(freq, n), *ds = b.io(step, n);
    if (b.ok() && n > 0) k_jp_fb_wt_setfreq<<<nblocks(n), TPB>>>(df, dfr, ds, n, samplerate, r_samplerate);
    return b.sync();
}
int jp_wt_inc_phase_deg(double *ptr, const double *phase_deg, long n)
{
    Bufs b;
    double *dp = b.io(ptr, n);
    const double *dph = b.in(phase_deg, n);
    if (b.ok() && n > 0) k_jp_wt_inc_phase_deg<<<nblocks(n), TPB>>>(dp, dph, n);
    return b.sync();
}
int jp_wt_advance_fraction(double *ptr, const double *f, long n)
{
    Bufs b;
    double *dp = b.io(ptr, n);
    const double *df = b.in(f, n);
    if (b.ok() && n > 0) k_jp_wt_advance_fraction<<<nblocks(n), TPB>>>(dp, df, n);
    return b.sync();
}
int jp_wt_passed(const double *last_ptr, const double *ptr, const double *step, const double *fraction_of_wave, double *frac, int *passed, long n)
{
    Bufs b;
    const double *dl = b.in(last_ptr, n), *dp = b.in(ptr, n), *ds = b.in(step, n), *dw = b.in(fraction_of_wave, n);
    double *dfr = b.io(frac, n);
    int *dpa = b.io(passed, n);
    if (b.ok() && n > 0) k_jp_wt_passed<<<nblocks(n), TPB>>>(dl, dp, ds, dw, dfr, dpa, n);
    return b.sync();
}
int jp_biquad(const double *x, double *st, double *y, long n, int steps, double b0, double b1, double b2, double a1, double a2)
{
    Bufs b;
    const double *dx = b.in(x, n * steps);
    double *ds = b.io(st, 4 * n), *dy = b.io(y, n * steps);
    if (b.ok() && n > 0) k_jp_biquad<<<nblocks(n), TPB>>>(dx, ds, dy, n, steps, b0, b1, b2, a1, a2);
    return b.sync();
}
int jp_diff_soft(const double *soft_in, double *diff_last, double *o, long n)
{
    Bufs b;
    const double *dsi = b.in(soft_in, n);
    double *dd = b.io(diff_last, n), *d = b.io(o, n);
    if (b.ok() && n > 0) k_jp_diff_soft<<<nblocks(n), TPB>>>(dsi, dd, d, n);
    return b.sync();
}
int jp_wt_next_symbol(double *ptr, double *step, double *last_ptr, long n)
{
    Bufs b;
    double *dp = b.io(ptr, n), *ds = b.io(step, n), *dl = b.io(last_ptr, n);
    if (b.ok() && n > 0) k_jp_wt_next_symbol<<<nblocks(n), TPB>>>(dp, ds, dl, n);
    return b.sync();
}
int jp_bd_set_phase_deg(const double *phase_deg, double *ptr, long n)
{
    Bufs b;
    const double *dph = b.in(phase_deg, n);
    double *dp = b.io(ptr, n);
    if (b.ok() && n > 0) k_jp_bd_set_phase_deg<<<nblocks(n), TPB>>>(dph, dp, n);
    return b.sync();
}

// the matched-filter instantiations of the sample kernels (tests/device_prims.py: FIR_ROWS, with their call sites)
#define JP_FIR(NAME, FORM, FIRN, LDSN, D, FUSED)                                                                                                     \
    int NAME(const double *taps, const double *tail_re, const double *tail_im, const double *ring_re, const double *ring_im, double *out_re,        \
             double *out_im)                                                                                                                         \
    {                                                                                                                                                \
        return run_fir<FORM, FIRN, LDSN, D, FUSED>(taps, tail_re, tail_im, ring_re, ring_im, out_re, out_im);                                       \
    }
JP_FIR(jp_fir_eval_40_24_8, 0, 40, 24, 8, false)
JP_FIR(jp_fir_eval_20_12_8, 0, 20, 12, 8, false)
JP_FIR(jp_fir_eval_fused_55_36_8, 0, 55, 36, 8, true)
JP_FIR(jp_fir_eval_sym_55_36_6, 1, 55, 36, 6, false)
JP_FIR(jp_fir_eval_sym_static_55_36_6, 2, 55, 36, 6, false)
JP_FIR(jp_fir_eval_sym_static_but_last_55_36_6, 3, 55, 36, 6, false)
#define JP_FIR_BLOCKS(NAME, FIRN, LDSN, D, FUSED, T0, BS)                                                                                            \
    int NAME(const double *taps, const double *tail_re, const double *tail_im, const double *ring_re, const double *ring_im,                       \
             const double *start_re, const double *start_im, double *out_re, double *out_im)                                                        \
    {                                                                                                                                                \
        return run_fir_blocks<FIRN, LDSN, D, FUSED, T0, BS>(taps, tail_re, tail_im, ring_re, ring_im, start_re, start_im, out_re, out_im);         \
    }
JP_FIR_BLOCKS(jp_fir_sum_blocks_80_36_8_t32_b4, 80, 36, 8, false, 32, 4)
JP_FIR_BLOCKS(jp_fir_sum_blocks_80_32_8_t18_b4, 80, 32, 8, false, 18, 4)
JP_FIR_BLOCKS(jp_fir_sum_blocks_160_72_8_t64_b4, 160, 72, 8, false, 64, 4)
JP_FIR_BLOCKS(jp_fir_sum_blocks_fused_55_36_8_t0_b6, 55, 36, 8, true, 0, 6)
}
