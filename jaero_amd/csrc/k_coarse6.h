// k_coarse6.h -- the 2^14-point coarse frequency estimator with TWO LDS exchanges per transform: 16384 = 32 x 32 x 16 (round 3).
//
// Same function as k_coarse5 / k_coarse4 (CoarseFreqEstimate::ProcessBasebandData + FreqOffsetEstimateSlot,
// JAERO/coarsefreqestimate.cpp:90-137, JAERO/oqpskdemodulator.cpp:629-677).  What round 3 measured: a transform's
// LDS traffic and its arithmetic do not overlap on this CU however they are arranged, so the only way left to shorten an estimate is to
// move fewer bytes through LDS.  16 x 16 x 16 x 4 needs three exchanges of all 32 points a thread holds; 32 x 32 x 16 needs two:
//
//   n = 512 n1 + 16 n2 + n3        k = k1 + 32 k2 + 1024 k3        (n1, n2, k1, k2 < 32;  n3, k3 < 16)
//   pass 1: FFT32 over n1, x W_N^(k1 (n mod 512))      exchange 1      pass 2: FFT32 over n2, x W_512^(k2 n3)      exchange 2
//   pass 3: two FFT16 over n3
//
// natural order on entry AND exit (slot = index >> 9, thread = index & 511), so ring / y[] accesses are whole 512-byte rows and the three
// transforms chain in registers.  The 32-point FFTs that made the first kernel of this shape (k_coarse2<14>) spill 359 registers are done
// in place: one radix-2 stage, then a 16-point FFT on each half; their outputs stay in SPLIT order (slot j < 16 = X[2j], slot 16 + j =
// X[2j + 1]), which only changes compile-time addresses of the exchange behind them.  Twiddles: even powers by a chain of products with
// step^2, each odd power one product more -- two live values instead of a table of 31.  Index maps, twiddles and bank behaviour:
// tests/test_coarse_fft14_e32_model.py.
// That is the form with the twiddles on a pass's OUTPUTS (C6_ABSORB 0; the burst acquisition's k_trident keeps it).  The estimate kernels and
// the channeliser run the form that moves them to the inputs of the next pass and absorbs them into its butterflies (C6_ABSORB 2 below,
// DESIGN 9 item 32): no twiddle products and no power chains, 842 of 8 021 vector instructions per estimate less.
#pragma once
#include <vector>
#include "k_coarse2.h"

#ifndef C4_TABN
#define C4_TABN 3584 // W8400: window table entries kept in LDS behind the exchange buffer (28 KiB): lockingbw < 10.49 kHz
#endif
#define C6_FENCE __builtin_amdgcn_sched_barrier(0)
__device__ __forceinline__ double2 c6_sq(const double2 a)
{
#pragma clang fp contract(fast)
    return make_double2(a.x * a.x - a.y * a.y, 2.0 * (a.x * a.y));
}

#ifndef C6_TRACE
#define C6_TRACE(i) // scripts/ubench/coarse_trace.hip defines it to record a clock per phase
#endif

// (value, bin) of the wavefront's first maximum in every lane: value descending, bin ascending, bin < 0 = no candidate.  The order is total,
// so any reduction tree gives the reference's ascending scan's answer.  Six DPP steps (quad permutes, half-row / row mirrors, the two
// row broadcasts of gfx9), then lane 63 holds the result.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ void c6_argmax_step(double &bv, int &bi)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(bv), __double2loint(bv), CTRL, ROWMASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(bv), __double2hiint(bv), CTRL, ROWMASK, 0xf, false);
    const int oi = __builtin_amdgcn_update_dpp(bi, bi, CTRL, ROWMASK, 0xf, false);
    const double ov = __hiloint2double(hi, lo);
    const bool take = (oi >= 0) & ((bi < 0) | (ov > bv) | ((ov == bv) & (oi < bi)));
    bv = take ? ov : bv;
    bi = take ? oi : bi;
}
__device__ __forceinline__ void c6_wave_argmax(double &bv, int &bi)
{
    c6_argmax_step<0xB1, 0xf>(bv, bi);  // quad_perm [1,0,3,2]
    c6_argmax_step<0x4E, 0xf>(bv, bi);  // quad_perm [2,3,0,1]
    c6_argmax_step<0x141, 0xf>(bv, bi); // row_half_mirror
    c6_argmax_step<0x140, 0xf>(bv, bi); // row_mirror: every lane of a row of 16 holds the row's result
    c6_argmax_step<0x142, 0xa>(bv, bi); // row_bcast:15 into rows 1 and 3
    c6_argmax_step<0x143, 0xc>(bv, bi); // row_bcast:31 into rows 2 and 3: lane 63 holds the wavefront's
    bv = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(bv), 63), __builtin_amdgcn_readlane(__double2loint(bv), 63));
    bi = __builtin_amdgcn_readlane(bi, 63);
}

#define C6_XCH 16448 // doubles: one plane of the whole transform (exchange 2: 16 rows at stride 513, + 8208 for the upper half of k2)

__device__ __forceinline__ constexpr int c6_k(int s) { return s < 16 ? 2 * s : 2 * (s - 16) + 1; }

// in-place forward 32-point DFT, natural order in, split order out
__device__ __forceinline__ void c6_fft32(CV<32> &x)
{
#pragma clang fp contract(fast)
#pragma unroll
    for (int j = 0; j < 16; j++)
    {
        const double ar = x.r[j], ai = x.i[j], br = x.r[j + 16], bi = x.i[j + 16];
        x.r[j] = ar + br; x.i[j] = ai + bi;
        double dr = ar - br, di = ai - bi;
        cmul_w64(dr, di, 2 * j); // W_32^j
        x.r[j + 16] = dr; x.i[j + 16] = di;
    }
    C6_FENCE;
#pragma unroll
    for (int h = 0; h < 2; h++)
    {
        CV<16> in, out;
#pragma unroll
        for (int j = 0; j < 16; j++) { in.r[j] = x.r[16 * h + j]; in.i[j] = x.i[16 * h + j]; }
        regfft<16>(in, out);
#pragma unroll
        for (int j = 0; j < 16; j++) { x.r[16 * h + j] = out.r[j]; x.i[16 * h + j] = out.i[j]; }
        C6_FENCE;
    }
}

// x[slot of k] *= p1^k for k = 1 .. 31 (split order): even powers e_j = p1^(2j) by a chain, each odd power one product more; three live
// values instead of a table of 31.  (Four interleaved chains of depth 5 instead of one of depth 15 measured no faster: 13.34 vs 13.19 ms.)
__device__ __forceinline__ void c6_twiddle32(CV<32> &x, const double2 p1)
{
#pragma clang fp contract(fast)
    auto app = [&](int slot, const double2 w) __attribute__((always_inline)) {
        const double r = x.r[slot] * w.x - x.i[slot] * w.y, i = x.r[slot] * w.y + x.i[slot] * w.x;
        x.r[slot] = r; x.i[slot] = i;
    };
    const double2 p2 = c6_sq(p1);
    double2 e = p2;
    app(16, p1);
#pragma unroll
    for (int j = 1; j < 16; j++)
    {
        app(j, e);
        app(16 + j, cmul2(e, p1));
        if (j < 15) e = cmul2(e, p2);
    }
}

// ---- absorbed twiddles.  The twiddle a pass used to apply to its outputs is moved to the inputs of the pass behind the exchange, where
// one thread's factors form a geometric sequence r^j -- and a decimation-in-frequency butterfly absorbs such a modulation: for a block of
// length M whose input j is meant times rho^j,
//     u = a + rho^(M/2) b,   v = a - rho^(M/2) b = 2 a - u          (6 fused multiply-adds)
// and the two halves are blocks of length M / 2 with ratios rho and rho W_M.  The 2 L - 1 multipliers of an L-point transform are constant
// roots times r^(L/2), .., r^2, r (squarings of the base), and a factor -i between two of them costs nothing.  Outputs stay in place, in
// BIT-REVERSED order, which only changes compile-time addresses behind them.  0: twiddles applied to the outputs as until now (both forms
// stay buildable: DESIGN 9 item 32), 1: only pass 2 absorbs and its outputs keep a twiddle, 2: every pass behind an exchange absorbs.
#ifndef C6_ABSORB
#define C6_ABSORB 2
#endif

// The instruction diet of DESIGN 9 item 34 (profiles/coarse_diet.md): one switch per item, 0 = the parent's code.
#ifndef C6_HIADDR
#define C6_HIADDR 1 // LDS bytes above 64 KiB addressed from a second per-thread base with immediate offsets
#endif
#ifndef C6_RINGADDR
#define C6_RINGADDR 1 // ring entries addressed by a 32-bit byte offset from a scalar base: add + mask per slot
#endif
#ifndef C6_BAND1
#define C6_BAND1 1 // band limit: one unsigned range test per slot
#endif
#ifndef C6_SQFMA
#define C6_SQFMA 1 // the squaring and |X|^2 with one product and one fused multiply-add each
#endif
#ifndef C6_LOGHALF
#define C6_LOGHALF 1 // 0.5 * log10 from halved constants (c6_log10_half)
#endif
#ifndef C6_P1FUSED
#define C6_P1FUSED 1 // pass 1's butterflies with a constant root in the fused form of the absorbed passes
#endif

__device__ __forceinline__ constexpr int c6_brev(int v, int bits)
{
    int r = 0;
    for (int i = 0; i < bits; i++) r |= ((v >> i) & 1) << (bits - 1 - i);
    return r;
}

// p * W_64^idx, 0 <= idx < 32: idx and idx + 16 share one product
__device__ __forceinline__ double2 c6_root_mul(const double2 p, int idx)
{
#pragma clang fp contract(fast)
    const int e = idx & 15;
    double2 r = p;
    if (e != 0)
    {
        const double wr = jd_w64r(e), wi = jd_w64i(e);
        r = make_double2(p.x * wr - p.y * wi, p.x * wi + p.y * wr);
    }
    return (idx & 16) ? make_double2(r.y, -r.x) : r;
}

// P[i] = r^(2^i), i < 5
__device__ __forceinline__ void c6_ratio_powers(const double2 r, double2 (&P)[5])
{
    P[0] = r;
#pragma unroll
    for (int i = 1; i < 5; i++) P[i] = c6_sq(P[i - 1]);
}

// In-place forward 32-point DFT, natural order in, X[k] left in slot c6_brev(k, 5): c6_afft<32, 0, 0> for the ratio 1, whose multipliers
// are the constant roots alone.  A first pass (no twiddle to absorb) in this form: the 34 butterflies with a root other than 1 and -i are
// six fused multiply-adds instead of four additions and a complex product (two products, two fused), the 46 others four additions.
__device__ __forceinline__ void c6_cfft32(CV<32> &x)
{
#pragma unroll
    for (int lv = 0; lv < 5; lv++)
    {
#pragma unroll
        for (int b = 0; b < (1 << lv); b++)
        {
            const int half = 16 >> lv, idx = half * 2 * c6_brev(b, lv), e = idx & 15; // the root W_64^idx, idx < 32
            const double cr = jd_w64r(e), ci = jd_w64i(e);
            const double wr = (idx & 16) ? ci : cr, wi = (idx & 16) ? -cr : ci;         // idx >= 16: -i times the root of idx - 16
#pragma unroll
            for (int j = 0; j < half; j++)
            {
                const int ia = 2 * half * b + j, ib = ia + half;
                const double ar = x.r[ia], ai = x.i[ia], br = x.r[ib], bi = x.i[ib];
                if (idx == 0) { x.r[ia] = ar + br; x.i[ia] = ai + bi; x.r[ib] = ar - br; x.i[ib] = ai - bi; }
                else if (idx == 16) { x.r[ia] = ar + bi; x.i[ia] = ai - br; x.r[ib] = ar - bi; x.i[ib] = ai + br; }
                else
                {
                    const double ur = __builtin_fma(-wi, bi, __builtin_fma(wr, br, ar));
                    const double ui = __builtin_fma(wr, bi, __builtin_fma(wi, br, ai));
                    x.r[ia] = ur; x.i[ia] = ui;
                    x.r[ib] = __builtin_fma(2.0, ar, -ur); x.i[ib] = __builtin_fma(2.0, ai, -ui);
                }
            }
        }
        C6_FENCE;
    }
}

// c6_cfft32 for an input whose slots SB .. 31 - SB are +0.0 at compile time (the boxcar band limit of a locking band that ends on slot
// boundaries).  Which slots hold a zero is followed through the network (`zero`, a constant once the loops are unrolled):
//   both inputs zero: nothing to do;      b zero: u = a + r 0 = a, v = 2 a - u = a: a renaming;
//   a zero: u = r b -- the product and the fused multiply-add the generic butterfly forms with a = 0 -- and v = 2 0 - u = -u.
// The same bits as c6_cfft32 on that input but for the sign of an exact zero (0 + r 0 is +0 where a renamed -0 stays -0), which reaches no
// |X|^2.  For SB = 7 the first level is renamings alone and the second has four of its 16 butterflies left as such; slot 32 - SB, zero as
// data in thread 0 only, is an ordinary input.  tests/test_coarse_band_model.py.
template <int SB>
__device__ __forceinline__ void c6_cfft32_band(CV<32> &x)
{
    unsigned zero = 0;
#pragma unroll
    for (int s = SB; s <= 31 - SB; s++) zero |= 1u << s;
#pragma unroll
    for (int lv = 0; lv < 5; lv++)
    {
#pragma unroll
        for (int b = 0; b < (1 << lv); b++)
        {
            const int half = 16 >> lv, idx = half * 2 * c6_brev(b, lv), e = idx & 15;
            const double cr = jd_w64r(e), ci = jd_w64i(e);
            const double wr = (idx & 16) ? ci : cr, wi = (idx & 16) ? -cr : ci;
#pragma unroll
            for (int j = 0; j < half; j++)
            {
                const int ia = 2 * half * b + j, ib = ia + half;
                const bool za = (zero >> ia) & 1u, zb = (zero >> ib) & 1u;
                const double ar = x.r[ia], ai = x.i[ia], br = x.r[ib], bi = x.i[ib];
                if (za && zb) continue;
                if (zb)
                {
                    x.r[ib] = ar; x.i[ib] = ai;
                    zero &= ~(1u << ib);
                }
                else if (za)
                {
                    double ur, ui;
                    if (idx == 0) { ur = br; ui = bi; }
                    else if (idx == 16) { ur = bi; ui = -br; }
                    else
                    {
                        ur = __builtin_fma(-wi, bi, wr * br);
                        ui = __builtin_fma(wr, bi, wi * br);
                    }
                    x.r[ia] = ur; x.i[ia] = ui;
                    x.r[ib] = -ur; x.i[ib] = -ui;
                    zero &= ~(1u << ia);
                }
                else if (idx == 0) { x.r[ia] = ar + br; x.i[ia] = ai + bi; x.r[ib] = ar - br; x.i[ib] = ai - bi; }
                else if (idx == 16) { x.r[ia] = ar + bi; x.i[ia] = ai - br; x.r[ib] = ar - bi; x.i[ib] = ai + br; }
                else
                {
                    const double ur = __builtin_fma(-wi, bi, __builtin_fma(wr, br, ar));
                    const double ui = __builtin_fma(wr, bi, __builtin_fma(wi, br, ai));
                    x.r[ia] = ur; x.i[ia] = ui;
                    x.r[ib] = __builtin_fma(2.0, ar, -ur); x.i[ib] = __builtin_fma(2.0, ai, -ui);
                }
            }
        }
        C6_FENCE;
    }
}

// In-place forward L-point DFT (L = 32, 16) of x[OFF .. OFF + L) times (r W_64^Z)^j, r^(2^i) in P; X[k] is left in slot OFF + c6_brev(k).
template <int L, int OFF, int Z>
__device__ __forceinline__ void c6_afft(CV<32> &x, const double2 (&P)[5])
{
    constexpr int LG = L == 32 ? 5 : 4, S = 64 / L;
#pragma unroll
    for (int lv = 0; lv < LG; lv++)
    {
#pragma unroll
        for (int b = 0; b < (1 << lv); b++)
        {
            const int half = L >> (lv + 1);
            const double2 w = c6_root_mul(P[LG - 1 - lv], half * (S * c6_brev(b, lv) + Z)); // (r W_64^Z W_L^q)^half, q = c6_brev(b)
#pragma unroll
            for (int j = 0; j < half; j++)
            {
                const int ia = OFF + 2 * half * b + j, ib = ia + half;
                const double ar = x.r[ia], ai = x.i[ia], br = x.r[ib], bi = x.i[ib];
                const double ur = __builtin_fma(-w.y, bi, __builtin_fma(w.x, br, ar));
                const double ui = __builtin_fma(w.x, bi, __builtin_fma(w.y, br, ai));
                x.r[ia] = ur; x.i[ia] = ui;
                x.r[ib] = __builtin_fma(2.0, ar, -ur); x.i[ib] = __builtin_fma(2.0, ai, -ui);
            }
        }
        C6_FENCE;
    }
}

// two 16-point transforms, of slots 0..15 times r^j and of slots 16..31 times (r W_32)^j
__device__ __forceinline__ void c6_afft16x2(CV<32> &x, const double2 r)
{
    double2 P[5];
    c6_ratio_powers(r, P);
    c6_afft<16, 0, 0>(x, P);
    c6_afft<16, 16, 2>(x, P);
}

// x[slot OFF + c6_brev(k)] *= c s^k for k < L: what is left of a pass's output twiddle when only the pass in front of it absorbs (C6_ABSORB 1)
template <int L, int OFF>
__device__ __forceinline__ void c6_twiddle_brev(CV<32> &x, const double2 c, const double2 s)
{
#pragma clang fp contract(fast)
    constexpr int LG = L == 32 ? 5 : 4;
    auto app = [&](int slot, const double2 w) __attribute__((always_inline)) {
        const double r = x.r[slot] * w.x - x.i[slot] * w.y, i = x.r[slot] * w.y + x.i[slot] * w.x;
        x.r[slot] = r; x.i[slot] = i;
    };
    const double2 s2 = c6_sq(s);
    double2 e = c;
#pragma unroll
    for (int j = 0; j < L / 2; j++)
    {
        app(OFF + c6_brev(2 * j, LG), e);
        app(OFF + c6_brev(2 * j + 1, LG), cmul2(e, s));
        if (j < L / 2 - 1) e = cmul2(e, s2);
    }
}

// The last pass of both workgroup transforms: slots 16 h + n3 -> FFT16 over n3 for h = 0, 1 -> X[.. k3 ..] in slot 2 k3 + h (natural order).
// ABSORBED: the inputs are meant times (r W_32^h)^n3.
template <bool ABSORBED>
__device__ __forceinline__ void c6_pass3(CV<32> &d, const double2 r)
{
    if constexpr (ABSORBED)
    {
        c6_afft16x2(d, r);
        const CV<32> o = d;
#pragma unroll
        for (int k3 = 0; k3 < 16; k3++)
        {
            d.r[2 * k3] = o.r[c6_brev(k3, 4)]; d.i[2 * k3] = o.i[c6_brev(k3, 4)];
            d.r[2 * k3 + 1] = o.r[16 + c6_brev(k3, 4)]; d.i[2 * k3 + 1] = o.i[16 + c6_brev(k3, 4)];
        }
    }
    else
    {
        CV<16> in, o0, o1;
#pragma unroll
        for (int j = 0; j < 16; j++) { in.r[j] = d.r[j]; in.i[j] = d.i[j]; }
        regfft<16>(in, o0);
        C6_FENCE;
#pragma unroll
        for (int j = 0; j < 16; j++) { in.r[j] = d.r[16 + j]; in.i[j] = d.i[16 + j]; }
        regfft<16>(in, o1);
#pragma unroll
        for (int k3 = 0; k3 < 16; k3++) { d.r[2 * k3] = o0.r[k3]; d.i[2 * k3] = o0.i[k3]; d.r[2 * k3 + 1] = o1.r[k3]; d.i[2 * k3 + 1] = o1.i[k3]; }
    }
}

// In-place forward 2^14-point DFT of the workgroup's data, natural distribution in and out.  xch: C6_XCH doubles.  AB > 0 (above):
//   pass 1: FFT32 over n1      exchange 1      pass 2: FFT32 over n2 of its input x W_1024^(k1 n2)      exchange 2
//   pass 3: two FFT16 over n3 of their input x W_N^((k1 + 32 k2) n3)
// (AB 1: pass 2's outputs x W_N^((k1 + 32 k2) n3) instead, pass 3 as for AB 0.)  Index maps, ratios and bank behaviour of this form:
// tests/test_coarse_fft14_absorbed_model.py.
// HI: the upper half of exchange 2 (byte offsets from 65 664, beyond the 16-bit offset field of a DS instruction) is addressed from bases
// of its own, formed once per transform, instead of one literal add per access.
// ZB > 0: the input's slots ZB .. 31 - ZB are +0.0 at compile time (pass 1 = c6_cfft32_band).
template <int AB = C6_ABSORB, bool P1 = (AB > 0) && C6_P1FUSED, bool HI = false, int ZB = 0>
__device__ __forceinline__ void wg_fft14_e32(CV<32> &d, double *xch, const double2 *__restrict__ tw, int t)
{
#pragma clang fp contract(fast)
    const int k1u = t >> 4, n3 = t & 15, odd = k1u & 1;
    // requested before the first butterfly.  AB 0: W_N^(n mod 512); W_512^n3.  Else W_1024^k1, the ratio pass 2 absorbs, and W_N^(k1 + 32
    // k2lo), pass 3's (its thread is t = k1 + 32 k2lo; the upper half of k2 has W_32 more), or for AB 1 the output twiddle's W_512^n3
    const double2 st1 = tw[AB ? 16 * k1u : t], st2 = tw[AB == 2 ? t : 32 * n3];
    double2 st3 = st2;
    if constexpr (AB == 1) st3 = tw[k1u * n3]; // W_N^(k1 n3)
    const int e1w0 = t, e1w1 = (t + 16) & 511;                  // exchange 1 writer: even / odd k1 rows (odd rows rotated by one n2 row)
    const int e1r = k1u * 512 + odd * 16 + n3;                  // reader: + 16 m, except the one row that wraps
    const int e1rw = e1r + 496 - 512 * odd;                     //   m = 31
    // exchange 2: row stride 513 -- a 64-bit LDS access is served 16 lanes at a time from 16 eight-byte bank pairs, and the 16 lanes of a
    // writer group differ in n3 only: an ODD stride spreads them over all 16 (514, chosen for a 32-lane rule, measured 403 M conflict cycles
    // per launch: SQ_LDS_BANK_CONFLICT)
    const int e2w = k1u + n3 * 513;                             // writer: + (k2 & 15) * 32 + (k2 >> 4) * 8208
    const int e2r = t;                                          // reader: + n3 * 513 + k2hi * 8208
    auto k2of = [](int s) __attribute__((always_inline)) { return AB ? c6_brev(s, 5) : c6_k(s); }; // the k2 that slot s holds behind pass 2
    auto k1of = [](int s) __attribute__((always_inline)) { return P1 ? c6_brev(s, 5) : c6_k(s); }; // the k1 behind pass 1 (P1: c6_cfft32)

    // ---- pass 1 ----
    static_assert(!(P1 && AB == 0), "the output twiddle of AB 0 expects split order");
    static_assert(ZB == 0 || P1, "the band-aware pass 1 is a form of c6_cfft32");
    if constexpr (ZB > 0) c6_cfft32_band<ZB>(d);
    else if constexpr (P1) c6_cfft32(d);
    else c6_fft32(d);
    if constexpr (AB == 0) c6_twiddle32(d, st1);
    C6_FENCE;
    // ---- exchange 1, a plane at a time ----
    jd_lds_barrier(); // the buffer is free (previous transform's last reads / the fold)
#pragma unroll
    for (int s = 0; s < 32; s++) xch[k1of(s) * 512 + ((k1of(s) & 1) ? e1w1 : e1w0)] = d.r[s];
    jd_lds_barrier();
#pragma unroll
    for (int m = 0; m < 32; m++) d.r[m] = xch[(m < 31 ? e1r + 16 * m : e1rw)];
    jd_lds_barrier();
#pragma unroll
    for (int s = 0; s < 32; s++) xch[k1of(s) * 512 + ((k1of(s) & 1) ? e1w1 : e1w0)] = d.i[s];
    jd_lds_barrier();
#pragma unroll
    for (int m = 0; m < 32; m++) d.i[m] = xch[(m < 31 ? e1r + 16 * m : e1rw)];
    C6_FENCE;
    // ---- pass 2 ----
    if constexpr (AB == 0)
    {
        c6_fft32(d);
        c6_twiddle32(d, st2);
    }
    else
    {
        double2 P[5];
        c6_ratio_powers(st1, P);
        c6_afft<32, 0, 0>(d, P);
        if constexpr (AB == 1) c6_twiddle_brev<32, 0>(d, st3, st2);
    }
    C6_FENCE;
    // ---- exchange 2 ----
    // the upper half of k2: + 8208.  HI: in the base, opaque so that the constant does not return to each access as a literal
    int e2wh = e2w + (HI ? 8208 : 0), e2rh = e2r + (HI ? 8208 : 0);
    if constexpr (HI) asm volatile("" : "+v"(e2wh), "+v"(e2rh));
    constexpr int UP = HI ? 0 : 8208;
    // HI: the stores in the order of k2, so that neighbours 256 bytes apart stand next to each other and pair into ds_write2_b64 (stores
    // from an opaque base are not moved past each other)
    auto sof = [](int q) __attribute__((always_inline)) { return !HI ? q : AB ? c6_brev(q, 5) : (q & 1) ? 16 + (q >> 1) : (q >> 1); };
    jd_lds_barrier();
#pragma unroll
    for (int q = 0; q < 32; q++) xch[(k2of(sof(q)) >> 4 ? e2wh + UP : e2w) + (k2of(sof(q)) & 15) * 32] = d.r[sof(q)];
    jd_lds_barrier();
#pragma unroll
    for (int m = 0; m < 32; m++) d.r[m] = xch[(m >> 4 ? e2rh + UP : e2r) + (m & 15) * 513]; // slot m = n3 + 16 k2hi
    jd_lds_barrier();
#pragma unroll
    for (int q = 0; q < 32; q++) xch[(k2of(sof(q)) >> 4 ? e2wh + UP : e2w) + (k2of(sof(q)) & 15) * 32] = d.i[sof(q)];
    jd_lds_barrier();
#pragma unroll
    for (int m = 0; m < 32; m++) d.i[m] = xch[(m >> 4 ? e2rh + UP : e2r) + (m & 15) * 513];
    C6_FENCE;
    // ---- pass 3: FFT16 over n3 for k2hi = 0, 1; X[.. + 1024 k3] -> slot 2 k3 + k2hi (= natural: k = slot * 512 + t) ----
    c6_pass3<AB == 2>(d, st2);
}


// In-place forward 2^13-point DFT of a 256-thread workgroup's data, natural distribution in and out (slot = index >> 8, thread = index & 255):
// 8192 = 32 x 16 x 16, the same two exchanges.  Half the threads of k_coarse6 with the same 32 points each, so TWO workgroups share a CU
// (2 x 64 KiB of LDS, one wavefront of each per SIMD): while one is in an exchange or waits for HBM the other computes -- the overlap a
// single workgroup cannot have.  k_coarse2<13> (16 x 32 x 16 on 512 threads) left half of them idle in its 32-point pass.
//   n = 256 n1 + 16 n2 + n3        k = k1 + 32 k2 + 512 k3        (n1, k1 < 32;  n2, n3, k2, k3 < 16)
//   AB 0: pass 1: FFT32 over n1, x W_N^(k1 (n mod 256))     exchange 1     pass 2: two FFT16 over n2 (k1 = k1a, k1a + 16), x W_256^(k2 n3)
//         exchange 2     pass 3: two FFT16 over n3 (k2 = k2lo, k2lo + 8)
//   else: pass 1: FFT32 over n1     exchange 1     pass 2: two FFT16 over n2 of their input x W_512^(k1 n2)     exchange 2
//         pass 3: two FFT16 over n3 of their input x W_N^((k1 + 32 k2) n3)       (AB 1: pass 2's outputs x that instead)
// Exchange 1: L = k1 * 256 + 16 n2 + n3 (both sides touch consecutive doubles per 16 lanes).  Exchange 2: L = k1 + 32 k2 + 513 n3 (the 16
// lanes of a writer group differ in n3 only: the odd stride spreads them over the 16 bank pairs; readers touch 64 consecutive doubles).
#define C6_XCH13 8208
template <int AB = C6_ABSORB, bool P1 = (AB > 0) && C6_P1FUSED>
__device__ __forceinline__ void wg_fft13_e32(CV<32> &d, double *xch, const double2 *__restrict__ tw, int t)
{
#pragma clang fp contract(fast)
    const int k1a = t >> 4, n3 = t & 15;
    // AB 0: W_N^(n mod 256); W_256^n3.  Else W_512^k1a, the ratio pass 2 absorbs (k1a + 16: W_32 more), and W_N^(k1 + 32 k2lo), pass 3's
    const double2 st1 = tw[AB ? 16 * k1a : t], st2 = tw[AB == 2 ? t : 32 * n3];
    const int e1r = k1a * 256 + n3;   // reader of exchange 1: + (m >> 4) * 4096 + (m & 15) * 16
    const int e2w = k1a + 513 * n3;   // writer of exchange 2: + 16 g + 32 k2
    auto k2of = [](int s) __attribute__((always_inline)) { return AB ? c6_brev(s & 15, 4) : (s & 15); }; // the k2 slot s holds behind pass 2
    auto k1of = [](int s) __attribute__((always_inline)) { return P1 ? c6_brev(s, 5) : c6_k(s); };       // the k1 behind pass 1 (P1: c6_cfft32)
    // ---- pass 1 ----
    static_assert(!(P1 && AB == 0), "the output twiddle of AB 0 expects split order");
    if constexpr (P1) c6_cfft32(d);
    else c6_fft32(d);
    if constexpr (AB == 0) c6_twiddle32(d, st1);
    C6_FENCE;
    // ---- exchange 1, a plane at a time ----
    jd_lds_barrier();
#pragma unroll
    for (int s = 0; s < 32; s++) (xch + k1of(s) * 256)[t] = d.r[s];
    jd_lds_barrier();
#pragma unroll
    for (int m = 0; m < 32; m++) d.r[m] = (xch + (m >> 4) * 4096 + (m & 15) * 16)[e1r];
    jd_lds_barrier();
#pragma unroll
    for (int s = 0; s < 32; s++) (xch + k1of(s) * 256)[t] = d.i[s];
    jd_lds_barrier();
#pragma unroll
    for (int m = 0; m < 32; m++) d.i[m] = (xch + (m >> 4) * 4096 + (m & 15) * 16)[e1r];
    C6_FENCE;
    // ---- pass 2: slots 0..15 = n2 for k1 = k1a, 16..31 for k1 = k1a + 16 ----
    if constexpr (AB == 0)
    {
#pragma unroll
        for (int g2 = 0; g2 < 2; g2++)
        {
            CV<16> in, out;
#pragma unroll
            for (int j = 0; j < 16; j++) { in.r[j] = d.r[16 * g2 + j]; in.i[j] = d.i[16 * g2 + j]; }
            regfft<16>(in, out);
            c4_twiddle16(out, st2);
#pragma unroll
            for (int j = 0; j < 16; j++) { d.r[16 * g2 + j] = out.r[j]; d.i[16 * g2 + j] = out.i[j]; }
            C6_FENCE;
        }
    }
    else
    {
        c6_afft16x2(d, st1);
        if constexpr (AB == 1)
        {
            c6_twiddle_brev<16, 0>(d, tw[n3 * k1a], st2);         // W_N^(k1 n3) W_256^(k2 n3)
            c6_twiddle_brev<16, 16>(d, tw[n3 * (k1a + 16)], st2);
        }
        C6_FENCE;
    }
    // ---- exchange 2: slot 16 g + k2 -> L = (k1a + 16 g) + 32 k2 + 513 n3; reader t3 = k1 + 32 k2lo, slot 16 h + n3 ----
    jd_lds_barrier();
#pragma unroll
    for (int s = 0; s < 32; s++) (xch + (s >> 4) * 16 + k2of(s) * 32)[e2w] = d.r[s];
    jd_lds_barrier();
#pragma unroll
    for (int m = 0; m < 32; m++) d.r[m] = (xch + (m >> 4) * 256 + (m & 15) * 513)[t];
    jd_lds_barrier();
#pragma unroll
    for (int s = 0; s < 32; s++) (xch + (s >> 4) * 16 + k2of(s) * 32)[e2w] = d.i[s];
    jd_lds_barrier();
#pragma unroll
    for (int m = 0; m < 32; m++) d.i[m] = (xch + (m >> 4) * 256 + (m & 15) * 513)[t];
    C6_FENCE;
    // ---- pass 3: FFT16 over n3 for h = 0, 1; X[t + 256 h + 512 k3] -> slot 2 k3 + h (natural) ----
    c6_pass3<AB == 2>(d, st2);
}

template <int LOG2N, int ZB = 0>
__device__ __forceinline__ void c6_fft(CV<32> &d, double *xch, const double2 *__restrict__ tw, int t)
{
    static_assert(ZB == 0 || LOG2N == 14, "the band-aware pass 1 exists for the 2^14-point transform");
    int tt = t; // laundered per call: nothing derived from it inside is shared between the three calls of an estimate and kept live
    asm volatile("" : "+v"(tt));
    if constexpr (LOG2N == 14) wg_fft14_e32<C6_ABSORB, (C6_ABSORB > 0) && C6_P1FUSED, C6_HIADDR != 0, ZB>(d, xch, tw, tt);
    else wg_fft13_e32<C6_ABSORB, (C6_ABSORB > 0) && C6_P1FUSED>(d, xch, tw, tt);
}

// the 8400 bps window's startbin + 2 table entries (coarsefreqestimate.cpp:61-74).  Out of line on purpose: it runs when a channel's locking
// bandwidth changes, and inlined into the persistent estimate loop the cosine's constants were hoisted out of that loop and kept -- spilled --
// across every estimate's three transforms.
__device__ __noinline__ void c6_build_window(double *wt, int startbin, int t, int nthreads)
{
    for (int i = t; i <= startbin + 1; i += nthreads)
    {
        const double c = cos(M_PI_2 * ((double)i) / ((double)startbin));
        wt[i] = (i == 0) ? 1.0 : ((i <= startbin) ? c * c : 0.0);
    }
}

#ifndef C6_YADDR
#define C6_YADDR 0 // band-aware instantiation only: y[] addressed by a 32-bit byte offset from a scalar row base per slot.  Built and not
                   // kept: the 32 row bases cost 46 more spilled scalar registers than the 64-bit adds they replace (profiles/coarse_band.md)
#endif
#ifndef C6_LOGSKIP
#define C6_LOGSKIP 1 // band-aware instantiation only: no logarithm for slots outside the squared signal's spectrum unless a lane exceeds 1
#endif

// SB > 0: the band-aware instantiation for channels whose locking band ends on slot boundaries: startbin = SB * NT,
// expectedpeakbin = EPB, i0 = N / 2 - startbin and i1 = N / 2 + startbin of the fold -- the host launches it for no other channel
// (band_class in jaero_hip.hip, computed with the expressions below), and then
//   * the band limit zeroes slots SB .. 31 - SB at compile time and tests thread 0 of slot 32 - SB, nothing else; with the zeros known,
//     the butterflies of the first transform's pass 3 whose outputs land in those slots are never formed, and pass 1 of the second
//     transform is c6_cfft32_band;
//   * the squared signal's spectrum is empty for |k| >= 2 startbin: slots that lie wholly there take the logarithm only if a lane of the
//     wavefront has |X|^2 > 1 (round-off of a very strong input), otherwise log10(fmax(., 1)) / 2 is the +0.0 that c6_log10_half(1) returns;
//   * only the y rows the fold reads are copied to LDS, and the fold's range is constant.
// SB = 0: the generic code, as before.
template <bool W8400, int LOG2N = 14, int SB = 0, int EPB = 0>
__device__ __forceinline__ void coarse6_body(const JGeom g, const JPtrs p, const int *__restrict__ chan_list, int nlist, const double2 *__restrict__ tw)
{
    constexpr int N = 1 << LOG2N;
    constexpr int E = 32;
    constexpr int NT = N / E;                                  // 512 threads for 2^14, 256 for 2^13
    constexpr int XCH = LOG2N == 14 ? C6_XCH : C6_XCH13;
    extern __shared__ __attribute__((aligned(16))) double xch[];
    __shared__ double red_val[NT / 64]; // one entry per wavefront
    __shared__ int red_idx[NT / 64];
    const int t0 = threadIdx.x;
    static_assert(SB == 0 || (!W8400 && LOG2N == 14 && SB >= 1 && SB <= 15 && EPB >= 1), "the band-aware instantiation is the 2^14-point boxcar's");
    const int nchp = g.nchp;
    int tab_startbin = -1; // W8400: the startbin the window table behind the exchange buffer was made for

    CV<E> d;
    int ch_next = ((int)blockIdx.x < nlist) ? (chan_list ? jd_sload(chan_list + blockIdx.x) : (int)blockIdx.x) : 0;
    int bp_next = jd_sload(p.I + (size_t)I_BB_PTR * nchp + ch_next);
    for (int li = blockIdx.x; li < nlist; li += gridDim.x)
    {
        int t = t0; // opaque once per estimate (what derives from it is 1-2 instructions; hoisted out of the persistent loop, ~100 live registers)
        asm volatile("" : "+v"(t));
        const int ch = ch_next, bb_ptr = bp_next;
        const double2 *__restrict__ ring = p.bbring + (size_t)ch * N;
        // the next estimate's channel and ring position: scalar loads (jaero_device.h), requested a whole estimate before the prefetch that
        // needs them
        const int ln = li + (int)gridDim.x;
        const bool has_next = ln < nlist;
        if (has_next)
        {
            ch_next = chan_list ? jd_sload(chan_list + ln) : ln;
            bp_next = jd_sload(p.I + (size_t)I_BB_PTR * nchp + ch_next);
        }
        const double lockingbw = jd_sload(p.S + (size_t)S_LOCKINGBW * nchp + ch);
        double fs_l = g.Fs; // opaque per estimate, as t: hoisted out of the loop Fs / N would be kept (spilled) across it, and a reload's wait
        asm volatile("" : "+s"(fs_l)); // stands behind every vector load in flight (vmcnt counts in order)
        // wave-uniform values that vector instructions compute (there is no scalar fp64): the integers go to scalar registers at once, the
        // doubles are formed again where the epilogue needs them -- left in vector registers they stay live across the three transforms
        // (k_coarse6_w8400 spilled 17 of them until round 4, and a reload's wait stands behind every load in flight)
        int startbin, expectedpeakbin;
        if constexpr (SB > 0) { startbin = SB * NT; expectedpeakbin = EPB; }
        else
        {
            const double hzperbin = fs_l * (1.0 / ((double)N)); // N a power of two: the same bits as the reference's quotient
            startbin = __builtin_amdgcn_readfirstlane((int)fmax(round(lockingbw / hzperbin), 1.0));
            expectedpeakbin = __builtin_amdgcn_readfirstlane((int)round(g.fb / (2.0 * hzperbin)));
        }
        const int stopbin = N - startbin;
        double *__restrict__ y = p.y + (size_t)ch * N;

        // bbtmpbuff[j] = bbcycbuff[(ptr+j)%N] (time order); for every list entry but the first these loads were issued while the
        // previous estimate was in its peak search / state machine
        if (li == (int)blockIdx.x)
        {
#if C6_RINGADDR
            const unsigned boff = ((unsigned)(bb_ptr + t) & (unsigned)(N - 1)) << 4;
#endif
#pragma unroll
            for (int s = 0; s < E; s++)
            {
#if C6_RINGADDR
                const double2 v = *(const double2 *)((const char *)ring + ((boff + (unsigned)(s * NT * 16)) & (unsigned)(N * 16 - 1)));
#else
                const double2 v = ring[(bb_ptr + s * NT + t) & (N - 1)];
#endif
                d.r[s] = v.x; d.i[s] = v.y;
            }
        }
        C6_TRACE(0);
        c6_fft<LOG2N>(d, xch, tw, t);
        C6_TRACE(1);
        // band limit (fb != 8400 boxcar, coarsefreqestimate.cpp:99) then inverse transform = forward on swapped planes
        if constexpr (SB > 0)
        {
#pragma unroll
            for (int s = 0; s < E; s++)
            {
                if (s >= SB && s <= E - 1 - SB) { d.r[s] = 0.0; d.i[s] = 0.0; } // bins startbin .. stopbin - 1
                else if (s == E - SB)                                            // bin stopbin
                {
                    const bool z = t == 0;
                    const double re = z ? 0.0 : d.r[s], im = z ? 0.0 : d.i[s];
                    d.r[s] = im; d.i[s] = re;
                }
                else { const double re = d.r[s]; d.r[s] = d.i[s]; d.i[s] = re; }
            }
        }
        else if constexpr (W8400)
        {
            // window[0] = 1, window[i] = window[N - i] = cos^2(pi/2 * i / startbin) for 1 <= i <= startbin, 0 elsewhere (:61-74).  Its
            // startbin + 1 distinct values come from a table in LDS behind the exchange buffer (entry startbin + 1 = 0 stands for every bin
            // the window zeroes), rebuilt only when startbin changes; a window wider than that space (lockingbw >= 10.49 kHz) is made per
            // estimate in the idle exchange buffer.
            const bool persistent = startbin < C4_TABN - 1;
            double *wt = persistent ? xch + XCH : xch;
            if (!persistent || startbin != tab_startbin)
            {
                jd_lds_barrier();
                c6_build_window(wt, startbin, t, NT);
                jd_lds_barrier();
                if (persistent) tab_startbin = startbin; // (a scalar register: startbin is one)
            }
#pragma unroll
            for (int s0 = 0; s0 < E; s0 += 8)
            {
#pragma unroll
                for (int s = s0; s < s0 + 8; s++)
                {
                    const int k = s * NT + t;
                    const int i = (k <= N / 2) ? k : N - k;
                    const double w = wt[i <= startbin ? i : startbin + 1];
                    const double re = d.r[s] * w, im = d.i[s] * w;
                    d.r[s] = im; d.i[s] = re;
                }
                C6_FENCE;
            }
            if (!persistent) jd_lds_barrier(); // the next transform's exchanges reuse the buffer
        }
        else
        {
#if C6_BAND1
            // one unsigned range test per slot instead of two compares: k in [startbin, stopbin] <=> (unsigned)(k - startbin) <= stopbin -
            // startbin.  A locking bandwidth above Fs / 2 makes the range empty (stopbin < startbin): -1 and 0 match no k >= 0.
            const int band_lo = stopbin < startbin ? -1 : startbin;
            const unsigned band_w = stopbin < startbin ? 0u : (unsigned)(stopbin - startbin);
#endif
#pragma unroll
            for (int s = 0; s < E; s++)
            {
                const int k = s * NT + t;
#if C6_BAND1
                const bool z = (unsigned)(k - band_lo) <= band_w;
#else
                const bool z = (k >= startbin) && (k <= stopbin);
#endif
                const double re = z ? 0.0 : d.r[s], im = z ? 0.0 : d.i[s];
                d.r[s] = im; d.i[s] = re;
            }
        }
        c6_fft<LOG2N, SB>(d, xch, tw, t);
        C6_TRACE(2);
        // swap back (x N / N = 1), square
#pragma unroll
        for (int s = 0; s < E; s++)
        {
            const double re = d.i[s], im = d.r[s];
#if C6_SQFMA
            d.r[s] = __builtin_fma(re, re, -(im * im));
            d.i[s] = 2.0 * (re * im); // the bits of re * im + im * re
#else
            d.r[s] = re * re - im * im;
            d.i[s] = re * im + im * re;
#endif
        }
        c6_fft<LOG2N>(d, xch, tw, t);
        C6_TRACE(3);
        // ---- epilogue.  Round 4 timed it phase by phase (scripts/ubench/coarse_trace.hip): 21 of an estimate's 52 us, most of it latency
        // chains with the whole workgroup waiting -- the fold's range checks as branches (three LDS round trips per candidate bin: 4.2 us), a
        // wavefront reduction through ds_bpermute (0.9 us), thread 0 alone loading the channel's state and evaluating the slot between two
        // barriers (3 us) -- and the rest the CU's own memory phase: a CU gets ~45 GB/s out of loads that miss L2 (the 45 loads behind the y
        // stores take a wavefront 7-8 us to issue), and no registers are free to request any of it a transform earlier (the transform needs
        // 196 of 256; holding 20 y values across it made it slower than the wait they save, touching the lines with one-dword loads cost more
        // issue time than it saved).  What is here now: 13.2 -> 12.4 ms per 65 536 estimates.
        jd_lds_barrier(); // the exchange buffer is free: it receives a copy of y for the fold below
        // smooth with fftshift: y[i] = y[i]*0.9 + 0.1*10*log10(fmax(abs(out[i]),1)), out[i] = X[i ^ N/2]
        // all 32 old y values are requested before the log10s (their registers: the imaginary plane, dead once only |X|^2 is kept); y and the
        // ring are streamed (read once, written once per estimate): non-temporal accesses
        CoarseSlotState cst;
        {
            // One pass per slot: log10, smooth, store, LDS copy -- and, into the four registers that frees, the NEXT estimate's ring entry of
            // that slot.  Requested in one burst behind the barrier, the 32 ring loads (and the 32 y stores in front of them) stalled every
            // wavefront of the workgroup at the same place for 7 us (a CU issues ~45 GB/s of loads that miss L2); spread over the logarithms,
            // one wavefront of a SIMD waits at a load while the other computes (12.6 -> 12.4 ms per 65 536 estimates).
            double yv[E];
            // y[] of the band-aware instantiation: the slot's row from the channel's scalar base, this thread's entry by a 32-bit byte offset
            [[maybe_unused]] unsigned yoff = 0;
            if constexpr (SB > 0 && C6_YADDR) { yoff = (unsigned)t << 3; asm volatile("" : "+v"(yoff)); }
            typedef __attribute__((address_space(1))) char c6_gchar;
            typedef __attribute__((address_space(1))) double c6_gdouble;
            [[maybe_unused]] auto yat = [&](int ib) __attribute__((always_inline)) {
                if constexpr (SB > 0 && C6_YADDR)
                {
                    // the row's base opaque (and still a global pointer), or the rows are formed from one another as 64-bit vector addresses
                    c6_gchar *row = (c6_gchar *)(y + ib);
                    asm volatile("" : "+s"(row));
                    return (c6_gdouble *)(row + yoff);
                }
                else return (c6_gdouble *)((y + ib) + t);
            };
#pragma unroll
#if C6_SQFMA
            for (int s = 0; s < E; s++) d.r[s] = __builtin_fma(d.r[s], d.r[s], d.i[s] * d.i[s]);
#else
            for (int s = 0; s < E; s++) d.r[s] = d.r[s] * d.r[s] + d.i[s] * d.i[s];
#endif
            C6_FENCE; // d.i is dead from here: its registers take the y values
            if constexpr (SB > 0)
            {
#pragma unroll
                for (int s = 0; s < E; s++) yv[s] = __builtin_nontemporal_load(yat((s * NT) ^ (N / 2)));
            }
            else
            {
#pragma unroll
            for (int s = 0; s < E; s++) yv[s] = __builtin_nontemporal_load((y + ((s * NT) ^ (N / 2))) + t); // (s*NT + t) ^ N/2: uniform base + t
            }
            C6_FENCE; // or the scheduler sinks every load to its use again
            // the channel's acquisition state, needed behind the peak search: in front of everything else that is requested below (vmcnt
            // retires in order), as ordinary loads
            cst = coarse_slot_load_v(g, p, ch);
            // laundered: known since the top of the estimate, the 32 ring addresses would otherwise be computed there and kept (spilled) across
            // the three transforms -- and every reload waits for all vector loads in flight
            int bpn = bp_next, chn = ch_next, tp = t;
#if C6_RINGADDR
            asm volatile("" : "+s"(bpn), "+s"(chn), "+v"(tp)); // wave-uniform: the ring's base stays in scalar registers
#else
            asm volatile("" : "+v"(bpn), "+v"(chn), "+v"(tp));
#endif
            // the y copy's rows above 64 KiB: from a base of their own (LOG2N 13: the buffer ends below)
            int tph = tp + ((C6_HIADDR && LOG2N == 14) ? N / 2 : 0);
            if constexpr (C6_HIADDR && LOG2N == 14) asm volatile("" : "+v"(tph));
            constexpr int UPH = (C6_HIADDR && LOG2N == 14) ? N / 2 : 0;
            typedef double c6_v2 __attribute__((ext_vector_type(2)));
            // band-aware instantiation: the slots that take no logarithm, the y rows the fold reads (y[i0 - EPB - 1 .. i1 + EPB]: only they
            // are copied to LDS), and what the slots without a logarithm leave for the pass behind the loop
            [[maybe_unused]] auto skips = [](int s) __attribute__((always_inline)) {
                return SB > 0 && C6_LOGSKIP && C6_LOGHALF && ((s < E / 2) ? (s >= 2 * SB) : (E - 1 - s >= 2 * SB));
            };
            [[maybe_unused]] auto copied = [](int ib) __attribute__((always_inline)) {
                return ib / NT >= (N / 2 - SB * NT - EPB - 1) / NT && ib / NT <= (N / 2 + SB * NT + EPB) / NT;
            };
            [[maybe_unused]] auto ycopy = [&](int ib, double yn) __attribute__((always_inline)) {
                if (UPH && ib >= UPH) (xch + (ib - UPH))[tph] = yn;
                else (xch + ib)[t] = yn;
            };
            [[maybe_unused]] double kx[E], ky[E];
            [[maybe_unused]] bool hot = false;
#if !C6_RINGADDR
            const c6_v2 *__restrict__ ringn = (const c6_v2 *)(p.bbring + (size_t)chn * N);
#endif
#if C6_RINGADDR
            // byte offset of this thread's entry of slot 0, once; a slot adds its constant and wraps in bytes
            const unsigned boffp = ((unsigned)(bpn + tp) & (unsigned)(N - 1)) << 4;
            const char *__restrict__ ringnb = (const char *)(p.bbring + (size_t)chn * N);
#else
            const int toffp = bpn + tp;
#endif
#pragma unroll
            for (int s = 0; s < E; s++)
            {
                const int ib = (s * NT) ^ (N / 2);
                // 0.1*10*log10(max(|X|,1)) -- C multiplies left to right: (0.1 * 10) * log10 = 1.0 * log10 -- == 0.5*log10(max(|X|^2,1)): no
                // hypot.  (Until tests/test_gpu_coarse.py compared y itself this line had 5.0, ten times the reference's increment: the same
                // peak bin as long as every candidate folds six terms, another one when y was 20 and the fold left the spectrum.)
                if constexpr (SB > 0)
                {
                    // a slot wholly outside the squared signal's spectrum (s NT .. s NT + NT - 1 all at |k| >= 2 startbin): its |X|^2 is
                    // round-off, the logarithm's argument 1.0 and its value the +0.0 added here -- unless a lane is above 1 (an input
                    // strong enough for round-off of that size): remembered, and those slots are done again behind the loop
                    double yn;
                    if (skips(s))
                    {
                        yn = yv[s] * 0.9 + 0.0;
                        kx[s] = d.r[s]; ky[s] = yv[s];
                        hot = hot | (d.r[s] > 1.0);
                    }
                    else yn = yv[s] * 0.9 + c6_log10_half(fmax(d.r[s], 1.0));
                    __builtin_nontemporal_store(yn, yat(ib));
                    if (copied(ib)) ycopy(ib, yn);
                }
                else
                {
#if C6_LOGHALF
                const double yn = yv[s] * 0.9 + c6_log10_half(fmax(d.r[s], 1.0));
#else
                const double yn = yv[s] * 0.9 + 0.5 * jd_log10(fmax(d.r[s], 1.0));
#endif
                __builtin_nontemporal_store(yn, (y + ib) + t);
                if (UPH && ib >= UPH) (xch + (ib - UPH))[tph] = yn;
                else (xch + ib)[t] = yn;
                }
                {
                    // unconditional: without a next estimate ch_next / bp_next still name this one (valid memory, result unused) -- under
                    // `if (has_next)` the old contents of d.r[s] had to stay live beside the new ones (151 spilled registers)
#if C6_RINGADDR
                    const c6_v2 v = __builtin_nontemporal_load((const c6_v2 *)(ringnb + ((boffp + (unsigned)(s * NT * 16)) & (unsigned)(N * 16 - 1))));
#else
                    const c6_v2 v = __builtin_nontemporal_load(ringn + ((toffp + s * NT) & (N - 1)));
#endif
                    d.r[s] = v.x; d.i[s] = v.y;
                }
                if ((s & 3) == 3) C6_FENCE; // four slots at a time: the scheduler may not gather the loads at either end again
            }
            if constexpr (SB > 0)
            {
                // rare: a lane of this wavefront had |X|^2 > 1 in a slot that took no logarithm.  Those slots again with it; the second store
                // of a thread to the same address lands behind its first
                if (__builtin_amdgcn_ballot_w64(hot) != 0)
                {
#pragma unroll
                    for (int s = 0; s < E; s++)
                    {
                        if (!skips(s)) continue;
                        const int ib = (s * NT) ^ (N / 2);
                        const double yn = ky[s] * 0.9 + c6_log10_half(fmax(kx[s], 1.0));
                        __builtin_nontemporal_store(yn, yat(ib));
                        if (copied(ib)) ycopy(ib, yn);
                    }
                }
            }
            C6_TRACE(4);
            jd_lds_barrier(); // the fold reads the LDS copy; the stores to y[] drain in the background
            C6_TRACE(5);
        }
        C6_TRACE(6);
        // fold + peak search (:116-131)
        double fs_e = g.Fs; // opaque again: the value above must not be kept for this
        asm volatile("" : "+s"(fs_e));
        const double hzperbin = fs_e * (1.0 / ((double)N));
        int i0, i1;
        if constexpr (SB > 0) { i0 = N / 2 - SB * NT; i1 = N / 2 + SB * NT; }
        else
        {
            i0 = __builtin_amdgcn_readfirstlane((int)round((-lockingbw / hzperbin) + ((double)(N / 2))));
            i1 = __builtin_amdgcn_readfirstlane((int)round((lockingbw / hzperbin) + ((double)(N / 2))));
        }
        static_assert(SB == 0 || ((N / 2 - SB * NT - EPB - 1 >= 0) && (N / 2 + SB * NT + EPB < N)), "the band-aware fold stays inside the spectrum");
        double best = 0;
        int besti = -1;
        // every index the fold touches lies inside the spectrum (always, unless lockingbw + fb/2 reaches Fs/2): no per-term range checks
        const bool fold_inside = (i0 - expectedpeakbin - 1 >= 0) && (i1 + expectedpeakbin < N) && (i0 >= 0);
        if (fold_inside)
        {
            // four candidate bins at a time, straight-line: their 24 LDS reads are requested together
            int nblk = (i1 - i0 + 4 * NT - 1) / (4 * NT);
            if constexpr (SB > 0) asm volatile("" : "+s"(nblk)); // a constant: opaque, so that the loop stays one
            for (int b = 0; b < nblk; b++)
            {
                double val[4];
#pragma unroll
                for (int u = 0; u < 4; u++)
                {
                    const int i = i0 + t + (4 * b + u) * NT;
                    const int ic = i < i1 ? i : i1 - 1;
                    const double *lo = xch + (ic - expectedpeakbin), *hi = xch + (ic + expectedpeakbin);
                    double v = 0;
                    v += (lo[1] + hi[-1]);  // j = -1
                    v += (lo[0] + hi[0]);   // j = 0
                    v += (lo[-1] + hi[1]);  // j = 1
                    val[u] = v;
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                {
                    const int i = i0 + t + (4 * b + u) * NT;
                    const bool take = (i < i1) & (val[u] > best);
                    best = take ? val[u] : best;
                    besti = take ? i : besti;
                }
            }
        }
        else
        {
            for (int i = i0 + t; i < i1; i += NT)
            {
                if ((i < 0) || (i >= N)) continue;
                double val = 0;
                for (int j = -1; j <= 1; j++)
                {
                    if (((i - expectedpeakbin - j) < 0) || ((i + expectedpeakbin + j) >= N)) continue;
                    val += (xch[i - expectedpeakbin - j] + xch[i + expectedpeakbin + j]);
                }
                if (val > best) { best = val; besti = i; }
            }
        }
        C6_TRACE(7);
        // first maximum over the workgroup (ties: the lower bin, as the reference's ascending scan keeps the first): DPP moves inside a
        // wavefront, one LDS round for the wavefronts' results, and then EVERY thread finishes the reduction and evaluates the slot itself
        // (thread 0 writes): no single-thread section with the workgroup waiting at a second barrier behind it, no flag to broadcast, and no
        // barrier that would drain the ring prefetch in flight
        int bigchange;
        {
            double bv = best;
            int bi = besti;
            c6_wave_argmax(bv, bi);
            if ((t & 63) == 0) { red_val[t >> 6] = bv; red_idx[t >> 6] = bi; }
            C6_TRACE(8);
            jd_lds_barrier();
            bv = red_val[0]; bi = red_idx[0];
#pragma unroll
            for (int w = 1; w < NT / 64; w++)
            {
                const double ov = red_val[w];
                const int oi = red_idx[w];
                const bool take = (oi >= 0) & ((bi < 0) | (ov > bv) | ((ov == bv) & (oi < bi)));
                bv = take ? ov : bv;
                bi = take ? oi : bi;
            }
            bigchange = coarse_slot_apply(g, p, ch, cst, (bi >= 0) ? bi : (N / 2), N, hzperbin, lockingbw, t == 0);
            C6_TRACE(9);
        }
        if (bigchange)
        {
            __syncthreads(); // rare (AFC recentre): this estimate's y stores must have landed before other threads overwrite the same rows
            double2 *ringw = p.bbring + (size_t)ch * N;
            for (int i = t; i < N; i += NT) { y[i] = 20; ringw[i] = make_double2(0.0, 0.0); }
        }
        C6_TRACE(10);
        // no barrier here: the next use of LDS is behind the first barrier of the next estimate's transform
    }
}

__global__ __launch_bounds__(C2_THREADS) void k_coarse6(const JGeom g, const JPtrs p, const int *__restrict__ chan_list,
                                                           int nlist, const double2 *__restrict__ tw)
{
    coarse6_body<false>(g, p, chan_list, nlist, tw);
}
// the band-aware instantiation for lockingbw 10.5 kHz at 48 kHz (the defaults of 10.5 kbps): startbin = 7 * 512, expectedpeakbin = 1792
#define C6_B7_SB 7
#define C6_B7_EPB 1792
__global__ __launch_bounds__(C2_THREADS) void k_coarse6_b7(const JGeom g, const JPtrs p, const int *__restrict__ chan_list,
                                                              int nlist, const double2 *__restrict__ tw)
{
    coarse6_body<false, 14, C6_B7_SB, C6_B7_EPB>(g, p, chan_list, nlist, tw);
}
__global__ __launch_bounds__(C2_THREADS) void k_coarse6_w8400(const JGeom g, const JPtrs p, const int *__restrict__ chan_list,
                                                                 int nlist, const double2 *__restrict__ tw)
{
    coarse6_body<true>(g, p, chan_list, nlist, tw);
}
// N = 2^13 (the MSK rates): 256 threads, two workgroups per CU (launch 2 x #CUs workgroups, C6_XCH13 doubles of dynamic LDS each)
__global__ __launch_bounds__(256, 2) void k_coarse6_13(const JGeom g, const JPtrs p, const int *__restrict__ chan_list,
                                                        int nlist, const double2 *__restrict__ tw)
{
    coarse6_body<false, 13>(g, p, chan_list, nlist, tw);
}

// ---- host side of the band-aware kernel.  A 2^14-point bank that is not an 8400 bps bank holds k_coarse6_b7 beside its generic kernel
// (rec.fn = nullptr: the bank has none).  A channel's estimates run it while cls[ch] is 1; lockingbw is live-settable per channel, so every
// writer of S_LOCKINGBW refreshes the byte (update_band_class in jaero_hip.hip: create, jaero_set_settings, the carry-over into a new bank).
// The kernel trusts the class: the host is the only gate.
template <class Rec>
struct CoarseBand
{
    Rec rec;
    std::vector<unsigned char> cls;          // per channel: 1 = in the band kernel's class
    std::vector<int> split;                  // a mixed list of estimates, the band part in front
    bool force_generic = false;              // test switch (jaero_debug_coarse_force_generic): every estimate takes the generic kernel
    long long est_generic = 0, est_band = 0; // estimates launched on either kernel since create (jaero_debug_coarse_band)
};
// 1: a channel with this locking bandwidth belongs to k_coarse6_b7 -- the expressions coarse6_body forms from the same doubles (startbin,
// expectedpeakbin, and the fold's i0 and i1, which round another sum than startbin does) give the kernel's constants
static inline int coarse_band_class_of(int nfft_log2, double Fs, double fb, double lockingbw)
{
    if (nfft_log2 != 14 || fb == 8400) return 0;
    const int N = 1 << 14;
    const double hzperbin = Fs * (1.0 / ((double)N));
    const int startbin = (int)fmax(round(lockingbw / hzperbin), 1.0);
    const int expectedpeakbin = (int)round(fb / (2.0 * hzperbin));
    const int i0 = (int)round((-lockingbw / hzperbin) + ((double)(N / 2)));
    const int i1 = (int)round((lockingbw / hzperbin) + ((double)(N / 2)));
    return startbin == C6_B7_SB * (N / 32) && expectedpeakbin == C6_B7_EPB && i0 == N / 2 - startbin && i1 == N / 2 + startbin;
}
