// wg_fft.h -- the workgroup FFTs: forward complex fp64 transforms of data a workgroup holds in registers (CV<L>), through LDS exchanges,
// natural order in and out.  Three sizes; `xch` is the caller's dynamic LDS, `tw` a table of exp(-2 pi i k / N):
//
//   pf_fft4096<NC>   4096 = 16 x 16 x 16     NC x 256 threads, 16 points each (NC channels side by side)     NC x 4096 doubles of LDS
//                    k_pre8400_fft (k_pre8400.h, NC 4: PF_THREADS, 128 KiB), k_hilbert_fft (k_burst_front.h, NC 4), k_rate_lines* (k_rate_body.h, NC 2: 64 KiB)
//   wg_fft13_e32     8192 = 32 x 16 x 16     256 threads, 32 points each, two workgroups per CU              C6_XCH13 doubles (65 664 bytes)
//                    k_coarse6_13 (k_coarse6.h), k_trident (k_burst_front.h, the output-twiddle form AB 0)
//   wg_fft14_e32     16384 = 32 x 32 x 16    C2_THREADS = 512 threads, 32 points each                        C6_XCH doubles (131 584 bytes)
//                    k_coarse6, k_coarse6_b7, k_coarse6_w8400 (k_coarse6.h, HI), k_chan_fwd (k_chan.h), k_capture_fwd (k_chan_capture.h)
//
// and the register transforms they are made of: regfft<L>, c6_fft32 / c6_cfft32 / c6_afft, the twiddle chains.  The workgroup barrier
// between the LDS exchanges is jd_lds_barrier (jaero_device.h).  Nothing here knows what the data is: the estimator's state machine is
// k_coarse.h, its kernels k_coarse6.h.
#pragma once
#include "jaero_device.h"
#include "fft_consts.h"

#define C2_THREADS 512

template <int L>
struct CV
{
    double r[L], i[L];
};

// y = x * W_64^IDX  (IDX is a compile-time constant after unrolling)
__device__ __forceinline__ void cmul_w64(double &re, double &im, int idx)
{
#pragma clang fp contract(fast)
    idx &= 63;
    if (idx == 0) return;
    if (idx == 16) { const double t = re; re = im; im = -t; return; }   // * (-i)
    if (idx == 32) { re = -re; im = -im; return; }
    if (idx == 48) { const double t = re; re = -im; im = t; return; }   // * (+i)
    const double wr = jd_w64r(idx), wi = jd_w64i(idx); // literals (fft_consts.h), not table loads
    const double nr = re * wr - im * wi;
    const double ni = re * wi + im * wr;
    re = nr; im = ni;
}

// forward DFT of length L held in registers (radix-4 decimation in frequency, radix-2 tail), natural order in & out
template <int L>
__device__ __forceinline__ void regfft(const CV<L> &x, CV<L> &y)
{
#pragma clang fp contract(fast)
    if constexpr (L == 1) { y.r[0] = x.r[0]; y.i[0] = x.i[0]; }
    else if constexpr (L == 2)
    {
        y.r[0] = x.r[0] + x.r[1]; y.i[0] = x.i[0] + x.i[1];
        y.r[1] = x.r[0] - x.r[1]; y.i[1] = x.i[0] - x.i[1];
    }
    else
    {
        constexpr int Q = L / 4;
        CV<Q> u0, u1, u2, u3, z0, z1, z2, z3;
#pragma unroll
        for (int j = 0; j < Q; j++)
        {
            const double ar = x.r[j], ai = x.i[j], br = x.r[j + Q], bi = x.i[j + Q];
            const double cr = x.r[j + 2 * Q], ci = x.i[j + 2 * Q], dr = x.r[j + 3 * Q], di = x.i[j + 3 * Q];
            const double t0r = ar + cr, t0i = ai + ci, t1r = ar - cr, t1i = ai - ci;
            const double t2r = br + dr, t2i = bi + di;
            const double t3r = (bi - di), t3i = -(br - dr); // -i (b - d)
            u0.r[j] = t0r + t2r; u0.i[j] = t0i + t2i;
            double v1r = t1r + t3r, v1i = t1i + t3i, v2r = t0r - t2r, v2i = t0i - t2i, v3r = t1r - t3r, v3i = t1i - t3i;
            cmul_w64(v1r, v1i, j * (64 / L));
            cmul_w64(v2r, v2i, 2 * j * (64 / L));
            cmul_w64(v3r, v3i, 3 * j * (64 / L));
            u1.r[j] = v1r; u1.i[j] = v1i; u2.r[j] = v2r; u2.i[j] = v2i; u3.r[j] = v3r; u3.i[j] = v3i;
        }
        regfft<Q>(u0, z0); regfft<Q>(u1, z1); regfft<Q>(u2, z2); regfft<Q>(u3, z3);
#pragma unroll
        for (int q = 0; q < Q; q++)
        {
            y.r[4 * q + 0] = z0.r[q]; y.i[4 * q + 0] = z0.i[q];
            y.r[4 * q + 1] = z1.r[q]; y.i[4 * q + 1] = z1.i[q];
            y.r[4 * q + 2] = z2.r[q]; y.i[4 * q + 2] = z2.i[q];
            y.r[4 * q + 3] = z3.r[q]; y.i[4 * q + 3] = z3.i[q];
        }
    }
}

// 32-point DFT with a bounded live set: one in-place radix-2 stage, then the two 16-point halves one after the other (regfft<32>
// transforms all 32 points at every level and needs ~256 registers while it does)
__device__ __forceinline__ void regfft32_seq(CV<32> &x, CV<32> &y)
{
#pragma clang fp contract(fast)
    CV<16> lo, hi, z;
#pragma unroll
    for (int j = 0; j < 16; j++)
    {
        const double ar = x.r[j], ai = x.i[j], br = x.r[j + 16], bi = x.i[j + 16];
        lo.r[j] = ar + br; lo.i[j] = ai + bi;
        double dr = ar - br, di = ai - bi;
        cmul_w64(dr, di, 2 * j); // W_32^j
        hi.r[j] = dr; hi.i[j] = di;
    }
    __builtin_amdgcn_sched_barrier(0);
    regfft<16>(lo, z);
#pragma unroll
    for (int q = 0; q < 16; q++) { y.r[2 * q] = z.r[q]; y.i[2 * q] = z.i[q]; }
    __builtin_amdgcn_sched_barrier(0);
    regfft<16>(hi, z);
#pragma unroll
    for (int q = 0; q < 16; q++) { y.r[2 * q + 1] = z.r[q]; y.i[2 * q + 1] = z.i[q]; }
    __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ double2 cmul2(const double2 a, const double2 b)
{
#pragma clang fp contract(fast)
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// tws[k] = base * step^k for k < 32, from two table values, by products of depth <= 6 (no per-element table gathers:
// 64 distinct 16-byte addresses per wave instruction were what bounded the first version of this kernel).
template <int E>
__device__ __forceinline__ void twiddle_powers(const double2 base, const double2 step, double2 (&B)[4], double2 (&A)[8])
{
    const double2 s2 = cmul2(step, step), s3 = cmul2(s2, step), s4 = cmul2(s2, s2);
    B[0] = base; B[1] = cmul2(base, step); B[2] = cmul2(base, s2); B[3] = cmul2(base, s3);
    A[0] = make_double2(1.0, 0.0);
    A[1] = s4; A[2] = cmul2(s4, s4); A[3] = cmul2(A[2], s4); A[4] = cmul2(A[2], A[2]);
    A[5] = cmul2(A[4], s4); A[6] = cmul2(A[3], A[3]); A[7] = cmul2(A[4], A[3]);
}

// v[k] *= step^k (k < 16), the powers by products of depth <= 6 (pf_fft4096's twiddle below)
__device__ __forceinline__ void c4_twiddle16(CV<16> &v, const double2 step) // v[k] *= step^k
{
#pragma clang fp contract(fast)
    double2 B[4], A[8];
    twiddle_powers<16>(make_double2(1.0, 0.0), step, B, A);
#pragma unroll
    for (int k = 1; k < 16; k++)
    {
        const double2 w = (k < 4) ? B[k & 3] : cmul2(A[k >> 2], B[k & 3]);
        const double r = v.r[k] * w.x - v.i[k] * w.y, i = v.r[k] * w.y + v.i[k] * w.x;
        v.r[k] = r; v.i[k] = i;
    }
}

// ---- the 2^14- and 2^13-point transforms with TWO LDS exchanges each: 16384 = 32 x 32 x 16 (round 3).
//
// What round 3 measured: a transform's LDS traffic and its arithmetic do not overlap on this CU however they are
// arranged, so the only way left to shorten one is to move fewer bytes through LDS.  16 x 16 x 16 x 4 needs three exchanges of all 32
// points a thread holds; 32 x 32 x 16 needs two:
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
#define C6_FENCE __builtin_amdgcn_sched_barrier(0)
__device__ __forceinline__ double2 c6_sq(const double2 a)
{
#pragma clang fp contract(fast)
    return make_double2(a.x * a.x - a.y * a.y, 2.0 * (a.x * a.y));
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
template <int AB = C6_ABSORB, bool P1 = (AB > 0), bool HI = false, int ZB = 0>
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
template <int AB = C6_ABSORB, bool P1 = (AB > 0)>
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

// ---- the 4096-point transform of the overlap-save filters (k_pre8400_fft, k_hilbert_fft) and the rate meter.  Thread (c = tid & 3,
// T = tid >> 2): channel c of the workgroup, 256 threads T per channel.
//   4096 = 16 x 16 x 16, 16 points per thread, thread T holds index T + 256 s in slot s on entry AND on exit of a transform:
//     pass 1  n = 256 n1 + n2 (n2 = T): 16-point DFT over n1 -> k1, times W_4096^(n2 k1)
//     exch 1  L = k1 * 256 + 16 m1 + m2          writer T = 16 m1 + m2 slot k1 -> reader T = 16 k1 + m2 slot m1
//     pass 2  16-point DFT over m1 -> q1, times W_256^(m2 q1)
//     exch 2  L = (q1 * 16 + m2) * 16 + (k1 ^ m2) writer T = 16 k1 + m2 slot q1 -> reader T = k1 + 16 q1 slot m2
//     pass 3  16-point DFT over m2 -> q2: X[k1 + 16 q1 + 256 q2] = X[T + 256 s]
//   LDS address = 4 L + c: a wavefront (16 T x 4 c) touches 64 consecutive doubles in every access but the writes of exchange 2, where
//   the swizzle k1 ^ m2 spreads each half wavefront over all banks.  Planes (re, im) go through the buffer one after the other.
//   Not bit-identical to the reference's FFT (JFFT is not vendored; other butterfly order): differences ~1e-16 of the signal peak.
#define PF_THREADS 1024

// NC: channels per workgroup (the LDS address of entry L of channel c is NC L + c); 4 in both overlap-save filters, 2 in k_rate_lines
template <int NC = 4>
__device__ __forceinline__ void pf_exchange1(double (&v)[16], double *xch, int T, int c)
{
    const int wb = T * NC + c, rb = ((T >> 4) * 256 + (T & 15)) * NC + c;
#pragma unroll
    for (int s = 0; s < 16; s++) xch[wb + s * 256 * NC] = v[s];
    jd_lds_barrier();
#pragma unroll
    for (int s = 0; s < 16; s++) v[s] = xch[rb + s * 16 * NC];
    jd_lds_barrier();
}

template <int NC = 4>
__device__ __forceinline__ void pf_exchange2(double (&v)[16], double *xch, int T, int c)
{
    const int hi = T >> 4, lo = T & 15;
    // writer: k1 = hi, m2 = lo, slot q1; reader: q1 = hi, k1 = lo, slot m2
    const int wb = (lo * 16 + (hi ^ lo)) * NC + c;
#pragma unroll
    for (int s = 0; s < 16; s++) xch[wb + s * 256 * NC] = v[s];
    jd_lds_barrier();
#pragma unroll
    for (int s = 0; s < 16; s++) v[s] = xch[((hi * 16 + s) * 16 + (lo ^ s)) * NC + c];
    jd_lds_barrier();
}

template <int NC = 4>
__device__ __forceinline__ void pf_fft4096(CV<16> &d, double *xch, const double2 *__restrict__ tw, int T, int c)
{
#pragma clang fp contract(fast)
    const double2 st1 = tw[T], st2 = tw[16 * (T & 15)];
    CV<16> o;
    regfft<16>(d, o);
    c4_twiddle16(o, st1);
    pf_exchange1<NC>(o.r, xch, T, c);
    pf_exchange1<NC>(o.i, xch, T, c);
    regfft<16>(o, d);
    c4_twiddle16(d, st2);
    pf_exchange2<NC>(d.r, xch, T, c);
    pf_exchange2<NC>(d.i, xch, T, c);
    regfft<16>(d, o);
#pragma unroll
    for (int s = 0; s < 16; s++) { d.r[s] = o.r[s]; d.i[s] = o.i[s]; }
}
