// k_coarse6.h -- the coarse frequency estimator: three workgroup transforms of 2^14 (k_coarse6, _b7, _w8400) or 2^13 points (k_coarse6_13)
// per estimate, chained in registers, and the epilogue behind them.  The transforms are wg_fft14_e32 / wg_fft13_e32 of wg_fft.h.
//
// Same function as k_coarse5 / k_coarse4 (CoarseFreqEstimate::ProcessBasebandData + FreqOffsetEstimateSlot,
// JAERO/coarsefreqestimate.cpp:90-137, JAERO/oqpskdemodulator.cpp:629-677).
#pragma once
#include <vector>
#include "wg_fft.h"
#include "k_coarse.h"

#ifndef C4_TABN
#define C4_TABN 3584 // W8400: window table entries kept in LDS behind the exchange buffer (28 KiB): lockingbw < 10.49 kHz
#endif
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

template <int LOG2N, int ZB = 0>
__device__ __forceinline__ void c6_fft(CV<32> &d, double *xch, const double2 *__restrict__ tw, int t)
{
    static_assert(ZB == 0 || LOG2N == 14, "the band-aware pass 1 exists for the 2^14-point transform");
    int tt = t; // laundered per call: nothing derived from it inside is shared between the three calls of an estimate and kept live
    asm volatile("" : "+v"(tt));
    if constexpr (LOG2N == 14) wg_fft14_e32<C6_ABSORB, (C6_ABSORB > 0), true, ZB>(d, xch, tw, tt); // HI: exchange 2's upper half from bases of its own
    else wg_fft13_e32<C6_ABSORB, (C6_ABSORB > 0)>(d, xch, tw, tt);
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

// The instruction diets behind this body were A/B'd switch by switch; what each kept form was measured against
// is in profiles/coarse_diet.md and profiles/coarse_band.md.
//
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
            // ring entries by a 32-bit byte offset from the scalar base: one add and one mask in bytes per slot
            const unsigned boff = ((unsigned)(bb_ptr + t) & (unsigned)(N - 1)) << 4;
#pragma unroll
            for (int s = 0; s < E; s++)
            {
                const double2 v = *(const double2 *)((const char *)ring + ((boff + (unsigned)(s * NT * 16)) & (unsigned)(N * 16 - 1)));
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
            // one unsigned range test per slot instead of two compares: k in [startbin, stopbin] <=> (unsigned)(k - startbin) <= stopbin -
            // startbin.  A locking bandwidth above Fs / 2 makes the range empty (stopbin < startbin): -1 and 0 match no k >= 0.
            const int band_lo = stopbin < startbin ? -1 : startbin;
            const unsigned band_w = stopbin < startbin ? 0u : (unsigned)(stopbin - startbin);
#pragma unroll
            for (int s = 0; s < E; s++)
            {
                const int k = s * NT + t;
                const bool z = (unsigned)(k - band_lo) <= band_w;
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
            d.r[s] = __builtin_fma(re, re, -(im * im)); // one product and one fused multiply-add
            d.i[s] = 2.0 * (re * im); // the bits of re * im + im * re
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
            // this thread's entry of y row ib: a uniform base + t (rows from scalar bases were built and not kept: profiles/coarse_band.md)
            auto yat = [&](int ib) __attribute__((always_inline)) { return (y + ib) + t; };
#pragma unroll
            for (int s = 0; s < E; s++) d.r[s] = __builtin_fma(d.r[s], d.r[s], d.i[s] * d.i[s]);
            C6_FENCE; // d.i is dead from here: its registers take the y values
#pragma unroll
            for (int s = 0; s < E; s++) yv[s] = __builtin_nontemporal_load(yat((s * NT) ^ (N / 2))); // (s*NT + t) ^ N/2
            C6_FENCE; // or the scheduler sinks every load to its use again
            // the channel's acquisition state, needed behind the peak search: in front of everything else that is requested below (vmcnt
            // retires in order), as ordinary loads
            cst = coarse_slot_load_v(g, p, ch);
            // laundered: known since the top of the estimate, the 32 ring addresses would otherwise be computed there and kept (spilled) across
            // the three transforms -- and every reload waits for all vector loads in flight
            int bpn = bp_next, chn = ch_next, tp = t;
            asm volatile("" : "+s"(bpn), "+s"(chn), "+v"(tp)); // wave-uniform: the ring's base stays in scalar registers
            // the y copy's rows above 64 KiB: from a base of their own (LOG2N 13: the buffer ends below)
            int tph = tp + (LOG2N == 14 ? N / 2 : 0);
            if constexpr (LOG2N == 14) asm volatile("" : "+v"(tph));
            constexpr int UPH = LOG2N == 14 ? N / 2 : 0;
            typedef double c6_v2 __attribute__((ext_vector_type(2)));
            // band-aware instantiation: the slots that take no logarithm, the y rows the fold reads (y[i0 - EPB - 1 .. i1 + EPB]: only they
            // are copied to LDS), and what the slots without a logarithm leave for the pass behind the loop
            [[maybe_unused]] auto skips = [](int s) __attribute__((always_inline)) {
                return SB > 0 && ((s < E / 2) ? (s >= 2 * SB) : (E - 1 - s >= 2 * SB));
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
            // byte offset of this thread's entry of slot 0, once; a slot adds its constant and wraps in bytes
            const unsigned boffp = ((unsigned)(bpn + tp) & (unsigned)(N - 1)) << 4;
            const char *__restrict__ ringnb = (const char *)(p.bbring + (size_t)chn * N);
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
                    // (inline and not ycopy: through the lambda k_coarse6 and k_coarse6_w8400 come out in another schedule)
                    const double yn = yv[s] * 0.9 + c6_log10_half(fmax(d.r[s], 1.0)); // the bits of 0.5 * jd_log10
                    __builtin_nontemporal_store(yn, yat(ib));
                    if (UPH && ib >= UPH) (xch + (ib - UPH))[tph] = yn;
                    else (xch + ib)[t] = yn;
                }
                {
                    // unconditional: without a next estimate ch_next / bp_next still name this one (valid memory, result unused) -- under
                    // `if (has_next)` the old contents of d.r[s] had to stay live beside the new ones (151 spilled registers)
                    const c6_v2 v = __builtin_nontemporal_load((const c6_v2 *)(ringnb + ((boffp + (unsigned)(s * NT * 16)) & (unsigned)(N * 16 - 1))));
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
