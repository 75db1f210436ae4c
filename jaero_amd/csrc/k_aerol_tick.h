// k_aerol_tick.h -- the updateDCD tick of the P-channel and R/T banks, in a header of its own so that tests/host_emul can run it on the CPU; included by
// aerol_host.h where the kernel has always stood.  (The C channel's is k_aerolc_tick_dcd, aerolc.h.)
#pragma once
#include "k_aerol.h"

// = AeroL::updateDCD (aerol.cpp:1109-1122), which the reference drives from a 1 s wall-clock QTimer: the caller ticks it once per
// second of signal time.  dcd_out (optional, [nchannels]) receives the datacd flags afterwards.
__global__ void k_aerol_tick_dcd(const AGeom g, const APtrs p, int *dcd_out)
{
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= g.nch) return;
    int dcdcount = ALD(AI_DCDCOUNT), datacd = ALD(AI_DATACD), ev_cnt = ALD(AI_EV_CNT), overflow = ALD(AI_OVERFLOW);
    if (dcdcount > 0) dcdcount -= 3;
    else if (dcdcount < 0) dcdcount = 0;
    if (datacd && !dcdcount)
    {
        datacd = 0;
        const long long bitidx = ((long long)(unsigned)ALD(AI_NBITS_LO)) | ((long long)ALD(AI_NBITS_HI) << 32);
        aerol_event(g, p, ch, ev_cnt, overflow, bitidx, 0, 0);
    }
    ALD(AI_DCDCOUNT) = dcdcount; ALD(AI_DATACD) = datacd; ALD(AI_EV_CNT) = ev_cnt; ALD(AI_OVERFLOW) = overflow;
    if (dcd_out) dcd_out[ch] = datacd;
}
