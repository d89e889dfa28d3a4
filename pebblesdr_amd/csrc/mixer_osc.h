// mixer_osc.h -- Mixer::processBlock's oscillator (pebblelib/mixer.cpp:42-81) for one sample of a call: the one device function behind
// the stand-alone mixer (k_mixer, kernels_frontend.h) and the band-pass that mixes in its own loads (k_fastfir_t128_mix,
// kernels_fastfir.h), so that the two routes of a receiver without a decimator rotate a sample by the same value.
#pragma once
#include "common.h"
#include "params.h"

namespace pg {

// sqrt(0.95)-bound amplitude recurrence of the reference's oscillator: a table through its transient, its limit behind it
__device__ __forceinline__ float osc_amp(const float *__restrict__ amp_tab, float a_inf, uint32_t n0, long long i)
{
    unsigned long long k = (unsigned long long)n0 + (unsigned long long)i;
    return k < (unsigned long long)kAmpTab ? amp_tab[k] : a_inf;
}

// the oscillator's value (amplitude included) at sample i of the call: one exact fp64-phase phasor per aligned group of four samples,
// the table step inside the group (the reference advances the phase before it multiplies: sample i carries phase (i + 1) inc)
__device__ __forceinline__ float2 mixer_osc(const ChanOsc *__restrict__ o, double phase0, uint32_t n0, const float *__restrict__ amp_tab, float a_inf, long long i)
{
    const float2 p0 = cis_cycles(phase0 + (double)((i & ~3LL) + 1) * o->inc);
    const float2 ph = cmul(p0, o->step[i & 3]);
    return cscale(ph, osc_amp(amp_tab, a_inf, n0, i));
}

}  // namespace pg
