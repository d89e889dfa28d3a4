// bank_geom.h -- the chunk geometry of one k_mix_dec_mfma launch (DecimCore::run_bank_mfma): waves per SIMD the chunks are sized for,
// final outputs per chunk, chunk pairs and workgroups.  Plain C++ (no HIP): tests/test_bank_decimator_host.py compiles it on the host
// to say which geometry each row of tests/bank_cases.py reaches.
#pragma once
#include <algorithm>
#include "decim_route.h"

namespace pg {

struct BankGeom {
    int waves;        // waves per SIMD the chunks are sized for (1 or 2 unless Tuning::bank_waves says otherwise)
    long long L;      // final outputs per chunk, a power of two >= 16
    long long pairs;  // chunk pairs (a wave runs two chunks)
    unsigned n_wg;    // main workgroups, then the history waves'
};

// len_out: final outputs of the call; C: channels; cic: a merged CIC3 in front of the hb11; warm: the instance's warm-up blocks
// ((HY - 8) / 8); minw: the most waves per SIMD its registers allow; has_fin2: the receiver runs two-stage calls; bank_waves, fused_l,
// hist_split: the Tuning fields of the same names
inline BankGeom bank_geometry(long long len_out, long long C, bool cic, int warm, int minw, bool has_fin2, int bank_waves, int fused_l, int hist_split)
{
    auto cdiv = [](long long a, long long b) { return (unsigned)((a + b - 1) / b); };
    const long long g32 = cdiv(C, 32);
    // One wave per SIMD pays the fewest warm-up blocks; two overlap what a lone wave leaves idle (measured on hb11 x 4, 15/19/31: 1200
    // clocks per block alone, 2075 for each of two) -- worth it once a chunk is long against its warm-up: from 128 outputs per chunk on
    int waves = bank_waves;
    // (a receiver that runs two-stage calls keeps one wave per SIMD at every batch size: the previous call's band-pass needs the other
    // half of the register file beside it -- 0.2385 ms per configs[2] call of 32 super-frames against 0.2546, 0.875 against 0.905 at 128)
    if (waves == 0) waves = (!has_fin2 && bank_long_call(len_out, C)) ? 2 : 1;
    if (waves > minw) waves = minw;  // (the instances with the longest halfbands need more than half a SIMD's registers)
    long long pairs_target = 1024LL * waves / g32;
    if (cic) pairs_target /= 2;  // (twelve pairs of lines per output instead of one window: the blocks are bound by what they fetch, and every chunk
                                 // fetches its 30 warm-up blocks again -- measured on configs[3]: 0.081 ms at 1024 waves, 0.075 at 512, 0.12 at 256)
    if (pairs_target < 1) pairs_target = 1;
    // a power of two (it divides the call's 2048 k outputs: the last chunk is a whole one), the nearest to the target above
    long long L = 16;
    if (fused_l > 0) {
        while (L * 2 <= fused_l) L *= 2;
    } else {
        const long long want = cdiv(len_out, 2 * pairs_target);
        while (L < want && L < 2048) L *= 2;
    }
    while (len_out % L != 0 && L > 16) L /= 2;
    while (2 * L <= warm) L *= 2;  // (only the first two chunks may reach in front of the call's start)
    const long long pairs = cdiv(cdiv(len_out, L), 2);
    const unsigned n_wg = (unsigned)(8 * cdiv(pairs, 8) * cdiv(g32, 4) + cdiv(g32, 4) * hist_split);
    return BankGeom{waves, L, pairs, n_wg};
}

}  // namespace pg
