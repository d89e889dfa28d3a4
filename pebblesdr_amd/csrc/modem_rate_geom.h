// modem_rate_geom.h -- the tile rule of one k_modem_rate_pack launch (modem_rate_plan, egress.hip): how many modem-rate outputs a
// workgroup carries through the cascade and how many float2 its two LDS buffers hold, or that no tile fits.  Plain C++ (no HIP):
// tests/test_modem_geom_host.py compiles it on the host to say which tile each row of tests/modem_geom_cases.py reaches.
#pragma once
#include <cstdint>

namespace pg {

struct ModemRateGeom {
    uint32_t tile;          // modem-rate outputs per workgroup: 256, halved down to 4 at the least
    uint32_t lds_a, lds_b;  // float2 of the span's buffer (tile * D + H, even) and of the first stage's outputs (even)
};

// D: the chain's decimation; H: its look-back in demodulator samples; out_spf: modem-rate samples per super-frame; taps0, stride0: the
// chain's first stage.  false: the span of the smallest tile exceeds 4096 samples of LDS (the plan refuses: unsupported)
inline bool modem_rate_geometry(uint64_t D, uint64_t H, uint64_t out_spf, int taps0, uint32_t stride0, ModemRateGeom *g)
{
    // the workgroup's tile: up to 256 outputs, fewer while the span tile * D + H would not fit 4096 samples of LDS
    uint64_t tile = 256;
    while (tile > 4 && tile / 2 >= out_spf) tile /= 2;
    while (tile > 4 && tile * D + H > 4096) tile /= 2;
    const uint64_t a = (tile * D + H + 1) & ~(uint64_t)1;
    if (a > 4096) return false;
    g->tile = (uint32_t)tile;
    g->lds_a = (uint32_t)a;
    g->lds_b = (uint32_t)(((a - taps0) / stride0 + 2) & ~(uint64_t)1);
    return true;
}

}  // namespace pg
