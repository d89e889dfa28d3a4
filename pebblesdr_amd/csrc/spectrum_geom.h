// spectrum_geom.h -- the frame chains of one display-transform launch (SpectrumCore::run, run_any, run_list_big): a workgroup walks G
// consecutive frames of a stream (SpectrumParams::frames_per_group), every chain but a call's first recomputes the frame in front of it.
// Chain length, chains, workgroups per stream and the chain slots no frame falls into, per kernel family.  Plain C++ (no HIP):
// tests/test_spectrum_chains_host.py compiles it on the host to say which geometry each row of tests/spectrum_cases.py reaches.
#pragma once

namespace pg {

enum class SpecFamily {
    q128,     // k_spectrum_q128: one (chain, q) per 128-item workgroup, placed in stretches of eight chains
    waves,    // k_spectrum<ZP> and k_spectrum_1to1: 4 / ZP chains per 256-item workgroup
    t128,     // k_spectrum_t128<2, ..>: two chains per 1024-item workgroup
    t128_one, // k_spectrum_t128<1, -1>: one chain per 512-item workgroup (T128_STAGGER=0)
    w64,      // k_spectrum_w64: one chain per 256-item workgroup
    any,      // k_spectrum_any: ZP workgroups per chain, ZP = bins / (the frame rounded up to a power of two)
    big,      // k_big256_rows / k_big_rows: eight workgroups per chain, sized by the streams of one batch
};

struct SpectrumGeom {
    int G;             // frames per chain
    long long chains;  // chains per stream that hold a frame: ceil(F / G); the last holds F - (chains - 1) G frames
    int chains_per_wg; // chains one workgroup walks (the ZP or eight workgroups that share one chain count as 1)
    unsigned wgs;      // workgroups launched per stream (grid.x)
    long long surplus; // chain slots of the grid beyond `chains`: wholly dead chains
};

// F: frames per stream of the launch (the listed frames of a gated call); S: streams of the handle; batch: streams of one launch of the
// 65536-point transform (`big` only: its chains are sized by the batch, every other family's by S)
inline SpectrumGeom spectrum_geometry(SpecFamily fam, long long F, long long S, long long bins, long long frame, long long batch)
{
    auto cdiv = [](long long a, long long b) { return (a + b - 1) / b; };
    auto clamp = [](long long g, long long hi) { return g < 1 ? 1 : (g > hi ? hi : g); };
    long long G = 1, per_wg = 1, wgs = 0;
    switch (fam) {
    case SpecFamily::q128: {
        // eight workgroups per CU: aim at 2048 resident workgroups; every chain recomputes one frame, so chains are as long as that allows
        const long long zp = bins / frame;
        G = clamp((F * S * zp) / 2048, 32);
        wgs = 8 * zp * cdiv(cdiv(F, G), 8);
        return SpectrumGeom{(int)G, cdiv(F, G), 1, (unsigned)wgs, 8 * cdiv(cdiv(F, G), 8) - cdiv(F, G)};
    }
    case SpecFamily::waves:
        per_wg = 4 / (bins / frame);               // wave groups (frames in flight) per workgroup
        G = clamp((F * S) / (1024 * per_wg), 16);  // aim for ~1024 workgroups; each group recomputes one extra frame
        wgs = cdiv(F, G * per_wg);
        break;
    case SpecFamily::t128:
    case SpecFamily::t128_one:
        // all workgroups resident at once (2 x 512 items per CU on 256 CUs) when the batch allows: every chain recomputes one frame, so
        // longer chains also mean less repeated work
        per_wg = fam == SpecFamily::t128 ? 2 : 1;
        G = clamp((F * S) / 512, 32);
        wgs = cdiv(cdiv(F, G), per_wg);
        break;
    case SpecFamily::w64:
        G = clamp(cdiv(F * S, 512), 32);  // two workgroups per CU: chains as long as keeps every workgroup resident at once
        wgs = cdiv(F, G);
        break;
    case SpecFamily::any: {
        long long M = 256;
        while (M < frame) M *= 2;
        const long long zp = bins / M;
        G = clamp((F * S * zp) / 1024, 32);  // chains as long as leaves about a thousand workgroups
        return SpectrumGeom{(int)G, cdiv(F, G), 1, (unsigned)(cdiv(F, G) * zp), 0};
    }
    case SpecFamily::big:
        G = clamp((F * batch * 8) / 512, 16);  // prefer chains as long as keeps >= 512 workgroups
        return SpectrumGeom{(int)G, cdiv(F, G), 1, (unsigned)(cdiv(F, G) * 8), 0};
    }
    return SpectrumGeom{(int)G, cdiv(F, G), (int)per_wg, (unsigned)wgs, wgs * per_wg - cdiv(F, G)};
}

}  // namespace pg
