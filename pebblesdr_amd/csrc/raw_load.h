// raw_load.h -- a stream still in the device's own sample format, and the loads that convert it (DeviceInterfaceBase::normalizeIQ,
// pebblelib/deviceinterfacebase.cpp:648-838, done in the first loads of the kernels that take the stream instead of a separate pass).
// The kernels include it through params.h.  It is also plain C++: tests/test_receiver_raw_host.py compiles it with g++ and runs every
// loader against the host conversion bit for bit (all byte pairs, all 16-bit values, the float corners, every IQ order).  On the host
// the vector types are the small structs below, __fmul_rn is a product rounded on its own (build with -ffp-contract=off) and
// __uint_as_float a bit copy.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define PG_RAW_FN __device__ __forceinline__
#define PG_RAW_FMUL_RN(a, b) __fmul_rn((a), (b))
#define PG_RAW_UINT_AS_FLOAT(u) __uint_as_float(u)
#else
#define PG_RAW_FN inline
struct char2 { signed char x, y; };
struct uchar2 { unsigned char x, y; };
struct short2 { short x, y; };
struct uint2 { unsigned x, y; };
struct uint4 { unsigned x, y, z, w; };
struct float2 { float x, y; };
struct float4 { float x, y, z, w; };
inline float2 make_float2(float x, float y) { return float2{x, y}; }
inline float pg_raw_host_uint_as_float(unsigned u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
#define PG_RAW_FMUL_RN(a, b) ((a) * (b))
#define PG_RAW_UINT_AS_FLOAT(u) pg_raw_host_uint_as_float(u)
#endif

namespace pg {

// base == nullptr: the float2 pointer is the input.
//   fmt 0 CPX8 int8 pairs, 1 CPXU8 (v - 128), 2 CPX16, 3 CPXFLOAT, 4 WAV PCM16; order 0 IQ, 1 QI, 2 I only, 3 Q only; scale includes the gain
struct RawSrc {
    const void *base;
    int fmt, order;
    float scale;
    int pad_;
};

// the format's constant folded into the gain (deviceinterfacebase.cpp:651,689,729; wavfile.cpp:299-300), rounded once to float
inline float raw_scale(int fmt, double gain)
{
    double scale = gain;
    if (fmt == 0 || fmt == 1) scale *= 1 / 128.0;
    else if (fmt == 2) scale *= 1 / 32768.0;
    else if (fmt == 4) scale *= 1 / 32767.0;
    return (float)scale;
}
constexpr size_t kRawPairBytes[5] = {2, 2, 4, 8, 4};  // bytes per IQ pair: CPX8, CPXU8, CPX16, CPXFLOAT, WAV PCM16

PG_RAW_FN float2 raw_load(const RawSrc &r, long long i)
{
    float a, b;
    if (r.fmt == 0) {
        const char2 v = reinterpret_cast<const char2 *>(r.base)[i];
        a = (float)v.x; b = (float)v.y;
    } else if (r.fmt == 1) {
        const uchar2 v = reinterpret_cast<const uchar2 *>(r.base)[i];
        a = (float)v.x - 128.0f; b = (float)v.y - 128.0f;
    } else if (r.fmt == 2 || r.fmt == 4) {
        const short2 v = reinterpret_cast<const short2 *>(r.base)[i];
        a = (float)v.x; b = (float)v.y;
    } else {
        const float2 v = reinterpret_cast<const float2 *>(r.base)[i];
        a = v.x; b = v.y;
    }
    a *= r.scale;
    b *= r.scale;
    return make_float2((r.order & 1) == 0 ? a : b, (r.order == 1 || r.order == 2) ? a : b);
}

// raw_load with the sample format a template constant, for kernels whose first use of a converted sample is an addition (the band-pass's
// first butterfly): the product with the scale is rounded on its own (__fmul_rn is never contracted into a fused multiply-add), so
// the sample is bit for bit what k_normalize_iq writes
template <int FMT>
PG_RAW_FN float2 raw_load1(const RawSrc &r, long long i)
{
    float a, b;
    if (FMT == 0 || FMT == 1) {  // (the pair as ONE 2-byte load: char2 / uchar2 came out as two byte loads)
        const unsigned w = reinterpret_cast<const unsigned short *>(r.base)[i];
        a = FMT == 0 ? (float)((int)(w << 24) >> 24) : (float)(w & 0xFFu) - 128.0f;
        b = FMT == 0 ? (float)((int)(w << 16) >> 24) : (float)(w >> 8) - 128.0f;
    } else if (FMT == 2 || FMT == 4) {
        const unsigned w = reinterpret_cast<const unsigned *>(r.base)[i];
        a = (float)((int)(w << 16) >> 16);
        b = (float)((int)w >> 16);
    } else {
        const float2 v = reinterpret_cast<const float2 *>(r.base)[i];
        a = v.x; b = v.y;
    }
    a = PG_RAW_FMUL_RN(a, r.scale);
    b = PG_RAW_FMUL_RN(b, r.scale);
    return make_float2((r.order & 1) == 0 ? a : b, (r.order == 1 || r.order == 2) ? a : b);
}

// four consecutive samples i .. i + 3 (i a multiple of 4) in one or two wide loads: 8 bytes for the int8 formats, 16 for int16, 32 for float.
// In two steps, so that a kernel can hold the words as they came (2, 4 or 8 registers) and convert where it uses the samples: a
// conversion behind the load makes the compiler wait for the load there.
template <int FMT>
struct RawQuad {
    uint4 a, b;  // 8-bit formats: a.x, a.y; 16-bit: a; float: a, b
};
template <int FMT>
PG_RAW_FN void raw_fetch4(const RawSrc &r, long long i, RawQuad<FMT> &w)
{
    if (FMT == 0 || FMT == 1) {
        const uint2 v = reinterpret_cast<const uint2 *>(r.base)[i >> 2];
        w.a.x = v.x; w.a.y = v.y;
    } else if (FMT == 2 || FMT == 4) {
        w.a = reinterpret_cast<const uint4 *>(r.base)[i >> 2];
    } else {
        w.a = reinterpret_cast<const uint4 *>(r.base)[i >> 1];
        w.b = reinterpret_cast<const uint4 *>(r.base)[(i >> 1) + 1];
    }
}
template <int FMT>
PG_RAW_FN void raw_convert4(const RawSrc &r, const RawQuad<FMT> &w, float2 (&o)[4])
{
    float v[8];
    if (FMT == 0 || FMT == 1) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const unsigned word = k < 4 ? w.a.x : w.a.y;
            const int sh = 8 * (k & 3);
            v[k] = FMT == 0 ? (float)((int)(word << (24 - sh)) >> 24) : (float)((word >> sh) & 0xFFu) - 128.0f;
        }
    } else if (FMT == 2 || FMT == 4) {
        const unsigned ww[4] = {w.a.x, w.a.y, w.a.z, w.a.w};
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = (float)((int)(ww[k >> 1] << (16 - 16 * (k & 1))) >> 16);
    } else {
        v[0] = PG_RAW_UINT_AS_FLOAT(w.a.x); v[1] = PG_RAW_UINT_AS_FLOAT(w.a.y); v[2] = PG_RAW_UINT_AS_FLOAT(w.a.z); v[3] = PG_RAW_UINT_AS_FLOAT(w.a.w);
        v[4] = PG_RAW_UINT_AS_FLOAT(w.b.x); v[5] = PG_RAW_UINT_AS_FLOAT(w.b.y); v[6] = PG_RAW_UINT_AS_FLOAT(w.b.z); v[7] = PG_RAW_UINT_AS_FLOAT(w.b.w);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float a = v[2 * k] * r.scale, b = v[2 * k + 1] * r.scale;
        o[k] = make_float2((r.order & 1) == 0 ? a : b, (r.order == 1 || r.order == 2) ? a : b);
    }
}
template <int FMT>
PG_RAW_FN void raw_load4(const RawSrc &r, long long i, float2 (&o)[4])
{
    RawQuad<FMT> w;
    raw_fetch4<FMT>(r, i, w);
    raw_convert4<FMT>(r, w, o);
}

// four consecutive samples from an even i that need not be a multiple of 4 (the lean first stage's windows start wherever the stride
// puts them): the 8- and 16-bit formats copy 8 / 16 bytes from the pair's own address, the float format reads two float4 (16-byte
// aligned at every even i)
template <int FMT>
PG_RAW_FN void raw_load4_even(const RawSrc &r, long long i, float2 (&o)[4])
{
    float v[8];
    if (FMT == 0 || FMT == 1) {
        unsigned w[2];
        __builtin_memcpy(w, reinterpret_cast<const unsigned char *>(r.base) + 2 * i, 8);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const unsigned word = w[k >> 2];
            const int sh = 8 * (k & 3);
            v[k] = FMT == 0 ? (float)((int)(word << (24 - sh)) >> 24) : (float)((word >> sh) & 0xFFu) - 128.0f;
        }
    } else if (FMT == 2 || FMT == 4) {
        unsigned w[4];
        __builtin_memcpy(w, reinterpret_cast<const unsigned char *>(r.base) + 4 * i, 16);
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = (float)((int)(w[k >> 1] << (16 - 16 * (k & 1))) >> 16);
    } else {
        const float4 a = reinterpret_cast<const float4 *>(r.base)[i >> 1], b = reinterpret_cast<const float4 *>(r.base)[(i >> 1) + 1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float a = v[2 * k] * r.scale, b = v[2 * k + 1] * r.scale;
        o[k] = make_float2((r.order & 1) == 0 ? a : b, (r.order == 1 || r.order == 2) ? a : b);
    }
}

}  // namespace pg
