// egress.hip -- the egress ring (egress.h), its two packing kernels and the receiver's audio output stage and IQ recording.
#include "receiver.h"
#include "modem_rate_geom.h"

namespace pg {

// ---- kernels ----
// Audio::SendToOutput (audiopa.cpp:304-343) for the selected rows of a call's audio buffer, one launch per call: a work-item takes four
// samples -- two 16-byte loads where the source row is 16-byte aligned, one or two 16-byte stores (8 for the mono format); the ragged
// end of a row and unaligned rows (a resampled buffer's odd pitch) go sample by sample.  Destination rows are 16-byte aligned by
// construction (EgressRing::row_pitch).  FMT: 0 float L, R; 1 PCM16 L, R; 2 PCM16 left only
template <int FMT>
static __global__ __launch_bounds__(256) void k_audio_pack(const float2 *__restrict__ audio, long long pitch, long long n, const EgressRow *__restrict__ tab,
                                                            unsigned char *__restrict__ dst, unsigned long long dst_pitch)
{
    const EgressRow r = tab[blockIdx.y];
    const float2 *src = audio + (long long)r.src * pitch;
    unsigned char *out = dst + (unsigned long long)blockIdx.y * dst_pitch;
    const bool vec = (reinterpret_cast<unsigned long long>(src) & 15ull) == 0;
    for (long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i0 < n; i0 += (long long)gridDim.x * 1024) {
        const int m = n - i0 >= 4 ? 4 : (int)(n - i0);
        float2 v[4];
        if (r.mute) {
            for (int k = 0; k < 4; k++) v[k] = make_float2(0.f, 0.f);
        } else if (vec && m == 4) {
            const float4 a = reinterpret_cast<const float4 *>(src + i0)[0], b = reinterpret_cast<const float4 *>(src + i0)[1];
            v[0] = make_float2(a.x, a.y); v[1] = make_float2(a.z, a.w); v[2] = make_float2(b.x, b.y); v[3] = make_float2(b.z, b.w);
        } else {
            for (int k = 0; k < 4; k++) v[k] = k < m ? src[i0 + k] : make_float2(0.f, 0.f);
        }
        if (!r.mute)  // (a muted row is zeros whatever the samples are, NaN included)
            for (int k = 0; k < 4; k++) v[k] = make_float2(audio_out_sample(v[k].x, r.g), audio_out_sample(v[k].y, r.g));
        if (FMT == 0) {
            float2 *o = reinterpret_cast<float2 *>(out) + i0;
            if (m == 4) {
                reinterpret_cast<float4 *>(o)[0] = make_float4(v[0].x, v[0].y, v[1].x, v[1].y);
                reinterpret_cast<float4 *>(o)[1] = make_float4(v[2].x, v[2].y, v[3].x, v[3].y);
            } else {
                for (int k = 0; k < m; k++) o[k] = v[k];
            }
        } else if (FMT == 1) {
            short2 q[4];
            for (int k = 0; k < 4; k++) q[k] = make_short2(audio_out_s16(v[k].x), audio_out_s16(v[k].y));
            short2 *o = reinterpret_cast<short2 *>(out) + i0;
            if (m == 4) {
                uint4 w;
                memcpy(&w, q, 16);
                *reinterpret_cast<uint4 *>(o) = w;
            } else {
                for (int k = 0; k < m; k++) o[k] = q[k];
            }
        } else {
            short q[4];
            for (int k = 0; k < 4; k++) q[k] = audio_out_s16(v[k].x);
            short *o = reinterpret_cast<short *>(out) + i0;
            if (m == 4) {
                uint2 w;
                memcpy(&w, q, 8);
                *reinterpret_cast<uint2 *>(o) = w;
            } else {
                for (int k = 0; k < m; k++) o[k] = q[k];
            }
        }
    }
}

// WavFile::WriteSamples' conversion (wavfile.cpp:386-388) of the streams a call's chain saw, left = I, right = Q.  RAW: the samples are
// still in the device's format and converted here exactly as k_normalize_iq converts them (raw_load: the same loader, the same scale)
template <bool RAW>
static __global__ __launch_bounds__(256) void k_iq_record(const float2 *__restrict__ iq, long long pitch, RawSrc raw, long long n, unsigned char *__restrict__ dst,
                                                           unsigned long long dst_pitch)
{
    const long long row = blockIdx.y;
    const float2 *src = RAW ? nullptr : iq + row * pitch;
    short2 *out = reinterpret_cast<short2 *>(dst + (unsigned long long)row * dst_pitch);
    const bool vec = !RAW && (reinterpret_cast<unsigned long long>(src) & 15ull) == 0;
    for (long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i0 < n; i0 += (long long)gridDim.x * 1024) {
        const int m = n - i0 >= 4 ? 4 : (int)(n - i0);
        float2 v[4];
        if (vec && m == 4) {
            const float4 a = reinterpret_cast<const float4 *>(src + i0)[0], b = reinterpret_cast<const float4 *>(src + i0)[1];
            v[0] = make_float2(a.x, a.y); v[1] = make_float2(a.z, a.w); v[2] = make_float2(b.x, b.y); v[3] = make_float2(b.z, b.w);
        } else {
            for (int k = 0; k < 4; k++) {
                if (k >= m) v[k] = make_float2(0.f, 0.f);
                else if (RAW) v[k] = raw_load(raw, row * n + i0 + k);  // (streams are stream-major: row r starts at pair r * n)
                else v[k] = src[i0 + k];
            }
        }
        short2 q[4];
        for (int k = 0; k < 4; k++) q[k] = make_short2(iq_record_s16(v[k].x), iq_record_s16(v[k].y));
        if (m == 4) {
            uint4 w;
            memcpy(&w, q, 16);
            *reinterpret_cast<uint4 *>(out + i0) = w;
        } else {
            for (int k = 0; k < m; k++) out[i0 + k] = q[k];
        }
    }
}

// The stream bank's IQ ring: k_iq_record with a row table.  Selected rows of the band-pass output (row r of the block is stream tab[r])
// as they are (S16 false: two 16-byte loads, two 16-byte stores per work-item) or through iq_record_s16 (four pairs, one 16-byte
// store).  A call's n is a multiple of the band-pass block, so rows are 16-byte aligned on both sides; anything else goes sample by
// sample like k_iq_record's ragged end.
// GATED (the bank's squelch): the samples of frame f of row r are replaced by zeros where gate[r * n_frames + f].open == 0 -- 0.0f pairs,
// which iq_record_s16 turns into 0 pairs; an open frame goes through the same loads, conversions and stores as without the gate.
template <bool S16, bool GATED>
__device__ __forceinline__ void iq_pack_body(const float2 *__restrict__ iq, long long pitch, long long n, const uint32_t *__restrict__ tab,
                                             unsigned char *__restrict__ dst, unsigned long long dst_pitch, const StreamGate *__restrict__ gate, long long frame)
{
    const float2 *src = iq + (long long)tab[blockIdx.y] * pitch;
    unsigned char *out = dst + (unsigned long long)blockIdx.y * dst_pitch;
    const bool vec = (reinterpret_cast<unsigned long long>(src) & 15ull) == 0 && (!GATED || (frame & 3) == 0);  // (four samples, one frame)
    const StreamGate *g = GATED ? gate + (long long)blockIdx.y * (n / frame) : nullptr;
    for (long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i0 < n; i0 += (long long)gridDim.x * 1024) {
        if (vec && n - i0 >= 4) {
            float4 a, b;
            if (GATED && !g[i0 / frame].open) {
                a = b = make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                a = reinterpret_cast<const float4 *>(src + i0)[0];
                b = reinterpret_cast<const float4 *>(src + i0)[1];
            }
            if (!S16) {
                float4 *o = reinterpret_cast<float4 *>(reinterpret_cast<float2 *>(out) + i0);
                o[0] = a;
                o[1] = b;
            } else {
                const short2 q0 = make_short2(iq_record_s16(a.x), iq_record_s16(a.y)), q1 = make_short2(iq_record_s16(a.z), iq_record_s16(a.w));
                const short2 q2 = make_short2(iq_record_s16(b.x), iq_record_s16(b.y)), q3 = make_short2(iq_record_s16(b.z), iq_record_s16(b.w));
                uint4 w;
                memcpy(&w.x, &q0, 4); memcpy(&w.y, &q1, 4); memcpy(&w.z, &q2, 4); memcpy(&w.w, &q3, 4);
                *reinterpret_cast<uint4 *>(reinterpret_cast<short2 *>(out) + i0) = w;
            }
        } else {  // (no registers indexed by a run-time count: that would cost the kernel LDS)
            for (long long i = i0; i < n && i < i0 + 4; i++) {
                const float2 v = (GATED && !g[i / frame].open) ? make_float2(0.f, 0.f) : src[i];
                if (!S16) reinterpret_cast<float2 *>(out)[i] = v;
                else reinterpret_cast<short2 *>(out)[i] = make_short2(iq_record_s16(v.x), iq_record_s16(v.y));
            }
        }
    }
}

template <bool S16>
static __global__ __launch_bounds__(256) void k_iq_pack(const float2 *__restrict__ iq, long long pitch, long long n, const uint32_t *__restrict__ tab,
                                                         unsigned char *__restrict__ dst, unsigned long long dst_pitch)
{
    iq_pack_body<S16, false>(iq, pitch, n, tab, dst, dst_pitch, nullptr, 1);
}
template <bool S16>
static __global__ __launch_bounds__(256) void k_iq_pack_gated(const float2 *__restrict__ iq, long long pitch, long long n, const uint32_t *__restrict__ tab,
                                                               unsigned char *__restrict__ dst, unsigned long long dst_pitch,
                                                               const StreamGate *__restrict__ gate, long long frame)
{
    iq_pack_body<S16, true>(iq, pitch, n, tab, dst, dst_pitch, gate, frame);
}

// The modem hook ring: the rows DigitalModemInterface::processBlock receives (receiver.cpp:979-980), behind the noise filter and ahead of
// the AGC, for the selected channels (row r of the block is channel tab[r] & ~kModemRowTuneOnly), and the block's trailer in the same
// launch.  A (row, super-frame) the reference never hands to the hook -- the bank's gate closed it (receiver.cpp:962-965), or the channel
// is in dmNONE (:968-971) -- is absent: zeros instead of the samples (0.0f pairs, which iq_record_s16 turns into 0 pairs) and flag 0 in
// trailer[r * n_sf + j]; a present one goes through k_iq_pack's loads, conversions and stores.  Every lane moves 16 bytes per access:
// F32 one 16-byte load and one 16-byte store of two samples (consecutive lanes, consecutive 16 bytes, both ways), S16 two 16-byte loads
// and one 16-byte store of four.  Rows whose source is not 16-byte aligned, or whose super-frame is no multiple of the lane's samples, go
// sample by sample.  The trailer (and its padding to 16 bytes) is written by the first workgroup of each row.
template <bool S16>
static __global__ __launch_bounds__(256) void k_modem_pack(const float2 *__restrict__ iq, long long pitch, int spf, int n_sf, const uint32_t *__restrict__ tab,
                                                            const unsigned char *__restrict__ gate, int gate_stride, unsigned char *__restrict__ dst,
                                                            unsigned long long dst_pitch)
{
    constexpr int SPL = S16 ? 4 : 2;  // samples per lane and step
    const uint32_t e = tab[blockIdx.y], ch = e & ~kModemRowTuneOnly;
    const bool tune_only = (e & kModemRowTuneOnly) != 0;
    const unsigned n = (unsigned)spf * (unsigned)n_sf;  // (run_modem_pack: below 2^31)
    const float2 *src = iq + (long long)ch * pitch;
    unsigned char *out = dst + (unsigned long long)blockIdx.y * dst_pitch;
    const unsigned char *g = gate ? gate + (long long)ch * gate_stride : nullptr;
    const bool whole = !tune_only && !g;  // every super-frame of the row is present: no look-up per step
    if (blockIdx.x == 0) {
        unsigned char *trailer = dst + (unsigned long long)gridDim.y * dst_pitch;
        for (int j = threadIdx.x; j < n_sf; j += 256) trailer[(unsigned long long)blockIdx.y * n_sf + j] = (!tune_only && (!g || g[j])) ? 1 : 0;
        if (blockIdx.y == 0) {
            const unsigned used = gridDim.y * (unsigned)n_sf, padded = (used + 15u) & ~15u;
            for (unsigned i = used + threadIdx.x; i < padded; i += 256) trailer[i] = 0;
        }
    }
    const bool vec = (reinterpret_cast<unsigned long long>(src) & 15ull) == 0 && spf % SPL == 0;  // (SPL samples, one super-frame; n % SPL == 0)
    for (unsigned i0 = (blockIdx.x * 256u + threadIdx.x) * SPL; i0 < n; i0 += gridDim.x * 256u * SPL) {
        if (vec) {
            const bool present = whole || (!tune_only && g[i0 / (unsigned)spf]);
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (present) {
                a = reinterpret_cast<const float4 *>(src + i0)[0];
                if (S16) b = reinterpret_cast<const float4 *>(src + i0)[1];
            }
            if (!S16) {
                *reinterpret_cast<float4 *>(reinterpret_cast<float2 *>(out) + i0) = a;
            } else {
                const short2 q0 = make_short2(iq_record_s16(a.x), iq_record_s16(a.y)), q1 = make_short2(iq_record_s16(a.z), iq_record_s16(a.w));
                const short2 q2 = make_short2(iq_record_s16(b.x), iq_record_s16(b.y)), q3 = make_short2(iq_record_s16(b.z), iq_record_s16(b.w));
                uint4 w;
                memcpy(&w.x, &q0, 4); memcpy(&w.y, &q1, 4); memcpy(&w.z, &q2, 4); memcpy(&w.w, &q3, 4);
                *reinterpret_cast<uint4 *>(reinterpret_cast<short2 *>(out) + i0) = w;
            }
        } else {
            for (unsigned i = i0; i < n && i < i0 + SPL; i++) {
                const bool present = whole || (!tune_only && g[i / (unsigned)spf]);
                const float2 v = present ? src[i] : make_float2(0.f, 0.f);
                if (!S16) reinterpret_cast<float2 *>(out)[i] = v;
                else reinterpret_cast<short2 *>(out)[i] = make_short2(iq_record_s16(v.x), iq_record_s16(v.y));
            }
        }
    }
}

// The same block at a modem rate: every present (row, super-frame) through the reference's Decimator chain for the ring's (max_bw,
// min_rate) -- pebblelib/decimator.cpp, vDSP path, as design::build_chain merges it; stage by stage k_morse_fir's arithmetic,
// out[o] = sum_p h[p] x[o stride - (T - 1) + p] with fmaf in tap order -- in ONE launch.  grid (tiles of modem-rate outputs, block rows,
// super-frames of the call); a workgroup carries one tile of one (row, super-frame) through the whole cascade in LDS:
//   load   tile * D + H demodulator samples: the tile's own and the H in front of them (16-byte loads where the row allows);
//   stages ping-pong between two LDS buffers; in local indices stage j is out[q] = sum_p h[p] in[q stride_j + p], because the span starts
//          exactly H = sum_j (T_j - 1) prod_{i<j} stride_i samples early and every stage's own look-back is the tail of that sum;
//   store  16 bytes per lane (two float pairs, or four PCM16 pairs by iq_record_s16).
// No per-stage state: a super-frame is a multiple of D, so recomputing every stage from the H raw samples in front of a segment IS the
// streaming decimator.  Those H samples are the tail of the nearest present super-frame j' < j of this call, still in the audio rows
// (the row's gate bytes say which), or, where there is none, the row's carry.  The carry is double-buffered by launch parity: every
// workgroup reads carry_in; the workgroup that owns the last tile of the row's last present super-frame writes carry_out from that
// super-frame's last H inputs; the first workgroup of a row without a present pair copies carry_in to carry_out.  The host flips the
// parity per launch, a dropped block launches nothing: the state stands still over what was not delivered.  Absent pairs store zeros
// and flag 0 and read nothing.  The first workgroup of each row writes the row's trailer flags, that of row 0 the trailer's padding.
// LDS: [lds_a float2][lds_b float2][n_stages * kMaxTaps float] (modem_rate_plan sizes it: under 64 KiB)
template <bool S16>
static __global__ __launch_bounds__(256) void k_modem_rate_pack(const float2 *__restrict__ iq, long long pitch, int spf, int n_sf,
                                                                 const uint32_t *__restrict__ tab, const unsigned char *__restrict__ gate, int gate_stride,
                                                                 unsigned char *__restrict__ dst, unsigned long long dst_pitch, ModemRateChain c,
                                                                 const float *__restrict__ taps, const float2 *__restrict__ carry_in,
                                                                 float2 *__restrict__ carry_out)
{
    constexpr int SPL = S16 ? 4 : 2;  // samples per lane and 16-byte store
    extern __shared__ float4 lds_rate[];
    float2 *A = reinterpret_cast<float2 *>(lds_rate), *B = A + c.lds_a;
    const int tid = threadIdx.x, r = blockIdx.y, j = blockIdx.z;
    const uint32_t e = tab[r], chn = e & ~kModemRowTuneOnly;
    const bool tune_only = (e & kModemRowTuneOnly) != 0;
    const float2 *src = iq + (long long)chn * pitch;
    const unsigned char *g = gate ? gate + (long long)chn * gate_stride : nullptr;
    const int D = c.D, H = c.H, m = spf / D;  // m modem-rate samples per super-frame
    const int o0 = (int)blockIdx.x * c.tile, tn = m - o0 < c.tile ? m - o0 : c.tile;
    // the row's present super-frames (uniform over the workgroup): the nearest one in front of j, and whether one follows
    int jprev = -1, any = 0, later = 0;
    for (int q = 0; q < n_sf; q++) {
        const int p = (!tune_only && (!g || g[q])) ? 1 : 0;
        any |= p;
        if (p && q < j) jprev = q;
        if (p && q > j) later = 1;
    }
    const bool present = !tune_only && (!g || g[j]);
    if (blockIdx.x == 0 && j == 0) {
        unsigned char *trailer = dst + (unsigned long long)gridDim.y * dst_pitch;
        for (int q = tid; q < n_sf; q += 256) trailer[(unsigned long long)r * n_sf + q] = (!tune_only && (!g || g[q])) ? 1 : 0;
        if (r == 0) {
            const unsigned used = gridDim.y * (unsigned)n_sf, padded = (used + 15u) & ~15u;
            for (unsigned i = used + tid; i < padded; i += 256) trailer[i] = 0;
        }
        if (!any)  // nothing of this row is delivered in this call: its history stands still
            for (int i = tid; i < H; i += 256) carry_out[(long long)r * H + i] = carry_in[(long long)r * H + i];
    }
    unsigned char *out = dst + (unsigned long long)r * dst_pitch;
    const long long at = (long long)j * m + o0;  // the tile's first sample of the block row
    const bool vec_out = m % SPL == 0 && c.tile % SPL == 0;  // (then o0, tn and `at` are multiples of SPL; block rows are 16-byte aligned)
    if (!present) {
        if (vec_out) {
            for (int q = tid * SPL; q < tn; q += 256 * SPL) {
                if (!S16) *reinterpret_cast<float4 *>(reinterpret_cast<float2 *>(out) + at + q) = make_float4(0.f, 0.f, 0.f, 0.f);
                else *reinterpret_cast<uint4 *>(reinterpret_cast<short2 *>(out) + at + q) = make_uint4(0u, 0u, 0u, 0u);
            }
        } else {
            for (int q = tid; q < tn; q += 256) {
                if (!S16) reinterpret_cast<float2 *>(out)[at + q] = make_float2(0.f, 0.f);
                else reinterpret_cast<short2 *>(out)[at + q] = make_short2(0, 0);
            }
        }
        return;
    }
    float *h = reinterpret_cast<float *>(B + c.lds_b);
    for (int i = tid; i < c.n_stages * kMaxTaps; i += 256) h[i] = taps[i];
    // the span: position p = o0 D - H + i of super-frame j, i in [0, tn D + H); p < 0 reaches into the look-back
    const int n0 = tn * D + H, p0 = o0 * D - H;
    const float2 *cur = src + (long long)j * spf;
    const float2 *back = jprev >= 0 ? src + (long long)(jprev + 1) * spf : carry_in + (long long)r * H + H;  // back[p], p in [-H, 0)
    // pairs of samples by one 16-byte load: the row, the super-frame, the span's start and the look-back are all even then
    const bool vec_in = (reinterpret_cast<unsigned long long>(src) & 15ull) == 0 && ((spf | p0 | H | n0) & 1) == 0;
    if (vec_in) {
        for (int i = tid * 2; i < n0; i += 512) {
            const int p = p0 + i;
            *reinterpret_cast<float4 *>(A + i) = *reinterpret_cast<const float4 *>((p >= 0 ? cur : back) + p);
        }
    } else {
        for (int i = tid; i < n0; i += 256) {
            const int p = p0 + i;
            A[i] = (p >= 0 ? cur : back)[p];
        }
    }
    __syncthreads();
    if (!later && o0 + tn == m)  // the row's last delivered samples: the next launch's look-back where it has no present pair in front
        for (int i = tid; i < H; i += 256) carry_out[(long long)r * H + i] = A[n0 - H + i];
    float2 *in = A, *res = B;
    int n = n0;
    for (int s = 0; s < c.n_stages; s++) {
        const int T = c.taps[s], st = c.stride[s];
        const int n_out = s == c.n_stages - 1 ? tn : (n - T) / st + 1;
        const float *hs = h + s * kMaxTaps;
        for (int q = tid; q < n_out; q += 256) {
            const float2 *x = in + q * st;
            float2 acc = make_float2(0.f, 0.f);
            for (int p = 0; p < T; p++) {
                const float2 v = x[p];
                acc.x = fmaf(v.x, hs[p], acc.x);
                acc.y = fmaf(v.y, hs[p], acc.y);
            }
            res[q] = acc;
        }
        __syncthreads();
        float2 *t = in; in = res; res = t;
        n = n_out;
    }
    if (vec_out) {
        for (int q = tid * SPL; q < tn; q += 256 * SPL) {
            const float4 a = *reinterpret_cast<const float4 *>(in + q);
            if (!S16) {
                *reinterpret_cast<float4 *>(reinterpret_cast<float2 *>(out) + at + q) = a;
            } else {
                const float4 b = *reinterpret_cast<const float4 *>(in + q + 2);
                const short2 q0 = make_short2(iq_record_s16(a.x), iq_record_s16(a.y)), q1 = make_short2(iq_record_s16(a.z), iq_record_s16(a.w));
                const short2 q2 = make_short2(iq_record_s16(b.x), iq_record_s16(b.y)), q3 = make_short2(iq_record_s16(b.z), iq_record_s16(b.w));
                uint4 w;
                memcpy(&w.x, &q0, 4); memcpy(&w.y, &q1, 4); memcpy(&w.z, &q2, 4); memcpy(&w.w, &q3, 4);
                *reinterpret_cast<uint4 *>(reinterpret_cast<short2 *>(out) + at + q) = w;
            }
        }
    } else {
        for (int q = tid; q < tn; q += 256) {
            const float2 v = in[q];
            if (!S16) reinterpret_cast<float2 *>(out)[at + q] = v;
            else reinterpret_cast<short2 *>(out)[at + q] = make_short2(iq_record_s16(v.x), iq_record_s16(v.y));
        }
    }
}

static unsigned pack_blocks(long long n)
{
    long long b = (n + 1023) / 1024;
    return (unsigned)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

int run_audio_pack(hipStream_t s, const float2 *audio, long long pitch, long long n, const EgressRow *d_tab, uint32_t rows, int format, void *dst,
                   uint64_t dst_pitch)
{
    if (n <= 0 || rows == 0) return 0;
    const dim3 grid(pack_blocks(n), rows);
    unsigned char *o = (unsigned char *)dst;
    if (format == PEBBLEGPU_AUDIO_F32) launch(k_audio_pack<0>, grid, dim3(256), s, audio, pitch, n, d_tab, o, (unsigned long long)dst_pitch);
    else if (format == PEBBLEGPU_AUDIO_S16) launch(k_audio_pack<1>, grid, dim3(256), s, audio, pitch, n, d_tab, o, (unsigned long long)dst_pitch);
    else launch(k_audio_pack<2>, grid, dim3(256), s, audio, pitch, n, d_tab, o, (unsigned long long)dst_pitch);
    PG_HIP(hipGetLastError());
    return 0;
}

int run_iq_record(hipStream_t s, const float2 *iq, long long pitch, const RawSrc *raw, long long n, uint32_t rows, void *dst, uint64_t dst_pitch)
{
    if (n <= 0 || rows == 0) return 0;
    const dim3 grid(pack_blocks(n), rows);
    unsigned char *o = (unsigned char *)dst;
    if (raw) launch(k_iq_record<true>, grid, dim3(256), s, (const float2 *)nullptr, 0LL, *raw, n, o, (unsigned long long)dst_pitch);
    else launch(k_iq_record<false>, grid, dim3(256), s, iq, pitch, RawSrc{nullptr, 0, 0, 0.f, 0}, n, o, (unsigned long long)dst_pitch);
    PG_HIP(hipGetLastError());
    return 0;
}

int run_iq_pack(hipStream_t s, const float2 *iq, long long pitch, long long n, const uint32_t *d_tab, uint32_t rows, int format, void *dst, uint64_t dst_pitch,
                const StreamGate *gate, long long frame)
{
    if (n <= 0 || rows == 0) return 0;
    const dim3 grid(pack_blocks(n), rows);
    unsigned char *o = (unsigned char *)dst;
    if (gate) {
        if (frame <= 0 || n % frame) return fail(PEBBLEGPU_E_INVALID, "a gated block of %lld samples in frames of %lld", n, frame);
        if (format == PEBBLEGPU_AUDIO_F32) launch(k_iq_pack_gated<false>, grid, dim3(256), s, iq, pitch, n, d_tab, o, (unsigned long long)dst_pitch, gate, frame);
        else launch(k_iq_pack_gated<true>, grid, dim3(256), s, iq, pitch, n, d_tab, o, (unsigned long long)dst_pitch, gate, frame);
    } else if (format == PEBBLEGPU_AUDIO_F32) {
        launch(k_iq_pack<false>, grid, dim3(256), s, iq, pitch, n, d_tab, o, (unsigned long long)dst_pitch);
    } else {
        launch(k_iq_pack<true>, grid, dim3(256), s, iq, pitch, n, d_tab, o, (unsigned long long)dst_pitch);
    }
    PG_HIP(hipGetLastError());
    return 0;
}

int run_modem_pack(hipStream_t s, const float2 *iq, long long pitch, long long spf, int n_sf, const uint32_t *d_tab, uint32_t rows, int format,
                   const unsigned char *gate, int gate_stride, void *dst, uint64_t dst_pitch)
{
    if (spf <= 0 || n_sf <= 0 || rows == 0) return 0;
    const long long n = spf * n_sf;
    if (n >= (1LL << 31)) return fail(PEBBLEGPU_E_SIZE, "a modem block of %lld samples per row", n);
    const int spl = format == PEBBLEGPU_AUDIO_F32 ? 2 : 4;
    long long b = (n + 256 * spl - 1) / (256 * spl);
    const dim3 grid((unsigned)(b > 1024 ? 1024 : b), rows);
    unsigned char *o = (unsigned char *)dst;
    if (format == PEBBLEGPU_AUDIO_F32) launch(k_modem_pack<false>, grid, dim3(256), s, iq, pitch, (int)spf, n_sf, d_tab, gate, gate_stride, o, (unsigned long long)dst_pitch);
    else launch(k_modem_pack<true>, grid, dim3(256), s, iq, pitch, (int)spf, n_sf, d_tab, gate, gate_stride, o, (unsigned long long)dst_pitch);
    PG_HIP(hipGetLastError());
    return 0;
}

// the chain for (demod_rate, max_bw, min_rate) and what the ring at a modem rate refuses; spf: demodulator samples per super-frame
int modem_rate_plan(uint32_t demod_rate, uint64_t spf, uint32_t max_bw, uint32_t min_rate, ModemRatePlan *out)
{
    if (max_bw == 0) return fail(PEBBLEGPU_E_INVALID, "a modem bandwidth of 0 Hz");
    if (demod_rate == 0) return fail(PEBBLEGPU_E_INVALID, "a demodulator rate of 0");
    ModemRatePlan p;
    p.chain = design::build_chain(demod_rate, max_bw, min_rate);  // min_rate 0: minDecimatedSampleRate (15000), as buildDecimationChain
    p.rate_int = (uint32_t)(int)p.chain.rate;
    if (p.chain.stages.size() > (size_t)kMaxStages) return fail(PEBBLEGPU_E_UNSUPPORTED, "a modem chain of %zu stages; at most %d are built", p.chain.stages.size(), kMaxStages);
    for (const design::Stage &st : p.chain.stages) {
        if (st.ntaps == 0)
            return fail(PEBBLEGPU_E_UNSUPPORTED, "the chain for (%u Hz, %u Hz) at %u samples/s contains a CIC3 stage (by %u): the merged CIC3's two-sample form is not built here",
                        max_bw, min_rate, demod_rate, st.stride);
        if (st.ntaps < 1 || st.ntaps > kMaxTaps) return fail(PEBBLEGPU_E_UNSUPPORTED, "a modem stage of %d taps", st.ntaps);
    }
    const uint64_t D = p.chain.total;
    if (spf % D != 0) return fail(PEBBLEGPU_E_SIZE, "a super-frame of %llu demodulator samples is no multiple of the modem chain's decimation by %llu",
                                  (unsigned long long)spf, (unsigned long long)D);
    uint64_t len = spf, scale = 1, H = 0;
    for (const design::Stage &st : p.chain.stages) {
        if (len < (uint64_t)st.ntaps)  // Decimator::process's fallback for short frames (decimator.cpp:602-625) would drop samples unfiltered
            return fail(PEBBLEGPU_E_SIZE, "a super-frame of %llu demodulator samples gives the modem chain's %d-tap stage %llu inputs", (unsigned long long)spf,
                        st.ntaps, (unsigned long long)len);
        H += (uint64_t)(st.ntaps - 1) * scale;
        scale *= st.stride;
        len /= st.stride;
    }
    if (H > spf) return fail(PEBBLEGPU_E_SIZE, "the modem chain looks back %llu demodulator samples, more than one super-frame of %llu", (unsigned long long)H,
                             (unsigned long long)spf);
    p.lookback = (uint32_t)H;
    p.out_spf = spf / D;
    if (!p.chain.stages.empty()) {
        ModemRateGeom g;  // the workgroup's tile and its two LDS buffers: modem_rate_geom.h
        if (!modem_rate_geometry(D, H, p.out_spf, p.chain.stages[0].ntaps, p.chain.stages[0].stride, &g))
            return fail(PEBBLEGPU_E_UNSUPPORTED, "a modem chain that decimates by %llu with a look-back of %llu samples exceeds the packing kernel's LDS tile",
                        (unsigned long long)D, (unsigned long long)H);
        p.tile = g.tile;
        p.lds_a = g.lds_a;
        p.lds_b = g.lds_b;
    }
    *out = p;
    return 0;
}

int run_modem_rate_pack(hipStream_t s, const float2 *iq, long long pitch, long long spf, int n_sf, const uint32_t *d_tab, uint32_t rows, int format,
                        const unsigned char *gate, int gate_stride, void *dst, uint64_t dst_pitch, const ModemRatePlan &plan, const float *d_taps,
                        float2 *d_carry, int parity)
{
    if (spf <= 0 || n_sf <= 0 || rows == 0) return 0;
    if ((uint64_t)spf != plan.out_spf * plan.chain.total || plan.tile == 0) return fail(PEBBLEGPU_E_SIZE, "a super-frame of %lld samples is not what the modem ring was opened for", spf);
    if (spf * n_sf >= (1LL << 31)) return fail(PEBBLEGPU_E_SIZE, "a modem block of %lld samples per row", spf * n_sf);
    ModemRateChain c;
    memset(&c, 0, sizeof(c));
    c.n_stages = (int)plan.chain.stages.size();
    c.D = (int)plan.chain.total;
    c.H = (int)plan.lookback;
    c.tile = (int)plan.tile;
    c.lds_a = (int)plan.lds_a;
    c.lds_b = (int)plan.lds_b;
    for (int j = 0; j < c.n_stages; j++) { c.taps[j] = plan.chain.stages[j].ntaps; c.stride[j] = (int)plan.chain.stages[j].stride; }
    const size_t lds = sizeof(float2) * ((size_t)plan.lds_a + plan.lds_b) + sizeof(float) * (size_t)c.n_stages * kMaxTaps;
    const dim3 grid((unsigned)((plan.out_spf + plan.tile - 1) / plan.tile), rows, (unsigned)n_sf);
    const size_t half = (size_t)rows * plan.lookback;
    const float2 *cin = d_carry + (parity ? half : 0);
    float2 *cout = d_carry + (parity ? 0 : half);
    unsigned char *o = (unsigned char *)dst;
    if (format == PEBBLEGPU_AUDIO_F32)
        launch_lds(k_modem_rate_pack<false>, grid, dim3(256), lds, s, iq, pitch, (int)spf, n_sf, d_tab, gate, gate_stride, o, (unsigned long long)dst_pitch, c, d_taps, cin, cout);
    else
        launch_lds(k_modem_rate_pack<true>, grid, dim3(256), lds, s, iq, pitch, (int)spf, n_sf, d_tab, gate, gate_stride, o, (unsigned long long)dst_pitch, c, d_taps, cin, cout);
    PG_HIP(hipGetLastError());
    return 0;
}

// ---- EgressRing ----
int EgressRing::open_ring(uint32_t slots, uint32_t n_rows, uint32_t bps, uint64_t max_n, uint32_t fmt, uint64_t extra_bytes)
{
    format = fmt;
    n_slots = slots;
    rows = n_rows;
    bytes_per_sample = bps;
    max_samples = max_n;
    slot_bytes = (uint64_t)n_rows * row_pitch(max_n, bps) + extra_bytes;
    if (!copy_stream) PG_HIP(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
    for (uint32_t i = 0; i < n_slots; i++) {
        EgressSlot &g = slot[i];
        g = EgressSlot{};
        PG_TRY(g.h.alloc(slot_bytes));
        PG_TRY(g.d.alloc(slot_bytes));
        PG_HIP(hipEventCreateWithFlags(&g.packed, hipEventDisableTiming));
        PG_HIP(hipEventCreateWithFlags(&g.copied, hipEventDisableTiming));
    }
    calls = head = tail = read = dropped = 0;
    dropped_run = 0;
    open = true;
    return 0;
}

void EgressRing::release()
{
    if (copy_stream) (void)hipStreamSynchronize(copy_stream);
    for (EgressSlot &g : slot) {
        if (g.packed) (void)hipEventDestroy(g.packed);
        if (g.copied) (void)hipEventDestroy(g.copied);
        g = EgressSlot{};
    }
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    copy_stream = nullptr;
    open = false;
    n_slots = 0;
}

void EgressRing::close_ring()
{
    std::unique_lock<std::mutex> lk(mu);
    open = false;  // (a reader that comes back from its wait finds the ring closed and leaves without touching a slot)
    cv.wait(lk, [this] { return !reader_waiting; });
    release();
}

EgressSlot *EgressRing::begin()
{
    std::lock_guard<std::mutex> lk(mu);
    const uint64_t call = calls++;
    if (head - tail >= n_slots) {  // the reader has not released the next slot: this call's block is dropped
        dropped++;
        dropped_run++;
        return nullptr;
    }
    EgressSlot &g = slot[head % n_slots];  // (not visible to the reader until commit() moves `head`)
    g.call = call;
    g.dropped_before = dropped_run;
    dropped_run = 0;
    return &g;
}

int EgressRing::commit(EgressSlot *g, hipStream_t s, uint64_t samples, uint64_t extra_bytes)
{
    g->samples = samples;
    g->pitch_bytes = row_pitch(samples, bytes_per_sample);
    g->has_copy = samples != 0 || extra_bytes != 0;
    if (g->has_copy) {
        PG_HIP(hipEventRecord(g->packed, s));
        PG_HIP(hipStreamWaitEvent(copy_stream, g->packed, 0));
        PG_HIP(hipMemcpyAsync(g->h, g->d, (size_t)(rows * g->pitch_bytes + extra_bytes), hipMemcpyDeviceToHost, copy_stream));
        PG_HIP(hipEventRecord(g->copied, copy_stream));
    }
    std::lock_guard<std::mutex> lk(mu);
    g->queued = true;
    g->handed = false;
    head++;
    return 0;
}

int EgressRing::next(int device, int wait, EgressBlock *b)
{
    *b = EgressBlock{};
    std::unique_lock<std::mutex> lk(mu);
    if (!open) return fail(PEBBLEGPU_E_INVALID, "the ring is not open");
    b->rows = rows;
    b->format = format;
    if (read == head) return 0;  // nothing queued
    EgressSlot &g = slot[read % n_slots];
    if (g.has_copy) {
        const hipEvent_t ev = g.copied;
        const uint64_t seq = read;
        reader_waiting = true;
        lk.unlock();  // the wait is on this slot's event alone, and not under the lock: the process thread goes on queueing
        hipError_t q = hipSetDevice(device);
        if (q == hipSuccess) q = wait ? hipEventSynchronize(ev) : hipEventQuery(ev);
        lk.lock();
        reader_waiting = false;
        cv.notify_all();
        if (q == hipErrorNotReady) return 0;
        PG_HIP(q);
        if (!open || read != seq) return fail(PEBBLEGPU_E_INVALID, "the ring was closed, or read by a second reader, during the wait");
    }
    g.handed = true;
    read++;
    b->call = g.call;
    b->samples = g.samples;
    b->pitch_bytes = g.pitch_bytes;
    b->host = g.h;
    b->dropped_before = g.dropped_before;
    b->aux = g.aux;
    b->rows = rows;
    b->format = format;
    return 0;
}

int EgressRing::finish(uint64_t call_index)
{
    std::lock_guard<std::mutex> lk(mu);
    if (!open) return fail(PEBBLEGPU_E_INVALID, "the ring is not open");
    if (tail == read) return fail(PEBBLEGPU_E_INVALID, "no block has been handed out that is still unreleased");
    EgressSlot &g = slot[tail % n_slots];
    if (g.call != call_index)
        return fail(PEBBLEGPU_E_INVALID, "blocks are released oldest first: call %llu is next, not %llu", (unsigned long long)g.call, (unsigned long long)call_index);
    g.queued = g.handed = false;
    tail++;
    return 0;
}

// ---- the receiver's two rings ----
int check_egress_slots(uint32_t n_slots)
{
    if (n_slots < kEgressMinSlots || n_slots > kEgressMaxSlots)
        return fail(PEBBLEGPU_E_INVALID, "n_slots %u: a ring has %u..%u slots", n_slots, kEgressMinSlots, kEgressMaxSlots);
    return 0;
}

int Receiver::audio_out_open(int format, const uint32_t *channels, uint32_t n_channels, uint32_t n_slots)
{
    if (format < 0 || format >= kAudioFormats) return fail(PEBBLEGPU_E_INVALID, "unknown audio format %d", format);
    if (int rc = check_egress_slots(n_slots)) return rc;
    if (channels && n_channels == 0) return fail(PEBBLEGPU_E_INVALID, "an empty channel list");
    std::vector<uint32_t> sel;
    if (!channels) {
        for (uint32_t c = 0; c < C; c++) sel.push_back(c);
    } else {
        std::vector<char> seen(C, 0);
        for (uint32_t i = 0; i < n_channels; i++) {
            if (channels[i] >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", channels[i]);
            if (seen[channels[i]]) return fail(PEBBLEGPU_E_INVALID, "channel %u is listed twice", channels[i]);
            seen[channels[i]] = 1;
            sel.push_back(channels[i]);
        }
    }
    std::lock_guard<std::mutex> g(mu_);
    if (aout_.open) return fail(PEBBLEGPU_E_INVALID, "the audio ring is already open");
    PG_HIP(hipSetDevice(device));
    const uint64_t max_n = audio_rate ? (uint64_t)rs_pitch : (uint64_t)audio.cap;
    if (!d_aout_tab_) PG_TRY(d_aout_tab_.alloc(C));
    std::lock_guard<std::mutex> lk(aout_.mu);
    if (int rc = aout_.open_ring(n_slots, (uint32_t)sel.size(), kAudioBytes[format], max_n, (uint32_t)format)) {
        aout_.release();
        return rc;
    }
    aout_format_ = format;
    aout_sel_ = sel;
    aout_tab_dirty_ = true;
    return 0;
}

int Receiver::audio_out_close()
{
    std::lock_guard<std::mutex> g(mu_);
    if (!aout_.open) return fail(PEBBLEGPU_E_INVALID, "the audio ring is not open");
    if (int rc = sync()) return rc;
    aout_.close_ring();
    return 0;
}

int Receiver::set_audio_level(uint32_t ch, float gain, int mute)
{
    if (ch >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", ch);
    if (!(gain >= 0.f) || !(gain <= 3.402823466e38f)) return fail(PEBBLEGPU_E_INVALID, "gain must be finite and >= 0");
    std::lock_guard<std::mutex> g(mu_);
    if (levels_.size() != C) levels_.assign(C, Level{});
    levels_[ch].gain = gain;
    levels_[ch].mute = mute != 0;
    aout_tab_dirty_ = true;
    return 0;
}

// the rows' table for the coming call.  Rare (open, a level change): both streams are drained first, since the packing kernel of an
// earlier call may still be reading the table -- the route the call then takes is the one it would have taken anyway
int Receiver::upload_audio_table()
{
    if (levels_.size() != C) levels_.assign(C, Level{});
    std::vector<EgressRow> tab(aout_sel_.size());
    for (size_t r = 0; r < tab.size(); r++) {
        const Level &l = levels_[aout_sel_[r]];
        tab[r] = EgressRow{l.gain / 100.f, l.mute ? 1 : 0, (int)aout_sel_[r], 0};  // gain / 100, audiopa.cpp:323
    }
    PG_HIP(hipStreamSynchronize(stream_));
    PG_HIP(hipStreamSynchronize(chain_stream_));
    PG_HIP(hipMemcpy(d_aout_tab_, tab.data(), sizeof(EgressRow) * tab.size(), hipMemcpyHostToDevice));
    aout_tab_dirty_ = false;
    return 0;
}

// behind the last writer of the call's audio buffer, on its stream: one launch, one event; n == 0 (closed squelch, tune-only): nothing
int Receiver::queue_audio_block(hipStream_t s, uint64_t n)
{
    EgressSlot *g = aout_.begin();
    if (!g) return 0;
    if (int rc = run_audio_pack(s, audio_ptr(), audio_pitch(), (long long)n, d_aout_tab_, aout_.rows, aout_format_, g->d, EgressRing::row_pitch(n, aout_.bytes_per_sample)))
        return rc;
    return aout_.commit(g, s, n);
}

// where the RAW_IQ tap's copy sits: behind the generator, ahead of the conditioners, on the main stream
int Receiver::queue_record_block(hipStream_t s, const float2 *iq, const RawSrc *raw, uint64_t n)
{
    EgressSlot *g = rec_.begin();
    if (!g) return 0;
    if (int rc = run_iq_record(s, iq, (long long)n, raw, (long long)n, S, g->d, EgressRing::row_pitch(n, 4))) return rc;
    return rec_.commit(g, s, n);
}

static void fill_block(pebblegpu_audio_block *b, const EgressBlock &e)
{
    b->format = e.format;
    b->call_index = e.call;
    b->host = e.host;
    b->samples_per_channel = e.host ? e.samples : 0;
    b->pitch_bytes = e.host ? e.pitch_bytes : 0;
    b->n_channels = e.rows;
    b->dropped_before = e.host ? e.dropped_before : 0;
}

int Receiver::audio_out_next(int wait, pebblegpu_audio_block *b)
{
    EgressBlock e;
    if (int rc = aout_.next(device, wait, &e)) return rc;
    fill_block(b, e);
    return 0;
}
int Receiver::audio_out_release(uint64_t call_index) { return aout_.finish(call_index); }
int Receiver::audio_out_dropped(uint64_t *blocks)
{
    std::lock_guard<std::mutex> lk(aout_.mu);
    if (!aout_.open) return fail(PEBBLEGPU_E_INVALID, "the audio ring is not open");
    *blocks = aout_.dropped;
    return 0;
}

// ---- the modem hook ring: what m_iDigitalModem->processBlock receives (receiver.cpp:979-980), for a host's own decoders ----
int Receiver::modem_out_open(int format, const uint32_t *channels, uint32_t n_channels, uint32_t n_slots)
{
    return modem_out_open_plan(format, channels, n_channels, n_slots, nullptr);
}

// the ring at a modem rate: the plan's refusals first (each leaves the handle as it was), then the plain ring's; an empty chain
// (min_rate at or above the demodulator rate, or no design fits: decimator.cpp:155-160 copies) IS the plain ring
int Receiver::modem_out_open_rate(int format, const uint32_t *channels, uint32_t n_channels, uint32_t n_slots, uint32_t max_bw, uint32_t min_rate)
{
    if (wfm) return fail(PEBBLEGPU_E_UNSUPPORTED, "the digital-modem hook is on the narrow branch (receiver.cpp:977-980): a WFM receiver has none");
    ModemRatePlan plan;
    if (int rc = modem_rate_plan(demod_rate_int, superframe / chain.total, max_bw, min_rate, &plan)) return rc;
    return modem_out_open_plan(format, channels, n_channels, n_slots, plan.chain.stages.empty() ? nullptr : &plan);
}

int Receiver::modem_out_open_plan(int format, const uint32_t *channels, uint32_t n_channels, uint32_t n_slots, const ModemRatePlan *plan)
{
    if (wfm) return fail(PEBBLEGPU_E_UNSUPPORTED, "the digital-modem hook is on the narrow branch (receiver.cpp:977-980): a WFM receiver has none");
    if (format != PEBBLEGPU_AUDIO_F32 && format != PEBBLEGPU_AUDIO_S16)
        return fail(PEBBLEGPU_E_INVALID, "modem blocks are PEBBLEGPU_AUDIO_F32 or PEBBLEGPU_AUDIO_S16 (I, Q pairs), not format %d", format);
    if (int rc = check_egress_slots(n_slots)) return rc;
    if (channels && n_channels == 0) return fail(PEBBLEGPU_E_INVALID, "an empty channel list");
    std::vector<uint32_t> sel;
    if (!channels) {
        for (uint32_t c = 0; c < C; c++) sel.push_back(c);
    } else {
        std::vector<char> seen(C, 0);
        for (uint32_t i = 0; i < n_channels; i++) {
            if (channels[i] >= C) return fail(PEBBLEGPU_E_INVALID, "channel %u out of range", channels[i]);
            if (seen[channels[i]]) return fail(PEBBLEGPU_E_INVALID, "channel %u is listed twice", channels[i]);
            seen[channels[i]] = 1;
            sel.push_back(channels[i]);
        }
    }
    std::lock_guard<std::mutex> g(mu_);
    if (mout_.open) return fail(PEBBLEGPU_E_INVALID, "the modem ring is already open");
    PG_HIP(hipSetDevice(device));
    const uint64_t max_n = (uint64_t)max_sf * (plan ? plan->out_spf : superframe / chain.total);
    if (!d_mout_tab_) PG_TRY(d_mout_tab_.alloc(C));
    if (plan) {  // the stages' taps as k_morse_fir takes them, and both halves of the carry at zero: a fresh Decimator's histories
        std::vector<float> h((size_t)kMaxTaps * plan->chain.stages.size(), 0.f);
        for (size_t j = 0; j < plan->chain.stages.size(); j++)
            for (int p = 0; p < plan->chain.stages[j].ntaps; p++) h[j * kMaxTaps + p] = (float)design::halfband_taps(plan->chain.stages[j].design)[p];
        PG_TRY(d_mrate_taps_.upload(h.data(), h.size()));
        PG_TRY(d_mrate_carry_.alloc_zero((size_t)2 * sel.size() * std::max<uint32_t>(plan->lookback, 1u)));
        PG_HIP(hipDeviceSynchronize());  // (the fill is over before a call's stream reads it)
    }
    std::lock_guard<std::mutex> lk(mout_.mu);
    const uint32_t bps = kAudioBytes[format];
    if (int rc = mout_.open_ring(n_slots, (uint32_t)sel.size(), bps, max_n, (uint32_t)format, modem_layout(bps, (uint32_t)sel.size(), 0, max_sf).trailer_bytes)) {
        mout_.release();
        return rc;
    }
    mrate_on_ = plan != nullptr;
    if (plan) mrate_ = *plan;
    mrate_parity_ = 0;
    mout_sel_ = sel;
    mout_tab_dirty_ = true;
    return 0;
}

int Receiver::modem_out_close()
{
    std::lock_guard<std::mutex> g(mu_);
    if (!mout_.open) return fail(PEBBLEGPU_E_INVALID, "the modem ring is not open");
    if (int rc = sync()) return rc;
    mout_.close_ring();
    mrate_on_ = false;  // (the next open starts a fresh decimator: both halves of the carry at zero)
    return 0;
}

// the selection for the coming call: the rows and which of them sit the call out in dmNONE.  Rare (open, a mode change), and drained
// like the audio ring's table: the packing kernel of an earlier call may still be reading it
int Receiver::upload_modem_table()
{
    std::vector<uint32_t> tab(mout_sel_.size());
    for (size_t r = 0; r < tab.size(); r++) tab[r] = mout_sel_[r] | (ctl_[mout_sel_[r]].mode == PEBBLEGPU_DM_NONE ? kModemRowTuneOnly : 0u);
    PG_HIP(hipStreamSynchronize(stream_));
    PG_HIP(hipStreamSynchronize(chain_stream_));
    PG_HIP(hipMemcpy(d_mout_tab_, tab.data(), sizeof(uint32_t) * tab.size(), hipMemcpyHostToDevice));
    mout_tab_dirty_ = false;
    return 0;
}

// behind the noise filter and ahead of the AGC (which works in place), on the chain's stream: one launch, one event; n_sf super-frames
// of spf samples, gate = the bank's decisions of this call or nullptr; n_sf == 0 (a one-channel receiver's closed call): nothing
int Receiver::queue_modem_block(hipStream_t s, long long spf, int n_sf, const unsigned char *gate)
{
    EgressSlot *g = mout_.begin();
    if (!g) return 0;
    g->aux = (uint32_t)n_sf;
    if (n_sf <= 0 || spf <= 0) return mout_.commit(g, s, 0);
    if (mrate_on_) {  // at a modem rate: one launch through the whole chain; the carry's parity flips with every launch and with nothing else
        const uint64_t m = mrate_.out_spf * (uint64_t)n_sf;
        const ModemLayout l = modem_layout(mout_.bytes_per_sample, mout_.rows, m, (uint32_t)n_sf);
        if (int rc = run_modem_rate_pack(s, audio.data(), audio.pitch, spf, n_sf, d_mout_tab_, mout_.rows, (int)mout_.format, gate, (int)max_sf, g->d, l.pitch, mrate_,
                                         d_mrate_taps_, d_mrate_carry_, mrate_parity_)) return rc;
        mrate_parity_ ^= 1;
        return mout_.commit(g, s, m, l.trailer_bytes);
    }
    const ModemLayout l = modem_layout(mout_.bytes_per_sample, mout_.rows, (uint64_t)spf * n_sf, (uint32_t)n_sf);
    if (int rc = run_modem_pack(s, audio.data(), audio.pitch, spf, n_sf, d_mout_tab_, mout_.rows, (int)mout_.format, gate, (int)max_sf, g->d, l.pitch)) return rc;
    return mout_.commit(g, s, (uint64_t)spf * n_sf, l.trailer_bytes);
}

int Receiver::modem_out_next(int wait, pebblegpu_modem_block *b)
{
    EgressBlock e;
    if (int rc = mout_.next(device, wait, &e)) return rc;
    const uint32_t n_sf = e.host && e.samples ? e.aux : 0;
    b->format = e.format;
    b->call_index = e.call;
    b->host = e.host;
    b->samples_per_channel = e.host ? e.samples : 0;
    b->pitch_bytes = e.host ? e.pitch_bytes : 0;
    b->n_channels = e.rows;
    b->dropped_before = e.host ? e.dropped_before : 0;
    b->rate = mrate_on_ ? mrate_.rate_int : demod_rate_int;
    b->n_superframes = n_sf;
    b->samples_per_superframe = n_sf ? e.samples / n_sf : 0;
    b->present = n_sf ? (const uint8_t *)e.host + (uint64_t)e.rows * e.pitch_bytes : nullptr;
    return 0;
}
int Receiver::modem_out_release(uint64_t call_index) { return mout_.finish(call_index); }
int Receiver::modem_out_dropped(uint64_t *blocks)
{
    std::lock_guard<std::mutex> lk(mout_.mu);
    if (!mout_.open) return fail(PEBBLEGPU_E_INVALID, "the modem ring is not open");
    *blocks = mout_.dropped;
    return 0;
}

int Receiver::record_open(uint32_t n_slots)
{
    if (int rc = check_egress_slots(n_slots)) return rc;
    std::lock_guard<std::mutex> g(mu_);
    if (rec_.open) return fail(PEBBLEGPU_E_INVALID, "the recording ring is already open");
    PG_HIP(hipSetDevice(device));
    std::lock_guard<std::mutex> lk(rec_.mu);
    if (int rc = rec_.open_ring(n_slots, S, 4, (uint64_t)max_sf * superframe, PEBBLEGPU_AUDIO_S16)) {
        rec_.release();
        return rc;
    }
    touched_ = true;  // the next call joins its two pipelines first (it runs on one stream from here on, as with a tap)
    return 0;
}

int Receiver::record_close()
{
    std::lock_guard<std::mutex> g(mu_);
    if (!rec_.open) return fail(PEBBLEGPU_E_INVALID, "the recording ring is not open");
    if (int rc = sync()) return rc;
    rec_.close_ring();
    touched_ = true;
    return 0;
}

int Receiver::record_next(int wait, pebblegpu_audio_block *b)
{
    EgressBlock e;
    if (int rc = rec_.next(device, wait, &e)) return rc;
    fill_block(b, e);
    return 0;
}
int Receiver::record_release(uint64_t call_index) { return rec_.finish(call_index); }

}  // namespace pg
