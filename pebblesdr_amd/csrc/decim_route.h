// decim_route.h -- which way one DecimCore::run call goes.  plan_decim_shape() derives from the chain, once per init, everything that is
// neither a buffer nor a tap value; plan_decim_route() picks from that shape and the facts of one call the kernels the call launches.
// Plain C++ (no HIP): tests/test_decim_route_host.py compiles it on the host and holds it to tests/decim_cases.py's route(), the
// independent statement of the same rule that the GPU tier compares kernel_name() with ("Routes of a decimator call").
#pragma once
#include <algorithm>
#include <cstddef>

namespace pg {

constexpr int kFrontT1 = 11;    // the hb11 the register fronts are built for (FrontTaps)
constexpr int kMaxCascade = 6;  // stages k_cascade fuses at most (CascadeParams)

// HY: depth of the first-stage history a call leaves (and chunk 0 reads) = 8 * warm + 8
template <int T1, int T2, int T3>
struct FusedDecGeom {
    static constexpr int halo = (T1 - 1) + 2 * (T2 - 1) + 4 * (T3 - 1);
    static constexpr int warm = halo / 8;
    static constexpr int HY = 8 * warm + 8;
    // running sums per stage: pending outputs at a block's start plus the ones its inputs start
    static constexpr int N1 = (T1 + 1) / 2 + 3, N2 = (T2 + 1) / 2 + 1, N3 = (T3 + 1) / 2;
    static_assert(T1 % 4 == 3 && T2 % 4 == 3 && T3 % 4 == 3, "halfbands have 4k + 3 taps (odd centre)");
};

// ---- k_mix_dec_mfma's instances, X(NP, T1, T2, T3, MINW): fronts (4 pairs: hb11 x S; 12: a merged CIC3 in front of it) x the halfband
// triples the reference's ladder puts behind them between 1 and 200 Msps (decimator.cpp:64-149); MINW: waves per SIMD the registers admit
// ((4, 15|19, 27, 59): 227 / 231 registers since the main loop stopped copying its fetched samples, half a SIMD's file).  cores.hip
// instantiates the kernels from this list, in this order ----
#define PG_BANK_DEC_INSTANCES(X)                                                                  \
    X(4, 15, 19, 31, 2) X(4, 15, 23, 43, 2) X(4, 15, 23, 47, 2) X(4, 15, 19, 35, 2)                \
    X(4, 15, 27, 59, 2) X(4, 19, 27, 59, 2)                                                       \
    X(12, 15, 23, 47, 1) X(12, 15, 19, 35, 1) X(12, 15, 27, 59, 1)

struct BankInstance { int np, t1, t2, t3, hy, nstate, minw; };
inline const BankInstance *bank_instance(int np, int t1, int t2, int t3)
{
#define PG_X(NP, T1, T2, T3, MINW) {NP, T1, T2, T3, FusedDecGeom<T1, T2, T3>::HY, FusedDecGeom<T1, T2, T3>::N1 + FusedDecGeom<T1, T2, T3>::N2 + FusedDecGeom<T1, T2, T3>::N3, MINW},
    static const BankInstance k[] = {PG_BANK_DEC_INSTANCES(PG_X)};
#undef PG_X
    for (const BankInstance &b : k)
        if (b.np == np && b.t1 == t1 && b.t2 == t2 && b.t3 == t3) return &b;
    return nullptr;
}

// a bank call of this many final outputs is "long": chunks of 128 outputs or more at one wave per SIMD (bank_geometry's choice of waves,
// DecimCore::long_call)
inline bool bank_long_call(long long len_out, long long C)
{
    const long long per = 2 * std::max(1LL, 1024LL / ((C + 31) / 32));
    return (len_out + per - 1) / per >= 128;
}

// ---- the tile of the fixed-tap k_cascade instances (three halfbands at stride 2: <15,23,47>, <15,19,31>).  A halfband output j reads
// the even offsets 2j, 2j + 2, .. 2j + T - 1 of its input and the one odd centre 2j + (T-1)/2 (T = 4k + 3, so the centre is odd); a
// work-item makes the outputs 2u and 2u + 1 from one window, which starts at input 4u.  The tile therefore lies in LDS as FOUR planes:
// plane r holds the inputs i = r (mod 4) at i >> 2, unit stride.  Then
//   - the window's (T+3)/2 even inputs 4u + 2k are reads of plane 0 (k even) or 2 (k odd) at u + (k >> 1): consecutive lanes, consecutive
//     8-byte slots, one plane per instruction;
//   - the two centres 4u + (T-1)/2 and 4u + 2 + (T-1)/2 are one read of plane 3 and one of plane 1 (or 1 and 3), again at unit stride;
//   - a stage's output 2u (2u + 1) is the next stage's input of plane 0 or 2 (1 or 3) by the parity of u, at u >> 1: a group of 16
//     lanes stores 8 consecutive slots of each of the two planes, and so does the tile load (lane v holds inputs 2v, 2v + 1).
// The LDS unit serves an 8-byte store 16 lanes at a time over 32 four-byte banks (a single 8-byte read 32 lanes over 64, a pair read
// like a store: tests/test_lds_exchange_banks_host.py): a group of stores is conflict-free when its 16 slots differ mod 16.  Planes 0
// and 2 (and 1 and 3) therefore start 8 slots apart mod 16: the plane pitch is = 8 (mod 16), the planes lie in the order 0, 2, 1, 3.
// The unit-stride reads are conflict-free under either read rule wherever the planes start.  One slot per plane beyond
// ceil(count / 4) is slack: with an odd count of final outputs the last work-item's unused second window reaches one input past the
// tile (read, never stored).
// Two such buffers: A holds the tile (c0 inputs) and later the second stage's outputs (c2), B the first stage's (c1).  At the tile of
// 256 final outputs every chain of the ladder stays under kCascadeFixedLdsCap = 32 KiB: five workgroups per CU's 160 KiB, as the three
// contiguous runs of the generic form gave (tests/test_cascade_tiles_host.py walks all of this).
constexpr int kCascadeFixedLdsCap = 32 * 1024;
constexpr int cascade_plane_pitch(int count) { return (((count + 3) / 4 + 1 + 7) / 16) * 16 + 8; }
constexpr int cascade_plane_base(int r, int pitch) { return (((r & 1) << 1) | ((r >> 1) & 1)) * pitch; }
constexpr int cascade_plane_slot(int i, int pitch) { return cascade_plane_base(i & 3, pitch) + (i >> 2); }
struct CascadeFixedTile { int c0, c1, c2, pitch_a, pitch_b, lds_bytes; };
constexpr CascadeFixedTile cascade_fixed_tile(int outb, int t0, int t1, int t2)
{
    const int c2 = 2 * outb + t2 - 1, c1 = 2 * c2 + t1 - 1, c0 = 2 * c1 + t0 - 1;
    const int pa = cascade_plane_pitch(c0), pb = cascade_plane_pitch(c1);
    return {c0, c1, c2, pa, pb, 4 * (pa + pb) * 8};
}
// the tile of final outputs o0 .. starts at this input (relative to the call's first; what lies before 0 is the head-room); a ragged last
// tile of n < outb outputs reads cascade_fixed_tile(n, ..).c0 inputs from there, which ends where the call's data ends
constexpr long long cascade_fixed_first(long long o0, int t0, int t1, int t2) { return ((o0 * 2 - (t2 - 1)) * 2 - (t1 - 1)) * 2 - (t0 - 1); }

// ---------------------------------------------------------------- the shape: what init derives from the chain
struct DecimStageDesc { int ntaps, stride; };  // ntaps 0: the reference's merged CIC3
struct DecimTuningFacts {
    bool no_fused_dec = false;  // Tuning::no_fused_dec: banks keep the two-kernel decimator
    bool bank_dec = true;       // Tuning::bank_dec: k_mix_dec_mfma where an instance exists (else k_mix_dec_fused where that exists)
};

struct DecimShape {
    unsigned C = 0;
    int n_stages = 0;
    long long total = 1;             // the chain's decimation
    int first_ntaps = 0, first_stride = 1;
    bool first_cic3 = false;
    // An empty chain (no halfband design fits the rate: 48 kHz narrow, WFM below 500 kHz): run() is the stand-alone mixer (k_mixer) into
    // buf0, which is then out() -- head-room = the consumer's look-back, refreshed by tail_job_out() like a single stage's.  No first
    // stage means no register front, no raw-converting loads, no decimator inside the transform and no second output buffer.
    bool zero_stage = false;
    bool bank_front = false;         // hb11 first stage in registers (k_mix_hb11_bank): a >= 16-channel bank off a shared stream, or one channel when asked
    // A second stage with a stride >= 8 (merged halfbands at high input rates) would make the fused cascade's tiles mostly
    // halo: it runs as its own strided FIR (k_fir_dec) from buf0 into buf1, and the fused rest reads buf1.
    bool wide = false;
    bool fused_front = false;        // merged CIC3 + wide halfband in one kernel (k_mix_cic_hb): nothing is written at the CIC rate
    int wide_taps = 0, wide_stride = 1;
    // stages 1.. (2.. behind a wide stage): one fused kernel (k_cascade)
    int nst = 0, casc_ntaps[kMaxCascade] = {}, casc_stride[kMaxCascade] = {};
    long long later = 1;             // their decimation
    bool three2 = false;             // three of them, each at stride 2: the form the fixed-tap kernels are built for
    int outb = 0, lds_half = 0;      // final outputs per k_cascade tile, float2 slots of its first ping-pong buffer
    size_t casc_lds_bytes = 0;
    size_t casc_fixed_lds_bytes = 0; // three2: the four-plane tile of the fixed-tap instances (cascade_fixed_tile)
    long long halo0 = 0;             // look-back of the whole cascade in its input's samples (the first-stage buffer's head-room)
    // the whole decimator in one kernel (k_mix_dec_fused): a >= 16-channel bank off one shared stream whose chain is hb11 x S
    // followed by hb15, hb19, hb31; calls inside an oscillator transient take the two-kernel route (both keep each other's history)
    bool fused_all = false;
    // the same chain with its first stage on the matrix pipe, one wave per (32 channels, two chunks): k_mix_dec_mfma (kernels_bank_dec.h),
    // the default route of such a bank; PEBBLEGPU_BANK_DEC=0 keeps the four-wave pipeline above
    bool bank_mfma = false;
    int bank_np = 0;                 // its front: 4 (hb11 x S) or 12 (a merged CIC3 in front)
    int fused_hy = 0;                // first-stage outputs of history either one-kernel route keeps
    int bank_nstate = 0, bank_minw = 2;  // running sums per channel of the chain's instance; waves per SIMD it admits
    int xh_depth = 16;               // samples of raw-input tail kept in d_xhist

    bool one_kernel() const { return fused_all || bank_mfma; }
    bool front_is_lds_free() const { return zero_stage || (C == 1 && (fused_front || bank_front)); }
    // the first kernels read raw device-format samples themselves (k_mix_hb11_lean + its edge launch): those kernels exist for this chain
    bool raw_front() const { return bank_front && C == 1 && !one_kernel(); }
};

// st: the chain's n_stages stages, at most kMaxCascade + 1 of them (DecimCore::init refuses longer chains)
inline DecimShape plan_decim_shape(const DecimStageDesc *st, int n_stages, unsigned C, const DecimTuningFacts &t)
{
    DecimShape s;
    s.C = C;
    s.n_stages = n_stages;
    if (n_stages == 0) {  // "No decimation, just return" (decimator.cpp:155-160)
        s.zero_stage = true;
        return s;
    }
    s.first_ntaps = st[0].ntaps;
    s.first_stride = st[0].stride;
    s.first_cic3 = st[0].ntaps == 0;
    // banks of >= 16 channels behind an hb11 first stage mix in registers when their input is one shared stream
    s.bank_front = !s.first_cic3 && s.first_ntaps == kFrontT1 && (C >= 16 || C == 1);
    // a wide second stage is peeled off the fused cascade
    s.wide = n_stages >= 3 && st[1].stride >= 8 && st[1].ntaps > 0;
    int kfirst = 1;
    if (s.wide) {
        s.wide_taps = st[1].ntaps;
        s.wide_stride = st[1].stride;
        kfirst = 2;
        s.fused_front = s.first_cic3 && st[1].ntaps == kFrontT1;  // k_mix_cic_hb is built for the hb11 the ladder always picks here
    }
    long long prod = 1;
    for (int k = 0; k < n_stages; k++) s.total *= st[k].stride;
    for (int k = kfirst; k < n_stages && s.nst < kMaxCascade; k++, s.nst++) {
        s.casc_ntaps[s.nst] = st[k].ntaps;
        s.casc_stride[s.nst] = st[k].stride;
        s.halo0 += (long long)(st[k].ntaps - 1) * prod;  // look-back of the whole cascade, in stage-0 output samples
        prod *= st[k].stride;
    }
    s.later = prod;
    if (s.nst > 0) {
        // largest power-of-two tile of final outputs whose two ping-pong buffers fit comfortably (<= 48 KiB)
        const long long lds_cap = 48LL * 1024;
        for (int outb = 256;; outb /= 2) {
            long long c0 = outb, c1 = 0;
            for (int k = s.nst; k >= 1; k--) {
                c1 = c0;
                c0 = c0 * s.casc_stride[k - 1] + s.casc_ntaps[k - 1] - 1;
            }
            // c0 = stage-0 samples a tile reads, c1 = outputs of the first fused stage (the largest intermediate)
            if ((c0 + c1) * 8 <= lds_cap || outb == 1) {
                s.outb = outb;
                s.lds_half = (int)c0;
                s.casc_lds_bytes = (size_t)(c0 + c1) * 8;
                break;
            }
        }
    }
    // the whole decimator in one kernel for banks off one shared stream: k_mix_dec_mfma for every chain of the form [cic3 x S0,] hb11 x S,
    // three halfbands at stride 2 whose tap counts are in its list; k_mix_dec_fused<15, 19, 31>, its predecessor, for
    // hb11 x S, hb15, hb19, hb31 (PEBBLEGPU_BANK_DEC=0)
    s.three2 = s.nst == 3 && s.casc_stride[0] == 2 && s.casc_stride[1] == 2 && s.casc_stride[2] == 2;
    if (s.three2) s.casc_fixed_lds_bytes = (size_t)cascade_fixed_tile(s.outb, s.casc_ntaps[0], s.casc_ntaps[1], s.casc_ntaps[2]).lds_bytes;
    const bool hb_front = s.bank_front && C >= 16 && !s.wide && s.first_stride <= 16;
    const bool cic_front = s.fused_front && C >= 16 && s.wide_stride == 16;
    const int *T = s.casc_ntaps;
    s.fused_all = hb_front && s.three2 && T[0] == 15 && T[1] == 19 && T[2] == 31 && !t.no_fused_dec;
    if (s.three2 && (hb_front || cic_front) && !t.no_fused_dec && t.bank_dec) {
        if (const BankInstance *b = bank_instance(cic_front ? 12 : 4, T[0], T[1], T[2])) {
            s.bank_mfma = true;
            s.bank_np = b->np;
            s.fused_hy = b->hy;
            s.bank_nstate = b->nstate;
            s.bank_minw = b->minw;
        }
    }
    if (s.fused_all && !s.bank_mfma) s.fused_hy = FusedDecGeom<15, 19, 31>::HY;
    if (s.one_kernel()) {
        if (s.halo0 < s.fused_hy) s.halo0 = s.fused_hy;  // the first-stage buffer's head-room doubles as these kernels' first-stage history
        s.xh_depth = cic_front ? 512 : 16;               // raw samples in front of a call that its first windows reach (11 S0 + 1 with a CIC3 in front)
    }
    return s;
}

// ---------------------------------------------------------------- the route of one call
struct DecimCallFacts {
    long long n = 0;               // input samples per stream, a multiple of the chain's decimation
    bool shared_input = false;
    bool transient = false;        // OscBank::any_transient()
    bool lds_free = false;         // DecimCall::lds_free
    int raw_fmt = -1;              // the input is still in this device sample format (RawSrc::fmt); -1: float2
    bool mix_in_consumer = false;  // DecimCall::mix_in_consumer
    bool in_aligned = true;        // the input pointer is a multiple of 8 bytes
    long long out_pitch = 0;       // row pitch of the buffer the call writes
    bool lean_edge_launch = false; // Tuning::lean_edge_launch
    bool ovl_pending = false;      // an empty chain: the consumer's own overlap row is newer than buf0's head-room (DecimCore::Carried)
    // (Tuning::no_fused_dec and Tuning::bank_dec act through the shape: init sizes the histories by them)
};

enum class DecimFront { None, InConsumer, Mixer, BankMfma, Fused, CicHb, Lean, Hb11Bank, Dec1, InSpectrum };
enum class DecimRest { None, FirDec, Cascade, FirDecCascade };

struct DecimRoute {
    DecimFront front = DecimFront::None;  // (InSpectrum is never planned here: DecimCore::run_beside_spectrum records it)
    long long len0 = 0, len1 = 0, len_out = 0;  // outputs of the first stage, of the wide stage, of the chain
    // the front kernel's instance and launch
    bool transient = false, uniform = false;  // k_mix_cic_hb / k_mix_hb11_bank<TRANSIENT, UNIFORM>
    int cl_log2 = 0, R = 0;                   // channels across the lanes of a wave; outputs per lane
    unsigned grid_x = 0, grid_y = 0;
    int raw_fmt = -1;                         // k_mix_hb11_lean<FMT>
    bool edge_launch = false;                 // ... with its edges as a launch of their own
    int cg = 1;                               // k_mix_dec1: channels per workgroup
    DecimRest rest = DecimRest::None;
    int cascade_inst = 0;                     // 0: k_cascade<0,0,0>, 1: <15,23,47>, 2: <15,19,31>
    unsigned tiles = 0;                       // k_cascade's workgroups per channel
    // an empty chain's hand-over, at the switch between its two routes only: the mixed overlap in front of the call lies in the consumer's
    // own row (InConsumer reads it there, Mixer first copies it into buf0's head-room) and not in the head-room a k_mixer call's tail
    // job refreshed; and where it lies behind the call
    bool ovl_from_row = false, ovl_pending = false;

    bool one_kernel() const { return front == DecimFront::BankMfma || front == DecimFront::Fused; }
    bool general() const { return front == DecimFront::CicHb || front == DecimFront::Lean || front == DecimFront::Hb11Bank || front == DecimFront::Dec1; }
    bool fir_dec() const { return rest == DecimRest::FirDec || rest == DecimRest::FirDecCascade; }
    bool cascade() const { return rest == DecimRest::Cascade || rest == DecimRest::FirDecCascade; }
    // the kernel the call used for the mixer + first stage (bench / profiling labels), and for the remaining stages
    const char *front_name() const
    {
        switch (front) {
        case DecimFront::InConsumer: return "k_fastfir_t128 (mixing)";
        case DecimFront::Mixer: return "k_mixer";
        case DecimFront::BankMfma: return "k_mix_dec_mfma";
        case DecimFront::Fused: return "k_mix_dec_fused";
        case DecimFront::CicHb: return "k_mix_cic_hb";
        case DecimFront::Lean: return "k_mix_hb11_lean";
        case DecimFront::Hb11Bank: return "k_mix_hb11_bank";
        case DecimFront::Dec1: return "k_mix_dec1";
        case DecimFront::InSpectrum: return "k_spectrum_t128 (decimator inside)";
        case DecimFront::None: break;
        }
        return "";
    }
    const char *rest_name() const { return rest == DecimRest::FirDec ? "k_fir_dec" : rest == DecimRest::Cascade ? "k_cascade" : rest == DecimRest::FirDecCascade ? "k_fir_dec + k_cascade" : ""; }
};

inline unsigned decim_cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// k_mix_cic_hb and k_mix_hb11_bank: channels across the lanes of a wave (the other lanes take further outputs), outputs per lane (a
// channel's R * OL outputs leave the wave as one row segment), and the grid over n_out outputs
inline void plan_channel_lanes(DecimRoute &r, unsigned C, long long n_out)
{
    r.cl_log2 = 0;
    while ((1u << r.cl_log2) < C && r.cl_log2 < 6) r.cl_log2++;
    r.R = r.cl_log2 == 6 ? 16 : 8;
    r.grid_x = decim_cdiv(n_out + 1, 4LL * r.R * (64 >> r.cl_log2));
    r.grid_y = decim_cdiv(C, 1u << r.cl_log2);
}

inline DecimRoute plan_decim_route(const DecimShape &s, const DecimCallFacts &f)
{
    DecimRoute r;
    r.len0 = f.n / s.first_stride;
    r.len_out = f.n / s.total;
    if (s.zero_stage) {
        // the consumer (the band-pass) rotates the samples in its own loads and nothing is launched, or the stand-alone mixer
        r.front = f.mix_in_consumer ? DecimFront::InConsumer : DecimFront::Mixer;
        r.ovl_from_row = f.ovl_pending;
        r.ovl_pending = f.mix_in_consumer;
        r.grid_x = decim_cdiv(f.n, 1024);
        r.grid_y = s.C;
        return r;
    }
    if (s.one_kernel() && f.shared_input && !f.transient) {
        // (k_mix_dec_mfma's sample fetches and result stores carry 32-bit byte offsets; its chunks are 16 outputs or more, two per wave)
        if (s.bank_mfma && (unsigned long long)f.n * 8 < 0xFFF00000ull && (unsigned long long)s.C * (unsigned long long)f.out_pitch * 8 < 0xFFF00000ull &&
            r.len_out >= 64 && f.in_aligned) {
            r.front = DecimFront::BankMfma;
            return r;
        }
        if (s.fused_all) {
            r.front = DecimFront::Fused;
            r.grid_y = decim_cdiv(s.C, 64);
            return r;
        }
    }
    if (s.fused_front) {
        r.front = DecimFront::CicHb;
        r.len1 = r.len0 / s.wide_stride;
        plan_channel_lanes(r, s.C, r.len1);
        r.transient = f.transient;
        r.uniform = r.cl_log2 == 6 && f.shared_input;  // the lanes of a wave share one window: scalar loads
    } else if (s.bank_front && s.C == 1 && f.lds_free && !f.transient) {
        // beside the spectrum kernel: the lean one-channel kernel for every output inside the call; the first outputs, whose windows reach
        // back into the mixed history, and the new history in one more workgroup of it or (A/B) in a launch of the general kernel
        r.front = DecimFront::Lean;
        r.R = 8;
        r.raw_fmt = f.raw_fmt < 0 ? -1 : f.raw_fmt <= 3 ? f.raw_fmt : 4;
        r.edge_launch = f.lean_edge_launch;
        r.grid_x = decim_cdiv(r.len0, 4LL * r.R * 64) + (r.edge_launch ? 0 : 1);
        r.grid_y = 1;
    } else if (s.bank_front && (s.C >= 16 ? f.shared_input : f.lds_free)) {
        // a bank off one shared stream: lanes = channels, windows in registers
        r.front = DecimFront::Hb11Bank;
        plan_channel_lanes(r, s.C, r.len0);
        r.transient = f.transient;
        r.uniform = r.cl_log2 == 6;
    } else {
        r.front = DecimFront::Dec1;
        // merged CIC3 over a shared stream: one workgroup mixes a group of channels from one fetch of the sample pairs
        r.cg = (s.first_cic3 && s.first_stride > 2 && f.shared_input) ? 8 : 1;
        r.grid_x = decim_cdiv(r.len0, 256);
        r.grid_y = decim_cdiv(s.C, r.cg);
    }
    // the peeled stride->=8 stage: every output reads its own taps-long window straight from buf0
    const bool fir = s.wide && !s.fused_front;
    if (fir) r.len1 = r.len0 / s.wide_stride;
    r.rest = s.nst > 0 ? (fir ? DecimRest::FirDecCascade : DecimRest::Cascade) : (fir ? DecimRest::FirDec : DecimRest::None);
    if (s.nst > 0) {
        const int *T = s.casc_ntaps;
        if (s.three2 && T[0] == 15 && T[1] == 23 && T[2] == 47) r.cascade_inst = 1;       // WFM from 20 Msps, narrow from 100 Msps
        else if (s.three2 && T[0] == 15 && T[1] == 19 && T[2] == 31) r.cascade_inst = 2;  // narrow at 2.048 Msps
        r.tiles = decim_cdiv(r.len_out, s.outb);
    }
    return r;
}

}  // namespace pg
