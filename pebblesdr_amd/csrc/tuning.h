// tuning.h -- the library's PEBBLEGPU_* environment switches (DESIGN.md section 8 has the table).  None changes results beyond
// rounding: they select alternate kernels and launch shapes for A/B measurements.  read_tuning() is the library's only reader of
// the environment; every handle calls it once when it is created and hands the result to its cores' init().
#pragma once
#include <cstddef>
#include <cstdlib>

namespace pg {

struct Tuning {
    // Receiver
    bool pipeline = false;            // PIPELINE=1: successive side-by-side calls stop joining their two streams
    bool fuse_dec = false;            // FUSE_DEC=1: the one-channel decimator inside k_spectrum_t128
    bool bank_pipeline = true;        // BANK_PIPELINE=0: every call of a receiver without a display transform on one stream
    bool bank_pipe_hostwait = true;   // BANK_PIPE_HOSTWAIT=0: a host ahead of the device waits in the queue, not on the host
    bool bank_pipe_extev = false;     // BANK_PIPE_EXTEV=1: the two-stage hand-over event completes with the bank kernel's dispatch
    bool bank_pipe_timed_ev = false;  // BANK_PIPE_TIMED_EV=1: the two-stage hand-over records the call's timing event
    int bank_pipe_nap = -1;           // BANK_PIPE_NAP_US=<us>, in 10 ns ticks: the nap in front of stage 2 (-1: none with three buffers, 8 us with two)
    bool end_records = false;         // EVENTS=full: every side-by-side call records an end event of its own
    // stream bank
    bool sb_side = false;             // SB_SIDE=1: the band-pass on a second stream beside the display transform
    // DecimCore
    bool no_fused_dec = false;        // NO_FUSED_DEC=1: banks take the two-kernel decimator; an empty chain takes k_mixer + k_fastfir_t128, not the mixing band-pass
    bool bank_dec = true;             // BANK_DEC=0: banks take k_mix_dec_fused where it exists instead of k_mix_dec_mfma
    int bank_waves = 0;               // BANK_WAVES=<1..4>: waves per SIMD k_mix_dec_mfma's chunks are sized for (0: by call length)
    int bank_osc_adv = 1;             // BANK_OSC_ADV=0: the oscillators' advance stays in the tail launch
    int bank_hsplit = 4;              // BANK_HSPLIT=<n>: history workgroups per channel group of k_mix_dec_mfma
    bool bank_clk = false;            // BANK_CLK=1: per-wave clock counts of every k_mix_dec_mfma launch on stderr
    int fused_l = -16;                // FUSED_L=<n>: final outputs per chunk of the bank decimators, a multiple of 16 (<= 0: chosen per call)
    bool bank_pipe_bufs2 = false;     // BANK_PIPE_BUFS=2: two decimator output buffers instead of three
    bool lean_edge_launch = false;    // LEAN_EDGE_LAUNCH=1: the one-channel first stage's edges as a launch of their own
    // FastFirCore
    bool ff_xcd = true;               // FF_XCD=0: k_fastfir_t128 on a (block, channel) grid
    int ff_twlds = -1;                // FF_TWLDS=0: twiddles through the cache, =1: copied to LDS, on both routes (-1: each route's own)
    size_t ff_padlds = 0;             // FF_PADLDS=<bytes>: extra LDS per k_fastfir_t128 workgroup of the stream bank
    // WfmCore
    bool rds = true;                  // RDS=0: dmFMS without its RDS branch
    // SpectrumCore
    bool spectrum_w64 = false;        // SPECTRUM_W64=1: 8192 bins on k_spectrum_w64
    bool spectrum_perq = false;       // SPECTRUM_PERQ=1: 8192 bins through k_spectrum_q128
    bool spectrum_fregs = false;      // SPECTRUM_FREGS=1: k_spectrum_q128's factors in registers
    int t128_stagger = 3;             // T128_STAGGER=<0..7>: barrier intervals between k_spectrum_t128's two halves
    int t128_padlds = 0;              // T128_PADLDS=<bytes>: extra LDS per k_spectrum_t128 workgroup
    long long big_batch_mb = 0;       // BIG_BATCH_MB=<n>: the 65536-point spectrum in batches of n MiB (0: the whole call)
    bool big_split32 = false;         // BIG_SPLIT32=1: the 65536-point spectrum on the 32 x 2048 kernels
};

// the switches as the environment sets them now (unset: the defaults above)
inline Tuning read_tuning()
{
    Tuning t;
    const char *e;
    e = getenv("PEBBLEGPU_PIPELINE");           t.pipeline = e && e[0] == '1';
    e = getenv("PEBBLEGPU_FUSE_DEC");           t.fuse_dec = e && e[0] == '1';
    e = getenv("PEBBLEGPU_BANK_PIPELINE");      t.bank_pipeline = !(e && e[0] == '0');
    e = getenv("PEBBLEGPU_BANK_PIPE_HOSTWAIT"); t.bank_pipe_hostwait = !(e && e[0] == '0');
    e = getenv("PEBBLEGPU_BANK_PIPE_EXTEV");    t.bank_pipe_extev = e && e[0] == '1';
    e = getenv("PEBBLEGPU_BANK_PIPE_TIMED_EV"); t.bank_pipe_timed_ev = e && e[0] == '1';
    e = getenv("PEBBLEGPU_BANK_PIPE_NAP_US");   t.bank_pipe_nap = e ? (int)(100.0 * atof(e)) : -1;
    e = getenv("PEBBLEGPU_EVENTS");             t.end_records = e && e[0] == 'f';
    e = getenv("PEBBLEGPU_SB_SIDE");            t.sb_side = e && e[0] == '1';
    e = getenv("PEBBLEGPU_NO_FUSED_DEC");       t.no_fused_dec = e && e[0] == '1';
    e = getenv("PEBBLEGPU_BANK_DEC");           t.bank_dec = !(e && e[0] == '0');
    e = getenv("PEBBLEGPU_BANK_WAVES");         t.bank_waves = e ? atoi(e) : 0;
    if (t.bank_waves < 0 || t.bank_waves > 4) t.bank_waves = 0;
    e = getenv("PEBBLEGPU_BANK_OSC_ADV");       t.bank_osc_adv = e ? atoi(e) : 1;
    e = getenv("PEBBLEGPU_BANK_HSPLIT");        t.bank_hsplit = e ? atoi(e) : 4;
    e = getenv("PEBBLEGPU_BANK_CLK");           t.bank_clk = e && e[0] == '1';
    e = getenv("PEBBLEGPU_FUSED_L");            t.fused_l = e ? atoi(e) : 0;
    if (t.fused_l < 16) t.fused_l = -1;
    t.fused_l &= ~15;
    e = getenv("PEBBLEGPU_BANK_PIPE_BUFS");     t.bank_pipe_bufs2 = e && e[0] == '2';
    e = getenv("PEBBLEGPU_LEAN_EDGE_LAUNCH");   t.lean_edge_launch = e && e[0] == '1';
    e = getenv("PEBBLEGPU_FF_XCD");             t.ff_xcd = !(e && e[0] == '0');
    e = getenv("PEBBLEGPU_FF_TWLDS");           t.ff_twlds = e && e[0] == '0' ? 0 : e && e[0] == '1' ? 1 : -1;
    e = getenv("PEBBLEGPU_FF_PADLDS");          t.ff_padlds = e ? (size_t)atol(e) : (size_t)0;
    e = getenv("PEBBLEGPU_RDS");                t.rds = !(e && e[0] == '0');
    e = getenv("PEBBLEGPU_SPECTRUM_W64");       t.spectrum_w64 = e && e[0] == '1';
    e = getenv("PEBBLEGPU_SPECTRUM_PERQ");      t.spectrum_perq = e && e[0] == '1';
    e = getenv("PEBBLEGPU_SPECTRUM_FREGS");     t.spectrum_fregs = e && e[0] == '1';
    e = getenv("PEBBLEGPU_T128_STAGGER");       t.t128_stagger = e ? atoi(e) : 3;
    e = getenv("PEBBLEGPU_T128_PADLDS");        t.t128_padlds = e ? atoi(e) : 0;
    e = getenv("PEBBLEGPU_BIG_BATCH_MB");       t.big_batch_mb = e ? atoll(e) : 0LL;
    e = getenv("PEBBLEGPU_BIG_SPLIT32");        t.big_split32 = e && e[0] == '1';
    return t;
}

}  // namespace pg
