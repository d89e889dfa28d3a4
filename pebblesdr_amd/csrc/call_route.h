// call_route.h -- which way one Receiver::process call goes: the streams it runs on, the kernels it takes and the events it records,
// decided once from facts captured before anything of the call is queued.  Plain C++ (no HIP): tests/test_call_route_host.py compiles
// it on the host and checks the table of routes against facts ("Routes of a receiver call").
#pragma once

namespace pg {

// what the decision reads (Receiver::call_facts fills it, directly behind the refusals that leave the handle usable)
struct CallFacts {
    // the call's arguments
    bool with_spectrum = false, with_chain = false, raw = false;
    unsigned long long n = 0;
    // the handle's shape
    unsigned C = 1, S = 1, nf = 2048, zoom_bins = 0;
    bool wfm = false;
    bool bank_pipe_ok = false;    // created without a display transform and with two decimator output buffers in mind (Receiver::bank_pipe_ok_)
    // the handle's state
    bool profiling = false;       // per-kernel events were asked for
    bool squelch_set = false;     // squelch_db_ > -120: the one-value gate with its host read-back
    bool bank_gate = false;       // per-channel thresholds, decided on the device
    bool gated = false;           // the spectrum's update timer is on
    bool touched = false;         // a setter ran since the last call
    bool cond_any = false, cond_dirty = false;  // input conditioners on / changed
    bool generator = false;       // the test bench's generator is on
    bool taps = false;            // some tap point is enabled
    bool recording = false;       // the recording ring is open
    bool ch0_tune_only = false;   // channel 0 is in DM_NONE
    bool scale_pending = false;   // the display ring has an auto-scale flag on and a recalc requested (m_scaleNeedsRecalc)
    // what the cores can do
    bool dec_lds_free_front = false;  // the decimator's first kernel can leave LDS alone (DecimCore::front_is_lds_free)
    bool dec_raw_front = false;       // ... and has a variant that converts raw samples in its loads (DecimCore::raw_front)
    bool dec_double_out = false, dec_triple_out = false;  // two / three decimator output buffers
    bool dec_long_call = false;       // DecimCore::long_call(n)
    bool dec_fuse_shape = false;      // chain and window fit the decimator inside the display transform (DecimCore::fuse_shape)
    bool osc_transient = false;       // some oscillator is inside its amplitude transient
    bool spec_raw_ready = false, spec_dec_ready = false;  // SpectrumCore::raw_ready / dec_ready
    // the Tuning fields that take part
    bool pipeline = false, fuse_dec = false, bank_pipe_extev = false, bank_pipe_timed_ev = false;
    // a receiver without a decimator (an empty chain); the defaults leave every other receiver's routes as they are
    bool dec_mix_in_consumer = false;  // the chain is empty and the band-pass has a variant that mixes in its loads (DecimCore::mix_in_consumer_ready)
    bool tap_post_mixer = false;       // the POST_MIXER tap is on: the mixed rows must exist
};

enum class CallTail { Narrow, BankGated, Wfm };

// what the rest of the call reads
struct CallRoute {
    bool side = false;       // the chain on its own stream beside the display transform
    bool bank_pipe = false;  // two-stage call: decimator on the main stream, the rest on the chain's stream behind a hand-over event
    bool plain = false;      // pipelined with its neighbours: the call does not join the two streams first
    bool raw_fused = false;  // raw input converted in the first kernels' own loads: no float2 copy of the stream
    bool staged = false;     // the input goes through the handle's staging buffer (a conversion pass, or the generator)
    bool fuse_dec = false;   // the decimator runs inside the display transform's kernel
    bool rot3 = false;       // the call rotates three decimator output buffers
    bool mid = false;        // the event behind the display transform is recorded
    bool done_in_kernel = false;  // the hand-over event is offered to the bank kernel's own dispatch (Tuning::bank_pipe_extev)
    bool timed_handover = false;  // the hand-over records the call's timing event instead of one without timing (Tuning::bank_pipe_timed_ev)
    CallTail tail = CallTail::Narrow;
    bool rescale = false;    // the display ring's recalc stage: k_scale_stats on the call's first computed spectrum row, ahead of the packing
                             // launch (a gated call that computes no row leaves the request pending: the timer's selection is made later)
    bool tune_only = false;  // one channel in DM_NONE: the call ends behind the band-pass like a closed gate (a gate closed by the
                             // squelch read-back is a run-time fact and not part of the route)
    bool mix_in_bandpass = false;  // an empty chain: no mixer launch, the band-pass rotates the stream's samples in its own loads
};

inline CallRoute plan_call_route(const CallFacts &f)
{
    CallRoute r;
    // side by side: the chain goes to its own stream while the display transform keeps the arithmetic units busy (only when
    // the chain's first kernel needs no LDS -- the transform's workgroups leave none -- and nothing downstream reads the
    // spectrum or a conditioned copy of the input)
    r.side = f.with_spectrum && f.with_chain && !f.profiling && !f.squelch_set && !f.bank_gate && f.dec_lds_free_front && !f.cond_any && !f.cond_dirty;
    // Two-stage calls of a receiver without a display transform: mixer + decimator (and the refresh of their histories) on the main
    // stream, band-pass, noise filter, AGC, demodulators and resampler on the chain's stream behind an event -- the decimator of the next
    // call does not wait for them (it writes the other output buffer; it does wait for the band-pass of the call before the last, which
    // read that buffer).  The decimator of a bank leaves the vector units idle two thirds of the time (one wave per SIMD, bound by
    // its own instruction stream): the band-pass of the previous call fits beside it.  Results are complete after sync().
    r.bank_pipe = f.bank_pipe_ok && f.with_chain && !f.with_spectrum && !f.profiling && !f.squelch_set && !f.bank_gate && !f.zoom_bins &&
                  !f.cond_any && !f.cond_dirty && !f.generator && !f.taps && !f.recording && f.dec_double_out;
    // Pipelined calls: the display transforms of successive calls follow one another on the main stream and the chains on the
    // chain's stream -- neither waits for the other's previous call (they share nothing: the transform carries its previous
    // amplitudes, the chain its histories and oscillators), so a call's short, LDS-hungry tail kernels run beside the NEXT
    // call's transform instead of on an idle GPU.  Results are complete after sync() (the contract of include/pebblegpu.h).
    // Anything else -- a control change to apply, a call of another shape -- first orders the two queues behind each other.
    // (a call with the test bench's generator on is staged through a buffer successive calls share, as a conditioned call is: it may run its
    // chain beside its own display transform -- the kernels of the same call without a generator, so that injecting on the device and
    // feeding the summed stream give the same audio bit for bit -- but never pipelined with its neighbours, and never raw-fused)
    r.plain = ((r.side && f.pipeline && !f.touched) || (r.bank_pipe && !f.touched)) && !f.generator;
    // Raw device-format input: when the call's first kernels convert in their own loads (the 8192-bin display transform
    // and the one-channel first stage beside it) there is no float2 copy of the stream at all; otherwise normalizeIQ runs
    // as its own pass into a staging buffer and the call goes on from there.
    const bool lds_free = r.side;  // what the call asks of the decimator's first kernel
    r.raw_fused = f.raw && r.side && f.S == 1 && f.spec_raw_ready && (f.dec_raw_front && lds_free && !f.osc_transient) && !f.generator;
    r.staged = (f.raw && !r.raw_fused) || f.generator;
    // One channel through hb11 x 8, hb15, hb23, hb47 beside the 8192-bin transform: the transform's workgroups can compute the decimator
    // from the frames they hold (k_spectrum_t128<.., DEC>): the stream crosses HBM once, nothing is written at the intermediate rates.
    // Opt-in (PEBBLEGPU_FUSE_DEC=1 when the receiver is created): measured slower -- the stages sit in the kernel's barrier intervals,
    // 0.297 ms against 0.247 beside the stand-alone first stage, the call 0.330 against 0.293
    r.fuse_dec = f.fuse_dec && !f.gated && r.side && f.with_chain && !f.pipeline && f.S == 1 && f.spec_dec_ready && f.nf == 2048 &&
                 (f.dec_fuse_shape && lds_free && !f.osc_transient);
    // three output buffers in rotation for short calls, two for long ones (chunks of 128 outputs or more: 0.917 / 0.923 ms per configs[2]
    // call of 128 super-frames with two against 0.950-0.989 with three, the same at 32, 0.0775 against 0.0658 at 8)
    r.rot3 = r.bank_pipe && f.dec_triple_out && !f.dec_long_call;
    // (every record is a ~5 us bubble in the stream: a call with no display transform does without the one behind it)
    r.mid = f.with_spectrum || f.profiling || r.side;
    r.done_in_kernel = r.bank_pipe && f.bank_pipe_extev;
    r.timed_handover = r.bank_pipe && f.bank_pipe_timed_ev;
    r.tail = f.wfm ? CallTail::Wfm : f.bank_gate ? CallTail::BankGated : CallTail::Narrow;
    // SpectrumWidget::recalcScale runs on "the next fft that has new data" (spectrumwidget.cpp:1184-1187): one more launch in this call,
    // none in any other
    r.rescale = f.scale_pending && f.with_spectrum;
    // dmNONE, "Tune only mode, no demod or output" (receiver.cpp:968-971): for the reference's own shape (one channel) the call
    // ends behind the band-pass; in a bank the tune-only channels sit out the noise filter, AGC and demodulators and their rows are cleared
    r.tune_only = !f.wfm && f.C == 1 && f.ch0_tune_only;
    // A receiver without a decimator: the mixer inside the band-pass's first loads (k_fastfir_t128_mix), unless something reads the
    // mixed rows -- the zoomed transform, the POST_MIXER tap, the per-kernel events of a profiled call -- or the bank's gate is on
    r.mix_in_bandpass = f.dec_mix_in_consumer && f.with_chain && !f.wfm && !f.zoom_bins && !f.tap_post_mixer && !f.bank_gate && !f.profiling;
    return r;
}

}  // namespace pg
