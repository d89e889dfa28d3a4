// egress.h -- host egress: ingest.h in the other direction.  A ring of pinned host slots that a small packing kernel, queued behind a
// process call on the call's own stream, fills through a device staging twin and a copy stream; the host waits for ONE slot's
// "copied" event, never for the device.  Three users in Receiver (egress.hip: audio, recording, and the modem hook ring below), two in
// the stream bank (streambank.hip: the band-passed IQ of selected streams and the display rows of a call's spectra; the ring itself
// knows neither), and the receiver's display ring (display.hip: one or two panes per slot, the ring's one "row" being the whole slot):
//   the audio output stage -- Receiver::processAudioData -> Audio::SendToOutput(in, n, m_gain, m_mute), application/receiver.cpp:1029-1035;
//                             the sample rule is pebblelib/audiopa.cpp:304-343 (the same clip in pebblelib/audioqt.cpp:169-211)
//   IQ recording           -- if (m_isRecording) m_recordingFile.WriteSamples(nextStep, numSamples), application/receiver.cpp:800-801;
//                             the conversion is pebblelib/wavfile.cpp:377-396
//   the modem hook         -- if (m_iDigitalModem != NULL) nextStep = m_iDigitalModem->processBlock(nextStep), application/receiver.cpp:979-980:
//                             the rows it receives, read-only, with a trailer of presence flags (k_modem_pack), or those rows through
//                             a modem's own Decimator chain first (k_modem_rate_pack)
// Per call: the packing kernel writes the next slot's twin on the stream where the call's last writer ran, an event is recorded
// there, the copy stream waits for it, copies device -> pinned host and records the slot's event.  Nothing the next call queues waits
// for that copy.  One block per process call, always (a call without audio yields a block of 0 samples); call indices count from
// open().  A slot is free once the reader has released it -- host-side bookkeeping only, so what is delivered and what is dropped
// does not depend on the device's timing.  A call that finds the next slot taken runs unchanged and its block is dropped and
// counted: the reference's producer drops a frame the same way when no buffer is free, and chain state never depends on the reader.
// Slots: 2..8; 4 cover the documented run-ahead of three calls (a two-stage call returns once the call three before it has completed).
#pragma once
#include <condition_variable>
#include <mutex>
#include "common.h"
#include "design.h"
#include "devmem.h"

namespace pg {

// ---- the sample rules, shared by the kernels and the host twins (pebblegpu_audio_out_convert / pebblegpu_iq_record_convert) ----
constexpr float kAudioMaxOutput = 0.9999f;  // const float maxOutput = 0.9999, audiopa.cpp:315

// out[i] *= (gain / 100); temp = out[i].real(); clip (audiopa.cpp:323-330), g = gain / 100.f.  The reference multiplies in double and
// narrows: float(double(a) * double(g)); the double product of two floats is exact, so that is ONE fp32 multiply, rounded on its own
__host__ __device__ inline float audio_out_sample(float a, float g)
{
#if defined(__HIP_DEVICE_COMPILE__)
    float t = __fmul_rn(a, g);  // (never contracted into anything)
#else
    float t = a * g;
#endif
    if (t > kAudioMaxOutput) t = kAudioMaxOutput;
    else if (t < -kAudioMaxOutput) t = -kAudioMaxOutput;
    return t;
}
// pcmData.left = value * 32767 (wavfile.cpp:387-388) on the clipped value: the product in double (an fp32 product can round up to the
// next integer and then truncates differently), the conversion truncates.  |t| <= 0.9999: always in range
__host__ __device__ inline int16_t audio_out_s16(float t) { return (int16_t)((double)t * 32767); }
// the same conversion on an unclipped IQ sample: where the reference's is undefined (|v * 32767| >= 32768) the value saturates to
// +-32767; NaN gives 0
__host__ __device__ inline int16_t iq_record_s16(float v)
{
    double d = (double)v * 32767;
    if (!(d == d)) return 0;
    if (d > 32767.0) d = 32767.0;
    else if (d < -32767.0) d = -32767.0;
    return (int16_t)d;
}

constexpr int kAudioFormats = 3;
constexpr uint32_t kAudioBytes[kAudioFormats] = {8, 4, 2};  // per sample and row: F32 L, R; S16 L, R; S16 left only
constexpr uint32_t kEgressMinSlots = 2, kEgressMaxSlots = 8;

// one selected row of the audio ring, as the packing kernel reads it (refreshed at call boundaries)
struct EgressRow {
    float g;        // gain / 100.f
    int mute;
    int src;        // row of the receiver's audio buffer
    int pad_;
};

struct EgressSlot {
    PinnedBuf<unsigned char> h;        // pinned host buffer ...
    DevBuf<unsigned char> d;           // ... and its device staging twin
    hipEvent_t packed = nullptr;       // behind the packing kernel, on the call's stream (no timing)
    hipEvent_t copied = nullptr;       // behind the copy, on the copy stream (no timing)
    uint64_t call = 0, samples = 0, pitch_bytes = 0;
    uint32_t dropped_before = 0;
    uint32_t aux = 0;                  // the owner's own word about the block, set before commit() (the display ring: first_row)
    bool queued = false;               // holds a block that has not been released
    bool handed = false;               // ... and next() has handed it out
    bool has_copy = false;             // a copy was queued for it (a block of 0 samples has none)
};

struct EgressBlock {
    uint64_t call = 0, samples = 0, pitch_bytes = 0;
    const void *host = nullptr;
    uint32_t dropped_before = 0, rows = 0, format = 0, aux = 0;
};

struct EgressRing {
    std::mutex mu;                     // the ring's bookkeeping; never held while waiting for an event
    std::condition_variable cv;        // close() waits here for a reader that is inside its event wait
    bool open = false, reader_waiting = false;
    uint32_t n_slots = 0, rows = 0, bytes_per_sample = 0, format = 0;  // format: what the blocks report (pebblegpu_audio_format)
    uint64_t max_samples = 0, slot_bytes = 0;
    EgressSlot slot[kEgressMaxSlots];
    hipStream_t copy_stream = nullptr;
    uint64_t calls = 0;                // process calls since open(): the next block's index
    uint64_t head = 0, tail = 0;       // slot sequence numbers: [tail, head) are queued, oldest first
    uint64_t read = 0;                 // ... and [tail, read) of them have been handed out
    uint64_t dropped = 0;
    uint32_t dropped_run = 0;          // blocks dropped since the last one that was queued

    static uint64_t row_pitch(uint64_t samples, uint32_t bytes_per_sample) { return (samples * bytes_per_sample + 15) & ~(uint64_t)15; }
    // allocates n_slots x (pinned buffer, twin, two events) for `rows` rows of at most max_samples; the caller has set the device
    // extra_bytes: room behind the rows for the owner's trailer (commit's extra_bytes)
    int open_ring(uint32_t slots, uint32_t n_rows, uint32_t bps, uint64_t max_n, uint32_t fmt, uint64_t extra_bytes = 0);
    void release();                    // (the owner has synchronised its streams)
    // close: the owner has synchronised its streams (every slot's event is complete); waits until a reader on another thread has left
    // its event wait, then frees the ring -- the events are never destroyed under a waiting reader
    void close_ring();
    // The producer's side, from a process call.  begin(): the slot the call's block goes to, or nullptr when the ring is full (the block
    // is dropped and counted); the call index advances either way.  commit(): an event on `s` behind the packing kernel, the copy of
    // rows * pitch bytes on the copy stream behind it, the slot's event; with samples == 0 nothing is queued at all.
    EgressSlot *begin();
    // extra_bytes (a multiple of 16): a trailer the packing launch wrote at rows * pitch, inside the one copy
    int commit(EgressSlot *g, hipStream_t s, uint64_t samples, uint64_t extra_bytes = 0);
    // The reader's side.  next(): the oldest block not handed out yet; wait != 0 blocks on that slot's event only; host == nullptr
    // when nothing is queued or (wait == 0) the copy has not completed.  finish(): takes the oldest unreleased block.
    int next(int device, int wait, EgressBlock *b);
    int finish(uint64_t call_index);
};

// rows x n float2 audio samples (row r at audio + tab[r].src * pitch) -> dst [rows][dst_pitch bytes] in `format`
int run_audio_pack(hipStream_t s, const float2 *audio, long long pitch, long long n, const EgressRow *d_tab, uint32_t rows, int format, void *dst,
                   uint64_t dst_pitch);
// rows x n IQ samples (float2 rows of `pitch`, or raw device-format pairs converted as k_normalize_iq converts them) -> PCM16 pairs
int run_iq_record(hipStream_t s, const float2 *iq, long long pitch, const struct RawSrc *raw, long long n, uint32_t rows, void *dst, uint64_t dst_pitch);
// = pebblegpu_stream_gate: one (selected stream, frame) of a stream-bank IQ block's trailer, and the gated packing kernel's table
struct StreamGate {
    float peak_db, avg_db, snr_db, floor_db;
    uint32_t open, row;
};
constexpr uint32_t kStreamGateCarried = 0xFFFFFFFEu, kStreamGateNone = 0xFFFFFFFFu;

// rows x n band-passed samples (row r at iq + tab[r] * pitch: the stream bank's selection) -> dst [rows][dst_pitch bytes]: the float2
// rows verbatim (PEBBLEGPU_AUDIO_F32) or PCM16 pairs by iq_record_s16 (PEBBLEGPU_AUDIO_S16)
// gate != nullptr: the gated instance -- frame f (of `frame` samples, n_frames = n / frame) of block row r is zeros where
// gate[r * n_frames + f].open == 0 and what the ungated instance writes everywhere else
int run_iq_pack(hipStream_t s, const float2 *iq, long long pitch, long long n, const uint32_t *d_tab, uint32_t rows, int format, void *dst, uint64_t dst_pitch,
                const StreamGate *gate = nullptr, long long frame = 0);
int check_egress_slots(uint32_t n_slots);

// ---- the modem hook ring (Receiver::modem_out_*): the rows DigitalModemInterface::processBlock receives (receiver.cpp:979-980) ----
// one selected row as k_modem_pack reads it: the channel's row of the narrow branch's buffer, bit 31 = the channel is in dmNONE this call
constexpr uint32_t kModemRowTuneOnly = 0x80000000u;
// a block's layout, one function for the producer, the reader and the host tier: row r at r * pitch, the trailer -- one byte per (row,
// super-frame), [r * n_sf + j], 1 = present -- at rows * pitch, padded to 16 bytes
struct ModemLayout { uint64_t pitch, trailer_off, trailer_bytes; };
inline ModemLayout modem_layout(uint32_t bytes_per_sample, uint32_t rows, uint64_t samples, uint32_t n_sf)
{
    ModemLayout l;
    l.pitch = EgressRing::row_pitch(samples, bytes_per_sample);
    l.trailer_off = (uint64_t)rows * l.pitch;
    l.trailer_bytes = ((uint64_t)rows * n_sf + 15) & ~(uint64_t)15;
    return l;
}
// rows x n samples of the narrow branch's buffer behind the noise filter (row r at iq + (tab[r] & ~kModemRowTuneOnly) * pitch), n = n_sf
// super-frames of spf samples -> dst [rows][dst_pitch bytes] in `format` (F32: the float2 rows verbatim; S16: iq_record_s16 pairs) and
// the trailer at dst + rows * dst_pitch.  A (row, super-frame) is absent -- zeros, flag 0 -- where the row is tune-only or
// gate[channel * gate_stride + j] == 0 (gate == nullptr: no gate)
int run_modem_pack(hipStream_t s, const float2 *iq, long long pitch, long long spf, int n_sf, const uint32_t *d_tab, uint32_t rows, int format,
                   const unsigned char *gate, int gate_stride, void *dst, uint64_t dst_pitch);

// ---- the same ring at a modem rate (Receiver::modem_out_open_rate): every selected row through the reference's own Decimator chain for
// (demodulator rate, max_bw, min_rate) -- Decimator::buildDecimationChain, pebblelib/decimator.cpp:64-149, what Morse::setSampleRate builds
// (morse.cpp:174-193) and runs at the head of processBlock -- before it crosses the link ----
// The plan, one function for pebblegpu_modem_rate_plan and the open: the chain, its look-back H = sum_j (T_j - 1) prod_{i<j} stride_i in
// demodulator samples (the raw samples in front of a segment from which every stage recomputes its own history), and the refusals
struct ModemRatePlan {
    design::Chain chain;
    uint32_t rate_int = 0;   // (uint32_t)(int)chain.rate: int actualModemRate, morse.cpp:193
    uint32_t lookback = 0;   // H
    uint64_t out_spf = 0;    // samples per super-frame behind the chain
    uint32_t tile = 0;       // modem-rate outputs one workgroup of k_modem_rate_pack carries (0: an empty chain, nothing to launch)
    uint32_t lds_a = 0, lds_b = 0;  // float2 of the kernel's two LDS buffers
};
int modem_rate_plan(uint32_t demod_rate, uint64_t spf, uint32_t max_bw, uint32_t min_rate, ModemRatePlan *out);
// what k_modem_rate_pack needs to know about the chain, by value
struct ModemRateChain {
    int n_stages, D, H, tile, lds_a, lds_b;
    int taps[kMaxStages], stride[kMaxStages];
};
// rows x n_sf super-frames of spf samples -> dst rows of n_sf * spf / D samples in `format` and the trailer, as run_modem_pack; taps:
// [stage][kMaxTaps] fp32; carry: [2][rows][H] float2, read at parity p and written at p ^ 1 (the caller flips p after every launch)
int run_modem_rate_pack(hipStream_t s, const float2 *iq, long long pitch, long long spf, int n_sf, const uint32_t *d_tab, uint32_t rows, int format,
                        const unsigned char *gate, int gate_stride, void *dst, uint64_t dst_pitch, const ModemRatePlan &plan, const float *d_taps,
                        float2 *d_carry, int parity);

}  // namespace pg
